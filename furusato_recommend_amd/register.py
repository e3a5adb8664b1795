"""Model registry with the reference's names (main.py:32-56, subset on the
hot path: 'lgn' = LightGCN, 'radj' = rAdjGCN, 'mf' = MF, 'sage' = GraphSAGE,
'sasrec' = SASRec)."""
from .graphsage import GraphSAGE
from .lightgcn import LightGCN
from .mf import MF
from .radj import rAdjGCN
from .sasrec import SASRec

MODELS = {
    "mf": MF,
    "lgn": LightGCN,
    "radj": rAdjGCN,
    "sage": GraphSAGE,
    "sasrec": SASRec,
}
