"""Model registry with the reference's names (main.py:32-56, subset on the
hot path: 'lgn' = LightGCN, 'lgnssm' = LightGCNSSM, 'radj' = rAdjGCN,
'mf' = MF, 'sage' = GraphSAGE, 'gnn' = GNN with conv = 'gat' (GATConv hops,
the default) or 'ggnn' (GatedGraphConv hops), 'tgrec' = TGRec
(TransformerConv hops), 'lightsage' = LightSAGE (weight-free residual-mean
hops), 'sasrec' = SASRec)."""
from .gnn import GNN
from .graphsage import GraphSAGE
from .lgcnssm import LightGCNSSM
from .lightsage import LightSAGE
from .lightgcn import LightGCN
from .mf import MF
from .radj import rAdjGCN
from .sasrec import SASRec
from .tgrec import TGRec

MODELS = {
    "mf": MF,
    "lgn": LightGCN,
    "lgnssm": LightGCNSSM,
    "radj": rAdjGCN,
    "sage": GraphSAGE,
    "gnn": GNN,
    "tgrec": TGRec,
    "lightsage": LightSAGE,
    "sasrec": SASRec,
}
