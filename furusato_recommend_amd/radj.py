"""rAdjGCN: LightGCN with the r-adjusted normalisation (model/radj.py).

Drop-in for ``model.radj.rAdjGCN`` (registered as 'radj' in main.py:36,
option ``--r`` = ``config["r"]``, parse.py:49): the propagation is

    y_i = Σ_{(j→i)} x_j / (deg_j^r · deg_i^(1−r))        (model/radj.py:28-44)

and everything else is LightGCN: the same driver surface, BPR loss, Adam and
the ``state_dict`` key ``all_embedding.weight``.  r = 0.5 is LightGCN itself
(bit for bit: the graph then carries no scales of its own), r = 0 the mean
over neighbours, r = 1 the column-normalised walk.  The propagation matrix
Â_r = D^−(1−r) A D^−r is not symmetric for r ≠ 0.5; the engine's backward
applies its transpose by swapping the two scales of the same launch
(engine.PropagationEngine._prop).  ``config["edge_weight"]``
together with r ≠ 0.5 is refused (ValueError).
"""
from __future__ import annotations

from .lightgcn import LightGCN


class rAdjGCN(LightGCN):  # noqa: N801  (the reference's class name)
    """model/radj.py:47-154 on MI355X.  ``config["dropout"]`` is refused
    (ValueError): edge dropout and the scales are not combined."""

    edge_dropout_supported = False

    def _graph_r(self, config) -> float:
        return float(config.get("r", 0.5))
