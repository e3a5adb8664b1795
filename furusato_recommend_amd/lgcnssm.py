"""LightGCNSSM: LightGCN trained with the sampled-softmax loss (the intent of
model/lgcnssm.py, registered as 'lgnssm').

The reference file is unfinished: ``neg_size`` is undefined, ``softmax_loss``
still computes the BPR softplus, and ``OneEpoch`` slices ``neg_size *
bpr_batch_size`` rows of triples its sampler never produces.  This class is
``LightGCN`` with ``config["loss"]`` defaulting to "ssm": K =
``config["neg_size"]`` negatives per positive, temperature
``config["ssm_temp"]``, the loss of DESIGN.md §18 (Wu et al., "On the
Effectiveness of Sampled Softmax Loss for Item Recommendation"); with K = 1
and temperature 1 it is LightGCN's BPR loss.  Everything else — the driver
surface, the ``state_dict`` key, edge weights, edge dropout — is LightGCN's.
"""
from __future__ import annotations

from .lightgcn import LightGCN


class LightGCNSSM(LightGCN):
    """model/lgcnssm.py:44-151 as it is evidently meant, on MI355X."""

    default_loss = "ssm"
