"""Generate the rAdjGCN fixtures by running the REFERENCE's own model/radj.py.

Run where the reference is mounted (see make_golden.py, whose shims, tiny
graph and dataset protocol this script imports unchanged):

    python tests/golden/make_golden_radj.py

For every (r, d, L) below: model/radj.py's rAdjGCN on tiny_graph(1) (200 x 50,
1 000 edges with duplicates, one isolated item), the triples recipe of the
lgcn_* fixtures (64 triples, four repeated users), the reference's own
forward / bpr_loss / stageOne.  Writes radj_r{100 r:03d}_d{D}_L{L}.npz with the
lgcn_* keys (without out_radj) plus ``r``.  No committed file may exceed
1 MiB: where the arrays of one configuration do not fit, ``grad``,
``emb_step1`` and ``emb_step2`` go to a sibling ``..._steps.npz``
(tests/radj_common.py loads the two as one fixture).
"""
from __future__ import annotations

import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from make_golden import OUT, REF, TinyDataset, install_shims, tiny_graph  # noqa: E402

CONFIGS = ((0.3, 64, 3), (0.7, 32, 2), (0.0, 16, 1), (1.0, 128, 3), (0.3, 256, 1))
MAX_BYTES = 1 << 20
STEP_KEYS = ("grad", "emb_step1", "emb_step2")


def stem(r, dim, L):
    return f"radj_r{int(round(100 * r)):03d}_d{dim}_L{L}"


def main():
    sys.dont_write_bytecode = True
    sys.argv = ["make_golden_radj"]
    sys.path.insert(0, REF)
    install_shims()
    from model import radj as ref_radj  # noqa: E402  (reference)

    n_users, m_items = 200, 50
    u, i = tiny_graph(1)
    ds = TinyDataset(u, i, n_users, m_items)
    for r, dim, L in CONFIGS:
        cfg = {"recdim": dim, "layer": L, "lr": 1e-3, "decay": 1e-4, "device": "cpu",
               "bpr_batch_size": 64, "r": r}
        g = torch.Generator().manual_seed(dim * 10 + L + int(round(1000 * r)))
        E0 = torch.randn(n_users + m_items, dim, generator=g) * 0.1
        m = ref_radj.rAdjGCN(cfg, ds)
        m.all_embedding.weight.data.copy_(E0)
        with torch.no_grad():
            ou, oi = m.forward()
            layers = [E0]
            x = E0
            for conv in m.layers:
                x = conv(x)
                layers.append(x)
        B = 64
        trip = np.stack([
            np.random.default_rng(7).integers(0, n_users, B),
            np.random.default_rng(8).integers(0, m_items - 1, B),
            np.random.default_rng(9).integers(0, m_items - 1, B)], 1)
        trip[:4, 0] = trip[4:8, 0]  # duplicate users inside the batch
        tu, tp, tn = (torch.tensor(trip[:, k]) for k in range(3))
        loss, reg = m.bpr_loss(tu, tp, tn)
        m.all_embedding.weight.grad = None
        (loss + cfg["decay"] * reg).backward()
        grad = m.all_embedding.weight.grad.detach().clone()
        m.all_embedding.weight.grad = None
        steps, step_losses = [], []
        for _ in range(2):
            step_losses.append(float(m.stageOne(tu, tp, tn)))
            steps.append(m.all_embedding.weight.detach().clone())
        arrs = dict(
            train_user=u, train_item=i, n_users=n_users, m_items=m_items, dim=dim,
            n_layers=L, lr=cfg["lr"], decay=cfg["decay"], r=r, emb0=E0.numpy(),
            out=torch.cat([ou, oi]).numpy(), layers=torch.stack(layers).numpy(),
            triples=trip, loss=float(loss), reg=float(reg), grad=grad.numpy(),
            emb_step1=steps[0].numpy(), emb_step2=steps[1].numpy(),
            step_losses=np.array(step_losses))
        path = os.path.join(OUT, stem(r, dim, L) + ".npz")
        side = os.path.join(OUT, stem(r, dim, L) + "_steps.npz")
        np.savez_compressed(path, **arrs)
        if os.path.exists(side):
            os.remove(side)
        if os.path.getsize(path) > MAX_BYTES:
            np.savez_compressed(path, **{k: v for k, v in arrs.items() if k not in STEP_KEYS})
            np.savez_compressed(side, **{k: arrs[k] for k in STEP_KEYS})
        sizes = [os.path.getsize(p) for p in (path, side) if os.path.exists(p)]
        assert max(sizes) <= MAX_BYTES, (path, sizes)
        print("radj", r, dim, L, float(loss), float(reg), sizes)


if __name__ == "__main__":
    main()
