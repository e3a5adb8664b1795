"""The seed pipeline shared by the three LightGCN losses (csrc/seedrun.h).

One workspace layout: for the same number of (node, occurrence) pairs and the
same n_nodes, mirec_bpr_seed_workspace, mirec_ssm_seed_workspace and
mirec_ssm_shared_seed_workspace return the same byte count, on either side of
the sort threshold (8 190 and 8 193 pairs), and each seed entry refuses a
workspace one byte short of it with MIREC_ERR_WORKSPACE.

One step: a train_step* call that sets edge dropout and is then refused for
its loss argument leaves the engine without dropout, so that the next step
equals, bit for bit, the same step on a fresh engine.

Graph: tests/ssm_common.py's 300 users x 40 items, d = 16."""
import ctypes

import numpy as np
import pytest
import torch

from tests.ssm_common import MI, NU, N, Ref

pytestmark = pytest.mark.gpu
D, L = 16, 2
LR, DECAY, TEMP = 1e-2, 1e-3, 0.2


def _api():
    from furusato_recommend_amd import _lib
    return _lib, _lib.lib, _lib.stream_handle()


# (B,), (B, K), (B, M) of the three losses for one pair count n
SHAPES = {8190: ((2730,), (1365, 4), (4000, 190)),
          8193: ((2731,), (2731, 1), (4000, 193))}


@pytest.mark.parametrize("n", sorted(SHAPES))
def test_one_workspace_layout(n):
    _lib, lib, st = _api()
    (B,), (Bs, K), (Bh, M) = SHAPES[n]
    assert 3 * B == (2 + K) * Bs == 2 * Bh + M == n
    nb = [ctypes.c_size_t(0) for _ in range(3)]
    assert lib.mirec_bpr_seed_workspace(B, N, ctypes.byref(nb[0])) == _lib.MIREC_OK
    assert lib.mirec_ssm_seed_workspace(Bs, K, N, ctypes.byref(nb[1])) == _lib.MIREC_OK
    assert lib.mirec_ssm_shared_seed_workspace(Bh, M, N, ctypes.byref(nb[2])) == _lib.MIREC_OK
    need = nb[0].value
    assert need > 4 * n and nb[1].value == need and nb[2].value == need

    # every buffer at the size a full call reads or writes, every id 0
    def f32(*s):
        return torch.zeros(*s, dtype=torch.float32, device="cuda")

    def i32(*s):
        return torch.zeros(*s, dtype=torch.int32, device="cuda")
    out, emb, rows = f32(N, D), f32(N, D), f32(Bh + M, D)
    ids, coef = i32(n), f32(n)
    keys, vals, ks = i32(n), i32(n), i32(n)
    slot = torch.full((N,), -1, dtype=torch.int32, device="cuda")
    seed_p, seed_e = f32(n, D), f32(n, D)
    ws = torch.zeros(need, dtype=torch.uint8, device="cuda")
    o, e, i, c = out.data_ptr(), emb.data_ptr(), ids.data_ptr(), coef.data_ptr()
    tail = (slot.data_ptr(), seed_p.data_ptr(), seed_e.data_ptr(), ks.data_ptr(), ws.data_ptr())

    def bpr(nbytes):
        return lib.mirec_bpr_seed(o, e, N, NU, D, B, i, i, i, c, keys.data_ptr(), vals.data_ptr(),
                                  DECAY, 1.0, L, *tail, nbytes, st)

    def ssm(nbytes):
        return lib.mirec_ssm_seed(o, e, N, NU, D, Bs, K, i, c, c, rows.data_ptr(),
                                  keys.data_ptr(), vals.data_ptr(), DECAY, 1.0, L, *tail, nbytes,
                                  st)

    def shared(nbytes):
        return lib.mirec_ssm_shared_seed(o, e, N, NU, D, Bh, M, i, c, rows.data_ptr(),
                                         keys.data_ptr(), vals.data_ptr(), DECAY, 1.0, L, *tail,
                                         nbytes, st)
    for call in (bpr, ssm, shared):
        assert call(need - 1) == _lib.ERR_WORKSPACE, call.__name__
    torch.cuda.synchronize()
    assert int((slot != -1).sum()) == 0 and not bool(seed_p.any())   # nothing was launched


def _i32(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().int().contiguous()


@pytest.fixture(scope="module")
def ref():
    return Ref()


@pytest.fixture(scope="module")
def graph(ref):
    from furusato_recommend_amd.graph import Graph
    return Graph.from_interactions(ref.ds.trainUser, ref.ds.trainItem, NU, MI, "cuda:0")


@pytest.mark.parametrize("loss", ["bpr", "ssm", "shared"])
def test_refused_step_leaves_no_dropout(ref, graph, loss):
    from furusato_recommend_amd.engine import AdamState, PropagationEngine
    u, p, neg = ref.batch(0, 4)                       # 64 pairs, 4 negatives each
    u, p = _i32(u), _i32(p)
    K, M = neg.shape[1], 24

    def run(refuse):
        eng = PropagationEngine(graph, D, L, 64, n_neg=K, n_shared=M)
        E = ref.emb(D).clone().cuda()
        adam = AdamState(E, lr=LR)
        if loss == "bpr":       # no shape check of its own: a batch above max_batch
            step, good, rest = eng.train_step, _i32(neg[:, 0]), (DECAY,)
            bad = (torch.cat([u, u[:1]]), torch.cat([p, p[:1]]), torch.cat([good, good[:1]]))
        elif loss == "ssm":     # neg [B] in place of [B, K]
            step, good, rest = eng.train_step_ssm, _i32(neg), (DECAY, TEMP)
            bad = (u, p, _i32(neg[:, 0]))
        else:                   # shared [1, M] in place of [M]
            step, good, rest = eng.train_step_ssm_shared, _i32(np.arange(M)), (DECAY, TEMP)
            bad = (u, p, good.view(1, M))
        if refuse:
            with pytest.raises(ValueError):
                step(E, adam, *bad, *rest, dropout=(0.5, 77))
            assert eng._drop is None
        out = float(step(E, adam, u, p, good, *rest))
        torch.cuda.synchronize()
        return out, E

    got, want = run(True), run(False)
    assert np.isfinite(want[0]) and got[0] == want[0]
    assert torch.equal(got[1].view(torch.int32), want[1].view(torch.int32))
