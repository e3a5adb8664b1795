"""csrc/ssm_shared.hip and the shared-set sampler / mask of csrc/sampler.hip
called directly through the C ABI, every width, against float64 numpy:
mirec_ssm_shared_keys, mirec_ssm_shared_mask (with and without the CSR's
sorted rows), mirec_ssm_shared_forward, mirec_ssm_shared_loss,
mirec_ssm_shared_seed / mirec_bpr_seed_reset (both sorts) and
mirec_shared_sample against its host twin.

Conventions (tests/test_ssm_kernels.py's).  Every output buffer starts as one
NaN bit pattern and is larger than what the kernel should write; untouched
regions are compared bitwise.  Every call runs twice into fresh buffers and
must repeat bitwise.  Integer outputs are compared exactly.

Tolerance (that file's protocol).  Each quantity is evaluated a second time on
the CPU in float32 numpy with the same max-subtracted algorithm, every sum one
term at a time in index order (shared_f32 / seeds_f32 below), and e32 is that
evaluation's error against float64.  A row of g or of the seeds is measured
as max_col |got - ref| / S with S = max_col of the sum of the absolute
products behind the row (a seed run's user entry counts its M + 1 rows, a
shared entry its B rows; over L + 1); a per-pair scalar as |got - ref| /
max(|ref|, floor), floor = 2^-24 A_t, A_t = (sum |out_u out_p| + max over
the unmasked j of sum |out_u out_nj|) / temp (times grad_scale / (B temp) for
coef and coef_pos; reg: 2^-24 reg).  A case passes when err <= FACTOR *
max(e32, 2^-24).

Factors in force (FACTOR): 2 for reg_shared and seed_e, 4 for terms, reg and
coef_pos, 8 for g and seed_p, 16 for coef and loss: each the next power of two
above the largest ratio measured below (tests/test_ssm_kernels.py's factors, 8
/ 16 / 32, were the starting point; none was exceeded).

Measured on an MI355X: the largest err / max(e32, 2^-24) over the cases of a
width, i.e. the factor each quantity needs:

    D       terms     reg  reg_sh    coef coef_pos       g    loss  seed_p  seed_e
    4        1.63    1.55    1.19    1.28     1.13    1.38    2.15    1.23    1.16
    8        3.17    1.05    1.02    5.79     1.86    6.08   11.22    6.11    1.01
    16       2.14    2.43    1.48   11.13     2.28    1.65    2.50    1.57    1.03
    32       2.27    1.29    1.49    1.89     2.13    1.29    1.34    1.55    1.02
    64       1.20    1.03    1.32    3.46     1.21    2.93    2.88    2.93    1.20
    128      1.31    1.49    1.01    1.37     1.00    1.39    3.66    1.39    1.08
    256      1.96    1.40    1.12    1.42     2.00    1.48    1.53    1.48    1.00

The largest: coef 6.5e-6 against e32 5.9e-7 (D = 16, B = 5, M = 257, temp 1),
loss 6.7e-7 against 4.7e-8 (D = 8, B = 65, M = 2, temp 0.2), g 3.3e-5 of S
against 5.5e-6 and the seed_p row it feeds (D = 8, B = 257, M = 63, temp 0.2).
Each of these batches holds the pair with one candidate 120 (temp 0.2: 600)
above its positive, the source of the largest ratios in
tests/test_ssm_kernels.py (the float32 rounding of that score passes through
the exponential into the pair's weights, and its term is the largest of the
batch); that it is the source here too has not been checked pair by pair.

Shapes.  For every D: (B, M) in (1, 1), (3, 65), (64, 64), (65, 2), (257, 63),
(5, 257) — across a 64-wide tile of the score kernel in both directions, all
below 8 192 keys (the small sort) — and one more batch whose sorted keys hold
runs of 1, 2, LPR-1, LPR, LPR+1 and 2 LPR+3 entries (LPR = D / 4: the seed
walk's round); at D = 4 also (4000, 257): 8 257 keys, the radix sort.  temp in
(1, 0.2), grad_scale in (1, 0.25).

Graph: 40 users x 300 items.  User 0 has no interaction, user 1 one, user 2
ninety, user 3 holds items 0 .. 149 and 299 — the pool every shared set is
drawn from, so a pair of user 3 has every candidate masked; users 5 .. 12 hold
items of 150 .. 297 only (none of their candidates is masked by the graph).

Dedicated pairs, as many as the batch admits (a batch shorter than five takes
a rotating subset; test_cases_cover_every_kind holds the coverage):
  allmask  user 3: terms = 0, coef_pos = 0, its coef row all zero, exactly
  posmask  user 5 with pos = shared[0], not an interaction of user 5: masked
           by the second clause alone
  zero     user 6 with a zero row of out: every weight 1 / (1 + #unmasked)
  big      user 7, one candidate with s - s+ = 120 at temp 1
  small    user 8, every candidate with s - s+ < -100
and from five shared slots / 16 pairs on: shared[-1] = shared[0] (a repeated
id), item 299 = m_items - 1 and item 0 in the set, users 0 and n_users - 1,
and id 20 as a shared slot, as the positive of another pair and as the user
of two further pairs (item node 20's run mixes positive and shared
occurrences; user node 20's run has two user occurrences).
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

from tests.ssm_common import F32, U24

pytestmark = pytest.mark.gpu

DIMS = (4, 8, 16, 32, 64, 128, 256)
SHAPES = ((1, 1), (3, 65), (64, 64), (65, 2), (257, 63), (5, 257))
CANARY = 0x7FC5A5A5
PAD = 7
TINY = 2.0 ** -126
NU, MI = 40, 300
NN = NU + MI
DECAY = 1e-4
FACTOR = {"terms": 4, "reg": 4, "reg_shared": 2, "coef": 16, "coef_pos": 4, "g": 8,
          "loss": 16, "seed_p": 8, "seed_e": 2}
KINDS = ("allmask", "posmask", "zero", "big", "small")
_SPECIAL_USER = {"allmask": 3, "posmask": 5, "zero": 6, "big": 7, "small": 8}
POOL = np.r_[np.arange(150), MI - 1]
SMALL_POS = 298


# ------------------------------------------------------------------ plumbing
def _api():
    from furusato_recommend_amd import _lib
    return _lib.lib, _lib.stream_handle()


def _canary_i32(*shape):
    return torch.full(shape, CANARY, dtype=torch.int32, device="cuda")


def _canary_f32(*shape):
    return _canary_i32(*shape).view(torch.float32)


def _canary_u8(n):
    return torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")


def _bits(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return a
    return a.view(np.int32) if a.dtype != np.int32 else a


def _is_canary(a):
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint8:
        return bool(np.all(a == 0xA5))
    return bool(np.all(_bits(a) == CANARY))


def _same_bits(r1, r2):
    assert r1.keys() == r2.keys()
    for k in r1:
        assert np.array_equal(_bits(r1[k]), _bits(r2[k])), k


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _np(t):
    return t.cpu().numpy().copy()


def _bound(name, e32):
    return FACTOR[name] * max(e32, U24)


def _report(tag, name, err, e32):
    print(f"[ssh] {tag} {name}: err={err:.3e} e32={e32:.3e} "
          f"err/e32={err / max(e32, U24):.2f} bound={_bound(name, e32):.3e}")


def _scalar_err(got, ref, floor):
    return np.abs(np.asarray(got, np.float64) - ref) / np.maximum(np.abs(ref), floor)


# --------------------------------------------------------------------- graph
@functools.lru_cache(maxsize=None)
def _interactions():
    rng = np.random.default_rng(31)
    rows = {0: np.array([], np.int64), 1: np.array([10]), 2: rng.choice(MI, 90, replace=False),
            3: POOL.copy()}
    for u in range(4, NU):
        if 5 <= u <= 12:
            rows[u] = 150 + rng.choice(148, int(rng.integers(3, 9)), replace=False)
        else:
            rows[u] = rng.choice(MI, int(rng.integers(3, 40)), replace=False)
    rows[4] = rng.choice(MI, 75, replace=False)
    u = np.concatenate([np.full(len(r), k) for k, r in rows.items()])
    i = np.concatenate(list(rows.values()))
    dup = rng.choice(len(u), 25, replace=False)               # multi-edges
    u, i = np.concatenate([u, u[dup]]), np.concatenate([i, i[dup]])
    order = rng.permutation(len(u))
    return u[order].astype(np.int64), i[order].astype(np.int64)


@functools.lru_cache(maxsize=None)
def _member():
    """member[u, i]: item i is a training positive of user u."""
    u, i = _interactions()
    m = np.zeros((NU, MI), bool)
    m[u, i] = True
    deg = np.bincount(u, minlength=NU)
    assert deg[0] == 0 and deg[1] == 1 and deg[2] >= 70 and deg[3] >= 70 and deg[4] >= 70
    assert m[3][POOL].all() and not m[5:13][:, POOL].any()
    return m


@pytest.fixture(scope="module")
def graphs():
    """The graph with its sorted user rows, and the same graph whose CSR does
    not carry them (the mask kernel then scans the rows)."""
    from furusato_recommend_amd.graph import Graph
    u, i = _interactions()
    a = Graph.from_interactions(u, i, NU, MI, "cuda:0")
    b = Graph.from_interactions(u, i, NU, MI, "cuda:0")
    assert a.csr.n_sorted >= NU and a.csr.col_sorted
    b.csr.col_sorted, b.csr.n_sorted = None, 0
    return a, b


def numpy_mask(users, pos, shared):
    return _member()[users][:, shared] | (np.asarray(shared)[None, :] == np.asarray(pos)[:, None])


# ---------------------------------------------------------------- references
def shared_ref(out, emb, users, pos, shared, mask, decay, temp, gs, L):
    """float64: the per-pair quantities, g [B + M, D], the loss, the seed
    tables over all nodes and the normalisers."""
    o, e = out.astype(np.float64), emb.astype(np.float64)
    u, p, n = np.asarray(users), NU + np.asarray(pos), NU + np.asarray(shared)
    B, M = len(u), len(n)
    ou, op, on = o[u], o[p], o[n]
    sp = (ou * op).sum(1) / temp
    s = ou @ on.T / temp
    sm = np.where(mask, -np.inf, s)
    mx = np.maximum(sp, sm.max(1))
    ex = np.exp(sm - mx[:, None])
    z = np.exp(sp - mx) + ex.sum(1)
    terms = (mx - sp) + np.log(z)
    coef = gs * (ex / z[:, None]) / (B * temp)
    cpos = coef.sum(1)
    g = np.concatenate([coef @ on - cpos[:, None] * op, coef.T @ ou])
    Sg = np.concatenate([np.abs(coef) @ np.abs(on) + np.abs(cpos)[:, None] * np.abs(op),
                         np.abs(coef).T @ np.abs(ou)])
    reg = 0.5 * ((e[u] ** 2).sum(1) + (e[p] ** 2).sum(1))
    reg_sh = 0.5 * (e[n] ** 2).sum(1)
    loss = terms.mean() + decay * (reg.sum() + reg_sh.sum()) / B
    gp, S, cnt = np.zeros_like(o), np.zeros_like(o), np.zeros(len(o))
    np.add.at(gp, u, g[:B])
    np.add.at(S, u, Sg[:B])
    np.add.at(gp, p, -cpos[:, None] * ou)
    np.add.at(S, p, np.abs(cpos)[:, None] * np.abs(ou))
    np.add.at(gp, n, g[B:])
    np.add.at(S, n, Sg[B:])
    np.add.at(cnt, np.concatenate([u, p, n]), 1.0)
    absdot = np.abs(ou) @ np.abs(on).T
    A = ((np.abs(ou * op)).sum(1) + np.where(mask, 0.0, absdot).max(1)) / temp
    return dict(terms=terms, coef=coef, coef_pos=cpos, g=g, Sg=Sg.max(1), reg=reg,
                reg_shared=reg_sh, loss=float(loss), x=s - sp[:, None], A=A,
                gp=gp * (1.0 / (L + 1)), ge=decay * cnt[:, None] * e / B * gs,
                S=S.max(1) / (L + 1))


def shared_f32(out, emb, users, pos, shared, mask, decay, temp, gs):
    """The same quantities in float32 numpy: the same max-subtracted
    algorithm, every sum one term at a time in index order."""
    u, p, n = np.asarray(users), NU + np.asarray(pos), NU + np.asarray(shared)
    B, M, D = len(u), len(n), out.shape[1]
    fb, ft = F32(B), F32(temp)
    ou, op, on = out[u], out[p], out[n]
    ps, s = np.zeros(B, F32), np.zeros((B, M), F32)
    for d in range(D):
        ps = ps + ou[:, d] * op[:, d]
        s = s + ou[:, d, None] * on[None, :, d]
    ps, s = ps / ft, s / ft
    mx = np.maximum(ps, np.where(mask, -np.inf, s).max(1)).astype(F32)
    with np.errstate(over="ignore", under="ignore"):
        e_pos = np.exp(ps - mx)
        ex = np.where(mask, F32(0), np.exp(s - mx[:, None])).astype(F32)
        s_neg = np.zeros(B, F32)
        for j in range(M):
            s_neg = s_neg + ex[:, j]
        z = e_pos + s_neg
        terms = np.where(mx == ps, np.log1p(s_neg), (mx - ps) + np.log(z)).astype(F32)
    scale = F32(gs) * (F32(1) / (z * fb * ft))
    coef = scale[:, None] * ex
    cpos = scale * s_neg
    gu = np.zeros((B, D), F32)
    for j in range(M):
        gu = gu + coef[:, j, None] * on[j]
    gu = gu - cpos[:, None] * op
    gs_ = np.zeros((M, D), F32)
    for t in range(B):
        gs_ = gs_ + coef[t][:, None] * ou[t]
    eu, ep, en = emb[u], emb[p], emb[n]
    reg = F32(0.5) * ((eu * eu).sum(1, dtype=F32) + (ep * ep).sum(1, dtype=F32))
    reg_sh = F32(0.5) * (en * en).sum(1, dtype=F32)
    loss = terms.sum(dtype=F32) / fb + F32(decay) * ((reg.sum(dtype=F32)
                                                      + reg_sh.sum(dtype=F32)) / fb)
    res = dict(terms=terms, coef=coef, coef_pos=cpos, g=np.concatenate([gu, gs_]), reg=reg,
               reg_shared=reg_sh, loss=loss)
    for k, a in res.items():
        assert a.dtype == F32, k
    return res


def occurrence_keys(users, pos, shared):
    return np.concatenate([users, NU + np.asarray(pos), NU + np.asarray(shared)]).astype(np.int64)


def seeds_f32(out, emb, users, f32, keys, decay, gs, L):
    """seed_p / seed_e of every head in float32, each run accumulated one
    entry at a time in stable sorted order: {head q: (row_p, row_e)}."""
    B, n = len(users), len(keys)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    re1 = F32(F32(decay) / F32(B) * F32(gs))
    div = F32(L + 1)
    res, q = {}, 0
    while q < n:
        node, gp, ge = ks[q], np.zeros(out.shape[1], F32), np.zeros(out.shape[1], F32)
        q2 = q
        while q2 < n and ks[q2] == node:
            occ = int(order[q2])
            if occ < B:
                gp = gp + f32["g"][occ]
            elif occ < 2 * B:
                gp = gp - f32["coef_pos"][occ - B] * out[users[occ - B]]
            else:
                gp = gp + f32["g"][occ - B]
            ge = ge + re1 * emb[node]
            q2 += 1
        res[q] = (gp / div, ge)
        q = q2
    return res


# --------------------------------------------------------------------- cases
def _run_lengths(D):
    L = D // 4
    return sorted({1, 2, L - 1, L, L + 1, 2 * L + 3} - {0})


def _kinds(D, B):
    k = min(B, 5)
    off = DIMS.index(D) if B < 5 else 0
    return [KINDS[(off + i) % 5] for i in range(k)]


@functools.lru_cache(maxsize=None)
def _case(D, B, M, runs=False):
    """out, emb (float32 [NN, D]), users, pos [B], shared [M], where[kind] =
    the pair of each dedicated kind.  ``runs``: the fillers' positives (and
    users) are grouped so that the sorted keys hold a run of every length of
    _run_lengths(D)."""
    rng = np.random.default_rng(1000003 * D + 1009 * B + M + (7 if runs else 0))
    out = (rng.standard_normal((NN, D)) * 0.5).astype(F32)
    emb = (rng.standard_normal((NN, D)) * 0.3).astype(F32)
    shared = rng.choice(POOL, M).astype(np.int64)
    if M >= 2:
        shared[-1] = shared[0]
    if M >= 5:
        shared[1], shared[2], shared[3] = MI - 1, 0, 20
    kinds = _kinds(D, B)
    nfill = B - len(kinds)
    fu = rng.integers(13, NU, nfill)
    fp = rng.integers(0, SMALL_POS, nfill)
    if runs:
        R = _run_lengths(D)
        assert nfill >= sum(R) and nfill >= sum(R[:-1])
        # positives: items 200, 201, .. in runs of every length; users: 13, 14, ..
        # in runs of every length but the longest
        fp[: sum(R)] = np.concatenate([np.full(r, 200 + i) for i, r in enumerate(R)])
        fp[sum(R):] = rng.integers(230, SMALL_POS, nfill - sum(R))
        fu[: sum(R[:-1])] = np.concatenate([np.full(r, 13 + i) for i, r in enumerate(R[:-1])])
        fu[sum(R[:-1]):] = rng.integers(13 + len(R), NU - 1, nfill - sum(R[:-1]))
    elif nfill >= 11:
        fu[0], fu[1], fp[2], fp[3] = 0, NU - 1, MI - 1, 0
        if M >= 5:
            fp[4], fu[5], fu[6] = 20, 20, 20
    su, sp_ = [], []
    for k in kinds:
        su.append(_SPECIAL_USER[k])
        sp_.append({"posmask": int(shared[0]), "small": SMALL_POS}.get(k, int(rng.integers(240, 298))))
    users = np.concatenate([fu, su]).astype(np.int64)
    pos = np.concatenate([fp, sp_]).astype(np.int64)
    perm = rng.permutation(B)
    users, pos = users[perm], pos[perm]
    where = {k: int(np.nonzero(users == _SPECIAL_USER[k])[0][0]) for k in kinds}
    o64 = out.astype(np.float64)
    if "zero" in where:
        out[6] = 0
    if "big" in where:
        x = (o64[NU + shared] - o64[NU + pos[where["big"]]]) @ o64[7]
        j0 = int(np.abs(x).argmax())
        out[7] = (o64[7] * (120.0 / x[j0])).astype(F32)
    if "small" in where:
        v = o64[8] / np.linalg.norm(o64[8])
        out[8], out[NU + SMALL_POS] = (2 * v).astype(F32), (100 * v).astype(F32)
    for a in (out, emb, users, pos, shared):
        a.setflags(write=False)
    return out, emb, users, pos, shared, where


def _runs_batch(D):
    return sum(_run_lengths(D)) + 24


def _all_cases():
    c = [(D, B, M, False) for D in DIMS for (B, M) in SHAPES]
    c += [(D, _runs_batch(D), 5, True) for D in DIMS]
    return c + [(4, 4000, 257, False)]


def _sorted_layout(keys):
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    heads = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
    lens = np.diff(np.r_[heads, len(keys)])
    return order, ks, heads, lens


def test_cases_cover_every_kind():
    """Host-side: the cases have the layout the GPU tests rely on."""
    member = _member()
    fractions = []
    for D in DIMS:
        seen = set()
        for (B, M) in SHAPES:
            out, emb, users, pos, shared, where = _case(D, B, M)
            mask = numpy_mask(users, pos, shared)
            ref = shared_ref(out, emb, users, pos, shared, mask, DECAY, 1.0, 1.0, 3)
            seen |= set(where)
            if B >= 5:
                assert set(where) == set(KINDS)
            assert 2 * B + M <= 8192
            x = ref["x"]
            for k, t in where.items():
                if k == "allmask":
                    assert mask[t].all() and ref["terms"][t] == 0.0
                elif k == "posmask":
                    assert pos[t] == shared[0] and not member[users[t], pos[t]]
                    assert mask[t, 0] and not member[users[t]][shared].any()
                elif k == "zero":
                    assert np.all(x[t] == 0.0) and not mask[t].all()
                elif k == "big":
                    assert not mask[t].any() and abs(x[t].max() - 120.0) < 1e-3
                else:
                    assert not mask[t].any() and np.all(x[t] < -100)
            if M >= 2:
                assert shared[0] == shared[-1]
            if M >= 5 and B >= 16:
                assert 0 in users and NU - 1 in users and MI - 1 in shared and 0 in shared
                assert 20 in shared and 20 in pos and np.sum(users == 20) >= 2
                assert MI - 1 in pos
            if B >= 16:
                fractions.append(mask.mean())
        assert seen == set(KINDS), D
        # the runs batch
        out, emb, users, pos, shared, where = _case(D, _runs_batch(D), 5, True)
        _, ks, heads, lens = _sorted_layout(occurrence_keys(users, pos, shared))
        assert set(_run_lengths(D)) <= set(lens.tolist()), D
        assert set(where) == set(KINDS)
    assert 0.02 < min(fractions) and max(fractions) < 0.6   # the mask is neither empty nor total
    out, emb, users, pos, shared, where = _case(4, 4000, 257)
    assert 2 * 4000 + 257 > 8192 and set(where) == set(KINDS)


# ------------------------------------------------------------------- callers
def _call_mask(lib, st, g, ids, B, M, alloc=None, null=None):
    mask = _canary_u8((alloc or B * M) + PAD)
    a = dict(users=ids[0].data_ptr(), pos=ids[1].data_ptr(), shared=ids[2].data_ptr(),
             mask=mask.data_ptr())
    if null is not None:
        a[null] = None
    rc = lib.mirec_ssm_shared_mask(g.csr_ptr(), a["users"], B, a["pos"], a["shared"], M, NU,
                                   a["mask"], st)
    return rc, mask


def _call_forward(lib, st, out_t, emb_t, D, B, M, ids, mask_t, temp, gs, alloc=None, null=None,
                  n_nodes=NN):
    ab, am = alloc or (B, M)
    n = 2 * ab + am
    r = dict(coef=_canary_f32(ab * am + PAD), coef_pos=_canary_f32(ab + PAD),
             terms=_canary_f32(ab + PAD), reg=_canary_f32(ab + PAD),
             reg_shared=_canary_f32(am + PAD), g=_canary_f32(ab + am + PAD, D),
             keys=_canary_i32(n + PAD), vals=_canary_i32(n + PAD))
    a = {k: v.data_ptr() for k, v in r.items()}
    a.update(out=out_t.data_ptr(), emb=emb_t.data_ptr(), users=ids[0].data_ptr(),
             pos=ids[1].data_ptr(), shared=ids[2].data_ptr(), mask=mask_t.data_ptr())
    if null is not None:
        a[null] = None
    rc = lib.mirec_ssm_shared_forward(a["out"], a["emb"], n_nodes, NU, D, B, M, a["users"],
                                      a["pos"], a["shared"], a["mask"], float(temp), float(gs),
                                      a["coef"], a["coef_pos"], a["terms"], a["reg"],
                                      a["reg_shared"], a["g"], a["keys"], a["vals"], st)
    return rc, r


def _call_seed(lib, st, out_t, emb_t, D, B, M, users_t, fwd, gs, L, ws_short=0, null=None):
    nb = ctypes.c_size_t(0)
    assert lib.mirec_ssm_shared_seed_workspace(B, M, NN, ctypes.byref(nb)) == 0
    ws = torch.zeros(nb.value + 256, dtype=torch.uint8, device="cuda")
    n = 2 * B + M
    r = dict(slot=torch.full((NN,), -1, dtype=torch.int32, device="cuda"),
             seed_p=_canary_f32(n + PAD, D), seed_e=_canary_f32(n + PAD, D),
             keys_sorted=_canary_i32(n + PAD))
    a = dict(out=out_t.data_ptr(), emb=emb_t.data_ptr(), users=users_t.data_ptr(),
             coef_pos=fwd["coef_pos"].data_ptr(), g=fwd["g"].data_ptr(),
             keys=fwd["keys"].data_ptr(), vals=fwd["vals"].data_ptr(), ws=ws.data_ptr())
    a.update({k: v.data_ptr() for k, v in r.items()})
    if null is not None:
        a[null] = None
    rc = lib.mirec_ssm_shared_seed(a["out"], a["emb"], NN, NU, D, B, M, a["users"], a["coef_pos"],
                                   a["g"], a["keys"], a["vals"], float(DECAY), float(gs), L,
                                   a["slot"], a["seed_p"], a["seed_e"], a["keys_sorted"], a["ws"],
                                   nb.value - ws_short, st)
    return rc, r


# ============================================================== 1. the kernels
@pytest.mark.parametrize("D,B,M,runs", [pytest.param(*c, id=f"D{c[0]}-B{c[1]}-M{c[2]}")
                                        for c in _all_cases()])
def test_ssm_shared_kernels(graphs, D, B, M, runs):
    lib, st = _api()
    out, emb, users, pos, shared, where = _case(D, B, M, runs)
    n = 2 * B + M
    out_t, emb_t = _dev(out, F32), _dev(emb, F32)
    ids = [_dev(a, np.int32) for a in (users, pos, shared)]
    keys = occurrence_keys(users, pos, shared)
    order, ks, heads, lens = _sorted_layout(keys)
    nodes = ks[heads]
    # ---- the mask, exactly, with and without the sorted rows
    mask = numpy_mask(users, pos, shared)
    masks = []
    for g in graphs:
        for _ in range(2):
            rc, mt = _call_mask(lib, st, g, ids, B, M)
            assert rc == 0
            got = _np(mt)
            assert np.array_equal(got[:B * M].reshape(B, M), mask.astype(np.uint8))
            assert _is_canary(got[B * M:])
            masks.append(mt)
    mask_t = masks[0]
    fails = []
    for temp, gs, L in ((1.0, 1.0, 3), (0.2, 0.25, 0), (1.0, 0.25, 3), (0.2, 1.0, 0)):
        ref = shared_ref(out, emb, users, pos, shared, mask, DECAY, temp, gs, L)
        f32 = shared_f32(out, emb, users, pos, shared, mask, DECAY, temp, gs)
        s32 = seeds_f32(out, emb, users, f32, keys, DECAY, gs, L)

        def run():
            rc, r = _call_forward(lib, st, out_t, emb_t, D, B, M, ids, mask_t, temp, gs)
            assert rc == 0
            loss, acc = _canary_f32(1 + PAD), _canary_f32(1 + PAD)
            acc[0] = 2.5
            assert lib.mirec_ssm_shared_loss(r["terms"].data_ptr(), r["reg"].data_ptr(),
                                             r["reg_shared"].data_ptr(), B, M, DECAY,
                                             loss.data_ptr(), acc.data_ptr(), st) == 0
            kk = _canary_i32(n + PAD)
            assert lib.mirec_ssm_shared_keys(ids[0].data_ptr(), ids[1].data_ptr(),
                                             ids[2].data_ptr(), B, M, NU, kk.data_ptr(), st) == 0
            rc, sd = _call_seed(lib, st, out_t, emb_t, D, B, M, ids[0], r, gs, L)
            assert rc == 0
            res = {k: _np(v) for k, v in r.items()}
            res.update(loss=_np(loss), acc=_np(acc), keys_only=_np(kk))
            res.update({k: _np(v) for k, v in sd.items()})
            for i in (1, 2):
                assert lib.mirec_bpr_seed_reset(sd["slot"].data_ptr(),
                                                sd["keys_sorted"].data_ptr(), n, st) == 0
                res[f"slot_reset{i}"] = _np(sd["slot"])
            return res

        r = run()
        _same_bits(r, run())
        tag = f"D={D} B={B} M={M} temp={temp} gs={gs} L={L}"
        # integers, exactly
        assert np.array_equal(r["keys"][:n], keys) and np.array_equal(r["keys_only"][:n], keys)
        assert np.array_equal(r["vals"][:n], np.arange(n))
        assert np.array_equal(r["keys_sorted"][:n], ks)
        slot = np.full(NN, -1, np.int64)
        slot[nodes] = heads
        assert np.array_equal(r["slot"], slot)
        assert np.all(r["slot_reset1"] == -1) and np.all(r["slot_reset2"] == -1)
        # canaries
        for k, cnt in (("coef", B * M), ("coef_pos", B), ("terms", B), ("reg", B),
                       ("reg_shared", M), ("g", B + M), ("keys", n), ("vals", n),
                       ("keys_only", n), ("loss", 1), ("acc", 1), ("keys_sorted", n)):
            assert _is_canary(r[k][cnt:]), k
        nonhead = np.ones(n + PAD, bool)
        nonhead[heads] = False
        assert _is_canary(r["seed_p"][nonhead]) and _is_canary(r["seed_e"][nonhead])
        for k, cnt in (("coef", B * M), ("coef_pos", B), ("terms", B), ("reg", B),
                       ("reg_shared", M), ("g", B + M), ("loss", 1)):
            assert np.all(np.isfinite(r[k][:cnt])), k
        # scalars
        coef = r["coef"][:B * M].reshape(B, M)
        assert np.all(coef[mask] == 0.0)                       # exact zeros where masked
        cfloor = ref["A"] * U24 * gs / (B * temp)
        got = {"terms": r["terms"][:B], "reg": r["reg"][:B], "reg_shared": r["reg_shared"][:M],
               "coef_pos": r["coef_pos"][:B], "coef": coef}
        floors = {"terms": ref["A"] * U24, "reg": ref["reg"] * U24,
                  "reg_shared": ref["reg_shared"] * U24, "coef_pos": cfloor,
                  "coef": cfloor[:, None]}
        for k in ("terms", "reg", "reg_shared", "coef", "coef_pos"):
            err = float(_scalar_err(got[k], ref[k], floors[k]).max())
            e32 = float(_scalar_err(f32[k], ref[k], floors[k]).max())
            _report(tag, k, err, e32)
            if not err <= _bound(k, e32):
                fails.append((tag, k, err, e32))
        # rows of g and of the seeds, normalised by the sum of their absolute
        # terms (a row whose every term is below float32's smallest normal
        # number must be zero to that size and stays out of the ratio)
        rows = (("g", r["g"][:B + M], f32["g"], ref["g"], ref["Sg"]),
                ("seed_p", r["seed_p"][heads], np.stack([s32[q][0] for q in heads]),
                 ref["gp"][nodes], ref["S"][nodes]),
                ("seed_e", r["seed_e"][heads], np.stack([s32[q][1] for q in heads]),
                 ref["ge"][nodes], np.abs(ref["ge"][nodes]).max(1)))
        for name, gotr, r32, rf, S in rows:
            live = S >= TINY
            assert np.all(np.abs(gotr[~live]) <= TINY), name
            if name == "seed_e":
                assert live.all()
            if live.any():
                Sl = S[live][:, None]
                err = float((np.abs(gotr[live].astype(np.float64) - rf[live]) / Sl).max())
                e32 = float((np.abs(r32[live].astype(np.float64) - rf[live]) / Sl).max())
                _report(tag, name, err, e32)
                if not err <= _bound(name, e32):
                    fails.append((tag, name, err, e32))
        # the dedicated pairs
        if "allmask" in where:
            t = where["allmask"]
            assert got["terms"][t] == 0 and got["coef_pos"][t] == 0 and np.all(coef[t] == 0)
        if "posmask" in where:
            t = where["posmask"]
            # (slot 0 and its repeat are masked, by this clause alone; the rest is not)
            assert coef[t, 0] == 0 and np.all(mask[t] == (shared == shared[0]))
            assert mask[t].all() or np.any(coef[t][~mask[t]] > 0)
        if "zero" in where:
            t = where["zero"]
            nun = int((~mask[t]).sum())
            c = F32(gs / ((nun + 1) * B * temp))
            assert np.all(np.abs(coef[t][~mask[t]] - c) <= 2 * np.spacing(c)), coef[t]
            lg = F32(np.log(nun + 1.0))
            assert abs(got["terms"][t] - lg) <= 2 * np.spacing(lg)
        if "big" in where:
            t = where["big"]
            xm = float(ref["x"][t].max())
            assert xm > 100
            assert xm * (1 - 1e-3) <= got["terms"][t] <= xm * (1 + 1e-3) + np.log(M + 1.0)
        if "small" in where:
            t = where["small"]
            assert got["terms"][t] == 0 and np.all(coef[t] == 0) and got["coef_pos"][t] == 0
            assert np.all(r["g"][t] == 0)
        # loss
        lerr = abs(float(r["loss"][0]) - ref["loss"]) / abs(ref["loss"])
        le32 = abs(float(f32["loss"]) - ref["loss"]) / abs(ref["loss"])
        _report(tag, "loss", lerr, le32)
        if not lerr <= _bound("loss", le32):
            fails.append((tag, "loss", lerr, le32))
        assert _bits(r["acc"][:1])[0] == _bits(np.array([F32(2.5) + r["loss"][0]], F32))[0]
        # seed_e is one multiply (tests/test_ssm_kernels.py: at most 7 spacings)
        re = (DECAY * lens / B * gs).astype(F32)[:, None]
        exp = re * emb[nodes]
        ulps = np.abs(r["seed_e"][heads].astype(np.float64) - exp) / np.spacing(np.abs(exp))
        assert ulps.max() <= 7, ulps.max()
    assert not fails, fails


# ================================================ 2. independence of the batch
@pytest.mark.parametrize("D", DIMS)
def test_terms_do_not_depend_on_the_other_pairs(graphs, D):
    """terms[t] of the (65, 2) and (257, 63) batches equals, bitwise, terms[0]
    of a one-pair call on pair t alone."""
    lib, st = _api()
    for (B, M) in ((65, 2), (257, 63)):
        out, emb, users, pos, shared, _ = _case(D, B, M)
        out_t, emb_t = _dev(out, F32), _dev(emb, F32)
        ids = [_dev(a, np.int32) for a in (users, pos, shared)]
        rc, mask_t = _call_mask(lib, st, graphs[0], ids, B, M)
        assert rc == 0
        rc, full = _call_forward(lib, st, out_t, emb_t, D, B, M, ids, mask_t, 0.2, 1.0)
        assert rc == 0
        alone = _canary_f32(B)
        s = dict(coef=_canary_f32(M), coef_pos=_canary_f32(1), reg=_canary_f32(1),
                 reg_shared=_canary_f32(M), g=_canary_f32(1 + M, D), keys=_canary_i32(2 + M),
                 vals=_canary_i32(2 + M))
        for t in range(B):
            rc = lib.mirec_ssm_shared_forward(
                out_t.data_ptr(), emb_t.data_ptr(), NN, NU, D, 1, M, ids[0].data_ptr() + 4 * t,
                ids[1].data_ptr() + 4 * t, ids[2].data_ptr(), mask_t.data_ptr() + t * M, 0.2, 1.0,
                s["coef"].data_ptr(), s["coef_pos"].data_ptr(), alone.data_ptr() + 4 * t,
                s["reg"].data_ptr(), s["reg_shared"].data_ptr(), s["g"].data_ptr(),
                s["keys"].data_ptr(), s["vals"].data_ptr(), st)
            assert rc == 0
        assert np.array_equal(_bits(_np(full["terms"])[:B]), _bits(_np(alone)))


# ===================================== 3. against the per-pair kernel (ssm.hip)
@pytest.mark.parametrize("D", [4, 64, 256])
def test_terms_agree_with_the_per_pair_kernel_when_nothing_is_masked(graphs, D):
    """No cell masked (users 5 .. 12, positives outside the pool): terms agree
    with mirec_ssm_forward on neg[t, :] = shared within the sum of the two
    kernels' bounds, and each passes against float64 on its own."""
    from tests import ssm_common
    from tests.test_ssm_kernels import FACTOR as FACTOR_PAIR
    lib, st = _api()
    B, M, temp = 70, 33, 0.2
    rng = np.random.default_rng(500 + D)
    out = (rng.standard_normal((NN, D)) * 0.5).astype(F32)
    emb = (rng.standard_normal((NN, D)) * 0.3).astype(F32)
    users, pos = rng.integers(5, 13, B), rng.integers(150, 298, B)
    shared = rng.choice(POOL, M)
    mask = numpy_mask(users, pos, shared)
    assert not mask.any()
    out_t, emb_t = _dev(out, F32), _dev(emb, F32)
    ids = [_dev(a, np.int32) for a in (users, pos, shared)]
    rc, mask_t = _call_mask(lib, st, graphs[0], ids, B, M)
    assert rc == 0 and not _np(mask_t)[:B * M].any()
    rc, r = _call_forward(lib, st, out_t, emb_t, D, B, M, ids, mask_t, temp, 1.0)
    assert rc == 0
    neg = np.tile(shared, (B, 1))
    neg_t = _dev(neg, np.int32)
    p = dict(coef=_canary_f32(B * M), coef_pos=_canary_f32(B), terms=_canary_f32(B),
             reg=_canary_f32(B), g_u=_canary_f32(B, D), keys=_canary_i32((2 + M) * B),
             vals=_canary_i32((2 + M) * B))
    assert lib.mirec_ssm_forward(out_t.data_ptr(), emb_t.data_ptr(), NN, NU, D, B, M,
                                 ids[0].data_ptr(), ids[1].data_ptr(), neg_t.data_ptr(), temp, 1.0,
                                 p["coef"].data_ptr(), p["coef_pos"].data_ptr(),
                                 p["terms"].data_ptr(), p["reg"].data_ptr(), p["g_u"].data_ptr(),
                                 p["keys"].data_ptr(), p["vals"].data_ptr(), st) == 0
    ref = shared_ref(out, emb, users, pos, shared, mask, DECAY, temp, 1.0, 3)
    f32 = shared_f32(out, emb, users, pos, shared, mask, DECAY, temp, 1.0)
    refp = ssm_common.reference(out, emb, users, pos, neg, NU, DECAY, temp, 1.0, 3)
    f32p = ssm_common.forward_f32(out, emb, users, pos, neg, NU, DECAY, temp, 1.0)
    assert np.allclose(ref["terms"], refp["terms"], rtol=1e-12, atol=1e-14)
    assert np.allclose(ref["A"], refp["A"], rtol=1e-12)
    floor = ref["A"] * U24
    a, b = _np(r["terms"])[:B], _np(p["terms"])
    b_sh = FACTOR["terms"] * max(float(_scalar_err(f32["terms"], ref["terms"], floor).max()), U24)
    b_pp = FACTOR_PAIR["terms"] * max(float(_scalar_err(f32p["terms"], ref["terms"], floor).max()),
                                      U24)
    e_sh = float(_scalar_err(a, ref["terms"], floor).max())
    e_pp = float(_scalar_err(b, ref["terms"], floor).max())
    e_x = float(_scalar_err(a, b.astype(np.float64), floor).max())
    print(f"[ssh] cross D={D}: shared {e_sh:.2e} (bound {b_sh:.2e}) per-pair {e_pp:.2e} "
          f"(bound {b_pp:.2e}) between {e_x:.2e}")
    assert e_sh <= b_sh and e_pp <= b_pp and e_x <= b_sh + b_pp


# ================================================================== 4. sampler
@pytest.mark.parametrize("n_sets,M", [(1, 1), (3, 257), (40, 2048)])
def test_device_sampler_equals_host_sampler(n_sets, M):
    from furusato_recommend_amd import _lib
    tot = n_sets * M

    def run():
        o = _canary_i32(tot + PAD)
        assert _lib.lib.mirec_shared_sample(1000, n_sets, M, ctypes.c_uint64(9),
                                            ctypes.c_uint64(77), o.data_ptr(),
                                            _lib.stream_handle()) == 0
        return dict(o=_np(o))
    r = run()
    _same_bits(r, run())
    h = np.full(tot, -7, np.int32)
    assert _lib.lib.mirec_cpu_shared_sample(1000, n_sets, M, ctypes.c_uint64(9),
                                            ctypes.c_uint64(77), h.ctypes.data, 4) == 0
    assert np.array_equal(r["o"][:tot], h) and _is_canary(r["o"][tot:])
    assert h.min() >= 0 and h.max() < 1000
    o = _canary_i32(8)
    for bad in ((0, 1, 4), (1000, 0, 4), (1000, 1, 0), (1000, 2 ** 16, 2 ** 15)):
        assert _lib.lib.mirec_shared_sample(*bad, ctypes.c_uint64(1), ctypes.c_uint64(0),
                                            o.data_ptr(), _lib.stream_handle()) == 1
    assert _lib.lib.mirec_shared_sample(1000, 1, 4, ctypes.c_uint64(1), ctypes.c_uint64(0), None,
                                        _lib.stream_handle()) == 1
    torch.cuda.synchronize()
    assert _is_canary(_np(o))


# ================================================================= 5. refusals
_BAD = ["m0", "m-1", "batch0", "batch-1", "temp0", "temp-1", "tempnan", "tempinf", "dim12",
        "no_items", "bm_2^31", "2b+m_2^31", "null:out", "null:emb", "null:users", "null:pos",
        "null:shared", "null:mask", "null:coef", "null:coef_pos", "null:terms", "null:reg",
        "null:reg_shared", "null:g", "null:keys", "null:vals"]


@pytest.mark.parametrize("what", _BAD)
def test_forward_refuses_and_writes_nothing(graphs, what):
    lib, st = _api()
    D, B, M, temp, null, n_nodes = 64, 16, 5, 1.0, None, NN
    out, emb, users, pos, shared, _ = _case(64, 64, 64)
    if what.startswith("null:"):
        null = what[5:]
    elif what.startswith("m"):
        M = int(what[1:])
    elif what.startswith("batch"):
        B = int(what[5:])
    elif what.startswith("temp"):
        temp = {"0": 0.0, "-1": -1.0, "nan": float("nan"), "inf": float("inf")}[what[4:]]
    elif what == "dim12":
        D = 12
    elif what == "no_items":
        n_nodes = NU
    elif what == "bm_2^31":
        B, M = 2 ** 16, 2 ** 15
    else:
        B, M = 2 ** 30, 1                                    # 2B + M > 2^31, B M < 2^31
    out_t, emb_t = _dev(out, F32), _dev(emb, F32)
    ids = [_dev(a, np.int32) for a in (users, pos, shared)]
    mask_t = torch.zeros(64 * 64, dtype=torch.uint8, device="cuda")
    for _ in range(2):
        rc, r = _call_forward(lib, st, out_t, emb_t, D, B, M, ids, mask_t, temp, 1.0,
                              alloc=(16, 5), null=null, n_nodes=n_nodes)
        torch.cuda.synchronize()
        assert rc == 1                                       # MIREC_ERR_ARG
        for k, v in r.items():
            assert _is_canary(_np(v)), k


@pytest.mark.parametrize("what", ["m0", "batch0", "bm_2^31", "2b+m_2^31", "null:users",
                                  "null:pos", "null:shared", "null:out"])
def test_keys_mask_loss_and_workspace_refuse(graphs, what):
    lib, st = _api()
    B, M, null = 16, 5, None
    out, emb, users, pos, shared, _ = _case(64, 64, 64)
    if what.startswith("null:"):
        null = what[5:]
    elif what == "m0":
        M = 0
    elif what == "batch0":
        B = 0
    elif what == "bm_2^31":
        B, M = 2 ** 16, 2 ** 15
    else:
        B, M = 2 ** 30, 1
    ids = [_dev(a, np.int32) for a in (users, pos, shared)]
    a = dict(users=ids[0].data_ptr(), pos=ids[1].data_ptr(), shared=ids[2].data_ptr())
    kk = _canary_i32(64)
    a["out"] = kk.data_ptr()
    if null is not None:
        a[null] = None
    assert lib.mirec_ssm_shared_keys(a["users"], a["pos"], a["shared"], B, M, NU, a["out"],
                                     st) == 1
    rc, mask = _call_mask(lib, st, graphs[0], ids, B, M, alloc=64,
                          null={"out": "mask"}.get(null, null))
    torch.cuda.synchronize()
    assert rc == 1 and _is_canary(_np(mask))
    if null is None:
        nb = ctypes.c_size_t(12345)
        assert lib.mirec_ssm_shared_seed_workspace(B, M, NN, ctypes.byref(nb)) == 1
        assert nb.value == 12345
        f = _canary_f32(8)
        for b, m in ((0, 4), (4, 0), (-1, 4)):
            assert lib.mirec_ssm_shared_loss(f.data_ptr(), f.data_ptr(), f.data_ptr(), b, m,
                                             DECAY, f.data_ptr(), None, st) == 1
    else:
        assert lib.mirec_ssm_shared_seed_workspace(16, 5, NN, None) == 1
        f = _canary_f32(8)
        assert lib.mirec_ssm_shared_loss(None, f.data_ptr(), f.data_ptr(), 4, 4, DECAY,
                                         f.data_ptr(), None, st) == 1
        assert lib.mirec_ssm_shared_loss(f.data_ptr(), f.data_ptr(), f.data_ptr(), 4, 4, DECAY,
                                         None, None, st) == 1
    torch.cuda.synchronize()
    assert _is_canary(_np(kk)) and _is_canary(_np(f))


@pytest.mark.parametrize("what", ["short", "null:g", "null:coef_pos", "null:slot", "null:seed_p",
                                  "null:keys_sorted", "null:ws", "layers-1"])
def test_seed_refuses_and_writes_nothing(graphs, what):
    from furusato_recommend_amd._lib import ERR_WORKSPACE
    lib, st = _api()
    D, B, M = 64, 64, 64
    out, emb, users, pos, shared, _ = _case(D, B, M)
    out_t, emb_t = _dev(out, F32), _dev(emb, F32)
    ids = [_dev(a, np.int32) for a in (users, pos, shared)]
    rc, mask_t = _call_mask(lib, st, graphs[0], ids, B, M)
    rc, fwd = _call_forward(lib, st, out_t, emb_t, D, B, M, ids, mask_t, 1.0, 1.0)
    assert rc == 0
    for _ in range(2):
        rc, r = _call_seed(lib, st, out_t, emb_t, D, B, M, ids[0], fwd, 1.0,
                           -1 if what == "layers-1" else 3, ws_short=1 if what == "short" else 0,
                           null=what[5:] if what.startswith("null:") else None)
        torch.cuda.synchronize()
        assert rc == (ERR_WORKSPACE if what == "short" else 1)
        assert np.all(_np(r["slot"]) == -1)
        for k in ("seed_p", "seed_e", "keys_sorted"):
            assert _is_canary(_np(r[k])), k
