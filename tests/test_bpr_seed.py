"""csrc/bpr.hip called directly through the C ABI, every width, against a
float64 autograd reference: mirec_bpr_forward / mirec_bpr_loss (softplus
branches, grad_scale, loss_accum, the loss kernel's stride loop),
mirec_bpr_seed / mirec_bpr_seed_reset (run lengths around every LPR = D/4
boundary of the seed walk, both sorts), mirec_seed_pack / mirec_seed_merge
(the data-parallel exchange) and mirec_seed_dense.

Conventions.  Every output buffer starts as one NaN bit pattern and is larger
than what the kernel should write; untouched regions are compared bitwise.
Every call runs twice into fresh buffers and must repeat bitwise.  Integer
outputs are compared exactly.

Tolerance.  Nothing is a fixed number: each case evaluates the same quantity a
second time on the CPU in float32 (numpy; per-triple dots with
sum(dtype=float32), runs accumulated one entry at a time in sorted order) and
e32 is that evaluation's error against float64.  A seed row q is measured as
max_col |got - ref| / S_q with S_q = max_col sum_i |c_i| |x_i,col| / (L+1)
over the run's entries (cancellation inside a row does not inflate the bound,
a large row does not hide a small one); a per-triple scalar as
|got - ref| / max(|ref|, floor), the floor being 2^-24 times the sum of the
absolute products the scalar is built from (times grad_scale / B for coef).
A case passes when err <= max(FACTOR * e32, FACTOR * 2^-24).

Factor in force: 8 for every quantity (seed_p, seed_e, coef, softplus, reg,
loss); none had to be raised.

Measured on an MI355X: the largest err / max(e32, 2^-24) over the cases of
a width (e32 is floored as the bound floors it: a batch of one triple can
have e32 == 0), i.e. the factor each quantity needs:

    D     seed_p  seed_e   coef  softplus   reg   loss
    4      1.27    0.75    1.86    1.38    1.06   1.38
    8      1.78    0.55    1.37    1.13    1.09   0.41
    16     1.04    0.41    2.75    2.52    1.05   1.00
    32     1.16    0.49    1.23    2.88    1.33   2.41
    64     1.47    0.32    1.47    3.01    1.47   3.31
    128    0.86    0.10    3.48    1.29    1.07   2.37
    256    1.02    0.06    2.30    1.30    1.46   1.93

The largest seed_p error was 9.0e-7 of S_q (D = 256, B = 2731); seed_e
against fp32(decay * cnt / B * grad_scale) * emb[node] differs by at most
2 ulp in every case.

Shapes of the forward cases.  A block handles P = 4 * 64 / LPR triples; the
batches are 1, P-1, P, P+1 and 2P+11 (D = 64 also 1025: the loss kernel's
1024-thread stride loop takes a second trip with one live thread).  Five
triples on dedicated nodes hit x > 20, 19 < x < 20, 0 < |x| < 1e-3,
x < -100 and pos == neg; a batch shorter than five takes a rotating subset
(the batches 1, P-1, P of D = 256 are 1, 3, 4 triples: together they cover
all five, test_forward_cases_cover_every_branch), and the id requirements
(user 0, user n_users-1, item m_items-1, one id used as user and as item)
hold from 16 triples on.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DIMS = (4, 8, 16, 32, 64, 128, 256)
CANARY = 0x7FC5A5A5  # a quiet NaN: no kernel here produces this pattern
U24 = 2.0 ** -24
FACTOR = {"seed_p": 8, "seed_e": 8, "coef": 8, "softplus": 8, "reg": 8, "loss": 8}
PAD = 7  # extra entries / rows behind every output
F32 = np.float32


# ------------------------------------------------------------------ plumbing
def _api():
    from furusato_recommend_amd import _lib
    return _lib.lib, _lib.stream_handle()


def _canary_i32(*shape):
    return torch.full(shape, CANARY, dtype=torch.int32, device="cuda")


def _canary_f32(*shape):
    return _canary_i32(*shape).view(torch.float32)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int32) if a.dtype != np.int32 else a


def _is_canary(a):
    return bool(np.all(_bits(a) == CANARY))


def _same_bits(r1, r2):
    assert r1.keys() == r2.keys()
    for k in r1:
        a, b = r1[k], r2[k]
        if isinstance(a, np.ndarray):
            assert np.array_equal(_bits(a), _bits(b)), k
        else:
            assert a == b, k


def _dev(a, dtype):
    return torch.from_numpy(np.array(a, dtype=dtype, order="C")).cuda()


def _np(t):
    return t.cpu().numpy().copy()


def _bound(name, e32):
    return max(FACTOR[name] * e32, FACTOR[name] * U24)


def _report(tag, name, err, e32):
    print(f"[bpr_seed] {tag} {name}: err={err:.3e} e32={e32:.3e} "
          f"err/e32={err / max(e32, U24):.2f} bound={_bound(name, e32):.3e}")


# ------------------------------------------------------- reference builders
def reference(out, emb, users, pos, neg, n_users, decay, grad_scale, n_layers):
    """float64 autograd: loss = softplus(neg - pos).mean() + decay * 0.5 *
    (|e_u|^2 + |e_p|^2 + |e_n|^2).sum() / B with out and emb as independent
    leaves.  Returns per-triple x, softplus, coef, reg, the loss, the seed
    tables gp (= d loss / d out * grad_scale / (L+1)) and ge (= d loss /
    d emb * grad_scale) over all nodes, the seed_p normaliser S and the
    per-triple sums of absolute products."""
    o = torch.tensor(np.asarray(out, np.float64), requires_grad=True)
    e = torch.tensor(np.asarray(emb, np.float64), requires_grad=True)
    u = torch.as_tensor(np.asarray(users)).long()
    p = torch.as_tensor(np.asarray(pos)).long() + n_users
    n = torch.as_tensor(np.asarray(neg)).long() + n_users
    B = u.numel()
    x = (o[u] * o[n]).sum(1) - (o[u] * o[p]).sum(1)
    x.retain_grad()
    sp = torch.nn.functional.softplus(x, threshold=20)
    reg = 0.5 * ((e[u] ** 2).sum(1) + (e[p] ** 2).sum(1) + (e[n] ** 2).sum(1))
    loss = sp.mean() + decay * reg.sum() / B
    loss.backward()
    coef = x.grad * grad_scale
    od = o.detach().numpy()
    c = np.abs(coef.numpy())[:, None]
    S = np.zeros_like(od)
    un, pn, nn_ = u.numpy(), p.numpy(), n.numpy()
    np.add.at(S, un, c * (np.abs(od[nn_]) + np.abs(od[pn])))
    np.add.at(S, pn, c * np.abs(od[un]))
    np.add.at(S, nn_, c * np.abs(od[un]))
    terms = np.abs(od[un] * od[pn]).sum(1) + np.abs(od[un] * od[nn_]).sum(1)
    return dict(x=x.detach().numpy(), softplus=sp.detach().numpy(), coef=coef.numpy(),
                reg=reg.detach().numpy(), loss=float(loss.detach()),
                gp=o.grad.numpy() * grad_scale / (n_layers + 1),
                ge=e.grad.numpy() * grad_scale,
                S=S.max(1) / (n_layers + 1), terms=terms)


def forward_f32(out, emb, users, pos, neg, n_users, decay, grad_scale):
    """The same per-triple quantities and the loss evaluated in float32 with
    plain numpy (the measure of what float32 can give, not the kernel)."""
    u, p, n = np.asarray(users), np.asarray(pos) + n_users, np.asarray(neg) + n_users
    B = F32(len(u))
    ou, op, on = out[u], out[p], out[n]
    ps = (ou * op).sum(1, dtype=F32)
    ns = (ou * on).sum(1, dtype=F32)
    x = ns - ps
    with np.errstate(over="ignore", under="ignore"):
        sp = np.where(x > 20, x, np.log1p(np.exp(x))).astype(F32)
        sig = np.where(x > 20, F32(1), F32(1) / (F32(1) + np.exp(-x))).astype(F32)
    coef = F32(grad_scale) * sig / B
    eu, ep, en = emb[u], emb[p], emb[n]
    reg = F32(0.5) * ((eu * eu).sum(1, dtype=F32) + (ep * ep).sum(1, dtype=F32)
                      + (en * en).sum(1, dtype=F32))
    loss = sp.sum(dtype=F32) / B + F32(decay) * (reg.sum(dtype=F32) / B)
    assert all(a.dtype == F32 for a in (sp, coef, reg)) and loss.dtype == F32
    return dict(softplus=sp, coef=coef, reg=reg, loss=loss)


def seeds_f32(out, emb, users, pos, neg, n_users, coef32, keys, decay, grad_scale, n_layers):
    """seed_p / seed_e of every head in float32: each run accumulated one
    entry at a time, in stable sorted order.  Returns {head q: (row_p, row_e)}."""
    B = len(users)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    re1 = F32(F32(decay) / F32(B) * F32(grad_scale))
    div = F32(n_layers + 1)
    res, q = {}, 0
    while q < 3 * B:
        node, gp, ge = ks[q], np.zeros(out.shape[1], F32), np.zeros(out.shape[1], F32)
        q2 = q
        while q2 < 3 * B and ks[q2] == node:
            role, t = divmod(int(order[q2]), B)
            c = coef32[t]
            if role == 0:
                gp = gp + c * out[n_users + neg[t]]
                gp = gp - c * out[n_users + pos[t]]
            elif role == 1:
                gp = gp - c * out[users[t]]
            else:
                gp = gp + c * out[users[t]]
            ge = ge + re1 * emb[node]
            q2 += 1
        assert gp.dtype == F32 and ge.dtype == F32
        res[q] = (gp / div, ge)
        q = q2
    return res


def _scalar_err(got, ref, floor):
    return np.abs(got.astype(np.float64) - ref) / np.maximum(np.abs(ref), floor)


# ============================================================ 1. forward/loss
N_USERS, M_ITEMS = 37, 29
KINDS = ("gt20", "19to20", "tiny", "lt-100", "same")
# dedicated nodes of the five branch triples: users 1..5, items 1..9
_SPECIAL = {"gt20": (1, 1, 2, 25.0), "19to20": (2, 3, 4, 19.5), "tiny": (3, 5, 6, 5e-4),
            "lt-100": (4, 7, 8, -120.0), "same": (5, 9, 9, None)}


def _forward_batches(D):
    P = 4 * 64 // (D // 4)
    b = {1, P - 1, P, P + 1, 2 * P + 11}
    if D == 64:
        b.add(1025)
    return sorted(x for x in b if x > 0)


def _special_kinds(batch):
    k = min(batch, 5)
    off = {1: 0, 3: 1, 4: 4}.get(batch, 0)
    return [KINDS[(off + i) % 5] for i in range(k)]


@functools.lru_cache(maxsize=None)
def _forward_case(D, batch):
    """out, emb (float32 [n_nodes, D]), triples, and the kind of each special
    triple's index.  Rows of out are rescaled so that x lands in each branch."""
    rng = np.random.default_rng(1000 * D + batch)
    n_nodes = N_USERS + M_ITEMS
    out = (rng.standard_normal((n_nodes, D)) * 0.5).astype(F32)
    emb = (rng.standard_normal((n_nodes, D)) * 0.3).astype(F32)
    kinds = _special_kinds(batch)
    nfill = batch - len(kinds)
    fu = rng.integers(6, N_USERS, nfill)
    fp = rng.integers(10, M_ITEMS, nfill)
    fn = rng.integers(10, M_ITEMS, nfill)
    if nfill >= 11:
        fu[0], fu[1], fp[2], fn[3] = 0, N_USERS - 1, M_ITEMS - 1, M_ITEMS - 1
        fu[4], fp[5] = 20, 20  # id 20 as a user and as an item: nodes 20 and 57
    users = np.concatenate([fu, [_SPECIAL[k][0] for k in kinds]]).astype(np.int64)
    pos = np.concatenate([fp, [_SPECIAL[k][1] for k in kinds]]).astype(np.int64)
    neg = np.concatenate([fn, [_SPECIAL[k][2] for k in kinds]]).astype(np.int64)
    perm = rng.permutation(batch)
    users, pos, neg = users[perm], pos[perm], neg[perm]
    where = {}
    for k in kinds:
        u, p, n, target = _SPECIAL[k]
        where[k] = int(np.nonzero(users == u)[0][0])
        if target is not None:
            o64 = out.astype(np.float64)
            x0 = o64[u] @ (o64[N_USERS + n] - o64[N_USERS + p])
            out[u] = (o64[u] * (target / x0)).astype(F32)
    out.setflags(write=False)
    emb.setflags(write=False)
    return out, emb, users, pos, neg, where


def _check_branches(x, where):
    for k, t in where.items():
        v = x[t]
        ok = {"gt20": v > 20, "19to20": 19 < v < 20, "tiny": 0 < abs(v) < 1e-3,
              "lt-100": v < -100, "same": v == 0.0}[k]
        assert ok, (k, v)


def test_forward_cases_cover_every_branch():
    """Host-side: every width's cases hit all five branches (each case of
    five or more triples on its own), and the id requirements hold."""
    for D in DIMS:
        seen = set()
        for batch in _forward_batches(D):
            out, emb, users, pos, neg, where = _forward_case(D, batch)
            ref = reference(out, emb, users, pos, neg, N_USERS, 1e-4, 1.0, 3)
            _check_branches(ref["x"], where)
            seen |= set(where)
            if batch >= 5:
                assert set(where) == set(KINDS)
                t = where["same"]
                assert pos[t] == neg[t]
            if batch >= 16:
                assert 0 in users and N_USERS - 1 in users
                assert M_ITEMS - 1 in pos or M_ITEMS - 1 in neg
                assert np.intersect1d(users, np.concatenate([pos, neg])).size > 0
        assert seen == set(KINDS), D


def _call_forward(lib, st, out_t, emb_t, n_nodes, n_users, D, batch, ids, gs, alloc):
    r = dict(coef=_canary_f32(alloc + PAD), softplus=_canary_f32(alloc + PAD),
             reg=_canary_f32(alloc + PAD), keys=_canary_i32(3 * alloc + PAD),
             vals=_canary_i32(3 * alloc + PAD))
    rc = lib.mirec_bpr_forward(out_t.data_ptr(), emb_t.data_ptr(), n_nodes, n_users, D, batch,
                               ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(),
                               float(gs), r["coef"].data_ptr(), r["softplus"].data_ptr(),
                               r["reg"].data_ptr(), r["keys"].data_ptr(), r["vals"].data_ptr(),
                               st)
    return rc, r


def _forward_cases():
    return [pytest.param(D, b, id=f"D{D}-B{b}") for D in DIMS for b in _forward_batches(D)]


@pytest.mark.parametrize("grad_scale", [1.0, 0.5, 0.125])
@pytest.mark.parametrize("D,batch", _forward_cases())
def test_bpr_forward_and_loss(D, batch, grad_scale):
    lib, st = _api()
    out, emb, users, pos, neg, where = _forward_case(D, batch)
    n_nodes, decay = N_USERS + M_ITEMS, 1e-4
    ref = reference(out, emb, users, pos, neg, N_USERS, decay, grad_scale, 3)
    f32 = forward_f32(out, emb, users, pos, neg, N_USERS, decay, grad_scale)
    _check_branches(ref["x"], where)
    out_t, emb_t = _dev(out, F32), _dev(emb, F32)
    ids = [_dev(a, np.int32) for a in (users, pos, neg)]

    def run():
        rc, r = _call_forward(lib, st, out_t, emb_t, n_nodes, N_USERS, D, batch, ids,
                              grad_scale, batch)
        assert rc == 0
        loss, acc = _canary_f32(1 + PAD), _canary_f32(1 + PAD)
        acc[0] = 2.5
        assert lib.mirec_bpr_loss(r["softplus"].data_ptr(), r["reg"].data_ptr(), batch, decay,
                                  loss.data_ptr(), acc.data_ptr(), st) == 0
        loss2 = _canary_f32(1 + PAD)
        assert lib.mirec_bpr_loss(r["softplus"].data_ptr(), r["reg"].data_ptr(), batch, decay,
                                  loss2.data_ptr(), None, st) == 0
        r.update(loss=loss, acc=acc, loss2=loss2)
        return {k: _np(v) for k, v in r.items()}

    r = run()
    _same_bits(r, run())
    B = batch
    # integers, exactly
    assert np.array_equal(r["keys"][:3 * B], np.concatenate([users, N_USERS + pos,
                                                             N_USERS + neg]))
    assert np.array_equal(r["vals"][:3 * B], np.arange(3 * B))
    # canaries
    for k in ("coef", "softplus", "reg"):
        assert _is_canary(r[k][B:]), k
    for k in ("keys", "vals"):
        assert _is_canary(r[k][3 * B:]), k
    for k in ("loss", "acc", "loss2"):
        assert _is_canary(r[k][1:]), k
    # per-triple scalars against float64
    tag = f"fwd D={D} B={B} gs={grad_scale}"
    rel_ok = np.ones(B, bool)
    if "lt-100" in where:  # expf underflows: absolute bound for this triple alone
        t = where["lt-100"]
        rel_ok[t] = False
        for k in ("softplus", "coef"):
            assert abs(float(r[k][t]) - ref[k][t]) <= U24 / B, (k, r[k][t])
    floors = {"softplus": ref["terms"] * U24, "coef": ref["terms"] * U24 * grad_scale / B,
              "reg": ref["reg"] * U24}
    fails = []
    for k in ("softplus", "coef", "reg"):
        m = rel_ok if k != "reg" else np.ones(B, bool)
        if not m.any():
            continue
        err = float(_scalar_err(r[k][:B], ref[k], floors[k])[m].max())
        e32 = float(_scalar_err(f32[k], ref[k], floors[k])[m].max())
        _report(tag, k, err, e32)
        if not err <= _bound(k, e32):
            fails.append((k, err, e32))
    if "same" in where:  # x == 0 exactly: log(2) and half of grad_scale / B to the ulp
        t = where["same"]
        assert abs(r["softplus"][t] - F32(np.log(2.0))) <= np.spacing(F32(np.log(2.0)))
        c = F32(0.5 * grad_scale / B)
        assert abs(r["coef"][t] - c) <= np.spacing(c)
    # loss
    lerr = abs(float(r["loss"][0]) - ref["loss"]) / abs(ref["loss"])
    le32 = abs(float(f32["loss"]) - ref["loss"]) / abs(ref["loss"])
    _report(tag, "loss", lerr, le32)
    if not lerr <= _bound("loss", le32):
        fails.append(("loss", lerr, le32))
    assert not fails, fails
    assert _bits(r["loss2"][:1])[0] == _bits(r["loss"][:1])[0]
    assert _bits(r["acc"][:1])[0] == _bits(np.array([F32(2.5) + r["loss"][0]], F32))[0]


@pytest.mark.parametrize("what", ["batch0", "dim12", "no_items"])
def test_bpr_forward_refuses_and_writes_nothing(what):
    lib, st = _api()
    out, emb, users, pos, neg, _ = _forward_case(64, 16)
    n_nodes, D, batch = N_USERS + M_ITEMS, 64, 16
    if what == "batch0":
        batch = 0
    elif what == "dim12":
        D = 12
    else:
        n_nodes = N_USERS
    out_t, emb_t = _dev(out, F32), _dev(emb, F32)
    ids = [_dev(a, np.int32) for a in (users, pos, neg)]
    for _ in range(2):
        rc, r = _call_forward(lib, st, out_t, emb_t, n_nodes, N_USERS, D, batch, ids, 1.0, 16)
        torch.cuda.synchronize()
        assert rc != 0
        for k, v in r.items():
            assert _is_canary(_np(v)), k


# ==================================================================== 2. seeds
def _run_lengths(D):
    L = D // 4
    return sorted({1, 2, 7, 8, 9, L - 1, L, L + 1, 2 * L, 2 * L + 1, 3 * L + 5} - {0})


@functools.lru_cache(maxsize=None)
def _seed_case(D, big):
    """Triples whose sorted key array has a run of every length of
    _run_lengths(D) (test_seed_layout asserts it, and the rest of the
    required layout).  Users, ascending id: 4G-1 singletons (so the next
    run's head is the last position of a block), one user per short run
    length, then random filler.  Items: one item per run length, about half
    of its occurrences positives and half negatives, random filler, and the
    last item as positive and negative of one triple."""
    rng = np.random.default_rng(77 * D + big)
    LPR = D // 4
    block = 4 * (64 // LPR)
    R = _run_lengths(D)
    R_user = [r for r in R[:-3] if r > 1][::-1] + [1]  # a long run right after the pad
    n_pad = block - 1
    u_fixed = n_pad + sum(R_user)
    i_fixed = sum(R) + 2
    B = 2731 if big else max(u_fixed + 8, (i_fixed + 8 + 1) // 2) + 5
    assert B >= u_fixed + 8 and 2 * B >= i_fixed + 8
    # users
    uocc = list(range(n_pad))
    uid = n_pad
    for r in R_user:
        uocc += [uid] * r
        uid += 1
    nfill = B - 1 - len(uocc)  # one user slot belongs to the pos == neg triple
    pool = max(4, nfill // 3)
    uocc += list(uid + rng.integers(0, pool, nfill))
    n_users = uid + pool
    same_user = n_users - 1
    # items
    pocc, nocc = [], []
    for iid, r in enumerate(R):
        pocc += [iid] * ((r + 1) // 2)
        nocc += [iid] * (r // 2)
    iid = len(R)
    fp, fn = B - 1 - len(pocc), B - 1 - len(nocc)
    pool = max(4, (fp + fn) // 3)
    pocc += list(iid + rng.integers(0, pool, fp))
    nocc += list(iid + rng.integers(0, pool, fn))
    m_items = iid + pool + 1  # the last item is not in the filler pool
    users = rng.permutation(np.asarray(uocc, np.int64))
    pos = rng.permutation(np.asarray(pocc, np.int64))
    neg = rng.permutation(np.asarray(nocc, np.int64))
    at = int(rng.integers(0, B))
    users = np.insert(users, at, same_user)
    pos = np.insert(pos, at, m_items - 1)
    neg = np.insert(neg, at, m_items - 1)
    n_nodes = n_users + m_items
    out = (rng.standard_normal((n_nodes, D)) * 0.4).astype(F32)
    emb = (rng.standard_normal((n_nodes, D)) * 0.3).astype(F32)
    out.setflags(write=False)
    emb.setflags(write=False)
    return out, emb, users, pos, neg, n_users, m_items, at


def _sorted_layout(users, pos, neg, n_users):
    B = len(users)
    keys = np.concatenate([users, n_users + pos, n_users + neg]).astype(np.int64)
    order = np.argsort(keys, kind="stable")
    ks = keys[order]
    heads = np.nonzero(np.r_[True, ks[1:] != ks[:-1]])[0]
    lens = np.diff(np.r_[heads, 3 * B])
    return keys, order, ks, heads, lens


def _seed_cases():
    return [pytest.param(D, big, id=f"D{D}-{'B2731' if big else 'small'}")
            for D in DIMS for big in ((0, 1) if D in (64, 256) else (0,))]


@pytest.mark.parametrize("D,big", _seed_cases())
def test_seed_layout(D, big):
    """Host-side: the batch of _seed_case has the layout the seed test
    relies on, so that it cannot rot."""
    out, emb, users, pos, neg, n_users, m_items, at = _seed_case(D, big)
    B = len(users)
    keys, order, ks, heads, lens = _sorted_layout(users, pos, neg, n_users)
    assert 3 * B == (8193 if big else 3 * B) and (big or 3 * B <= 8192)
    assert set(_run_lengths(D)) <= set(lens.tolist())
    # an item that is the positive of some triples and the negative of
    # others, and a user with a run of its own
    both = np.intersect1d(pos, neg)
    assert any(np.sum(pos == i) + np.sum(neg == i) > 2 and
               not np.any((pos == i) & (neg == i)) for i in both)
    assert np.max(np.bincount(users)) > 1
    assert pos[at] == neg[at] and np.sum(pos == neg) >= 1
    # the highest node closes the array with a run of two or more
    assert ks[-1] == n_users + m_items - 1 and lens[-1] >= 2
    assert heads[-1] + lens[-1] == 3 * B
    # a run of more than one entry whose head is the last position of a block
    block = 4 * (64 // (D // 4))
    assert np.any((heads % block == block - 1) & (lens > 1))


def _call_seed(lib, st, out_t, emb_t, n_nodes, n_users, D, B, ids, fwd, decay, gs, L,
               ws_short=0):
    nb = ctypes.c_size_t(0)
    assert lib.mirec_bpr_seed_workspace(B, n_nodes, ctypes.byref(nb)) == 0
    ws = torch.zeros(nb.value + 256, dtype=torch.uint8, device="cuda")
    r = dict(slot=torch.full((n_nodes,), -1, dtype=torch.int32, device="cuda"),
             seed_p=_canary_f32(3 * B + PAD, D), seed_e=_canary_f32(3 * B + PAD, D),
             keys_sorted=_canary_i32(3 * B + PAD))
    rc = lib.mirec_bpr_seed(out_t.data_ptr(), emb_t.data_ptr(), n_nodes, n_users, D, B,
                            ids[0].data_ptr(), ids[1].data_ptr(), ids[2].data_ptr(),
                            fwd["coef"].data_ptr(), fwd["keys"].data_ptr(),
                            fwd["vals"].data_ptr(), float(decay), float(gs), L,
                            r["slot"].data_ptr(), r["seed_p"].data_ptr(),
                            r["seed_e"].data_ptr(), r["keys_sorted"].data_ptr(), ws.data_ptr(),
                            nb.value - ws_short, st)
    return rc, r


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("n_layers", [0, 3])
@pytest.mark.parametrize("D,big", _seed_cases())
def test_bpr_seed(D, big, n_layers, grad_scale):
    lib, st = _api()
    out, emb, users, pos, neg, n_users, m_items, _ = _seed_case(D, big)
    B, n_nodes, decay = len(users), n_users + m_items, 1e-4
    keys, order, ks, heads, lens = _sorted_layout(users, pos, neg, n_users)
    ref = reference(out, emb, users, pos, neg, n_users, decay, grad_scale, n_layers)
    out_t, emb_t = _dev(out, F32), _dev(emb, F32)
    ids = [_dev(a, np.int32) for a in (users, pos, neg)]

    def run():
        rc, fwd = _call_forward(lib, st, out_t, emb_t, n_nodes, n_users, D, B, ids, grad_scale,
                                B)
        assert rc == 0
        rc, r = _call_seed(lib, st, out_t, emb_t, n_nodes, n_users, D, B, ids, fwd, decay,
                           grad_scale, n_layers)
        assert rc == 0
        res = {k: _np(v) for k, v in r.items()}
        res["coef"] = _np(fwd["coef"])
        # reset, twice (the second finds every slot already -1)
        for i in (1, 2):
            assert lib.mirec_bpr_seed_reset(r["slot"].data_ptr(), r["keys_sorted"].data_ptr(),
                                            3 * B, st) == 0
            res[f"slot_reset{i}"] = _np(r["slot"])
        return res

    r = run()
    _same_bits(r, run())
    # integers, exactly
    assert np.array_equal(r["keys_sorted"][:3 * B], ks)
    assert _is_canary(r["keys_sorted"][3 * B:])
    slot = np.full(n_nodes, -1, np.int64)
    slot[ks[heads]] = heads
    assert np.array_equal(r["slot"], slot)
    assert np.all(r["slot_reset1"] == -1) and np.all(r["slot_reset2"] == -1)
    # non-head rows and the rows past 3B are untouched
    nonhead = np.ones(3 * B + PAD, bool)
    nonhead[heads] = False
    assert _is_canary(r["seed_p"][nonhead]) and _is_canary(r["seed_e"][nonhead])
    # heads against float64
    f32 = forward_f32(out, emb, users, pos, neg, n_users, decay, grad_scale)
    s32 = seeds_f32(out, emb, users, pos, neg, n_users, f32["coef"], keys, decay, grad_scale,
                    n_layers)
    nodes = ks[heads]
    gp32 = np.stack([s32[q][0] for q in heads])
    ge32 = np.stack([s32[q][1] for q in heads])
    tag = f"seed D={D} B={B} L={n_layers} gs={grad_scale}"
    fails = []
    Sp = ref["S"][nodes][:, None]
    Se = np.abs(ref["ge"][nodes]).max(1)[:, None]
    for name, got, g32, rf, S in (("seed_p", r["seed_p"][heads], gp32, ref["gp"][nodes], Sp),
                                  ("seed_e", r["seed_e"][heads], ge32, ref["ge"][nodes], Se)):
        assert np.all(S > 0)
        errq = (np.abs(got.astype(np.float64) - rf) / S).max(1)
        e32q = (np.abs(g32.astype(np.float64) - rf) / S).max(1)
        assert not np.isnan(errq).any()
        err, e32 = float(errq.max()), float(e32q.max())
        _report(tag, name, err, e32)
        if not err <= _bound(name, e32):
            w = int(errq.argmax())
            fails.append((name, err, e32, f"head {heads[w]} node {nodes[w]} run {lens[w]}"))
    assert not fails, fails
    # seed_e is one multiply: fp32(decay * cnt / B * grad_scale) * emb[node], to 2 ulp
    re = (decay * lens / B * grad_scale).astype(F32)[:, None]
    exp = re * emb[nodes]
    ulps = np.abs(r["seed_e"][heads].astype(np.float64) - exp) / np.spacing(np.abs(exp))
    print(f"[bpr_seed] {tag} seed_e one-multiply: max {ulps.max():.2f} ulp")
    w = np.unravel_index(int(ulps.argmax()), ulps.shape)
    assert ulps.max() <= 2, (ulps.max(), f"run {lens[w[0]]}")


@pytest.mark.parametrize("D", [4, 64, 256])
def test_bpr_seed_short_workspace_is_refused(D):
    from furusato_recommend_amd._lib import ERR_WORKSPACE
    lib, st = _api()
    out, emb, users, pos, neg, n_users, m_items, _ = _seed_case(D, 0)
    B, n_nodes = len(users), n_users + m_items
    out_t, emb_t = _dev(out, F32), _dev(emb, F32)
    ids = [_dev(a, np.int32) for a in (users, pos, neg)]
    rc, fwd = _call_forward(lib, st, out_t, emb_t, n_nodes, n_users, D, B, ids, 1.0, B)
    assert rc == 0
    for _ in range(2):
        rc, r = _call_seed(lib, st, out_t, emb_t, n_nodes, n_users, D, B, ids, fwd, 1e-4, 1.0,
                           3, ws_short=1)
        torch.cuda.synchronize()
        assert rc == ERR_WORKSPACE
        assert np.all(_np(r["slot"]) == -1)
        for k in ("seed_p", "seed_e", "keys_sorted"):
            assert _is_canary(_np(r[k])), k


# ============================================================ 3. pack / merge
MERGE_NODES = 500
GUARD = 64  # canary words on either side of the slot map


def _merge_case(n, world, kind, D):
    """Per rank: a sorted key array with runs (shared and private nodes; the
    last node in two ranks, or in the only one) and random rows."""
    rng = np.random.default_rng(10007 * n + 31 * world + D + (kind == "single"))
    sizes = [n // world] * world
    sizes[-1] += n - sum(sizes)
    ranks = []
    for rk, m in enumerate(sizes):
        if kind == "single":
            keys = np.full(m, 123, np.int64)
        else:
            pool = np.r_[np.arange(0, 120), 200 + 60 * rk + np.arange(60)]
            keys = rng.choice(pool, m)
            if rk in (0, 1) and m > 0:
                keys[:min(m, 3 - rk)] = MERGE_NODES - 1
            keys = np.sort(keys)
        ranks.append((keys, rng.standard_normal((m, D)).astype(F32),
                      rng.standard_normal((m, D)).astype(F32)))
    return ranks


def _merge_cases():
    cases = []
    for D in (4, 64, 256):
        for n in (1, 600, 8192, 8193):
            for world in ((1,) if n == 1 else (1, 2, 3)):
                cases.append(pytest.param(D, n, world, "runs", id=f"D{D}-n{n}-w{world}"))
        cases.append(pytest.param(D, 600, 1, "single", id=f"D{D}-n600-single"))
    return cases


@pytest.mark.parametrize("D,n,world,kind", _merge_cases())
def test_seed_pack_and_merge(D, n, world, kind):
    lib, st = _api()
    ranks = _merge_case(n, world, kind, D)
    if kind == "runs" and n > 1:
        assert sum(MERGE_NODES - 1 in k for k, _, _ in ranks) >= min(world, 2)
        if world > 1:
            shared = np.intersect1d(ranks[0][0], ranks[1][0])
            assert shared.size > 1 and np.setdiff1d(ranks[0][0], ranks[1][0]).size > 0
    rows_p = np.concatenate([r[1] for r in ranks])
    rows_e = np.concatenate([r[2] for r in ranks])

    def run():
        packed = []
        for keys, _, _ in ranks:
            m = len(keys)
            pk, kt = _canary_i32(m + PAD), _dev(keys, np.int32)
            assert lib.mirec_seed_pack(kt.data_ptr(), m, MERGE_NODES, pk.data_ptr(), st) == 0
            packed.append(_np(pk))
        res = {f"packed{i}": p for i, p in enumerate(packed)}
        gathered = np.concatenate([p[:len(k)] for p, (k, _, _) in zip(packed, ranks)])
        nb = ctypes.c_size_t(0)
        assert lib.mirec_seed_merge_workspace(n, MERGE_NODES, ctypes.byref(nb)) == 0
        ws = torch.zeros(nb.value + 256, dtype=torch.uint8, device="cuda")
        buf = _canary_i32(MERGE_NODES + 2 * GUARD)
        slot = buf[GUARD:GUARD + MERGE_NODES]
        slot.fill_(-1)
        r = dict(seed_p=_canary_f32(n + PAD, D), seed_e=_canary_f32(n + PAD, D),
                 keys_sorted=_canary_i32(n + PAD))
        gt, pt, et = _dev(gathered, np.int32), _dev(rows_p, F32), _dev(rows_e, F32)
        assert lib.mirec_seed_merge(gt.data_ptr(), pt.data_ptr(), et.data_ptr(),
                                    n, D, MERGE_NODES, slot.data_ptr(), r["seed_p"].data_ptr(),
                                    r["seed_e"].data_ptr(), r["keys_sorted"].data_ptr(),
                                    ws.data_ptr(), nb.value, st) == 0
        res.update({k: _np(v) for k, v in r.items()})
        res["buf"] = _np(buf)
        assert lib.mirec_bpr_seed_reset(slot.data_ptr(), r["keys_sorted"].data_ptr(), n,
                                        st) == 0
        res["buf_reset"] = _np(buf)
        return res

    r = run()
    _same_bits(r, run())
    # pack: the key at heads, the sentinel elsewhere
    exp_packed = []
    for i, (keys, _, _) in enumerate(ranks):
        m = len(keys)
        head = np.r_[True, keys[1:] != keys[:-1]][:m]
        exp = np.where(head, keys, MERGE_NODES)
        assert np.array_equal(r[f"packed{i}"][:m], exp), i
        assert _is_canary(r[f"packed{i}"][m:]), i
        exp_packed.append(exp)
    if kind == "single":
        assert exp_packed[0][0] == 123 and np.all(exp_packed[0][1:] == MERGE_NODES)
    # merge: the stable order of the concatenation, sentinels (all last) as -1
    gathered = np.concatenate(exp_packed)
    order = np.argsort(gathered, kind="stable")
    ks = gathered[order]
    n_real = int(np.sum(ks != MERGE_NODES))
    assert np.all(ks[n_real:] == MERGE_NODES)
    ks = np.where(ks == MERGE_NODES, -1, ks)
    assert np.array_equal(r["keys_sorted"][:n], ks)
    assert _is_canary(r["keys_sorted"][n:])
    heads = np.nonzero(np.r_[True, ks[1:] != ks[:-1]][:n] & (ks >= 0))[0]
    slot = np.full(MERGE_NODES, -1, np.int64)
    slot[ks[heads]] = heads
    assert np.array_equal(r["buf"][GUARD:GUARD + MERGE_NODES], slot)
    # rows: float32 sums in gathered order, from zero, bitwise
    exp_p, exp_e = np.zeros((len(heads), D), F32), np.zeros((len(heads), D), F32)
    for j, q in enumerate(heads):
        q2 = q
        while q2 < n and ks[q2] == ks[q]:
            exp_p[j] = exp_p[j] + rows_p[order[q2]]
            exp_e[j] = exp_e[j] + rows_e[order[q2]]
            q2 += 1
    assert np.array_equal(_bits(r["seed_p"][heads]), _bits(exp_p))
    assert np.array_equal(_bits(r["seed_e"][heads]), _bits(exp_e))
    nonhead = np.ones(n + PAD, bool)
    nonhead[heads] = False
    assert _is_canary(r["seed_p"][nonhead]) and _is_canary(r["seed_e"][nonhead])
    # the reset skips the -1 keys: nothing is written in front of the map
    for k in ("buf", "buf_reset"):
        assert _is_canary(r[k][:GUARD]) and _is_canary(r[k][GUARD + MERGE_NODES:]), k
    assert np.all(r["buf_reset"][GUARD:GUARD + MERGE_NODES] == -1)


# ================================================================== 4. dense
@pytest.mark.parametrize("D", [4, 32, 256])
def test_seed_dense(D):
    lib, st = _api()
    rng = np.random.default_rng(D)
    n_nodes, cap, count = 300, 128, 70
    lst = rng.permutation(n_nodes)[:cap]  # distinct; the entries past count stay untouched
    slot = np.full(n_nodes, -1, np.int64)
    slot[lst[:50]] = rng.permutation(64)[:50]
    dinv = rng.uniform(0.05, 1.0, n_nodes).astype(F32)
    seed = rng.standard_normal((64, D)).astype(F32)
    lst_t, cnt_t = _dev(lst, np.int32), _dev([count], np.int32)
    slot_t, dinv_t, seed_t = _dev(slot, np.int32), _dev(dinv, F32), _dev(seed, F32)

    def run():
        res = {}
        dense = _canary_f32(n_nodes + PAD, D)
        assert lib.mirec_seed_dense(lst_t.data_ptr(), cnt_t.data_ptr(), 0, slot_t.data_ptr(),
                                    dinv_t.data_ptr(), seed_t.data_ptr(), D, dense.data_ptr(),
                                    0, st) == 0
        res["noop"] = _np(dense)
        assert lib.mirec_seed_dense(lst_t.data_ptr(), cnt_t.data_ptr(), cap, slot_t.data_ptr(),
                                    dinv_t.data_ptr(), seed_t.data_ptr(), D, dense.data_ptr(),
                                    0, st) == 0
        res["write"] = _np(dense)
        assert lib.mirec_seed_dense(lst_t.data_ptr(), cnt_t.data_ptr(), cap, None, None, None,
                                    D, dense.data_ptr(), 1, st) == 0
        res["clear"] = _np(dense)
        return res

    r = run()
    _same_bits(r, run())
    assert _is_canary(r["noop"])
    listed = lst[:count]
    unlisted = np.ones(n_nodes + PAD, bool)
    unlisted[listed] = False
    exp = np.zeros((count, D), F32)
    exp[:50] = dinv[listed[:50], None] * seed[slot[listed[:50]]]
    assert exp.dtype == F32
    assert np.array_equal(_bits(r["write"][listed]), _bits(exp))
    assert np.all(_bits(r["write"][listed[50:]]) == 0)
    assert _is_canary(r["write"][unlisted])
    assert np.all(_bits(r["clear"][listed]) == 0)
    assert _is_canary(r["clear"][unlisted])
