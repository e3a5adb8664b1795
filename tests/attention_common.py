"""Shared by tests/test_attention_host.py and tests/test_attention_kernels.py:
the float64 restatement of the causal attention core (csrc/attention.hip,
csrc/attn_wave.hip), its float32 twin for the kernel tolerance protocol, the
per-row error measure, the input regimes, the shapes the GPU file runs, and a
Python restatement of the order / packs rules of
mirec_attention_length_order.  Nothing here is collected by pytest and
nothing here touches a GPU.

One (sequence, head) with q, k, v, dout of shape [T, dh], causal:
    s = q k^T / sqrt(dh),  P = softmax(s),  out = P v
    lse2 = log2 sum_k 2^(s log2 e)
    dP = dout v^T,  delta = rowsum(P * dP) (= rowsum(dout * out))
    dS = P * (dP - delta) / sqrt(dh)
    dq = dS k,  dk = dS^T q,  dv = P^T dout

The measure.  Row r of a quantity is measured as max_col |got - ref| / N_r,
N_r being the float64 formula with every product term made absolute
(cancellation inside a row does not inflate the bound, a large row does not
hide a small one): out N = P |v|; with aP = |dout| |v|^T and
A = P * (aP + rowsum(P * aP)) / sqrt(dh): dq N = A |k|, dk N = A^T |q|;
dv N = P^T |dout|; delta N = rowsum(P * aP); each the max over columns and
floored at 2^-24 times the largest N_r of that (sequence, head, quantity): an
absolute error below one float32 ulp of the unit's largest row is the
documented flush of probabilities under 2^-126 (csrc/common.h), not a
defect.  lse2 is measured as |got - ref| / max(1, |ref|).  A case's err is
the max over its rows; e32 is the float32 twin's err.
"""
import functools

import numpy as np

F32 = np.float32
U24 = 2.0 ** -24
LOG2E = 1.4426950408889634
MAX_T = 64   # longer sequences are cut to their first 64 rows
BLK = 16     # block edge

REGIMES = ("unit", "sharp", "offset")

# ------------------------------------------------- the shapes of the GPU file
UNIFORM_T = (1, 15, 16, 17, 33, 50, 64)
UNIFORM_BATCH = (1, 5)
UNIFORM_HEADS = (1, 3)
UNIFORM_DH_BLOCK = (3, 20, 64)   # scalar / float4 loads, DPAD 32 / 64
UNIFORM_DH_WAVE = (16, 64)
PACKED_LENGTHS = (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 0, 0, 5)
PACKED_HEADS = 3                 # h * dh odd for odd dh: unaligned scalar loads
DH_BLOCK = (1, 3, 4, 8, 12, 20, 31, 32, 33, 48, 63, 64)
DH_PACKED_BWD = (4, 8, 12, 20, 32, 36, 60, 64)
DH_WAVE = (16, 32, 64)
CUT_LENGTHS = (5, 70, 20, 64, 1, 70)
CUT_DH = {"varlen": (20, 64), "ordered": (20, 64), "wave": (16, 64),
          "packed_bwd": (20, 64), "packed_bwd_lse": (20, 64)}
# NaN / clean sequences alternate; by the pack rules every pack class (3 + 1,
# 2 + 2, 1 x 4) has a pack holding both parities (test_attention_host.py)
ISOLATION_LENGTHS = (40, 16, 33, 15, 20, 30, 7, 9, 3, 12, 64, 0, 2, 5)
ISOLATION_DH = {"varlen": (3, 20, 64), "wave": (16, 64), "packed_bwd": (20, 64),
                "packed_bwd_lse": (20, 64)}
# mirec_attention_length_order: every branch of the pack rules
ORDER_LENGTH_LISTS = {
    "more1than3": (40, 5, 33, 1, 16, 48, 9, 3, 64, 20, 2),      # n31 = count3
    "fewer1than3": (40, 5, 33, 48, 47, 64, 20, 35),             # n31 = count1
    "odd2": (17, 32, 20, 5, 64),
    "ones_not_x4": (1, 2, 3, 4, 5, 16, 15),
    "only_empty": (0, 0, 0),
    "single": (23,),
    "single_empty": (0,),
    "len70": (70, 3, 70, 40, 0, 16),
    "edges": PACKED_LENGTHS,
    "isolation": ISOLATION_LENGTHS,
    "cut": CUT_LENGTHS,
}


def big_length_list():
    """B = 1030 (more sequences than the ordering pass has threads): every
    length 0..70 many times over."""
    return tuple(int(x) for x in np.random.default_rng(1030).integers(0, 71, 1030))


def all_order_length_lists():
    d = dict(ORDER_LENGTH_LISTS)
    d["b1030"] = big_length_list()
    return d


# ---------------------------------------------------------------- references
def _causal(T):
    return np.tril(np.ones((T, T), dtype=bool))


def reference(q, k, v, dout):
    """float64: out, lse2, delta, dq, dk, dv of one (sequence, head), and the
    per-row normalisers N[quantity] of the measure."""
    q, k, v, dout = (np.asarray(x, np.float64) for x in (q, k, v, dout))
    T, dh = q.shape
    sc = 1.0 / np.sqrt(dh)
    mask = _causal(T)
    s = np.where(mask, q @ k.T * sc, -np.inf)
    m = s.max(1, keepdims=True)
    e = np.exp(s - m)
    l = e.sum(1, keepdims=True)
    P = e / l
    lse2 = (m[:, 0] + np.log(l[:, 0])) * LOG2E
    out = P @ v
    dP = dout @ v.T
    delta = (P * dP).sum(1)
    dS = P * (dP - delta[:, None]) * sc
    aP = np.abs(dout) @ np.abs(v).T
    n_delta = (P * aP).sum(1)
    A = P * (aP + n_delta[:, None]) * sc
    N = dict(out=(P @ np.abs(v)).max(1), dq=(A @ np.abs(k)).max(1),
             dk=(A.T @ np.abs(q)).max(1), dv=(P.T @ np.abs(dout)).max(1), delta=n_delta)
    N = {name: np.maximum(x, U24 * x.max()) for name, x in N.items()}
    return dict(out=out, lse2=lse2, delta=delta, dq=dS @ k, dk=dS.T @ q, dv=P.T @ dout, N=N)


def twin32(q, k, v, dout, from_lse):
    """The same quantities in numpy float32 by the algorithm the kernels
    document: per-pair dots, scores times float32(scale * log2 e), a
    max-subtracted exp2, and with ``from_lse`` (phase B of the workgroup
    backwards, the wave backward, packed_bwd_lse) P = exp2(fma(s, c2, -lse2))
    from the float32 lse2."""
    q, k, v, dout = (np.asarray(x, F32) for x in (q, k, v, dout))
    T, dh = q.shape
    scale = F32(1) / np.sqrt(F32(dh))
    c2 = F32(scale * F32(LOG2E))
    mask = _causal(T)
    with np.errstate(under="ignore", over="ignore", invalid="ignore"):
        s = (q[:, None, :] * k[None, :, :]).sum(2, dtype=F32)
        x = np.where(mask, s * c2, F32(-np.inf)).astype(F32)
        m = x.max(1, keepdims=True)
        e = np.exp2(x - m)
        l = e.sum(1, dtype=F32, keepdims=True)
        P = e * (F32(1) / l)
        lse2 = (m + np.log2(l))[:, 0]
        if from_lse:  # one fma (the product is not rounded), one exp2
            x64 = s.astype(np.float64) * np.float64(c2) - lse2[:, None].astype(np.float64)
            P = np.exp2(np.where(mask, x64, -np.inf).astype(F32))
        out = (P[:, :, None] * v[None, :, :]).sum(1, dtype=F32)
        dP = (dout[:, None, :] * v[None, :, :]).sum(2, dtype=F32)
        delta = (P * dP).sum(1, dtype=F32)
        dS = P * (dP - delta[:, None]) * scale
        dq = (dS[:, :, None] * k[None, :, :]).sum(1, dtype=F32)
        dk = (dS[:, :, None] * q[:, None, :]).sum(0, dtype=F32)
        dv = (P[:, :, None] * dout[:, None, :]).sum(0, dtype=F32)
    res = dict(out=out, lse2=lse2, delta=delta, dq=dq, dk=dk, dv=dv)
    assert all(a.dtype == F32 for a in res.values())
    return res


# -------------------------------------------------------------------- inputs
def unit_inputs(regime, T, dh, rng):
    """q, k, v, dout (float32 [T, dh]) of one (sequence, head)."""
    g = lambda: rng.standard_normal((T, dh))  # noqa: E731
    if regime == "unit":
        q, k = g(), g()
    elif regime == "sharp":   # scaled logits of std ~30: a near one-hot softmax
        q, k = np.sqrt(30.0) * g(), np.sqrt(30.0) * g()
    elif regime == "offset":  # every scaled logit ~ +300
        c = np.sqrt(300.0 * np.sqrt(dh))
        u = np.ones(dh) / np.sqrt(dh)
        q, k = c * u + 0.5 * g(), c * u + 0.5 * g()
    else:
        raise ValueError(regime)
    return tuple(np.asarray(a, F32) for a in (q, k, g(), g()))


class Batch:
    """A batch of sequences in the kernels' memory layout.  qkv [n, 3 d] and
    dout [n, d] hold every row of every sequence (all of a sequence longer
    than 64 rows, too); ``rows`` marks the rows a kernel reads and writes
    (the first 64 of each sequence).  ref / t32 / t32l: float64 reference,
    plain float32 twin, from-lse float32 twin, as [n, d] (out, dq, dk, dv)
    and [n, H] (lse2, delta) arrays; N[quantity]: [n, H] normalisers."""

    def __init__(self, regime, lengths, heads, dh, seed=0):
        self.regime, self.lengths, self.heads, self.dh = regime, tuple(lengths), heads, dh
        self.d = d = heads * dh
        self.offsets = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int32)
        self.n = n = int(self.offsets[-1])
        rng = np.random.default_rng([seed, REGIMES.index(regime), heads, dh, len(lengths)])
        self.qkv = np.zeros((n, 3 * d), F32)
        self.dout = np.zeros((n, d), F32)
        self.rows = np.zeros(n, bool)
        self.seq_of_row = np.zeros(n, np.int64)
        z = lambda w, t=np.float64: np.zeros((n, w), t)  # noqa: E731
        self.ref = dict(out=z(d), dq=z(d), dk=z(d), dv=z(d), lse2=z(heads), delta=z(heads))
        self.t32 = {k_: a.astype(F32) for k_, a in self.ref.items()}
        self.t32l = {k_: a.astype(F32) for k_, a in self.ref.items()}
        self.N = {k_: z(heads) for k_ in ("out", "dq", "dk", "dv", "delta")}
        for b, L in enumerate(lengths):
            r0 = int(self.offsets[b])
            self.seq_of_row[r0:r0 + L] = b
            T = min(L, MAX_T)
            self.rows[r0:r0 + T] = True
            for h in range(heads):
                if L == 0:
                    continue
                q, k, v, do = unit_inputs(regime, L, dh, rng)
                cs = slice(h * dh, (h + 1) * dh)
                self.qkv[r0:r0 + L, cs] = q
                self.qkv[r0:r0 + L, d + h * dh:d + (h + 1) * dh] = k
                self.qkv[r0:r0 + L, 2 * d + h * dh:2 * d + (h + 1) * dh] = v
                self.dout[r0:r0 + L, cs] = do
                q, k, v, do = q[:T], k[:T], v[:T], do[:T]
                r64 = reference(q, k, v, do)
                rs = slice(r0, r0 + T)
                for dst, src in ((self.ref, r64), (self.t32, twin32(q, k, v, do, False)),
                                 (self.t32l, twin32(q, k, v, do, True))):
                    for name in ("out", "dq", "dk", "dv"):
                        dst[name][rs, cs] = src[name]
                    dst["lse2"][rs, h] = src["lse2"]
                    dst["delta"][rs, h] = src["delta"]
                for name in self.N:
                    self.N[name][rs, h] = r64["N"][name]

    def err(self, name, got):
        """The case's err of quantity ``name`` over the rows a kernel writes
        (every one of them: nothing is skipped)."""
        got = np.asarray(got, np.float64)[: self.n][self.rows]
        ref = self.ref[name][self.rows]
        if got.shape[0] == 0:
            return 0.0
        if name == "lse2":
            e = np.abs(got - ref) / np.maximum(1.0, np.abs(ref))
        elif name == "delta":
            e = np.abs(got - ref) / self.N[name][self.rows]
        else:
            a = np.abs(got - ref).reshape(-1, self.heads, self.dh).max(2)
            e = a / self.N[name][self.rows]
        return float(e.max())

    def e32(self, name, from_lse):
        return self.err(name, (self.t32l if from_lse else self.t32)[name])

    def twin_finite(self):
        return all(np.isfinite(a).all() for t in (self.t32, self.t32l) for a in t.values())

    def norms_positive(self):
        return all(bool((a[self.rows] > 0).all()) for a in self.N.values())


@functools.lru_cache(maxsize=None)
def batch(regime, lengths, heads, dh, seed=0):
    """The cached Batch (computed once, shared, never modified)."""
    return Batch(regime, lengths, heads, dh, seed)


def uniform_cases(dhs):
    """(lengths, heads, dh) of the uniform form's cases."""
    return [((T,) * B, H, dh) for dh in dhs for T in UNIFORM_T for B in UNIFORM_BATCH
            for H in UNIFORM_HEADS]


def bucket_order(lengths):
    """The bucketed form's input: (stable order by bucket ceil(len / 16) in
    1..4, the four bucket_end counts of that order)."""
    nb = np.clip((np.asarray(lengths, np.int64) + BLK - 1) // BLK, 1, 4)
    order = np.argsort(nb, kind="stable")
    return order, tuple(int(x) for x in np.cumsum(np.bincount(nb - 1, minlength=4)))


def every_gpu_batch():
    """(regime, lengths, heads, dh) of every batch the GPU file builds."""
    keys = []
    for regime in REGIMES:
        for lengths, H, dh in uniform_cases(UNIFORM_DH_BLOCK) + uniform_cases(UNIFORM_DH_WAVE):
            keys.append((regime, lengths, H, dh))
        for dh in sorted(set(DH_BLOCK) | set(DH_PACKED_BWD) | set(DH_WAVE)):
            keys.append((regime, PACKED_LENGTHS, PACKED_HEADS, dh))
        order, _ = bucket_order(PACKED_LENGTHS)
        for dh in DH_BLOCK:
            keys.append((regime, tuple(PACKED_LENGTHS[i] for i in order), PACKED_HEADS, dh))
        for dhs in CUT_DH.values():
            for dh in dhs:
                keys.append((regime, CUT_LENGTHS, 2, dh))
    for dhs in ISOLATION_DH.values():
        for dh in dhs:
            keys.append(("unit", ISOLATION_LENGTHS, PACKED_HEADS, dh))
    return sorted(set(keys))


# ------------------------------------------------------------------ the packs
def block_class(L):
    return (min(L, MAX_T) + BLK - 1) // BLK


def pack_rules(lengths, order=None):
    """The rules in the comment above length_order_kernel, restated.  order:
    the sequences by clamped length, longest first (given, or a stable sort;
    the order among equal lengths is free).  Over that order: each 4-block
    sequence is a pack of its own; each 3-block sequence is a pack and takes,
    while there are any, the next-longest 1-block sequence into slot 1; the
    2-block sequences go two to a pack; the remaining 1-block sequences four
    to a pack; empty sequences are in no pack.  Returns (order, packs): packs
    a list of four (first row, clamped length) slots, (0, 0) when empty, in
    the order 4-block, 3-block, 2-block, 1-block packs."""
    L = np.minimum(np.asarray(lengths, np.int64), MAX_T)
    offs = np.concatenate([[0], np.cumsum(lengths)]).astype(np.int64)
    if order is None:
        order = np.argsort(-L, kind="stable")
    order = [int(b) for b in order]
    slot = lambda b: (int(offs[b]), int(L[b]))  # noqa: E731
    cls = {k: [b for b in order if block_class(int(L[b])) == k] for k in range(5)}
    n31 = min(len(cls[3]), len(cls[1]))
    packs = [[slot(b)] for b in cls[4]]
    for i, b in enumerate(cls[3]):
        packs.append([slot(b)] + ([slot(cls[1][i])] if i < n31 else []))
    for i in range(0, len(cls[2]), 2):
        packs.append([slot(b) for b in cls[2][i:i + 2]])
    rest = cls[1][n31:]
    for i in range(0, len(rest), 4):
        packs.append([slot(b) for b in rest[i:i + 4]])
    packs = [p + [(0, 0)] * (4 - len(p)) for p in packs]
    return order, packs


def packs_array(packs):
    """The int32 words the ordering pass writes: [count, 0, 0, 0, 8 per pack]."""
    flat = [len(packs), 0, 0, 0]
    for p in packs:
        for r0, L in p:
            flat += [r0, L]
    return np.asarray(flat, np.int32)
