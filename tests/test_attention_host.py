"""The CPU half of the attention kernel tests (tests/test_attention_kernels.py
is the GPU half): the float64 restatement in tests/attention_common.py against
torch float64 autograd, the conditions the GPU file's measure rests on (every
normaliser positive, the float32 twin finite, no row and no case skipped), and
the restatement of the pack rules of mirec_attention_length_order."""
import ast
import os

import numpy as np
import pytest
import torch

from tests import attention_common as ac

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.mark.parametrize("dh", [1, 20, 64])
@pytest.mark.parametrize("T", [1, 2, 17, 64])
@pytest.mark.parametrize("regime", ac.REGIMES)
def test_reference_matches_float64_autograd(regime, T, dh):
    """out, lse2, delta, dq, dk, dv == torch float64 autograd through an
    explicit masked softmax, to 1e-12 of each quantity's largest entry."""
    rng = np.random.default_rng([T, dh, ac.REGIMES.index(regime)])
    q, k, v, do = ac.unit_inputs(regime, T, dh, rng)
    r = ac.reference(q, k, v, do)
    tq, tk, tv = (torch.tensor(a, dtype=torch.float64, requires_grad=True) for a in (q, k, v))
    s = tq @ tk.T / np.sqrt(dh)
    s = s.masked_fill(~torch.tril(torch.ones(T, T, dtype=torch.bool)), float("-inf"))
    P = torch.softmax(s, dim=1)
    out = P @ tv
    tdo = torch.tensor(do, dtype=torch.float64)
    gq, gk, gv = torch.autograd.grad(out, (tq, tk, tv), tdo)
    lse2 = torch.logsumexp(s, dim=1) * ac.LOG2E
    delta = (tdo * out).sum(1)
    for name, t in (("out", out), ("dq", gq), ("dk", gk), ("dv", gv), ("lse2", lse2),
                    ("delta", delta)):
        t = t.detach().numpy()
        assert np.abs(r[name] - t).max() <= 1e-12 * max(np.abs(t).max(), 1.0), name


def test_twin_with_exact_arithmetic_is_the_reference():
    """The twin's algorithm (base-2 softmax from scale * log2 e, with and
    without the lse shortcut) evaluates the same function: close to float64 at
    unit scale (a wrong constant or mask in the twin would show here, not as a
    wide tolerance in the GPU file)."""
    rng = np.random.default_rng(3)
    q, k, v, do = ac.unit_inputs("unit", 33, 20, rng)
    r = ac.reference(q, k, v, do)
    for from_lse in (False, True):
        t = ac.twin32(q, k, v, do, from_lse)
        for name in ("out", "dq", "dk", "dv", "lse2", "delta"):
            assert np.abs(t[name] - r[name]).max() < 2e-5 * max(1.0, np.abs(r[name]).max()), name


def test_measure_conditions_hold_for_every_gpu_batch():
    """Condition, not measurement: over every regime and shape of the GPU
    file every row's normaliser is > 0 and both float32 twins are finite, so
    err is defined for every row and e32 is a finite number."""
    keys = ac.every_gpu_batch()
    assert len(keys) > 100
    for key in keys:
        b = ac.batch(*key)
        assert b.norms_positive(), key
        assert b.twin_finite(), key
        # the measure covers every row a kernel writes, and only those
        want = sum(min(L, ac.MAX_T) for L in b.lengths)
        assert int(b.rows.sum()) == want, key
        for name in ("out", "dq", "dk", "dv", "lse2", "delta"):
            for from_lse in (False, True):
                assert np.isfinite(b.e32(name, from_lse)), (key, name)


def test_e32_at_unit_scale_is_a_few_ulp():
    """At unit scale the twin is within 16 x 2^-24 of float64 in every
    quantity: the GPU file's bound FACTOR x e32 stays a float32-rounding
    bound, it cannot hide a percent-level error."""
    for dh in (1, 20, 64):
        b = ac.batch("unit", ac.PACKED_LENGTHS, ac.PACKED_HEADS, dh)
        for name in ("out", "dq", "dk", "dv", "lse2", "delta"):
            for from_lse in (False, True):
                assert b.e32(name, from_lse) <= 16 * ac.U24, (dh, name, from_lse)


def test_gpu_file_skips_nothing():
    """Condition: tests/test_attention_kernels.py has no skip / xfail /
    importorskip, takes its shapes from attention_common, and parametrises
    over every regime, form and head dim listed there."""
    path = os.path.join(HERE, "test_attention_kernels.py")
    src = open(path).read()
    tree = ast.parse(src)
    names = {n.attr for n in ast.walk(tree) if isinstance(n, ast.Attribute)} | \
        {n.id for n in ast.walk(tree) if isinstance(n, ast.Name)}
    assert not names & {"skip", "skipif", "xfail", "importorskip"}
    from tests import test_attention_kernels as tk
    assert tk.REGIMES == ac.REGIMES == ("unit", "sharp", "offset")
    assert tk.DH_OF_FORM["varlen"] == tk.DH_OF_FORM["bucketed"] == tk.DH_OF_FORM["ordered"] \
        == (1, 3, 4, 8, 12, 20, 31, 32, 33, 48, 63, 64)
    assert tk.DH_OF_FORM["packed_bwd"] == tk.DH_OF_FORM["packed_bwd_lse"] \
        == (4, 8, 12, 20, 32, 36, 60, 64)
    assert tk.DH_OF_FORM["wave"] == (16, 32, 64)
    assert ac.PACKED_LENGTHS == (0, 1, 2, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 0, 0, 5)
    assert ac.UNIFORM_T == (1, 15, 16, 17, 33, 50, 64)
    assert ac.UNIFORM_BATCH == (1, 5) and ac.UNIFORM_HEADS == (1, 3)
    assert all(v == 8 for v in tk.FACTOR.values())
    raised = {("sharp", k) for k, v in tk.FACTOR_SHARP.items() if v != 8}
    assert raised == set(tk.FACTOR_REASONS) and all(v >= 8 for v in tk.FACTOR_SHARP.values())


# ----------------------------------------------------------------- the packs
@pytest.mark.parametrize("name", sorted(ac.all_order_length_lists()))
def test_pack_rules(name):
    """Every non-empty sequence sits in exactly one slot, a pack holds at
    most 4 blocks, and the packs are composed as stated: 4; 3 (+ 1 while
    there are 1-block sequences, the longest first); 2 + 2; 1 x 4."""
    lengths = ac.all_order_length_lists()[name]
    offs = np.concatenate([[0], np.cumsum(lengths)])
    order, packs = ac.pack_rules(lengths)
    L = np.minimum(np.asarray(lengths), ac.MAX_T)
    assert sorted(order) == list(range(len(lengths)))
    assert all(L[order[i]] >= L[order[i + 1]] for i in range(len(order) - 1))
    want = sorted((int(offs[b]), int(L[b])) for b in range(len(lengths)) if L[b] > 0)
    got = sorted(s for p in packs for s in p if s != (0, 0))
    assert got == want                       # exactly one slot each (rows are distinct)
    cnt = {k: sum(1 for x in L if ac.block_class(int(x)) == k) for k in range(5)}
    n31 = min(cnt[3], cnt[1])
    comp = []
    for p in packs:
        assert len(p) == 4
        ks = [ac.block_class(Ls) for _, Ls in p if Ls > 0]
        assert ks and sum(ks) <= 4
        assert all(s == (0, 0) for s in p[len(ks):])   # filled slots first
        comp.append(tuple(ks))
    assert comp.count((4,)) == cnt[4]
    assert comp.count((3, 1)) == n31 and comp.count((3,)) == cnt[3] - n31
    assert comp.count((2, 2)) == cnt[2] // 2 and comp.count((2,)) == cnt[2] % 2
    ones = cnt[1] - n31
    assert comp.count((1, 1, 1, 1)) == ones // 4
    assert sum(1 for c in comp if set(c) == {1} and len(c) < 4) == (1 if ones % 4 else 0)
    assert len(packs) == cnt[4] + cnt[3] + (cnt[2] + 1) // 2 + (ones + 3) // 4
    # the order of the packs: longest first
    firsts = [p[0][1] for p in packs]
    assert firsts == sorted(firsts, reverse=True)
    # the 1-block riders of the 3-block packs are the longest 1-block ones
    riders = [p[1][1] for p in packs if ac.block_class(p[0][1]) == 3 and p[1] != (0, 0)]
    ones_sorted = sorted((int(x) for x in L if 0 < x <= 16), reverse=True)
    assert riders == ones_sorted[:n31]


def test_length_lists_reach_every_branch():
    """The lists of the GPU test: n31 = either count, an odd number of 2-block
    sequences, a 1-block remainder, only empties, B = 1, B > 1024, length 70."""
    def counts(name):
        L = ac.all_order_length_lists()[name]
        return {k: sum(1 for x in L if ac.block_class(x) == k) for k in range(5)}
    c = counts("more1than3")
    assert c[1] > c[3] > 0
    c = counts("fewer1than3")
    assert c[3] > c[1] > 0
    assert counts("odd2")[2] % 2 == 1
    c = counts("ones_not_x4")
    assert c[3] == 0 and c[1] % 4 != 0
    assert set(ac.ORDER_LENGTH_LISTS["only_empty"]) == {0}
    assert len(ac.ORDER_LENGTH_LISTS["single"]) == 1
    assert len(ac.big_length_list()) == 1030
    assert 70 in ac.ORDER_LENGTH_LISTS["len70"] and 70 in ac.CUT_LENGTHS


def test_isolation_lengths_mix_parities_in_every_pack_class():
    """Section 3.5's lengths put an odd- and an even-numbered sequence into
    one pack of each shared class: 3 + 1, 2 + 2 and 1 x 4."""
    lengths = ac.ISOLATION_LENGTHS
    offs = [int(x) for x in np.concatenate([[0], np.cumsum(lengths)])]
    seq_at = {offs[b]: b for b in range(len(lengths)) if lengths[b] > 0}
    _, packs = ac.pack_rules(lengths)
    mixed = set()
    for p in packs:
        ks = tuple(ac.block_class(L) for _, L in p if L > 0)
        par = {seq_at[r0] % 2 for r0, L in p if L > 0}
        if len(par) == 2:
            mixed.add(ks)
    assert {(3, 1), (2, 2), (1, 1, 1, 1)} <= mixed
