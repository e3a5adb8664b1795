"""rAdjGCN without a GPU: the host scale builder, the committed fixtures
against a float64 restatement of model/radj.py:28-44, and the registry."""
import numpy as np
import pytest

from tests.radj_common import CONFIGS, RADJ, Radj64, load, rel


def tiny_rowptr(f):
    nu, mi = int(f["n_users"]), int(f["m_items"])
    dst = np.concatenate([f["train_item"] + nu, f["train_user"]])
    deg = np.bincount(dst, minlength=nu + mi)
    return np.concatenate([[0], np.cumsum(deg)]).astype(np.int64), deg


def test_fixture_set():
    assert set(RADJ) == set(CONFIGS)


@pytest.mark.parametrize("r", [0.0, 0.3, 0.5, 1.0])
def test_radj_scales(r):
    from furusato_recommend_amd.graph import radj_scales
    rowptr, deg = tiny_rowptr(load("radj_r030_d64_L3.npz"))
    assert deg[-1] == 0 and deg.max() > 1  # the isolated item; multi-edges counted
    a, b = radj_scales(rowptr, r)
    assert a.dtype == np.float32 and b.dtype == np.float32 and a.shape == b.shape == deg.shape
    d = deg.astype(np.float64)
    pos = d > 0
    # float64 powers of the row lengths, rounded once
    ea = np.where(pos, np.maximum(d, 1.0) ** -r, 0.0)
    eb = np.where(pos, np.maximum(d, 1.0) ** -(1.0 - r), 0.0)
    assert np.array_equal(a, ea.astype(np.float32))
    assert np.array_equal(b, eb.astype(np.float32))
    assert a[-1] == 0.0 and b[-1] == 0.0
    # a · b = 1 / deg within 2 ulp
    inv = np.where(pos, 1.0 / np.maximum(d, 1.0), 0.0).astype(np.float32)
    prod = a * b
    assert np.all(np.abs(prod - inv) <= 2 * np.spacing(inv))
    if r == 0.5:  # both are dinv
        assert np.array_equal(a, b)


@pytest.mark.parametrize("r", [-0.1, 1.5, float("nan"), float("inf")])
def test_radj_scales_rejects(r):
    from furusato_recommend_amd.graph import radj_scales
    with pytest.raises(ValueError):
        radj_scales(np.array([0, 1, 2], np.int64), r)


@pytest.mark.parametrize("name", RADJ)
def test_fixture_against_float64_restatement(name):
    """layers / out of the reference's rAdjGCN vs radj.py:28-44 restated in
    float64 plus the layer mean (1e-6); the training keys are consistent with
    it too (loss, reg, gradient: 1e-5)."""
    f = load(name)
    r, d, L = CONFIGS[name]
    assert float(f["r"]) == r and int(f["dim"]) == d and int(f["n_layers"]) == L
    for k in ("emb0", "layers", "out", "triples", "loss", "reg", "grad", "emb_step1",
              "emb_step2", "step_losses", "r"):
        assert k in f, k
    assert "out_radj" not in f
    o = Radj64(f["train_user"], f["train_item"], f["n_users"], f["m_items"], r)
    lay = o.layers(f["emb0"], L)
    assert f["layers"].shape == (L + 1, o.n, d)
    assert np.array_equal(f["layers"][0], f["emb0"])
    for k in range(L + 1):
        assert rel(f["layers"][k], lay[k]) < 1e-6, k
    assert rel(f["out"], sum(lay) / (L + 1)) < 1e-6
    # r ≠ 0.5 is visible: LightGCN's normalisation would not pass
    if r != 0.5:
        sym = Radj64(f["train_user"], f["train_item"], f["n_users"], f["m_items"], 0.5)
        assert rel(f["layers"][1], sym.conv(lay[0])) > 1e-3
    loss, reg, g = o.loss_grad(f["emb0"], L, f["triples"], float(f["decay"]))
    assert abs(loss - float(f["loss"])) < 1e-5 * abs(loss)
    assert abs(reg - float(f["reg"])) < 1e-5 * abs(reg)
    assert rel(f["grad"], g) < 1e-5
    E, losses = o.train(f["emb0"], L, [f["triples"]] * 2, float(f["lr"]), float(f["decay"]))
    assert rel(f["emb_step2"], E) < 1e-4
    assert np.allclose(f["step_losses"], losses, rtol=1e-5, atol=0)


def test_registry():
    import furusato_recommend_amd as pkg
    from furusato_recommend_amd.lightgcn import LightGCN
    assert pkg.MODELS["radj"] is pkg.rAdjGCN
    assert issubclass(pkg.rAdjGCN, LightGCN) and pkg.rAdjGCN is not LightGCN
    assert pkg.MODELS["lgn"] is LightGCN


def test_launcher_option():
    import furusato_recommend_amd.train_dp as T
    cfg = T.build_config(T.parse_args(["--model", "radj", "--r", "0.3"]), "cuda:0")
    assert cfg["r"] == 0.3 and cfg["checkpoint_path"].endswith("ddp_radj_all.pth")
    assert T.build_config(T.parse_args([]), "cuda:0")["r"] == 0.5  # parse.py:49's default


def test_prop_launch_bytes_keyword():
    from furusato_recommend_amd._lib import IN_PRESCALED
    from furusato_recommend_amd.engine import prop_launch_bytes
    base = prop_launch_bytes(IN_PRESCALED, 1000, 5000, 64, xs_out=True, out=True)
    assert prop_launch_bytes(IN_PRESCALED, 1000, 5000, 64, xs_out=True, out=True,
                             scaled=True) == base + 1000 * 4


def test_struct_mirror_has_scales():
    from furusato_recommend_amd._lib import Prop
    names = [n for n, _ in Prop._fields_]
    assert names[-3:] == ["scale_src", "scale_dst", "scale_next"]
