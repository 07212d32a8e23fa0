"""The float64 restatement of the frame MLP's backward (tests/td_mlp_grad_restatement.py) against torch's float64
autograd through the reference expression (models/modules/dynamic.py:11-40), against central differences, at the kink and at
depth 1; the inputs of the GPU test keep their margin from the kink; the surface the GPU test calls exists.  No GPU."""
import importlib
import inspect
import os

import numpy as np
import pytest
import torch

import td_mlp_grad_restatement as mr
from conftest import ROOT

PKG = "neural-waveshaping-synthesis_amd"
IDS = [f"{'x'.join(map(str, s))}-{b}x{t}" for s, (b, t) in mr.CASES]


@pytest.mark.parametrize("sizes,shape", mr.CASES, ids=IDS)
def test_the_restatement_is_torchs_float64_gradient(sizes, shape):
    P = mr.params(sizes)
    x, g = mr.inputs(sizes, *shape)
    want = mr.torch_autograd_grads(x, g, *P, torch.float64)
    got = mr.flat(*mr.backward(x, g, *P))
    assert len(got) == len(want) == 1 + 4 * sizes[3] - 2
    for name, a, w in zip(mr.names(sizes[3]), got, want):
        assert a.shape == w.shape, name
        assert mr.rel_l2(a, w) <= 1e-9, (name, mr.rel_l2(a, w))
    y = mr.torch_reference(*[torch.tensor(np.array(x), dtype=torch.float64)],
                           *[[torch.tensor(a, dtype=torch.float64) for a in lst] for lst in P])
    assert mr.rel_l2(mr.forward(x, *P), y.numpy()) <= 1e-12


@pytest.mark.parametrize("sizes,shape", mr.CASES, ids=IDS)
def test_inputs_keep_the_margin_and_torch_float32_is_a_yardstick(sizes, shape):
    """the redraw ends in at most 6 rounds, no |v| is below 1e-3, and torch's float32 autograd is between 5e-8 and 2e-6 from
    float64 for every gradient tensor: a yardstick that is neither exact by accident nor broken by a flipped sign.
    The lower bound cannot hold in two places, and there it is replaced by what can: (a) with B T = 1 the last bias's gradient
    is g itself, exact in any arithmetic - torch's distance must then be exactly 0 (and the GPU test's 10 x 0 asks the kernel
    for the exact value); (b) a tensor of fewer than 8 elements that torch happens to round almost correctly sits at the level of
    one rounding, 2^-24 / sqrt(3) = 3.4e-8 on average - measured 2.5e-8 (dx of (6, 6, 9, 1) at (1, 1), 6 elements), 4.4e-8 and
    4.2e-8 (db_1, 7 elements, and db_2, 3 elements, of (5, 7, 3, 3) at (3, 33)), and so does dW = g (x) x of the bare convolution at
    B T = 1, one product and one rounding per element (2.9e-8); for those the floor is 1e-8."""
    P = mr.params(sizes)
    x, g = mr.inputs(sizes, *shape)
    assert x.dtype == g.dtype == np.float32 and x.shape == (shape[0], sizes[0], shape[1]) and g.shape == (shape[0], sizes[2], shape[1])
    assert mr.redraw_rounds(sizes, *shape) <= 6
    assert mr.min_abs_v(x, *P).min() >= mr.MARGIN
    for lst in (P[2], P[3]):
        for a in lst:
            assert np.all(a != 0.0) and np.all(a != 1.0)
    want, yard = mr.reference(sizes, *shape)
    for name, d, w in zip(mr.names(sizes[3]), yard, want):
        assert d <= 2e-6, (name, d)
        if name == f"b{sizes[3] - 1}" and shape == (1, 1):
            assert d == 0.0, (name, d)
        else:
            one_rounding = sizes[3] == 1 and shape == (1, 1)
            assert d >= (5e-8 if w.size >= 8 and not one_rounding else 1e-8), (name, d, w.size)


def test_directional_derivatives_in_float64():
    """(f(theta + h delta) - f(theta - h delta)) / 2h against <vjp, delta>, f = <y, g>, for x and each parameter group at
    (5, 7, 3, 3), (2, 5)"""
    sizes, (B, T) = (5, 7, 3, 3), (2, 5)
    P = [[a.astype(np.float64) for a in lst] for lst in mr.params(sizes)]
    x, g = (a.astype(np.float64) for a in mr.inputs(sizes, B, T))
    dx, dW, db, dgam, dbet = mr.backward(x, g, *P)
    rng = np.random.default_rng(7)
    f = lambda xx, PP: float(np.sum(mr.forward(xx, *PP) * g))
    h = 1e-6
    d = rng.standard_normal(x.shape)
    num = (f(x + h * d, P) - f(x - h * d, P)) / (2 * h)
    assert abs(num - np.sum(dx * d)) <= 1e-7 * max(1.0, abs(num)), ("x", num, np.sum(dx * d))
    for gi, (grads, name) in enumerate(zip((dW, db, dgam, dbet), ("W", "b", "gamma", "beta"))):
        deltas = [rng.standard_normal(a.shape) for a in P[gi]]
        shifted = lambda s: [lst if k != gi else [a + s * dd for a, dd in zip(lst, deltas)] for k, lst in enumerate(P)]
        num = (f(x, shifted(h)) - f(x, shifted(-h))) / (2 * h)
        ana = sum(np.sum(ga * dd) for ga, dd in zip(grads, deltas))
        assert abs(num - ana) <= 1e-7 * max(1.0, abs(num)), (name, num, ana)


def test_the_kink_convention_is_torchs():
    """gamma_1 = beta_1 = 0: every v_1 is exactly 0, LeakyReLU' there is the slope, dbeta_1 = slope sum da_1 - and torch agrees"""
    sizes, (B, T) = (5, 7, 3, 3), (2, 5)
    W, b, gam, bet = mr.params(sizes)
    gam[1], bet[1] = np.zeros_like(gam[1]), np.zeros_like(bet[1])
    x, g = mr.inputs(sizes, B, T)
    assert not mr.forward_all(x, W, b, gam, bet)[4][1].any()
    dx, dW, db, dgam, dbet = mr.backward(x, g, W, b, gam, bet)
    da1 = np.einsum("ok,bot->bkt", W[2].astype(np.float64), g.astype(np.float64))
    assert np.allclose(dbet[1], mr.SLOPE * da1.sum(axis=(0, 2)), rtol=1e-12, atol=0.0)
    assert not dx.any() and not dW[0].any() and not dW[1].any()          # gamma = 0 lets nothing through
    want = mr.torch_autograd_grads(x, g, W, b, gam, bet, torch.float64)
    k = mr.names(3).index("beta1")
    assert mr.rel_l2(dbet[1], want[k]) <= 1e-12


def test_depth_one_is_a_convolution():
    sizes, (B, T) = (6, 6, 9, 1), (3, 33)
    W, b, gam, bet = mr.params(sizes)
    assert gam == [] and bet == []
    x, g = mr.inputs(sizes, B, T)
    dx, dW, db, dgam, dbet = mr.backward(x, g, W, b, gam, bet)
    x64, g64 = x.astype(np.float64), g.astype(np.float64)
    assert dgam == [] and dbet == []
    assert np.allclose(dW[0], sum(np.outer(g64[bb, :, t], x64[bb, :, t]) for bb in range(B) for t in range(T)), rtol=1e-12, atol=1e-12)
    assert np.allclose(db[0], g64.sum(axis=(0, 2)), rtol=1e-12, atol=1e-12)
    assert np.allclose(dx, np.einsum("ok,bot->bkt", W[0].astype(np.float64), g64), rtol=1e-12, atol=1e-12)


def test_zero_gradient_in_zero_gradient_out():
    sizes = (5, 7, 3, 3)
    x, g = mr.inputs(sizes, 3, 33)
    for a in mr.flat(*mr.backward(x, np.zeros_like(g), *mr.params(sizes))):
        assert not a.any()


# ---- the surface (no GPU, no library load) ----------------------------------------------------------------------------------------
def test_the_op_exists_on_every_layer():
    lib = importlib.import_module(PKG + "._lib")
    assert {"nws_td_mlp_grad", "nws_td_mlp_grad_workspace_bytes"} <= set(lib._PROTOTYPES)
    assert len(lib._PROTOTYPES["nws_td_mlp_grad"][1]) == 22 and len(lib._PROTOTYPES["nws_td_mlp_grad_workspace_bytes"][1]) == 7
    header = open(os.path.join(ROOT, "include", "nws_hip.h")).read()
    assert "int nws_td_mlp_grad(" in header and "size_t nws_td_mlp_grad_workspace_bytes(" in header
    cops = importlib.import_module(PKG + "._cops").CtypesOps
    assert list(inspect.signature(cops.td_mlp_grad).parameters)[1:] == ["x", "grad_y", "weights", "biases", "ln_w", "ln_b", "eps",
                                                                        "slope", "want_params"]
    build = importlib.import_module(PKG + ".build")
    assert "td_mlp_grad.hip" in build.SOURCES and "-fno-slp-vectorize" in build.EXTRA_FLAGS["td_mlp_grad.hip"]


def test_the_module_surface_and_its_refusals_on_the_host():
    dyn = importlib.import_module(PKG + ".models.modules.dynamic")
    mlp = dyn.TimeDistributedMLP(5, 7, 3, 3)
    assert mlp.differentiable is False and dyn.TimeDistributedMLP.differentiable is False
    assert list(inspect.signature(dyn.td_mlp_vjp).parameters) == ["x", "net", "grad_y", "want_params"]
    assert list(inspect.signature(mlp.vjp).parameters) == ["grad_y", "x", "want_params"]
    with pytest.raises(RuntimeError, match=r"expected \(B, 5, T\)"):
        mlp.vjp(torch.zeros(2, 3, 4), torch.zeros(2, 6, 4))
    with pytest.raises(RuntimeError):                                         # CPU tensors: no arithmetic fallback
        mlp.vjp(torch.zeros(2, 3, 4), torch.zeros(2, 5, 4))
    bad = torch.nn.Sequential(torch.nn.Conv1d(4, 4, 1), torch.nn.Conv1d(4, 4, 1))
    with pytest.raises(RuntimeError, match="unexpected layer stack"):
        dyn.td_mlp_vjp(torch.zeros(1, 4, 2), bad, torch.zeros(1, 4, 2))
    model = importlib.import_module(PKG + ".models.neural_waveshaping").NeuralWaveshaping
    assert inspect.signature(model.pre_reverb_parts).parameters["want_emb"].default is False
