"""The float64 restatement of the oscillator branch's backward (tests/newt_grad_restatement.py) against torch's
float64 autograd through the reference expression (models/modules/shaping.py:67-79), against central differences, and at the edges
of the upsampling's transpose; the surface the GPU test calls exists and refuses on the host.  No GPU."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import newt_grad_restatement as nr
from conftest import ROOT

PKG = "neural-waveshaping-synthesis_amd"


@pytest.mark.parametrize("which,shape", nr.CASES, ids=nr.IDS)
def test_the_restatement_is_torchs_float64_gradient(which, shape):
    """1e-9 relative L2 for every tensor of every case (the project's figure)"""
    P = nr.params(which)
    exciter, emb, g = nr.inputs(which, *shape)
    B, T = shape
    assert exciter.shape == (B, nr.S, 128 * T) and emb.shape == (B, nr.EMB, T) and g.shape == (B, 1, 128 * T)
    assert exciter.dtype == emb.dtype == g.dtype == np.float32
    assert nr.redraw_rounds(which, *shape) < 50 and nr.min_abs_v(emb, P).min() >= nr.MARGIN
    want = nr.torch_autograd_grads(exciter, emb, g, P, torch.float64)
    got = nr.backward(exciter, emb, g, P)
    assert set(got) == set(want) == set(nr.ALL_NAMES) and len(nr.PARAM_KEYS) == 25
    for name in nr.ALL_NAMES:
        assert got[name].shape == want[name].shape, name
        assert nr.rel_l2(got[name], want[name]) <= 1e-9, (name, nr.rel_l2(got[name], want[name]))
    t64 = lambda a: torch.tensor(np.array(a), dtype=torch.float64)
    y = nr.torch_newt(t64(exciter), t64(emb), {k: t64(v) for k, v in P.items()})
    assert nr.rel_l2(nr.forward(exciter, emb, P), y.numpy()) <= 1e-12


@pytest.mark.parametrize("which", nr.SETS)
def test_torch_float32_is_a_yardstick(which):
    """torch's float32 autograd is no further than 1e-5 from float64 for any tensor at (3, 3): the GPU bar of 10 x that stays under
    its cap of 1e-4; and the floor of the yardstick is one float32 rounding"""
    want, yard = nr.reference(which, 3, 3)
    assert set(yard) == set(nr.ALL_NAMES) and nr.FLOOR == 2.0 ** -24
    for name in nr.ALL_NAMES:
        assert nr.FLOOR <= yard[name] <= 1e-5, (name, yard[name])


def test_directional_derivatives_in_float64():
    """(f(theta + h delta) - f(theta - h delta)) / 2h against <vjp, delta>, f = <out, g>, for the exciter, film and each
    parameter group of the sample-rate part, and for emb through the whole module, at (2, 3)"""
    which, (B, T) = "default", (2, 3)
    P = {k: v.astype(np.float64) for k, v in nr.params(which).items()}
    exciter, emb, g = (a.astype(np.float64) for a in nr.inputs(which, B, T))
    film = nr.mr.forward(emb, *nr.mlp_lists(P))
    grads = nr.rate_backward(exciter, film, g, P)
    rng = np.random.default_rng(11)
    h = 1e-6
    f = lambda e, fl, PP: float(np.sum(nr.rate_forward(e, fl, PP) * g))

    def check(name, num, ana):
        assert abs(num - ana) <= 1e-6 * max(1.0, abs(num)), (name, num, ana)

    d = rng.standard_normal(exciter.shape)
    check("exciter", (f(exciter + h * d, film, P) - f(exciter - h * d, film, P)) / (2 * h), np.sum(grads["exciter"] * d))
    d = rng.standard_normal(film.shape)
    check("film", (f(exciter, film + h * d, P) - f(exciter, film - h * d, P)) / (2 * h), np.sum(grads["film"] * d))
    groups = (("shaping_fn.input_scale",), ("shaping_fn.net.0.weight", "shaping_fn.net.0.bias"),
              ("shaping_fn.net.2.weight", "shaping_fn.net.2.bias"), ("shaping_fn.net.4.weight", "shaping_fn.net.4.bias"),
              ("shaping_fn.net.6.weight", "shaping_fn.net.6.bias"), ("mixer.0.weight", "mixer.0.bias"))
    assert sorted(k for grp in groups for k in grp) == sorted(nr.RATE_KEYS)
    for grp in groups:
        deltas = {k: rng.standard_normal(P[k].shape) for k in grp}
        shifted = lambda s: {k: (v + s * deltas[k] if k in deltas else v) for k, v in P.items()}
        num = (f(exciter, film, shifted(h)) - f(exciter, film, shifted(-h))) / (2 * h)
        check(grp, num, sum(np.sum(grads[k] * deltas[k]) for k in grp))
    full = nr.backward(exciter, emb, g, P)
    d = rng.standard_normal(emb.shape)
    F = lambda c: float(np.sum(nr.forward(exciter, c, P) * g))
    check("emb", (F(emb + h * d) - F(emb - h * d)) / (2 * h), np.sum(full["emb"] * d))


def test_the_edges_of_the_upsampling_transpose():
    # T = 1: both weights land on frame 0, so dfilm is the plain sum over the hop
    i0, i1, w0, w1 = nr.lerp_table(1)
    assert not i0.any() and not i1.any() and np.allclose(w0 + w1, 1.0)
    d = np.random.default_rng(2).standard_normal((2, 5, 128))
    assert np.allclose(nr.upsample_transpose(d, 1)[..., 0], d.sum(axis=-1), rtol=1e-13, atol=1e-13)
    # the first 64 samples have w1 = 0 and contribute nothing through it; the last 64 put both weights on frame T - 1
    T = 3
    i0, i1, w0, w1 = nr.lerp_table(T)
    assert not w1[:64].any() and np.all(w0[:64] == 1.0) and not i0[:64].any()
    assert np.all(i0[-64:] == T - 1) and np.all(i1[-64:] == T - 1) and np.all(w1[-64:] > 0)
    d = np.zeros((1, 1, 128 * T))
    d[..., :64] = 1.0
    assert np.array_equal(nr.upsample_transpose(d, T)[0, 0], [64.0, 0.0, 0.0])
    d = np.zeros((1, 1, 128 * T))
    d[..., -64:] = 1.0
    assert np.allclose(nr.upsample_transpose(d, T)[0, 0], [0.0, 0.0, 64.0], rtol=1e-13, atol=1e-13)
    # every aligned block of 64 samples names one (i0, i1) pair, and the transpose is the adjoint of the upsampling
    for TT in (1, 2, 3, 5):
        a, b, _, _ = nr.lerp_table(TT)
        for j in range(2 * TT):
            assert len(set(a[64 * j:64 * j + 64])) == 1 and len(set(b[64 * j:64 * j + 64])) == 1
        rng = np.random.default_rng(TT)
        film, dd = rng.standard_normal((2, 3, TT)), rng.standard_normal((2, 3, 128 * TT))
        assert abs(np.sum(nr.upsample(film) * dd) - np.sum(film * nr.upsample_transpose(dd, TT))) <= 1e-10
    # ... and it is torch's upsampling
    film = np.random.default_rng(9).standard_normal((2, 4, 5))
    up = torch.nn.functional.interpolate(torch.tensor(film), size=128 * 5, mode="linear").numpy()
    assert np.allclose(nr.upsample(film), up, rtol=1e-13, atol=1e-13)


def test_zero_gradient_in_zero_gradient_out():
    exciter, emb, g = nr.inputs("default", 1, 2)
    for a in nr.backward(exciter, emb, np.zeros_like(g), nr.params("default")).values():
        assert not a.any()


# ---- the surface (no GPU) ---------------------------------------------------------------------------------------------------------------
def test_the_op_exists_on_every_layer():
    lib = importlib.import_module(PKG + "._lib")
    header = open(os.path.join(ROOT, "include", "nws_hip.h")).read()
    names = set(re.findall(r"\b(nws_newt_grad\w*)\s*\(", header))
    assert names == {"nws_newt_grad", "nws_newt_grad_workspace_bytes"} and names <= set(lib._PROTOTYPES)
    assert len(lib._PROTOTYPES["nws_newt_grad"][1]) == 22 and len(lib._PROTOTYPES["nws_newt_grad_workspace_bytes"][1]) == 3
    assert "#define NWS_ABI_VERSION 6" in header
    cops = importlib.import_module(PKG + "._cops").CtypesOps
    assert list(inspect.signature(cops.newt_grad).parameters)[1:] == ["wdesc", "exciter", "film", "grad_out", "want_exciter", "want_params"]
    ops = open(os.path.join(ROOT, PKG, "csrc", "torch_ops.cpp")).read()
    assert ('m.def("newt_grad(Tensor wdesc, Tensor exciter, Tensor film, Tensor grad_out, bool want_exciter, bool want_params) '
            '-> Tensor[]"') in ops
    build = importlib.import_module(PKG + ".build")
    assert "newt_grad.hip" in build.SOURCES and "-fno-slp-vectorize" in build.EXTRA_FLAGS["newt_grad.hip"]


def test_refusals_are_decided_on_the_host():
    """every refusal of nws_newt_grad returns before the first device call, so it can be asked for without a GPU"""
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    UNSUPPORTED, BAD_ARG = -1, -2
    film_part = lambda B, T: B * 256 * 2 * T * 2 * 4
    row = (64 * 170 + 64 + 4) * 4
    assert L.nws_newt_grad_workspace_bytes(3, 3, 0) == film_part(3, 3)
    assert L.nws_newt_grad_workspace_bytes(3, 3, 1) == film_part(3, 3) + 1 * row           # 18 units: one workgroup per shaper
    assert L.nws_newt_grad_workspace_bytes(1, 17, 1) == film_part(1, 17) + 2 * row         # 34 units: two
    # 64 000 units: at most 256 partials, 4 waves each -> 252 units per workgroup, 254 workgroups per shaper
    assert L.nws_newt_grad_workspace_bytes(64, 500, 1) == film_part(64, 500) + 254 * row
    assert [L.nws_newt_grad_workspace_bytes(*a) for a in ((0, 5, 1), (5, 0, 1), (-1, 5, 0), (1, 65536, 1), (1 << 20, 1 << 10, 0))] == [0] * 5

    fake = 4096                                                      # never followed: every call below is refused on the host
    w = lib.NwsWeights()
    for f in ("shaper_in_scale", "shaper_w0", "shaper_b0", "shaper_w2", "shaper_b2", "shaper_w4", "shaper_b4", "shaper_w6", "shaper_b6",
              "newt_out_w", "newt_out_b"):
        setattr(w, f, fake)
    nbytes = L.nws_newt_grad_workspace_bytes(3, 3, 1)

    def call(**kw):
        a = dict(w=C.byref(w), exciter=fake, film=fake, g=fake, B=3, T=3, ge=fake, gf=fake, gp=[fake] * 11, ws=fake, ws_bytes=nbytes)
        a.update(kw)
        return L.nws_newt_grad(a["w"], a["exciter"], a["film"], a["g"], a["B"], a["T"], a["ge"], a["gf"], *a["gp"], a["ws"],
                               a["ws_bytes"], None)

    ten = lambda i: [None if k == i else fake for k in range(11)]
    for bad in (dict(w=None), dict(exciter=None), dict(film=None), dict(g=None), dict(gf=None), dict(ws=None), dict(ws_bytes=nbytes - 4),
                dict(gp=ten(0)), dict(gp=ten(5)), dict(gp=ten(10)), dict(gp=[fake] + [None] * 10), dict(T=0), dict(B=0), dict(B=-3)):
        assert call(**bad) == BAD_ARG, bad
    assert call(w=C.byref(lib.NwsWeights())) == BAD_ARG
    assert call(T=65536) == UNSUPPORTED and call(B=1 << 20, T=1 << 10) == UNSUPPORTED
    lut = lib.NwsWeights.from_buffer_copy(bytes(w))
    lut.lut = fake
    assert call(w=C.byref(lut)) == UNSUPPORTED
    small = L.nws_newt_grad_workspace_bytes(3, 3, 0)
    assert call(gp=[None] * 11, ws_bytes=small - 4) == BAD_ARG and call(gp=[None] * 11, ws=None) == BAD_ARG


def test_the_module_surface_and_its_refusals_on_the_host():
    shaping = importlib.import_module(PKG + ".models.modules.shaping")
    dyn = importlib.import_module(PKG + ".models.modules.dynamic")
    importlib.import_module(PKG).ensure_default_config()                      # depth 4 and the sine activations come from newt.gin
    m = shaping.NEWT()
    assert m.differentiable is False and shaping.NEWT.differentiable is False
    sig = inspect.signature(m.vjp).parameters
    assert list(sig) == ["grad_out", "exciter", "control_embedding", "want_params", "want_exciter"]
    assert sig["want_params"].default is True and sig["want_exciter"].default is True
    assert sorted(k for k, _ in m.named_parameters()) == sorted(nr.PARAM_KEYS) and len(nr.PARAM_KEYS) == 25
    with pytest.raises(RuntimeError):                                         # CPU tensors: no arithmetic fallback
        m.vjp(torch.zeros(2, 1, 256), torch.zeros(2, 64, 256), torch.zeros(2, 128, 2))
    # another size set raises and names it, with the flag in the forward and without it in vjp
    other = shaping.NEWT(n_waveshapers=32)
    with pytest.raises(RuntimeError, match="this is 32 shapers of width 8"):
        other.vjp(torch.zeros(2, 1, 256), torch.zeros(2, 32, 256), torch.zeros(2, 128, 2))
    wide = shaping.NEWT(shaping_fn_size=16)
    wide.differentiable = True
    with pytest.raises(RuntimeError, match="64 shapers of width 16"):
        wide(torch.zeros(2, 64, 256, requires_grad=True), torch.zeros(2, 128, 2))
    # FastNEWT: the table has no backward
    fast = shaping.FastNEWT.__new__(shaping.FastNEWT)
    torch.nn.Module.__init__(fast)
    assert fast.differentiable is False
    fast.differentiable = False
    for attempt in (lambda: setattr(fast, "differentiable", True), lambda: fast.vjp(None, None, None)):
        with pytest.raises(RuntimeError, match="lookup table has no backward") as e:
            attempt()
        assert "exact NEWT" in str(e.value) and "reference" in str(e.value)
    # Conv1x1
    conv = dyn.Conv1x1(101, 64, 1)
    assert conv.differentiable is False and dyn.Conv1x1.differentiable is False
    sig = inspect.signature(conv.vjp).parameters
    assert list(sig) == ["grad_y", "x", "want_params"] and sig["want_params"].default is True
    with pytest.raises(RuntimeError, match=r"expected \(B, 101, N\)"):
        conv.vjp(torch.zeros(2, 64, 4), torch.zeros(2, 100, 4))
    with pytest.raises(RuntimeError):                                         # CPU tensors
        conv.vjp(torch.zeros(2, 64, 4), torch.zeros(2, 101, 4))
    # the Lightning hooks still raise with the pinned phrase, and now name the new link and its script
    pkg = importlib.import_module(PKG)
    pkg.ensure_default_config()
    model = pkg.NeuralWaveshaping()
    assert isinstance(model.harmonic_mixer, dyn.Conv1x1) and model.newt.differentiable is False
    for call in (lambda: model.training_step({}, 0), model.configure_optimizers):
        with pytest.raises(NotImplementedError, match="no backward pass in this package") as e:
            call()
        assert "NEWT" in str(e.value) and "control encoder" in str(e.value) and "scripts/fit_newt.py" in str(e.value)


def test_the_fit_script_has_the_conventions_of_fit_noise():
    text = open(os.path.join(ROOT, "scripts", "fit_newt.py")).read()
    for opt in ('"--params"', '"--seed"', '"--model-checkpoint"', '"--dataset-root"', '"--output"', '"--steps"'):
        assert opt in text, opt
    assert '["shapers", "branch", "model"]' in text and "--use-fastnewt" not in text
    assert "write_checkpoint" in text and "torch.cuda.manual_seed" in text
