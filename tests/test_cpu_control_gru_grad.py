"""The float64 restatement of the control encoder's backward (tests/control_gru_grad_restatement.py) against torch's
float64 autograd through nn.GRU + Conv1d, its two forms against each other, against central differences; torch's float32 autograd
as the yardstick of the GPU test; the surface the GPU test calls exists and the C ABI refuses on the host.  No GPU."""
import ctypes as C
import importlib
import inspect
import os
import re

import numpy as np
import pytest
import torch

import control_gru_grad_restatement as gr
from conftest import ROOT

PKG = "neural-waveshaping-synthesis_amd"


@pytest.mark.parametrize("which,shape,state", gr.CASES, ids=gr.IDS)
def test_the_restatement_is_torchs_float64_gradient(which, shape, state):
    """every tensor of every case: dx, dh0, the four GRU gradients and, through the composed module, proj's two; the coefficient
    form against the direct chain rule"""
    B, T = shape
    P = gr.params(which)
    x, h0, G, ghT = gr.inputs(which, B, T, state)
    direct = gr.backward_direct(x, h0, G, ghT, *P[:4])
    coef = gr.backward_coef(x, h0, G, ghT, *P[:4])
    want = gr.torch_autograd_grads(x, h0, G, ghT, P, torch.float64)
    assert len(direct) == len(coef) == len(want) == 6
    for name, d, c, w in zip(gr.NAMES, direct, coef, want):
        assert d.shape == c.shape == w.shape, name
        assert gr.rel_l2(c, d) <= 1e-12, (name, gr.rel_l2(c, d))
        assert gr.rel_l2(c, w) <= 1e-9, (name, gr.rel_l2(c, w))
    # the composed module: grad_emb through proj, then the recurrence
    g_emb = np.random.default_rng(5).standard_normal((B, gr.H, T)).astype(np.float32)
    got = gr.module_backward(x, h0, g_emb, ghT, P)
    want = gr.torch_autograd_grads(x, h0, None, ghT, P, torch.float64, g_emb=g_emb)
    assert len(got) == len(want) == 8
    for name, a, w in zip(gr.NAMES + ("W_p", "b_p"), got, want):
        assert a.shape == w.shape and gr.rel_l2(a, w) <= 1e-9, (name, gr.rel_l2(a, w))
    # the forward itself
    gru, _ = gr.torch_modules(P, torch.float64)
    with torch.no_grad():
        h0t = None if h0 is None else torch.tensor(h0, dtype=torch.float64)[None]
        out = gru(torch.tensor(x, dtype=torch.float64).transpose(1, 2), h0t)[0]
    assert gr.rel_l2(gr.forward(x, h0, *P[:4])["h"], out.numpy()) <= 1e-12


@pytest.mark.parametrize("which,shape,state", gr.CASES, ids=gr.IDS)
def test_torch_float32_is_a_yardstick(which, shape, state):
    """torch's float32 CPU autograd is below 1e-5 from float64 for every tensor of every case, so ten times the yardstick stays
    under the 1e-4 cap of the GPU test (measured here: 2e-8 .. 6e-6)"""
    x, h0, G, ghT = gr.inputs(which, *shape, state)
    assert x.dtype == G.dtype == np.float32 and x.shape == (shape[0], 2, shape[1]) and G.shape == (shape[0], shape[1], gr.H)
    assert (h0 is None) == (ghT is None) == (not state)
    want, yard = gr.reference(which, *shape, state)
    for name, d, w in zip(gr.NAMES, yard, want):
        # (one frame from h0 = 0: dW_hh = v (x) 0 is exactly zero, for torch too - the GPU test's 10 x 0 then asks the kernel for zeros)
        assert np.isfinite(w).all() and (np.any(w != 0.0) or (name == "W_hh" and shape[1] == 1 and not state and d == 0.0)), name
        print(f"{which} {shape} {'state' if state else 'nostate'} {name}: torch float32 {d:.2e}")
        assert d < 1e-5, (name, d)


def test_directional_derivatives_in_float64():
    """(f(theta + h delta) - f(theta - h delta)) / 2h against <vjp, delta>, f = <gru_out, G> + <h_T, grad_hT>, for x, h0 and each
    parameter group at (2, 5)"""
    B, T = 2, 5
    for which in gr.SETS:
        P = [a.astype(np.float64) for a in gr.params(which)[:4]]
        x, h0, G, ghT = (a.astype(np.float64) for a in gr.inputs(which, B, T, True))
        grads = gr.backward_coef(x, h0, G, ghT, *P)
        rng = np.random.default_rng(7)

        def f(xx, hh, PP):
            h = gr.forward(xx, hh, *PP)["h"]
            return float(np.sum(h * G) + np.sum(h[:, -1] * ghT))
        eps = 1e-6
        d = rng.standard_normal(x.shape)
        num = (f(x + eps * d, h0, P) - f(x - eps * d, h0, P)) / (2 * eps)
        assert abs(num - np.sum(grads[0] * d)) <= 1e-7 * max(1.0, abs(num)), ("x", num)
        d = rng.standard_normal(h0.shape)
        num = (f(x, h0 + eps * d, P) - f(x, h0 - eps * d, P)) / (2 * eps)
        assert abs(num - np.sum(grads[1] * d)) <= 1e-7 * max(1.0, abs(num)), ("h0", num)
        for k, name in enumerate(gr.NAMES[2:]):
            d = rng.standard_normal(P[k].shape)
            shifted = lambda s: [a + s * d if i == k else a for i, a in enumerate(P)]
            num = (f(x, h0, shifted(eps)) - f(x, h0, shifted(-eps))) / (2 * eps)
            ana = np.sum(grads[2 + k] * d)
            assert abs(num - ana) <= 1e-7 * max(1.0, abs(num)), (which, name, num, ana)


def test_zero_gradient_in_zero_gradient_out():
    x, h0, G, _ = gr.inputs("packaged", 3, 33, True)
    for a in gr.backward_coef(x, h0, np.zeros_like(G), None, *gr.params("packaged")[:4]):
        assert not a.any()


# ---- the surface (no GPU) -----------------------------------------------------------------------------------------------------------
def test_every_new_header_symbol_has_a_prototype():
    with open(os.path.join(ROOT, "include", "nws_hip.h")) as f:
        names = set(re.findall(r"\b(nws_control_gru_grad\w*)\s*\(", f.read()))
    assert names == {"nws_control_gru_grad_workspace_bytes", "nws_control_gru_grad"}
    lib = importlib.import_module(PKG + "._lib")
    assert names <= set(lib._PROTOTYPES)
    assert len(lib._PROTOTYPES["nws_control_gru_grad"][1]) == 18 and len(lib._PROTOTYPES["nws_control_gru_grad_workspace_bytes"][1]) == 3
    assert lib.ABI_VERSION == 6
    with open(os.path.join(ROOT, PKG, "build.py")) as f:
        assert '"control_gru_grad.hip"' in f.read()
    build = importlib.import_module(PKG + ".build")
    assert "control_gru_grad.hip" in build.SOURCES and "-fno-slp-vectorize" in build.EXTRA_FLAGS["control_gru_grad.hip"]
    cops = importlib.import_module(PKG + "._cops").CtypesOps
    assert list(inspect.signature(cops.control_gru_grad).parameters)[1:] == ["wdesc", "control", "h0", "gru_out", "grad_out", "grad_hT",
                                                                             "want_params"]
    eng = importlib.import_module(PKG + ".engine").Engine
    assert list(inspect.signature(eng.control_gru_grad).parameters)[1:4] == ["control", "gru_out", "grad_out"]


def test_c_abi_refusals_are_decided_before_anything_is_enqueued():
    """every refusal of nws_control_gru_grad returns before the first device call, so it can be asked for without a GPU"""
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    OK, UNSUPPORTED, BAD_ARG = 0, -1, -2
    H = gr.H
    planes = lambda B, T: 6 * B * T * H * 4
    assert L.nws_control_gru_grad_workspace_bytes(3, 33, 0) == planes(3, 33)
    # with parameters: one row of 1536 column sums per (utterance, 32-frame chunk), P = min(ceil(U / 8), 32) partials of dW_hh
    assert L.nws_control_gru_grad_workspace_bytes(3, 33, 1) == planes(3, 33) + (6 * 1536 + 1 * 384 * 128) * 4
    assert L.nws_control_gru_grad_workspace_bytes(64, 500, 1) == planes(64, 500) + (1024 * 1536 + 32 * 384 * 128) * 4
    assert [L.nws_control_gru_grad_workspace_bytes(*a) for a in ((0, 5, 1), (5, 0, 1), (-1, 5, 0), (65536, 5, 1))] == [0] * 4
    assert L.nws_control_gru_grad_workspace_bytes(65535, 1, 0) == planes(65535, 1)

    fake = 4096                                                      # never followed: every call below is refused on the host
    w = lib.NwsWeights()
    for f in ("gru_w_ih", "gru_w_hh", "gru_b_ih", "gru_b_hh"):
        setattr(w, f, fake)
    nbytes = L.nws_control_gru_grad_workspace_bytes(3, 33, 1)

    def call(**kw):
        a = dict(w=C.byref(w), control=fake, B=3, C=2, T=33, h0=None, gru_out=fake, grad_out=fake, grad_hT=None, gc=fake, gh0=fake,
                 gwi=fake, gwh=fake, gbi=fake, gbh=fake, ws=fake, ws_bytes=nbytes)
        a.update(kw)
        return L.nws_control_gru_grad(a["w"], a["control"], a["B"], a["C"], a["T"], a["h0"], a["gru_out"], a["grad_out"], a["grad_hT"],
                                      a["gc"], a["gh0"], a["gwi"], a["gwh"], a["gbi"], a["gbh"], a["ws"], a["ws_bytes"], None)

    for bad in (dict(w=None), dict(control=None), dict(gru_out=None), dict(grad_out=None), dict(ws=None), dict(ws_bytes=nbytes - 4),
                dict(ws=fake + 4), dict(gwi=None), dict(gwh=None), dict(gbi=None), dict(gbh=None), dict(gwi=None, gwh=None, gbi=None),
                dict(C=1), dict(T=0), dict(B=0), dict(B=-3)):
        assert call(**bad) == BAD_ARG, bad
    empty = lib.NwsWeights()
    assert call(w=C.byref(empty)) == BAD_ARG
    assert call(B=65536) == UNSUPPORTED
    # without parameters the smaller workspace serves; it is still required
    small = L.nws_control_gru_grad_workspace_bytes(3, 33, 0)
    none4 = dict(gwi=None, gwh=None, gbi=None, gbh=None)
    assert call(ws_bytes=small - 4, **none4) == BAD_ARG and call(ws=None, **none4) == BAD_ARG
    assert OK == 0


def test_the_module_surface_and_its_refusals_on_the_host():
    nw = importlib.import_module(PKG + ".models.neural_waveshaping")
    m = nw.ControlModule(2, 128, 128)
    assert m.differentiable is False and nw.ControlModule.differentiable is False
    assert list(inspect.signature(m.vjp).parameters) == ["grad_emb", "x", "want_params"]
    assert inspect.signature(m.vjp).parameters["want_params"].default is True
    assert set(k for k, _ in m.named_parameters()) == {"gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0",
                                                       "proj.weight", "proj.bias"}
    with pytest.raises(RuntimeError):                                         # CPU tensors: no arithmetic fallback
        m.vjp(torch.zeros(2, 128, 4), torch.zeros(2, 2, 4))
    other = nw.ControlModule(2, 64, 128)
    with pytest.raises(RuntimeError):
        other.vjp(torch.zeros(2, 128, 4), torch.zeros(2, 2, 4))
    pkg = importlib.import_module(PKG)
    pkg.ensure_default_config()
    model = pkg.NeuralWaveshaping()
    for call in (lambda: model.training_step({}, 0), model.configure_optimizers):
        with pytest.raises(NotImplementedError, match="no backward pass in this package") as e:
            call()
        assert "ControlModule" in str(e.value) or "control encoder" in str(e.value)
