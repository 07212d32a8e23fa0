"""The reverb's transpose without a GPU: the float64 restatement the kernels are held to (tests/reverb_grad_restatement.py;
DESIGN.md 3.14) in its two forms and against torch's float64 autograd through the reference expression, and the host side of the
feature (workspace size, ABI prototypes, refusals of the C entry points, the module's flag and refusals)."""
import ctypes as C
import importlib
import os
import re

import numpy as np
import pytest
import torch

import reverb_grad_restatement as rr
from conftest import ROOT

PKG = "neural-waveshaping-synthesis_amd"


# (2, 40, 63) is the case with N < ir_len + 1: the circular length is the impulse response's, x and g are the padded side
@pytest.mark.parametrize("B,N,ir_len", ((2, 96, 63), (3, 200, 127), (2, 40, 63)))
def test_fft_form_equals_the_explicit_index_form(B, N, ir_len):
    x, g, ir = rr.inputs(B, N, ir_len)
    for name, fft, explicit in (("y", rr.forward(x, ir), rr.forward_explicit(x, ir)),
                                ("dx", rr.grad_x(g, ir), rr.grad_x_explicit(g, ir)),
                                ("dir", rr.grad_ir(x, g, ir_len), rr.grad_ir_explicit(x, g, ir_len))):
        assert fft.dtype == np.float64 and fft.shape == explicit.shape
        dist = rr.rel_l2(fft, explicit)
        print(f"({B}, {N}, ir {ir_len}) {name}: FFT form from explicit form {dist:.2e}")
        assert dist <= 1e-12
    assert rr.grad_x(g, ir).shape == (B, N) and rr.grad_ir(x, g, ir_len).shape == (ir_len,)


@pytest.mark.parametrize("B,N,ir_len", ((3, 640, 1999), (2, 4000, 1999), (3, 1152, 31999)))
def test_restatement_equals_torch_float64_autograd(B, N, ir_len):
    """both sides are float64: 1e-9 relative L2, the bar of test_cpu_stft_grad.py"""
    x, g, ir = rr.inputs(B, N, ir_len)
    dx64, dir64 = rr.torch_autograd_grads(x, g, ir, torch.float64)
    for name, got, want in (("dx", rr.grad_x(g, ir), dx64), ("dir", rr.grad_ir(x, g, ir_len), dir64)):
        dist = rr.rel_l2(got, want)
        print(f"({B}, {N}, ir {ir_len}) {name}: restatement from float64 autograd {dist:.2e}")
        assert dist <= 1e-9


def test_inputs_are_deterministic_and_the_wet_path_weighs_like_the_dry_one():
    x, g, ir = rr.inputs(3, 1152, 31999)
    assert x.dtype == g.dtype == ir.dtype == np.float32 and x.shape == g.shape == (3, 1152) and ir.shape == (1, 31999)
    assert rr.inputs(3, 1152, 31999)[0] is x and not np.array_equal(x, g)
    big = rr.inputs(3, 64000, 31999)
    wet = rr.forward(big[0], big[2]) - big[0]
    ratio = float(np.sqrt(np.mean(wet ** 2)) / np.sqrt(np.mean(big[0].astype(np.float64) ** 2)))
    assert 0.3 <= ratio <= 30.0, ratio


def _plan(lib, N, ir_len_plus1):
    plan = lib.NwsReverbPlan()
    assert lib.lib().nws_reverb_plan(N, ir_len_plus1, C.byref(plan)) == 0
    return plan


def test_workspace_bytes_is_host_only_and_monotonic():
    lib = importlib.import_module(PKG + "._lib")
    size, fwd = lib.lib().nws_reverb_grad_workspace_bytes, lib.lib().nws_reverb_workspace_bytes
    for N in (640, 1152, 128 * 251, 64000, 128 * 504, 128 * 1001):
        plan = _plan(lib, N, 32000)
        assert size(None, 3, 1) == 0 and size(C.byref(plan), 0, 1) == 0 and size(C.byref(plan), -1, 0) == 0
        bad = lib.NwsReverbPlan(plan.L, plan.N1, plan.N2 + 1, plan.Lc, plan.hist, plan.nblk)
        assert size(C.byref(bad), 3, 1) == 0 and size(C.byref(bad), 3, 0) == 0
        last = (0, 0)
        for B in (1, 2, 3, 4, 7, 64, 65):
            x_only, both = size(C.byref(plan), B, 0), size(C.byref(plan), B, 1)
            assert 0 < x_only <= both
            assert x_only == fwd(C.byref(plan), B)                     # dL/dx is the forward's launches in the forward's scratch
            assert x_only >= last[0] and both >= last[1]
            # the spectra of the x slots and of the g slots, planar, plus the summed cross spectrum and its lags
            pairs = (B + 1) // 2
            assert both >= 4 * (4 * pairs * plan.nblk + 3) * plan.L
            last = (x_only, both)


def test_header_prototypes():
    with open(os.path.join(ROOT, "include", "nws_hip.h")) as f:
        names = set(re.findall(r"\b(nws_reverb_grad\w*)\s*\(", f.read()))
    assert names == {"nws_reverb_grad_workspace_bytes", "nws_reverb_grad_x", "nws_reverb_grad_ir"}
    lib = importlib.import_module(PKG + "._lib")
    assert names <= set(lib._PROTOTYPES)
    assert lib.ABI_VERSION == 6


def test_c_abi_refusals_are_decided_before_anything_is_enqueued():
    lib = importlib.import_module(PKG + "._lib")
    L = lib.lib()
    UNSUPPORTED, BAD_ARG, WORKSPACE = -1, -2, -3
    fake = 256                                # a non-NULL address nothing may dereference before the sizes are accepted
    plan = _plan(lib, 64000, 32000)
    ols = _plan(lib, 128 * 251, 32000)
    assert plan.Lc == 0 and ols.Lc == 128 * 251
    big = 1 << 50

    def gx(p=plan, t=fake, s=fake, g=fake, B=3, N=64000, dx=fake, ws=fake, nbytes=big):
        return L.nws_reverb_grad_x(C.byref(p) if p is not None else None, t, s, g, B, N, dx, ws, nbytes, None)

    def gi(p=plan, t=fake, x=fake, g=fake, B=3, N=64000, ir_len=31999, d=fake, ws=fake, nbytes=big):
        return L.nws_reverb_grad_ir(C.byref(p) if p is not None else None, t, x, g, B, N, ir_len, d, ws, nbytes, None)

    for bad in (dict(p=None), dict(t=None), dict(s=None), dict(g=None), dict(dx=None), dict(ws=None), dict(B=0), dict(N=0),
                dict(N=64001), dict(p=ols)):
        assert gx(**bad) == BAD_ARG, bad
    for bad in (dict(p=None), dict(t=None), dict(x=None), dict(g=None), dict(d=None), dict(ws=None), dict(B=0), dict(N=0),
                dict(N=64001), dict(ir_len=0), dict(ir_len=64000), dict(p=ols), dict(p=ols, N=128 * 251, ir_len=1999)):
        assert gi(**bad) == BAD_ARG, bad
    assert gx(nbytes=L.nws_reverb_grad_workspace_bytes(C.byref(plan), 3, 0) - 1) == WORKSPACE
    assert gi(nbytes=L.nws_reverb_grad_workspace_bytes(C.byref(plan), 3, 1) - 1) == WORKSPACE
    assert gi(nbytes=L.nws_reverb_grad_workspace_bytes(C.byref(plan), 3, 0)) == WORKSPACE
    assert gx(B=2 * 65535 + 1) == UNSUPPORTED and gi(B=2 * 65535 + 1) == UNSUPPORTED


def test_module_flag_and_refusals():
    shaping = importlib.import_module(PKG + ".models.modules.shaping")
    rev = shaping.Reverb(2, 1000)
    assert rev.differentiable is False and "differentiable" not in rev.state_dict() and callable(rev.vjp)
    assert set(rev.state_dict()) == {"ir", "initial_zero"}
    x = torch.zeros(2, 640)
    for flag in (False, True):
        rev.differentiable = flag
        with pytest.raises(RuntimeError, match="no CPU fallback|AMD GPU|cuda"):
            rev.vjp(x, x)
        with pytest.raises(RuntimeError, match="no CPU fallback|AMD GPU|cuda"):
            rev(x.clone().requires_grad_())
    nw = importlib.import_module(PKG + ".models.neural_waveshaping")
    assert callable(nw.NeuralWaveshaping.pre_reverb)
