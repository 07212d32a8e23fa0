"""-m gpu: the backward of the control encoder (csrc/control_gru_grad.hip through the op, ControlModule.vjp and
ControlModule.differentiable) against the float64 restatement of its definition
(tests/control_gru_grad_restatement.py).

Parameter sets: 'packaged' = embedding.* of tests/golden/weights_vn.npz under a smooth control (0.5 + 0.25 sin + 0.02 normal: under
white noise the packaged recurrence is chaotic and float32 itself is 1e-4 .. 6e-3 from float64); 'default' = torch's default
initialisation under normal control.  Shapes (B, T): (1, 1) the minimum; (1, 2) one carried step; (3, 33) an odd batch, one frame
past the 32-frame tile of the parallel kernels; (2, 500) the training length, four dW_hh partials; (1, 1030) one block past the
forward's 1024-frame staging; (3, 700) 66 (utterance, chunk) units, so nine dW_hh partials - the segment sum's second trip of
p += 8, a count that is no multiple of eight.  Each once with h0 and grad_hT and once without.

Bar, for every returned tensor: the relative L2 from float64 is at most 10 x the distance of torch's float32 CPU autograd from
the same restatement on the same inputs - the yardstick is computed in the test; the factor and the reasoning are
test_gpu_fir_noise_grad.py's: another summation order, an estimate and not a measurement - and never beyond the project's parity
bar, 1e-4.  The kernel's gates start from the forward kernel's own gru_out; that is part of what is measured.

Measured on the MI355X, the worst tensor of each case as kernel | torch float32 CPU autograd | ratio (its name), then the largest
kernel distance of the case; "state" = with h0 and grad_hT:
    packaged  (1, 1)     state  x    4.55e-7 | 3.90e-7 | 1.17      x    4.55e-7
                         none   x    3.43e-7 | 7.57e-8 | 4.53      x    3.43e-7     (two elements, torch rounds them almost correctly)
              (1, 2)     state  W_hh 2.75e-7 | 2.31e-7 | 1.19      x    3.17e-7
                         none   W_hh 2.70e-7 | 1.28e-7 | 2.10      x    3.34e-7
              (3, 33)    state  x    1.37e-6 | 1.25e-6 | 1.10      h0   1.39e-6
                         none   W_ih 1.03e-6 | 8.31e-7 | 1.24      x    2.56e-6
              (2, 500)   state  h0   7.53e-6 | 5.08e-6 | 1.48      h0   7.53e-6
                         none   h0   1.91e-6 | 1.46e-6 | 1.30      W_hh 2.50e-6
              (1, 1030)  state  x    3.90e-6 | 3.60e-6 | 1.08      W_hh 4.20e-6
                         none   W_ih 1.05e-5 | 4.66e-6 | 2.24      b_ih 1.10e-5
              (3, 700)   state  b_ih 4.19e-6 | 2.53e-6 | 1.66      h0   5.41e-6
                         none   h0   5.24e-6 | 2.68e-6 | 1.96      W_hh 5.99e-6
    default   (1, 1)     state  b_ih 8.63e-8 | 5.76e-8 | 1.50      x    2.48e-7
                         none   b_hh 9.85e-8 | 6.15e-8 | 1.60      b_hh 9.85e-8
              (1, 2)     state  x    1.54e-7 | 1.12e-7 | 1.37      x    1.54e-7
                         none   W_hh 8.42e-7 | 9.87e-8 | 8.53      W_hh 8.42e-7     (the closest to the bar, see below)
              (3, 33)    state  W_hh 3.16e-7 | 1.22e-7 | 2.60      W_hh 3.16e-7
                         none   W_hh 4.08e-7 | 1.41e-7 | 2.89      W_hh 4.08e-7
              (2, 500)   state  W_hh 4.70e-7 | 4.00e-7 | 1.17      W_hh 4.70e-7
                         none   W_hh 4.80e-7 | 4.51e-7 | 1.06      W_hh 4.80e-7
              (1, 1030)  state  x    2.31e-7 | 2.27e-7 | 1.02      W_hh 4.42e-7
                         none   x    2.34e-7 | 2.28e-7 | 1.03      W_hh 4.20e-7
              (3, 700)   state  x    2.30e-7 | 2.26e-7 | 1.02      W_hh 4.61e-7
                         none   x    2.27e-7 | 2.23e-7 | 1.02      W_hh 4.32e-7
The 8.53: at (1, 2) without h0, dW_hh = v_1 (x) h_0 is one outer product with the forward kernel's h_0 = (1 - z) n; under the default
initialisation |n| ~ 0.1 and the forward kernel evaluates (1 - z) - 2 (1 - z) s, one rounding at magnitude 1 - ~1e-6 relative to such
an h_0, where torch rounds tanh itself.  It is the forward's arithmetic and averages out over more frames (2.9 at 33, 1.1 at 500).
At (1, 1) without h0, dW_hh = v (x) 0 is exactly zero for torch and for the kernel.
ControlModule.vjp at packaged (3, 33): x 7.48e-7 | 8.26e-7, W_ih 9.91e-7 | 9.92e-7, W_hh 1.01e-6 | 9.72e-7, b_ih 9.91e-7 | 9.17e-7, b_hh
9.99e-7 | 9.56e-7, W_p 3.71e-7 | 3.58e-7, b_p 1.06e-7 | 1.51e-7.  Split at t = 16: the data gradients came out bit-equal to one pass.
Adam, 30 steps at lr 1e-3 on the 6 tensors: kernels 0.9387 -> 0.2860; torch float32 CPU autograd 0.9387 -> 0.2680 (0.973 of its
decrease); the perturbation of 0.05 needed no enlarging.
The same file passes with NWS_BACKEND=ctypes (the ctypes binding instead of torch.ops), with the same figures."""
import copy
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import control_gru_grad_restatement as gr
import fir_noise_grad_restatement as nr
import td_mlp_grad_restatement as mr
from gpu_util import build_model, dev, record

pytestmark = pytest.mark.gpu

FACTOR = 10.0
CAP = 1e-4
BAD_ARG, UNSUPPORTED = -2, -1
H = gr.H


def _binding():
    from nws_amd.engine import binding

    return binding()


def _dyn():
    from nws_amd.models.modules import dynamic

    return dynamic


@functools.lru_cache(maxsize=None)
def _module(which, hidden=H):
    """a ControlModule with the parameters of a set on the device"""
    from nws_amd.models.neural_waveshaping import ControlModule

    m = ControlModule(2, hidden, H)
    if hidden == H:
        P = gr.params(which)
        with torch.no_grad():
            for p, a in zip((m.gru.weight_ih_l0, m.gru.weight_hh_l0, m.gru.bias_ih_l0, m.gru.bias_hh_l0), P[:4]):
                p.copy_(torch.as_tensor(a))
            m.proj.weight.copy_(torch.as_tensor(P[4]).reshape(H, H, 1))
            m.proj.bias.copy_(torch.as_tensor(P[5]))
    return m.cuda()


def _opt(a):
    return None if a is None else dev(a)


def _forward(which, x, h0):
    m = _module(which)
    with torch.no_grad():
        return _binding().control_gru(m._wdesc(), x, h0, False)


def _op(which, x, h0, gru_out, G, ghT, want_params=True):
    with torch.no_grad():
        return list(_binding().control_gru_grad(_module(which)._wdesc(), x, h0, gru_out, G, ghT, want_params))


@pytest.mark.parametrize("which,shape,state", gr.CASES, ids=gr.IDS)
def test_every_gradient_against_the_restatement(which, shape, state):
    B, T = shape
    x, h0, G, ghT = gr.inputs(which, B, T, state)
    want, yard = gr.reference(which, B, T, state)
    xd, h0d, Gd, ghTd = dev(x), _opt(h0), dev(G), _opt(ghT)
    gru_out, _ = _forward(which, xd, h0d)
    out = _op(which, xd, h0d, gru_out, Gd, ghTd)
    assert len(out) == len(want) == 6
    dists = []
    for name, o, w in zip(gr.NAMES, out, want):
        assert tuple(o.shape) == w.shape and o.dtype == torch.float32 and o.is_cuda and not o.requires_grad, name
        dists.append(gr.rel_l2(o.cpu().numpy(), w))
    tag = f"{which}_{B}x{T}_{'state' if state else 'nostate'}"
    for name, d, y in zip(gr.NAMES, dists, yard):
        print(f"{tag} {name}: kernel {d:.2e} | torch float32 autograd {y:.2e} | ratio {d / y if y else float(d != 0):.2f}")
    record(f"control_gru_grad/{tag}", **{n: d for n, d in zip(gr.NAMES, dists)}, **{n + "_torch_f32": y for n, y in zip(gr.NAMES, yard)})

    # exact cases: equal inputs, equal bits; the data gradients alone; no gradient in, none out; a third channel is not read
    again = _op(which, xd, h0d, gru_out, Gd, ghTd)
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    only = _op(which, xd, h0d, gru_out, Gd, ghTd, want_params=False)
    assert len(only) == 2 and torch.equal(only[0], out[0]) and torch.equal(only[1], out[1])
    for wp in (True, False):
        for o in _op(which, xd, h0d, gru_out, torch.zeros_like(Gd), None, want_params=wp):
            assert torch.equal(o, torch.zeros_like(o))
    x3 = torch.cat((xd, torch.full((B, 1, T), 1e30, device="cuda")), dim=1).contiguous()
    g3, _ = _forward(which, x3, h0d)
    assert torch.equal(g3, gru_out)
    assert all(torch.equal(a, o) for a, o in zip(_op(which, x3, h0d, gru_out, Gd, ghTd), out))

    for name, d, y in zip(gr.NAMES, dists, yard):
        assert d <= FACTOR * y and d <= CAP, (name, d, y)


def test_vjp_is_the_op_composed_with_td_mlp_vjp():
    which, (B, T) = "packaged", (3, 33)
    m = _module(which)
    x, _, _, _ = gr.inputs(which, B, T, False)
    xd = dev(x)
    g_emb = dev(np.random.default_rng(5).standard_normal((B, H, T)).astype(np.float32))
    gru_out, _ = _forward(which, xd, None)
    g_h, pg = _dyn().td_mlp_vjp(gru_out.transpose(1, 2).contiguous(), m.proj, g_emb)
    out = _op(which, xd, None, gru_out, g_h.transpose(1, 2).contiguous(), None)
    gx, grads = m.vjp(g_emb, xd)
    keys = ["gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0", "proj.weight", "proj.bias"]
    assert list(grads) == keys and set(keys) == set(m.state_dict())
    assert torch.equal(gx, out[0]) and not gx.requires_grad
    for k, o in zip(keys, out[2:] + [pg["weight"], pg["bias"]]):
        assert torch.equal(grads[k], o) and not grads[k].requires_grad, k
    gx0, none = m.vjp(g_emb, xd, want_params=False)
    assert none == {} and torch.equal(gx0, gx)
    # ... and it is the gradient: the composed module against the restatement, under the op's bar
    P = gr.params(which)
    want = gr.module_backward(x, None, g_emb.cpu().numpy(), None, P)
    yard = [gr.rel_l2(a, w) for a, w in zip(gr.torch_autograd_grads(x, None, None, None, P, torch.float32, g_emb=g_emb.cpu().numpy()), want)]
    got = [gx] + [grads[k] for k in keys]
    for name, a, w, y in zip(("x", "W_ih", "W_hh", "b_ih", "b_hh", "W_p", "b_p"), got, want[:1] + want[2:], yard[:1] + yard[2:]):
        d = gr.rel_l2(a.cpu().numpy().reshape(w.shape), w)
        print(f"ControlModule.vjp {name}: kernel {d:.2e} | torch float32 autograd {y:.2e}")
        assert d <= FACTOR * y and d <= CAP, (name, d, y)
    # the engine's launcher is the same op
    model = build_model(fast=True)
    eng = model._engine
    ctl = dev(x)
    go = eng.control_gru(ctl)
    a = eng.control_gru_grad(ctl, go, g_h.transpose(1, 2).contiguous())
    wd = model.embedding._wdesc()
    with torch.no_grad():
        b = list(_binding().control_gru_grad(wd, ctl, None, go, g_h.transpose(1, 2).contiguous(), None, True))
    assert len(a) == 6 and all(torch.equal(p, q) for p, q in zip(a, b))


def test_a_split_sequence_is_the_one_pass_gradient():
    """(3, 33) split at t = 16: the second half's backward with the first half's hT as its h0, its grad_h0 handed to the first
    half as grad_hT.  The summed parameter gradients and the concatenated grad_control agree with the one-pass result within the
    bar; whether the data gradients came out bit-equal is recorded (they should: per frame the same operations in the same order)."""
    which, (B, T), cut = "packaged", (3, 33), 16
    x, h0, G, ghT = gr.inputs(which, B, T, True)
    want, yard = gr.reference(which, B, T, True)
    xd, h0d, Gd, ghTd = dev(x), dev(h0), dev(G), dev(ghT)
    full_out, _ = _forward(which, xd, h0d)
    one = _op(which, xd, h0d, full_out, Gd, ghTd)
    xa, xb = xd[:, :, :cut].contiguous(), xd[:, :, cut:].contiguous()
    ga, hmid = _forward(which, xa, h0d)
    gb, _ = _forward(which, xb, hmid)
    assert torch.equal(torch.cat((ga, gb), dim=1), full_out)
    second = _op(which, xb, hmid, gb, Gd[:, cut:].contiguous(), ghTd)
    first = _op(which, xa, h0d, ga, Gd[:, :cut].contiguous(), second[1])
    got = [torch.cat((first[0], second[0]), dim=2), first[1]] + [a + b for a, b in zip(first[2:], second[2:])]
    bit_equal = torch.equal(got[0], one[0]) and torch.equal(got[1], one[1])
    print(f"split at {cut}: data gradients bit-equal to one pass: {bit_equal}")
    record("control_gru_grad/split_3x33_at_16", data_bit_equal=float(bit_equal))
    for name, a, w, y in zip(gr.NAMES, got, want, yard):
        d = gr.rel_l2(a.cpu().numpy(), w)
        assert d <= FACTOR * y and d <= CAP, (name, d, y)


# ---- refusals: decided on the host, before any launch -------------------------------------------------------------------------------
def _raw(which, x, gru_out, G, null=(), ws_short=False, Cc=None, T=None):
    """nws_control_gru_grad through ctypes: (return code, every output tensor filled with NaN beforehand, the workspace)"""
    from nws_amd import _lib

    B, C0, T0 = x.shape
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    outs = [nan(B, 2, T0), nan(B, H), nan(3 * H, 2), nan(3 * H, H), nan(3 * H), nan(3 * H)]
    L = _lib.lib()
    nbytes = L.nws_control_gru_grad_workspace_bytes(B, T0, 1)
    assert nbytes > L.nws_control_gru_grad_workspace_bytes(B, T0, 0) > 0
    ws = torch.full((nbytes,), 0x7f, dtype=torch.uint8, device="cuda")
    a = dict(control=x.data_ptr(), gru_out=gru_out.data_ptr(), grad_out=G.data_ptr(), ws=ws.data_ptr(), gwi=outs[2].data_ptr(),
             gwh=outs[3].data_ptr(), gbi=outs[4].data_ptr(), gbh=outs[5].data_ptr())
    for k in null:
        a[k] = None
    w = _lib.NwsWeights.from_buffer_copy(_module(which)._wdesc().numpy())
    rc = L.nws_control_gru_grad(C.byref(w), a["control"], B, C0 if Cc is None else Cc, T0 if T is None else T, None, a["gru_out"],
                                a["grad_out"], None, outs[0].data_ptr(), outs[1].data_ptr(), a["gwi"], a["gwh"], a["gbi"], a["gbh"],
                                a["ws"], nbytes - 4 if ws_short else nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, outs, ws


def test_refusals_return_before_any_launch():
    which, (B, T) = "packaged", (3, 33)
    x, _, G, _ = gr.inputs(which, B, T, False)
    xd, Gd = dev(x), dev(G)
    gru_out, _ = _forward(which, xd, None)
    for kw in (dict(null=("control",)), dict(null=("gru_out",)), dict(null=("grad_out",)), dict(null=("ws",)), dict(ws_short=True),
               dict(null=("gwh",)), dict(Cc=1), dict(T=0)):
        rc, outs, ws = _raw(which, xd, gru_out, Gd, **kw)
        assert rc == BAD_ARG, (kw, rc)
        assert all(torch.isnan(o).all() for o in outs), kw                   # untouched
        assert bool((ws == 0x7f).all()), kw
    # and a valid call right after gives the op's bits
    rc, outs, _ = _raw(which, xd, gru_out, Gd)
    assert rc == 0
    assert all(torch.equal(a, o) for a, o in zip(outs, _op(which, xd, None, gru_out, Gd, None)))


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def test_autograd_carries_the_bits_of_vjp():
    which, (B, T) = "packaged", (3, 33)
    plain = _module(which)
    mod = copy.deepcopy(plain)
    mod.differentiable = True
    x, _, _, _ = gr.inputs(which, B, T, False)
    xd = dev(x)
    g = dev(np.random.default_rng(6).standard_normal((B, H, T)).astype(np.float32))
    with torch.no_grad():
        want_y = plain(xd)
    want_x, want = plain.vjp(g, xd)

    # the flag off: today's forward - no graph, and an x that requires grad is refused
    assert plain.differentiable is False and not plain(xd).requires_grad
    with pytest.raises(RuntimeError, match="inference-only"):
        plain(xd.clone().requires_grad_())

    leaf = xd.clone().requires_grad_()
    y = mod(leaf)
    assert y.requires_grad and torch.equal(y.detach(), want_y)
    (y * g).sum().backward()
    assert torch.equal(leaf.grad, want_x)
    named = dict(mod.named_parameters())
    assert set(named) == set(want)
    for k, p in named.items():
        assert p.grad is not None and p.grad.shape == p.shape and torch.equal(p.grad, want[k].view_as(p)), k

    # no parameter requires grad: the data gradient alone, the same bits; nothing requires grad: the plain forward
    for p in mod.parameters():
        p.requires_grad_(False)
        p.grad = None
    leaf.grad = None
    (mod(leaf) * g).sum().backward()
    assert torch.equal(leaf.grad, want_x) and all(p.grad is None for p in mod.parameters())
    assert not mod(xd).requires_grad and torch.equal(mod(xd), want_y)
    with torch.no_grad():                                                     # vjp does not look at the flag or the grad mode
        assert torch.equal(mod.vjp(g, xd)[0], want_x) and not mod(leaf).requires_grad
    # one parameter alone: x and the others get nothing
    mod.gru.weight_hh_l0.requires_grad_(True)
    y = mod(xd)
    assert y.requires_grad
    (y * g).sum().backward()
    assert torch.equal(mod.gru.weight_hh_l0.grad, want["gru.weight_hh_l0"])
    assert all(p.grad is None for k, p in mod.named_parameters() if k != "gru.weight_hh_l0")

    # another size runs on the runtime-size path and has no backward: with the flag set it raises, without it the forward runs
    small = _module("default", hidden=64)
    with torch.no_grad():
        assert small(xd).shape == (B, H, T)
    flagged = copy.deepcopy(small)
    flagged.differentiable = True
    with pytest.raises(RuntimeError, match="GRU\\(2 -> 128\\) only"):
        flagged(xd)
    with pytest.raises(RuntimeError, match="GRU\\(2 -> 128\\) only"):
        small.vjp(g, xd)


# ---- it optimises -------------------------------------------------------------------------------------------------------------------
FIT_B, FIT_T, FIT_STEPS, FIT_LR, FIT_PERTURB = 2, 24, 30, 1e-3, 0.05
HGEN = (128, 128, 129, 4)


def _fit_problem():
    P = gr.params("packaged")
    rng = np.random.default_rng(31)
    student = list(P)
    student[1] = (P[1] + FIT_PERTURB * rng.standard_normal(P[1].shape)).astype(np.float32)
    student[2] = (P[2] + FIT_PERTURB * rng.standard_normal(P[2].shape)).astype(np.float32)
    x = gr.inputs("packaged", FIT_B, FIT_T, False, seed=1)[0]
    u = rng.random(128 * FIT_T - 1).astype(np.float32)
    z = np.load(gr.GOLDEN)
    conv_at, norm_at = (0, 3, 6, 9), (1, 4, 7)
    hgen = ([z[f"h_generator.net.{i}.weight"].reshape(z[f"h_generator.net.{i}.weight"].shape[:2]).astype(np.float32) for i in conv_at],
            [z[f"h_generator.net.{i}.bias"].astype(np.float32) for i in conv_at],
            [z[f"h_generator.net.{i}.layer_norm.weight"].astype(np.float32) for i in norm_at],
            [z[f"h_generator.net.{i}.layer_norm.bias"].astype(np.float32) for i in norm_at])
    return P, student, x, u, hgen


def _torch_stft_loss(x, y, eps=1e-8):
    """the reference loss (auraloss's default resolutions) through torch.stft, differentiable in x"""
    import stft_loss_restatement as sr

    total = 0.0
    for n_fft, hop, win in sr.DEFAULT_RESOLUTIONS:
        w = torch.hann_window(win, dtype=x.dtype)

        def mag(s):
            S = torch.stft(s, n_fft, hop, win, window=w, center=True, pad_mode="reflect", normalized=False, onesided=True,
                           return_complex=True)
            return torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=eps))
        xm, ym = mag(x), mag(y)
        total = total + torch.norm(ym - xm, p="fro") / torch.norm(ym, p="fro") + (torch.log(xm) - torch.log(ym)).abs().mean()
    return total / len(sr.DEFAULT_RESOLUTIONS)


@functools.lru_cache(maxsize=None)
def _torch_trajectory():
    """the same fit by torch's float32 CPU autograd through nn.GRU, Conv1d, the reference MLP and noise expressions and torch.stft,
    from the same start"""
    teacher, student, x, u, hgen = _fit_problem()
    t = lambda lst: [torch.tensor(np.array(a)) for a in lst]
    hg = [t(lst) for lst in hgen]
    xt, ut, win = torch.tensor(x).transpose(1, 2).contiguous(), torch.tensor(u), torch.hann_window(256)

    def render(gru, proj):
        emb = proj(gru(xt)[0].transpose(1, 2))
        return nr.torch_reference(mr.torch_reference(emb, *hg), ut, win)[0]
    with torch.no_grad():
        target = render(*gr.torch_modules(teacher, torch.float32))
    gru, proj = gr.torch_modules(student, torch.float32)
    opt = torch.optim.Adam(list(gru.parameters()) + list(proj.parameters()), lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = _torch_stft_loss(render(gru, proj), target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def _set_params(m, P):
    with torch.no_grad():
        for p, a in zip((m.gru.weight_ih_l0, m.gru.weight_hh_l0, m.gru.bias_ih_l0, m.gru.bias_hh_l0), P[:4]):
            p.copy_(torch.as_tensor(a))
        m.proj.weight.copy_(torch.as_tensor(P[4]).reshape(H, H, 1))
        m.proj.bias.copy_(torch.as_tensor(P[5]))


def test_it_optimises():
    """Adam(lr 1e-3), 30 steps over the six tensors of a ControlModule whose gru.weight_hh_l0 and gru.bias_ih_l0 were perturbed by
    0.05 normal, towards the noise its teacher (the packaged encoder followed by the packaged h_generator) makes from the same
    control and excitation, through ControlModule, h_generator and FIRNoiseSynth (all differentiable=True) and the differentiable
    STFT loss.  This objective has no oscillator branch, so the gradient is the whole gradient.  The loss falls, by at least 0.8 of
    what torch's float32 CPU autograd achieves from the same start (rounding makes Adam trajectories drift apart)."""
    import nws_amd as nws

    teacher, student, x, u, _ = _fit_problem()
    model = build_model(fast=True)
    hgen, syn = model.h_generator, model.noise_synth
    for p in hgen.parameters():
        p.requires_grad_(False)
    hgen.differentiable = True
    syn.differentiable = True
    xd, ud = dev(x), dev(u)
    enc = copy.deepcopy(_module("packaged"))
    _set_params(enc, teacher)
    with torch.no_grad():
        target = syn(hgen(enc(xd)), noise=ud)[:, 0]
    _set_params(enc, student)
    enc.differentiable = True
    loss_fn = nws.MultiResolutionSTFTLoss(differentiable=True)
    opt = torch.optim.Adam(enc.parameters(), lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = loss_fn(syn(hgen(enc(xd)), noise=ud)[:, 0], target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    ref = _torch_trajectory()
    print(f"Adam, {FIT_STEPS} steps at lr {FIT_LR} on 6 tensors, ({FIT_B}, {FIT_T}): kernels {losses[0]:.4f} -> {losses[-1]:.4f}; "
          f"torch float32 CPU autograd {ref[0]:.4f} -> {ref[-1]:.4f}")
    print("kernels:", " ".join(f"{v:.4f}" for v in losses))
    print("torch:  ", " ".join(f"{v:.4f}" for v in ref))
    record("control_gru_grad/adam_30_steps", first=losses[0], last=losses[-1], torch_first=ref[0], torch_last=ref[-1],
           kernels=" ".join(f"{v:.5f}" for v in losses), torch=" ".join(f"{v:.5f}" for v in ref))
    assert all(p.grad is not None for p in enc.parameters())
    assert ref[-1] < ref[0]
    assert losses[-1] < losses[0]
    assert losses[0] - losses[-1] >= 0.8 * (ref[0] - ref[-1])
