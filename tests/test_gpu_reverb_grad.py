"""-m gpu: the transpose of the learned reverb (csrc/reverb_fft.hip through Reverb.vjp and Reverb.differentiable)
against the float64 restatement of its definition (tests/reverb_grad_restatement.py).

Every case has B = 3 - an odd batch, one utterance pair is half empty - and a 31 999-tap impulse response that weighs about as
much as the dry path.  The lengths are the smallest at which each path exists:
    640        short-buffer form (time domain, one launch)
    1152       smallest FFT call; Lc = 32000 > N, so the lags wrap
    128 x 251  overlap-save, two 125 x 512 blocks whose history / look-ahead wraps Lc = 32128
    64000      125 x 512 wave-per-row row pass: the training shape's plan
    128 x 504  DFT-matrix column pass (63 x 1024)
and N = 128 x 1001 pins each overlap-save block size (125 x 512, 125 x 1024, 125 x 2048) through NWS_REVERB_OLS_N2.

Bars.  dL/dx is the forward's arithmetic with a conjugated spectrum: relative RMS <= 3e-6 from float64, the bar
test_gpu_parity.py::test_reverb_stage holds the forward to; the forward's own distance on the same inputs is recorded beside
it.  dL/d(ir) passes through two forward transforms, a sum of B/2 x blocks products per bin and one inverse transform: the
yardstick is computed in the test - the distance of torch's float32 CPU autograd through the reference's rfft / irfft
expression from the same restatement on the same inputs - and the kernel may be at most 10 x that (the factor and the reasoning
of test_gpu_stft_grad.py: another transform and a different summation order, an estimate and not a measurement), and never
beyond the project's parity bar, 1e-4.

Measured on the MI355X, forward | dx | dir kernel | dir torch float32 CPU autograd | ratio:
    640              2.46e-7 | 1.90e-7 | 1.99e-7 | 2.61e-7 | 0.76
    1152             1.10e-7 | 1.09e-7 | 2.07e-7 | 2.76e-7 | 0.75
    128 x 251        2.33e-7 | 2.31e-7 | 2.46e-7 | 4.82e-7 | 0.51
    64000            2.32e-7 | 2.32e-7 | 2.41e-7 | 2.91e-7 | 0.83
    128 x 504        3.55e-7 | 3.54e-7 | 3.77e-7 | 2.84e-7 | 1.33
    128 x 1001, 125 x 512 / 1024 / 2048 blocks: dx 2.30e-7 / 2.36e-7 / 2.42e-7, dir 2.52e-7 / 2.48e-7 / 2.51e-7 | 3.07e-7
Adam, 30 steps at lr 3e-3 on ir: kernels 1.1543 -> 0.4279, torch float32 CPU 1.1543 -> 0.5398.  reverb(pre_reverb) from the fused
forward: 2.7e-6.  fit_reverb.py, 5 steps at lr 3e-3: 5.247 -> 4.892.
The same file passes with NWS_BACKEND=ctypes (the ctypes binding instead of torch.ops)."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import reverb_grad_restatement as rr
from conftest import ROOT
from gpu_util import build_model, dev, record

pytestmark = pytest.mark.gpu

B = 3
IR_LEN = 31999
LENGTHS = (640, 1152, 128 * 251, 64000, 128 * 504)
OLS_N = 128 * 1001
DX_TOL = 3e-6
DIR_FACTOR = 10.0
DIR_CAP = 1e-4


def _nws():
    import nws_amd as nws

    return nws


def _reverb(ir):
    rev = _nws().Reverb(2, 16000)
    assert rev.ir.shape == (1, IR_LEN)
    with torch.no_grad():
        rev.ir.copy_(torch.as_tensor(np.array(ir)).reshape(1, -1))
    return rev.cuda()


@functools.lru_cache(maxsize=None)
def _reference(N):
    """(y, dx, dir) in float64 and the distances (dx, dir) of torch's float32 CPU autograd from them; read-only"""
    x, g, ir = rr.inputs(B, N, IR_LEN)
    y, dx, dr = rr.forward(x, ir), rr.grad_x(g, ir), rr.grad_ir(x, g, IR_LEN)
    dx32, dir32 = rr.torch_autograd_grads(x, g, ir, torch.float32)
    for a in (y, dx, dr):
        a.setflags(write=False)
    return y, dx, dr, rr.rel_l2(dx32, dx), rr.rel_l2(dir32, dr)


def _check_shape(N, tag):
    x, g, ir = rr.inputs(B, N, IR_LEN)
    y64, dx64, dir64, yard_dx, yard_dir = _reference(N)
    rev = _reverb(ir)
    xd, gd = dev(x), dev(g)
    y = rev(xd)
    assert not y.requires_grad                                        # the default flag: no graph, as before
    dx, none = rev.vjp(xd, gd, need_ir=False)
    assert none is None and dx.shape == (B, N) and dx.dtype == torch.float32 and dx.is_cuda and not dx.requires_grad
    none, dr = rev.vjp(xd, gd, need_x=False)
    assert none is None and dr.shape == (1, IR_LEN) and dr.dtype == torch.float32 and dr.is_cuda and not dr.requires_grad
    assert rev.vjp(xd, gd, need_x=False, need_ir=False) == (None, None)
    both = rev.vjp(xd, gd)                                            # equal inputs, equal bits; each part on its own or together
    assert torch.equal(both[0], dx) and torch.equal(both[1], dr)
    fwd, dist_dx, dist_dir = rr.rel_l2(y.cpu().numpy(), y64), rr.rel_l2(dx.cpu().numpy(), dx64), rr.rel_l2(dr.cpu().numpy().ravel(), dir64)
    print(f"{tag} (3, {N}): forward {fwd:.2e}  dx {dist_dx:.2e} (torch float32 {yard_dx:.2e})  "
          f"dir {dist_dir:.2e} | torch float32 autograd {yard_dir:.2e} | ratio {dist_dir / yard_dir:.2f}")
    record(f"reverb_grad/{tag}_{B}x{N}", forward_rel_rms=fwd, dx_rel_rms=dist_dx, dx_torch_f32_rel_rms=yard_dx, dir_rel_l2=dist_dir,
           dir_torch_f32_rel_l2=yard_dir, dir_ratio=dist_dir / yard_dir)
    # exact: no gradient comes in, none goes out
    zeros = torch.zeros_like(gd)
    zx, zi = rev.vjp(xd, zeros)
    assert torch.equal(zx, zeros) and torch.equal(zi, torch.zeros(1, IR_LEN, device="cuda"))
    assert dist_dx <= DX_TOL
    assert dist_dir <= DIR_FACTOR * yard_dir and dist_dir <= DIR_CAP


@pytest.mark.parametrize("N", LENGTHS)
def test_both_gradients_against_the_restatement(N):
    _check_shape(N, "plan")


@pytest.mark.parametrize("n2", (512, 1024, 2048))
def test_overlap_save_block_sizes(n2, monkeypatch):
    import ctypes as C

    from nws_amd import _lib
    from nws_amd import engine as nws_engine

    monkeypatch.setenv("NWS_REVERB_OLS_N2", str(n2))
    plan = _lib.NwsReverbPlan()
    assert _lib.lib().nws_reverb_plan(OLS_N, IR_LEN + 1, C.byref(plan)) == 0
    assert (plan.N1, plan.N2, plan.Lc, plan.hist) == (125, n2, OLS_N, IR_LEN) and plan.nblk == -(-OLS_N // (125 * n2 - IR_LEN))
    nws_engine._PLAN_CACHE.clear()
    try:
        _check_shape(OLS_N, f"ols_n2_{n2}")
    finally:
        nws_engine._PLAN_CACHE.clear()


def test_autograd_carries_the_bits_of_vjp():
    N = 1152
    x, g, ir = rr.inputs(B, N, IR_LEN)
    xd, gd = dev(x), dev(g)
    rev = _reverb(ir)
    want_y = rev(xd)
    want_dx, want_dir = rev.vjp(xd, gd)
    assert not want_y.requires_grad

    leaf = xd.clone().requires_grad_()
    with pytest.raises(RuntimeError, match="inference-only"):          # the default flag: as today
        rev(leaf)
    rev.differentiable = True
    with torch.no_grad():                                              # vjp does not look at the grad mode
        again = rev.vjp(leaf, gd)
        assert torch.equal(again[0], want_dx) and torch.equal(again[1], want_dir)
        assert not rev(leaf).requires_grad
    y = rev(leaf)
    assert y.requires_grad and torch.equal(y.detach(), want_y)
    (y * gd).sum().backward()
    assert leaf.grad.shape == (B, N) and torch.equal(leaf.grad, want_dx)
    assert rev.ir.grad.shape == (1, IR_LEN) and torch.equal(rev.ir.grad, want_dir)

    # only the gradient that is needed: an x without grad, and an ir without grad
    rev.ir.grad = None
    y = rev(xd)
    assert y.requires_grad and torch.equal(y.detach(), want_y)
    (y * gd).sum().backward()
    assert torch.equal(rev.ir.grad, want_dir) and xd.grad is None
    rev.ir.requires_grad_(False)
    rev.ir.grad, leaf.grad = None, None
    (rev(leaf) * gd).sum().backward()
    assert torch.equal(leaf.grad, want_dx) and rev.ir.grad is None
    assert not rev(xd).requires_grad                                   # nothing requires grad: the plain forward
    rev.ir.requires_grad_(True)

    # an in-place change of ir (an optimiser step) is seen by the next forward and the next backward
    with torch.no_grad():
        rev.ir.mul_(0.5).add_(0.001)
    fresh = _reverb(rev.ir.detach().cpu().numpy())
    leaf.grad, rev.ir.grad = None, None
    y = rev(leaf)
    assert torch.equal(y.detach(), fresh(xd)) and not torch.equal(y.detach(), want_y)
    (y * gd).sum().backward()
    fdx, fdir = fresh.vjp(xd, gd)
    assert torch.equal(leaf.grad, fdx) and torch.equal(rev.ir.grad, fdir) and not torch.equal(fdx, want_dx)


def test_odd_circular_length_has_a_forward_and_refuses_a_gradient():
    x, g, ir = rr.inputs(B, 1152, IR_LEN)
    rev = _reverb(ir)
    xd = torch.randn(2, 32001, device="cuda")
    assert rev(xd).shape == (2, 32001)
    with pytest.raises(RuntimeError, match="odd circular length"):
        rev.vjp(xd, xd)
    rev.differentiable = True
    with pytest.raises(RuntimeError, match="odd circular length"):
        rev(xd.clone().requires_grad_())


# ---- it optimises ------------------------------------------------------------------------------------------------------------------
FIT_B, FIT_N, FIT_STEPS, FIT_LR = 2, 4096, 30, 3e-3


def _torch_stft_loss(x, y, eps=1e-8):
    """the default multi-resolution loss written with torch.stft (tests/stft_grad_restatement.torch_autograd_grad's expression)"""
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


def _torch_reverb(x, ir):
    import torch.nn.functional as F

    ir_ = torch.cat((torch.zeros(1, 1, dtype=x.dtype), ir), dim=-1)
    x_ = F.pad(x, (0, ir_.shape[-1] - x.shape[-1]))
    return x + torch.fft.irfft(torch.fft.rfft(x_) * torch.fft.rfft(ir_))[..., : x.shape[-1]]


def torch_fit(pre, ir_true, steps=FIT_STEPS, lr=FIT_LR):
    """(first loss, last loss) of Adam on ir from 0.5 ir_true, float32 CPU autograd through torch.stft and rfft / irfft"""
    pre, ir_true = torch.as_tensor(np.array(pre)), torch.as_tensor(np.array(ir_true)).reshape(1, -1)
    with torch.no_grad():
        target = _torch_reverb(pre, ir_true)
    ir = (0.5 * ir_true).clone().requires_grad_()
    opt = torch.optim.Adam([ir], lr=lr)
    first = None
    for _ in range(steps):
        opt.zero_grad()
        loss = _torch_stft_loss(_torch_reverb(pre, ir), target)
        loss.backward()
        opt.step()
        first = float(loss.detach()) if first is None else first
    with torch.no_grad():
        return first, float(_torch_stft_loss(_torch_reverb(pre, ir), target))


def test_it_optimises():
    """Adam on reverb.ir through the differentiable loss, from half the true impulse response: the kernel path must lower the loss
    by at least half of what torch's float32 CPU autograd lowers it by on the same problem - a guard against a wrong sign or
    scale, not a measurement.  The learning rate was chosen on the CPU so that torch's run lowers the loss by a third or more
    (1e-3: 1.154 -> 0.735, 3e-3: 1.154 -> 0.540, 1e-2: 1.154 -> 0.566)."""
    nws = _nws()
    pre, _, ir_true = rr.inputs(FIT_B, FIT_N, IR_LEN)
    t_first, t_last = torch_fit(pre, ir_true)
    assert t_last <= t_first * (2.0 / 3.0), (t_first, t_last)
    pre_d = dev(pre)
    target = _reverb(ir_true)(pre_d)
    rev = _reverb(0.5 * np.asarray(ir_true))
    rev.differentiable = True
    loss_fn = nws.MultiResolutionSTFTLoss(differentiable=True)
    opt = torch.optim.Adam([rev.ir], lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = loss_fn(rev(pre_d), target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    with torch.no_grad():
        first, last = float(losses[0]), float(loss_fn(rev(pre_d), target))
    print(f"Adam, {FIT_STEPS} steps at lr {FIT_LR} on ir, (2, 4096): kernels {first:.4f} -> {last:.4f}, torch float32 CPU {t_first:.4f} -> {t_last:.4f}")
    record("reverb_grad/adam_30_steps", first=first, last=last, torch_first=t_first, torch_last=t_last)
    assert first - last >= 0.5 * (t_first - t_last)


# ---- the model ----------------------------------------------------------------------------------------------------------------------
def _controls(n, T, seed):
    g = torch.Generator().manual_seed(seed)
    return 180.0 + 400.0 * torch.rand(n, 1, T, generator=g), torch.randn(n, 2, T, generator=g), g


def test_pre_reverb_is_the_reverbs_input():
    """pre_reverb runs the stage kernels module by module and not forward_audio_pre, so reverb(pre_reverb(.)) is the fused
    forward within the parity bar (1e-4 relative RMS), not to the bit"""
    model = build_model(fast=True)
    f0, control, g = _controls(2, 16, 5)
    pu, nz = torch.rand(101, generator=g).cuda(), torch.rand(128 * 16 - 1, generator=g).cuda()
    want = model(f0.cuda(), control.cuda(), phase_u=pu, noise=nz)
    pre = model.pre_reverb(f0.cuda(), control.cuda(), phase_u=pu, noise=nz)
    assert pre.shape == (2, 128 * 16) and not pre.requires_grad
    assert torch.equal(pre, model.pre_reverb(f0.cuda(), control.cuda(), pu, nz))
    got = model.reverb(pre)
    dist = rr.rel_l2(got.cpu().numpy(), want.cpu().numpy())
    print(f"reverb(pre_reverb) from forward: {dist:.2e} relative RMS")
    record("reverb_grad/pre_reverb", rel_rms=dist)
    assert dist <= 1e-4
    torch.cuda.manual_seed(11)                                         # the same draws as forward, in the same order
    a = model(f0.cuda(), control.cuda())
    torch.cuda.manual_seed(11)
    b = model.reverb(model.pre_reverb(f0.cuda(), control.cuda()))
    assert rr.rel_l2(b.cpu().numpy(), a.cpu().numpy()) <= 1e-4


def test_fit_reverb_script(tmp_path):
    """scripts/fit_reverb.py as a subprocess on four T = 16 items whose targets are the model's own render through a stronger
    impulse response: exit code 0, the printed loss falls, and the written checkpoint loads and differs in reverb.ir only"""
    import re

    T, names = 16, ("a", "b", "c", "d")
    ckpt = os.path.join(ROOT, "tests", "golden", "weights_vn.npz")
    root = tmp_path / "data"
    for sub in ("control", "audio"):
        os.makedirs(root / "train" / sub)
    mean, std = np.array([[300.0], [0.5]]), np.array([[80.0], [0.2]])
    np.save(root / "data_mean.npy", mean)
    np.save(root / "data_std.npy", std)
    control = np.random.default_rng(3).standard_normal((len(names), 2, T)).astype(np.float32)
    model = build_model(fast=True)
    f0 = (control[:, 0:1].astype(np.float64) * std[0] + mean[0]).astype(np.float32)
    torch.cuda.manual_seed(0)
    pre = model.pre_reverb(torch.from_numpy(f0).cuda(), torch.from_numpy(control).cuda())
    strong = _reverb(rr.inputs(B, 1152, IR_LEN)[2])
    audio = strong(pre).cpu().numpy()
    for k, name in enumerate(names):
        np.save(root / "train" / "control" / f"control_{name}.npy", control[k])
        np.save(root / "train" / "audio" / f"audio_{name}.npy", audio[k])
    out = tmp_path / "fitted.npz"
    run = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fit_reverb.py"), "--model-checkpoint", ckpt, "--dataset-root",
                          str(root), "--split", "train", "--steps", "5", "--lr", "3e-3", "--output", str(out), "--use-fastnewt",
                          "--seed", "0"], capture_output=True, text=True, cwd=str(tmp_path))
    assert run.returncode == 0, run.stdout + run.stderr
    losses = [float(v) for v in re.findall(r"step \d+: loss ([0-9.]+)", run.stdout)]
    print(run.stdout)
    assert len(losses) == 5 and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    record("reverb_grad/fit_reverb_script", first=losses[0], last=losses[-1])
    before, after = np.load(ckpt), np.load(out)
    assert set(before.files) == set(after.files)
    for k in before.files:
        assert (k == "reverb.ir") != np.array_equal(before[k], after[k]), k
    fitted = _nws().NeuralWaveshaping.load_from_checkpoint(str(out))
    assert np.array_equal(fitted.reverb.ir.detach().numpy(), after["reverb.ir"])
