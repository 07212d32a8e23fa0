"""-m gpu: the backward of the frame MLP (csrc/td_mlp_grad.hip through the op, td_mlp_vjp, TimeDistributedMLP.vjp and
TimeDistributedMLP.differentiable) against the float64 restatement of its definition
(tests/td_mlp_grad_restatement.py).

Size sets (in, hidden, out, depth): (128, 128, 129, 4) h_generator, one channel past four 32-row tiles; (128, 128, 256, 4) newt.mlp;
(5, 7, 3, 3) every guard, the scalar weight loads, less than one tile and one K chunk; (40, 72, 33, 3) in != hidden, a partial K
chunk, a partial tile; (6, 6, 9, 1) a bare convolution.  Shapes (B, T): (1, 1) the minimum; (3, 33) an odd batch and one frame
past a tile; (2, 500), the training length and more than one K-split partial (4), for the two packaged size sets; (3, 700) for
(5, 7, 3, 3): 66 (utterance, chunk) units, so nine dW partials - the segment sum's second trip of p += 8, a count that is no multiple
of eight.
Inputs: td_mlp_grad_restatement.params / inputs (no |v| within 1e-3 of the LeakyReLU's kink).

Bar, for every returned tensor: the relative L2 from float64 is at most 10 x the distance of torch's float32 CPU autograd through
the reference expression from the same restatement on the same inputs - the yardstick is computed in the test; the factor and
the reasoning are test_gpu_fir_noise_grad.py's: another summation order, an estimate and not a measurement - and never beyond the
project's parity bar, 1e-4.  (At (1, 1) the last bias's gradient is g itself: torch's distance is 0 and the kernel's must be.)

Measured on the MI355X, the worst tensor of each case as kernel | torch float32 CPU autograd | ratio (its name), then the largest
kernel distance of the case:
    (128, 128, 129, 4)  (1, 1)    W3     3.19e-7 | 2.41e-7 | 1.32      gamma0 5.66e-7
                        (3, 33)   gamma1 5.45e-7 | 4.25e-7 | 1.28      gamma1 5.45e-7
                        (2, 500)  gamma2 4.90e-7 | 4.89e-7 | 1.00      gamma2 4.90e-7
    (128, 128, 256, 4)  (1, 1)    W3     3.02e-7 | 2.14e-7 | 1.41      gamma0 4.95e-7
                        (3, 33)   b1     4.82e-7 | 4.43e-7 | 1.09      gamma2 5.28e-7
                        (2, 500)  gamma0 5.14e-7 | 5.13e-7 | 1.00      gamma1 5.32e-7
    (5, 7, 3, 3)        (1, 1)    b0     2.88e-7 | 4.51e-8 | 6.38      W0     2.97e-7
                        (3, 33)   b2     8.05e-8 | 4.23e-8 | 1.90      x      3.02e-7
                        (3, 700)  W2     2.55e-7 | 2.03e-7 | 1.25      W0     3.17e-7
    (40, 72, 33, 3)     (1, 1)    W1     2.50e-7 | 1.33e-7 | 1.88      x      3.47e-7
                        (3, 33)   beta1  1.73e-7 | 1.26e-7 | 1.37      gamma1 2.93e-7
    (6, 6, 9, 1)        (1, 1)    W0     2.91e-8 | 2.91e-8 | 1.00      W0     2.91e-8
                        (3, 33)   W0     1.92e-7 | 9.26e-8 | 2.07      W0     1.92e-7
Adam, 30 steps at lr 1e-3 on the 14 tensors: kernels 1.5273 -> 0.7080; torch float32 CPU autograd 1.5273 -> 0.7033 (0.994 of its
decrease).  fit_noise.py --h-generator all, 5 steps at lr 3e-4: 2.6405 -> 2.0919 (--with-reverb: 2.0876).
The same file passes with NWS_BACKEND=ctypes (the ctypes binding instead of torch.ops)."""
import ctypes as C
import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import fir_noise_grad_restatement as nr
import td_mlp_grad_restatement as mr
from conftest import ROOT
from gpu_util import build_model, dev, record

pytestmark = pytest.mark.gpu

FACTOR = 10.0
CAP = 1e-4
BAD_ARG, UNSUPPORTED = -2, -1
IDS = [f"{'x'.join(map(str, s))}-{b}x{t}" for s, (b, t) in mr.CASES]


def _nws():
    import nws_amd as nws

    return nws


def _binding():
    from nws_amd.engine import binding

    return binding()


def _dyn():
    from nws_amd.models.modules import dynamic

    return dynamic


def _dev_params(P):
    return [[dev(a) for a in lst] for lst in P]


def _op(x, g, P, want_params=True):
    return _binding().td_mlp_grad(x, g, *P, mr.EPS, mr.SLOPE, want_params)


def _module(sizes, P, differentiable=False):
    """a TimeDistributedMLP (or, at depth 1, a bare Conv1d) with the parameters P on the device"""
    cin, hidden, cout, depth = sizes
    dyn = _dyn()
    W, b, gam, bet = P
    if depth == 1:
        net = torch.nn.Conv1d(cin, cout, 1)
        convs, norms = [net], []
    else:
        net = dyn.TimeDistributedMLP(cin, hidden, cout, depth)
        convs = [m for m in net.net if isinstance(m, torch.nn.Conv1d)]
        norms = [m for m in net.net if isinstance(m, dyn.TimeDistributedLayerNorm)]
        net.differentiable = differentiable
    with torch.no_grad():
        for c, w, bb in zip(convs, W, b):
            c.weight.copy_(torch.as_tensor(np.asarray(w))[:, :, None])
            c.bias.copy_(torch.as_tensor(np.asarray(bb)))
        for n, ga, be in zip(norms, gam, bet):
            n.layer_norm.weight.copy_(torch.as_tensor(np.asarray(ga)))
            n.layer_norm.bias.copy_(torch.as_tensor(np.asarray(be)))
    return net.cuda()


def _offset_view(t):
    """the same values in a contiguous view that starts 4 bytes into its storage (16-byte alignment lost)"""
    buf = torch.empty(t.numel() + 1, device="cuda")
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.is_contiguous() and v.data_ptr() % 16 == 4
    return v


@pytest.mark.parametrize("sizes,shape", mr.CASES, ids=IDS)
def test_every_gradient_against_the_restatement(sizes, shape):
    B, T = shape
    depth = sizes[3]
    P = mr.params(sizes)
    x, g = mr.inputs(sizes, B, T)
    want, yard = mr.reference(sizes, B, T)
    Pd, xd, gd = _dev_params(P), dev(x), dev(g)
    out = _op(xd, gd, Pd)
    assert len(out) == len(want) == 4 * depth - 1
    names = mr.names(depth)
    dists = []
    for name, o, w in zip(names, out, want):
        assert o.shape == w.shape and o.dtype == torch.float32 and o.is_cuda and not o.requires_grad, name
        dists.append(mr.rel_l2(o.cpu().numpy(), w))
    tag = "x".join(map(str, sizes)) + f"_{B}x{T}"
    for name, d, y in zip(names, dists, yard):
        print(f"{tag} {name}: kernel {d:.2e} | torch float32 autograd {y:.2e} | ratio {d / y if y else float(d != 0):.2f}")
    record(f"td_mlp_grad/{tag}", **{n: d for n, d in zip(names, dists)}, **{n + "_torch_f32": y for n, y in zip(names, yard)})

    # exact cases: equal inputs, equal bits; the data gradient alone; no gradient in, none out; unaligned weights
    again = _op(xd, gd, Pd)
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    only = _op(xd, gd, Pd, want_params=False)
    assert len(only) == 1 and torch.equal(only[0], out[0])
    for o in _op(xd, torch.zeros_like(gd), Pd):
        assert torch.equal(o, torch.zeros_like(o))
    assert torch.equal(_op(xd, torch.zeros_like(gd), Pd, want_params=False)[0], torch.zeros_like(xd))
    shifted = [[_offset_view(t) for t in Pd[0]]] + Pd[1:]
    assert all(torch.equal(a, o) for a, o in zip(_op(xd, gd, shifted), out))

    # vjp is the op: through the module (or td_mlp_vjp on the bare convolution), keys as in the state dict
    net = _module(sizes, P)
    if depth == 1:
        gx, grads = _dyn().td_mlp_vjp(xd, net, gd)
        keys = ["weight", "bias"]
    else:
        gx, grads = net.vjp(gd, xd)
        conv_at, norm_at = [3 * i for i in range(depth)], [3 * i + 1 for i in range(depth - 1)]
        keys = ([f"net.{i}.weight" for i in conv_at] + [f"net.{i}.bias" for i in conv_at]
                + [f"net.{i}.layer_norm.weight" for i in norm_at] + [f"net.{i}.layer_norm.bias" for i in norm_at])
        assert set(keys) == set(net.state_dict())
        gx0, none = net.vjp(gd, xd, want_params=False)
        assert none == {} and torch.equal(gx0, out[0])
    assert list(grads) == keys and torch.equal(gx, out[0])
    for k, o in zip(keys, out[1:]):
        assert torch.equal(grads[k].reshape(o.shape), o) and not grads[k].requires_grad, k

    for name, d, y in zip(names, dists, yard):
        assert d <= FACTOR * y and d <= CAP, (name, d, y)


# ---- refusals: decided on the host, before any launch -------------------------------------------------------------------------------
def _raw(x, g, P, sizes, depth=None, null=None, ws_short=False, want=True):
    """nws_td_mlp_grad through ctypes: (return code, every output tensor, filled with NaN beforehand)"""
    from nws_amd import _lib

    cin, hidden, cout, d = sizes
    depth = d if depth is None else depth
    B, _, T = x.shape
    arr = lambda ts: (C.c_void_p * 16)(*[t.data_ptr() for t in ts])
    nan = lambda t: torch.full_like(t, float("nan"))
    gx, gW, gb, gg, gl = nan(x), [nan(t) for t in P[0]], [nan(t) for t in P[1]], [nan(t) for t in P[2]], [nan(t) for t in P[3]]
    L = _lib.lib()
    nbytes = L.nws_td_mlp_grad_workspace_bytes(B, cin, hidden, cout, d, T, 1)
    assert nbytes > 0 and L.nws_td_mlp_grad_workspace_bytes(B, cin, hidden, cout, d, T, 0) == 0
    ws = torch.full((nbytes,), 0x7f, dtype=torch.uint8, device="cuda")
    args = dict(x=x.data_ptr(), g=g.data_ptr(), gx=gx.data_ptr(), ws=ws.data_ptr())
    if null:
        args[null] = None
    rc = L.nws_td_mlp_grad(args["x"], args["g"], B, cin, hidden, cout, depth, T, arr(P[0]), arr(P[1]), arr(P[2]), arr(P[3]), mr.EPS,
                           mr.SLOPE, args["gx"], arr(gW) if want else None, arr(gb) if want else None, arr(gg) if want else None,
                           arr(gl) if want else None, args["ws"], nbytes - 4 if ws_short else nbytes,
                           torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, [gx] + gW + gb + gg + gl, ws


def test_refusals_return_before_any_launch():
    sizes, (B, T) = (40, 72, 33, 3), (3, 33)
    P = mr.params(sizes)
    x, g = mr.inputs(sizes, B, T)
    Pd, xd, gd = _dev_params(P), dev(x), dev(g)
    for kw, code in ((dict(null="x"), BAD_ARG), (dict(null="g"), BAD_ARG), (dict(null="gx"), BAD_ARG), (dict(null="ws"), BAD_ARG),
                     (dict(depth=9), UNSUPPORTED), (dict(depth=0), UNSUPPORTED), (dict(ws_short=True), BAD_ARG)):
        rc, outs, ws = _raw(xd, gd, Pd, sizes, **kw)
        assert rc == code, (kw, rc)
        assert all(torch.isnan(o).all() for o in outs), kw                   # untouched
        assert bool((ws == 0x7f).all()), kw
    # a width beyond the plan: sizes only, refused before the pointers are followed
    from nws_amd import _lib

    assert _lib.lib().nws_td_mlp_grad_workspace_bytes(2, 300, 300, 5, 2, 4, 1) == 0
    # and a valid call right after gives the op's bits
    rc, outs, _ = _raw(xd, gd, Pd, sizes)
    assert rc == 0
    assert all(torch.equal(a, o) for a, o in zip(outs, _op(xd, gd, Pd)))
    rc, outs, ws = _raw(xd, gd, Pd, sizes, want=False, null="ws")            # the data gradient needs no workspace
    assert rc == 0 and torch.equal(outs[0], _op(xd, gd, Pd)[0]) and all(torch.isnan(o).all() for o in outs[1:])


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def test_autograd_carries_the_bits_of_vjp():
    sizes, (B, T) = (40, 72, 33, 3), (3, 33)
    P = mr.params(sizes)
    x, g = mr.inputs(sizes, B, T)
    xd, gd = dev(x), dev(g)
    plain, mlp = _module(sizes, P), _module(sizes, P, differentiable=True)
    with torch.no_grad():
        want_y = plain(xd)
    want_x, want = plain.vjp(gd, xd)

    # the flag off: today's forward - no graph, and an x that requires grad is refused
    assert plain.differentiable is False and not plain(xd).requires_grad
    with pytest.raises(RuntimeError, match="inference-only"):
        plain(xd.clone().requires_grad_())

    leaf = xd.clone().requires_grad_()
    y = mlp(leaf)
    assert y.requires_grad and torch.equal(y.detach(), want_y)
    (y * gd).sum().backward()
    assert torch.equal(leaf.grad, want_x)
    named = dict(mlp.named_parameters())
    assert set(named) == set(want)
    for k, p in named.items():
        assert p.grad is not None and p.grad.shape == p.shape and torch.equal(p.grad, want[k].view_as(p)), k

    # no parameter requires grad: the data gradient alone, the same bits; nothing requires grad: the plain forward
    for p in mlp.parameters():
        p.requires_grad_(False)
        p.grad = None
    leaf.grad = None
    (mlp(leaf) * gd).sum().backward()
    assert torch.equal(leaf.grad, want_x) and all(p.grad is None for p in mlp.parameters())
    assert not mlp(xd).requires_grad
    with torch.no_grad():                                                     # vjp does not look at the flag or the grad mode
        assert torch.equal(mlp.vjp(gd, xd)[0], want_x) and not mlp(leaf).requires_grad
    # parameters alone: x gets nothing
    next(mlp.parameters()).requires_grad_(True)
    y = mlp(xd)
    assert y.requires_grad
    (y * gd).sum().backward()
    first = next(iter(named))
    assert torch.equal(named[first].grad, want[first].view_as(named[first]))

    # the bare convolution of ControlModule.proj
    conv = torch.nn.Conv1d(128, 128, 1).cuda()
    gen = torch.Generator().manual_seed(3)
    h, gg = torch.randn(2, 128, 33, generator=gen).cuda(), torch.randn(2, 128, 33, generator=gen).cuda()
    gx, grads = _dyn().td_mlp_vjp(h, conv, gg)
    assert list(grads) == ["weight", "bias"] and grads["weight"].shape == conv.weight.shape
    w64 = conv.weight.detach().double().cpu().numpy()[:, :, 0]
    ref_x = np.einsum("ok,bot->bkt", w64, gg.double().cpu().numpy())
    ref_w = np.einsum("bot,bkt->ok", gg.double().cpu().numpy(), h.double().cpu().numpy())
    assert mr.rel_l2(gx.cpu().numpy(), ref_x) <= 1e-6 and mr.rel_l2(grads["weight"].cpu().numpy()[:, :, 0], ref_w) <= 1e-6
    assert mr.rel_l2(grads["bias"].cpu().numpy(), gg.double().sum(dim=(0, 2)).cpu().numpy()) <= 1e-6


# ---- it optimises -------------------------------------------------------------------------------------------------------------------
FIT_SIZES, FIT_B, FIT_T, FIT_STEPS, FIT_LR = (128, 128, 129, 4), 2, 24, 30, 1e-3


def _fit_problem():
    teacher = mr.params(FIT_SIZES, seed=1)
    other = mr.params(FIT_SIZES, seed=2)
    student = [list(lst) for lst in teacher]
    for i in (2, 3):                                                          # the last two layers redrawn
        student[0][i], student[1][i] = other[0][i], other[1][i]
    student[2][2], student[3][2] = other[2][2], other[3][2]
    rng = np.random.default_rng(24)
    emb = rng.standard_normal((FIT_B, 128, FIT_T)).astype(np.float32)
    u = rng.random(128 * FIT_T - 1).astype(np.float32)
    return teacher, student, emb, u


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
    """the same fit by torch's float32 CPU autograd through the reference expressions and torch.stft, from the same start"""
    teacher, student, emb, u = _fit_problem()
    t = lambda lst, grad=False: [torch.tensor(np.array(a), requires_grad=grad) for a in lst]
    embt, ut, win = torch.tensor(emb), torch.tensor(u), torch.hann_window(256)
    with torch.no_grad():
        target = nr.torch_reference(mr.torch_reference(embt, *[t(lst) for lst in teacher]), ut, win)[0]
    leaves = [t(lst, True) for lst in student]
    opt = torch.optim.Adam([p for lst in leaves for p in lst], lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = _torch_stft_loss(nr.torch_reference(mr.torch_reference(embt, *leaves), ut, win)[0], target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_it_optimises():
    """Adam(lr 1e-3), 30 steps over all 14 tensors of an h_generator whose last two layers were redrawn, towards the noise its
    teacher makes from the same embedding and excitation, through FIRNoiseSynth(differentiable=True) and the differentiable STFT
    loss.  The loss falls, by at least 0.8 of what torch's float32 CPU autograd achieves from the same start (rounding makes Adam
    trajectories drift apart; the noise gradient's own fit ended within 1.2 % of torch's)."""
    nws = _nws()
    teacher, student, emb, u = _fit_problem()
    embd, ud = dev(emb), dev(u)
    syn = nws.FIRNoiseSynth(256, 128).cuda()
    syn.differentiable = True
    with torch.no_grad():
        target = syn(_module(FIT_SIZES, teacher)(embd), noise=ud)[:, 0]
    mlp = _module(FIT_SIZES, student, differentiable=True)
    loss_fn = nws.MultiResolutionSTFTLoss(differentiable=True)
    opt = torch.optim.Adam(mlp.parameters(), lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = loss_fn(syn(mlp(embd), noise=ud)[:, 0], target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    ref = _torch_trajectory()
    print(f"Adam, {FIT_STEPS} steps at lr {FIT_LR} on 14 tensors, ({FIT_B}, {FIT_T}): kernels {losses[0]:.4f} -> {losses[-1]:.4f}; "
          f"torch float32 CPU autograd {ref[0]:.4f} -> {ref[-1]:.4f}")
    print("kernels:", " ".join(f"{v:.4f}" for v in losses))
    print("torch:  ", " ".join(f"{v:.4f}" for v in ref))
    record("td_mlp_grad/adam_30_steps", first=losses[0], last=losses[-1], torch_first=ref[0], torch_last=ref[-1],
           kernels=" ".join(f"{v:.5f}" for v in losses), torch=" ".join(f"{v:.5f}" for v in ref))
    assert all(p.grad is not None for p in mlp.parameters())
    assert ref[-1] < ref[0]
    assert losses[-1] < losses[0]
    assert losses[0] - losses[-1] >= 0.8 * (ref[0] - ref[-1])


# ---- the script ---------------------------------------------------------------------------------------------------------------------
FIT_SCRIPT_STEPS, FIT_SCRIPT_LR, FIT_SCRIPT_PERTURB = 5, "3e-4", 0.2


@pytest.mark.parametrize("with_reverb", (False, True))
def test_fit_noise_script_fits_the_whole_h_generator(tmp_path, with_reverb):
    """scripts/fit_noise.py --h-generator all as a child process on four T = 16 items rendered by the same checkpoint with the
    weight of h_generator's second hidden layer (net.3) perturbed by 0.2 normal: 5 steps at lr 3e-4.  The CPU restatement of the
    same objective (oracle.newt_oracle for the frozen part on these controls, torch's float32 autograd through the reference MLP
    and noise expressions, the reverb and torch.stft, host draws) falls at every step there: 2.596, 2.446, 2.301, 2.173, 2.060
    (lr 1e-4: 2.596 -> 2.397; 1e-3: 2.596 -> 1.501; a perturbation of 0.05 starts at 0.259, where Adam's first steps at 3e-4 and
    1e-3 overshoot in the restatement too: 0.296 and 0.618).  Exit code 0, the last printed loss below the first,
    and the written checkpoint loads and differs from the input in exactly the 14 h_generator.* keys (and reverb.ir with the
    flag)."""
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
    with torch.no_grad():
        w = model.h_generator.net[3].weight
        w.add_(FIT_SCRIPT_PERTURB * torch.randn(w.shape, generator=torch.Generator().manual_seed(4)).cuda())
    f0 = (control[:, 0:1].astype(np.float64) * std[0] + mean[0]).astype(np.float32)
    torch.cuda.manual_seed(0)
    audio = model(torch.from_numpy(f0).cuda(), torch.from_numpy(control).cuda()).cpu().numpy()
    for k, name in enumerate(names):
        np.save(root / "train" / "control" / f"control_{name}.npy", control[k])
        np.save(root / "train" / "audio" / f"audio_{name}.npy", audio[k])
    out = tmp_path / "fitted.npz"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fit_noise.py"), "--model-checkpoint", ckpt, "--dataset-root", str(root),
           "--split", "train", "--steps", str(FIT_SCRIPT_STEPS), "--lr", FIT_SCRIPT_LR, "--output", str(out), "--use-fastnewt", "--seed", "0",
           "--h-generator", "all"]
    if with_reverb:
        cmd += ["--with-reverb", "--reverb-lr", "1e-4"]
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    losses = [float(v) for v in re.findall(r"step \d+: loss ([0-9.]+)", run.stdout)]
    print(run.stdout)
    assert len(losses) == FIT_SCRIPT_STEPS and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    record("td_mlp_grad/fit_noise_script_all" + ("_with_reverb" if with_reverb else ""), first=losses[0], last=losses[-1])
    before, after = np.load(ckpt), np.load(out)
    changed = {k for k in before.files if k.startswith("h_generator.")} | ({"reverb.ir"} if with_reverb else set())
    assert len(changed) == 14 + int(with_reverb)
    assert set(before.files) == set(after.files)
    for k in before.files:
        assert (k in changed) != np.array_equal(before[k], after[k]), k
        assert before[k].shape == after[k].shape and before[k].dtype == after[k].dtype, k
    fitted = _nws().NeuralWaveshaping.load_from_checkpoint(str(out))
    for k, p in fitted.h_generator.state_dict().items():
        assert np.array_equal(p.numpy(), after["h_generator." + k]), k
