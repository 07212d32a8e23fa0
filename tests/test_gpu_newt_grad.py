"""-m gpu: the backward of the oscillator branch (csrc/newt_grad.hip through the op, NEWT.vjp, NEWT.differentiable, Conv1x1.vjp and
scripts/fit_newt.py) against the float64 restatement of its definition (tests/newt_grad_restatement.py).

Input sets: 'packaged' = newt.* of tests/golden/weights_vn.npz under the oracle's exciter and embedding of smooth controls;
'default' = the modules' own initialisation under normal inputs.  Shapes (B, T): (1, 1) the minimum, both lerp edges in one hop;
(1, 2) one interior boundary; (3, 3) an odd batch, an interior frame between the clamped edges; (2, 33) several partials; (1, 17)
34 blocks of 64 samples - a workgroup covers 32, blocks come two to a frame, so this is the first shape past one workgroup; (2, 65)
260 blocks, nine partial rows - the segment sum's second trip of p += 8, a count that is no multiple of eight.

Bar, for every returned tensor: the relative L2 from float64 is at most 10 x the distance of torch's float32 CPU autograd from the
same restatement on the same inputs (the yardstick is computed in the test and floored at 2^-24, one float32 rounding), and never
beyond the project's parity bar, 1e-4 (FACTOR, CAP of test_gpu_control_gru_grad.py).  The kernel's FiLM parameters come from the
forward MLP kernel's own float32 film; that is part of what is measured.

The measured figures (kernel | torch float32 CPU autograd | ratio per case) are in DESIGN.md 3.18."""
import copy
import ctypes as C
import functools
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import newt_grad_restatement as nr
from conftest import ROOT
from gpu_util import build_model, dev, record

pytestmark = pytest.mark.gpu

FACTOR = 10.0
CAP = 1e-4
BAD_ARG = -2


def _nws():
    import nws_amd as nws

    return nws


def _binding():
    from nws_amd.engine import binding

    return binding()


@functools.lru_cache(maxsize=None)
def _module(which):
    """a NEWT with the parameters of a set on the device"""
    nws = _nws()
    nws.ensure_default_config()
    from nws_amd.models.modules.shaping import NEWT

    m = NEWT()
    m.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in nr.params(which).items()})
    return m.cuda()


def _op(which, exc, film, g, want_exciter=True, want_params=True):
    with torch.no_grad():
        return list(_binding().newt_grad(_module(which)._wdesc(), exc, film, g, want_exciter, want_params))


def _check(tag, names, got, want, yard):
    dists = {}
    for name, o in zip(names, got):
        w = want[name]
        assert tuple(o.shape) == w.shape and o.dtype == torch.float32 and o.is_cuda and not o.requires_grad, name
        dists[name] = nr.rel_l2(o.cpu().numpy(), w)
        print(f"{tag} {name}: kernel {dists[name]:.2e} | torch float32 autograd {yard[name]:.2e} | ratio {dists[name] / yard[name]:.2f}")
    worst = max(names, key=lambda n: dists[n] / yard[n])
    record(f"newt_grad/{tag}", worst=worst, worst_kernel=dists[worst], worst_torch_f32=yard[worst], worst_ratio=dists[worst] / yard[worst],
           **{n: d for n, d in dists.items()}, **{n + "_torch_f32": yard[n] for n in names})
    return dists


@pytest.mark.parametrize("which,shape", nr.CASES, ids=nr.IDS)
def test_every_gradient_against_the_restatement(which, shape):
    B, T = shape
    exciter, emb, g = nr.inputs(which, B, T)
    want, yard = nr.reference(which, B, T)
    m = _module(which)
    ed, cd, gd = dev(exciter), dev(emb), dev(g)
    with torch.no_grad():
        film = m.mlp(cd)
    out = _op(which, ed, film, gd)
    assert len(out) == len(nr.OP_NAMES) == 13
    d_op = _check(f"op_{which}_{B}x{T}", nr.OP_NAMES, out, want, yard)
    ge, gemb, grads = m.vjp(gd, ed, cd)
    assert set(grads) == set(nr.PARAM_KEYS) == set(k for k, _ in m.named_parameters())
    names = ("exciter", "emb") + nr.PARAM_KEYS
    d_vjp = _check(f"vjp_{which}_{B}x{T}", names, [ge, gemb] + [grads[k] for k in nr.PARAM_KEYS], want, yard)
    assert torch.equal(ge, out[1]) and all(torch.equal(grads[k], o) for k, o in zip(nr.RATE_KEYS, out[2:]))

    # exact cases: equal inputs, equal bits; fewer outputs leave the others' bits alone; no gradient in, none out
    again = _op(which, ed, film, gd)
    assert all(torch.equal(a, o) for a, o in zip(again, out))
    only = _op(which, ed, film, gd, want_exciter=True, want_params=False)
    assert len(only) == 2 and torch.equal(only[0], out[0]) and torch.equal(only[1], out[1])
    only = _op(which, ed, film, gd, want_exciter=False, want_params=True)
    assert len(only) == 12 and torch.equal(only[0], out[0]) and all(torch.equal(a, o) for a, o in zip(only[1:], out[2:]))
    only = _op(which, ed, film, gd, want_exciter=False, want_params=False)
    assert len(only) == 1 and torch.equal(only[0], out[0])
    for we, wp in ((True, True), (False, False)):
        for o in _op(which, ed, film, torch.zeros_like(gd), we, wp):
            assert torch.equal(o, torch.zeros_like(o))
    ge0, gemb0, none = m.vjp(gd, ed, cd, want_params=False, want_exciter=False)
    assert ge0 is None and none == {} and torch.equal(gemb0, gemb)

    for dists, names_ in ((d_op, nr.OP_NAMES), (d_vjp, names)):
        for name in names_:
            assert dists[name] <= FACTOR * yard[name] and dists[name] <= CAP, (name, dists[name], yard[name])


def test_conv1x1_vjp_is_the_convolutions_gradient():
    """harmonic_mixer, Conv1d(101 -> 64, 1) at N = 128 x 3 through the existing td_mlp_grad op"""
    from nws_amd.models.modules.dynamic import Conv1x1

    x, g, W, b = nr.conv_case()
    want, yard = nr.conv_reference()
    conv = Conv1x1(nr.K, nr.S, 1)
    conv.load_state_dict({"weight": torch.as_tensor(W), "bias": torch.as_tensor(b)})
    conv = conv.cuda()
    xd, gd = dev(x), dev(g)
    gx, grads = conv.vjp(gd, xd)
    assert list(grads) == ["weight", "bias"]
    d = _check("conv1x1_vjp_2x384", ("x", "weight", "bias"), [gx, grads["weight"].view(nr.S, nr.K, 1), grads["bias"]], want, yard)
    gx0, none = conv.vjp(gd, xd, want_params=False)
    assert none == {} and torch.equal(gx0, gx)
    # autograd: the same bits, the plain forward's bits, and only what requires grad
    with torch.no_grad():
        y0 = conv(xd)
    with pytest.raises(RuntimeError, match="inference-only"):
        conv(xd.clone().requires_grad_())
    flagged = copy.deepcopy(conv)
    flagged.differentiable = True
    leaf = xd.clone().requires_grad_()
    y = flagged(leaf)
    assert y.requires_grad and torch.equal(y.detach(), y0)
    (y * gd).sum().backward()
    assert torch.equal(leaf.grad, gx) and torch.equal(flagged.weight.grad, grads["weight"].view_as(flagged.weight))
    assert torch.equal(flagged.bias.grad, grads["bias"])
    flagged.weight.requires_grad_(False)
    flagged.weight.grad = flagged.bias.grad = None
    (flagged(xd) * gd).sum().backward()
    assert flagged.weight.grad is None and torch.equal(flagged.bias.grad, grads["bias"])
    for name in ("x", "weight", "bias"):
        assert d[name] <= FACTOR * yard[name] and d[name] <= CAP, (name, d[name], yard[name])


# ---- refusals: decided on the host, before any launch -------------------------------------------------------------------------------
def _raw(which, exc, film, g, null=(), ws_short=False, drop_param=None):
    """nws_newt_grad through ctypes: (return code, every output tensor filled with NaN beforehand, the workspace)"""
    from nws_amd import _lib

    B, _, N = exc.shape
    T = film.shape[2]
    P = nr.params(which)
    nan = lambda *s: torch.full(s, float("nan"), device="cuda")
    outs = [nan(B, nr.FILM, T), nan(B, nr.S, N)] + [nan(*P[k].shape) for k in nr.RATE_KEYS]
    L = _lib.lib()
    nbytes = L.nws_newt_grad_workspace_bytes(B, T, 1)
    assert nbytes > L.nws_newt_grad_workspace_bytes(B, T, 0) > 0
    ws = torch.full((nbytes,), 0x7f, dtype=torch.uint8, device="cuda")
    a = dict(exciter=exc.data_ptr(), film=film.data_ptr(), grad_out=g.data_ptr(), grad_film=outs[0].data_ptr(), ws=ws.data_ptr())
    for k in null:
        a[k] = None
    gp = [o.data_ptr() for o in outs[2:]]
    if drop_param is not None:
        gp[drop_param] = None
    w = _lib.NwsWeights.from_buffer_copy(_module(which)._wdesc().numpy())
    rc = L.nws_newt_grad(C.byref(w), a["exciter"], a["film"], a["grad_out"], B, T, outs[1].data_ptr(), a["grad_film"], *gp, a["ws"],
                         nbytes - 4 if ws_short else nbytes, torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return rc, outs, ws


def test_refusals_return_before_any_launch():
    which, (B, T) = "packaged", (3, 3)
    exciter, emb, g = nr.inputs(which, B, T)
    ed, gd = dev(exciter), dev(g)
    with torch.no_grad():
        film = _module(which).mlp(dev(emb))
    for kw in (dict(null=("exciter",)), dict(null=("film",)), dict(null=("grad_out",)), dict(null=("grad_film",)), dict(null=("ws",)),
               dict(ws_short=True), dict(drop_param=3), dict(drop_param=10)):
        rc, outs, ws = _raw(which, ed, film, gd, **kw)
        assert rc == BAD_ARG, (kw, rc)
        assert all(torch.isnan(o).all() for o in outs), kw                   # untouched
        assert bool((ws == 0x7f).all()), kw
    rc, outs, _ = _raw(which, ed, film, gd)                                   # and a valid call right after gives the op's bits
    assert rc == 0
    assert all(torch.equal(a, o) for a, o in zip(outs, _op(which, ed, film, gd)))


# ---- autograd -----------------------------------------------------------------------------------------------------------------------
def test_autograd_carries_the_bits_of_vjp():
    which, (B, T) = "packaged", (3, 3)
    plain = _module(which)
    mod = copy.deepcopy(plain)
    mod.differentiable = True
    exciter, emb, g = nr.inputs(which, B, T)
    ed, cd, gd = dev(exciter), dev(emb), dev(g)
    with torch.no_grad():
        want_y = plain(ed, cd)
    want_e, want_c, want = plain.vjp(gd, ed, cd)

    # the flag off: today's forward - no graph, and an input that requires grad is refused
    assert plain.differentiable is False and not plain(ed, cd).requires_grad
    for args in ((ed.clone().requires_grad_(), cd), (ed, cd.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="inference-only"):
            plain(*args)

    e_leaf, c_leaf = ed.clone().requires_grad_(), cd.clone().requires_grad_()
    y = mod(e_leaf, c_leaf)
    assert y.requires_grad and torch.equal(y.detach(), want_y)
    (y * gd).sum().backward()
    assert torch.equal(e_leaf.grad, want_e) and torch.equal(c_leaf.grad, want_c)
    named = dict(mod.named_parameters())
    assert set(named) == set(want) and len(named) == 25
    for k, p in named.items():
        assert p.grad is not None and p.grad.shape == p.shape and torch.equal(p.grad, want[k].view_as(p)), k

    # no parameter requires grad: the data gradients alone, the same bits; nothing requires grad: the plain forward
    for p in mod.parameters():
        p.requires_grad_(False)
        p.grad = None
    e_leaf.grad = c_leaf.grad = None
    (mod(e_leaf, cd) * gd).sum().backward()
    assert torch.equal(e_leaf.grad, want_e) and c_leaf.grad is None and all(p.grad is None for p in mod.parameters())
    assert not mod(ed, cd).requires_grad and torch.equal(mod(ed, cd), want_y)
    with torch.no_grad():                                                     # vjp does not look at the flag or the grad mode
        assert torch.equal(mod.vjp(gd, ed, cd)[1], want_c) and not mod(e_leaf, cd).requires_grad
    # one parameter alone: the inputs and the others get nothing
    mod.shaping_fn.net[4].weight.requires_grad_(True)
    y = mod(ed, cd)
    assert y.requires_grad
    (y * gd).sum().backward()
    assert torch.equal(mod.shaping_fn.net[4].weight.grad, want["shaping_fn.net.4.weight"])
    assert all(p.grad is None for k, p in mod.named_parameters() if k != "shaping_fn.net.4.weight")
    # hooks on an inner module: the flagged forward refuses, the plain one runs the modules one by one
    h = mod.mixer[0].register_forward_hook(lambda *a: None)
    with pytest.raises(RuntimeError, match="hooks"):
        mod(ed, cd)
    h.remove()
    # the lookup table has no backward
    fast = _nws().FastNEWT(plain)
    with pytest.raises(RuntimeError, match="lookup table has no backward"):
        fast.differentiable = True
    with pytest.raises(RuntimeError, match="lookup table has no backward"):
        fast.vjp(gd, ed, cd)
    assert fast.differentiable is False and fast(ed, cd).shape == want_y.shape


# ---- it optimises -------------------------------------------------------------------------------------------------------------------
FIT_B, FIT_T, FIT_STEPS, FIT_LR, FIT_PERTURB = 2, 24, 30, 1e-3, 0.05
FIT_KEYS = ("shaping_fn.net.4.weight", "shaping_fn.net.4.bias", "shaping_fn.net.6.weight", "shaping_fn.net.6.bias", "mixer.0.weight",
            "mixer.0.bias")


def _fit_problem():
    """teacher = packaged harmonic_mixer and newt; student = the same with shaping_fn.net.4.*, net.6.* and mixer.0.* perturbed by
    0.05 normal; the oscillator bank and the control embedding of the packaged inputs at (2, 24), fixed"""
    z = np.load(nr.GOLDEN)
    teacher = dict(nr.params("packaged"))
    mixer = (z["harmonic_mixer.weight"].astype(np.float32), z["harmonic_mixer.bias"].astype(np.float32))
    rng = np.random.default_rng(41)
    student = dict(teacher)
    for k in FIT_KEYS:
        student[k] = (teacher[k] + FIT_PERTURB * rng.standard_normal(teacher[k].shape)).astype(np.float32)
    _, emb, _ = nr.inputs("packaged", FIT_B, FIT_T)
    return teacher, student, mixer, nr.oscillator_bank(FIT_B, FIT_T), emb


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
    teacher, student, mixer, osc, emb = _fit_problem()
    t = lambda d, grad=False: {k: torch.tensor(np.array(v), requires_grad=grad) for k, v in d.items()}
    osct, embt = torch.tensor(np.array(osc)), torch.tensor(np.array(emb))
    conv = torch.nn.functional.conv1d
    with torch.no_grad():
        target = nr.torch_newt(conv(osct, torch.tensor(mixer[0]), torch.tensor(mixer[1])), embt, t(teacher))[:, 0]
    leaves = t(student, True)
    mw, mb = torch.tensor(mixer[0], requires_grad=True), torch.tensor(mixer[1], requires_grad=True)
    opt = torch.optim.Adam(list(leaves.values()) + [mw, mb], lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = _torch_stft_loss(nr.torch_newt(conv(osct, mw, mb), embt, leaves)[:, 0], target)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    return losses


def test_it_optimises():
    """Adam(lr 1e-3), 30 steps over the 27 tensors of harmonic_mixer and newt, towards the signal the packaged pair makes from
    the same oscillator bank and embedding, through Conv1x1 and NEWT (differentiable=True) and the differentiable STFT loss.  The
    loss falls, by at least 0.8 of what torch's float32 CPU autograd achieves from the same start (rounding makes
    Adam trajectories drift apart)."""
    nws = _nws()
    from nws_amd.models.modules.dynamic import Conv1x1

    teacher, student, mixer, osc, emb = _fit_problem()
    oscd, embd = dev(osc), dev(emb)
    hm = Conv1x1(nr.K, nr.S, 1)
    hm.load_state_dict({"weight": torch.as_tensor(mixer[0]), "bias": torch.as_tensor(mixer[1])})
    hm = hm.cuda()
    newt = copy.deepcopy(_module("packaged"))
    with torch.no_grad():
        target = newt(hm(oscd), embd)[:, 0].contiguous()
    newt.load_state_dict({k: torch.as_tensor(np.array(v)) for k, v in student.items()})
    newt.differentiable = True
    hm.differentiable = True
    params = list(hm.parameters()) + list(newt.parameters())
    assert len(params) == 27
    loss_fn = nws.MultiResolutionSTFTLoss(differentiable=True)
    opt = torch.optim.Adam(params, lr=FIT_LR)
    losses = []
    for _ in range(FIT_STEPS):
        opt.zero_grad()
        loss = loss_fn(newt(hm(oscd), embd)[:, 0].contiguous(), target)
        loss.backward()
        opt.step()
        losses.append(loss.detach())
    losses = [float(v) for v in losses]
    ref = _torch_trajectory()
    print(f"Adam, {FIT_STEPS} steps at lr {FIT_LR} on 27 tensors, ({FIT_B}, {FIT_T}): kernels {losses[0]:.4f} -> {losses[-1]:.4f}; "
          f"torch float32 CPU autograd {ref[0]:.4f} -> {ref[-1]:.4f}")
    print("kernels:", " ".join(f"{v:.4f}" for v in losses))
    print("torch:  ", " ".join(f"{v:.4f}" for v in ref))
    record("newt_grad/adam_30_steps", first=losses[0], last=losses[-1], torch_first=ref[0], torch_last=ref[-1],
           kernels=" ".join(f"{v:.5f}" for v in losses), torch=" ".join(f"{v:.5f}" for v in ref))
    assert all(p.grad is not None for p in params)
    assert ref[-1] < ref[0]
    assert losses[-1] < losses[0]
    assert losses[0] - losses[-1] >= 0.8 * (ref[0] - ref[-1])


# ---- the script ---------------------------------------------------------------------------------------------------------------------
FIT_SCRIPT_STEPS = 5
MODE_KEYS = {"shapers": lambda k: k.startswith("newt.shaping_fn.") or k.startswith("newt.mixer."),
             "branch": lambda k: k.startswith("newt.") or k.startswith("harmonic_mixer."),
             "model": lambda k: True}
MODE_COUNT = {"shapers": 11, "branch": 27, "model": 48}


def _dataset(tmp_path):
    """four T = 16 items rendered by the packaged checkpoint with the shapers' third layer (newt.shaping_fn.net.4) perturbed by
    0.2 normal: targets the packaged checkpoint is near but not at"""
    T, names = 16, ("a", "b", "c", "d")
    root = tmp_path / "data"
    for sub in ("control", "audio"):
        os.makedirs(root / "train" / sub)
    mean, std = np.array([[300.0], [0.5]]), np.array([[80.0], [0.2]])
    np.save(root / "data_mean.npy", mean)
    np.save(root / "data_std.npy", std)
    control = np.random.default_rng(3).standard_normal((len(names), 2, T)).astype(np.float32)
    model = build_model(fast=False)
    with torch.no_grad():
        w = model.newt.shaping_fn.net[4].weight
        w.add_(0.2 * torch.randn(w.shape, generator=torch.Generator().manual_seed(4)).cuda())
    f0 = (control[:, 0:1].astype(np.float64) * std[0] + mean[0]).astype(np.float32)
    torch.cuda.manual_seed(0)
    audio = model(torch.from_numpy(f0).cuda(), torch.from_numpy(control).cuda()).cpu().numpy()
    for k, name in enumerate(names):
        np.save(root / "train" / "control" / f"control_{name}.npy", control[k])
        np.save(root / "train" / "audio" / f"audio_{name}.npy", audio[k])
    return root, f0, control, audio


@pytest.mark.parametrize("mode", ("shapers", "branch", "model"))
def test_fit_newt_script(tmp_path, mode):
    """scripts/fit_newt.py as a child process, 5 steps per mode at lr 1e-4: exit code 0, the last printed loss below the first, and
    the written checkpoint loads and differs from the input in exactly the keys of the mode.  The learning rate: the start is the
    trained checkpoint, one layer away from the target, and Adam's first step moves every element of every tensor by lr whatever
    its gradient - at the hparams' 1e-3 that first step overshoots with 27 and 48 tensors (0.286 -> 0.663 and 1.401, then falling;
    the 11 shaper tensors fall from the first step), at 1e-4 every mode falls at every step (branch 0.2865 -> 0.1761, model
    0.2865 -> 0.1952 on the MI355X)."""
    ckpt = os.path.join(ROOT, "tests", "golden", "weights_vn.npz")
    root, _, _, _ = _dataset(tmp_path)
    out = tmp_path / "fitted.npz"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "fit_newt.py"), "--model-checkpoint", ckpt, "--dataset-root", str(root),
           "--split", "train", "--steps", str(FIT_SCRIPT_STEPS), "--output", str(out), "--seed", "0", "--params", mode, "--lr", "1e-4"]
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    losses = [float(v) for v in re.findall(r"step \d+: loss ([0-9.]+)", run.stdout)]
    print(run.stdout)
    record(f"newt_grad/fit_newt_script_{mode}", first=losses[0], last=losses[-1], losses=" ".join(f"{v:.5f}" for v in losses))
    assert len(losses) == FIT_SCRIPT_STEPS and all(np.isfinite(losses)) and losses[-1] < losses[0], losses
    before, after = np.load(ckpt), np.load(out)
    state = [k for k in before.files if not k.startswith("__")]
    params = set(k for k, _ in build_model(fast=False).named_parameters())
    changed = {k for k in state if k in params and MODE_KEYS[mode](k)}
    assert len(changed) == MODE_COUNT[mode]
    assert set(before.files) == set(after.files)
    for k in before.files:
        assert (k in changed) != np.array_equal(before[k], after[k]), k
        assert before[k].shape == after[k].shape and before[k].dtype == after[k].dtype, k
    fitted = _nws().NeuralWaveshaping.load_from_checkpoint(str(out))
    for k, p in fitted.state_dict().items():
        if k in after.files:
            assert np.array_equal(p.numpy(), after[k]), k


def test_the_whole_model_chain_is_the_links_composed(tmp_path):
    """--params model: after one backward of one batch every parameter's .grad is the chain composed by hand from the links' vjp
    methods - the loss, the reverb, NEWT, Conv1x1, FIRNoiseSynth, h_generator, and ControlModule fed the SUM of the two branches'
    dL/d(emb) - within float32 addition order (1e-6 relative L2).  This checks the plumbing; the numbers are each link's own test."""
    nws = _nws()
    spec = importlib.util.spec_from_file_location("fit_newt_script", os.path.join(ROOT, "scripts", "fit_newt.py"))
    fit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fit)
    _, f0, control, audio = _dataset(tmp_path)
    f0d, cd, ad = dev(f0), dev(control), dev(audio)
    model = build_model(fast=False)
    fitted = fit.fitted_parameters(model, "model")
    assert len(fitted) == 48 and all(p.requires_grad for p in fitted.values())
    loss_fn = nws.MultiResolutionSTFTLoss(differentiable=True)
    torch.cuda.manual_seed(0)
    loss = loss_fn(model.reverb(fit.pre_reverb(model, f0d, cd, "model")), ad)
    loss.backward()
    assert all(p.grad is not None for p in fitted.values())

    from nws_amd.models.modules.dynamic import upsample_linear

    torch.cuda.manual_seed(0)
    with torch.no_grad():
        _, _, phase_u, noise = model._checked_inputs(f0d, cd, None, None)
        sig = model.osc(upsample_linear(f0d, 128)[:, 0], phase_u=phase_u)
        ctl = cd[:, 0:2].contiguous()
        exc = model.harmonic_mixer(sig)
        emb = model.embedding(ctl)
        H = model.h_generator(emb)
        pre = model.newt(exc, emb)[:, 0] + model.noise_synth(H, noise=noise)[:, 0]
        loss2, g_y = loss_fn.loss_and_grad(model.reverb(pre), ad)
        g_pre, g_ir = model.reverb.vjp(pre, g_y)
        g_exc, g_emb_newt, newt_grads = model.newt.vjp(g_pre[:, None, :].contiguous(), exc, emb)
        _, mixer_grads = model.harmonic_mixer.vjp(g_exc, sig)
        g_emb_noise, h_grads = model.h_generator.vjp(model.noise_synth.vjp(g_pre, noise), emb)
        _, enc_grads = model.embedding.vjp(g_emb_newt + g_emb_noise, ctl)
    assert torch.equal(loss2, loss.detach())
    by_hand = {"reverb.ir": g_ir}
    for prefix, grads in (("newt.", newt_grads), ("harmonic_mixer.", mixer_grads), ("h_generator.", h_grads), ("embedding.", enc_grads)):
        by_hand.update({prefix + k: v for k, v in grads.items()})
    assert set(by_hand) == set(fitted)
    worst = 0.0
    for k, p in fitted.items():
        d = nr.rel_l2(p.grad.cpu().numpy(), by_hand[k].reshape(p.shape).cpu().numpy())
        worst = max(worst, d)
        assert d <= 1e-6, (k, d)
    record("newt_grad/model_chain", worst_rel_l2=worst)
