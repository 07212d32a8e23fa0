"""-m gpu: models with another waveshaper bank train end to end: the oscillator branch's backward at any bank size
(csrc/g_newt_grad.hip) under NeuralWaveshaping.differentiable, nws.optim.Adam and scripts/train.py.  Every other link takes its sizes
at run time already; the hop (128), the noise filter (256 / 128) and the GRU (2 -> 128) are the packaged ones.

T = 16 items in batches of 2.  The gin bindings that choose the sizes are set by each test and put back."""
import contextlib
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from conftest import ROOT
from gpu_util import dev, record

pytestmark = pytest.mark.gpu

CKPT = os.path.join(ROOT, "tests", "golden", "weights_vn.npz")
TRAIN_GIN = os.path.join(ROOT, "neural-waveshaping-synthesis_amd", "gin", "train", "train_newt.gin")
T = 16
MEAN, STD = np.array([[300.0], [0.5]]), np.array([[80.0], [0.2]])
# (a), (c): 12 shapers of width 16 and depth 3 - the reference class's width and depth - on 40 harmonics
OTHER_BANK = {"NeuralWaveshaping.n_waveshapers": 12, "NEWT.n_waveshapers": 12, "NEWT.shaping_fn_size": 16, "TrainableNonlinearity.depth": 3,
              "HarmonicOscillator.n_harmonics": 40}
LR, CLIP, STEPS = 1e-4, 2.0, 5


def _nws():
    import nws_amd as nws

    return nws


@contextlib.contextmanager
def bindings(values):
    """the packaged configuration with these bindings changed; put back afterwards"""
    nws = _nws()
    nws.ensure_default_config()
    gin = nws.gin
    before = {k: gin.query_parameter(k) for k in values}
    try:
        for k, v in values.items():
            gin.bind_parameter(k, v)
        yield
    finally:
        for k, v in before.items():
            gin.bind_parameter(k, v)


def _controls(n, seed):
    control = np.random.default_rng(seed).standard_normal((n, 2, T)).astype(np.float32)
    f0 = (control[:, 0:1].astype(np.float64) * STD[0] + MEAN[0]).astype(np.float32)
    return f0, control


def _render(model, f0, control):
    torch.cuda.manual_seed(0)
    with torch.no_grad():
        return model(dev(f0), dev(control)).cpu().numpy()


def _packaged():
    nws = _nws()
    nws.ensure_default_config()
    return nws.NeuralWaveshaping.load_from_checkpoint(CKPT).cuda().eval()


# ---- (a) gradients arrive ---------------------------------------------------------------------------------------------------------------
def test_every_parameter_gets_a_gradient():
    nws = _nws()
    f0, control = _controls(2, 3)
    batch = {"audio": dev(_render(_packaged(), f0, control)), "f0": dev(f0), "control": dev(control)}

    def make():
        torch.manual_seed(0)
        return nws.NeuralWaveshaping().cuda()

    def step():
        model = make()
        model.differentiable = True
        torch.cuda.manual_seed(0)
        loss = model.training_step(batch, 0)
        loss.backward()
        return model, loss.detach()

    with bindings(OTHER_BANK):
        model, loss = step()
        sh = model.newt.shaping_fn
        assert (model.newt.n_waveshapers, sh.width, sh.depth, model.osc.n_harmonics) == (12, 16, 3, 40)
        assert model.harmonic_mixer.weight.shape == (12, 40, 1) and not model._engine.specialised()
        assert loss.shape == () and bool(torch.isfinite(loss))
        named = dict(model.named_parameters())
        assert len(named) == 46                                      # the packaged 48 less one hidden layer of the shapers
        for k, p in named.items():
            assert p.grad is not None and p.grad.shape == p.shape and bool(torch.isfinite(p.grad).all()), k
        again, loss2 = step()
        assert torch.equal(loss, loss2)
        for k, p in again.named_parameters():
            assert torch.equal(p.grad, named[k].grad), k
        # under no_grad the flag changes nothing: the flag-less model's forward, to the bit
        plain = make()
        torch.cuda.manual_seed(1)
        got = model.validation_step(batch, 0)
        torch.cuda.manual_seed(1)
        want = plain.validation_step(batch, 0)
        assert torch.equal(got, want) and not got.requires_grad
        record("training_sizes/gradients_arrive", loss=float(loss), val_loss=float(got))


# ---- (b) it optimises ---------------------------------------------------------------------------------------------------------------------
N_CUT = 24
CUT_BANK = {"NeuralWaveshaping.n_waveshapers": N_CUT, "NEWT.n_waveshapers": N_CUT}


def _cut_state():
    """the packaged weights cut to their first 24 shapers: harmonic_mixer's rows, the four FiLM groups of newt.mlp's last layer, the
    shapers' and the output mixer's slices - a trained-like model that is not the packaged size set"""
    from nws_amd.checkpoint import read_checkpoint

    S, W, n = 64, 8, N_CUT
    state = {k: np.asarray(v) for k, v in read_checkpoint(CKPT)[0].items()}
    groups = np.concatenate([np.arange(r * S, r * S + n) for r in range(4)])
    for k in ("harmonic_mixer.weight", "harmonic_mixer.bias", "newt.shaping_fn.net.6.weight", "newt.shaping_fn.net.6.bias"):
        state[k] = state[k][:n]
    for k in ("newt.mlp.net.9.weight", "newt.mlp.net.9.bias"):
        state[k] = state[k][groups]
    for k in ("newt.shaping_fn.net.0.weight", "newt.shaping_fn.net.0.bias", "newt.shaping_fn.net.2.weight", "newt.shaping_fn.net.2.bias",
              "newt.shaping_fn.net.4.weight", "newt.shaping_fn.net.4.bias"):
        state[k] = state[k][:n * W]
    for k in ("newt.shaping_fn.input_scale", "newt.mixer.0.weight"):
        state[k] = state[k][:, :n]
    return {k: torch.as_tensor(np.ascontiguousarray(v)) for k, v in state.items()}


def test_it_optimises():
    """five steps at lr 1e-4 with the total gradient norm clipped to 2, the same seed at every step (the pattern and the bar of
    test_gpu_training.py): ours against clip_grad_norm_ + torch.optim.Adam on the same HIP gradients, from the teacher with the
    shapers' third layer perturbed by 0.2 normal, towards the teacher's own render"""
    nws = _nws()
    f0, control = _controls(2, 3)

    def make():
        model = nws.NeuralWaveshaping()
        model.load_state_dict(_cut_state())
        return model.cuda()

    with bindings(CUT_BANK):
        teacher = make().eval()
        sh = teacher.newt.shaping_fn
        assert (teacher.newt.n_waveshapers, sh.width, sh.depth) == (N_CUT, 8, 4) and not teacher.newt._specialised(128)
        batch = {"audio": dev(_render(teacher, f0, control)), "f0": dev(f0), "control": dev(control)}

        def run(ours):
            model = make()
            with torch.no_grad():
                w = model.newt.shaping_fn.net[4].weight
                w.add_(0.2 * torch.randn(w.shape, generator=torch.Generator().manual_seed(4)).cuda())
            model.differentiable = True
            params = list(model.parameters())
            opt = nws.optim.Adam(params, lr=LR, max_grad_norm=CLIP) if ours else torch.optim.Adam(params, lr=LR)
            losses = []
            for _ in range(STEPS):
                torch.cuda.manual_seed(0)
                loss = model.training_step(batch, 0)
                loss.backward()
                if not ours:
                    torch.nn.utils.clip_grad_norm_(params, CLIP, 2.0)
                opt.step()
                opt.zero_grad(set_to_none=True)
                losses.append(loss.detach())
            return [float(v) for v in losses]

        mine, ref = run(True), run(False)
    print("nws.optim.Adam:                    ", " ".join(f"{v:.5f}" for v in mine))
    print("clip_grad_norm_ + torch.optim.Adam:", " ".join(f"{v:.5f}" for v in ref))
    record("training_sizes/adam_5_steps", ours=" ".join(f"{v:.6f}" for v in mine), torch=" ".join(f"{v:.6f}" for v in ref))
    assert mine[0] == ref[0]
    assert mine[-1] < mine[0]
    assert mine[0] - mine[-1] >= 0.8 * (ref[0] - ref[-1])


# ---- (c) the script ---------------------------------------------------------------------------------------------------------------------------
def test_train_script_on_another_bank(tmp_path):
    """scripts/train.py as one fresh child process on a gin file that includes the packaged training file and rebinds the bank: four
    steps from initialisation, and the checkpoint it writes loads into a model of the gin file's shapes that renders"""
    nws = _nws()
    root = tmp_path / "data"
    for sub in ("control", "audio"):
        os.makedirs(root / "train" / sub)
    np.save(root / "data_mean.npy", MEAN)
    np.save(root / "data_std.npy", STD)
    f0, control = _controls(4, 3)
    audio = _render(_packaged(), f0, control)
    for k, name in enumerate(("a", "b", "c", "d")):
        np.save(root / "train" / "control" / f"control_{name}.npy", control[k])
        np.save(root / "train" / "audio" / f"audio_{name}.npy", audio[k])
    gin_file = tmp_path / "other_bank.gin"
    gin_file.write_text(f"include '{TRAIN_GIN}'\n" + "".join(f"{k} = {v}\n" for k, v in OTHER_BANK.items()))
    out = tmp_path / "run"
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--gin-file", str(gin_file), "--dataset-path", str(root),
           "--output-dir", str(out), "--batch-size", "2", "--max-steps", "4", "--seed", "0"]
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=str(tmp_path), timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    print(run.stdout)
    losses = [float(v) for v in re.findall(r"step \d+: train loss ([0-9.eE+-]+|nan|inf)", run.stdout)]
    record("training_sizes/train_script", losses=" ".join(f"{v:.5f}" for v in losses))
    assert len(losses) == 4 and all(np.isfinite(losses)), run.stdout
    with bindings(OTHER_BANK):
        model = nws.NeuralWaveshaping.load_from_checkpoint(str(out / "last.ckpt")).cuda().eval()
        sh = model.newt.shaping_fn
        assert (model.newt.n_waveshapers, sh.width, sh.depth, model.osc.n_harmonics) == (12, 16, 3, 40)
        assert model.newt.shaping_fn.net[2].weight.shape == (12 * 16, 16, 1) and model.harmonic_mixer.weight.shape == (12, 40, 1)
        saved = torch.load(str(out / "last.ckpt"), map_location="cpu", weights_only=False)
        assert saved["global_step"] == 4
        assert set(k for k, _ in model.named_parameters()) <= set(saved["state_dict"])
        for k, v in model.state_dict().items():
            if k in saved["state_dict"]:
                assert torch.equal(v.cpu(), torch.as_tensor(saved["state_dict"][k])), k
        y = _render(model, f0[:2], control[:2])
        assert y.shape == (2, T * 128) and np.isfinite(y).all() and np.abs(y).max() > 0
