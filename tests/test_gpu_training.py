"""-m gpu: the training loop closed: the two Lightning hooks behind NeuralWaveshaping.differentiable, nws.optim.Adam
under them with no stale derived tables in the fused forward, five optimiser steps against clip_grad_norm_ + torch.optim.Adam on the
same HIP gradients, and scripts/train.py as a child process with a resumed run equal to the uninterrupted one to the bit.

Data, the recipe of test_gpu_newt_grad._dataset: four T = 16 train items rendered by the packaged checkpoint with the shapers' third
layer (newt.shaping_fn.net.4.weight) perturbed by 0.2 normal - targets the packaged checkpoint is near but not at - and two val
items made the same way."""
import importlib.util
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_step_restatement as ar
from conftest import ROOT
from gpu_util import build_model, dev, record

pytestmark = pytest.mark.gpu

CKPT = os.path.join(ROOT, "tests", "golden", "weights_vn.npz")
TRAIN_GIN = os.path.join(ROOT, "neural-waveshaping-synthesis_amd", "gin", "train", "train_newt.gin")
LR, CLIP, STEPS = 1e-4, 2.0, 5


def _nws():
    import nws_amd as nws

    return nws


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    """(root, {split: (f0, control, audio)})"""
    T = 16
    root = tmp_path_factory.mktemp("training") / "data"
    os.makedirs(root)
    mean, std = np.array([[300.0], [0.5]]), np.array([[80.0], [0.2]])
    np.save(root / "data_mean.npy", mean)
    np.save(root / "data_std.npy", std)
    model = build_model(fast=False)
    with torch.no_grad():
        w = model.newt.shaping_fn.net[4].weight
        w.add_(0.2 * torch.randn(w.shape, generator=torch.Generator().manual_seed(4)).cuda())
    splits = {}
    for split, names, seed in (("train", ("a", "b", "c", "d"), 3), ("val", ("e", "f"), 5)):
        for sub in ("control", "audio"):
            os.makedirs(root / split / sub)
        control = np.random.default_rng(seed).standard_normal((len(names), 2, T)).astype(np.float32)
        f0 = (control[:, 0:1].astype(np.float64) * std[0] + mean[0]).astype(np.float32)
        torch.cuda.manual_seed(0)
        audio = model(torch.from_numpy(f0).cuda(), torch.from_numpy(control).cuda()).cpu().numpy()
        for k, name in enumerate(names):
            np.save(root / split / "control" / f"control_{name}.npy", control[k])
            np.save(root / split / "audio" / f"audio_{name}.npy", audio[k])
        splits[split] = (f0, control, audio)
    return root, splits


def _batch(splits, split="train"):
    f0, control, audio = splits[split]
    return {"audio": dev(audio), "f0": dev(f0), "control": dev(control)}


def _flagged():
    model = build_model(fast=False)
    model.differentiable = True
    return model


# ---- the hooks ------------------------------------------------------------------------------------------------------------------------
def test_hooks(data):
    nws = _nws()
    _, splits = data
    batch = _batch(splits)
    plain = build_model(fast=False)
    for call in (lambda: plain.training_step(batch, 0), plain.configure_optimizers):
        with pytest.raises(NotImplementedError, match="no backward pass in this package"):
            call()
    model = _flagged()
    assert all(p.requires_grad for p in model.parameters()) and len(list(model.parameters())) == 48
    torch.cuda.manual_seed(0)
    loss = model.training_step(batch, 0)
    assert loss.requires_grad and loss.shape == ()
    loss.backward()
    # scripts/fit_newt.py's `model` composition under the same seed
    spec = importlib.util.spec_from_file_location("fit_newt_script", os.path.join(ROOT, "scripts", "fit_newt.py"))
    fit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fit)
    twin = build_model(fast=False)
    fitted = fit.fitted_parameters(twin, "model")
    loss_fn = nws.MultiResolutionSTFTLoss(differentiable=True)
    torch.cuda.manual_seed(0)
    want = loss_fn(twin.reverb(fit.pre_reverb(twin, batch["f0"], batch["control"], "model")), batch["audio"])
    want.backward()
    named = dict(model.named_parameters())
    assert set(named) == set(fitted)
    worst, same = 0.0, torch.equal(loss.detach(), want.detach())
    for k, p in fitted.items():
        assert named[k].grad is not None, k
        worst = max(worst, ar.rel_l2(named[k].grad.cpu().numpy(), p.grad.cpu().numpy()))
        same = same and torch.equal(named[k].grad, p.grad)
    print(f"training_step against fit_newt's composition: bit-equal {same}, worst relative L2 {worst:.2e}")
    record("training/hooks", bit_equal=float(same), worst_rel_l2=worst)
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-6 * abs(float(want.detach())) and worst <= 1e-6
    # under no_grad the flag changes nothing: the fused forward's bits
    torch.cuda.manual_seed(1)
    got = model.validation_step(batch, 0)
    torch.cuda.manual_seed(1)
    assert torch.equal(got, plain.validation_step(batch, 0)) and not got.requires_grad
    # the lookup table keeps refusing, and nothing is half set
    fast = build_model(fast=True)
    with pytest.raises(RuntimeError, match="lookup table has no backward"):
        fast.differentiable = True
    assert fast.differentiable is False and not any(getattr(fast, n).differentiable for n in fast._TRAINED)


def test_no_stale_tables_after_a_step(data):
    """the optimiser writes through raw pointers; everything derived from the weights (the engine's pointer struct and tables, the
    modules' descriptors, the reverb spectrum, the folded frame-MLP tables) keys on Tensor._version, which the op raises"""
    nws = _nws()
    _, splits = data
    batch, val = _batch(splits), _batch(splits, "val")
    model = _flagged()
    opt = nws.optim.Adam(model.parameters(), lr=1e-3, max_grad_norm=CLIP)
    torch.cuda.manual_seed(0)
    before = model.validation_step(val, 0)                     # the fused path has built and cached its tables
    torch.cuda.manual_seed(0)
    model.training_step(batch, 0).backward()
    start = {k: v.clone() for k, v in model.state_dict().items()}
    opt.step()
    opt.zero_grad(set_to_none=True)
    params = set(k for k, _ in model.named_parameters())
    assert all(torch.equal(start[k], v) != (k in params) for k, v in model.state_dict().items())       # every parameter moved
    fresh = build_model(fast=False)
    fresh.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    fresh.differentiable = True
    torch.cuda.manual_seed(0)
    got = model.validation_step(val, 0)
    torch.cuda.manual_seed(0)
    want = fresh.validation_step(val, 0)
    assert torch.equal(got, want) and not torch.equal(got, before)
    torch.cuda.manual_seed(0)
    got = model.training_step(batch, 0)
    torch.cuda.manual_seed(0)
    want = fresh.training_step(batch, 0)
    assert torch.equal(got.detach(), want.detach())


def test_it_optimises(data):
    """five steps at lr 1e-4 (at the hparams' 1e-3 the first step overshoots from the trained checkpoint) with the
    total gradient norm clipped to 2: ours against clip_grad_norm_ + torch.optim.Adam on the same HIP gradients, same start, same
    seed at every step.  The trajectories drift with rounding, so the bar is the project's: at least 0.8 of torch's decrease."""
    nws = _nws()
    _, splits = data
    batch = _batch(splits)

    def run(ours):
        model = _flagged()
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
    record("training/adam_5_steps", ours=" ".join(f"{v:.6f}" for v in mine), torch=" ".join(f"{v:.6f}" for v in ref))
    assert mine[0] == ref[0]
    assert mine[-1] < mine[0]
    assert mine[0] - mine[-1] >= 0.8 * (ref[0] - ref[-1])


# ---- the script ---------------------------------------------------------------------------------------------------------------------------
def _train(root, out, steps, restore, cwd):
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "train.py"), "--gin-file", TRAIN_GIN, "--dataset-path", str(root), "--output-dir",
           str(out), "--batch-size", "2", "--max-steps", str(steps), "--seed", "0", "--restore-checkpoint", str(restore)]
    run = subprocess.run(cmd, capture_output=True, text=True, cwd=str(cwd), timeout=300)
    assert run.returncode == 0, run.stdout + run.stderr
    return run.stdout


def _load(path):
    return torch.load(str(path), map_location="cpu", weights_only=False)


def test_train_script_and_resume(data, tmp_path):
    nws = _nws()
    root, _ = data
    out = tmp_path / "six"
    stdout = _train(root, out, 6, CKPT, tmp_path)
    print(stdout)
    losses = [float(v) for v in re.findall(r"step \d+: train loss ([0-9.eE+-]+|nan|inf)", stdout)]
    record("training/train_script", losses=" ".join(f"{v:.5f}" for v in losses))
    assert len(losses) == 6 and all(np.isfinite(losses)), stdout
    assert len(re.findall(r"^epoch \d+: step \d+  train loss \S+  grad norm \S+  lr \S+  val loss [0-9.]+", stdout, re.M)) == 3
    assert "carries no optimiser state" in stdout             # an .npz starts fresh optimiser state from its weights
    for name in ("data_mean.npy", "data_std.npy"):
        assert np.array_equal(np.load(out / name), np.load(root / name))
    start = np.load(CKPT)
    params = set(k for k, _ in build_model(fast=False).named_parameters())
    for name in ("last.ckpt", "best.ckpt"):
        model = nws.NeuralWaveshaping.load_from_checkpoint(str(out / name))
        state = model.state_dict()
        assert params <= set(state) and len(params) == 48
        if name == "last.ckpt":
            for k, v in state.items():
                assert np.array_equal(v.numpy(), start[k]) != (k in params), k                   # all 48 moved, nothing else did
    six = _load(out / "last.ckpt")
    assert six["global_step"] == 6 and six["lr_schedulers"][0]["last_epoch"] == 6 and len(six["optimizer_states"][0]["state"]) == 48
    # three steps, then the rest from its last.ckpt: the same bits
    stdout = _train(root, tmp_path / "three", 3, CKPT, tmp_path)
    assert _load(tmp_path / "three" / "last.ckpt")["global_step"] == 3
    stdout = _train(root, tmp_path / "resumed", 6, tmp_path / "three" / "last.ckpt", tmp_path)
    assert "resuming" in stdout and [float(v) for v in re.findall(r"step \d+: train loss ([0-9.]+)", stdout)] == losses[3:]
    res = _load(tmp_path / "resumed" / "last.ckpt")
    assert res["global_step"] == 6 and res["lr_schedulers"][0]["last_epoch"] == 6 and res["epoch"] == six["epoch"]
    assert set(res["state_dict"]) == set(six["state_dict"])
    for k, v in six["state_dict"].items():
        assert torch.equal(v, res["state_dict"][k]), k
    a, b = six["optimizer_states"][0], res["optimizer_states"][0]
    assert a["param_groups"] == b["param_groups"] and set(a["state"]) == set(b["state"])
    for i, s in a["state"].items():
        assert int(s["step"]) == int(b["state"][i]["step"]) == 6
        assert torch.equal(s["exp_avg"], b["state"][i]["exp_avg"]) and torch.equal(s["exp_avg_sq"], b["state"][i]["exp_avg_sq"]), i
