"""No GPU: the optimiser step's restatement against torch in float64, the optimiser's state-dict exchange with torch.optim.Adam, the
C ABI's refusals, the training hooks behind NeuralWaveshaping.differentiable, the training checkpoint, scripts/train.py's command
line and the packaged training gin."""
import copy
import importlib
import importlib.util
import inspect
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import adam_step_restatement as ar
from conftest import GOLDEN, ROOT, write_lightning_ckpt

PKG = "neural-waveshaping-synthesis_amd"
nws = importlib.import_module(PKG)
_lib = importlib.import_module(PKG + "._lib")
ckpt = importlib.import_module(PKG + ".checkpoint")
BAD_ARG = -2


@pytest.mark.parametrize("max_norm", (ar.MAX_NORM, math.inf), ids=("clipped", "unclipped"))
@pytest.mark.parametrize("case", ar.CASES)
def test_restatement_is_clip_grad_norm_and_adam_in_float64(case, max_norm):
    """1e-9 relative L2, the bar of the other restatements: three steps under StepLR(2, 0.5), every tensor's p, m and v and the
    total norm; with max_norm 2 the first and third steps clip, the second does not"""
    want = ar.torch_trajectory(case, torch.float64, max_norm)
    got = ar.trajectory(case, max_norm, np.float64)
    assert len(want) == len(got) == ar.STEPS
    clipped = []
    for (_, (wp, wm, wv, wt)), (gp, gm, gv, gt) in zip(want, got):
        assert abs(float(gt) - wt) <= 1e-12 * wt
        clipped.append(wt > max_norm)
        for k in range(len(wp)):
            assert ar.rel_l2(gp[k], wp[k]) <= 1e-9 and ar.rel_l2(gm[k], wm[k]) <= 1e-9 and ar.rel_l2(gv[k], wv[k]) <= 1e-9, k
    assert clipped == ([True, False, True] if max_norm == ar.MAX_NORM else [False] * 3)


def test_restatement_constants_are_the_kernels():
    assert (ar.C, ar.THREADS, ar.TABLE) == (_lib.ADAM_CHUNK, _lib.ADAM_THREADS, _lib.ADAM_TABLE)
    header = open(os.path.join(ROOT, "include", "nws_hip.h")).read()
    assert f"#define NWS_ADAM_CHUNK {ar.C} " in header and f"#define NWS_ADAM_TABLE {ar.TABLE} " in header
    assert "#define NWS_ABI_VERSION 6" in header                  # symbols were added, nothing changed
    spec = importlib.util.spec_from_file_location("nws_build", os.path.join(ROOT, PKG, "build.py"))
    build = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(build)
    assert "adam_step.hip" in build.SOURCES and "-fno-slp-vectorize" in build.EXTRA_FLAGS["adam_step.hip"]
    source = open(os.path.join(ROOT, PKG, "csrc", "adam_step.hip")).read()
    assert "atomic" not in source.replace("no atomics", "")


def test_no_clipping_is_exactly_one():
    for dt in (np.float32, np.float64):
        assert ar.clip_coefficient(dt(3.0), math.inf, dt) == 1.0 and ar.clip_coefficient(dt(3.0), 1e30, dt) == 1.0
        assert ar.clip_coefficient(dt(0.0), 2.0, dt) == 1.0 and ar.clip_coefficient(dt(4.0), 2.0, dt) < 0.5
        assert np.isnan(ar.clip_coefficient(dt(np.nan), 2.0, dt))


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------------
def _records(ns, null=None):
    recs = (_lib.NwsAdamTensor * max(1, len(ns)))()
    for k, n in enumerate(ns):
        fields = dict(param=0x1000, grad=0x2000, exp_avg=0x3000, exp_avg_sq=0x4000)
        if null is not None and null[0] == k:
            fields[null[1]] = None
        recs[k] = _lib.NwsAdamTensor(fields["param"], fields["grad"], fields["exp_avg"], fields["exp_avg_sq"], n)
    return recs


def test_bad_arguments_return_codes_without_touching_the_gpu():
    """every refusal is decided on the host, before the first launch: the pointers here are never dereferenced"""
    L = _lib.lib()
    ok = _records([5, ar.C + 1])
    assert L.nws_adam_workspace_bytes(ok, 2) == 8 * 3                      # one double per chunk: 1 + 2
    assert L.nws_adam_workspace_bytes(_records([ar.C] * 65 + [2 * ar.C + 1]), 66) == 8 * 68
    assert L.nws_adam_workspace_bytes(ok, 0) == 0 and L.nws_adam_workspace_bytes(None, 2) == 0
    assert L.nws_adam_workspace_bytes(_records([5, 0]), 2) == 0
    args = (1, 1e-3, 0.9, 0.999, 1e-8, 2.0, 0x5000, 0x6000, 24, None)      # step .. stream
    call = lambda recs, n, *a: L.nws_adam_step(recs, n, *a)
    assert call(ok, 0, *args) == BAD_ARG and call(ok, -1, *args) == BAD_ARG and call(None, 2, *args) == BAD_ARG
    for field in ("param", "grad", "exp_avg", "exp_avg_sq"):
        assert call(_records([5, ar.C + 1], null=(1, field)), 2, *args) == BAD_ARG, field
    assert call(_records([5, 0]), 2, *args) == BAD_ARG and call(_records([-3, 4]), 2, *args) == BAD_ARG
    assert call(ok, 2, 0, *args[1:]) == BAD_ARG and call(ok, 2, -1, *args[1:]) == BAD_ARG                  # step < 1
    assert call(ok, 2, *args[:6], None, *args[7:]) == BAD_ARG                                             # no total
    assert call(ok, 2, *args[:7], None, 24, None) == BAD_ARG                                              # no workspace
    assert call(ok, 2, *args[:7], 0x6000, 23, None) == BAD_ARG and call(ok, 2, *args[:7], 0x6000, 0, None) == BAD_ARG
    assert call(ok, 2, *args[:7], 0x6004, 24, None) == BAD_ARG                                            # not 8-byte aligned
    assert call(_records([(1 << 40) + 1]), 1, *args) == -1                                                # beyond the kernels' range
    for name in ("nws_adam_workspace_bytes", "nws_adam_step"):
        assert name in _lib.EXPORTED_SYMBOLS
    assert L.nws_abi_version() == 6


# ---- the optimiser ------------------------------------------------------------------------------------------------------------------
def _leaves(dtype=torch.float32):
    g = torch.Generator().manual_seed(5)
    ps = [torch.nn.Parameter(torch.randn(s, generator=g, dtype=dtype)) for s in ((3, 2), (5,), (1,))]
    for p in ps:
        p.grad = torch.randn(p.shape, generator=g, dtype=dtype)
    return ps


def test_optimizer_surface_and_no_cpu_fallback():
    assert nws.optim.Adam is importlib.import_module(PKG + ".optim").Adam and issubclass(nws.optim.Adam, torch.optim.Optimizer)
    sig = inspect.signature(nws.optim.Adam.__init__)
    assert [(n, p.default) for n, p in list(sig.parameters.items())[2:]] == [("lr", 1e-3), ("betas", (0.9, 0.999)), ("eps", 1e-8),
                                                                               ("max_grad_norm", None)]
    assert "not rewritten" in " ".join(nws.optim.Adam.__doc__.split()).lower()
    ps = _leaves()
    opt = nws.optim.Adam(ps, lr=1e-2, max_grad_norm=2.0)
    before = [p.detach().clone() for p in ps]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        opt.step()
    assert all(torch.equal(a, p) for a, p in zip(before, ps)) and opt.state_dict()["state"] == {} and opt.last_grad_norm is None
    # nothing to do without gradients
    for p in ps:
        p.grad = None
    assert opt.step() is None
    # groups that differ are refused
    ps = _leaves()
    opt = nws.optim.Adam([{"params": ps[:1]}, {"params": ps[1:], "lr": 1e-4}], lr=1e-3)
    with pytest.raises(RuntimeError, match="different lr, betas or eps"):
        opt.step()
    for bad in (dict(lr=-1.0), dict(eps=-1.0), dict(betas=(1.0, 0.9)), dict(max_grad_norm=0.0)):
        with pytest.raises(ValueError):
            nws.optim.Adam(_leaves(), **bad)


@pytest.mark.parametrize("step_as", ("int", "tensor"))
def test_state_dict_moves_to_torch_adam_and_back(step_as):
    """torch.optim.Adam's layout, state[i] = {step, exp_avg, exp_avg_sq}: from torch into ours with step as an int (the reference's
    shipped checkpoints) or a tensor, and from ours into torch, which then steps as if the state had been its own"""
    ps = _leaves()
    theirs = torch.optim.Adam(ps, lr=3e-3, betas=(0.8, 0.95), eps=1e-7)
    theirs.step()
    theirs.step()
    sd = copy.deepcopy(theirs.state_dict())                    # state_dict() hands out the optimiser's own dicts and tensors
    assert set(sd["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    for s in sd["state"].values():
        s["step"] = int(s["step"]) if step_as == "int" else torch.tensor(float(s["step"]))
    ours = nws.optim.Adam(_leaves(), lr=1e-3)
    ours.load_state_dict(sd)
    g = ours.param_groups[0]
    assert (g["lr"], tuple(g["betas"]), g["eps"]) == (3e-3, (0.8, 0.95), 1e-7) and ours._hyper_parameters() == (3e-3, 0.8, 0.95, 1e-7)
    for p, q in zip(ours.param_groups[0]["params"], ps):
        assert int(ours.state[p]["step"]) == 2
        assert torch.equal(ours.state[p]["exp_avg"], theirs.state[q]["exp_avg"])
        assert torch.equal(ours.state[p]["exp_avg_sq"], theirs.state[q]["exp_avg_sq"])
    back = ours.state_dict()
    assert set(back) == {"state", "param_groups"} and set(back["state"]) == {0, 1, 2}
    assert set(back["state"][0]) == {"step", "exp_avg", "exp_avg_sq"}
    # ... and into torch: the continued run equals the uninterrupted one to the bit
    qs = _leaves()
    with torch.no_grad():
        for q, p in zip(qs, ps):
            q.copy_(p)
    again = torch.optim.Adam(qs, lr=1e-3)
    again.load_state_dict(back)
    theirs.step()
    again.step()
    assert all(torch.equal(p, q) for p, q in zip(ps, qs))
    # a scheduler drives lr through param_groups
    sched = torch.optim.lr_scheduler.StepLR(ours, 1, 0.5)
    lr0 = ours._hyper_parameters()[0]
    for p in ours.param_groups[0]["params"]:
        p.grad = None
    ours.step()
    sched.step()
    assert ours._hyper_parameters()[0] == 0.5 * lr0


# ---- the hooks ----------------------------------------------------------------------------------------------------------------------
SUB_FLAGS = ("embedding", "harmonic_mixer", "newt", "h_generator", "noise_synth", "reverb")


def _flags(model):
    return [getattr(model, n).differentiable for n in SUB_FLAGS] + [model.stft_loss.differentiable]


def test_hooks_are_behind_the_flag():
    nws.ensure_default_config()
    model = nws.NeuralWaveshaping(learning_rate=2e-3, lr_decay=0.7, lr_decay_interval=123)
    assert nws.NeuralWaveshaping.differentiable is False and "differentiable" not in model.__dict__       # the class default
    assert model.differentiable is False and _flags(model) == [False] * 7
    for call in (lambda: model.training_step({}, 0), model.configure_optimizers):
        with pytest.raises(NotImplementedError, match="no backward pass in this package") as e:
            call()
        assert "NeuralWaveshaping.differentiable" in str(e.value)
    model.differentiable = True
    assert model.differentiable is True and _flags(model) == [True] * 7
    conf = model.configure_optimizers()
    assert set(conf) == {"optimizer", "lr_scheduler"} and set(conf["lr_scheduler"]) == {"scheduler", "interval"}
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    assert type(opt) is nws.optim.Adam and opt.param_groups[0]["lr"] == 2e-3 and opt.max_grad_norm is None
    assert [id(p) for p in opt.param_groups[0]["params"]] == [id(p) for p in model.parameters()] and len(opt.param_groups) == 1
    assert isinstance(sched, torch.optim.lr_scheduler.StepLR) and sched.optimizer is opt
    assert (sched.step_size, sched.gamma, conf["lr_scheduler"]["interval"]) == (123, 0.7, "step")
    # on the CPU the flagged forward still refuses: no CPU fallback, flag or not
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        model.training_step({"audio": torch.zeros(1, 256), "f0": torch.full((1, 1, 2), 200.0), "control": torch.zeros(1, 2, 2)}, 0)
    model.differentiable = False
    assert model.differentiable is False and _flags(model) == [False] * 7
    with pytest.raises(NotImplementedError):
        model.configure_optimizers()
    # an object from before the flag existed (the lookup table's refusal needs a GPU: tests/test_gpu_training.py)
    model.__dict__.pop("differentiable")
    assert model.differentiable is False


# ---- checkpoints --------------------------------------------------------------------------------------------------------------------
def test_training_checkpoint_round_trip(tmp_path, weights):
    nws.ensure_default_config()
    model = nws.NeuralWaveshaping()
    model.differentiable = True
    conf = model.configure_optimizers()
    opt, sched = conf["optimizer"], conf["lr_scheduler"]["scheduler"]
    for k, p in enumerate(model.parameters()):                # state as a step would leave it
        opt.state[p] = {"step": torch.tensor(7.0), "exp_avg": torch.full_like(p, 0.5 + k), "exp_avg_sq": torch.full_like(p, 0.25)}
    sched.last_epoch = 7
    path = tmp_path / "run" / "last.ckpt"
    ckpt.write_training_checkpoint(str(path), model, opt, sched, 7, 2, extra={"best_val_loss": 0.5})
    raw = torch.load(str(path), weights_only=False)
    assert {"state_dict", "hyper_parameters", "optimizer_states", "lr_schedulers", "global_step", "epoch", "best_val_loss"} == set(raw)
    o, s, step, epoch = ckpt.read_training_state(str(path))
    assert (step, epoch) == (7, 2) and s["last_epoch"] == 7 and s["step_size"] == model.lr_decay_interval
    assert ckpt.read_training_extra(str(path)) == {"best_val_loss": 0.5}
    assert len(o["state"]) == 48 and int(o["state"][3]["step"]) == 7 and float(o["state"][3]["exp_avg"].flatten()[0]) == 3.5
    theirs = torch.optim.Adam(nws.NeuralWaveshaping().parameters())
    theirs.load_state_dict(o)                                 # torch.optim.Adam's layout
    state, hp = ckpt.read_checkpoint(str(path))               # and the model half reads as before
    assert hp == {k: v for k, v in model.hparams.items()} and set(state) == set(model.state_dict())
    again = nws.NeuralWaveshaping.load_from_checkpoint(str(path))
    assert all(torch.equal(a, b) for a, b in zip(again.state_dict().values(), model.state_dict().values()))
    # files without a trainer's state
    plain = tmp_path / "plain.ckpt"
    write_lightning_ckpt(str(plain), weights)                 # optimizer_states: [], lr_schedulers: []
    assert ckpt.read_training_state(str(plain)) == (None, None, 120000, 3) and ckpt.read_training_extra(str(plain)) == {}
    assert ckpt.read_training_state(os.path.join(GOLDEN, "weights_vn.npz")) == (None, None, None, None)
    assert ckpt.read_training_extra(os.path.join(GOLDEN, "weights_vn.npz")) == {}


# ---- the script and its gin file -------------------------------------------------------------------------------------------------------
def test_train_script_help_and_refusals(tmp_path):
    script = os.path.join(ROOT, "scripts", "train.py")
    run = subprocess.run([sys.executable, script, "--help"], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stderr
    for option in ("--gin-file", "--dataset-path", "--urmp", "--instrument", "--device", "--restore-checkpoint", "--load-data-to-memory",
                   "--with-wandb", "--output-dir", "--max-steps", "--batch-size", "--seed", "--val-every-epochs"):
        assert option in run.stdout, option
    run = subprocess.run([sys.executable, script, "--gin-file", "x.gin", "--dataset-path", str(tmp_path), "--with-wandb"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode != 0 and "no wandb" in run.stderr


def test_packaged_train_gin_parses():
    gin = nws.gin
    path = os.path.join(ROOT, PKG, "gin", "train", "train_newt.gin")
    gin.clear_config()
    try:
        gin.parse_config_file(path)
        assert gin.query_parameter("trainer_kwargs.gradient_clip_val") == 2.0
        assert gin.query_parameter("trainer_kwargs.max_steps") == 120000
        assert gin.query_parameter("GeneralDataModule.batch_size") == 8 and gin.query_parameter("URMPDataModule.batch_size") == 8
        assert gin.query_parameter("NeuralWaveshaping.learning_rate") == 1e-3
        assert gin.query_parameter("NeuralWaveshaping.lr_decay") == 0.9 and gin.query_parameter("NeuralWaveshaping.lr_decay_interval") == 10000
        assert gin.query_parameter("NeuralWaveshaping.control_hop") == 128           # the include of the model gin
        model = nws.NeuralWaveshaping()
        assert (model.learning_rate, model.lr_decay, model.lr_decay_interval) == (1e-3, 0.9, 10000)
        with pytest.raises(ValueError):
            gin.query_parameter("trainer_kwargs.accelerator")
    finally:
        gin.clear_config()
        nws.ensure_default_config()
