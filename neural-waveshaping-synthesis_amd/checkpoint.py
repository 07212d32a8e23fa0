"""Checkpoint front end.

Reads either
  * a PyTorch-Lightning ``.ckpt`` as shipped by the reference (checkpoints/nws/*/last.ckpt: torch
    zip-pickle with ``state_dict`` and ``hyper_parameters``; the pickle references one
    pytorch_lightning class, resolved here with a throw-away stand-in so Lightning is not needed), or
  * a flat ``.npz`` of state-dict arrays (tests/golden/weights_vn.npz).
and the ``data_mean.npy`` / ``data_std.npy`` normalisation statistics next to it; ``write_checkpoint`` writes a checkpoint
back with named tensors replaced (scripts/fit_reverb.py, scripts/fit_noise.py).
"""
import contextlib
import os
import sys
import types

import numpy as np
import torch

_HPARAM_KEYS = ("n_waveshapers", "control_hop", "sample_rate", "learning_rate", "lr_decay", "lr_decay_interval",
                "log_audio")


@contextlib.contextmanager
def _lightning_standin():
    names = ["pytorch_lightning", "pytorch_lightning.callbacks", "pytorch_lightning.callbacks.model_checkpoint"]
    added = []
    for n in names:
        if n not in sys.modules:
            sys.modules[n] = types.ModuleType(n)
            added.append(n)
    mc = sys.modules[names[2]]
    if not hasattr(mc, "ModelCheckpoint"):
        mc.ModelCheckpoint = type("ModelCheckpoint", (), {})
    try:
        yield
    finally:
        for n in added:
            sys.modules.pop(n, None)


def read_checkpoint(path):
    """-> (state_dict as {key: tensor/array}, hyper-parameters dict)."""
    if str(path).endswith(".npz"):
        z = np.load(path)
        state = {k: z[k] for k in z.files if not k.startswith("__")}
        if "__hparams__" in z.files:        # fixtures of non-default gin configurations carry their constructor arguments
            import json

            return state, {k: v for k, v in json.loads(str(z["__hparams__"])).items() if k in _HPARAM_KEYS}
        return state, dict(n_waveshapers=64, control_hop=128, sample_rate=16000)
    with _lightning_standin():
        ck = torch.load(path, map_location="cpu", weights_only=False)
    hp = {k: v for k, v in dict(ck.get("hyper_parameters", {})).items() if k in _HPARAM_KEYS}
    return dict(ck["state_dict"]), hp


def write_checkpoint(path, source, replace):
    """Write the checkpoint `source` to `path` with the tensors named in `replace` ({state-dict key: tensor}) replaced, each
    cast to the dtype it has in the source: as .npz (every array of the source is kept, the `__`-prefixed ones too) or, for any
    other suffix, as a torch checkpoint with `state_dict` and `hyper_parameters`."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    replace = {k: v.detach().cpu() for k, v in replace.items()}
    if str(path).endswith(".npz"):
        if str(source).endswith(".npz"):
            z = np.load(source)
            arrays = {k: z[k] for k in z.files}
        else:
            arrays = {k: np.asarray(v) for k, v in read_checkpoint(source)[0].items()}
        for k, v in replace.items():
            arrays[k] = v.numpy().astype(arrays[k].dtype)
        np.savez(path, **arrays)
        return
    state, hparams = read_checkpoint(source)
    state = {k: torch.as_tensor(v) for k, v in state.items()}
    for k, v in replace.items():
        state[k] = v.to(state[k].dtype)
    torch.save({"state_dict": state, "hyper_parameters": hparams}, path)


def _to_cpu(obj):
    """tensors of a nested state dict as compact CPU tensors (a view into a flat state buffer is saved as its own elements)"""
    if isinstance(obj, torch.Tensor):
        return obj.detach().cpu().clone()
    if isinstance(obj, dict):
        return {k: _to_cpu(v) for k, v in obj.items()}
    if isinstance(obj, (list, tuple)):
        return type(obj)(_to_cpu(v) for v in obj)
    return obj


def write_training_checkpoint(path, model, optimizer, scheduler, global_step, epoch, extra=None):
    """A torch checkpoint with Lightning's keys, everything on the CPU: `state_dict`, `hyper_parameters`, `optimizer_states`
    ([optimizer.state_dict()], torch.optim.Adam's layout), `lr_schedulers` ([scheduler.state_dict()]), `global_step`, `epoch`, and
    the entries of `extra`.  `read_checkpoint` / `load_from_checkpoint` read the first two, `read_training_state` the others."""
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    ck = dict(extra or {})
    ck.update({"state_dict": _to_cpu(dict(model.state_dict())),
               "hyper_parameters": {k: v for k, v in dict(model.hparams).items() if k in _HPARAM_KEYS},
               "optimizer_states": [_to_cpu(optimizer.state_dict())], "lr_schedulers": [_to_cpu(scheduler.state_dict())],
               "global_step": int(global_step), "epoch": int(epoch)})
    torch.save(ck, path)


def read_training_state(path):
    """-> (optimizer state dict, scheduler state dict, global_step, epoch) of a checkpoint, None for each one the file lacks: an
    `.npz` lacks all four, a checkpoint with `optimizer_states: []` (as written without a trainer's state) the first."""
    if str(path).endswith(".npz"):
        return None, None, None, None
    with _lightning_standin():
        ck = torch.load(path, map_location="cpu", weights_only=False)
    first = lambda key: (ck.get(key) or [None])[0]
    number = lambda key: int(ck[key]) if ck.get(key) is not None else None
    return first("optimizer_states"), first("lr_schedulers"), number("global_step"), number("epoch")


_LIGHTNING_KEYS = ("state_dict", "hyper_parameters", "optimizer_states", "lr_schedulers", "global_step", "epoch", "callbacks",
                   "pytorch-lightning_version")


def read_training_extra(path):
    """the `extra` entries of `write_training_checkpoint` (every top-level key that is not one of Lightning's); {} for an `.npz`"""
    if str(path).endswith(".npz"):
        return {}
    with _lightning_standin():
        ck = torch.load(path, map_location="cpu", weights_only=False)
    return {k: v for k, v in ck.items() if k not in _LIGHTNING_KEYS}


def load_normalisation(checkpoint_dir):
    """data_mean / data_std rows 0 (f0) and 1 (loudness) as float64 (reference: colab cell 6, 15)."""
    mean = np.load(os.path.join(checkpoint_dir, "data_mean.npy")).astype(np.float64).reshape(-1)
    std = np.load(os.path.join(checkpoint_dir, "data_std.npy")).astype(np.float64).reshape(-1)
    return mean, std


def make_control(f0_hz, loudness, mean, std):
    """control = stack((f0 - mean0)/std0, (loudness - mean1)/std1); F0 itself stays in Hz."""
    f0_hz = np.asarray(f0_hz, dtype=np.float64)
    loudness = np.asarray(loudness, dtype=np.float64)
    c = np.stack([(f0_hz - mean[0]) / std[0], (loudness - mean[1]) / std[1]], axis=-2)
    return torch.as_tensor(f0_hz, dtype=torch.float32).unsqueeze(-2), torch.as_tensor(c, dtype=torch.float32)
