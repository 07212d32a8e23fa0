import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden")

# The pipeline's five streams need hardware queues of their own (pipeline.placed_streams: GPU_MAX_HW_QUEUES >= 12); the package
# only sets 16 when the variable is unset, so an environment that presets a smaller count would make the placement tests (and
# the tools they start as subprocesses) run on shared queues.  Set before anything in this process starts the HIP runtime.
if int(os.environ.get("GPU_MAX_HW_QUEUES") or 0) < 12:
    os.environ["GPU_MAX_HW_QUEUES"] = "16"


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a real MI355X (run with `-m gpu` on the GPU box)")


def pytest_collection_modifyitems(config, items):
    """`gpu`-marked tests need the MI355X: without one they are skipped (not failed with hipErrorNoDevice), so a plain
    `pytest tests` works on a CPU-only machine."""
    try:
        import torch
        have = torch.cuda.is_available()
    except Exception:
        have = False
    if have:
        return
    skip = pytest.mark.skip(reason="needs a real MI355X (torch.cuda.is_available() is False)")
    for item in items:
        if "gpu" in item.keywords:
            item.add_marker(skip)


def load_npz(name):
    z = np.load(os.path.join(GOLDEN, name))
    return {k: z[k] for k in z.files}


@pytest.fixture(scope="session")
def weights():
    w = load_npz("weights_vn.npz")
    return {k: v for k, v in w.items() if not k.startswith("__")}


@pytest.fixture(scope="session")
def g1():
    return load_npz("g1_realistic.npz")


LIGHTNING_MODULES = ["pytorch_lightning", "pytorch_lightning.callbacks", "pytorch_lightning.callbacks.model_checkpoint"]


def write_lightning_ckpt(path, weights):
    """A pytorch-lightning 1.2.8 style `.ckpt` of `weights`: a torch zip-pickle with `state_dict`, `hyper_parameters` and a
    `callbacks` dict keyed by the ModelCheckpoint CLASS - the one global of the pickle that needs Lightning.  A throw-away
    stand-in class is registered while pickling and removed again, so that loading the file needs the front end's stand-in."""
    import types

    import torch

    assert not any(n in sys.modules for n in LIGHTNING_MODULES)          # no Lightning in the test environment
    mods = {n: types.ModuleType(n) for n in LIGHTNING_MODULES}
    ModelCheckpoint = type("ModelCheckpoint", (), {"__module__": LIGHTNING_MODULES[2]})
    mods[LIGHTNING_MODULES[2]].ModelCheckpoint = ModelCheckpoint
    sys.modules.update(mods)
    try:
        torch.save({"epoch": 3, "global_step": 120000, "pytorch-lightning_version": "1.2.8",
                    "callbacks": {ModelCheckpoint: {"best_model_score": torch.tensor(1.0), "best_model_path": "x.ckpt"}},
                    "optimizer_states": [], "lr_schedulers": [],
                    "state_dict": {k: torch.as_tensor(v) for k, v in weights.items()},
                    "hyper_parameters": {"n_waveshapers": 64, "control_hop": 128, "sample_rate": 16000, "learning_rate": 1e-3,
                                         "lr_decay": 0.9, "lr_decay_interval": 10000, "log_audio": False}}, path)
    finally:
        for n in LIGHTNING_MODULES:
            sys.modules.pop(n, None)


def rms(a):
    a = np.asarray(a, dtype=np.float64)
    return float(np.sqrt(np.mean(a * a)))
