"""Control-feature dataset reader for batched offline rendering.

Directory layout written by the reference's preprocessing (data/utils/create_dataset.py, read by
data/general.py:9-57):  <root>/data_mean.npy, <root>/data_std.npy  (C,1) statistics, and per split
<root>/<split>/control/control_<name>.npy  (C,T) NORMALISED controls, optionally
<root>/<split>/audio/audio_<name>.npy target audio.  As in the reference's GeneralDataset.__getitem__,
F0 in Hz is recovered by de-normalising row 0; the model gets F0 in Hz and the normalised controls.
"""
from __future__ import annotations

import os
from collections import defaultdict

import numpy as np


class ControlDataset:
    def __init__(self, root: str, split: str = "test"):
        self.root, self.split = root, split
        self.control_dir = os.path.join(root, split, "control")
        self.audio_dir = os.path.join(root, split, "audio")
        if not os.path.isdir(self.control_dir):
            raise FileNotFoundError(f"no control features under {self.control_dir}")
        self.names = sorted(f[len("control_"):-4] for f in os.listdir(self.control_dir)
                            if f.startswith("control_") and f.endswith(".npy"))
        self.mean = np.load(os.path.join(root, "data_mean.npy")).astype(np.float64)
        self.std = np.load(os.path.join(root, "data_std.npy")).astype(np.float64)

    def __len__(self):
        return len(self.names)

    def item(self, name: str):
        control = np.load(os.path.join(self.control_dir, f"control_{name}.npy"))
        denorm = control.astype(np.float64) * self.std + self.mean      # general.py:49
        out = {"name": name, "control": control.astype(np.float32), "f0": denorm[0:1].astype(np.float32)}
        ap = os.path.join(self.audio_dir, f"audio_{name}.npy")
        if os.path.exists(ap):
            out["audio"] = np.load(ap).astype(np.float32)
        return out

    def shard(self, rank: int, world: int):
        """Round-robin split of the (sorted) item list: independent objects, no collective needed."""
        return self.names[rank::world]

    def groups(self, names, batch_size: int):
        """The names of every batch `batches` yields, without loading the items (`group_names` over the items' frame counts)."""
        frames = {n: np.load(os.path.join(self.control_dir, f"control_{n}.npy"), mmap_mode="r").shape[-1] for n in names}
        return group_names(names, frames, batch_size)

    def collate(self, names):
        """One batch of the named items (of equal frame count)."""
        items = [self.item(n) for n in names]
        return {"names": [it["name"] for it in items],
                "f0": np.stack([it["f0"] for it in items]),
                "control": np.stack([it["control"] for it in items]),
                "audio": [it.get("audio") for it in items]}

    def batches(self, names, batch_size: int):
        """Group items of equal frame count (forward needs a rectangular batch), keep file order inside a group."""
        for group in self.groups(names, batch_size):
            yield self.collate(group)


def group_names(names, frames, batch_size: int):
    """`names` grouped by frame count (`frames[name]`, ascending), the given order kept inside a group, in runs of at most
    `batch_size`: the batches of `ControlDataset.batches` as lists of names."""
    by_len = defaultdict(list)
    for n in names:
        by_len[frames[n]].append(n)
    return [by_len[T][i:i + batch_size] for T in sorted(by_len) for i in range(0, len(by_len[T]), batch_size)]


def rank_batches(groups, world: int, rank: int):
    """Data-parallel training (scripts/train.py --gpus N): `groups` are the global batches, `group_names(order, frames, W b)`.
    Rank `rank` takes the items `shard_bounds(n, world, rank)` of a global batch of n items; a global batch with n < world is left
    out on every rank, so every rank takes the same number of steps and none gets an empty batch.
    -> (this rank's batches as lists of names, the number of global batches left out); world = 1 gives `groups` back."""
    from .parallel import shard_bounds

    kept = [g for g in groups if len(g) >= world]
    mine = []
    for g in kept:
        lo, hi = shard_bounds(len(g), world, rank)
        mine.append(list(g[lo:hi]))
    return mine, len(groups) - len(kept)
