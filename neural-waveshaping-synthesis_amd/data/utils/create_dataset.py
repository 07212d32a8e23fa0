"""A folder of recordings -> a dataset in the layout `dataset.ControlDataset` and scripts/resynthesise_dataset.py read
(mirror of neural_waveshaping_synthesis/data/utils/create_dataset.py:13-166):

    <root>/data_mean.npy, <root>/data_std.npy                  (C, 1) statistics of the control rows
    <root>/<split>/audio/audio_<file>_<j>.npy                  segment j of <file>.wav, divided by the largest sample of all
    <root>/<split>/control/control_<file>_<j>.npy              (3 + n_mfcc, T) float64, normalised: f0, loudness, confidence, MFCC

Segments are staged under <root>/temp/ until the statistics of all of them are known.  The split draws a permutation from
numpy's global generator (seed it for a reproducible split); it is not scikit-learn's train_test_split, which the reference
uses and this package does not depend on, so the same seed gives another assignment than the reference's.
"""
from __future__ import annotations

import os
import shutil
from typing import Sequence

import numpy as np

from ... import ginlite as gin
from .preprocess_audio import preprocess_audio


def create_directories(target_root: str, names: Sequence[str]):
    for name in names:
        os.makedirs(os.path.join(target_root, name), exist_ok=True)


def _split_sizes(n: int, proportions: Sequence[float]):
    """floor(p n) for the first split, the rest shared out among the others in the same way"""
    if len(proportions) == 1:
        return [n]
    first = int(np.floor(n * (proportions[0] / float(np.sum(proportions))) + 1e-9))
    return [first] + _split_sizes(n - first, proportions[1:])


def make_splits(audio_list: Sequence[str], control_list: Sequence[str], splits: Sequence[str], split_proportions: Sequence[float]):
    """:31-70.  {split: {"audio": [...], "control": [...]}}: a random assignment of the (audio, control) pairs, split i
    getting its share of what the splits in front of it left"""
    if len(splits) != len(split_proportions) or len(splits) < 1:
        raise ValueError("splits and split_proportions must have the same length, at least 1")
    if len(audio_list) != len(control_list):
        raise ValueError("audio_list and control_list must pair up")
    n = len(audio_list)
    sizes = _split_sizes(n, list(split_proportions))
    if min(sizes) < 1:
        raise ValueError(f"{n} segments cannot fill the splits {tuple(splits)} in the proportions {tuple(split_proportions)}: "
                         f"they would hold {tuple(sizes)}")
    order = np.random.permutation(n)
    out, at = {}, 0
    for split, size in zip(splits, sizes):
        chosen = order[at:at + size]
        out[split] = {"audio": [audio_list[i] for i in chosen], "control": [control_list[i] for i in chosen]}
        at += size
    return out


def control_statistics(means, stds, lengths):
    """:124-129.  Per-segment means / standard deviations (C,) and lengths -> data_mean, data_std (C, 1): the mean of the
    means, and the root of the length-weighted mean of the variances"""
    means, stds = np.stack(means, axis=-1), np.stack(stds, axis=-1)
    lengths = np.asarray(lengths, dtype=np.float64)[None, :]
    data_mean = means.mean(axis=-1)[:, None]
    data_std = np.sqrt((lengths * stds ** 2).sum(axis=-1) / lengths.sum())[:, None]
    return data_mean, data_std


def lazy_create_dataset(files: Sequence[str], output_directory: str, splits: Sequence[str], split_proportions: Sequence[float]):
    """:73-148.  Needs the directories create_dataset makes.  Nothing is written outside temp/ before the split is known to
    work: too few segments for the splits raise with the output directory holding no statistics and no segment."""
    staged = []                                   # (audio file, control file, per-row mean, per-row std, frames) of every segment
    audio_max = 1e-5
    temp = os.path.join(output_directory, "temp")
    for file, segments in zip(files, preprocess_audio(files)):
        name = os.path.split(file)[-1].replace(".wav", "")
        for j, (audio, f0, confidence, loudness, mfcc) in enumerate(zip(*segments)):
            audio_max = max(audio_max, float(np.abs(audio).max()))
            control = np.concatenate((np.stack((f0, loudness, confidence), axis=0), mfcc), axis=0).astype(np.float64)
            entry = (f"audio_{name}_{j}.npy", f"control_{name}_{j}.npy", control.mean(axis=-1), control.std(axis=-1), control.shape[-1])
            np.save(os.path.join(temp, "audio", entry[0]), audio)
            np.save(os.path.join(temp, "control", entry[1]), control)
            staged.append(entry)
    if not staged:
        print("no segment passed the confidence threshold: nothing to split")
        return
    audio_files, control_files, means, stds, lengths = zip(*staged)
    assignment = make_splits(audio_files, control_files, splits, split_proportions)         # raises before anything is written
    data_mean, data_std = control_statistics(means, stds, lengths)
    np.save(os.path.join(output_directory, "data_mean.npy"), data_mean)
    np.save(os.path.join(output_directory, "data_std.npy"), data_std)
    for split, lists in assignment.items():
        for f in lists["audio"]:
            np.save(os.path.join(output_directory, split, "audio", f), np.load(os.path.join(temp, "audio", f)) / audio_max)
        for f in lists["control"]:
            control = np.load(os.path.join(temp, "control", f))
            np.save(os.path.join(output_directory, split, "control", f), (control - data_mean) / data_std)
        print(f"{split}: {len(lists['audio'])} segments")


@gin.configurable
def create_dataset(files: Sequence[str], output_directory: str, splits: Sequence[str] = ("train", "val", "test"),
                   split_proportions: Sequence[float] = (0.8, 0.1, 0.1), lazy: bool = True):
    """:151-166.  Only the lazy form exists (segments staged on disk one file at a time), as in the reference; lazy=False,
    which the reference accepts and then does nothing for, is refused."""
    if not lazy:
        raise NotImplementedError("create_dataset: only lazy=True is implemented (the reference has no other form either)")
    folders = [os.path.join(output_directory, part) for part in (*splits, "temp")]
    for folder in folders:
        create_directories(folder, ("audio", "control"))
    try:
        lazy_create_dataset(files, output_directory, splits, split_proportions)
    finally:
        shutil.rmtree(folders[-1])
