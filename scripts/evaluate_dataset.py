#!/usr/bin/env python
"""Score a checkpoint on a dataset split in the metric the model was trained on: the multi-resolution STFT loss between
the render and the target audio (what the reference logs as test/loss; models/neural_waveshaping.py:152-162 there),
`NeuralWaveshaping.test_step` per batch.  Render and loss both run as HIP kernels; one number per batch is read back.

    python scripts/evaluate_dataset.py --model-checkpoint ckpt --dataset-root data/ [--split test] [--use-fastnewt]

Items without target audio are left out (and counted).  The hidden draws of every forward (phase offsets, noise excitation)
come from the device generator, seeded with --seed: a run repeats to the bit, and two checkpoints or the exact and the
FastNEWT shapers are scored on the same draws.
"""
import importlib
import os
import sys

import click
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@click.command()
@click.option("--model-gin", default=None)
@click.option("--model-checkpoint", required=True)
@click.option("--dataset-root", required=True)
@click.option("--split", default="test")
@click.option("--batch-size", default=64)
@click.option("--use-fastnewt", is_flag=True)
@click.option("--seed", default=0, help="seeds the device generator the hidden draws of forward() come from")
def main(model_gin, model_checkpoint, dataset_root, split, batch_size, use_fastnewt, seed):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    ds_mod = importlib.import_module("neural-waveshaping-synthesis_amd.dataset")
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(dev)
    if model_gin:
        nws.gin.parse_config_file(model_gin)
    else:
        nws.ensure_default_config()
    data = ds_mod.ControlDataset(dataset_root, split)
    model = nws.NeuralWaveshaping.load_from_checkpoint(model_checkpoint).eval()
    if use_fastnewt:
        model.newt = nws.FastNEWT(model.newt)
    model = model.to(dev)
    with_audio = [n for n in data.names if os.path.exists(os.path.join(data.audio_dir, f"audio_{n}.npy"))]
    if len(with_audio) < len(data):
        print(f"{len(data) - len(with_audio)} of {len(data)} items of {split!r} have no target audio and are left out")
    if not with_audio:
        raise click.ClickException(f"no item of {split!r} under {dataset_root} has target audio: nothing to score")
    torch.cuda.manual_seed(int(seed))
    losses, sizes = [], []
    for k, batch in enumerate(data.batches(with_audio, batch_size)):
        dev_batch = {"audio": torch.from_numpy(np.stack(batch["audio"])).to(dev),
                     "f0": torch.from_numpy(batch["f0"]).to(dev), "control": torch.from_numpy(batch["control"]).to(dev)}
        loss = float(model.test_step(dev_batch, k))
        losses.append(loss)
        sizes.append(len(batch["names"]))
        print(f"batch {k}: {sizes[-1]} items of {batch['f0'].shape[-1]} frames, loss {loss:.6f}")
    mean = float(np.average(losses, weights=sizes))
    print(f"{split}/loss {mean:.6f}  (mean of the batch losses weighted by batch size, {sum(sizes)} items in {len(sizes)} batches; "
          "the spectral convergence is a ratio of norms over a batch, so this is not the loss of the split as one batch)")


if __name__ == "__main__":
    main()
