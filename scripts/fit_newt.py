#!/usr/bin/env python
"""Fit the oscillator branch of a checkpoint - or the whole model - to a set of recordings.  The oscillator branch has a backward
pass (csrc/newt_grad.hip), and so have the control encoder (3.17), the frame MLPs (3.16), the noise filter (3.15),
the reverb (3.14) and the loss (3.13): every parameter of the packaged model gets a gradient computed by HIP kernels.

    python scripts/fit_newt.py --model-checkpoint ckpt --dataset-root data/ --split train --steps 200 \\
        --params {shapers,branch,model} --output ckpt_out [--lr 1e-3] [--seed 0]

--params shapers: the 64 waveshapers and their mix, `newt.shaping_fn.*` and `newt.mixer.*` (11 tensors).  The noise channel and
    the control embedding are rendered without a graph; oscillator bank -> `harmonic_mixer` -> `newt` (differentiable) carries
    the gradient.
--params branch: the 27 tensors of `harmonic_mixer.*` and `newt.*` - the FiLM MLP `newt.mlp` included; the control embedding is
    still an input without a graph.
--params model: every parameter.  `embedding`, `harmonic_mixer`, `newt`, `h_generator`, `noise_synth`, `reverb` and the loss are
    all set differentiable; the control embedding carries its graph into both branches and autograd adds the two shares before
    `ControlModule`'s backward takes them.

The pre-reverb signal is `newt(exciter, emb)[:, 0] + noise_synth(h_generator(emb))[:, 0]`, as in scripts/fit_noise.py.  The
optimiser is the reference's `configure_optimizers`: Adam(lr) with StepLR(lr_decay_interval, lr_decay), all three from the model's
hparams (--lr replaces the first).  The batches' gradients are summed and Adam takes one step per pass over the split.  The hidden
draws of the render (phase offsets, noise excitation) come from the device generator, re-seeded with --seed at the start of every
step: the printed losses are values of one fixed objective and a run repeats to the bit.  There is no FastNEWT option: the lookup
table has no backward and training uses the exact shapers, as the reference does.  The output is written in the input's format and
differs from the input checkpoint in exactly the fitted keys; `NeuralWaveshaping.load_from_checkpoint` reads it.

`--model-gin` names the model's gin file when it is not the packaged one.  A model with another waveshaper bank (up to 64 shapers of
width up to 16 and depth up to 4), harmonic count, sample rate or reverb length fits in all three modes: its oscillator branch's
backward is csrc/g_newt_grad.hip, and the tensor counts above change with the shapers' depth.
"""
import importlib
import os
import sys

import click
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

MODES = ["shapers", "branch", "model"]


def fitted_parameters(model, mode):
    """{state-dict key: parameter} of a mode, after setting the flags the mode needs; every other parameter is frozen"""
    named = dict(model.named_parameters())
    if mode == "shapers":
        keys = [k for k in named if k.startswith("newt.shaping_fn.") or k.startswith("newt.mixer.")]
    elif mode == "branch":
        keys = [k for k in named if k.startswith("newt.") or k.startswith("harmonic_mixer.")]
    else:
        keys = list(named)
    for k, p in named.items():
        p.requires_grad_(k in keys)
    model.newt.differentiable = True
    model.reverb.differentiable = True                      # dL/dx of the reverb is what reaches both branches
    model.harmonic_mixer.differentiable = mode != "shapers"
    for m in (model.embedding, model.h_generator, model.noise_synth):
        m.differentiable = mode == "model"
    return {k: named[k] for k in keys}


def pre_reverb(model, f0, control, mode):
    """the reverb's input (B, N) with the graph a mode needs; draws the two hidden inputs in the forward's order"""
    # the composition NeuralWaveshaping.forward runs under its `differentiable` flag: one copy, in the package
    return importlib.import_module("neural-waveshaping-synthesis_amd.models.neural_waveshaping").pre_reverb_graph(model, f0, control, mode)


@click.command()
@click.option("--model-gin", default=None)
@click.option("--model-checkpoint", required=True)
@click.option("--dataset-root", required=True)
@click.option("--split", default="train")
@click.option("--batch-size", default=64)
@click.option("--steps", default=100, help="optimiser steps; each one passes over every batch of the split once")
@click.option("--params", "mode", type=click.Choice(MODES), default="branch",
              help="shapers: newt.shaping_fn.* and newt.mixer.*; branch: harmonic_mixer.* and newt.*; model: every parameter")
@click.option("--lr", default=None, type=float, help="Adam's learning rate (default: the model's learning_rate hparam)")
@click.option("--output", required=True, help="checkpoint to write (.npz: flat arrays; anything else: a torch checkpoint)")
@click.option("--seed", default=0, help="seeds the device generator the hidden draws of the render come from, at every step")
def main(model_gin, model_checkpoint, dataset_root, split, batch_size, steps, mode, lr, output, seed):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    ds_mod = importlib.import_module("neural-waveshaping-synthesis_amd.dataset")
    ckpt = importlib.import_module("neural-waveshaping-synthesis_amd.checkpoint")
    dev = torch.device("cuda", int(os.environ.get("LOCAL_RANK", 0)))
    torch.cuda.set_device(dev)
    if model_gin:
        nws.gin.parse_config_file(model_gin)
    else:
        nws.ensure_default_config()
    data = ds_mod.ControlDataset(dataset_root, split)
    model = nws.NeuralWaveshaping.load_from_checkpoint(model_checkpoint).eval().to(dev)
    fitted = fitted_parameters(model, mode)
    loss_fn = nws.MultiResolutionSTFTLoss(differentiable=True)
    # the reference's configure_optimizers (models/neural_waveshaping.py:92-102)
    opt = torch.optim.Adam(list(fitted.values()), lr=float(model.learning_rate if lr is None else lr))
    sched = torch.optim.lr_scheduler.StepLR(opt, int(model.lr_decay_interval), float(model.lr_decay))
    with_audio = [n for n in data.names if os.path.exists(os.path.join(data.audio_dir, f"audio_{n}.npy"))]
    if len(with_audio) < len(data):
        print(f"{len(data) - len(with_audio)} of {len(data)} items of {split!r} have no target audio and are left out")
    if not with_audio:
        raise click.ClickException(f"no item of {split!r} under {dataset_root} has target audio: nothing to fit to")
    for step in range(int(steps)):
        torch.cuda.manual_seed(int(seed))
        opt.zero_grad(set_to_none=True)
        losses, sizes = [], []
        for batch in data.batches(with_audio, batch_size):
            audio = torch.from_numpy(np.stack(batch["audio"])).to(dev)
            f0, control = torch.from_numpy(batch["f0"]).to(dev), torch.from_numpy(batch["control"]).to(dev)
            pre = pre_reverb(model, f0, control, mode)
            if pre.shape != audio.shape:
                raise click.ClickException(f"the model renders {tuple(pre.shape)} but the batch's audio is {tuple(audio.shape)}")
            loss = loss_fn(model.reverb(pre), audio)
            loss.backward()                                   # the batches' gradients add up in the parameters' .grad
            losses.append(float(loss))
            sizes.append(len(batch["names"]))
        opt.step()
        sched.step()
        print(f"step {step}: loss {float(np.average(losses, weights=sizes)):.6f}  ({sum(sizes)} items in {len(sizes)} batches)")
    ckpt.write_checkpoint(output, model_checkpoint, dict(fitted))
    print(f"wrote {output}: {len(fitted)} tensors ({mode}) fitted in {int(steps)} steps, every other tensor as in {model_checkpoint}")


if __name__ == "__main__":
    main()
