#!/usr/bin/env python
"""Time the noise branch and its backward (csrc/fir_noise.hip, csrc/fir_noise_grad.hip) on the MI355X with the
method of scripts/time_stft_loss.py: HIP events on the launch stream around windows of `--inner` calls, every variant warmed up
first, the windows of the variants alternated so that they share whatever else the machine is doing; median / min / max per call.

Variants: the forward `fir_noise` (taps given), `fir_noise_grad` (dL/d(taps)), `fir_from_h_grad` (dL/dH from it),
`FIRNoiseSynth.vjp` (both), `sum_batch_time` (the reduction onto a per-band offset) and - where torch's FFT runs on the device -
torch's own autograd through the reference expression (models/modules/generators.py:21-35) on the same device and shape
(forward + backward to H, eager).

    python scripts/time_fir_noise_grad.py [--batch-size 64] [--frames 500]
"""
import importlib
import json
import os
import sys

import click
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_autograd_step(H, noise, g, window):
    """forward and backward (to H) of the reference's expression with the excitation injected, on H's device"""
    ones = torch.ones(256, device=H.device)

    def step():
        Hl = H.detach().requires_grad_()
        h = torch.fft.irfft(torch.complex(Hl, torch.zeros_like(Hl)).transpose(1, 2)).roll(128, -1) * window.view(1, 1, -1)
        X = torch.stft(noise, 256, 128, window=ones, return_complex=True).unsqueeze(0)
        y = torch.istft(X * torch.fft.rfft(h).transpose(1, 2), 256, 128, window=ones, center=False)[:, : Hl.shape[-1] * 128]
        y.backward(g)
        return Hl.grad
    return step


@click.command()
@click.option("--batch-size", default=64)
@click.option("--frames", default=500)
@click.option("--inner", default=20, help="calls per timed window")
@click.option("--windows", default=15, help="timed windows per variant")
@click.option("--warmup", default=5)
@click.option("--json-out", default=None, help="also write the table as JSON")
def main(batch_size, frames, inner, windows, warmup, json_out):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    engine = importlib.import_module("neural-waveshaping-synthesis_amd.engine")
    if not torch.cuda.is_available():
        raise SystemExit("time_fir_noise_grad: needs the GPU (a CPU run cannot give a time)")
    B, T = batch_size, frames
    gen = torch.Generator(device="cuda").manual_seed(0)
    H = 0.5 + 0.3 * torch.randn(B, 129, T, device="cuda", generator=gen)
    u = torch.rand(128 * T - 1, device="cuda", generator=gen)
    g = torch.randn(B, 128 * T, device="cuda", generator=gen)
    syn = nws.FIRNoiseSynth(256, 128).cuda()
    b = engine.binding()
    D = syn._design_matrix(H.device)
    fir = b.fir_from_h(H, D)
    du = b.fir_noise_grad(u, g)
    dH = b.fir_from_h_grad(du, D)
    variants = {"fir_noise (forward)": lambda: b.fir_noise(fir, u, None, -1),
                "fir_noise_grad": lambda: b.fir_noise_grad(u, g),
                "fir_from_h_grad": lambda: b.fir_from_h_grad(du, D),
                "FIRNoiseSynth.vjp": lambda: syn.vjp(g, u),
                "sum_batch_time": lambda: b.sum_batch_time(dH)}
    step = torch_autograd_step(H, u, g, syn.window)
    try:
        step()
        variants["torch autograd through stft / istft"] = step
    except Exception as e:              # no FFT library for this device: the figure stays unmeasured
        print(f"torch autograd through stft / istft does not run here ({type(e).__name__}: {e}): unmeasured")
    for call in variants.values():
        for _ in range(warmup):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(windows):
        for name, call in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    print(f"B {B} x T {T} ({128 * T} samples); {windows} windows of {inner} calls; ms per call")
    table = {}
    for name in variants:
        t = np.array(times[name])
        table[name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}
        print(f"{name:38s} median {np.median(t):8.4f}  min {t.min():8.4f}  max {t.max():8.4f}")
    if json_out:
        os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
        with open(json_out, "w") as f:
            json.dump({"B": B, "T": T, "inner": inner, "windows": windows, "variants": table}, f, indent=1)


if __name__ == "__main__":
    main()
