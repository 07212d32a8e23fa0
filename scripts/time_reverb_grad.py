#!/usr/bin/env python
"""Time the learned reverb and its transpose (csrc/reverb_fft.hip) on the MI355X with the method of
scripts/time_stft_loss.py: HIP events on the launch stream around windows of `--inner` calls, every variant warmed up first,
the windows of the variants alternated so that they share whatever else the machine is doing; median / min / max per call.

Variants: the forward `reverb`, `reverb_grad_x` (dL/dx), `reverb_grad_ir` (dL/d(ir), summed over the batch), and - where
torch's FFT runs on the device - torch's own autograd through the reference's rfft / irfft expression on the same device and
shape (forward + backward to x and ir, eager).

    python scripts/time_reverb_grad.py [--batch-size 64] [--length-in-seconds 4]
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


def torch_autograd_step(x, g, ir):
    """forward and backward (to x and ir) of the reference's expression (models/modules/shaping.py:161-173) on x's device"""
    import torch.nn.functional as F

    zero = torch.zeros(1, 1, device=x.device)

    def step():
        xl, irl = x.detach().requires_grad_(), ir.detach().requires_grad_()
        ir_ = torch.cat((zero, irl), dim=-1)
        if xl.shape[-1] > ir_.shape[-1]:
            ir_, x_ = F.pad(ir_, (0, xl.shape[-1] - ir_.shape[-1])), xl
        else:
            x_ = F.pad(xl, (0, ir_.shape[-1] - xl.shape[-1]))
        y = xl + torch.fft.irfft(torch.fft.rfft(x_) * torch.fft.rfft(ir_))[..., : xl.shape[-1]]
        y.backward(g)
        return xl.grad, irl.grad
    return step


@click.command()
@click.option("--batch-size", default=64)
@click.option("--length-in-seconds", default=4.0)
@click.option("--sample-rate", default=16000)
@click.option("--inner", default=20, help="calls per timed window")
@click.option("--windows", default=15, help="timed windows per variant")
@click.option("--warmup", default=5)
@click.option("--json-out", default=None, help="also write the table as JSON")
def main(batch_size, length_in_seconds, sample_rate, inner, windows, warmup, json_out):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    if not torch.cuda.is_available():
        raise SystemExit("time_reverb_grad: needs the GPU (a CPU run cannot give a time)")
    B, N = batch_size, int(sample_rate * length_in_seconds)
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(B, N, device="cuda", generator=gen)
    g = torch.randn(B, N, device="cuda", generator=gen)
    rev = nws.Reverb(2, int(sample_rate)).cuda()          # the model's: 2 s of impulse response
    ir_len = rev.ir.shape[-1]
    with torch.no_grad():
        rev.ir.copy_(0.2 * torch.exp(-6.0 * torch.arange(ir_len, device="cuda") / ir_len) * torch.randn(ir_len, device="cuda", generator=gen))
    rev.ir.requires_grad_(False)          # the timed forward is the plain one: no graph, no warning about one
    variants = {"reverb (forward)": lambda: rev(x),
                "reverb_grad_x": lambda: rev.vjp(x, g, need_ir=False),
                "reverb_grad_ir": lambda: rev.vjp(x, g, need_x=False),
                "both gradients": lambda: rev.vjp(x, g)}
    step = torch_autograd_step(x, g, rev.ir.detach())
    try:
        step()
        variants["torch autograd through rfft / irfft"] = step
    except Exception as e:              # no FFT library for this device: the figure stays unmeasured
        print(f"torch autograd through rfft / irfft does not run here ({type(e).__name__}: {e}): unmeasured")
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
    print(f"B {B} x N {N} ({length_in_seconds} s at {sample_rate} Hz), {ir_len} taps; {windows} windows of {inner} calls; ms per call")
    table = {}
    for name in variants:
        t = np.array(times[name])
        table[name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}
        print(f"{name:38s} median {np.median(t):8.4f}  min {t.min():8.4f}  max {t.max():8.4f}")
    if json_out:
        os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
        with open(json_out, "w") as f:
            json.dump({"B": B, "N": N, "ir_len": int(ir_len), "inner": inner, "windows": windows, "variants": table}, f, indent=1)


if __name__ == "__main__":
    main()
