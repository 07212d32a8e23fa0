#!/usr/bin/env python
"""Time the multi-resolution STFT loss (csrc/stft_loss.hip) on the MI355X: HIP events on the launch stream around windows
of `--inner` calls, every shape warmed up first, the windows of the variants alternated so that they share whatever else the
machine is doing.  Prints, for the default loss and for each of its resolutions alone: median / min / max time per call over
the windows, the fp32 matrix work the kernels execute (2 signals x padded rows x K columns run x padded frames x 2) and the
rate that makes.  Each resolution is also timed with a full-width window (win_length = n_fft), where the K loop cannot skip
anything: the difference is what skipping the columns outside the window is worth.

`--backward` times `loss_and_grad` (the loss and dL/dx, csrc/stft_grad.hip) the same way, for the default loss and for each of its
resolutions alone, beside the forward call and - where torch.stft runs on the device - beside torch's own autograd through
torch.stft on the same device and shape (forward + backward of the same expression, eager).

    python scripts/time_stft_loss.py [--batch-size 64] [--length-in-seconds 4] [--backward]
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


def matrix_flop(B, N, n_fft, hop, win_length):
    """fp32 multiply-adds x 2 that stft_loss_kernel executes for one resolution (padding of rows, K and frames included)"""
    rows = (2 * (n_fft // 2 + 1) + 31) // 32 * 32             # M-tiles of 32 rows (Re / Im interleaved)
    frames = (1 + N // hop + 31) // 32 * 32
    k_lo = ((n_fft - win_length) // 2) & ~3
    k = ((n_fft - win_length) // 2 + win_length - k_lo + 15) & ~15
    return 2.0 * 2 * B * rows * k * frames


def torch_autograd_step(x, y, resolutions, eps=1e-8):
    """the default loss written with torch.stft, forward and backward to x, on x's device"""
    windows = [torch.hann_window(w, device=x.device) for _, _, w in resolutions]

    def step():
        leaf = x.detach().requires_grad_()
        total = 0.0
        for (n_fft, hop, win), w in zip(resolutions, windows):
            def mag(s):
                S = torch.stft(s, n_fft, hop, win, window=w, center=True, pad_mode="reflect", normalized=False, onesided=True,
                               return_complex=True)
                return torch.sqrt(torch.clamp(S.real ** 2 + S.imag ** 2, min=eps))
            xm, ym = mag(leaf), mag(y)
            total = total + torch.norm(ym - xm, p="fro") / torch.norm(ym, p="fro") + (torch.log(xm) - torch.log(ym)).abs().mean()
        (total / len(resolutions)).backward()
        return leaf.grad
    return step


@click.command()
@click.option("--batch-size", default=64)
@click.option("--length-in-seconds", default=4.0)
@click.option("--sample-rate", default=16000)
@click.option("--inner", default=20, help="calls per timed window")
@click.option("--windows", default=15, help="timed windows per variant")
@click.option("--warmup", default=5)
@click.option("--json-out", default=None, help="also write the table as JSON")
@click.option("--backward", is_flag=True, help="time loss_and_grad (and torch's autograd through torch.stft beside it)")
def main(batch_size, length_in_seconds, sample_rate, inner, windows, warmup, json_out, backward):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    if not torch.cuda.is_available():
        raise SystemExit("time_stft_loss: needs the GPU (a CPU run cannot give a time)")
    B, N = batch_size, int(sample_rate * length_in_seconds)
    g = torch.Generator(device="cuda").manual_seed(0)
    x = 0.3 * torch.randn(B, N, device="cuda", generator=g)
    y = 0.3 * torch.randn(B, N, device="cuda", generator=g)
    default = nws.MultiResolutionSTFTLoss()
    res = list(zip(default.fft_sizes, default.hop_sizes, default.win_lengths))
    # name -> (call, fp32 matrix work of the forward kernels or None)
    variants = {"default (3 resolutions)": (lambda: default(x, y), sum(matrix_flop(B, N, *r) for r in res))}
    if backward:
        variants["default loss_and_grad"] = (lambda: default.loss_and_grad(x, y), None)
        for n, h, w in res:
            variants[f"({n}, {h}, {w}) loss_and_grad"] = (lambda m=nws.STFTLoss(n, h, w): m.loss_and_grad(x, y), None)
        step = torch_autograd_step(x, y, res)
        try:
            step()
            variants["torch autograd through torch.stft"] = (step, None)
        except Exception as e:          # no FFT library for this device: the figure stays unmeasured
            print(f"torch autograd through torch.stft does not run here ({type(e).__name__}: {e}): unmeasured")
    else:
        for n, h, w in res:
            variants[f"({n}, {h}, {w})"] = (lambda m=nws.STFTLoss(n, h, w): m(x, y), matrix_flop(B, N, n, h, w))
            variants[f"({n}, {h}, {n}) full window"] = (lambda m=nws.STFTLoss(n, h, n): m(x, y), matrix_flop(B, N, n, h, n))
    for call, _ in variants.values():
        for _ in range(warmup):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(windows):
        for name, (call, _) in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    print(f"B {B} x N {N} ({length_in_seconds} s at {sample_rate} Hz); {windows} windows of {inner} calls; ms per call")
    table = {}
    for name, (_, flop) in variants.items():
        t = np.array(times[name])
        med = float(np.median(t))
        table[name] = {"median_ms": med, "min_ms": float(t.min()), "max_ms": float(t.max())}
        line = f"{name:38s} median {med:8.4f}  min {t.min():8.4f}  max {t.max():8.4f}"
        if flop is not None:
            table[name].update(matrix_gflop=flop * 1e-9, matrix_tflops_at_median=flop / (med * 1e-3) * 1e-12)
            line += f"   {flop * 1e-9:8.2f} GFLOP  {table[name]['matrix_tflops_at_median']:6.1f} TFLOP/s"
        print(line)
    if json_out:
        os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
        with open(json_out, "w") as f:
            json.dump({"B": B, "N": N, "inner": inner, "windows": windows, "variants": table}, f, indent=1)


if __name__ == "__main__":
    main()
