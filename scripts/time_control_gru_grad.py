#!/usr/bin/env python
"""Time the control encoder's recurrence and its backward (csrc/control_gru.hip control_gru_kernel, csrc/control_gru_grad.hip,
DESIGN.md 3.17) on the MI355X with the method of scripts/time_stft_loss.py: HIP events on the launch stream
around windows of `--inner` calls, every variant warmed up first, the windows of the variants alternated so that they share
whatever else the machine is doing; median / min / max per call.

Variants at (B, T): the forward `control_gru`, `control_gru_grad` without and with the parameter gradients, the C entry point with
neither grad_control nor parameters (the coefficient pass and the sequential kernel alone), and torch's eager nn.GRU forward +
backward (to x and the four parameters) on the same device.  Default nn.GRU initialisation, normal control.

    python scripts/time_control_gru_grad.py [--batch-size 64] [--frames 500]
"""
import ctypes as C
import importlib
import json
import os
import sys

import click
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def torch_autograd_step(gru, x_btc, g):
    """forward and backward (to x and every parameter) of nn.GRU on x's device"""
    def step():
        leaf = x_btc.detach().requires_grad_()
        for p in gru.parameters():
            p.grad = None
        out, _ = gru(leaf)
        out.backward(g)
        return leaf.grad
    return step


@click.command()
@click.option("--batch-size", default=64)
@click.option("--frames", default=500)
@click.option("--inner", default=20, help="calls per timed window")
@click.option("--windows", default=15, help="timed windows per variant")
@click.option("--warmup", default=5)
@click.option("--json-out", default=None, help="also write the table as JSON")
def main(batch_size, frames, inner, windows, warmup, json_out):
    engine = importlib.import_module("neural-waveshaping-synthesis_amd.engine")
    lib = importlib.import_module("neural-waveshaping-synthesis_amd._lib")
    nw = importlib.import_module("neural-waveshaping-synthesis_amd.models.neural_waveshaping")
    if not torch.cuda.is_available():
        raise SystemExit("time_control_gru_grad: needs the GPU (a CPU run cannot give a time)")
    B, T = batch_size, frames
    torch.manual_seed(0)
    mod = nw.ControlModule(2, 128, 128).cuda()
    gen = torch.Generator(device="cuda").manual_seed(0)
    x = torch.randn(B, 2, T, device="cuda", generator=gen)
    g = torch.randn(B, T, 128, device="cuda", generator=gen)
    b = engine.binding()
    L = lib.lib()
    with torch.no_grad():
        wdesc = mod._wdesc()
        gru_out = b.control_gru(wdesc, x, None, False)[0]
    workspace = {"with parameters": int(L.nws_control_gru_grad_workspace_bytes(B, T, 1)),
                 "data only": int(L.nws_control_gru_grad_workspace_bytes(B, T, 0))}
    w = lib.NwsWeights.from_buffer_copy(wdesc.numpy())
    ws = torch.empty(workspace["data only"], dtype=torch.uint8, device="cuda")
    gh0 = torch.empty(B, 128, device="cuda")

    def sequential_only():
        lib.check(L.nws_control_gru_grad(C.byref(w), x.data_ptr(), B, 2, T, None, gru_out.data_ptr(), g.data_ptr(), None, None,
                                         gh0.data_ptr(), None, None, None, None, ws.data_ptr(), ws.numel(),
                                         torch.cuda.current_stream().cuda_stream), "nws_control_gru_grad")

    x_btc = x.transpose(1, 2).contiguous()
    variants = {
        "control_gru (forward)": lambda: b.control_gru(wdesc, x, None, False),
        "control_gru_grad, data only": lambda: b.control_gru_grad(wdesc, x, None, gru_out, g, None, False),
        "control_gru_grad, with parameters": lambda: b.control_gru_grad(wdesc, x, None, gru_out, g, None, True),
        "coefficients + sequential kernel alone (C ABI)": sequential_only,
        "torch nn.GRU (forward + backward)": torch_autograd_step(mod.gru, x_btc, g),
    }
    with torch.no_grad():
        for name, call in variants.items():
            if not name.startswith("torch"):
                for _ in range(warmup):
                    call()
    for _ in range(warmup):
        variants["torch nn.GRU (forward + backward)"]()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(windows):
        for name, call in variants.items():
            with torch.set_grad_enabled(name.startswith("torch")):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                for _ in range(inner):
                    call()
                e1.record()
                e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    print(f"B {B} x T {T}; {windows} windows of {inner} calls; ms per call")
    for tag, n in workspace.items():
        print(f"workspace, {tag}: {n} bytes ({n / 2 ** 20:.1f} MiB)")
    table = {}
    for name in variants:
        t = np.array(times[name])
        table[name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}
        print(f"{name:56s} median {np.median(t):8.4f}  min {t.min():8.4f}  max {t.max():8.4f}")
    if json_out:
        os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
        with open(json_out, "w") as f:
            json.dump({"B": B, "T": T, "inner": inner, "windows": windows, "workspace_bytes": workspace, "variants": table}, f, indent=1)


if __name__ == "__main__":
    main()
