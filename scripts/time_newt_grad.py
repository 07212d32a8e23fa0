#!/usr/bin/env python
"""Time the stand-alone NEWT forward and its backward (csrc/exciter_newt.hip newt_apply_kernel, csrc/newt_grad.hip)
on the MI355X with the method of scripts/time_td_mlp_grad.py: HIP events on the launch stream around windows of `--inner` calls,
every variant warmed up first, the windows of the variants alternated so that they share whatever else the machine is doing;
median / min / max per call.

Variants at (B, T): the forward `newt_apply` with the exact shapers, `newt_grad` with the exciter's gradient and without the
parameter gradients, `newt_grad` with both, and torch's own autograd through the reference expression (upsample, FiLM, grouped
1x1 convolutions with sines, FiLM, mix) on the same device and shape (forward + backward to the exciter, film and the eleven
parameters, eager).  The FiLM MLP is not part of any variant: scripts/time_td_mlp_grad.py times it.

`--shapers / --width / --depth` (defaults: the packaged 64 / 8 / 4) choose the bank.  At the packaged sizes the runtime-size op
`g_newt_grad` (csrc/g_newt_grad.hip) is timed beside `newt_grad` in the same call; at any other size set the variants
are the runtime-size forward `g_newt_apply`, `g_newt_grad` without and with the parameter gradients, and torch's autograd.

    python scripts/time_newt_grad.py [--batch-size 64] [--frames 500] [--shapers 64] [--width 8] [--depth 4]
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


def torch_autograd_step(exciter, film, g, newt):
    """forward and backward (to the exciter, film and the 2 depth + 3 sample-rate parameters) of the reference's expression"""
    F = torch.nn.functional
    S = newt.n_waveshapers
    sh = newt.shaping_fn
    D = sh.depth
    tensors = [sh.input_scale] + [p for i in range(D) for p in (sh.net[2 * i].weight, sh.net[2 * i].bias)] + [newt.mixer[0].weight, newt.mixer[0].bias]

    def step():
        leaves = [t.detach().requires_grad_() for t in [exciter, film] + tensors]
        e, fl, c = leaves[0], leaves[1], leaves[2]
        g_i, b_i, g_n, b_n = torch.split(F.interpolate(fl, size=e.shape[-1], mode="linear"), S, 1)
        x = c * (g_i * e + b_i)
        for k in range(D):
            x = torch.sin(F.conv1d(x, leaves[3 + 2 * k], leaves[4 + 2 * k], groups=S))
        y = F.conv1d(g_n * x + b_n, leaves[3 + 2 * D], leaves[4 + 2 * D])
        y.backward(g)
        return [t.grad for t in leaves]
    return step


@click.command()
@click.option("--batch-size", default=64)
@click.option("--frames", default=500)
@click.option("--inner", default=3, help="calls per timed window")
@click.option("--windows", default=7, help="timed windows per variant")
@click.option("--warmup", default=2)
@click.option("--json-out", default=None, help="also write the table as JSON")
@click.option("--shapers", default=64, help="NEWT.n_waveshapers")
@click.option("--width", default=8, help="NEWT.shaping_fn_size")
@click.option("--depth", default=4, help="TrainableNonlinearity.depth")
@click.option("--torch-autograd/--no-torch-autograd", "with_torch", default=True,
              help="also time torch's autograd (its activations take gigabytes at the wide banks)")
def main(batch_size, frames, inner, windows, warmup, json_out, shapers, width, depth, with_torch):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    engine = importlib.import_module("neural-waveshaping-synthesis_amd.engine")
    lib = importlib.import_module("neural-waveshaping-synthesis_amd._lib")
    shaping = importlib.import_module("neural-waveshaping-synthesis_amd.models.modules.shaping")
    if not torch.cuda.is_available():
        raise SystemExit("time_newt_grad: needs the GPU (a CPU run cannot give a time)")
    nws.ensure_default_config()
    B, T = batch_size, frames
    torch.manual_seed(0)
    packaged = (shapers, width, depth) == (lib.N_SHAPERS, lib.SHAPER_WIDTH, 4)
    newt = shaping.NEWT(n_waveshapers=shapers, shaping_fn_size=width)
    if not packaged:
        newt.shaping_fn = shaping.TrainableNonlinearity(shapers, width, nonlinearity=shaping.Sine, depth=depth)
    newt = newt.cuda()
    for p in newt.parameters():
        p.requires_grad_(False)
    gen = torch.Generator(device="cuda").manual_seed(0)
    exciter = torch.randn(B, newt.n_waveshapers, T * lib.HOP, device="cuda", generator=gen)
    film = torch.randn(B, 4 * shapers, T, device="cuda", generator=gen)
    g = torch.randn(B, 1, T * lib.HOP, device="cuda", generator=gen)
    b = engine.binding()
    sdesc, mw, mb = newt._g_shaper(), newt.mixer[0].weight, newt.mixer[0].bias
    runtime = {
        "g_newt_grad, exciter and film": lambda: b.g_newt_grad(sdesc, exciter, film, g, mw, mb, True, False),
        "g_newt_grad, with parameters": lambda: b.g_newt_grad(sdesc, exciter, film, g, mw, mb, True, True),
    }
    if packaged:
        wdesc = newt._wdesc()
        workspace = {str(w): int(lib.lib().nws_newt_grad_workspace_bytes(B, T, w)) for w in (0, 1)}
        variants = {
            "newt_apply (forward)": lambda: b.newt_apply(wdesc, exciter, film),
            "newt_grad, exciter and film": lambda: b.newt_grad(wdesc, exciter, film, g, True, False),
            "newt_grad, with parameters": lambda: b.newt_grad(wdesc, exciter, film, g, True, True),
            "torch autograd (forward + backward)": torch_autograd_step(exciter, film, g, newt),
            **runtime,
        }
    else:
        import ctypes as C

        d = lib.NwsShaperDesc.from_buffer_copy(sdesc.numpy())
        workspace = {str(w): int(lib.lib().nws_g_newt_grad_workspace_bytes(C.byref(d), B, T, w)) for w in (0, 1)}
        variants = {
            "g_newt_apply (forward)": lambda: b.g_newt_apply(sdesc, exciter, film, mw, mb),
            **runtime,
            "torch autograd (forward + backward)": torch_autograd_step(exciter, film, g, newt),
        }
    if not with_torch:
        del variants["torch autograd (forward + backward)"]
    with torch.no_grad():
        for name, call in variants.items():
            if not name.startswith("torch"):
                for _ in range(warmup):
                    call()
    for _ in range(warmup if with_torch else 0):
        variants["torch autograd (forward + backward)"]()
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
    if not packaged:
        print(f"{shapers} shapers of width {width} and depth {depth}")
    print(f"B {B} x T {T}; {windows} windows of {inner} calls; ms per call")
    print(f"workspace: {workspace['0']} bytes without, {workspace['1']} bytes with parameters ({workspace['1'] / 2 ** 20:.1f} MiB)")
    table = {}
    for name in variants:
        t = np.array(times[name])
        table[name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}
        print(f"{name:40s} median {np.median(t):9.4f}  min {t.min():9.4f}  max {t.max():9.4f}")
    if json_out:
        os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
        with open(json_out, "w") as f:
            json.dump({"B": B, "T": T, "shapers": shapers, "width": width, "depth": depth, "inner": inner, "windows": windows, "workspace_bytes": workspace, "variants": table}, f, indent=1)


if __name__ == "__main__":
    main()
