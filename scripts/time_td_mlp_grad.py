#!/usr/bin/env python
"""Time the frame MLP and its backward (csrc/stages.hip td_mlp_kernel, csrc/td_mlp_grad.hip) on the MI355X with the
method of scripts/time_stft_loss.py: HIP events on the launch stream around windows of `--inner` calls, every
variant warmed up first, the windows of the variants alternated so that they share whatever else the machine is doing; median /
min / max per call.

Both packaged size sets, (128, 128, 129, 4) (h_generator) and (128, 128, 256, 4) (newt.mlp).  Variants: the forward `td_mlp`,
`td_mlp_grad` without and with the parameter gradients, and torch's own autograd through conv1d / layer_norm / leaky_relu on the
same device and shape (forward + backward to x and every parameter, eager).

    python scripts/time_td_mlp_grad.py [--batch-size 64] [--frames 500]
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

SIZES = ((128, 128, 129, 4), (128, 128, 256, 4))


def random_mlp(sizes, gen):
    cin, hidden, cout, depth = sizes
    w = [cin] + [hidden] * (depth - 1) + [cout]
    rn = lambda *s: torch.randn(*s, device="cuda", generator=gen)
    ws = [rn(w[i + 1], w[i]) / w[i] ** 0.5 for i in range(depth)]
    bs = [0.1 * rn(w[i + 1]) for i in range(depth)]
    gs = [1.0 + 0.1 * rn(hidden) for _ in range(depth - 1)]
    ls = [0.1 * rn(hidden) for _ in range(depth - 1)]
    return ws, bs, gs, ls


def torch_autograd_step(x, g, ws, bs, gs, ls):
    """forward and backward (to x and every parameter) of the reference's expression on x's device"""
    F = torch.nn.functional

    def step():
        leaves = [t.detach().requires_grad_() for t in [x] + ws + bs + gs + ls]
        d = len(ws)
        h, W, b, ga, be = leaves[0], leaves[1:1 + d], leaves[1 + d:1 + 2 * d], leaves[1 + 2 * d:2 * d + d], leaves[2 * d + d:]
        for i in range(d):
            h = F.conv1d(h, W[i][:, :, None], b[i])
            if i < d - 1:
                h = F.leaky_relu(F.layer_norm(h.transpose(1, 2), (h.shape[1],), ga[i], be[i], 1e-5).transpose(1, 2), 0.01)
        h.backward(g)
        return [t.grad for t in leaves]
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
    if not torch.cuda.is_available():
        raise SystemExit("time_td_mlp_grad: needs the GPU (a CPU run cannot give a time)")
    B, T = batch_size, frames
    gen = torch.Generator(device="cuda").manual_seed(0)
    b = engine.binding()
    variants, workspace = {}, {}
    for sizes in SIZES:
        ws, bs, gs, ls = random_mlp(sizes, gen)
        x = torch.randn(B, sizes[0], T, device="cuda", generator=gen)
        g = torch.randn(B, sizes[2], T, device="cuda", generator=gen)
        tag = "x".join(map(str, sizes))
        workspace[tag] = int(lib.lib().nws_td_mlp_grad_workspace_bytes(B, *sizes, T, 1))
        variants[f"{tag} td_mlp (forward)"] = lambda x=x, p=(ws, bs, gs, ls): b.td_mlp(x, *p, 1e-5, 0.01)
        variants[f"{tag} td_mlp_grad, data only"] = lambda x=x, g=g, p=(ws, bs, gs, ls): b.td_mlp_grad(x, g, *p, 1e-5, 0.01, False)
        variants[f"{tag} td_mlp_grad, with parameters"] = lambda x=x, g=g, p=(ws, bs, gs, ls): b.td_mlp_grad(x, g, *p, 1e-5, 0.01, True)
        variants[f"{tag} torch autograd (forward + backward)"] = torch_autograd_step(x, g, ws, bs, gs, ls)
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
    print(f"B {B} x T {T}; {windows} windows of {inner} calls; ms per call")
    for tag, n in workspace.items():
        print(f"{tag}: workspace with parameters {n} bytes ({n / 2 ** 20:.1f} MiB)")
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
