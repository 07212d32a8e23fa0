#!/usr/bin/env python
"""Time the optimiser step (csrc/adam_step.hip) on the MI355X with the method of scripts/time_newt_grad.py: HIP
events on the launch stream around windows of `--inner` calls, every variant warmed up first, the windows of the variants
alternated so that they share whatever else the machine is doing; median / min / max per call.

Variants on the packaged model's 48 parameter tensors (266 945 floats) with gradients of norm 4, clipped to 2: the `adam_step`
operator (two launches); `clip_grad_norm_` + `torch.optim.Adam(foreach=True)`; the same with `fused=True`.

--training-step: one training step at (--batch-size, --frames) - the reference trains at (8, 500) - taken apart into its links,
each timed on its own with the same method: the forward link by link, the loss, the backward link by link through the `vjp`
methods (the chain `training_step` + `backward` run through autograd), and the optimiser.

--grad-exchange: the two kernels of data-parallel training (csrc/grad_reduce.hip) on the same tensors in the same
windows, with the optimiser step beside them: `grad_pack` of the 48 gradients and one loss element into a row, `grad_reduce` of
W = 2 and W = 8 such rows.  The all-gather between them is not here: one process, one GPU.

    python scripts/time_adam_step.py [--training-step] [--grad-exchange] [--batch-size 8] [--frames 500]
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


def timed(variants, inner, windows, warmup):
    """{name: [ms per call, one per window]}: warm every variant up, then alternate their windows"""
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
    return times


def report(times):
    table = {}
    for name, ts in times.items():
        t = np.array(ts)
        table[name] = {"median_ms": float(np.median(t)), "min_ms": float(t.min()), "max_ms": float(t.max())}
        print(f"{name:48s} median {np.median(t):9.4f}  min {t.min():9.4f}  max {t.max():9.4f}")
    return table


def optimiser_variants(nws, model):
    def leaves():
        ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
        gen = torch.Generator(device="cuda").manual_seed(0)
        gs = [torch.randn(p.shape, device="cuda", generator=gen) for p in ps]
        scale = 4.0 / float(torch.sqrt(sum((g.double() ** 2).sum() for g in gs)))
        for p, g in zip(ps, gs):
            p.grad = scale * g
        return ps

    def ours():
        ps = leaves()
        opt = nws.optim.Adam(ps, lr=1e-3, max_grad_norm=2.0)
        return opt.step

    def theirs(**kw):
        ps = leaves()
        opt = torch.optim.Adam(ps, lr=1e-3, **kw)
        keep = [p.grad.clone() for p in ps]

        def step():
            for p, g in zip(ps, keep):                       # clip_grad_norm_ scales .grad in place: hand it the same input
                p.grad.copy_(g)                              # every call (48 small copies, counted: ours needs none)
            torch.nn.utils.clip_grad_norm_(ps, 2.0, 2.0)
            opt.step()
        return step

    def theirs_no_restore(**kw):
        ps = leaves()
        opt = torch.optim.Adam(ps, lr=1e-3, **kw)

        def step():
            torch.nn.utils.clip_grad_norm_(ps, 2.0, 2.0)     # after the first call the norm is 2 and the clip a multiplication by ~1
            opt.step()
        return step

    return {"adam_step (nws.optim.Adam.step)": ours(),
            "clip_grad_norm_ + Adam(foreach=True)": theirs_no_restore(foreach=True),
            "clip_grad_norm_ + Adam(fused=True)": theirs_no_restore(fused=True),
            "the same, .grad restored first (foreach)": theirs(foreach=True)}


def grad_exchange_variants(nws, model):
    from importlib import import_module

    b = import_module("neural-waveshaping-synthesis_amd.engine").binding()
    gen = torch.Generator(device="cuda").manual_seed(0)
    ps = [torch.nn.Parameter(p.detach().clone()) for p in model.parameters()]
    for p in ps:
        p.grad = 1e-3 * torch.randn(p.shape, device="cuda", generator=gen)
    loss = torch.ones(1, device="cuda")
    P = sum(p.numel() for p in ps)
    stride = -(-(P + 1) // 4) * 4
    rows = {W: torch.randn(W, stride, device="cuda", generator=gen) for W in (2, 8)}
    mean = torch.zeros(stride, device="cuda")
    tensors = [p.grad for p in ps] + [loss]
    opt = nws.optim.Adam(ps, lr=1e-3, max_grad_norm=2.0)
    out = {"grad_pack (48 gradients + loss into a row)": lambda: b.grad_pack(tensors, rows[2][0])}
    for W in (2, 8):
        out[f"grad_reduce W = {W}, P = {P + 1}"] = lambda W=W: b.grad_reduce(rows[W], mean[:P + 1])
    out["adam_step (nws.optim.Adam.step)"] = opt.step
    return out


def training_step_variants(nws, model, B, T):
    dyn = importlib.import_module("neural-waveshaping-synthesis_amd.models.modules.dynamic")
    gen = torch.Generator(device="cuda").manual_seed(0)
    f0 = 200.0 + 300.0 * torch.rand(B, 1, T, device="cuda", generator=gen)
    control = torch.randn(B, 2, T, device="cuda", generator=gen)
    audio = 0.1 * torch.randn(B, T * int(model.control_hop), device="cuda", generator=gen)
    batch = {"audio": audio, "f0": f0, "control": control}
    opt = nws.optim.Adam(model.parameters(), lr=1e-6, max_grad_norm=2.0)
    loss_fn = model.stft_loss
    with torch.no_grad():
        _, _, phase_u, noise = model._checked_inputs(f0, control, None, None)
        f0_up = dyn.upsample_linear(f0, int(model.control_hop))
        sig = model.osc(f0_up[:, 0], phase_u=phase_u)
        ctl = control[:, 0:2].contiguous()
        exc = model.harmonic_mixer(sig)
        emb = model.embedding(ctl)
        H = model.h_generator(emb)
        pre = model.newt(exc, emb)[:, 0] + model.noise_synth(H, noise=noise)[:, 0]
        y = model.reverb(pre)
        _, g_y = loss_fn.loss_and_grad(y, audio)
        g_pre, _ = model.reverb.vjp(pre, g_y)
        g_pre3 = g_pre[:, None, :].contiguous()
        g_exc, g_emb_newt, _ = model.newt.vjp(g_pre3, exc, emb)
        g_H = model.noise_synth.vjp(g_pre, noise)
        g_emb_noise, _ = model.h_generator.vjp(g_H, emb)
        g_emb = g_emb_newt + g_emb_noise

    def whole():
        torch.cuda.manual_seed(0)
        model.training_step(batch, 0).backward()
        opt.step()
        opt.zero_grad(set_to_none=True)

    def forward_and_backward():
        torch.cuda.manual_seed(0)
        model.training_step(batch, 0).backward()
        opt.zero_grad(set_to_none=True)

    def optimiser():
        for p in model.parameters():
            p.grad = torch.zeros_like(p) if p.grad is None else p.grad
        opt.step()

    ng = torch.no_grad()

    def no_grad(fn):
        def call():
            with ng:
                return fn()
        return call

    links = {
        "whole step (training_step, backward, optimiser)": whole,
        "training_step + backward (autograd)": forward_and_backward,
        "forward: upsample + oscillator bank": no_grad(lambda: model.osc(dyn.upsample_linear(f0, int(model.control_hop))[:, 0], phase_u=phase_u)),
        "forward: harmonic_mixer": no_grad(lambda: model.harmonic_mixer(sig)),
        "forward: embedding (GRU + proj)": no_grad(lambda: model.embedding(ctl)),
        "forward: newt": no_grad(lambda: model.newt(exc, emb)),
        "forward: h_generator": no_grad(lambda: model.h_generator(emb)),
        "forward: noise_synth": no_grad(lambda: model.noise_synth(H, noise=noise)),
        "forward: reverb": no_grad(lambda: model.reverb(pre)),
        "loss": no_grad(lambda: loss_fn(y, audio)),
        "backward: loss (dL/dy)": no_grad(lambda: loss_fn._grad(y, audio)),
        "backward: reverb.vjp": no_grad(lambda: model.reverb.vjp(pre, g_y)),
        "backward: newt.vjp": no_grad(lambda: model.newt.vjp(g_pre3, exc, emb)),
        "backward: harmonic_mixer.vjp": no_grad(lambda: model.harmonic_mixer.vjp(g_exc, sig)),
        "backward: noise_synth.vjp": no_grad(lambda: model.noise_synth.vjp(g_pre, noise)),
        "backward: h_generator.vjp": no_grad(lambda: model.h_generator.vjp(g_H, emb)),
        "backward: embedding.vjp": no_grad(lambda: model.embedding.vjp(g_emb, ctl)),
        "optimiser (nws.optim.Adam.step, clip 2)": optimiser,
    }
    return links


@click.command()
@click.option("--training-step", is_flag=True, help="also take one training step apart, link by link")
@click.option("--grad-exchange", is_flag=True, help="also time grad_pack and grad_reduce (W = 2, 8) beside the optimiser step")
@click.option("--batch-size", default=8)
@click.option("--frames", default=500)
@click.option("--inner", default=3, help="calls per timed window")
@click.option("--windows", default=7, help="timed windows per variant")
@click.option("--warmup", default=2)
@click.option("--json-out", default=None, help="also write the tables as JSON")
def main(training_step, grad_exchange, batch_size, frames, inner, windows, warmup, json_out):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    if not torch.cuda.is_available():
        raise SystemExit("time_adam_step: needs the GPU (a CPU run cannot give a time)")
    nws.ensure_default_config()
    model = nws.NeuralWaveshaping.load_from_checkpoint(os.path.join(ROOT, "tests", "golden", "weights_vn.npz")).cuda()
    out = {"inner": inner, "windows": windows}
    print(f"the optimiser step on {len(list(model.parameters()))} tensors, {sum(p.numel() for p in model.parameters())} floats; "
          f"{windows} windows of {inner} calls; ms per call")
    out["optimiser"] = report(timed(optimiser_variants(nws, model), inner, windows, warmup))
    if grad_exchange:
        print(f"the gradient exchange's kernels beside the optimiser step; {windows} windows of {inner} calls; ms per call")
        out["grad_exchange"] = report(timed(grad_exchange_variants(nws, model), inner, windows, warmup))
    if training_step:
        model.differentiable = True
        print(f"one training step at ({batch_size}, {frames}), link by link; ms per call")
        out["training_step"] = report(timed(training_step_variants(nws, model, batch_size, frames), inner, windows, warmup))
    if json_out:
        os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
        with open(json_out, "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()
