#!/usr/bin/env python
"""Time the analysis streams that turn chunked audio into the model's control inputs on the MI355X: `StreamLoudness` alone
(csrc/loudness_stream.hip), `StreamF0` alone, `StreamControl` (both, and make_control on the
device), beside the offline `loudness_frames` on the whole clip in the same call; with --release DB_PER_S also a releasing
`StreamLoudness` and the whole-clip `causal_loudness_frames` with and without that release.

The method of scripts/time_f0_stream.py: HIP events on the launch stream around windows of `--inner` back-to-back `push` calls,
every variant warmed up first, the windows of the variants alternated; median / min / max per step over the windows, for
B in {1, 16} and chunks of 128 / 256 / 1024 samples.  The pushes walk through a tone chunk by chunk, round and round (the pYIN
stream's work depends on what it hears).

    python scripts/time_control_stream.py [--seconds 4] [--lag 8] [--release 6] [--json-out table.json]
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from time_f0_stream import vibrato, windows_of  # noqa: E402


@click.command()
@click.option("--seconds", default=4.0, help="length of the tone and of the offline call that is timed")
@click.option("--lag", default=8, type=click.IntRange(0, 255), show_default=True)
@click.option("--release", default=0.0, type=click.FloatRange(0.0), show_default=True,
              help="also time the releasing stream and the whole-clip causal extractor at this many dB per second")
@click.option("--inner", default=50, help="calls per timed window")
@click.option("--windows", default=15, help="timed windows per variant")
@click.option("--warmup", default=20)
@click.option("--json-out", default=None, help="also write the table as JSON")
def main(seconds, lag, release, inner, windows, warmup, json_out):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    streaming = importlib.import_module("neural-waveshaping-synthesis_amd.streaming")
    ldx = importlib.import_module("neural-waveshaping-synthesis_amd.data.utils.loudness_extraction")
    if not torch.cuda.is_available():
        raise SystemExit("time_control_stream: needs the GPU (a CPU run cannot give a time)")
    nws.ensure_default_config()
    model = nws.NeuralWaveshaping.load_from_checkpoint(os.path.join(ROOT, "tests", "golden", "weights_vn.npz")).eval().cuda()
    sr = int(model.sample_rate)
    audio = torch.from_numpy(vibrato(sr, seconds)).cuda().unsqueeze(0)
    N = audio.shape[1]
    table = {}
    for B in (1, 16):
        rows = audio.expand(B, N).contiguous()
        calls = {f"offline loudness_frames, {N} samples": lambda r=rows: ldx.loudness_frames(r, 1024, 128)}
        if release > 0.0:
            calls[f"causal_loudness_frames, {N} samples"] = lambda r=rows: ldx.causal_loudness_frames(r, 1024, 128, lag, sample_rate=sr)
            calls[f"causal_loudness_frames releasing, {N} samples"] = lambda r=rows: ldx.causal_loudness_frames(
                r, 1024, 128, lag, release_db_per_s=release, sample_rate=sr)
        for chunk in (128, 256, 1024):
            pieces = [rows[:, at:at + chunk].contiguous() for at in range(0, N - chunk + 1, chunk)]
            streams = {"StreamLoudness": streaming.StreamLoudness(B, lag=lag), "StreamF0": streaming.StreamF0(B, sr, lag=lag),
                       "StreamControl": streaming.StreamControl(model, B, lag=lag)}
            if release > 0.0:
                streams["StreamLoudness releasing"] = streaming.StreamLoudness(B, lag=lag, release_db_per_s=release, sample_rate=sr)
            for name, s in streams.items():
                def call(s=s, pieces=pieces, at=[0]):
                    s.push(pieces[at[0] % len(pieces)])
                    at[0] += 1
                calls[f"{name} chunk {chunk:4d}"] = call
        # (2^21 hops of samples a stream: (warmup + windows * inner) pushes of 1024 samples stay far below it)
        times = windows_of(calls, inner, windows, warmup)
        print(f"B {B}, lag {lag}: {windows} windows of {inner} calls; us per call: median | min | max")
        for name, t in times.items():
            t = 1e3 * np.array(t)
            table[f"B {B}, {name}"] = {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max())}
            print(f"  {name:44s} {np.median(t):9.2f} | {t.min():9.2f} | {t.max():9.2f}")
    if release > 0.0:          # the whole-clip calls at the flagship batch as well
        rows = audio.expand(64, N).contiguous()
        calls = {f"offline loudness_frames, {N} samples": lambda: ldx.loudness_frames(rows, 1024, 128),
                 f"causal_loudness_frames, {N} samples": lambda: ldx.causal_loudness_frames(rows, 1024, 128, lag, sample_rate=sr),
                 f"causal_loudness_frames releasing, {N} samples": lambda: ldx.causal_loudness_frames(
                     rows, 1024, 128, lag, release_db_per_s=release, sample_rate=sr)}
        print(f"B 64, lag {lag}: us per call: median | min | max")
        for name, t in windows_of(calls, inner, windows, warmup).items():
            t = 1e3 * np.array(t)
            table[f"B 64, {name}"] = {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max())}
            print(f"  {name:44s} {np.median(t):9.2f} | {t.min():9.2f} | {t.max():9.2f}")
    hop_ms = 1e3 * 128 / sr
    one = table["B 1, StreamLoudness chunk  128"]["median_us"]
    print(f"a one-hop step of StreamLoudness at B = 1: {one:.1f} us = {100 * one / (1e3 * hop_ms):.2f} % of its {hop_ms:.0f} ms hop")
    if json_out:
        os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
        with open(json_out, "w") as f:
            json.dump({"samples": N, "lag": lag, "inner": inner, "windows": windows, "times": table}, f, indent=1)


if __name__ == "__main__":
    main()
