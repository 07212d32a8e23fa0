#!/usr/bin/env python
"""Time the fixed-lag pYIN stream (csrc/pyin_stream.hip, streaming.StreamF0) on the MI355X and show what a lag
costs in agreement with the offline decode.

Times: HIP events on the launch stream around windows of `--inner` back-to-back `push` calls (the method of DESIGN.md 3.12), every
variant warmed up first, the windows of the variants alternated; median / min / max per step over the windows, for
B in {1, 16}, chunk in {128, 256, 1024} samples and lag in {0, 4, 8, 32} frames, beside the offline `pyin_frames` on the same
audio in the same call.  A stream is reset (outside the timed window) before it reaches its frame limit.

Agreement: per lag, the share of frames whose voiced flag equals the offline decode's, and the share of equal bins among the
frames voiced in both, on a wav file (mono, at --sample-rate) or the built-in vibrato tone with silence around it.

    python scripts/time_f0_stream.py [--wav in.wav] [--seconds 4] [--json-out table.json]
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


def vibrato(sr, seconds, f=220.0):
    n = int(sr * seconds)
    t = np.arange(n) / sr
    ph = 2 * np.pi * np.cumsum(f * (1 + 0.01 * np.sin(2 * np.pi * 5.5 * t))) / sr
    x = 0.3 * np.sin(ph) + 0.15 * np.sin(2 * ph) + 0.08 * np.sin(3 * ph)
    x[: n // 8] = 0.0
    x[-n // 8:] = 0.0
    return (x + 1e-3 * np.random.default_rng(0).standard_normal(n)).astype(np.float32)


def windows_of(calls, inner, windows, warmup):
    """{name: [ms per call of each window]}: the variants' windows alternate"""
    for call in calls.values():
        for _ in range(warmup):
            call()
    torch.cuda.synchronize()
    times = {k: [] for k in calls}
    for _ in range(windows):
        for name, call in calls.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(inner):
                call()
            e1.record()
            e1.synchronize()
            times[name].append(e0.elapsed_time(e1) / inner)
    return times


@click.command()
@click.option("--wav", default=None, type=click.Path(exists=True), help="mono wav at --sample-rate (default: a vibrato tone)")
@click.option("--seconds", default=4.0, help="length of the built-in tone and of the offline call that is timed")
@click.option("--sample-rate", default=16000)
@click.option("--inner", default=50, help="calls per timed window")
@click.option("--windows", default=15, help="timed windows per variant")
@click.option("--warmup", default=20)
@click.option("--json-out", default=None, help="also write both tables as JSON")
def main(wav, seconds, sample_rate, inner, windows, warmup, json_out):
    importlib.import_module("neural-waveshaping-synthesis_amd")
    streaming = importlib.import_module("neural-waveshaping-synthesis_amd.streaming")
    fe = importlib.import_module("neural-waveshaping-synthesis_amd.data.utils.f0_extraction")
    if not torch.cuda.is_available():
        raise SystemExit("time_f0_stream: needs the GPU (a CPU run cannot give a time)")
    if wav:
        from scipy.io import wavfile
        sr, x = wavfile.read(wav)
        if sr != sample_rate or x.ndim != 1:
            raise SystemExit(f"{wav}: expected a mono file at {sample_rate} Hz")
        x = x.astype(np.float32) / (float(np.iinfo(x.dtype).max) + 1.0) if np.issubdtype(x.dtype, np.integer) else x.astype(np.float32)
    else:
        x = vibrato(sample_rate, seconds)
    audio = torch.from_numpy(x).cuda().unsqueeze(0)
    N = audio.shape[1]

    # ---- agreement with the offline decode, per lag --------------------------------------------------------------------
    f0_off, _, st_off = fe.pyin_frames(audio, sample_rate)
    n_bins = int(fe.binding().pyin_table(*fe._config(sample_rate, 65.0, 2093.0, 1024, 128))[4])
    agreement = {}
    print(f"agreement with the offline decode ({'the built-in vibrato' if not wav else wav}, {N} samples, {st_off.shape[1]} frames)")
    for lag in (0, 1, 2, 3, 4, 8, 16, 32):
        s = streaming.StreamF0(1, sample_rate, lag=lag)
        outs = [s.push(audio[:, at:at + 1024], final=at + 1024 >= N) for at in range(0, N, 1024)]
        st = torch.cat([o[2] for o in outs], dim=1)
        v_off, v_lag = st_off[0] < n_bins, st[0] < n_bins
        both = v_off & v_lag
        flags = float((v_off == v_lag).double().mean())
        bins = float((st[0][both] == st_off[0][both]).double().mean()) if bool(both.any()) else 1.0
        agreement[lag] = {"voiced_flags_equal": flags, "bins_equal_where_both_voiced": bins, "latency_ms": 1e3 * s.latency_samples / sample_rate}
        print(f"lag {lag:3d} ({agreement[lag]['latency_ms']:6.1f} ms): voiced flags equal {100 * flags:6.2f} %, bins equal where both voiced "
              f"{100 * bins:6.2f} %")

    # ---- time per step ---------------------------------------------------------------------------------------------------
    table = {}
    for B in (1, 16):
        rows = audio.expand(B, N).contiguous()
        calls = {}
        n_off = min(N, int(sample_rate * seconds))
        calls[f"offline pyin_frames, {n_off} samples"] = lambda r=rows[:, :n_off].contiguous(): fe.pyin_frames(r, sample_rate)
        for chunk in (128, 256, 1024):
            # the clip chunk by chunk, round and round (the observation stage's work depends on what it hears: one chunk repeated
            # is a tone of the chunk's period)
            pieces = [rows[:, at:at + chunk].contiguous() for at in range(0, N - chunk + 1, chunk)]
            for lag in (0, 4, 8, 32):
                s = streaming.StreamF0(B, sample_rate, lag=lag)

                def call(s=s, pieces=pieces, at=[0]):
                    s.push(pieces[at[0] % len(pieces)])
                    at[0] += 1
                calls[f"stream chunk {chunk:4d} lag {lag:2d}"] = call
        # (2^21 hops of samples a stream: (warmup + windows * inner) pushes of 1024 samples stay far below it)
        times = windows_of(calls, inner, windows, warmup)
        print(f"B {B}: {windows} windows of {inner} calls; us per call: median | min | max")
        for name, t in times.items():
            t = 1e3 * np.array(t)
            table[f"B {B}, {name}"] = {"median_us": float(np.median(t)), "min_us": float(t.min()), "max_us": float(t.max())}
            print(f"  {name:40s} {np.median(t):9.2f} | {t.min():9.2f} | {t.max():9.2f}")
    if json_out:
        os.makedirs(os.path.dirname(os.path.abspath(json_out)), exist_ok=True)
        with open(json_out, "w") as f:
            json.dump({"samples": N, "inner": inner, "windows": windows, "agreement": agreement, "times": table}, f, indent=1)


if __name__ == "__main__":
    main()
