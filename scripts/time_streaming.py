#!/usr/bin/env python
"""Latency of the STATEFUL streaming path (NewtStream.push): hops of `--hop-frames` control frames (2 = 256 samples =
16 ms of audio) pushed back to back, HIP-event timed per push.  Unlike scripts/time_buffer_sizes.py (stateless, hipGraph)
every push carries GRU / phase / noise / reverb state and applies the 2 s reverb as a linear convolution of the stream
(csrc/stream.hip); steady-state hops replay a hipGraph unless --no-graph.  Host wall-clock per push is reported beside the
HIP-event latency (a push returns a fresh tensor: input copy + graph launch + output copy).
--slots: the slot mode (model.voices(B)) under a random note-on / note-off schedule (every hop each idle slot starts
with probability --note-on, each active one stops with probability --note-off); same timing, events written every hop.
--model-gin FILE: a model of another architecture (its stream runs on the runtime-size kernels, DESIGN.md 3.21, its slot stream
too, 3.28), with the weights of --checkpoint, or seeded random ones when none is named: the hop's latency depends on the sizes,
not on the values.
--runtime-size: the packaged model on the runtime-size stream (with --slots: on the runtime-size slot stream), to compare the two
paths on one set of sizes.
--output-rate R: after every hop its samples go through a StreamResampler(model rate -> R) (csrc/resample_stream.hip, DESIGN.md
3.23), with --static-io through its captured hop: the hop's latency with and without the converter, the converter's own time
and the output sample count are reported beside the figures above.  Not with --slots."""
import importlib
import os
import sys

import click
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


@click.command()
@click.option("--checkpoint", default=None, help="default: the packaged weights, or seeded random ones with --model-gin")
@click.option("--model-gin", default=None, help="the model's gin file when it is not the packaged one")
@click.option("--runtime-size", is_flag=True, default=False, help="force the runtime-size stream (GenericNewtStream)")
@click.option("--batch-size", default=1)
@click.option("--hop-frames", default=2)
@click.option("--num-hops", default=500)
@click.option("--use-fast-newt/--no-fast-newt", default=True)
@click.option("--graph/--no-graph", default=True)
@click.option("--static-io/--copy-io", default=False, help="time NewtStream.hop(): the caller fills the captured hop's own "
              "input buffers and reads its output buffer (no input / output copies), like an audio callback would")
@click.option("--json-out", default=None)
@click.option("--slots", is_flag=True, default=False, help="time the slot mode (VoiceStream) under a random note-on/off schedule")
@click.option("--note-on", default=0.2, help="--slots: per-hop start probability of an idle slot")
@click.option("--note-off", default=0.1, help="--slots: per-hop stop probability of an active slot")
@click.option("--seed", default=0)
@click.option("--output-rate", default=None, type=int, help="convert every hop to this sample rate with a StreamResampler and time it")
@click.option("--gc/--no-gc", "keep_gc", default=True, help="--no-gc: Python's cyclic garbage collector off during the timed hops "
              "(what a host with a real-time audio callback does); reported in the result")
def main(checkpoint, model_gin, runtime_size, batch_size, hop_frames, num_hops, use_fast_newt, graph, static_io, json_out, slots, note_on,
         note_off, seed, output_rate, keep_gc):
    if output_rate is not None and slots:
        raise click.UsageError("--output-rate times the converter behind model.stream(B); it does not combine with --slots")
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    nws.ensure_default_config()
    if model_gin:
        nws.gin.parse_config_file(model_gin)
    if checkpoint is None and model_gin:
        torch.manual_seed(seed)
        model = nws.NeuralWaveshaping().cuda().eval()
    else:
        model = nws.NeuralWaveshaping.load_from_checkpoint(checkpoint or os.path.join(ROOT, "tests", "golden", "weights_vn.npz")).cuda().eval()
    if use_fast_newt:
        model.newt = nws.FastNEWT(model.newt)
    K = hop_frames
    f0 = 220 + 20 * torch.rand(batch_size, 1, K, device="cuda")
    control = torch.randn(batch_size, 2, K, device="cuda")
    rng = np.random.default_rng(seed)

    def events():
        """this hop's (start, stop) slot lists: random note-ons on idle slots, note-offs on active ones"""
        if not slots:
            return {}
        st = s.slot_states()
        start = [b for b, x in enumerate(st) if x == "idle" and rng.random() < note_on]
        stop = [b for b, x in enumerate(st) if x == "active" and rng.random() < note_off]
        return {"start": start, "stop": stop}

    with torch.no_grad():
        st_mod = importlib.import_module("neural-waveshaping-synthesis_amd.streaming")
        if runtime_size:
            s = (st_mod.GenericVoiceStream if slots else st_mod.GenericNewtStream)(model, batch_size, graph=graph)
        else:
            s = model.voices(batch_size, graph=graph) if slots else model.stream(batch_size, graph=graph)
        conv = None
        if output_rate is not None:
            conv = importlib.import_module("neural-waveshaping-synthesis_amd.streaming").StreamResampler(
                int(model.sample_rate), output_rate, batch_size, graph=graph)
        for _ in range(20):
            y = s.push(f0, control, **events())
            if conv is not None:
                conv.push(y)
        if static_io:
            f0_in, c_in = s.static_io(K)[:2]
            f0_in.copy_(f0[:, 0])
            c_in.copy_(control)
            if conv is not None:
                x_in = conv.static_io(K * 128)[0]
        torch.cuda.synchronize()
        import gc
        import time
        lat, wall, lat_conv, lat_both, out_samples = [], [], [], [], 0
        if not keep_gc:
            gc.collect()
            gc.disable()
        n_events = 0
        for _ in range(num_hops):
            ev = events()
            n_events += len(ev.get("start", ())) + len(ev.get("stop", ()))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            y = s.hop(K, **ev) if static_io else s.push(f0, control, **ev)
            e1.record()
            if conv is not None:
                # the hop's samples through the converter on the same stream; e1 splits the pair
                e2 = torch.cuda.Event(enable_timing=True)
                if static_io:
                    x_in.copy_(y)
                    out_samples += conv.hop().shape[1]
                else:
                    out_samples += conv.push(y).shape[1]
                e2.record()
                e2.synchronize()
                lat_conv.append(e1.elapsed_time(e2) * 1e3)
                lat_both.append(e0.elapsed_time(e2) * 1e3)
            else:
                e1.synchronize()
            wall.append((time.perf_counter() - t0) * 1e6)
            lat.append(e0.elapsed_time(e1) * 1e3)
    gc.enable()
    lat, wall = np.array(lat), np.array(wall)
    period = K * 128 / float(model.sample_rate) * 1e6
    res = {"stream": type(s).__name__, "batch": batch_size, "hop_samples": K * 128, "graph": bool(graph), "static_io": bool(static_io), "hops": num_hops, "python_gc": bool(keep_gc),
           "slots": bool(slots), "events": n_events,
           "p50_us": float(np.percentile(lat, 50)), "p99_us": float(np.percentile(lat, 99)), "max_us": float(lat.max()),
           "wall_p50_us": float(np.percentile(wall, 50)), "wall_p99_us": float(np.percentile(wall, 99)),
           "x_realtime_p50": period / float(np.percentile(lat, 50))}
    print(f"{type(s).__name__}: stateful streaming{' (slots, %d events)' % n_events if slots else ''}, batch {batch_size}, hop {K * 128} samples ({period / 1e3:.1f} ms), graph={graph}, static_io={static_io}, gc={keep_gc}: p50 {res['p50_us']:.1f} us  "
          f"p99 {res['p99_us']:.1f} us  (host wall p50 {res['wall_p50_us']:.1f} / p99 {res['wall_p99_us']:.1f} us)  -> "
          f"{res['x_realtime_p50']:.1f}x real-time")
    if conv is not None:
        lat_conv, lat_both = np.array(lat_conv), np.array(lat_both)
        res.update({"output_rate": int(output_rate), "output_samples": int(out_samples),
                    "converter_p50_us": float(np.percentile(lat_conv, 50)), "converter_p99_us": float(np.percentile(lat_conv, 99)),
                    "p50_with_converter_us": float(np.percentile(lat_both, 50)), "p99_with_converter_us": float(np.percentile(lat_both, 99))})
        print(f"  + StreamResampler {int(model.sample_rate)} -> {output_rate} Hz ({'captured hop' if static_io else 'push'}): converter p50 "
              f"{res['converter_p50_us']:.1f} us  p99 {res['converter_p99_us']:.1f} us; hop with converter p50 "
              f"{res['p50_with_converter_us']:.1f} us  p99 {res['p99_with_converter_us']:.1f} us; {out_samples} samples out "
              f"(host wall above includes the converter)")
    if json_out:
        import json
        with open(json_out, "a") as f:
            f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
