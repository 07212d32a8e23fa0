#!/usr/bin/env python
"""Latency of the note player's hop (streaming.NotePlayer.hop: the control launch, the slot stream's captured hop, the mix;
DESIGN.md 3.27) under a random note-on / note-off schedule, HIP-event timed per hop by the method of scripts/time_streaming.py
--slots --static-io.  The bare VoiceStream.hop of the same size is timed in the same call, alternated with the player hop by hop
under a schedule of the same statistics, so that both see the same machine.  Every hop each idle slot gets a note with
probability --note-on and each held note is released with probability --note-off.  Host wall-clock is reported beside the
HIP-event latency.
--model-gin FILE: a model of another architecture (parsed on top of the packaged gin; player and bare stream then run on the
runtime-size slot stream), with the weights of --checkpoint, or seeded random ones when none is named.
--runtime-size: the packaged model on the runtime-size slot stream, to compare the two paths on one set of sizes."""
import gc
import importlib
import json
import os
import sys
import time

import click
import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0 = time.perf_counter()
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3, (time.perf_counter() - t0) * 1e6


@click.command()
@click.option("--checkpoint", default=None, help="default: the packaged weights, or seeded random ones with --model-gin")
@click.option("--model-gin", default=None, help="the model's gin file when it is not the packaged one")
@click.option("--runtime-size", is_flag=True, default=False, help="force the runtime-size slot stream (GenericVoiceStream)")
@click.option("--voices", default="4,16", show_default=True, help="comma-separated voice counts")
@click.option("--hop-frames", default=2, show_default=True)
@click.option("--channels", default=1, type=click.IntRange(1, 2), show_default=True)
@click.option("--num-hops", default=500, show_default=True)
@click.option("--use-fast-newt/--no-fast-newt", default=True)
@click.option("--note-on", default=0.2, show_default=True, help="per-hop probability that an idle slot gets a note")
@click.option("--note-off", default=0.1, show_default=True, help="per-hop probability that a held note is released")
@click.option("--release", default=4, show_default=True, help="release frames of the player's envelope")
@click.option("--seed", default=0)
@click.option("--gc/--no-gc", "keep_gc", default=True, help="--no-gc: Python's cyclic garbage collector off during the timed hops")
@click.option("--json-out", default=None)
def main(checkpoint, model_gin, runtime_size, voices, hop_frames, channels, num_hops, use_fast_newt, note_on, note_off, release, seed,
         keep_gc, json_out):
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    streaming = importlib.import_module("neural-waveshaping-synthesis_amd.streaming")
    nws.ensure_default_config()
    if model_gin:
        nws.gin.parse_config_file(model_gin)
    if checkpoint is None and model_gin:
        torch.manual_seed(seed)
        model = nws.NeuralWaveshaping().cuda().eval()
    else:
        model = nws.NeuralWaveshaping.load_from_checkpoint(checkpoint or os.path.join(ROOT, "tests", "golden", "weights_vn.npz")).cuda().eval()
    checkpoint = checkpoint or os.path.join(ROOT, "tests", "golden", "weights_vn.npz")      # the normalisation statistics
    if use_fast_newt:
        model.newt = nws.FastNEWT(model.newt)
    K = hop_frames
    period = K * 128 / float(model.sample_rate) * 1e6
    z = np.load(checkpoint) if str(checkpoint).endswith(".npz") else {}
    norm = (z["__data_mean__"].reshape(-1), z["__data_std__"].reshape(-1)) if "__data_mean__" in getattr(z, "files", ()) else ([300.0, 0.6], [150.0, 0.15])
    for B in (int(v) for v in voices.split(",")):
        rng = np.random.default_rng(seed)
        with torch.no_grad():
            player = model.player(B, hop_frames=K, channels=channels, normalisation=norm, release=release)
            if runtime_size:
                # the player's stream is what model.voices picks: swap in the runtime-size class before the first hop
                player.stream = streaming.GenericVoiceStream(model, B)
                bare = streaming.GenericVoiceStream(model, B)
            else:
                bare = model.voices(B)
            held = {}

            def player_events():
                for h in [h for h in held if rng.random() < note_off]:
                    player.note_off(h)
                    del held[h]
                for _ in range(sum(1 for s in player.stream.slot_states() if s == "idle" and rng.random() < note_on)):
                    h = player.note_on(float(rng.integers(40, 90)), float(rng.uniform(0.2, 1.0)), float(rng.uniform(-1, 1)))
                    if h is not None:
                        held[h] = True

            def bare_events():
                st = bare.slot_states()
                return {"start": [b for b, x in enumerate(st) if x == "idle" and rng.random() < note_on],
                        "stop": [b for b, x in enumerate(st) if x == "active" and rng.random() < note_off]}

            f0 = 220 + 20 * torch.rand(B, 1, K, device="cuda")
            control = torch.randn(B, 2, K, device="cuda")
            for _ in range(20):
                player_events()
                player.hop()
                bare.push(f0, control, **bare_events())
            f0_in, c_in = bare.static_io(K)[:2]
            f0_in.copy_(f0[:, 0])
            c_in.copy_(control)
            torch.cuda.synchronize()
            if not keep_gc:
                gc.collect()
                gc.disable()
            lat = {"player": [], "bare": []}
            wall = {"player": [], "bare": []}
            for _ in range(num_hops):
                player_events()
                a, w = timed(player.hop)
                lat["player"].append(a)
                wall["player"].append(w)
                ev = bare_events()
                a, w = timed(lambda: bare.hop(K, **ev))
                lat["bare"].append(a)
                wall["bare"].append(w)
            gc.enable()
            player.check()
            dropped = player.dropped
            player.close()
            bare.close()
        res = {"stream": type(bare).__name__, "voices": B, "hop_samples": K * 128, "channels": channels, "hops": num_hops, "python_gc": bool(keep_gc), "dropped": dropped}
        for name in ("player", "bare"):
            res.update({f"{name}_p50_us": float(np.percentile(lat[name], 50)), f"{name}_p99_us": float(np.percentile(lat[name], 99)),
                        f"{name}_max_us": float(np.max(lat[name])), f"{name}_wall_p50_us": float(np.percentile(wall[name], 50)),
                        f"{name}_wall_p99_us": float(np.percentile(wall[name], 99))})
        res["player_p99_over_period"] = res["player_p99_us"] / period
        print(f"NotePlayer.hop, {B} voices, hop {K * 128} samples ({period / 1e3:.1f} ms): p50 {res['player_p50_us']:.1f} us  p99 "
              f"{res['player_p99_us']:.1f} us  (host wall p50 {res['player_wall_p50_us']:.1f} / p99 {res['player_wall_p99_us']:.1f} us) = "
              f"{100 * res['player_p99_over_period']:.1f} % of the hop at p99;  bare {type(bare).__name__}.hop: p50 {res['bare_p50_us']:.1f} us  p99 "
              f"{res['bare_p99_us']:.1f} us  (host wall p50 {res['bare_wall_p50_us']:.1f} / p99 {res['bare_wall_p99_us']:.1f} us)")
        if json_out:
            with open(json_out, "a") as f:
                f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
