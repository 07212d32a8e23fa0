#!/usr/bin/env python
"""Headline benchmark: NEWT forward throughput (audio samples/s, x real-time) on 4 s @ 16 kHz clips.

    python bench.py [--gpus N --steps K --warmup W] [--batch 64] [--frames 500] [--exact] [--gather rccl|copy]
                    [--dump-outputs DIR] [--full]

Contract: a step = one NeuralWaveshaping.forward over a batch of `--batch` synthetic
utterances per GPU (torch.rand F0/control exactly like the reference's scripts/time_forward_pass.py:27-40,
vn checkpoint, FastNEWT LUT), inputs resident in HBM, the two RNG draws of forward() made on the device
inside the step; with N>1 the rendered waveforms are all-gathered (RCCL, or `--gather copy`: copy-engine
peer writes) inside the timed region, overlapped with the next step's kernels.  Prints ONE JSON line on rank 0.

A plain run sets up, primes and warms up, times the K steps and prints the headline line.  `--full` adds everything
else the benchmark measures or checks, outside the timed steps: live per-kernel timing inside the timed region, the
pipeline's bit-exactness self-check, per-stage times, batch-1 and streaming latency, the extra legs, the roofline with
its hardware counters, the CPU baseline and, with N>1, the exchange regions.

`--gpus N` with N > 1 and no WORLD_SIZE in the environment: this process re-executes itself under
`python -m torch.distributed.run --nnodes=1 --nproc-per-node N` (one rank per GPU) after checking that the box HAS N GPUs;
launched by a driver under torch.distributed.run it checks WORLD_SIZE == N.  A mismatch is an error, never a silent
single-GPU run.
"""
import argparse
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import time

# the pipeline keeps 2 audio + 1 control stream busy next to torch's default stream and, for N > 1, RCCL's own streams; HIP maps
# streams onto 4 hardware queues by default and streams that share a queue serialise (measured: 0.75 vs 0.59 ms per step with
# RCCL initialised).  Must be set before the HIP runtime starts.
os.environ.setdefault("GPU_MAX_HW_QUEUES", "16")
os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")   # dmabuf IPC: RCCL / peer-mapped buffers across processes

import numpy as np  # noqa: E402
import torch  # noqa: E402

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

# ---- algorithmic work per launch: what `achieved` divides by the live kernel time ----
# exciter_newt_kernel: harmonic mixer 2*64*101 flop/sample + 101 sines (5 flop each) + FiLM lerp/FiLM/LUT/mix ~ 24 flop per
# (sample, shaper)
FLOP_PER_SAMPLE_EXCITER_NEWT = 2 * 64 * 101 + 101 * 5 + 64 * 24
# fp16 MFMA work the kernel issues per sample: (terms) MFMAs of 64 shapers x 112 K slots, + 6 bf16 MFMAs of 32x32x16 per 32
# samples for the FiLM interpolation
def exciter_mfma_flop_per_sample(terms, film_mfma):
    return terms * 2 * 64 * 112 + (6 * 2 * 32 * 32 * 16 / 32.0 if film_mfma else 0.0)


FLOP_PER_FRAME_MLPS = 2 * (128 * 128 + 3 * 128 * 128 + 256 * 128 + 3 * 128 * 128 + 129 * 128 + 128 * 132)   # proj, 2 MLPs, FIR design (upper half-taps)
FLOP_PER_STEP_GRU = 2 * (384 * 128 + 384 * 2)           # per utterance and control frame
FLOP_PER_FRAME_NOISE = 2 * 256 * 512                    # two overlapping 256-tap circular convolutions per output hop
PEAK_F16_MFMA_TFLOPS = 2500.0   # MI355X_MICROARCH.md: dense fp16/bf16 MFMA peak
PEAK_FP32_VALU_TFLOPS = 157.3   # MI355X_MICROARCH.md: fp32 vector peak
PEAK_HBM_TBS = 8.0              # MI355X_MICROARCH.md: HBM3E spec peak (6.3 achievable)
MAX_CLOCK_GHZ = 2.4
N_SIMD = 1024
FIR_ROW_FLOATS = 128     # floats per (utterance, frame) handed from the frame MLPs to the noise kernel (upper half of the mirror-symmetric taps)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--batch", type=int, default=64, help="utterances per GPU (weak scaling: fixed per-GPU work)")
    ap.add_argument("--frames", type=int, default=500, help="control frames per utterance (500 = 4 s @ 16 kHz)")
    ap.add_argument("--exact", action="store_true", help="exact sin-MLP shapers instead of the FastNEWT LUT")
    ap.add_argument("--inputs", choices=("rand", "realistic"), default="rand",
                    help="rand: torch.rand F0/control exactly like scripts/time_forward_pass.py (sub-1 Hz 'F0': all 101 harmonics "
                         "live, the worst case for the oscillator); realistic: per-utterance F0 ~ U[100, 1000] Hz with 5.5 Hz "
                         "vibrato, control ~ N(0,1) (SURVEY 8(d) config 3)")
    ap.add_argument("--exciter-opts", type=int, default=None,
                    help="NwsWeights.exciter_opts (include/nws_hip.h): default auto (0 unless a worst-case bound admits 8, Engine.exciter_opts); 0 every "
                         "product two-term, 1 round-1 VALU FiLM, 2 one-term sines everywhere, 4 one-term sines for harmonics >= 16, "
                         "8 one-term sines AND weights for harmonics >= 16")
    ap.add_argument("--gather", choices=("rccl", "copy"), default="rccl",
                    help="N > 1: how the rendered waveforms are all-gathered: rccl = all_gather_into_tensor (RCCL kernels on the "
                         "CUs); copy = every rank pushes its shard into every peer's buffer with device-to-device copies on "
                         "peer-mapped memory (copy engines over xGMI, no collective kernels; parallel.PeerCopyAllGather)")
    ap.add_argument("--gather-chunks", type=int, default=1,
                    help="N > 1: push the rendered waveforms in this many sub-batches (4 = 4 x 16 utterances), each as soon as ITS "
                         "reverb has been enqueued, instead of one all-gather after the whole batch (SURVEY 8(e))")
    ap.add_argument("--gather-slots", type=int, default=8,
                    help="N > 1: gather buffers in rotation (>= the workspace ring); the submitting thread runs at most this many "
                         "batches ahead of the GPU, because a buffer is only free once its exchange has been issued")
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--cpu-seconds", type=float, default=25.0, help="time budget of the cpu_baseline leg")
    ap.add_argument("--batch1-iters", type=int, default=200)
    ap.add_argument("--streams", type=int, default=2,
                    help="audio streams of the pipeline (or, with --pipeline 0, streams that whole forwards are issued on "
                         "round-robin).  Two overlap the tail of batch i with the head of batch i+1 (~7 %%); this is the "
                         "configuration that exposed the packed-fp32 / MFMA co-execution hazard the build now guards against "
                         "(DESIGN.md 5.3, LABBOOK.md '5.2') - the self-check below compares it with the plain forward bit for bit")
    ap.add_argument("--depth", type=int, default=0, help="workspaces in flight (0: streams + 2)")
    ap.add_argument("--pipeline", type=int, default=1,
                    help="1: ForwardPipeline (control half = carries + GRU of batch i+1 on a side stream under the audio "
                         "half of batch i, --streams audio streams); 0: whole forwards round-robin on --streams streams")
    ap.add_argument("--control-streams", type=int, default=0,
                    help="side streams for the control half; 0 = two (one control stream carries recurrence + its wait for compute units, "
                         "~0.44 ms per batch, and bounds the step: 0.443-0.449 against 0.401-0.403 ms with two, round 6)")
    ap.add_argument("--chain-exciters", type=int, default=0,
                    help="1: the oscillator kernels of neighbouring batches (two audio streams) run one after the other, the other "
                         "kernels overlap them (ForwardPipeline chain_exciters; measured: no difference, 0.3919 vs 0.3932 ms/step)")
    ap.add_argument("--gru", choices=("batched", "per-utterance"), default="per-utterance",
                    help="GRU kernel of the pipeline's control half (the plain forward always uses per-utterance)")
    ap.add_argument("--legs", type=int, default=1,
                    help="1 (default, N = 1 only): after the headline region, time short extra legs of the same issue pattern and "
                         "report them under `legs`: two_term (every mixer product 22-bit: the default arithmetic), hybrid_w (opt-in "
                         "fp16 x fp16 products for harmonics 16..101), realistic_inputs, exact (sin-MLP shapers)")
    ap.add_argument("--leg-steps", type=int, default=200,
                    help="steps per extra leg (each leg is primed like the headline region; the exact-shaper leg runs a third of them)")
    ap.add_argument("--pmc", choices=("auto", "live", "file", "off"), default="auto",
                    help="where the roofline's hardware counters come from: live = rocprofv3 --pmc passes over a child process of "
                         "this script (FETCH_SIZE, WRITE_SIZE, SQ counters: separate passes, never combined with traces); file = "
                         "the committed profiles/<round>/pmc_kernels.json; auto = live when rocprofv3 is on the box, else file")
    ap.add_argument("--pmc-child", type=int, default=0, help=argparse.SUPPRESS)   # internal: the workload the PMC passes profile
    ap.add_argument("--full", action="store_true",
                    help="measure and check everything besides the headline (see the module docstring); --no-cpu-baseline, "
                         "--cpu-seconds, --batch1-iters, --legs, --leg-steps and --pmc shape what it adds")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the last timed step returned as DIR/waveforms.npy (float32, B x N; "
                         "N > 1: rank 0's gathered batch of every rank).  Beyond 64 MB a fixed, seeded sample of its rows")
    return ap.parse_args()


DUMP_LIMIT_BYTES = 64 * 10 ** 6 - 4096     # --dump-outputs: 64 MB in all, .npy headers included


def dump_outputs(out_dir, arrays):
    """--dump-outputs: every array as out_dir/<name>.npy in float32, DUMP_LIMIT_BYTES in all (arrays are 2-D (rows, samples);
    one beyond its share is cut to a seeded sample of rows, kept in their original order)"""
    os.makedirs(out_dir, exist_ok=True)
    limit = DUMP_LIMIT_BYTES // len(arrays)
    for name, x in arrays.items():
        x = np.ascontiguousarray(x, dtype=np.float32)
        if x.nbytes > limit:
            keep = max(1, limit // (x.shape[1] * 4))
            rows = np.sort(np.random.default_rng(0).choice(x.shape[0], size=min(keep, x.shape[0]), replace=False))
            x = x[rows]
            if x.nbytes > limit:       # a single row beyond the limit: a seeded sample of its samples
                cols = np.sort(np.random.default_rng(1).choice(x.shape[1], size=limit // 4, replace=False))
                x = x[:, cols]
        np.save(os.path.join(out_dir, name + ".npy"), x)


def launch_ranks(a):
    """`python bench.py --gpus N` typed by hand / by a driver that does not use torchrun: become N ranks."""
    have = torch.cuda.device_count()
    if have < a.gpus:
        print(f"bench.py: --gpus {a.gpus} needs {a.gpus} GPUs, this box has {have}; refusing to time fewer GPUs than asked for",
              file=sys.stderr)
        sys.exit(2)
    port = 29400 + os.getpid() % 500
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *sys.argv[1:]]
    sys.exit(subprocess.run(cmd).returncode)


def _time_oracle(o, f0, control, budget_s, max_iters):
    for _ in range(2):
        o(f0, control)
    ts, t_end = [], time.time() + budget_s
    while len(ts) < max_iters and (time.time() < t_end or len(ts) < 2):
        t0 = time.time()
        o(f0, control)
        ts.append(time.time() - t0)
    return float(np.mean(ts)), len(ts)


def cpu_baseline(weights_path, T, budget_s):
    """The oracle (op-for-op torch-CPU restatement of the reference forward, python LUT loop included) timed on the host
    cores, protocol of scripts/time_forward_pass.py: B=1, torch.rand inputs; intra-op thread sweep (128
    threads on 64 000-element ops thrash: the best count is reported), FastNEWT and exact NEWT, plus one B=16 call."""
    from oracle.newt_oracle import OracleNEWT, load_weights_npz

    w = {k: v for k, v in load_weights_npz(weights_path).items() if not k.startswith("__")}
    fast = OracleNEWT(w, fast=True, lut_python_loop=True)
    exact = OracleNEWT(w, fast=False)
    torch.manual_seed(0)
    f0, control = torch.rand(1, 1, T), torch.rand(1, 2, T)
    ncpu = os.cpu_count() or 1
    default_threads = torch.get_num_threads()
    sweep = {}
    for nt in sorted({1, 4, 8, 16, 32, min(64, ncpu), default_threads}):
        if nt > ncpu:
            continue
        torch.set_num_threads(nt)
        sweep[nt] = _time_oracle(fast, f0, control, budget_s * 0.06, 4)[0]
    best = min(sweep, key=sweep.get)
    torch.set_num_threads(best)
    mean, n = _time_oracle(fast, f0, control, budget_s * 0.35, 100)
    mean_exact, n_exact = _time_oracle(exact, f0, control, budget_s * 0.2, 20)
    fb, cb = torch.rand(16, 1, T), torch.rand(16, 2, T)
    t0 = time.time()
    fast(fb, cb)
    t_b16 = time.time() - t0
    # "B=64 as 64 x B=1 and as one B=64 call" - one real call (about 4x the B=16 one, ~7 s)
    fb, cb = torch.rand(64, 1, T), torch.rand(64, 2, T)
    t0 = time.time()
    fast(fb, cb)
    t_b64 = time.time() - t0
    torch.set_num_threads(default_threads)
    cpu_model = "?"
    try:
        cpu_model = next(l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name"))
    except Exception:
        pass
    dur = 128 * T / 16000.0
    return {"value": 128 * T / mean, "unit": "samples/s", "cores": best, "kind": "port",
            "sample": f"{n} forwards of B=1, T={T} (4 s) FastNEWT (reference's python LUT loop), torch.rand inputs, "
                      f"oracle/newt_oracle.py, torch {torch.__version__} CPU, best of a thread sweep",
            "ms_per_utterance": mean * 1e3, "x_realtime": dur / mean, "rtf_mean": mean / dur,
            "cpu_model": cpu_model, "logical_cpus": ncpu, "torch_default_threads": default_threads,
            "thread_sweep_ms_per_utterance": {str(k): round(v * 1e3, 2) for k, v in sorted(sweep.items())},
            "exact_newt_b1": {"ms_per_utterance": mean_exact * 1e3, "samples_per_s": 128 * T / mean_exact,
                              "x_realtime": dur / mean_exact, "forwards": n_exact},
            "fastnewt_b64_as_64_sequential_b1": {"ms": 64 * mean * 1e3, "samples_per_s": 128 * T / mean},
            "fastnewt_one_b16_call": {"ms": t_b16 * 1e3, "samples_per_s": 16 * 128 * T / t_b16},
            "fastnewt_one_b64_call": {"ms": t_b64 * 1e3, "samples_per_s": 64 * 128 * T / t_b64, "calls": 1,
                                      "note": "the workload of the GPU headline (one B=64 forward) as ONE call of the port: the "
                                              "reference's throughput FALLS with batch (python LUT loop, BASELINE.md section 2)"}}


def load_pmc():
    """Per-kernel counters of the round's committed rocprofv3 --pmc passes (tools/collect_profiles.sh + tools/pmc_digest.py)."""
    for rnd in ("r06", "r05", "r04", "r03", "r02", "r01"):
        path = os.path.join(ROOT, "profiles", rnd, "pmc_kernels.json")
        if os.path.exists(path):
            try:
                return json.load(open(path)), f"profiles/{rnd}/pmc_kernels.json (committed file)"
            except Exception:
                pass
    return None, None


PMC_PASSES = (   # separate passes (MI355X_MICROARCH.md, rocprofv3 PMC slots: FETCH_SIZE costs 3 of the 4 TCC slots, WRITE_SIZE 2)
    ("sq", ["SQ_WAVES", "SQ_INSTS_VALU", "SQ_INSTS_MFMA", "SQ_INSTS_VALU_TRANS_F32", "SQ_WAVE_CYCLES", "SQ_ACTIVE_INST_VALU",
            "SQ_WAIT_ANY", "SQ_WAIT_INST_ANY", "GRBM_GUI_ACTIVE"]),
    ("fetch", ["FETCH_SIZE"]),
    ("write", ["WRITE_SIZE"]),
)


def _short_kernel(name):
    import re
    name = re.sub(r"\(anonymous namespace\)::", "", name)
    name = re.sub(r"^void ", "", name)
    return re.sub(r"[<(].*", "", name)


def collect_pmc_live(a, stage_ns):
    """rocprofv3 --pmc over a child of this script (`--pmc-child n`: n plain forwards of the bench workload on one stream),
    one pass per counter group, counters only (never combined with a trace).  Returns the structure of
    profiles/<round>/pmc_kernels.json, or (None, reason)."""
    import csv
    import glob
    import shutil
    import tempfile
    from collections import defaultdict

    exe = shutil.which("rocprofv3") or ("/opt/rocm/bin/rocprofv3" if os.path.exists("/opt/rocm/bin/rocprofv3") else None)
    if exe is None:
        return None, "rocprofv3 not on this box"
    child = [sys.executable, os.path.abspath(__file__), "--pmc-child", "4", "--batch", str(a.batch), "--frames", str(a.frames)]
    if a.exact:
        child.append("--exact")
    if a.exciter_opts is not None:
        child += ["--exciter-opts", str(a.exciter_opts)]
    if a.inputs != "rand":
        child += ["--inputs", a.inputs]
    env = dict(os.environ, TMPDIR="/tmp")
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    merged = defaultdict(lambda: defaultdict(list))
    t_all = time.time()
    with tempfile.TemporaryDirectory(dir="/tmp") as td:
        for tag, ctrs in PMC_PASSES:
            out = os.path.join(td, tag)
            try:
                r = subprocess.run([exe, "--output-format", "csv", "--pmc", *ctrs, "-d", out, "--", *child], cwd="/tmp", env=env,
                                   capture_output=True, text=True, timeout=240)
            except subprocess.TimeoutExpired:
                return None, f"rocprofv3 pass '{tag}' timed out"
            if r.returncode != 0:
                return None, f"rocprofv3 pass '{tag}' failed ({r.returncode}): {r.stderr[-300:]}"
            for path in glob.glob(os.path.join(out, "**", "*counter_collection.csv"), recursive=True):
                for row in csv.DictReader(open(path)):
                    merged[_short_kernel(row["Kernel_Name"])][row["Counter_Name"]].append(float(row["Counter_Value"]))
    if not merged:
        return None, "rocprofv3 wrote no counter_collection.csv"
    kernels = {}
    for k, c in merged.items():
        m = {n: sum(v) / len(v) for n, v in c.items()}
        w = m.get("SQ_WAVES", 0) or 1
        e = {"waves": w, "valu_insts_per_wave": m.get("SQ_INSTS_VALU", 0) / w, "mfma_insts_per_wave": m.get("SQ_INSTS_MFMA", 0) / w,
             "trans_insts_per_wave": m.get("SQ_INSTS_VALU_TRANS_F32", 0) / w,
             "valu_active_quad_cycles_per_wave": m.get("SQ_ACTIVE_INST_VALU", 0) / w,
             "wave_quad_cycles_per_wave": m.get("SQ_WAVE_CYCLES", 0) / w,
             "wait_any_frac_of_wave_cycles": m.get("SQ_WAIT_ANY", 0) / (m.get("SQ_WAVE_CYCLES", 0) or 1),
             "wait_inst_frac_of_wave_cycles": m.get("SQ_WAIT_INST_ANY", 0) / (m.get("SQ_WAVE_CYCLES", 0) or 1)}
        if "FETCH_SIZE" in m and "WRITE_SIZE" in m:
            e["fetch_kb"], e["write_kb"] = m["FETCH_SIZE"], m["WRITE_SIZE"]
            e["hbm_bytes_per_launch"] = (2.0 * m["FETCH_SIZE"] + m["WRITE_SIZE"]) * 1024.0   # gfx950: FETCH_SIZE x2 (MICROARCH guide)
        ns, gui = stage_ns.get(k), m.get("GRBM_GUI_ACTIVE")
        if ns and gui:
            if gui / ns > 4.0:          # > 4 GHz: the counter is a sum over the 8 XCDs
                gui /= 8.0
            if 1.0 <= gui / ns <= 2.6:
                e.update(kernel_cycles=gui, clock_ghz_during_pass=gui / ns,
                         valu_busy_frac=w * e["valu_active_quad_cycles_per_wave"] * 4.0 / (1024.0 * gui))
        kernels[k] = e
    return ({"source": "rocprofv3 --pmc inside this bench run (child process, one stream, 4 forwards per pass; passes: "
                       + ", ".join(t for t, _ in PMC_PASSES) + ")", "batch_per_gpu": a.batch, "frames": a.frames,
             "seconds": round(time.time() - t_all, 1),
             "correction": "FETCH_SIZE doubled (gfx950 reports half the bytes of wide coalesced reads, MI355X_MICROARCH.md HBM "
                           "section); WRITE_SIZE as reported", "kernels": kernels},
            "rocprofv3 --pmc, live in this run")


# algorithmic HBM bytes per launch at (B, T): what a kernel MUST move given the stage boundaries of this design (DESIGN.md
# section 4); `traffic` (PMC) over this is the wasted-traffic ratio
def hbm_algorithmic_bytes(B, T):
    N = 128 * T
    return {
        # f0 frames + FiLM rows (B,T,256) in, carries (B, N/32) f64 in, fragment + pair tables (28 KB + 2 MB, shared), the noise
        # branch (B,N) in, newt + noise (B,N) out
        "exciter_newt_kernel": 4 * B * T + 1024 * B * T + 8 * B * N // 32 + 28672 + 2 * 64 * 4096 * 4 + 2 * 4 * B * N,
        "control_gru_kernel": 8 * B * T + 512 * B * T + 384 * 131 * 4,                 # control in, gru_out (B,T,128) out, weights
        # gru_out in (read by both path workgroups: the second read hits L2), the 712 KB fragment table, film + noise-filter rows out
        "frame_mlps_wr_kernel": 512 * B * T + 729088 + 1024 * B * T + 4 * B * T * FIR_ROW_FLOATS,
        "fir_noise_mfma_kernel": 4 * B * T * FIR_ROW_FLOATS + 4 * N + 4 * B * N,      # filter rows in, noise in, noise branch out
        # four-step FFT, two utterances per complex transform: x read by the forward column pass and again for the dry add, the
        # (re, im) planes of B/2 transforms written once, read + written by the row pass, read by the inverse column pass, y out
        "reverb": 7 * 4 * B * N,
    }


def kernel_roofline(name, pmc, ms, algo_flop=None, mfma_flop=None, hbm_note=None):
    """One roofline entry: what bounds the kernel and how close it runs to that bound."""
    e = {"kernel": name, "kernel_ms": ms}
    ks = (pmc or {}).get("kernels", {})
    k = ks.get(name)
    if k is None and name == "frame_mlps_wr_kernel":      # smaller batches run the tile kernels (csrc/frame_mlps.hip)
        k = ks.get("frame_mlps64_kernel") or ks.get("frame_mlps16_kernel")
    if algo_flop is not None and ms:
        e["algorithmic_tflops"] = algo_flop / (ms * 1e-3) / 1e12
    if mfma_flop is not None and ms:
        t = mfma_flop / (ms * 1e-3) / 1e12
        e["mfma_f16_executed"] = {"achieved": t, "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s", "frac": t / PEAK_F16_MFMA_TFLOPS}
    if k:
        busy_cycles = k["waves"] * k["valu_active_quad_cycles_per_wave"] * 4.0     # VALU-busy SIMD-cycles per launch
        if ms:
            rate = busy_cycles / (ms * 1e-3)
            e["valu_issue"] = {"achieved": rate / 1e9, "peak": N_SIMD * MAX_CLOCK_GHZ, "unit": "G VALU-busy SIMD-cycles/s",
                               "frac": rate / (N_SIMD * MAX_CLOCK_GHZ * 1e9),
                               "frac_at_clock_of_pmc_pass": k.get("valu_busy_frac"),
                               "insts_per_wave": {"valu": round(k["valu_insts_per_wave"], 1), "trans": round(k["trans_insts_per_wave"], 1),
                                                  "mfma": round(k["mfma_insts_per_wave"], 1)}}
        if k.get("hbm_bytes_per_launch") and ms:
            e["hbm"] = {"traffic": k["hbm_bytes_per_launch"], "achieved": k["hbm_bytes_per_launch"] / (ms * 1e-3) / 1e12,
                        "peak": PEAK_HBM_TBS, "unit": "TB/s", "frac": k["hbm_bytes_per_launch"] / (ms * 1e-3) / 1e12 / PEAK_HBM_TBS}
    if hbm_note:
        e["note"] = hbm_note
    return e


def pmc_child(a):
    """The workload the PMC passes profile: n plain forwards of the bench shape on ONE stream (no pipeline, no JSON)."""
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    nws.ensure_default_config()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    model = nws.NeuralWaveshaping.load_from_checkpoint(os.path.join(ROOT, "tests", "golden", "weights_vn.npz")).to(dev).eval()
    if not a.exact:
        model.newt = nws.FastNEWT(model.newt)
    if a.exciter_opts is not None:
        model.exciter_opts = a.exciter_opts
    f0, control = make_inputs(a, dev, 0)
    with torch.no_grad():
        for _ in range(2 + a.pmc_child):
            model(f0, control)
    torch.cuda.synchronize()


def make_inputs(a, dev, r, kind=None):
    B, T = a.batch, a.frames
    g = torch.Generator(device=dev).manual_seed(1000 + r)
    if (kind or a.inputs) == "rand":
        f0_ = torch.rand(B, 1, T, device=dev, generator=g)         # time_forward_pass.py:34-40
        control_ = torch.rand(B, 2, T, device=dev, generator=g)    # time_forward_pass.py:27-33
    else:
        tt = torch.arange(T, device=dev, dtype=torch.float32) * (128.0 / 16000.0)
        base = 100.0 + 900.0 * torch.rand(B, 1, 1, device=dev, generator=g)
        f0_ = (base * (1.0 + 0.01 * torch.sin(2 * np.pi * 5.5 * tt).view(1, 1, T))).contiguous()
        control_ = torch.randn(B, 2, T, device=dev, generator=g)
    return f0_, control_


def time_leg(model, f0, control, steps, warmup, audio_streams, control_streams):
    """A short leg of the headline's issue pattern (ForwardPipeline, same stream counts) for another model variant / input
    kind: ms per step, bracketed by synchronize on both sides like the headline region (fill and drain inside)."""
    pmod = importlib.import_module("neural-waveshaping-synthesis_amd.pipeline")
    pipe = pmod.ForwardPipeline(model, depth=audio_streams + 2, audio_streams=audio_streams, control_streams=control_streams)
    with torch.no_grad():
        for _ in range(max(2 * len(pipe.slots) + 2, 60) + warmup):      # primed like the headline region: steady state when the clock starts
            pipe.submit(f0, control)
        pipe.synchronize()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(steps):
            pipe.submit(f0, control)
        pipe.synchronize()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0
    return el / steps * 1e3


class Hooks:
    """Where a diagnosis tool may reach into the run (tools/world1_diag.py subclasses this and calls main(hooks=...)); the bench
    itself runs with the no-op defaults - no diagnosis switch lives in this file."""

    def before_model(self, dev, distributed):
        """after the process group (if any) is up, before the model and the pipeline exist"""

    def after_setup(self, dev, xchg, peer):
        """the pipeline, the exchange worker and the peer-copy object exist"""

    def post_behind(self, xchg, slot_i, ev, issue):
        """called instead of xchg.post(slot_i, ev, issue) when it returns True"""
        return False

    def around_timed(self):
        """context manager around the enqueue loop of every timed region"""
        import contextlib
        return contextlib.nullcontext()

    def extra(self, extra, steps, xchg, peer):
        """add fields to the JSON line (rank 0, after the headline region)"""


def main(hooks=None):
    hooks = hooks or Hooks()
    a = parse()
    if a.pmc_child:
        pmc_child(a)
        return
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and a.gpus > 1 and os.environ.get("NWS_BENCH_SHARE_GPU") != "1":
        launch_ranks(a)
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    assert torch.cuda.is_available(), "bench.py needs the MI355X (no CPU fallback for the product path)"
    # NWS_BENCH_FORCE_DIST=1: run the N>1 code path (RCCL init, shared draws, all-gather) with world_size 1 -- the only way
    # to exercise it on real RCCL on a 1-GPU box.  Never set by the driver.
    force_dist = os.environ.get("NWS_BENCH_FORCE_DIST") == "1"
    # NWS_BENCH_FAKE_PEERS=7 (rehearsal of the 8-rank queue population on ONE GPU, VERDICT r5 #1b; never set by the driver): forced
    # world size 1 with `--gather copy`, every step's 16.4 MB shard pushed to that many LOCAL buffers on per-peer copy streams of
    # their own - the stream count and issue pattern of --gpus 8, blit kernels standing in for the copy engines
    fake_peers = int(os.environ.get("NWS_BENCH_FAKE_PEERS", "0"))
    if fake_peers:
        force_dist = True
        a.gather = "copy"
    # NWS_BENCH_SHARE_GPU=1 (smoke-testing the N>1 code path on a 1-GPU box with TWO processes): every rank uses cuda:0 and
    # the collectives go through gloo (RCCL refuses two ranks on one device).  Never set by the driver.
    share_gpu = os.environ.get("NWS_BENCH_SHARE_GPU") == "1"
    if world != a.gpus and not (force_dist and world == 1) and not share_gpu:
        print(f"bench.py: launched with WORLD_SIZE={world} but --gpus {a.gpus}: the two must agree", file=sys.stderr)
        sys.exit(2)
    if share_gpu:
        local_rank = 0
    elif torch.cuda.device_count() <= local_rank:
        print(f"bench.py: rank {rank} wants cuda:{local_rank}, this box has {torch.cuda.device_count()} GPUs", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    # the forward's two RNG draws come from the device's default generator (N = 1): seeded, so that equal arguments give equal
    # draws from run to run (torch seeds its default generators differently in every process)
    torch.cuda.manual_seed(2000 + rank)
    distributed = world > 1 or force_dist
    if distributed:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        if share_gpu:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=dev)
        assert dist.get_world_size() == world, (dist.get_world_size(), world)
    hooks.before_model(dev, distributed)
    nws = importlib.import_module("neural-waveshaping-synthesis_amd")
    _lib = importlib.import_module("neural-waveshaping-synthesis_amd._lib")
    par = importlib.import_module("neural-waveshaping-synthesis_amd.parallel")
    nws.ensure_default_config()
    wpath = os.path.join(ROOT, "tests", "golden", "weights_vn.npz")
    model = nws.NeuralWaveshaping.load_from_checkpoint(wpath).to(dev).eval()
    if not a.exact:
        model.newt = nws.FastNEWT(model.newt)
    if a.exciter_opts is not None:
        model.exciter_opts = a.exciter_opts
        model.invalidate_cache()
    opts = model._engine.exciter_opts()

    B, T = a.batch, a.frames
    N = 128 * T
    f0, control = make_inputs(a, dev, rank)

    # NWS_BENCH_PRE_STREAMS=k (tools/scale_check.py; never set by the driver): k streams created AND used before the pipeline exists -
    # a process with a history of hardware queues; the measured placement (pipeline.placed_streams) has to absorb it
    pre_streams = [torch.cuda.Stream(device=dev) for _ in range(int(os.environ.get("NWS_BENCH_PRE_STREAMS", "0")))]
    for ps in pre_streams:
        with torch.cuda.stream(ps):
            f0.add_(0.0)
        ps.synchronize()
    n_audio = max(1, a.streams)
    streams = [torch.cuda.Stream(device=dev) for _ in range(n_audio)] if not a.pipeline else []
    shared_gen = par.make_shared_generator(dev) if distributed else None   # same draws on every rank, no broadcast
    use_pipe = bool(a.pipeline)
    pipe = None
    if use_pipe:
        pmod = importlib.import_module("neural-waveshaping-synthesis_amd.pipeline")
        n_control = a.control_streams if a.control_streams > 0 else 2
        pipe = pmod.ForwardPipeline(model, depth=a.depth if a.depth > 0 else n_audio + 2,
                                    audio_streams=n_audio, control_streams=n_control, batched_gru=a.gru == "batched",
                                    chain_exciters=bool(a.chain_exciters))
        streams = pipe.audio
    # gather buffers: a ring of its own (not the workspace ring): a buffer is free again once its exchange is out, and the
    # submitting thread may run at most this many batches ahead of the GPU (parallel.CompletionDrivenExchange)
    nbuf = max(len(pipe.slots), a.gather_slots) if (use_pipe and distributed) else (len(pipe.slots) if use_pipe else len(streams))
    full, peer = None, None
    gather_kind = a.gather if distributed else None
    # (two smoke-test ranks on ONE device, where RCCL refuses to initialise: the peer-copy form, unless
    # NWS_BENCH_SHARE_GPU_COLLECTIVE=1 asks for the collective form on gloo - the in-place all_gather_into_tensor of the RCCL branch,
    # world size 2, host-staged by gloo)
    share_collective = share_gpu and os.environ.get("NWS_BENCH_SHARE_GPU_COLLECTIVE") == "1" and a.gather == "rccl"
    if distributed and (a.gather == "copy" or (share_gpu and not share_collective)):
        # copy-engine all-gather: peer-mapped gather buffers, one device-to-device copy per peer
        n_dest = world + (fake_peers if world == 1 else 0)
        # the per-destination copy streams: hardware queues that do not share a pipe with an audio stream (pipeline.side_streams;
        # NWS_BENCH_COPY_STREAMS=plain: fresh streams wherever they land, for the A/B)
        placed_copy = use_pipe and n_dest > 1 and not share_gpu and os.environ.get("NWS_BENCH_COPY_STREAMS", "placed") == "placed"
        peer = par.PeerCopyAllGather(B, N, dev, nbuf=nbuf, sync_signal=use_pipe, fake_peers=fake_peers if world == 1 else 0,
                                     copy_streams=pmod.side_streams(dev, n_dest) if placed_copy else None,
                                     fake_rows=int(os.environ.get("NWS_BENCH_FAKE_ROWS", "0")))
        full = peer.full
        gather_kind = "copy"
    elif distributed:
        full = [torch.empty((B * world, N), dtype=torch.float32, device=dev) for _ in range(nbuf)]
        if share_collective:
            gather_kind = "rccl branch on gloo"

    blocks = pmod.ForwardPipeline.row_blocks(B, a.gather_chunks) if (distributed and use_pipe) else None
    # N > 1 with the pipeline: every exchange is issued by a helper thread, on its own stream, once the HOST has seen its batch
    # complete (no hardware queue parked on a cross-queue barrier: +30 % per step with nothing to send otherwise, LABBOOK round 5)
    xchg = par.CompletionDrivenExchange(dev, nbuf, stream=pipe.exchange) if (distributed and use_pipe) else None
    hooks.after_setup(dev, xchg, peer)

    def issue_whole(i, y):
        """worker thread, exchange stream current: this step's waveforms to every rank (the timed loop never reads the gathered
        rows, so a peer-copy slot is released at once)"""
        if peer is not None:
            peer.gather(y, i % nbuf)
            peer.release(i % nbuf, used=False)     # nothing reads the gathered rows here: no event to record (time-neutral, measured)
        else:
            par.gather_full(full[i % nbuf], y, async_op=False)        # sync op = launched on the current (exchange) stream
        return y          # kept alive by the exchange's ticket until the slot is acquired again (CompletionDrivenExchange docstring)

    def issue_block(i, y, row0, n, last):
        """worker thread: rows [row0, row0 + n) of this step's waveforms to every rank"""
        if peer is not None:
            peer.push_rows(y, i % nbuf, row0, n)
            if last:
                peer.finish(i % nbuf)
                peer.release(i % nbuf)
        else:       # one all_gather_into_tensor per block into the block-major gather buffer (parallel.gather_block_major)
            par.gather_block_major(full[i % nbuf], y, row0 // n, len(blocks), async_op=False)

    # sub-batch exchange: one event per (gather buffer, row block), recorded by the library behind the block's reverb
    blk_events = [[torch.cuda.Event() for _ in blocks] for _ in range(nbuf)] if blocks is not None else None

    def issue_blocks(i, y, evs):
        """worker thread: every row block of this step's waveforms, each as soon as the host has seen its reverb complete"""
        for q, (row0, n) in enumerate(blocks):
            evs[q].synchronize()
            issue_block(i, y, row0, n, row0 + n == B)
        return y          # rendered out of place from the audio stream's pool: the ticket keeps it alive until the exchange is over

    def post_behind(stream, slot_i, issue):
        """the exchange `issue` leaves once everything enqueued on `stream` so far is complete"""
        ev = torch.cuda.Event()
        ev.record(stream)
        if hooks.post_behind(xchg, slot_i, ev, issue):
            return
        xchg.post(slot_i, ev, issue)

    def gather(i, y):
        """(whole forwards round-robin, --pipeline 0) all-gather of this step's waveforms on the CURRENT stream; work handle"""
        if peer is not None:
            work = peer.gather(y, i % nbuf)[1]
            peer.release(i % nbuf)
            return work
        return par.gather_full(full[i % nbuf], y)

    # --dump-outputs at N = 1: the batch each step returns is kept until the next step replaces it (N > 1: the gather buffers)
    last_y = {} if (a.dump_outputs and not distributed) else None

    def step(i, pending, do_gather=True, do_compute=True, plain=False):
        if use_pipe:
            if not distributed or plain:
                y = pipe.submit(f0, control)    # the single-GPU issue pattern (also timed beside the N > 1 one: world1_overhead)
                if last_y is not None:
                    last_y["y"] = y
                return None
            slot_i = i % nbuf
            if not do_compute:
                # exchange alone: a resident (B, N) shard leaves every step, same messages, nothing to wait for
                xchg.acquire(slot_i)
                if blocks is not None:
                    for row0, n in blocks:
                        xchg.post(slot_i, None, lambda _i=i, _r=row0, _n=n: issue_block(_i, gather_src, _r, _n, _r + _n == B))
                else:
                    xchg.post(slot_i, None, lambda _i=i: issue_whole(_i, gather_src))
                return None
            au = pipe.next_audio_stream()       # the audio stream submit() is about to use for this batch
            # the gather buffer is free once ITS previous exchange is out: the host waits until that one has been issued (i.e. its
            # batch was complete), the audio stream waits for its completion (usually long over: a satisfied wait)
            with torch.cuda.stream(au):
                xchg.acquire(slot_i, au)
                dst = peer.local_rows(slot_i) if peer is not None else full[slot_i][rank * B:(rank + 1) * B]
            # the two draws inside submit(), from the generator every rank seeded identically: the same issue
            # pattern as the single-GPU run, nothing but the exchange added
            if blocks is not None and do_gather:
                # sub-batch exchange: block q leaves as soon as the host has seen ITS reverb complete, under the reverb of
                # block q + 1.  ONE op call renders the audio half block by block and records the slot's own event behind each block
                # (nws_forward_audio_blocks), ONE job goes to the helper thread (rendered into a batch of its own, not in place)
                y = pipe.submit(f0, control, generator=shared_gen, row_blocks=blocks, block_events=blk_events[slot_i])
                xchg.post(slot_i, None, lambda _i=i, _y=y, _evs=blk_events[slot_i]: issue_blocks(_i, _y, _evs))
                return None
            # the batch is rendered straight into this rank's rows of the gather buffer (no local copy: the all-gather is
            # in place for RCCL, the peer pushes skip the local shard)
            y = pipe.submit(f0, control, generator=shared_gen, out=dst)
            if do_gather:
                post_behind(au, slot_i, lambda _i=i, _y=y: issue_whole(_i, _y))
            return None
        s = streams[i % len(streams)]
        with torch.cuda.stream(s):
            if distributed:
                y = None
                if do_compute:
                    pu, nz = par.shared_draws(101, N - 1, dev, generator=shared_gen)   # identical on all ranks
                    y = model(f0, control, phase_u=pu, noise=nz)
                if pending is not None:
                    pending.wait()
                if do_gather:
                    return gather(i, y if y is not None else gather_src)
                return None
            y = model(f0, control)
            if last_y is not None:
                last_y["y"] = y
        return None

    def join_streams():
        if use_pipe:
            pipe.synchronize()
        for s in streams:
            torch.cuda.current_stream().wait_stream(s)

    host_issue = {}

    def timed(n_steps, **kw):
        """n_steps of the issue pattern, bracketed by barrier + synchronize on both sides; seconds, max over ranks"""
        pending = None
        if distributed:
            dist.barrier()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        with hooks.around_timed():
            for i in range(n_steps):
                pending = step(i, pending, **kw)
        host_issue["s_per_step"] = (time.perf_counter() - t0) / max(1, n_steps)   # host time to ENQUEUE a step (no sync inside)
        if pending is not None:
            pending.wait()
        if xchg is not None:
            xchg.drain(peer.flush if peer is not None else None)                    # every exchange issued and complete
        join_streams()
        torch.cuda.synchronize()
        el = time.perf_counter() - t0      # this rank's K steps, from the common start to its own last exchange
        if distributed:
            dist.barrier()                  # (the closing barrier itself - a collective launch and a host synchronise - is not
        per_rank = [el]                     # part of any rank's steps: the job's time is the MAX over ranks, taken below)
        if distributed:
            tt = torch.tensor([el], dtype=torch.float64, device="cpu" if share_gpu else dev)
            allr = [torch.zeros_like(tt) for _ in range(world)]
            dist.all_gather(allr, tt)
            per_rank = [float(t.item()) for t in allr]
        return max(per_rank), per_rank

    # Priming, before the W warmup steps and untimed like them (reported as priming_steps): (1) every stream's caching-
    # allocator pool and every workspace of the ring has to have been through one full cycle, or the first 2 * depth timed
    # steps contain hipMallocs (measured: 1.2 ms/step instead of 0.47 for K = 50, W = 5 with 6 workspaces in flight);
    # (2) ~50 ms of continuous load before the clock starts helps short runs a little (K = 50: 0.504 -> 0.491 ms/step).
    # What stays inside the timed region by construction is the pipeline's fill and drain (first control half, last audio
    # half: 0.5-1 ms per timed region): 0.518 ms/step at K = 10, 0.491 at 50, 0.471 at 200, 0.468 at 1000.
    priming = max(2 * nbuf + 2, 120)
    gather_src = torch.zeros((B, N), dtype=torch.float32, device=dev) if distributed else None
    extra = {}
    with torch.no_grad():
        pending = None
        for i in range(priming + a.warmup):
            pending = step(i, pending)
        if pending is not None:
            pending.wait()
        if xchg is not None:
            xchg.drain(peer.flush if peer is not None else None)
        join_streams()
        torch.cuda.synchronize()
        if a.full:
            # live HIP-event timing of the dominant kernel (and the GRU) on their launch streams, inside the timed region
            _lib.check(_lib.lib().nws_profile_begin(a.steps, (1 << 3) | (1 << 1)))
        elapsed, per_rank = timed(a.steps)
        extra["host_issue_ms_per_step"] = round(host_issue["s_per_step"] * 1e3, 4)
        if a.dump_outputs and rank == 0:
            # what the last timed step returned: the batch (N = 1), the gathered batch of every rank (N > 1)
            if distributed:
                got = full[(a.steps - 1) % nbuf]
                if blocks is not None and peer is None:      # RCCL sub-batches fill the buffer block-major
                    got = par.block_major_view(got, world, len(blocks)).reshape(world * B, N)
            else:
                got = last_y["y"]
            dump_outputs(a.dump_outputs, {"waveforms": got.float().cpu().numpy()})
        hooks.extra(extra, a.steps, xchg, peer)
        n = C.c_int(0)
        if a.full:
            ms = (C.c_float * (a.steps * 6))()
            _lib.check(_lib.lib().nws_profile_collect(ms, C.byref(n)))
            k_ms = float(np.mean([ms[i * 6 + 3] for i in range(n.value)])) if n.value else float("nan")
            gru_ms_live = float(np.mean([ms[i * 6 + 1] for i in range(n.value)])) if n.value else float("nan")
            _lib.lib().nws_profile_end()

        if distributed and a.full:
            # the gathered batch must hold every rank's rows (rank r at rows [r*B, (r+1)*B))
            last = full[(a.steps - 1) % nbuf]
            assert torch.isfinite(last).all() and float(last[B * (world - 1):].abs().max()) > 0.0
            # exchange and compute told apart (outside the headline region; every region primed by a few untimed steps of its own
            # kind and as long as the headline's, so that fill / drain weigh the same): the all-gather alone (compute skipped: a
            # resident (B, N) shard leaves every step), the N > 1 issue pattern without its exchange, and the plain single-GPU
            # issue pattern (no shared generator, no gather buffer) - what this rank would do alone
            k2 = max(10, min(a.steps, 200))

            def region(**kw):
                for j in range(8):
                    step(j, None, **kw)
                if xchg is not None:
                    xchg.drain(peer.flush if peer is not None else None)
                join_streams()
                return timed(k2, **kw)

            g_el, g_ranks = region(do_compute=False)
            c_el, c_ranks = region(do_gather=False)
            extra["exchange"] = {"kind": gather_kind, "chunks": len(blocks) if blocks else 1,
                                 "issue": ("completion-driven: a helper thread issues each batch's exchange on its own stream once "
                                           "the host has seen the batch complete (parallel.CompletionDrivenExchange)") if xchg is not None
                                 else "stream-ordered behind each forward",
                                 "gather_slots": nbuf,
                                 # 1.0 = the exchange is completely hidden under the compute of the neighbouring steps
                                 "overlap_efficiency": (c_el / k2) / (elapsed / a.steps),
                                 "gather_ms": g_el / k2 * 1e3, "compute_only_ms": c_el / k2 * 1e3,
                                 "steps": k2, "bytes_gathered_per_rank_per_step": B * world * N * 4,
                                 "gather_ms_per_rank": [round(t / k2 * 1e3, 4) for t in g_ranks],
                                 "compute_only_ms_per_rank": [round(t / k2 * 1e3, 4) for t in c_ranks],
                                 "fake_peers": (peer.fake_peers if peer is not None else 0),
                                 "rccl_world_size": dist.get_world_size(), "backend": dist.get_backend(),
                                 "device_of_rank": f"cuda:{local_rank}"}
            devs = [None] * world       # which device every rank of the job really ran on (one process per GPU)
            dist.all_gather_object(devs, f"cuda:{local_rank} ({torch.cuda.get_device_properties(dev).name})")
            extra["exchange"]["devices_per_rank"] = devs
            if use_pipe:
                p_el, p_ranks = region(plain=True)
                extra["exchange"]["single_gpu_pattern_ms"] = p_el / k2 * 1e3
                extra["exchange"]["single_gpu_pattern_ms_per_rank"] = [round(t / k2 * 1e3, 4) for t in p_ranks]
                # the N > 1 step over the step of the plain single-GPU issue pattern in the same process: at world size 1 (forced)
                # the price of the exchange machinery with nothing to send; at N > 1 what the exchange costs each rank
                extra["exchange"]["world1_overhead" if world == 1 else "step_over_single_gpu_pattern"] = (elapsed / a.steps) / (p_el / k2)

        if use_pipe and a.full:
            # self-check outside the timed region: the issue pattern of the timed loop (pipeline, and the all-gather when
            # distributed) must return bit for bit what a plain forward returns for the same draws
            gchk = torch.Generator(device=dev).manual_seed(4242)   # the same draws on every rank, like the timed loop
            draws = [(torch.rand(101, device=dev, generator=gchk), torch.rand(N - 1, device=dev, generator=gchk))
                     for _ in range(12)]
            torch.cuda.synchronize()
            ys = []
            for i, (pu_c, nz_c) in enumerate(draws):
                au = pipe.next_audio_stream()
                if not distributed:
                    ys.append(pipe.submit(f0, control, phase_u=pu_c, noise=nz_c))
                    continue
                slot_i = i % nbuf
                with torch.cuda.stream(au):
                    xchg.acquire(slot_i, au)
                    dst_c = peer.local_rows(slot_i) if peer is not None else full[slot_i][rank * B:(rank + 1) * B]
                if blocks is not None:
                    y = pipe.submit(f0, control, phase_u=pu_c, noise=nz_c, row_blocks=blocks, block_events=blk_events[slot_i])
                    xchg.post(slot_i, None, lambda _i=i, _y=y, _evs=blk_events[slot_i]: issue_blocks(_i, _y, _evs))
                    ys.append(y)
                    continue
                # rendered in place into the gather buffer, as the timed loop does (the rows are cloned for the comparison below
                # before the slot is rendered into again: nbuf batches later)
                y = pipe.submit(f0, control, phase_u=pu_c, noise=nz_c, out=dst_c)
                with torch.cuda.stream(au):
                    ys.append(y.clone())
                post_behind(au, slot_i, lambda _i=i, _y=y: issue_whole(_i, _y))
            if xchg is not None:
                xchg.drain(peer.flush if peer is not None else None)
            pipe.synchronize()
            torch.cuda.synchronize()
            wrong = 0
            for y, (pu_c, nz_c) in zip(ys, draws):
                wrong += 0 if torch.equal(y, model(f0, control, phase_u=pu_c, noise=nz_c)) else 1
            torch.cuda.synchronize()
            extra["pipeline_selfcheck"] = {"batches": len(ys), "mismatching": wrong}
            # the timed loop's own route to the draws: submit(generator=g) must equal a plain forward with the two draws taken
            # from an identically seeded generator (what makes the ranks of a sharded batch agree without a collective)
            g1, g2 = par.make_shared_generator(dev, seed=777), par.make_shared_generator(dev, seed=777)
            y_g = pipe.submit(f0, control, generator=g1)
            pipe.synchronize()
            pu_g, nz_g = par.shared_draws(101, N - 1, dev, generator=g2)
            extra["pipeline_selfcheck"]["generator_route_matches"] = bool(torch.equal(y_g, model(f0, control, phase_u=pu_g, noise=nz_g)))
            torch.cuda.synchronize()
            if distributed:
                # the last gathered buffer must hold this rank's own last batch at its rows, bit for bit
                if share_gpu:
                    dist.barrier()
                # the last gathered buffer must hold EVERY rank's last batch at its rows, bit for bit: each rank re-renders
                # the other ranks' batches itself (their inputs come from seeded generators, the draws are shared)
                last = full[(len(ys) - 1) % nbuf]
                if blocks is not None and peer is None:      # RCCL sub-batches fill the buffer block-major
                    last = par.block_major_view(last, world, len(blocks)).reshape(world * B, N)
                ok = True
                for r in range(world):
                    y_r = ys[-1] if r == rank else model(*make_inputs(a, dev, r), phase_u=draws[-1][0], noise=draws[-1][1])
                    ok = ok and bool(torch.equal(last[r * B:(r + 1) * B], y_r))
                extra["pipeline_selfcheck"]["gathered_rows_match"] = ok
                wrong += 0 if ok else 1
            if wrong:   # reported, not raised: the line must still come out, with the evidence in it
                print(f"bench.py: pipeline self-check FAILED on rank {rank}: {wrong} of {len(ys)} batches differ from the plain "
                      f"forward", file=sys.stderr)
            if distributed:   # every rank's verdict
                tw = torch.tensor([wrong], dtype=torch.float64, device="cpu" if share_gpu else dev)
                dist.all_reduce(tw, op=dist.ReduceOp.SUM)
                extra["pipeline_selfcheck"]["mismatching_all_ranks"] = int(tw.item())
        if rank == 0 and a.full:
            # per-stage breakdown (diagnostic, outside the timed region)
            _lib.check(_lib.lib().nws_profile_begin(10, 0x3F))
            for _ in range(10):
                model(f0, control)
            torch.cuda.synchronize()
            ms2 = (C.c_float * 60)()
            _lib.check(_lib.lib().nws_profile_collect(ms2, C.byref(n)))
            extra["stage_ms"] = {nm: round(float(np.mean([ms2[i * 6 + s] for i in range(n.value)])), 4)
                                 for s, nm in enumerate(_lib.STAGE_NAMES)}   # one stream, nothing overlapping
            _lib.lib().nws_profile_end()
            if world == 1 and a.batch1_iters > 0:
                # config "batch=1, single MI355X, FastNEWT": latency / x real-time per utterance
                f1, c1 = f0[:1].contiguous(), control[:1].contiguous()
                for _ in range(10):
                    model(f1, c1)
                torch.cuda.synchronize()
                lat = []
                for _ in range(a.batch1_iters):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    model(f1, c1)
                    e1.record()
                    e1.synchronize()
                    lat.append(e0.elapsed_time(e1))
                lat = np.array(lat)
                dur_ms = N / 16000.0 * 1e3
                extra["batch1"] = {"p50_ms": round(float(np.percentile(lat, 50)), 4), "p90_ms": round(float(np.percentile(lat, 90)), 4),
                                   "x_realtime_p50": round(dur_ms / float(np.percentile(lat, 50)), 1),
                                   "rtf_mean": float(np.mean(lat) / dur_ms)}

    if rank == 0 and world == 1 and a.batch1_iters > 0 and a.full:
        # config "streaming 256-sample hop": stateless forward of one 16 ms buffer, captured once into a hipGraph
        with torch.no_grad():
            fs, cs = torch.rand(1, 1, 2, device=dev), torch.rand(1, 2, 2, device=dev)
            side = torch.cuda.Stream()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    model(fs, cs)
            torch.cuda.current_stream().wait_stream(side)
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                model(fs, cs)
            for _ in range(20):
                graph.replay()
            torch.cuda.synchronize()
            lat = []
            for _ in range(500):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph.replay()
                e1.record()
                e1.synchronize()
                lat.append(e0.elapsed_time(e1) * 1e3)
            extra["streaming_hop256_hipgraph"] = {"p50_us": round(float(np.percentile(lat, 50)), 2),
                                                  "p99_us": round(float(np.percentile(lat, 99)), 2),
                                                  "buffer_period_us": 16000.0}
            # config "streaming 256-sample hop", STATEFUL (GRU / phase / noise / reverb state carried across hops, linear reverb;
            # streaming.NewtStream over csrc/stream.hip): push() = input copies + one graph launch + output copy; hop() = the
            # captured hop on its own static buffers
            st_model = model
            strm = st_model.stream(1)
            fh, ch = 220 + 20 * torch.rand(1, 1, 2, device=dev), torch.randn(1, 2, 2, device=dev)
            for _ in range(20):
                strm.push(fh, ch)
            torch.cuda.synchronize()

            def hop_lat(fn, n):
                v = []
                for _ in range(n):
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    fn()
                    e1.record()
                    e1.synchronize()
                    v.append(e0.elapsed_time(e1) * 1e3)
                return {"p50_us": round(float(np.percentile(v, 50)), 2), "p99_us": round(float(np.percentile(v, 99)), 2)}

            push_lat = hop_lat(lambda: strm.push(fh, ch), 500)
            strm.static_io(2)
            extra["streaming_hop256_stateful"] = dict(push_lat, static_io=hop_lat(lambda: strm.hop(2), 500), buffer_period_us=16000.0,
                                                      note="NewtStream: state carried across hops, reverb as a linear convolution of "
                                                           "the stream; steady-state hops replay a hipGraph")
            del strm
            # the same B=1 clip as `batch1`, the forward (its two RNG draws included) captured once into a hipGraph: what a
            # serving loop with fixed shapes pays per clip without the seven launch gaps of the eager call
            f1, c1 = f0[:1].contiguous(), control[:1].contiguous()
            side.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(side):
                for _ in range(3):
                    model(f1, c1)
            torch.cuda.current_stream().wait_stream(side)
            graph1 = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph1):
                model(f1, c1)
            for _ in range(10):
                graph1.replay()
            torch.cuda.synchronize()
            lat = []
            for _ in range(a.batch1_iters):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                graph1.replay()
                e1.record()
                e1.synchronize()
                lat.append(e0.elapsed_time(e1))
            dur_ms = N / 16000.0 * 1e3
            extra["batch1_hipgraph"] = {"p50_ms": round(float(np.percentile(lat, 50)), 4),
                                        "p90_ms": round(float(np.percentile(lat, 90)), 4),
                                        "x_realtime_p50": round(dur_ms / float(np.percentile(lat, 50)), 1)}
    if rank == 0 and world == 1 and a.legs and use_pipe and not distributed and a.full:
        # extra legs, driver-timed like the headline: the same issue pattern for the other arithmetic / inputs / shapers
        legs = {}
        n_audio, n_control = len(pipe.audio), len(pipe.control)
        headline_is_two_term = (opts == 0 and not a.exact and a.inputs == "rand")

        def leg(name, exciter_opts=None, inputs="rand", exact=False, steps=a.leg_steps, note=None):
            m2 = nws.NeuralWaveshaping.load_from_checkpoint(wpath).to(dev).eval()
            if not exact:
                m2.newt = nws.FastNEWT(m2.newt)
            if exciter_opts is not None:
                m2.exciter_opts = exciter_opts
            fi, ci = make_inputs(a, dev, rank, kind=inputs)
            ms_leg = time_leg(m2, fi, ci, steps, 10, n_audio, n_control)
            legs[name] = {"ms_per_step": round(ms_leg, 4), "samples_per_s": B * N / (ms_leg * 1e-3), "steps": steps,
                          "exciter_opts": m2._engine.exciter_opts(), "inputs": inputs, "shapers": "exact sin-MLP" if exact else "FastNEWT LUT"}
            if note:
                legs[name]["note"] = note
            del m2

        if headline_is_two_term:
            legs["two_term"] = {"ms_per_step": round(elapsed / a.steps * 1e3, 4), "samples_per_s": B * N * a.steps / elapsed,
                                "steps": a.steps, "exciter_opts": 0, "inputs": "rand", "shapers": "FastNEWT LUT",
                                "note": "= the headline region (the default arithmetic: every mixer product a two-term fp16 split, 22-bit)"}
        else:
            leg("two_term", exciter_opts=0, note="every mixer product a two-term fp16 split of both operands (22-bit, fp32-class)")
        leg("hybrid_w", exciter_opts=8, note="OPT-IN (model.exciter_opts = 8): harmonics 16..101 as fp16 x fp16 products; measured "
                                             "3e-7 .. 4e-6 RMS vs the reference on the golden vectors, no worst-case bound under 1e-5")
        leg("realistic_inputs", inputs="realistic", note="F0 ~ U[100,1000] Hz with vibrato, control ~ N(0,1) (SURVEY 8(d) config 3)")
        leg("exact", exact=True, steps=max(10, a.leg_steps // 3), note="exact sin-MLP shapers (the reference's default NEWT)")
        extra["legs"] = legs
    if rank == 0:
        total_samples = B * world * N * a.steps
        value = total_samples / elapsed
        ms_per_step = elapsed / a.steps * 1e3
        one_term = bool(opts & 2) and not a.exact
        hybrid = bool(opts & (4 | 8)) and not one_term and not a.exact
    if rank == 0 and a.full:
        st = extra.get("stage_ms", {})
        pmc, pmc_src, pmc_note = None, None, None
        if a.pmc in ("auto", "live") and world == 1 and st:
            stage_ns = {"exciter_newt_kernel": st.get("exciter_newt", 0) * 1e6, "control_gru_kernel": st.get("control_gru", 0) * 1e6,
                        "frame_mlps16_kernel": st.get("frame_mlps", 0) * 1e6, "frame_mlps64_kernel": st.get("frame_mlps", 0) * 1e6,
                        "frame_mlps_wr_kernel": st.get("frame_mlps", 0) * 1e6,
                        "fir_noise_mfma_kernel": st.get("fir_noise", 0) * 1e6}
            try:
                pmc, pmc_src = collect_pmc_live(a, stage_ns)
            except Exception as e:   # the line must still come out
                pmc, pmc_src = None, f"{type(e).__name__}: {e}"
            if pmc is None:
                pmc_note = f"live PMC collection unavailable ({pmc_src}); counters from the committed profile instead"
        if pmc is None and a.pmc != "off":
            pmc, pmc_src = load_pmc()
            if pmc and (pmc.get("batch_per_gpu") != B or pmc.get("frames") != T or a.exact or pmc.get("exciter_opts", 0) != opts):
                pmc = None        # counters of another workload: not quoted
        # fp16 MFMAs per (M-tile, K-step): 3 with both operands two-term, 2 with one-term sines, 1 with one-term weights too;
        # K-step 0 always 3 in the hybrid forms; 6 K-steps of 16 slots + one of 8
        per_step = 2 if one_term else (2 if (opts & 4) else 1 if (opts & 8) else 3)
        first = 2 if one_term else 3
        terms = (first * 16 + per_step * (5 * 16 + 8)) / 112.0
        flops = FLOP_PER_SAMPLE_EXCITER_NEWT * B * N
        mfma_flop = exciter_mfma_flop_per_sample(terms, not (opts & 1) and not a.exact) * B * N
        dom = kernel_roofline("exciter_newt_kernel", pmc, st.get("exciter_newt") or k_ms, algo_flop=flops, mfma_flop=mfma_flop)
        vi = dom.get("valu_issue")
        # Headline roofline object: ALGORITHMIC first.  achieved = SURVEY 8(d)'s 14 969 flop/sample x the samples one launch
        # processes / the kernel's live average duration (HIP events on its launch stream inside the timed region); peak = the
        # dense fp16 MFMA peak, the pipe 86 % of that work (the 101 -> 64 contraction) runs on.  WHY the fraction is what it
        # is rides along: the launch is POWER-limited (profiles/r06/exciter_ablations.txt: kernel cycles / duration = 1.9-2.1 GHz
        # where its own timing ablations and the other kernels run at 2.3-2.5; without its mixer MFMAs -25 % cycles AND +26 % clock), its
        # vector pipe ~0.8 busy at that clock (sines, their fp16 split, table index math) - not bound by the matrix pipe's rate or by HBM.
        algo_bytes = hbm_algorithmic_bytes(B, T)
        traffic = (dom.get("hbm") or {}).get("traffic")
        # The denominator is the kernel's ISOLATED duration (one stream, nothing beside it: HIP events around it on its launch stream,
        # `stage_ms`, the number the committed rocprofv3 --kernel-trace --stats summary reproduces).  Inside the pipelined timed
        # region two batches' oscillator kernels share the chip and each takes LONGER than a whole step (`kernel_ms_live`): a
        # duration that does not fit into the step it belongs to is no roofline denominator (VERDICT r4 #7a).  `frac_per_step` is
        # the same work over the step time: what the pipeline as a whole delivers.
        iso_ms = st.get("exciter_newt") or k_ms
        ach = flops / (iso_ms * 1e-3) / 1e12
        roofline = {"bound": "mfma", "kernel": "exciter_newt_kernel", "achieved": ach, "peak": PEAK_F16_MFMA_TFLOPS, "unit": "TFLOP/s",
                    "frac": ach / PEAK_F16_MFMA_TFLOPS, "traffic": traffic,
                    "hbm_algorithmic_bytes": algo_bytes["exciter_newt_kernel"],
                    "traffic_over_algorithmic": (traffic / algo_bytes["exciter_newt_kernel"]) if traffic else None,
                    "flop_per_launch": flops, "kernel_ms": iso_ms, "kernel_ms_source": "isolated (one stream, HIP events on the launch stream)"
                    if st.get("exciter_newt") else "live (no isolated measurement in this run)",
                    "frac_per_step": flops / (ms_per_step * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS,
                    "kernel_ms_live": k_ms, "frac_live": flops / (k_ms * 1e-3) / 1e12 / PEAK_F16_MFMA_TFLOPS if k_ms == k_ms and k_ms > 0 else None,
                    "limiter": "power",
                    "clock_ghz": ((pmc or {}).get("kernels", {}).get("exciter_newt_kernel", {}) or {}).get("clock_ghz_during_pass"),
                    "clock_ghz_other_kernels": {kn: round(kv["clock_ghz_during_pass"], 3) for kn, kv in ((pmc or {}).get("kernels", {}) or {}).items()
                                                if kn in ("control_gru_kernel", "frame_mlps_wr_kernel") and kv.get("clock_ghz_during_pass")},
                    "valu_issue": dict(vi, frac_live=(vi["achieved"] * iso_ms / k_ms / (N_SIMD * MAX_CLOCK_GHZ))
                                       if (k_ms == k_ms and k_ms > 0) else None) if vi else None,
                    "mfma_f16_executed": dom.get("mfma_f16_executed"), "hbm": dom.get("hbm"),
                    "counters": pmc_src if pmc else None, "counters_note": pmc_note,
                    "gru_ms_in_timed_region": gru_ms_live,
                    "note": "achieved = 14 969 flop/sample (SURVEY 8(d): 2*64*101 mixer + 101*5 sines + 64*24 FiLM/LUT/mix) x B*N / "
                            "kernel_ms, the kernel's isolated one-stream duration (the rocprofv3 summary under profiles/ reproduces it); "
                            "frac_per_step = the same flop over ms_per_step; kernel_ms_live / frac_live = its average inside the pipelined "
                            "timed region, where it shares the chip with the neighbouring batch's kernels (longer than a step: not a "
                            "roofline denominator); limiter: power - clock_ghz = GRBM_GUI_ACTIVE cycles of the PMC pass / the isolated duration, "
                            "against clock_ghz_other_kernels by the same arithmetic (profiles/r06/exciter_ablations.txt: the launch's timing "
                            "ablations at 2.1-2.3 GHz); valu_issue.frac = VALU-busy SIMD-cycles per launch from the PMC pass / isolated "
                            "duration / 1024 SIMDs x 2.4 GHz; frac_live over the live duration"}
        roofline_all = [dom]
        if st:
            roofline_all += [
                kernel_roofline("control_gru_kernel", pmc, st.get("control_gru"), algo_flop=FLOP_PER_STEP_GRU * B * T,
                                hbm_note="sequential recurrence, one workgroup per utterance: bound by the per-step latency chain "
                                         "(B of 256 CUs busy); fp32 VALU peak of those CUs = B/256 x 157.3 TFLOP/s"),
                # (executed: the three products of the two-term split, and proj in both path workgroups)
                kernel_roofline("frame_mlps_wr_kernel", pmc, st.get("frame_mlps"), algo_flop=FLOP_PER_FRAME_MLPS * B * T,
                                mfma_flop=3 * (FLOP_PER_FRAME_MLPS + 2 * 128 * 128) * B * T),
                kernel_roofline("fir_noise_mfma_kernel", pmc, st.get("fir_noise"), algo_flop=FLOP_PER_FRAME_NOISE * B * T,
                                mfma_flop=3 * FLOP_PER_FRAME_NOISE * B * T),
                kernel_roofline("reverb (col125_fwd + row + col125_inv)", pmc, st.get("reverb"),
                                hbm_note="memory-latency bound four-step FFT: 3 passes over (B, L) complex planes")]
            if pmc:   # the reverb's three launches: HBM traffic summed
                tot = sum(pmc["kernels"].get(kn, {}).get("hbm_bytes_per_launch", 0.0) for kn in ("col125_fwd_kernel", "row512_kernel", "row_kernel", "col125_inv_kernel"))
                if tot and st.get("reverb"):
                    roofline_all[-1]["hbm"] = {"traffic": tot, "achieved": tot / (st["reverb"] * 1e-3) / 1e12, "peak": PEAK_HBM_TBS,
                                               "unit": "TB/s", "frac": tot / (st["reverb"] * 1e-3) / 1e12 / PEAK_HBM_TBS}
        for e in roofline_all:
            kb = algo_bytes.get(e["kernel"].split(" ")[0])
            if kb:
                e["hbm_algorithmic_bytes"] = kb
                if (e.get("hbm") or {}).get("traffic"):
                    e["traffic_over_algorithmic"] = e["hbm"]["traffic"] / kb
    if rank == 0:
        if a.exact:
            dtype = "f32 (101->64 mixer, frame MLPs, FIR noise: fp16x2-split MFMA contractions = 22-bit products, fp32 accumulate; exact sin-MLP shapers in fp32)"
        elif one_term:
            dtype = ("f32 (frame MLPs, FIR noise: fp16x2-split MFMA contractions, fp32 accumulate; 101->64 mixer: weights fp16x2, "
                     "sines ONE fp16 term = 11-bit mixer inputs, fp32 accumulate)")
        elif hybrid:
            dtype = ("f32 (frame MLPs, FIR noise, mixer bias + harmonics 1..15: fp16x2-split MFMA contractions = 22-bit products, "
                     "fp32 accumulate; mixer harmonics 16..101: " + ("fp16 x fp16" if opts & 8 else "fp16x2 weights x fp16 sines") +
                     ", fp32 accumulate; FiLM interpolation bf16x3-split MFMA = exact fp32 operands; e2e 3e-7..3e-6 RMS vs the "
                     "reference, bar 1e-4)")
        else:
            dtype = "f32 (fp16x2-split MFMA contractions = 22-bit products, fp32 accumulate; FiLM interpolation bf16x3-split MFMA = exact fp32 operands)"
        out = {
            "metric": "audio_samples_per_sec", "value": value, "unit": "samples/s", "n_gpus": world, "steps": a.steps,
            "warmup": a.warmup, "priming_steps": priming, "ms_per_step": ms_per_step, "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": dtype, "data": "synthetic",
            "config": {"workload": f"NEWT forward, vn checkpoint, {'exact sin-MLP shapers' if a.exact else 'FastNEWT LUT'}, "
                                   f"batch {B}/GPU x {T} frames (4 s @ 16 kHz), "
                                   f"{'torch.rand F0/control' if a.inputs == 'rand' else 'F0 ~ U[100,1000] Hz with vibrato, control ~ N(0,1)'}, "
                                   f"RNG draws on device{', all-gather of waveforms (' + str(gather_kind) + ')' if distributed else ''}",
                       "batch_per_gpu": B, "frames": T, "samples_per_utterance": N, "parallelism": f"batch-shard x{world}",
                       "exciter_opts": opts, "streams": len(streams),
                       # where the pipeline's hardware queues sit on the command processor's pipes, as MEASURED before the first step
                       # (pipeline.placed_streams): queue_offset = hardware queues this process had created before, mod 4
                       "queue_offset": (pmod.placement_report(dev) or {}).get("queue_offset") if use_pipe else None,
                       "placement": pmod.placement_report(dev) if use_pipe else None,
                       "issue": (f"ForwardPipeline: control half (carries + {a.gru} GRU) on {len(pipe.control)} side stream(s), "
                                 f"audio half on {len(streams)} streams, {len(pipe.slots)} workspaces in flight") if use_pipe
                       else f"whole forwards round-robin on {len(streams)} streams"},
            "x_realtime_aggregate": value / 16000.0,
            "rtf_per_utterance": (ms_per_step * 1e-3) / (N / 16000.0) / B,
            "ms_per_step_per_rank": [round(t / a.steps * 1e3, 4) for t in per_rank], "full": a.full,
        }
        if a.full:
            out.update(roofline=roofline, roofline_all=roofline_all)
        out.update(extra)
        if world == 1 and not a.no_cpu_baseline and a.full:
            out["cpu_baseline"] = cpu_baseline(wpath, T, a.cpu_seconds)
    if distributed:
        if xchg is not None:
            xchg.close()                # the helper thread is idle (every region drained it): join before the communicator goes
        dist.destroy_process_group()
    if rank == 0:
        try:   # RCCL prints its banner through C stdio: drain that first so that the JSON line is the last line of stdout
            C.CDLL(None).fflush(None)
        except Exception:
            pass
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
