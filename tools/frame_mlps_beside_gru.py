#!/usr/bin/env python
"""The folded frame-MLP launch at B x T (default 64 x 500), back to back on one stream, in both forms (8 and 12 waves per
workgroup, nws_debug_frame_mlps_spec_waves): alone, and with per-utterance recurrences for B utterances kept resident on a
high-priority side stream WITHOUT dependencies (the pattern of tools/audio_only_rate.py).  A CU that holds a recurrence workgroup
(256 registers per wave) takes no 8-wave frame-MLP workgroup (2 x 184 registers per SIMD), so the 250 workgroups of that form
run as two rounds on the 192 CUs that are left; the 168 workgroups of the 12-wave form fit.  GPU only.
Measured on MI355X: profiles/frame_mlps_12wave_ab.txt.   B= T= N= (timed launches) NGRU= (recurrences enqueued beside them)"""
import ctypes as C
import importlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
nws = importlib.import_module("neural-waveshaping-synthesis_amd")
_lib = importlib.import_module("neural-waveshaping-synthesis_amd._lib")
nws.ensure_default_config()
m = nws.NeuralWaveshaping.load_from_checkpoint(os.path.join(ROOT, "tests/golden/weights_vn.npz")).cuda().eval()
m.newt = nws.FastNEWT(m.newt)
eng = m._engine
B, T = int(os.environ.get("B", 64)), int(os.environ.get("T", 500))
N, NGRU = int(os.environ.get("N", 200)), int(os.environ.get("NGRU", 160))
wdesc, _, _ = eng.weights()
L = _lib.lib()
torch.manual_seed(0)
f0 = torch.rand(B, 1, T, device="cuda")
control = torch.rand(B, 2, T, device="cuda")
gru = torch.rand(B, T, 128, device="cuda") * 2 - 1
film = torch.empty(B, T, 256, device="cuda")
spec = torch.empty(B, T, 132, device="cuda")
spare = [eng.new_workspace(B, T) for _ in range(2)]
eng.forward_control(f0, control, spare[0], batched_gru=False)
torch.cuda.synchronize()


def launch(waves):
    _lib.check(L.nws_debug_frame_mlps_spec_waves(C.byref(wdesc), gru.data_ptr(), B * T, film.data_ptr(), spec.data_ptr(), waves,
                                                 _lib.stream_ptr()), "nws_debug_frame_mlps_spec_waves")


def timed(waves, beside):
    main, side = torch.cuda.Stream(), torch.cuda.Stream(priority=-1)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    g0, g1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    if beside:
        with torch.cuda.stream(side):
            g0.record()
            for i in range(NGRU):     # enough of them to outlast the timed launches: checked below
                eng.forward_control(f0, control, spare[i % 2], batched_gru=False)
            g1.record()
    with torch.cuda.stream(main):
        if beside:
            torch.cuda._sleep(200000)    # the first recurrence takes its CUs first
        for _ in range(10):
            launch(waves)
        e0.record()
        for _ in range(N):
            launch(waves)
        e1.record()
    e1.synchronize()
    still = (not g1.query()) if beside else None
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / N * 1e3, still, (g0.elapsed_time(g1) / NGRU * 1e3 if beside else float("nan"))


with torch.no_grad():
    for waves in (8, 12):
        for rep in range(3):
            alone, _, _ = timed(waves, False)
            beside, still, gru_us = timed(waves, True)
            print(f"waves {waves} rep {rep}: alone {alone:.2f} us/launch; beside a resident recurrence {beside:.2f} us/launch "
                  f"(ratio {beside / alone:.3f}; recurrence still running at the end: {still}; recurrence {gru_us:.1f} us/launch)", flush=True)
