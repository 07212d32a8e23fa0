"""-m gpu: the pYIN kernels (csrc/pyin.hip through both bindings) against the float64 restatement of the definition
(tests/pyin_restatement.py).  Every stage is compared on the GPU's own input to that stage, so that a threshold
decision or a tie in one stage does not blur the check of the next; the end-to-end check from audio comes on top.

Bounds.  CMND: the GPU may carry 4x the max-abs error of the SAME restatement evaluated in float32 numpy on the same input (a
sequential fp32 accumulation of 512 terms grows like sqrt(n), numpy's pairwise one like log n: sqrt(512) / log2(512) = 2.5).
Observation stage: counts and bins identical (bins one off on <= 0.1 % of candidates: rint at a half), probabilities to 1e-9.
Decode: the GPU path's log-probability, evaluated in float64 on the host, >= the restatement's optimum - 1e-6, states
identical on >= 99 % of frames.  End to end: voiced flag differs on <= 1 % of frames, bins within 1 on >= 99 % of the frames
both call voiced."""
import functools
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch
from scipy.io import wavfile

import pyin_restatement as pr
from conftest import ROOT
from gpu_util import record

pytestmark = pytest.mark.gpu

SR = 16000


def _phase(freq):
    return 2 * np.pi * np.cumsum(freq) / SR


def _vibrato(seconds, f=220.0, seed=0):
    t = np.arange(int(SR * seconds)) / SR
    ph = _phase(f * (1 + 0.01 * np.sin(2 * np.pi * 5.5 * t)))
    return 0.3 * np.sin(ph) + 0.15 * np.sin(2 * ph) + 0.08 * np.sin(3 * ph)


@functools.lru_cache(maxsize=None)
def _cases():
    g = np.random.default_rng(11)
    n = lambda k: g.standard_normal(k)
    sil = np.zeros(3200)
    gl = 0.3 * np.sin(_phase(110.0 * 4.0 ** (np.arange(SR) / SR)))
    return {
        "vibrato_silence_noise": (np.concatenate([sil, _vibrato(0.6), sil]) + 1e-3 * n(16000), {}),
        "glissando_110_440": (gl, {}),
        "white_noise": (0.3 * n(8000), {}),
        "all_zero": (np.zeros(4000), {}),
        "constant": (np.full(4000, 0.25), {}),
        "odd_length_4099": (_vibrato(4099 / SR, 330.0) + 1e-3 * n(4099), {}),
        "short_600": (_vibrato(600 / SR, 440.0) + 1e-3 * n(600), {}),
        "frame_block_plus_one": (_vibrato(4100 / SR, 180.0) + 1e-3 * n(4100), {}),                    # 33 frames: 32 + 1
        "frame_256_hop_100": (_vibrato(3001 / SR, 300.0) + 1e-3 * n(3001), {"frame_length": 256, "hop_length": 100}),
        "fmin_100_fmax_800": (_vibrato(0.5, 250.0) + 1e-3 * n(8000), {"fmin": 100.0, "fmax": 800.0}),
        # transition window 21 instead of 31 (the decode's runtime-width form), eight shared block sums per frame instead of four
        "hop_64": (np.concatenate([_vibrato(0.2, 260.0), np.zeros(1600)]) + 1e-3 * n(4800), {"hop_length": 64}),
        "long_10s": (_vibrato(10.0, 196.0) * (1 + 0.3 * np.sin(2 * np.pi * 0.7 * np.arange(10 * SR) / SR)) + 1e-3 * n(10 * SR), {}),
    }


NAMES = list(_cases())


def _kw(c):
    return dict(sample_rate=c.sr, minimum_frequency=c.fmin, maximum_frequency=c.fmax, frame_length=c.frame_length, hop_length=c.hop)


@functools.lru_cache(maxsize=None)
def _gpu(name):
    """every stage on the GPU, each fed the stage before it + the one-call form: computed once per case"""
    import nws_amd  # noqa: F401
    from nws_amd.data.utils import f0_extraction as fe
    x, kw = _cases()[name]
    c = pr.config(**kw)
    a = torch.from_numpy(x.astype(np.float32)).cuda().unsqueeze(0)
    yin = fe.pyin_cmnd(a, **_kw(c))
    obs = fe.pyin_observe(yin, **_kw(c))
    states, f0 = fe.pyin_viterbi(*obs, **_kw(c))
    whole = fe.pyin_frames(a, **_kw(c))
    torch.cuda.synchronize()
    T = 1 + x.size // c.hop
    assert yin.shape == (1, T, c.lags) and states.shape == (1, T)
    out = dict(c=c, x32=x.astype(np.float32), yin=yin[0].cpu().numpy(), cand_bin=obs[0][0].cpu().numpy(), cand_prob=obs[1][0].cpu().numpy(),
               count=obs[2][0].cpu().numpy(), voiced_prob=obs[3][0].cpu().numpy(), states=states[0].cpu().numpy(),
               f0=f0[0].cpu().numpy())
    # the one-call form is the three stages on one stream
    assert torch.equal(whole[0], f0) and torch.equal(whole[1], obs[3]) and torch.equal(whole[2], states)
    return out


@functools.lru_cache(maxsize=None)
def _ref(name):
    """the restatement from audio in float64 (timed: the label beside the GPU's times)"""
    x, kw = _cases()[name]
    t0 = time.perf_counter()
    r = pr.pyin(x.astype(np.float32).astype(np.float64), pr.config(**kw))
    r.seconds = time.perf_counter() - t0
    return r


@pytest.mark.parametrize("name", NAMES)
def test_cmnd_within_four_times_the_float32_restatement(name):
    g, r = _gpu(name), _ref(name)
    c = g["c"]
    y32 = pr.cmnd(pr.difference(g["x32"], c, np.float32), c, np.float32)
    err32 = float(np.abs(y32.astype(np.float64) - r.yin).max())
    err = float(np.abs(g["yin"].astype(np.float64) - r.yin).max())
    record("pyin_cmnd_" + name, max_abs_err_gpu=err, max_abs_err_float32_numpy=err32, frames=int(r.yin.shape[0]))
    print(name, "cmnd max abs err: gpu", err, "float32 numpy", err32)
    assert np.isfinite(g["yin"]).all()
    assert err <= 4 * err32, (name, err, err32)


@pytest.mark.parametrize("name", NAMES)
def test_observation_stage_on_the_gpus_own_yin(name):
    g = _gpu(name)
    c = g["c"]
    cb, cp, cnt, vp = pr.observe(g["yin"], c)
    assert np.array_equal(g["count"], cnt), name
    n = int(cnt.sum())
    mask = np.arange(c.lags)[None, :] < cnt[:, None]
    assert np.all(g["cand_bin"][~mask] == -1) and np.all(g["cand_prob"][~mask] == 0)
    dbin = np.abs(g["cand_bin"][mask].astype(np.int64) - cb[mask])
    off = int((dbin != 0).sum())
    perr = float(np.abs(g["cand_prob"][mask] - cp[mask]).max()) if n else 0.0
    verr = float(np.abs(g["voiced_prob"] - vp).max())
    record("pyin_observe_" + name, candidates=n, bins_off_by_one=off, max_prob_err=perr, max_voiced_prob_err=verr)
    print(name, "candidates", n, "bins off", off, "prob err", perr, "voiced_prob err", verr)
    assert dbin.max(initial=0) <= 1 and off <= 0.001 * n, (name, off, n)
    assert perr <= 1e-9 and verr <= 1e-9, (name, perr, verr)


@pytest.mark.parametrize("name", NAMES)
def test_decode_on_the_gpus_own_observations(name):
    g = _gpu(name)
    c = g["c"]
    obs = (g["cand_bin"].astype(np.int64), g["cand_prob"], g["count"].astype(np.int64), g["voiced_prob"])
    states, best = pr.viterbi(*obs, c)
    assert g["states"].min() >= 0 and g["states"].max() < 2 * c.n_bins
    got = pr.path_log_probability(g["states"], *obs, c)
    same = float(np.mean(g["states"] == states))
    record("pyin_viterbi_" + name, logp_gpu_path=got, logp_optimum=best, states_identical=same, frames=int(states.size))
    print(name, "log-probability: gpu path", got, "optimum", best, "identical states", same)
    assert got >= best - 1e-6, (name, got, best)
    assert same >= 0.99, (name, same)
    f0, voiced = pr.decode(g["states"], c)
    assert np.allclose(g["f0"], f0, rtol=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_end_to_end_from_audio(name):
    g, r = _gpu(name), _ref(name)
    c = g["c"]
    voiced = g["states"] < c.n_bins
    flag_diff = float(np.mean(voiced != r.voiced))
    both = voiced & r.voiced
    near = float(np.mean(np.abs(g["states"][both] - r.states[both]) <= 1)) if both.any() else 1.0
    record("pyin_end_to_end_" + name, voiced_flag_differs=flag_diff, bins_within_one=near, voiced_frames=int(both.sum()),
           restatement_cpu_seconds=r.seconds, audio_seconds=_cases()[name][0].size / SR)
    print(name, "voiced flag differs", flag_diff, "bins within one", near, "voiced frames", int(both.sum()))
    assert flag_diff <= 0.01 and near >= 0.99, (name, flag_diff, near)
    if name in ("vibrato_silence_noise", "glissando_110_440", "long_10s"):
        assert both.sum() >= 0.5 * voiced.size                      # the test is not vacuous: these inputs are pitched
    if name in ("white_noise", "all_zero", "constant"):
        assert not voiced.any()


def test_batch_rows_equal_their_single_row_results_bit_for_bit():
    import nws_amd  # noqa: F401
    from nws_amd.data.utils import f0_extraction as fe
    cs = _cases()
    rows = [cs["vibrato_silence_noise"][0][3000:11000], cs["white_noise"][0][:8000], cs["glissando_110_440"][0][:8000]]
    a = torch.from_numpy(np.stack(rows).astype(np.float32)).cuda()

    def stages(x):
        yin = fe.pyin_cmnd(x)
        obs = fe.pyin_observe(yin)
        return (yin, *obs, *fe.pyin_viterbi(*obs), *fe.pyin_frames(x, fill_na=0.0))

    whole = stages(a)
    for i in range(3):
        for w, s in zip(whole, stages(a[i:i + 1].clone())):
            assert torch.equal(w[i:i + 1], s), i
    # fill_na replaces F0 on the unvoiced frames only (row 1 is noise: all of them)
    f0_fill, states = whole[-3], whole[-1]
    nb = pr.config().n_bins
    assert torch.all(f0_fill[states >= nb] == 0) and torch.all(f0_fill[states < nb] > 0) and torch.all(f0_fill[1] == 0)
    assert torch.equal(whole[6][states < nb], f0_fill[states < nb])


CHILD = """
import sys
import numpy as np, torch
sys.path.insert(0, {root!r})
import nws_amd
from nws_amd import engine
from nws_amd.data.utils import f0_extraction as fe
assert engine.ops() is None                      # the ctypes binding
z = np.load({inp!r})
a = torch.from_numpy(z["audio"]).cuda()
yin = fe.pyin_cmnd(a)
obs = fe.pyin_observe(yin)
states, f0 = fe.pyin_viterbi(*obs)
whole = fe.pyin_frames(a)
f0n, vpn = fe.extract_f0_with_pyin(z["audio"][0], 16000, interpolate_fn=None)
np.savez({out!r}, yin=yin.cpu().numpy(), cand_bin=obs[0].cpu().numpy(), cand_prob=obs[1].cpu().numpy(), count=obs[2].cpu().numpy(),
         voiced_prob=obs[3].cpu().numpy(), states=states.cpu().numpy(), f0=f0.cpu().numpy(), w_f0=whole[0].cpu().numpy(),
         w_vp=whole[1].cpu().numpy(), w_states=whole[2].cpu().numpy(), f0n=f0n, vpn=vpn)
"""


@pytest.mark.skipif(os.environ.get("NWS_BACKEND") == "ctypes", reason="already the ctypes pass")
def test_both_bindings_give_equal_results(tmp_path):
    import nws_amd  # noqa: F401
    from nws_amd import engine
    from nws_amd.data.utils import f0_extraction as fe
    assert engine.ops() is torch.ops.newt_hip
    cs = _cases()
    audio = np.stack([cs["vibrato_silence_noise"][0][3000:9000], cs["glissando_110_440"][0][:6000]]).astype(np.float32)
    inp, out, script = str(tmp_path / "in.npz"), str(tmp_path / "out.npz"), str(tmp_path / "child.py")
    np.savez(inp, audio=audio)
    with open(script, "w") as f:
        f.write(CHILD.format(root=ROOT, inp=inp, out=out))
    r = subprocess.run([sys.executable, script], env=dict(os.environ, NWS_BACKEND="ctypes"), capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    z = np.load(out)
    a = torch.from_numpy(audio).cuda()
    yin = fe.pyin_cmnd(a)
    obs = fe.pyin_observe(yin)
    states, f0 = fe.pyin_viterbi(*obs)
    whole = fe.pyin_frames(a)
    f0n, vpn = fe.extract_f0_with_pyin(audio[0], 16000, interpolate_fn=None)
    mine = dict(yin=yin, cand_bin=obs[0], cand_prob=obs[1], count=obs[2], voiced_prob=obs[3], states=states, f0=f0, w_f0=whole[0],
                w_vp=whole[1], w_states=whole[2])
    for k, v in mine.items():
        assert np.array_equal(z[k], v.cpu().numpy()), k
    assert isinstance(f0n, np.ndarray) and f0n.dtype == np.float64 and f0n.shape == vpn.shape == (1 + 6000 // 128,)
    assert np.array_equal(z["f0n"], f0n) and np.array_equal(z["vpn"], vpn)


def test_front_end_shapes_interpolation_and_bad_arguments():
    import nws_amd  # noqa: F401
    from nws_amd import engine
    from nws_amd.data.utils import f0_extraction as fe
    from nws_amd.data.utils.upsampling import linear_interpolation
    x = _cases()["glissando_110_440"][0][:6000].astype(np.float32)
    f0, vp = fe.extract_f0_with_pyin(x, 16000, interpolate_fn=None)
    up_f0, up_vp = fe.extract_f0_with_pyin(x, 16000)                      # the reference's default: sample rate
    assert up_f0.shape == up_vp.shape == (6000,)
    assert np.array_equal(up_f0, linear_interpolation(f0, 1024, 128, original_length=6000))
    assert np.array_equal(up_vp, linear_interpolation(vp, 1024, 128, original_length=6000))
    tf0, tvp = fe.extract_f0_with_pyin(torch.from_numpy(x).cuda(), 16000, interpolate_fn=None)
    assert tf0.is_cuda and tf0.shape == (47,) and np.array_equal(tf0.cpu().numpy().astype(np.float64), f0)
    bf0, bvp = fe.extract_f0_with_pyin(torch.from_numpy(np.stack([x, x])).cuda(), 16000, interpolate_fn=None)
    assert bf0.shape == bvp.shape == (2, 47) and torch.equal(bf0[1], tf0) and torch.equal(bvp[0], tvp)
    a = torch.from_numpy(x).cuda().unsqueeze(0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fe.pyin_frames(torch.from_numpy(x).unsqueeze(0))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        fe.pyin_frames(a.double())
    with pytest.raises(RuntimeError, match="frame_length / 2"):
        fe.pyin_frames(a[:, :512])                                         # shorter than the reflect padding
    with pytest.raises(RuntimeError, match="unsupported configuration"):
        fe.pyin_frames(a, frame_length=4096)                               # more than 512 lags
    with pytest.raises(RuntimeError, match="unsupported configuration"):
        fe.pyin_frames(a, minimum_frequency=20.0, maximum_frequency=16000.0)      # more than 1024 pitch bins
    with pytest.raises(RuntimeError, match="unsupported configuration"):
        fe.pyin_cmnd(a, hop_length=2048)
    # a table of another configuration is refused by the binding; the launchers return their codes
    cfg, other = (16000.0, 65.0, 2093.0, 1024, 128), (16000.0, 100.0, 800.0, 1024, 128)
    with pytest.raises(RuntimeError, match="table"):
        engine.binding().pyin(a, fe._table(other, a.device), *cfg, False, 0.0)
    with pytest.raises(RuntimeError):
        engine.binding().pyin_observe(fe.pyin_cmnd(a), fe._table(cfg, a.device), *other)
    from nws_amd import _lib
    L = _lib.lib()
    table = fe._table(cfg, a.device)
    out_f, out_d, out_i = torch.empty(47, device="cuda"), torch.empty(47, dtype=torch.float64, device="cuda"), torch.empty(47, dtype=torch.int32, device="cuda")
    ws = torch.empty(L.nws_pyin_workspace_bytes(1, 6000, *cfg), dtype=torch.uint8, device="cuda")
    args = (a.data_ptr(), 1, 6000, *cfg, table.data_ptr(), 0, 0.0, out_f.data_ptr(), out_d.data_ptr(), out_i.data_ptr(), ws.data_ptr())
    assert L.nws_pyin(*args, ws.numel() - 1, None) == -3                   # workspace too small
    assert L.nws_pyin(a.data_ptr(), 1, 512, *args[3:], ws.numel(), None) == -2
    assert L.nws_pyin(a.data_ptr(), 1, 6000, 16000.0, 65.0, 2093.0, 4096, 128, *args[8:], ws.numel(), None) == -1
    assert L.nws_pyin(*args, ws.numel(), None) == 0
    torch.cuda.synchronize()
    assert np.array_equal(out_f.cpu().numpy().astype(np.float64), f0)


def test_timbre_transfer_script_writes_a_wav_of_the_inputs_length(tmp_path):
    t = np.arange(SR) / SR
    x = (0.3 * np.sin(2 * np.pi * 220.0 * t) * np.minimum(1.0, 10 * t)).astype(np.float32)
    src, dst = str(tmp_path / "in.wav"), str(tmp_path / "out.wav")
    wavfile.write(src, SR, x)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "timbre_transfer.py"), src, dst, "--use-fastnewt"],
                       capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    sr, y = wavfile.read(dst)
    assert sr == SR and y.shape == x.shape and y.dtype == np.float32 and np.isfinite(y).all() and np.abs(y).max() > 1e-4
    assert "median F0 2" in r.stdout, r.stdout                  # 220 Hz within a bin or two
    wavfile.write(src, 22050, x)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "timbre_transfer.py"), src, dst], capture_output=True,
                       text=True, timeout=300, cwd=ROOT)
    assert r.returncode != 0 and "resample" in r.stderr


def test_stage_times_on_the_bench_shape_and_one_minute():
    """no bar: there is no earlier implementation to compare with.  hipEvents on the launch stream, recorded for DESIGN.md"""
    import nws_amd  # noqa: F401
    from nws_amd.data.utils import f0_extraction as fe
    g = torch.Generator(device="cuda").manual_seed(3)
    for tag, shape in (("64x4s", (64, 64000)), ("1x60s", (1, 60 * SR))):
        t = torch.arange(shape[1], device="cuda") / SR
        a = (0.3 * torch.sin(2 * torch.pi * 220.0 * t)).repeat(shape[0], 1) + 0.01 * torch.randn(shape, device="cuda", generator=g)
        yin = fe.pyin_cmnd(a)
        obs = fe.pyin_observe(yin)
        fe.pyin_viterbi(*obs)
        steps = {"cmnd": lambda: fe.pyin_cmnd(a), "observe": lambda: fe.pyin_observe(yin), "viterbi": lambda: fe.pyin_viterbi(*obs),
                 "whole": lambda: fe.pyin_frames(a)}
        ms = {}
        for k, fn in steps.items():
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(3):
                fn()
            e1.record()
            e1.synchronize()
            ms[k] = e0.elapsed_time(e1) / 3
        record("pyin_time_" + tag, x_realtime=a.numel() / SR / (ms["whole"] * 1e-3), **{k + "_ms": v for k, v in ms.items()})
        print(tag, ms)
        assert all(np.isfinite(v) and v > 0 for v in ms.values())
