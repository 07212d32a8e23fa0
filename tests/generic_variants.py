"""Shared by test_cpu_generic_variants.py and test_gpu_generic_variants.py (plain numpy / torch-CPU, no GPU): the end-to-end
cases that steer NeuralWaveshaping.forward onto one kernel variant of csrc/generic.hip each, the product model and the oracle of
a case, the whole-signal and block-wise bars, and models of the defects the block-wise bar is there to catch.

A case's output is the PRE-reverb signal: reverb.ir is zero, Reverb.forward is x + conv(x, ir), so an error stays where the
kernel made it instead of being spread over a second of tail."""
import ctypes as C
import importlib

import numpy as np
import torch
import torch.nn.functional as F

from conftest import rms

BLOCK = 512            # samples per row and block: the largest span one workgroup of g_exciter_newt_mfma_kernel writes (tpw = 4)
REL_BAR = 1e-5         # x max(RMS(ref), 1e-3): the random sweep's bar (test_gpu_generic.py), whole-signal and per block
ABS_BAR = 1e-4

FAM_STAGES, FAM_MFMA, FAM_THREAD = 0, 1, 2
GRU_DEFAULT, GRU_QUAD, GRU_STREAM = 0, 1, 2


def _case(hop, T, B, S, OC=1, K=20, width=4, depth=3, C_total=2, f0=None, modes=("exact", "fast"), **plan):
    return dict(hop=hop, T=T, B=B, S=S, OC=OC, K=K, width=width, depth=depth, C_total=C_total, f0=f0, modes=modes, plan=plan)


# plan: what nws_debug_generic_exciter_plan must report for the case - `fast` / `exact`: (family, MT or SB, OCT, tpw), `grid`: tpw
# by the workgroup-count rule alone (where an LDS rule lowers it), `lds`: (low, high] bytes of the FastNEWT launch.
# B x ceil(N / 512) >= 1024 is what keeps tpw = 4: hop 16, T = 481, B = 64 is N = 7696, 16 spans per row, the last with 16 live samples.
CASES = {
    "tpw4": _case(16, 481, 64, 8, fast=(FAM_MFMA, 1, 1, 4), exact=(FAM_MFMA, 1, 0, 4)),
    # hop 25 divides neither 32 nor 128: tiles straddle frames, the staged FiLM window starts inside a frame (N = 7700)
    "tpw4_hop25": _case(25, 308, 64, 8, fast=(FAM_MFMA, 1, 1, 4), exact=(FAM_MFMA, 1, 0, 4)),
    # 16 x 34 = 544 < 1024 <= 31 x 34 = 1054 workgroups
    "tpw2": _case(16, 481, 34, 8, fast=(FAM_MFMA, 1, 1, 2), exact=(FAM_MFMA, 1, 0, 2)),
    # N = 368 = 2 x 128 + 112: three workgroups per row, the last tile with 16 live samples
    "mt2_s33": _case(16, 23, 2, 33, fast=(FAM_MFMA, 2, 1, 1), exact=(FAM_MFMA, 2, 0, 1)),
    "mt2_s48": _case(16, 23, 2, 48, fast=(FAM_MFMA, 2, 1, 1), exact=(FAM_MFMA, 2, 0, 1)),
    "mt2_s64": _case(16, 23, 2, 64, fast=(FAM_MFMA, 2, 1, 1), exact=(FAM_MFMA, 2, 0, 1)),
    # MT = 2 keeps tpw = 4 under the 40 KB goal only with few FiLM frames per span: hop 40 (15 frames, 40 320 B); N = 7720
    "mt2_tpw4": _case(40, 193, 64, 48, fast=(FAM_MFMA, 2, 1, 4), exact=(FAM_MFMA, 2, 0, 4), lds=(32768, 40960)),
    "oct4_oc3_mt1": _case(16, 23, 2, 8, OC=3, fast=(FAM_MFMA, 1, 4, 1), exact=(FAM_MFMA, 1, 0, 1)),
    "oct4_oc4_mt1": _case(16, 23, 2, 8, OC=4, fast=(FAM_MFMA, 1, 4, 1), exact=(FAM_MFMA, 1, 0, 1)),
    "oct4_oc3_mt2": _case(16, 23, 2, 40, OC=3, fast=(FAM_MFMA, 2, 4, 1), exact=(FAM_MFMA, 2, 0, 1)),
    "oct4_oc4_mt2": _case(16, 23, 2, 40, OC=4, fast=(FAM_MFMA, 2, 4, 1), exact=(FAM_MFMA, 2, 0, 1)),
    # the 40 KB goal lowers tpw 4 -> 2 (67 -> 35 staged frames, 40 704 B)
    "lds_goal_hop8": _case(8, 961, 64, 8, fast=(FAM_MFMA, 1, 1, 2), exact=(FAM_MFMA, 1, 0, 4), grid=4, lds=(32768, 40960)),
    # hop 8 with 64 shapers: NO tpw meets the goal (tpw = 1 is 48 512 B), so the goal leaves tpw alone and the
    # two-workgroups-per-CU rule (80 KB) lowers it 4 -> 2 (81 280 B)
    "lds_80k_hop8_s64": _case(8, 961, 64, 64, width=2, depth=2, fast=(FAM_MFMA, 2, 1, 2), exact=(FAM_MFMA, 2, 0, 4), grid=4,
                              lds=(40960, 81920)),
    # 1250 harmonics: the fp16 mixer fragments (79 K-steps x 2 112 B) exceed 160 KB, the thread-per-sample kernel runs;
    # N = 320: two workgroups, the second with 64 live samples.  F0 of 5 .. 15 Hz keeps hundreds of harmonics below Nyquist
    "sb8": _case(16, 20, 1, 5, K=1250, f0=(5.0, 15.0), fast=(FAM_THREAD, 8, 1, 0), exact=(FAM_THREAD, 8, 0, 0)),
    "sb16": _case(16, 20, 1, 12, K=1250, f0=(5.0, 15.0), fast=(FAM_THREAD, 16, 1, 0), exact=(FAM_THREAD, 16, 0, 0)),
    "sb32": _case(16, 20, 1, 20, K=1250, f0=(5.0, 15.0), fast=(FAM_THREAD, 32, 1, 0), exact=(FAM_THREAD, 32, 0, 0)),
    # |phase| x (16 K16 + 1) > 6e6: F0 of 0.11 .. 0.125 sr (four harmonics below Nyquist) over 294 912 samples ends at a phase of
    # ~2.2e5 rad, x 33 = 7.2e6: the last fifth of the row takes g_mix_tile<MT, true>
    "wide": _case(64, 4608, 1, 4, K=24, f0=(1760.0, 2000.0), fast=(FAM_MFMA, 1, 1, 2), exact=(FAM_MFMA, 1, 0, 2)),
    # one row of 262 272 > 2048 x 128 samples: the second trip of g_film_shaper_kernel<16>'s grid-stride loop
    "film16_long": _case(128, 2049, 1, 2, width=16, modes=("exact",), exact=(FAM_MFMA, 1, 0, 2)),
    # control (B, 4, T): the recurrence reads the first two of four channels (C_total > C_in)
    "control_extra": _case(16, 23, 3, 8, C_total=4, fast=(FAM_MFMA, 1, 1, 1), exact=(FAM_MFMA, 1, 0, 1)),
}
SR = 16000
TABLE = dict(table_size=512, table_min=-4.0, table_max=4.0)


def gin_text(c):
    hop, S = c["hop"], c["S"]
    ir = 2 * (hop // 2 + 2)                      # even, >= hop + 2
    return f"""
Reverb.sr = 500
Reverb.length_in_seconds = 1
noise_synth/FIRNoiseSynth.hop_length = {hop}
noise_synth/FIRNoiseSynth.ir_length = {ir}
noise_synth/TimeDistributedMLP.depth = 3
noise_synth/TimeDistributedMLP.out_size = {ir // 2 + 1}
noise_synth/TimeDistributedMLP.hidden_size = 20
noise_synth/TimeDistributedMLP.in_size = 12
TrainableNonlinearity.depth = {c["depth"]}
NEWT.shaping_fn_size = {c["width"]}
NEWT.out_channels = {c["OC"]}
NEWT.control_embedding_size = 12
NEWT.n_waveshapers = {S}
HarmonicOscillator.sample_rate = {SR}
HarmonicOscillator.n_harmonics = {c["K"]}
ControlModule.embedding_size = 12
ControlModule.hidden_size = 24
ControlModule.control_size = 2
NeuralWaveshaping.sample_rate = {SR}
NeuralWaveshaping.control_hop = {hop}
NeuralWaveshaping.n_waveshapers = {S}
"""


class configured:
    """`with configured(case):` - the case's gin bindings, the default configuration restored afterwards"""

    def __init__(self, c):
        self.c = c

    def __enter__(self):
        nws = importlib.import_module("neural-waveshaping-synthesis_amd")
        nws.gin.clear_config()
        nws.gin.parse_config(gin_text(self.c))
        return nws

    def __exit__(self, *exc):
        nws = importlib.import_module("neural-waveshaping-synthesis_amd")
        nws.gin.clear_config()
        nws.gin.parse_config_file(nws.DEFAULT_GIN)
        return False


def build_model(nws, name):
    """The product's own constructors under the case's gin bindings (call inside `configured`), as the random sweep of
    test_gpu_generic.py builds its models: LUT argument kept inside the table - and a silent reverb.  Returns (model on the CPU,
    state dict as numpy)."""
    c = CASES[name]
    S = c["S"]
    torch.manual_seed(sum(map(ord, name)))
    m = nws.NeuralWaveshaping().eval()
    with torch.no_grad():
        m.reverb.ir.zero_()
        m.newt.mlp.net[-1].weight[:2 * S] *= 0.5
        m.newt.mlp.net[-1].bias[:2 * S] *= 0.5
        m.newt.shaping_fn.input_scale.mul_(0.3)
    return m, {k: v.detach().cpu().numpy().copy() for k, v in m.state_dict().items()}


def inputs(name):
    c = CASES[name]
    rng = np.random.default_rng(sum(map(ord, name)))
    B, T, hop = c["B"], c["T"], c["hop"]
    if c["f0"] is None:      # the sweep's F0: some harmonics cross Nyquist
        f0 = (100.0 + 0.3 * SR * rng.random((B, 1, 1)) * rng.random((B, 1, T))).astype(np.float32)
    else:
        lo, hi = c["f0"]
        f0 = (lo + (hi - lo) * rng.random((B, 1, T))).astype(np.float32)
    control = rng.standard_normal((B, c["C_total"], T)).astype(np.float32)
    pu = rng.random(c["K"]).astype(np.float32)
    nz = rng.random(hop * T - 1).astype(np.float32)
    return f0, control, pu, nz


def make_oracle(w, c, fast):
    from oracle.newt_oracle import OracleNEWT

    return OracleNEWT(w, fast=fast, lut_python_loop=False, sample_rate=SR, control_hop=c["hop"], **TABLE)


def size_only_desc(c, fast):
    """NwsGenericModel with the sizes the plan query reads (no GPU, no pointers but a non-NULL stand-in for the table)"""
    _lib = importlib.import_module("neural-waveshaping-synthesis_amd._lib")
    g = _lib.NwsGenericModel()
    g.n_shapers, g.n_harmonics, g.out_channels, g.hop = c["S"], c["K"], c["OC"], c["hop"]
    g.shaper.n_shapers = c["S"]
    if fast:
        g.shaper.lut = 1
    return g


def exciter_plan(desc, B, T):
    _lib = importlib.import_module("neural-waveshaping-synthesis_amd._lib")
    out = (C.c_int * 8)()
    rc = _lib.lib().nws_debug_generic_exciter_plan(C.byref(desc), B, T, out)
    assert rc == 0, rc
    return dict(zip(("family", "size", "oct", "tpw", "nf", "lds", "follow", "tpw_grid"), out))


def gru_plan(hidden, c_in):
    _lib = importlib.import_module("neural-waveshaping-synthesis_amd._lib")
    out = (C.c_int * 4)()
    rc = _lib.lib().nws_debug_generic_gru_plan(hidden, c_in, out)
    assert rc == 0, rc
    return dict(zip(("kernel", "kq", "threads", "lds"), out))


def assert_plan(name, mode, p):
    """the case launches the variant it is named for"""
    c = CASES[name]
    want = c["plan"][mode]
    assert (p["family"], p["size"], p["oct"], p["tpw"]) == want, (name, mode, p)
    assert p["follow"] == (1 if mode == "exact" else 0), (name, mode, p)
    if mode == "fast":
        if "grid" in c["plan"]:
            assert p["tpw_grid"] == c["plan"]["grid"] > p["tpw"], (name, p)          # an LDS rule lowered tpw
        if "lds" in c["plan"]:
            lo, hi = c["plan"]["lds"]
            assert lo < p["lds"] <= hi, (name, p)
    if p["family"] == FAM_MFMA:
        assert p["nf"] == 128 * p["tpw"] // c["hop"] + 3, (name, p)


def errors(y, ref):
    """(whole-signal RMS error, worst RMS error over the blocks of 512 samples of every row, scale = max(RMS(ref), 1e-3))"""
    y, ref = np.asarray(y, np.float64), np.asarray(ref, np.float64)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    d2 = (y - ref) ** 2
    N = d2.shape[-1]
    edges = np.arange(0, N, BLOCK)
    sums = np.add.reduceat(d2, edges, axis=-1)
    counts = np.diff(np.append(edges, N))
    worst = float(np.sqrt((sums / counts).max()))
    return rms(y - ref), worst, max(rms(ref), 1e-3)


def passes(y, ref):
    e, worst, scale = errors(y, ref)
    return e <= ABS_BAR and e <= REL_BAR * scale and worst <= REL_BAR * scale


# ---- stage cases ----------------------------------------------------------------------------------------------------------
# (hidden, C_in) -> (kernel, kq, workgroup size) that nws_debug_generic_gru_plan must report
GRU_PLANS = {(1, 1): (GRU_QUAD, 8, 64), (16, 2): (GRU_QUAD, 8, 64), (17, 3): (GRU_QUAD, 8, 128), (32, 2): (GRU_QUAD, 8, 128),
             (33, 2): (GRU_QUAD, 16, 192), (64, 5): (GRU_QUAD, 16, 256), (65, 2): (GRU_QUAD, 32, 320),
             (127, 2): (GRU_QUAD, 32, 512), (128, 3): (GRU_QUAD, 32, 512), (128, 44): (GRU_STREAM, 0, 256),
             (129, 2): (GRU_STREAM, 0, 256), (256, 2): (GRU_STREAM, 0, 256), (128, 2): (GRU_DEFAULT, 0, 0),
             (16, 70): (GRU_STREAM, 0, 256)}


def random_mlp(in_size, hidden, out_size, depth, seed, dtype=torch.float32):
    """weights / biases / LayerNorm gains / offsets of a TimeDistributedMLP (Conv1d's own initialisation, gains about 1)"""
    g = torch.Generator().manual_seed(seed)
    ws, bs, gs, ls = [], [], [], []
    for i in range(depth):
        cin = in_size if i == 0 else hidden
        cout = out_size if i == depth - 1 else hidden
        k = 1.0 / np.sqrt(cin)
        ws.append(((torch.rand(cout, cin, generator=g) * 2 - 1) * k).to(dtype))
        bs.append(((torch.rand(cout, generator=g) * 2 - 1) * k).to(dtype))
        if i < depth - 1:
            gs.append((1.0 + 0.2 * torch.randn(cout, generator=g)).to(dtype))
            ls.append((0.1 * torch.randn(cout, generator=g)).to(dtype))
    return ws, bs, gs, ls


# ---- defects ------------------------------------------------------------------------------------------------------------------
DEFECTS = {"film_frame_early": "tpw4_hop25", "shapers_32_up_dropped": "mt2_s48", "channel_3_dropped": "oct4_oc4_mt2",
           "row_tail_zero": "mt2_s33"}


def defective_output(o, st, defect, tpw=4):
    """What the forward would return for the oracle's own intermediates `st` (OracleNEWT.forward(..., stages=st), silent reverb)
    if the oscillator-to-NEWT kernel had one defect:
      film_frame_early       the last 32-sample tile of ONE span of 128 tpw samples (row 0, the span in the middle) interpolates
                             its FiLM rows one frame early - a staging window that starts one frame off for that tile
      shapers_32_up_dropped  shapers 32 and up never reach the NEWT mixer (the second M-tile is lost)
      channel_3_dropped      NEWT output channel 3 is never written (counts as zero)
      row_tail_zero          the last N mod 32 samples of row 0 never get their NEWT output (the partial tile is skipped)"""
    exciter, film = st["exciter"], st["film"]
    N, S = exciter.shape[-1], o.n_waveshapers
    up = F.interpolate(film, size=N, mode="linear")
    if defect == "film_frame_early":
        early = F.interpolate(torch.cat((film[..., :1], film[..., :-1]), dim=-1), size=N, mode="linear")
        span = 128 * tpw
        end = span * (N // span // 2 + 1)
        up = up.clone()
        up[0, :, end - 32:end] = early[0, :, end - 32:end]
    g_i, b_i, g_n, b_n = torch.split(up, S, 1)
    x = g_i * exciter + b_i
    x = o.lut_shaper(x) if o.fast else o.exact_shaper(x)
    x = g_n * x + b_n
    wmix = o.w["newt.mixer.0.weight"].clone()
    if defect == "shapers_32_up_dropped":
        wmix[:, 32:] = 0.0
    newt = F.conv1d(x, wmix, o.w["newt.mixer.0.bias"])
    if defect == "channel_3_dropped":
        newt[:, 3] = 0.0
    if defect == "row_tail_zero":
        assert N % 32
        newt[0, :, N - N % 32:] = 0.0
    return (torch.cat((newt, st["noise_out"].unsqueeze(1)), dim=1).sum(1)).numpy()
