"""The two size sets of the runtime-size stream's tests (tests/test_gpu_g_streaming.py, tests/test_cpu_g_streaming.py), built
from gin text with seeded initialisation; the packaged gin is put back whatever happens.

bank: the packaged file with 12 shapers of width 16 and depth 3 on 40 harmonics (the bank tests/test_gpu_training_sizes.py
trains); everything else is packaged, so the recurrence is the packaged kernel with carried state.
odd: nothing divides anything - 5 shapers of width 3 and depth 2, 7 harmonics, two NEWT output channels, a GRU of 33 units,
a 17-d embedding, h_generator 17 -> 20 -> 20 -> 129, 8 kHz, a reverb of 999 taps; hop 128 and 256 noise taps as the stream needs."""
import numpy as np
import torch

BANK_GIN = """
NeuralWaveshaping.n_waveshapers = 12
NEWT.n_waveshapers = 12
NEWT.shaping_fn_size = 16
TrainableNonlinearity.depth = 3
HarmonicOscillator.n_harmonics = 40
"""

ODD_GIN = """
Reverb.sr = 1000
Reverb.length_in_seconds = 1
noise_synth/FIRNoiseSynth.hop_length = 128
noise_synth/FIRNoiseSynth.ir_length = 256
noise_synth/TimeDistributedMLP.depth = 3
noise_synth/TimeDistributedMLP.out_size = 129
noise_synth/TimeDistributedMLP.hidden_size = 20
noise_synth/TimeDistributedMLP.in_size = 17
TrainableNonlinearity.depth = 2
NEWT.shaping_fn_size = 3
NEWT.out_channels = 2
NEWT.control_embedding_size = 17
NEWT.n_waveshapers = 5
HarmonicOscillator.sample_rate = 8000
HarmonicOscillator.n_harmonics = 7
ControlModule.embedding_size = 17
ControlModule.hidden_size = 33
ControlModule.control_size = 2
NeuralWaveshaping.sample_rate = 8000
NeuralWaveshaping.control_hop = 128
NeuralWaveshaping.n_waveshapers = 5
"""

SIZES = {"bank": (BANK_GIN, 16000, 12, 40), "odd": (ODD_GIN, 8000, 5, 7)}      # gin text, sample rate, shapers, harmonics
TABLE = dict(table_size=512, table_min=-4.0, table_max=4.0)


def build_from_gin(text, seed=0, fast=False, device="cuda", packaged_first=True):
    """(model on `device`, state dict as numpy) of the configuration `text` names, with the initialisation of
    tests/test_gpu_generic.py's sweep: an audible impulse response and the table's argument kept inside the table."""
    import nws_amd as nws

    nws.gin.clear_config()
    try:
        if packaged_first:
            nws.gin.parse_config_file(nws.DEFAULT_GIN)
        nws.gin.parse_config(text)
        torch.manual_seed(seed)
        m = nws.NeuralWaveshaping().eval()
        S = m.newt.n_waveshapers
        with torch.no_grad():
            L = m.reverb.ir.numel()
            m.reverb.ir.copy_(torch.randn_like(m.reverb.ir) * 0.05 * torch.exp(-torch.arange(L) / (L / 4.0)))
            m.newt.mlp.net[-1].weight[:2 * S] *= 0.5
            m.newt.mlp.net[-1].bias[:2 * S] *= 0.5
            m.newt.shaping_fn.input_scale.mul_(0.3)
        w = {k: v.detach().cpu().numpy() for k, v in m.state_dict().items()}
        m = m.to(device)
        if fast:
            m.newt = nws.FastNEWT(m.newt, **TABLE)
        return m, w
    finally:
        nws.gin.clear_config()
        nws.gin.parse_config_file(nws.DEFAULT_GIN)


def build(sizes, fast, seed=0, device="cuda"):
    text = SIZES[sizes][0]
    return build_from_gin(text, seed=seed, fast=fast, device=device, packaged_first=(sizes == "bank"))


def oracle_for(sizes, w, fast):
    from oracle.newt_oracle import OracleNEWT

    return OracleNEWT(w, sample_rate=SIZES[sizes][1], control_hop=128, fast=fast, lut_python_loop=False, **TABLE)


def inputs(sizes, B, F, seed):
    """f0 / control / the two hidden draws, drawn as tests/test_gpu_streaming.py::test_stream_equals_one_shot draws them"""
    K = SIZES[sizes][3]
    g = torch.Generator().manual_seed(seed)
    f0 = (120 + 600 * torch.rand(B, 1, 1, generator=g)) * (1 + 0.03 * torch.randn(B, 1, F, generator=g))
    control = torch.randn(B, 2, F, generator=g)
    pu, nz = torch.rand(K, generator=g), torch.rand(128 * F - 1, generator=g)
    return f0, control, pu, nz


def run_stream(model, chunks, f0, control, pu, nz, **kw):
    """push the chunk schedule; -> (stream, output (B, 128 F), pre-reverb tap (B, 128 F)) as numpy"""
    B = f0.shape[0]
    s = model.stream(B, phase_u=pu.cuda(), noise=None if nz is None else nz.cuda(), **kw)
    ys, pres, k = [], [], 0
    for i, K in enumerate(chunks):
        y = s.push(f0[:, :, k:k + K].cuda(), control[:, :, k:k + K].cuda(), final=(i == len(chunks) - 1))
        ys.append(y.cpu().numpy())
        pres.append(s._last_pre.cpu().numpy())
        k += K
    return s, np.concatenate(ys, axis=1), np.concatenate(pres, axis=1)
