"""-m gpu: the B >= 16 FIR-noise kernel (csrc/fir_noise.hip, fir_noise_spectral_kernel: per-frame circular convolution as a
product of spectra, two frames of one utterance per complex 256-point transform, runs of seven hops per wave).

Bars are the stage test's (tests/test_gpu_parity.py): max-abs row error <= 2e-6 * row max + 1e-12 against the oracle's
STFT / iSTFT formulation, the same against the packed-fp32 kernel that serves B < 16 where the oracle cannot run.  Shapes are
chosen around the kernel's seams: runs of 7 hops (T = 8, 9, 33, 500, 501 end a run after 1, 2, 5, 3, 4 hops), frame pairs that
start one frame before the run, eight utterances per workgroup and two per wave in the halves of packed instructions (B = 17, 33, 65
leave one live HALF of one wave in the last workgroup: its partner is the same row again, computed and not stored)."""
import numpy as np
import pytest
import torch

from gpu_util import build_model

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def oracle(weights):
    from oracle.newt_oracle import OracleNEWT

    return OracleNEWT(weights, fast=False)


@pytest.fixture(scope="module")
def eng():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return build_model(False)._engine


def taps_from_h(H):
    """(B, 129, T) filter magnitudes -> (B, T, 128) upper half-taps, the layout nws_fir_noise takes"""
    Ht = H.transpose(1, 2)
    h = torch.fft.irfft(torch.complex(Ht, torch.zeros_like(Ht))).roll(128, -1) * torch.hann_window(256).view(1, 1, -1)
    return h[..., 128:].contiguous()


def make_case(B, T, seed=None):
    g = torch.Generator().manual_seed(100 * B + T if seed is None else seed)
    H = 0.02 * torch.rand(B, 129, T, generator=g) ** 3 + 1e-4
    H[0] *= 50.0                                    # one loud utterance, one (nearly) silent
    H[1] *= 1e-4
    noise = torch.rand(max(128 * T - 1, 2), generator=g)
    add = torch.randn(B, 128 * T, generator=g)
    return H, noise, add


def small_kernel(eng, h, noise, **kw):
    """the packed-fp32 kernel of B < 16, on slices of 8 rows"""
    return torch.cat([eng.fir_noise(h[i:i + 8].contiguous(), noise, **kw) for i in range(0, h.shape[0], 8)])


@pytest.mark.parametrize("T", [2, 3, 8, 9, 33, 500, 501])
@pytest.mark.parametrize("B", [16, 17, 33, 64, 65])
def test_spectral_kernel_against_oracle(eng, oracle, B, T):
    H, noise, add = make_case(B, T)
    ref = oracle.fir_noise(H, noise)[:, 0].numpy()
    h = taps_from_h(H).cuda()
    out = eng.fir_noise(h, noise.cuda()).cpu().numpy()
    rowmax = np.abs(ref).max(axis=1)
    err = np.abs(out - ref).max(axis=1)
    print(f"B={B} T={T}: worst row error / row max = {(err / rowmax).max():.3e} (bar 2e-6)")
    assert np.all(err <= 2e-6 * rowmax + 1e-12), (err / rowmax).max()
    # add_in: the other branch's samples are added last, in fp32, to the value the call without them stores: the same bits
    # as that one addition done here
    out2 = eng.fir_noise(h, noise.cuda(), add_in=add.cuda()).cpu().numpy()
    assert np.array_equal(out2, add.numpy() + out)


@pytest.mark.parametrize("B", [16, 65])
def test_single_frame_against_small_kernel(eng, B):
    """T = 1: the oracle's reflect padding needs more than 128 noise samples, so the packed-fp32 kernel is the reference"""
    H, noise, add = make_case(B, 1)
    h = taps_from_h(H).cuda()
    ref = small_kernel(eng, h, noise.cuda()).cpu().numpy()
    out = eng.fir_noise(h, noise.cuda()).cpu().numpy()
    rowmax = np.abs(ref).max(axis=1)
    err = np.abs(out - ref).max(axis=1)
    print(f"B={B} T=1: worst row error / row max = {(err / rowmax).max():.3e} (bar 2e-6)")
    assert np.all(err <= 2e-6 * rowmax + 1e-12), (err / rowmax).max()
    out2 = eng.fir_noise(h, noise.cuda(), add_in=add.cuda()).cpu().numpy()
    assert np.array_equal(out2, add.numpy() + out)


@pytest.mark.parametrize("B,T", [(16, 9), (33, 16), (64, 3)])
def test_window_form_against_small_kernel(eng, B, T):
    """nws_fir_noise_window with origin 0 (frame t covers noise[128 t, +256)) and a noise_len that ends inside the last frame,
    so the reflection at the stream's end is exercised.  With add_in the stored value is one fp32 addition on top of what the call
    without it stores: checked as those exact bits, so the relative bar of the quiet rows is not diluted by the sum's rounding"""
    H, _, add = make_case(B, T)
    g = torch.Generator().manual_seed(7 * B + T)
    n_len = 128 * (T - 1) + 100
    noise = torch.rand(128 * (T + 1), generator=g).cuda()
    h = taps_from_h(H).cuda()
    ref = small_kernel(eng, h, noise, origin=0, noise_len=n_len).cpu().numpy()
    out = eng.fir_noise(h, noise, origin=0, noise_len=n_len).cpu().numpy()
    rowmax = np.abs(ref).max(axis=1)
    err = np.abs(out - ref).max(axis=1)
    print(f"window B={B} T={T}: worst row error / row max = {(err / rowmax).max():.3e} (bar 2e-6)")
    assert np.all(err <= 2e-6 * rowmax + 1e-12), (err / rowmax).max()
    out2 = eng.fir_noise(h, noise, add_in=add.cuda(), origin=0, noise_len=n_len).cpu().numpy()
    assert np.array_equal(out2, add.numpy() + out)


def test_bits_repeat_and_do_not_depend_on_the_batch(eng):
    B, T = 64, 33
    H, noise, _ = make_case(B, T)
    h = taps_from_h(H).cuda()
    nz = noise.cuda()
    out = eng.fir_noise(h, nz)
    assert torch.equal(out, eng.fir_noise(h, nz))
    for i in range(0, B, 16):
        assert torch.equal(out[i:i + 16], eng.fir_noise(h[i:i + 16].contiguous(), nz)), i
    # a row's neighbours in the workgroup change (rows 3 .. 18 put old row 3 into wave 0)
    assert torch.equal(out[3:19], eng.fir_noise(h[3:19].contiguous(), nz))


def test_bad_taps_stay_inside_their_utterance(eng):
    B, T = 64, 33
    H, noise, _ = make_case(B, T)
    h = taps_from_h(H).cuda()
    nz = noise.cuda()
    clean = eng.fir_noise(h, nz)
    bad = h.clone()
    bad[5] = float("nan")
    bad[20] = float("inf")
    bad[41, 7, 3] = float("nan")          # one tap of one frame
    out = eng.fir_noise(bad, nz)
    keep = [b for b in range(B) if b not in (5, 20, 41)]
    assert torch.equal(out[keep], clean[keep])
    for b in (4, 6, 19, 21, 40, 42):
        assert bool(torch.isfinite(out[b]).all()), b
    # inside the utterance a bad frame reaches its own two hops and, through its pair partner, at most one hop more each way
    touched = (out[41] != clean[41]).view(T, 128).any(dim=1).nonzero().flatten().tolist()
    assert touched and set(touched) <= {6, 7, 8, 9}, touched
