"""The spectrum hand-over between the frame MLPs and the noise kernel (include/nws_hip.h): proj folded into the
first hidden layer of newt.mlp and of h_generator, h_generator's output layer emitting the real filter spectrum G = S H, and the
batched noise kernel reading G instead of half-taps.

CPU part (no GPU): the library's host fold against a float64 restatement from tests/golden/weights_vn.npz, and S against the
transform the noise kernel runs (csrc/fir_spectral_fft.h compiled for the host, on the kernel's own even extension of the designed
half rows).  GPU part (-m gpu): the folded wave-resident kernel, the spectrum-in noise kernel, the forward end to end and the
range guard.  Bars are stated at each check."""
import importlib
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from conftest import ROOT, rms

PKG = "neural-waveshaping-synthesis_amd"
WEIGHTS = os.path.join(ROOT, "tests", "golden", "weights_vn.npz")
H_, NB = 128, 129


def _lib():
    return importlib.import_module(PKG + "._lib")


def design_matrix(window):
    """nws_fir_design_matrix restated: D[n][k] = window[n] c_k cos(2 pi k (n - 128) / 256) / 256, fp32, (256, 132)"""
    n, k = np.arange(256), np.arange(NB)
    m = (n - 128) & 255
    c = np.where((k == 0) | (k == 128), 1.0, 2.0)
    D = np.zeros((256, 132), np.float32)
    D[:, :NB] = (np.asarray(window, np.float64)[:, None] * c[None] * np.cos(2 * np.pi * ((m[:, None] * k[None]) & 255) / 256) / 256)
    return D


def spectrum_map(D):
    S = torch.empty(NB * NB, dtype=torch.float64)
    Dt = torch.from_numpy(np.ascontiguousarray(D, dtype=np.float32))
    assert _lib().lib().nws_fir_spectrum_map(Dt.data_ptr(), S.data_ptr()) == 0
    return S.view(NB, NB).numpy()


def cpu_model():
    nws = importlib.import_module(PKG)
    nws.ensure_default_config()
    return nws.NeuralWaveshaping.load_from_checkpoint(WEIGHTS)


def split_folded(f):
    f = np.asarray(f)
    o = 2 * H_ * H_ + NB * H_
    return dict(w1n=f[:H_ * H_].reshape(H_, H_), w1h=f[H_ * H_:2 * H_ * H_].reshape(H_, H_), wg=f[2 * H_ * H_:o].reshape(NB, H_),
                b1n=f[o:o + H_], b1h=f[o + H_:o + 2 * H_], bg=f[o + 2 * H_:o + 2 * H_ + NB], pad=f[o + 2 * H_ + NB:])


# ---- CPU ---------------------------------------------------------------------------------------------------------------------
def test_folded_weights_against_float64_restatement(weights):
    """W1' = W1 Wp, b1' = W1 bp + b1 (both paths), W_G = S W_out, b_G = S b_out: float64 sums rounded once to fp32, so the
    library's values are the rounded restatement up to the last place (2^-23 relative; 1e-10 absolute for entries that cancel)"""
    m = cpu_model()
    D = design_matrix(weights["noise_synth.window"])
    got = split_folded(m._engine.spec_fold(torch.from_numpy(D)).numpy())
    w = {k: np.asarray(v, np.float64) for k, v in weights.items()}
    Wp, bp = w["embedding.proj.weight"][:, :, 0], w["embedding.proj.bias"]
    S = spectrum_map(D)
    ref = {}
    for tag, pre in (("n", "newt.mlp"), ("h", "h_generator")):
        W1, b1 = w[pre + ".net.0.weight"][:, :, 0], w[pre + ".net.0.bias"]
        ref["w1" + tag], ref["b1" + tag] = W1 @ Wp, W1 @ bp + b1
    ref["wg"], ref["bg"] = S @ w["h_generator.net.9.weight"][:, :, 0], S @ w["h_generator.net.9.bias"]
    for k, r in ref.items():
        assert got[k].dtype == np.float32 and got[k].shape == r.shape, k
        err = np.abs(got[k].astype(np.float64) - r)
        assert np.all(err <= 2.0 ** -23 * np.abs(r) + 1e-10), (k, float(err.max()))
    assert np.all(got["pad"] == 0.0) and got["pad"].size == 3
    # the shipped weights pass the range guard; scaled so that only the folded product outgrows it, they fail it alone
    assert m._engine.fp16_mlp_safe() and m._engine.fp16_spec_safe(m._engine.spec_fold(torch.from_numpy(D)))
    with torch.no_grad():
        m.embedding.proj.weight.mul_(30.0)
        m.newt.mlp.net[0].weight.mul_(30.0)
    assert m._engine.fp16_mlp_safe() and not m._engine.fp16_spec_safe(m._engine.spec_fold(torch.from_numpy(D)))


SPEC_HARNESS = r"""
#include <cmath>
#include <cstdio>
#include <cstdlib>
#define NWS_SP_FN inline
#define NWS_SP_TABLE static const
#include "fir_spectral_fft.h"
// the lane-by-lane walk of sp_fft256 of tests/test_fir_spectral_fft.py
static void fft256(C16 (&z)[16]) {
  float tw[1024], xr[kSpPlane], xi[kSpPlane];
  for (int k = 0; k < 16; ++k) for (int q = 0; q < 16; ++q) {
    float* e = &tw[kSpTwStride * k + 4 * q];
    sp_twiddle(q * k, e[0], e[2]);
    e[1] = e[0]; e[3] = e[2];
  }
  for (int l = 0; l < 16; ++l) {
    sp_pass1<false>(z[l], &tw[4 * l]);
    for (int k = 0; k < 16; ++k) { xr[k * kSpRow + l] = z[l].re[k]; xi[k * kSpRow + l] = z[l].im[k]; }
  }
  for (int l = 0; l < 16; ++l) {
    for (int j = 0; j < 16; ++j) { z[l].re[j] = xr[l * kSpRow + j]; z[l].im[j] = xi[l * kSpRow + j]; }
    sp_dft16<false>(z[l]);
  }
}
// stdin: pairs of half rows u_a[128], u_b[128]; stdout: (lane k1, register k2) of sp_filter_spectrum's result as G_a, G_b of bin
// k1 + 16 k2, 256 bins each.  The even extension is the kernel's: e[16 j + l] = u[16 j + l] for j < 8, u[128] := 0, else u[256 - n].
int main() {
  float ua[129], ub[129];
  for (;;) {
    for (int d = 0; d < 128; ++d) if (scanf("%f", &ua[d]) != 1) return 0;
    for (int d = 0; d < 128; ++d) if (scanf("%f", &ub[d]) != 1) return 1;
    ua[128] = ub[128] = 0.0f;
    C16 g[16];
    for (int l = 0; l < 16; ++l) for (int j = 0; j < 16; ++j) {
      const int n = 16 * j + l, d = n <= 128 ? n : 256 - n;
      g[l].re[j] = ua[d]; g[l].im[j] = ub[d];
    }
    fft256(g);
    for (int k = 0; k < 256; ++k) printf("%.9e %.9e\n", g[k & 15].re[k >> 4], g[k & 15].im[k >> 4]);
  }
}
"""


def test_spectrum_map_against_the_kernels_transform(weights, tmp_path):
    """S by its definition in float64 (real DFT of the even extension of the designed half rows), and against what
    sp_filter_spectrum computes from those half rows: sign, scale and bin order are the kernel's own, read off the header it runs.
    A 256-point fp32 transform is good to 4e-6 of the largest bin (tests/test_fir_spectral_fft.py)."""
    D = design_matrix(weights["noise_synth.window"])
    S = spectrum_map(D)
    u = D[128:, :NB].astype(np.float64)                           # u[d][band]
    e = np.zeros((256, NB))
    e[:128] = u
    e[129:] = u[1:][::-1]                                         # e[256 - d] = u[d], e[128] = 0
    assert np.abs(S - np.fft.rfft(e, axis=0).real).max() <= 1e-13
    # periodic Hann: the three-tap smoothing (1/4, 1/2, 1/4), doubled onto the edge bins
    assert abs(S[64, 64] - 0.5) < 1e-6 and abs(S[64, 63] - 0.25) < 1e-6 and abs(S[64, 65] - 0.25) < 1e-6 and abs(S[0, 1] - 0.5) < 1e-6
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "no host C++ compiler (the package's own build needs one too)"
    src, exe = tmp_path / "spec_harness.cpp", tmp_path / "spec_harness"
    src.write_text(SPEC_HARNESS)
    subprocess.run([cxx, "-O1", "-std=c++17", "-ffp-contract=off", f"-I{os.path.join(ROOT, PKG, 'csrc')}", str(src), "-o", str(exe)],
                   check=True)
    rng = np.random.default_rng(5)
    Hs = np.zeros((6, NB))
    for i, band in enumerate((0, 1, 64, 127, 128)):
        Hs[i, band] = 1.0                                         # unit band vectors
    Hs[5] = rng.uniform(0.0, 1.0, NB) ** 3
    rows = (D[128:, :NB] @ Hs.T.astype(np.float32)).T.astype(np.float32)          # half rows as the frame MLPs would store them
    text = "\n".join(" ".join(f"{v:.9e}" for v in np.concatenate([rows[2 * p], rows[2 * p + 1]])) for p in range(3))
    out = subprocess.run([str(exe)], input=text + "\n", check=True, capture_output=True, text=True).stdout
    G = np.array([[float(x) for x in line.split()] for line in out.splitlines()]).reshape(3, 256, 2)
    for i in range(6):
        got = G[i // 2, :, i % 2]
        ref = S @ Hs[i]
        big = np.abs(ref).max()
        assert np.abs(got[:NB] - ref).max() <= 4e-6 * big, (i, np.abs(got[:NB] - ref).max() / big)
        assert np.abs(got[129:] - ref[1:128][::-1]).max() <= 4e-6 * big      # G[256 - k] = G[k]: what the noise kernel reads by address


# ---- GPU ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def models():
    from gpu_util import build_model

    assert torch.cuda.is_available(), "these tests need the MI355X"
    return build_model(False), build_model(True)


@pytest.fixture(scope="module")
def S64(models):
    return spectrum_map(models[0]._engine.fir_design().cpu().numpy().reshape(256, 132))


def frame_path64(w, gru):
    """float64: gru (B, T, 128) -> film (B, T, 256), H (B, T, 129), G (B, T, 129) = the real spectrum of the frame's zero-phase
    filter window * roll(irfft(H)), rolled back (generators.py:22-27)"""
    w = {k: torch.as_tensor(np.asarray(v), dtype=torch.float64) for k, v in w.items()}
    x0 = gru.double() @ w["embedding.proj.weight"][:, :, 0].T + w["embedding.proj.bias"]

    def mlp(pre):
        x = x0
        for i in range(4):
            x = x @ w[f"{pre}.net.{3 * i}.weight"][:, :, 0].T + w[f"{pre}.net.{3 * i}.bias"]
            if i < 3:
                ln = f"{pre}.net.{3 * i + 1}.layer_norm"
                x = torch.nn.functional.leaky_relu(torch.nn.functional.layer_norm(x, (H_,), w[ln + ".weight"], w[ln + ".bias"]), 0.01)
        return x

    film, H = mlp("newt.mlp"), mlp("h_generator")
    h = torch.fft.irfft(torch.complex(H, torch.zeros_like(H))).roll(128, -1) * w["noise_synth.window"].view(1, 1, -1)
    return film, H, torch.fft.rfft(h.roll(-128, -1)).real


def taps_to_spectrum64(u):
    """float64: stored half rows (.., 128) -> G (.., 129), the even extension's real DFT (no rounding of its own worth the name)"""
    d, k = np.arange(128), np.arange(NB)
    C = 2.0 * np.cos(2 * np.pi * ((k[:, None] * d[None]) & 255) / 256)
    C[:, 0] = 1.0
    return u.double() @ torch.from_numpy(C.T)


def row_err(x, ref):
    """worst row of max |x - ref| / max |ref| over the rows (all leading axes)"""
    x, ref = x.double().reshape(-1, x.shape[-1]), ref.reshape(-1, ref.shape[-1])
    return float(((x - ref).abs().amax(1) / ref.abs().amax(1)).max())


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(17, 70), (16, 2)])
def test_folded_wave_resident_kernel(models, weights, B, T):
    """frame_mlps_wr_kernel<false, true> through nws_debug_frame_mlps_kernel(2): 17 x 70 frames = five 256-frame blocks that
    straddle utterances, the last one partial; 16 x 2 = one partial wave.  FiLM rows and spectrum rows against the float64
    restatement, worst row error relative to the row maximum.  The bar is the PARENT path's own figure on the same inputs (its
    FiLM rows; its tap rows taken to spectra in float64) times two - the factor covers the changed summation order.
    Measured on MI355X (17 x 70 | 16 x 2): FiLM rows new 2.9e-6 | 1.2e-6 against parent 4.4e-6 | 1.5e-6; spectrum rows new 9.2e-5 |
    5.2e-5 against parent 1.9e-4 | 1.4e-4 (LABBOOK 'Frame MLPs emit filter spectra')."""
    L = _lib().lib()
    eng = models[0]._engine
    g = torch.Generator().manual_seed(31 * B + T)
    gru = torch.tanh(torch.randn(B, T, 128, generator=g))
    film64, _, G64 = frame_path64(weights, gru)
    assert L.nws_debug_frame_mlps_kernel(2) == 0
    try:
        assert L.nws_frame_mlps_spec_serves(eng.weights()[0], B, T) == 1
        film, spec = eng.frame_mlps_spec(gru.cuda())
        _, film_p, _, fir_p = eng.frame_mlps(gru.cuda())
    finally:
        L.nws_debug_frame_mlps_kernel(0)
    assert spec.shape == (B, T, 132) and film.shape == (B, T, 256)
    assert bool((spec[..., NB:] == 0).all())                      # the three floats behind bin 128 are not written
    new = dict(film=row_err(film.cpu(), film64), spec=row_err(spec[..., :NB].cpu(), G64))
    par = dict(film=row_err(film_p.cpu(), film64), spec=row_err(taps_to_spectrum64(fir_p.cpu()), G64))
    print(f"B={B} T={T}: worst row error / row max  film new {new['film']:.3e} parent {par['film']:.3e} | "
          f"spectrum new {new['spec']:.3e} parent {par['spec']:.3e}")
    from gpu_util import record
    record(f"frame_spec_rows_B{B}_T{T}", film_new=new["film"], film_parent=par["film"], spec_new=new["spec"], spec_parent=par["spec"])
    assert new["film"] <= 2.0 * par["film"], (new, par)
    assert new["spec"] <= 2.0 * par["spec"], (new, par)


def noise_case(B, T, S):
    g = torch.Generator().manual_seed(100 * B + T)
    H = 0.02 * torch.rand(B, NB, T, generator=g) ** 3 + 1e-4
    H[0] *= 50.0                                                  # one loud utterance, one (nearly) silent
    H[1] *= 1e-4
    noise = torch.rand(128 * T - 1, generator=g)
    add = torch.randn(B, 128 * T, generator=g)
    spec = torch.full((B, T, 132), float("nan"))                  # what is behind bin 128 is never read
    spec[..., :NB] = (H.double().transpose(1, 2) @ torch.from_numpy(S.T)).float()
    return H, noise, add, spec


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(17, 70), (16, 9)])
def test_spectrum_in_noise_kernel(models, weights, S64, B, T):
    """fir_noise_spectral_kernel<true>: 17 utterances = a partial group of eight with one live half of a wave; T = 70, 9 = runs of
    seven hops that do not divide T; first / last frame silence at both ends.  Against the oracle's STFT / iSTFT formulation and
    against the tap-form kernel on the same H, both at the bar of tests/test_gpu_fir_spectral.py: 2e-6 of the row maximum."""
    from oracle.newt_oracle import OracleNEWT

    eng = models[0]._engine
    H, noise, add, spec = noise_case(B, T, S64)
    ref = OracleNEWT(weights, fast=False).fir_noise(H, noise)[:, 0].numpy()
    out = eng.fir_noise_spec(spec.cuda(), noise.cuda()).cpu().numpy()
    taps = eng.fir_noise(_taps(H).cuda(), noise.cuda()).cpu().numpy()
    rowmax = np.abs(ref).max(axis=1)
    e_orc, e_tap = np.abs(out - ref).max(axis=1), np.abs(out - taps).max(axis=1)
    print(f"B={B} T={T}: worst row error / row max = {(e_orc / rowmax).max():.3e} vs oracle, {(e_tap / rowmax).max():.3e} vs tap form (bar 2e-6)")
    assert np.all(e_orc <= 2e-6 * rowmax + 1e-12), (e_orc / rowmax).max()
    assert np.all(e_tap <= 2e-6 * rowmax + 1e-12), (e_tap / rowmax).max()
    out2 = eng.fir_noise_spec(spec.cuda(), noise.cuda(), add_in=add.cuda()).cpu().numpy()
    assert np.array_equal(out2, add.numpy() + out)                # add_in: one fp32 addition on top of the same bits
    # one NaN frame in one utterance: every other utterance's rows keep their bits
    bad = spec.clone()
    bad[3, T // 2, :NB] = float("nan")
    outb = eng.fir_noise_spec(bad.cuda(), noise.cuda()).cpu().numpy()
    keep = [b for b in range(B) if b != 3]
    assert np.array_equal(outb[keep], out[keep])
    touched = np.nonzero((outb[3] != out[3]).reshape(T, 128).any(axis=1))[0].tolist()
    assert touched and set(touched) <= {T // 2 - 1, T // 2, T // 2 + 1, T // 2 + 2}, touched


def _taps(H):
    Ht = H.transpose(1, 2)
    h = torch.fft.irfft(torch.complex(Ht, torch.zeros_like(Ht))).roll(128, -1) * torch.hann_window(256).view(1, 1, -1)
    return h[..., 128:].contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("B,T", [(17, 70), (64, 260)])
def test_forward_with_spectrum_hand_over_against_the_oracle(models, weights, B, T):
    """model() end to end on the new pair at the parity bar of tests/test_gpu_parity.py (test_shape_sweep_matches_the_oracle:
    <= 1e-4 RMS and <= 2e-5 of the output's RMS), model.exciter_opts left as those tests leave it (automatic).  64 x 260 takes the
    pair by itself; 17 x 70 is too few frames for the wave-resident kernel and is put on it through nws_debug_frame_mlps_kernel(2)."""
    from oracle.newt_oracle import OracleNEWT

    L = _lib().lib()
    fast = models[1]
    g = torch.Generator().manual_seed(1000 * B + T)
    f0 = 80.0 + 1500.0 * torch.rand(B, 1, 1, generator=g) * (0.5 + torch.rand(B, 1, T, generator=g))
    control = torch.randn(B, 2, T, generator=g)
    pu, nz = torch.rand(101, generator=g), torch.rand(128 * T - 1, generator=g)
    rows = sorted({0, B // 2, B - 1})
    L.nws_debug_frame_mlps_kernel(2 if B * T < 16000 else 0)
    try:
        assert L.nws_frame_mlps_spec_serves(fast._engine.weights()[0], B, T) == 1
        with torch.no_grad():
            y = fast(f0.cuda(), control.cuda(), phase_u=pu.cuda(), noise=nz.cuda()).cpu().numpy()
            L.nws_debug_forward_spec(0)
            y_taps = fast(f0.cuda(), control.cuda(), phase_u=pu.cuda(), noise=nz.cuda()).cpu().numpy()
    finally:
        L.nws_debug_forward_spec(1)
        L.nws_debug_frame_mlps_kernel(0)
    ref = OracleNEWT(weights, fast=True, lut_python_loop=False)(f0[rows], control[rows], pu, nz).numpy()
    errs = [rms(y[r] - ref[i]) for i, r in enumerate(rows)]
    errs_taps = [rms(y_taps[r] - ref[i]) for i, r in enumerate(rows)]
    print(f"B={B} T={T}: RMS error vs oracle {max(errs):.3e} (tap hand-over {max(errs_taps):.3e}), out RMS {rms(ref):.3e}, "
          f"spectrum vs tap hand-over RMS {rms(y - y_taps):.3e}")
    assert y.shape == (B, 128 * T)
    assert max(errs) <= 1e-4 and max(errs) <= 2e-5 * max(rms(ref), 1e-3), (errs, rms(ref))


@pytest.mark.gpu
def test_failed_range_guard_keeps_the_tap_hand_over(models):
    """proj and newt.mlp's first layer scaled by 30: every single layer still passes fp16_mlp_safe, their folded product does not
    pass fp16_spec_safe.  The weights then carry no folded tables and the forward is the tap hand-over bit for bit - the same bits
    as with the spectrum pair switched off - while the unscaled model does take the pair (and differs in the last places)."""
    from gpu_util import build_model

    L = _lib().lib()
    B, T = 64, 70
    g = torch.Generator().manual_seed(77)
    f0 = 100.0 + 600.0 * torch.rand(B, 1, T, generator=g)
    control = torch.randn(B, 2, T, generator=g)
    pu, nz = torch.rand(101, generator=g).cuda(), torch.rand(128 * T - 1, generator=g).cuda()
    m = build_model(True)
    with torch.no_grad():
        m.embedding.proj.weight.mul_(30.0)
        m.newt.mlp.net[0].weight.mul_(30.0)
    w = m._engine.weights()[0]
    assert w.mlp_frags and w.mlp_spec == 0

    def both(model):
        try:
            L.nws_debug_frame_mlps_kernel(2)          # 64 x 70 frames: the wave-resident kernel by request
            with torch.no_grad():
                a = model(f0.cuda(), control.cuda(), phase_u=pu, noise=nz)
                L.nws_debug_forward_spec(0)
                b = model(f0.cuda(), control.cuda(), phase_u=pu, noise=nz)
        finally:
            L.nws_debug_forward_spec(1)
            L.nws_debug_frame_mlps_kernel(0)
        return a, b

    a, b = both(m)
    assert torch.equal(a, b) and bool(torch.isfinite(a).all())
    ok = models[1]
    assert ok._engine.weights()[0].mlp_spec == 1
    a, b = both(ok)
    assert not torch.equal(a, b) and rms((a - b).cpu().numpy()) <= 1e-6
