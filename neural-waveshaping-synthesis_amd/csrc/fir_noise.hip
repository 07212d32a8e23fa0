// Time-varying FIR filtered noise (FIRNoiseSynth.forward, models/modules/generators.py:30-35).
//
// The reference multiplies a rectangular-window STFT (n_fft 256, hop 128, center/reflect) of one
// shared U[0,1) noise vector by the per-frame filter spectrum and inverts with istft(center=False):
// per frame that is a 256-point CIRCULAR convolution of the noise frame with the frame's FIR
// (SURVEY.md App. A.6), overlap-added and divided by the overlap count (1 for n < 128, else 2).
//
// Design: one wave produces one 128-sample output hop of one utterance.  Lanes
// 0-31 compute the first half of frame t's circular convolution (4 outputs each), lanes 32-63 the
// second half of frame t-1's; the two contributions meet with one half-swap.  Taps and noise are
// staged in LDS per workgroup (4 consecutive hops share 5 frames).  Each lane keeps a sliding
// 8-tap register window of the taps and of a copy delayed by one sample (so that tap PAIRS are
// even-aligned for both output parities): two ds_read_b128 of taps + one broadcast ds_read_b128 of
// noise feed 8 v_pk_fma_f32 = 16 MACs.  The NEWT branch is added here (cat + sum(1), models/neural_waveshaping.py:85-86).
#include "fir_spectral_wave.h"  // padded_noise and the wave-level transform pieces: shared with fir_noise_grad.hip

namespace {

constexpr int kL = NWS_FIR_LEN;  // 256
constexpr int kHop = NWS_HOP;    // 128
constexpr int kHalf = NWS_FIR_HALF;  // taps per stored row: h[128 .. 255]
constexpr int kHopsPerBlock = 4;

struct NoiseLds {
  float taps[kHopsPerBlock + 1][kL];          // fir of frames t0-1 .. t0+3
  float taps1[kHopsPerBlock + 1][kL];         // the same taps delayed by one: taps1[k] = taps[(k-1) & 255]
  float sig[(kHopsPerBlock + 1) * kHop + kHop];  // padded noise [128(t0-1), 128(t0+3)+256)
};

// slot mode of a streaming window (ROWS): row b's noise reflects about its own bounds rows[b].x (first) and rows[b].y (last
// sample) instead of 0 and len - 1, and its frames start at window frame rows[b].z: earlier frames are silent and the first
// one's left hop is that frame alone (overlap count 1), as at the start of a one-shot signal
__device__ __forceinline__ float row_noise(const float* __restrict__ noise, int lo, int hi, int origin, int i) {
  int s = i - origin;
  if (s < lo) s = 2 * lo - s;
  if (s > hi) s = 2 * hi - s;
  s = s < 0 ? 0 : s;
  return noise[s];
}

template <bool ROWS>
__global__ __launch_bounds__(256) void fir_noise_kernel(const float* __restrict__ fir, const float* __restrict__ noise,
                                                        const float* __restrict__ add_in, int T, int len, int origin,
                                                        float* __restrict__ out, const int4* __restrict__ rows) {
  __shared__ __attribute__((aligned(16))) NoiseLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int half = lane >> 5, q = lane & 31;
  const int b = blockIdx.y;
  const int t0 = blockIdx.x * kHopsPerBlock;
  const int N = T * kHop;
  int4 rb = make_int4(0, 0, 0, 0);
  if constexpr (ROWS) rb = rows[b];
  const int t_lo = ROWS ? rb.z : 0;

  // fir holds the upper half-taps u[d] = h[128 + d]; the row is symmetric about tap 128 and h[0] = 0 (include/nws_hip.h)
  for (int e = tid; e < (kHopsPerBlock + 1) * kL; e += 256) {
    const int fr = e >> 8, k = e & 255;
    const int t = t0 - 1 + fr;
    const int d = k >= kHalf ? k - kHalf : kHalf - k;      // k = 0 -> d = 128: the zero tap
    const float v = (t >= t_lo && t < T && d < kHalf) ? fir[((size_t)b * T + t) * kHalf + d] : 0.0f;
    L.taps[fr][k] = v;
    L.taps1[fr][(k + 1) & 255] = v;
  }
  for (int e = tid; e < (kHopsPerBlock + 1) * kHop + kHop; e += 256) {
    const int i = (t0 - 1) * kHop + e;  // index into the padded noise, valid range [0, N+255)
    float v = 0.0f;
    if (i >= 0 && i < N + kL - 1) v = ROWS ? row_noise(noise, rb.x, rb.y, origin, i) : padded_noise(noise, len, origin, i);
    L.sig[e] = v;
  }
  __syncthreads();

  const int t = t0 + wave;  // output hop
  if (t >= T) return;
  // half 0: frame t, outputs y_t[4q .. 4q+3];  half 1: frame t-1, outputs y_{t-1}[128+4q .. ]
  const int slot = wave + 1 - half;            // frame slot in LDS (frame t0-1+slot)
  const int nb = half * kHop + 4 * q;          // first output index inside the frame
  const float* f = &L.sig[slot * kHop];        // frame samples f[0..255]
  const float* h = L.taps[slot];

  // y[nb+i] = sum_m f[m] h[(nb+i-m) & 255], four outputs per lane, TWO taps per packed FMA:
  //   y_i += {f[m+1], f[m]} * {A[je], A[je+1]}   (m even; lanes: f[m+1] h[n_i-m-1]  and  f[m] h[n_i-m])
  // the pair (A[je], A[je+1]) must be even-aligned: for odd i it is (h[j-1], h[j]) of the natural array, for even i
  // (h[j-1], h[j]) = (h1[j], h1[j+1]) of the copy delayed by one sample.  With base = nb - m0 (multiple of 4) the pairs
  // needed per 4 taps are at base-2, base, base+2 of each array: a sliding window of two quads (hi = [base, base+4),
  // lo = [base-4, base)), one new ds_read_b128 per array per iteration.
  const float* h1 = L.taps1[slot];
  f32x2 a0 = {0.0f, 0.0f}, a1 = {0.0f, 0.0f}, a2 = {0.0f, 0.0f}, a3 = {0.0f, 0.0f};
  float4 hi0 = *reinterpret_cast<const float4*>(&h[nb & 255]);
  float4 hi1 = *reinterpret_cast<const float4*>(&h1[nb & 255]);
#pragma unroll 4
  for (int m0 = 0; m0 < kL; m0 += 4) {
    const float4 lo0 = *reinterpret_cast<const float4*>(&h[(nb - m0 - 4) & 255]);
    const float4 lo1 = *reinterpret_cast<const float4*>(&h1[(nb - m0 - 4) & 255]);
    const float4 fv = *reinterpret_cast<const float4*>(&f[m0]);
    const f32x2 fs0 = {fv.y, fv.x}, fs1 = {fv.w, fv.z};
    // odd outputs (natural taps)
    a1 = fma2(fs0, f32x2{hi0.x, hi0.y}, a1);
    a3 = fma2(fs0, f32x2{hi0.z, hi0.w}, a3);
    a1 = fma2(fs1, f32x2{lo0.z, lo0.w}, a1);
    a3 = fma2(fs1, f32x2{hi0.x, hi0.y}, a3);
    // even outputs (taps delayed by one)
    a0 = fma2(fs0, f32x2{hi1.x, hi1.y}, a0);
    a2 = fma2(fs0, f32x2{hi1.z, hi1.w}, a2);
    a0 = fma2(fs1, f32x2{lo1.z, lo1.w}, a0);
    a2 = fma2(fs1, f32x2{hi1.x, hi1.y}, a2);
    hi0 = lo0;
    hi1 = lo1;
  }
  const float y0 = a0.x + a0.y, y1 = a1.x + a1.y, y2 = a2.x + a2.y, y3 = a3.x + a3.y;
  // overlap-add of the two frames covering this hop, divided by the overlap count
  const float o0 = y0 + nws_swap_halves(y0);
  const float o1 = y1 + nws_swap_halves(y1);
  const float o2 = y2 + nws_swap_halves(y2);
  const float o3 = y3 + nws_swap_halves(y3);
  if (half == 0) {
    const float inv = t == t_lo ? 1.0f : 0.5f;
    const size_t o = (size_t)b * N + (size_t)t * kHop + 4 * q;
    float4 r = make_float4(o0 * inv, o1 * inv, o2 * inv, o3 * inv);
    if (add_in != nullptr) {
      const float4 a = *reinterpret_cast<const float4*>(&add_in[o]);
      r.x = a.x + r.x;
      r.y = a.y + r.y;
      r.z = a.z + r.z;
      r.w = a.w + r.w;
    }
    *reinterpret_cast<float4*>(&out[o]) = r;
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// Batched form (B >= 16): the per-frame circular convolution as the reference does it, a product of spectra, in fp32 on the
// vector pipe.  Per frame: Y_t = X_t H_t, y_t = IDFT(Y_t), then the overlap-add above.
//  * The stored tap row is the upper half u[d] = h[128 + d] of a row mirror-symmetric about tap 128 with h[0] = 0: rolled
//    back by 128 it is real and even, e[n] = u[min(n, 256 - n)] (u[128] := 0), so its DFT G is REAL and H[k] = (-1)^k G[k].
//  * Two frames of ONE utterance share a complex transform in both directions: DFT(e_a + i e_b) = G_a + i G_b needs no split
//    because both spectra are real, and IDFT(X_a H_a + i X_b H_b) = y_a + i y_b.  Frames of different utterances never share a
//    transform: an Inf / NaN in one utterance's taps leaves every other row bit-for-bit alone.  Inside an utterance a bad
//    frame reaches its pair partner too, i.e. one hop further than the two hops the frame itself covers.
//  * One transform = 16 lanes x 16 points (fir_spectral_fft.h).  A wave runs four of them side by side, the four consecutive
//    frame pairs (t0-1, t0) .. (t0+5, t0+6), and does so for TWO utterances at once: every value is a two-float vector
//    (.x = utterance b0, .y = utterance b0 + 1), so the butterflies are v_pk_add / v_pk_mul / v_pk_fma_f32 with no operand
//    swizzle - the two halves of a packed instruction are independent IEEE operations, an utterance's bits do not depend on
//    which half it rides in or on its neighbour.  (Packing re with im instead would need the swizzle the build refuses.)
//  * The wave writes the seven hops t0 .. t0+6.  Hop t = first half of y_t + second half of y_t-1: inside a lane for the odd
//    member of a pair, one 16-lane shift for the even one; the run's first frame only supplies the second half (recomputed by
//    this run, written by nobody: no atomics, no dependence on launch order or on the batch).
//  * The noise spectra are shared by every utterance: wave 0 of the workgroup (4 waves = 8 utterances on the same run)
//    transforms the four noise frame pairs, separates each pair with the k <-> -k mirror through LDS and leaves, per bin,
//    S = (-1)^k X_a / 256 and D = (-1)^k i X_b / 256; the product of a bin is then P = G_a S + G_b D (two FMAs per part).
//    THE FILTER SPECTRUM IS ONE STEP (sp_filter_spectrum): a forward path that hands over spectra instead of taps replaces it.
//  * Frames outside [0, T) are silent by a select on the loaded taps (and on their half of the result: the partner's rounding
//    residue does not leak into a silent frame); rows >= B compute on a clamped row and store nothing.
// Memory: every tap row is read once by its run (the run's first frame a second time by the run before, on the same L2: the
// block order below); lane l of a transform reads u[16 j + l], 64 contiguous bytes per 16 lanes.
constexpr int kSpWaves = 4;          // waves per workgroup, two utterances each
constexpr int kSpUtt = 2 * kSpWaves; // utterances per workgroup
constexpr int kSpPairs = 4;          // frame pairs per wave = transforms running side by side
constexpr int kSpHops = 2 * kSpPairs - 1;

struct SpectralLds {
  float4 sd[kSpPairs][9][16];                  // [pair][k2][k1] = (S.re, S.im, D.re, D.im) of bin k1 + 16 k2 <= 143; the bins
                                               // above 128 are read at their mirror image (sp_product)
  float4 tw[256];                              // (cos, cos, sin, sin)(2 pi l k / 256) at [k][l]
  f32x2 x[kSpWaves][kSpPairs * kSpPlane];      // the 16 x 16 transposes of a wave's four transforms, re then im through the
                                               // same plane (47 KB per workgroup: three of them on a CU)
};

// Spectrum of the filters of a frame pair from their stored half rows: on return (lane k1, register k2) holds
// (G_a, G_b)[k1 + 16 k2] as (re, im).  ua / ub: u[16 j + l] of the two rows, already zero for a silent frame.
__device__ __forceinline__ void sp_filter_spectrum(C16T<f32x2>& z, const f32x2 (&ua)[8], const f32x2 (&ub)[8], const float* tw,
                                                   f32x2* x, int lane, int l) {
  // e[16 j + l] for j >= 8 is u[16 (16 - j) - l]: register 15 - j of lane 16 - l, or for l = 0 the lane's own register 16 - j
  const int src = (lane & 48) | ((16 - l) & 15);
  const f32x2 zero = {0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    z.re[j] = ua[j];
    z.im[j] = ub[j];
  }
#pragma unroll
  for (int j = 8; j < 16; ++j) {
    const f32x2 ma = sp_shfl(ua[15 - j], src), mb = sp_shfl(ub[15 - j], src);
    const f32x2 oa = j == 8 ? zero : ua[(16 - j) & 7], ob = j == 8 ? zero : ub[(16 - j) & 7];   // u[128] := 0 (h[0] = 0)
    z.re[j] = sp_select(l == 0, oa, ma);
    z.im[j] = sp_select(l == 0, ob, mb);
  }
  sp_fft256<false>(z, tw, x, l);
}

// SPEC: `fir` holds rows of NWS_SPEC_ROW floats, the filter spectrum G[0 .. 128] itself (nws_frame_mlps_spec), and the two utterances'
// G_a, G_b are loaded straight into (lane k1, register k2) = G[k1 + 16 k2], where sp_filter_spectrum would have left them; a bin
// above 128 is read at its mirror image 256 - k (G is real and even).  Register j < 8 of a transform's 16 lanes reads the 64
// contiguous bytes G[16 j .. 16 j + 15], register j >= 8 the 64 bytes G[241 - 16 j .. 256 - 16 j]: whole segments either way.  No
// mirror exchange and no filter transform (32 more loads per lane instead); silence, clamping and containment as in the tap form.
template <bool SPEC>
__global__ __launch_bounds__(64 * kSpWaves, 3) void fir_noise_spectral_kernel(const float* __restrict__ fir,
                                                                             const float* __restrict__ noise,
                                                                             const float* __restrict__ add_in, int B, int T, int len,
                                                                             int origin, float* __restrict__ out, int nruns, int total) {
  __shared__ __attribute__((aligned(16))) SpectralLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l = lane & 15;
  // Workgroups are dealt to the eight XCDs round-robin (block i -> XCD i % 8; placement only matters for speed).  The list of
  // (utterance block, run) with the run fastest is cut into eight contiguous chunks, one per XCD, so that the tap row two
  // neighbouring runs both read (frame t0 - 1 of one = frame t0 + 6 of the other) comes from one L2.
  const int per_xcd = gridDim.x >> 3;                           // gridDim.x = 8 ceil(total / 8)
  const int id = (blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);
  if (id >= total) return;
  const int run = id % nruns;
  const int b0 = (id / nruns) * kSpUtt + 2 * wave, b1 = b0 + 1; // .x | .y
  const int t0 = run * kSpHops;
  const int ta = t0 - 1 + 2 * g, tb = ta + 1;                   // this transform's frames (Re | Im)
  const int N = T * kHop;
  const bool oka = ta >= 0 && ta < T, okb = tb < T;
  const int tac = ta < 0 ? 0 : (ta < T ? ta : T - 1), tbc = tb < T ? tb : T - 1;

  // tap rows first: they fly under the twiddle set-up and, in wave 0, under the noise transform.  Always-in-bounds addresses
  // and a select afterwards (never a multiplication: 0 * Inf = NaN would leak a clamped row into a silent frame).
  const int bc0 = b0 < B ? b0 : B - 1, bc1 = b1 < B ? b1 : B - 1;
  constexpr int kRow = SPEC ? NWS_SPEC_ROW : kHalf;
  const float* rowa0 = &fir[((size_t)bc0 * T + tac) * kRow + l];
  const float* rowb0 = &fir[((size_t)bc0 * T + tbc) * kRow + l];
  const float* rowa1 = &fir[((size_t)bc1 * T + tac) * kRow + l];
  const float* rowb1 = &fir[((size_t)bc1 * T + tbc) * kRow + l];
  f32x2 ua[SPEC ? 16 : 8], ub[SPEC ? 16 : 8];   // SPEC: (G_a, G_b)[l + 16 j] of the two utterances
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    ua[j] = f32x2{rowa0[16 * j], rowa1[16 * j]};
    ub[j] = f32x2{rowb0[16 * j], rowb1[16 * j]};
  }
  if constexpr (SPEC) {
    // bin l + 16 j >= 128 at 256 - 16 j - l (row + l - 2 l); j = 8: 128 - l, which is bin 128 itself for l = 0
#pragma unroll
    for (int j = 8; j < 16; ++j) {
      const int m = 256 - 16 * j - 2 * l;
      ua[j] = f32x2{rowa0[m], rowa1[m]};
      ub[j] = f32x2{rowb0[m], rowb1[m]};
    }
  }
  sp_fill_twiddles(L.tw, tid);
  const float* tw = reinterpret_cast<const float*>(&L.tw[l]);
  __syncthreads();

  f32x2* x = &L.x[wave][g * kSpPlane];
  if (wave == 0) {
    // noise frames ta | tb (reflect padding resolved here; a frame position outside the padded signal reads as 0)
    C16 z;
    float* xs = reinterpret_cast<float*>(x);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int i0 = kHop * ta + 16 * j + l, i1 = i0 + kHop;
      const bool in0 = i0 >= 0 && i0 < N + kL - 1, in1 = i1 >= 0 && i1 < N + kL - 1;
      const float v0 = padded_noise(noise, len, origin, in0 ? i0 : origin);
      const float v1 = padded_noise(noise, len, origin, in1 ? i1 : origin);
      z.re[j] = in0 ? v0 : 0.0f;
      z.im[j] = in1 ? v1 : 0.0f;
    }
    sp_fft256<false>(z, tw, xs, l);
    // Z = X_a + i X_b in (lane k1, register k2).  X_a = (Z[k] + conj Z[-k]) / 2, i X_b = (Z[k] - conj Z[-k]) / 2: the
    // mirror through this transform's own LDS plane, in natural order
    float mr[16], mi[16];
    sp_mirror(z.re, mr, xs, l);
    sp_mirror(z.im, mi, xs, l);
    const float c = (l & 1) ? -(1.0f / 512.0f) : (1.0f / 512.0f);   // (-1)^k / 2 / 256, exact
#pragma unroll
    for (int j = 0; j < 9; ++j)      // bins 0 .. 143; S[-k] = conj S[k] and D[-k] = -conj D[k] give the rest
      L.sd[g][j][l] = make_float4(c * (z.re[j] + mr[j]), c * (z.im[j] - mi[j]), c * (z.re[j] - mr[j]), c * (z.im[j] + mi[j]));
  }
  const f32x2 zero = {0.0f, 0.0f};
#pragma unroll
  for (int j = 0; j < (SPEC ? 16 : 8); ++j) {
    ua[j] = sp_select(oka, ua[j], zero);
    ub[j] = sp_select(okb, ub[j], zero);
  }
  C16T<f32x2> z;
  if constexpr (SPEC) {
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      z.re[j] = ua[j];
      z.im[j] = ub[j];
    }
  } else {
    sp_filter_spectrum(z, ua, ub, tw, x, lane, l);
  }
  __syncthreads();                                               // the noise spectra are in place

  // the other branch's samples of the hops this lane stores (cat + sum(1)): requested before the inverse transform
  const bool has_add = add_in != nullptr;
  const bool sta = g > 0 && ta < T, stb = tb < T;
  const size_t oa0 = (size_t)bc0 * N + (size_t)tac * kHop + l, ob0 = (size_t)bc0 * N + (size_t)tbc * kHop + l;
  const size_t oa1 = (size_t)bc1 * N + (size_t)tac * kHop + l, ob1 = (size_t)bc1 * N + (size_t)tbc * kHop + l;
  f32x2 adda[8], addb[8];
  if (has_add) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      adda[j] = f32x2{add_in[oa0 + 16 * j], add_in[oa1 + 16 * j]};
      addb[j] = f32x2{add_in[ob0 + 16 * j], add_in[ob1 + 16 * j]};
    }
  }
  // P = G_a S + G_b D per bin, element by element: S and D are one float each for both utterances, and a packed instruction
  // would have to broadcast the upper register of a loaded pair.  Bin k = l + 16 j > 143 reads its mirror image 256 - k =
  // (lane 16 - l, register 15 - j), for l = 0 (lane 0, register 16 - j): S[k] = conj S[-k], D[k] = -conj D[-k].
  const float4* sdm = &L.sd[g][l == 0 ? 1 : 0][(16 - l) & 15];
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const f32x2 ga = z.re[j], gb = z.im[j];
    if (j < 9) {
      const float4 sd = L.sd[g][j][l];
      z.re[j] = f32x2{fmaf(ga.x, sd.x, gb.x * sd.z), fmaf(ga.y, sd.x, gb.y * sd.z)};
      z.im[j] = f32x2{fmaf(ga.x, sd.y, gb.x * sd.w), fmaf(ga.y, sd.y, gb.y * sd.w)};
    } else {
      const float4 sd = sdm[(15 - j) * 16];
      z.re[j] = f32x2{fmaf(ga.x, sd.x, -(gb.x * sd.z)), fmaf(ga.y, sd.x, -(gb.y * sd.z))};
      z.im[j] = f32x2{fmaf(gb.x, sd.w, -(ga.x * sd.y)), fmaf(gb.y, sd.w, -(ga.y * sd.y))};
    }
  }
  sp_fft256<true>(z, tw, x, l);
  // (lane l, register j) = y_a[l + 16 j] + i y_b[l + 16 j]; overlap-add, divided by the overlap count (1 in the signal's
  // first hop, else 2; a stored hop ta is never the first)
  const float invb = tb == 0 ? 1.0f : 0.5f;
  f32x2 ha[8], hb[8];
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    const f32x2 ya0 = sp_select(oka, z.re[j], zero), ya1 = sp_select(oka, z.re[j + 8], zero);
    const f32x2 yb0 = sp_select(okb, z.im[j], zero), yb1 = sp_select(okb, z.im[j + 8], zero);
    // second half of frame ta - 1: the pair to the left (pair 0 wraps to pair 3; its hop ta belongs to the run before, sta = false)
    const f32x2 prev = sp_shfl(yb1, (lane - 16) & 63);
    ha[j] = (ya0 + prev) * 0.5f;
    hb[j] = (yb0 + ya1) * invb;
    if (has_add) {
      ha[j] = adda[j] + ha[j];
      hb[j] = addb[j] + hb[j];
    }
  }
  if (sta) {
    if (b0 < B) {
#pragma unroll
      for (int j = 0; j < 8; ++j) out[oa0 + 16 * j] = ha[j].x;
    }
    if (b1 < B) {
#pragma unroll
      for (int j = 0; j < 8; ++j) out[oa1 + 16 * j] = ha[j].y;
    }
  }
  if (stb) {
    if (b0 < B) {
#pragma unroll
      for (int j = 0; j < 8; ++j) out[ob0 + 16 * j] = hb[j].x;
    }
    if (b1 < B) {
#pragma unroll
      for (int j = 0; j < 8; ++j) out[ob1 + 16 * j] = hb[j].y;
    }
  }
}

}  // namespace

extern "C" int nws_fir_noise_window(const float* fir, const float* noise, int noise_len, int origin, const float* add_in,
                                    int B, int T, float* out, void* stream) {
  if (!fir || !noise || !out || B <= 0 || T <= 0 || noise_len < 2 || origin < 0) return NWS_ERR_BAD_ARG;
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  if (B >= 16) {  // shared noise spectra, one wave per two utterances and run of seven hops
    const long long nruns = (T + kSpHops - 1) / kSpHops, total = nruns * ((B + kSpUtt - 1) / kSpUtt);
    if (total > (1ll << 30)) return NWS_ERR_UNSUPPORTED;
    const dim3 grid((unsigned)(8 * ((total + 7) / 8)));           // see the XCD note in the kernel
    fir_noise_spectral_kernel<false><<<grid, 64 * kSpWaves, 0, (hipStream_t)stream>>>(fir, noise, add_in, B, T, noise_len, origin, out,
                                                                                    (int)nruns, (int)total);
    NWS_CHECK_LAUNCH();
    return NWS_OK;
  }
  const dim3 grid((T + kHopsPerBlock - 1) / kHopsPerBlock, B);
  fir_noise_kernel<false><<<grid, 256, 0, (hipStream_t)stream>>>(fir, noise, add_in, T, noise_len, origin, out, nullptr);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

// slot mode of a streaming window (stream.hip): per-row reflection bounds and first frames, every B on the per-utterance kernel
// (the B >= 16 spectral kernel shares one set of noise spectra over eight rows; per-row edges would need their own)
extern "C" int nws_fir_noise_window_rows(const float* fir, const float* noise, int origin, const int4* rows, int B, int T,
                                         float* out, void* stream) {
  if (!fir || !noise || !out || !rows || B <= 0 || T <= 0 || origin < 0) return NWS_ERR_BAD_ARG;
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  const dim3 grid((T + kHopsPerBlock - 1) / kHopsPerBlock, B);
  fir_noise_kernel<true><<<grid, 256, 0, (hipStream_t)stream>>>(fir, noise, nullptr, T, 0, origin, out, rows);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

extern "C" int nws_fir_noise(const float* fir, const float* noise, const float* add_in, int B, int T, float* out,
                             void* stream) {
  return nws_fir_noise_window(fir, noise, T * kHop - 1, kL / 2, add_in, B, T, out, stream);
}

// the batched kernel on rows of filter spectra (whole-clip framing: origin 128, N - 1 noise samples)
extern "C" int nws_fir_noise_spec(const float* spec, const float* noise, const float* add_in, int B, int T, float* out, void* stream) {
  if (!spec || !noise || !out || B <= 0 || T <= 0) return NWS_ERR_BAD_ARG;
  if (B < 16 || B > 65535) return NWS_ERR_UNSUPPORTED;
  const long long nruns = (T + kSpHops - 1) / kSpHops, total = nruns * ((B + kSpUtt - 1) / kSpUtt);
  if (total > (1ll << 30)) return NWS_ERR_UNSUPPORTED;
  const dim3 grid((unsigned)(8 * ((total + 7) / 8)));           // see the XCD note in the kernel
  fir_noise_spectral_kernel<true><<<grid, 64 * kSpWaves, 0, (hipStream_t)stream>>>(spec, noise, add_in, B, T, T * kHop - 1, kL / 2, out,
                                                                                 (int)nruns, (int)total);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}
