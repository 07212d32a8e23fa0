// Backward of the noise branch (FIRNoiseSynth, models/modules/generators.py:21-35) with respect to the filter, DESIGN.md 3.15.
//
// For a fixed excitation draw the forward  H -> fir_from_h -> fir_noise  is linear in H, so the backward is the transpose of the
// two ops, link by link, with nothing saved but the excitation:
//
//   g^[j]    = g[j] / c[j]  (j < N; c = 1 in the first hop, else 2),  0 for N <= j < N + 128 (the cropped half of frame T - 1)
//   dh_t[m]  = sum_{n<256} g^[128 t + n] x_t[(n - m) mod 256]          x_t[n] = noise[refl(128 (t - 1) + n)]
//   du_t[d]  = dh_t[128 + d] + dh_t[128 - d]  (d = 1 .. 127),  du_t[0] = dh_t[128]        (B, T, 128): nws_fir_noise_grad
//   dH[k, t] = sum_{d<128} D[128 + d][k] du_t[d]                                          (B, 129, T): nws_fir_from_h_grad
//
// fir_noise_grad_kernel: dh_t = IDFT(conj(X_t) G_t) with the 16 lanes x 16 points transform of fir_spectral_fft.h, laid out like
// the forward's batched kernel (fir_noise.hip): a wave runs four transforms side by side, the frame pairs (t0, t0+1) ..
// (t0+6, t0+7) of one tile of EIGHT frames, for two utterances at once (.x = utterance b0, .y = b0 + 1: packed instructions with
// no operand swizzle, the two halves independent IEEE operations).  Four waves = eight utterances share the tile's noise spectra,
// which wave 0 computes once per workgroup.
//  * Two gradient frames of one utterance share a complex transform: Z = DFT(g^_a + i g^_b).  Unlike the forward's real-even
//    filter rows their spectra are complex, so the pair is separated with the k <-> -k mirror M[k] = conj Z[-k]:
//    G_a = (Z + M) / 2, i G_b = (Z - M) / 2.  Both dh are real, so ONE inverse transform returns them as Re and Im:
//      P = conj(X_a) G_a + i conj(X_b) G_b = Z S + M D,   S = (conj X_a + conj X_b) / 2,  D = (conj X_a - conj X_b) / 2
//    (S and D carry the 1 / 256 of the inverse transform and are stored for all 256 bins: 16 KB).
//  * The loads resolve the reflect fold of the noise (padded_noise), the 1 / c[j] scale (a multiplication by 1 or 0.5: exact)
//    and the cropped half of the last frame (a select: 0).  Frames >= T and rows >= B load clamped addresses and store nothing.
//  * Every frame's du row is written by exactly one wave, nothing is accumulated across waves, no atomics: equal inputs give
//    equal bits whatever the launch order.  g = 0 gives exactly 0 (Z = 0, products and sums of zeros).
// fir_from_h_grad_kernel: the transposed design-matrix product in plain fp32, sequential over d (a fixed order).
// sum_batch_time_kernel: (B, C, T) -> (C) in fp64 in a fixed order: carries a gradient onto a per-channel offset.
#include "fir_spectral_wave.h"  // padded_noise and the wave-level transform pieces: shared with fir_noise.hip

namespace {

constexpr int kHop = NWS_HOP;        // 128
constexpr int kHalf = NWS_FIR_HALF;  // values per stored row: the gradient of u[d] = h[128 + d]
constexpr int kGWaves = 4;           // waves per workgroup, two utterances each
constexpr int kGUtt = 2 * kGWaves;   // utterances per workgroup
constexpr int kGPairs = 4;           // frame pairs per wave = transforms running side by side
constexpr int kGTile = 2 * kGPairs;  // frames per workgroup (the frame tile)

struct GradLds {
  float4 sd[kGPairs][16][16];                  // [pair][k2][k1] = (S.re, S.im, D.re, D.im) of bin k1 + 16 k2
  float4 tw[256];                              // (cos, cos, sin, sin)(2 pi l k / 256) at [k][l]
  f32x2 x[kGWaves][kGPairs * kSpPlane];        // per transform: the 16 x 16 transpose plane, also the 256-entry mirror plane
};

__global__ __launch_bounds__(64 * kGWaves) void fir_noise_grad_kernel(const float* __restrict__ noise,
                                                                      const float* __restrict__ grad_out, int B, int T,
                                                                      float* __restrict__ grad_fir, int ntiles) {
  __shared__ __attribute__((aligned(16))) GradLds L;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int g = lane >> 4, l = lane & 15;
  const int tile = blockIdx.x % ntiles;                            // the tile fastest: neighbours read neighbouring noise
  const int b0 = (blockIdx.x / ntiles) * kGUtt + 2 * wave, b1 = b0 + 1;   // .x | .y
  const int ta = tile * kGTile + 2 * g, tb = ta + 1;               // this transform's frames (Re | Im)
  const int N = T * kHop;
  const bool oka = ta < T, okb = tb < T;
  const bool live = b0 < B;                                        // wave-uniform: a wave without utterances only meets the barriers
  const int tac = oka ? ta : T - 1, tbc = okb ? tb : T - 1;
  const int bc0 = b0 < B ? b0 : B - 1, bc1 = b1 < B ? b1 : B - 1;

  // g^ frames first (they fly under the twiddle set-up and, in wave 0, under the noise transform): always-in-bounds addresses, a
  // select for the cropped half and the frames past the end, and the exact scale 1 / c[j]
  C16T<f32x2> z;
  if (live) {
    const float* ga0 = &grad_out[(size_t)bc0 * N], *ga1 = &grad_out[(size_t)bc1 * N];
    const f32x2 zero = {0.0f, 0.0f};
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int ja = kHop * tac + 16 * j + l, jb = kHop * tbc + 16 * j + l;       // sample index of frame entry n = 16 j + l
      const bool ina = oka && ja < N, inb = okb && jb < N;
      const int jac = ja < N ? ja : N - 1, jbc = jb < N ? jb : N - 1;
      const float sa = ja < kHop ? 1.0f : 0.5f, sb = jb < kHop ? 1.0f : 0.5f;
      z.re[j] = sp_select(ina, f32x2{ga0[jac], ga1[jac]} * sa, zero);
      z.im[j] = sp_select(inb, f32x2{ga0[jbc], ga1[jbc]} * sb, zero);
    }
  }
  sp_fill_twiddles(L.tw, tid);
  const float* tw = reinterpret_cast<const float*>(&L.tw[l]);
  __syncthreads();

  f32x2* x = &L.x[wave][g * kSpPlane];
  if (wave == 0) {
    // noise frames ta | tb of the tile, shared by every utterance; a frame >= T reads clamped positions and is never used
    C16 n;
    float* xs = reinterpret_cast<float*>(x);
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      n.re[j] = padded_noise(noise, N - 1, kHop, kHop * tac + 16 * j + l);   // the whole-clip form: origin = 128
      n.im[j] = padded_noise(noise, N - 1, kHop, kHop * tbc + 16 * j + l);
    }
    sp_fft256<false>(n, tw, xs, l);
    // Zn = X_a + i X_b:  X_a = (Zn[k] + conj Zn[-k]) / 2,  X_b = (Zn[k] - conj Zn[-k]) / (2 i)
    float mr[16], mi[16];
    sp_mirror(n.re, mr, xs, l);
    sp_mirror(n.im, mi, xs, l);
    const float c = 1.0f / 1024.0f;                                // 1/2 (separation) x 1/2 (S, D) x 1/256 (inverse transform)
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const float xar = n.re[j] + mr[j], xai = n.im[j] - mi[j];   // 2 X_a
      const float xbr = n.im[j] + mi[j], xbi = mr[j] - n.re[j];   // 2 X_b
      L.sd[g][j][l] = make_float4(c * (xar + xbr), -(c * (xai + xbi)), c * (xar - xbr), -(c * (xai - xbi)));
    }
  }
  f32x2 mr[16], mi[16];
  if (live) {
    sp_fft256<false>(z, tw, x, l);
    sp_mirror(z.re, mr, x, l);
    sp_mirror(z.im, mi, x, l);
  }
  __syncthreads();                                                 // the noise spectra are in place
  if (!live) return;

  // P = Z S + M D per bin with M = conj Z[-k] = (mr, -mi); S and D are one float each for both utterances, so the products are
  // written element by element (a packed form would broadcast the upper register of a loaded pair: the refused swizzle)
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const float4 sd = L.sd[g][j][l];
    const f32x2 zr = z.re[j], zi = z.im[j], ar = mr[j], ai = mi[j];
    z.re[j] = f32x2{fmaf(zr.x, sd.x, -(zi.x * sd.y)) + fmaf(ar.x, sd.z, ai.x * sd.w),
                    fmaf(zr.y, sd.x, -(zi.y * sd.y)) + fmaf(ar.y, sd.z, ai.y * sd.w)};
    z.im[j] = f32x2{fmaf(zr.x, sd.y, zi.x * sd.x) + fmaf(ar.x, sd.w, -(ai.x * sd.z)),
                    fmaf(zr.y, sd.y, zi.y * sd.x) + fmaf(ar.y, sd.w, -(ai.y * sd.z))};
  }
  sp_fft256<true>(z, tw, x, l);
  // (lane l, register j) = dh_a[l + 16 j] + i dh_b[l + 16 j].  The fold onto the stored half row: d = l + 16 jj takes
  // dh[128 + d] = register 8 + jj of this lane and dh[128 - d] = register 7 - jj of lane 16 - l, for l = 0 register 8 - jj of the
  // lane itself (jj = 0: d = 0 has no partner)
  const int src = (lane & 48) | ((16 - l) & 15);
  const f32x2 zero = {0.0f, 0.0f};
  f32x2 da[8], db[8];
#pragma unroll
  for (int jj = 0; jj < 8; ++jj) {
    const f32x2 ma = sp_shfl(z.re[7 - jj], src), mb = sp_shfl(z.im[7 - jj], src);
    const f32x2 oa = jj == 0 ? zero : z.re[8 - jj], ob = jj == 0 ? zero : z.im[8 - jj];
    da[jj] = z.re[8 + jj] + sp_select(l == 0, oa, ma);
    db[jj] = z.im[8 + jj] + sp_select(l == 0, ob, mb);
  }
  float* ra0 = &grad_fir[((size_t)bc0 * T + tac) * kHalf + l], *rb0 = &grad_fir[((size_t)bc0 * T + tbc) * kHalf + l];
  float* ra1 = &grad_fir[((size_t)bc1 * T + tac) * kHalf + l], *rb1 = &grad_fir[((size_t)bc1 * T + tbc) * kHalf + l];
  if (oka) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) ra0[16 * jj] = da[jj].x;
    if (b1 < B) {
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) ra1[16 * jj] = da[jj].y;
    }
  }
  if (okb) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) rb0[16 * jj] = db[jj].x;
    if (b1 < B) {
#pragma unroll
      for (int jj = 0; jj < 8; ++jj) rb1[16 * jj] = db[jj].y;
    }
  }
}

// dH[b][k][t] = sum_{d<128} D[128 + d][k] du[b][t][d]: the transpose of fir_from_h_kernel (stages.hip).  One workgroup = 64
// frames of one utterance, staged transposed in LDS; wave w of twelve owns the 11 columns 11 w .. 11 w + 10 of D (132 = 12 x 11:
// the three padding columns are computed and not stored), every lane one frame.  The D values are wave-uniform (scalar loads),
// the sum runs over d in order.
constexpr int kHT = 64;              // frames per workgroup
constexpr int kHCols = 11;           // design-matrix columns per wave
constexpr int kHWaves = 132 / kHCols;

__global__ __launch_bounds__(64 * kHWaves) void fir_from_h_grad_kernel(const float* __restrict__ du, const float* __restrict__ D,
                                                                       int T, float* __restrict__ dH) {
  __shared__ float ds[kHalf][kHT + 1];
  const int b = blockIdx.y, t0 = blockIdx.x * kHT;
  for (int e = threadIdx.x; e < kHT * kHalf; e += 64 * kHWaves) {
    const int f = e >> 7, d = e & (kHalf - 1);
    ds[d][f] = t0 + f < T ? du[((size_t)b * T + t0 + f) * kHalf + d] : 0.0f;
  }
  __syncthreads();
  const int f = threadIdx.x & 63;
  const int k0 = kHCols * __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  float acc[kHCols];
#pragma unroll
  for (int i = 0; i < kHCols; ++i) acc[i] = 0.0f;
#pragma unroll 4
  for (int d = 0; d < kHalf; ++d) {
    const float v = ds[d][f];
    const float* row = &D[(kHalf + d) * 132 + k0];
#pragma unroll
    for (int i = 0; i < kHCols; ++i) acc[i] = fmaf(row[i], v, acc[i]);
  }
  if (t0 + f < T) {
#pragma unroll
    for (int i = 0; i < kHCols; ++i)
      if (k0 + i < NWS_N_BANDS) dH[((size_t)b * NWS_N_BANDS + k0 + i) * T + t0 + f] = acc[i];
  }
}

// out[c] = sum_{b, t} x[b][c][t] in fp64, in a fixed order: thread i of the channel's workgroup adds the elements t = i, i + 256,
// ... of utterance 0, then of utterance 1, ... one after the other, then the 256 partial sums meet in a fixed tree.
__global__ __launch_bounds__(256) void sum_batch_time_kernel(const float* __restrict__ x, int B, int C, int T,
                                                             float* __restrict__ out) {
  __shared__ double part[256];
  const int c = blockIdx.x;
  double s = 0.0;
  for (int b = 0; b < B; ++b) {
    const float* row = &x[((size_t)b * C + c) * T];
    for (int t = threadIdx.x; t < T; t += 256) s += (double)row[t];
  }
  part[threadIdx.x] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
    __syncthreads();
  }
  if (threadIdx.x == 0) out[c] = (float)part[0];
}

}  // namespace

extern "C" int nws_fir_noise_grad(const float* noise, const float* grad_out, int B, int T, float* grad_fir, void* stream) {
  if (!noise || !grad_out || !grad_fir || B < 1 || T < 2) return NWS_ERR_BAD_ARG;
  if (T > (1 << 23)) return NWS_ERR_UNSUPPORTED;                    // sample indices stay below 2^30
  const long long ntiles = (T + kGTile - 1) / kGTile, total = ntiles * ((B + kGUtt - 1) / kGUtt);
  if (total > (1ll << 30)) return NWS_ERR_UNSUPPORTED;
  fir_noise_grad_kernel<<<dim3((unsigned)total), 64 * kGWaves, 0, (hipStream_t)stream>>>(noise, grad_out, B, T, grad_fir, (int)ntiles);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

extern "C" int nws_fir_from_h_grad(const float* grad_fir, const float* fir_design, int B, int T, float* grad_H, void* stream) {
  if (!grad_fir || !fir_design || !grad_H || B < 1 || T < 2) return NWS_ERR_BAD_ARG;
  if (B > 65535 || T > (1 << 23)) return NWS_ERR_UNSUPPORTED;
  fir_from_h_grad_kernel<<<dim3((T + kHT - 1) / kHT, B), 64 * kHWaves, 0, (hipStream_t)stream>>>(grad_fir, fir_design, T, grad_H);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

extern "C" int nws_sum_batch_time(const float* x, int B, int C, int T, float* out, void* stream) {
  if (!x || !out || B < 1 || C < 1 || T < 1) return NWS_ERR_BAD_ARG;
  sum_batch_time_kernel<<<dim3(C), 256, 0, (hipStream_t)stream>>>(x, B, C, T, out);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}
