// Backward of NEWT.forward on a materialised exciter (models/modules/shaping.py:67-79, TrainableNonlinearity :36-37; forward:
// newt_apply_kernel<kModeExact> of exciter_newt.hip), DESIGN.md 3.18.  Packaged sizes: 64 shapers, width 8, depth 4, hop 128,
// one output channel.
//
// Forward per utterance b, shaper s, sample n (film rows s, 64+s, 128+s, 192+s upsampled x128 by nws_lerp_coeff / nws_lerp):
//   x = gi e + bi   a = c x   z1 = w0 a + b0   h1 = sin z1   z2 = W2 h1 + b2   h2 = sin z2   z3 = W4 h2 + b4   h3 = sin z3
//   z4 = w6 . h3 + b6   y = sin z4   v = gn y + bn   out[b][n] = sum_s m_s v + m_b
// Backward for g = dL/d(out): dv = m_s g, then the chain of DESIGN.md 3.18 down to de = gi dx; every parameter gradient is a sum
// over (b, n), dfilm the transpose of the upsampling.
//
// Nothing is saved.  Three kernels, no atomics:
//  * newt_grad_kernel: the shaper is wave-uniform (blockIdx.x), lane = sample.  The (b, 64-sample block) pairs of a shaper's rows
//    form one list of U = 2 B T units; workgroup p of P covers `chunk` consecutive units, each of its 4 waves a quarter of them.
//    Per unit the wave recomputes the forward of its 64 samples with the arithmetic of exact_shaper_precise (weights of the one
//    shaper from LDS at wave-uniform addresses, FiLM as multiply then add, nws_lerp), with nws_sincosf_nocall for the cosines,
//    and walks the chain back.  grad_exciter leaves as one coalesced store.  A 64-sample block aligned to 64 has ONE (i0, i1)
//    frame pair, so its share of dfilm is two wave sums per FiLM row, sum w0 d and sum w1 d: 8 floats per unit into the
//    workspace.  The 172 parameter sums of the shaper (170 of shaping_fn, dm_s, and dm_b = sum g, which every shaper computes
//    and shaper 0 writes) are per-lane accumulators over the wave's units, reduced across the wave once, across the 4 waves
//    through LDS in wave order, and written as partial row p.
//  * newt_grad_fold_kernel: dfilm[b][c][t] = the at most six block sums that name frame t, added in float64 in block order.
//  * nws_segment_sum_kernel (grad_sums.h): out[e] = sum_p part[p][e] in float64 in a fixed order, rounded once.
// Every output element is written by one thread and every sum runs in an order that depends on (B, T) only: equal inputs give
// equal bits.  g = 0 gives zeros: every output is a sum of products with the factor dv = m_s g (or g itself).
#include "grad_sums.h"

namespace {

constexpr int kS = NWS_N_SHAPERS;
constexpr int kBlk = 64;           // samples per unit: one wave, one (i0, i1) pair
constexpr int kWaves = 4;
constexpr int kMinChunk = 32;      // units per workgroup while that gives at most kMaxP workgroups per shaper
constexpr int kMaxP = 256;
constexpr int kNAcc = 172;

// one partial row of the parameter sums, in the order and layout of the eleven gradient tensors
constexpr int kOffC = 0;               // input_scale (1, 64, 1)
constexpr int kOffW0 = 64;             // net.0.weight (512, 1, 1)
constexpr int kOffB0 = kOffW0 + 512;
constexpr int kOffW2 = kOffB0 + 512;   // net.2.weight (512, 8, 1): [(s 8 + o) 8 + i]
constexpr int kOffB2 = kOffW2 + 4096;
constexpr int kOffW4 = kOffB2 + 512;
constexpr int kOffB4 = kOffW4 + 4096;
constexpr int kOffW6 = kOffB4 + 512;   // net.6.weight (64, 8, 1)
constexpr int kOffB6 = kOffW6 + 512;
constexpr int kOffM = kOffB6 + 64;     // mixer.0.weight (1, 64, 1)
constexpr int kOffMB = kOffM + 64;     // mixer.0.bias (1)
constexpr int kParStride = kOffMB + 4;
static_assert(kOffMB == 10944, "64 x 170 shaper parameters + 64 mixer weights");

// the weights of ONE shaper, laid out like its slice of exciter_newt.hip's ShaperLds (w2t / w4t: [in][out])
struct Shaper1 {
  float w0[8], b0[8];
  float w2t[64], b2[8];
  float w4t[64], b4[8];
  float w6[8];
  float b6, c, m, pad;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// local index of an accumulator (red[] below) -> its place in a partial row
__device__ __forceinline__ int par_offset(int k, int s) {
  if (k < 1) return kOffC + s;
  if (k < 9) return kOffW0 + s * 8 + (k - 1);
  if (k < 17) return kOffB0 + s * 8 + (k - 9);
  if (k < 81) return kOffW2 + s * 64 + (k - 17);
  if (k < 89) return kOffB2 + s * 8 + (k - 81);
  if (k < 153) return kOffW4 + s * 64 + (k - 89);
  if (k < 161) return kOffB4 + s * 8 + (k - 153);
  if (k < 169) return kOffW6 + s * 8 + (k - 161);
  if (k < 170) return kOffB6 + s;
  if (k < 171) return kOffM + s;
  return kOffMB;
}

template <bool PARAMS>
__global__ __launch_bounds__(256) void newt_grad_kernel(NwsWeights w, const float* __restrict__ exciter,
                                                        const float* __restrict__ film, const float* __restrict__ g, int T,
                                                        int U, int chunk, float* __restrict__ grad_exciter,
                                                        float* __restrict__ part_film, float* __restrict__ part_par) {
  __shared__ Shaper1 W;
  __shared__ float red[kWaves][kNAcc];
  const int s = blockIdx.x, p = blockIdx.y;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  if (tid < 8) {
    W.w0[tid] = w.shaper_w0[s * 8 + tid];
    W.b0[tid] = w.shaper_b0[s * 8 + tid];
    W.b2[tid] = w.shaper_b2[s * 8 + tid];
    W.b4[tid] = w.shaper_b4[s * 8 + tid];
    W.w6[tid] = w.shaper_w6[s * 8 + tid];
  }
  if (tid < 64) {   // tid = o 8 + in  ->  [in][o]
    const int o = tid >> 3, in = tid & 7;
    W.w2t[in * 8 + o] = w.shaper_w2[s * 64 + tid];
    W.w4t[in * 8 + o] = w.shaper_w4[s * 64 + tid];
  }
  if (tid == 0) {
    W.b6 = w.shaper_b6[s];
    W.c = w.shaper_in_scale[s];
    W.m = w.newt_out_w[s];
    W.pad = 0.0f;
  }
  __syncthreads();

  const int N = T * NWS_HOP, nblk = 2 * T;
  const int q = chunk / kWaves;                                   // chunk is a multiple of kWaves
  const long long base = (long long)p * chunk + (long long)wave * q;
  const int u0 = (int)(base < U ? base : U);
  const int u1 = (int)(base + q < U ? base + q : U);

  float a_c = 0.0f, a_b6 = 0.0f, a_m = 0.0f, a_mb = 0.0f;
  float a_w0[8], a_b0[8], a_b2[8], a_b4[8], a_w6[8], a_W2[64], a_W4[64];
#pragma unroll
  for (int i = 0; i < 8; ++i) a_w0[i] = a_b0[i] = a_b2[i] = a_b4[i] = a_w6[i] = 0.0f;
#pragma unroll
  for (int i = 0; i < 64; ++i) a_W2[i] = a_W4[i] = 0.0f;

  for (int u = u0; u < u1; ++u) {
    const int b = u / nblk, j = u - b * nblk;
    const int n = j * kBlk + lane;
    const NwsLerp lc = nws_lerp_coeff(n, T);
    const float* fb = film + (size_t)b * NWS_FILM_CH * T;
    const float g_i = nws_lerp(fb[(size_t)s * T + lc.i0], fb[(size_t)s * T + lc.i1], lc.w0, lc.w1);
    const float b_i = nws_lerp(fb[(size_t)(kS + s) * T + lc.i0], fb[(size_t)(kS + s) * T + lc.i1], lc.w0, lc.w1);
    const float g_n = nws_lerp(fb[(size_t)(2 * kS + s) * T + lc.i0], fb[(size_t)(2 * kS + s) * T + lc.i1], lc.w0, lc.w1);
    const float b_n = nws_lerp(fb[(size_t)(3 * kS + s) * T + lc.i0], fb[(size_t)(3 * kS + s) * T + lc.i1], lc.w0, lc.w1);
    const size_t eoff = ((size_t)b * kS + s) * N + n;
    const float e = exciter[eoff];
    const float gv = g[(size_t)b * N + n];

    // ---- forward, the arithmetic of newt_apply_kernel<kModeExact> / exact_shaper_precise ----
    const float x = g_i * e + b_i;
    const float a = W.c * x;
    float h1[8], c1[8], h2[8], c2[8], h3[8], c3[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) nws_sincosf_nocall(fmaf(W.w0[i], a, W.b0[i]), h1[i], c1[i]);
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float acc = W.b2[o];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = fmaf(W.w2t[i * 8 + o], h1[i], acc);
      nws_sincosf_nocall(acc, h2[o], c2[o]);
    }
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      float acc = W.b4[o];
#pragma unroll
      for (int i = 0; i < 8; ++i) acc = fmaf(W.w4t[i * 8 + o], h2[i], acc);
      nws_sincosf_nocall(acc, h3[o], c3[o]);
    }
    float z4 = W.b6;
#pragma unroll
    for (int i = 0; i < 8; ++i) z4 = fmaf(W.w6[i], h3[i], z4);
    float y, c4;
    nws_sincosf_nocall(z4, y, c4);

    // ---- backward ----
    const float dv = W.m * gv;
    if (PARAMS) {
      a_m = fmaf(gv, g_n * y + b_n, a_m);
      a_mb += gv;
    }
    const float dgn = dv * y;
    const float dz4 = (g_n * dv) * c4;
    if (PARAMS) a_b6 += dz4;
    float dz[8], dh[8];
#pragma unroll
    for (int o = 0; o < 8; ++o) {
      if (PARAMS) a_w6[o] = fmaf(dz4, h3[o], a_w6[o]);
      dz[o] = (W.w6[o] * dz4) * c3[o];                         // dz3
      if (PARAMS) a_b4[o] += dz[o];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float acc = 0.0f;
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        if (PARAMS) a_W4[o * 8 + i] = fmaf(dz[o], h2[i], a_W4[o * 8 + i]);
        acc = fmaf(W.w4t[i * 8 + o], dz[o], acc);
      }
      dh[i] = acc * c2[i];                                     // dz2
    }
#pragma unroll
    for (int o = 0; o < 8; ++o)
      if (PARAMS) a_b2[o] += dh[o];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      float acc = 0.0f;
#pragma unroll
      for (int o = 0; o < 8; ++o) {
        if (PARAMS) a_W2[o * 8 + i] = fmaf(dh[o], h1[i], a_W2[o * 8 + i]);
        acc = fmaf(W.w2t[i * 8 + o], dh[o], acc);
      }
      dz[i] = acc * c1[i];                                     // dz1
    }
    float da = 0.0f;
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (PARAMS) {
        a_w0[i] = fmaf(dz[i], a, a_w0[i]);
        a_b0[i] += dz[i];
      }
      da = fmaf(W.w0[i], dz[i], da);
    }
    if (PARAMS) a_c = fmaf(da, x, a_c);
    const float dx = W.c * da;
    const float dgi = dx * e;
    if (grad_exciter != nullptr) grad_exciter[eoff] = g_i * dx;

    // ---- this block's share of dfilm: rows s, 64+s, 128+s, 192+s get d = dgi, dx, dgn, dv ----
    const float d4[4] = {dgi, dx, dgn, dv};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s0 = wave_sum(lc.w0 * d4[r]);
      const float s1 = wave_sum(lc.w1 * d4[r]);
      if (lane == 0) {
        float* pf = part_film + (((size_t)b * NWS_FILM_CH + r * kS + s) * nblk + j) * 2;
        pf[0] = s0;
        pf[1] = s1;
      }
    }
  }

  if (PARAMS) {
    auto flush = [&](float v, int k) {
      const float t = wave_sum(v);
      if (lane == 0) red[wave][k] = t;
    };
    flush(a_c, 0);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      flush(a_w0[i], 1 + i);
      flush(a_b0[i], 9 + i);
      flush(a_b2[i], 81 + i);
      flush(a_b4[i], 153 + i);
      flush(a_w6[i], 161 + i);
    }
#pragma unroll
    for (int i = 0; i < 64; ++i) {
      flush(a_W2[i], 17 + i);
      flush(a_W4[i], 89 + i);
    }
    flush(a_b6, 169);
    flush(a_m, 170);
    flush(a_mb, 171);
    __syncthreads();
    if (tid < kNAcc && (tid < kNAcc - 1 || s == 0)) {
      double tot = 0.0;
#pragma unroll
      for (int v = 0; v < kWaves; ++v) tot += (double)red[v][tid];
      part_par[(size_t)p * kParStride + par_offset(tid, s)] = (float)tot;
    }
  }
}

// dfilm[b][c][t]: the transpose of the x128 linear upsampling.  Block j of a row (samples 64 j .. 64 j + 63) names frames
// (i0, i1) = nws_lerp_coeff(64 j, T); frame t is named by blocks 2t-1 .. 2t+2 and, at the clamped ends, by block 0 / 2T-1.
__global__ __launch_bounds__(256) void newt_grad_fold_kernel(const float* __restrict__ part_film, int T, long long total,
                                                             float* __restrict__ grad_film) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const int t = (int)(idx % T);
  const int nblk = 2 * T;
  const float* row = part_film + (size_t)(idx / T) * nblk * 2;
  double acc = 0.0;
  auto take = [&](int j) {
    const NwsLerp L = nws_lerp_coeff(j * kBlk, T);
    if (L.i0 == t) acc += (double)row[2 * j];
    if (L.i1 == t) acc += (double)row[2 * j + 1];
  };
  const int lo = 2 * t - 1 > 0 ? 2 * t - 1 : 0, hi = 2 * t + 2 < nblk - 1 ? 2 * t + 2 : nblk - 1;
  if (lo > 0) take(0);
  for (int j = lo; j <= hi; ++j) take(j);
  if (hi < nblk - 1) take(nblk - 1);
  grad_film[idx] = (float)acc;
}

struct Plan {
  int U, chunk, P;
  size_t off_par, bytes;      // part_film at 0; offsets in floats
  bool ok;
};

Plan make_plan(int B, int T, bool want) {
  Plan pl{};
  // lerp coefficients are exact for n < 2^23; the unit list and the fold kernel's grid stay inside int
  pl.ok = B >= 1 && T >= 1 && T <= 65535 && (long long)B * T <= (1ll << 28);
  if (!pl.ok) return pl;
  pl.U = 2 * B * T;
  int chunk = (pl.U + kMaxP - 1) / kMaxP;
  chunk = (chunk + kWaves - 1) / kWaves * kWaves;
  pl.chunk = chunk < kMinChunk ? kMinChunk : chunk;
  pl.P = (pl.U + pl.chunk - 1) / pl.chunk;
  pl.off_par = (size_t)B * NWS_FILM_CH * 2 * T * 2;
  pl.bytes = (pl.off_par + (want ? (size_t)pl.P * kParStride : 0)) * sizeof(float);
  return pl;
}

}  // namespace

extern "C" size_t nws_newt_grad_workspace_bytes(int B, int T, int want_params) {
  const Plan pl = make_plan(B, T, want_params != 0);
  return pl.ok ? pl.bytes : 0;
}

extern "C" int nws_newt_grad(const NwsWeights* w, const float* exciter, const float* film, const float* grad_out, int B, int T,
                             float* grad_exciter, float* grad_film, float* grad_in_scale, float* grad_w0, float* grad_b0,
                             float* grad_w2, float* grad_b2, float* grad_w4, float* grad_b4, float* grad_w6, float* grad_b6,
                             float* grad_mix_w, float* grad_mix_b, void* workspace, size_t workspace_bytes, void* stream) {
  if (!w || !exciter || !film || !grad_out || !grad_film || B < 1 || T < 1) return NWS_ERR_BAD_ARG;
  float* gp[11] = {grad_in_scale, grad_w0, grad_b0, grad_w2, grad_b2, grad_w4, grad_b4, grad_w6, grad_b6, grad_mix_w, grad_mix_b};
  int given = 0;
  for (int i = 0; i < 11; ++i) given += gp[i] != nullptr;
  if (given != 0 && given != 11) return NWS_ERR_BAD_ARG;
  const bool want = given == 11;
  if (w->lut != nullptr) return NWS_ERR_UNSUPPORTED;      // the lookup table has no backward
  if (!w->shaper_in_scale || !w->shaper_w0 || !w->shaper_b0 || !w->shaper_w2 || !w->shaper_b2 || !w->shaper_w4 || !w->shaper_b4 ||
      !w->shaper_w6 || !w->shaper_b6 || !w->newt_out_w || !w->newt_out_b)
    return NWS_ERR_BAD_ARG;
  const Plan pl = make_plan(B, T, want);
  if (!pl.ok) return NWS_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < pl.bytes) return NWS_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const dim3 grid(kS, pl.P);
  if (want)
    newt_grad_kernel<true><<<grid, 256, 0, st>>>(*w, exciter, film, grad_out, T, pl.U, pl.chunk, grad_exciter, ws, ws + pl.off_par);
  else
    newt_grad_kernel<false><<<grid, 256, 0, st>>>(*w, exciter, film, grad_out, T, pl.U, pl.chunk, grad_exciter, ws, nullptr);
  NWS_CHECK_LAUNCH();
  const long long total = (long long)B * NWS_FILM_CH * T;
  newt_grad_fold_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(ws, T, total, grad_film);
  NWS_CHECK_LAUNCH();
  if (!want) return NWS_OK;
  SumSeg segs[11];
  const int offs[11] = {kOffC, kOffW0, kOffB0, kOffW2, kOffB2, kOffW4, kOffB4, kOffW6, kOffB6, kOffM, kOffMB};
  const int ns[11] = {64, 512, 512, 4096, 512, 4096, 512, 512, 64, 64, 1};
  for (int i = 0; i < 11; ++i) segs[i] = SumSeg{gp[i], offs[i], ns[i]};
  nws_segment_sums(ws + pl.off_par, pl.P, kParStride, segs, 11, st);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}
