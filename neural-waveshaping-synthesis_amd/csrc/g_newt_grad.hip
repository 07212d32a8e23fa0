// Backward of NEWT.forward on a materialised exciter at any bank size (models/modules/shaping.py:67-79, TrainableNonlinearity
// :36-37; forward: g_film_shaper_kernel + g_conv1x1_kernel of generic.hip), DESIGN.md 3.20.  S <= 64 shapers of width W <= 16 and
// depth D <= 4 (D grouped convolutions), hop 128, one output channel.
//
// Forward per utterance b, shaper s, sample n (film rows s, S+s, 2S+s, 3S+s upsampled x128 by nws_lerp_coeff / nws_lerp):
//   x = gi e + bi   a = c x
//   D = 1: y = sin(w0 a + b0)
//   D >= 2: h_1 = sin(w0 a + b0) (W)   h_{l+1} = sin(W_l h_l + b_l), l = 1 .. D-2   y = sin(w_{D-1} . h_{D-1} + b_{D-1})
//   v = gn y + bn   out[b][n] = sum_s m_s v + m_b
// Backward for g = dL/d(out): dv = m_s g, then the chain of DESIGN.md 3.18 with the hidden-layer step D - 2 times.  The gradient is
// that of this expression with nws_sincosf_nocall's sines (the runtime-size forward's v_sin_f32 is about 4e-7 rad away).
//
// Nothing is saved.  The frame of newt_grad.hip: the shaper is wave-uniform (blockIdx.x), lane = sample, units of 64 samples with
// one (i0, i1) pair, the (B, T)-only partition of the U = 2 B T units into P partial rows, dfilm as two wave sums per FiLM row and
// the fold kernel, nws_segment_sums for the partial rows.  The vector and scalar sums (at most 5 W + 4) are per-lane accumulators.
// A hidden layer's dW[o][i] = sum_n dz[o][n] h[i][n] does not fit the register file at width 16 (two layers: 512 per lane), so it
// runs on the fp32 matrix pipe: the wave writes its dz and h columns into LDS tiles [16][65] (lane = sample), reads them back
// transposed - A[o = lane & 15][k = lane >> 4], B[k][i = lane & 15] - and walks the unit's 64 samples in 16 steps of
// v_mfma_f32_16x16x4_f32: exact fp32 products in a fixed k order, 4 accumulator registers per layer.  Widths below the compiled
// tile (4, 8, 16) run with zero weights in the padding: sin 0 = 0 there and every padded dz is a product with a zero weight.
// Every output element is written by one thread and every sum runs in an order that depends on the sizes only: equal inputs give
// equal bits.  g = 0 gives zeros: every output is a sum of products with the factor dv = m_s g (or g itself).
#include "grad_sums.h"

namespace {

constexpr int kBlk = 64;           // samples per unit: one wave, one (i0, i1) pair
constexpr int kWaves = 4;
constexpr int kMinChunk = 32;      // units per workgroup while that gives at most kMaxP workgroups per shaper
constexpr int kMaxP = 256;
constexpr int kMaxS = 64, kMaxW = 16, kMaxD = 4;
constexpr int kTile = 16;          // the matrix tile; also the stride of a hidden layer's reduction rows
constexpr int kTileRow = kBlk + 1; // padded: the transposed reads of 16 rows land in different banks

// what the kernel reads: the shapers and the mixer, and where each gradient lies inside a partial row
struct GDesc {
  int S, W, D;
  const float* in_scale;
  const float* w[kMaxD];
  const float* b[kMaxD];
  const float* mix_w;
  int off_c, off_w[kMaxD], off_b[kMaxD], off_m, off_mb, stride;   // in floats
};

// the weights of ONE shaper, zero-padded to the compiled width WP (hidden: [in][out])
template <int WP>
struct Shaper1 {
  float w0[WP], b0[WP];
  float wh[2][WP * WP], bh[2][WP];
  float wl[WP];
  float bl, c, m, pad;
};

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

// D: the depth; WP: the compiled width (D = 1 has none and is compiled at 4); NH = D - 2 hidden layers
template <int D, int WP, bool PARAMS>
__global__ __launch_bounds__(256) void g_newt_grad_kernel(GDesc d, const float* __restrict__ exciter, const float* __restrict__ film,
                                                          const float* __restrict__ g, int T, int U, int chunk,
                                                          float* __restrict__ grad_exciter, float* __restrict__ part_film,
                                                          float* __restrict__ part_par) {
  constexpr int NH = D >= 2 ? D - 2 : 0;
  constexpr int NV = 5 * WP + 4;                         // c | w0 | b0 | bh[0] | bh[1] | wl | bl | m | mb
  __shared__ Shaper1<WP> Wt;
  __shared__ float red[kWaves][NV];
  __shared__ float tile[kWaves][2][NH ? kTile * kTileRow : 1];      // [wave][dz | h][row][sample]
  __shared__ float redh[kWaves][NH ? NH : 1][NH ? kTile * kTile : 1];
  const int s = blockIdx.x, p = blockIdx.y;
  const int S = d.S, W = d.W;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  if (tid < WP) {
    const bool in = tid < W;
    if (D == 1) {
      Wt.w0[tid] = tid == 0 ? d.w[0][s] : 0.0f;
      Wt.b0[tid] = tid == 0 ? d.b[0][s] : 0.0f;
      Wt.wl[tid] = 0.0f;
    } else {
      Wt.w0[tid] = in ? d.w[0][s * W + tid] : 0.0f;
      Wt.b0[tid] = in ? d.b[0][s * W + tid] : 0.0f;
      Wt.wl[tid] = in ? d.w[D - 1][s * W + tid] : 0.0f;
    }
#pragma unroll
    for (int l = 0; l < 2; ++l) Wt.bh[l][tid] = (l < NH && in) ? d.b[1 + l][s * W + tid] : 0.0f;
  }
#pragma unroll
  for (int l = 0; l < 2; ++l)
    for (int k = tid; k < WP * WP; k += 256) {            // k = o WP + i  ->  [i][o]
      const int o = k / WP, i = k - o * WP;
      Wt.wh[l][i * WP + o] = (l < NH && o < W && i < W) ? d.w[1 + l][((size_t)s * W + o) * W + i] : 0.0f;
    }
  if (tid == 0) {
    Wt.bl = D == 1 ? 0.0f : d.b[D - 1][s];
    Wt.c = d.in_scale[s];
    Wt.m = d.mix_w[s];
    Wt.pad = 0.0f;
  }
  if (NH) {                                               // rows past WP of the tiles are read by the matrix steps and never written
    float* t0 = &tile[wave][0][0];
    for (int k = lane; k < 2 * kTile * kTileRow; k += 64) t0[k] = 0.0f;
  }
  __syncthreads();

  const int N = T * NWS_HOP, nblk = 2 * T;
  const int q = chunk / kWaves;                                   // chunk is a multiple of kWaves
  const long long base = (long long)p * chunk + (long long)wave * q;
  const int u0 = (int)(base < U ? base : U);
  const int u1 = (int)(base + q < U ? base + q : U);

  float a_c = 0.0f, a_bl = 0.0f, a_m = 0.0f, a_mb = 0.0f;
  float a_w0[WP], a_b0[WP], a_wl[WP], a_bh[2][WP];
#pragma unroll
  for (int i = 0; i < WP; ++i) a_w0[i] = a_b0[i] = a_wl[i] = a_bh[0][i] = a_bh[1][i] = 0.0f;
  f32x4 a_W[2] = {{0.0f, 0.0f, 0.0f, 0.0f}, {0.0f, 0.0f, 0.0f, 0.0f}};      // dW[o = 4 (lane >> 4) + r][i = lane & 15]

  for (int u = u0; u < u1; ++u) {
    // the weights are read from LDS inside the unit: without the tile stores of PARAMS nothing in the loop writes LDS, the reads
    // are hoisted out of it into up to 468 registers, and the kernel runs one wave per SIMD at twice the time
    asm volatile("" ::: "memory");
    const int b = u / nblk, j = u - b * nblk;
    const int n = j * kBlk + lane;
    const NwsLerp lc = nws_lerp_coeff(n, T);
    const float* fb = film + (size_t)b * 4 * S * T;
    const float g_i = nws_lerp(fb[(size_t)s * T + lc.i0], fb[(size_t)s * T + lc.i1], lc.w0, lc.w1);
    const float b_i = nws_lerp(fb[(size_t)(S + s) * T + lc.i0], fb[(size_t)(S + s) * T + lc.i1], lc.w0, lc.w1);
    const float g_n = nws_lerp(fb[(size_t)(2 * S + s) * T + lc.i0], fb[(size_t)(2 * S + s) * T + lc.i1], lc.w0, lc.w1);
    const float b_n = nws_lerp(fb[(size_t)(3 * S + s) * T + lc.i0], fb[(size_t)(3 * S + s) * T + lc.i1], lc.w0, lc.w1);
    const size_t eoff = ((size_t)b * S + s) * N + n;
    const float e = exciter[eoff];
    const float gv = g[(size_t)b * N + n];

    // ---- forward ----
    const float x = g_i * e + b_i;
    const float a = Wt.c * x;
    float h[NH + 1][WP], c[NH + 1][WP];                     // h_1 .. h_{D-1} and the cosines of their arguments
    float y, cy;
    if (D == 1) {
      nws_sincosf_nocall(fmaf(Wt.w0[0], a, Wt.b0[0]), y, cy);
    } else {
#pragma unroll
      for (int i = 0; i < WP; ++i) nws_sincosf_nocall(fmaf(Wt.w0[i], a, Wt.b0[i]), h[0][i], c[0][i]);
#pragma unroll
      for (int l = 0; l < NH; ++l)
#pragma unroll
        for (int o = 0; o < WP; ++o) {
          float acc = Wt.bh[l][o];
#pragma unroll
          for (int i = 0; i < WP; ++i) acc = fmaf(Wt.wh[l][i * WP + o], h[l][i], acc);
          nws_sincosf_nocall(acc, h[l + 1][o], c[l + 1][o]);
        }
      float z = Wt.bl;
#pragma unroll
      for (int i = 0; i < WP; ++i) z = fmaf(Wt.wl[i], h[NH][i], z);
      nws_sincosf_nocall(z, y, cy);
    }

    // ---- backward ----
    const float dv = Wt.m * gv;
    if (PARAMS) {
      a_m = fmaf(gv, g_n * y + b_n, a_m);
      a_mb += gv;
    }
    const float dgn = dv * y;
    const float dzl = (g_n * dv) * cy;                     // d / d(argument of the last sine)
    float da = 0.0f;
    if (D == 1) {
      if (PARAMS) {
        a_w0[0] = fmaf(dzl, a, a_w0[0]);
        a_b0[0] += dzl;
      }
      da = Wt.w0[0] * dzl;
    } else {
      if (PARAMS) a_bl += dzl;
      float dz[WP];
#pragma unroll
      for (int o = 0; o < WP; ++o) {
        if (PARAMS) a_wl[o] = fmaf(dzl, h[NH][o], a_wl[o]);
        dz[o] = (Wt.wl[o] * dzl) * c[NH][o];
      }
#pragma unroll
      for (int l = NH - 1; l >= 0; --l) {                  // dz is d / d(z_{l+2}); the layer's inputs are h[l]
        if (PARAMS) {
          float* tz = &tile[wave][0][0];
          float* th = &tile[wave][1][0];
          __builtin_amdgcn_wave_barrier();
#pragma unroll
          for (int o = 0; o < WP; ++o) {
            a_bh[l][o] += dz[o];
            tz[o * kTileRow + lane] = dz[o];
            th[o * kTileRow + lane] = h[l][o];
          }
          __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
          __builtin_amdgcn_wave_barrier();
          __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
          const int r0 = (lane & 15) * kTileRow + (lane >> 4);
#pragma unroll
          for (int k = 0; k < kBlk / 4; ++k)
            a_W[l] = __builtin_amdgcn_mfma_f32_16x16x4f32(tz[r0 + 4 * k], th[r0 + 4 * k], a_W[l], 0, 0, 0);
          __builtin_amdgcn_wave_barrier();
        }
        float dn[WP];
#pragma unroll
        for (int i = 0; i < WP; ++i) {
          float acc = 0.0f;
#pragma unroll
          for (int o = 0; o < WP; ++o) acc = fmaf(Wt.wh[l][i * WP + o], dz[o], acc);
          dn[i] = acc * c[l][i];
        }
#pragma unroll
        for (int i = 0; i < WP; ++i) dz[i] = dn[i];
      }
#pragma unroll
      for (int i = 0; i < WP; ++i) {
        if (PARAMS) {
          a_w0[i] = fmaf(dz[i], a, a_w0[i]);
          a_b0[i] += dz[i];
        }
        da = fmaf(Wt.w0[i], dz[i], da);
      }
    }
    if (PARAMS) a_c = fmaf(da, x, a_c);
    const float dx = Wt.c * da;
    const float dgi = dx * e;
    if (grad_exciter != nullptr) grad_exciter[eoff] = g_i * dx;

    // ---- this block's share of dfilm: rows s, S+s, 2S+s, 3S+s get d = dgi, dx, dgn, dv ----
    const float d4[4] = {dgi, dx, dgn, dv};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float s0 = wave_sum(lc.w0 * d4[r]);
      const float s1 = wave_sum(lc.w1 * d4[r]);
      if (lane == 0) {
        float* pf = part_film + (((size_t)b * 4 * S + r * S + s) * nblk + j) * 2;
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
    for (int i = 0; i < WP; ++i) {
      flush(a_w0[i], 1 + i);
      flush(a_b0[i], 1 + WP + i);
      flush(a_bh[0][i], 1 + 2 * WP + i);
      flush(a_bh[1][i], 1 + 3 * WP + i);
      flush(a_wl[i], 1 + 4 * WP + i);
    }
    flush(a_bl, 5 * WP + 1);
    flush(a_m, 5 * WP + 2);
    flush(a_mb, 5 * WP + 3);
#pragma unroll
    for (int l = 0; l < NH; ++l)
#pragma unroll
      for (int r = 0; r < 4; ++r) redh[wave][l][(4 * (lane >> 4) + r) * kTile + (lane & 15)] = a_W[l][r];
    __syncthreads();
    float* row = part_par + (size_t)p * d.stride;
    if (tid < NV) {
      double tot = 0.0;
#pragma unroll
      for (int v = 0; v < kWaves; ++v) tot += (double)red[v][tid];
      const int k = tid - 1, f = k / WP, i = k - f * WP;      // for 1 <= tid <= 5 WP: field f, element i
      int off = -1;
      if (tid == 0) off = d.off_c + s;
      else if (tid == 5 * WP + 1) off = D >= 2 ? d.off_b[D - 1] + s : -1;
      else if (tid == 5 * WP + 2) off = d.off_m + s;
      else if (tid == 5 * WP + 3) off = s == 0 ? d.off_mb : -1;
      else if (D == 1) off = i == 0 ? (f == 0 ? d.off_w[0] + s : f == 1 ? d.off_b[0] + s : -1) : -1;
      else if (i < W) {
        if (f == 0) off = d.off_w[0] + s * W + i;
        else if (f == 1) off = d.off_b[0] + s * W + i;
        else if (f == 2) off = NH >= 1 ? d.off_b[1] + s * W + i : -1;
        else if (f == 3) off = NH >= 2 ? d.off_b[2] + s * W + i : -1;
        else off = d.off_w[D - 1] + s * W + i;
      }
      if (off >= 0) row[off] = (float)tot;
    }
#pragma unroll
    for (int l = 0; l < NH; ++l) {
      const int o = tid >> 4, i = tid & 15;
      if (o < W && i < W) {
        double tot = 0.0;
#pragma unroll
        for (int v = 0; v < kWaves; ++v) tot += (double)redh[v][l][tid];
        row[d.off_w[1 + l] + ((size_t)s * W + o) * W + i] = (float)tot;
      }
    }
  }
}

// dfilm[b][c][t]: the transpose of the x128 linear upsampling, newt_grad_fold_kernel of newt_grad.hip for any channel count.
// Block j of a row (samples 64 j .. 64 j + 63) names frames (i0, i1) = nws_lerp_coeff(64 j, T); frame t is named by blocks
// 2t-1 .. 2t+2 and, at the clamped ends, by block 0 / 2T-1.
__global__ __launch_bounds__(256) void g_newt_grad_fold_kernel(const float* __restrict__ part_film, int T, long long total,
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
  int seg_off[2 * kMaxD + 3], seg_n[2 * kMaxD + 3], nseg, stride;      // the 2 D + 3 gradients inside a partial row
  size_t off_par, bytes;      // part_film at 0; offsets in floats
  bool ok;
};

bool sizes_ok(const NwsShaperDesc* d) {
  return d->lut == nullptr && d->n_shapers >= 1 && d->n_shapers <= kMaxS && d->width >= 1 && d->width <= kMaxW && d->depth >= 1 &&
         d->depth <= kMaxD;
}

// the partition of newt_grad.hip's make_plan: a function of (B, T) only
Plan make_plan(const NwsShaperDesc* d, int B, int T, bool want) {
  Plan pl{};
  // lerp coefficients are exact for n < 2^23; the unit list and the fold kernel's grid stay inside int
  pl.ok = d && sizes_ok(d) && B >= 1 && T >= 1 && T <= 65535 && (long long)B * T <= (1ll << 28);
  if (!pl.ok) return pl;
  const int S = d->n_shapers, W = d->width, D = d->depth;
  int at = 0, k = 0;
  auto seg = [&](int n) {
    pl.seg_off[k] = at;
    pl.seg_n[k++] = n;
    at += n;
  };
  seg(S);                                                   // input_scale
  for (int l = 0; l < D; ++l) {
    const bool first = l == 0, last = l == D - 1;
    seg(D == 1 ? S : first || last ? S * W : S * W * W);    // net.{2l}.weight
    seg(last ? S : S * W);                                  // net.{2l}.bias
  }
  seg(S);                                                   // mixer.0.weight
  seg(1);                                                   // mixer.0.bias
  pl.nseg = k;
  pl.stride = (at + 3) / 4 * 4;
  pl.U = 2 * B * T;
  int chunk = (pl.U + kMaxP - 1) / kMaxP;
  chunk = (chunk + kWaves - 1) / kWaves * kWaves;
  pl.chunk = chunk < kMinChunk ? kMinChunk : chunk;
  pl.P = (pl.U + pl.chunk - 1) / pl.chunk;
  pl.off_par = (size_t)B * 4 * S * 2 * T * 2;
  pl.bytes = (pl.off_par + (want ? (size_t)pl.P * pl.stride : 0)) * sizeof(float);
  return pl;
}

template <int D, int WP>
void launch(bool want, dim3 grid, hipStream_t st, const GDesc& gd, const float* exciter, const float* film, const float* g, int T,
            const Plan& pl, float* grad_exciter, float* ws) {
  if (want)
    g_newt_grad_kernel<D, WP, true><<<grid, 256, 0, st>>>(gd, exciter, film, g, T, pl.U, pl.chunk, grad_exciter, ws, ws + pl.off_par);
  else
    g_newt_grad_kernel<D, WP, false><<<grid, 256, 0, st>>>(gd, exciter, film, g, T, pl.U, pl.chunk, grad_exciter, ws, nullptr);
}

template <int D>
void launch_width(int W, bool want, dim3 grid, hipStream_t st, const GDesc& gd, const float* exciter, const float* film, const float* g,
                  int T, const Plan& pl, float* grad_exciter, float* ws) {
  if (W <= 4)
    launch<D, 4>(want, grid, st, gd, exciter, film, g, T, pl, grad_exciter, ws);
  else if (W <= 8)
    launch<D, 8>(want, grid, st, gd, exciter, film, g, T, pl, grad_exciter, ws);
  else
    launch<D, 16>(want, grid, st, gd, exciter, film, g, T, pl, grad_exciter, ws);
}

}  // namespace

extern "C" size_t nws_g_newt_grad_workspace_bytes(const NwsShaperDesc* d, int B, int T, int want_params) {
  const Plan pl = make_plan(d, B, T, want_params != 0);
  return pl.ok ? pl.bytes : 0;
}

extern "C" int nws_g_newt_grad(const NwsShaperDesc* d, const float* mix_w, const float* mix_b, const float* exciter, const float* film,
                               const float* grad_out, int B, int T, int hop, float* grad_exciter, float* grad_film,
                               float* const* param_grads, void* workspace, size_t workspace_bytes, void* stream) {
  if (!d || !mix_w || !mix_b || !exciter || !film || !grad_out || !grad_film || B < 1 || T < 1 || hop < 1) return NWS_ERR_BAD_ARG;
  if (d->n_shapers < 1 || (d->lut == nullptr && (d->width < 1 || d->depth < 1))) return NWS_ERR_BAD_ARG;
  if (!sizes_ok(d) || hop != NWS_HOP) return NWS_ERR_UNSUPPORTED;      // a table, or width, depth or shapers out of range
  const int D = d->depth, ngrad = 2 * D + 3;
  if (!d->in_scale) return NWS_ERR_BAD_ARG;
  for (int l = 0; l < D; ++l)
    if (!d->w[l] || !d->b[l]) return NWS_ERR_BAD_ARG;
  int given = 0;
  if (param_grads)
    for (int i = 0; i < ngrad; ++i) given += param_grads[i] != nullptr;
  if (given != 0 && given != ngrad) return NWS_ERR_BAD_ARG;
  const bool want = given == ngrad;
  const Plan pl = make_plan(d, B, T, want);
  if (!pl.ok) return NWS_ERR_UNSUPPORTED;
  if (!workspace || workspace_bytes < pl.bytes) return NWS_ERR_BAD_ARG;

  GDesc gd{};
  gd.S = d->n_shapers;
  gd.W = d->width;
  gd.D = D;
  gd.in_scale = d->in_scale;
  gd.mix_w = mix_w;
  gd.off_c = pl.seg_off[0];
  for (int l = 0; l < D; ++l) {
    gd.w[l] = d->w[l];
    gd.b[l] = d->b[l];
    gd.off_w[l] = pl.seg_off[1 + 2 * l];
    gd.off_b[l] = pl.seg_off[2 + 2 * l];
  }
  gd.off_m = pl.seg_off[ngrad - 2];
  gd.off_mb = pl.seg_off[ngrad - 1];
  gd.stride = pl.stride;

  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const dim3 grid(gd.S, pl.P);
  switch (D) {
    case 1: launch<1, 4>(want, grid, st, gd, exciter, film, grad_out, T, pl, grad_exciter, ws); break;
    case 2: launch_width<2>(gd.W, want, grid, st, gd, exciter, film, grad_out, T, pl, grad_exciter, ws); break;
    case 3: launch_width<3>(gd.W, want, grid, st, gd, exciter, film, grad_out, T, pl, grad_exciter, ws); break;
    default: launch_width<4>(gd.W, want, grid, st, gd, exciter, film, grad_out, T, pl, grad_exciter, ws); break;
  }
  NWS_CHECK_LAUNCH();
  const long long total = (long long)B * 4 * gd.S * T;
  g_newt_grad_fold_kernel<<<(unsigned)((total + 255) / 256), 256, 0, st>>>(ws, T, total, grad_film);
  NWS_CHECK_LAUNCH();
  if (!want) return NWS_OK;
  SumSeg segs[2 * kMaxD + 3];
  for (int i = 0; i < ngrad; ++i) segs[i] = SumSeg{param_grads[i], pl.seg_off[i], pl.seg_n[i]};
  nws_segment_sums(ws + pl.off_par, pl.P, pl.stride, segs, ngrad, st);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}
