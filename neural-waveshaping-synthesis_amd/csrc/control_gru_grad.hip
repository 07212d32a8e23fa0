// Backward of the control encoder GRU(2 -> 128) (models/neural_waveshaping.py:17-26; forward: control_gru_kernel of
// control_gru.hip), DESIGN.md 3.17.
//
// Forward per utterance, gate order [r; z; n], x_t in R^2, h_{-1} = h0:
//   r = sigmoid(W_ir x_t + b_ir + W_hr h_{t-1} + b_hr)   z likewise   q = W_hn h_{t-1} + b_hn
//   n = tanh(W_in x_t + b_in + r q)                       h_t = (1 - z) n + z h_{t-1}
// Backward for G_t = dL/d(h_t) and an optional dL/d(h_T), walking t downwards, carry_T = dL/d(h_T) or 0:
//   dh_t = G_t + carry_{t+1}
//   c_n = (1 - z)(1 - n^2)   c_z = (h_{t-1} - n) z (1 - z)   c_q = c_n r   c_r = c_n q r (1 - r)
//   u_t = [c_r; c_z; c_n] * dh_t (input side)            v_t = [c_r; c_z; c_q] * dh_t (hidden side)
//   carry_t = z * dh_t + W_hh^T v_t                       dL/d(h0) = carry_0
//   dW_ih = sum u_t (x) x_t   db_ih = sum u_t   dW_hh = sum v_t (x) h_{t-1}   db_hh = sum v_t   dL/d(x_t) = W_ih^T u_t
//
// The coefficients z, c_r, c_z, c_q, c_n depend on the forward only; the one serial piece is dh_t and the 128 x 384 product.
//  * control_gru_coef_kernel (parallel): one workgroup = one utterance x 32 frames.  h_{t-1} is the forward's own gru_out shifted by
//    one frame (h0 in front), staged in LDS as [unit][frame]; the hidden-side pre-activations W_hh h_{t-1} are a 384 x 128 by
//    128 x 32 product on the fp32 matrix pipe (v_mfma_f32_32x32x2_f32, exact fp32 products): wave w owns units [32w, 32w + 32)
//    of all three gates, so a lane finds r, z and q of one (unit, frame) in the same accumulator slot and evaluates the gates
//    there with the forward's v_exp / v_rcp forms.  n = 1 - 2s and 1 - n^2 = 4 s (1 - s) with s = 1 / (1 + 2^(2 a log2 e)): no
//    cancellation where tanh saturates.  Five planes (B, T, 128) go to the workspace, 16 bytes per store.
//  * control_gru_bptt_kernel (sequential): one workgroup per utterance, persistent over the T steps, W_hh resident in registers
//    as the TRANSPOSE of the forward's operand: wave w owns outputs [32w, 32w + 32); lane l = 32a + 16s + 8k + p holds the four
//    outputs 32w + 4p + [0, 4) restricted to the contraction slice 4a + 2s + k (rows [48 (4a+2s+k), +48) of the 384): 192 weights
//    per lane, 96 packed FMAs per step like the forward, 12 broadcast ds_read_b128 of v_t (the slices lie 208 bytes apart in
//    LDS so the eight addresses of a read fall into different banks).  The reduction over the eight slices hands every lane ONE
//    output, 32w + 4p + 2a + s: two v_permlane32_swap (bit a: lanes a=0 keep outputs 0 and 1, a=1 outputs 2 and 3), one
//    v_permlane16_swap (bit s: which of the two), one DPP add (bit k: row_ror:8, both replicas get the sum).  Measured at
//    (64, 500): coefficients + this kernel 342 us against 362 us for the forward's own layout (two outputs per lane, four
//    slices of 96, 24 reads, one swap of each kind).  The lane of an output then adds z dh_t, forms
//    dh_{t-1} = G_{t-1} + carry_t and the three products of v_{t-1}, writes them into the other half of a ping-pong LDS buffer
//    and dh_{t-1} to the workspace: ONE barrier per step that waits on LDS only (the forward's).  G_{t-1} and the four
//    coefficients of frame t - 1 are requested at the top of step t and arrive under its FMAs.
//  * control_gru_grad_side_kernel (parallel, only when grad_control or the parameter gradients are wanted): one workgroup = one
//    utterance x 32 frames on the VALU.  dL/d(x_t) = W_ih^T u_t for its frames; with parameters the sums over its 32 frames
//    of u_t, v_t and u_t (x) x_t as one row of column sums.
//  * control_gru_grad_whh_kernel (with parameters): dW_hh[i][k] = sum v_t[i] h_{t-1}[k], a contraction over the B T frames on the
//    matrix pipe; one workgroup = one 32-row strip x one of P ranges of the (utterance, 32-frame chunk) list, P from (B, T) only.
//    The range split, the products of the tile and its write-out are grad_sums.h's (nws_unit_range, dw_tile_step,
//    dw_tile_store); the two fetches and the staging are this kernel's.
//  * nws_segment_sum_kernel (grad_sums.h): out[e] = sum_p part[p][e] in float64 in a fixed order, rounded once.
// Every output element is written by one thread, every sum runs in an order that depends on the sizes only, no atomics: equal
// inputs give equal bits.  G = 0 without dL/d(h_T) gives zeros: every output is a sum of products with a factor that is zero.
#include "grad_sums.h"

namespace {

constexpr int kH = NWS_HIDDEN;      // 128
constexpr int kG = 3 * kH;          // 384 gate rows
constexpr int kFT = 32;             // frames per workgroup of the parallel kernels
constexpr int kSlice = 48;          // contraction rows per lane slice of the BPTT kernel
constexpr int kSlicePad = 52;       // ... and their distance in LDS (floats)
constexpr int kNcol = 4 * kG;       // one row of column sums: db_ih (384) | db_hh (384) | dW_ih (768)
constexpr float kSig = -1.4426950408889634f, kTanh = 2.8853900817779268f;

// workgroup barrier that orders LDS traffic only (control_gru.hip): the dh_t stores are never drained on the critical path
__device__ __forceinline__ void gg_lds_barrier() {
  asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
}

struct GruW {
  const float* w_ih;   // (384, 2)
  const float* w_hh;   // (384, 128)
  const float* b_ih;   // (384)
  const float* b_hh;   // (384)
};

// planes: z | c_r | c_z | c_q | c_n, each (B, T, 128), `plane` floats apart
__global__ __launch_bounds__(256) void control_gru_coef_kernel(GruW w, const float* __restrict__ control, int C, int T,
                                                               const float* __restrict__ h0, const float* __restrict__ gru_out,
                                                               float* __restrict__ planes, size_t plane) {
  __shared__ float hp[kH * 33];       // h_{t-1} as [unit][frame]
  __shared__ float xs[2][kFT];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * kFT;
  const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  for (int i = tid; i < kH * kFT; i += 256) {
    const int k = i & (kH - 1), f = i >> 7, t = t0 + f;
    float v = 0.0f;
    if (t < T) {
      if (t == 0)
        v = h0 != nullptr ? h0[(size_t)b * kH + k] : 0.0f;
      else
        v = gru_out[((size_t)b * T + (t - 1)) * kH + k];
    }
    hp[k * 33 + f] = v;
  }
  if (tid < 2 * kFT) {
    const int c = tid >> 5, f = tid & 31, t = t0 + f;
    xs[c][f] = t < T ? control[((size_t)b * C + c) * T + t] : 0.0f;
  }
  __syncthreads();

  // hidden-side pre-activations: tile g = rows g*128 + 32 wave + [0, 32) of W_hh, columns = the 32 frames
  f32x16 acc[3];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[g][r] = 0.0f;
    const float* wr = w.w_hh + (size_t)(g * kH + 32 * wave + col) * kH;
    for (int k0 = 0; k0 < kH; k0 += 32) {
      const int kb = k0 + 16 * half;
      float av[16], bv[16];
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) {
        av[s2] = wr[kb + s2];
        bv[s2] = hp[(kb + s2) * 33 + col];
      }
#pragma unroll
      for (int s2 = 0; s2 < 16; ++s2) acc[g] = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s2], bv[s2], acc[g], 0, 0, 0);
    }
  }

  const int t = t0 + col;
  if (t >= T) return;
  const float x0 = xs[0][col], x1 = xs[1][col];
  float* out = planes + ((size_t)b * T + t) * kH + 32 * wave + 4 * half;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    float zv[4], crv[4], czv[4], cqv[4], cnv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      const int r = 4 * j + e;
      const int unit = 32 * wave + nws_frag_row(r, half);
      const float* wi = w.w_ih + (size_t)unit * 2;
      const float ar = fmaf(wi[1], x1, fmaf(wi[0], x0, w.b_ih[unit])) + (acc[0][r] + w.b_hh[unit]);
      const float az = fmaf(wi[2 * kH + 1], x1, fmaf(wi[2 * kH], x0, w.b_ih[kH + unit])) + (acc[1][r] + w.b_hh[kH + unit]);
      const float in = fmaf(wi[4 * kH + 1], x1, fmaf(wi[4 * kH], x0, w.b_ih[2 * kH + unit]));
      const float q = acc[2][r] + w.b_hh[2 * kH + unit];
      // sigmoid(a) = 1 / (1 + 2^(-a log2 e));  tanh(a) = 1 - 2 s, 1 - tanh^2(a) = 4 s (1 - s), s = 1 / (1 + 2^(2 a log2 e))
      const float rg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kSig * ar));
      const float zg = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kSig * az));
      const float s = __builtin_amdgcn_rcpf(1.0f + __builtin_amdgcn_exp2f(kTanh * fmaf(rg, q, in)));
      const float n = fmaf(-2.0f, s, 1.0f);
      const float omz = 1.0f - zg;
      const float cn = omz * (4.0f * s * (1.0f - s));
      zv[e] = zg;
      cnv[e] = cn;
      czv[e] = (hp[unit * 33 + col] - n) * (zg * omz);
      cqv[e] = cn * rg;
      crv[e] = cn * q * (rg * (1.0f - rg));
    }
    float* o = out + 8 * j;
    *reinterpret_cast<float4*>(o) = make_float4(zv[0], zv[1], zv[2], zv[3]);
    *reinterpret_cast<float4*>(o + plane) = make_float4(crv[0], crv[1], crv[2], crv[3]);
    *reinterpret_cast<float4*>(o + 2 * plane) = make_float4(czv[0], czv[1], czv[2], czv[3]);
    *reinterpret_cast<float4*>(o + 3 * plane) = make_float4(cqv[0], cqv[1], cqv[2], cqv[3]);
    *reinterpret_cast<float4*>(o + 4 * plane) = make_float4(cnv[0], cnv[1], cnv[2], cnv[3]);
  }
}

// where row i of the 384 lies in a v buffer: the eight 48-row slices 52 floats apart
__device__ __forceinline__ int gg_slot(int i) { return i + (kSlicePad - kSlice) * (i / kSlice); }

// v + (v of lane l ^ 8): a rotation by 8 inside the 16-lane row, on the VALU (DPP row_ror:8)
__device__ __forceinline__ float gg_sum_xor8(float v) {
  return v + __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x128, 0xf, 0xf, false));
}

__global__ __launch_bounds__(256, 1) void control_gru_bptt_kernel(const float* __restrict__ w_hh, int T,
                                                                  const float* __restrict__ grad_out,
                                                                  const float* __restrict__ grad_hT,
                                                                  const float* __restrict__ planes, size_t plane,
                                                                  float* __restrict__ dh_plane, float* __restrict__ grad_h0) {
  __shared__ __attribute__((aligned(16))) float v_lds[2][8 * kSlicePad];
  const int tid = threadIdx.x, b = blockIdx.x;
  const int lane = tid & 63, wave = tid >> 6;
  const int a = lane >> 5, s = (lane >> 4) & 1, k = (lane >> 3) & 1;
  const int sl = 4 * a + 2 * s + k;            // contraction slice
  const int ob = 32 * wave + 4 * (lane & 7);   // FMA phase: outputs ob .. ob + 3
  const int unit = ob + 2 * a + s;             // after the reduction: this lane's output
  const bool writer = k == 0;                  // one of the two replicas stores
  __builtin_amdgcn_s_setprio(3);

  // wreg[u][c] = (W_hh[48 sl + 2c][ob + u], W_hh[48 sl + 2c + 1][ob + u])
  f32x2 wreg[4][kSlice / 2];
#pragma unroll
  for (int c = 0; c < kSlice / 2; ++c) {
    const float* r0 = w_hh + (size_t)(kSlice * sl + 2 * c) * kH + ob;
#pragma unroll
    for (int u = 0; u < 4; ++u) wreg[u][c] = f32x2{r0[u], r0[kH + u]};
  }

  const float* zp = planes;
  const float* crp = planes + plane;
  const float* czp = planes + 2 * plane;
  const float* cqp = planes + 3 * plane;
  const size_t row0 = (size_t)b * T * kH + unit;
  const int s_r = gg_slot(unit), s_z = gg_slot(kH + unit), s_q = gg_slot(2 * kH + unit);

  // frame T - 1 starts from dL/d(h_T)
  float zd;
  {
    const size_t idx = row0 + (size_t)(T - 1) * kH;
    const float dh = grad_out[idx] + (grad_hT != nullptr ? grad_hT[(size_t)b * kH + unit] : 0.0f);
    if (writer) {
      v_lds[0][s_r] = crp[idx] * dh;
      v_lds[0][s_z] = czp[idx] * dh;
      v_lds[0][s_q] = cqp[idx] * dh;
      dh_plane[idx] = dh;
    }
    zd = zp[idx] * dh;
  }
  __syncthreads();

  int cur = 0;
  for (int t = T - 1; t >= 0; --t) {
    // frame t - 1: nothing here depends on the recurrence, so it is requested now and arrives under the FMAs
    float G = 0.0f, zn = 0.0f, cr = 0.0f, cz = 0.0f, cq = 0.0f;
    const size_t idx = row0 + (size_t)(t > 0 ? t - 1 : 0) * kH;
    if (t > 0) {
      G = grad_out[idx];
      zn = zp[idx];
      cr = crp[idx];
      cz = czp[idx];
      cq = cqp[idx];
    }
    const float4* vp = reinterpret_cast<const float4*>(&v_lds[cur][kSlicePad * sl]);
    f32x2 acc[4][2];
#pragma unroll
    for (int u = 0; u < 4; ++u) acc[u][0] = acc[u][1] = f32x2{0.0f, 0.0f};
    float4 vb[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) vb[i] = vp[i];
#pragma unroll
    for (int q = 0; q < kSlice / 4; ++q) {
      const float4 vv = vb[q & 3];
      const f32x2 v01 = {vv.x, vv.y}, v23 = {vv.z, vv.w};
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u][0] = __builtin_elementwise_fma(wreg[u][2 * q], v01, acc[u][0]);
#pragma unroll
      for (int u = 0; u < 4; ++u) acc[u][1] = __builtin_elementwise_fma(wreg[u][2 * q + 1], v23, acc[u][1]);
      if (q + 4 < kSlice / 4) vb[q & 3] = vp[q + 4];
      __builtin_amdgcn_sched_barrier(0);
    }
    float o[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const f32x2 su = acc[u][0] + acc[u][1];
      o[u] = nws_add_scalar(su.x, su.y);
    }
    // over the slice bit a: lanes a=0 receive both halves of outputs 0 and 1, lanes a=1 of outputs 2 and 3;
    // over the bit s: rows s=0 keep the first of those two, rows s=1 the second; over the bit k: both replicas get the sum
    const auto e = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[0]), __float_as_uint(o[2]), false, false);
    const auto f = __builtin_amdgcn_permlane32_swap(__float_as_uint(o[1]), __float_as_uint(o[3]), false, false);
    const float x0 = __uint_as_float(e[0]) + __uint_as_float(e[1]), x1 = __uint_as_float(f[0]) + __uint_as_float(f[1]);
    const auto g2 = __builtin_amdgcn_permlane16_swap(__float_as_uint(x0), __float_as_uint(x1), false, false);
    const float carry = zd + gg_sum_xor8(__uint_as_float(g2[0]) + __uint_as_float(g2[1]));
    if (t > 0) {
      const float dh = G + carry;
      if (writer) {
        v_lds[cur ^ 1][s_r] = cr * dh;
        v_lds[cur ^ 1][s_z] = cz * dh;
        v_lds[cur ^ 1][s_q] = cq * dh;
        dh_plane[idx] = dh;
      }
      zd = zn * dh;
      gg_lds_barrier();
      cur ^= 1;
    } else if (grad_h0 != nullptr && writer) {
      grad_h0[(size_t)b * kH + unit] = carry;
    }
  }
}

// LDS: pc [64][129] partial products of W_ih^T u per (frame, channel) and unit | comb [10][128] | xs [2][32]
__global__ __launch_bounds__(256) void control_gru_grad_side_kernel(const float* __restrict__ w_ih, const float* __restrict__ control,
                                                                    int C, int T, const float* __restrict__ planes, size_t plane,
                                                                    const float* __restrict__ dh_plane,
                                                                    float* __restrict__ grad_control, float* __restrict__ col_part) {
  __shared__ float pc[2 * kFT * 129];
  __shared__ float comb[10][kH];
  __shared__ float xs[2][kFT];
  const int tid = threadIdx.x, b = blockIdx.y, t0 = blockIdx.x * kFT;
  const int unit = tid & (kH - 1), fh = tid >> 7;
  const bool want = col_part != nullptr, gc = grad_control != nullptr;
  if (tid < 2 * kFT) {
    const int c = tid >> 5, f = tid & 31, t = t0 + f;
    xs[c][f] = t < T ? control[((size_t)b * C + c) * T + t] : 0.0f;
  }
  __syncthreads();
  float wi[3][2];
#pragma unroll
  for (int g = 0; g < 3; ++g) {
    wi[g][0] = w_ih[(size_t)(g * kH + unit) * 2];
    wi[g][1] = w_ih[(size_t)(g * kH + unit) * 2 + 1];
  }
  const float* crp = planes + plane;
  const float* czp = planes + 2 * plane;
  const float* cqp = planes + 3 * plane;
  const float* cnp = planes + 4 * plane;
  float sums[10];
#pragma unroll
  for (int j = 0; j < 10; ++j) sums[j] = 0.0f;
  for (int ff = 0; ff < kFT / 2; ++ff) {
    const int f = fh * (kFT / 2) + ff, t = t0 + f;
    float ur = 0.0f, uz = 0.0f, un = 0.0f, vq = 0.0f;
    if (t < T) {
      const size_t idx = ((size_t)b * T + t) * kH + unit;
      const float dh = dh_plane[idx];
      ur = crp[idx] * dh;
      uz = czp[idx] * dh;
      un = cnp[idx] * dh;
      vq = cqp[idx] * dh;
    }
    const float x0 = xs[0][f], x1 = xs[1][f];
    sums[0] += ur;
    sums[1] += uz;
    sums[2] += un;
    sums[3] += vq;
    sums[4] = fmaf(ur, x0, sums[4]);
    sums[5] = fmaf(ur, x1, sums[5]);
    sums[6] = fmaf(uz, x0, sums[6]);
    sums[7] = fmaf(uz, x1, sums[7]);
    sums[8] = fmaf(un, x0, sums[8]);
    sums[9] = fmaf(un, x1, sums[9]);
    if (gc) {
      pc[(2 * f) * 129 + unit] = fmaf(wi[2][0], un, fmaf(wi[1][0], uz, wi[0][0] * ur));
      pc[(2 * f + 1) * 129 + unit] = fmaf(wi[2][1], un, fmaf(wi[1][1], uz, wi[0][1] * ur));
    }
  }
  if (fh == 1) {
#pragma unroll
    for (int j = 0; j < 10; ++j) comb[j][unit] = sums[j];
  }
  __syncthreads();
  if (want && fh == 0) {
    float* row = col_part + ((size_t)b * gridDim.x + blockIdx.x) * kNcol;
#pragma unroll
    for (int j = 0; j < 10; ++j) sums[j] += comb[j][unit];
    row[unit] = sums[0];                    // db_ih
    row[kH + unit] = sums[1];
    row[2 * kH + unit] = sums[2];
    row[kG + unit] = sums[0];               // db_hh
    row[kG + kH + unit] = sums[1];
    row[kG + 2 * kH + unit] = sums[3];
#pragma unroll
    for (int g = 0; g < 3; ++g) {           // dW_ih
      row[2 * kG + (g * kH + unit) * 2] = sums[4 + 2 * g];
      row[2 * kG + (g * kH + unit) * 2 + 1] = sums[5 + 2 * g];
    }
  }
  if (gc && tid < 2 * kFT) {
    const int f = tid >> 1, c = tid & 1, t = t0 + f;
    float s = 0.0f;
    for (int k = 0; k < kH; ++k) s += pc[tid * 129 + k];
    if (t < T) grad_control[((size_t)b * 2 + c) * T + t] = s;
  }
}

// part[p][i][k] = sum over the (utterance, chunk) units of range p of v[i] h_{t-1}[k];  LDS: sA [32][33] | sB [128][33]
__global__ __launch_bounds__(256) void control_gru_grad_whh_kernel(const float* __restrict__ h0, const float* __restrict__ gru_out,
                                                                   const float* __restrict__ planes, size_t plane,
                                                                   const float* __restrict__ dh_plane, int T, int nchunk, int U,
                                                                   float* __restrict__ part) {
  __shared__ float sA[32 * 33];
  __shared__ float sB[kH * 33];
  const int mt = blockIdx.x, p = blockIdx.y;
  const int tid = threadIdx.x;
  const int lane = tid & 63, wave = tid >> 6, half = lane >> 5, col = lane & 31;
  const int gate = mt >> 2, ub = 32 * (mt & 3);
  const float* coef = planes + (size_t)(gate == 0 ? 1 : gate == 1 ? 2 : 3) * plane;      // c_r, c_z, c_q
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
  float ra[4], rb[16];
  auto fetch = [&](int u) {
    const int b = u / nchunk, tb = (u - b * nchunk) * kFT;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int t = tb + (tid >> 5) + 8 * q;
      float v = 0.0f;
      if (t < T) {
        const size_t idx = ((size_t)b * T + t) * kH + ub + (tid & 31);
        v = coef[idx] * dh_plane[idx];
      }
      ra[q] = v;
    }
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int t = tb + (tid >> 7) + 2 * q, k = tid & (kH - 1);
      float v = 0.0f;
      if (t < T) {
        if (t == 0)
          v = h0 != nullptr ? h0[(size_t)b * kH + k] : 0.0f;
        else
          v = gru_out[((size_t)b * T + (t - 1)) * kH + k];
      }
      rb[q] = v;
    }
  };
  const UnitRange ur = nws_unit_range(p, gridDim.y, U);
  if (ur.u0 < ur.u1) fetch(ur.u0);
  for (int u = ur.u0; u < ur.u1; ++u) {
#pragma unroll
    for (int q = 0; q < 4; ++q) sA[(tid & 31) * 33 + (tid >> 5) + 8 * q] = ra[q];
#pragma unroll
    for (int q = 0; q < 16; ++q) sB[(tid & (kH - 1)) * 33 + (tid >> 7) + 2 * q] = rb[q];
    __syncthreads();
    if (u + 1 < ur.u1) fetch(u + 1);                                // in flight under this unit's products
    float av[16];
    dw_read16(sA, col, half, av);
    dw_tile_step(av, sB, 32 * wave + col, half, acc);               // wave w owns the 32-column tile w
    __syncthreads();
  }
  dw_tile_store(acc, part + (size_t)p * kG * kH, kG, kH, 32 * mt, 32 * wave + col, half);
}

struct GPlan {
  int ntile, U, P;
  size_t plane, off_dh, off_col, off_w, bytes;      // offsets in floats
  bool ok;
};

GPlan make_plan(int B, int T, bool want) {
  GPlan pl{};
  pl.ok = B >= 1 && T >= 1 && B <= 65535;
  if (!pl.ok) return pl;
  pl.ntile = (T + kFT - 1) / kFT;
  const long long U = (long long)B * pl.ntile;
  if (U > kMaxUnits) {
    pl.ok = false;
    return pl;
  }
  pl.U = (int)U;
  pl.P = nws_partial_count(U);
  pl.plane = (size_t)B * T * kH;
  pl.off_dh = 5 * pl.plane;
  pl.off_col = 6 * pl.plane;
  pl.off_w = pl.off_col + (want ? (size_t)pl.U * kNcol : 0);
  pl.bytes = (pl.off_w + (want ? (size_t)pl.P * kG * kH : 0)) * sizeof(float);
  return pl;
}

}  // namespace

extern "C" size_t nws_control_gru_grad_workspace_bytes(int B, int T, int want_params) {
  const GPlan pl = make_plan(B, T, want_params != 0);
  return pl.ok ? pl.bytes : 0;
}

extern "C" int nws_control_gru_grad(const NwsWeights* w, const float* control, int B, int C, int T, const float* h0,
                                    const float* gru_out, const float* grad_out, const float* grad_hT, float* grad_control,
                                    float* grad_h0, float* grad_w_ih, float* grad_w_hh, float* grad_b_ih, float* grad_b_hh,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  if (!w || !w->gru_w_ih || !w->gru_w_hh || !w->gru_b_ih || !w->gru_b_hh || !control || !gru_out || !grad_out) return NWS_ERR_BAD_ARG;
  if (B <= 0 || T <= 0 || C < 2) return NWS_ERR_BAD_ARG;
  const int given = (grad_w_ih != nullptr) + (grad_w_hh != nullptr) + (grad_b_ih != nullptr) + (grad_b_hh != nullptr);
  if (given != 0 && given != 4) return NWS_ERR_BAD_ARG;
  const bool want = given == 4;
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  const GPlan pl = make_plan(B, T, want);
  if (!pl.ok) return NWS_ERR_UNSUPPORTED;
  // (the planes are written 16 bytes at a time)
  if (!workspace || workspace_bytes < pl.bytes || (reinterpret_cast<uintptr_t>(workspace) & 15) != 0) return NWS_ERR_BAD_ARG;

  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  const GruW gw{w->gru_w_ih, w->gru_w_hh, w->gru_b_ih, w->gru_b_hh};
  control_gru_coef_kernel<<<dim3(pl.ntile, B), 256, 0, st>>>(gw, control, C, T, h0, gru_out, ws, pl.plane);
  NWS_CHECK_LAUNCH();
  control_gru_bptt_kernel<<<B, 256, 0, st>>>(gw.w_hh, T, grad_out, grad_hT, ws, pl.plane, ws + pl.off_dh, grad_h0);
  NWS_CHECK_LAUNCH();
  if (!want && grad_control == nullptr) return NWS_OK;
  control_gru_grad_side_kernel<<<dim3(pl.ntile, B), 256, 0, st>>>(gw.w_ih, control, C, T, ws, pl.plane, ws + pl.off_dh, grad_control,
                                                                  want ? ws + pl.off_col : nullptr);
  NWS_CHECK_LAUNCH();
  if (!want) return NWS_OK;
  control_gru_grad_whh_kernel<<<dim3(kG / 32, pl.P), 256, 0, st>>>(h0, gru_out, ws, pl.plane, ws + pl.off_dh, T, pl.ntile, pl.U,
                                                                   ws + pl.off_w);
  NWS_CHECK_LAUNCH();
  const SumSeg rw[1] = {{grad_w_hh, 0, kG * kH}};
  nws_segment_sums(ws + pl.off_w, pl.P, (long long)kG * kH, rw, 1, st);
  NWS_CHECK_LAUNCH();
  const SumSeg rc[3] = {{grad_b_ih, 0, kG}, {grad_b_hh, kG, kG}, {grad_w_ih, 2 * kG, 2 * kG}};
  nws_segment_sums(ws + pl.off_col, pl.U, (long long)kNcol, rc, 3, st);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}
