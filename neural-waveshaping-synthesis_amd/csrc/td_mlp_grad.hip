// Backward of TimeDistributedMLP (models/modules/dynamic.py:11-40; forward: td_mlp_kernel of stages.hip), DESIGN.md 3.16.
//
// Forward per frame, layers i = 0 .. depth-1, a_{-1} = x:
//   z_i = W_i a_{i-1} + b_i,  n_i = (z_i - mean_c z_i) rstd_i,  v_i = gamma_i n_i + beta_i,  a_i = leaky(v_i),  y = z_{depth-1}
// Backward for g = dL/dy, dz_{depth-1} = g, walking i downwards:
//   dW_i = sum_{b,t} dz_i (x) a_{i-1}   db_i = sum_{b,t} dz_i   da_{i-1} = W_i^T dz_i   (da_{-1} = dL/dx)
//   dv_i = da_i (v_i > 0 ? 1 : slope)   dbeta_i = sum dv_i   dgamma_i = sum dv_i n_i   dn_i = gamma_i dv_i
//   dz_i = rstd_i (dn_i - mean_c dn_i - n_i mean_c(dn_i n_i))
//
// Nothing is saved but x.  Three kernels, every product exact fp32 (v_mfma_f32_32x32x2_f32 or plain VALU), no atomics:
//  * td_mlp_grad_data_kernel: one workgroup = one utterance x 32 frames, like the forward.  It repeats the forward sweep of
//    layers 0 .. depth-2 with the forward's own arithmetic and keeps n_i of every layer in LDS (a_i and the sign of v_i follow from
//    n_i with the forward's two roundings, so they are not stored) and rstd_i per frame.  The backward sweep contracts W_i^T dz_i
//    on the matrix pipe: the weights are read transposed straight from memory (for a fixed output channel the 32 lanes of a
//    half-wave read 32 consecutive input channels: coalesced dword loads, any alignment), dz_i comes from LDS, g from memory.
//    dL/dx leaves from the accumulators.  With parameter gradients wanted it also writes the planes a_i and dz_i (i < depth-1) and,
//    per workgroup, the column sums over its 32 frames of dz_i, dv_i and dv_i n_i (and of g) into the workspace.
//  * td_mlp_grad_weights_kernel: dW_i[o][k] = sum over frames of dz_i[o] a_{i-1}[k], a contraction over the B T frames on the
//    matrix pipe.  One workgroup = one 32-row strip of one layer's dW x one of P ranges of the (utterance, 32-frame chunk) list;
//    P depends on (B, T) only.  The partial strips go to the workspace.  The range split, the products of a tile and its
//    write-out are grad_sums.h's (nws_unit_range, dw_tile_step, dw_tile_store); the two fetches and the staging are this kernel's.
//  * nws_segment_sum_kernel (grad_sums.h): out[e] = sum_p part[p][e] in float64 in a fixed order, rounded once.  One launch for
//    the dW partials, one for the column sums.
// Every output element is written by one thread, every sum runs in an order that depends on the sizes only: equal inputs give
// equal bits.  g = 0 gives zeros: every output is a sum of products with a factor that is exactly zero.
#include "grad_sums.h"

namespace {

constexpr int kFT = 32;         // frames per workgroup
constexpr int kMaxDepth = 8;
constexpr int kMaxWidth = 256;  // layer widths the plan covers (two 32-column tiles per wave in the weights kernel)
constexpr int kLdsMax = 160 * 1024;

struct GradArgs {
  const float* w[kMaxDepth];
  const float* b[kMaxDepth];
  const float* ln_g[kMaxDepth];
  const float* ln_b[kMaxDepth];
};

// LDS: act [maxw][33] | n_0 .. n_{depth-2} [hidden][33] each | red [2][8][32] | rstd [depth-1][32]
__global__ __launch_bounds__(256) void td_mlp_grad_data_kernel(GradArgs a, const float* __restrict__ x,
                                                               const float* __restrict__ g, int in_size, int hidden,
                                                               int out_size, int depth, int T, float eps, float slope,
                                                               float* __restrict__ grad_x, float* __restrict__ a_planes,
                                                               float* __restrict__ dz_planes, float* __restrict__ col_part,
                                                               int ncol) {
  extern __shared__ float lds[];
  const int maxw = in_size > hidden ? in_size : hidden;
  const size_t plane = (size_t)hidden * 33;
  float* act = lds;
  float* nbase = lds + (size_t)maxw * 33;
  float* red = nbase + (size_t)(depth - 1) * plane;
  float* rstd_s = red + 512;
  const int B = gridDim.y, b = blockIdx.y, t0 = blockIdx.x * kFT;
  const int f = threadIdx.x & 31, cg = threadIdx.x >> 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;
  const int t = t0 + f;
  const bool live = t < T;
  const bool want = col_part != nullptr;
  float* colrow = want ? col_part + ((size_t)b * gridDim.x + blockIdx.x) * ncol : nullptr;
  const size_t hplane = (size_t)B * hidden * T;     // one (B, hidden, T) plane of the workspace

  for (int c = cg; c < in_size; c += 8) act[c * 33 + f] = live ? x[((size_t)b * in_size + c) * T + t] : 0.0f;
  __syncthreads();

  // ---- forward sweep, layers 0 .. depth-2: td_mlp_kernel's arithmetic; plane `layer` keeps n, act the layer's output ----
  for (int layer = 0; layer < depth - 1; ++layer) {
    const int cin = layer == 0 ? in_size : hidden;
    const int cout = hidden;
    const float* __restrict__ W = a.w[layer];
    const float* __restrict__ bias = a.b[layer];
    float* np = nbase + layer * plane;
    const bool vec = (cin & 3) == 0 && (reinterpret_cast<uintptr_t>(W) & 15) == 0;
    for (int mt = wave; 32 * mt < cout; mt += 4) {
      const int row = 32 * mt + col;
      const float* wr = W + (size_t)(row < cout ? row : cout - 1) * cin;
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
      for (int k0 = 0; k0 < cin; k0 += 32) {
        const int kb = k0 + 16 * half;
        float av[16];
        if (vec && kb + 16 <= cin) {
#pragma unroll
          for (int q4 = 0; q4 < 4; ++q4) {
            const float4 v4 = *reinterpret_cast<const float4*>(wr + kb + 4 * q4);
            av[4 * q4] = v4.x;
            av[4 * q4 + 1] = v4.y;
            av[4 * q4 + 2] = v4.z;
            av[4 * q4 + 3] = v4.w;
          }
        } else {
#pragma unroll
          for (int s2 = 0; s2 < 16; ++s2) av[s2] = kb + s2 < cin ? wr[kb + s2] : 0.0f;
        }
        if (row >= cout) {
#pragma unroll
          for (int s2 = 0; s2 < 16; ++s2) av[s2] = 0.0f;
        }
        float bv[16];
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
          const int k = kb + s2 < cin ? kb + s2 : cin - 1;      // rows beyond cin meet zero weights
          bv[s2] = act[k * 33 + col];
        }
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s2], bv[s2], acc, 0, 0, 0);
      }
#pragma unroll
      for (int r = 0; r < 16; ++r) {
        const int c = 32 * mt + nws_frag_row(r, half);
        if (c < cout) np[c * 33 + col] = acc[r] + bias[c];
      }
    }
    __syncthreads();
    float s1 = 0.0f;
    for (int c = cg; c < cout; c += 8) s1 += np[c * 33 + f];
    red[cg * 32 + f] = s1;
    __syncthreads();
    float mean = 0.0f;
    for (int q = 0; q < 8; ++q) mean += red[q * 32 + f];
    mean /= (float)cout;
    float s2 = 0.0f;
    for (int c = cg; c < cout; c += 8) {
      const float d = np[c * 33 + f] - mean;
      s2 = fmaf(d, d, s2);
    }
    red[256 + cg * 32 + f] = s2;
    __syncthreads();
    float var = 0.0f;
    for (int q = 0; q < 8; ++q) var += red[256 + q * 32 + f];
    // a frame past the end carries x = 0 and g = 0: rstd = 0 keeps its n finite whatever eps is, so its products are zeros
    const float rstd = live ? 1.0f / sqrtf(var / (float)cout + eps) : 0.0f;
    if (cg == 0) rstd_s[layer * 32 + f] = rstd;
    const float* __restrict__ gam = a.ln_g[layer];
    const float* __restrict__ bet = a.ln_b[layer];
    float* ap = want ? a_planes + layer * hplane + (size_t)b * hidden * T + t : nullptr;
    for (int c = cg; c < cout; c += 8) {
      const float n = (np[c * 33 + f] - mean) * rstd;
      const float v = n * gam[c] + bet[c];
      const float av = v > 0.0f ? v : slope * v;
      np[c * 33 + f] = n;
      act[c * 33 + f] = av;
      if (want && live) ap[(size_t)c * T] = av;
    }
    __syncthreads();
  }

  // the column sum of g over this tile: the partial of db_{depth-1}
  if (want) {
    for (int c = threadIdx.x; c < out_size; c += 256) {
      const float* gr = g + ((size_t)b * out_size + c) * T;
      float s = 0.0f;
      for (int ff = 0; ff < kFT; ++ff) s += t0 + ff < T ? gr[t0 + ff] : 0.0f;
      colrow[3 * (depth - 1) * hidden + c] = s;
    }
  }

  // ---- backward sweep: layer L turns dz_L (g, or the plane the previous step left) into dv_{L-1}, then dz_{L-1} ----
  for (int layer = depth - 1; layer >= 0; --layer) {
    const int cin = layer == 0 ? in_size : hidden;                 // rows of the product W^T dz
    const int cout = layer == depth - 1 ? out_size : hidden;       // its contraction length
    const float* __restrict__ W = a.w[layer];
    const bool top = layer == depth - 1;
    // dz_L sits where layer L + 1 wrote it; dv_{L-1} goes to a plane nobody needs any more (n_L: dz_L is done)
    const float* dzp = top ? nullptr : (layer == depth - 2 ? act : nbase + (layer + 1) * plane);
    float* outp = top ? act : nbase + layer * plane;
    const float* np = layer > 0 ? nbase + (layer - 1) * plane : nullptr;
    const float* __restrict__ gam = layer > 0 ? a.ln_g[layer - 1] : nullptr;
    const float* __restrict__ bet = layer > 0 ? a.ln_b[layer - 1] : nullptr;
    const float* gcol = g + (size_t)b * out_size * T + (live ? t : T - 1);     // frame t0 + col (f == col)
    for (int mt = wave; 32 * mt < cin; mt += 4) {
      const int row = 32 * mt + col;                               // input channel of this lane's A rows
      const float* wc = W + (row < cin ? row : cin - 1);
      f32x16 acc;
#pragma unroll
      for (int r = 0; r < 16; ++r) acc[r] = 0.0f;
      for (int k0 = 0; k0 < cout; k0 += 32) {
        const int kb = k0 + 16 * half;
        float av[16], bv[16];
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) {
          const int k = kb + s2 < cout ? kb + s2 : cout - 1;
          const float wv = wc[(size_t)k * cin];
          av[s2] = (kb + s2 < cout && row < cin) ? wv : 0.0f;
          if (top) {
            const float gv = gcol[(size_t)k * T];
            bv[s2] = live ? gv : 0.0f;
          } else {
            bv[s2] = dzp[k * 33 + col];
          }
        }
#pragma unroll
        for (int s2 = 0; s2 < 16; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s2], bv[s2], acc, 0, 0, 0);
      }
      if (layer == 0) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = 32 * mt + nws_frag_row(r, half);
          if (c < cin && live) grad_x[((size_t)b * in_size + c) * T + t] = acc[r];
        }
      } else {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          const int c = 32 * mt + nws_frag_row(r, half);
          if (c < cin) {
            const float v = np[c * 33 + col] * gam[c] + bet[c];     // the forward's v, rounding for rounding
            outp[c * 33 + col] = acc[r] * (v > 0.0f ? 1.0f : slope);
          }
        }
      }
    }
    if (layer == 0) break;
    __syncthreads();
    // LayerNorm backward of layer L - 1 over the hidden channels of frame f; dbeta and dgamma partials from the same plane
    const int li = layer - 1;
    if (want) {
      for (int c = threadIdx.x; c < hidden; c += 256) {
        float sb = 0.0f, sg = 0.0f;
        for (int ff = 0; ff < kFT; ++ff) {
          const float dv = outp[c * 33 + ff];
          sb += dv;
          sg = fmaf(dv, np[c * 33 + ff], sg);
        }
        colrow[(3 * li + 1) * hidden + c] = sb;
        colrow[(3 * li + 2) * hidden + c] = sg;
      }
    }
    float s1 = 0.0f, s2 = 0.0f;
    for (int c = cg; c < hidden; c += 8) {
      const float dn = gam[c] * outp[c * 33 + f];
      s1 += dn;
      s2 = fmaf(dn, np[c * 33 + f], s2);
    }
    red[cg * 32 + f] = s1;
    red[256 + cg * 32 + f] = s2;
    __syncthreads();
    float m1 = 0.0f, m2 = 0.0f;
    for (int q = 0; q < 8; ++q) {
      m1 += red[q * 32 + f];
      m2 += red[256 + q * 32 + f];
    }
    m1 /= (float)hidden;
    m2 /= (float)hidden;
    const float rstd = rstd_s[li * 32 + f];
    float* zp = want ? dz_planes + li * hplane + (size_t)b * hidden * T + t : nullptr;
    for (int c = cg; c < hidden; c += 8) {
      const float dn = gam[c] * outp[c * 33 + f];
      const float dz = live ? rstd * ((dn - m1) - np[c * 33 + f] * m2) : 0.0f;
      outp[c * 33 + f] = dz;
      if (want && live) zp[(size_t)c * T] = dz;
    }
    __syncthreads();
    if (want) {
      for (int c = threadIdx.x; c < hidden; c += 256) {
        float s = 0.0f;
        for (int ff = 0; ff < kFT; ++ff) s += outp[c * 33 + ff];
        colrow[(3 * li) * hidden + c] = s;
      }
    }
  }
}

struct WLayer {
  const float* dz;    // (B, cout, T)
  const float* a;     // (B, cin, T)
  float* part;        // this layer's (cout, cin) block of partial 0; partial p lies p * wsum floats further
  int cout, cin, strip0;
};
struct WArgs {
  WLayer L[kMaxDepth];
};

// LDS: sA [32][33] | sB [cin][33]
__global__ __launch_bounds__(256) void td_mlp_grad_weights_kernel(WArgs wa, int depth, int T, int nchunk, int U,
                                                                  long long wsum) {
  extern __shared__ float lds[];
  int li = 0;
  for (int i = 1; i < depth; ++i)
    if ((int)blockIdx.x >= wa.L[i].strip0) li = i;
  const float* __restrict__ dz = wa.L[li].dz;
  const float* __restrict__ ap = wa.L[li].a;
  const int cout = wa.L[li].cout, cin = wa.L[li].cin;
  const int mt = blockIdx.x - wa.L[li].strip0;
  const int p = blockIdx.y;
  float* sA = lds;
  float* sB = lds + 32 * 33;
  const int f = threadIdx.x & 31, cg = threadIdx.x >> 5;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, half = lane >> 5, col = lane & 31;

  f32x16 acc0, acc1;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    acc0[r] = 0.0f;
    acc1[r] = 0.0f;
  }
  float ra[4], rb[kMaxWidth / 8];
  // unit u = (utterance, 32-frame chunk): this thread's share of the two staged tiles, rows and frames past the end as zeros
  auto fetch = [&](int u) {
    const int b = u / nchunk, t = (u - b * nchunk) * kFT + f;
    const bool live = t < T;
    const int tc = live ? t : T - 1;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int row = 32 * mt + cg + 8 * q;
      const float v = dz[((size_t)b * cout + (row < cout ? row : cout - 1)) * T + tc];
      ra[q] = (live && row < cout) ? v : 0.0f;
    }
#pragma unroll
    for (int q = 0; q < kMaxWidth / 8; ++q) {
      const int row = cg + 8 * q;
      if (8 * q < cin) {                                            // (uniform)
        const float v = ap[((size_t)b * cin + (row < cin ? row : cin - 1)) * T + tc];
        rb[q] = (live && row < cin) ? v : 0.0f;
      }
    }
  };
  // wave w owns the 32-column tiles w and w + 4; columns beyond cin are computed and not stored
  const int c0 = 32 * wave + col, c1 = 32 * (wave + 4) + col;
  const UnitRange ur = nws_unit_range(p, gridDim.y, U);
  if (ur.u0 < ur.u1) fetch(ur.u0);
  for (int u = ur.u0; u < ur.u1; ++u) {
#pragma unroll
    for (int q = 0; q < 4; ++q) sA[(cg + 8 * q) * 33 + f] = ra[q];
#pragma unroll
    for (int q = 0; q < kMaxWidth / 8; ++q)
      if (cg + 8 * q < cin) sB[(cg + 8 * q) * 33 + f] = rb[q];
    __syncthreads();
    if (u + 1 < ur.u1) fetch(u + 1);                                // in flight under this unit's products
    float av[16];
    dw_read16(sA, col, half, av);
    if (32 * wave < cin) dw_tile_step(av, sB, c0 < cin ? c0 : cin - 1, half, acc0);
    if (32 * (wave + 4) < cin) dw_tile_step(av, sB, c1 < cin ? c1 : cin - 1, half, acc1);
    __syncthreads();
  }
  float* out = wa.L[li].part + (size_t)p * wsum;
  dw_tile_store(acc0, out, cout, cin, 32 * mt, c0, half);
  dw_tile_store(acc1, out, cout, cin, 32 * mt, c1, half);
}

static_assert(3 * kMaxDepth <= kMaxSumSegs, "the column sums of every layer in one launch");

struct Plan {
  int ntile, U, P, ncol, strips;
  size_t lds_data, lds_w;
  size_t plane, off_a, off_dz, off_col, off_w, wsum, bytes;      // offsets in floats
  bool ok;
};

Plan make_plan(int B, int in_size, int hidden, int out_size, int depth, int T) {
  Plan pl{};
  const int maxw = in_size > hidden ? in_size : hidden;
  pl.ok = depth >= 1 && depth <= kMaxDepth && in_size <= kMaxWidth && hidden <= kMaxWidth && out_size <= kMaxWidth;
  pl.lds_data = ((size_t)maxw * 33 + (size_t)(depth - 1) * hidden * 33 + 512 + (size_t)(depth - 1) * 32) * sizeof(float);
  pl.lds_w = ((size_t)32 * 33 + (size_t)maxw * 33) * sizeof(float);
  if (pl.lds_data > (size_t)kLdsMax) pl.ok = false;
  pl.ntile = (T + kFT - 1) / kFT;
  const long long U = (long long)B * pl.ntile;
  if (U > kMaxUnits) pl.ok = false;
  pl.U = (int)U;
  pl.P = nws_partial_count(U);
  pl.ncol = 3 * (depth - 1) * hidden + out_size;
  pl.plane = (size_t)B * hidden * T;
  pl.wsum = 0;
  pl.strips = 0;
  for (int i = 0; i < depth; ++i) {
    const int cin = i == 0 ? in_size : hidden, cout = i == depth - 1 ? out_size : hidden;
    pl.wsum += (size_t)cin * cout;
    pl.strips += (cout + 31) / 32;
  }
  pl.off_a = 0;
  pl.off_dz = pl.off_a + (size_t)(depth - 1) * pl.plane;
  pl.off_col = pl.off_dz + (size_t)(depth - 1) * pl.plane;
  pl.off_w = pl.off_col + (size_t)pl.U * pl.ncol;
  pl.bytes = (pl.off_w + (size_t)pl.P * pl.wsum) * sizeof(float);
  return pl;
}

}  // namespace

extern "C" size_t nws_td_mlp_grad_workspace_bytes(int B, int in_size, int hidden, int out_size, int depth, int T, int want_params) {
  if (!want_params || B < 1 || T < 1 || in_size < 1 || hidden < 1 || out_size < 1 || depth < 1 || depth > kMaxDepth) return 0;
  const Plan pl = make_plan(B, in_size, hidden, out_size, depth, T);
  return pl.ok ? pl.bytes : 0;
}

extern "C" int nws_td_mlp_grad(const float* x, const float* grad_y, int B, int in_size, int hidden, int out_size, int depth, int T,
                               const float* const* w, const float* const* b, const float* const* ln_g, const float* const* ln_b,
                               float ln_eps, float leaky_slope, float* grad_x, float* const* grad_w, float* const* grad_b,
                               float* const* grad_ln_g, float* const* grad_ln_b, void* workspace, size_t workspace_bytes,
                               void* stream) {
  if (!x || !grad_y || !grad_x || !w || !b || !ln_g || !ln_b || B <= 0 || T <= 0 || in_size <= 0 || hidden <= 0 || out_size <= 0)
    return NWS_ERR_BAD_ARG;
  if (depth < 1 || depth > kMaxDepth || B > 65535) return NWS_ERR_UNSUPPORTED;
  if ((grad_w == nullptr) != (grad_b == nullptr)) return NWS_ERR_BAD_ARG;
  const bool want = grad_w != nullptr;
  if (want && depth > 1 && (!grad_ln_g || !grad_ln_b)) return NWS_ERR_BAD_ARG;
  GradArgs a{};
  for (int i = 0; i < depth; ++i) {
    if (!w[i] || !b[i] || (want && (!grad_w[i] || !grad_b[i]))) return NWS_ERR_BAD_ARG;
    a.w[i] = w[i];
    a.b[i] = b[i];
    if (i < depth - 1) {
      if (!ln_g[i] || !ln_b[i] || (want && (!grad_ln_g[i] || !grad_ln_b[i]))) return NWS_ERR_BAD_ARG;
      a.ln_g[i] = ln_g[i];
      a.ln_b[i] = ln_b[i];
    }
  }
  const Plan pl = make_plan(B, in_size, hidden, out_size, depth, T);
  if (!pl.ok) return NWS_ERR_UNSUPPORTED;
  if (want && (!workspace || workspace_bytes < pl.bytes)) return NWS_ERR_BAD_ARG;
  static unsigned long long attr_devices = 0;
  if (nws_first_use_on_device(attr_devices)) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(td_mlp_grad_data_kernel),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, kLdsMax);
    if (e != hipSuccess) return (int)e;
  }
  hipStream_t st = (hipStream_t)stream;
  float* ws = static_cast<float*>(workspace);
  td_mlp_grad_data_kernel<<<dim3(pl.ntile, B), 256, pl.lds_data, st>>>(
      a, x, grad_y, in_size, hidden, out_size, depth, T, ln_eps, leaky_slope, grad_x, want ? ws + pl.off_a : nullptr,
      want ? ws + pl.off_dz : nullptr, want ? ws + pl.off_col : nullptr, pl.ncol);
  NWS_CHECK_LAUNCH();
  if (!want) return NWS_OK;

  WArgs wa{};
  SumSeg rw[kMaxDepth], rc[3 * kMaxDepth];
  size_t woff = 0;
  int strip = 0, nc = 0;
  for (int i = 0; i < depth; ++i) {
    const int cin = i == 0 ? in_size : hidden, cout = i == depth - 1 ? out_size : hidden;
    wa.L[i].dz = i == depth - 1 ? grad_y : ws + pl.off_dz + (size_t)i * pl.plane;
    wa.L[i].a = i == 0 ? x : ws + pl.off_a + (size_t)(i - 1) * pl.plane;
    wa.L[i].part = ws + pl.off_w + woff;           // partial p of every layer side by side: row p of [P][wsum]
    wa.L[i].cout = cout;
    wa.L[i].cin = cin;
    wa.L[i].strip0 = strip;
    rw[i] = SumSeg{grad_w[i], (long long)woff, cin * cout};
    strip += (cout + 31) / 32;
    woff += (size_t)cin * cout;
  }
  td_mlp_grad_weights_kernel<<<dim3(pl.strips, pl.P), 256, pl.lds_w, st>>>(wa, depth, T, pl.ntile, pl.U, (long long)pl.wsum);
  NWS_CHECK_LAUNCH();
  nws_segment_sums(ws + pl.off_w, pl.P, (long long)pl.wsum, rw, depth, st);
  NWS_CHECK_LAUNCH();
  // db, dbeta, dgamma: the column sums of all workgroups of the data kernel, one launch
  for (int i = 0; i < depth - 1; ++i) {
    rc[nc++] = SumSeg{grad_b[i], (long long)(3 * i) * hidden, hidden};
    rc[nc++] = SumSeg{grad_ln_b[i], (long long)(3 * i + 1) * hidden, hidden};
    rc[nc++] = SumSeg{grad_ln_g[i], (long long)(3 * i + 2) * hidden, hidden};
  }
  rc[nc++] = SumSeg{grad_b[depth - 1], (long long)3 * (depth - 1) * hidden, out_size};
  nws_segment_sums(ws + pl.off_col, pl.U, (long long)pl.ncol, rc, nc, st);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}
