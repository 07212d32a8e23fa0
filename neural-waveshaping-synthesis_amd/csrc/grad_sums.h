// The sums over partials and the dW contraction step that the parameter gradients share (td_mlp_grad.hip, control_gru_grad.hip,
// newt_grad.hip), DESIGN.md 3.16.  Both carry the backwards' contract: every output element is written by one thread and every
// sum runs in an order that depends on the sizes only, no atomics - equal inputs give equal bits.
//  * nws_segment_sum_kernel / nws_segment_sums: out[e] = sum_p part[p][e] in float64 in a fixed order (eight interleaved
//    sequential sums, then those eight in order), rounded once; a table of (destination, offset, length) segments of a partial
//    row is the kernel argument, one launch per block of partials.
//  * dW[i][k] = sum over frames of A[i][frame] B[k][frame], a contraction over the B T frames on the fp32 matrix pipe
//    (v_mfma_f32_32x32x2_f32, exact fp32 products): the (utterance, 32-frame chunk) list of U units is split into
//    P = nws_partial_count(U) ranges (nws_unit_range); a workgroup walks its range - stage sA [32][33] and sB [cin][33], barrier,
//    request the next unit, products, barrier - where dw_read16 / dw_tile_step are the products of one accumulator tile and
//    dw_tile_store writes it into partial p.  What is fetched, how it is staged, and the loop itself are each kernel's: with
//    the loop as a function template over fetch / stage / products callables the compiler kept 198 VGPRs for
//    td_mlp_grad_weights_kernel where the loop written out takes 170 (one closure besides the fetch is enough for that).
#pragma once
#include "nws_common.h"

namespace {

constexpr int kMaxSumSegs = 24;                 // the largest table: three column sums for each of the frame MLP's 8 layers
constexpr long long kMaxUnits = 1ll << 30;      // the unit list, and every index into it, stays inside int

struct SumSeg {
  float* dst;
  long long off;      // first element of the segment inside a partial row
  int n;
};
struct SumSegs {
  SumSeg s[kMaxSumSegs];
};

// dst[e] = sum_p part[p * stride + off + e] in float64: thread (e, j) adds p = j, j + 8, ... in turn, then j = 0 .. 7 in order
__global__ __launch_bounds__(256) void nws_segment_sum_kernel(const float* __restrict__ part, int P, long long stride, SumSegs ra) {
  __shared__ double sums[8][32];
  const SumSeg sg = ra.s[blockIdx.y];
  if ((int)blockIdx.x * 32 >= sg.n) return;
  const int e = blockIdx.x * 32 + (threadIdx.x & 31), j = threadIdx.x >> 5;
  double s = 0.0;
  if (e < sg.n)
    for (int p = j; p < P; p += 8) s += (double)part[(size_t)p * stride + sg.off + e];
  sums[j][threadIdx.x & 31] = s;
  __syncthreads();
  if (j == 0 && e < sg.n) {
    double tot = 0.0;
    for (int q = 0; q < 8; ++q) tot += sums[q][threadIdx.x & 31];
    sg.dst[e] = (float)tot;
  }
}

// one launch: the nseg <= kMaxSumSegs segments of the P partial rows `stride` floats apart; the caller checks the launch
inline void nws_segment_sums(const float* part, int P, long long stride, const SumSeg* segs, int nseg, hipStream_t st) {
  SumSegs ra{};
  int maxn = 0;
  for (int i = 0; i < nseg; ++i) {
    ra.s[i] = segs[i];
    if (segs[i].n > maxn) maxn = segs[i].n;
  }
  nws_segment_sum_kernel<<<dim3((maxn + 31) / 32, nseg), 256, 0, st>>>(part, P, stride, ra);
}

// the number of dW partials for U <= kMaxUnits units: a function of (B, T) only - about eight units each, at most 32
inline int nws_partial_count(long long U) {
  const long long p = (U + 7) / 8;
  return (int)(p < 32 ? p : 32);
}

struct UnitRange {
  int u0, u1;
};

// the units [u0, u1) of range p of P
__device__ __forceinline__ UnitRange nws_unit_range(int p, int P, int U) {
  return UnitRange{(int)((long long)p * U / P), (int)((long long)(p + 1) * U / P)};
}

// lane (col, half) of a 32x32x2 product: its 16 operands from row `row` of a staged [rows][33] tile, frames 16 half + [0, 16)
__device__ __forceinline__ void dw_read16(const float* tile, int row, int half, float (&v)[16]) {
#pragma unroll
  for (int s2 = 0; s2 < 16; ++s2) v[s2] = tile[row * 33 + 16 * half + s2];
}

// acc[i][k] += sum over the 32 staged frames of A[i][frame] B[k][frame]: av = this lane's row of sA, `row` its row of sB
__device__ __forceinline__ void dw_tile_step(const float (&av)[16], const float* sB, int row, int half, f32x16& acc) {
  float bv[16];
  dw_read16(sB, row, half, bv);
#pragma unroll
  for (int s2 = 0; s2 < 16; ++s2) acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s2], bv[s2], acc, 0, 0, 0);
}

// the accumulator tile of lane (c - its column, half) into a row-major (rows, cols) matrix, tile rows row0 .. row0 + 31
__device__ __forceinline__ void dw_tile_store(const f32x16& acc, float* out, int rows, int cols, int row0, int c, int half) {
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int o = row0 + nws_frag_row(r, half);
    if (o < rows && c < cols) out[(size_t)o * cols + c] = acc[r];
  }
}

}  // namespace
