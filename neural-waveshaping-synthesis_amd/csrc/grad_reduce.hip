// Data-parallel training: the gradients of W ranks averaged in rank order.  The exchange between the ranks moves
// data only (an all-gather of one row per rank); the sum is formed here, in an order fixed by the sizes, so every rank holds the
// same bits whatever library carried the rows, and a W-rank run equals a one-process emulation of it to the bit.
//
//   pack:    dst[off_k + i] = src_k[i]                                  off_k = sum of the sizes of the tensors in front of k
//   reduce:  out[i] = (float)((sum_{r = 0 .. W-1} (double)rows[r stride + i]) / (double)W)
//
// The sum runs in float64 in ascending r, is divided once in float64 and rounded once to float32: IEEE operations throughout, so
// a float64 restatement on the host gives the same bits (tests/grad_reduce_restatement.py).  W = 1 is a copy of the row.
// Two kernels, no atomics, the backwards' contract (grad_sums.h): every output element is written by one thread.
//  * grad_pack_kernel: the tensor table is a kernel argument of at most kTable entries, as in adam_sumsq_kernel; workgroup
//    (chunk x, tensor y) copies one kChunk-element chunk of one tensor; more tensors take further launches.
//  * grad_reduce_kernel: thread per element, each of a workgroup's 256 threads its four elements in turn.
// Accesses are coalesced dwords: views into a flat buffer are only 4-byte aligned.
#include "nws_common.h"

namespace {

constexpr int kChunk = NWS_ADAM_CHUNK;          // elements per workgroup
constexpr int kThreads = 256;
constexpr int kPer = kChunk / kThreads;
constexpr int kTable = NWS_ADAM_TABLE;
constexpr unsigned long long kMaxElems = 1ull << 40;      // a tensor or a row; its chunks stay far inside a grid's x range
constexpr int kMaxWorld = NWS_GRAD_MAX_WORLD;

struct PackEntry {
  const float* src;
  float* dst;
  long long n;
};
struct PackTable {
  PackEntry t[kTable];
};

__global__ __launch_bounds__(kThreads) void grad_pack_kernel(PackTable tb) {
  const PackEntry e = tb.t[blockIdx.y];
  const long long i0 = (long long)blockIdx.x * kChunk;
  if (i0 >= e.n) return;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const long long i = i0 + threadIdx.x + j * kThreads;
    if (i < e.n) e.dst[i] = e.src[i];
  }
}

__global__ __launch_bounds__(kThreads) void grad_reduce_kernel(const float* __restrict__ rows, int world, long long n,
                                                               long long row_stride, float* __restrict__ out) {
  const long long i0 = (long long)blockIdx.x * kChunk;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const long long i = i0 + threadIdx.x + j * kThreads;
    if (i >= n) continue;
    if (world == 1) {         // the row's own bits, a NaN's payload included
      out[i] = rows[i];
      continue;
    }
    double s = 0.0;
    for (int r = 0; r < world; ++r) s += (double)rows[r * row_stride + i];
    out[i] = (float)(s / (double)world);
  }
}

}  // namespace

extern "C" int nws_grad_pack(const NwsGradTensor* tensors, int n, float* dst, size_t dst_elems, void* stream) {
  if (tensors == nullptr || n < 1 || dst == nullptr) return NWS_ERR_BAD_ARG;
  unsigned long long total = 0;
  bool too_large = false;
  for (int k = 0; k < n; ++k) {
    if (tensors[k].src == nullptr || tensors[k].n < 1) return NWS_ERR_BAD_ARG;
    if (tensors[k].n > kMaxElems) too_large = true;
    else total += tensors[k].n;         // n * 2^40 < 2^64: no wrap
  }
  if (too_large) return NWS_ERR_UNSUPPORTED;
  if (dst_elems < total) return NWS_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  size_t off = 0;
  for (int k0 = 0; k0 < n; k0 += kTable) {
    const int cnt = n - k0 < kTable ? n - k0 : kTable;
    PackTable tb{};
    long long maxc = 0;
    for (int k = 0; k < cnt; ++k) {
      const long long len = (long long)tensors[k0 + k].n;
      const long long c = (len + kChunk - 1) / kChunk;
      tb.t[k] = PackEntry{tensors[k0 + k].src, dst + off, len};
      off += (size_t)len;
      if (c > maxc) maxc = c;
    }
    grad_pack_kernel<<<dim3((unsigned)maxc, cnt), kThreads, 0, st>>>(tb);
    NWS_CHECK_LAUNCH();
  }
  return NWS_OK;
}

extern "C" int nws_grad_reduce(const float* rows, int world, size_t n, size_t row_stride, float* out, void* stream) {
  if (rows == nullptr || out == nullptr || world < 1 || n < 1 || row_stride < n) return NWS_ERR_BAD_ARG;
  if (world > kMaxWorld || row_stride > kMaxElems) return NWS_ERR_UNSUPPORTED;
  // out may not lie in (or reach into) the rows: another thread's addend would be somebody's result
  const uintptr_t r0 = reinterpret_cast<uintptr_t>(rows), r1 = r0 + (uintptr_t)world * row_stride * sizeof(float);
  const uintptr_t o0 = reinterpret_cast<uintptr_t>(out), o1 = o0 + n * sizeof(float);
  if (o0 < r1 && r0 < o1) return NWS_ERR_BAD_ARG;
  const unsigned blocks = (unsigned)((n + kChunk - 1) / kChunk);
  grad_reduce_kernel<<<dim3(blocks), kThreads, 0, (hipStream_t)stream>>>(rows, world, (long long)n, (long long)row_stride, out);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}
