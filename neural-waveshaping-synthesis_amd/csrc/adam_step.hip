// Gradient-norm clipping and Adam for every tensor of a model in two launches: the arithmetic of
// torch.nn.utils.clip_grad_norm_(max_norm, 2.0) followed by torch.optim.Adam (weight_decay 0, no amsgrad, no maximize).
//
//   total = sqrt(sum_k sum_i g_k[i]^2)                      float64 sums, rounded once to float32
//   c     = min(max_norm / (total + 1e-6), 1)               float32; max_norm = +inf gives exactly 1
//   gc    = c g
//   m'    = m + (1 - beta1)(gc - m)
//   v'    = beta2 v + (1 - beta2) gc^2
//   p'    = p - (lr / (1 - beta1^t)) m' / (sqrt(v') / sqrt(1 - beta2^t) + eps)
//
// Two kernels, no atomics, the backwards' contract (grad_sums.h): every output element is written by one thread and every sum
// runs in an order that depends on the tensor sizes only - equal inputs give equal bits.
//  * adam_sumsq_kernel: workgroup (chunk x, tensor y) adds the squares of one kChunk-element chunk of one gradient in float64
//    (each thread its four elements in turn, then a fixed tree over LDS) and writes ONE partial into the workspace slot
//    `slot0 of the tensor + x`, a function of the sizes.
//  * adam_update_kernel: every workgroup first adds ALL partials in float64 - thread j takes p = j, j + 256, ... in turn, then the
//    same tree - so every workgroup holds the same c to the bit; then it updates its own chunk.  Workgroup (0, 0) of the first
//    launch writes total.
// The tensor table is a kernel argument of at most kTable entries (as SumSegs is); more tensors take further launches of each
// kernel over the same workspace: all the sums first, then all the updates.  The gradients are read, never written.  Accesses are
// coalesced dwords: views into a flat state buffer are only 4-byte aligned.
#include "nws_common.h"

namespace {

constexpr int kChunk = NWS_ADAM_CHUNK;          // elements per workgroup
constexpr int kThreads = 256;
constexpr int kPer = kChunk / kThreads;
constexpr int kTable = NWS_ADAM_TABLE;
constexpr long long kMaxElems = 1ll << 40;      // a tensor; its chunks stay far inside a grid's x range
constexpr long long kMaxPartials = 1ll << 32;

struct SumEntry {
  const float* grad;
  long long n;
  long long slot0;      // the workspace slot of this tensor's first chunk
};
struct SumTable {
  SumEntry t[kTable];
};
struct AdamEntry {
  float* param;
  const float* grad;
  float* m;
  float* v;
  long long n;
};
struct AdamTable {
  AdamEntry t[kTable];
};
struct AdamScalars {
  float max_norm, one_minus_b1, beta2, one_minus_b2, step_size, bc2_sqrt, eps;
};

// the 256 threads' values in a fixed order: sums[j] += sums[j + s], s = 128, 64, .. 1; every thread returns the total
__device__ __forceinline__ double block_total(double s, double* sums, int tid) {
  sums[tid] = s;
  __syncthreads();
#pragma unroll
  for (int w = kThreads / 2; w >= 1; w >>= 1) {
    if (tid < w) sums[tid] += sums[tid + w];
    __syncthreads();
  }
  return sums[0];
}

__global__ __launch_bounds__(kThreads) void adam_sumsq_kernel(SumTable tb, double* __restrict__ part) {
  __shared__ double sums[kThreads];
  const SumEntry e = tb.t[blockIdx.y];
  const long long i0 = (long long)blockIdx.x * kChunk;
  if (i0 >= e.n) return;
  const int tid = threadIdx.x;
  double s = 0.0;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const long long i = i0 + tid + j * kThreads;
    if (i < e.n) {
      const double g = (double)e.grad[i];
      s += g * g;
    }
  }
  const double tot = block_total(s, sums, tid);
  if (tid == 0) part[e.slot0 + blockIdx.x] = tot;
}

__global__ __launch_bounds__(kThreads) void adam_update_kernel(AdamTable tb, const double* __restrict__ part, long long n_part,
                                                               AdamScalars sc, float* __restrict__ total_out) {
  __shared__ double sums[kThreads];
  const AdamEntry e = tb.t[blockIdx.y];
  const long long i0 = (long long)blockIdx.x * kChunk;
  if (i0 >= e.n) return;
  const int tid = threadIdx.x;
  double s = 0.0;
  for (long long p = tid; p < n_part; p += kThreads) s += part[p];
  const float total = (float)sqrt(block_total(s, sums, tid));
  const float r = sc.max_norm / (total + 1e-6f);
  const float c = r > 1.0f ? 1.0f : r;          // a NaN stays a NaN, as torch's clamp keeps it
  if (total_out != nullptr && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0) *total_out = total;
#pragma unroll
  for (int j = 0; j < kPer; ++j) {
    const long long i = i0 + tid + j * kThreads;
    if (i < e.n) {
      const float g = c * e.grad[i];
      const float m0 = e.m[i];
      const float m1 = m0 + sc.one_minus_b1 * (g - m0);
      const float v1 = sc.beta2 * e.v[i] + sc.one_minus_b2 * (g * g);
      const float denom = sqrtf(v1) / sc.bc2_sqrt + sc.eps;
      e.m[i] = m1;
      e.v[i] = v1;
      e.param[i] = e.param[i] - sc.step_size * (m1 / denom);
    }
  }
}

// the number of partials of the n tensors (one per chunk, tensors in call order), or -1 for what is refused / -2 for what is not
// served; every record is checked here, before anything is launched
long long plan_partials(const NwsAdamTensor* tensors, int n, bool pointers) {
  if (tensors == nullptr || n < 1) return -1;
  long long total = 0;
  for (int k = 0; k < n; ++k) {
    const NwsAdamTensor& t = tensors[k];
    if (t.n < 1) return -1;
    if (pointers && (!t.param || !t.grad || !t.exp_avg || !t.exp_avg_sq)) return -1;
    if (t.n > kMaxElems) return -2;
    total += (t.n + kChunk - 1) / kChunk;
    if (total > kMaxPartials) return -2;
  }
  return total;
}

}  // namespace

extern "C" size_t nws_adam_workspace_bytes(const NwsAdamTensor* tensors, int n) {
  const long long parts = plan_partials(tensors, n, false);
  return parts > 0 ? (size_t)parts * sizeof(double) : 0;
}

extern "C" int nws_adam_step(const NwsAdamTensor* tensors, int n, long long step, double lr, double beta1, double beta2, double eps,
                             double max_norm, float* total_norm, void* workspace, size_t workspace_bytes, void* stream) {
  if (step < 1 || total_norm == nullptr) return NWS_ERR_BAD_ARG;
  const long long parts = plan_partials(tensors, n, true);
  if (parts == -2) return NWS_ERR_UNSUPPORTED;
  if (parts < 1) return NWS_ERR_BAD_ARG;
  if (workspace == nullptr || (reinterpret_cast<uintptr_t>(workspace) & 7) != 0 || workspace_bytes < (size_t)parts * sizeof(double))
    return NWS_ERR_BAD_ARG;
  hipStream_t st = (hipStream_t)stream;
  double* part = static_cast<double*>(workspace);
  // the bias corrections in float64 on the host, each factor rounded once
  const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
  AdamScalars sc;
  sc.max_norm = (float)max_norm;
  sc.one_minus_b1 = (float)(1.0 - beta1);
  sc.beta2 = (float)beta2;
  sc.one_minus_b2 = (float)(1.0 - beta2);
  sc.step_size = (float)(lr / bc1);
  sc.bc2_sqrt = (float)sqrt(bc2);
  sc.eps = (float)eps;
  long long slot = 0;
  for (int k0 = 0; k0 < n; k0 += kTable) {
    const int cnt = n - k0 < kTable ? n - k0 : kTable;
    SumTable tb{};
    long long maxc = 0;
    for (int k = 0; k < cnt; ++k) {
      const long long c = (tensors[k0 + k].n + kChunk - 1) / kChunk;
      tb.t[k] = SumEntry{tensors[k0 + k].grad, tensors[k0 + k].n, slot};
      slot += c;
      if (c > maxc) maxc = c;
    }
    adam_sumsq_kernel<<<dim3((unsigned)maxc, cnt), kThreads, 0, st>>>(tb, part);
    NWS_CHECK_LAUNCH();
  }
  for (int k0 = 0; k0 < n; k0 += kTable) {
    const int cnt = n - k0 < kTable ? n - k0 : kTable;
    AdamTable tb{};
    long long maxc = 0;
    for (int k = 0; k < cnt; ++k) {
      const NwsAdamTensor& t = tensors[k0 + k];
      const long long c = (t.n + kChunk - 1) / kChunk;
      tb.t[k] = AdamEntry{t.param, t.grad, t.exp_avg, t.exp_avg_sq, t.n};
      if (c > maxc) maxc = c;
    }
    adam_update_kernel<<<dim3((unsigned)maxc, cnt), kThreads, 0, st>>>(tb, part, parts, sc, k0 == 0 ? total_norm : nullptr);
    NWS_CHECK_LAUNCH();
  }
  return NWS_OK;
}
