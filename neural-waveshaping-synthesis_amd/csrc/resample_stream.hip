// Streaming sample-rate converter: the converter of resample.hip on chunks, with the state carried between calls.
//   DESIGN.md 3.23 holds the definition (tests/resample_stream_restatement.py restates it in float64); symbols as in 3.10.
//
// A stream keeps per row two 64-bit counters (n_seen: input samples consumed, t_next: outputs emitted) and the last
// taps - 1 input samples.  Output t, with n = floor(t M / L) and r = (t M) mod L, is row r of the weight bank of
// nws_resample_bank against x[n - left + 1 .. n + right], x = everything pushed so far, zero before sample 0.  It leaves once
// x[n + right] has been pushed: after n_seen samples E(n_seen) = ceil((n_seen - right) L / M) outputs have left (0 up to
// n_seen = right).  A final step treats x as zero beyond its end and emits up to the offline length (n_seen L) / M.
//
// resample_stream_kernel: one launch per step, one workgroup per row.  The workgroup reads its row's counters, stages
// [taps - 1 samples of history | n new samples | `right` zeros on a final step] in LDS, computes outputs t_next .. E - 1,
// and behind a barrier writes the last taps - 1 staged samples back as the new history and advances the counters.  Nothing
// outside the workgroup touches the row's state: no atomics, no second launch; every read of the old history goes through
// the LDS copy, so the write-back cannot race it.
// SIXTEEN LANES PER OUTPUT: lane l of a group sums taps l, l + 16, l + 32, ... in that order on one chain of FMAs - the weight
// row is read from the bank in 64-byte runs, the window from 16 consecutive LDS words - and the sixteen partial sums meet in a
// butterfly (partner l ^ 8, then ^ 4, ^ 2, ^ 1; every lane ends with the same bits because fp32 addition commutes).  The order
// of summation is a function of `taps` alone, hence of (sr_in, sr_out): never of the chunk size, of B, of the output's place in
// the chunk or of the row.  Taps that fall on the zero history or the zero extension multiply a real 0.0f from LDS.
//
// Limits: B <= 65 535; taps - 1 + n + right floats within 64 KB of LDS (kLdsFloats; no launch attribute needed),
// which bounds a step's n by nws_resample_stream_max_chunk; (kLdsFloats + 2) L + M below 2^31 (32-bit phase arithmetic inside a step).
#include "nws_common.h"

namespace {

constexpr int kThreads = 1024, kGroup = 16, kGroups = kThreads / kGroup;
constexpr int kOutputs = 4, kTaps = 8;     // outputs a group takes at once, taps of each a lane loads at once
constexpr int kLdsFloats = 64 * 1024 / 4;

struct StreamDims {
  int L, M, taps, left, right;
  int hist;        // taps - 1
  int max_chunk;   // most new samples of one step
};

__host__ bool stream_dims(int sr_in, int sr_out, StreamDims* d) {
  int32_t v[6];
  if (nws_resample_dims(sr_in, sr_out, v) != NWS_OK) return false;
  d->L = v[0], d->M = v[1], d->taps = v[2], d->left = v[3], d->right = v[4];
  d->hist = d->taps - 1;
  d->max_chunk = kLdsFloats - d->hist - d->right;
  if (d->max_chunk < 1) return false;
  if (((long long)kLdsFloats + 2) * d->L + d->M > 0x7fffffffLL) return false;
  return true;
}

__host__ size_t state_bytes(int B, const StreamDims& d) {
  const size_t raw = (size_t)B * (2 * sizeof(long long) + (size_t)d.hist * sizeof(float));
  return (raw + 15) / 16 * 16;
}

// outputs emitted in all after n_seen samples; with `final` the offline length
__host__ __device__ __forceinline__ long long emitted(long long n_seen, int L, int M, int right, int final) {
  if (final) return (n_seen * L) / M;
  return n_seen <= right ? 0 : ((n_seen - right) * L + M - 1) / M;
}

// most outputs one step of n samples can emit, whatever the stream has seen
__host__ long long max_out(long long n, const StreamDims& d, int final) {
  return final ? ((n + d.right) * d.L) / d.M : (n * d.L + d.M - 1) / d.M;
}

struct StreamGeom {
  int L, M, taps, right, hist;
  int B, n, final, max_out, y_stride;
};

__global__ __launch_bounds__(kThreads) void resample_stream_kernel(unsigned char* __restrict__ state, const float* __restrict__ x,
                                                                   const float* __restrict__ bank, StreamGeom k,
                                                                   float* __restrict__ y) {
  extern __shared__ float xs[];      // xs[a] = x[n_seen - hist + a]
  const int tid = threadIdx.x, row = blockIdx.x;
  long long* cnt = reinterpret_cast<long long*>(state) + 2 * (size_t)row;
  float* hist = reinterpret_cast<float*>(state + (size_t)k.B * 2 * sizeof(long long)) + (size_t)row * k.hist;
  const long long n_seen = cnt[0], t_next = cnt[1];
  const int live = k.hist + k.n, total = live + (k.final ? k.right : 0);
  const float* xr = x + (size_t)row * k.n;
  for (int a = tid; a < total; a += kThreads) xs[a] = a < k.hist ? hist[a] : (a < live ? xr[a - k.hist] : 0.0f);
  // the step's outputs: t_next .. t_end - 1.  A state that nws_resample_stream_reset did not write cannot take the stores
  // past the row of y or the reads past the staged samples: the count is clamped and every window checked
  const long long t_end = emitted(n_seen + k.n, k.L, k.M, k.right, k.final);
  const long long want = t_end - t_next;
  const long long tm = t_next * k.M, q0 = tm / k.L;
  const long long a_long = q0 - n_seen + k.right;       // staged word of the first tap of output t_next
  const bool sane = n_seen >= 0 && t_next >= 0 && a_long >= 0 && a_long <= total;
  const int count = (int)(want < 0 || !sane ? 0 : (want > k.max_out ? k.max_out : want));
  const int a_first = sane ? (int)a_long : 0;
  const unsigned r0 = (unsigned)(tm - q0 * k.L);
  const int lane = tid & (kGroup - 1);
  float* yr = y + (size_t)row * k.y_stride;
  __syncthreads();
  // a group takes kOutputs outputs a turn (i, i + kGroups, ...) and kTaps taps of each per lane at a time, so that
  // kOutputs kTaps weight loads are in flight together.  A lane's taps past the row's end weigh 0.0f against 0.0f.
  for (int i0 = tid / kGroup; i0 < count; i0 += kGroups * kOutputs) {
    const float* w[kOutputs];
    const float* xw[kOutputs];
    bool ok[kOutputs];
    float acc[kOutputs];
#pragma unroll
    for (int u = 0; u < kOutputs; ++u) {
      const int i = i0 + u * kGroups;
      const unsigned v = r0 + (unsigned)i * (unsigned)k.M, dq = v / (unsigned)k.L, r = v - dq * (unsigned)k.L;
      const int a0 = a_first + (int)dq;
      ok[u] = i < count && a0 >= 0 && a0 + k.taps <= total;
      w[u] = bank + (ok[u] ? (size_t)r * k.taps : 0);        // (an output that is not computed reads row 0 against word 0)
      xw[u] = xs + (ok[u] ? a0 : 0);
      acc[u] = 0.0f;
    }
    for (int c0 = lane; c0 < k.taps; c0 += kGroup * kTaps) {
      float wv[kOutputs][kTaps], xv[kOutputs][kTaps];
#pragma unroll
      for (int j = 0; j < kTaps; ++j) {
        const int c = c0 + j * kGroup, cc = min(c, k.taps - 1);
#pragma unroll
        for (int u = 0; u < kOutputs; ++u) {
          const float wl = w[u][cc], xl = xw[u][cc];
          wv[u][j] = c < k.taps ? wl : 0.0f;
          xv[u][j] = c < k.taps ? xl : 0.0f;
        }
      }
#pragma unroll
      for (int j = 0; j < kTaps; ++j) {
#pragma unroll
        for (int u = 0; u < kOutputs; ++u) acc[u] = fmaf(wv[u][j], xv[u][j], acc[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < kOutputs; ++u) {
#pragma unroll
      for (int m = kGroup / 2; m >= 1; m >>= 1) acc[u] = nws_add_scalar(acc[u], __shfl_xor(acc[u], m, kGroup));
      if (lane == 0 && ok[u]) yr[i0 + u * kGroups] = acc[u];
    }
  }
  __syncthreads();      // behind the last read of the staged history
  for (int a = tid; a < k.hist; a += kThreads) hist[a] = xs[k.n + a];
  if (tid == 0) {
    cnt[0] = n_seen + k.n;
    cnt[1] = t_next + count;
  }
}

}  // namespace

extern "C" {

size_t nws_resample_stream_state_bytes(int B, int sr_in, int sr_out) {
  StreamDims d;
  if (B < 1 || B > 65535 || !stream_dims(sr_in, sr_out, &d)) return 0;
  return state_bytes(B, d);
}

int nws_resample_stream_max_chunk(int sr_in, int sr_out) {
  StreamDims d;
  return stream_dims(sr_in, sr_out, &d) ? d.max_chunk : 0;
}

int nws_resample_stream_reset(void* state, size_t bytes, int B, int sr_in, int sr_out, void* stream) {
  StreamDims d;
  if (!state || B < 1) return NWS_ERR_BAD_ARG;
  if (B > 65535 || !stream_dims(sr_in, sr_out, &d)) return NWS_ERR_UNSUPPORTED;
  const size_t need = state_bytes(B, d);
  if (bytes < need) return NWS_ERR_BAD_ARG;
  const hipError_t e = hipMemsetAsync(state, 0, need, (hipStream_t)stream);
  return e == hipSuccess ? NWS_OK : (int)e;
}

int64_t nws_resample_stream_emitted(int64_t n_seen, int sr_in, int sr_out, int final) {
  StreamDims d;
  if (n_seen < 0 || !stream_dims(sr_in, sr_out, &d) || n_seen > (INT64_MAX - d.M) / d.L) return -1;
  return (int64_t)emitted(n_seen, d.L, d.M, d.right, final ? 1 : 0);
}

int nws_resample_stream_max_out(int n, int sr_in, int sr_out, int final) {
  StreamDims d;
  if (n < 0 || !stream_dims(sr_in, sr_out, &d)) return -1;
  const long long m = max_out(n, d, final ? 1 : 0);
  return m > 0x7fffffffLL ? -1 : (int)m;
}

int nws_resample_stream_step(void* state, size_t bytes, const float* x, int B, int n, int sr_in, int sr_out, const float* bank_dev,
                             int final, float* y, int y_stride, void* stream) {
  StreamDims d;
  if (!state || !bank_dev || !y || B < 1 || n < 0 || (n == 0 && !final) || (n > 0 && !x)) return NWS_ERR_BAD_ARG;
  if (B > 65535 || !stream_dims(sr_in, sr_out, &d) || n > d.max_chunk) return NWS_ERR_UNSUPPORTED;
  const long long m = max_out(n, d, final ? 1 : 0);       // (kLdsFloats L) / M + 1 at the most: an int by stream_dims
  if (y_stride < m || bytes < state_bytes(B, d)) return NWS_ERR_BAD_ARG;
  const StreamGeom k{d.L, d.M, d.taps, d.right, d.hist, B, n, final ? 1 : 0, (int)m, y_stride};
  const size_t lds = (size_t)(d.hist + n + (final ? d.right : 0)) * sizeof(float);
  resample_stream_kernel<<<(unsigned)B, kThreads, lds, (hipStream_t)stream>>>(static_cast<unsigned char*>(state), x, bank_dev, k, y);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

}  // extern "C"
