// MFCC feature, the last analysis feature of the reference's control files:
//   neural_waveshaping_synthesis/data/utils/mfcc_extraction.py:7-13 (extract_mfcc -> librosa.feature.mfcc with librosa 0.8.0's
//   defaults): power STFT -> Slaney mel filter bank -> power_to_db(ref 1, amin 1e-10, top_db 80) -> orthonormal DCT-II.
//   DESIGN.md 3.11 holds the definition the kernels are tested against; parity with librosa itself is unpinned.
//
// Three passes on one stream:
//   1. the loudness feature's power pass (loudness.hip: the windowed-DFT GEMM on v_mfma_f32_32x32x2_f32), power kept as
//      (B, bins, frames_pad) - the same kernel, the same DFT operand, nothing of the STFT is written twice;
//   2. mfcc_mel_kernel: the mel matrix is sparse (a bin feeds at most two filters), so it runs on the vector pipe and not
//      as a dense GEMM.  LANES RUN OVER FRAMES (power is contiguous along frames); a filter is a (first bin, count) span
//      whose weights are the same for the whole wave - scalar loads, as in resample.hip.  One chain of FMAs per filter in bin
//      order.  Leaves the per-utterance maximum of the mel power in one word (atomicMax on the float bits: mel power is
//      non-negative and log is monotone, so the maximum of the dB values is the dB value of that maximum);
//   3. mfcc_dct_kernel: lanes over frames, a loop over the mel bands: dB, clip, then sixteen DCT accumulators in registers
//      with the DCT row entries as wave-uniform scalars (blockIdx.y picks the sixteen).  The accumulators are fp64 (fp32
//      entries, fp32 dB values, exact products): a chain of 128 fp32 additions towards |c[0]| ~ 1000 was the largest error of
//      the feature, and the pass is a few per cent of the power pass either way.
// The order of every sum is a function of the configuration alone: a row of a batch equals its own B = 1 result bit for bit.
//
// The DCT is taken of db - max_db (in [-top_db, 0]) and sqrt(n_mels) max_db is added to coefficient 0: the rows j >= 1 of the
// DCT matrix sum to zero, so this is the same number in exact arithmetic, and in fp32 it keeps the rounding of the matrix
// entries from being multiplied by the utterance's level (an all-zero utterance gives exact zeros for j >= 1).
//
// Limits (NWS_ERR_UNSUPPORTED): n_fft / hop as nws_loudness; 1 <= n_mfcc <= n_mels <= 1024; sample_rate > 0; B <= 65535.
#include <math.h>

#include <vector>

#include "nws_common.h"

namespace {

constexpr int kMaxMels = 1024;
constexpr int kJ = 16;                  // DCT coefficients per workgroup of pass 3
constexpr float kAmin = 1e-10f, kAminDb = -100.0f, kTopDb = 80.0f;

struct MfccDims {
  int bins, n_mels, n_mfcc, jpad, nnz, off_w, off_dct, words;
};

struct MfccTable {          // the filter bank of (sample_rate, n_fft, n_mels); n_mfcc only sizes the DCT part of the table
  double sr = 0.0;
  int n_fft = 0, n_mels = 0;
  std::vector<int> first, count;
  std::vector<double> weights;           // the non-zero span of every filter, one after the other
};

__host__ double hz_to_mel(double f) {    // Slaney: linear below 1 kHz, logarithmic above
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return f >= min_log_hz ? min_log_mel + log(f / min_log_hz) / logstep : f / f_sp;
}

__host__ double mel_to_hz(double m) {
  const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = log(6.4) / 27.0;
  return m >= min_log_mel ? min_log_hz * exp(logstep * (m - min_log_mel)) : f_sp * m;
}

// numpy.linspace(a, b, n)[i]
__host__ double linspace_at(double a, double b, int n, int i) {
  if (n < 2) return a;
  return i == n - 1 ? b : a + (double)i * ((b - a) / (double)(n - 1));
}

__host__ bool mfcc_config_ok(double sr, int n_fft, int n_mfcc, int n_mels) {
  return sr > 0.0 && sr <= 1.0e9 && nws_loudness_dft_bytes(n_fft) != 0 && n_mels >= 1 && n_mels <= kMaxMels && n_mfcc >= 1 &&
         n_mfcc <= n_mels;
}

// the filter bank of a configuration in fp64 (spans of non-zero weights); the launcher asks for the same one call after call
__host__ const MfccTable* mfcc_table(double sr, int n_fft, int n_mfcc, int n_mels) {
  if (!mfcc_config_ok(sr, n_fft, n_mfcc, n_mels)) return nullptr;
  static thread_local MfccTable c;
  if (c.sr == sr && c.n_fft == n_fft && c.n_mels == n_mels) return &c;
  const int bins = n_fft / 2 + 1;
  std::vector<double> mel_f(n_mels + 2);
  const double m_lo = hz_to_mel(0.0), m_hi = hz_to_mel(0.5 * sr);
  for (int i = 0; i < n_mels + 2; ++i) mel_f[i] = mel_to_hz(linspace_at(m_lo, m_hi, n_mels + 2, i));
  c.first.assign(n_mels, 0);
  c.count.assign(n_mels, 0);
  c.weights.clear();
  for (int i = 0; i < n_mels; ++i) {
    const double lo = mel_f[i], mid = mel_f[i + 1], hi = mel_f[i + 2], norm = 2.0 / (hi - lo);
    int first = -1, last = -2;
    for (int k = 0; k < bins; ++k) {
      const double f = linspace_at(0.0, 0.5 * sr, bins, k);
      const double w = fmin((f - lo) / (mid - lo), (hi - f) / (hi - mid));
      if (w > 0.0) {
        if (first < 0) first = k;
        last = k;
      }
    }
    c.first[i] = first < 0 ? 0 : first;
    c.count[i] = first < 0 ? 0 : last - first + 1;
    for (int k = first; first >= 0 && k <= last; ++k) {
      const double f = linspace_at(0.0, 0.5 * sr, bins, k);
      const double w = fmin((f - lo) / (mid - lo), (hi - f) / (hi - mid));
      c.weights.push_back((w > 0.0 ? w : 0.0) * norm);
    }
  }
  c.sr = sr, c.n_fft = n_fft, c.n_mels = n_mels;
  return &c;
}

__host__ MfccDims mfcc_dims(const MfccTable& c, int n_mfcc) {
  MfccDims d;
  d.bins = c.n_fft / 2 + 1;
  d.n_mels = c.n_mels;
  d.n_mfcc = n_mfcc;
  d.jpad = (n_mfcc + kJ - 1) / kJ * kJ;
  d.nnz = (int)c.weights.size();
  d.off_w = 3 * c.n_mels;
  d.off_dct = d.off_w + d.nnz;
  d.words = d.off_dct + c.n_mels * d.jpad;
  return d;
}

__device__ __forceinline__ float power_db(float p) { return p > kAmin ? 10.0f * log10f(p) : kAminDb; }

// grid (frame tiles of 64, B); wave w of a workgroup sums filters w, w + 4, ... (their spans grow with the index)
__global__ __launch_bounds__(256) void mfcc_mel_kernel(const float* __restrict__ power, const float* __restrict__ table, int bins,
                                                       int n_mels, int off_w, int nnz, int frames, int frames_pad,
                                                       float* __restrict__ mel, unsigned* __restrict__ mel_max) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int t = blockIdx.x * 64 + lane, b = blockIdx.y;
  const bool live = t < frames;
  const int* spans = reinterpret_cast<const int*>(table);
  const float* weights = table + off_w;
  const float* P = power + (size_t)b * bins * frames_pad + (live ? t : frames - 1);   // a lane beyond the end re-reads the last frame
  float mx = 0.0f;
  for (int i = wave; i < n_mels; i += 4) {
    // a table is accepted by its size: a span that does not fit THIS configuration's bins or weights (a table of another
    // configuration with the same word count) is cut, so that whatever the table holds no read leaves power or the table
    const int first = min(max(spans[3 * i], 0), bins), off = spans[3 * i + 2];
    int count = min(max(spans[3 * i + 1], 0), bins - first);
    if (off < 0 || off > nnz - count) count = 0;
    const float* w = weights + (count ? off : 0);
    const float* p = P + (size_t)first * frames_pad;
    float a = 0.0f;
#pragma unroll 4
    for (int k = 0; k < count; ++k) a = fmaf(w[k], p[(size_t)k * frames_pad], a);
    if (live) {
      mel[((size_t)b * n_mels + i) * frames_pad + t] = a;
      mx = fmaxf(mx, a);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (lane == 0) atomicMax(&mel_max[b], __float_as_uint(mx));
}

// grid (frame tiles of 256, groups of kJ coefficients, B); dct: (n_mels, jpad), column j scaled by s_j, zero beyond n_mfcc
__global__ __launch_bounds__(256) void mfcc_dct_kernel(const float* __restrict__ mel, const unsigned* __restrict__ mel_max,
                                                       const float* __restrict__ dct, int n_mels, int n_mfcc, int jpad, int frames,
                                                       int frames_pad, double sqrt_mels, float* __restrict__ out) {
  const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.z;
  const int j0 = blockIdx.y * kJ;
  if (t >= frames) return;
  const float max_db = power_db(__uint_as_float(mel_max[b]));
  const float* x = mel + (size_t)b * n_mels * frames_pad + t;
  const float* row = dct + j0;
  double acc[kJ];      // fp64: 128 fp32 roundings on the way to |c[0]| ~ 1000 would be the largest error of the whole feature
#pragma unroll
  for (int j = 0; j < kJ; ++j) acc[j] = 0.0;
  for (int m = 0; m < n_mels; ++m) {
    const double d = (double)fmaxf(power_db(x[(size_t)m * frames_pad]) - max_db, -kTopDb);
#pragma unroll
    for (int j = 0; j < kJ; ++j) acc[j] = __builtin_fma((double)row[j], d, acc[j]);
    row += jpad;
  }
#pragma unroll
  for (int j = 0; j < kJ; ++j) {
    if (j0 + j < n_mfcc) {
      const double v = j0 + j == 0 ? acc[j] + sqrt_mels * (double)max_db : acc[j];      // s_0 n_mels max_db
      out[((size_t)b * n_mfcc + j0 + j) * frames + t] = (float)v;
    }
  }
}

__host__ size_t align256(size_t n) { return (n + 255) & ~size_t(255); }

}  // namespace

extern "C" {

int nws_mfcc_dims(double sample_rate, int n_fft, int n_mfcc, int n_mels, int32_t* dims) {
  if (!dims) return NWS_ERR_BAD_ARG;
  const MfccTable* c = mfcc_table(sample_rate, n_fft, n_mfcc, n_mels);
  if (!c) return NWS_ERR_UNSUPPORTED;
  const MfccDims d = mfcc_dims(*c, n_mfcc);
  const int32_t v[8] = {d.bins, d.n_mels, d.n_mfcc, d.jpad, d.nnz, d.off_w, d.off_dct, d.words};
  for (int i = 0; i < 8; ++i) dims[i] = v[i];
  return NWS_OK;
}

size_t nws_mfcc_table_bytes(double sample_rate, int n_fft, int n_mfcc, int n_mels) {
  const MfccTable* c = mfcc_table(sample_rate, n_fft, n_mfcc, n_mels);
  return c ? (size_t)mfcc_dims(*c, n_mfcc).words * sizeof(float) : 0;
}

int nws_mfcc_table(double sample_rate, int n_fft, int n_mfcc, int n_mels, float* table_host) {
  if (!table_host) return NWS_ERR_BAD_ARG;
  const MfccTable* c = mfcc_table(sample_rate, n_fft, n_mfcc, n_mels);
  if (!c) return NWS_ERR_UNSUPPORTED;
  const MfccDims d = mfcc_dims(*c, n_mfcc);
  int32_t* spans = reinterpret_cast<int32_t*>(table_host);
  int off = 0;
  for (int i = 0; i < n_mels; ++i) {
    spans[3 * i] = c->first[i];
    spans[3 * i + 1] = c->count[i];
    spans[3 * i + 2] = off;
    off += c->count[i];
  }
  for (int i = 0; i < d.nnz; ++i) table_host[d.off_w + i] = (float)c->weights[i];
  float* dct = table_host + d.off_dct;
  for (int m = 0; m < n_mels; ++m)
    for (int j = 0; j < d.jpad; ++j) {
      const double s = sqrt((j == 0 ? 1.0 : 2.0) / (double)n_mels);
      dct[(size_t)m * d.jpad + j] = j < n_mfcc ? (float)(s * cos(M_PI * (double)j * (double)(2 * m + 1) / (double)(2 * n_mels))) : 0.0f;
    }
  return NWS_OK;
}

size_t nws_mfcc_workspace_bytes(int B, int N, int n_fft, int hop, int n_mels) {
  const size_t stft = nws_loudness_workspace_bytes(B, N, n_fft, hop);
  if (stft == 0 || n_mels < 1 || n_mels > kMaxMels) return 0;
  const size_t frames_pad = ((size_t)nws_loudness_frames(N, hop) + 31) / 32 * 32;
  return align256(stft) + align256((size_t)B * sizeof(unsigned)) + (size_t)B * n_mels * frames_pad * sizeof(float);
}

int nws_mfcc(const float* audio, int B, int N, double sample_rate, int n_fft, int hop, int n_mfcc, int n_mels, const float* dft,
             const float* table, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!audio || !dft || !table || !out || !workspace || B < 1) return NWS_ERR_BAD_ARG;
  const MfccTable* c = mfcc_table(sample_rate, n_fft, n_mfcc, n_mels);
  if (!c || B > 65535 || nws_loudness_workspace_bytes(1, n_fft, n_fft, hop) == 0) return NWS_ERR_UNSUPPORTED;
  if (N <= n_fft / 2) return NWS_ERR_BAD_ARG;  // reflect padding needs more than n_fft/2 samples
  const size_t stft = nws_loudness_workspace_bytes(B, N, n_fft, hop);
  if (stft == 0) return NWS_ERR_UNSUPPORTED;
  if (workspace_bytes < nws_mfcc_workspace_bytes(B, N, n_fft, hop, n_mels)) return NWS_ERR_WORKSPACE;
  const MfccDims d = mfcc_dims(*c, n_mfcc);
  const int frames = nws_loudness_frames(N, hop);
  const int frames_pad = (frames + 31) / 32 * 32;
  // workspace: [max power bits | power (B, bins, frames_pad)] as nws_loudness lays them out, [max mel bits], mel (B, n_mels, frames_pad)
  char* ws = static_cast<char*>(workspace);
  unsigned* max_bits = reinterpret_cast<unsigned*>(ws);
  float* power = reinterpret_cast<float*>(ws + align256((size_t)B * sizeof(unsigned)));
  unsigned* mel_max = reinterpret_cast<unsigned*>(ws + align256(stft));
  float* mel = reinterpret_cast<float*>(ws + align256(stft) + align256((size_t)B * sizeof(unsigned)));
  hipStream_t st = (hipStream_t)stream;
  const int rc = nws_stft_power_pass(audio, B, N, n_fft, hop, dft, power, max_bits, stream);
  if (rc != NWS_OK) return rc;
  const hipError_t e = hipMemsetAsync(mel_max, 0, (size_t)B * sizeof(unsigned), st);
  if (e != hipSuccess) return (int)e;
  mfcc_mel_kernel<<<dim3((frames + 63) / 64, B), 256, 0, st>>>(power, table, d.bins, n_mels, d.off_w, d.nnz, frames, frames_pad, mel,
                                                                  mel_max);
  NWS_CHECK_LAUNCH();
  mfcc_dct_kernel<<<dim3((frames + 255) / 256, d.jpad / kJ, B), 256, 0, st>>>(mel, mel_max, table + d.off_dct, n_mels, n_mfcc, d.jpad,
                                                                              frames, frames_pad, sqrt((double)n_mels), out);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

}  // extern "C"
