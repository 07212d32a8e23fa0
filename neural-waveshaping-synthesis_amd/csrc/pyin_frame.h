// pYIN, the per-frame work that the offline extractor (pyin.hip) and the fixed-lag stream (pyin_stream.hip) share:
//   the configuration's derived sizes, the difference / CMND of a tile of frames from a staged sample window, the
//   observation of a frame, and one max-plus step of the decode with its (max, lowest index) reduction.
// The two forms must produce the same bits for the same frame, so neither keeps a copy of its own:
// every sum below is formed in an order that depends on the configuration alone - never on the batch row, on the frame's
// place in its tile, or on where the samples came from.
#pragma once
#include <math.h>

#include "nws_common.h"

namespace {

constexpr int kFrames = 32;        // frames per workgroup of the difference kernel
constexpr int kMaxLags = 512;      // observation kernel: 8 chunks of 64 lanes
constexpr int kMaxChunks = 8;
constexpr int kThresholds = 100;
constexpr int kMaxBins = 1024;     // Viterbi: one thread per pitch bin
constexpr int kMaxWidth = 127;     // backpointer byte = half * width + offset; 255 = jump from the global maximum
constexpr int kJump = 255;
constexpr size_t kLdsCap = 160 * 1024;
constexpr int kHdr = 16;           // doubles in front of the tables
constexpr float kTiny32 = 1.17549435e-38f;
constexpr double kTiny64 = 2.2250738585072014e-308;
constexpr double kSwitchProb = 0.01, kNoTroughProb = 0.01, kMaxTransitionRate = 35.92, kResolution = 0.1, kBoltzmann = 2.0;

struct PyinDims {
  int min_period, max_period, lags, n_bps, n_bins, width, W, q;   // q: hop blocks per frame in the shared form, 0 = plain form
  int frame_length, hop;
  double sr, fmin;
  // table offsets (doubles)
  int o_beta, o_E, o_D, o_logw, o_lrs, o_f0, n_table;
  size_t cmnd_lds;
};

__host__ inline bool pyin_dims(double sr, double fmin, double fmax, int fl, int hop, PyinDims* d) {
  if (!(sr > 0.0) || !(fmin > 0.0) || !(fmax > fmin) || fl < 8 || fl > 2 * kMaxLags || hop < 1 || hop > fl) return false;
  if (!(sr / fmin < 1e6) || !(fmax / fmin < 1e6) || !(sr / fmax < 1e6)) return false;
  d->frame_length = fl;
  d->hop = hop;
  d->sr = sr;
  d->fmin = fmin;
  d->W = fl / 2;
  d->min_period = (int)floor(sr / fmax) > 1 ? (int)floor(sr / fmax) : 1;
  const int mp = (int)ceil(sr / fmin);
  d->max_period = mp < fl - d->W - 1 ? mp : fl - d->W - 1;
  d->lags = d->max_period - d->min_period + 1;
  if (d->lags < 3 || d->lags > kMaxLags) return false;
  d->n_bps = (int)ceil(1.0 / kResolution);
  d->n_bins = (int)floor(12.0 * d->n_bps * log2(fmax / fmin)) + 1;
  d->width = (int)rint(kMaxTransitionRate * 12.0 * hop / sr) * d->n_bps + 1;
  if (d->n_bins < 1 || d->n_bins > kMaxBins || d->width > kMaxWidth || !(d->width & 1)) return false;
  const size_t span = (size_t)(kFrames - 1) * hop + fl, LP = (size_t)d->max_period + 1;
  d->q = 0;
  d->cmnd_lds = (span + kFrames * LP) * sizeof(float);
  if (d->W % hop == 0) {
    const size_t shared = (span + (kFrames + d->W / hop - 1) * LP) * sizeof(float);
    if (shared <= 64 * 1024) {
      d->q = d->W / hop;
      d->cmnd_lds = shared;
    }
  }
  if (d->cmnd_lds > kLdsCap) return false;
  const int h = (d->width - 1) / 2;
  d->o_beta = kHdr;
  d->o_E = d->o_beta + kThresholds;
  d->o_D = d->o_E + d->lags;
  d->o_logw = d->o_D + d->lags + 1;
  d->o_lrs = d->o_logw + h + 1;
  d->o_f0 = d->o_lrs + d->n_bins;
  d->n_table = d->o_f0 + d->n_bins;
  return true;
}

__host__ inline size_t pyin_align256(size_t n) { return (n + 255) & ~size_t(255); }

// sum_{j < n} (xa[j] - xb[j])^2: two packed accumulators (4 interleaved chains), then the tail
__device__ __forceinline__ float sqdiff_sum(const float* xa, const float* xb, int n) {
  f32x2 acc0 = {0.0f, 0.0f}, acc1 = {0.0f, 0.0f};
  int j = 0;
  for (; j + 4 <= n; j += 4) {
    const f32x2 a0 = {xa[j], xa[j + 1]}, b0 = {xb[j], xb[j + 1]};
    const f32x2 a1 = {xa[j + 2], xa[j + 3]}, b1 = {xb[j + 2], xb[j + 3]};
    const f32x2 d0 = a0 - b0, d1 = a1 - b1;
    acc0 = fma2(d0, d0, acc0);
    acc1 = fma2(d1, d1, acc1);
  }
  float s = nws_add_scalar(nws_add_scalar(acc0.x, acc1.x), nws_add_scalar(acc0.y, acc1.y));
  for (; j < n; ++j) {
    const float d = xa[j] - xb[j];
    s = fmaf(d, d, s);
  }
  return s;
}

// Difference function + cumulative-mean normalisation of the kFrames frames from frame t0 on, by one workgroup of 256 threads.
// `sample(i)` is the signal at the (padded) position i, i = 0 being sample 0 of the row: the caller resolves the reflection at
// the edges, and may return anything for positions that only frames >= t_end touch.  Frame t < t_end is written to
// out + (t - t0) * lags; `lds` holds PyinDims::cmnd_lds bytes.
template <class Sample>
__device__ __forceinline__ void pyin_cmnd_tile(Sample sample, int t0, int t_end, const PyinDims& k, float* __restrict__ out,
                                               float* lds) {
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int fl = k.frame_length, hop = k.hop, maxp = k.max_period, LP = maxp + 1;
  const int span = (kFrames - 1) * hop + fl;
  float* xs = lds;
  float* P = lds + span;  // [rows][LP], tau = 0 .. max_period (tau = 0 unused)
  const long long first = (long long)hop * t0 - fl / 2;  // centre padding: frame t covers [hop t - fl/2, hop t + fl/2)
  const int nfr = t_end - t0 < kFrames ? t_end - t0 : kFrames;   // frames of this tile that exist: the others cost nothing
  for (int j = tid; j < (nfr - 1) * hop + fl; j += 256) xs[j] = sample(first + j);
  __syncthreads();
  const int rows = k.q ? nfr + k.q - 1 : nfr;
  const int n = k.q ? hop : k.W;
  for (int item = tid; item < rows * maxp; item += 256) {
    const int r = item / maxp, tau = item - r * maxp + 1;
    const float* xa = xs + r * hop;
    P[r * LP + tau] = sqdiff_sum(xa, xa + tau, n);
  }
  __syncthreads();
  if (k.q > 1) {
    // d_f = P(f) + P(f + 1) + ...: a column belongs to one thread, rows ascend, so the sums may replace P(f) in place
    for (int tau = 1 + tid; tau <= maxp; tau += 256) {
      for (int f = 0; f < nfr; ++f) {
        float s = P[f * LP + tau];
        for (int i = 1; i < k.q; ++i) s += P[(f + i) * LP + tau];
        P[f * LP + tau] = s;
      }
    }
    __syncthreads();
  }
  for (int f = wave; f < kFrames; f += 4) {
    const int t = t0 + f;
    if (t >= t_end) break;  // wave-uniform
    float carry = 0.0f;
    float* o = out + (size_t)f * k.lags;
    for (int c0 = 1; c0 <= maxp; c0 += 64) {
      const int tau = c0 + lane;
      const float v = tau <= maxp ? P[f * LP + tau] : 0.0f;
      float s = v;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const float o2 = __shfl_up(s, off, 64);
        if (lane >= off) s += o2;
      }
      const float cum = carry + s;
      carry = __shfl(cum, 63, 64);
      if (tau >= k.min_period && tau <= maxp) o[tau - k.min_period] = v / (kTiny32 + cum / (float)tau);
    }
  }
}

// Observation of the four frames 4 blockIdx.x .. + 3 of row blockIdx.y, by one workgroup of 256 threads: one wave per frame,
// lanes over lags.  The rank of a trough among the troughs under a threshold is a popcount of a ballot mask below the lane.
// Threshold compares, probabilities, parabolic shift and bin in fp64.  All arrays are (rows, T, ...).
__device__ __forceinline__ void pyin_observe_block(const float* __restrict__ yin, int T, const PyinDims& k,
                                                   const double* __restrict__ table, int* __restrict__ cand_bin,
                                                   double* __restrict__ cand_prob, int* __restrict__ count,
                                                   double* __restrict__ voiced_prob) {
  __shared__ double sE[kMaxLags], sD[kMaxLags + 1], sBeta[kThresholds];
  __shared__ double sProb[4][kMaxLags];
  __shared__ int sBin[4][kMaxLags];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int lags = k.lags, b = blockIdx.y;
  for (int i = tid; i < lags; i += 256) sE[i] = table[k.o_E + i];
  for (int i = tid; i <= lags; i += 256) sD[i] = table[k.o_D + i];
  for (int i = tid; i < kThresholds; i += 256) sBeta[i] = table[k.o_beta + i];
  __syncthreads();
  const int t = blockIdx.x * 4 + wave;
  const bool valid = t < T;
  const float* y = yin + ((size_t)b * T + (valid ? t : T - 1)) * lags;
  const int nch = (lags + 63) >> 6;
  const unsigned long long below = (1ull << lane) - 1ull;

  float yv[kMaxChunks];
  bool tr[kMaxChunks];
  double p[kMaxChunks];
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c) {
    yv[c] = 0.0f;
    tr[c] = false;
    p[c] = 0.0;
    if (c < nch) {
      const int i = 64 * c + lane;
      if (i < lags) {
        const float yc = y[i];
        yv[c] = yc;
        if (i == 0) tr[c] = yc < y[1];
        else if (i < lags - 1) tr[c] = yc < y[i - 1] && yc <= y[i + 1];
      }
    }
  }
  double no_trough = 0.0;
  for (int th = 1; th <= kThresholds; ++th) {
    const double theta = (double)th / 100.0, bk = sBeta[th - 1];
    unsigned long long m[kMaxChunks];
    int n = 0;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
      m[c] = 0;
      if (c < nch) {
        m[c] = __ballot(tr[c] && (double)yv[c] < theta);
        n += __popcll(m[c]);
      }
    }
    if (n == 0) {
      no_trough += bk;
      continue;
    }
    const double dn = sD[n];
    int base = 0;
#pragma unroll
    for (int c = 0; c < kMaxChunks; ++c) {
      if (c < nch) {
        if ((m[c] >> lane) & 1ull) p[c] += sE[base + __popcll(m[c] & below)] / dn * bk;
        base += __popcll(m[c]);
      }
    }
  }
  // the lowest trough (the first of equal ones) takes the mass of the thresholds no trough is below
  float best = INFINITY;
  int best_i = 0x7fffffff;
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c)
    if (c < nch && tr[c] && yv[c] < best) {
      best = yv[c];
      best_i = 64 * c + lane;
    }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const float ov = __shfl_xor(best, off, 64);
    const int oi = __shfl_xor(best_i, off, 64);
    if (ov < best || (ov == best && oi < best_i)) {
      best = ov;
      best_i = oi;
    }
  }
  int base = 0;
#pragma unroll
  for (int c = 0; c < kMaxChunks; ++c) {
    if (c < nch) {
      const int i = 64 * c + lane;
      if (tr[c] && i == best_i) p[c] += kNoTroughProb * no_trough;
      const bool cand = tr[c] && p[c] > 0.0;
      const unsigned long long mc = __ballot(cand);
      if (cand) {
        double shift = 0.0;
        if (i > 0 && i < lags - 1) {
          const double y0 = (double)y[i - 1], y1 = (double)yv[c], y2 = (double)y[i + 1];
          const double a = y0 + y2 - 2.0 * y1, bb = (y2 - y0) / 2.0;
          if (fabs(bb) < fabs(a)) shift = -bb / a;
        }
        const double f0 = k.sr / ((double)(k.min_period + i) + shift);
        double bin = rint((double)(12 * k.n_bps) * log2(f0 / k.fmin));
        bin = bin < 0.0 ? 0.0 : (bin > (double)k.n_bins ? (double)k.n_bins : bin);
        const int pos = base + __popcll(mc & below);
        sBin[wave][pos] = (int)bin;
        sProb[wave][pos] = p[c];
      }
      base += __popcll(mc);
    }
  }
  __syncthreads();
  // obs[bin] is ASSIGNED in lag order: a later candidate of the same bin replaces an earlier one.  Periods rise strictly with
  // the trough index (troughs are >= 2 lags apart, |shift| < 1), so bins never rise and equal bins are neighbours in the list.
  // Bin n_pitch_bins belongs to the unvoiced half and is overwritten there.
  double vsum = 0.0;
  const size_t fo = ((size_t)b * T + (valid ? t : 0)) * lags;
  for (int idx = lane; idx < lags; idx += 64) {
    int bin = -1;
    double pr = 0.0;
    if (idx < base) {
      bin = sBin[wave][idx];
      pr = sProb[wave][idx];
      if (bin < k.n_bins && (idx == base - 1 || sBin[wave][idx + 1] != bin)) vsum += pr;
    }
    if (valid) {
      cand_bin[fo + idx] = bin;
      cand_prob[fo + idx] = pr;
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) vsum += __shfl_xor(vsum, off, 64);
  if (valid && lane == 0) {
    count[(size_t)b * T + t] = base;
    voiced_prob[(size_t)b * T + t] = vsum < 0.0 ? 0.0 : (vsum > 1.0 ? 1.0 : vsum);
  }
}

// ---- the decode: one workgroup of 1024 threads per row, thread j owns pitch bin j in both halves of the state space ---------
// (max, lowest index) of a frame's value vector over the wave -> redv / redi[wave]; vv / vuu are thread j's voiced and
// unvoiced values (V itself, not V - log rowsum)
__device__ __forceinline__ void pyin_wave_max(double vv, double vuu, int j, int npb, bool active, double* redv, int* redi) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double v = vv;
  int i = j;
  if (vuu > v) {
    v = vuu;
    i = npb + j;
  }
  if (!active) {
    v = -INFINITY;
    i = 0x7fffffff;
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const double ov = __shfl_xor(v, off, 64);
    const int oi = __shfl_xor(i, off, 64);
    if (ov > v || (ov == v && oi < i)) {
      v = ov;
      i = oi;
    }
  }
  if (lane == 0) {
    redv[wave] = v;
    redi[wave] = i;
  }
}

// the 16 waves' maxima -> the frame's maximum and its lowest state (every thread computes the same pair)
__device__ __forceinline__ void pyin_global_max(const double* redv, const int* redi, double& G, int& gi) {
  G = -INFINITY;
  gi = 0x7fffffff;
  for (int w = 0; w < 16; ++w) {
    const double v = redv[w];
    const int i = redi[w];
    if (v > G || (v == G && i < gi)) {
      G = v;
      gi = i;
    }
  }
}

// One max-plus step for target bin j.  pa / pu point at entry j of the previous frame's voiced / unvoiced row of
// value - log rowsum (h entries of -inf on either side of a row: the band needs no range checks); G is that frame's maximum.
// One pass of the triangle over each source half serves both target halves; ascending source index and strict compares, so
// ties go to the lowest source.  Returns the best predecessor value of the voiced and the unvoiced target (the observation
// is not added yet) and their backpointer bytes: half * width + offset, or kJump = from the global maximum.
// HC: half width of the transition window at compile time (15 = librosa's 35.92 octaves / s at hop 128 / 16 kHz: the band
// unrolls, its 62 LDS reads are in flight together and the window weights stay in scalar registers across steps); 0 = runtime
template <int HC>
__device__ __forceinline__ void pyin_maxplus(const double* pa, const double* pu, const double* __restrict__ logw, int h,
                                             int width, double G, double ltiny, double l1s, double lsw, double& best_v,
                                             int& code_v, double& best_u, int& code_u) {
  double mv = -INFINITY, mu = -INFINITY;
  int kv = h, ku = h;
  auto source = [&](int o) {
    const double lw = logw[o < 0 ? -o : o];
    const double a = pa[o] + lw, u = pu[o] + lw;
    if (a > mv) {
      mv = a;
      kv = o + h;
    }
    if (u > mu) {
      mu = u;
      ku = o + h;
    }
  };
  if constexpr (HC > 0) {
#pragma unroll
    for (int o = -HC; o <= HC; ++o) source(o);
  } else {
    for (int o = -h; o <= h; ++o) source(o);
  }
  const double cj = G + ltiny;
  // voiced target: voiced sources stay in the half, unvoiced ones switch
  best_v = mv + l1s;
  code_v = kv;
  if (mu + lsw > best_v) {
    best_v = mu + lsw;
    code_v = width + ku;
  }
  if (cj > best_v) {
    best_v = cj;
    code_v = kJump;
  }
  // unvoiced target
  best_u = mv + lsw;
  code_u = kv;
  if (mu + l1s > best_u) {
    best_u = mu + l1s;
    code_u = width + ku;
  }
  if (cj > best_u) {
    best_u = cj;
    code_u = kJump;
  }
}

// the state a backpointer byte of state s leads to; `jump`: the previous frame's lowest best state
__device__ __forceinline__ int pyin_predecessor(int code, int s, int jump, int npb, int width, int h) {
  int r;
  if (code == kJump) {
    r = jump;
  } else {
    const int bin = s >= npb ? s - npb : s;
    const int half = code >= width ? 1 : 0;
    r = half * npb + bin + (code - half * width) - h;
  }
  return r < 0 ? 0 : (r >= 2 * npb ? 2 * npb - 1 : r);
}

}  // namespace
