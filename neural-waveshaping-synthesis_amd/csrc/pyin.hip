// pYIN F0 extractor, the other half of the analysis front end (loudness.hip is the first):
//   neural_waveshaping_synthesis/data/utils/f0_extraction.py:61-92 (extract_f0_with_pyin -> librosa.pyin) as three stages.
//   DESIGN.md 3.9 holds the definition the kernels are tested against; parity with librosa itself is unpinned.
//
// 1. pyin_cmnd_kernel: YIN difference function as SQUARED DIFFERENCES + cumulative-mean normalisation.  A workgroup owns 32
//    frames; the 31 hop + frame_length samples they are cut from are staged in LDS once (reflect padding resolved there).
//    When hop divides W = frame_length / 2 the frames share per-hop block sums P(u, tau) = sum_{j < hop} (x[u hop + j] -
//    x[u hop + j + tau])^2: d_t = P(t) + .. + P(t + W/hop - 1), a quarter of the work at 1024 / 128.  Otherwise (or when the
//    block sums do not fit LDS) every frame sums its own W terms.  Both are the same sum of non-negative terms; the order of
//    summation depends on the configuration only, never on the batch row or the frame's place in its tile.  Packed fp32
//    (two samples per instruction, no operand swizzles); the prefix sum over lags is an in-wave scan.
// 2. pyin_observe_kernel: one wave per frame, lanes over lags.  The rank of a trough among the troughs under a threshold is
//    a popcount of a ballot mask below the lane.  Threshold compares, probabilities, parabolic shift and bin in fp64.  Output
//    is the sparse candidate list (bin, prob) in lag order + count + voiced_prob; the dense observation matrix never exists.
// 3. pyin_viterbi_kernel: one persistent workgroup per utterance, one thread per pitch bin (both halves of the state space).
//    The value vector lives in LDS in fp64, double buffered as value - log rowsum; one max-plus pass of the triangle over each
//    source half serves both target halves.  Transitions outside the band have probability 0, i.e. log(0 + tiny): their
//    best source is the previous step's global maximum, found as a by-product of the step before (backpointer 255 + one
//    word per frame).  One barrier per step: the next frame's observations are scattered into a rotating third buffer.
//    One byte of backpointer per state and frame; the backtrace runs at the end of the same launch.
//
// Limits (NWS_ERR_UNSUPPORTED beyond them): lags = max_period - min_period + 1 <= 512 (frame_length <= 1024),
// n_pitch_bins <= 1024, transition window <= 127, B <= 65535, the difference kernel's tile
// (31 hop + frame_length + 32 (max_period + 1) floats) <= 160 KB of LDS.
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

__host__ bool pyin_dims(double sr, double fmin, double fmax, int fl, int hop, PyinDims* d) {
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

__global__ __launch_bounds__(256) void pyin_cmnd_kernel(const float* __restrict__ audio, int N, int T, PyinDims k,
                                                        float* __restrict__ yin) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int t0 = blockIdx.x * kFrames, b = blockIdx.y;
  const int fl = k.frame_length, hop = k.hop, maxp = k.max_period, LP = maxp + 1;
  const int span = (kFrames - 1) * hop + fl;
  float* xs = lds;
  float* P = lds + span;  // [rows][LP], tau = 0 .. max_period (tau = 0 unused)
  const float* x = audio + (size_t)b * N;
  const long long first = (long long)hop * t0 - fl / 2;  // centre padding: frame t covers [hop t - fl/2, hop t + fl/2)
  for (int j = tid; j < span; j += 256) xs[j] = x[reflect_index(first + j, N)];
  __syncthreads();
  const int rows = k.q ? kFrames + k.q - 1 : kFrames;
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
      for (int f = 0; f < kFrames; ++f) {
        float s = P[f * LP + tau];
        for (int i = 1; i < k.q; ++i) s += P[(f + i) * LP + tau];
        P[f * LP + tau] = s;
      }
    }
    __syncthreads();
  }
  for (int f = wave; f < kFrames; f += 4) {
    const int t = t0 + f;
    if (t >= T) break;  // wave-uniform
    float carry = 0.0f;
    float* out = yin + ((size_t)b * T + t) * k.lags;
    for (int c0 = 1; c0 <= maxp; c0 += 64) {
      const int tau = c0 + lane;
      const float v = tau <= maxp ? P[f * LP + tau] : 0.0f;
      float s = v;
#pragma unroll
      for (int off = 1; off < 64; off <<= 1) {
        const float o = __shfl_up(s, off, 64);
        if (lane >= off) s += o;
      }
      const float cum = carry + s;
      carry = __shfl(cum, 63, 64);
      if (tau >= k.min_period && tau <= maxp) out[tau - k.min_period] = v / (kTiny32 + cum / (float)tau);
    }
  }
}

__global__ __launch_bounds__(256) void pyin_observe_kernel(const float* __restrict__ yin, int T, PyinDims k,
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

// HC: half width of the transition window at compile time (15 = librosa's 35.92 octaves / s at hop 128 / 16 kHz: the band
// unrolls, its 62 LDS reads are in flight together and the window weights stay in scalar registers across steps); 0 = runtime
template <int HC>
__global__ __launch_bounds__(1024) void pyin_viterbi_kernel(const int* __restrict__ cand_bin, const double* __restrict__ cand_prob,
                                                            const int* __restrict__ count, const double* __restrict__ voiced_prob,
                                                            int T, PyinDims k, const double* __restrict__ table,
                                                            unsigned char* __restrict__ bp, int* __restrict__ gidx, int fill,
                                                            float fill_value, int* __restrict__ states, float* __restrict__ f0) {
  extern __shared__ double vl[];
  const int npb = k.n_bins, width = k.width, h = HC > 0 ? HC : (width - 1) / 2, lags = k.lags, S = 2 * npb;
  const int row = npb + 2 * h;      // a value row carries h entries of -inf on either side: the band needs no range checks
  double* va = vl;                  // [2][row] voiced value - log rowsum
  double* vu = va + 2 * row;        // [2][row] unvoiced value - log rowsum
  double* lobs = vu + 2 * row;      // [3][npb] log(obs + tiny) of the voiced states, frames t, t + 1 and the slot being cleared
  double* lrs = lobs + 3 * npb;     // [npb]
  double* redv = lrs + npb;         // [2][16] per-wave maxima of the value vector
  double* lunv = redv + 32;         // [4] log(obs + tiny) of the unvoiced states
  int* redi = reinterpret_cast<int*>(lunv + 4);   // [2][16]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, b = blockIdx.x, j = tid;
  const bool active = j < npb;
  const double l1s = table[8], lsw = table[9], ltiny = table[10], linit = table[11];
  const double* logw = table + k.o_logw;   // read at wave-uniform indices: scalar loads
  const unsigned char* bpb = bp + (size_t)b * T * S;
  unsigned char* bpw = bp + (size_t)b * T * S;
  int* gb = gidx + (size_t)b * T;

  if (active) {
    lrs[j] = table[k.o_lrs + j];
    lobs[j] = ltiny;
    lobs[npb + j] = ltiny;
    lobs[2 * npb + j] = ltiny;
  }
  for (int i = tid; i < 4 * row; i += 1024) va[i] = -INFINITY;   // va and vu are adjacent: pads (and everything else)

  // A frame's sparse observations: candidate c belongs to thread c (lags <= 512).  Loaded one step ahead of their use, so that
  // no step waits for global memory: fetch(t + 2) is issued at the head of step t, put(t + 1) follows the step's arithmetic.
  struct Obs {
    int bin, nxt, cnt;
    double prob, vp;
  };
  auto fetch = [&](int tn) {
    Obs o = {-1, -1, 0, 0.0, 0.0};
    if (tn < T) {
      const size_t fr = (size_t)b * T + tn;
      o.cnt = count[fr];
      if (tid < lags) {
        o.bin = cand_bin[fr * lags + tid];
        o.nxt = tid + 1 < lags ? cand_bin[fr * lags + tid + 1] : -1;
        o.prob = cand_prob[fr * lags + tid];
      }
      if (tid == 1023) o.vp = voiced_prob[fr];
    }
    return o;
  };
  auto put = [&](int tn, const Obs& o) {   // into slot tn % 3 (cleared two steps earlier); a later candidate of a bin replaces it
    if (tn >= T) return;
    const int cnt = o.cnt < lags ? o.cnt : lags;
    if (tid < cnt && o.bin >= 0 && o.bin < npb && (tid == cnt - 1 || o.nxt != o.bin))
      lobs[(tn % 3) * npb + o.bin] = log(o.prob + kTiny64);
    if (tid == 1023) lunv[tn % 3] = log((1.0 - o.vp) / (double)npb + kTiny64);
  };
  auto reduce = [&](double vv, double vuu, int slot) {   // (max, lowest index) over the wave -> redv / redi[slot][wave]
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
      redv[slot * 16 + wave] = v;
      redi[slot * 16 + wave] = i;
    }
  };
  auto global_max = [&](int slot, double& G, int& gi) {
    G = -INFINITY;
    gi = 0x7fffffff;
    for (int w = 0; w < 16; ++w) {
      const double v = redv[slot * 16 + w];
      const int i = redi[slot * 16 + w];
      if (v > G || (v == G && i < gi)) {
        G = v;
        gi = i;
      }
    }
  };

  Obs next = fetch(0);
  __syncthreads();
  put(0, next);
  next = fetch(1);
  __syncthreads();
  {
    // initial distribution: uniform over the unvoiced half
    double Vv = -INFINITY, Vu = -INFINITY;
    if (active) {
      Vv = ltiny + lobs[j];
      Vu = linit + lunv[0];
      va[h + j] = Vv - lrs[j];
      vu[h + j] = Vu - lrs[j];
    }
    reduce(Vv, Vu, 0);
    put(1, next);
    next = fetch(2);
  }
  __syncthreads();

  for (int t = 1; t < T; ++t) {
    const int cur = t & 1, prev = cur ^ 1;
    const Obs ahead = fetch(t + 2);
    double G;
    int gi;
    global_max(prev, G, gi);
    if (tid == 0) gb[t] = gi;
    double Vv = -INFINITY, Vu = -INFINITY;
    if (active) {
      const double* pa = va + prev * row + h + j;
      const double* pu = vu + prev * row + h + j;
      double mv = -INFINITY, mu = -INFINITY;
      int kv = h, ku = h;
      auto source = [&](int o) {   // ascending source index, strict compare: ties go to the lowest source
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
      double best = mv + l1s;
      int code = kv;
      if (mu + lsw > best) {
        best = mu + lsw;
        code = width + ku;
      }
      if (cj > best) {
        best = cj;
        code = kJump;
      }
      Vv = best + lobs[(t % 3) * npb + j];
      bpw[(size_t)t * S + j] = (unsigned char)code;
      // unvoiced target
      best = mv + lsw;
      code = kv;
      if (mu + l1s > best) {
        best = mu + l1s;
        code = width + ku;
      }
      if (cj > best) {
        best = cj;
        code = kJump;
      }
      Vu = best + lunv[t % 3];
      bpw[(size_t)t * S + npb + j] = (unsigned char)code;
      va[cur * row + h + j] = Vv - lrs[j];
      vu[cur * row + h + j] = Vu - lrs[j];
      lobs[((t + 2) % 3) * npb + j] = ltiny;   // the slot frame t - 1 used
    }
    reduce(Vv, Vu, cur);
    put(t + 1, next);
    next = ahead;
    __syncthreads();
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    double G;
    int s;
    global_max((T - 1) & 1, G, s);   // lowest final state among equal ones
    for (int t = T - 1; t >= 0; --t) {
      const int bin = s >= npb ? s - npb : s;
      states[(size_t)b * T + t] = s;
      f0[(size_t)b * T + t] = (s >= npb && fill) ? fill_value : (float)table[k.o_f0 + bin];
      if (t == 0) break;
      const int code = bpb[(size_t)t * S + s];
      if (code == kJump) {
        s = gb[t];
      } else {
        const int half = code >= width ? 1 : 0;
        s = half * npb + bin + (code - half * width) - h;
      }
      s = s < 0 ? 0 : (s >= S ? S - 1 : s);
    }
  }
}

__host__ size_t viterbi_lds_bytes(int npb) {   // 4 padded value rows, 3 observation rows, row sums, reduction slots
  return ((size_t)4 * (npb + kMaxWidth - 1) + 4 * npb + 32 + 4) * sizeof(double) + 32 * sizeof(int);
}
__host__ size_t align256(size_t n) { return (n + 255) & ~size_t(255); }
__host__ size_t viterbi_ws_bytes(int B, int T, int npb) {
  return align256((size_t)B * T * sizeof(int)) + align256((size_t)B * T * 2 * npb);
}

}  // namespace

extern "C" {

int nws_pyin_frames(int N, int hop) { return (N <= 0 || hop <= 0) ? 0 : 1 + N / hop; }

int nws_pyin_dims(double sample_rate, double fmin, double fmax, int frame_length, int hop, int32_t* dims) {
  PyinDims d;
  if (!dims) return NWS_ERR_BAD_ARG;
  if (!pyin_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return NWS_ERR_UNSUPPORTED;
  const int32_t v[8] = {d.min_period, d.max_period, d.lags, d.n_bps, d.n_bins, d.width, d.W, d.q};
  for (int i = 0; i < 8; ++i) dims[i] = v[i];
  return NWS_OK;
}

size_t nws_pyin_table_bytes(double sample_rate, double fmin, double fmax, int frame_length, int hop) {
  PyinDims d;
  if (!pyin_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return 0;
  return (size_t)d.n_table * sizeof(double);
}

int nws_pyin_table(double sample_rate, double fmin, double fmax, int frame_length, int hop, double* table_host) {
  PyinDims d;
  if (!table_host) return NWS_ERR_BAD_ARG;
  if (!pyin_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return NWS_ERR_UNSUPPORTED;
  double* t = table_host;
  for (int i = 0; i < kHdr; ++i) t[i] = 0.0;
  const int dims[8] = {d.min_period, d.max_period, d.lags, d.n_bps, d.n_bins, d.width, d.W, d.q};
  for (int i = 0; i < 8; ++i) t[i] = (double)dims[i];
  t[8] = log(1.0 - kSwitchProb);
  t[9] = log(kSwitchProb);
  t[10] = log(kTiny64);
  t[11] = log(1.0 / (double)d.n_bins + kTiny64);
  // beta(2, 18) mass of [(k - 1) / 100, k / 100]: cdf(x) = 1 - (1 - x)^18 (1 + 18 x)
  auto cdf = [](double x) { return 1.0 - pow(1.0 - x, 18.0) * (1.0 + 18.0 * x); };
  for (int kk = 1; kk <= kThresholds; ++kk) t[d.o_beta + kk - 1] = cdf((double)kk / 100.0) - cdf((double)(kk - 1) / 100.0);
  // Boltzmann prior of the m-th of n troughs: E[m] / D[n]
  for (int m = 0; m < d.lags; ++m) t[d.o_E + m] = (1.0 - exp(-kBoltzmann)) * exp(-kBoltzmann * m);
  for (int n = 0; n <= d.lags; ++n) t[d.o_D + n] = 1.0 - exp(-kBoltzmann * n);
  // triangle window w[k] = 1 - k / (h + 1) and the sum of each source bin's truncated row
  const int h = (d.width - 1) / 2;
  for (int kk = 0; kk <= h; ++kk) t[d.o_logw + kk] = log(1.0 - (double)kk / (double)(h + 1));
  for (int i = 0; i < d.n_bins; ++i) {
    double s = 0.0;
    for (int o = -h; o <= h; ++o)
      if (i + o >= 0 && i + o < d.n_bins) s += 1.0 - (double)(o < 0 ? -o : o) / (double)(h + 1);
    t[d.o_lrs + i] = log(s);
    t[d.o_f0 + i] = fmin * exp2((double)i / (12.0 * d.n_bps));
  }
  return NWS_OK;
}

size_t nws_pyin_workspace_bytes(int B, int N, double sample_rate, double fmin, double fmax, int frame_length, int hop) {
  PyinDims d;
  if (B <= 0 || N <= 0 || !pyin_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return 0;
  const size_t T = (size_t)nws_pyin_frames(N, hop), n = (size_t)B * T * d.lags;
  return viterbi_ws_bytes(B, (int)T, d.n_bins) + align256(n * sizeof(double)) + align256(n * sizeof(float)) +
         align256(n * sizeof(int)) + align256((size_t)B * T * sizeof(int));
}

int nws_pyin_cmnd(const float* audio, int B, int N, double sample_rate, double fmin, double fmax, int frame_length, int hop,
                  float* yin, void* stream) {
  PyinDims d;
  if (!audio || !yin || B <= 0 || N <= 0) return NWS_ERR_BAD_ARG;
  if (!pyin_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return NWS_ERR_UNSUPPORTED;
  if (N <= frame_length / 2) return NWS_ERR_BAD_ARG;  // reflect padding needs more than frame_length / 2 samples
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  static unsigned long long attr_devices = 0;
  if (nws_first_use_on_device(attr_devices)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pyin_cmnd_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCap);
    if (e != hipSuccess) return (int)e;
  }
  const int T = nws_pyin_frames(N, hop);
  const dim3 grid((T + kFrames - 1) / kFrames, B);
  pyin_cmnd_kernel<<<grid, 256, d.cmnd_lds, (hipStream_t)stream>>>(audio, N, T, d, yin);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

int nws_pyin_observe(const float* yin, int B, int T, double sample_rate, double fmin, double fmax, int frame_length, int hop,
                     const double* table, int* cand_bin, double* cand_prob, int* count, double* voiced_prob, void* stream) {
  PyinDims d;
  if (!yin || !table || !cand_bin || !cand_prob || !count || !voiced_prob || B <= 0 || T <= 0) return NWS_ERR_BAD_ARG;
  if (!pyin_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return NWS_ERR_UNSUPPORTED;
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  const dim3 grid((T + 3) / 4, B);
  pyin_observe_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(yin, T, d, table, cand_bin, cand_prob, count, voiced_prob);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

int nws_pyin_viterbi(const int* cand_bin, const double* cand_prob, const int* count, const double* voiced_prob, int B, int T,
                     double sample_rate, double fmin, double fmax, int frame_length, int hop, const double* table,
                     int fill_unvoiced, float fill_value, int* states, float* f0, void* workspace, size_t workspace_bytes,
                     void* stream) {
  PyinDims d;
  if (!cand_bin || !cand_prob || !count || !voiced_prob || !table || !states || !f0 || !workspace || B <= 0 || T <= 0)
    return NWS_ERR_BAD_ARG;
  if (!pyin_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return NWS_ERR_UNSUPPORTED;
  if (workspace_bytes < viterbi_ws_bytes(B, T, d.n_bins)) return NWS_ERR_WORKSPACE;
  const auto kernel = d.width == 31 ? pyin_viterbi_kernel<15> : pyin_viterbi_kernel<0>;
  static unsigned long long attr_devices = 0;
  if (nws_first_use_on_device(attr_devices)) {
    for (const auto fn : {pyin_viterbi_kernel<15>, pyin_viterbi_kernel<0>}) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                               (int)viterbi_lds_bytes(kMaxBins));
      if (e != hipSuccess) return (int)e;
    }
  }
  int* gidx = static_cast<int*>(workspace);
  unsigned char* bp = static_cast<unsigned char*>(workspace) + align256((size_t)B * T * sizeof(int));
  kernel<<<B, 1024, viterbi_lds_bytes(d.n_bins), (hipStream_t)stream>>>(cand_bin, cand_prob, count, voiced_prob, T, d, table, bp,
                                                                        gidx, fill_unvoiced ? 1 : 0, fill_value, states, f0);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

int nws_pyin(const float* audio, int B, int N, double sample_rate, double fmin, double fmax, int frame_length, int hop,
             const double* table, int fill_unvoiced, float fill_value, float* f0, double* voiced_prob, int* states,
             void* workspace, size_t workspace_bytes, void* stream) {
  PyinDims d;
  if (!audio || !table || !f0 || !voiced_prob || !states || !workspace || B <= 0 || N <= 0) return NWS_ERR_BAD_ARG;
  if (!pyin_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return NWS_ERR_UNSUPPORTED;
  if (workspace_bytes < nws_pyin_workspace_bytes(B, N, sample_rate, fmin, fmax, frame_length, hop)) return NWS_ERR_WORKSPACE;
  const int T = nws_pyin_frames(N, hop);
  const size_t n = (size_t)B * T * d.lags;
  char* p = static_cast<char*>(workspace);
  void* vws = p;
  p += viterbi_ws_bytes(B, T, d.n_bins);
  double* cand_prob = reinterpret_cast<double*>(p);
  p += align256(n * sizeof(double));
  float* yin = reinterpret_cast<float*>(p);
  p += align256(n * sizeof(float));
  int* cand_bin = reinterpret_cast<int*>(p);
  p += align256(n * sizeof(int));
  int* count = reinterpret_cast<int*>(p);
  int rc = nws_pyin_cmnd(audio, B, N, sample_rate, fmin, fmax, frame_length, hop, yin, stream);
  if (rc != NWS_OK) return rc;
  rc = nws_pyin_observe(yin, B, T, sample_rate, fmin, fmax, frame_length, hop, table, cand_bin, cand_prob, count, voiced_prob,
                        stream);
  if (rc != NWS_OK) return rc;
  return nws_pyin_viterbi(cand_bin, cand_prob, count, voiced_prob, B, T, sample_rate, fmin, fmax, frame_length, hop, table,
                          fill_unvoiced, fill_value, states, f0, vws, viterbi_ws_bytes(B, T, d.n_bins), stream);
}

}  // extern "C"
