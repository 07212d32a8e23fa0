// pYIN F0 extractor, the other half of the analysis front end (loudness.hip is the first):
//   neural_waveshaping_synthesis/data/utils/f0_extraction.py:61-92 (extract_f0_with_pyin -> librosa.pyin) as three stages.
//   DESIGN.md 3.9 holds the definition the kernels are tested against; parity with librosa itself is unpinned.
//   The per-frame work of each stage lives in pyin_frame.h, shared with the fixed-lag stream (pyin_stream.hip).
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
#include "pyin_frame.h"

namespace {

__global__ __launch_bounds__(256) void pyin_cmnd_kernel(const float* __restrict__ audio, int N, int T, PyinDims k,
                                                        float* __restrict__ yin) {
  extern __shared__ float lds[];
  const int t0 = blockIdx.x * kFrames, b = blockIdx.y;
  const float* x = audio + (size_t)b * N;
  pyin_cmnd_tile([&](long long i) { return x[reflect_index(i, N)]; }, t0, T, k, yin + ((size_t)b * T + t0) * k.lags, lds);
}

__global__ __launch_bounds__(256) void pyin_observe_kernel(const float* __restrict__ yin, int T, PyinDims k,
                                                           const double* __restrict__ table, int* __restrict__ cand_bin,
                                                           double* __restrict__ cand_prob, int* __restrict__ count,
                                                           double* __restrict__ voiced_prob) {
  pyin_observe_block(yin, T, k, table, cand_bin, cand_prob, count, voiced_prob);
}

// HC: half width of the transition window at compile time (pyin_maxplus); 0 = runtime
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
  const int tid = threadIdx.x, b = blockIdx.x, j = tid;
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
    pyin_wave_max(Vv, Vu, j, npb, active, redv, redi);
    put(1, next);
    next = fetch(2);
  }
  __syncthreads();

  for (int t = 1; t < T; ++t) {
    const int cur = t & 1, prev = cur ^ 1;
    const Obs ahead = fetch(t + 2);
    double G;
    int gi;
    pyin_global_max(redv + prev * 16, redi + prev * 16, G, gi);
    if (tid == 0) gb[t] = gi;
    double Vv = -INFINITY, Vu = -INFINITY;
    if (active) {
      double best_v, best_u;
      int code_v, code_u;
      pyin_maxplus<HC>(va + prev * row + h + j, vu + prev * row + h + j, logw, h, width, G, ltiny, l1s, lsw, best_v, code_v,
                       best_u, code_u);
      Vv = best_v + lobs[(t % 3) * npb + j];
      bpw[(size_t)t * S + j] = (unsigned char)code_v;
      Vu = best_u + lunv[t % 3];
      bpw[(size_t)t * S + npb + j] = (unsigned char)code_u;
      va[cur * row + h + j] = Vv - lrs[j];
      vu[cur * row + h + j] = Vu - lrs[j];
      lobs[((t + 2) % 3) * npb + j] = ltiny;   // the slot frame t - 1 used
    }
    pyin_wave_max(Vv, Vu, j, npb, active, redv + cur * 16, redi + cur * 16);
    put(t + 1, next);
    next = ahead;
    __syncthreads();
  }
  __threadfence();
  __syncthreads();
  if (tid == 0) {
    double G;
    int s;
    pyin_global_max(redv + ((T - 1) & 1) * 16, redi + ((T - 1) & 1) * 16, G, s);   // lowest final state among equal ones
    for (int t = T - 1; t >= 0; --t) {
      const int bin = s >= npb ? s - npb : s;
      states[(size_t)b * T + t] = s;
      f0[(size_t)b * T + t] = (s >= npb && fill) ? fill_value : (float)table[k.o_f0 + bin];
      if (t == 0) break;
      s = pyin_predecessor(bpb[(size_t)t * S + s], s, gb[t], npb, width, h);
    }
  }
}

__host__ size_t viterbi_lds_bytes(int npb) {   // 4 padded value rows, 3 observation rows, row sums, reduction slots
  return ((size_t)4 * (npb + kMaxWidth - 1) + 4 * npb + 32 + 4) * sizeof(double) + 32 * sizeof(int);
}
__host__ size_t align256(size_t n) { return pyin_align256(n); }
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
