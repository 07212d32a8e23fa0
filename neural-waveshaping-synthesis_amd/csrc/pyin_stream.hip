// Fixed-lag pYIN stream: F0 from chunked audio with a bounded delay.  DESIGN.md 3.24 holds the definition
// (tests/pyin_stream_restatement.py restates it); symbols as in pyin.hip / DESIGN.md 3.9, W = frame_length / 2, L = lag.
//
// The stream is the offline extractor's forward pass, frame by frame as the samples arrive - the same CMND, observations,
// value vectors and backpointers, bit for bit (the per-frame code is pyin_frame.h, shared with pyin.hip) - read out by another
// backtrace: frame e leaves once frame e + L exists, as the state at e of the path that ends in argmax V_{e + L}.
//   F(n) = 0 for n <= W, else 1 + (n - W) / hop   frames computed after n samples (all of a frame's samples exist)
//   E(n) = max(0, F(n) - L)                       frames emitted after n samples
// A step with `final` is the step without it followed by a flush: the frames F(N) .. T - 1, T = 1 + N / hop, are computed with
// the right edge reflected about N, and every frame not yet emitted leaves as the state of the path that ends in argmax V_{T-1}.
//
// A pass (a step is one pass; a final step with samples is two) is four launches on the caller's stream:
//   pyin_stream_cmnd_kernel      the new frames' CMND from [history | chunk], tiles of 32 frames as offline
//   pyin_stream_observe_kernel   their observations (pyin_observe_block on the pass's frames)
//   pyin_stream_forward_kernel   one workgroup per row: loads V, runs the new frames' max-plus steps, writes backpointers, jump
//                                words and voiced_prob into the rings, stores V
//   pyin_stream_emit_kernel      one workgroup per row, one thread per emitted frame: walks its <= L backpointers (on a flush
//                                T - 1 - e of them), writes state / f0 / voiced_prob; then moves the sample history on and
//                                advances the counters
// A pass without new frames launches the last kernel only.  No atomics, nothing read back, no waits between workgroups.
// The host passes n_seen (its mirror of the row counter) so that every size and every refusal is decided before the first
// launch; the forward and the emit kernel compare it with the device's counters and leave state and outputs untouched if they
// differ (a step on a stream that was not reset, or that has had `final`).
//
// V is never renormalised (that would change bits against offline).  A frame lowers the maximum of V by at most
// 2 |log(tiny)| + log(2 n_pitch_bins) < 1500, so after 2^21 frames |V| < 3.2e9 and one ulp of V is below 1e-6, four orders under
// the smallest difference between two transition weights: streams are refused beyond 2^21 frames (4.6 h at hop 128 / 16 kHz).
#include "pyin_frame.h"
#include "frame_stream.h"  // frames_done, hist_start: shared with loudness_stream.hip

namespace {

constexpr int kRing = 512;               // frames of backpointers, jump words and voiced_prob a row keeps
constexpr int kStepFrames = 256;         // most new frames of one pass
constexpr int kMaxLag = 255;
constexpr long long kMaxStreamFrames = 1LL << 21;

struct StreamLayout {   // byte offsets inside a row of the state blob; every part 8-byte aligned
  size_t cnt, gmax, v, vp, gw, hist, bp, row;
};

__host__ __device__ inline StreamLayout stream_layout(int npb, int fl) {
  StreamLayout l;
  l.cnt = 0;                                              // int64 n_seen, frames computed, frames emitted, finished
  l.gmax = l.cnt + 4 * sizeof(long long);                 // double max V of the last frame, int64 its lowest state
  l.v = l.gmax + 16;                                      // double [2 npb]: V - log rowsum of the last frame
  l.vp = l.v + (size_t)2 * npb * sizeof(double);          // double [kRing] voiced_prob of frame t at t % kRing
  l.gw = l.vp + (size_t)kRing * sizeof(double);           // int32 [kRing] jump word of frame t: argmax V_{t-1}
  l.hist = l.gw + (size_t)kRing * sizeof(int);            // float [fl] samples hist_start(n_seen) .. n_seen - 1
  l.bp = l.hist + (((size_t)fl * sizeof(float) + 7) & ~size_t(7));   // uint8 [kRing][2 npb] backpointers
  l.row = l.bp + (((size_t)kRing * 2 * npb + 7) & ~size_t(7));
  return l;
}

__host__ bool stream_dims(double sr, double fmin, double fmax, int fl, int hop, PyinDims* d) {
  if (!pyin_dims(sr, fmin, fmax, fl, hop, d)) return false;
  return (d->W + hop - 1) / hop <= kStepFrames;           // a flush computes at most ceil(W / hop) frames
}

// most new frames of one pass of a step of n samples, whatever the stream has seen: n / hop + 1, met by the step that starts at
// n_seen = W (F = 0, not the 1 its closed form would give there) and computes frames 0 .. n / hop; a flush <= ceil(W / hop)
__host__ int pass_frames_bound(int n, const PyinDims& d, int final) {
  int m = n / d.hop + 1;
  if (final && (d.W + d.hop - 1) / d.hop > m) m = (d.W + d.hop - 1) / d.hop;
  return m < 1 ? 1 : m;
}

struct StreamWs {
  size_t yin, cand_bin, cand_prob, count, vp, total;
};
__host__ StreamWs stream_ws(int B, int frames, int lags) {
  const size_t n = (size_t)B * frames * lags;
  StreamWs w;
  w.cand_prob = 0;
  w.vp = w.cand_prob + pyin_align256(n * sizeof(double));
  w.yin = w.vp + pyin_align256((size_t)B * frames * sizeof(double));
  w.cand_bin = w.yin + pyin_align256(n * sizeof(float));
  w.count = w.cand_bin + pyin_align256(n * sizeof(int));
  w.total = w.count + pyin_align256((size_t)B * frames * sizeof(int));
  return w;
}

struct StreamPass {
  int B, n, flush, lag;
  long long n_seen, n_total;        // samples before and after the pass
  long long hs0, hs1;               // hist_start before and after
  int f0, f1, e0, e1;               // frames computed / emitted before and after
  int out_off, out_stride;
};

__device__ __forceinline__ bool stream_state_matches(const long long* cnt, const StreamPass& g) {
  return cnt[0] == g.n_seen && cnt[1] == g.f0 && cnt[2] == g.e0 && cnt[3] == 0;
}

__global__ __launch_bounds__(256) void pyin_stream_cmnd_kernel(const unsigned char* __restrict__ state, const float* __restrict__ x,
                                                               StreamPass g, PyinDims k, float* __restrict__ yin) {
  extern __shared__ float lds[];
  const int b = blockIdx.y, nf = g.f1 - g.f0, t0 = g.f0 + blockIdx.x * kFrames;
  const StreamLayout l = stream_layout(k.n_bins, k.frame_length);
  const float* hist = reinterpret_cast<const float*>(state + (size_t)b * l.row + l.hist);
  const float* xr = x + (size_t)b * g.n;
  const long long N = g.n_total;
  // position i of the padded row: reflected about 0, on a flush about N; samples that do not exist (they belong to frames this
  // pass does not compute) read as 0
  auto sample = [&](long long i) {
    if (i < 0) i = -i;
    if (g.flush && i >= N) i = 2 * (N - 1) - i;
    if (i < g.hs0 || i >= N) return 0.0f;
    return i < g.n_seen ? hist[i - g.hs0] : xr[i - g.n_seen];
  };
  pyin_cmnd_tile(sample, t0, g.f1, k, yin + ((size_t)b * nf + (size_t)blockIdx.x * kFrames) * k.lags, lds);
}

__global__ __launch_bounds__(256) void pyin_stream_observe_kernel(const float* __restrict__ yin, int nf, PyinDims k,
                                                                  const double* __restrict__ table, int* __restrict__ cand_bin,
                                                                  double* __restrict__ cand_prob, int* __restrict__ count,
                                                                  double* __restrict__ voiced_prob) {
  pyin_observe_block(yin, nf, k, table, cand_bin, cand_prob, count, voiced_prob);
}

template <int HC>
__global__ __launch_bounds__(1024) void pyin_stream_forward_kernel(unsigned char* __restrict__ state, StreamPass g, PyinDims k,
                                                                   const double* __restrict__ table,
                                                                   const int* __restrict__ cand_bin,
                                                                   const double* __restrict__ cand_prob,
                                                                   const int* __restrict__ count,
                                                                   const double* __restrict__ voiced_prob) {
  extern __shared__ double vl[];
  const int npb = k.n_bins, width = k.width, h = HC > 0 ? HC : (width - 1) / 2, lags = k.lags, S = 2 * npb;
  const int row = npb + 2 * h;
  double* va = vl;                  // [2][row] voiced value - log rowsum
  double* vu = va + 2 * row;        // [2][row] unvoiced value - log rowsum
  double* lobs = vu + 2 * row;      // [npb] log(obs + tiny) of the voiced states of the frame in hand
  double* lrs = lobs + npb;         // [npb]
  double* redv = lrs + npb;         // [2][16]
  double* lunv = redv + 32;         // [4], one used
  int* redi = reinterpret_cast<int*>(lunv + 4);   // [2][16]
  const int tid = threadIdx.x, b = blockIdx.x, j = tid, nf = g.f1 - g.f0;
  const bool active = j < npb;
  const StreamLayout l = stream_layout(npb, k.frame_length);
  unsigned char* rs = state + (size_t)b * l.row;
  const long long* cnt = reinterpret_cast<const long long*>(rs + l.cnt);
  if (!stream_state_matches(cnt, g)) return;    // workgroup-uniform, in front of every barrier
  double* sG = reinterpret_cast<double*>(rs + l.gmax);
  long long* sgi = reinterpret_cast<long long*>(rs + l.gmax + 8);
  double* Vm = reinterpret_cast<double*>(rs + l.v);
  double* vpr = reinterpret_cast<double*>(rs + l.vp);
  int* gwr = reinterpret_cast<int*>(rs + l.gw);
  unsigned char* bpr = rs + l.bp;
  const double l1s = table[8], lsw = table[9], ltiny = table[10], linit = table[11];
  const double* logw = table + k.o_logw;

  if (active) lrs[j] = table[k.o_lrs + j];
  for (int i = tid; i < 4 * row; i += 1024) va[i] = -INFINITY;
  __syncthreads();
  double G = -INFINITY;
  int gi = 0;
  if (g.f0 > 0) {
    const int prev = (g.f0 - 1) & 1;
    if (active) {
      va[prev * row + h + j] = Vm[j];
      vu[prev * row + h + j] = Vm[npb + j];
    }
    G = sG[0];
    gi = (int)sgi[0];
    gi = gi < 0 ? 0 : (gi >= S ? S - 1 : gi);
  }
  for (int t = g.f0; t < g.f1; ++t) {
    const size_t fr = (size_t)b * nf + (t - g.f0);
    const int cur = t & 1, prev = cur ^ 1;
    // the frame's sparse observations: candidate c belongs to thread c (lags <= 512); a later candidate of a bin replaces it
    int c_bin = -1, c_nxt = -1;
    double c_prob = 0.0;
    const int c_cnt = min(count[fr], lags);
    if (tid < lags) {
      c_bin = cand_bin[fr * lags + tid];
      c_nxt = tid + 1 < lags ? cand_bin[fr * lags + tid + 1] : -1;
      c_prob = cand_prob[fr * lags + tid];
    }
    if (active) lobs[j] = ltiny;
    __syncthreads();
    if (tid < c_cnt && c_bin >= 0 && c_bin < npb && (tid == c_cnt - 1 || c_nxt != c_bin)) lobs[c_bin] = log(c_prob + kTiny64);
    if (tid == 1023) {
      const double vp = voiced_prob[fr];
      lunv[0] = log((1.0 - vp) / (double)npb + kTiny64);
      vpr[t % kRing] = vp;
    }
    __syncthreads();
    double Vv = -INFINITY, Vu = -INFINITY;
    if (t == 0) {
      // initial distribution: uniform over the unvoiced half
      if (active) {
        Vv = ltiny + lobs[j];
        Vu = linit + lunv[0];
      }
    } else {
      if (tid == 0) gwr[t % kRing] = gi;
      if (active) {
        double best_v, best_u;
        int code_v, code_u;
        pyin_maxplus<HC>(va + prev * row + h + j, vu + prev * row + h + j, logw, h, width, G, ltiny, l1s, lsw, best_v, code_v,
                         best_u, code_u);
        Vv = best_v + lobs[j];
        Vu = best_u + lunv[0];
        bpr[(size_t)(t % kRing) * S + j] = (unsigned char)code_v;
        bpr[(size_t)(t % kRing) * S + npb + j] = (unsigned char)code_u;
      }
    }
    if (active) {
      va[cur * row + h + j] = Vv - lrs[j];
      vu[cur * row + h + j] = Vu - lrs[j];
    }
    pyin_wave_max(Vv, Vu, j, npb, active, redv + cur * 16, redi + cur * 16);
    __syncthreads();
    pyin_global_max(redv + cur * 16, redi + cur * 16, G, gi);
  }
  if (nf > 0) {
    const int last = (g.f1 - 1) & 1;
    if (active) {
      Vm[j] = va[last * row + h + j];
      Vm[npb + j] = vu[last * row + h + j];
    }
    if (tid == 0) {
      sG[0] = G;
      sgi[0] = gi;
    }
  }
}

__global__ __launch_bounds__(256) void pyin_stream_emit_kernel(unsigned char* __restrict__ state, const float* __restrict__ x,
                                                               StreamPass g, PyinDims k, const double* __restrict__ table, int fill,
                                                               float fill_value, float* __restrict__ f0, double* __restrict__ vp_out,
                                                               int* __restrict__ states) {
  extern __shared__ float hs[];     // [frame_length] the row's new history
  const int tid = threadIdx.x, b = blockIdx.x, npb = k.n_bins, S = 2 * npb, width = k.width, h = (width - 1) / 2;
  const StreamLayout l = stream_layout(npb, k.frame_length);
  unsigned char* rs = state + (size_t)b * l.row;
  long long* cnt = reinterpret_cast<long long*>(rs + l.cnt);
  if (!stream_state_matches(cnt, g)) return;    // workgroup-uniform, in front of the barrier
  const long long* sgi = reinterpret_cast<const long long*>(rs + l.gmax + 8);
  const double* vpr = reinterpret_cast<const double*>(rs + l.vp);
  const int* gwr = reinterpret_cast<const int*>(rs + l.gw);
  const unsigned char* bpr = rs + l.bp;
  float* hist = reinterpret_cast<float*>(rs + l.hist);
  const int last = g.f1 - 1;
  for (int e = g.e0 + tid; e < g.e1; e += 256) {
    // the path that ends in argmax V_start (lowest state among equal ones): the jump word of frame start + 1 where that
    // frame exists, the value the forward kernel left for the newest frame
    const int start = g.flush ? last : e + g.lag;
    int s = start >= last ? (int)sgi[0] : gwr[(start + 1) % kRing];
    s = s < 0 ? 0 : (s >= S ? S - 1 : s);
    for (int t = start; t > e; --t) s = pyin_predecessor(bpr[(size_t)(t % kRing) * S + s], s, gwr[t % kRing], npb, width, h);
    const size_t o = (size_t)b * g.out_stride + g.out_off + (e - g.e0);
    const int bin = s >= npb ? s - npb : s;
    states[o] = s;
    f0[o] = (s >= npb && fill) ? fill_value : (float)table[k.o_f0 + bin];
    vp_out[o] = vpr[e % kRing];
  }
  // the history moves on: staged in LDS, because the new one overlaps the old one
  const int keep = (int)(g.n_total - g.hs1);
  const float* xr = x + (size_t)b * g.n;
  if (g.n > 0) {
    for (int a = tid; a < keep; a += 256) {
      const long long i = g.hs1 + a;
      hs[a] = i < g.n_seen ? hist[i - g.hs0] : xr[i - g.n_seen];
    }
  }
  __syncthreads();
  if (g.n > 0)
    for (int a = tid; a < keep; a += 256) hist[a] = hs[a];
  if (tid == 0) {
    cnt[0] = g.n_total;
    cnt[1] = g.f1;
    cnt[2] = g.e1;
    cnt[3] = g.flush ? 1 : 0;
  }
}

__host__ size_t forward_lds_bytes(int npb, int h) {
  return ((size_t)4 * (npb + 2 * h) + 2 * npb + 32 + 4) * sizeof(double) + 32 * sizeof(int);
}

__host__ int run_pass(unsigned char* state, const float* x, const StreamPass& g, const PyinDims& d, const double* table, int fill,
                      float fill_value, float* f0, double* vp, int* states, void* workspace, hipStream_t stream) {
  const int nf = g.f1 - g.f0;
  if (nf > 0) {
    const StreamWs w = stream_ws(g.B, nf, d.lags);
    char* p = static_cast<char*>(workspace);
    float* yin = reinterpret_cast<float*>(p + w.yin);
    int* cand_bin = reinterpret_cast<int*>(p + w.cand_bin);
    double* cand_prob = reinterpret_cast<double*>(p + w.cand_prob);
    int* count = reinterpret_cast<int*>(p + w.count);
    double* wvp = reinterpret_cast<double*>(p + w.vp);
    pyin_stream_cmnd_kernel<<<dim3((nf + kFrames - 1) / kFrames, g.B), 256, d.cmnd_lds, stream>>>(state, x, g, d, yin);
    NWS_CHECK_LAUNCH();
    pyin_stream_observe_kernel<<<dim3((nf + 3) / 4, g.B), 256, 0, stream>>>(yin, nf, d, table, cand_bin, cand_prob, count, wvp);
    NWS_CHECK_LAUNCH();
    const auto kernel = d.width == 31 ? pyin_stream_forward_kernel<15> : pyin_stream_forward_kernel<0>;
    kernel<<<g.B, 1024, forward_lds_bytes(d.n_bins, (d.width - 1) / 2), stream>>>(state, g, d, table, cand_bin, cand_prob, count, wvp);
    NWS_CHECK_LAUNCH();
  }
  pyin_stream_emit_kernel<<<g.B, 256, (size_t)d.frame_length * sizeof(float), stream>>>(state, x, g, d, table, fill, fill_value, f0, vp,
                                                                                      states);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

__host__ long long emitted_after(long long n, const PyinDims& d, int lag, int final) {
  if (final) return 1 + n / d.hop;
  const long long f = frames_done(n, d.W, d.hop) - lag;
  return f < 0 ? 0 : f;
}

}  // namespace

extern "C" {

size_t nws_pyin_stream_state_bytes(int B, double sample_rate, double fmin, double fmax, int frame_length, int hop) {
  PyinDims d;
  if (B < 1 || B > 65535 || !stream_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return 0;
  return (size_t)B * stream_layout(d.n_bins, d.frame_length).row;
}

int nws_pyin_stream_max_chunk(double sample_rate, double fmin, double fmax, int frame_length, int hop) {
  PyinDims d;
  return stream_dims(sample_rate, fmin, fmax, frame_length, hop, &d) ? kStepFrames * d.hop : 0;
}

size_t nws_pyin_stream_workspace_bytes(int B, int n, double sample_rate, double fmin, double fmax, int frame_length, int hop,
                                       int final) {
  PyinDims d;
  if (B < 1 || B > 65535 || n < 0 || !stream_dims(sample_rate, fmin, fmax, frame_length, hop, &d) || n > kStepFrames * d.hop) return 0;
  return stream_ws(B, pass_frames_bound(n, d, final ? 1 : 0), d.lags).total;
}

int64_t nws_pyin_stream_frames(int64_t n_seen, double sample_rate, double fmin, double fmax, int frame_length, int hop, int final) {
  PyinDims d;
  if (n_seen < 0 || !stream_dims(sample_rate, fmin, fmax, frame_length, hop, &d) || n_seen > kMaxStreamFrames * d.hop) return -1;
  if (final) return n_seen <= d.W ? -1 : 1 + n_seen / d.hop;
  return frames_done(n_seen, d.W, d.hop);
}

int64_t nws_pyin_stream_emitted(int64_t n_seen, double sample_rate, double fmin, double fmax, int frame_length, int hop, int lag,
                                int final) {
  PyinDims d;
  if (n_seen < 0 || lag < 0 || lag > kMaxLag || !stream_dims(sample_rate, fmin, fmax, frame_length, hop, &d) ||
      n_seen > kMaxStreamFrames * d.hop)
    return -1;
  if (final && n_seen <= d.W) return -1;
  return emitted_after(n_seen, d, lag, final ? 1 : 0);
}

int nws_pyin_stream_reset(void* state, size_t bytes, int B, double sample_rate, double fmin, double fmax, int frame_length, int hop,
                          void* stream) {
  PyinDims d;
  if (!state || B < 1) return NWS_ERR_BAD_ARG;
  if (B > 65535 || !stream_dims(sample_rate, fmin, fmax, frame_length, hop, &d)) return NWS_ERR_UNSUPPORTED;
  const size_t need = (size_t)B * stream_layout(d.n_bins, d.frame_length).row;
  if (bytes < need) return NWS_ERR_BAD_ARG;
  const hipError_t e = hipMemsetAsync(state, 0, need, (hipStream_t)stream);
  return e == hipSuccess ? NWS_OK : (int)e;
}

int nws_pyin_stream_step(void* state, size_t bytes, const float* x, int B, int n, int64_t n_seen, double sample_rate, double fmin,
                         double fmax, int frame_length, int hop, int lag, const double* table_dev, int final, int fill_unvoiced,
                         float fill_value, float* f0, double* voiced_prob, int* states, int out_stride, void* workspace,
                         size_t workspace_bytes, void* stream) {
  PyinDims d;
  if (!state || !table_dev || !f0 || !voiced_prob || !states || !workspace || B < 1 || n < 0 || n_seen < 0 ||
      (n == 0 && !final) || (n > 0 && !x) || lag < 0 || lag > kMaxLag)
    return NWS_ERR_BAD_ARG;
  if (B > 65535 || !stream_dims(sample_rate, fmin, fmax, frame_length, hop, &d) || n > kStepFrames * d.hop ||
      n_seen > kMaxStreamFrames * d.hop - n)
    return NWS_ERR_UNSUPPORTED;
  const long long N = n_seen + n;
  if (final && N <= d.W) return NWS_ERR_BAD_ARG;          // reflect padding needs more than frame_length / 2 samples, as offline
  const long long e_before = emitted_after(n_seen, d, lag, 0), e_mid = emitted_after(N, d, lag, 0);
  const long long e_after = final ? emitted_after(N, d, lag, 1) : e_mid;
  if (out_stride < e_after - e_before) return NWS_ERR_BAD_ARG;
  if (bytes < (size_t)B * stream_layout(d.n_bins, d.frame_length).row) return NWS_ERR_BAD_ARG;
  if (workspace_bytes < stream_ws(B, pass_frames_bound(n, d, final ? 1 : 0), d.lags).total) return NWS_ERR_BAD_ARG;
  static unsigned long long attr_devices = 0;
  if (nws_first_use_on_device(attr_devices)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(pyin_stream_cmnd_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCap);
    if (e != hipSuccess) return (int)e;
  }
  unsigned char* st = static_cast<unsigned char*>(state);
  const int fill = fill_unvoiced ? 1 : 0;
  if (n > 0) {
    const StreamPass g{B, n, 0, lag, n_seen, N, hist_start(n_seen, d.W, d.hop), hist_start(N, d.W, d.hop),
                       (int)frames_done(n_seen, d.W, d.hop), (int)frames_done(N, d.W, d.hop), (int)e_before, (int)e_mid, 0, out_stride};
    const int rc = run_pass(st, x, g, d, table_dev, fill, fill_value, f0, voiced_prob, states, workspace, (hipStream_t)stream);
    if (rc != NWS_OK) return rc;
  }
  if (final) {
    const long long hs = hist_start(N, d.W, d.hop);
    const StreamPass g{B, 0, 1, lag, N, N, hs, hs, (int)frames_done(N, d.W, d.hop), (int)(1 + N / d.hop), (int)e_mid, (int)e_after,
                       (int)(e_mid - e_before), out_stride};
    return run_pass(st, x, g, d, table_dev, fill, fill_value, f0, voiced_prob, states, workspace, (hipStream_t)stream);
  }
  return NWS_OK;
}

}  // extern "C"
