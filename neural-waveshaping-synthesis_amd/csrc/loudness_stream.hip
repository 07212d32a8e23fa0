// Loudness stream: the loudness feature from chunked audio with a bounded delay and a causal reference level.  DESIGN.md 3.25
// holds the definition (tests/loudness_stream_restatement.py restates it); symbols as in pyin_stream.hip / DESIGN.md 3.24,
// W = n_fft / 2, L = lag.
//
// The offline extractor (loudness.hip) normalises by the maximum power of the WHOLE clip, which a stream does not have.  Here a
// row carries one float M: with `track` the running maximum of the frames' peak powers p(t) = max_k P(t, k), started at
// initial_power; without it initial_power for good.  Frame e leaves once frame e + L exists, measured against M(e + L); a flush
// measures what is left against M(T - 1).  The reference of a frame depends on e, L and the signal alone, never on the chunking.
//   F(n) = 0 for n <= W, else 1 + (n - W) / hop   frames computed after n samples (all of a frame's samples exist)
//   E(n) = max(0, F(n) - L)                       frames emitted after n samples
// A step with `final` is the step without it followed by a flush: the frames F(N) .. T - 1, T = 1 + N / hop, are computed with
// the right edge reflected about N.
//
// P(t, k) has the bits loudness_power_kernel writes for that frame of the whole signal: the same tile_transform<1> of
// stft_tile.h on a tile staged from [history | chunk] (a column of the 32x32x2 MFMA accumulates over K in an order that does not
// depend on the column).  The dB pass is loudness_db.h, shared with the offline kernel.
//
// A pass (a step is one pass; a final step with samples is two) is two launches on the caller's stream:
//   loudness_stream_power_kernel  grid (frame tiles, M-tile groups, B): the new frames' power into the P ring, p(t) by atomicMax
//                                 on the float bits into the (zeroed) scratch
//   loudness_stream_emit_kernel   one workgroup per row: extends the M ring (serial prefix maximum over <= 257 new frames), emits
//                                 the released frames, moves the sample history on, advances the counters
// A pass without new frames launches the second only.  Nothing is read back, no workgroup waits for another.  The host passes
// n_seen (its mirror of the row counter) so that every size and refusal is decided before the first launch; both kernels compare
// it with the device's counters and leave state and outputs untouched if they differ.
//
// With a release (the _release entry points) M decays by the factor rho per frame, never below the row's floor F:
// loudness_level.h has the step.  M is no longer monotone then, so frame e is measured against the maximum of M over e .. e + L
// (on a flush over e .. T - 1), which at rho = 1 is the M(e + L) above.  The floors live behind the B rows of the blob
// (nws_loudness_stream_release_state_bytes), so a row keeps the layout above; such a row carries track = 3.
#include "stft_tile.h"
#include "loudness_db.h"
#include "loudness_level.h"
#include "frame_stream.h"  // frames_done, hist_start: shared with pyin_stream.hip

namespace {

constexpr int kRing = 512;               // frames of P and M a row keeps: <= 255 waiting for their lag + <= 257 new ones
constexpr int kStepFrames = 256;         // hops of the largest chunk; a pass computes at most one frame more
constexpr int kMaxLag = 255;
constexpr long long kMaxStreamFrames = 1LL << 21;   // as the pYIN stream it is paired with (frame counters are int)

struct LoudLayout {   // byte offsets inside a row of the state blob; every part 8-byte aligned
  size_t cnt, ref, hist, mring, pring, row;
};

__host__ __device__ inline LoudLayout loud_layout(int n_fft) {
  LoudLayout l;
  l.cnt = 0;                                             // int64 n_seen, frames computed, frames emitted, finished
  l.ref = l.cnt + 4 * sizeof(long long);                 // float M, int32 track
  l.hist = l.ref + 8;                                    // float [n_fft] samples hist_start(n_seen) .. n_seen - 1
  l.mring = l.hist + (((size_t)n_fft * sizeof(float) + 7) & ~size_t(7));   // float [kRing] M(t) at t % kRing
  l.pring = l.mring + (size_t)kRing * sizeof(float);     // float [bins][kRing] P(t, k) at k kRing + t % kRing
  l.row = l.pring + (((size_t)(n_fft / 2 + 1) * kRing * sizeof(float) + 7) & ~size_t(7));
  return l;
}

// what the offline extractor serves, and a flush of at most ceil(W / hop) <= 256 frames
__host__ bool stream_ok(int n_fft, int hop) {
  return n_fft_ok(n_fft) && hop >= 1 && hop <= n_fft && tile_ok(n_fft, hop, 1) && (n_fft / 2 + hop - 1) / hop <= kStepFrames;
}

// most new frames of one pass of a step of n samples, whatever the stream has seen: n / hop + 1, met by the step that starts at
// n_seen = W (F = 0, not the 1 its closed form would give there) and computes frames 0 .. n / hop; a flush <= ceil(W / hop)
__host__ int pass_frames_bound(int n, int n_fft, int hop, int final) {
  int m = n / hop + 1;
  const int fl = (n_fft / 2 + hop - 1) / hop;
  if (final && fl > m) m = fl;
  return m;
}

__host__ size_t stream_ws_bytes(int B, int frames) { return ((size_t)B * frames * sizeof(unsigned) + 255) & ~size_t(255); }

constexpr int kTrackRelease = 3;         // the row's track word after nws_loudness_stream_reset_release: tracking, floors in the blob

// the floors F[B] of a releasing stream follow the B rows
__host__ inline size_t release_bytes(int B, int n_fft) { return (size_t)B * loud_layout(n_fft).row + (((size_t)B * sizeof(float) + 7) & ~size_t(7)); }

struct LoudPass {
  int B, n, flush, lag;
  int track;                        // the track word the caller expects of every row; -1: any
  float rho;                        // release factor, 1: none
  long long n_seen, n_total;        // samples before and after the pass
  long long hs0, hs1;               // hist_start before and after
  int f0, f1, e0, e1;               // frames computed / emitted before and after
  int out_off, out_stride;
};

__device__ __forceinline__ bool stream_state_matches(const unsigned char* rs, const LoudLayout& l, const LoudPass& g) {
  const long long* cnt = reinterpret_cast<const long long*>(rs + l.cnt);
  const int track = *reinterpret_cast<const int*>(rs + l.ref + 4);
  return cnt[0] == g.n_seen && cnt[1] == g.f0 && cnt[2] == g.e0 && cnt[3] == 0 && (g.track < 0 || track == g.track);
}

// grid (tiles of 32 new frames, groups of 4 M-tiles, B); pmax (B, f1 - f0) zeroed
__global__ __launch_bounds__(256) void loudness_stream_power_kernel(unsigned char* __restrict__ state, const float* __restrict__ x,
                                                                    LoudPass g, int n_fft, int hop, const float* __restrict__ dft,
                                                                    int m_tiles, unsigned* __restrict__ pmax) {
  extern __shared__ float xs[];  // skewed window of the frame tile
  const TileCoord c;
  const LoudLayout l = loud_layout(n_fft);
  unsigned char* rs = state + (size_t)c.b * l.row;
  if (!stream_state_matches(rs, l, g)) return;   // workgroup-uniform, in front of the barrier
  const float* hist = reinterpret_cast<const float*>(rs + l.hist);
  const float* xr = x + (size_t)c.b * g.n;
  const long long N = g.n_total;
  // position i of the padded row: reflected about 0, on a flush about N; samples that do not exist (they belong to frames this
  // pass does not compute) read as 0
  auto sample = [&](long long i) {
    if (i < 0) i = -i;
    if (g.flush && i >= N) i = 2 * (N - 1) - i;
    if (i < g.hs0 || i >= N) return 0.0f;
    return i < g.n_seen ? hist[i - g.hs0] : xr[i - g.n_seen];
  };
  tile_stage_from(sample, n_fft, hop, (long long)g.f0 + c.t0, xs);
  if (c.mt >= m_tiles) return;
  TileAcc a;
  tile_transform<1>(dft, xs, n_fft, hop, c.mt, 0, n_fft / 2, a);
  // rows (r, r+1), r even = (Re, Im) of bin tile_bin(c.mt, r, c.kh); column = frame f0 + t0 + col
  const int t = g.f0 + c.t0 + c.col;
  const int bins = n_fft / 2 + 1;
  float* pring = reinterpret_cast<float*>(rs + l.pring);
  float mx = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int bin = tile_bin(c.mt, r, c.kh);
    const float p = fmaf(a.x[r], a.x[r], a.x[r + 1] * a.x[r + 1]);
    if (bin < bins && t < g.f1) {
      pring[(size_t)bin * kRing + (t & (kRing - 1))] = p;
      mx = fmaxf(mx, p);
    }
  }
  mx = fmaxf(mx, __shfl_xor(mx, 32, 64));   // the two lane halves hold bins of the same frame
  if (c.kh == 0 && t < g.f1) atomicMax(&pmax[(size_t)c.b * (g.f1 - g.f0) + (t - g.f0)], __float_as_uint(mx));
}

__global__ __launch_bounds__(256) void loudness_stream_emit_kernel(unsigned char* __restrict__ state, const float* __restrict__ x,
                                                                   LoudPass g, int n_fft, const unsigned* __restrict__ pmax,
                                                                   float amin, float top_db, int normalise,
                                                                   const float* __restrict__ floors, float* __restrict__ loud,
                                                                   float* __restrict__ ref_out) {
  extern __shared__ float hs[];     // [n_fft] the row's new history, then [kStepFrames + 1] M of the pass's new frames
  float* sm = hs + n_fft;
  const int tid = threadIdx.x, b = blockIdx.x, bins = n_fft / 2 + 1, nf = g.f1 - g.f0;
  const LoudLayout l = loud_layout(n_fft);
  unsigned char* rs = state + (size_t)b * l.row;
  long long* cnt = reinterpret_cast<long long*>(rs + l.cnt);
  if (!stream_state_matches(rs, l, g)) return;    // workgroup-uniform, in front of every barrier
  float* Mp = reinterpret_cast<float*>(rs + l.ref);
  const int track = *reinterpret_cast<const int*>(rs + l.ref + 4);
  float* hist = reinterpret_cast<float*>(rs + l.hist);
  float* mring = reinterpret_cast<float*>(rs + l.mring);
  const float* pring = reinterpret_cast<const float*>(rs + l.pring);
  // the M ring grows by the new frames: the serial level recurrence (track) or the constant (fixed reference)
  for (int i = tid; i < nf; i += 256) sm[i] = __uint_as_float(pmax[(size_t)b * nf + i]);
  __syncthreads();
  if (tid == 0 && nf > 0) {
    float M = *Mp;
    const float F = floors ? floors[b] : 0.0f;   // read at rho < 1 only, and then it is there
    for (int i = 0; i < nf; ++i) {
      if (track) M = loudness_level_step(M, sm[i], F, g.rho);
      sm[i] = M;
    }
    *Mp = M;
  }
  __syncthreads();
  for (int i = tid; i < nf; i += 256) mring[(g.f0 + i) & (kRing - 1)] = sm[i];
  // M(t) of a frame this pass computed is in LDS, of an earlier one in the ring
  auto M_of = [&](int t) { return t >= g.f0 ? sm[t - g.f0] : mring[t & (kRing - 1)]; };
  for (int e = g.e0 + tid; e < g.e1; e += 256) {
    const int end = g.flush ? g.f1 - 1 : e + g.lag;
    float ref = M_of(end);
    if (g.rho < 1.0f)   // a decaying M is not monotone: the largest level the frame's window holds (<= 511 frames, all in LDS or ring)
      for (int t = e; t < end; ++t) ref = fmaxf(ref, M_of(t));
    const size_t o = (size_t)b * g.out_stride + g.out_off + (e - g.e0);
    loud[o] = loudness_frame_db(pring + (e & (kRing - 1)), kRing, bins, ref, amin, top_db, normalise);
    ref_out[o] = ref;
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

// after the blob was zeroed: M = initial_power of the row, track as given; floors (a releasing stream) = initial_power too
__global__ void loudness_stream_init_kernel(unsigned char* __restrict__ state, int B, size_t row, size_t ref_off,
                                            const float* __restrict__ initial_power, int track, float* __restrict__ floors) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  *reinterpret_cast<float*>(state + (size_t)b * row + ref_off) = initial_power[b];
  *reinterpret_cast<int*>(state + (size_t)b * row + ref_off + 4) = track;
  if (floors) floors[b] = initial_power[b];
}

__host__ int run_pass(unsigned char* state, const float* x, const LoudPass& g, int n_fft, int hop, const float* dft, float amin,
                      float top_db, int normalise, float* loud, float* ref_out, void* workspace, hipStream_t stream) {
  const int nf = g.f1 - g.f0;
  unsigned* pmax = static_cast<unsigned*>(workspace);
  if (nf > 0) {
    const hipError_t e = hipMemsetAsync(pmax, 0, (size_t)g.B * nf * sizeof(unsigned), stream);
    if (e != hipSuccess) return (int)e;
    const int m_tiles = rows_padded(n_fft) / 32;
    const dim3 grid((nf + kFrames - 1) / kFrames, (m_tiles + 3) / 4, g.B);
    loudness_stream_power_kernel<<<grid, 256, tile_lds_bytes(n_fft, hop, 1), stream>>>(state, x, g, n_fft, hop, dft, m_tiles, pmax);
    NWS_CHECK_LAUNCH();
  }
  const float* floors = g.rho < 1.0f ? reinterpret_cast<const float*>(state + (size_t)g.B * loud_layout(n_fft).row) : nullptr;
  loudness_stream_emit_kernel<<<g.B, 256, (size_t)(n_fft + kStepFrames + 1) * sizeof(float), stream>>>(
      state, x, g, n_fft, pmax, amin, top_db, normalise, floors, loud, ref_out);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

__host__ long long emitted_after(long long n, int n_fft, int hop, int lag, int final) {
  if (final) return 1 + n / hop;
  const long long f = frames_done(n, n_fft / 2, hop) - lag;
  return f < 0 ? 0 : f;
}

}  // namespace

extern "C" {

size_t nws_loudness_stream_state_bytes(int B, int n_fft, int hop) {
  if (B < 1 || B > 65535 || !stream_ok(n_fft, hop)) return 0;
  return (size_t)B * loud_layout(n_fft).row;
}

int nws_loudness_stream_max_chunk(int n_fft, int hop) { return stream_ok(n_fft, hop) ? kStepFrames * hop : 0; }

size_t nws_loudness_stream_workspace_bytes(int B, int n, int n_fft, int hop, int final) {
  if (B < 1 || B > 65535 || n < 0 || !stream_ok(n_fft, hop) || n > kStepFrames * hop) return 0;
  return stream_ws_bytes(B, pass_frames_bound(n, n_fft, hop, final ? 1 : 0));
}

int64_t nws_loudness_stream_frames(int64_t n_seen, int n_fft, int hop, int final) {
  if (n_seen < 0 || !stream_ok(n_fft, hop) || n_seen > kMaxStreamFrames * hop) return -1;
  if (final) return n_seen <= n_fft / 2 ? -1 : 1 + n_seen / hop;
  return frames_done(n_seen, n_fft / 2, hop);
}

int64_t nws_loudness_stream_emitted(int64_t n_seen, int n_fft, int hop, int lag, int final) {
  if (n_seen < 0 || lag < 0 || lag > kMaxLag || !stream_ok(n_fft, hop) || n_seen > kMaxStreamFrames * hop) return -1;
  if (final && n_seen <= n_fft / 2) return -1;
  return emitted_after(n_seen, n_fft, hop, lag, final ? 1 : 0);
}

size_t nws_loudness_stream_release_state_bytes(int B, int n_fft, int hop) {
  if (B < 1 || B > 65535 || !stream_ok(n_fft, hop)) return 0;
  return release_bytes(B, n_fft);
}

}  // extern "C"

namespace {

// track: 0 / 1 of nws_loudness_stream_reset, kTrackRelease of nws_loudness_stream_reset_release (the blob holds the floors then)
__host__ int reset_impl(void* state, size_t bytes, int B, int n_fft, int hop, const float* initial_power, int track, void* stream) {
  if (!state || !initial_power || B < 1) return NWS_ERR_BAD_ARG;
  if (B > 65535 || !stream_ok(n_fft, hop)) return NWS_ERR_UNSUPPORTED;
  const LoudLayout l = loud_layout(n_fft);
  const size_t rows = (size_t)B * l.row, need = track == kTrackRelease ? release_bytes(B, n_fft) : rows;
  if (bytes < need) return NWS_ERR_BAD_ARG;
  const hipError_t e = hipMemsetAsync(state, 0, need, (hipStream_t)stream);
  if (e != hipSuccess) return (int)e;
  unsigned char* st = static_cast<unsigned char*>(state);
  loudness_stream_init_kernel<<<(B + 255) / 256, 256, 0, (hipStream_t)stream>>>(
      st, B, l.row, l.ref, initial_power, track, track == kTrackRelease ? reinterpret_cast<float*>(st + rows) : nullptr);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

// track -1: whatever the rows carry (the step without a release); rho < 1 needs the floors, so kTrackRelease
__host__ int step_impl(void* state, size_t bytes, const float* x, int B, int n, int64_t n_seen, int n_fft, int hop, int lag, int track,
                       float rho, const float* dft, float amin, float top_db, int normalise, int final, float* loudness_out,
                       float* ref_out, int out_stride, void* workspace, size_t workspace_bytes, void* stream) {
  if (!state || !dft || !loudness_out || !ref_out || !workspace || B < 1 || n < 0 || n_seen < 0 || (n == 0 && !final) ||
      (n > 0 && !x) || lag < 0 || lag > kMaxLag || !(amin > 0.0f) || !(top_db >= 0.0f))
    return NWS_ERR_BAD_ARG;
  if (B > 65535 || !stream_ok(n_fft, hop) || n > kStepFrames * hop || n_seen > kMaxStreamFrames * hop - n) return NWS_ERR_UNSUPPORTED;
  const int W = n_fft / 2;
  const long long N = n_seen + n;
  if (final && N <= W) return NWS_ERR_BAD_ARG;            // reflect padding needs more than n_fft / 2 samples, as offline
  const long long e_before = emitted_after(n_seen, n_fft, hop, lag, 0), e_mid = emitted_after(N, n_fft, hop, lag, 0);
  const long long e_after = final ? emitted_after(N, n_fft, hop, lag, 1) : e_mid;
  if (out_stride < e_after - e_before) return NWS_ERR_BAD_ARG;
  if (bytes < (rho < 1.0f ? release_bytes(B, n_fft) : (size_t)B * loud_layout(n_fft).row)) return NWS_ERR_BAD_ARG;
  if (workspace_bytes < stream_ws_bytes(B, pass_frames_bound(n, n_fft, hop, final ? 1 : 0))) return NWS_ERR_BAD_ARG;
  static unsigned long long attr_devices = 0;
  if (nws_first_use_on_device(attr_devices)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(loudness_stream_power_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCap);
    if (e != hipSuccess) return (int)e;
  }
  unsigned char* st = static_cast<unsigned char*>(state);
  const int norm = normalise ? 1 : 0;
  if (n > 0) {
    const LoudPass g{B, n, 0, lag, track, rho, n_seen, N, hist_start(n_seen, W, hop), hist_start(N, W, hop), (int)frames_done(n_seen, W, hop),
                     (int)frames_done(N, W, hop), (int)e_before, (int)e_mid, 0, out_stride};
    const int rc = run_pass(st, x, g, n_fft, hop, dft, amin, top_db, norm, loudness_out, ref_out, workspace, (hipStream_t)stream);
    if (rc != NWS_OK) return rc;
  }
  if (final) {
    const long long hs = hist_start(N, W, hop);
    const LoudPass g{B, 0, 1, lag, track, rho, N, N, hs, hs, (int)frames_done(N, W, hop), (int)(1 + N / hop), (int)e_mid, (int)e_after,
                     (int)(e_mid - e_before), out_stride};
    return run_pass(st, x, g, n_fft, hop, dft, amin, top_db, norm, loudness_out, ref_out, workspace, (hipStream_t)stream);
  }
  return NWS_OK;
}

}  // namespace

extern "C" {

int nws_loudness_stream_reset(void* state, size_t bytes, int B, int n_fft, int hop, const float* initial_power, int track,
                              void* stream) {
  return reset_impl(state, bytes, B, n_fft, hop, initial_power, track ? 1 : 0, stream);
}

int nws_loudness_stream_reset_release(void* state, size_t bytes, int B, int n_fft, int hop, const float* floor_power, void* stream) {
  return reset_impl(state, bytes, B, n_fft, hop, floor_power, kTrackRelease, stream);
}

int nws_loudness_stream_step(void* state, size_t bytes, const float* x, int B, int n, int64_t n_seen, int n_fft, int hop, int lag,
                             const float* dft, float amin, float top_db, int normalise, int final, float* loudness_out,
                             float* ref_out, int out_stride, void* workspace, size_t workspace_bytes, void* stream) {
  return step_impl(state, bytes, x, B, n, n_seen, n_fft, hop, lag, -1, 1.0f, dft, amin, top_db, normalise, final, loudness_out, ref_out,
                   out_stride, workspace, workspace_bytes, stream);
}

int nws_loudness_stream_step_release(void* state, size_t bytes, const float* x, int B, int n, int64_t n_seen, int n_fft, int hop,
                                     int lag, float release_factor, int track, const float* dft, float amin, float top_db,
                                     int normalise, int final, float* loudness_out, float* ref_out, int out_stride, void* workspace,
                                     size_t workspace_bytes, void* stream) {
  if (!(release_factor > 0.0f && release_factor <= 1.0f) || (release_factor < 1.0f && !track)) return NWS_ERR_BAD_ARG;
  return step_impl(state, bytes, x, B, n, n_seen, n_fft, hop, lag, release_factor < 1.0f ? kTrackRelease : -1, release_factor, dft,
                   amin, top_db, normalise, final, loudness_out, ref_out, out_stride, workspace, workspace_bytes, stream);
}

}  // extern "C"
