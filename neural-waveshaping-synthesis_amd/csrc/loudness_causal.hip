// Whole-clip extractor of the loudness stream's feature: what the concatenated pushes of a loudness stream
// (loudness_stream.hip) give for a clip, computed in one call, bit for bit, whatever the chunking would have been.  A dataset built
// with it measures every frame against the reference the live chain will use, not against the peak of the whole clip.
//
// Four stages on the caller's stream:
//   nws_stft_power_pass             loudness.hip's: P (B, bins, frames_pad), the bits the stream's power kernel writes
//   loudness_causal_peak_kernel     one thread per frame: p(t) = max_k P(t, k)  -> peak_out (B, T)
//   loudness_causal_level_kernel    one workgroup per row: p staged through LDS in blocks of kLevelBlock, one lane runs the serial
//                                   recurrence of loudness_level.h (M(-1) = F), M (B, T) into the workspace
//   loudness_causal_db_kernel       one thread per frame: ref(e) = max of M over e .. e + L for e < F(N) - L, over e .. T - 1 for the
//                                   frames a flush releases, then the dB pass of loudness_db.h against that frame's own reference
// Without `track` M = F, the fixed reference of 3.25.
#include "loudness_db.h"
#include "loudness_level.h"
#include "frame_stream.h"  // frames_done: the stream's flush boundary

namespace {

constexpr int kLevelBlock = 1024;
constexpr int kMaxLag = 255;

__global__ void loudness_causal_peak_kernel(const float* __restrict__ power, int bins, int frames, int frames_pad,
                                            float* __restrict__ peak) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= frames) return;
  const float* p = power + (size_t)b * bins * frames_pad + t;
  float mx = 0.0f;
  for (int k = 0; k < bins; ++k) mx = fmaxf(mx, p[(size_t)k * frames_pad]);
  peak[(size_t)b * frames + t] = mx;
}

__global__ __launch_bounds__(256) void loudness_causal_level_kernel(const float* __restrict__ peak, int frames,
                                                                    const float* __restrict__ floors, int track, float rho,
                                                                    float* __restrict__ level) {
  __shared__ float sm[kLevelBlock];
  const int tid = threadIdx.x, b = blockIdx.x;
  const float F = floors ? floors[b] : 0.0f;
  float M = F;   // lane 0's, carried from block to block
  for (int t0 = 0; t0 < frames; t0 += kLevelBlock) {
    const int n = min(kLevelBlock, frames - t0);
    for (int i = tid; i < n; i += 256) sm[i] = peak[(size_t)b * frames + t0 + i];
    __syncthreads();
    if (tid == 0) {
      for (int i = 0; i < n; ++i) {
        if (track) M = loudness_level_step(M, sm[i], F, rho);
        sm[i] = M;
      }
    }
    __syncthreads();
    for (int i = tid; i < n; i += 256) level[(size_t)b * frames + t0 + i] = sm[i];
    __syncthreads();
  }
}

// frames e < released take the window that ends at e + lag, the others the one that ends at the clip's last frame
__global__ void loudness_causal_db_kernel(const float* __restrict__ power, const float* __restrict__ level, int bins, int frames,
                                          int frames_pad, int lag, int released, float rho, float amin, float top_db, int normalise,
                                          float* __restrict__ out, float* __restrict__ ref_out) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (e >= frames) return;
  const float* M = level + (size_t)b * frames;
  const int end = e < released ? e + lag : frames - 1;
  float ref = M[end];
  if (rho < 1.0f)
    for (int t = e; t < end; ++t) ref = fmaxf(ref, M[t]);
  out[(size_t)b * frames + e] = loudness_frame_db(power + (size_t)b * bins * frames_pad + e, frames_pad, bins, ref, amin, top_db,
                                                  normalise);
  ref_out[(size_t)b * frames + e] = ref;
}

__host__ size_t level_bytes(int B, int frames) { return ((size_t)B * frames * sizeof(float) + 255) & ~size_t(255); }

// what nws_loudness serves and the stream serves: its sizes (at most 256 hops in half a frame) and its length (2^21 hops)
__host__ bool causal_ok(int B, int N, int n_fft, int hop) {
  return B >= 1 && B <= 65535 && N >= 1 && nws_loudness_stream_state_bytes(1, n_fft, hop) != 0 &&
         nws_loudness_stream_frames(N, n_fft, hop, 0) >= 0 && nws_loudness_workspace_bytes(B, N, n_fft, hop) != 0;
}

}  // namespace

extern "C" {

size_t nws_loudness_causal_workspace_bytes(int B, int N, int n_fft, int hop) {
  if (!causal_ok(B, N, n_fft, hop)) return 0;
  return nws_loudness_workspace_bytes(B, N, n_fft, hop) + level_bytes(B, nws_loudness_frames(N, hop));
}

int nws_loudness_causal(const float* audio, int B, int N, int n_fft, int hop, const float* dft, int lag, float release_factor,
                        const float* floor_power, int track, float amin, float top_db, int normalise, float* loudness_out,
                        float* ref_out, float* peak_out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!audio || !dft || !loudness_out || !ref_out || !peak_out || !workspace || B <= 0) return NWS_ERR_BAD_ARG;
  if (nws_loudness_workspace_bytes(1, 1, n_fft, hop) == 0) return NWS_ERR_BAD_ARG;      // as nws_loudness
  if (N <= n_fft / 2) return NWS_ERR_BAD_ARG;
  if (!(amin > 0.0f) || !(top_db >= 0.0f)) return NWS_ERR_BAD_ARG;
  if (lag < 0 || lag > kMaxLag) return NWS_ERR_BAD_ARG;
  if (!(release_factor > 0.0f && release_factor <= 1.0f) || (release_factor < 1.0f && !track)) return NWS_ERR_BAD_ARG;
  if (!track && !floor_power) return NWS_ERR_BAD_ARG;                                   // a fixed reference has to be given
  if (!causal_ok(B, N, n_fft, hop)) return NWS_ERR_UNSUPPORTED;
  if (workspace_bytes < nws_loudness_causal_workspace_bytes(B, N, n_fft, hop)) return NWS_ERR_WORKSPACE;
  const int frames = nws_loudness_frames(N, hop);
  const int frames_pad = (frames + 31) / 32 * 32;
  const int bins = n_fft / 2 + 1;
  const size_t max_bytes = ((size_t)B * sizeof(unsigned) + 255) & ~size_t(255);
  char* ws = static_cast<char*>(workspace);
  unsigned* max_bits = reinterpret_cast<unsigned*>(ws);
  float* power = reinterpret_cast<float*>(ws + max_bytes);
  float* level = reinterpret_cast<float*>(ws + nws_loudness_workspace_bytes(B, N, n_fft, hop));
  hipStream_t st = (hipStream_t)stream;
  const int rc = nws_stft_power_pass(audio, B, N, n_fft, hop, dft, power, max_bits, stream);
  if (rc != NWS_OK) return rc;
  const dim3 grid((frames + 255) / 256, B);
  loudness_causal_peak_kernel<<<grid, 256, 0, st>>>(power, bins, frames, frames_pad, peak_out);
  NWS_CHECK_LAUNCH();
  loudness_causal_level_kernel<<<B, 256, 0, st>>>(peak_out, frames, floor_power, track ? 1 : 0, release_factor, level);
  NWS_CHECK_LAUNCH();
  const long long released = frames_done(N, n_fft / 2, hop) - lag;      // the frames that leave before the flush
  loudness_causal_db_kernel<<<grid, 256, 0, st>>>(power, level, bins, frames, frames_pad, lag, released < 0 ? 0 : (int)released,
                                                  release_factor, amin, top_db, normalise ? 1 : 0, loudness_out, ref_out);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

}  // extern "C"
