// Perceptual-loudness feature (the step BEFORE the synthesis path):
//   neural_waveshaping_synthesis/data/utils/loudness_extraction.py:10-67 with gin/data/urmp_4second_crepe.gin:11-14:
//   |librosa.stft(audio, n_fft 1024, hop 128, hann, center/reflect)| -> amplitude_to_db(ref=np.max, amin=epsilon, top_db 80)
//   -> mean over bins -> (L + 80) / 80.   (The A-weighting of :25-38 is computed and then NOT applied by the reference.)
//
// Design: the windowed real DFT of every frame is ONE GEMM against a constant matrix with the hann window folded in,
//   S[row][t] = sum_n D[row][n] * x_pad[hop t + n],   rows interleaved (2k = Re, 2k+1 = Im of bin k),
// on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulate: the reference's own transform is a float32 FFT).
// A workgroup = 32 frames x 4 M-tiles; the 31 hop + n_fft samples the 32 overlapping frames are cut from are staged in LDS
// once (reflect padding resolved there), skewed by one word per 128 so that the 32 lanes of a B-operand read (stride hop)
// fall into different banks.  Re/Im of a bin are adjacent accumulator registers of one lane -> power in-lane; the
// spectrogram is kept as (B, bins, frames) so that both its write and the second pass are coalesced along frames.
// The dB reference is the maximum over the WHOLE spectrogram of an utterance: pass 1 leaves it in one word per utterance
// (atomicMax on the float bits, valid for non-negative values), pass 2 clips, averages and normalises.
#include "stft_tile.h"  // the tile, its limits and the operand's size: shared with stft_loss.hip and stft_grad.hip
#include "loudness_db.h"  // the dB pass of one frame: shared with loudness_stream.hip

namespace {

// grid (frame tiles, groups of 4 M-tiles, B).  K is the whole transform: k_lo = 0, lane half kh takes n_fft / 2 kh + s
__global__ __launch_bounds__(256) void loudness_power_kernel(const float* __restrict__ audio, int N, int n_fft, int hop,
                                                             int frames, int frames_pad, const float* __restrict__ dft,
                                                             int m_tiles, float* __restrict__ power,
                                                             unsigned* __restrict__ max_bits) {
  extern __shared__ float xs[];  // skewed window of the frame tile
  const TileCoord c;
  TileAcc a;
  if (!tile_prologue<1>(c, {audio}, N, n_fft, hop, dft, m_tiles, 0, n_fft / 2, xs, a)) return;
  // rows (r, r+1), r even = (Re, Im) of bin tile_bin(c.mt, r, c.kh); column = frame t0 + col
  const int t = c.t0 + c.col;
  const int bins = n_fft / 2 + 1;
  float mx = 0.0f;
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    const int bin = tile_bin(c.mt, r, c.kh);
    const float p = fmaf(a.x[r], a.x[r], a.x[r + 1] * a.x[r + 1]);
    if (bin < bins && t < frames) {
      power[((size_t)c.b * bins + bin) * frames_pad + t] = p;
      mx = fmaxf(mx, p);
    }
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off, 64));
  if (c.lane == 0) atomicMax(&max_bits[c.b], __float_as_uint(mx));
}

__global__ void loudness_db_kernel(const float* __restrict__ power, const unsigned* __restrict__ max_bits, int bins,
                                   int frames, int frames_pad, float amin, float top_db, int normalise,
                                   float* __restrict__ out) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int b = blockIdx.y;
  if (t >= frames) return;
  out[(size_t)b * frames + t] = loudness_frame_db(power + (size_t)b * bins * frames_pad + t, frames_pad, bins,
                                                  __uint_as_float(max_bits[b]), amin, top_db, normalise);
}

// the shared limits (stft_tile.h) for one staged signal, and hop <= n_fft: e.g. n_fft 2048 allows hop <= 1250, n_fft 1024 hop <= 1024
__host__ bool fft_ok(int n_fft, int hop) { return n_fft_ok(n_fft) && hop <= n_fft && tile_ok(n_fft, hop, 1); }

}  // namespace

extern "C" {

size_t nws_loudness_dft_bytes(int n_fft) {
  if (!fft_ok(n_fft, 1)) return 0;
  return dft_operand_bytes(n_fft);
}

// the operand of the STFT loss (stft_loss.hip holds the kernel) with the hann window as long as the transform
int nws_loudness_dft_matrix(int n_fft, float* dft_out, void* stream) {
  if (!fft_ok(n_fft, 1) || !dft_out) return NWS_ERR_BAD_ARG;
  return nws_stft_loss_dft_matrix(n_fft, n_fft, dft_out, stream);
}

int nws_loudness_frames(int N, int hop) { return (N <= 0 || hop <= 0) ? 0 : frames_of(N, hop); }

size_t nws_loudness_workspace_bytes(int B, int N, int n_fft, int hop) {
  if (B <= 0 || N <= 0 || !fft_ok(n_fft, hop)) return 0;
  const size_t frames_pad = ((size_t)nws_loudness_frames(N, hop) + 31) / 32 * 32;
  return ((size_t)B * (n_fft / 2 + 1) * frames_pad) * sizeof(float) + (((size_t)B * sizeof(unsigned) + 255) & ~size_t(255));
}

// The power pass alone: power (B, bins, frames_pad) and the per-utterance maximum of it as float bits (max_bits (B), zeroed
// here).  The caller has checked the sizes (nws_loudness_workspace_bytes != 0, N > n_fft / 2).  Shared with mfcc.hip.
int nws_stft_power_pass(const float* audio, int B, int N, int n_fft, int hop, const float* dft, float* power,
                        unsigned* max_bits, void* stream) {
  const int frames = nws_loudness_frames(N, hop);
  const int frames_pad = (frames + 31) / 32 * 32;
  hipStream_t st = (hipStream_t)stream;
  hipError_t e = hipMemsetAsync(max_bits, 0, (size_t)B * sizeof(unsigned), st);
  if (e != hipSuccess) return (int)e;
  const int m_tiles = rows_padded(n_fft) / 32;
  const size_t lds = tile_lds_bytes(n_fft, hop, 1);
  static unsigned long long attr_devices = 0;
  if (nws_first_use_on_device(attr_devices)) {
    e = hipFuncSetAttribute(reinterpret_cast<const void*>(loudness_power_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                            (int)kLdsCap);
    if (e != hipSuccess) return (int)e;
  }
  const dim3 grid(frames_pad / kFrames, (m_tiles + 3) / 4, B);
  loudness_power_kernel<<<grid, 256, lds, st>>>(audio, N, n_fft, hop, frames, frames_pad, dft, m_tiles, power, max_bits);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

int nws_loudness(const float* audio, int B, int N, int n_fft, int hop, const float* dft, float amin, float top_db,
                 int normalise, float* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (!audio || !dft || !out || !workspace || B <= 0 || !fft_ok(n_fft, hop)) return NWS_ERR_BAD_ARG;
  if (N <= n_fft / 2) return NWS_ERR_BAD_ARG;  // reflect padding needs more than n_fft/2 samples (as in the reference)
  if (!(amin > 0.0f) || !(top_db >= 0.0f)) return NWS_ERR_BAD_ARG;
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  if (workspace_bytes < nws_loudness_workspace_bytes(B, N, n_fft, hop)) return NWS_ERR_WORKSPACE;
  const int frames = nws_loudness_frames(N, hop);
  const int frames_pad = (frames + 31) / 32 * 32;
  const int bins = n_fft / 2 + 1;
  const size_t max_bytes = ((size_t)B * sizeof(unsigned) + 255) & ~size_t(255);
  unsigned* max_bits = static_cast<unsigned*>(workspace);
  float* power = reinterpret_cast<float*>(static_cast<char*>(workspace) + max_bytes);
  hipStream_t st = (hipStream_t)stream;
  const int rc = nws_stft_power_pass(audio, B, N, n_fft, hop, dft, power, max_bits, stream);
  if (rc != NWS_OK) return rc;
  const dim3 g2((frames + 255) / 256, B);
  loudness_db_kernel<<<g2, 256, 0, st>>>(power, max_bits, bins, frames, frames_pad, amin, top_db, normalise, out);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

// The power pass alone, handed out as power_out (B) floats: the clip maximum nws_loudness normalises by.  A loudness stream with
// this value as its fixed reference is nws_loudness of the clip; measured on a sound check it is a calibration.
int nws_loudness_peak_power(const float* audio, int B, int N, int n_fft, int hop, const float* dft, float* power_out,
                            void* workspace, size_t workspace_bytes, void* stream) {
  if (!audio || !dft || !power_out || !workspace || B <= 0 || !fft_ok(n_fft, hop)) return NWS_ERR_BAD_ARG;
  if (N <= n_fft / 2) return NWS_ERR_BAD_ARG;
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  if (workspace_bytes < nws_loudness_workspace_bytes(B, N, n_fft, hop)) return NWS_ERR_WORKSPACE;
  const size_t max_bytes = ((size_t)B * sizeof(unsigned) + 255) & ~size_t(255);
  unsigned* max_bits = static_cast<unsigned*>(workspace);
  float* power = reinterpret_cast<float*>(static_cast<char*>(workspace) + max_bytes);
  const int rc = nws_stft_power_pass(audio, B, N, n_fft, hop, dft, power, max_bits, stream);
  if (rc != NWS_OK) return rc;
  const hipError_t e = hipMemcpyAsync(power_out, max_bits, (size_t)B * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream);
  return e == hipSuccess ? NWS_OK : (int)e;
}

}  // extern "C"
