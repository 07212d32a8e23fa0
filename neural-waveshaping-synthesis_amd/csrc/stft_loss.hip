// Multi-resolution STFT loss: the number the reference logs as val/loss and test/loss
//   (models/neural_waveshaping.py:93, 104-112, 136-165: auraloss.freq.MultiResolutionSTFTLoss()(recon, audio), auraloss 0.2.1).
//   DESIGN.md 3.12 holds the definition the kernels are tested against; parity with auraloss itself is unpinned.
//
// Per resolution (n_fft, hop, win_length): torch.stft (periodic hann of win_length centred in n_fft, centre / reflect padding,
// 1 + N / hop frames) of x and of y, mag = sqrt(max(re^2 + im^2, eps)), and four sums over the whole (B, bins, frames) array:
//   sum (y_mag - x_mag)^2, sum y_mag^2, sum |ln x_mag - ln y_mag|, sum |x_mag - y_mag|.
//
// Three kernels:
//   stft_loss_dft_kernel       the constant operand, the only builder of it (nws_loudness_dft_matrix asks for win_length = n_fft):
//                              rows 2k / 2k+1 = w[n] cos / -w[n] sin of bin k in plain row-major order, evaluated in double with
//                              exact phase reduction, w = the periodic hann window of win_length centred in n_fft, zero outside
//                              it; rows beyond 2 (n_fft/2 + 1) are zero.
//   stft_loss_kernel           (the tile itself lives in stft_tile.h, which loudness.hip and stft_grad.hip share)
//                              32 frames x 4 M-tiles per workgroup, skewed LDS staging with reflect padding resolved there,
//                              v_mfma_f32_32x32x2_f32, with BOTH signals staged and two
//                              accumulator sets fed by one A operand.  The K loop runs over the columns the window covers only
//                              (rounded out to 16): 59 / 59 / 47 % of K at the defaults.  Re / Im of a bin are adjacent
//                              accumulator registers of one lane, so both magnitudes are formed in-lane; the four sums are
//                              reduced lane -> wave -> workgroup in fp64 in a fixed order and ONE record of four doubles per
//                              workgroup goes to memory.  No spectrogram is written.
//   stft_loss_finalise_kernel  one workgroup: the records of each resolution summed in a fixed order in fp64, then sc / log /
//                              lin, the weighted sum per resolution and the mean over resolutions.
// No atomics: two calls on the same inputs give the same bits.  Nothing is read back: the call only enqueues.
//
// Limits: n_fft a power of two in [64, 2048]; both tiles of 31 hop + n_fft samples (+ skew words) within 160 KB of LDS
// (n_fft 2048: hop <= 589, n_fft 1024: hop <= 622); B <= 65535; at most 8 resolutions.
#include "stft_tile.h"  // the tile, its limits and the refusals: shared with stft_grad.hip

namespace {

__global__ void stft_loss_dft_kernel(int n_fft, int win_length, int rows_pad, float* __restrict__ out) {
  const long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (long long)rows_pad * n_fft) return;
  const int row = (int)(e / n_fft), n = (int)(e - (long long)row * n_fft);
  const int k = row >> 1;
  const int m = n - (n_fft - win_length) / 2;  // position inside the centred window (torch.stft pads the window on both sides)
  float v = 0.0f;
  if (k <= n_fft / 2 && m >= 0 && m < win_length) {
    const double w = 0.5 - 0.5 * cospi(2.0 * (double)m / (double)win_length);  // periodic hann
    const long long kn = ((long long)k * n) % n_fft;                           // exact phase reduction
    double s, c;
    sincospi(2.0 * (double)kn / (double)n_fft, &s, &c);
    v = (float)((row & 1) ? -w * s : w * c);
  }
  out[e] = v;
}

// grid (frame tiles, groups of 4 M-tiles, B).  K runs over [k_lo, k_lo + 2 k_half): lane half kh takes k_lo + k_half kh + s.
__global__ __launch_bounds__(256) void stft_loss_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int n_fft,
                                                        int hop, int frames, const float* __restrict__ dft, int m_tiles, int k_lo,
                                                        int k_half, float eps, double* __restrict__ partials) {
  extern __shared__ __align__(16) float lds[];  // skewed windows of the frame tile: x, then y
  const TileCoord c;
  TileAcc a;
  double s_sc = 0.0, s_y2 = 0.0, s_log = 0.0, s_lin = 0.0;
  if (tile_prologue<2>(c, {x, y}, N, n_fft, hop, dft, m_tiles, k_lo, k_half, lds, a)) {
    // rows (r, r+1), r even = (Re, Im) of bin tile_bin(c.mt, r, c.kh); column = frame t0 + col
    const int bins = n_fft / 2 + 1;
    const bool frame_ok = c.t0 + c.col < frames;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      if (tile_bin(c.mt, r, c.kh) < bins && frame_ok) {
        const float xm = sqrtf(fmaxf(fmaf(a.x[r], a.x[r], a.x[r + 1] * a.x[r + 1]), eps));  // the clamp is on the power
        const float ym = sqrtf(fmaxf(fmaf(a.y[r], a.y[r], a.y[r + 1] * a.y[r + 1]), eps));
        const float d = ym - xm;
        s_sc += (double)d * (double)d;
        s_y2 += (double)ym * (double)ym;
        s_log += (double)fabsf(logf(xm) - logf(ym));
        s_lin += (double)fabsf(d);
      }
    }
  }
  double s[4] = {s_sc, s_y2, s_log, s_lin};
  tile_reduce(c, s, lds, partials);
}

struct FinaliseArgs {
  int R;
  unsigned long long rec_off[kMaxRes], rec_n[kMaxRes];  // records of resolution r: [rec_off, rec_off + rec_n)
  double count[kMaxRes];                                // B bins frames
  double w_sc, w_log, w_lin;
};

// out[0] = loss, out[1 + 3 r + (0, 1, 2)] = (sc_r, log_r, lin_r)
__global__ __launch_bounds__(256) void stft_loss_finalise_kernel(const double* __restrict__ partials, FinaliseArgs a,
                                                                 float* __restrict__ out) {
  __shared__ double red[4][256];
  const int tid = threadIdx.x;
  double total = 0.0;
  for (int r = 0; r < a.R; ++r) {
    records_sum(partials + 4 * a.rec_off[r], a.rec_n[r], red);
    if (tid == 0) {
      const double sc = sqrt(red[0][0]) / sqrt(red[1][0]);  // ||y_mag - x_mag||_F / ||y_mag||_F
      const double lg = red[2][0] / a.count[r], ln = red[3][0] / a.count[r];
      out[1 + 3 * r] = (float)sc;
      out[2 + 3 * r] = (float)lg;
      out[3 + 3 * r] = (float)ln;
      total += a.w_sc * sc + a.w_log * lg + a.w_lin * ln;
    }
    __syncthreads();
  }
  if (tid == 0) out[0] = (float)(total / (double)a.R);
}

}  // namespace

extern "C" {

size_t nws_stft_loss_dft_bytes(int n_fft, int win_length) {
  if (!n_fft_ok(n_fft) || win_length < 1 || win_length > n_fft) return 0;
  return dft_operand_bytes(n_fft);
}

int nws_stft_loss_dft_matrix(int n_fft, int win_length, float* dft_out, void* stream) {
  if (!dft_out || win_length < 1 || win_length > n_fft) return NWS_ERR_BAD_ARG;
  if (!n_fft_ok(n_fft)) return NWS_ERR_UNSUPPORTED;
  const long long n = (long long)rows_padded(n_fft) * n_fft;
  stft_loss_dft_kernel<<<(unsigned)((n + 255) / 256), 256, 0, (hipStream_t)stream>>>(n_fft, win_length, rows_padded(n_fft), dft_out);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

size_t nws_stft_loss_workspace_bytes(int B, int N, int R, const int* n_ffts, const int* hops) {
  if (check_sizes(B, N, R, n_ffts, hops, nullptr) != NWS_OK) return 0;
  unsigned long long records = 0;
  for (int r = 0; r < R; ++r) records += grid_of(B, N, n_ffts[r], hops[r]).records;
  return (size_t)records * 4 * sizeof(double);
}

int nws_stft_loss(const float* x, const float* y, int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths,
                  const float* const* dfts, float w_sc, float w_log_mag, float w_lin_mag, float eps, float* out, void* workspace,
                  size_t workspace_bytes, void* stream) {
  if (!x || !y || !win_lengths || !dfts || !out || !workspace) return NWS_ERR_BAD_ARG;
  const int rc = check_sizes(B, N, R, n_ffts, hops, win_lengths);
  if (rc != NWS_OK) return rc;
  for (int r = 0; r < R; ++r)
    if (!dfts[r]) return NWS_ERR_BAD_ARG;
  if (!(eps > 0.0f)) return NWS_ERR_BAD_ARG;
  if (workspace_bytes < nws_stft_loss_workspace_bytes(B, N, R, n_ffts, hops)) return NWS_ERR_WORKSPACE;

  hipStream_t st = (hipStream_t)stream;
  static unsigned long long attr_devices = 0;
  if (nws_first_use_on_device(attr_devices)) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(stft_loss_kernel),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCap);
    if (e != hipSuccess) return (int)e;
  }
  double* partials = static_cast<double*>(workspace);
  FinaliseArgs fa;
  fa.R = R;
  fa.w_sc = (double)w_sc, fa.w_log = (double)w_log_mag, fa.w_lin = (double)w_lin_mag;
  unsigned long long off = 0;
  for (int r = 0; r < kMaxRes; ++r) fa.rec_off[r] = fa.rec_n[r] = 0, fa.count[r] = 1.0;
  for (int r = 0; r < R; ++r) {
    const int n_fft = n_ffts[r], hop = hops[r], win = win_lengths[r];
    const Grid g = grid_of(B, N, n_fft, hop);
    const KRange k = k_range_of(n_fft, win);
    stft_loss_kernel<<<dim3(g.gx, g.gy, (unsigned)B), 256, tile_lds_bytes(n_fft, hop, 2), st>>>(
        x, y, N, n_fft, hop, frames_of(N, hop), dfts[r], rows_padded(n_fft) / 32, k.k_lo, k.k_len / 2, eps, partials + 4 * off);
    NWS_CHECK_LAUNCH();
    fa.rec_off[r] = off;
    fa.rec_n[r] = g.records;
    fa.count[r] = (double)B * (double)(n_fft / 2 + 1) * (double)frames_of(N, hop);
    off += g.records;
  }
  stft_loss_finalise_kernel<<<1, 256, 0, st>>>(partials, fa, out);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

}  // extern "C"
