// The STFT tile of the multi-resolution loss, shared by its forward (stft_loss.hip) and its gradient (stft_grad.hip):
// 32 frames x 4 M-tiles per workgroup of 256 threads, the 31 hop + n_fft samples of the frame tile of BOTH signals staged once
// in skewed LDS with the reflect padding resolved there, v_mfma_f32_32x32x2_f32 with two accumulator sets fed by one A operand,
// K over the columns the centred window covers only.  Also the host side both entry points decide their refusals with.
#pragma once
#include "nws_common.h"

namespace {

constexpr int kFrames = 32;  // frames per workgroup (MFMA N)
constexpr int kMaxRes = NWS_STFT_LOSS_MAX_RES;
constexpr size_t kLdsCap = 160 * 1024;

__device__ __forceinline__ int reflect_index(long long i, int N) {  // numpy / torch "reflect" (no edge repeat), one fold each side
  if (i < 0) i = -i;
  if (i >= N) i = 2LL * (N - 1) - i;
  return (int)(i < 0 ? 0 : i);
}

__device__ __forceinline__ int skew(int j) { return j + (j >> 7); }

// words of one staged signal: the tile's span + skew words
__device__ __forceinline__ int tile_words(int n_fft, int hop) {
  const int span = (kFrames - 1) * hop + n_fft;
  return span + (span >> 7) + 1;
}

// every thread of the workgroup: rows xr, yr of the two signals -> xs, ys (tile_words apart), frames t0 .. t0 + 31; ends in a barrier
__device__ __forceinline__ void tile_stage(const float* __restrict__ xr, const float* __restrict__ yr, int N, int n_fft, int hop, int t0,
                                           float* xs, float* ys) {
  const int span = (kFrames - 1) * hop + n_fft;
  const long long first = (long long)hop * t0 - n_fft / 2;  // center=True: frame t covers [hop t - n_fft/2, hop t + n_fft/2)
  for (int j = threadIdx.x; j < span; j += 256) {
    const int i = reflect_index(first + j, N);
    xs[skew(j)] = xr[i];
    ys[skew(j)] = yr[i];
  }
  __syncthreads();
}

// one wave: M-tile mt of both transforms.  K runs over [k_lo, k_lo + 2 k_half): lane half kh takes k_lo + k_half kh + s.
// rows (r, r+1), r even, of ax / ay = (Re, Im) of bin tile_bin(mt, r, kh); column = frame t0 + (lane & 31)
__device__ __forceinline__ void tile_transform(const float* __restrict__ dft, const float* xs, const float* ys, int n_fft, int hop,
                                               int mt, int k_lo, int k_half, f32x16& ax, f32x16& ay) {
  const int lane = threadIdx.x & 63, kh = lane >> 5, col = lane & 31;
  const float* arow = dft + (size_t)(32 * mt + col) * n_fft + k_lo + k_half * kh;
  const int boff = hop * col + k_lo + k_half * kh;
  for (int s0 = 0; s0 < k_half; s0 += 8) {
    const float4 a0 = *reinterpret_cast<const float4*>(arow + s0), a1 = *reinterpret_cast<const float4*>(arow + s0 + 4);
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = skew(boff + s0 + i);
      ax = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], xs[j], ax, 0, 0, 0);
      ay = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], ys[j], ay, 0, 0, 0);
    }
  }
}

__device__ __forceinline__ int tile_bin(int mt, int r, int kh) { return 16 * mt + ((r & 3) >> 1) + 4 * (r >> 2) + 2 * kh; }

__host__ int rows_padded(int n_fft) { return ((2 * (n_fft / 2 + 1)) + 31) / 32 * 32; }
__host__ bool n_fft_ok(int n_fft) { return n_fft >= 64 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0; }
// LDS of one workgroup: the 31 hop + n_fft samples its 32 overlapping frames are cut from (+ skew words), for BOTH signals
__host__ size_t tile_lds_bytes(int n_fft, int hop) {
  const size_t span = (size_t)(kFrames - 1) * hop + n_fft;
  return 2 * (span + (span >> 7) + 1) * sizeof(float);
}
__host__ bool tile_ok(int n_fft, int hop) { return hop >= 1 && tile_lds_bytes(n_fft, hop) <= kLdsCap; }
__host__ int frames_of(int N, int hop) { return 1 + N / hop; }

struct Grid {
  unsigned gx, gy;
  unsigned long long records;
};
__host__ Grid grid_of(int B, int N, int n_fft, int hop) {
  Grid g;
  g.gx = (unsigned)((frames_of(N, hop) + kFrames - 1) / kFrames);
  g.gy = (unsigned)((rows_padded(n_fft) / 32 + 3) / 4);
  g.records = (unsigned long long)B * g.gy * g.gx;
  return g;
}

// the columns the centred window covers, rounded out to a multiple of 16 that starts on a multiple of 4 (float4 loads of A)
struct KRange {
  int k_lo, k_len;
};
__host__ KRange k_range_of(int n_fft, int win) {
  KRange k;
  k.k_lo = ((n_fft - win) / 2) & ~3;
  k.k_len = ((n_fft - win) / 2 + win - k.k_lo + 15) & ~15;
  if (k.k_lo + k.k_len > n_fft) k.k_lo = n_fft - k.k_len;
  return k;
}

// NWS_OK, or why the sizes are refused; nothing here touches the device
__host__ int check_sizes(int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths) {
  if (!n_ffts || !hops || B < 1 || N < 1 || R < 1 || R > kMaxRes) return NWS_ERR_BAD_ARG;
  for (int r = 0; r < R; ++r) {
    if (hops[r] < 1) return NWS_ERR_BAD_ARG;
    if (win_lengths && (win_lengths[r] < 1 || win_lengths[r] > n_ffts[r])) return NWS_ERR_BAD_ARG;
    if (!n_fft_ok(n_ffts[r])) return NWS_ERR_UNSUPPORTED;
    if (N <= n_ffts[r] / 2) return NWS_ERR_BAD_ARG;  // reflect padding needs more than n_fft/2 samples (as in torch.stft)
    if (!tile_ok(n_ffts[r], hops[r])) return NWS_ERR_UNSUPPORTED;
  }
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  return NWS_OK;
}

}  // namespace
