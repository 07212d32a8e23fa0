// The STFT tile, the only one: shared by the loudness / MFCC power pass (loudness.hip, one signal) and by the multi-resolution
// loss and its gradient (stft_loss.hip, stft_grad.hip, two signals):
// 32 frames x 4 M-tiles per workgroup of 256 threads, the 31 hop + n_fft samples of the frame tile of every signal staged once
// in skewed LDS with the reflect padding resolved there, v_mfma_f32_32x32x2_f32 with one accumulator set per signal fed by one
// A operand, K over the columns the centred window covers only.  Also the fixed-order fp64 reductions of the loss kernels and
// the host side every entry point decides its refusals with.
#pragma once
#include "nws_common.h"

namespace {

constexpr int kFrames = 32;  // frames per workgroup (MFMA N)
constexpr int kMaxRes = NWS_STFT_LOSS_MAX_RES;
constexpr size_t kLdsCap = 160 * 1024;

// one word per 128 so that the 32 lanes of a B-operand read (stride hop) fall into different banks
__device__ __forceinline__ int skew(int j) { return j + (j >> 7); }

// words of one staged signal: the tile's span + skew words
__device__ __forceinline__ int tile_words(int n_fft, int hop) {
  const int span = (kFrames - 1) * hop + n_fft;
  return span + (span >> 7) + 1;
}

// every thread of the workgroup: rows[s] of the S (1 or 2) signals -> lds + s tile_words, frames t0 .. t0 + 31; ends in a barrier
template <int S>
__device__ __forceinline__ void tile_stage(const float* const (&rows)[S], int N, int n_fft, int hop, int t0, float* lds) {
  static_assert(S == 1 || S == 2, "one or two signals");
  const int span = (kFrames - 1) * hop + n_fft;
  float* xs = lds;
  float* ys = lds + tile_words(n_fft, hop);
  const long long first = (long long)hop * t0 - n_fft / 2;  // center=True: frame t covers [hop t - n_fft/2, hop t + n_fft/2)
  for (int j = threadIdx.x; j < span; j += 256) {
    const int i = reflect_index(first + j, N);
    xs[skew(j)] = rows[0][i];
    if constexpr (S == 2) ys[skew(j)] = rows[1][i];
  }
  __syncthreads();
}

// The same tile of ONE signal that is not a row in memory: sample(i) is position i of the padded row (a stream's
// [history | chunk], with the reflections resolved by the caller and 0 where a sample does not exist yet); frames t0 .. t0 + 31.
// Every thread of the workgroup; ends in a barrier.  tile_transform<1> reads what this leaves exactly as it reads tile_stage's.
template <class Sample>
__device__ __forceinline__ void tile_stage_from(Sample sample, int n_fft, int hop, long long t0, float* lds) {
  const int span = (kFrames - 1) * hop + n_fft;
  const long long first = (long long)hop * t0 - n_fft / 2;
  for (int j = threadIdx.x; j < span; j += 256) lds[skew(j)] = sample(first + j);
  __syncthreads();
}

// the accumulators of a wave's M-tile: x of the first signal, y of the second (S == 2 only).  Two named vectors: the compiler
// keeps an ARRAY of accumulators apart less well (the K loop then comes out scheduled differently)
struct TileAcc {
  f32x16 x = {}, y = {};
};

// one wave: M-tile mt of the S transforms.  K runs over [k_lo, k_lo + 2 k_half): lane half kh takes k_lo + k_half kh + s.
// rows (r, r+1), r even, of acc.x / acc.y = (Re, Im) of bin tile_bin(mt, r, kh) of the signal; column = frame t0 + (lane & 31)
template <int S>
__device__ __forceinline__ void tile_transform(const float* __restrict__ dft, const float* lds, int n_fft, int hop, int mt, int k_lo,
                                               int k_half, TileAcc& acc) {
  static_assert(S == 1 || S == 2, "one or two signals");
  const int lane = threadIdx.x & 63, kh = lane >> 5, col = lane & 31;
  const float* xs = lds;
  const float* ys = lds + tile_words(n_fft, hop);
  const float* arow = dft + (size_t)(32 * mt + col) * n_fft + k_lo + k_half * kh;
  const int boff = hop * col + k_lo + k_half * kh;
  for (int s0 = 0; s0 < k_half; s0 += 8) {
    const float4 a0 = *reinterpret_cast<const float4*>(arow + s0), a1 = *reinterpret_cast<const float4*>(arow + s0 + 4);
    const float av[8] = {a0.x, a0.y, a0.z, a0.w, a1.x, a1.y, a1.z, a1.w};
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const int j = skew(boff + s0 + i);
      acc.x = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], xs[j], acc.x, 0, 0, 0);
      if constexpr (S == 2) acc.y = __builtin_amdgcn_mfma_f32_32x32x2f32(av[i], ys[j], acc.y, 0, 0, 0);
    }
  }
}

__device__ __forceinline__ int tile_bin(int mt, int r, int kh) { return 16 * mt + ((r & 3) >> 1) + 4 * (r >> 2) + 2 * kh; }

// A thread's place in the grid (frame tiles, groups of 4 M-tiles, B) every tile kernel is launched on
struct TileCoord {
  int tid, lane, wave, kh, col, t0, mt, b;
  __device__ __forceinline__ TileCoord()
      : tid(threadIdx.x), lane(tid & 63), wave(tid >> 6), kh(lane >> 5), col(lane & 31), t0(blockIdx.x * kFrames),
        mt(blockIdx.y * 4 + wave), b(blockIdx.z) {}
  // the workgroup's record in a (B, M-tile groups, frame tiles) array
  __device__ __forceinline__ size_t record() const { return ((size_t)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x; }
};

// The prologue of a tile kernel: rows b of the S signals (B, N) staged in lds (tile_lds_bytes), then M-tile c.mt of their transforms
// in acc, which the caller has zeroed.  false: the wave has no M-tile (it took part in the staging and its barrier; acc untouched)
template <int S>
__device__ __forceinline__ bool tile_prologue(const TileCoord& c, const float* const (&signals)[S], int N, int n_fft, int hop,
                                              const float* __restrict__ dft, int m_tiles, int k_lo, int k_half, float* lds,
                                              TileAcc& acc) {
  const float* rows[S];
#pragma unroll
  for (int s = 0; s < S; ++s) rows[s] = signals[s] + (size_t)c.b * N;
  tile_stage(rows, N, n_fft, hop, c.t0, lds);
  if (c.mt >= m_tiles) return false;
  tile_transform<S>(dft, lds, n_fft, hop, c.mt, k_lo, k_half, acc);
  return true;
}

// The Q sums of a tile kernel's threads -> the workgroup's record of Q doubles in records, in a fixed order: lanes by
// __shfl_xor 32 .. 1, then the four waves as ((w0 + w1) + w2) + w3 through the first 32 Q bytes of lds, which every wave is done
// with (a barrier comes first)
template <int Q>
__device__ __forceinline__ void tile_reduce(const TileCoord& c, double (&s)[Q], float* lds, double* __restrict__ records) {
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] += __shfl_xor(s[q], off, 64);
  }
  __syncthreads();
  double* red = reinterpret_cast<double*>(lds);
  if (c.lane == 0) {
#pragma unroll
    for (int q = 0; q < Q; ++q) red[Q * c.wave + q] = s[q];
  }
  __syncthreads();
  if (c.tid < Q) records[Q * c.record() + c.tid] = ((red[c.tid] + red[Q + c.tid]) + red[2 * Q + c.tid]) + red[3 * Q + c.tid];
}

// One workgroup of 256 threads: n records of Q doubles -> red[q][0], in a fixed order: thread i adds records i, i + 256, ... one
// after the other, then the 256 partial sums halve from 128.  Ends in a barrier.
template <int Q>
__device__ __forceinline__ void records_sum(const double* __restrict__ records, unsigned long long n, double (&red)[Q][256]) {
  const int tid = threadIdx.x;
  double s[Q] = {};
  for (unsigned long long i = tid; i < n; i += 256) {
#pragma unroll
    for (int q = 0; q < Q; ++q) s[q] += records[Q * i + q];
  }
#pragma unroll
  for (int q = 0; q < Q; ++q) red[q][tid] = s[q];
  __syncthreads();
  for (int off = 128; off >= 1; off >>= 1) {
    if (tid < off) {
#pragma unroll
      for (int q = 0; q < Q; ++q) red[q][tid] += red[q][tid + off];
    }
    __syncthreads();
  }
}

__host__ int rows_padded(int n_fft) { return ((2 * (n_fft / 2 + 1)) + 31) / 32 * 32; }
__host__ bool n_fft_ok(int n_fft) { return n_fft >= 64 && n_fft <= 2048 && (n_fft & (n_fft - 1)) == 0; }
// the window-folded DFT operand of a transform length: rows_padded rows of n_fft floats
__host__ size_t dft_operand_bytes(int n_fft) { return (size_t)rows_padded(n_fft) * n_fft * sizeof(float); }
// LDS of one workgroup: the 31 hop + n_fft samples its 32 overlapping frames are cut from (+ skew words), for every signal
__host__ size_t tile_lds_bytes(int n_fft, int hop, int signals) {
  const size_t span = (size_t)(kFrames - 1) * hop + n_fft;
  return signals * (span + (span >> 7) + 1) * sizeof(float);
}
__host__ bool tile_ok(int n_fft, int hop, int signals) { return hop >= 1 && tile_lds_bytes(n_fft, hop, signals) <= kLdsCap; }
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

// NWS_OK, or why the sizes of the two-signal kernels are refused; nothing here touches the device
__host__ int check_sizes(int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths) {
  if (!n_ffts || !hops || B < 1 || N < 1 || R < 1 || R > kMaxRes) return NWS_ERR_BAD_ARG;
  for (int r = 0; r < R; ++r) {
    if (hops[r] < 1) return NWS_ERR_BAD_ARG;
    if (win_lengths && (win_lengths[r] < 1 || win_lengths[r] > n_ffts[r])) return NWS_ERR_BAD_ARG;
    if (!n_fft_ok(n_ffts[r])) return NWS_ERR_UNSUPPORTED;
    if (N <= n_ffts[r] / 2) return NWS_ERR_BAD_ARG;  // reflect padding needs more than n_fft/2 samples (as in torch.stft)
    if (!tile_ok(n_ffts[r], hops[r], 2)) return NWS_ERR_UNSUPPORTED;
  }
  if (B > 65535) return NWS_ERR_UNSUPPORTED;
  return NWS_OK;
}

}  // namespace
