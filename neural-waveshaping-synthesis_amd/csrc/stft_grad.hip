// Gradient of the multi-resolution STFT loss (stft_loss.hip) with respect to the reconstruction x: DESIGN.md 3.13.
//
// Per resolution, with X = STFT(x), p = Re^2 + Im^2, x_mag = sqrt(max(p, eps)), y_mag likewise, C = B bins frames:
//   g    = (1/R) [ w_sc (x_mag - y_mag) / (||y_mag - x_mag||_F ||y_mag||_F) + w_log sign(ln x_mag - ln y_mag) / (C x_mag)
//                  + w_lin sign(x_mag - y_mag) / C ]              sign(0) = 0; the first term is 0 when its norm is 0
//   G_re = g Re X / x_mag, G_im = g Im X / x_mag where p >= eps, 0 under the clamp
//   z_t[n] = sum_k D[2k][n] G_re[k,t] + D[2k+1][n] G_im[k,t]       D: the operand of stft_loss_dft_kernel
//   dL/dx[i] = sum of z_t[n] over the padded positions hop t - n_fft/2 + n that the reflect padding maps to i
//
// Five kernels per resolution, all on the caller's stream:
//   stft_grad_norm_kernel      the forward tile (stft_tile.h); one record of two doubles per workgroup: sum (y_mag - x_mag)^2, sum y_mag^2
//   stft_grad_coef_kernel      one workgroup: the records summed in a fixed order in fp64 -> w_sc / (R ||y - x|| ||y||), or 0
//   stft_grad_spectrum_kernel  the forward tile again; G formed in-lane from the accumulators, written to the workspace as
//                              [b][frame tile][row][32 frames] (rows 2k / 2k+1 = G_re / G_im, zero past the last bin and frame)
//   stft_grad_back_kernel      z = D^T G on the matrix pipe: M = the window's columns (rounded out to 32), N = 32 frames, K = rows;
//                              A is the same dft tensor read transposed (a lane's 32 columns are contiguous), B is G.  Two M-tiles
//                              per wave share every G load.  z goes to the workspace as [b][frame][column] through an LDS transpose.
//   stft_grad_gather_kernel    one thread per output sample: the overlap-add and the reflect fold as a gather over the (at most
//                              three) padded positions that map to it and the frames that cover them, in a fixed order; the first
//                              resolution writes grad_out, the others add to it.
// No floating-point atomics: two calls on equal inputs give equal bits.  Nothing is read back: the call only enqueues.
// Limits: those of nws_stft_loss (stft_tile.h: check_sizes).
#include <algorithm>

#include "stft_tile.h"

namespace {

constexpr int kBackTiles = 2;  // M-tiles per wave of stft_grad_back_kernel

// grid (frame tiles, groups of 4 M-tiles, B), as stft_loss_kernel
__global__ __launch_bounds__(256) void stft_grad_norm_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int n_fft,
                                                             int hop, int frames, const float* __restrict__ dft, int m_tiles, int k_lo,
                                                             int k_half, float eps, double* __restrict__ records) {
  extern __shared__ __align__(16) float lds[];
  const TileCoord c;
  TileAcc a;
  double s_sc = 0.0, s_y2 = 0.0;
  if (tile_prologue<2>(c, {x, y}, N, n_fft, hop, dft, m_tiles, k_lo, k_half, lds, a)) {
    const int bins = n_fft / 2 + 1;
    const bool frame_ok = c.t0 + c.col < frames;
#pragma unroll
    for (int r = 0; r < 16; r += 2) {
      if (tile_bin(c.mt, r, c.kh) < bins && frame_ok) {
        const float xm = sqrtf(fmaxf(fmaf(a.x[r], a.x[r], a.x[r + 1] * a.x[r + 1]), eps));
        const float ym = sqrtf(fmaxf(fmaf(a.y[r], a.y[r], a.y[r + 1] * a.y[r + 1]), eps));
        const float d = ym - xm;
        s_sc += (double)d * (double)d;
        s_y2 += (double)ym * (double)ym;
      }
    }
  }
  double s[2] = {s_sc, s_y2};
  tile_reduce(c, s, lds, records);
}

// coef[0] = w_sc_over_r / (||y_mag - x_mag||_F ||y_mag||_F), 0 where the first norm is 0 (the subgradient torch takes there)
__global__ __launch_bounds__(256) void stft_grad_coef_kernel(const double* __restrict__ records, unsigned long long n, double w_sc_over_r,
                                                             double* __restrict__ coef) {
  __shared__ double red[2][256];
  records_sum(records, n, red);
  if (threadIdx.x == 0) coef[0] = red[0][0] > 0.0 ? w_sc_over_r / (sqrt(red[0][0]) * sqrt(red[1][0])) : 0.0;
}

__device__ __forceinline__ float sign_of(float v) { return (float)(v > 0.0f) - (float)(v < 0.0f); }

// grid as stft_grad_norm_kernel.  G of frame tile blockIdx.x of row b: rows_pad x 32 floats at ((b gridDim.x + blockIdx.x) rows_pad + row) 32 + col
__global__ __launch_bounds__(256) void stft_grad_spectrum_kernel(const float* __restrict__ x, const float* __restrict__ y, int N, int n_fft,
                                                                 int hop, int frames, const float* __restrict__ dft, int m_tiles, int k_lo,
                                                                 int k_half, float eps, const double* __restrict__ coef, float c_log,
                                                                 float c_lin, float* __restrict__ G) {
  extern __shared__ __align__(16) float lds[];
  const TileCoord c;
  TileAcc a;
  if (!tile_prologue<2>(c, {x, y}, N, n_fft, hop, dft, m_tiles, k_lo, k_half, lds, a)) return;
  const f32x16 &ax = a.x, &ay = a.y;
  const int mt = c.mt, kh = c.kh, col = c.col;
  const float c_sc = (float)coef[0];
  const int bins = n_fft / 2 + 1;
  const bool frame_ok = c.t0 + col < frames;
  float* out = G + (((size_t)c.b * gridDim.x + blockIdx.x) * (32 * (size_t)m_tiles) + 32 * (size_t)mt) * 32 + col;
#pragma unroll
  for (int r = 0; r < 16; r += 2) {
    float g_re = 0.0f, g_im = 0.0f;
    if (tile_bin(mt, r, kh) < bins && frame_ok) {
      const float p = fmaf(ax[r], ax[r], ax[r + 1] * ax[r + 1]);
      if (p >= eps) {  // the clamp passes no gradient below eps
        const float xm = sqrtf(p);
        const float ym = sqrtf(fmaxf(fmaf(ay[r], ay[r], ay[r + 1] * ay[r + 1]), eps));
        const float d = xm - ym;
        const float g = c_sc * d + c_log * sign_of(logf(xm) - logf(ym)) / xm + c_lin * sign_of(d);
        const float s = g / xm;
        g_re = s * ax[r];
        g_im = s * ax[r + 1];
      }
    }
    const int row = (r & 3) + 8 * (r >> 2) + 4 * kh;  // accumulator register r of lane half kh
    out[(size_t)row * 32] = g_re;
    out[(size_t)(row + 1) * 32] = g_im;
  }
}

// grid (frame tiles, groups of 4 kBackTiles M-tiles, B).  z[n, t] = sum_row D[row][n_lo + n] G[row][t], n < 32 n_tiles, t < 32;
// z of row b: ((b gridDim.x + blockIdx.x) 32 + t) (32 n_tiles) + n
__global__ __launch_bounds__(256) void stft_grad_back_kernel(const float* __restrict__ dft, const float* __restrict__ G, int n_fft,
                                                             int rows_pad, int n_lo, int n_tiles, float* __restrict__ z) {
  __shared__ float patch[4][kBackTiles][32 * 33];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kh = lane >> 5, col = lane & 31;
  const int mt0 = (blockIdx.y * 4 + wave) * kBackTiles;
  const size_t tile = (size_t)blockIdx.z * gridDim.x + blockIdx.x;
  if (mt0 < n_tiles) {
    const bool two = mt0 + 1 < n_tiles;
    const float* a0 = dft + (size_t)kh * n_fft + n_lo + 32 * mt0 + col;  // A[m][k] = D[k][n_lo + 32 mt + m]: the operand read transposed
    const float* a1 = a0 + (two ? 32 : 0);
    const float* bp = G + (tile * rows_pad + kh) * 32 + col;
    f32x16 acc0 = {}, acc1 = {};
    for (int k0 = 0; k0 < rows_pad; k0 += 16) {
      float av0[8], av1[8], bv[8];
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        av0[i] = a0[(size_t)(k0 + 2 * i) * n_fft];
        av1[i] = a1[(size_t)(k0 + 2 * i) * n_fft];
        bv[i] = bp[(size_t)(k0 + 2 * i) * 32];
      }
#pragma unroll
      for (int i = 0; i < 8; ++i) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av0[i], bv[i], acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av1[i], bv[i], acc1, 0, 0, 0);
      }
    }
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int n = (r & 3) + 8 * (r >> 2) + 4 * kh;
      patch[wave][0][n * 33 + col] = acc0[r];
      patch[wave][1][n * 33 + col] = acc1[r];
    }
  }
  __syncthreads();
  if (mt0 < n_tiles) {
    const int n_len = 32 * n_tiles;
    for (int q = 0; q < kBackTiles && mt0 + q < n_tiles; ++q) {
      float* out = z + (tile * 32 + kh) * n_len + 32 * (mt0 + q) + col;
#pragma unroll
      for (int j = 0; j < 16; ++j) out[(size_t)(2 * j) * n_len] = patch[wave][q][col * 33 + 2 * j + kh];
    }
  }
}

// grid (ceil(N / 256), B).  Sample i collects z_t[n] from the padded positions p = hop t - n_fft/2 + n with reflect_index(p) = i:
// p = i, p = -i (1 <= i <= n_fft/2) and p = 2 (N - 1) - i (N - 1 - n_fft/2 <= i <= N - 2), in that order, frames ascending.
__global__ __launch_bounds__(256) void stft_grad_gather_kernel(const float* __restrict__ z, int N, int n_fft, int hop, int frames,
                                                               int frames_pad, int n_lo, int n_len, int first, float* __restrict__ grad) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  const int b = blockIdx.y;
  const long long half = n_fft / 2;
  const float* zb = z + (size_t)b * frames_pad * n_len;
  float acc = 0.0f;
  for (int s = 0; s < 3; ++s) {
    long long p = i;
    if (s == 1) {
      if (i < 1 || i > half) continue;
      p = -i;
    } else if (s == 2) {
      p = 2LL * (N - 1) - i;
      if (i > N - 2 || p > N + half - 1) continue;
    }
    const long long q = p + half - n_lo;  // n - n_lo = q - hop t must lie in [0, n_len)
    if (q < 0) continue;
    long long t_hi = q / hop;
    if (t_hi > frames - 1) t_hi = frames - 1;
    long long t_lo = q - n_len + 1 <= 0 ? 0 : (q - n_len + hop) / hop;  // ceil((q - n_len + 1) / hop)
    for (long long t = t_lo; t <= t_hi; ++t) acc += zb[(size_t)t * n_len + (size_t)(q - hop * t)];
  }
  float* g = grad + (size_t)b * N + i;
  *g = first ? acc : *g + acc;
}

// the columns stft_grad_back_kernel produces: the K range of the forward rounded out to whole M-tiles of 32
struct NRange {
  int n_lo, n_tiles;
};
__host__ NRange n_range_of(int n_fft, int win) {
  const KRange k = k_range_of(n_fft, win);
  NRange n;
  n.n_lo = k.k_lo & ~31;
  n.n_tiles = (k.k_lo + k.k_len - n.n_lo + 31) / 32;  // n_fft is a multiple of 32: n_lo + 32 n_tiles <= n_fft
  return n;
}

__host__ size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

// workspace: [coef: 1 double][records of the largest grid: 2 doubles each][G of the largest resolution][z of the largest resolution]
struct Layout {
  size_t rec_off, g_off, z_off, total;
};
__host__ Layout layout_of(int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths) {
  size_t rec = 0, g = 0, z = 0;
  for (int r = 0; r < R; ++r) {
    const Grid gr = grid_of(B, N, n_ffts[r], hops[r]);
    const size_t tiles = (size_t)B * gr.gx;
    rec = std::max(rec, (size_t)gr.records * 2 * sizeof(double));
    g = std::max(g, tiles * rows_padded(n_ffts[r]) * 32 * sizeof(float));
    z = std::max(z, tiles * 32 * (32 * (size_t)n_range_of(n_ffts[r], win_lengths[r]).n_tiles) * sizeof(float));
  }
  Layout l;
  l.rec_off = 256;
  l.g_off = l.rec_off + align256(rec);
  l.z_off = l.g_off + align256(g);
  l.total = l.z_off + align256(z);
  return l;
}

}  // namespace

extern "C" {

size_t nws_stft_grad_workspace_bytes(int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths) {
  if (!win_lengths || check_sizes(B, N, R, n_ffts, hops, win_lengths) != NWS_OK) return 0;
  return layout_of(B, N, R, n_ffts, hops, win_lengths).total;
}

int nws_stft_grad(const float* x, const float* y, int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths,
                  const float* const* dfts, float w_sc, float w_log_mag, float w_lin_mag, float eps, float* grad_out, void* workspace,
                  size_t workspace_bytes, void* stream) {
  if (!x || !y || !win_lengths || !dfts || !grad_out || !workspace) return NWS_ERR_BAD_ARG;
  const int rc = check_sizes(B, N, R, n_ffts, hops, win_lengths);
  if (rc != NWS_OK) return rc;
  for (int r = 0; r < R; ++r)
    if (!dfts[r]) return NWS_ERR_BAD_ARG;
  if (!(eps > 0.0f)) return NWS_ERR_BAD_ARG;
  const Layout l = layout_of(B, N, R, n_ffts, hops, win_lengths);
  if (workspace_bytes < l.total) return NWS_ERR_WORKSPACE;

  hipStream_t st = (hipStream_t)stream;
  static unsigned long long attr_devices = 0;
  if (nws_first_use_on_device(attr_devices)) {
    for (const void* k : {reinterpret_cast<const void*>(stft_grad_norm_kernel), reinterpret_cast<const void*>(stft_grad_spectrum_kernel)}) {
      const hipError_t e = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, (int)kLdsCap);
      if (e != hipSuccess) return (int)e;
    }
  }
  char* ws = static_cast<char*>(workspace);
  double* coef = reinterpret_cast<double*>(ws);
  double* records = reinterpret_cast<double*>(ws + l.rec_off);
  float* G = reinterpret_cast<float*>(ws + l.g_off);
  float* z = reinterpret_cast<float*>(ws + l.z_off);
  for (int r = 0; r < R; ++r) {
    const int n_fft = n_ffts[r], hop = hops[r], frames = frames_of(N, hop), rows_pad = rows_padded(n_fft);
    const Grid g = grid_of(B, N, n_fft, hop);
    const KRange k = k_range_of(n_fft, win_lengths[r]);
    const NRange n = n_range_of(n_fft, win_lengths[r]);
    const double count = (double)B * (double)(n_fft / 2 + 1) * (double)frames;
    const dim3 tile_grid(g.gx, g.gy, (unsigned)B);
    stft_grad_norm_kernel<<<tile_grid, 256, tile_lds_bytes(n_fft, hop, 2), st>>>(x, y, N, n_fft, hop, frames, dfts[r], rows_pad / 32, k.k_lo,
                                                                               k.k_len / 2, eps, records);
    NWS_CHECK_LAUNCH();
    stft_grad_coef_kernel<<<1, 256, 0, st>>>(records, g.records, (double)w_sc / (double)R, coef);
    NWS_CHECK_LAUNCH();
    stft_grad_spectrum_kernel<<<tile_grid, 256, tile_lds_bytes(n_fft, hop, 2), st>>>(
        x, y, N, n_fft, hop, frames, dfts[r], rows_pad / 32, k.k_lo, k.k_len / 2, eps, coef, (float)((double)w_log_mag / ((double)R * count)),
        (float)((double)w_lin_mag / ((double)R * count)), G);
    NWS_CHECK_LAUNCH();
    stft_grad_back_kernel<<<dim3(g.gx, (unsigned)((n.n_tiles + 4 * kBackTiles - 1) / (4 * kBackTiles)), (unsigned)B), 256, 0, st>>>(
        dfts[r], G, n_fft, rows_pad, n.n_lo, n.n_tiles, z);
    NWS_CHECK_LAUNCH();
    stft_grad_gather_kernel<<<dim3((unsigned)((N + 255) / 256), (unsigned)B), 256, 0, st>>>(z, N, n_fft, hop, frames, (int)g.gx * 32, n.n_lo,
                                                                                          32 * n.n_tiles, r == 0, grad_out);
    NWS_CHECK_LAUNCH();
  }
  return NWS_OK;
}

}  // extern "C"
