// Band-limited sample-rate converter, the step in front of the two analysis kernels (pyin.hip, loudness.hip):
//   neural_waveshaping_synthesis/data/utils/preprocess_audio.py:65-66 (resample_audio -> resampy.resample, kaiser_best).
//   DESIGN.md 3.10 holds the definition the kernel is tested against; parity with resampy itself is unpinned.
//
// With L = sr_out / gcd and M = sr_in / gcd, output t = j + p L (period p, place j in the period) sits at input position
// p M + j M / L: sample n = p M + floor(j M / L), phase numerator r = (j M) mod L.  Its value is row r of the weight bank
// (L rows of `taps` fp32 weights, built in fp64 on the host) against x[n - left + 1 .. n + right], zero outside the row.
//
// resample_kernel: a workgroup owns 64 G consecutive periods and up to 160 places j of them.  It stages the
// 64 G M + taps - 1 input samples those periods touch in LDS once (the zero extension is resolved there).  LANES RUN OVER
// PERIODS, so the weight of a tap is the same for the whole wave - a scalar load that feeds the FMA as a scalar-register
// operand, no LDS traffic and no vector register - and the only vector operand is an LDS word, read at a stride of M words
// between lanes.  An odd M is free of bank conflicts; an even M >= 8 gets one pad word per period (stride M + 1), and a run of
// taps is then cut at the period boundaries the pad sits on.  A wave sums FOUR consecutive places at once: their windows of x
// overlap in all but floor((j + 3) M / L) - floor(j M / L) words, so an LDS pair is read once for four packed FMAs (scalar
// weight pair x LDS pair; even taps in .x of the accumulator, odd taps in .y; no operand swizzle).  Results go through an LDS
// tile (odd row stride) so that the stores to y are consecutive words.
// The sum of one output: the taps in front of the overlap, the overlap, the taps behind it; every run in steps of eight,
// its remainder on .x; .x + .y at the end.  The runs depend on j only: the order of summation is a function of
// (sr_in, sr_out), never of the batch row, B or the output's place in its tile.
//
// resample_direct_kernel: one thread per output, operands from global memory.  Taken when 64 periods do not fit LDS
// (M above ~500: e.g. 192 kHz -> 44.1 kHz).  Four chains over the taps.
//
// Limits (NWS_ERR_UNSUPPORTED): rates below 1, a bank above 64 MB, n_out or the grid above 2^31 - 1.
#include <math.h>

#include "nws_common.h"

namespace {

constexpr int kNumZeros = 64, kNb = 512, kNwin = kNumZeros * kNb + 1;
constexpr double kRolloff = 0.9475937167399596, kBeta = 14.769656459379492;
constexpr size_t kMaxBankBytes = (size_t)64 << 20;
constexpr int kThreads = 1024, kWaves = kThreads / 64;
constexpr int kLdsFloats = 160 * 1024 / 4;
constexpr int kMaxPlaces = 160;     // places j of a period per workgroup (output tile: 64 G rows of them)
constexpr int kPlaces = 4;          // places a wave sums at once on the same LDS reads

struct ResampleDims {
  int L, M, taps, left, right, step;
  double ratio, scale;
  // kernel geometry
  int pad;      // 1: one pad word per period in LDS
  int G;        // groups of 64 periods per workgroup; 0: direct kernel
  int JC, nchunk;   // places per workgroup, workgroups per period tile
};

__host__ long long gcd_ll(long long a, long long b) {
  while (b) {
    const long long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

// offsets into the half window of phase numerator r: left wing, right wing (resampy 0.2.2's arithmetic)
__host__ void wing_offsets(const ResampleDims& d, int r, int* off_l, double* eta_l, int* off_r, double* eta_r) {
  const double frac = d.scale * ((double)r / (double)d.L);
  double idx = frac * (double)kNb;
  *off_l = (int)idx;
  *eta_l = idx - (double)*off_l;
  idx = (d.scale - frac) * (double)kNb;
  *off_r = (int)idx;
  *eta_r = idx - (double)*off_r;
}

__host__ bool resample_dims(long long sr_in, long long sr_out, ResampleDims* d) {
  if (sr_in < 1 || sr_out < 1 || sr_in > 0x7fffffffLL || sr_out > 0x7fffffffLL) return false;
  static thread_local long long c_in = 0, c_out = 0;      // the launcher asks for the same pair call after call
  static thread_local ResampleDims cached;
  if (sr_in == c_in && sr_out == c_out) {
    *d = cached;
    return true;
  }
  const long long g = gcd_ll(sr_in, sr_out);
  d->L = (int)(sr_out / g);
  d->M = (int)(sr_in / g);
  d->ratio = (double)sr_out / (double)sr_in;
  d->scale = d->ratio < 1.0 ? d->ratio : 1.0;
  d->step = (int)(d->scale * (double)kNb);
  if (d->step < 1) return false;                                         // ratio below 1 / 512: more than 2^15 taps a wing
  if ((size_t)d->L * 2 * (kNumZeros - 1) * sizeof(float) > kMaxBankBytes) return false;   // before the loop over L
  d->left = d->right = 0;
  for (int r = 0; r < d->L; ++r) {
    int ol, orr;
    double el, er;
    wing_offsets(*d, r, &ol, &el, &orr, &er);
    const int nl = (kNwin - ol) / d->step, nr = (kNwin - orr) / d->step;
    d->left = nl > d->left ? nl : d->left;
    d->right = nr > d->right ? nr : d->right;
  }
  d->taps = d->left + d->right;
  if (d->left < 1 || (size_t)d->L * d->taps * sizeof(float) > kMaxBankBytes) return false;
  d->pad = (d->M % 2 == 0 && d->M >= 8) ? 1 : 0;
  const int nchunk = (d->L + kMaxPlaces - 1) / kMaxPlaces;
  d->nchunk = nchunk;
  d->JC = (d->L + nchunk - 1) / nchunk;
  const long long per_group = 64LL * ((long long)d->M + d->pad + (d->JC | 1));
  const long long fit = ((long long)kLdsFloats - 2LL * d->taps - 2) / per_group;   // taps + the pad words among them
  const int quads = (d->JC + kPlaces - 1) / kPlaces;
  const int want = (4 * kWaves + quads - 1) / quads;                     // about four (places, group) items per wave
  d->G = (int)(fit < want ? (fit < 0 ? 0 : fit) : want);
  c_in = sr_in;
  c_out = sr_out;
  cached = *d;
  return true;
}

__host__ long long resample_length(long long N, const ResampleDims& d) { return N < 1 ? 0 : (N * d.L) / d.M; }

// I0 by its power series: every term is positive, so the sum carries no cancellation
__host__ double bessel_i0(double x) {
  const double q = 0.25 * x * x;
  double term = 1.0, sum = 1.0;
  for (int k = 1; k < 500; ++k) {
    term *= q / ((double)k * (double)k);
    sum += term;
    if (term < 1e-18 * sum) break;
  }
  return sum;
}

struct Geometry {
  int L, M, taps, lead, pad, G, JC, nchunk;
  int N, n_out, tiles;
};

// acc[i] += w[i][0 .. n) . x[o .. o + n) for R rows of weights at once, x = the lane's period in LDS from logical word o on.
// Eight taps a step: four packed FMAs per row (even taps in .x, odd taps in .y) on four LDS pairs that all R rows share; the
// remainder of a run goes to .x.  With pad words in LDS a run is cut at the period boundaries it crosses.
template <int R>
__device__ __forceinline__ void taps_run(const float* xl, int pad, int M, int o, int n, const float* const (&w)[R],
                                         f32x2 (&acc)[R]) {
  int c = 0;
  while (c < n) {
    const int q = pad ? (o + c) / M : 0;
    const int seg = pad ? min(n - c, (q + 1) * M - (o + c)) : n - c;
    const float* xv = xl + o + c + q;
    int i = 0;
    for (; i + 8 <= seg; i += 8) {
      const f32x2 x0 = {xv[i], xv[i + 1]}, x1 = {xv[i + 2], xv[i + 3]}, x2 = {xv[i + 4], xv[i + 5]}, x3 = {xv[i + 6], xv[i + 7]};
#pragma unroll
      for (int u = 0; u < R; ++u) {
        const float* ww = w[u] + c + i;
        acc[u] = fma2(f32x2{ww[0], ww[1]}, x0, acc[u]);
        acc[u] = fma2(f32x2{ww[2], ww[3]}, x1, acc[u]);
        acc[u] = fma2(f32x2{ww[4], ww[5]}, x2, acc[u]);
        acc[u] = fma2(f32x2{ww[6], ww[7]}, x3, acc[u]);
      }
    }
    for (; i < seg; ++i) {
      const float xi = xv[i];
#pragma unroll
      for (int u = 0; u < R; ++u) acc[u].x = fmaf(w[u][c + i], xi, acc[u].x);
    }
    c += seg;
  }
}

// R consecutive places j .. j + R - 1 of one period, all 64 periods of a group: their windows of x overlap in all but
// d = n(j + R - 1) - n(j) words, so the overlap is read from LDS once for the R of them; what sticks out in front and behind
// is summed place by place.  Every place: head, overlap, tail, in that order.
template <int R>
__device__ __forceinline__ void places_run(const float* __restrict__ bank, const Geometry& k, const float* xl, int j, float* out) {
  int n[R];
  const float* row[R];
#pragma unroll
  for (int u = 0; u < R; ++u) {
    const long long jm = (long long)(j + u) * k.M;
    n[u] = (int)(jm / k.L);
    row[u] = bank + (size_t)(jm - (long long)n[u] * k.L) * k.taps;
  }
  f32x2 acc[R];
#pragma unroll
  for (int u = 0; u < R; ++u) acc[u] = f32x2{0.0f, 0.0f};
  const int d = n[R - 1] - n[0], common = k.taps - d;
  if (R > 1 && common > 0) {
    const float* w[R];
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int head = n[R - 1] - n[u];
      if (head > 0) {
        const float* const w1[1] = {row[u]};
        f32x2 a1[1] = {acc[u]};
        taps_run<1>(xl, k.pad, k.M, n[u], head, w1, a1);
        acc[u] = a1[0];
      }
      w[u] = row[u] + head;
    }
    taps_run<R>(xl, k.pad, k.M, n[R - 1], common, w, acc);
#pragma unroll
    for (int u = 1; u < R; ++u) {
      const int tail = n[u] - n[0];
      if (tail > 0) {
        const float* const w1[1] = {row[u] + k.taps - tail};
        f32x2 a1[1] = {acc[u]};
        taps_run<1>(xl, k.pad, k.M, n[0] + k.taps, tail, w1, a1);
        acc[u] = a1[0];
      }
    }
  } else {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const float* const w1[1] = {row[u]};
      f32x2 a1[1] = {acc[u]};
      taps_run<1>(xl, k.pad, k.M, n[u], k.taps, w1, a1);
      acc[u] = a1[0];
    }
  }
#pragma unroll
  for (int u = 0; u < R; ++u) out[u] = nws_add_scalar(acc[u].x, acc[u].y);
}

__global__ __launch_bounds__(kThreads) void resample_kernel(const float* __restrict__ x, const float* __restrict__ bank,
                                                            Geometry k, float* __restrict__ y) {
  extern __shared__ float lds[];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int L = k.L, M = k.M, Mp = M + k.pad, periods = 64 * k.G;
  // blockIdx.x = (row * tiles + tile) * nchunk + chunk: the workgroups that stage the same samples are neighbours
  const int chunk = blockIdx.x % k.nchunk, rt = blockIdx.x / k.nchunk;
  const int tile = rt % k.tiles, row = rt / k.tiles;
  const int j0 = chunk * k.JC, nj = min(k.JC, L - j0), JCp = k.JC | 1;
  const int span = periods * M + k.taps - 1;              // logical word a holds x[P0 M - lead + a]
  float* xs = lds;
  float* ys = lds + span + (k.pad ? span / M : 0) + 1;
  const long long P0 = (long long)tile * periods;
  const long long first = P0 * M - k.lead;
  const float* xr = x + (size_t)row * k.N;
  for (int a = tid; a < span; a += kThreads) {
    const long long i = first + a;
    xs[k.pad ? a + a / M : a] = (i >= 0 && i < k.N) ? xr[i] : 0.0f;
  }
  __syncthreads();
  const int quads = (nj + kPlaces - 1) / kPlaces;         // places in fours, the last group what is left
  for (int item = wave; item < quads * k.G; item += kWaves) {      // wave-uniform
    const int grp = item / quads, jj = (item - grp * quads) * kPlaces, left = nj - jj;
    const float* xl = xs + (grp * 64 + lane) * Mp;
    float* out = ys + (grp * 64 + lane) * JCp + jj;
    if (left >= 4) {
      float v[4];
      places_run<4>(bank, k, xl, j0 + jj, v);
      out[0] = v[0], out[1] = v[1], out[2] = v[2], out[3] = v[3];
    } else if (left == 3) {
      float v[3];
      places_run<3>(bank, k, xl, j0 + jj, v);
      out[0] = v[0], out[1] = v[1], out[2] = v[2];
    } else if (left == 2) {
      float v[2];
      places_run<2>(bank, k, xl, j0 + jj, v);
      out[0] = v[0], out[1] = v[1];
    } else {
      float v[1];
      places_run<1>(bank, k, xl, j0 + jj, v);
      out[0] = v[0];
    }
  }
  __syncthreads();
  float* yr = y + (size_t)row * k.n_out;
  for (int i = tid; i < periods * nj; i += kThreads) {
    const int p = i / nj, jj = i - p * nj;
    const long long t = (P0 + p) * L + j0 + jj;
    if (t < k.n_out) yr[t] = ys[p * JCp + jj];
  }
}

__global__ __launch_bounds__(256) void resample_direct_kernel(const float* __restrict__ x, const float* __restrict__ bank,
                                                              Geometry k, float* __restrict__ y) {
  const int row = blockIdx.x / k.tiles;
  const long long t = (long long)(blockIdx.x % k.tiles) * 256 + threadIdx.x;
  if (t >= k.n_out) return;
  const long long tm = t * k.M, n = tm / k.L;
  const int r = (int)(tm - n * k.L);
  const float* w = bank + (size_t)r * k.taps;
  const float* xr = x + (size_t)row * k.N;
  const long long base = n - k.lead;
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  int c = 0;
  for (; c + 8 <= k.taps; c += 8) {
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const long long i = base + c + u;
      a[u & 3] = fmaf(w[c + u], (i >= 0 && i < k.N) ? xr[i] : 0.0f, a[u & 3]);
    }
  }
  for (; c < k.taps; ++c) {
    const long long i = base + c;
    a[0] = fmaf(w[c], (i >= 0 && i < k.N) ? xr[i] : 0.0f, a[0]);
  }
  y[(size_t)row * k.n_out + t] = (a[0] + a[1]) + (a[2] + a[3]);
}

}  // namespace

extern "C" {

int nws_resample_dims(int sr_in, int sr_out, int32_t* dims) {
  ResampleDims d;
  if (!dims) return NWS_ERR_BAD_ARG;
  if (!resample_dims(sr_in, sr_out, &d)) return NWS_ERR_UNSUPPORTED;
  const int32_t v[6] = {d.L, d.M, d.taps, d.left, d.right, d.step};
  for (int i = 0; i < 6; ++i) dims[i] = v[i];
  return NWS_OK;
}

int64_t nws_resample_length(int64_t N, int sr_in, int sr_out) {
  ResampleDims d;
  if (N < 1 || N > 0x7fffffffLL || !resample_dims(sr_in, sr_out, &d)) return 0;
  return (int64_t)resample_length(N, d);
}

size_t nws_resample_bank_bytes(int sr_in, int sr_out) {
  ResampleDims d;
  if (!resample_dims(sr_in, sr_out, &d)) return 0;
  return (size_t)d.L * d.taps * sizeof(float);
}

int nws_resample_bank(int sr_in, int sr_out, float* bank_host) {
  ResampleDims d;
  if (!bank_host) return NWS_ERR_BAD_ARG;
  if (!resample_dims(sr_in, sr_out, &d)) return NWS_ERR_UNSUPPORTED;
  double* win = new double[2 * (size_t)kNwin];
  double* delta = win + kNwin;
  const double i0_beta = bessel_i0(kBeta);
  for (int i = 0; i < kNwin; ++i) {
    const double u = (double)i / (double)(kNwin - 1);
    const double kaiser = bessel_i0(kBeta * sqrt(1.0 - u * u)) / i0_beta;
    const double px = M_PI * (kRolloff * ((double)i * ((double)kNumZeros / (double)(kNwin - 1))));
    const double sinc = i == 0 ? 1.0 : sin(px) / px;
    win[i] = kRolloff * sinc * kaiser;
    if (d.ratio < 1.0) win[i] *= d.ratio;
  }
  for (int i = 0; i + 1 < kNwin; ++i) delta[i] = win[i + 1] - win[i];
  delta[kNwin - 1] = 0.0;
  for (int r = 0; r < d.L; ++r) {
    float* row = bank_host + (size_t)r * d.taps;
    for (int c = 0; c < d.taps; ++c) row[c] = 0.0f;
    int ol, orr;
    double el, er;
    wing_offsets(d, r, &ol, &el, &orr, &er);
    const int nl = (kNwin - ol) / d.step, nr = (kNwin - orr) / d.step;
    for (int i = 0; i < nl; ++i) row[d.left - 1 - i] = (float)(win[ol + i * d.step] + el * delta[ol + i * d.step]);
    for (int i = 0; i < nr; ++i) row[d.left + i] = (float)(win[orr + i * d.step] + er * delta[orr + i * d.step]);
  }
  delete[] win;
  return NWS_OK;
}

int nws_resample(const float* x, int B, int N, int sr_in, int sr_out, const float* bank_dev, float* y, void* stream) {
  ResampleDims d;
  if (!x || !bank_dev || !y || B < 1 || N < 1) return NWS_ERR_BAD_ARG;
  if (!resample_dims(sr_in, sr_out, &d)) return NWS_ERR_UNSUPPORTED;
  const long long n_out = resample_length(N, d);
  if (n_out < 1) return NWS_ERR_BAD_ARG;
  if (n_out > 0x7fffffffLL) return NWS_ERR_UNSUPPORTED;
  Geometry k{d.L, d.M, d.taps, d.left - 1, d.pad, d.G, d.JC, d.nchunk, N, (int)n_out, 0};
  if (d.G > 0) {
    const long long periods = (n_out + d.L - 1) / d.L, per_tile = 64LL * d.G;
    const long long tiles = (periods + per_tile - 1) / per_tile, blocks = tiles * d.nchunk * B;
    if (blocks > 0x7fffffffLL) return NWS_ERR_UNSUPPORTED;
    k.tiles = (int)tiles;
    const long long span = per_tile * d.M + d.taps - 1;
    const size_t lds = (size_t)(span + (d.pad ? span / d.M : 0) + 1 + per_tile * (d.JC | 1)) * sizeof(float);
    static unsigned long long attr_devices = 0;
    if (nws_first_use_on_device(attr_devices)) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(resample_kernel),
                                               hipFuncAttributeMaxDynamicSharedMemorySize, kLdsFloats * (int)sizeof(float));
      if (e != hipSuccess) return (int)e;
    }
    resample_kernel<<<(unsigned)blocks, kThreads, lds, (hipStream_t)stream>>>(x, bank_dev, k, y);
  } else {
    const long long tiles = (n_out + 255) / 256, blocks = tiles * B;
    if (blocks > 0x7fffffffLL) return NWS_ERR_UNSUPPORTED;
    k.tiles = (int)tiles;
    resample_direct_kernel<<<(unsigned)blocks, 256, 0, (hipStream_t)stream>>>(x, bank_dev, k, y);
  }
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

}  // extern "C"
