// The wave-level half of the 256-point transform of fir_spectral_fft.h, device only: the two-float value type, the 16 x 16
// transpose and the k <-> -k mirror through a transform's LDS plane, the twiddle table, and the reflect-padded noise.  Shared by
// the batched forward (fir_noise.hip) and the backward (fir_noise_grad.hip) of the noise branch; fir_spectral_fft.h itself holds
// the part that also compiles for the host.
#pragma once
#include "nws_common.h"
#include "fir_spectral_fft.h"

// the two-float value type of fir_spectral_fft.h's templates
template <>
struct SpOps<f32x2> {
  static __device__ __forceinline__ f32x2 fma(f32x2 a, f32x2 b, f32x2 c) { return __builtin_elementwise_fma(a, b, c); }
  static __device__ __forceinline__ f32x2 of(float v) { return f32x2{v, v}; }
  static __device__ __forceinline__ f32x2 at(const float* p) { return *reinterpret_cast<const f32x2*>(p); }
};

namespace {

// reflect-padded noise (torch.stft center=True, pad_mode="reflect", pad 128 each side).  Whole clip: origin = 128, len = N-1.
// Streaming windows pass the absolute noise stream with origin 0 and a len that only bites at the stream's end.
__device__ __forceinline__ float padded_noise(const float* __restrict__ noise, int len, int origin, int i) {
  int s = i - origin;
  if (s < 0) s = -s;
  if (s > len - 1) s = 2 * (len - 1) - s;
  s = s < 0 ? 0 : s;
  return noise[s];
}

// W256^(l k): the twiddle between the two passes, the same table in both directions, (cos, cos, sin, sin)(2 pi l k / 256) at
// [k][l] (each value twice: SpOps::at); thread tid of 256 fills entry tid.  In LDS because 30 registers of them per lane cost a
// wave per SIMD; a wave's four transforms read the same 256 B per k: broadcast
__device__ __forceinline__ void sp_fill_twiddles(float4* tw, int tid) {
  float c, s;
  sp_twiddle((tid & 15) * (tid >> 4), c, s);
  tw[tid] = make_float4(c, c, s, s);
}

// a wave's LDS traffic is ordered by itself; this keeps the compiler from moving accesses across an exchange
__device__ __forceinline__ void sp_wave_sync() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the 16 x 16 transpose: (register k, lane l) -> (lane k, register l).  Rows of 17 entries: 8-byte entries of 16 lanes x 4
// transforms fall on distinct bank pairs both ways (fir_spectral_fft.h)
template <class T>
__device__ __forceinline__ void sp_transpose(T (&v)[16], T* x, int l) {
#pragma unroll
  for (int k = 0; k < 16; ++k) x[k * kSpRow + l] = v[k];
  sp_wave_sync();
#pragma unroll
  for (int j = 0; j < 16; ++j) v[j] = x[l * kSpRow + j];
  sp_wave_sync();
}
// 256-point transform of (lane l, register j) = x[16 j + l] into (lane k1, register k2) = X[k1 + 16 k2]; INV: the same with
// conjugate twiddles, (lane k1, register k2) -> (lane l, register j), no scaling.  x: this transform's LDS plane.
template <bool INV, class T>
__device__ __forceinline__ void sp_fft256(C16T<T>& z, const float* tw, T* x, int l) {
  sp_pass1<INV>(z, tw);
  sp_transpose(z.re, x, l);
  sp_transpose(z.im, x, l);
  sp_dft16<INV>(z);
}
// (lane k1, register k2) = V[k1 + 16 k2]  ->  m = V[(256 - k) & 255] through the transform's plane, in natural order
template <class T>
__device__ __forceinline__ void sp_mirror(const T (&v)[16], T (&m)[16], T* x, int l) {
#pragma unroll
  for (int j = 0; j < 16; ++j) x[l + 16 * j] = v[j];
  sp_wave_sync();
#pragma unroll
  for (int j = 0; j < 16; ++j) m[j] = x[(256 - (l + 16 * j)) & 255];
  sp_wave_sync();
}

__device__ __forceinline__ f32x2 sp_shfl(f32x2 v, int src) { return f32x2{__shfl(v.x, src, 64), __shfl(v.y, src, 64)}; }
__device__ __forceinline__ f32x2 sp_select(bool c, f32x2 a, f32x2 b) { return f32x2{c ? a.x : b.x, c ? a.y : b.y}; }

}  // namespace
