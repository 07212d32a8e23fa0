// 256-point complex FFT pieces of the batched FIR-noise kernel (fir_noise.hip, fir_noise_spectral_kernel) and of its backward
// (fir_noise_grad.hip); the wave-level, device-only half is fir_spectral_wave.h.  Here: a 16-point DFT in
// registers and the W256 twiddles.  256 = 16 x 16: sixteen lanes hold sixteen points each, one transpose through LDS between
// the two register passes.  re and im sit in separate registers: the "times -i" of a packed complex type is exactly the
// operand swizzle the build refuses.  Everything is a template on the value type T: float, or a two-float
// vector that runs the same transform on two independent data sets (two utterances) with packed instructions and no swizzle.
//
// No device-only construct in here: tests/test_fir_spectral_fft.py compiles the header for the host (NWS_SP_FN = inline) and
// checks both passes against a float64 DFT.
#pragma once

#ifndef NWS_SP_FN
#define NWS_SP_FN __device__ __forceinline__
#endif
#ifndef NWS_SP_TABLE
#define NWS_SP_TABLE __device__ const
#endif

template <class T>
struct C16T {
  T re[16], im[16];
};
typedef C16T<float> C16;

// What the templates need of a value type T, in one place (a two-float vector type specialises this where it is defined):
// `fma`; `of`: T from one float (every element); `at`: T from a table entry stored twice in a row (a vector loads both of
// its elements instead of broadcasting one: a broadcast of the upper register of a loaded pair is the operand swizzle the
// build refuses).
template <class T>
struct SpOps {
  static NWS_SP_FN T fma(T a, T b, T c) { return fmaf(a, b, c); }
  static NWS_SP_FN T of(float v) { return v; }
  static NWS_SP_FN T at(const float* p) { return p[0]; }
};

// cos(2 pi m / 256), m = 0 .. 64, rounded once from float64
NWS_SP_TABLE float kSpCosQ[65] = {
    1.0f, 0.999698818f, 0.99879545f, 0.997290432f, 0.99518472f, 0.992479563f, 0.989176512f, 0.985277653f, 0.980785251f,
    0.975702107f, 0.970031261f, 0.963776052f, 0.956940353f, 0.949528158f, 0.941544056f, 0.932992816f, 0.923879504f,
    0.914209783f, 0.903989315f, 0.893224299f, 0.881921291f, 0.870086968f, 0.857728601f, 0.84485358f, 0.831469595f,
    0.817584813f, 0.803207517f, 0.78834641f, 0.773010433f, 0.757208824f, 0.740951121f, 0.724247098f, 0.707106769f,
    0.689540565f, 0.671558976f, 0.653172851f, 0.634393275f, 0.615231574f, 0.59569931f, 0.575808167f, 0.555570245f,
    0.534997642f, 0.514102757f, 0.492898196f, 0.471396744f, 0.449611336f, 0.427555084f, 0.405241311f, 0.382683426f,
    0.359895051f, 0.336889863f, 0.313681751f, 0.290284663f, 0.266712755f, 0.242980182f, 0.219101235f, 0.195090324f,
    0.170961887f, 0.146730468f, 0.122410677f, 0.0980171412f, 0.0735645667f, 0.0490676761f, 0.024541229f, 0.0f};

// (cos, sin)(2 pi m / 256), 0 <= m < 256, from the quarter-wave table
NWS_SP_FN void sp_twiddle(int m, float& c, float& s) {
  const int q = m >> 6, r = m & 63;
  const float a = kSpCosQ[r], b = kSpCosQ[64 - r];
  c = q == 0 ? a : (q == 1 ? -b : (q == 2 ? -a : b));
  s = q == 0 ? b : (q == 1 ? a : (q == 2 ? -b : -a));
}

// v * exp(-+ 2 pi i m / 256) given (c, s) = (cos, sin)(2 pi m / 256); INV: the conjugate
template <bool INV, class T>
NWS_SP_FN void sp_cmul(T& re, T& im, T cc, T s) {
  const T sg = INV ? -s : s;
  const T r = SpOps<T>::fma(re, cc, im * sg), i = SpOps<T>::fma(im, cc, -(re * sg));
  re = r;
  im = i;
}

template <bool INV, class T>
NWS_SP_FN void sp_dft4(T& r0, T& i0, T& r1, T& i1, T& r2, T& i2, T& r3, T& i3) {
  const T sr0 = r0 + r2, si0 = i0 + i2, dr0 = r0 - r2, di0 = i0 - i2;
  const T sr1 = r1 + r3, si1 = i1 + i3, dr1 = r1 - r3, di1 = i1 - i3;
  // forward: -i d1 = (d1i, -d1r);  inverse: +i d1 = (-d1i, d1r)
  if (!INV) {
    r1 = dr0 + di1; i1 = di0 - dr1;
    r3 = dr0 - di1; i3 = di0 + dr1;
  } else {
    r1 = dr0 - di1; i1 = di0 + dr1;
    r3 = dr0 + di1; i3 = di0 - dr1;
  }
  r0 = sr0 + sr1; i0 = si0 + si1;
  r2 = sr0 - sr1; i2 = si0 - si1;
}

// in-place DFT of 16 points, natural order in and out; INV: conjugate twiddles (no scaling).
// n = 4 n1 + n2, k = k1 + 4 k2:  X[k1 + 4 k2] = sum_n2 W4^(n2 k2) W16^(n2 k1) sum_n1 W4^(n1 k1) x[4 n1 + n2]
template <bool INV, class T>
NWS_SP_FN void sp_dft16(C16T<T>& v) {
  constexpr float kC[10] = {1.0f, 0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f, 0.0f,
                            -0.38268343236508977f, -0.70710678118654752f, -0.92387953251128674f, -1.0f, -0.92387953251128674f};
  constexpr float kS[10] = {0.0f, 0.38268343236508977f, 0.70710678118654752f, 0.92387953251128674f, 1.0f,
                            0.92387953251128674f, 0.70710678118654752f, 0.38268343236508977f, 0.0f, -0.38268343236508977f};
#pragma unroll
  for (int n2 = 0; n2 < 4; ++n2)      // over n1: A[n2][k1] lands at index 4 k1 + n2
    sp_dft4<INV>(v.re[n2], v.im[n2], v.re[4 + n2], v.im[4 + n2], v.re[8 + n2], v.im[8 + n2], v.re[12 + n2], v.im[12 + n2]);
#pragma unroll
  for (int k1 = 1; k1 < 4; ++k1) {
#pragma unroll
    for (int n2 = 1; n2 < 4; ++n2) {
      const int m = n2 * k1, e = 4 * k1 + n2;
      if (m == 4) {                   // -i (forward), +i (inverse)
        const T r = INV ? -v.im[e] : v.im[e], i = INV ? v.re[e] : -v.re[e];
        v.re[e] = r;
        v.im[e] = i;
      } else {
        sp_cmul<INV>(v.re[e], v.im[e], SpOps<T>::of(kC[m]), SpOps<T>::of(kS[m]));
      }
    }
  }
#pragma unroll
  for (int k1 = 0; k1 < 4; ++k1)      // over n2: X[k1 + 4 k2] lands at index 4 k1 + k2
    sp_dft4<INV>(v.re[4 * k1], v.im[4 * k1], v.re[4 * k1 + 1], v.im[4 * k1 + 1], v.re[4 * k1 + 2], v.im[4 * k1 + 2],
                 v.re[4 * k1 + 3], v.im[4 * k1 + 3]);
#pragma unroll
  for (int a = 0; a < 4; ++a) {       // 4 x 4 transpose to natural order (register renaming)
#pragma unroll
    for (int b = a + 1; b < 4; ++b) {
      const T r = v.re[4 * a + b], i = v.im[4 * a + b];
      v.re[4 * a + b] = v.re[4 * b + a];
      v.im[4 * a + b] = v.im[4 * b + a];
      v.re[4 * b + a] = r;
      v.im[4 * b + a] = i;
    }
  }
}

// rows of the 16 x 16 transpose in LDS: 17 floats, and 16 x 17 per transform.  Writers (register k, lane l) -> [k][l], readers
// (lane k, register l): 16 lanes x 4 transforms of a wave hit 64 distinct banks both ways (17 k mod 16 is a bijection).
constexpr int kSpRow = 17;
constexpr int kSpPlane = 16 * kSpRow;
constexpr int kSpTwStride = 64;

// First pass of the 256-point transform, up to the exchange (sp_fft256 of fir_spectral_wave.h: this, the transpose, sp_dft16):
//   tw: (cos, cos, sin, sin)(2 pi l k / 256) of this lane at tw[64 k .. 64 k + 3] (kSpTwStride: 16 lanes x 4 floats);
//   forward: lane l holds x[16 j + l] in register j;  after sp_dft16 + twiddle W256^(l k1), register k1 is Y[l][k1];
//   transpose: lane k1 holds Y[l][k1] in register l;  after sp_dft16, register k2 is X[k1 + 16 k2].
//   inverse: the same two passes on (lane k1, register k2) with conjugate twiddles give x[l + 16 j] in (lane l, register j).
template <bool INV, class T>
NWS_SP_FN void sp_pass1(C16T<T>& z, const float* tw) {
  sp_dft16<INV>(z);
#pragma unroll
  for (int k = 1; k < 16; ++k) sp_cmul<INV>(z.re[k], z.im[k], SpOps<T>::at(&tw[kSpTwStride * k]), SpOps<T>::at(&tw[kSpTwStride * k + 2]));
}
