// The releasing reference level of DESIGN.md 3.26, one step of it, shared by the loudness stream (loudness_stream.hip) and the
// whole-clip extractor (loudness_causal.hip):
//   d = rho M(t - 1);  if d < 2^-126: d = 0;  M(t) = max(p(t), F, d)          rho in (0, 1), fp32, one product, nothing fused
// The explicit flush makes the result independent of the denormal mode.  rho = 1 is the running maximum of 3.25, max(M(t - 1),
// p(t)): the product is exact there, nothing is flushed, and M >= F holds by induction from M(-1) = F.
#pragma once
#include "nws_common.h"

namespace {

__device__ __forceinline__ float loudness_level_step(float M, float p, float F, float rho) {
  if (!(rho < 1.0f)) return fmaxf(M, p);
  float d = __fmul_rn(rho, M);
  if (d < 1.17549435e-38f) d = 0.0f;   // 2^-126
  return fmaxf(fmaxf(p, F), d);
}

}  // namespace
