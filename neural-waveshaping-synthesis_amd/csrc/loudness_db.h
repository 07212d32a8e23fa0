// The dB pass of the loudness feature for ONE frame, shared by the offline extractor (loudness.hip, reference = the clip's
// maximum power) and the loudness stream (loudness_stream.hip, reference = the causal level of DESIGN.md 3.25):
//   db(k) = k10 log2(max(amin^2, P(k))) - k10 log2(max(amin^2, ref)),   l = sum_k max(db(k), -top_db) / bins   [, (l + 80) / 80]
// The fp32 sum runs over k = 0 .. bins - 1 in that order: the order is part of both definitions (their bits are compared).
#pragma once
#include "nws_common.h"

namespace {

// p[k stride] = power of bin k of the frame; ref = the reference power the clip at -top_db hangs below
__device__ __forceinline__ float loudness_frame_db(const float* __restrict__ p, size_t stride, int bins, float ref, float amin,
                                                   float top_db, int normalise) {
  const float k10 = 3.0102999566398120f;  // 10 / log2(10)
  const float floor_p = amin * amin;
  const float ref_db = k10 * __log2f(fmaxf(floor_p, ref));
  // with ref = the maximum of the spectrogram log_spec.max() is 0 by construction, so the top_db clip sits at -top_db
  float s = 0.0f;
  for (int k = 0; k < bins; ++k) {
    const float db = k10 * __log2f(fmaxf(floor_p, p[(size_t)k * stride])) - ref_db;
    s += fmaxf(db, -top_db);
  }
  float l = s / (float)bins;
  if (normalise) l = (l + 80.0f) / 80.0f;
  return l;
}

}  // namespace
