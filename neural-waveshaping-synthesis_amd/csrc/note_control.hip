// Note player: the two small kernels around a slot stream's hop (nws_stream_step_slots, stream.hip).
//
//   note_control_kernel   in front of the hop: the frame-rate controls of every slot's held or released note - F0 in Hz and the two
//                         normalised control channels - from the hop's event words, a per-slot note table and a per-slot frame
//                         counter.  One thread per (slot, frame): 16 frame lanes per slot, 16 slots per workgroup.  Every value is
//                         a closed form in the voice's frame index j; nothing but the integer counter is carried, so a voice's bits
//                         do not depend on how its frames are cut into hops.
//   voice_mix_kernel      behind the hop: out[c, n] = sum_b gain[b, c] o[b, n], b ascending in ONE fp32 chain of fmaf per output
//                         element, every element written by one thread (no atomics: two calls give equal bits).  float4 loads and
//                         stores when every row is 16-byte aligned (N a multiple of 4, aligned bases); a row length that is not a
//                         multiple of 4 misaligns the rows behind the first, so such a call takes the scalar kernel whole.
//
// The envelope is evaluated from the end it has to hit: an attack as p - (p - q) (A - 1 - j) / A, a release as
// q + (h_off - q) (R - m) / R.  These are the definition's q + (p - q) (j + 1) / A and h_off + (q - h_off) m / R rearranged so
// that the last attack frame is p and the last release frame is q bit for bit, in any precision.
// The vibrato phase is a float64 product reduced in float64 (its error does not grow with j); everything else is fp32, with the
// library's -ffp-contract=off: the float32 restatement of tests/note_control_restatement.py follows it rounding for rounding up to
// exp2 and sin.
#include "nws_common.h"

namespace {

constexpr int kMaxFrames = 16;            // frames per hop: the slot stream's limit
constexpr int kMaxSlots = 65535;
constexpr int kMaxCount = 1 << 30;        // the frame counter saturates here (99 days at 8 ms)
constexpr int kMaxParamFrames = 1 << 24;  // A, D, R, delay, ramp: exact as fp32

__host__ __device__ inline size_t counters_bytes(int B) { return ((size_t)B * sizeof(int) + 15) & ~size_t(15); }

// h(j) of the definition; h(-1) = q
__device__ __forceinline__ float note_held_level(int j, float p, const NwsNotePlayer& P) {
  if (j < 0) return P.silence;
  if (j < P.attack) return p - (p - P.silence) * ((float)(P.attack - 1 - j) / (float)P.attack);
  if (j < P.attack + P.decay) return p - P.drop * ((float)(j - P.attack + 1) / (float)P.decay);
  return p - P.drop;
}

__global__ __launch_bounds__(256) void note_control_kernel(const int* __restrict__ ev, const NwsNote* __restrict__ notes,
                                                           int* __restrict__ counter, int B, int K, NwsNotePlayer P,
                                                           float* __restrict__ f0, float* __restrict__ control) {
  const int k = threadIdx.x & (kMaxFrames - 1);
  const int b = blockIdx.x * (256 / kMaxFrames) + (threadIdx.x >> 4);
  int e = 0, base = 0;
  if (b < B) {
    e = ev[b];
    base = (e & NWS_SLOT_START) ? 0 : counter[b];
  }
  __syncthreads();   // every frame lane of a slot has read its counter
  if (b >= B) return;
  const bool active = (e & NWS_SLOT_ACTIVE) != 0;
  if (k == 0 && active) counter[b] = min(base + K, kMaxCount);
  if (k >= K) return;
  float f = 0.0f, c0 = 0.0f, c1 = 0.0f;   // an idle or releasing slot: finite values the stream never reads into an output
  if (active) {
    const NwsNote n = notes[b];
    const int j = base + k;
    const int j_off = max(n.j_off, 0);
    const float p = P.peak_lo + n.velocity * (P.peak_hi - P.peak_lo);
    float l;
    if (j < j_off) {
      l = note_held_level(j, p, P);
    } else {
      const float h_off = note_held_level(j_off - 1, p, P);
      const int m = min(j - j_off + 1, P.release);
      l = P.silence + (h_off - P.silence) * ((float)(P.release - m) / (float)P.release);
    }
    const float r = fminf(fmaxf((float)(j - P.vib_delay) / (float)P.vib_ramp, 0.0f), 1.0f);
    const double turns = P.vib_rate * (double)NWS_HOP * (double)j / P.sample_rate;
    const float frac = (float)(turns - floor(turns));
    const float cents = P.vib_depth * r * __builtin_amdgcn_sinf(frac);   // v_sin_f32 takes its argument in turns
    f = 440.0f * exp2f((n.pitch - 69.0f) / 12.0f + cents / 1200.0f);
    c0 = (f - P.mean[0]) / P.std[0];
    c1 = (l - P.mean[1]) / P.std[1];
  }
  f0[(size_t)b * K + k] = f;
  control[((size_t)b * 2 + 0) * K + k] = c0;
  control[((size_t)b * 2 + 1) * K + k] = c1;
}

template <int C>
__global__ __launch_bounds__(256) void voice_mix_vec_kernel(const float* __restrict__ o, const float* __restrict__ gain, int B,
                                                            int N, float* __restrict__ out) {
  const int n = 4 * (blockIdx.x * 256 + threadIdx.x);
  if (n >= N) return;   // N is a multiple of 4 here
  float4 acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll 4
  for (int b = 0; b < B; ++b) {
    const float4 v = *reinterpret_cast<const float4*>(o + (size_t)b * N + n);
#pragma unroll
    for (int c = 0; c < C; ++c) {
      const float g = gain[(size_t)b * C + c];
      acc[c].x = fmaf(g, v.x, acc[c].x);
      acc[c].y = fmaf(g, v.y, acc[c].y);
      acc[c].z = fmaf(g, v.z, acc[c].z);
      acc[c].w = fmaf(g, v.w, acc[c].w);
    }
  }
#pragma unroll
  for (int c = 0; c < C; ++c) *reinterpret_cast<float4*>(out + (size_t)c * N + n) = acc[c];
}

template <int C>
__global__ __launch_bounds__(256) void voice_mix_scalar_kernel(const float* __restrict__ o, const float* __restrict__ gain, int B,
                                                               int N, float* __restrict__ out) {
  const long long n = (long long)blockIdx.x * 256 + threadIdx.x;
  if (n >= N) return;
  float acc[C];
#pragma unroll
  for (int c = 0; c < C; ++c) acc[c] = 0.0f;
#pragma unroll 4
  for (int b = 0; b < B; ++b) {
    const float v = o[(size_t)b * N + n];
#pragma unroll
    for (int c = 0; c < C; ++c) acc[c] = fmaf(gain[(size_t)b * C + c], v, acc[c]);
  }
#pragma unroll
  for (int c = 0; c < C; ++c) out[(size_t)c * N + n] = acc[c];
}

template <int C>
__host__ void launch_mix(const float* o, const float* gain, int B, int N, float* out, hipStream_t st) {
  const bool vec = N % 4 == 0 && (((uintptr_t)o | (uintptr_t)out) & 15) == 0;
  if (vec) {
    voice_mix_vec_kernel<C><<<(N / 4 + 255) / 256, 256, 0, st>>>(o, gain, B, N, out);
  } else {
    voice_mix_scalar_kernel<C><<<(unsigned)(((long long)N + 255) / 256), 256, 0, st>>>(o, gain, B, N, out);
  }
}

__host__ bool frames_ok(int v, int least) { return v >= least && v <= kMaxParamFrames; }

}  // namespace

extern "C" {

size_t nws_note_control_state_bytes(int B) { return B >= 1 && B <= kMaxSlots ? counters_bytes(B) : 0; }

int nws_note_control_reset(void* state, size_t state_bytes, int B, void* stream) {
  if (!state || B < 1) return NWS_ERR_BAD_ARG;
  if (B > kMaxSlots) return NWS_ERR_UNSUPPORTED;
  if (state_bytes < counters_bytes(B)) return NWS_ERR_BAD_ARG;
  const hipError_t e = hipMemsetAsync(state, 0, counters_bytes(B), (hipStream_t)stream);
  return e == hipSuccess ? NWS_OK : (int)e;
}

int nws_note_control(const NwsNotePlayer* player, const int* events, const NwsNote* notes, void* state, size_t state_bytes, int B,
                     int K, float* f0, float* control, void* stream) {
  if (!player || !events || !notes || !state || !f0 || !control) return NWS_ERR_BAD_ARG;
  if (B < 1 || K < 1 || K > kMaxFrames) return NWS_ERR_BAD_ARG;
  const NwsNotePlayer& P = *player;
  if (!frames_ok(P.attack, 0) || !frames_ok(P.decay, 0) || !frames_ok(P.release, 1) || !frames_ok(P.vib_delay, 0) ||
      !frames_ok(P.vib_ramp, 1))
    return NWS_ERR_BAD_ARG;
  if (!(P.sample_rate > 0.0) || !(P.vib_rate >= 0.0) || !(P.std[0] > 0.0f) || !(P.std[1] > 0.0f) || !(P.drop >= 0.0f))
    return NWS_ERR_BAD_ARG;
  if (B > kMaxSlots) return NWS_ERR_UNSUPPORTED;
  if (state_bytes < counters_bytes(B)) return NWS_ERR_BAD_ARG;
  const int per_block = 256 / kMaxFrames;
  note_control_kernel<<<(B + per_block - 1) / per_block, 256, 0, (hipStream_t)stream>>>(events, notes, static_cast<int*>(state), B, K,
                                                                                       P, f0, control);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

int nws_voice_mix(const float* o, const float* gain, int B, int N, int C, float* out, void* stream) {
  if (!o || !gain || !out || B < 1 || N < 1 || (C != 1 && C != 2)) return NWS_ERR_BAD_ARG;
  if (B > kMaxSlots) return NWS_ERR_UNSUPPORTED;
  if (C == 1) launch_mix<1>(o, gain, B, N, out, (hipStream_t)stream);
  else launch_mix<2>(o, gain, B, N, out, (hipStream_t)stream);
  NWS_CHECK_LAUNCH();
  return NWS_OK;
}

}  // extern "C"
