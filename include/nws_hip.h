/*
 * nws_hip.h — C-ABI of the MI355X (gfx950) NEWT synthesis engine.
 *
 * The reference (ben-hayes/neural-waveshaping-synthesis) has no FFI: its hot path sits behind
 * a Python nn.Module.  This header is the drop-in boundary *below* that
 * surface: every entry point replaces one block of ATen calls made by the reference's
 * forward().  Citations are relative to /root/reference/neural_waveshaping_synthesis/.
 *
 * Conventions
 *   - plain pointers and sizes only; all pointers are DEVICE pointers to contiguous fp32 unless
 *     stated otherwise; `stream` is a hipStream_t passed as void* (NULL = default stream).
 *   - every launcher returns 0 on success, a positive hipError_t if the HIP runtime failed, or
 *     one of the negative NWS_ERR_* codes below.  Nothing is synchronised: work is enqueued on
 *     `stream` exactly like the ATen ops it replaces.
 *   - kernels are specialised for the architecture of gin/models/newt.gin (the only one the
 *     reference ships): 101 harmonics, 64 waveshapers, hidden/embedding 128, shaper MLP width 8
 *     depth 4, control hop 128, FIR length 256.  Other sizes return NWS_ERR_UNSUPPORTED.
 *   - B = batch, T = control frames, N = 128*T samples.
 *   - the analysis front end in front of the forward path (data/utils/ of the reference) takes audio (B, N) of any
 *     length: nws_resample (any integer sample rate to any other), nws_loudness, nws_pyin, nws_mfcc.  Their constant
 *     operands (weight bank, DFT matrix, fp64 table, filter table) are built once per configuration by the entry points
 *     beside them.  Chunked audio: nws_resample_stream_*, nws_pyin_stream_* and nws_loudness_stream_* keep their state in a blob.
 */
#ifndef NWS_HIP_H
#define NWS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NWS_ABI_VERSION 6

#define NWS_N_HARMONICS 101
#define NWS_N_SHAPERS 64
#define NWS_HIDDEN 128
#define NWS_HOP 128
#define NWS_FIR_LEN 256
#define NWS_N_BANDS 129      /* FIR_LEN/2 + 1 */
#define NWS_FIR_HALF 128     /* taps handed from the frame MLPs to the noise kernel per frame: h[128 .. 255] (see nws_frame_mlps) */
#define NWS_SHAPER_WIDTH 8
#define NWS_FILM_CH 256      /* 4 * N_SHAPERS */

enum {
  NWS_OK = 0,
  NWS_ERR_UNSUPPORTED = -1, /* sizes outside the compiled specialisation */
  NWS_ERR_BAD_ARG = -2,     /* NULL / non-positive / misaligned argument */
  NWS_ERR_WORKSPACE = -3    /* workspace too small */
};

/* Device pointers to the parameters, in the reference's own state_dict layouts. */
typedef struct NwsWeights {
  /* embedding = ControlModule (models/neural_waveshaping.py:17-26) */
  const float* gru_w_ih;  /* (384, 2)   rows [r; z; n] */
  const float* gru_w_hh;  /* (384, 128) */
  const float* gru_b_ih;  /* (384) */
  const float* gru_b_hh;  /* (384) */
  const float* proj_w;    /* (128, 128) Conv1d k=1 */
  const float* proj_b;    /* (128) */
  /* harmonic_mixer = Conv1d(101, 64, 1) (models/neural_waveshaping.py:54) */
  const float* mixer_w;   /* (64, 101) */
  const float* mixer_b;   /* (64) */
  const void* mixer_frags; /* optional 28672 B from nws_mixer_frags(): [mixer_b | mixer_w] as two fp16 terms in MFMA
                              fragment order; NULL -> every workgroup splits the weights itself (slower prologue) */
  /* newt.mlp = TimeDistributedMLP(128,128,256,depth=4) (models/modules/shaping.py:53-55) */
  const float* newt_mlp_w[4]; /* (128,128) x3, (256,128) */
  const float* newt_mlp_b[4];
  const float* newt_ln_g[3];  /* LayerNorm weight (128) */
  const float* newt_ln_b[3];
  /* h_generator = TimeDistributedMLP(128,128,129,depth=4) (models/neural_waveshaping.py:58-59) */
  const float* hgen_w[4];     /* (128,128) x3, (129,128) */
  const float* hgen_b[4];
  const float* hgen_ln_g[3];
  const float* hgen_ln_b[3];
  /* optional NWS_MLP_FRAGS_BYTES from nws_mlp_frags(): proj / newt.mlp / h_generator / FIR-design weights as two fp16 terms in MFMA
   * fragment order -> frame MLPs on the fp16 matrix pipe; NULL -> exact-fp32 MFMA kernel */
  const void* mlp_frags;
  /* newt.shaping_fn = TrainableNonlinearity(64, 8, depth=4) (models/modules/shaping.py:15-37) */
  const float* shaper_in_scale; /* (64) */
  const float* shaper_w0; /* (512)    net.0.weight (512,1,1) */
  const float* shaper_b0; /* (512) */
  const float* shaper_w2; /* (512, 8) net.2.weight */
  const float* shaper_b2; /* (512) */
  const float* shaper_w4; /* (512, 8) net.4.weight */
  const float* shaper_b4; /* (512) */
  const float* shaper_w6; /* (64, 8)  net.6.weight */
  const float* shaper_b6; /* (64) */
  const float* shaper_turns; /* optional (64, NWS_SHAPER_TURNS_ROW) from nws_shaper_turns(): all four layers of each shaper
                                times 1/(2 pi), hidden layers transposed, read by scalar loads; NULL -> weights staged in
                                LDS per workgroup (slower exact mode) */
  /* FastNEWT.lookup_table (models/modules/shaping.py:103-105); NULL selects the exact shapers */
  const float* lut;       /* (64, lut_size) */
  const float* lut_pairs; /* optional (64, lut_size, 2) from nws_lut_pairs(): {T[i], T[i+1]-T[i]}; NULL -> two gathers */
  int32_t lut_size;       /* 4096 */
  float lut_min;          /* -3 */
  float lut_max;          /* +3 */
  /* newt.mixer = Conv1d(64, 1, 1) (models/modules/shaping.py:63-65) */
  const float* newt_out_w; /* (64) */
  const float* newt_out_b; /* (1) */
  /* noise_synth.window (models/modules/generators.py:20), periodic Hann(256) */
  const float* noise_window; /* (256) */
  /* options of the fused oscillator + waveshaper kernel's FastNEWT path (0 = default: FiLM interpolation on the matrix
   * pipe, sines as two fp16 terms = 22-bit products) */
  int32_t exciter_opts;
  /* nonzero: mlp_frags is NWS_MLP_FRAGS_BYTES + NWS_MLP_SPEC_BYTES long and nws_mlp_spec_frags() has filled the second part (proj
   * folded into the first hidden layers, h_generator's output layer emitting filter spectra): the forward may hand spectra
   * instead of taps from the frame MLPs to the noise kernel (nws_frame_mlps_spec).  Sits in what was padding: a caller that
   * zero-fills the struct and never sets it keeps the tap hand-over. */
  int32_t mlp_spec;
  /* optional (64) from nws_exciter_bound(): X[s] >= |harmonic_mixer output of shaper s| for ANY phases (sum_k |W[s][k]| + |b[s]|,
   * rounded up).  With it the fused kernel proves per workgroup, from the FiLM rows it stages, which groups of eight shapers keep
   * their table index inside the table whatever the oscillator does, and runs those lookups without floor / clamp (bit-identical
   * there; everything else takes the reference's clamped form, shaping.py:136-151).  NULL -> every lookup clamped. */
  const float* exciter_bound;
} NwsWeights;
#define NWS_EXCITER_VALU_FILM 1 /* round-1 form: FiLM parameters interpolated on the VALU (kept for A/B timing) */
#define NWS_EXCITER_ONE_TERM 2  /* sines as ONE fp16 term: 2 instead of 3 MFMAs per product and no residual split (-15 %
                                   kernel time); mixer inputs carry 11 bits: 4e-6 .. 1.1e-5 RMS end to end on the shipped
                                   checkpoints instead of ~3e-7 */
#define NWS_EXCITER_HYBRID 4    /* two fp16 terms for the mixer bias + harmonics 1..15 (K-step 0: 61-85 % of the mixer's
                                   weight energy in the shipped checkpoints), one term for harmonics 16..101 */
#define NWS_EXCITER_HYBRID_W 8  /* NWS_EXCITER_HYBRID plus: the mixer WEIGHTS of harmonics 16..101 as one fp16 term as well
                                   (one MFMA per product there instead of two) */
#define NWS_EXCITER_BANK_NOFRACT 16 /* exact sin-MLP shapers (shaping.py:36-37): the hidden and output layers' pre-activations are
                                   provably inside v_sin_f32's own +-256-turn domain (sum |W| + |b| per row, checked by the caller
                                   from the weights), so their sines skip the v_fract: 17 of an evaluation's 25 (the 8 first-layer sines keep it: their argument is unbounded) */

int nws_abi_version(void);
/* sizeof of the C structs above as this library was compiled (0 NwsWeights, 1 NwsReverbPlan, 2 NwsForwardAux, 3 NwsShaperDesc, 4 NwsGenericModel): lets a
 * foreign-language binding verify its own struct declarations at load time */
size_t nws_sizeof(int which);
const char* nws_error_string(int code);

/* ---- hardware self-test: MFMA fragment layout the kernels rely on (returns #mismatches in *bad) ---- */
int nws_selftest_mfma(int32_t* bad_out /* device int32[1] */, void* stream);

/* ---- accurate sinf used by the oscillator / shapers, exposed for testing: y[i] = sin(x[i]) ---- */
int nws_sin(const float* x, float* y, int64_t n, void* stream);

/*
 * Exciter phase carries.  Replaces the double-accumulated torch.cumsum of
 * models/modules/generators.py:59 at 32-sample granularity:
 *   carry[b][c] = sum_{n < 32c} f0_up[b][n]   (float64, exclusive)
 * f0 (B,T) Hz frames are linearly upsampled x128 on the fly exactly like
 * F.upsample(mode="linear") (models/neural_waveshaping.py:75); if f0_up != NULL the (B,N)
 * already-upsampled F0 is used instead (public render_exciter(), :64-67).
 */
int nws_phase_carry(const float* f0, const float* f0_up, int B, int T, double* carry /* (B, N/32) */, void* stream);

/*
 * Fused harmonic exciter + waveshaper bank:
 *   HarmonicOscillator.forward (models/modules/generators.py:58-66)
 *   harmonic_mixer Conv1d 101->64 (models/neural_waveshaping.py:66)
 *   NEWT.forward / FastNEWT.shaping_fn: FiLM -> shaper (LUT or sin-MLP) -> FiLM -> Conv1d 64->1
 *   (models/modules/shaping.py:67-79, :136-151)
 * film: (B, T, 256) frame-major FiLM parameters [g_idx | b_idx | g_norm | b_norm] (output of
 *       nws_frame_mlps), linearly upsampled on the fly (shaping.py:69).
 * phase_u: (101) the U[0,1) draws of generators.py:55; rand_phase: (101) the osc.rand_phase buffer (= tau);
 *          the kernel forms shift = fl(fl(u * rand_phase) - pi) exactly like _create_phase_shift.
 * exciter_out: optional (B, 64, N) materialised exciter (render_exciter()); newt_out: optional (B, N).
 */
int nws_exciter_newt(const NwsWeights* w, const float* f0, const float* f0_up, const double* carry,
                     const float* phase_u, const float* rand_phase, const float* film, int B, int T,
                     float sample_rate, float* exciter_out, float* newt_out, void* stream);
/* same with newt_out = add_in + NEWT sum; add_in (B, N) or NULL (the noise branch of neural_waveshaping.py:81 when the
 * FIR-noise kernel ran first); add_in may not alias newt_out */
int nws_exciter_newt_add(const NwsWeights* w, const float* f0, const float* f0_up, const double* carry,
                         const float* phase_u, const float* rand_phase, const float* film, const float* add_in, int B,
                         int T, float sample_rate, float* exciter_out, float* newt_out, void* stream);

/*
 * Control encoder: GRU(2->128, h0=0) over T frames of control[:, 0:2]
 * (models/neural_waveshaping.py:69-72, :24-25).  control: (B, C, T) with C >= 2.
 * gru_out: (B, T, 128).
 */
int nws_control_gru(const NwsWeights* w, const float* control, int B, int C, int T, float* gru_out, void* stream);
/* same with an explicit initial state h0 (B,128) [NULL = zeros] and the final state written to hT (B,128) [NULL = dropped]:
 * stateful streaming; the reference's forward is the h0 = 0 case */
int nws_control_gru_state(const NwsWeights* w, const float* control, int B, int C, int T, const float* h0, float* gru_out,
                          float* hT, void* stream);
/* nws_control_gru + nws_phase_carry in ONE launch (grid 2B: B workgroups run the recurrences, B more compute the carries
 * beside them): the control-rate half of a forward; f0 (B,T) Hz, carry_out (B, 4T) doubles */
int nws_control_gru_carry(const NwsWeights* w, const float* control, const float* f0, int B, int C, int T, float* gru_out,
                          double* carry_out, void* stream);
/* the same recurrence, 16 utterances per workgroup on the matrix cores (fp16 two-term split, fp32 accumulate): ~2x the
 * latency of the per-utterance kernel above but ~1/10 of its VALU work per utterance and 1/16 of its workgroups -- the
 * form to run beside throughput kernels of other streams (nws_forward_control, batched_gru = 1).  Any B >= 1. */
int nws_control_gru_batched(const NwsWeights* w, const float* control, int B, int C, int T, const float* h0, float* gru_out,
                            float* hT, void* stream);
/* The backward of nws_control_gru_state for grad_out = dL/d(gru_out) (B, T, 128) and grad_hT = dL/d(hT) (B, 128)
 * [NULL = zeros].  control, h0 and gru_out are the forward's own input, initial state [NULL = zeros] and output: the recurrence is
 * not run again.  grad_control (B, 2, T) [NULL = not wanted] is the gradient of channels 0 and 1 of control (the only ones read;
 * C >= 2 is control's channel count), grad_h0 (B, 128) [NULL = dropped], and grad_w_ih (384, 2), grad_w_hh (384, 128), grad_b_ih
 * (384), grad_b_hh (384) - all four or none - the gradients of w->gru_*.  Exact fp32 products, sums over batch and time in a fixed
 * order in float64, no atomics: equal inputs give equal bits, grad_out = 0 without grad_hT gives zeros.
 * Launches on `stream` (gate coefficients, the sequential kernel, then - when asked for - the input gradient with the column sums,
 * the dW_hh contraction and two reductions), reads nothing back and decides every refusal before the first launch:
 * NWS_ERR_BAD_ARG for a NULL required pointer, some but not all of the four parameter gradients, a size < 1, C < 2, or a workspace
 * that is NULL, not 16-byte aligned or smaller than nws_control_gru_grad_workspace_bytes; NWS_ERR_UNSUPPORTED for B > 65 535 (or
 * more than 2^30 32-frame chunks in all).  The workspace (six (B, T, 128) planes, with want_params the partial sums too) is needed
 * in every form; nws_control_gru_grad_workspace_bytes is 0 for sizes that are refused. */
size_t nws_control_gru_grad_workspace_bytes(int B, int T, int want_params);
int nws_control_gru_grad(const NwsWeights* w, const float* control, int B, int C, int T, const float* h0 /* NULL = zeros */,
                         const float* gru_out, const float* grad_out /* (B,T,128) */, const float* grad_hT /* NULL = zeros */,
                         float* grad_control /* (B,2,T), NULL = not wanted */, float* grad_h0 /* (B,128), NULL = dropped */,
                         float* grad_w_ih, float* grad_w_hh, float* grad_b_ih, float* grad_b_hh /* all four or none */,
                         void* workspace, size_t workspace_bytes, void* stream);

/*
 * Frame-rate MLPs on the GRU output (one kernel):
 *   emb  = proj(gru_out)                         models/neural_waveshaping.py:26
 *   film = newt.mlp(emb)                         models/modules/shaping.py:68, dynamic.py:20-40
 *   H    = h_generator(emb)                      models/neural_waveshaping.py:82
 *   fir  = window * roll(irfft(H), 128)          models/modules/generators.py:22-27 (zero-phase FIR design)
 * emb_out (B,128,T) [optional], film_out (B,T,256), H_out (B,T,129) [optional], fir_out (B,T,128).
 * fir_design: (256, 132) constant matrix from nws_fir_design_matrix().
 * fir_out holds the UPPER HALF of every frame's taps, u[d] = h[128 + d], d = 0..127: H is real, so irfft(H) is even and with
 * a window symmetric about tap 128 whose tap 0 is zero (the reference's periodic Hann, generators.py:20) the rolled,
 * windowed response satisfies h[128 - d] = h[128 + d], h[0] = 0.  Half the bytes between the two kernels; the noise
 * kernels mirror the row while staging it.  The caller checks the window (engine.py: any other window takes the
 * runtime-size path, whose nws_g_fir_design emits full rows).
 */
int nws_frame_mlps(const NwsWeights* w, const float* gru_out, const float* fir_design, int B, int T,
                   float* emb_out, float* film_out, float* H_out, float* fir_out, void* stream);

/* pre-split weight fragments for the fp16 two-term frame-MLP kernel (valid while |layer inputs| stay inside fp16 range:
 * the caller checks the weight-norm bounds, see engine.py) */
#define NWS_MLP_FRAGS_BYTES 1474560
int nws_mlp_frags(const NwsWeights* w, const float* fir_design /* (256,132) */, void* frags_out, void* stream);

/* D[n][k]: fir[n] = sum_k D[n][k] H[k]  (irfft + roll(128) + window folded), (256, 132) fp32, cols 129..131 = 0. */
int nws_fir_design_matrix(const float* window /* (256) */, float* D_out, void* stream);

/*
 * Spectrum hand-over.  Everything between the GRU output and the first LayerNorm of either frame MLP, and
 * everything between h_generator's last LayerNorm and the noise kernel's product of spectra, is linear in model constants:
 *   W1' = W1 Wp, b1' = W1 bp + b1          proj folded into the first Conv1d of newt.mlp and of h_generator
 *   W_G = S W_out, b_G = S b_out           h_generator's last layer emits G = S H, the REAL spectrum of the frame's zero-phase filter
 * S (129 x 129) is bands -> spectrum in exactly the form the noise kernel multiplies with: u[d] = D[128 + d] H are the stored
 * half-taps, e[n] = u[min(n, 256 - n)] (u[128] := 0) the even extension, G[k] = sum_n e[n] cos(2 pi k n / 256), k = 0 .. 128
 * (forward transform, no scaling, bin k at index k; G[256 - k] = G[k]).  It depends on noise_synth.window only.
 * nws_fir_spectrum_map and nws_mlp_spec_fold are HOST functions on host pointers (float64 sums rounded once to fp32; no GPU):
 *   folded_out: [W1' newt.mlp (128,128) | W1' h_generator (128,128) | W_G (129,128) | b1' newt.mlp (128) | b1' h_generator (128) |
 *                b_G (129) + 3 zeros]
 * nws_mlp_spec_frags splits a device copy of `folded` into the fragment order of the wave-resident kernel and writes the
 * NWS_MLP_SPEC_BYTES behind the first NWS_MLP_FRAGS_BYTES of `frags` (which nws_mlp_frags fills).  The caller checks the folded
 * weights against the fp16 range (engine.py) before it sets NwsWeights.mlp_spec.
 */
#define NWS_SPEC_ROW 132             /* floats per (utterance, frame) row of filter spectra: G[0 .. 128], 16-byte aligned rows */
#define NWS_MLP_SPEC_BYTES 200704
#define NWS_MLP_SPEC_FOLD_FLOATS 49668
int nws_fir_spectrum_map(const float* fir_design /* host (256,132) */, double* S_out /* host (129,129) */);
int nws_mlp_spec_fold(const float* proj_w, const float* proj_b, const float* newt_w0, const float* newt_b0, const float* hgen_w0,
                      const float* hgen_b0, const float* hgen_w3 /* (129,128) */, const float* hgen_b3 /* (129) */,
                      const double* S /* (129,129) */, float* folded_out /* NWS_MLP_SPEC_FOLD_FLOATS */);
int nws_mlp_spec_frags(const float* folded /* device */, void* frags /* device, NWS_MLP_FRAGS_BYTES + NWS_MLP_SPEC_BYTES */, void* stream);
/* 1 when nws_frame_mlps_spec / nws_fir_noise_spec serve this size: w->mlp_frags and w->mlp_spec are set, nws_frame_mlps would take
 * its wave-resident kernel (B x T frames fill the chip) and nws_fir_noise its batched kernel (B >= 16); else 0 */
int nws_frame_mlps_spec_serves(const NwsWeights* w, int B, int T);
/* nws_frame_mlps with the folded weights: film_out (B,T,256) as before, spec_out (B,T,NWS_SPEC_ROW) rows G[0 .. 128] (the three
 * floats behind them are not written).  NWS_ERR_UNSUPPORTED where nws_frame_mlps_spec_serves is 0. */
int nws_frame_mlps_spec(const NwsWeights* w, const float* gru_out, int B, int T, float* film_out, float* spec_out, void* stream);
/* The same launch for a caller that runs it apart from the recurrence that produced gru_out (the audio half of a pipeline), so
 * that the per-utterance recurrence of a neighbouring batch of B utterances is expected to hold B compute units meanwhile
 * (beside_recurrence != 0).  Where the 2 ceil(B T / 256) workgroups of the 8-wave kernel no longer fit the remaining compute
 * units in one round and the 2 ceil(B T / 384) workgroups of its 12-wave form do, that form runs: the same bits.
 * nws_frame_mlps_spec_waves answers which form it would be (8 or 12; 0 where nws_frame_mlps_spec_serves is 0) and launches nothing. */
int nws_frame_mlps_spec_beside(const NwsWeights* w, const float* gru_out, int B, int T, float* film_out, float* spec_out,
                               int beside_recurrence, void* stream);
int nws_frame_mlps_spec_waves(const NwsWeights* w, int B, int T, int beside_recurrence);

/*
 * Time-varying FIR noise (models/modules/generators.py:30-35): rectangular-window STFT of the
 * shared noise vector (N-1 samples, reflect-padded by 128), per-frame 256-point CIRCULAR
 * convolution with fir[b][t], overlap-add / overlap count.   out = add_in + noise_branch
 * (the cat+sum of models/neural_waveshaping.py:85-86); add_in may be NULL.
 */
int nws_fir_noise(const float* fir /* (B,T,128): upper half-taps, see nws_frame_mlps */, const float* noise /* (N-1) */, const float* add_in /* (B,N) */,
                  int B, int T, float* out /* (B,N) */, void* stream);
/* general form: STFT frame t covers noise[128 t - origin, 128 t - origin + 256), reflected about 0 and noise_len-1 like
 * torch.stft's reflect padding (nws_fir_noise == origin 128, noise_len N-1); streaming windows use origin 0 */
int nws_fir_noise_window(const float* fir, const float* noise, int noise_len, int origin, const float* add_in, int B, int T,
                         float* out, void* stream);
/* nws_fir_noise on rows of filter spectra (nws_frame_mlps_spec: spec[b][t][k] = G[k], k = 0 .. 128, row stride NWS_SPEC_ROW)
 * instead of half-taps: the batched kernel without its tap loads, mirror exchange and filter transform; everything behind the
 * product of spectra is the same code.  B >= 16 only (NWS_ERR_UNSUPPORTED below; the per-utterance kernel convolves taps). */
int nws_fir_noise_spec(const float* spec /* (B,T,NWS_SPEC_ROW) */, const float* noise /* (N-1) */, const float* add_in /* (B,N) */,
                       int B, int T, float* out /* (B,N) */, void* stream);

/* The transpose of nws_fir_noise and of nws_fir_from_h for g = dL/d(out) (B,N), N = 128 T.  For a fixed
 * excitation the noise branch is linear in H, so nothing is saved but the noise vector.  Whole-clip form only (origin 128,
 * noise_len N-1); the windowed streaming form has no backward, and neither the excitation nor the design matrix gets a gradient.
 *   g^[j]          = g[b,j] / c[j] (c = 1 for j < 128, else 2; 0 for N <= j < N + 128: the cropped half of frame T-1)
 *   dh[b,t,m]      = sum_{n<256} g^[128 t + n] x_t[(n - m) mod 256],  x_t[n] = noise[refl(128 (t-1) + n)]
 *   grad_fir[b,t,d] = dh[b,t,128+d] + dh[b,t,128-d] (d = 1..127), dh[b,t,128] (d = 0): the gradient of the stored half row
 *   grad_H[b,k,t]  = sum_{d<128} fir_design[128+d][k] grad_fir[b,t,d]
 * nws_fir_noise_grad: one launch, per frame pair one forward and one inverse 256-point transform, the noise spectra once per
 * workgroup; every row of grad_fir is written by one wave, no atomics: equal inputs give equal bits.  nws_fir_from_h_grad: one
 * launch, plain fp32, summed over d in order.  Both launch on `stream`, read nothing back and decide every refusal before the
 * launch: NWS_ERR_BAD_ARG for a NULL pointer, B < 1 or T < 2; NWS_ERR_UNSUPPORTED for T > 2^23, more than 2^30 workgroups
 * (nws_fir_noise_grad: ceil(T/8) ceil(B/8)) or B > 65 535 (nws_fir_from_h_grad). */
int nws_fir_noise_grad(const float* noise /* (N-1) */, const float* grad_out /* (B,N) */, int B, int T,
                       float* grad_fir /* (B,T,128) */, void* stream);
int nws_fir_from_h_grad(const float* grad_fir /* (B,T,128) */, const float* fir_design /* (256,132) */, int B, int T,
                        float* grad_H /* (B,129,T) */, void* stream);
/* out[c] = sum over b and t of x[b,c,t], accumulated in float64 in a fixed order (per channel: 256 partial sums, each over
 * t = i, i + 256, ... of utterance 0, 1, ... in turn, then a fixed tree), rounded once to fp32: equal inputs give equal bits.  Carries a gradient of shape (B,C,T) onto a
 * per-channel offset.  NWS_ERR_BAD_ARG for a NULL pointer or a size < 1. */
int nws_sum_batch_time(const float* x /* (B,C,T) */, int B, int C, int T, float* out /* (C) */, void* stream);

/* ---- learned reverb (models/modules/shaping.py:161-173): y = x + circconv_Lc(x, [0, ir])[:N], Lc = max(N, ir_len+1) ----
 * A plan exists for EVERY even circular length (the reference takes any N; for an odd Lc its rfft / irfft pair is not a
 * circular convolution at all - runtime-size path, nws_g_reverb_direct).  Two forms:
 *   direct (Lc == 0): the L-point four-step transform IS the circular convolution, L = max(N, ir_len+1) = N1 * N2 with
 *     N1 = 125 (radix-5 column pass) or N1 <= 128 (DFT-matrix column pass on the matrix cores);
 *   overlap-save (Lc > 0): every other length.  The signal is read as Lc-periodic (zeros between N and Lc); block j of
 *     L = 125 * 2^k points starts `hist` = ir_len samples before output j * (L - hist), its last L - hist points are
 *     final samples of the circular convolution - the wrap-around is in the loads, nothing is folded afterwards.
 *     nblk = ceil(N / (L - hist)) transforms per utterance pair instead of one. */
typedef struct NwsReverbPlan {
  int32_t L;     /* transform length */
  int32_t N1;    /* column-DFT size  (L = N1 * N2) */
  int32_t N2;    /* row-FFT size, power of two, 32 .. 4096 */
  int32_t Lc;    /* 0: direct; else the reference's circular length, served by overlap-save blocks of L points */
  int32_t hist;  /* overlap-save: samples of history in front of every block (= ir_len); 0 when direct */
  int32_t nblk;  /* transforms per utterance pair (1 when direct) */
  int32_t reserved[2];
} NwsReverbPlan;

int nws_reverb_plan(int N, int ir_len_plus1, NwsReverbPlan* plan /* host */);
/* 1 when `plan` renders Reverb.forward for N samples (ir_len_plus1 > 0: and for that impulse-response length), else 0 */
int nws_reverb_plan_serves(const NwsReverbPlan* plan, int N, int ir_len_plus1);
/* bytes of the constant tables (DFT matrices + twiddles) and of the IR spectrum for a plan */
size_t nws_reverb_table_bytes(const NwsReverbPlan* plan);
size_t nws_reverb_spectrum_bytes(const NwsReverbPlan* plan);
size_t nws_reverb_workspace_bytes(const NwsReverbPlan* plan, int B);
int nws_reverb_build_tables(const NwsReverbPlan* plan, void* tables, void* stream);
/* spectrum of ir_ = [0, ir] zero-padded to L, in the engine's own (k1,k2) order; the buffer (nws_reverb_spectrum_bytes =
 * 3 L floats) holds Sre | Sim | ir_ itself, which nws_reverb uses for buffers of <= 1024 samples (time-domain form) */
int nws_reverb_ir_spectrum(const NwsReverbPlan* plan, const void* tables, const float* ir, int ir_len,
                           void* spectrum, void* workspace, size_t workspace_bytes, void* stream);
int nws_reverb(const NwsReverbPlan* plan, const void* tables, const void* spectrum, const float* x /* (B,N) */,
               int B, int N, float* y /* (B,N) */, void* workspace, size_t workspace_bytes, void* stream);

/* The transpose of nws_reverb for g = dL/dy (B,N), same plan, tables and spectrum:
 *   dx[b,i]  = g[b,i] + sum_m h[m] g_[b,(i+m) mod Lc]           i < N          (circular correlation with h = [0, ir, 0...])
 *   dir[j-1] = sum_b sum_{n<N} g[b,n] x_[b,(n-j) mod Lc]        j = 1..ir_len  (summed over the batch)
 * grad_x is the forward's three launches with the conjugated spectrum; grad_ir transforms the x pairs and the g pairs, sums
 * conj(Zx) Zg per bin over pairs and blocks in a fixed order (no atomics: equal inputs give equal bits) and runs ONE inverse
 * transform.  Both launch on `stream`, read nothing back, and refuse like nws_reverb (NWS_ERR_BAD_ARG, NWS_ERR_WORKSPACE,
 * NWS_ERR_UNSUPPORTED beyond 65 535 utterance pairs) before the first launch.  Workspace: nws_reverb_grad_workspace_bytes
 * (host only; 0 for a bad plan or B < 1; want_ir = 0: what grad_x needs = nws_reverb_workspace_bytes). */
size_t nws_reverb_grad_workspace_bytes(const NwsReverbPlan* plan, int B, int want_ir);
int nws_reverb_grad_x(const NwsReverbPlan* plan, const void* tables, const void* spectrum, const float* g /* (B,N) */,
                      int B, int N, float* dx /* (B,N) */, void* workspace, size_t workspace_bytes, void* stream);
int nws_reverb_grad_ir(const NwsReverbPlan* plan, const void* tables, const float* x /* (B,N) */, const float* g /* (B,N) */,
                       int B, int N, int ir_len, float* dir /* (ir_len) */, void* workspace, size_t workspace_bytes,
                       void* stream);

/* streaming (LINEAR, non-wrapping) variant, one chunk of M samples: y = x + wet[0:M] + tail_in[0:M]; tail_out = shifted
 * tail_in + rest of wet.  plan->L >= M + tail_len (tail_len = len(ir)+1 = 32000); workspace (2*ceil(B/2)*L + B*L) floats. */
int nws_reverb_linear_chunk(const NwsReverbPlan* plan, const void* tables, const void* spectrum, const float* x, int B, int M,
                            const float* tail_in, float* tail_out, int tail_len, float* y, void* workspace,
                            size_t workspace_bytes, void* stream);

/*
 * ---- Stateful streaming (csrc/stream.hip): the reference's buffer benchmark (scripts/time_buffer_sizes.py:50-72)
 * restarts the GRU, the oscillator phase and the reverb with every buffer; here B parallel streams carry them across chunks.
 * The concatenated output equals the one-shot forward up to the reverb input for ANY chunking, and the learned reverb
 * (models/modules/shaping.py:161-173) is applied as a linear convolution of the stream.  All state lives in one caller-owned
 * device blob behind fixed pointers: a steady-state hop is eight launches that can be captured into a hipGraph.
 * `plan` (the L = 64 000 plan of nws_reverb_plan(64000, ir_len + 1)) is only needed for chunks beyond 2048 samples and for
 * nws_stream_reverb_tail; pass NULL to nws_stream_state_bytes when the stream never takes more than 16 frames at a time.
 */
size_t nws_stream_state_bytes(int B, int max_frames, int ir_len, const NwsReverbPlan* plan);
int nws_stream_reset(void* state, size_t state_bytes, void* stream);
int nws_stream_out_samples(int K, int first, int final);   /* 128 K (-64 for the first chunk, +64 for the final one) */
long long nws_stream_noise_start(int first, long long frames_seen);
int nws_stream_noise_draws(int K, int first, long long frames_seen);
int nws_stream_step(const NwsWeights* w, const float* fir_design, const NwsReverbPlan* plan, const void* reverb_tables,
                    const void* reverb_spectrum, void* state, size_t state_bytes, int B, int max_frames, const float* f0 /* (B,K) */,
                    const float* control /* (B,C,K) */, int C, int K, int first, int final, long long frames_seen,
                    long long nz_prev_start, float sample_rate, const float* phase_u, const float* rand_phase,
                    const float* noise_new, const float* noise_all, int noise_all_len, const float* ir, int ir_len,
                    float* out /* (B, M) */, float* pre_out /* optional (B, M) */, void* stream);
int nws_stream_reverb_tail(const NwsReverbPlan* plan, const void* reverb_tables, const void* reverb_spectrum, void* state,
                           size_t state_bytes, int B, int max_frames, int ir_len, float* tail_out /* (B, ir_len + 1) */,
                           void* workspace, size_t workspace_bytes, void* stream);

/*
 * Slot mode of the stateful stream: B independent voice slots that start and stop on their own, one hop of K <= 16 frames per
 * call, (B, 128 K) out every hop.  `events` is a (B) int32 array in DEVICE memory with this hop's word per slot, read by the
 * hop's launches (a captured hop stays valid whatever the events):
 *   NWS_SLOT_ACTIVE             the slot's voice covers this hop's frames (set together with START on the voice's first hop)
 *   NWS_SLOT_START              this hop's frames are the voice's first frames (its recurrence, phase and noise start here)
 *   NWS_SLOT_STOP               this hop's frames are the voice's last frames
 *   NWS_SLOT_RELEASE            (alone) the hop after the stop hop: the voice's last 64 samples come out
 *   0                           idle: inputs are not read into any output; the slot emits its dry signal 0 and its reverb tail
 * Voice v of slot b, starting at stream frame a with T frames, is the one-shot pre-reverb signal of its own (f0, control) with the
 * stream's phase draw and the noise samples [128 a, 128 (a + T) - 1) of the stream's noise, placed at output samples
 * [128 a + 64, 128 (a + T) + 64); out = dry + linear reverb of the slot's dry signal.  The first call (frames_seen == 0) is an
 * all-idle pre-roll whose output the caller drops.  NWS_ERR_UNSUPPORTED for K > 16.  State: nws_stream_slot_state_bytes.  Hops of
 * one or two frames take the four-launch form up to B = 512 slots, everything else the seven-launch form.
 */
/* byte offset of the stream's position counters (int64 [8]) in the state blob; counters[5] != 0: a frame-MLP workgroup of a
 * four-launch hop gave up waiting for its recurrence rows (that hop's rows are NaN) */
size_t nws_stream_counters_offset(int B, int max_frames, int ir_len);
/* state blob of a slot-mode stream (hops of at most max_frames <= 16 frames: no FFT reverb buffers) */
size_t nws_stream_slot_state_bytes(int B, int max_frames, int ir_len);
#define NWS_SLOT_START 1
#define NWS_SLOT_STOP 2
#define NWS_SLOT_RELEASE 4
#define NWS_SLOT_ACTIVE 8
int nws_stream_step_slots(const NwsWeights* w, const float* fir_design, void* state, size_t state_bytes, int B, int max_frames,
                          const float* f0 /* (B,K) */, const float* control /* (B,C,K) */, int C, int K, long long frames_seen,
                          long long nz_prev_start, float sample_rate, const float* phase_u, const float* rand_phase,
                          const float* noise_new, const float* noise_all, int noise_all_len, const float* ir, int ir_len,
                          const int* events /* (B) device */, float* out /* (B, 128 K) */, float* pre_out /* optional */,
                          void* stream);

/*
 * Stand-alone forms of the reference's sub-modules ("the seven module classes" are public interface).  Inside
 * nws_forward the same arithmetic is fused; these entry points serve callers that invoke a sub-module on its own
 * (model.osc(f0), model.newt(exciter, emb), model.h_generator(emb), model.noise_synth(H), ...).
 */
/* HarmonicOscillator.forward (models/modules/generators.py:58-66): f0_up (B, N) Hz at sample rate, N a multiple of 128;
 * carry from nws_phase_carry(NULL, f0_up, B, N/128, .); phase_u / rand_phase as in nws_exciter_newt; out (B, 101, N) */
int nws_oscillator(const float* f0_up, const double* carry, const float* phase_u, const float* rand_phase, int B, int N,
                   float sample_rate, float* out, void* stream);
/* NEWT.forward / FastNEWT.forward on a materialised exciter (models/modules/shaping.py:67-79): exciter (B, 64, N),
 * film (B, 256, T) = newt.mlp(control_embedding) channel-major as the reference's Conv1d stack returns it; out (B, N).
 * w: shaper_* or lut fields, newt_out_w / newt_out_b. */
int nws_newt_apply(const NwsWeights* w, const float* exciter, const float* film, int B, int T, float* out, void* stream);
/* The backward of nws_newt_apply with the exact shapers for grad_out = dL/d(out) (B, N): grad_film (B, 256, T),
 * grad_exciter (B, 64, N) unless NULL, and, when all eleven are given, the parameter gradients in the layout of their parameters:
 * shaping_fn.input_scale (64), net.0.weight / bias (512 each), net.2.weight (512, 8) / bias (512), net.4.weight / bias likewise,
 * net.6.weight (64, 8) / bias (64), mixer.0.weight (64) / bias (1).  Nothing is saved by the forward: it is recomputed per
 * sample from exciter and film with nws_newt_apply's arithmetic.  No atomics, sums over batch and time in a fixed order in
 * float64: equal inputs give equal bits, grad_out = 0 gives zeros.  Launches on `stream` (the recomputing kernel, the fold of the
 * upsampling's transpose, with parameters one reduction), reads nothing back and decides every refusal before the first launch:
 * NWS_ERR_BAD_ARG for a NULL required pointer (w's shaper_* and newt_out_* fields included), some but not all of the eleven
 * parameter gradients, a size < 1, or a workspace that is NULL or smaller than nws_newt_grad_workspace_bytes;
 * NWS_ERR_UNSUPPORTED for T > 65 535, B T > 2^28, or a w that carries a lookup table (FastNEWT has no backward).
 * nws_newt_grad_workspace_bytes: 0 for sizes that are refused. */
size_t nws_newt_grad_workspace_bytes(int B, int T, int want_params);
int nws_newt_grad(const NwsWeights* w, const float* exciter, const float* film, const float* grad_out, int B, int T,
                  float* grad_exciter /* may be NULL */, float* grad_film, float* grad_in_scale, float* grad_w0, float* grad_b0,
                  float* grad_w2, float* grad_b2, float* grad_w4, float* grad_b4, float* grad_w6, float* grad_b6,
                  float* grad_mix_w, float* grad_mix_b, void* workspace, size_t workspace_bytes, void* stream);
/* TimeDistributedMLP.forward (models/modules/dynamic.py:20-40), any sizes: x (B, in, T) -> y (B, out, T);
 * depth Conv1d(k=1) layers (HOST arrays of depth device pointers: w[i] (rows_i, cols_i), b[i]), LayerNorm over channels
 * (ln_g[i], ln_b[i], i < depth-1, biased variance, eps) + LeakyReLU(slope) after every layer but the last.
 * 1 <= depth <= 8 (depth 1 = a bare Conv1d(k=1), e.g. ControlModule.proj), max(in, hidden) <= ~600 (LDS). */
int nws_td_mlp(const float* x, int B, int in_size, int hidden, int out_size, int depth, int T, const float* const* w,
               const float* const* b, const float* const* ln_g, const float* const* ln_b, float ln_eps, float leaky_slope,
               float* y, void* stream);
/* The backward of nws_td_mlp for grad_y = dL/dy (B, out, T): grad_x (B, in, T) and, when grad_w and grad_b are
 * given, the gradient of every parameter: grad_w[i] like w[i], grad_b[i] like b[i] (depth entries each), grad_ln_g[i] and
 * grad_ln_b[i] (depth-1 entries each).  grad_w == grad_b == NULL: the data gradient alone, no workspace.  Nothing is saved by the
 * forward: the frame tile's forward is recomputed from x.  Exact fp32 products, sums over batch and time in a fixed order in
 * float64, no atomics: equal inputs give equal bits, grad_y = 0 gives zeros.  LeakyReLU' at v = 0 is `leaky_slope` (torch's).
 * Launches on `stream` (the recomputing kernel, then with parameters the dW contraction and two reductions), reads nothing back
 * and decides every refusal before the first launch: NWS_ERR_BAD_ARG for a NULL required pointer, a size < 1 or a workspace
 * smaller than nws_td_mlp_grad_workspace_bytes; NWS_ERR_UNSUPPORTED for depth outside 1 .. 8, B > 65 535, a layer width above
 * 256 or more than 160 KB of LDS ((max(in, hidden) + (depth-1) hidden) 132 bytes + 2 KB + (depth-1) 128).
 * nws_td_mlp_grad_workspace_bytes: 0 without want_params or for sizes that are refused. */
size_t nws_td_mlp_grad_workspace_bytes(int B, int in_size, int hidden, int out_size, int depth, int T, int want_params);
int nws_td_mlp_grad(const float* x, const float* grad_y, int B, int in_size, int hidden, int out_size, int depth, int T,
                    const float* const* w, const float* const* b, const float* const* ln_g, const float* const* ln_b,
                    float ln_eps, float leaky_slope, float* grad_x /* (B,in,T) */, float* const* grad_w, float* const* grad_b,
                    float* const* grad_ln_g, float* const* grad_ln_b, void* workspace, size_t workspace_bytes, void* stream);
/* TimeDistributedLayerNorm.forward (dynamic.py:11-17): LayerNorm over the channel axis of (B, C, T) */
int nws_td_layer_norm(const float* x, const float* gain, const float* bias, int B, int C, int T, float eps, float* y,
                      void* stream);
/* FiLM.forward (dynamic.py:6-8): y = gamma * x + beta on n equally laid out elements */
int nws_film(const float* x, const float* gamma, const float* beta, int64_t n, float* y, void* stream);
/* zero-phase FIR design of FIRNoiseSynth.forward (generators.py:22-28): H (B, 129, T) -> fir (B, T, 128) upper half-taps
 * (window * roll(irfft(H), 128))[128:256]; feed nws_fir_noise with them */
int nws_fir_from_h(const float* H, const float* fir_design /* (256,132) */, int B, int T, float* fir_out, void* stream);

/* ---- FastNEWT table (models/modules/shaping.py:107-119): table[s][i] = shaper_s(linspace(min,max,size)[i]) ---- */
int nws_shaper_table(const NwsWeights* w, int table_size, float table_min, float table_max, float* table_out, void* stream);

/* mixer_b (64) as K slot 0 and mixer_w (64,101) as K slots 1..101 (slots 102..111 zero) -> W_hi | W_lo fp16 fragments
   (7 K-steps x 2 M-tiles x 2 halves x 32 lanes x 8 halfs, twice) */
#define NWS_MIXER_FRAGS_BYTES 28672
int nws_mixer_frags(const float* mixer_w, const float* mixer_b, void* frags_out, void* stream);
/* X[s] = (sum_k |mixer_w[s][k]| + |mixer_b[s]|) * (1 + 2^-10): the worst-case magnitude of the exciter of shaper s
 * (NwsWeights.exciter_bound) */
int nws_exciter_bound(const float* mixer_w, const float* mixer_b, float* bound_out /* device, 64 floats */, void* stream);
/* Exact-mode companion of nws_lut_pairs: the TrainableNonlinearity weights (models/modules/shaping.py:15-37) of `w`
 * (shaper_* fields) as the (64, NWS_SHAPER_TURNS_ROW) fp32 table the fused kernel's shaper bank reads. */
#define NWS_SHAPER_TURNS_ROW 176
int nws_shaper_turns(const NwsWeights* w, float* table_out /* device, 64 * NWS_SHAPER_TURNS_ROW floats */, void* stream);

/* derived gather-friendly form of a FastNEWT table: pairs[s][i] = {table[s][i], fl(table[s][min(i+1,size-1)] - table[s][i])} */
int nws_lut_pairs(const float* table /* (64, size) */, int table_size, float* pairs_out /* (64, size, 2) */, void* stream);

/* exact shapers on an arbitrary (B,64,N) tensor (TrainableNonlinearity.forward, shaping.py:36-37) / LUT lookup (:136-151) */
int nws_shaper_apply(const NwsWeights* w, const float* x, int64_t B, int64_t N, float* y, void* stream);

/*
 * Whole forward (models/neural_waveshaping.py:74-90) as one enqueue: phase carries -> GRU -> frame MLPs ->
 * fused exciter+NEWT -> FIR noise (+sum) -> reverb.  All scratch lives in `workspace`
 * (nws_forward_workspace_bytes).  phase_u (101) and noise (N-1) are the two RNG draws of forward().
 */
typedef struct NwsForwardAux {
  const float* fir_design;       /* (256,132) */
  const NwsReverbPlan* plan;     /* host */
  const void* reverb_tables;
  const void* reverb_spectrum;
} NwsForwardAux;

size_t nws_forward_workspace_bytes(const NwsReverbPlan* plan, int B, int T);
int nws_forward(const NwsWeights* w, const NwsForwardAux* aux, const float* f0 /* (B,T) */, const float* control /* (B,C,T) */,
                int B, int C, int T, float sample_rate, const float* phase_u, const float* rand_phase,
                const float* noise, float* out /* (B,N) */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * The same forward in two halves for throughput pipelines: `control` = phase carries + GRU (writes the head of the
 * workspace, nws_forward_control_bytes), `audio` = frame MLPs .. reverb (reads the head, uses the rest).  Same workspace
 * layout as nws_forward; one workspace per batch in flight.  The control half of batch i+1 may run on another stream while
 * the audio half of batch i runs (order them with events).  batched_gru != 0 selects nws_control_gru_batched.
 */
size_t nws_forward_control_bytes(int B, int T);
int nws_forward_control(const NwsWeights* w, const float* f0, const float* control, int B, int C, int T, int batched_gru,
                        void* workspace, size_t workspace_bytes, void* stream);
int nws_forward_audio(const NwsWeights* w, const NwsForwardAux* aux, const float* f0, int B, int T, float sample_rate,
                      const float* phase_u, const float* rand_phase, const float* noise, float* out, void* workspace,
                      size_t workspace_bytes, void* stream);

/* nws_forward_audio with two optional hipEvent_t hooks around the oscillator + waveshaper kernel (NULL = none): the stream
 * waits for `wait_before_exciter` right before that kernel and records `record_after_exciter` right after it.  A pipeline
 * that alternates batches over several streams chains them so that the VALU-saturated kernels of neighbouring batches run
 * one after the other while their matrix / memory kernels (frame MLPs, noise, reverb) overlap it (pipeline.py). */
int nws_forward_audio_ev(const NwsWeights* w, const NwsForwardAux* aux, const float* f0, int B, int T, float sample_rate,
                         const float* phase_u, const float* rand_phase, const float* noise, float* out, void* workspace,
                         size_t workspace_bytes, void* stream, void* wait_before_exciter, void* record_after_exciter);

/* The audio half in two parts for multi-GPU callers that push sub-batches of finished waveforms to their peers while the
 * reverb of the next sub-batch still runs: nws_forward_audio_pre = everything up to the reverb input of the
 * whole batch (kept in the workspace), nws_forward_reverb_rows = the reverb of rows [row0, row0 + nrows) (row0 even) into the
 * same rows of out (B, N).  pre + reverb_rows over all rows == nws_forward_audio, bit for bit. */
int nws_forward_audio_pre(const NwsWeights* w, const NwsForwardAux* aux, const float* f0, int B, int T, float sample_rate,
                          const float* phase_u, const float* rand_phase, const float* noise, void* workspace,
                          size_t workspace_bytes, void* stream);
int nws_forward_reverb_rows(const NwsForwardAux* aux, int B, int T, int row0, int nrows, float* out, void* workspace,
                            size_t workspace_bytes, void* stream);
/* The two above in ONE call for a fixed list of row blocks: audio_pre, then for q = 0 .. nblocks - 1 the reverb of rows
 * [row0[q], row0[q] + nrows[q]) followed by hipEventRecord(events[q], stream) when events and events[q] are non-NULL - a multi-GPU
 * caller's helper thread waits on those events (host side) and pushes each sub-batch as it completes (bench.py --gather-chunks:
 * one op call per step instead of 1 + nblocks, and no event record through the host language per block).  The blocks must tile
 * [0, B) in order, even sizes except the last.  Same bits as nws_forward_audio. */
int nws_forward_audio_blocks(const NwsWeights* w, const NwsForwardAux* aux, const float* f0, int B, int T, float sample_rate,
                             const float* phase_u, const float* rand_phase, const float* noise, float* out, void* workspace,
                             size_t workspace_bytes, void* stream, const int32_t* row0, const int32_t* nrows,
                             void* const* events /* hipEvent_t[nblocks] or NULL */, int nblocks);

/*
 * Perceptual-loudness feature, the step before the synthesis path:
 * neural_waveshaping_synthesis/data/utils/loudness_extraction.py:10-67 (extract_perceptual_loudness) with the shipped
 * configuration gin/data/urmp_4second_crepe.gin:11-14 = mean over bins of
 * amplitude_to_db(|stft(audio, n_fft, hop, hann, center/reflect)|, ref=max, amin, top_db), optionally (L + 80) / 80.
 * audio (B, N) fp32 -> out (B, 1 + N / hop).  `dft` is the constant windowed-DFT operand for n_fft (build once).
 * n_fft: power of two in [64, 2048]; 1 <= hop <= n_fft; N > n_fft / 2.  The reference's optional interpolate_fn is a
 * host callable on the returned frames and stays on the Python side.
 */
size_t nws_loudness_dft_bytes(int n_fft);
int nws_loudness_dft_matrix(int n_fft, float* dft_out, void* stream);
int nws_loudness_frames(int N, int hop);
size_t nws_loudness_workspace_bytes(int B, int N, int n_fft, int hop);
int nws_loudness(const float* audio, int B, int N, int n_fft, int hop, const float* dft, float amin, float top_db,
                 int normalise, float* out, void* workspace, size_t workspace_bytes, void* stream);
/* The clip maximum nws_loudness normalises by, as power_out (B) floats on the device: the power pass alone (workspace and
 * refusals as nws_loudness).  A calibration value for a loudness stream's fixed reference. */
int nws_loudness_peak_power(const float* audio, int B, int N, int n_fft, int hop, const float* dft, float* power_out,
                            void* workspace, size_t workspace_bytes, void* stream);

/*
 * Loudness stream: the feature above from chunked audio with a bounded delay and a causal reference level (DESIGN.md 3.25 is the
 * definition; W = n_fft / 2).  Frames and emission are the pYIN stream's below: after n samples F(n) = 0 for n <= W, else
 * 1 + (n - W) / hop frames are computed and E(n) = max(0, F(n) - lag) have left, 0 <= lag <= 255; a step with `final` (n may be
 * 0) ends the stream at N = n_seen + n, computes the frames F(N) .. T - 1, T = 1 + N / hop, with the right edge reflected about
 * N and releases the rest.  P(t, k), the power of bin k of frame t, has the bits nws_loudness computes for that frame of the
 * whole signal, whatever the chunking; p(t) = max_k P(t, k).
 * Reference level: a row carries one float M.  nws_loudness_stream_reset sets it to initial_power[b] >= 0 (device memory) and
 * fixes `track`: with it M(t) = max(M(t - 1), p(t)), without it M(t) = initial_power.  A frame e that leaves in a step without
 * `final` is measured against ref(e) = M(e + lag), one the flush releases against M(T - 1):
 *   db(k) = 10 log10(max(amin^2, P(e, k))) - 10 log10(max(amin^2, ref(e))),  loudness = mean_k max(db(k), -top_db) [, (l + 80) / 80]
 * term for term nws_loudness's dB pass, the sum over k in order.  Without `track` a signal louder than its reference gives
 * values above 0 dB (above 1 normalised); they are not clipped.  track with initial_power 0 is the running reference; no track
 * with nws_loudness_peak_power of the clip is nws_loudness of the clip, bit for bit, at any lag and chunking; so is the
 * running reference at lag >= T - 1.  The maximum does not decay here: one click pins the reference until the next reset (the _release
 * entry points below add a decay).
 * Row b's new frames go to columns 0 .. of row b of the (B, out_stride) outputs loudness_out and ref_out (the reference power
 * each frame was measured against); the rest is untouched.  Latency: W + lag hop samples.
 * State blob (nws_loudness_stream_state_bytes; device memory, 8-byte aligned), B rows of
 *   int64 n_seen, frames computed, frames emitted, finished | float M, int32 track | float [n_fft] sample history (the pYIN
 *   stream's rule) | float [512] ring of M(t) at t % 512 | float [n_fft / 2 + 1][512] ring of P(t, k) at k 512 + t % 512;
 *   each part padded to 8 bytes.
 * The caller mirrors n_seen and passes it to every step; all sizes and refusals are decided on the host before the first launch,
 * nothing is read back.  The kernels compare n_seen with the blob's counters and leave state and outputs untouched when they
 * differ (a stream never reset, or one that has had `final`).  Two launches and one memset a pass (a final step with samples is
 * two passes), one launch when the pass computes no frame.
 * Limits (NWS_ERR_UNSUPPORTED / 0 / -1): n_fft and hop nws_loudness refuses or with more than 256 hops in W, B > 65 535,
 * n > nws_loudness_stream_max_chunk = 256 hop, more than 2^21 hop samples in all.  NULL state, dft, initial_power, workspace or
 * output, NULL x with n > 0, B < 1, n < 0, n_seen < 0, n = 0 without `final`, `final` with N <= W, out_stride below the step's
 * emission, a state below nws_loudness_stream_state_bytes, a workspace below nws_loudness_stream_workspace_bytes, lag outside
 * 0 .. 255, amin <= 0, top_db < 0: NWS_ERR_BAD_ARG.  Every refusal leaves state and outputs untouched.
 *   nws_loudness_stream_frames / _emitted   host arithmetic: F(n_seen) / E(n_seen), with `final` T (-1: refused).
 *   nws_loudness_stream_workspace_bytes     scratch of a step of n samples, whatever the stream has seen.
 */
size_t nws_loudness_stream_state_bytes(int B, int n_fft, int hop);
int nws_loudness_stream_max_chunk(int n_fft, int hop);
size_t nws_loudness_stream_workspace_bytes(int B, int n, int n_fft, int hop, int final);
int64_t nws_loudness_stream_frames(int64_t n_seen, int n_fft, int hop, int final);
int64_t nws_loudness_stream_emitted(int64_t n_seen, int n_fft, int hop, int lag, int final);
int nws_loudness_stream_reset(void* state, size_t bytes, int B, int n_fft, int hop, const float* initial_power, int track,
                              void* stream);
int nws_loudness_stream_step(void* state, size_t bytes, const float* x, int B, int n, int64_t n_seen, int n_fft, int hop, int lag,
                             const float* dft, float amin, float top_db, int normalise, int final, float* loudness_out,
                             float* ref_out, int out_stride, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Loudness stream with a release: the tracked level falls by a constant factor per frame, so a click no longer
 * pins the reference.  release_factor rho = float(10^(-release_db_per_s hop / (10 sample_rate))), 0 < rho <= 1, computed by the
 * caller in double and rounded once; F = floor_power[b] >= 0.  In fp32, one product, nothing fused:
 *   d = rho M(t - 1);  if d < 2^-126: d = 0;  M(t) = max(p(t), F, d);  M(-1) = F
 * A decaying M is not monotone, so a frame e that leaves in a step without `final` is measured against
 * ref(e) = max_{t = e .. e + lag} M(t), one the flush releases against max_{t = e .. T - 1} M(t); ref(e) >= p(e) always.  At
 * rho = 1 this is the stream above, bit for bit (nothing is flushed there).  The bits depend on the signal, lag and rho alone, never
 * on the chunking.
 *   nws_loudness_stream_release_state_bytes  the blob of a releasing stream: the B rows above, then float F[B] padded to 8 bytes.
 *   nws_loudness_stream_reset_release        a tracking stream at M = F with the floors stored; its rows carry track = 3.
 *   nws_loudness_stream_step_release         nws_loudness_stream_step with release_factor; `track` is the caller's mirror of how the
 *     stream was reset.  At release_factor 1 it is nws_loudness_stream_step on either kind of blob.  Below 1 the blob must come from
 *     nws_loudness_stream_reset_release (the kernels compare the rows' track word and leave everything untouched otherwise).
 * Further refusals (NWS_ERR_BAD_ARG, before any launch): release_factor NaN or outside (0, 1]; release_factor < 1 without track;
 * release_factor < 1 on a blob below nws_loudness_stream_release_state_bytes.
 */
size_t nws_loudness_stream_release_state_bytes(int B, int n_fft, int hop);
int nws_loudness_stream_reset_release(void* state, size_t bytes, int B, int n_fft, int hop, const float* floor_power, void* stream);
int nws_loudness_stream_step_release(void* state, size_t bytes, const float* x, int B, int n, int64_t n_seen, int n_fft, int hop,
                                     int lag, float release_factor, int track, const float* dft, float amin, float top_db,
                                     int normalise, int final, float* loudness_out, float* ref_out, int out_stride, void* workspace,
                                     size_t workspace_bytes, void* stream);

/*
 * The loudness stream's feature of a whole clip in one call: audio (B, N) -> loudness_out, ref_out, peak_out (B, 1 + N / hop) each,
 * the concatenated outputs of a stream over the clip (any chunking, then the flush), bit for bit, and p(t).  Frames
 * e < F(N) - lag take the window e .. e + lag, the rest the window e .. T - 1.  track: the running (releasing) reference from
 * floor_power (device memory, B floats; NULL: 0); no track: floor_power is the fixed reference.
 * Refusals: nws_loudness's, lag outside 0 .. 255, release_factor as above, NULL floor_power without track (NWS_ERR_BAD_ARG); sizes
 * the stream refuses or a clip beyond 2^21 hops (NWS_ERR_UNSUPPORTED); a workspace below nws_loudness_causal_workspace_bytes
 * (NWS_ERR_WORKSPACE).
 */
size_t nws_loudness_causal_workspace_bytes(int B, int N, int n_fft, int hop);
int nws_loudness_causal(const float* audio, int B, int N, int n_fft, int hop, const float* dft, int lag, float release_factor,
                        const float* floor_power, int track, float amin, float top_db, int normalise, float* loudness_out,
                        float* ref_out, float* peak_out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * pYIN F0 extractor, the other analysis feature in front of the synthesis path:
 * neural_waveshaping_synthesis/data/utils/f0_extraction.py:61-92 (extract_f0_with_pyin -> librosa.pyin) with librosa's own
 * constants (100 thresholds, beta(2, 18) prior, Boltzmann parameter 2, resolution 0.1, max_transition_rate 35.92, switch_prob
 * 0.01, no_trough_prob 0.01, centre / reflect padding).  DESIGN.md 3.9 is the definition; parity with librosa is unpinned.
 * A configuration is (sample_rate, fmin, fmax, frame_length, hop); nws_pyin_dims gives its derived sizes
 * dims[8] = {min_period, max_period, lags, n_bins_per_semitone, n_pitch_bins, transition window, W = frame_length / 2,
 * hop blocks per frame in the shared-sum form of the difference kernel (0: plain form)}.
 * Limits (NWS_ERR_UNSUPPORTED, 0 bytes): lags <= 512 (frame_length <= 1024), n_pitch_bins <= 1024 (2048 states), transition
 * window <= 127, hop <= frame_length, B <= 65535, 31 hop + frame_length + 32 (max_period + 1) floats <= 160 KB of LDS.
 * N > frame_length / 2 (reflect padding), T = 1 + N / hop frames.
 *   nws_pyin_table   fills a HOST buffer of nws_pyin_table_bytes with the fp64 constants of a configuration (threshold prior,
 *                    Boltzmann terms, log transition window, log row sums, F0 of every bin); copy it to the device once.
 *   nws_pyin_cmnd    audio (B, N) -> yin (B, T, lags) fp32: squared-difference YIN + cumulative-mean normalisation.
 *   nws_pyin_observe yin -> sparse observations per frame: cand_bin / cand_prob (B, T, lags) in lag order (entries beyond
 *                    count are -1 / 0), count (B, T), voiced_prob (B, T) fp64.
 *   nws_pyin_viterbi observations -> states (B, T) int32 in [0, 2 n_pitch_bins) (voiced bins, then unvoiced bins) and
 *                    f0 (B, T) = fmin 2^(bin / (12 n_bps)); fill_unvoiced != 0 writes fill_value on unvoiced frames.
 *                    Workspace: the first part of nws_pyin_workspace_bytes (one byte per state and frame + one word per frame).
 *   nws_pyin         the three stages on one stream.
 */
int nws_pyin_frames(int N, int hop);
int nws_pyin_dims(double sample_rate, double fmin, double fmax, int frame_length, int hop, int32_t* dims);
size_t nws_pyin_table_bytes(double sample_rate, double fmin, double fmax, int frame_length, int hop);
int nws_pyin_table(double sample_rate, double fmin, double fmax, int frame_length, int hop, double* table_host);
size_t nws_pyin_workspace_bytes(int B, int N, double sample_rate, double fmin, double fmax, int frame_length, int hop);
int nws_pyin_cmnd(const float* audio, int B, int N, double sample_rate, double fmin, double fmax, int frame_length, int hop,
                  float* yin, void* stream);
int nws_pyin_observe(const float* yin, int B, int T, double sample_rate, double fmin, double fmax, int frame_length, int hop,
                     const double* table, int* cand_bin, double* cand_prob, int* count, double* voiced_prob, void* stream);
int nws_pyin_viterbi(const int* cand_bin, const double* cand_prob, const int* count, const double* voiced_prob, int B, int T,
                     double sample_rate, double fmin, double fmax, int frame_length, int hop, const double* table,
                     int fill_unvoiced, float fill_value, int* states, float* f0, void* workspace, size_t workspace_bytes,
                     void* stream);
int nws_pyin(const float* audio, int B, int N, double sample_rate, double fmin, double fmax, int frame_length, int hop,
             const double* table, int fill_unvoiced, float fill_value, float* f0, double* voiced_prob, int* states,
             void* workspace, size_t workspace_bytes, void* stream);

/*
 * Fixed-lag pYIN stream: F0 from chunked audio with a bounded delay (DESIGN.md 3.24 is the definition; symbols as above,
 * W = frame_length / 2).  It is nws_pyin's forward pass - the same CMND, observations, value vectors V and backpointers, bit for
 * bit, whatever the chunking - read out by another backtrace.  A stream is made for (B, configuration); all rows advance in
 * lock-step.  After n samples
 *   F(n) = 0 for n <= W, else 1 + (n - W) / hop     frames are computed (frame t as soon as all its samples exist), and
 *   E(n) = max(0, F(n) - lag)                       frames have left: frame e is the state at e of the backtrace that starts at
 *                                                   argmax V_{e + lag} (lowest index on ties), 0 <= lag <= 255.
 * A step with `final` (n may be 0) ends the stream at N = n_seen + n; it is the step without `final` followed by a flush: the
 * frames F(N) .. T - 1, T = 1 + N / hop, are computed with the right edge reflected about N, and every frame not yet emitted
 * leaves from argmax V_{T - 1}.  With lag >= T - 1 nothing leaves before `final` and the output is nws_pyin's, bit for bit.
 * Per emitted frame: states (int32, [voiced bins | unvoiced bins]), f0 (fill_unvoiced as in nws_pyin_viterbi) and voiced_prob,
 * all three delayed alike; row b's new frames go to columns 0 .. of row b of the (B, out_stride) outputs, the rest is untouched.
 * Latency: W + lag hop samples.
 * State blob (nws_pyin_stream_state_bytes; device memory, 8-byte aligned), B rows of
 *   int64 n_seen, frames computed, frames emitted, finished | double max V_last, int64 argmax V_last |
 *   double [2 n_pitch_bins] V_last - log rowsum, as the offline kernel keeps V between steps | double [512] voiced_prob ring |
 *   int32 [512] jump-word ring (argmax V_{t-1} at frame t) | float [frame_length] sample history: what the frames still to come and a
 *   flush need, fewer than frame_length samples | uint8 [512][2 n_pitch_bins] backpointer ring, frame t at slot t % 512;
 *   each part padded to 8 bytes.
 * The caller mirrors n_seen and passes it to every step, so that all sizes and refusals are decided on the host before the first
 * launch; nothing is read back.  The kernels compare it with the blob's counters and leave state and outputs untouched when they
 * differ - a stream that was never reset, or one that has had `final`: it accepts nothing until the next reset.
 * V is never renormalised (that would change bits): a frame lowers max V by less than 1500, so up to 2^21 frames one ulp of V
 * stays below 1e-6; a stream is refused beyond 2^21 hop samples (4.6 h at hop 128 / 16 kHz).
 * Limits (NWS_ERR_UNSUPPORTED / 0 / -1): a configuration nws_pyin_dims refuses or with more than 256 hops in W, B > 65 535,
 * n > nws_pyin_stream_max_chunk = 256 hop, more than 2^21 hop samples in all.  NULL state, table, workspace or output, NULL x
 * with n > 0, B < 1, n < 0, n_seen < 0, n = 0 without `final`, `final` with N <= W, out_stride below the step's emission, a state
 * below nws_pyin_stream_state_bytes, a workspace below nws_pyin_stream_workspace_bytes, lag outside 0 .. 255: NWS_ERR_BAD_ARG.
 * Every refusal leaves state and outputs untouched; everything runs on `stream`, four launches a pass (a final step with samples
 * is two passes), one when the pass computes no frame.
 *   nws_pyin_stream_frames           host arithmetic: F(n_seen), with `final` T (-1: unsupported, n_seen < 0, `final` with N <= W).
 *   nws_pyin_stream_emitted          host arithmetic: E(n_seen), with `final` T; a step emits the difference (-1 as above).
 *   nws_pyin_stream_workspace_bytes  scratch of a step of n samples, whatever the stream has seen.
 *   nws_pyin_stream_reset            zeroes the blob.
 */
size_t nws_pyin_stream_state_bytes(int B, double sample_rate, double fmin, double fmax, int frame_length, int hop);
int nws_pyin_stream_max_chunk(double sample_rate, double fmin, double fmax, int frame_length, int hop);
size_t nws_pyin_stream_workspace_bytes(int B, int n, double sample_rate, double fmin, double fmax, int frame_length, int hop,
                                       int final);
int64_t nws_pyin_stream_frames(int64_t n_seen, double sample_rate, double fmin, double fmax, int frame_length, int hop, int final);
int64_t nws_pyin_stream_emitted(int64_t n_seen, double sample_rate, double fmin, double fmax, int frame_length, int hop, int lag,
                                int final);
int nws_pyin_stream_reset(void* state, size_t bytes, int B, double sample_rate, double fmin, double fmax, int frame_length, int hop,
                          void* stream);
int nws_pyin_stream_step(void* state, size_t bytes, const float* x, int B, int n, int64_t n_seen, double sample_rate, double fmin,
                         double fmax, int frame_length, int hop, int lag, const double* table_dev, int final, int fill_unvoiced,
                         float fill_value, float* f0, double* voiced_prob, int* states, int out_stride, void* workspace,
                         size_t workspace_bytes, void* stream);

/*
 * Band-limited sample-rate converter, the step in front of the two analysis features:
 * neural_waveshaping_synthesis/data/utils/preprocess_audio.py:65-66 (resample_audio -> resampy.resample, filter kaiser_best).
 * DESIGN.md 3.10 is the definition (resampy 0.2.2's interpolation with n_out = (N L) / M in integers and the exact rational
 * position t M / L of output t); parity with resampy is unpinned.  Rates are integers; L = sr_out / gcd, M = sr_in / gcd.
 * nws_resample_dims gives dims[6] = {L, M, taps, left, right, window step}: an output is `taps` = left + right weights
 * against x[n - left + 1 .. n + right], zero outside the row.
 * Limits (NWS_ERR_UNSUPPORTED, 0 bytes / 0 samples): rates below 1, a bank above 64 MB (every pair of the standard rates
 * 8000 .. 192000 Hz stays below 1.3 MB), more than 2^31 - 1 outputs a row.  N < 1, B < 1, n_out < 1, NULL: NWS_ERR_BAD_ARG.
 *   nws_resample_length  n_out = (N L) / M of a row of N samples, in 64-bit arithmetic (0: unsupported rates or N < 1).
 *   nws_resample_bank    fills a HOST buffer of nws_resample_bank_bytes with the L rows of `taps` weights, row-major by the
 *                        phase numerator r = (t M) mod L, computed in fp64 and rounded once to fp32; column c weighs
 *                        x[n + c - (left - 1)], unused columns are 0.  Copy it to the device once.
 *   nws_resample         x (B, N) -> y (B, n_out) with the device copy of that bank.  A row's result does not depend on B.
 */
int nws_resample_dims(int sr_in, int sr_out, int32_t* dims);
int64_t nws_resample_length(int64_t N, int sr_in, int sr_out);
size_t nws_resample_bank_bytes(int sr_in, int sr_out);
int nws_resample_bank(int sr_in, int sr_out, float* bank_host);
int nws_resample(const float* x, int B, int N, int sr_in, int sr_out, const float* bank_dev, float* y, void* stream);

/*
 * Streaming sample-rate converter: nws_resample on chunks with the state carried between calls, so that a stream at one rate
 * can feed, or be fed by, a device at another (DESIGN.md 3.23 is the definition; symbols as above).  A stream is made for
 * (B, sr_in, sr_out) and keeps per row two 64-bit counters: n_seen (input samples consumed) and t_next (outputs emitted).
 * Output t = row (t M) mod L of the bank against x[n - left + 1 .. n + right], n = (t M) / L, x = all samples pushed so far and
 * zero before sample 0.  It is emitted once x[n + right] has been pushed: after n_seen samples
 *   E(n_seen) = 0 for n_seen <= right, else ceil((n_seen - right) L / M)
 * outputs have left, and a step of n samples emits outputs [t_next, E(n_seen + n)) - possibly none.  A step with `final` (n may be
 * 0) treats x as zero beyond its end and emits up to the offline length (n_seen L) / M; the stream is then finished until the next
 * reset.  Latency: `right` input samples.  Any chunking of the same input gives the same output bits (the order in which an
 * output's taps are summed depends on the rates alone); the bits are not those of nws_resample, which sums in another order.
 * State blob (nws_resample_stream_state_bytes, a multiple of 16; device memory, 8-byte aligned):
 *   B x {int64 n_seen, int64 t_next} | B x (taps - 1) floats: the last taps - 1 input samples of each row | padding to 16 bytes.
 * Limits: B <= 65 535; a step's n <= nws_resample_stream_max_chunk (taps - 1 + n + right floats fit 64 KB of LDS:
 * 16 195 samples at 16 -> 48 kHz, 11 707 at 192 -> 8 kHz with its 3 119 taps); rates nws_resample_dims refuses, taps - 1 + right >= 16 384, or (16 386 L + M) >= 2^31:
 * NWS_ERR_UNSUPPORTED / 0 bytes / 0 samples.  NULL state, bank or y, NULL x with n > 0, B < 1, n < 0, n = 0 without `final`,
 * y_stride below nws_resample_stream_max_out, a state smaller than nws_resample_stream_state_bytes: NWS_ERR_BAD_ARG.  Every
 * refusal is decided before the launch; nothing is read back; everything runs on `stream`.
 *   nws_resample_stream_reset    zeroes the blob: n_seen = t_next = 0, a history of zeros.
 *   nws_resample_stream_emitted  host arithmetic: E(n_seen), with `final` the offline length (n_seen L) / M; -1: unsupported rates,
 *                                n_seen < 0 or beyond 64-bit arithmetic.
 *   nws_resample_stream_max_out  host arithmetic: the most outputs one step of n samples can emit whatever the stream has seen:
 *                                ceil(n L / M), with `final` ((n + right) L) / M; -1: unsupported rates, n < 0.
 *   nws_resample_stream_step     one launch, one workgroup per row: x (B, n) -> row b of y (B, y_stride) receives its outputs from
 *                                column 0, the rest is left untouched; `bank_dev` is the device copy of nws_resample_bank.  The
 *                                caller mirrors the counters with nws_resample_stream_emitted to know how many columns are new.
 */
size_t nws_resample_stream_state_bytes(int B, int sr_in, int sr_out);
int nws_resample_stream_max_chunk(int sr_in, int sr_out);
int nws_resample_stream_reset(void* state, size_t bytes, int B, int sr_in, int sr_out, void* stream);
int64_t nws_resample_stream_emitted(int64_t n_seen, int sr_in, int sr_out, int final);
int nws_resample_stream_max_out(int n, int sr_in, int sr_out, int final);
int nws_resample_stream_step(void* state, size_t bytes, const float* x, int B, int n, int sr_in, int sr_out, const float* bank_dev,
                             int final, float* y, int y_stride, void* stream);

/*
 * MFCC feature, the remaining analysis feature of the reference's control files:
 * neural_waveshaping_synthesis/data/utils/mfcc_extraction.py:7-13 (extract_mfcc -> librosa.feature.mfcc with librosa 0.8.0's
 * defaults) = power STFT (the loudness feature's: periodic hann, centre / reflect padding, T = 1 + N / hop frames), Slaney mel
 * filter bank (fmin 0, fmax sample_rate / 2, Slaney norm), power_to_db (ref 1, amin 1e-10, top_db 80 against the maximum of the
 * whole utterance), orthonormal DCT-II over the mel axis, first n_mfcc rows.  DESIGN.md 3.11 is the definition; parity with
 * librosa is unpinned.  audio (B, N) fp32 -> out (B, n_mfcc, T).  An empty filter (low sample_rate, many bands) is amin.
 * A configuration is (sample_rate, n_fft, n_mfcc, n_mels); nws_mfcc_dims gives dims[8] = {bins, n_mels, n_mfcc, n_mfcc
 * rounded up to 16 (jpad), non-zero filter weights (nnz), word offset of the weights, word offset of the DCT rows, words}.
 * Limits (NWS_ERR_UNSUPPORTED, 0 bytes): n_fft and hop as nws_loudness, 1 <= n_mfcc <= n_mels <= 1024, sample_rate > 0,
 * B <= 65535.  NULL, B < 1, N <= n_fft / 2: NWS_ERR_BAD_ARG, nothing launched.
 *   nws_mfcc_table  fills a HOST buffer of nws_mfcc_table_bytes, built in fp64 and rounded once to fp32; 4-byte words:
 *                   n_mels int32 triplets (first bin, count, offset into the weights) | nnz fp32 weights, span after span |
 *                   DCT entries (n_mels, jpad) fp32, column j scaled by s_j, zero from n_mfcc on.  Copy it to the device once.
 *   nws_mfcc        the three passes on one stream; `dft` is nws_loudness_dft_matrix of n_fft, `table` the device copy of the
 *                   table.  Workspace: nws_mfcc_workspace_bytes.  A row's result does not depend on B.
 */
int nws_mfcc_dims(double sample_rate, int n_fft, int n_mfcc, int n_mels, int32_t* dims);
size_t nws_mfcc_table_bytes(double sample_rate, int n_fft, int n_mfcc, int n_mels);
int nws_mfcc_table(double sample_rate, int n_fft, int n_mfcc, int n_mels, float* table_host);
size_t nws_mfcc_workspace_bytes(int B, int N, int n_fft, int hop, int n_mels);
int nws_mfcc(const float* audio, int B, int N, double sample_rate, int n_fft, int hop, int n_mfcc, int n_mels, const float* dft,
             const float* table, float* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Multi-resolution STFT loss (csrc/stft_loss.hip): what the reference logs as val/loss and test/loss,
 * auraloss.freq.MultiResolutionSTFTLoss()(recon, audio) of auraloss 0.2.1 (models/neural_waveshaping.py:93, 104-112, 136-165).
 * DESIGN.md 3.12 is the definition; parity with auraloss is unpinned.  x (the reconstruction) and y (the target): (B, N) fp32.
 * Resolution r = (n_ffts[r], hops[r], win_lengths[r]), R <= NWS_STFT_LOSS_MAX_RES of them:
 *   STFT      torch.stft: periodic hann of win_length centred in n_fft ((n_fft - win_length) / 2 zeros on the left), centre /
 *             reflect padding, 1 + N / hop frames, n_fft / 2 + 1 bins
 *   mag       sqrt(max(re^2 + im^2, eps))
 *   sc_r      ||y_mag - x_mag||_F / ||y_mag||_F,  log_r = mean |ln x_mag - ln y_mag|,  lin_r = mean |x_mag - y_mag|
 *   loss      (sum_r w_sc sc_r + w_log_mag log_r + w_lin_mag lin_r) / R
 * out: 1 + 3 R floats on the device: the loss, then (sc_r, log_r, lin_r) per resolution.  Forward only.
 *   nws_stft_loss_dft_matrix  the constant operand of a resolution (nws_stft_loss_dft_bytes), built on the device once
 *   nws_stft_loss             one fused kernel per resolution (no spectrogram reaches memory: one record of four fp64 sums per
 *                             workgroup into the workspace) + a one-workgroup finalise kernel.  No atomics: equal inputs give
 *                             equal bits.  Enqueue only.  Workspace: nws_stft_loss_workspace_bytes.
 * NWS_ERR_BAD_ARG: NULL, B < 1, R outside [1, 8], hop < 1, N <= n_fft / 2 (reflect padding), win_length outside [1, n_fft],
 * eps <= 0.  NWS_ERR_UNSUPPORTED (0 bytes): n_fft not a power of two in [64, 2048]; the two signal tiles of a workgroup,
 * 2 x (31 hop + n_fft) samples (+ skew words), over 160 KB of LDS (n_fft 2048: hop <= 589); B > 65535.  All of it is decided
 * before anything is enqueued.
 */
#define NWS_STFT_LOSS_MAX_RES 8
size_t nws_stft_loss_dft_bytes(int n_fft, int win_length);
int nws_stft_loss_dft_matrix(int n_fft, int win_length, float* dft_out, void* stream);
size_t nws_stft_loss_workspace_bytes(int B, int N, int R, const int* n_ffts, const int* hops);
int nws_stft_loss(const float* x, const float* y, int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths,
                  const float* const* dfts, float w_sc, float w_log_mag, float w_lin_mag, float eps, float* out, void* workspace,
                  size_t workspace_bytes, void* stream);

/*
 * Gradient of that loss with respect to the reconstruction x (csrc/stft_grad.hip; DESIGN.md 3.13 is the definition).  Same
 * arguments, operands (dfts) and refusals as the forward call above; grad_out: (B, N) fp32 on the device, overwritten.  There is no gradient
 * with respect to the target y.  Per resolution: the forward tile twice (the two Frobenius sums as per-workgroup fp64 records
 * reduced in a fixed order, then G formed in-lane), z = D^T G on the matrix pipe, and the overlap-add with the reflect fold as a
 * gather.  No floating-point atomics: equal inputs give equal bits.  Enqueue only.  The workspace (nws_stft_grad_workspace_bytes,
 * 0 for a refused size) holds G and z of the largest resolution - spectrogram-sized - and is reused across resolutions;
 * NWS_ERR_WORKSPACE if it is too small.
 */
size_t nws_stft_grad_workspace_bytes(int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths);
int nws_stft_grad(const float* x, const float* y, int B, int N, int R, const int* n_ffts, const int* hops, const int* win_lengths,
                  const float* const* dfts, float w_sc, float w_log_mag, float w_lin_mag, float eps, float* grad_out, void* workspace,
                  size_t workspace_bytes, void* stream);

/*
 * ---- The optimiser step (csrc/adam_step.hip) -----------------------------------------------------------
 * torch.nn.utils.clip_grad_norm_(max_norm, 2.0) followed by torch.optim.Adam (weight_decay 0, no amsgrad, no maximize) over n
 * float32 tensors in two launches (two more for every further NWS_ADAM_TABLE tensors):
 *   total = sqrt(sum_k sum_i g_k[i]^2)   float64 sums in an order fixed by the sizes, rounded once to float32
 *   c     = min(max_norm / (total + 1e-6), 1)   in float32 (max_norm = +inf: exactly 1);   gc = c g
 *   m'    = m + (1 - beta1)(gc - m);   v' = beta2 v + (1 - beta2) gc^2
 *   p'    = p - (lr / (1 - beta1^step)) m' / (sqrt(v') / sqrt(1 - beta2^step) + eps)
 * with the bias corrections computed on the host in float64.  param, exp_avg and exp_avg_sq are updated in place; grad is read
 * and NOT rewritten (clip_grad_norm_ scales it in place; this does not); total_norm: one device float.  No atomics: equal inputs
 * give equal bits.  NaN and Inf follow the formula.  `tensors` is a HOST array of n records of device pointers (each tensor
 * contiguous, 4-byte aligned, n elements).  Launches on `stream`, reads nothing back and decides every refusal before the first
 * launch: NWS_ERR_BAD_ARG for n < 1, a NULL pointer, a tensor of fewer than 1 element, step < 1, or a workspace that is NULL, not
 * 8-byte aligned or smaller than nws_adam_workspace_bytes (one double per NWS_ADAM_CHUNK elements of every tensor, rounded up per
 * tensor; 0 for what is refused; only the records' n fields are read); NWS_ERR_UNSUPPORTED for a tensor above 2^40 elements.
 */
#define NWS_ADAM_CHUNK 1024 /* elements a workgroup sums and updates */
#define NWS_ADAM_TABLE 64   /* tensors per launch */
typedef struct NwsAdamTensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  long long n;
} NwsAdamTensor;
size_t nws_adam_workspace_bytes(const NwsAdamTensor* tensors, int n);
int nws_adam_step(const NwsAdamTensor* tensors, int n, long long step, double lr, double beta1, double beta2, double eps,
                  double max_norm, float* total_norm, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ---- Gradient averaging for data-parallel training (csrc/grad_reduce.hip) -------------------------------
 * The ranks' gradients travel as rows of one (world, row_stride) buffer (an all-gather: data only); the mean is formed here in
 * rank order, so every rank holds the same bits whatever carried the rows.  No atomics, every output element written by one
 * thread.  Both launch on `stream`, read nothing back and decide every refusal before the first launch.
 *
 * nws_grad_pack: the n tensors (a HOST array of records of device pointers; each tensor contiguous, 4-byte aligned) copied one
 * after the other into dst[0 .. sum n); at most NWS_ADAM_TABLE tensors per launch.  NWS_ERR_BAD_ARG for n < 1, a NULL pointer, a
 * tensor of fewer than 1 element or dst_elems < sum n; NWS_ERR_UNSUPPORTED for a tensor above 2^40 elements.
 *
 * nws_grad_reduce: for i < n
 *   out[i] = (float)((sum_{r = 0 .. world-1} (double)rows[r row_stride + i]) / (double)world)
 * the sum in float64 in ascending r, divided once in float64, rounded once to float32; NaN and Inf follow the formula; world = 1
 * returns the row's own bits.  NWS_ERR_BAD_ARG for a NULL pointer, world < 1, n < 1, row_stride < n, or out[0 .. n) overlapping
 * [rows, rows + world row_stride); NWS_ERR_UNSUPPORTED for world > NWS_GRAD_MAX_WORLD or a row_stride above 2^40.
 */
#define NWS_GRAD_MAX_WORLD 1024
typedef struct NwsGradTensor {
  const float* src;
  size_t n;
} NwsGradTensor;
int nws_grad_pack(const NwsGradTensor* tensors, int n, float* dst, size_t dst_elems, void* stream);
int nws_grad_reduce(const float* rows, int world, size_t n, size_t row_stride, float* out, void* stream);

/*
 * ---- Runtime-size path (csrc/generic.hip): every gin-configurable size of the reference ------------------------------
 * The fused kernels above are compiled for gin/models/newt.gin.  These entry points take the sizes as arguments and run
 * one plain-fp32 stage kernel each (correct first, stage boundaries materialised); nws_forward_generic chains them into
 * NeuralWaveshaping.forward (models/neural_waveshaping.py:74-90) for ANY configuration:
 *   HarmonicOscillator.n_harmonics (generators.py:40-48), NeuralWaveshaping.n_waveshapers / control_hop (:31-62),
 *   NEWT.shaping_fn_size / out_channels (shaping.py:41-65), TrainableNonlinearity.depth (:15-34),
 *   ControlModule.hidden_size / embedding_size (neural_waveshaping.py:17-23), the h_generator's depth / hidden_size,
 *   FIRNoiseSynth.ir_length / hop_length (generators.py:13-19), Reverb.sr * length_in_seconds (shaping.py:156-158),
 *   FastNEWT table_size / table_min / table_max (shaping.py:83-105).
 */
/* TrainableNonlinearity(channels = n_shapers, width, depth) (shaping.py:15-37) or a FastNEWT table (lut != NULL) */
typedef struct NwsShaperDesc {
  int32_t n_shapers, width, depth, lut_size;
  float lut_min, lut_max;
  const float* in_scale; /* (n_shapers) */
  const float* w[8];     /* net.{2i}.weight: depth 1: (S); else layer 0: (S*width); hidden: (S*width, width); last: (S, width) */
  const float* b[8];     /* net.{2i}.bias */
  const float* lut;      /* (n_shapers, lut_size) or NULL */
} NwsShaperDesc;

typedef struct NwsGenericModel {
  int32_t control_size;   /* GRU input channels consumed (the reference's get_embedding always feeds 2, :69-72) */
  int32_t gru_hidden, embedding, n_harmonics, n_shapers;
  int32_t hop;            /* control_hop == FIRNoiseSynth.hop_length */
  int32_t newt_mlp_depth; /* 4 (NEWT hard-codes depth=4, shaping.py:53-55) */
  int32_t hgen_depth, hgen_hidden;
  int32_t fir_len;        /* FIRNoiseSynth.ir_length (even); the h_generator emits fir_len/2 + 1 bands */
  int32_t out_channels;   /* NEWT.out_channels (summed by forward's cat + sum(1)) */
  int32_t ir_len;         /* len(reverb.ir) = sr * length_in_seconds - 1 */
  float ln_eps, leaky_slope;
  const float *gru_w_ih, *gru_w_hh, *gru_b_ih, *gru_b_hh; /* (3H, control_size), (3H, H), (3H), (3H) */
  const float *proj_w, *proj_b;                           /* (embedding, H), (embedding) */
  const float *mixer_w, *mixer_b;                         /* (n_shapers, n_harmonics), (n_shapers) */
  const float* newt_mlp_w[8];
  const float* newt_mlp_b[8];
  const float* newt_ln_g[8];
  const float* newt_ln_b[8];
  const float* hgen_w[8];
  const float* hgen_b[8];
  const float* hgen_ln_g[8];
  const float* hgen_ln_b[8];
  const float *newt_out_w, *newt_out_b; /* (out_channels, n_shapers), (out_channels) */
  const float* noise_window;            /* (fir_len) */
  const float* ir;                      /* (ir_len) */
  NwsShaperDesc shaper;
} NwsGenericModel;

size_t nws_g_gru_workspace_bytes(int hidden);
/* torch.nn.GRU(C_in -> hidden, batch_first) over control[:, 0:C_in] of (B, C_total, T); out (B, T, hidden); h0 / hT optional */
int nws_g_gru(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, const float* control, int B,
              int C_total, int C_in, int hidden, int T, const float* h0, float* out, float* hT, void* workspace,
              size_t workspace_bytes, void* stream);
int nws_g_bth_to_bht(const float* x, int B, int T, int H, float* y, void* stream);
/* F.upsample(f0, T*hop, "linear") (f0 (B,T); or f0_up (B, T) given with hop = 1) + the double-accumulated cumsum and the
 * fp32 chain of generators.py:59: phase = fl(fl(tau * c) / sr).  f0_up_out optional. */
int nws_g_phase(const float* f0, const float* f0_up, int B, int T, int hop, float sample_rate, float* f0_up_out,
                float* phase_out, void* stream);
/* F.upsample(x, T * hop, mode="linear") row by row: x (rows, T) -> y (rows, T * hop) (neural_waveshaping.py:75, shaping.py:69) */
int nws_g_upsample(const float* x, int64_t rows, int T, int hop, float* y, void* stream);
/* HarmonicOscillator.forward (generators.py:58-66) for K harmonics: out (B, K, N) */
int nws_g_oscillator(const float* f0_up, const float* phase, const float* phase_u, const float* rand_phase, int K, int B, int N,
                     float sample_rate, float* out, void* stream);
/* nn.Conv1d(Cin, Cout, 1) on (B, Cin, N); bias may be NULL */
int nws_g_conv1x1(const float* x, const float* w, const float* bias, int B, int Cin, int Cout, int N, float* y, void* stream);
/* TrainableNonlinearity.forward / FastNEWT.shaping_fn on (rows = B * n_shapers, N) */
int nws_g_shaper_apply(const NwsShaperDesc* d, const float* x, int64_t rows, int64_t N, float* y, void* stream);
int nws_g_shaper_table(const NwsShaperDesc* d, int table_size, float table_min, float table_max, float* table_out, void* stream);
/* NEWT.forward before the mixer (shaping.py:68-76): exciter (B,S,N), film (B,4S,T) channel-major -> (B,S,N) */
int nws_g_film_shaper(const NwsShaperDesc* d, const float* exciter, const float* film, int B, int T, int hop, float* out,
                      void* stream);
/* The backward of nws_g_film_shaper followed by the Conv1d(S -> 1) mixer - NEWT.forward at any bank size - for grad_out =
 * dL/d(out) (B, N), N = 128 T (csrc/g_newt_grad.hip): 1 <= n_shapers <= 64, 1 <= width <= 16, 1 <= depth <= 4,
 * hop 128, one output channel (mix_w (S), mix_b (1)).  grad_film (B, 4S, T), grad_exciter (B, S, N) unless NULL, and, when
 * param_grads is given with all of its 2 depth + 3 entries, the parameter gradients in the layout of their parameters, in this
 * order: shaping_fn.input_scale, then net.{2l}.weight, net.{2l}.bias for l = 0 .. depth-1 (the shapes of NwsShaperDesc.w / .b),
 * then mixer.0.weight (S), mixer.0.bias (1).  Nothing is saved by the forward: it is recomputed per sample from exciter and film;
 * the gradient is that of the exact expression with the full-range sine (the forward kernel's hardware sine at widths 4 / 8 / 16
 * is about 4e-7 rad away).  The hidden layers' weight gradients are sums of exact fp32 products on the matrix pipe.  No atomics,
 * every sum in an order fixed by the sizes: equal inputs give equal bits, grad_out = 0 gives zeros, and neither grad_exciter nor
 * param_grads changes the other outputs' bits.  Launches on `stream`, reads nothing back and decides every refusal before the
 * first launch: NWS_ERR_BAD_ARG for a NULL required pointer (d's in_scale / w / b entries below depth included), some but not all
 * of the 2 depth + 3 parameter gradients, a size < 1, or a workspace that is NULL or smaller than
 * nws_g_newt_grad_workspace_bytes; NWS_ERR_UNSUPPORTED for a descriptor that carries a table (FastNEWT has no backward),
 * hop != 128, n_shapers > 64, width > 16, depth > 4, T > 65 535 or B T > 2^28.  nws_g_newt_grad_workspace_bytes: 0 for sizes that
 * are refused. */
size_t nws_g_newt_grad_workspace_bytes(const NwsShaperDesc* d, int B, int T, int want_params);
int nws_g_newt_grad(const NwsShaperDesc* d, const float* mix_w, const float* mix_b, const float* exciter, const float* film,
                    const float* grad_out, int B, int T, int hop, float* grad_exciter /* may be NULL */, float* grad_film,
                    float* const* param_grads /* NULL, or a HOST array of 2 depth + 3 device pointers */, void* workspace,
                    size_t workspace_bytes, void* stream);
/* FIRNoiseSynth (generators.py:21-35) for any even ir_length >= hop: H (B, L/2+1, T) -> taps (B, T, L); then the noise
 * branch (+ the sum over `add_channels` channels of add_in (B, add_channels, N), NULL = none) -> out (B, N) */
int nws_g_fir_design(const float* H, const float* window, int fir_len, int B, int T, float* fir_out, void* stream);
int nws_g_fir_noise(const float* fir, const float* noise, int fir_len, int hop, int B, int T, const float* add_in,
                    int add_channels, float* out, void* stream);
/* Reverb.forward without a transform plan (nws_reverb_plan serves every even circular length; this entry point is what is left):
 * the circular convolution summed in the time domain when L = max(N, ir_len + 1) is even; for ODD L the reference's own
 * rfft(L) / irfft(L - 1) result (shaping.py:171-173 passes no length to irfft: not a circular convolution), evaluated in float64
 * at O(L^2) with stream-ordered scratch (hipMallocAsync); NWS_ERR_UNSUPPORTED for odd L > 2^22 */
int nws_g_reverb_direct(const float* x, const float* ir, int ir_len, int B, int N, float* y, void* stream);

size_t nws_forward_generic_workspace_bytes(const NwsGenericModel* m, int B, int T);
/* plan / reverb_tables / reverb_spectrum / reverb_workspace: from nws_reverb_plan & co when the plan exists for
 * (T*hop, ir_len+1), else all NULL (time-domain reverb) */
int nws_forward_generic(const NwsGenericModel* m, const float* f0, const float* control, int B, int C, int T, float sample_rate,
                        const float* phase_u, const float* rand_phase, const float* noise, const NwsReverbPlan* plan,
                        const void* reverb_tables, const void* reverb_spectrum, void* reverb_workspace,
                        size_t reverb_workspace_bytes, float* out, void* workspace, size_t workspace_bytes, void* stream);

/*
 * ---- Stateful streaming on the runtime-size path (csrc/generic.hip): nws_stream_step's contract for any model
 * nws_forward_generic takes whose control hop is 128, whose noise filter has 256 taps under a window symmetric about tap 128
 * (the caller checks the window, as for nws_frame_mlps) and whose impulse response fits the ring (ir_len < 32 768).  The
 * argument list is nws_stream_step's with the model descriptor in place of NwsWeights; the design matrix, the impulse response
 * and its length come from the descriptor.  nws_stream_reset, nws_stream_out_samples, nws_stream_noise_draws and
 * nws_stream_noise_start serve both paths; the state blob has its own layout (nws_g_stream_state_bytes, nws_g_stream_reverb_tail).
 * One call is one chunk of K <= max_frames frames: out (B, M), M = nws_stream_out_samples(K, first, final); phase_u and
 * rand_phase hold n_harmonics values; out_channels > 1 are summed (models/neural_waveshaping.py:84-86).  Nothing is allocated,
 * read back or synchronised, and every refusal is decided before the first launch, with outputs and state untouched:
 * NWS_ERR_BAD_ARG for a NULL required pointer, an incomplete descriptor, B < 1, K < 1, K > max_frames, C < control_size, both or
 * neither of noise_new / noise_all, `first` disagreeing with frames_seen == 0, or a chunk beyond 2048 samples without a plan that
 * holds ir_len + M samples; NWS_ERR_UNSUPPORTED for another hop or filter length, ir_len >= 32 768, B > 65 535 or layer widths
 * the stage kernels refuse; NWS_ERR_WORKSPACE for a state blob smaller than nws_g_stream_state_bytes (which is 0 for every
 * size that is refused).
 */
size_t nws_g_stream_state_bytes(const NwsGenericModel* m, int B, int max_frames, int ir_len, const NwsReverbPlan* plan);
int nws_g_stream_step(const NwsGenericModel* m, const NwsReverbPlan* plan, const void* reverb_tables, const void* reverb_spectrum,
                      void* state, size_t state_bytes, int B, int max_frames, const float* f0 /* (B,K) */,
                      const float* control /* (B,C,K) */, int C, int K, int first, int final, long long frames_seen,
                      long long nz_prev_start, float sample_rate, const float* phase_u, const float* rand_phase,
                      const float* noise_new, const float* noise_all, int noise_all_len, float* out /* (B, M) */,
                      float* pre_out /* optional (B, M) */, void* stream);
int nws_g_stream_reverb_tail(const NwsGenericModel* m, const NwsReverbPlan* plan, const void* reverb_tables,
                             const void* reverb_spectrum, void* state, size_t state_bytes, int B, int max_frames,
                             float* tail_out /* (B, ir_len + 1) */, void* workspace, size_t workspace_bytes, void* stream);

/*
 * Slot mode of the runtime-size stream (csrc/generic.hip): nws_stream_step_slots' contract - B voice slots, one hop
 * of 1 <= K <= 16 frames per call, (B, 128 K) out, `events` a (B) int32 array of NWS_SLOT_* words in DEVICE memory read by the
 * launches, the call with frames_seen == 0 the all-idle pre-roll - for every model nws_g_stream_step serves.  The argument list is
 * nws_stream_step_slots' with the model descriptor in place of the weights, the design matrix and the impulse response.  A chain of
 * launches: nothing waits inside a launch, so there is no give-up flag to read.  Refusals, all before the first launch with
 * outputs and state untouched: those of nws_g_stream_step, NWS_ERR_BAD_ARG for events == NULL, NWS_ERR_UNSUPPORTED for K > 16 or
 * max_frames > 16, NWS_ERR_WORKSPACE for a blob smaller than nws_g_stream_slot_state_bytes - which is 0 for every size
 * nws_g_stream_state_bytes refuses and for max_frames > 16.  The blob is a plain stream's without a plan (every offset of it where it
 * was) followed by two per-row arrays; nws_stream_reset and nws_g_stream_reverb_tail serve it.
 */
size_t nws_g_stream_slot_state_bytes(const NwsGenericModel* m, int B, int max_frames, int ir_len);
int nws_g_stream_step_slots(const NwsGenericModel* m, void* state, size_t state_bytes, int B, int max_frames,
                            const float* f0 /* (B,K) */, const float* control /* (B,C,K) */, int C, int K, long long frames_seen,
                            long long nz_prev_start, float sample_rate, const float* phase_u, const float* rand_phase,
                            const float* noise_new, const float* noise_all, int noise_all_len, const int* events /* (B) device */,
                            float* out /* (B, 128 K) */, float* pre_out /* optional */, void* stream);

/*
 * Note player (ABI v6; csrc/note_control.hip; no reference counterpart: the reference renders recordings only).
 * The two launches around a hop of nws_stream_step_slots that turn notes into a signal.
 *
 * nws_note_control: ONE launch on `stream` in front of the hop.  Reads the hop's event words `events` (B) int32 with the NWS_SLOT_*
 * bits - the tensor the slot stream itself reads -, the per-slot note table `notes` (B), which the host writes only when a note
 * starts or ends, and the per-slot int32 frame counters in `state`; writes f0 (B, K) in Hz and control (B, 2, K), normalised with
 * mean / std.  A slot with NWS_SLOT_ACTIVE gets frames j = j0 .. j0 + K - 1 of its voice, j0 = 0 with NWS_SLOT_START and the
 * slot's counter otherwise, and leaves j0 + K in the counter (saturating at 2^30); every other slot gets f0 = 0, control = 0 and
 * keeps its counter.  With p = peak_lo + velocity (peak_hi - peak_lo), q = silence, A / D / R = attack / decay / release:
 *     h(j)  = p - (p - q) (A - 1 - j) / A  for j < A;   p - drop (j - A + 1) / D  for A <= j < A + D;   p - drop  beyond;  h(-1) = q
 *     l(j)  = h(j)  for j < j_off;   q + (h(j_off - 1) - q) (R - min(j - j_off + 1, R)) / R  from j_off on
 *     c(j)  = vib_depth clamp((j - vib_delay) / vib_ramp, 0, 1) sin(2 pi frac(vib_rate 128 j / sample_rate))      [cents]
 *     f0(j) = 440 2^((pitch - 69) / 12 + c(j) / 1200),   control(j) = ((f0(j) - mean[0]) / std[0], (l(j) - mean[1]) / std[1])
 * Closed forms in j: a voice's bits do not depend on how its frames are cut into hops.  The vibrato phase is formed and reduced in
 * float64; the rest is fp32.  Nothing is read back, nothing is allocated, and no argument of a steady hop changes: the launch can
 * be captured, or sit in front of a captured hop on that hop's own input buffers.
 * nws_note_control_state_bytes: size of the counter blob (0 for B outside 1 .. 65 535); nws_note_control_reset zeroes it.
 *
 * nws_voice_mix: out[c, n] = sum_b gain[b, c] o[b, n] for o (B, N), gain (B, C), out (C, N), C = 1 or 2.  b ascending in one fp32
 * chain of fused multiply-adds per output element, each element written by one thread, no atomics: two calls give equal bits.
 * float4 loads and stores when N is a multiple of 4 and o and out are 16-byte aligned, a scalar kernel otherwise.
 *
 * Every refusal is decided before the first launch and leaves state and outputs untouched.  NWS_ERR_BAD_ARG: a NULL pointer,
 * B / K / N < 1, K > 16, C outside {1, 2}, release < 1, vib_ramp < 1, a negative attack / decay / vib_delay / drop / vib_rate, a
 * frame count above 2^24, sample_rate <= 0, std <= 0, a state blob below nws_note_control_state_bytes.  NWS_ERR_UNSUPPORTED:
 * B > 65 535.
 */
typedef struct NwsNotePlayer {
  double vib_rate;       /* Hz */
  double sample_rate;    /* of the model: a frame is 128 samples */
  int attack, decay, release;   /* A >= 0, D >= 0, R >= 1 frames */
  int vib_delay, vib_ramp;      /* frames; ramp >= 1 */
  float drop;            /* sustain level below the peak; loudness units: (dB + 80) / 80 */
  float silence;         /* q */
  float peak_lo, peak_hi; /* peak loudness at velocity -> 0 and at velocity 1 */
  float vib_depth;       /* cents */
  float mean[2], std[2]; /* the checkpoint's statistics of F0 and loudness */
} NwsNotePlayer;
typedef struct NwsNote {
  float pitch;     /* MIDI note number */
  float velocity;  /* (0, 1] */
  int j_off;       /* first release frame; 2^31 - 1 while the note is held */
  int reserved;
} NwsNote;
size_t nws_note_control_state_bytes(int B);
int nws_note_control_reset(void* state, size_t state_bytes, int B, void* stream);
int nws_note_control(const NwsNotePlayer* player, const int* events /* (B) */, const NwsNote* notes /* (B) */, void* state,
                     size_t state_bytes, int B, int K, float* f0 /* (B, K) */, float* control /* (B, 2, K) */, void* stream);
int nws_voice_mix(const float* o /* (B, N) */, const float* gain /* (B, C) */, int B, int N, int C, float* out /* (C, N) */,
                  void* stream);

/* Diagnostic entry points (kernel ablations for timing, the co-execution hazard probes) are declared in nws_hip_debug.h: they are
 * exported by the same library but are not part of the product ABI. */

/*
 * Live profiling of nws_forward (bench.py's roofline leg): hipEvents are recorded on the launch stream around
 * the stages selected by stage_mask (bit 0 phase carries, 1 GRU, 2 frame MLPs, 3 exciter+NEWT, 4 FIR noise,
 * 5 reverb) for the next `slots` calls.  nws_profile_collect synchronises the events and writes
 * ms_out[call][6] (-1 for unselected stages).
 */
#define NWS_N_STAGES 6
int nws_profile_begin(int slots, unsigned stage_mask);
int nws_profile_collect(float* ms_out /* host, slots*6 */, int* n_out /* host */);
int nws_profile_end(void);

/* Waveform exchange of the multi-GPU path, host side (ABI v6; SURVEY 8(e) - the reference has no collective code:
 * gin/train/train_newt.gin:13 is its only trace of more than one GPU).  nws_peer_push: for i < n, one asynchronous device-to-device
 * copy of `bytes` from src to dst[i] (a peer-mapped or local device pointer) on streams[i], then hipEventRecord(events[i],
 * streams[i]) when events and events[i] are non-NULL - one call per step instead of n copies + n records through the host
 * language.  nws_events_wait: hipEventSynchronize on every non-NULL event (HOST-side wait; the calling thread blocks). */
int nws_peer_push(int n, void* const* dst, const void* src, size_t bytes, void* const* streams, void* const* events);
int nws_events_wait(int n, void* const* events);
/* hipStreamSynchronize on every stream (HOST-side wait): the pushes of the previous step are awaited this way - no event record
 * per copy on the copy queues (every record is one more packet for the command processor beside the pipeline's own). */
int nws_streams_wait(int n, void* const* streams);

/* Which pipe of the command processor serves a stream's hardware queue (ABI v6; no reference counterpart: the reference enqueues
 * everything on one stream, models/neural_waveshaping.py:74-90 - this serves the throughput mode of that forward,
 * ForwardPipeline, whose five streams must sit on the pipes in a fixed pattern: DESIGN.md 5.2).
 * Launches a grid of `groups` one-wave workgroups on `stream_hold` that each hold 64 000 B of LDS (two per CU: the grid is handed
 * out in rounds of 512) and spin for `spin_us` microseconds, and right behind it ONE wave on `stream_touch` that stores the
 * wall clock; synchronises both streams (a measurement, not a hot-path call) and returns in *frac_out
 *     (touch time - first workgroup start) / (last workgroup start - first workgroup start):
 * ~0 when the second queue was served while the first was dispatching (different pipes), >= ~1 when it had to wait for the
 * whole grid to be handed out (same pipe, or one hardware queue shared by both streams); -1 when the grid was too small to
 * be held (groups <= 512).  `scratch`: device memory, 32 bytes. */
int nws_queue_probe(void* stream_hold, void* stream_touch, int groups, int spin_us, unsigned long long* scratch, float* frac_out /* host */);

#ifdef __cplusplus
}
#endif
#endif /* NWS_HIP_H */
