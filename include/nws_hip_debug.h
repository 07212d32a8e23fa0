/*
 * Diagnostic entry points of libnws_hip.so - NOT part of the product ABI (include/nws_hip.h).  (The probes that demonstrate the
 * MI355X co-execution hazard live in a library of their own, include/nws_probe.h -> libnws_probe.so: their kernels contain the
 * instruction form the build refuses in this one.)  Used by tools/ and tests; a binding of the product path never needs this file.
 */
#ifndef NWS_HIP_DEBUG_H
#define NWS_HIP_DEBUG_H
#include "nws_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Tests / measurements: which frame-MLP kernel nws_frame_mlps launches - 0 automatic (wave-resident frames from 8192 frames up,
 * tile kernels below), 1 the tile kernels, 2 wave-resident frames at any size.  Any other mode: NWS_ERR_BAD_ARG. */
int nws_debug_frame_mlps_kernel(int mode);

/* Tests / A-B measurements: on = 0 keeps the forward on the tap hand-over (nws_frame_mlps + nws_fir_noise) where it would hand
 * filter spectra over (nws_frame_mlps_spec_serves then answers 0); any other value restores the default. */
int nws_debug_forward_spec(int on);

/* Tests / A-B measurements: the form of the folded frame-MLP launch (nws_frame_mlps_spec, nws_frame_mlps_spec_beside and the
 * forwards) - 0 by the rule of nws_frame_mlps_spec_beside, 8 or 12 that many waves per workgroup wherever it runs.  Any other
 * value: NWS_ERR_BAD_ARG.  nws_debug_frame_mlps_last_waves: the form of the most recent folded launch of this process (0: none yet). */
int nws_debug_frame_mlps_waves(int waves);
int nws_debug_frame_mlps_last_waves(void);

/* Tests: the folded wave-resident kernel in the form of `waves` (8 or 12) waves per workgroup on F flattened frames of any
 * count (gru_out (F,128) -> film_out (F,256), spec_out (F,NWS_SPEC_ROW)), whatever the size rules of nws_frame_mlps_spec say.
 * NWS_ERR_UNSUPPORTED without the folded tables (w->mlp_spec) or beyond the kernel's 32-bit byte offsets. */
int nws_debug_frame_mlps_spec_waves(const NwsWeights* w, const float* gru_out, int F, float* film_out, float* spec_out, int waves,
                                    void* stream);

/* Diagnostics only (tools/cu_pressure.py): a resident load of `groups` 256-thread workgroups that keep their CUs' vector pipes
 * busy for `spin_us` microseconds of the wall clock - what a collective's ring kernels take from the oscillator kernel. */
int nws_debug_queue_busy(int groups, int spin_us, float* sink /* device float[256] */, void* stream);

/* Tests: which oscillator-to-NEWT kernel nws_forward_generic launches for `model` (sizes and shaper.lut == NULL only: no pointer
 * is followed) at batch B and T frames, and with what.  Reports, launches nothing, changes nothing.
 *   out[0] family: 0 none (more than 64 shapers / 4 output channels, or LDS: the stage kernels run), 1 g_exciter_newt_mfma_kernel
 *                  <MT, OCT>, 2 g_exciter_newt_kernel<SB, EXC_ONLY> (thread per sample: the mixer fragments do not fit LDS)
 *   out[1] MT (family 1) or SB (family 2)     out[2] OCT: 1 / 2 / 4, 0 = the kernel stops at the exciter (sin-MLP shapers)
 *   out[3] tpw, tiles of 32 samples per wave (family 1)     out[4] nf, FiLM frames staged per workgroup
 *   out[5] dynamic LDS bytes     out[6] 1: nws_g_film_shaper and nws_g_conv1x1 follow the kernel
 *   out[7] tpw by the ">= 1024 workgroups" rule alone, before the LDS rules lowered it (family 1) */
int nws_debug_generic_exciter_plan(const NwsGenericModel* model, int B, int T, int out[8]);

/* Tests: which recurrence nws_g_gru launches.  out[0]: 0 the default-shape kernel of csrc/control_gru.hip (hidden 128, C_in 2),
 * 1 g_gru_q_kernel<kq> (W_hh in registers), 2 g_gru_kernel (W_hh streamed from L2); out[1] kq (8 / 16 / 32, else 0); out[2]
 * workgroup size; out[3] dynamic LDS bytes.  NWS_ERR_UNSUPPORTED where nws_g_gru refuses. */
int nws_debug_generic_gru_plan(int hidden, int C_in, int out[4]);

#ifdef __cplusplus
}
#endif
#endif /* NWS_HIP_DEBUG_H */
