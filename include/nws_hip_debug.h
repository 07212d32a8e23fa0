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

/* Diagnostics only (tools/cu_pressure.py): a resident load of `groups` 256-thread workgroups that keep their CUs' vector pipes
 * busy for `spin_us` microseconds of the wall clock - what a collective's ring kernels take from the oscillator kernel. */
int nws_debug_queue_busy(int groups, int spin_us, float* sink /* device float[256] */, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* NWS_HIP_DEBUG_H */
