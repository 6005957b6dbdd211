/* ladcast_hip_ext.h -- entry points of libladcast_hip.so that were added after the recorded set of ladcast_hip.h.
 *
 * ladcast_hip.h is held to a fixed list of entry points and structs by the ABI tests; an entry point that comes later is declared here,
 * with flat scalar and pointer arguments and no struct of its own.  The conventions are those of ladcast_hip.h, which this header
 * includes for the status codes: every pointer is a DEVICE pointer unless said otherwise, every function returns LDC_OK or a negative
 * status and launches nothing on an error, `stream` is a hipStream_t.  The ABI version stays LDC_ABI_VERSION (5): the additions are
 * additive.  ladcast_amd.abi reads this header as it reads the first one (EXT_CONSTANTS, EXT_SIGNATURES) and ladcast_amd.hip binds its
 * symbols at load.
 */
#ifndef LADCAST_HIP_EXT_H
#define LADCAST_HIP_EXT_H

#include "ladcast_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Per-point score maps, accumulated on the device over initial times (score_maps.hip): for chosen channels and
 * for planes that pool one or more lead times, the additive sufficient statistics of bias, RMSE, spread, spread-skill ratio, CRPS and
 * ACC at EVERY grid point.  ladcast_amd.evaluate.score_maps derives the scores on the host in float64.  Not in the reference.
 * Addressing of forecast, inverse normalisation (mean == NULL: physical units), truth and climatology tables (clim == NULL: no ACC
 * terms) exactly as ldc_rollout_regional; there is no lat_weight: the maps are unweighted, weights enter when maps are pooled on the
 * host.  1 <= M <= 64.
 * channel_idx:   DEVICE int [Cm], the channels (0 .. C - 1) of the forecast that get maps; any order, need not be contiguous.
 * plane_of_lead: DEVICE int [L], the plane 0 .. P - 1 that lead time l of this call adds to, or -1: skipped.  Several lead times may
 *   share a plane (a lead-time bin).  The values of both arrays are the caller's responsibility, as with truth_slot.
 * Per point the eight fp32 values e, se, var, skill, spread, fa * ta, fa * fa, ta * ta and the two validity flags are those of
 * ldc_rollout_regional, bit for bit (one device function serves both kernels).
 *   sums   [Cm][P][LDC_SCORE_MAPS_TERMS][H * W] fp64, terms in the order above: a valid point adds double(v) to terms 0 .. 4, an ACC-valid
 *     point also to terms 5 .. 7; an invalid point adds nothing.  +-inf are ordinary values.
 *   counts [Cm][P][LDC_SCORE_MAPS_COUNTS][H * W] int32: valid, invalid, ACC-valid samples of the point.
 *   Both are READ AND ADDED TO; the caller zeroes them once (ldc_score_maps_bytes(Cm, P, H, W) = 76 bytes per entry for the two
 *   together; 0 for sizes the call refuses).  With clim == NULL terms 5 .. 7 and count 2 are not touched.  Planes no lead time of the
 *   call names are not touched.
 * One thread owns a (channel, plane, point) in a launch and there are no atomics: the lead times of a call that share a plane are added
 * in ascending order onto the loaded value, in registers, so a plane costs one read-modify-write per call.  The bits of a plane depend
 * on the sequence of (call, lead time) contributions alone - not on L, on how the lead times are batched into calls, on Cm, P, the
 * other channels or the strides - and two runs give the same bits.
 * LDC_ERR_ARG: a null or non-positive argument, clim without clim_slot, mean without std_; LDC_ERR_UNSUPPORTED: M > 64, Cm > 65535,
 * P > 65535 or H * W > 2^24; LDC_ERR_ALIGN: sums not 8-byte aligned.  Nothing is launched on an error. */
#define LDC_SCORE_MAPS_TERMS 8
#define LDC_SCORE_MAPS_COUNTS 3
long long ldc_score_maps_bytes(int Cm, int P, int H, int W);
int ldc_rollout_score_maps(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride, const float* mean,
                           const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                           long long truth_channel_stride, const int* truth_slot, const float* clim, long long clim_slot_stride,
                           long long clim_channel_stride, const int* clim_slot, const int* channel_idx, int Cm, const int* plane_of_lead,
                           int P, int M, int C, int L, int H, int W, double* sums, int* counts, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LADCAST_HIP_EXT_H */
