// Per-point score maps of a decoded forecast, accumulated on the device over initial times: for Cm chosen
// channels and P planes that pool one or more lead times each, the additive sufficient statistics of bias, RMSE, spread, spread-skill
// ratio, CRPS (skill / spread) and ACC at every grid point.  The result is as large as the field, so it never goes to the host per
// initial time: the buffers live on the device, every call adds to them in place, and they are read back once.  Not in the reference.
// Addressing is that of ldc_rollout_regional (regional.hip) without lat_weight: the maps are unweighted.  The eight fp32 point values
// and the two validity flags are ensemble_point_values (ensemble_common.h), the function regional_kernel calls: the same bits.  The whole
// file is built with -ffp-contract=off.
// sums   [Cm][P][8][H * W] fp64, term-major so that a wave's accesses are contiguous: e, se, var, skill, spread, fa*ta, fa*fa, ta*ta.
//        A valid point adds double(v) to terms 0 .. 4, an ACC-valid point also to 5 .. 7; an invalid point adds nothing.
// counts [Cm][P][3][H * W] int32: valid, invalid, ACC-valid.  Without a climatology terms 5 .. 7 and count 2 are not touched.
// One thread per (channel, plane, point): grid (tiles of 256 points, Cm, P), no atomics.  The thread loads its accumulators, walks the
// lead times of the call in ascending order, adds those whose plane_of_lead is its plane, and stores: one read-modify-write per call
// however many lead times the plane pools, and the bits of a plane depend on the sequence of contributions alone.  A workgroup whose plane
// no lead time of the call names exits before it loads a member or an accumulator.
#include <math.h>

#include "../../include/ladcast_hip_ext.h"
#include "ensemble_common.h"

namespace {

constexpr int TPB = 256;
constexpr int NT = LDC_SCORE_MAPS_TERMS;
constexpr int NC = LDC_SCORE_MAPS_COUNTS;

struct MapArgs {
  RolloutView v;       // clim nullptr: no ACC terms; lat_w unused
  const int* chan;     // [Cm]
  const int* plane;    // [L]
  double* sums;        // [Cm][P][NT][HW]
  int* counts;         // [Cm][P][NC][HW]
  int L, P;
};

template <int NP, int NUSE, bool INV>
__global__ __launch_bounds__(TPB) void score_maps_kernel(MapArgs a) {
  const int ci = blockIdx.y, pl = blockIdx.z;
  int l0 = 0;
  while (l0 < a.L && a.plane[l0] != pl) ++l0;  // uniform over the workgroup
  if (l0 == a.L) return;
  const int HW = a.v.H * a.v.W;
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= HW) return;  // the padding threads of the last tile; no barrier below
  const int c = a.chan[ci];
  const bool has_clim = a.v.clim != nullptr;
  const InvNorm nrm = view_norm<INV>(a.v, c);
  const long long ent = static_cast<long long>(ci) * a.P + pl;
  double* sp = a.sums + ent * NT * HW + p;
  int* cp = a.counts + ent * NC * HW + p;
  double acc[NT];
#pragma unroll
  for (int k = 0; k < NT; ++k) acc[k] = (k < 5 || has_clim) ? sp[static_cast<long long>(k) * HW] : 0.0;
  int n_val = cp[0], n_inv = cp[HW], n_acc = has_clim ? cp[2 * static_cast<long long>(HW)] : 0;
  for (int l = l0; l < a.L; ++l) {
    if (a.plane[l] != pl) continue;
    const float* cbase = view_clim(a.v, c, l);
    const PointValues pv = ensemble_point_values<NP, NUSE, INV>(view_forecast(a.v, c, l) + p, a.v.fc_ms, nrm, a.v.M, view_truth(a.v, c, l) + p,
                                                                cbase ? cbase + p : nullptr);
    if (pv.valid) {
      acc[0] += static_cast<double>(pv.e);
      acc[1] += static_cast<double>(pv.se);
      acc[2] += static_cast<double>(pv.var);
      acc[3] += static_cast<double>(pv.skill);
      acc[4] += static_cast<double>(pv.spread);
      ++n_val;
    } else {
      ++n_inv;
    }
    if (pv.acc_valid) {
      acc[5] += static_cast<double>(pv.fta);
      acc[6] += static_cast<double>(pv.ffa);
      acc[7] += static_cast<double>(pv.tta);
      ++n_acc;
    }
  }
#pragma unroll
  for (int k = 0; k < NT; ++k)
    if (k < 5 || has_clim) sp[static_cast<long long>(k) * HW] = acc[k];
  cp[0] = n_val;
  cp[HW] = n_inv;
  if (has_clim) cp[2 * static_cast<long long>(HW)] = n_acc;
}

template <bool INV>
void launch_score_maps(const MapArgs& a, dim3 grid, hipStream_t s) {
  ldc_dispatch_sort_arm(a.v.M, [&](auto np, auto nuse) {
    hipLaunchKernelGGL((score_maps_kernel<decltype(np)::value, decltype(nuse)::value, INV>), grid, dim3(TPB), 0, s, a);
  });
}

}  // namespace

extern "C" long long ldc_score_maps_bytes(int Cm, int P, int H, int W) {
  if (Cm <= 0 || Cm > 65535 || P <= 0 || P > 65535 || H <= 0 || W <= 0) return 0;
  if (static_cast<long long>(H) * W > (1ll << 24)) return 0;
  return static_cast<long long>(Cm) * P * H * W * (NT * 8 + NC * 4);
}

extern "C" int ldc_rollout_score_maps(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                      const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                                      long long truth_channel_stride, const int* truth_slot, const float* clim, long long clim_slot_stride,
                                      long long clim_channel_stride, const int* clim_slot, const int* channel_idx, int Cm,
                                      const int* plane_of_lead, int P, int M, int C, int L, int H, int W, double* sums, int* counts,
                                      void* stream) {
  MapArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, clim, clim_slot_stride, clim_channel_stride, clim_slot, nullptr, M, C, L, H, W, L, 0,
                       true, false) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(channel_idx);
  LDC_CHECK_PTR(plane_of_lead);
  LDC_CHECK_PTR(sums);
  LDC_CHECK_PTR(counts);
  if (Cm <= 0 || P <= 0) return LDC_ERR_ARG;
  if (M > 64 || Cm > 65535 || P > 65535 || static_cast<long long>(H) * W > (1ll << 24)) return LDC_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(sums) & 7u) != 0) return LDC_ERR_ALIGN;  // fp64
  a.chan = channel_idx;
  a.plane = plane_of_lead;
  a.sums = sums;
  a.counts = counts;
  a.L = L;
  a.P = P;
  dim3 grid(ldc_cdiv(static_cast<long long>(H) * W, TPB), Cm, P);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) launch_score_maps<true>(a, grid, s);
  else launch_score_maps<false>(a, grid, s);
  return ldc_launch_status();
}
