// Shared by the threshold-event kernels (events.hip: the point-wise verification histogram; fss.hip: the neighbourhood verification): the
// classification of one grid point of one event, in one place so that both give the same n, o and validity.
#pragma once
#include "ensemble_common.h"

// DIR > 0: a > thr; DIR < 0: a < thr.  A NaN compares false either way (such a point is not valid and is never counted).
template <int DIR>
__device__ __forceinline__ int hit(float a, float thr) {
  if constexpr (DIR > 0) return a > thr ? 1 : 0;
  else return a < thr ? 1 : 0;
}

// What a grid point says about an event: n of the M members show it, the truth does (o = 1) or does not, and the point counts
// (valid) when no member, not the truth and (anomaly) not the climatology is NaN.  n and o are meaningful at valid points only.
struct EventPoint {
  int n, o;
  bool valid;
};

// f: member 0 of the point, members fc_ms apart; t, cl: truth and climatology there (cl = 0 when the event is no anomaly event).
// NMAX > 0: M <= NMAX members loaded into registers before they are compared; NMAX == 0: any M, streamed.  Members after the inverse
// normalisation (INV), anomaly as one fp32 subtraction each.
template <int NMAX, bool INV, int DIR>
__device__ __forceinline__ EventPoint classify_event_point(const float* f, long long fc_ms, int M, float t, float cl, bool anom, float thr,
                                                           const InvNorm& nrm) {
  constexpr int NX = NMAX > 0 ? NMAX : 1;
  int n = 0;
  bool nan_m = false;
  if constexpr (NMAX > 0) {
    float x[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = i < M ? load_member<false>(f, i, fc_ms, nrm) : 0.f;  // every load issued before a value is used
#pragma unroll
    for (int i = 0; i < NX; ++i)
      if (i < M) {
        float v = x[i];
        if constexpr (INV) v = inv_norm(v, nrm);
        nan_m = nan_m || (v != v);
        const float u = anom ? v - cl : v;
        n += hit<DIR>(u, thr);
      }
  } else {
    for (int i = 0; i < M; ++i) {
      const float v = load_member<INV>(f, i, fc_ms, nrm);
      nan_m = nan_m || (v != v);
      const float u = anom ? v - cl : v;
      n += hit<DIR>(u, thr);
    }
  }
  const int o = hit<DIR>(anom ? t - cl : t, thr);
  return EventPoint{n, o, !nan_m && t == t && cl == cl};
}
