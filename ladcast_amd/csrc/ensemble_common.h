// Shared by the ensemble-statistics kernels (scoring.hip, reliability.hip, spectrum.hip, products.hip, regional.hip, score_maps.hip, energy.hip and, through
// events_common.h, events.hip and fss.hip): the fused inverse normalisation, the register sort with its (NP, NUSE) ladder over the ensemble
// size, the members-in-registers ladder, the point values that the regional scores and the score maps share, and RolloutView - how the
// ten entry points that read a decoded rollout (ldc_rollout_scores, ldc_validation_scores, ldc_rollout_reliability / _spectrum / _products /
// _events / _fss / _regional / _score_maps / _energy) address a forecast, its truth and its climatology, with the one host function that
// checks and fills it.  ldc_ensemble_scores (one lead time, no slots) keeps its own.
#pragma once
#include <math.h>

#include <type_traits>

#include "common.h"

// The inverse normalisation of decode_latent_ens fused into the load: (v / target_std) * sd + mn, every operation rounded on its own as
// chan_affine_kernel (layout.hip) and track_gather_kernel (track.hip) round theirs - those files are built with -ffp-contract=off, not
// every file that includes this one is, so the contraction is switched off here.  x / 1 == x: the division is skipped for the default
// target_std.
struct InvNorm {
  float target_std, sd, mn;
  bool unit;  // target_std == 1
};

__device__ __forceinline__ float inv_norm(float v, const InvNorm& n) {
#pragma clang fp contract(off)
  const float q = n.unit ? v : v / n.target_std;
  const float m = q * n.sd;
  return m + n.mn;
}

__device__ __forceinline__ InvNorm make_inv_norm(float target_std, const float* sd, const float* mean, int c) {
  return InvNorm{target_std, sd[c], mean[c], target_std == 1.0f};
}

// Batcher's odd-even merge sort for NP = 2^k registers, fully unrolled (compile-time register indices).  Every
// comparator is ascending (min to the lower index), so comparators that touch an index >= NUSE -- registers that hold
// the +inf padding behind the members -- are no-ops and are pruned at compile time.
template <int NP, int NUSE>
__device__ __forceinline__ void sort_network(float (&x)[NP]) {
#pragma unroll
  for (int p = 1; p < NP; p <<= 1) {
#pragma unroll
    for (int k = p; k >= 1; k >>= 1) {
#pragma unroll
      for (int j = k % p; j <= NP - 1 - k; j += 2 * k) {
#pragma unroll
        for (int i = 0; i < k; ++i) {
          const int lo_i = i + j, hi_i = i + j + k;
          if (hi_i < NUSE && (lo_i / (2 * p)) == (hi_i / (2 * p))) {
            const float a = x[lo_i], b = x[hi_i];
            x[lo_i] = fminf(a, b);
            x[hi_i] = fmaxf(a, b);
          }
        }
      }
    }
  }
}

// The sort arm that serves M <= 64 members: NUSE = M rounded up to a multiple of 8 (16 below 16), NP = the next power of two.  Calls
// f(integral_constant<NP>, integral_constant<NUSE>), from which the caller launches its kernel<NP, NUSE>.
template <class F>
static inline void ldc_dispatch_sort_arm(int M, F&& f) {
  using std::integral_constant;
  if (M <= 8) f(integral_constant<int, 8>{}, integral_constant<int, 8>{});
  else if (M <= 16) f(integral_constant<int, 16>{}, integral_constant<int, 16>{});
  else if (M <= 24) f(integral_constant<int, 32>{}, integral_constant<int, 24>{});
  else if (M <= 32) f(integral_constant<int, 32>{}, integral_constant<int, 32>{});
  else if (M <= 40) f(integral_constant<int, 64>{}, integral_constant<int, 40>{});
  else if (M <= 48) f(integral_constant<int, 64>{}, integral_constant<int, 48>{});
  else if (M <= 56) f(integral_constant<int, 64>{}, integral_constant<int, 56>{});
  else f(integral_constant<int, 64>{}, integral_constant<int, 64>{});
}

// The members-in-registers arm that serves M members: NMAX = 8 / 16 / 32 / 64 registers with compile-time indices, or 0 = any M, streamed.
// Calls f(integral_constant<NMAX>), from which the caller launches its kernel<NMAX>.
template <class F>
static inline void ldc_dispatch_member_arm(int M, F&& f) {
  using std::integral_constant;
  if (M <= 8) f(integral_constant<int, 8>{});
  else if (M <= 16) f(integral_constant<int, 16>{});
  else if (M <= 32) f(integral_constant<int, 32>{});
  else if (M <= 64) f(integral_constant<int, 64>{});
  else f(integral_constant<int, 0>{});
}

// A decoded rollout as every rollout entry point reads it: the forecast (M, C, L, H, W) by member / lead / channel strides with a contiguous
// (H, W) plane (the (ens, C, T, H, W) array or the decoder's frame-major (L * ens, C, H, W) output), truth and climatology as tables of
// planes with a slot per lead time, the optional inverse normalisation.  The first member of each kernel's argument struct.
struct RolloutView {
  const float* fc;
  const float* truth;  // nullptr: the entry point has no truth (products)
  const float* clim;   // nullptr: none
  const float* lat_w;  // [H]
  const int* tr_slot;  // [L]
  const int* cl_slot;  // [L]
  const float* mean;   // [C] or nullptr (forecast already in physical units)
  const float* sd;     // [C]
  float target_std;
  long long fc_ms, fc_ls, fc_cs, tr_ss, tr_cs, cl_ss, cl_cs;  // elements
  int M, C, H, W;
};

// Plane (channel c, lead time l): member 0 of the forecast, the truth, the climatology (nullptr without one).
__device__ __forceinline__ const float* view_forecast(const RolloutView& v, int c, int l) {
  return v.fc + static_cast<long long>(l) * v.fc_ls + static_cast<long long>(c) * v.fc_cs;
}
__device__ __forceinline__ const float* view_truth(const RolloutView& v, int c, int l) {
  return v.truth + static_cast<long long>(v.tr_slot[l]) * v.tr_ss + static_cast<long long>(c) * v.tr_cs;
}
__device__ __forceinline__ const float* view_clim(const RolloutView& v, int c, int l) {
  return v.clim ? v.clim + static_cast<long long>(v.cl_slot[l]) * v.cl_ss + static_cast<long long>(c) * v.cl_cs : nullptr;
}
template <bool INV>
__device__ __forceinline__ InvNorm view_norm(const RolloutView& v, int c) {
  if constexpr (INV) return make_inv_norm(v.target_std, v.sd, v.mean, c);
  else return InvNorm{};
}
// Member i of the point f points at (member 0), after the inverse normalisation.
template <bool INV>
__device__ __forceinline__ float load_member(const float* f, int i, long long fc_ms, const InvNorm& nrm) {
  float v = f[static_cast<long long>(i) * fc_ms];
  if constexpr (INV) v = inv_norm(v, nrm);
  return v;
}

// The per-point values of the regional scores and the score maps (regional.hip, score_maps.hip; the formulas in regional.hip's header), every
// one fp32 and formed in one fixed order, so that both kernels hold the same bits: mean sequential in member order, var two-pass, skill,
// spread through the sorted members with one explicit fused multiply-add per step, the anomalies against the climatology and their three
// products.  valid: no member and not the truth is NaN; acc_valid: valid and the climatology is not NaN.  f: member 0 of the point, tp: its
// truth, clp: its climatology or nullptr (fta, ffa, tta are then 0 and acc_valid false).  Contraction is switched off here as in inv_norm.
struct PointValues {
  float e, se, var, skill, spread, fta, ffa, tta;
  bool valid, acc_valid;
};

template <int NP, int NUSE, bool INV>
__device__ __forceinline__ PointValues ensemble_point_values(const float* f, long long fc_ms, const InvNorm& nrm, int M, const float* tp,
                                                             const float* clp) {
#pragma clang fp contract(off)
  const float Mf = static_cast<float>(M);
  float x[NP];
  bool nan_m = false;
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (i < NUSE && i < M) {
      const float v = load_member<INV>(f, i, fc_ms, nrm);
      x[i] = v;
      sum += v;
      nan_m = nan_m || (v != v);
    } else {
      x[i] = INFINITY;  // sorts behind every member
    }
  }
  const float t = *tp;
  float skill = 0.f;
#pragma unroll
  for (int i = 0; i < NUSE; ++i)
    if (i < M) skill += fabsf(t - x[i]);
  skill /= Mf;
  const float mean = sum / Mf;
  float ss = 0.f;
#pragma unroll
  for (int i = 0; i < NUSE; ++i)
    if (i < M) {
      const float d = x[i] - mean;
      ss += d * d;
    }
  float var = 0.f, spread = 0.f;
  if (M >= 2) {
    var = ss / (Mf - 1.0f);
    sort_network<NP, NUSE>(x);
    float ws = 0.f;
#pragma unroll
    for (int i = 0; i < NUSE; ++i)
      if (i < M) ws = fmaf(x[i], 2.0f * static_cast<float>(i + 1) - Mf - 1.0f, ws);
    spread = 2.0f * ws / (Mf * (Mf - 1.0f));
  }
  PointValues r{};
  r.e = mean - t;
  r.se = r.e * r.e;
  r.var = var;
  r.skill = skill;
  r.spread = spread;
  r.valid = !nan_m && t == t;
  if (clp) {
    const float cl = *clp;
    const float fa = mean - cl, ta = t - cl;
    r.fta = fa * ta;
    r.ffa = fa * fa;
    r.tta = ta * ta;
    r.acc_valid = r.valid && cl == cl;
  }
  return r;
}

// Checks and fills the view from the leading C arguments of a rollout entry point, in ABI order, for a forecast written to columns
// l_off .. l_off + L - 1 of L_total: LDC_OK or LDC_ERR_ARG.  Entry points without a climatology pass nullptr, 0, 0, nullptr; with_truth =
// false (products) also waives truth, truth_slot and lat_weight; with_weight = false (score maps: unweighted) waives lat_weight alone.  Pointer checks and limits of its own (LDC_ERR_UNSUPPORTED) stay with each
// entry point, behind this call.
static inline int ldc_rollout_view(RolloutView* v, const float* forecast, long long member_stride, long long lead_stride,
                                   long long channel_stride, const float* mean, const float* std_, float target_std, const float* truth,
                                   long long truth_slot_stride, long long truth_channel_stride, const int* truth_slot, const float* clim,
                                   long long clim_slot_stride, long long clim_channel_stride, const int* clim_slot, const float* lat_weight,
                                   int M, int C, int L, int H, int W, int L_total, int l_off, bool with_truth = true, bool with_weight = true) {
  LDC_CHECK_PTR(forecast);
  if (with_truth) {
    LDC_CHECK_PTR(truth);
    LDC_CHECK_PTR(truth_slot);
    if (with_weight) LDC_CHECK_PTR(lat_weight);
  }
  if (clim != nullptr) LDC_CHECK_PTR(clim_slot);
  if (mean != nullptr && std_ == nullptr) return LDC_ERR_ARG;
  if (M <= 0 || C <= 0 || L <= 0 || H <= 0 || W <= 0 || L_total <= 0 || l_off < 0) return LDC_ERR_ARG;
  if (static_cast<long long>(l_off) + L > L_total) return LDC_ERR_ARG;
  *v = RolloutView{forecast, truth, clim, lat_weight, truth_slot, clim_slot, mean, std_, target_std,
                   member_stride, lead_stride, channel_stride, truth_slot_stride, truth_channel_stride, clim_slot_stride, clim_channel_stride,
                   M, C, H, W};
  return LDC_OK;
}
