// Shared by the ensemble-statistics kernels (scoring.hip, reliability.hip, spectrum.hip, products.hip): the fused inverse normalisation,
// the register sort with its (NP, NUSE) ladder over the ensemble size, and the argument checks of the entry points that address a forecast
// by member / lead / channel strides.
#pragma once
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

// What ldc_rollout_scores, ldc_validation_scores, ldc_rollout_reliability, ldc_rollout_spectrum and ldc_rollout_products ask of a forecast
// (M, C, L, H, W) written to columns l_off .. l_off + L - 1 of L_total, and of its inverse normalisation: LDC_OK or LDC_ERR_ARG.  Pointer
// checks and limits of its own (LDC_ERR_UNSUPPORTED) stay with each entry point.
static inline int ldc_check_forecast_args(int M, int C, int L, int H, int W, int L_total, int l_off, const float* mean, const float* std_) {
  if (mean != nullptr && std_ == nullptr) return LDC_ERR_ARG;
  if (M <= 0 || C <= 0 || L <= 0 || H <= 0 || W <= 0 || L_total <= 0 || l_off < 0) return LDC_ERR_ARG;
  if (static_cast<long long>(l_off) + L > L_total) return LDC_ERR_ARG;
  return LDC_OK;
}
