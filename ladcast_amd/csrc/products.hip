// Ensemble products of a decoded forecast: per grid point the ensemble mean, spread, range, quantile maps and
// probabilities of exceeding a threshold - what an ensemble forecast is consumed as, for a forecast that has no truth yet.  Not in the
// reference.  The forecast is addressed as ldc_rollout_scores (scoring.hip) addresses it: member / lead / channel strides, a contiguous
// (H, W) plane, the optional fused inverse normalisation (inv_norm, ensemble_common.h); grid (point blocks, selected channel, lead time),
// output columns at l_off.
// Pointwise: one thread per grid point, consecutive threads along W (coalesced loads and stores), no workspace, no reduction.
// Per point, M members x_i in member order (after the inverse normalisation):
//   mean = (x_0 + ... + x_{M-1}) / M                       sequential fp32 sum
//   std  = sqrt(sum_i (x_i - mean)^2 / (M - 1))            two-pass, member order; M == 1: sqrt(0 / 0) = NaN (ddof = 1, as reliability.hip)
//   min, max
//   quantile (lo, t): x_(lo) when t == 0, else a + (b - a) * t with a = x_(lo), b = x_(min(lo + 1, M - 1)) - numpy's method="linear";
//     (lo, t) come from the host (float64 arithmetic on q (M - 1)); three fp32 operations, the file is built with -ffp-contract=off
//   exceed (thr, dir): #{x_i > thr} / M (dir +1) or #{x_i < thr} / M (dir -1); a NaN threshold gives NaN
// A point with a NaN member is NaN in every output; +-inf are ordinary ordered values.
// Two arms.  With quantiles the members live in registers and are sorted by the pruned odd-even merge network of ensemble_common.h (M <= 64,
// the same (NP, NUSE) ladder); a and b are picked by an unrolled compare-and-select over the registers, because a runtime index would
// send the array to scratch.  Without quantiles nothing is sorted: the streaming arm serves 1 <= M <= 1024 and reads the members a
// second time for the squared deviations.
#include <math.h>

#include "ensemble_common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_M = 1024;
constexpr int MAX_SORT_M = 64;
constexpr int MAX_Q = LDC_PRODUCTS_MAX_QUANTILES;
constexpr int MAX_P = LDC_PRODUCTS_MAX_THRESHOLDS;

struct ProdArgs {
  RolloutView v;     // the forecast only: no truth, no climatology
  const int* chan;   // [Cs] or nullptr (all channels, in order)
  const float* thr;  // [P][Cs]
  float* stats;      // [4][Cs][L_total][HW] or nullptr
  float* quant;      // [Q][Cs][L_total][HW] or nullptr
  float* exceed;     // [P][Cs][L_total][HW] or nullptr
  int Cs, HW, L_total, l_off;
  int Q, P;  // 0 when the output is not asked for
  ldc_products_desc d;
};

// what the first pass over the members gathers, in member order
struct Pass1 {
  float sum, mn, mx;
  bool nan_m;
  int cnt[MAX_P];
};

__device__ __forceinline__ void pass1_init(Pass1& s) {
  s.sum = 0.f;
  s.mn = INFINITY;
  s.mx = -INFINITY;
  s.nan_m = false;
#pragma unroll
  for (int k = 0; k < MAX_P; ++k) s.cnt[k] = 0;
}

__device__ __forceinline__ void pass1_add(Pass1& s, float v, const float (&thr)[MAX_P], unsigned gt_mask, int P) {
  s.sum += v;
  s.mn = fminf(s.mn, v);
  s.mx = fmaxf(s.mx, v);
  s.nan_m = s.nan_m || (v != v);
#pragma unroll
  for (int k = 0; k < MAX_P; ++k)
    if (k < P) s.cnt[k] += (((gt_mask >> k) & 1u) ? v > thr[k] : v < thr[k]) ? 1 : 0;
}

// NP > 0: M <= NUSE members in registers, sorted for the quantiles; NP == 0: any M, no quantiles, the members are read again for std
template <int NP, int NUSE, bool INV>
__global__ __launch_bounds__(TPB) void products_kernel(ProdArgs a) {
  const int p = blockIdx.x * TPB + threadIdx.x;
  if (p >= a.HW) return;  // no barrier below
  const int cs = blockIdx.y, l = blockIdx.z;
  const int c = a.chan != nullptr ? a.chan[cs] : cs;
  const int M = a.v.M, P = a.P;
  const float* f = view_forecast(a.v, c, l) + p;
  const InvNorm nrm = view_norm<INV>(a.v, c);
  float thr[MAX_P];
  unsigned gt_mask = 0u;
#pragma unroll
  for (int k = 0; k < MAX_P; ++k) {
    thr[k] = k < P ? a.thr[static_cast<long long>(k) * a.Cs + cs] : 0.f;
    if (k < P && a.d.thr_dir[k] > 0) gt_mask |= 1u << k;
  }
  const float Mf = static_cast<float>(M);
  const float nanv = __builtin_nanf("");
  const long long plane = static_cast<long long>(a.L_total) * a.HW;  // one channel of one output
  const long long at = (static_cast<long long>(cs) * a.L_total + a.l_off + l) * a.HW + p;
  const long long kstep = static_cast<long long>(a.Cs) * plane;  // one plane of stats / quant / exceed
  Pass1 s;
  pass1_init(s);
  float ss = 0.f, mean;
  if constexpr (NP > 0) {
    float x[NP];
#pragma unroll
    for (int i = 0; i < NP; ++i) {
      if (i < NUSE && i < M) {
        const float v = load_member<INV>(f, i, a.v.fc_ms, nrm);
        x[i] = v;
        pass1_add(s, v, thr, gt_mask, P);
      } else {
        x[i] = INFINITY;  // sorts behind every member
      }
    }
    mean = s.sum / Mf;
    if (a.stats != nullptr) {
#pragma unroll
      for (int i = 0; i < NUSE; ++i)
        if (i < M) {
          const float e = x[i] - mean;
          ss += e * e;
        }
    }
    if (a.Q > 0) {
      sort_network<NP, NUSE>(x);
      for (int q = 0; q < a.Q; ++q) {
        const int lo = a.d.q_lo[q];
        const int hi = min(lo + 1, M - 1);
        const float t = a.d.q_t[q];
        float va = x[0], vb = x[0];
#pragma unroll
        for (int i = 1; i < NUSE; ++i) {  // compile-time register indices: a runtime x[lo] would put x into scratch
          va = i == lo ? x[i] : va;
          vb = i == hi ? x[i] : vb;
        }
        const float d = vb - va;
        const float r = t == 0.f ? va : va + d * t;
        a.quant[q * kstep + at] = s.nan_m ? nanv : r;
      }
    }
  } else {
    for (int i = 0; i < M; ++i) pass1_add(s, load_member<INV>(f, i, a.v.fc_ms, nrm), thr, gt_mask, P);
    mean = s.sum / Mf;
    if (a.stats != nullptr) {
      for (int i = 0; i < M; ++i) {
        const float e = load_member<INV>(f, i, a.v.fc_ms, nrm) - mean;
        ss += e * e;
      }
    }
  }
  if (a.stats != nullptr) {
    const float sd = sqrtf(ss / (Mf - 1.0f));  // one member: sqrt(0 / 0)
    a.stats[at] = s.nan_m ? nanv : mean;
    a.stats[kstep + at] = s.nan_m ? nanv : sd;
    a.stats[2 * kstep + at] = s.nan_m ? nanv : s.mn;
    a.stats[3 * kstep + at] = s.nan_m ? nanv : s.mx;
  }
#pragma unroll
  for (int k = 0; k < MAX_P; ++k)
    if (k < P) {
      const float pr = static_cast<float>(s.cnt[k]) / Mf;
      a.exceed[k * kstep + at] = (s.nan_m || thr[k] != thr[k]) ? nanv : pr;
    }
}

template <bool INV>
void launch_products(const ProdArgs& a, dim3 grid, hipStream_t s) {
  if (a.Q == 0) hipLaunchKernelGGL((products_kernel<0, 0, INV>), grid, dim3(TPB), 0, s, a);
  else
    ldc_dispatch_sort_arm(a.v.M, [&](auto np, auto nuse) {
      hipLaunchKernelGGL((products_kernel<decltype(np)::value, decltype(nuse)::value, INV>), grid, dim3(TPB), 0, s, a);
    });
}

}  // namespace

extern "C" int ldc_sizeof_products_desc(void) { return static_cast<int>(sizeof(ldc_products_desc)); }

extern "C" int ldc_rollout_products(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                    const float* mean, const float* std_, float target_std, const int* channels, int M, int C, int Cs, int L,
                                    int H, int W, const ldc_products_desc* desc, const float* thr, float* stats, float* quant, float* exceed,
                                    int L_total, int l_off, void* stream) {
  ProdArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, nullptr, 0, 0, nullptr, nullptr, 0,
                       0, nullptr, nullptr, M, C, L, H, W, L_total, l_off, /*with_truth=*/false) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(desc);
  if (Cs <= 0 || (channels == nullptr && Cs != C)) return LDC_ERR_ARG;
  if (desc->n_quant < 0 || desc->n_quant > MAX_Q || desc->n_thr < 0 || desc->n_thr > MAX_P) return LDC_ERR_ARG;
  const int Q = quant != nullptr ? desc->n_quant : 0;
  const int P = exceed != nullptr ? desc->n_thr : 0;
  if (stats == nullptr && Q == 0 && P == 0) return LDC_ERR_ARG;  // nothing to compute
  if (P > 0) LDC_CHECK_PTR(thr);
  for (int q = 0; q < Q; ++q) {
    const float t = desc->q_t[q];
    if (desc->q_lo[q] < 0 || desc->q_lo[q] > M - 1 || !(t >= 0.f && t <= 1.f)) return LDC_ERR_ARG;
  }
  for (int k = 0; k < P; ++k)
    if (desc->thr_dir[k] != 1 && desc->thr_dir[k] != -1) return LDC_ERR_ARG;
  if (M > MAX_M || Cs > 65535 || L > 65535 || static_cast<long long>(H) * W > (1ll << 24)) return LDC_ERR_UNSUPPORTED;
  if (Q > 0 && M > MAX_SORT_M) return LDC_ERR_UNSUPPORTED;
  a.chan = channels;
  a.thr = thr;
  a.stats = stats;
  a.quant = quant;
  a.exceed = exceed;
  a.Cs = Cs; a.HW = H * W; a.L_total = L_total; a.l_off = l_off;
  a.Q = Q; a.P = P;
  a.d = *desc;
  dim3 grid(ldc_cdiv(a.HW, TPB), Cs, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) launch_products<true>(a, grid, s);
  else launch_products<false>(a, grid, s);
  return ldc_launch_status();
}
