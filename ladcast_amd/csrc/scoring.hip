// Ensemble scoring of a decoded forecast: CRPS skill / spread / total, ensemble-mean
// latitude-weighted MSE and anomaly correlation, per channel, for one lead time.
//   reference: ladcast/evaluate/utils.py:40-149 (pointwise_crps_skill, pointwise_crps_spread, get_crps, get_acc) and the
//   per-lead-time block of ladcast/evaluate/evaluate_ens_gpu.py:339-425, which runs ~40 torch ops (a sort over the
//   ensemble axis among them) over the (ens, C, H, W) slice = ~15 passes over 0.5 GB at ens = 50.
// Here the slice is read ONCE (HBM-bound: M x C x H x W x 4 bytes): one thread per grid point keeps its M members in
// registers, sorts them with a fully unrolled, pruned odd-even merge network (compile-time register indices), and the workgroup
// reduces the seven weighted sums of its points; a second tiny kernel adds the per-workgroup partials in a fixed
// order (deterministic, no float atomics) and applies the reference's mean / nanmean rules.
//   spread(point) = 2 / (M (M - 1)) * sum_i (2 i - M - 1) x_(i)      (x_(1) <= ... <= x_(M))
//   skill(point)  = mean_i |truth - x_i|,   crps = skill - spread / 2
//   mse = mean_hw[(mean_i x_i - truth)^2 w(lat)],  acc = <fa ta w> / sqrt(<fa^2 w> <ta^2 w>), fa = mean_i x_i - clim
// Points where any member, the truth (or the climatology, for ACC) is NaN are NaN in the reference's maps: channel
// `nan_channel` (SST: NaN over land) averages with nanmean, every other channel with mean (one NaN -> NaN), ACC
// always with nanmean -- reproduced through the valid-point counts.
// Two entry points share the per-point body (score_point) and the per-(channel, lead time) finish (finish_point), so they give the
// same bits: ldc_ensemble_scores (one lead time, optional point maps) and ldc_rollout_scores (every lead time of a decode batch in one
// launch, grid z = lead time: forecast addressed by member / lead / channel strides, optional fused inverse normalisation, truth and
// climatology as tables with a slot per lead time, output columns at an offset; the driver of evaluate_ens_gpu.py:268-425).
// A third, ldc_validation_scores, is the rollout entry point without climatology plus the per-member squared error of the validation
// hook (train_AR.py:281-312): ens_mse = mean_hw[(mean_i x_i - t)^2 w], single_mse = mean_{i,hw}[(x_i - t)^2 w], crps; plain mean everywhere.
#include <math.h>

#include "ensemble_common.h"

namespace {

constexpr int NQ = 8;  // partial sums per workgroup: w*skill, w*spread, w*crps, w*se, w*fa*ta, w*fa^2, w*ta^2 (ACC-valid), counts
constexpr int TPB = 256;
// values per partial record: the 15 sums and counts below; the validation entry point (SINGLE) reduces only what it returns - the
// weighted crps, squared error of the mean and per-member squared error, their three valid-point counts and the point count
constexpr int nrec(bool single) { return single ? 7 : NQ + 7; }

struct ScoreArgs {
  const float* fc;     // [M] x [C] x [HW], strides below (elements)
  const float* truth;  // [C] x [HW]
  const float* clim;   // [C] x [HW] or nullptr
  const float* lat_w;  // [H]
  long long fc_ms, fc_cs, tr_cs, cl_cs;
  int M, C, H, W;
  float* skill_map;   // optional [C][HW]
  float* spread_map;  // optional [C][HW]
  float* part;        // [C][nblk][NQ + 1]
  int nblk;
};

// One grid point of one (channel, lead time): the M member loads, sort, skill / spread / crps / se, the ACC terms, the validity flags
// and the fixed-order workgroup reduction of the 15 partial sums into part_dst[NQ + 7].  f / tp / clp point at this thread's point
// (member 0; clp nullptr = no ACC); skill_dst / spread_dst: this point's map entries or nullptr.  Shared by both entry points, so
// that they give the same bits.  SINGLE (ldc_validation_scores) adds sum_i (x_i - t)^2 / M, taken from the unsorted registers in member
// order; its record is {w*crps, w*se, w*single, their three valid-point counts, points}: each value is computed and reduced exactly as the
// same value without it (every entry of a record goes through the reduction on its own), the entries it does not return are left out.
template <int NP, int NUSE, bool INV, bool SINGLE = false>  // NUSE = members rounded up to a multiple of 8 (<= NP = next power of two)
__device__ __forceinline__ void score_point(const float* f, long long ms, int M, const float* tp, const float* clp, const float* wp,
                                            bool in, float* skill_dst, float* spread_dst, float* part_dst, const InvNorm& nrm) {
  constexpr int NR = nrec(SINGLE);
  __shared__ float red[4][NR];
  float x[NP];
  bool nan_m = false;
  float sum = 0.f;
#pragma unroll
  for (int i = 0; i < NP; ++i) {
    if (i < NUSE && i < M) {
      const float v = load_member<INV>(f, i, ms, nrm);
      x[i] = v;
      sum += v;  // same left-to-right order as torch's mean over dim 0 for small M is not guaranteed; tolerance in tests
      nan_m = nan_m || (v != v);
    } else {
      x[i] = INFINITY;  // sorts behind every member
    }
  }
  const float t = *tp;
  const float w = *wp;
  const float Mf = static_cast<float>(M);
  float skill = 0.f;
#pragma unroll
  for (int i = 0; i < NUSE; ++i)
    if (i < M) skill += fabsf(t - x[i]);
  skill /= Mf;
  float single = 0.f;
  if constexpr (SINGLE) {
#pragma unroll
    for (int i = 0; i < NUSE; ++i)
      if (i < M) {
        const float d = x[i] - t;
        single += d * d;
      }
    single /= Mf;  // M == 1: (x_0 - t)^2 / 1, the bits of se below
  }
  float spread = 0.f;
  if (M >= 2) {
    sort_network<NP, NUSE>(x);
    float ws = 0.f;
#pragma unroll
    for (int i = 0; i < NUSE; ++i)
      if (i < M) ws += x[i] * (2.0f * static_cast<float>(i + 1) - Mf - 1.0f);
    spread = 2.0f * ws / (Mf * (Mf - 1.0f));
  }
  const float nanv = __builtin_nanf("");
  if (nan_m && M >= 2) spread = nanv;  // the sort would have dropped the NaNs; one member: the reference's spread is zeros, NaN or not
  if (in) {
    if (skill_dst) *skill_dst = skill;
    if (spread_dst) *spread_dst = spread;
  }
  const float mean = sum / Mf;
  const float se = (mean - t) * (mean - t);
  const float crps = skill - 0.5f * spread;
  // validity per reduced quantity (NaN propagates through the reference's elementwise ops)
  const bool v_skill = in && skill == skill, v_spread = in && spread == spread, v_crps = in && crps == crps, v_se = in && se == se;
  float fa = 0.f, ta = 0.f;
  bool v_acc = false;
  if (clp) {
    const float cl = *clp;
    fa = mean - cl;
    ta = t - cl;
    // the reference takes three independent nanmeans; a point is dropped from each where that product is NaN
    v_acc = in;
  }
  const float q0 = v_skill ? skill * w : 0.f, q1 = v_spread ? spread * w : 0.f, q2 = v_crps ? crps * w : 0.f, q3 = v_se ? se * w : 0.f;
  const float fta = fa * ta * w, ffa = fa * fa * w, tta = ta * ta * w;
  const bool v4 = v_acc && fta == fta, v5 = v_acc && ffa == ffa, v6 = v_acc && tta == tta;
  // fixed-order workgroup reduction of the 15 (SINGLE: 7) partial sums: lanes by butterfly, then the 4 wave totals in order
  float v[NR];
  if constexpr (SINGLE) {
    const bool v_single = in && single == single;
    v[0] = q2; v[1] = q3; v[2] = v_single ? single * w : 0.f;
    v[3] = v_crps ? 1.f : 0.f; v[4] = v_se ? 1.f : 0.f; v[5] = v_single ? 1.f : 0.f; v[6] = in ? 1.f : 0.f;
  } else {
    v[0] = q0; v[1] = q1; v[2] = q2; v[3] = q3;
    v[4] = v4 ? fta : 0.f; v[5] = v5 ? ffa : 0.f; v[6] = v6 ? tta : 0.f;
    // counts of valid points (exact in fp32 up to 2^24 points)
    v[7] = v_skill ? 1.f : 0.f; v[8] = v_spread ? 1.f : 0.f; v[9] = v_crps ? 1.f : 0.f; v[10] = v_se ? 1.f : 0.f;
    v[11] = v4 ? 1.f : 0.f; v[12] = v5 ? 1.f : 0.f; v[13] = v6 ? 1.f : 0.f; v[14] = in ? 1.f : 0.f;
  }
  const int wave = threadIdx.x >> 6;
#pragma unroll
  for (int i = 0; i < NR; ++i) {
    const float t_ = wave_sum(v[i]);
    if ((threadIdx.x & 63) == 0) red[wave][i] = t_;
  }
  __syncthreads();
  if (threadIdx.x < NR) {
    const int i = threadIdx.x;
    part_dst[i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

template <int NP, int NUSE>
__global__ __launch_bounds__(TPB) void ensemble_scores_kernel(ScoreArgs a) {
  const int c = blockIdx.y;
  const int HW = a.H * a.W;
  const int p = blockIdx.x * TPB + threadIdx.x;
  const bool in = p < HW;
  const int pp = in ? p : 0;
  score_point<NP, NUSE, false>(a.fc + static_cast<long long>(c) * a.fc_cs + pp, a.fc_ms, a.M, a.truth + static_cast<long long>(c) * a.tr_cs + pp,
                               a.clim ? a.clim + static_cast<long long>(c) * a.cl_cs + pp : nullptr, a.lat_w + pp / a.W, in,
                               a.skill_map ? a.skill_map + static_cast<long long>(c) * HW + p : nullptr,
                               a.spread_map ? a.spread_map + static_cast<long long>(c) * HW + p : nullptr,
                               a.part + (static_cast<long long>(c) * a.nblk + blockIdx.x) * (NQ + 7), InvNorm{});
}

// Every lead time of a decode batch in one launch: grid (nblk, C, L).  The forecast, truth and climatology (nullptr = no ACC) are addressed
// through the RolloutView; the optional inverse normalisation is applied to every forecast value as it is loaded.
struct RolloutArgs {
  RolloutView v;
  float* part;  // [L][C][nblk][nrec(SINGLE)]
  int nblk;
};

template <int NP, int NUSE, bool INV, bool SINGLE>
__global__ __launch_bounds__(TPB) void rollout_scores_kernel(RolloutArgs a) {
  const int c = blockIdx.y, l = blockIdx.z;
  const int HW = a.v.H * a.v.W;
  const int p = blockIdx.x * TPB + threadIdx.x;
  const bool in = p < HW;
  const int pp = in ? p : 0;
  const float* clp = view_clim(a.v, c, l);
  score_point<NP, NUSE, INV, SINGLE>(view_forecast(a.v, c, l) + pp, a.v.fc_ms, a.v.M, view_truth(a.v, c, l) + pp, clp ? clp + pp : nullptr,
                                     a.v.lat_w + pp / a.v.W, in, nullptr, nullptr,
                                     a.part + ((static_cast<long long>(l) * a.v.C + c) * a.nblk + blockIdx.x) * nrec(SINGLE),
                                     view_norm<INV>(a.v, c));
}

// The five scores of one (channel, lead time) from its nblk partial records.  One wave: lane j adds the partial records
// j, j + 64, ... in order, then a fixed butterfly (deterministic); lane 0 holds the result.  dst[k * dst_stride], k < 5 =
// acc, mse, crps_spread, crps_skill, crps.  SINGLE: records of 7 (score_point), dst[k * dst_stride], k < 3 = ens_mse, single_mse, crps (no
// nanmean, no ACC); ens_mse and crps are formed from the same sums in the same order as without it.
template <bool SINGLE = false>
__device__ __forceinline__ void finish_point(const float* __restrict__ part, int nblk, bool nanmean, int has_clim, float* __restrict__ dst,
                                             long long dst_stride) {
  constexpr int NR = nrec(SINGLE);
  float s[NR];
#pragma unroll
  for (int i = 0; i < NR; ++i) s[i] = 0.f;
  for (int b = threadIdx.x; b < nblk; b += 64) {
    const float* src = part + static_cast<long long>(b) * NR;
#pragma unroll
    for (int i = 0; i < NR; ++i) s[i] += src[i];
  }
#pragma unroll
  for (int i = 0; i < NR; ++i) s[i] = wave_sum(s[i]);
  if (threadIdx.x != 0) return;
  const float nanv = __builtin_nanf("");
  const float total = s[NR - 1];
  // mean: any NaN point -> NaN; nanmean: average over the valid points (all invalid -> NaN, as torch.nanmean)
  auto avg = [&](float sum, float cnt) {
    if (nanmean) return cnt > 0.f ? sum / cnt : nanv;
    return cnt == total ? sum / total : nanv;
  };
  if constexpr (SINGLE) {
    dst[0 * dst_stride] = avg(s[1], s[4]);
    dst[1 * dst_stride] = avg(s[2], s[5]);
    dst[2 * dst_stride] = avg(s[0], s[3]);
  } else {
    const float skill = avg(s[0], s[7]), spread = avg(s[1], s[8]), crps = avg(s[2], s[9]), mse = avg(s[3], s[10]);
    float acc = nanv;
    if (has_clim) {
      const float n4 = s[11] > 0.f ? s[4] / s[11] : nanv, n5 = s[12] > 0.f ? s[5] / s[12] : nanv, n6 = s[13] > 0.f ? s[6] / s[13] : nanv;
      acc = n4 / sqrtf(n5 * n6);
    }
    dst[0 * dst_stride] = acc;
    dst[1 * dst_stride] = mse;
    dst[2 * dst_stride] = spread;
    dst[3 * dst_stride] = skill;
    dst[4 * dst_stride] = crps;
  }
}

// out: [5][C] = acc, mse, crps_spread, crps_skill, crps.  One wave per channel.
__global__ __launch_bounds__(64) void ensemble_scores_finish_kernel(const float* __restrict__ part, int nblk, int C, int nan_channel,
                                                                    int has_clim, float* __restrict__ out) {
  const int c = blockIdx.x;
  finish_point(part + static_cast<long long>(c) * nblk * (NQ + 7), nblk, c == nan_channel, has_clim, out + c, C);
}

// out: [5][C][L_total], columns l_off .. l_off + L - 1.  One wave per (channel, lead time): grid (C, L).
__global__ __launch_bounds__(64) void rollout_scores_finish_kernel(const float* __restrict__ part, int nblk, int C, int nan_channel,
                                                                   int has_clim, float* __restrict__ out, int L_total, int l_off) {
  const int c = blockIdx.x, l = blockIdx.y;
  finish_point(part + (static_cast<long long>(l) * C + c) * nblk * (NQ + 7), nblk, c == nan_channel, has_clim,
               out + static_cast<long long>(c) * L_total + l_off + l, static_cast<long long>(C) * L_total);
}

// out: [3][C][L_total] = ens_mse, single_mse, crps, columns l_off .. l_off + L - 1.  One wave per (channel, lead time): grid (C, L).
__global__ __launch_bounds__(64) void validation_scores_finish_kernel(const float* __restrict__ part, int nblk, int C, float* __restrict__ out,
                                                                      int L_total, int l_off) {
  const int c = blockIdx.x, l = blockIdx.y;
  finish_point<true>(part + (static_cast<long long>(l) * C + c) * nblk * nrec(true), nblk, false, 0,
                     out + static_cast<long long>(c) * L_total + l_off + l, static_cast<long long>(C) * L_total);
}

}  // namespace

extern "C" long long ldc_ensemble_scores_workspace_bytes(int C, int H, int W) {
  if (C <= 0 || H <= 0 || W <= 0) return 0;
  return static_cast<long long>(C) * ldc_cdiv(static_cast<long long>(H) * W, TPB) * (NQ + 7) * static_cast<long long>(sizeof(float));
}

extern "C" int ldc_ensemble_scores(const float* forecast, long long member_stride, long long channel_stride, const float* truth,
                                   long long truth_channel_stride, const float* clim, long long clim_channel_stride,
                                   const float* lat_weight, int M, int C, int H, int W, int nan_channel, float* out,
                                   float* skill_map, float* spread_map, void* workspace, long long workspace_bytes,
                                   void* stream) {
  LDC_CHECK_PTR(forecast);
  LDC_CHECK_PTR(truth);
  LDC_CHECK_PTR(lat_weight);
  LDC_CHECK_PTR(out);
  LDC_CHECK_PTR(workspace);
  if (M <= 0 || C <= 0 || H <= 0 || W <= 0) return LDC_ERR_ARG;
  if (M > 64 || C > 65535) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < ldc_ensemble_scores_workspace_bytes(C, H, W)) return LDC_ERR_ARG;
  ScoreArgs a{};
  a.fc = forecast;
  a.truth = truth;
  a.clim = clim;
  a.lat_w = lat_weight;
  a.fc_ms = member_stride;
  a.fc_cs = channel_stride;
  a.tr_cs = truth_channel_stride;
  a.cl_cs = clim_channel_stride;
  a.M = M; a.C = C; a.H = H; a.W = W;
  a.skill_map = skill_map;
  a.spread_map = spread_map;
  a.part = static_cast<float*>(workspace);
  a.nblk = static_cast<int>(ldc_cdiv(static_cast<long long>(H) * W, TPB));
  dim3 grid(a.nblk, C);
  hipStream_t s = static_cast<hipStream_t>(stream);
  ldc_dispatch_sort_arm(M, [&](auto np, auto nuse) {
    hipLaunchKernelGGL((ensemble_scores_kernel<decltype(np)::value, decltype(nuse)::value>), grid, dim3(TPB), 0, s, a);
  });
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(ensemble_scores_finish_kernel, dim3(C), dim3(64), 0, s, a.part, a.nblk, C, nan_channel,
                     clim != nullptr ? 1 : 0, out);
  return ldc_launch_status();
}

extern "C" long long ldc_rollout_scores_workspace_bytes(int C, int L, int H, int W) {
  if (C <= 0 || L <= 0 || H <= 0 || W <= 0) return 0;
  return static_cast<long long>(L) * ldc_ensemble_scores_workspace_bytes(C, H, W);
}

namespace {
template <bool INV, bool SINGLE = false>
void launch_rollout(const RolloutArgs& a, dim3 grid, hipStream_t s) {
  ldc_dispatch_sort_arm(a.v.M, [&](auto np, auto nuse) {
    hipLaunchKernelGGL((rollout_scores_kernel<decltype(np)::value, decltype(nuse)::value, INV, SINGLE>), grid, dim3(TPB), 0, s, a);
  });
}
}  // namespace

extern "C" int ldc_rollout_scores(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                  const float* mean, const float* std_, float target_std, const float* truth,
                                  long long truth_slot_stride, long long truth_channel_stride, const int* truth_slot, const float* clim,
                                  long long clim_slot_stride, long long clim_channel_stride, const int* clim_slot,
                                  const float* lat_weight, int M, int C, int L, int H, int W, int nan_channel, float* out, int L_total,
                                  int l_off, void* workspace, long long workspace_bytes, void* stream) {
  RolloutArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, clim, clim_slot_stride, clim_channel_stride, clim_slot, lat_weight, M, C, L, H, W,
                       L_total, l_off) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(out);
  LDC_CHECK_PTR(workspace);
  if (M > 64 || C > 65535 || L > 65535) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < ldc_rollout_scores_workspace_bytes(C, L, H, W)) return LDC_ERR_ARG;
  a.part = static_cast<float*>(workspace);
  a.nblk = static_cast<int>(ldc_cdiv(static_cast<long long>(H) * W, TPB));
  dim3 grid(a.nblk, C, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) launch_rollout<true>(a, grid, s);
  else launch_rollout<false>(a, grid, s);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(rollout_scores_finish_kernel, dim3(C, L), dim3(64), 0, s, a.part, a.nblk, C, nan_channel, clim != nullptr ? 1 : 0,
                     out, L_total, l_off);
  return ldc_launch_status();
}

// The validation hook's three scores (ladcast/train_AR.py:281-312): ldc_rollout_scores without a climatology and without a nanmean
// channel, plus the per-member squared error.
extern "C" long long ldc_validation_scores_workspace_bytes(int C, int L, int H, int W) {
  if (C <= 0 || L <= 0 || H <= 0 || W <= 0) return 0;
  return static_cast<long long>(L) * C * ldc_cdiv(static_cast<long long>(H) * W, TPB) * nrec(true) * static_cast<long long>(sizeof(float));
}

extern "C" int ldc_validation_scores(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                     const float* mean, const float* std_, float target_std, const float* truth,
                                     long long truth_slot_stride, long long truth_channel_stride, const int* truth_slot,
                                     const float* lat_weight, int M, int C, int L, int H, int W, float* out, int L_total, int l_off,
                                     void* workspace, long long workspace_bytes, void* stream) {
  RolloutArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, nullptr, 0, 0, nullptr, lat_weight, M, C, L, H, W, L_total, l_off) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(out);
  LDC_CHECK_PTR(workspace);
  if (M > 64 || C > 65535 || L > 65535) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < ldc_validation_scores_workspace_bytes(C, L, H, W)) return LDC_ERR_ARG;
  a.part = static_cast<float*>(workspace);
  a.nblk = static_cast<int>(ldc_cdiv(static_cast<long long>(H) * W, TPB));
  dim3 grid(a.nblk, C, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) launch_rollout<true, true>(a, grid, s);
  else launch_rollout<false, true>(a, grid, s);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(validation_scores_finish_kernel, dim3(C, L), dim3(64), 0, s, a.part, a.nblk, C, out, L_total, l_off);
  return ldc_launch_status();
}
