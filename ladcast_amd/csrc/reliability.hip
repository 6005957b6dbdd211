// Ensemble reliability of a decoded forecast: spread-skill ratio and rank histogram per (channel, lead time).
// Not in the reference (ladcast/evaluate/utils.py stops at CRPS and ACC); the pair WeatherBench2 reports beside CRPS.
// Addressing is that of ldc_rollout_scores (scoring.hip): forecast by member / lead / channel strides, optional fused inverse
// normalisation (inv_norm, ensemble_common.h), truth as a table of planes with a slot per lead time, lat_weight[H], grid (point blocks,
// C, L), output columns at l_off.
// Per grid point, M members x_i in member order, truth t, weight w:
//   mean = (x_0 + ... + x_{M-1}) / M          (the sum of score_point, scoring.hip: ens_mse holds ldc_rollout_scores' bits for M <= 64)
//   se   = (mean - t)^2
//   var  = sum_i (x_i - mean)^2 / (M - 1)     two-pass, fp32 terms in member order; M == 1: 0 / 0 = NaN (ddof = 1)
//   lt = #{x_i < t}, eq = #{x_i == t}, rank bin = lt + (eq >> 1) in 0 .. M: ties take the deterministic mid-rank
//   the point counts in the histogram when no member and not the truth is NaN; +-inf are ordinary ordered values
// No sort, so no 64-member limit: M <= 64 keeps the members in registers (compile-time indices), 64 < M <= 1024 reads them a second
// time for the variance.  The whole file is built with -ffp-contract=off: every product and sum is rounded on its own.
// Reduction without float atomics, in a fixed order.  A workgroup covers `tpw` consecutive tiles of 256 points:
//   sums / counts: per thread over its tiles in order, lanes by butterfly, the 4 wave totals pairwise (one tile: score_point's order)
//   histogram: every thread publishes (bin, w) of its point to LDS (bin -1: not valid); thread b <= M walks the tile's 256 points in
//     index order (every lane reads the same address: an LDS broadcast, no bank conflict; b128 reads, 4 points each) and keeps the
//     count and the weight sum of bin b in registers across the tiles: one sequential sum over the workgroup's points
//   finish launch, one workgroup per (channel, lead time): sums as finish_point (lane j adds records j, j + 64, ... then a butterfly),
//     bin b adds the records' entries in record order.
#include <math.h>

#include "ensemble_common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_M = 1024;
constexpr int HEAD = 8;  // words in front of a record's bins: sum w*se, sum w*var (fp32); counts of valid se, valid var, points, invalid (int32); 2 pad
constexpr int KB_MAX = (MAX_M + 1 + TPB - 1) / TPB;  // bins per thread of the streaming kernel

// tiles per workgroup: the record grows with M (2 (M + 1) + HEAD words), so the tiles per record grow with it and the workspace stays level
constexpr int tiles_per_wg(int M) { return M <= 64 ? 1 : (M + 63) / 64; }
constexpr int rec_words(int M) { return HEAD + 2 * (M + 1); }

struct RelArgs {
  RolloutView v;   // no climatology
  unsigned* part;  // [L][C][nrec][rec_words(M)]
  int ntile, tpw, nrec;
};

// NMAX > 0: M <= NMAX members in registers; NMAX == 0: any M, the members are read again for the variance
template <int NMAX, bool INV>
__global__ __launch_bounds__(TPB) void reliability_kernel(RelArgs a) {
  constexpr int KB = NMAX > 0 ? 1 : KB_MAX;
  constexpr int NX = NMAX > 0 ? NMAX : 1;
  __shared__ __attribute__((aligned(16))) int s_bin[TPB];
  __shared__ __attribute__((aligned(16))) float s_w[TPB];
  __shared__ float red_f[4][2];
  __shared__ int red_i[4][4];
  const int c = blockIdx.y, l = blockIdx.z;
  const int M = a.v.M;
  const int HW = a.v.H * a.v.W;
  const int tid = threadIdx.x;
  const float* fbase = view_forecast(a.v, c, l);
  const float* tbase = view_truth(a.v, c, l);
  const InvNorm nrm = view_norm<INV>(a.v, c);
  const float Mf = static_cast<float>(M);
  float acc_se = 0.f, acc_var = 0.f;
  int n_se = 0, n_var = 0, n_in = 0, n_inv = 0;
  int hc[KB];
  float hw[KB];
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    hc[k] = 0;
    hw[k] = 0.f;
  }
  const int tile0 = blockIdx.x * a.tpw;
  const int tile1 = min(tile0 + a.tpw, a.ntile);
  for (int tile = tile0; tile < tile1; ++tile) {
    const int p = tile * TPB + tid;
    const bool in = p < HW;
    const int pp = in ? p : 0;
    const float* f = fbase + pp;
    const float t = tbase[pp];
    const float w = a.v.lat_w[pp / a.v.W];
    float sum = 0.f, ss = 0.f;
    int lt = 0, eq = 0;
    bool nan_m = false;
    float mean;
    if constexpr (NMAX > 0) {
      float x[NX];
#pragma unroll
      for (int i = 0; i < NX; ++i) {
        if (i < M) {
          const float v = load_member<INV>(f, i, a.v.fc_ms, nrm);
          x[i] = v;
          sum += v;
          nan_m = nan_m || (v != v);
          lt += v < t ? 1 : 0;
          eq += v == t ? 1 : 0;
        } else {
          x[i] = 0.f;
        }
      }
      mean = sum / Mf;
#pragma unroll
      for (int i = 0; i < NX; ++i)
        if (i < M) {
          const float e = x[i] - mean;
          ss += e * e;
        }
    } else {
      for (int i = 0; i < M; ++i) {
        const float v = load_member<INV>(f, i, a.v.fc_ms, nrm);
        sum += v;
        nan_m = nan_m || (v != v);
        lt += v < t ? 1 : 0;
        eq += v == t ? 1 : 0;
      }
      mean = sum / Mf;
      for (int i = 0; i < M; ++i) {
        const float e = load_member<INV>(f, i, a.v.fc_ms, nrm) - mean;
        ss += e * e;
      }
    }
    const float d = mean - t;
    const float se = d * d;
    const float var = ss / (Mf - 1.0f);  // one member: 0 / 0
    const bool v_se = in && se == se, v_var = in && var == var;
    const bool v_hist = in && !nan_m && t == t;
    acc_se += v_se ? se * w : 0.f;
    acc_var += v_var ? var * w : 0.f;
    n_se += v_se ? 1 : 0;
    n_var += v_var ? 1 : 0;
    n_in += in ? 1 : 0;
    n_inv += (in && !v_hist) ? 1 : 0;
    __syncthreads();  // the walk of the tile before is over
    s_bin[tid] = v_hist ? lt + (eq >> 1) : -1;
    s_w[tid] = w;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KB; ++k) {
      const int b = tid + k * TPB;
      if (b <= M) {
        int cnt = hc[k];
        float ws = hw[k];
#pragma unroll 4
        for (int q = 0; q < TPB; q += 4) {
          const int4 bb = *reinterpret_cast<const int4*>(&s_bin[q]);
          const float4 ww = *reinterpret_cast<const float4*>(&s_w[q]);
          cnt += bb.x == b ? 1 : 0;
          ws += bb.x == b ? ww.x : 0.f;
          cnt += bb.y == b ? 1 : 0;
          ws += bb.y == b ? ww.y : 0.f;
          cnt += bb.z == b ? 1 : 0;
          ws += bb.z == b ? ww.z : 0.f;
          cnt += bb.w == b ? 1 : 0;
          ws += bb.w == b ? ww.w : 0.f;
        }
        hc[k] = cnt;
        hw[k] = ws;
      }
    }
  }
  unsigned* rec = a.part + ((static_cast<long long>(l) * a.v.C + c) * a.nrec + blockIdx.x) * rec_words(M);
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int b = tid + k * TPB;
    if (b <= M) {
      rec[HEAD + b] = static_cast<unsigned>(hc[k]);
      rec[HEAD + M + 1 + b] = __float_as_uint(hw[k]);
    }
  }
  const int wave = tid >> 6;
  const float r_se = wave_sum(acc_se), r_var = wave_sum(acc_var);
  const int i_se = wave_sum(n_se), i_var = wave_sum(n_var), i_in = wave_sum(n_in), i_inv = wave_sum(n_inv);
  if ((tid & 63) == 0) {
    red_f[wave][0] = r_se;
    red_f[wave][1] = r_var;
    red_i[wave][0] = i_se;
    red_i[wave][1] = i_var;
    red_i[wave][2] = i_in;
    red_i[wave][3] = i_inv;
  }
  __syncthreads();
  if (tid < 2) rec[tid] = __float_as_uint((red_f[0][tid] + red_f[1][tid]) + (red_f[2][tid] + red_f[3][tid]));
  else if (tid < 6) rec[tid] = static_cast<unsigned>((red_i[0][tid - 2] + red_i[1][tid - 2]) + (red_i[2][tid - 2] + red_i[3][tid - 2]));
  else if (tid < HEAD) rec[tid] = 0u;
}

// One workgroup per (channel, lead time): grid (C, L).  out [3][C][L_total] = ens_mse, ens_var, ssr; hist_count / hist_weight
// [C][L_total][M + 1]; n_invalid [C][L_total]; columns l_off .. l_off + L - 1.
__global__ __launch_bounds__(TPB) void reliability_finish_kernel(const unsigned* __restrict__ part, int nrec, int M, int C, int nan_channel,
                                                                 float* __restrict__ out, int* __restrict__ hist_count,
                                                                 float* __restrict__ hist_weight, int* __restrict__ n_invalid, int L_total,
                                                                 int l_off) {
  const int c = blockIdx.x, l = blockIdx.y;
  const int RW = rec_words(M);
  const unsigned* base = part + (static_cast<long long>(l) * C + c) * nrec * RW;
  const long long col = static_cast<long long>(c) * L_total + l_off + l;
  for (int b = threadIdx.x; b <= M; b += TPB) {
    int cnt = 0;
    float ws = 0.f;
    for (int r = 0; r < nrec; ++r) {
      const unsigned* src = base + static_cast<long long>(r) * RW + HEAD;
      cnt += static_cast<int>(src[b]);
      ws += __uint_as_float(src[M + 1 + b]);
    }
    hist_count[col * (M + 1) + b] = cnt;
    hist_weight[col * (M + 1) + b] = ws;
  }
  if (threadIdx.x >= 64) return;
  float s_se = 0.f, s_var = 0.f;
  int k_se = 0, k_var = 0, k_in = 0, k_inv = 0;
  for (int r = threadIdx.x; r < nrec; r += 64) {
    const unsigned* src = base + static_cast<long long>(r) * RW;
    s_se += __uint_as_float(src[0]);
    s_var += __uint_as_float(src[1]);
    k_se += static_cast<int>(src[2]);
    k_var += static_cast<int>(src[3]);
    k_in += static_cast<int>(src[4]);
    k_inv += static_cast<int>(src[5]);
  }
  s_se = wave_sum(s_se);
  s_var = wave_sum(s_var);
  k_se = wave_sum(k_se);
  k_var = wave_sum(k_var);
  k_in = wave_sum(k_in);
  k_inv = wave_sum(k_inv);
  if (threadIdx.x != 0) return;
  const float nanv = __builtin_nanf("");
  const bool nanmean = c == nan_channel;
  // mean: any NaN point -> NaN; nanmean: average over the valid points (none -> NaN); the counts are exact in fp32 (H * W <= 2^24)
  auto avg = [&](float sum, int cnt) {
    if (nanmean) return cnt > 0 ? sum / static_cast<float>(cnt) : nanv;
    return cnt == k_in ? sum / static_cast<float>(k_in) : nanv;
  };
  const float mse = avg(s_se, k_se), var = avg(s_var, k_var);
  const float Mf = static_cast<float>(M);
  const long long plane = static_cast<long long>(C) * L_total;
  out[col] = mse;
  out[plane + col] = var;
  out[2 * plane + col] = sqrtf((Mf + 1.0f) / Mf) * sqrtf(var / mse);
  n_invalid[col] = k_inv;
}

template <bool INV>
void launch_reliability(const RelArgs& a, dim3 grid, hipStream_t s) {
  ldc_dispatch_member_arm(a.v.M, [&](auto nmax) {
    hipLaunchKernelGGL((reliability_kernel<decltype(nmax)::value, INV>), grid, dim3(TPB), 0, s, a);
  });
}

}  // namespace

extern "C" long long ldc_rollout_reliability_workspace_bytes(int M, int C, int L, int H, int W) {
  if (M <= 0 || M > MAX_M || C <= 0 || L <= 0 || H <= 0 || W <= 0) return 0;
  const long long ntile = (static_cast<long long>(H) * W + TPB - 1) / TPB;
  const long long nrec = (ntile + tiles_per_wg(M) - 1) / tiles_per_wg(M);
  return static_cast<long long>(L) * C * nrec * rec_words(M) * static_cast<long long>(sizeof(unsigned));
}

extern "C" int ldc_rollout_reliability(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                       const float* mean, const float* std_, float target_std, const float* truth,
                                       long long truth_slot_stride, long long truth_channel_stride, const int* truth_slot,
                                       const float* lat_weight, int M, int C, int L, int H, int W, int nan_channel, float* out,
                                       int* hist_count, float* hist_weight, int* n_invalid, int L_total, int l_off, void* workspace,
                                       long long workspace_bytes, void* stream) {
  RelArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, nullptr, 0, 0, nullptr, lat_weight, M, C, L, H, W, L_total, l_off) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(out);
  LDC_CHECK_PTR(hist_count);
  LDC_CHECK_PTR(hist_weight);
  LDC_CHECK_PTR(n_invalid);
  LDC_CHECK_PTR(workspace);
  if (M > MAX_M || C > 65535 || L > 65535 || static_cast<long long>(H) * W > (1ll << 24)) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < ldc_rollout_reliability_workspace_bytes(M, C, L, H, W)) return LDC_ERR_ARG;
  a.part = static_cast<unsigned*>(workspace);
  a.ntile = ldc_cdiv(static_cast<long long>(H) * W, TPB);
  a.tpw = tiles_per_wg(M);
  a.nrec = ldc_cdiv(a.ntile, a.tpw);
  dim3 grid(a.nrec, C, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) launch_reliability<true>(a, grid, s);
  else launch_reliability<false>(a, grid, s);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(reliability_finish_kernel, dim3(C, L), dim3(TPB), 0, s, a.part, a.nrec, M, C, nan_channel, out, hist_count, hist_weight,
                     n_invalid, L_total, l_off);
  return ldc_launch_status();
}
