// Regional ensemble scores of a decoded forecast: one pass over a decode batch returns, for up to 32 regions that
// may overlap, the additive sufficient statistics of bias, RMSE, spread, spread-skill ratio, CRPS (skill / spread) and ACC per (region,
// channel, lead time).  The sums add over initial times; ladcast_amd.evaluate.regional_scores derives the scores on the host in float64.
// Not in the reference.  Addressing is that of ldc_rollout_scores (scoring.hip): forecast by member / lead / channel strides, optional
// fused inverse normalisation (inv_norm, ensemble_common.h), truth and climatology as tables of planes with a slot per lead time,
// lat_weight[H], output columns at l_off.  region_mask[H * W]: bit r of the word of point p says that p belongs to region r < R <= 32.
// Per grid point that lies in at least one region, members x_i in member order after the inverse normalisation, truth t, weight w,
// climatology a, every value fp32 and formed as the kernel that already has it forms it (ensemble_point_values, ensemble_common.h: the
// one function that this kernel and score_maps.hip call, so that the maps hold these bits):
//   mean   = (x_0 + ... + x_{M-1}) / M, e = mean - t, se = e * e            (score_point, scoring.hip)
//   var    = sum_i (x_i - mean)^2 / (M - 1), two-pass in member order       (reliability.hip); M == 1: 0
//   skill  = sum_i |t - x_i| / M                                            (score_point)
//   spread = 2 ws / (M (M - 1)), ws = sum_i x_(i) (2 i - M - 1) over the sorted members, each step one fused multiply-add as the
//            contracted build of score_point has it; M == 1: 0
//   fa = mean - a, ta = t - a; fta = fa * ta, ffa = fa * fa, tta = ta * ta  (one fp32 product each)
//   valid: no member and not the truth is NaN; ACC-valid: valid and a is not NaN; +-inf are ordinary values (the sums follow IEEE)
// A point of no region is not read.  The whole file is built with -ffp-contract=off.
// sums [R][C][L_total][10] fp64 = over the region's valid points  sum w, w e, w se, w var, w skill, w spread,
//                                 over its ACC-valid points       sum w, w fta, w ffa, w tta          (zeros without clim)
//   every term double(w) * double(v): exact, so the only rounding behind the fp32 point values is that of the fp64 additions
// counts [R][C][L_total][3] int32 = valid, invalid, ACC-valid points of the region
// Reduction without atomics, in a fixed order that does not depend on R or on the other regions.  A workgroup covers TPW consecutive
// tiles of 256 points; a tile without a point of any region is skipped before a member is loaded:
//   every thread publishes its point's 10 terms (fp64) and three mask words (valid / ACC-valid / invalid: the region bits or 0) to LDS
//   thread (r, s), r = tid & 31, s = tid >> 5, walks the tile's 256 points in index order (all lanes of a slot read the same address: an
//     LDS broadcast) and adds the terms of the points whose mask has bit r: slots 0 .. 4 two sums each (terms 2 s, 2 s + 1), slot 6 the
//     three counts; the accumulators stay in registers across the workgroup's tiles: one sequential sum over the workgroup's points
//   one record [32][10 fp64 + 4 int32] per workgroup; finish launch, one workgroup per (channel, lead time): entry (r, k) adds the
//     records' entries in record order.
#include <math.h>

#include "ensemble_common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_R = 32;
constexpr int NS = 10;   // sums per region
constexpr int NCNT = 3;  // counts per region
// tiles per workgroup: fixed, because the grouping of the fp64 additions must not depend on R.  A record holds MAX_R * (10 fp64 + 4 int32)
// = 3072 bytes whatever R is, so the workspace is 3072 / (8 * 256) = 1.5 bytes per point and (channel, lead time)
constexpr int TPW = 8;
constexpr int REC_BYTES = MAX_R * (NS * 8 + 4 * 4);
constexpr int REC_CNT_OFF = MAX_R * NS * 8;  // the counts follow the sums: [32][4] int32

struct RegArgs {
  RolloutView v;        // clim nullptr: no ACC terms
  const unsigned* reg;  // [H * W]
  unsigned char* part;  // [L][C][nrec][REC_BYTES]
  int R, ntile, nrec;
};

template <int NP, int NUSE, bool INV>
__global__ __launch_bounds__(TPB) void regional_kernel(RegArgs a) {
  __shared__ __attribute__((aligned(16))) double s_val[TPB * NS];
  __shared__ __attribute__((aligned(16))) unsigned s_m[3][TPB];  // valid, ACC-valid, invalid
  const int c = blockIdx.y, l = blockIdx.z;
  const int M = a.v.M;
  const int HW = a.v.H * a.v.W;
  const int tid = threadIdx.x;
  const int r = tid & 31, s = tid >> 5;
  const unsigned rmask = a.R >= 32 ? 0xffffffffu : ((1u << a.R) - 1u);
  const float* fbase = view_forecast(a.v, c, l);
  const float* tbase = view_truth(a.v, c, l);
  const float* cbase = view_clim(a.v, c, l);
  const InvNorm nrm = view_norm<INV>(a.v, c);
  double acc0 = 0.0, acc1 = 0.0;
  int n_val = 0, n_inv = 0, n_acc = 0;
  const int tile0 = blockIdx.x * TPW;
  const int tile1 = min(tile0 + TPW, a.ntile);
  for (int tile = tile0; tile < tile1; ++tile) {
    const int p = tile * TPB + tid;
    const unsigned m = p < HW ? (a.reg[p] & rmask) : 0u;  // the padding threads of the last tile belong to no region
    // also the barrier behind the walk of the tile before; a tile without a point of any region costs one mask load
    if (!__syncthreads_or(m != 0u)) continue;
    unsigned mv = 0u, ma = 0u, mi = 0u;
    if (m != 0u) {
      const PointValues pv = ensemble_point_values<NP, NUSE, INV>(fbase + p, a.v.fc_ms, nrm, M, tbase + p, cbase ? cbase + p : nullptr);
      const float w = a.v.lat_w[p / a.v.W];
      const double wd = static_cast<double>(w);
      double* dst = &s_val[tid * NS];
      dst[0] = wd;
      dst[1] = wd * static_cast<double>(pv.e);
      dst[2] = wd * static_cast<double>(pv.se);
      dst[3] = wd * static_cast<double>(pv.var);
      dst[4] = wd * static_cast<double>(pv.skill);
      dst[5] = wd * static_cast<double>(pv.spread);
      if (cbase) {
        dst[6] = wd;
        dst[7] = wd * static_cast<double>(pv.fta);
        dst[8] = wd * static_cast<double>(pv.ffa);
        dst[9] = wd * static_cast<double>(pv.tta);
      }
      mv = pv.valid ? m : 0u;
      mi = pv.valid ? 0u : m;
      ma = pv.acc_valid ? m : 0u;
    }
    s_m[0][tid] = mv;
    s_m[1][tid] = ma;
    s_m[2][tid] = mi;
    __syncthreads();
    if (r < a.R) {
      if (s < 5) {
        const unsigned* mk = s_m[s < 3 ? 0 : 1];
        const double* col = &s_val[2 * s];
#pragma unroll 2
        for (int q = 0; q < TPB; q += 4) {
          const uint4 mm = *reinterpret_cast<const uint4*>(&mk[q]);
          const double2 v0 = *reinterpret_cast<const double2*>(&col[(q + 0) * NS]);
          const double2 v1 = *reinterpret_cast<const double2*>(&col[(q + 1) * NS]);
          const double2 v2 = *reinterpret_cast<const double2*>(&col[(q + 2) * NS]);
          const double2 v3 = *reinterpret_cast<const double2*>(&col[(q + 3) * NS]);
          const bool b0 = (mm.x >> r) & 1u, b1 = (mm.y >> r) & 1u, b2 = (mm.z >> r) & 1u, b3 = (mm.w >> r) & 1u;
          acc0 = b0 ? acc0 + v0.x : acc0;  // a point of another region is not added at all: no term of it, not even a zero
          acc1 = b0 ? acc1 + v0.y : acc1;
          acc0 = b1 ? acc0 + v1.x : acc0;
          acc1 = b1 ? acc1 + v1.y : acc1;
          acc0 = b2 ? acc0 + v2.x : acc0;
          acc1 = b2 ? acc1 + v2.y : acc1;
          acc0 = b3 ? acc0 + v3.x : acc0;
          acc1 = b3 ? acc1 + v3.y : acc1;
        }
      } else if (s == 6) {
#pragma unroll 2
        for (int q = 0; q < TPB; q += 4) {
          const uint4 kv = *reinterpret_cast<const uint4*>(&s_m[0][q]);
          const uint4 ka = *reinterpret_cast<const uint4*>(&s_m[1][q]);
          const uint4 ki = *reinterpret_cast<const uint4*>(&s_m[2][q]);
          n_val += static_cast<int>(((kv.x >> r) & 1u) + ((kv.y >> r) & 1u) + ((kv.z >> r) & 1u) + ((kv.w >> r) & 1u));
          n_acc += static_cast<int>(((ka.x >> r) & 1u) + ((ka.y >> r) & 1u) + ((ka.z >> r) & 1u) + ((ka.w >> r) & 1u));
          n_inv += static_cast<int>(((ki.x >> r) & 1u) + ((ki.y >> r) & 1u) + ((ki.z >> r) & 1u) + ((ki.w >> r) & 1u));
        }
      }
    }
  }
  // the record: every entry of every region is written, zeros where the workgroup met no point (or no climatology)
  unsigned char* rec = a.part + ((static_cast<long long>(l) * a.v.C + c) * a.nrec + blockIdx.x) * REC_BYTES;
  if (s < 5) {
    double* d = reinterpret_cast<double*>(rec) + r * NS + 2 * s;
    d[0] = acc0;
    d[1] = acc1;
  } else if (s == 6) {
    int* d = reinterpret_cast<int*>(rec + REC_CNT_OFF) + r * 4;
    d[0] = n_val;
    d[1] = n_inv;
    d[2] = n_acc;
    d[3] = 0;
  }
}

// One workgroup per (channel, lead time): grid (C, L).  sums [R][C][L_total][10], counts [R][C][L_total][3]; column l_off + l.
__global__ __launch_bounds__(TPB) void regional_finish_kernel(const unsigned char* __restrict__ part, int nrec, int R, int C,
                                                              double* __restrict__ sums, int* __restrict__ counts, int L_total, int l_off) {
  const int c = blockIdx.x, l = blockIdx.y;
  const unsigned char* base = part + (static_cast<long long>(l) * C + c) * nrec * REC_BYTES;
  for (int i = threadIdx.x; i < R * (NS + NCNT); i += TPB) {
    const int r = i / (NS + NCNT), k = i % (NS + NCNT);
    const long long col = (static_cast<long long>(r) * C + c) * L_total + l_off + l;
    if (k < NS) {
      double acc = 0.0;
      for (int b = 0; b < nrec; ++b) acc += reinterpret_cast<const double*>(base + static_cast<long long>(b) * REC_BYTES)[r * NS + k];
      sums[col * NS + k] = acc;
    } else {
      int n = 0;
      for (int b = 0; b < nrec; ++b)
        n += reinterpret_cast<const int*>(base + static_cast<long long>(b) * REC_BYTES + REC_CNT_OFF)[r * 4 + (k - NS)];
      counts[col * NCNT + (k - NS)] = n;
    }
  }
}

template <bool INV>
void launch_regional(const RegArgs& a, dim3 grid, hipStream_t s) {
  ldc_dispatch_sort_arm(a.v.M, [&](auto np, auto nuse) {
    hipLaunchKernelGGL((regional_kernel<decltype(np)::value, decltype(nuse)::value, INV>), grid, dim3(TPB), 0, s, a);
  });
}

}  // namespace

extern "C" long long ldc_rollout_regional_workspace_bytes(int M, int R, int C, int L, int H, int W) {
  if (M <= 0 || M > 64 || R <= 0 || R > MAX_R || C <= 0 || C > 65535 || L <= 0 || L > 65535 || H <= 0 || W <= 0) return 0;
  if (static_cast<long long>(H) * W > (1ll << 24)) return 0;
  const long long ntile = (static_cast<long long>(H) * W + TPB - 1) / TPB;
  const long long nrec = (ntile + TPW - 1) / TPW;
  return static_cast<long long>(L) * C * nrec * REC_BYTES;
}

extern "C" int ldc_rollout_regional(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                    const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                                    long long truth_channel_stride, const int* truth_slot, const float* clim, long long clim_slot_stride,
                                    long long clim_channel_stride, const int* clim_slot, const float* lat_weight,
                                    const unsigned* region_mask, int R, int M, int C, int L, int H, int W, double* sums, int* counts,
                                    int L_total, int l_off, void* workspace, long long workspace_bytes, void* stream) {
  RegArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, clim, clim_slot_stride, clim_channel_stride, clim_slot, lat_weight, M, C, L, H, W,
                       L_total, l_off) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(region_mask);
  LDC_CHECK_PTR(sums);
  LDC_CHECK_PTR(counts);
  LDC_CHECK_PTR(workspace);
  if (R <= 0) return LDC_ERR_ARG;
  if (M > 64 || R > MAX_R || C > 65535 || L > 65535 || static_cast<long long>(H) * W > (1ll << 24)) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < ldc_rollout_regional_workspace_bytes(M, R, C, L, H, W)) return LDC_ERR_ARG;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || (reinterpret_cast<uintptr_t>(sums) & 7u) != 0) return LDC_ERR_ALIGN;  // fp64
  a.reg = region_mask;
  a.R = R;
  a.part = static_cast<unsigned char*>(workspace);
  a.ntile = ldc_cdiv(static_cast<long long>(H) * W, TPB);
  a.nrec = ldc_cdiv(a.ntile, TPW);
  dim3 grid(a.nrec, C, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) launch_regional<true>(a, grid, s);
  else launch_regional<false>(a, grid, s);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(regional_finish_kernel, dim3(C, L), dim3(TPB), 0, s, a.part, a.nrec, R, C, sums, counts, L_total, l_off);
  return ldc_launch_status();
}
