// Energy score of a decoded ensemble: per (channel, lead time) of a decode batch the pairwise squared distances
// between all members and the truth over every grid point, and from them the multivariate generalisation of the CRPS,
//   ES = mean_i ||x_i - t|| - 1/2 mean_{i,j} ||x_i - x_j||,   ||.|| the latitude-weighted RMS norm of a whole field,
// per channel and per group of channels (each divided by its scale).  Not in the reference.  Addressing is that of ldc_rollout_regional
// (regional.hip): forecast by member / lead / channel strides, optional fused inverse normalisation (inv_norm, ensemble_common.h), truth
// as a table of planes with a slot per lead time, lat_weight[H], output columns at l_off.  The whole file is built with -ffp-contract=off.
// Per (channel c, lead l): vectors y_0 .. y_{M-1} the members after the inverse normalisation, y_M the truth, N = M + 1.
//   valid p: no member and not the truth is NaN; +-inf are ordinary values (inf - inf makes the affected entries NaN, as IEEE says)
//   D2[a][b] = sum over valid p of double(w_p) * double(sq), d = y_a[p] - y_b[p] (one fp32 subtraction), sq = d * d (one fp32 product),
//              w_p = lat_weight[row(p)]; the product is exact, so one fused multiply-add per term rounds exactly as the addition alone
//   Wv = sum over valid p of double(w_p);  norm(a, b) = sqrt(D2[a][b] / Wv)
//   skill = sum_i norm(i, M) / M;  spread = sum_{i != j} norm(i, j) / M^2;  spread_fair = the same sum / (M (M - 1)), 0 at M == 1
//   es = skill - 0.5 spread;  es_fair = skill - 0.5 spread_fair;  all NaN when Wv == 0.  Sums in (i, j) lexicographic order.
//   group g: D2_g[a][b] = sum over c in g, ascending, of D2_c[a][b] * inv_scale2[c];  Wv_g = sum over c in g of Wv_c
// Tiling.  The N x N matrix is cut into 4 x 4 blocks, NB = ceil(N / 4) per side; only the NBP = NB (NB + 1) / 2 blocks on or above the
// diagonal are computed (D2 is symmetric: (x - y)^2 and (y - x)^2 are the same bits).  A thread owns ONE block - 16 fp64 accumulators in
// registers - and one of SL point slices; a workgroup of 256 threads serves BPG = min(NBP, 256) blocks x SL slices (SL the largest power of
// two with BPG * SL <= 256, at most PT), and NBP > 256 (M >= 88) spreads the blocks over NGRP = ceil(NBP / 256) workgroups.  A workgroup
// walks a chunk of CHUNK_TILES tiles of PT = 32 points.  A tile is staged in LDS point-major, s_y[p][RS] (RS = 4 NB or 4 (NB + 1): RS / 4
// odd, so consecutive rows start on different banks), each member value loaded from HBM once per workgroup, i.e. once per 256 / SL blocks
// of 16 pairs.  An invalid point (and the padding behind the last point) is REPLACED by zeros with weight 0: it adds +0.0, which changes
// no bit, and 0 * NaN never forms.  The walk reads per point two float4 (the block's row and column values; lanes of one slice read the
// same point: a broadcast) and the weight, and does 16 x (v_sub_f32, v_mul_f32, v_cvt_f64_f32, v_fma_f64).
// Reduction without atomics in an order that depends on H, W and M only: a thread adds its slice's points in index order; the slices of a
// workgroup are added in slice order (through LDS); one record [NBP][16] fp64 per chunk goes to the workspace; the finish launch, one
// workgroup per (channel, lead time), adds the records in chunk order, keeps the totals for the group launch, writes dist2 when asked and
// forms the five scores: 256 norms at a time are computed in parallel and added by one thread in (i, j) order (the diagonal adds +0.0).
// The group launch, one workgroup per (group, lead time), forms D2_g entry by entry from the channel totals and scores it the same way.
#include <math.h>

#include "ensemble_common.h"

namespace {

constexpr int TPB = 256;
constexpr int PT = 32;             // points per tile
constexpr int CHUNK_TILES = 128;   // tiles per workgroup: 4096 points
constexpr int NVG = TPB / PT;      // staging: thread (vg, sp) loads vectors vg, vg + 8, ... of point sp
constexpr int MAX_M = 256;
constexpr int MAX_G = 32;
constexpr int BLK = 16;            // entries of a 4 x 4 block

struct Geo {
  int N, NB, NBP, RS, BPG, SL, NGRP;
};

__host__ __device__ inline Geo make_geo(int M) {
  Geo g;
  g.N = M + 1;
  g.NB = (g.N + 3) / 4;
  g.NBP = g.NB * (g.NB + 1) / 2;
  g.RS = 4 * (g.NB | 1);
  g.BPG = g.NBP < TPB ? g.NBP : TPB;
  g.SL = 1;
  while (g.SL * 2 * g.BPG <= TPB && g.SL * 2 <= PT) g.SL *= 2;
  g.NGRP = (g.NBP + TPB - 1) / TPB;
  return g;
}

// block (bi, bj), bi <= bj, of the upper triangle: row bi holds NB - bi blocks
__host__ __device__ inline int block_index(int bi, int bj, int NB) { return bi * NB - bi * (bi - 1) / 2 + (bj - bi); }

// entry (a, b), a != b, of a [NBP][16] record
__device__ __forceinline__ long long entry_index(int a, int b, int NB) {
  const int lo = a < b ? a : b, hi = a < b ? b : a;
  return static_cast<long long>(block_index(lo >> 2, hi >> 2, NB)) * BLK + (lo & 3) * 4 + (hi & 3);
}

// the workspace: doubles first (8-byte aligned), the int32 counts last
struct WsLayout {
  long long part, tot, wv_part, wv_tot, ninv_part, bytes;  // offsets in bytes
};

__host__ inline WsLayout ws_layout(const Geo& g, int C, int L, int nchunk) {
  const long long CL = static_cast<long long>(C) * L, rec = static_cast<long long>(g.NBP) * BLK * 8;
  WsLayout w;
  w.part = 0;
  w.tot = w.part + CL * nchunk * rec;
  w.wv_part = w.tot + CL * rec;
  w.wv_tot = w.wv_part + CL * nchunk * 8;
  w.ninv_part = w.wv_tot + CL * 8;
  w.bytes = (w.ninv_part + CL * nchunk * 4 + 7) & ~7ll;
  return w;
}

struct EnArgs {
  RolloutView v;    // no climatology
  double* part;    // [L][C][nchunk][NBP][16]
  double* wv_part;  // [L][C][nchunk]
  int* ninv_part;   // [L][C][nchunk]
  int ntile, nchunk;
};

template <bool INV>
__global__ __launch_bounds__(TPB) void energy_pair_kernel(EnArgs a) {
  // sized at the launch (pair_lds_bytes): the tile as floats [PT][RS]; after the walk one block row of the slices' accumulators at a time,
  // doubles [TPB][4].  What the tile does not need at small M goes to occupancy: 4 workgroups per CU at M = 256, the VGPRs' 6 below M = 128
  extern __shared__ __attribute__((aligned(16))) double s_buf[];
  __shared__ double s_w[PT];
  __shared__ double s_wred[PT];
  __shared__ int s_cnt[PT];
  __shared__ unsigned char s_nan[NVG][PT];
  float* s_y = reinterpret_cast<float*>(s_buf);
  const Geo g = make_geo(a.v.M);
  const int c = blockIdx.y, l = blockIdx.z;
  const int chunk = blockIdx.x / g.NGRP, grp = blockIdx.x % g.NGRP;
  const int M = a.v.M, N = g.N, RS = g.RS;
  const int HW = a.v.H * a.v.W;
  const int tid = threadIdx.x;
  const int sp = tid & (PT - 1), vg = tid / PT;
  const int s = tid / g.BPG, bpl = tid % g.BPG;
  const int bp = grp * TPB + bpl;
  const bool active = s < g.SL && bp < g.NBP;
  int bi = 0, bj = 0;
  if (active) {
    int rem = bp;
    while (rem >= g.NB - bi) {
      rem -= g.NB - bi;
      ++bi;
    }
    bj = bi + rem;
  }
  const float* fbase = view_forecast(a.v, c, l);
  const float* tbase = view_truth(a.v, c, l);
  const InvNorm nrm = view_norm<INV>(a.v, c);
  for (int i = N + vg; i < RS; i += NVG) s_y[sp * RS + i] = 0.f;  // the columns behind the truth: never written again
  double acc[4][4];
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int q = 0; q < 4; ++q) acc[r][q] = 0.0;
  double wacc = 0.0;
  int n_inv = 0;
  const int tile0 = chunk * CHUNK_TILES;
  const int tile1 = min(tile0 + CHUNK_TILES, a.ntile);
  for (int tile = tile0; tile < tile1; ++tile) {
    const int p = tile * PT + sp;
    const bool inb = p < HW;
    bool nan = false;
    for (int i = vg; i < N; i += NVG) {
      float v = 0.f;
      if (inb) v = i < M ? load_member<INV>(fbase + p, i, a.v.fc_ms, nrm) : tbase[p];
      nan = nan || (v != v);
      s_y[sp * RS + i] = v;
    }
    s_nan[vg][sp] = nan ? 1 : 0;
    __syncthreads();
    bool bad = !inb;
#pragma unroll
    for (int k = 0; k < NVG; ++k) bad = bad || (s_nan[k][sp] != 0);
    if (bad)  // replaced, not multiplied by zero: the point adds +0.0 to every sum
      for (int i = vg; i < N; i += NVG) s_y[sp * RS + i] = 0.f;
    if (vg == 0) {
      s_w[sp] = bad ? 0.0 : static_cast<double>(a.v.lat_w[p / a.v.W]);
      n_inv += (bad && inb) ? 1 : 0;
    }
    __syncthreads();
    if (active) {
      const float* ra = s_y + 4 * bi;
      const float* rb = s_y + 4 * bj;
#pragma unroll 2
      for (int q = s; q < PT; q += g.SL) {
        const float4 va = *reinterpret_cast<const float4*>(ra + q * RS);
        const float4 vb = *reinterpret_cast<const float4*>(rb + q * RS);
        const double w = s_w[q];
        const float xa[4] = {va.x, va.y, va.z, va.w};
        const float xb[4] = {vb.x, vb.y, vb.z, vb.w};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
          for (int k = 0; k < 4; ++k) {
            const float d = xa[r] - xb[k];
            const float sq = d * d;
            acc[r][k] = fma(w, static_cast<double>(sq), acc[r][k]);  // the product is exact: one rounding, that of the addition
          }
        wacc = wacc + w;
      }
    }
    __syncthreads();
  }
  // the slices of a block, added in slice order, one block row at a time (the last barrier of the loop stands before the first store)
  double* s_red = s_buf;
  if (active && bp == 0) s_wred[s] = wacc;
  if (vg == 0) s_cnt[sp] = n_inv;
  const long long rec = (static_cast<long long>(l) * a.v.C + c) * a.nchunk + chunk;
#pragma unroll
  for (int r = 0; r < 4; ++r) {
#pragma unroll
    for (int k = 0; k < 4; ++k) s_red[tid * 4 + k] = acc[r][k];
    __syncthreads();
    if (active && s == 0) {
      double* dst = a.part + (rec * g.NBP + bp) * BLK + r * 4;
      for (int k = 0; k < 4; ++k) {
        double t = s_red[bpl * 4 + k];
        for (int q = 1; q < g.SL; ++q) t = t + s_red[(q * g.BPG + bpl) * 4 + k];
        dst[k] = t;
      }
    }
    __syncthreads();
  }
  if (tid == 0 && grp == 0) {
    double t = s_wred[0];
    for (int q = 1; q < g.SL; ++q) t = t + s_wred[q];
    int n = 0;
    for (int q = 0; q < PT; ++q) n += s_cnt[q];
    a.wv_part[rec] = t;
    a.ninv_part[rec] = n;
  }
}

// The five scores of one matrix: d2(a, b) gives entry a != b, Wv the weight.  Every thread of the workgroup calls it; thread 0 gets the
// result: out[0 .. 3] = es, es_fair, skill, spread.  256 norms at a time, added by thread 0 in (i, j) order; the diagonal adds +0.0.
template <class D2F>
__device__ void energy_scores(D2F d2, double Wv, int M, double* s_norm, double* out) {
  const int tid = threadIdx.x;
  double skill_sum = 0.0, spread_sum = 0.0;
  for (int base = 0; base < M; base += TPB) {
    const int i = base + tid;
    s_norm[tid] = i < M ? sqrt(d2(i, M) / Wv) : 0.0;
    __syncthreads();
    if (tid == 0) {
      const int n = min(TPB, M - base);
      for (int q = 0; q < n; ++q) skill_sum = skill_sum + s_norm[q];
    }
    __syncthreads();
  }
  const int MM = M * M;
  for (int base = 0; base < MM; base += TPB) {
    const int e = base + tid;
    double v = 0.0;
    if (e < MM) {
      const int i = e / M, j = e % M;
      if (i != j) v = sqrt(d2(i, j) / Wv);
    }
    s_norm[tid] = v;
    __syncthreads();
    if (tid == 0) {
      const int n = min(TPB, MM - base);
      for (int q = 0; q < n; ++q) spread_sum = spread_sum + s_norm[q];
    }
    __syncthreads();
  }
  if (tid == 0) {
    const double Md = static_cast<double>(M);
    double skill = skill_sum / Md;
    double spread = spread_sum / (Md * Md);
    double fair = M > 1 ? spread_sum / (Md * (Md - 1.0)) : 0.0;
    if (!(Wv != 0.0)) skill = spread = fair = NAN;
    out[0] = skill - 0.5 * spread;
    out[1] = skill - 0.5 * fair;
    out[2] = skill;
    out[3] = spread;
  }
}

// One workgroup per (channel, lead time): grid (C, L).
__global__ __launch_bounds__(TPB) void energy_finish_kernel(const double* __restrict__ part, const double* __restrict__ wv_part,
                                                            const int* __restrict__ ninv_part, double* __restrict__ tot,
                                                            double* __restrict__ wv_tot, int nchunk, int M, int C, double* __restrict__ energy,
                                                            int* __restrict__ n_invalid, double* __restrict__ dist2, int L_total, int l_off) {
  __shared__ double s_norm[TPB];
  __shared__ double s_wv;
  const Geo g = make_geo(M);
  const int c = blockIdx.x, l = blockIdx.y;
  const int tid = threadIdx.x;
  const long long cl = static_cast<long long>(l) * C + c;
  const long long recn = static_cast<long long>(g.NBP) * BLK;
  double* t = tot + cl * recn;
  for (long long e = tid; e < recn; e += TPB) {
    double acc = part[cl * nchunk * recn + e];
    for (int k = 1; k < nchunk; ++k) acc = acc + part[(cl * nchunk + k) * recn + e];
    t[e] = acc;
  }
  const long long col = static_cast<long long>(c) * L_total + l_off + l;
  if (tid == 0) {
    double w = wv_part[cl * nchunk];
    int n = ninv_part[cl * nchunk];
    for (int k = 1; k < nchunk; ++k) {
      w = w + wv_part[cl * nchunk + k];
      n += ninv_part[cl * nchunk + k];
    }
    s_wv = w;
    wv_tot[cl] = w;
    n_invalid[col] = n;
  }
  __syncthreads();  // the totals of this workgroup are read back below
  const double Wv = s_wv;
  const int N = g.N, NB = g.NB;
  if (dist2 != nullptr) {
    double* d = dist2 + col * N * N;
    for (int e = tid; e < N * N; e += TPB) {
      const int i = e / N, j = e % N;
      d[e] = i == j ? 0.0 : t[entry_index(i, j, NB)];
    }
  }
  double out[4];
  energy_scores([&](int i, int j) { return t[entry_index(i, j, NB)]; }, Wv, M, s_norm, out);
  if (tid == 0) {
    const long long plane = static_cast<long long>(C) * L_total;
#pragma unroll
    for (int k = 0; k < 4; ++k) energy[k * plane + col] = out[k];
    energy[4 * plane + col] = Wv;
  }
}

// One workgroup per (group, lead time): grid (G, L), after the finish launch.
__global__ __launch_bounds__(TPB) void energy_group_kernel(const double* __restrict__ tot, const double* __restrict__ wv_tot,
                                                           const unsigned* __restrict__ group_mask, const double* __restrict__ inv_scale2,
                                                           int G, int M, int C, double* __restrict__ energy_group, int L_total, int l_off) {
  __shared__ double s_norm[TPB];
  __shared__ double s_wv;
  const Geo g = make_geo(M);
  const int gi = blockIdx.x, l = blockIdx.y;
  const int tid = threadIdx.x;
  const long long recn = static_cast<long long>(g.NBP) * BLK;
  const double* t = tot + static_cast<long long>(l) * C * recn;
  if (tid == 0) {
    double w = 0.0;
    for (int c = 0; c < C; ++c)
      if ((group_mask[c] >> gi) & 1u) w = w + wv_tot[static_cast<long long>(l) * C + c];
    s_wv = w;
  }
  __syncthreads();
  const double Wv = s_wv;
  const int NB = g.NB;
  double out[4];
  energy_scores(
      [&](int i, int j) {
        const long long e = entry_index(i, j, NB);
        double acc = 0.0;
        for (int c = 0; c < C; ++c)
          if ((group_mask[c] >> gi) & 1u) acc = acc + t[c * recn + e] * inv_scale2[c];
        return acc;
      },
      Wv, M, s_norm, out);
  if (tid == 0) {
    const long long plane = static_cast<long long>(G) * L_total;
    const long long col = static_cast<long long>(gi) * L_total + l_off + l;
#pragma unroll
    for (int k = 0; k < 4; ++k) energy_group[k * plane + col] = out[k];
    energy_group[4 * plane + col] = Wv;
  }
}

// the pair kernel's LDS: the tile, or a block row of every thread's accumulators, whichever is larger
static inline unsigned pair_lds_bytes(const Geo& g) {
  const unsigned tile = PT * g.RS * 4u, red = TPB * 4u * 8u;
  return tile > red ? tile : red;
}

}  // namespace

extern "C" long long ldc_rollout_energy_workspace_bytes(int M, int C, int G, int L, int H, int W) {
  if (M <= 0 || M > MAX_M || G < 0 || G > MAX_G || C <= 0 || C > 65535 || L <= 0 || L > 65535 || H <= 0 || W <= 0) return 0;
  if (static_cast<long long>(H) * W > (1ll << 24)) return 0;
  const int ntile = ldc_cdiv(static_cast<long long>(H) * W, PT);
  return ws_layout(make_geo(M), C, L, ldc_cdiv(ntile, CHUNK_TILES)).bytes;
}

extern "C" int ldc_rollout_energy(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                  const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                                  long long truth_channel_stride, const int* truth_slot, const float* lat_weight, const unsigned* group_mask,
                                  const double* inv_scale2, int G, int M, int C, int L, int H, int W, double* energy, double* energy_group,
                                  int* n_invalid, double* dist2, int L_total, int l_off, void* workspace, long long workspace_bytes,
                                  void* stream) {
  EnArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, nullptr, 0, 0, nullptr, lat_weight, M, C, L, H, W, L_total, l_off) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(energy);
  LDC_CHECK_PTR(n_invalid);
  LDC_CHECK_PTR(workspace);
  if (G < 0) return LDC_ERR_ARG;
  if (G > 0) {
    LDC_CHECK_PTR(group_mask);
    LDC_CHECK_PTR(inv_scale2);
    LDC_CHECK_PTR(energy_group);
  } else if (energy_group != nullptr) {
    return LDC_ERR_ARG;  // energy_group is NULL iff G == 0
  }
  if (M > MAX_M || G > MAX_G || C > 65535 || L > 65535 || static_cast<long long>(H) * W > (1ll << 24)) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < ldc_rollout_energy_workspace_bytes(M, C, G, L, H, W)) return LDC_ERR_ARG;
  const auto misaligned = [](const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7u) != 0; };  // fp64
  if (misaligned(workspace) || misaligned(energy) || misaligned(energy_group) || misaligned(dist2) || misaligned(inv_scale2))
    return LDC_ERR_ALIGN;
  const Geo g = make_geo(M);
  a.ntile = ldc_cdiv(static_cast<long long>(H) * W, PT);
  a.nchunk = ldc_cdiv(a.ntile, CHUNK_TILES);
  const WsLayout w = ws_layout(g, C, L, a.nchunk);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  a.part = reinterpret_cast<double*>(ws + w.part);
  a.wv_part = reinterpret_cast<double*>(ws + w.wv_part);
  a.ninv_part = reinterpret_cast<int*>(ws + w.ninv_part);
  double* tot = reinterpret_cast<double*>(ws + w.tot);
  double* wv_tot = reinterpret_cast<double*>(ws + w.wv_tot);
  dim3 grid(a.nchunk * g.NGRP, C, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) hipLaunchKernelGGL(energy_pair_kernel<true>, grid, dim3(TPB), pair_lds_bytes(g), s, a);
  else hipLaunchKernelGGL(energy_pair_kernel<false>, grid, dim3(TPB), pair_lds_bytes(g), s, a);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(energy_finish_kernel, dim3(C, L), dim3(TPB), 0, s, a.part, a.wv_part, a.ninv_part, tot, wv_tot, a.nchunk, M, C, energy,
                     n_invalid, dist2, L_total, l_off);
  st = ldc_launch_status();
  if (st != LDC_OK || G == 0) return st;
  hipLaunchKernelGGL(energy_group_kernel, dim3(G, L), dim3(TPB), 0, s, tot, wv_tot, group_mask, inv_scale2, G, M, C, energy_group, L_total,
                     l_off);
  return ldc_launch_status();
}
