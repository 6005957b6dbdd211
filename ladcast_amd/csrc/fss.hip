// Neighbourhood verification of threshold events of a decoded ensemble: the sufficient statistics of the
// fractions skill score (Roberts & Lean 2008) per (event, neighbourhood radius, lead time).  Not in the reference.  Addressing, events
// and the classification of a grid point are those of ldc_rollout_events (events.hip; classify_event_point, events_common.h).
// Per event e and radius r the window of a centre p = (i, j) is rows i - r .. i + r clipped to 0 .. H - 1 and columns j - r .. j + r
// modulo W (longitude is periodic).  Over the valid points q of the window, exact integers:
//   N = #valid, Sn = sum n(q), So = sum o(q)
// A centre contributes when p itself is valid (so N >= 1).  Per contributing centre, fp64, every operation rounded on its own (the file is
// built with -ffp-contract=off), w = double(lat_weight[i]):
//   Pf = double(Sn) / (double(M) * double(N)),  Po = double(So) / double(N),  a = w * Pf,  b = w * Po,  d = Pf - Po
//   terms { w, a, b, a * Pf, b * Po, (w * d) * d }
// Four passes per call and a finish, every one over grid (.., E, L):
//   count   one thread per point: classify, write the packed word  n | o << 11 | valid << 12  (0 for an invalid point) to the workspace
//   rows    one wave per row: the running sums of (n, o, valid) along the row, 64 columns per step by a wave scan, into the summed-area
//           table T of (H + 1) x (W + 1) entries whose row 0 and column 0 are zero: T[i + 1][j + 1] = row i, columns 0 .. j
//   columns one thread per column: the running sum down the rows, in place: T[i][j] = sum over rows < i and columns < j
//   window  one thread per centre: per radius the four corners of the clipped row range at the window's two column ends, and once more
//           at column W where the window crosses the seam (the sum is then T(.., W) - T(.., lo) + T(.., hi)); the six terms
// Integer widths: three uint32 per table entry.  So, N <= H W <= 2^24; Sn <= M H W, and the call refuses M H W > 2^31.  Differences of
// entries are taken in unsigned arithmetic and are the exact window sums.
// Reduction without float atomics, in a fixed order: the 64 lanes of a wave by butterfly (6 levels), the 4 wave totals pairwise (2
// levels), one record of S x 6 sums per workgroup; the finish launch, one workgroup per (event, lead time), adds the records in record
// order.  The invalid centres are counted the same way in integers.
#include <math.h>
#include <stdint.h>

#include "events_common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_M = 1024;
constexpr int NT = 6;  // terms per (event, radius, lead time)
constexpr int N_BITS = 11, O_BIT = 11, V_BIT = 12;  // the packed word: n in 0 .. 1024, o, valid
constexpr long long MAX_SN = 1ll << 31;  // M H W at most: Sn in uint32

struct Sat {
  unsigned sn, so, nv;
};

__device__ __forceinline__ Sat operator+(const Sat& a, const Sat& b) { return Sat{a.sn + b.sn, a.so + b.so, a.nv + b.nv}; }
__device__ __forceinline__ Sat operator-(const Sat& a, const Sat& b) { return Sat{a.sn - b.sn, a.so - b.so, a.nv - b.nv}; }

struct FssArgs {
  RolloutView v;     // clim nullptr: no anomaly event
  int E, S;
  double* rec;       // [L][E][nrec][S][6]
  int* rec_inv;      // [L][E][nrec]
  unsigned* packed;  // [L][E][H W]
  Sat* sat;          // [L][E][H + 1][W + 1]
  int nrec;          // tiles of 256 points per plane
  int radius[LDC_FSS_SCALES_MAX];
  ldc_events_desc d;
};

struct Layout {
  long long rec, rec_inv, packed, sat, total;  // byte offsets, each a multiple of 8
};

inline long long up8(long long v) { return (v + 7) & ~7ll; }

inline Layout layout_of(int E, int S, int L, int H, int W) {
  const long long planes = static_cast<long long>(L) * E, HW = static_cast<long long>(H) * W;
  const long long nrec = (HW + TPB - 1) / TPB;
  Layout o{};
  o.rec = 0;
  o.rec_inv = o.rec + planes * nrec * S * NT * static_cast<long long>(sizeof(double));
  o.packed = o.rec_inv + up8(planes * nrec * static_cast<long long>(sizeof(int)));
  o.sat = o.packed + up8(planes * HW * static_cast<long long>(sizeof(unsigned)));
  o.total = o.sat + up8(planes * (H + 1ll) * (W + 1ll) * static_cast<long long>(sizeof(Sat)));
  return o;
}

__device__ __forceinline__ long long plane_of(const FssArgs& a) { return static_cast<long long>(blockIdx.z) * a.E + blockIdx.y; }

template <int NMAX, bool INV, int DIR>
__device__ __forceinline__ void count_body(const FssArgs& a) {
  const int e = blockIdx.y, l = blockIdx.z;
  const int HW = a.v.H * a.v.W;
  const int p = blockIdx.x * TPB + threadIdx.x;
  const bool in = p < HW;
  const int pp = in ? p : 0;
  const int c = a.d.channel[e];
  const float thr = a.d.thr[e];
  const bool anom = a.d.anomaly[e] != 0;
  const float t = view_truth(a.v, c, l)[pp];
  const float cl = anom ? view_clim(a.v, c, l)[pp] : 0.f;
  const EventPoint pt =
      classify_event_point<NMAX, INV, DIR>(view_forecast(a.v, c, l) + pp, a.v.fc_ms, a.v.M, t, cl, anom, thr, view_norm<INV>(a.v, c));
  if (!in) return;
  const unsigned word = pt.valid ? static_cast<unsigned>(pt.n) | static_cast<unsigned>(pt.o) << O_BIT | 1u << V_BIT : 0u;
  a.packed[plane_of(a) * HW + p] = word;
}

// the direction is uniform per workgroup: one branch, two specialised bodies
template <int NMAX, bool INV>
__global__ __launch_bounds__(TPB) void fss_count_kernel(FssArgs a) {
  if (a.d.dir[blockIdx.y] > 0) count_body<NMAX, INV, 1>(a);
  else count_body<NMAX, INV, -1>(a);
}

// Grid (H, E, L), one wave: row blockIdx.x of the plane, 64 columns per step.
__global__ __launch_bounds__(64) void fss_rows_kernel(FssArgs a) {
  const int i = blockIdx.x, lane = threadIdx.x;
  const int W = a.v.W, W1 = a.v.W + 1;
  const unsigned* src = a.packed + plane_of(a) * a.v.H * W + static_cast<long long>(i) * W;
  Sat* tab = a.sat + plane_of(a) * (a.v.H + 1) * W1;
  if (i == 0)
    for (int j = lane; j < W1; j += 64) tab[j] = Sat{0u, 0u, 0u};
  Sat* dst = tab + static_cast<long long>(i + 1) * W1;
  if (lane == 0) dst[0] = Sat{0u, 0u, 0u};
  Sat carry{0u, 0u, 0u};
  for (int j0 = 0; j0 < W; j0 += 64) {
    const int j = j0 + lane;
    const unsigned word = j < W ? src[j] : 0u;
    Sat v{word & ((1u << N_BITS) - 1u), (word >> O_BIT) & 1u, (word >> V_BIT) & 1u};
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const Sat up{__shfl_up(v.sn, o, 64), __shfl_up(v.so, o, 64), __shfl_up(v.nv, o, 64)};
      if (lane >= o) v = v + up;
    }
    v = v + carry;
    if (j < W) dst[j + 1] = v;
    carry = Sat{__shfl(v.sn, 63, 64), __shfl(v.so, 63, 64), __shfl(v.nv, 63, 64)};
  }
}

// Grid (ceil(W / 64), E, L), one wave: columns 1 .. W of the table, the running sum down rows 1 .. H (row 0 and column 0 stay zero).
__global__ __launch_bounds__(64) void fss_cols_kernel(FssArgs a) {
  const int j = 1 + blockIdx.x * 64 + threadIdx.x;
  if (j > a.v.W) return;
  const int W1 = a.v.W + 1;
  Sat* col = a.sat + plane_of(a) * (a.v.H + 1) * W1 + j;
  Sat acc{0u, 0u, 0u};
  constexpr int NB = 8;  // rows loaded before any is stored: the loads of a batch are in flight together (a store may alias a later load
                         // for all the compiler knows, so a plain loop waits for every load in turn)
  for (int i0 = 1; i0 <= a.v.H; i0 += NB) {
    Sat v[NB];
#pragma unroll
    for (int k = 0; k < NB; ++k) v[k] = i0 + k <= a.v.H ? col[static_cast<long long>(i0 + k) * W1] : Sat{0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < NB; ++k) {
      acc = acc + v[k];
      if (i0 + k <= a.v.H) col[static_cast<long long>(i0 + k) * W1] = acc;
    }
  }
}

// Grid (nrec, E, L), 256 threads: one centre per thread, one record per workgroup.
__global__ __launch_bounds__(TPB) void fss_window_kernel(FssArgs a) {
  __shared__ double red[LDC_FSS_SCALES_MAX][4][NT];
  __shared__ int red_i[4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int H = a.v.H, W = a.v.W, W1 = a.v.W + 1, HW = a.v.H * a.v.W;
  const int p = blockIdx.x * TPB + tid;
  const bool in = p < HW;
  const int pp = in ? p : 0;
  const int i = pp / W, j = pp - i * W;
  const long long plane = plane_of(a);
  const bool contrib = in && ((a.packed[plane * HW + pp] >> V_BIT) & 1u) != 0u;
  const double w = contrib ? static_cast<double>(a.v.lat_w[i]) : 0.0;
  const double dM = static_cast<double>(a.v.M);
  const Sat* tab = a.sat + plane * (H + 1) * W1;
  const double s_w = wave_sum(w);
  for (int s = 0; s < a.S; ++s) {
    const int r = a.radius[s];
    const Sat* top = tab + static_cast<long long>(max(i - r, 0)) * W1;
    const Sat* bot = tab + static_cast<long long>(min(i + r, H - 1) + 1) * W1;
    const int c0 = j - r, c1 = j + r + 1;  // columns c0 .. c1 - 1; 2 r + 1 <= W: at most one end lies outside 0 .. W
    const bool wrap = c0 < 0 || c1 > W;
    const int lo = c0 < 0 ? c0 + W : c0, hi = c1 > W ? c1 - W : c1;
    Sat sum = (bot[hi] - top[hi]) - (bot[lo] - top[lo]);
    if (wrap) sum = sum + (bot[W] - top[W]);
    const double dN = contrib ? static_cast<double>(sum.nv) : 1.0;
    const double Pf = static_cast<double>(sum.sn) / (dM * dN);
    const double Po = static_cast<double>(sum.so) / dN;
    const double fa = w * Pf, fb = w * Po, d = Pf - Po;
    const double t1 = contrib ? fa : 0.0, t2 = contrib ? fb : 0.0;
    const double t3 = contrib ? fa * Pf : 0.0, t4 = contrib ? fb * Po : 0.0, t5 = contrib ? (w * d) * d : 0.0;
    const double r1 = wave_sum(t1), r2 = wave_sum(t2), r3 = wave_sum(t3), r4 = wave_sum(t4), r5 = wave_sum(t5);
    if (lane == 0) {
      red[s][wave][0] = s_w;
      red[s][wave][1] = r1;
      red[s][wave][2] = r2;
      red[s][wave][3] = r3;
      red[s][wave][4] = r4;
      red[s][wave][5] = r5;
    }
  }
  const int i_inv = wave_sum((in && !contrib) ? 1 : 0);
  if (lane == 0) red_i[wave] = i_inv;
  __syncthreads();
  const long long rec = plane * a.nrec + blockIdx.x;
  if (tid < a.S * NT) {
    const int s = tid / NT, k = tid - s * NT;
    a.rec[rec * a.S * NT + tid] = (red[s][0][k] + red[s][1][k]) + (red[s][2][k] + red[s][3][k]);
  }
  if (tid == 0) a.rec_inv[rec] = (red_i[0] + red_i[1]) + (red_i[2] + red_i[3]);
}

// One workgroup of two waves per (event, lead time): grid (E, L).  fss_sums [E][S][L_total][6]; n_invalid [E][L_total]; columns
// l_off .. l_off + L - 1.  Thread t < 6 S adds entry t of the records in record order; the second wave counts the invalid centres.
__global__ __launch_bounds__(128) void fss_finish_kernel(const double* __restrict__ rec, const int* __restrict__ rec_inv, int nrec, int E, int S,
                                                         double* __restrict__ fss_sums, int* __restrict__ n_invalid, int L_total, int l_off) {
  const int e = blockIdx.x, l = blockIdx.y, tid = threadIdx.x;
  const long long base = (static_cast<long long>(l) * E + e) * nrec;
  if (tid < S * NT) {
    const int s = tid / NT, k = tid - s * NT;
    double acc = 0.0;
    constexpr int NB = 8;  // records loaded together; added in record order all the same
    for (int r0 = 0; r0 < nrec; r0 += NB) {
      double v[NB];
#pragma unroll
      for (int k = 0; k < NB; ++k) v[k] = r0 + k < nrec ? rec[(base + r0 + k) * S * NT + tid] : 0.0;
#pragma unroll
      for (int k = 0; k < NB; ++k)
        if (r0 + k < nrec) acc += v[k];
    }
    fss_sums[((static_cast<long long>(e) * S + s) * L_total + l_off + l) * NT + k] = acc;
  }
  if (tid < 64) return;
  int k_inv = 0;
  for (int r = tid - 64; r < nrec; r += 64) k_inv += rec_inv[base + r];
  k_inv = wave_sum(k_inv);
  if (tid == 64) n_invalid[static_cast<long long>(e) * L_total + l_off + l] = k_inv;
}

template <bool INV>
void launch_count(const FssArgs& a, dim3 grid, hipStream_t s) {
  ldc_dispatch_member_arm(a.v.M, [&](auto nmax) {
    hipLaunchKernelGGL((fss_count_kernel<decltype(nmax)::value, INV>), grid, dim3(TPB), 0, s, a);
  });
}

bool sizes_served(int M, int E, int S, int L, int H, int W) {
  if (M <= 0 || M > MAX_M || E <= 0 || E > LDC_EVENTS_MAX || S <= 0 || S > LDC_FSS_SCALES_MAX || L <= 0 || L > 65535 || H <= 0 || W <= 0) return false;
  const long long HW = static_cast<long long>(H) * W;
  return HW <= (1ll << 24) && HW * M <= MAX_SN;
}

}  // namespace

extern "C" long long ldc_rollout_fss_workspace_bytes(int M, int E, int S, int L, int H, int W) {
  if (!sizes_served(M, E, S, L, H, W)) return 0;
  return layout_of(E, S, L, H, W).total;
}

extern "C" int ldc_rollout_fss(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride, const float* mean,
                               const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                               long long truth_channel_stride, const int* truth_slot, const float* clim, long long clim_slot_stride,
                               long long clim_channel_stride, const int* clim_slot, const float* lat_weight, int M, int C, int L, int H, int W,
                               const ldc_events_desc* desc, const int* radii, int S, double* fss_sums, int* n_invalid, int L_total, int l_off,
                               void* workspace, long long workspace_bytes, void* stream) {
  FssArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, clim, clim_slot_stride, clim_channel_stride, clim_slot, lat_weight, M, C, L, H, W,
                       L_total, l_off) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(desc);
  LDC_CHECK_PTR(radii);
  LDC_CHECK_PTR(fss_sums);
  LDC_CHECK_PTR(n_invalid);
  LDC_CHECK_PTR(workspace);
  const int E = desc->n_events;
  if (E < 1 || E > LDC_EVENTS_MAX) return LDC_ERR_ARG;
  for (int e = 0; e < E; ++e) {
    if (desc->channel[e] < 0 || desc->channel[e] >= C) return LDC_ERR_ARG;
    if (desc->dir[e] != 1 && desc->dir[e] != -1) return LDC_ERR_ARG;
    if (desc->anomaly[e] != 0 && desc->anomaly[e] != 1) return LDC_ERR_ARG;
    if (desc->anomaly[e] == 1 && clim == nullptr) return LDC_ERR_ARG;
    if (desc->thr[e] != desc->thr[e]) return LDC_ERR_ARG;
  }
  if (S < 1 || S > LDC_FSS_SCALES_MAX) return LDC_ERR_ARG;
  for (int s = 0; s < S; ++s)
    if (radii[s] < 0 || 2ll * radii[s] + 1 > W) return LDC_ERR_ARG;  // a wider window would meet itself across the seam
  if (!sizes_served(M, E, S, L, H, W)) return LDC_ERR_UNSUPPORTED;
  if ((reinterpret_cast<uintptr_t>(workspace) & 7u) != 0 || (reinterpret_cast<uintptr_t>(fss_sums) & 7u) != 0) return LDC_ERR_ALIGN;  // fp64
  const Layout lay = layout_of(E, S, L, H, W);
  if (workspace_bytes < lay.total) return LDC_ERR_ARG;
  a.E = E; a.S = S;
  char* ws = static_cast<char*>(workspace);
  a.rec = reinterpret_cast<double*>(ws + lay.rec);
  a.rec_inv = reinterpret_cast<int*>(ws + lay.rec_inv);
  a.packed = reinterpret_cast<unsigned*>(ws + lay.packed);
  a.sat = reinterpret_cast<Sat*>(ws + lay.sat);
  a.nrec = ldc_cdiv(static_cast<long long>(H) * W, TPB);
  for (int s = 0; s < S; ++s) a.radius[s] = radii[s];
  a.d = *desc;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) launch_count<true>(a, dim3(a.nrec, E, L), s);
  else launch_count<false>(a, dim3(a.nrec, E, L), s);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(fss_rows_kernel, dim3(H, E, L), dim3(64), 0, s, a);
  if ((st = ldc_launch_status()) != LDC_OK) return st;
  hipLaunchKernelGGL(fss_cols_kernel, dim3(ldc_cdiv(W, 64), E, L), dim3(64), 0, s, a);
  if ((st = ldc_launch_status()) != LDC_OK) return st;
  hipLaunchKernelGGL(fss_window_kernel, dim3(a.nrec, E, L), dim3(TPB), 0, s, a);
  if ((st = ldc_launch_status()) != LDC_OK) return st;
  hipLaunchKernelGGL(fss_finish_kernel, dim3(E, L), dim3(128), 0, s, a.rec, a.rec_inv, a.nrec, E, S, fss_sums, n_invalid, L_total, l_off);
  return ldc_launch_status();
}
