// Verification of threshold events of a decoded ensemble: per (event, lead time) the joint histogram of "how many
// of the M members show the event" (0 .. M) against "did the truth show it" (0 / 1), counted and latitude-weighted.  It is the sufficient
// statistic of the Brier score with its reliability / resolution / uncertainty decomposition, of the reliability diagram and of the ROC
// curve (ladcast_amd/evaluate/utils.py: event_scores derives them on the host in float64).  Not in the reference.
// Addressing is that of ldc_rollout_reliability (reliability.hip): forecast by member / lead / channel strides, optional fused inverse
// normalisation (inv_norm, ensemble_common.h), truth as a table of planes with a slot per lead time, lat_weight[H], output columns at
// l_off; the optional climatology table is addressed as in ldc_rollout_scores (scoring.hip).  Grid (records, E, L): one event per
// workgroup; event e reads channel channel[e], so several events on one channel read its members once each (from cache after the first).
// Per grid point of event e, members x_i in member order after the inverse normalisation, truth t, climatology a, threshold thr:
//   u_i = x_i or x_i - a, v = t or t - a      (anomaly: one fp32 subtraction each)
//   n = #{u_i > thr} in 0 .. M, o = v > thr   (dir == -1: < in place of >)
//   bin key = 2 n + o in 0 .. 2 (M + 1) - 1: the layout [M + 1][2] of the outputs
//   the point is valid when no member, not the truth and (anomaly) not the climatology is NaN; +-inf are ordinary ordered values
// No second pass over the members, so the arms differ only in how the loads are issued: M <= 64 loads the members into registers with
// compile-time indices (arms 8 / 16 / 32 / 64) and compares then, 64 < M <= 1024 streams them.  Built with -ffp-contract=off.
// Reduction without float atomics, in a fixed order.  A workgroup covers `tpw` consecutive tiles of 256 points:
//   every thread publishes (key, w) of its point to LDS (key -1: not valid or past the plane); the tile's 256 points are walked once in
//     index order (every lane reads the same address: an LDS broadcast, no bank conflict; b128 reads, 4 points each) and thread t
//     compares each key against its bins t, t + 256, ... (at most 9 at M = 1024; slots past 2 (M + 1) are skipped by a workgroup-uniform
//     branch), keeping the count and the weight sum of each in registers across the tiles: one sequential sum over the workgroup's points
//   the invalid points: per thread, lanes by butterfly, the 4 wave totals pairwise (integers)
//   finish launch, one workgroup per (event, lead time): bin b adds the records' entries in record order, thread 0 the invalid counts.
#include <math.h>

#include "events_common.h"

namespace {

constexpr int TPB = 256;
constexpr int MAX_M = 1024;
constexpr int HEAD = 4;  // words in front of a record's bins: the invalid points (int32), 3 pad
constexpr int KB_MAX = (2 * (MAX_M + 1) + TPB - 1) / TPB;  // bins per thread of the streaming kernel: 9

// tiles per workgroup: the record grows with M (4 (M + 1) + HEAD words, twice reliability.hip's), so the tiles per record grow twice as
// fast and the workspace stays level: about half a word per point
constexpr int tiles_per_wg(int M) { return M <= 32 ? 1 : (M + 31) / 32; }
constexpr int n_bins(int M) { return 2 * (M + 1); }
constexpr int rec_words(int M) { return HEAD + 2 * n_bins(M); }

struct EvArgs {
  RolloutView v;   // clim nullptr: no anomaly event
  unsigned* part;  // [L][E][nrec][rec_words(M)]
  int E, ntile, tpw, nrec;
  ldc_events_desc d;
};

// NMAX > 0: M <= NMAX members loaded into registers before they are compared; NMAX == 0: any M, streamed (classify_event_point,
// events_common.h: the per-point classification that fss.hip shares)
template <int NMAX, bool INV, int DIR>
__device__ __forceinline__ void events_body(const EvArgs& a, int* s_key, float* s_w, int* red_i) {
  constexpr int KB = NMAX > 0 ? 1 : KB_MAX;
  const int e = blockIdx.y, l = blockIdx.z;
  const int M = a.v.M;
  const int HW = a.v.H * a.v.W;
  const int tid = threadIdx.x;
  const int c = a.d.channel[e];
  const float thr = a.d.thr[e];
  const bool anom = a.d.anomaly[e] != 0;
  const float* fbase = view_forecast(a.v, c, l);
  const float* tbase = view_truth(a.v, c, l);
  const float* cbase = anom ? view_clim(a.v, c, l) : nullptr;
  const InvNorm nrm = view_norm<INV>(a.v, c);
  const int nk = (n_bins(M) + TPB - 1) / TPB;  // bin slots per thread in use: workgroup-uniform
  int n_inv = 0;
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
    const float cl = anom ? cbase[pp] : 0.f;
    const EventPoint pt = classify_event_point<NMAX, INV, DIR>(f, a.v.fc_ms, M, t, cl, anom, thr, nrm);
    const int n = pt.n, o = pt.o;
    const bool valid = in && pt.valid;
    n_inv += (in && !valid) ? 1 : 0;
    __syncthreads();  // the walk of the tile before is over
    s_key[tid] = valid ? 2 * n + o : -1;
    s_w[tid] = w;
    __syncthreads();
#pragma unroll 2
    for (int q = 0; q < TPB; q += 4) {
      const int4 bb = *reinterpret_cast<const int4*>(&s_key[q]);
      const float4 ww = *reinterpret_cast<const float4*>(&s_w[q]);
#pragma unroll
      for (int k = 0; k < KB; ++k) {
        if (k < nk) {
          const int b = tid + k * TPB;  // a key is below 2 (M + 1): a thread whose bin lies past the last one never matches
          int cnt = hc[k];
          float ws = hw[k];
          cnt += bb.x == b ? 1 : 0;
          ws += bb.x == b ? ww.x : 0.f;
          cnt += bb.y == b ? 1 : 0;
          ws += bb.y == b ? ww.y : 0.f;
          cnt += bb.z == b ? 1 : 0;
          ws += bb.z == b ? ww.z : 0.f;
          cnt += bb.w == b ? 1 : 0;
          ws += bb.w == b ? ww.w : 0.f;
          hc[k] = cnt;
          hw[k] = ws;
        }
      }
    }
  }
  const int NB = n_bins(M);
  unsigned* rec = a.part + ((static_cast<long long>(l) * a.E + e) * a.nrec + blockIdx.x) * rec_words(M);
#pragma unroll
  for (int k = 0; k < KB; ++k) {
    const int b = tid + k * TPB;
    if (b < NB) {
      rec[HEAD + b] = static_cast<unsigned>(hc[k]);
      rec[HEAD + NB + b] = __float_as_uint(hw[k]);
    }
  }
  const int i_inv = wave_sum(n_inv);
  if ((tid & 63) == 0) red_i[tid >> 6] = i_inv;
  __syncthreads();
  if (tid == 0) rec[0] = static_cast<unsigned>((red_i[0] + red_i[1]) + (red_i[2] + red_i[3]));
  else if (tid < HEAD) rec[tid] = 0u;
}

// the direction is uniform per workgroup: one branch, two specialised bodies
template <int NMAX, bool INV>
__global__ __launch_bounds__(TPB) void events_kernel(EvArgs a) {
  __shared__ __attribute__((aligned(16))) int s_key[TPB];
  __shared__ __attribute__((aligned(16))) float s_w[TPB];
  __shared__ int red_i[4];
  if (a.d.dir[blockIdx.y] > 0) events_body<NMAX, INV, 1>(a, s_key, s_w, red_i);
  else events_body<NMAX, INV, -1>(a, s_key, s_w, red_i);
}

// One workgroup per (event, lead time): grid (E, L).  hist_count / hist_weight [E][L_total][M + 1][2]; n_invalid [E][L_total]; columns
// l_off .. l_off + L - 1.
__global__ __launch_bounds__(TPB) void events_finish_kernel(const unsigned* __restrict__ part, int nrec, int M, int E,
                                                            int* __restrict__ hist_count, float* __restrict__ hist_weight,
                                                            int* __restrict__ n_invalid, int L_total, int l_off) {
  const int e = blockIdx.x, l = blockIdx.y;
  const int RW = rec_words(M), NB = n_bins(M);
  const unsigned* base = part + (static_cast<long long>(l) * E + e) * nrec * RW;
  const long long col = static_cast<long long>(e) * L_total + l_off + l;
  for (int b = threadIdx.x; b < NB; b += TPB) {
    int cnt = 0;
    float ws = 0.f;
    for (int r = 0; r < nrec; ++r) {
      const unsigned* src = base + static_cast<long long>(r) * RW + HEAD;
      cnt += static_cast<int>(src[b]);
      ws += __uint_as_float(src[NB + b]);
    }
    hist_count[col * NB + b] = cnt;
    hist_weight[col * NB + b] = ws;
  }
  if (threadIdx.x >= 64) return;
  int k_inv = 0;
  for (int r = threadIdx.x; r < nrec; r += 64) k_inv += static_cast<int>(base[static_cast<long long>(r) * RW]);
  k_inv = wave_sum(k_inv);
  if (threadIdx.x == 0) n_invalid[col] = k_inv;
}

template <bool INV>
void launch_events(const EvArgs& a, dim3 grid, hipStream_t s) {
  ldc_dispatch_member_arm(a.v.M, [&](auto nmax) {
    hipLaunchKernelGGL((events_kernel<decltype(nmax)::value, INV>), grid, dim3(TPB), 0, s, a);
  });
}

}  // namespace

extern "C" int ldc_sizeof_events_desc(void) { return static_cast<int>(sizeof(ldc_events_desc)); }

extern "C" long long ldc_rollout_events_workspace_bytes(int M, int E, int L, int H, int W) {
  if (M <= 0 || M > MAX_M || E <= 0 || E > LDC_EVENTS_MAX || L <= 0 || L > 65535 || H <= 0 || W <= 0) return 0;
  if (static_cast<long long>(H) * W > (1ll << 24)) return 0;
  const long long ntile = (static_cast<long long>(H) * W + TPB - 1) / TPB;
  const long long nrec = (ntile + tiles_per_wg(M) - 1) / tiles_per_wg(M);
  return static_cast<long long>(L) * E * nrec * rec_words(M) * static_cast<long long>(sizeof(unsigned));
}

extern "C" int ldc_rollout_events(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                  const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                                  long long truth_channel_stride, const int* truth_slot, const float* clim, long long clim_slot_stride,
                                  long long clim_channel_stride, const int* clim_slot, const float* lat_weight, int M, int C, int L, int H,
                                  int W, const ldc_events_desc* desc, int* hist_count, float* hist_weight, int* n_invalid, int L_total,
                                  int l_off, void* workspace, long long workspace_bytes, void* stream) {
  EvArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, clim, clim_slot_stride, clim_channel_stride, clim_slot, lat_weight, M, C, L, H, W,
                       L_total, l_off) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(desc);
  LDC_CHECK_PTR(hist_count);
  LDC_CHECK_PTR(hist_weight);
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
  if (M > MAX_M || L > 65535 || static_cast<long long>(H) * W > (1ll << 24)) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < ldc_rollout_events_workspace_bytes(M, E, L, H, W)) return LDC_ERR_ARG;
  a.E = E;
  a.part = static_cast<unsigned*>(workspace);
  a.ntile = ldc_cdiv(static_cast<long long>(H) * W, TPB);
  a.tpw = tiles_per_wg(M);
  a.nrec = ldc_cdiv(a.ntile, a.tpw);
  a.d = *desc;
  dim3 grid(a.nrec, E, L);
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (mean != nullptr) launch_events<true>(a, grid, s);
  else launch_events<false>(a, grid, s);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(events_finish_kernel, dim3(E, L), dim3(TPB), 0, s, a.part, a.nrec, M, E, hist_count, hist_weight, n_invalid, L_total,
                     l_off);
  return ldc_launch_status();
}
