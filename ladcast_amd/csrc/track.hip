// Tropical-cyclone tracking on decoded fields (evaluate/track.py:151-335 of the reference): the channel gather with the inverse
// normalisation of decode_latent_ens, the ensemble nanmean, and the local-minimum tracker itself.
// Built with -ffp-contract=off: the gather must round as chan_affine does, the coordinate arithmetic as Python's float ops do.
#include <math.h>

#include "common.h"

namespace {

constexpr int kWave = 64;

struct ldc_track_channels {  // launch argument: the gathered channels
  int n;
  int idx[LDC_TRACK_MAX_CHANNELS];
};
struct ldc_track_boxes {  // launch argument: inner_box_sizes
  int n;
  int inner[LDC_TRACK_MAX_BOXES];
};

// out[b][t_off + t][k][p] = (x[b*sb + t*st + ch[k]*sc + p] / target_std) * sd[ch[k]] + mean[ch[k]]: chan_affine_kernel's inverse,
// same operations in the same order (layout.hip), on the channels the tracker reads only
__global__ __launch_bounds__(256) void track_gather_kernel(const float* __restrict__ x, long long sb, long long st, long long sc,
                                                           ldc_track_channels ch, const float* __restrict__ mean,
                                                           const float* __restrict__ sd, float target_std, float* __restrict__ out,
                                                           int T, int T_total, int t_off, long long HW) {
  const long long p = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (p >= HW) return;
  const int k = blockIdx.y % ch.n, t = blockIdx.y / ch.n, b = blockIdx.z;
  const int c = ch.idx[k];
  const float v = x[b * sb + t * st + c * sc + p];
  out[((static_cast<long long>(b) * T_total + t_off + t) * ch.n + k) * HW + p] = (v / target_std) * sd[c] + mean[c];
}

// np.nanmean(x, axis=0) on float32: NaNs replaced by +0, summed in member order starting from member 0, divided by the count
// (numpy divides in float64 and casts back; for two fp32 operands that double rounding equals the fp32 division)
__global__ __launch_bounds__(256) void track_nanmean_kernel(const float* __restrict__ x, long long member_stride, int E, long long n,
                                                            float* __restrict__ out) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  float acc = 0.f;
  int cnt = 0;
  for (int e = 0; e < E; ++e) {
    const float v = x[e * member_stride + i];
    const bool ok = !isnan(v);
    const float w = ok ? v : 0.f;
    acc = e == 0 ? w : acc + w;
    cnt += ok;
  }
  out[i] = acc / static_cast<float>(cnt);
}

// ---- tracker --------------------------------------------------------------------------------------------------------------
// Python's float `%` (CPython float_rem): fmod, then the sign of the divisor; a zero remainder becomes +0.0 for m > 0
__device__ __forceinline__ double py_mod(double x, double m) {
  double r = fmod(x, m);
  if (r != 0.0) {
    if ((m < 0.0) != (r < 0.0)) r += m;
  } else {
    r = copysign(0.0, m);
  }
  return r;
}

// c ascending: number of entries with c[i] < x (= first i with c[i] >= x), and number with c[i] <= x
__device__ __forceinline__ int count_lt(const double* c, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid] >= x) hi = mid; else lo = mid + 1;
  }
  return lo;
}
__device__ __forceinline__ int count_le(const double* c, int n, double x) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (c[mid] <= x) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// select_box as index ranges: rows [r0, r0 + nr); columns [a0, a0 + na) then [b0, b0 + nb), in ascending coordinate order (the
// order where(..., drop=True) keeps).  Bounds are found by comparing against the coordinate arrays, as the masks do.
struct Box {
  int r0, nr, a0, na, b0, nb;
  __device__ int ncols() const { return na + nb; }
  __device__ int col(int k) const { return k < na ? a0 + k : b0 + (k - na); }
};

__device__ __forceinline__ Box select_box(const double* lat, int H, const double* lon, int W, double lat_lo, double lat_hi,
                                          double lon_s, double lon_e) {
  Box b;
  const double mn = lat_hi < lat_lo ? lat_hi : lat_lo, mx = lat_hi > lat_lo ? lat_hi : lat_lo;  // Python min / max
  b.r0 = count_lt(lat, H, mn);
  b.nr = max(count_le(lat, H, mx) - b.r0, 0);
  if (lon_s <= lon_e) {  // lon_s <= lon <= lon_e
    b.a0 = count_lt(lon, W, lon_s);
    b.na = max(count_le(lon, W, lon_e) - b.a0, 0);
    b.b0 = 0;
    b.nb = 0;
  } else {  // lon >= lon_s or lon <= lon_e: the small longitudes first
    b.a0 = 0;
    b.na = count_le(lon, W, lon_e);
    b.b0 = count_lt(lon, W, lon_s);
    b.nb = W - b.b0;
  }
  return b;
}

// pandas Index.get_indexer(method="nearest") on an ascending index: pad / backfill neighbours, the left one only when strictly
// closer (or when there is no right one); index -1 reads the last entry as numpy does
__device__ __forceinline__ int nearest(const double* c, int n, double x) {
  const int pad = count_le(c, n, x) - 1;
  int bf = count_lt(c, n, x);
  if (bf == n) bf = -1;
  const double ld = fabs(c[pad < 0 ? n - 1 : pad] - x), rd = fabs(c[bf < 0 ? n - 1 : bf] - x);
  const int i = (ld < rd || bf == -1) ? pad : bf;
  return i < 0 ? 0 : i;
}

struct MinResult {
  int found;
  double la, lo;
  float v;
};

// find_local_minimum (track.py:173-238) by one wave: one candidate per lane (looping when the outer box holds more than 64), each
// lane scans its candidate's neighbourhood from global memory, a wave reduction on (distance key, visiting index) picks the winner
// (Python's min keeps the first of equal keys).  Every lane returns the same result.
__device__ MinResult find_local_min(const float* __restrict__ f, const double* lat, int H, const double* lon, int W, double lat0,
                                    double lon0, int inner) {
  const int lane = threadIdx.x;
  const double outer = static_cast<double>(inner) + 3.0;  // inner_deg + NEIGHBOR_DEG * 2
  const double half_o = outer / 2.0, half_i = static_cast<double>(inner) / 2.0;
  const double lat_lo = lat0 - half_o, lat_hi = lat0 + half_o;
  const double lon_s = py_mod(lon0 - half_o, 360.0), lon_e = py_mod(lon0 + half_o, 360.0);
  const Box ob = select_box(lat, H, lon, W, lat_lo, lat_hi, lon_s, lon_e);
  const int nc = ob.ncols(), n = ob.nr * nc;
  double best_key = INFINITY;
  int best_q = 0x7fffffff;
  for (int q = lane; q < n; q += kWave) {
    const int r = ob.r0 + q / nc, c = ob.col(q % nc);
    const double la = lat[r], lo = lon[c];
    const float v = f[static_cast<long long>(r) * W + c];
    if (isnan(v)) continue;  // NaN == min is never true
    const Box nb = select_box(lat, H, lon, W, la - half_i, la + half_i, py_mod(lo - half_i, 360.0), py_mod(lo + half_i, 360.0));
    const int nnc = nb.ncols();
    if (nb.nr * nnc == 0) continue;
    float m = NAN;  // .min() skips NaN
    for (int i = 0; i < nb.nr; ++i) {
      const float* row = f + static_cast<long long>(nb.r0 + i) * W;
      for (int k = 0; k < nnc; ++k) {
        const float u = row[nb.col(k)];
        if (!isnan(u) && (isnan(m) || u < m)) m = u;
      }
    }
    if (!(v == m)) continue;
    // edge points (track.py:220-229), literally: one-sided longitude tests
    if (fabs(la - lat_lo) < 1e-6 || fabs(la - lat_hi) < 1e-6 || fabs(py_mod(lo - lon_s, 360.0)) < 1e-6 ||
        fabs(py_mod(lo - lon_e, 360.0)) < 1e-6)
      continue;
    // (la - lat0)**2 + ((lo - lon0 + 180) % 360 - 180)**2 as d * d, each product correctly rounded.  On the default grid every
    // difference is a multiple of 0.5 whose square is exact, so d * d equals CPython's pow(d, 2); the same holds on any dyadic
    // grid and centre.  Elsewhere pow(d, 2) may differ from d * d by one rounding per term (ladcast_hip.h states the contract)
    const double dla = la - lat0, dlo = py_mod(lo - lon0 + 180.0, 360.0) - 180.0;
    const double key = dla * dla + dlo * dlo;
    if (key < best_key) {  // q grows per lane: the first of equal keys stays
      best_key = key;
      best_q = q;
    }
  }
#pragma unroll
  for (int off = kWave / 2; off > 0; off >>= 1) {
    const double ok = __shfl_xor(best_key, off);
    const int oq = __shfl_xor(best_q, off);
    if (ok < best_key || (ok == best_key && oq < best_q)) {
      best_key = ok;
      best_q = oq;
    }
  }
  MinResult res;
  res.found = best_q != 0x7fffffff;
  res.la = res.lo = 0.0;
  res.v = 0.f;
  if (res.found) {
    const int r = ob.r0 + best_q / nc, c = ob.col(best_q % nc);
    res.la = lat[r];
    res.lo = lon[c];
    res.v = f[static_cast<long long>(r) * W + c];
  }
  return res;
}

__device__ __forceinline__ void load_grid(double* s_lat, double* s_lon, const double* glat, int H, const double* glon, int W) {
  for (int i = threadIdx.x; i < H; i += kWave) s_lat[i] = glat[i];
  for (int i = threadIdx.x; i < W; i += kWave) s_lon[i] = glon[i];
  __syncthreads();
}

// track_first_n_steps (track.py:243-335): one workgroup (one wave) per track, every step and every inner box size in the kernel
__global__ __launch_bounds__(kWave) void track_kernel(const float* __restrict__ fields, long long track_stride, long long frame_stride,
                                                      long long mslp_off, long long z_off, const float* __restrict__ lsm,
                                                      const double* __restrict__ glat, int H, const double* __restrict__ glon, int W,
                                                      const double* __restrict__ lat0, const double* __restrict__ lon0, int n_steps,
                                                      ldc_track_boxes boxes, int enforce_msl, double* __restrict__ out_lat,
                                                      double* __restrict__ out_lon, int* __restrict__ out_code) {
  __shared__ double s_lat[LDC_TRACK_MAX_GRID], s_lon[LDC_TRACK_MAX_GRID];
  load_grid(s_lat, s_lon, glat, H, glon, W);
  const int e = blockIdx.x;
  const float* base = fields + e * track_stride;
  double cla = lat0[e], clo = lon0[e];
  const long long o = static_cast<long long>(e) * (n_steps + 1);
  if (threadIdx.x == 0) {
    out_lat[o] = cla;
    out_lon[o] = clo;
  }
  for (int step = 1; step <= n_steps; ++step) {
    const double pla = cla, plo = clo;
    const float* frame = base + step * frame_stride;
    int code = 0;
    float mval = 0.f;
    if (!enforce_msl) mval = lsm[static_cast<long long>(nearest(s_lat, H, cla)) * W + nearest(s_lon, W, clo)];
    if (mval < 0.5f) {
      for (int k = 0; k < boxes.n && !code; ++k) {
        const MinResult r = find_local_min(frame + mslp_off, s_lat, H, s_lon, W, cla, clo, boxes.inner[k]);
        if (r.found && (pla != r.la || plo != r.lo)) {
          cla = r.la;
          clo = r.lo;
          code = 1 + k;
        }
      }
    }
    if (!code && !enforce_msl) {
      for (int k = 0; k < boxes.n && !code; ++k) {
        const MinResult r = find_local_min(frame + z_off, s_lat, H, s_lon, W, cla, clo, boxes.inner[k]);
        if (r.found && (pla != r.la || plo != r.lo)) {
          cla = r.la;
          clo = r.lo;
          code = 1 + boxes.n + k;
        }
      }
    }
    if (threadIdx.x == 0) {
      out_lat[o + step] = cla;
      out_lon[o + step] = clo;
      out_code[static_cast<long long>(e) * n_steps + step - 1] = code;
    }
  }
}

// a batch of single find_local_minimum calls: query q searches fields + field_idx[q] * field_stride around (lat0[q], lon0[q])
__global__ __launch_bounds__(kWave) void track_query_kernel(const float* __restrict__ fields, long long field_stride,
                                                            const int* __restrict__ field_idx, const double* __restrict__ glat, int H,
                                                            const double* __restrict__ glon, int W, const double* __restrict__ lat0,
                                                            const double* __restrict__ lon0, const int* __restrict__ inner,
                                                            int* __restrict__ found, double* __restrict__ out_la,
                                                            double* __restrict__ out_lo, float* __restrict__ out_v) {
  __shared__ double s_lat[LDC_TRACK_MAX_GRID], s_lon[LDC_TRACK_MAX_GRID];
  load_grid(s_lat, s_lon, glat, H, glon, W);
  const int q = blockIdx.x;
  if (inner[q] < 0 || inner[q] > LDC_TRACK_MAX_INNER) {  // the host binding refuses these before launch; never searched
    if (threadIdx.x == 0) found[q] = LDC_ERR_UNSUPPORTED;
    return;
  }
  const MinResult r = find_local_min(fields + field_idx[q] * field_stride, s_lat, H, s_lon, W, lat0[q], lon0[q], inner[q]);
  if (threadIdx.x == 0) {
    found[q] = r.found;
    out_la[q] = r.la;
    out_lo[q] = r.lo;
    out_v[q] = r.v;
  }
}

int check_grid(const double* glat, int H, const double* glon, int W) {
  LDC_CHECK_PTR(glat);
  LDC_CHECK_PTR(glon);
  if (H <= 0 || W <= 0) return LDC_ERR_ARG;
  if (H > LDC_TRACK_MAX_GRID || W > LDC_TRACK_MAX_GRID) return LDC_ERR_UNSUPPORTED;
  return LDC_OK;
}

}  // namespace

extern "C" int ldc_track_gather(const float* x, long long sb, long long st, long long sc, int B, int T, long long HW,
                                const int* channels, int n_ch, const float* mean, const float* std_, float target_std, float* out,
                                int T_total, int t_off, void* stream) {
  LDC_CHECK_PTR(x);
  LDC_CHECK_PTR(channels);
  LDC_CHECK_PTR(mean);
  LDC_CHECK_PTR(std_);
  LDC_CHECK_PTR(out);
  if (B <= 0 || T <= 0 || HW <= 0 || n_ch <= 0 || t_off < 0 || t_off + T > T_total) return LDC_ERR_ARG;
  // grid.y = T * n_ch and grid.z = B are limited to 65535 by the launch
  if (n_ch > LDC_TRACK_MAX_CHANNELS || B > 65535 || static_cast<long long>(T) * n_ch > 65535) return LDC_ERR_UNSUPPORTED;
  ldc_track_channels ch;
  ch.n = n_ch;
  for (int k = 0; k < LDC_TRACK_MAX_CHANNELS; ++k) ch.idx[k] = k < n_ch ? channels[k] : 0;
  for (int k = 0; k < n_ch; ++k)
    if (ch.idx[k] < 0) return LDC_ERR_ARG;
  hipLaunchKernelGGL(track_gather_kernel, dim3(ldc_cdiv(HW, 256), T * n_ch, B), dim3(256), 0, static_cast<hipStream_t>(stream), x,
                     sb, st, sc, ch, mean, std_, target_std, out, T, T_total, t_off, HW);
  return ldc_launch_status();
}

extern "C" int ldc_track_nanmean(const float* x, long long member_stride, int E, long long n, float* out, void* stream) {
  LDC_CHECK_PTR(x);
  LDC_CHECK_PTR(out);
  if (E <= 0 || n <= 0 || member_stride < 0) return LDC_ERR_ARG;
  hipLaunchKernelGGL(track_nanmean_kernel, dim3(ldc_cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), x, member_stride,
                     E, n, out);
  return ldc_launch_status();
}

extern "C" int ldc_track_storms(const float* fields, long long track_stride, long long frame_stride, long long mslp_off,
                                long long z_off, const float* lsm, const double* lat, int H, const double* lon, int W,
                                const double* lat0, const double* lon0, int n_tracks, int n_steps, const int* inner_box_sizes,
                                int n_boxes, int enforce_msl, double* out_lat, double* out_lon, int* out_code, void* stream) {
  LDC_CHECK_PTR(fields);
  LDC_CHECK_PTR(lat0);
  LDC_CHECK_PTR(lon0);
  LDC_CHECK_PTR(inner_box_sizes);
  LDC_CHECK_PTR(out_lat);
  LDC_CHECK_PTR(out_lon);
  const int g = check_grid(lat, H, lon, W);
  if (g != LDC_OK) return g;
  if (n_tracks <= 0 || n_steps < 0 || n_boxes <= 0) return LDC_ERR_ARG;
  if (n_steps > 0 && out_code == nullptr) return LDC_ERR_ARG;
  if (!enforce_msl && (lsm == nullptr || z_off < 0)) return LDC_ERR_ARG;
  if (n_boxes > LDC_TRACK_MAX_BOXES) return LDC_ERR_UNSUPPORTED;
  ldc_track_boxes boxes;
  boxes.n = n_boxes;
  for (int k = 0; k < LDC_TRACK_MAX_BOXES; ++k) boxes.inner[k] = k < n_boxes ? inner_box_sizes[k] : 0;
  for (int k = 0; k < n_boxes; ++k) {
    if (boxes.inner[k] < 0) return LDC_ERR_ARG;
    if (boxes.inner[k] > LDC_TRACK_MAX_INNER) return LDC_ERR_UNSUPPORTED;
  }
  hipLaunchKernelGGL(track_kernel, dim3(n_tracks), dim3(kWave), 0, static_cast<hipStream_t>(stream), fields, track_stride, frame_stride,
                     mslp_off, z_off, lsm, lat, H, lon, W, lat0, lon0, n_steps, boxes, enforce_msl ? 1 : 0, out_lat, out_lon, out_code);
  return ldc_launch_status();
}

extern "C" int ldc_track_local_min(const float* fields, long long field_stride, const int* field_idx, const double* lat, int H,
                                   const double* lon, int W, const double* lat0, const double* lon0, const int* inner, int n_queries,
                                   int* found, double* out_lat, double* out_lon, float* out_val, void* stream) {
  LDC_CHECK_PTR(fields);
  LDC_CHECK_PTR(field_idx);
  LDC_CHECK_PTR(lat0);
  LDC_CHECK_PTR(lon0);
  LDC_CHECK_PTR(inner);
  LDC_CHECK_PTR(found);
  LDC_CHECK_PTR(out_lat);
  LDC_CHECK_PTR(out_lon);
  LDC_CHECK_PTR(out_val);
  const int g = check_grid(lat, H, lon, W);
  if (g != LDC_OK) return g;
  if (n_queries <= 0) return LDC_ERR_ARG;
  hipLaunchKernelGGL(track_query_kernel, dim3(n_queries), dim3(kWave), 0, static_cast<hipStream_t>(stream), fields, field_stride,
                     field_idx, lat, H, lon, W, lat0, lon0, inner, found, out_lat, out_lon, out_val);
  return ldc_launch_status();
}
