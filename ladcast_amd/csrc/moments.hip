// Dataset statistics (reference: ladcast/preprocecss/compute_mean_std_era5.py - xarray's mean / std with skipna over time and the grid -
// and the latent statistics the reference ships as a JSON without the code that made it): per channel the count, the mean and the sum of
// squared deviations from the mean (M2) of all non-NaN values of a strided fp32 batch, streamed: a call either overwrites the state or
// merges the batch into it (Chan's pairwise update), so a dataset read in batches of any size gives the statistics of the whole.
//   ldc_field_moments: every (b, c) plane is cut into chunks of at most CHUNK_POINTS values (whole rows, or pieces of one row when a row is
//     longer), one workgroup each.  A thread holds its <= 16 values in registers, so a chunk is treated by the corrected two-pass
//     algorithm at no extra traffic: pass 1 the count and the sum -> the pivot K = sum / n (the chunk's own mean, a true division, so a
//     constant chunk gives K = the value and everything after it is exactly zero); pass 2 s = sum (x - K), q = sum (x - K)^2 ->
//     mean = K + s / n, M2 = q - s^2 / n.  No division per value, and no cancellation: s is rounding residue only.
//     The record (n, mean, M2) goes to the caller's workspace, ordered [c][b][chunk].
//   A second launch, one wave per channel, merges a channel's records the same way one level up: n = sum n_i, pivot K = sum n_i mean_i / n,
//     t = sum n_i (mean_i - K), u = sum M2_i + n_i (mean_i - K)^2 -> mean = K + t / n, M2 = u - t^2 / n; lane j takes records j, j + 64, ...
//     in order, then a fixed butterfly.  One Chan update merges that into the state when accumulate is set.
// All arithmetic is fp64 (an fp32 value is an exact double); nothing is contracted (built with -ffp-contract=off, fma where written).
// No float atomics: the same call sequence gives the same bits.
#include <math.h>

#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int PER_THREAD = 16;                  // values a thread holds in registers
constexpr int CHUNK_POINTS = TPB * PER_THREAD;  // 4096 values (16 KiB) per workgroup
constexpr int NP = 4;                           // doubles per partial record: n, mean, M2, pad

struct Geometry {
  int rows;    // rows per chunk (1 when a row is cut into pieces)
  int wseg;    // columns per chunk (W, or CHUNK_POINTS when W is larger: the last piece of a row may be shorter)
  int nrc;     // chunks along H
  int ncc;     // chunks along W
  long long nchunk;  // nrc * ncc, per plane
};

inline Geometry geometry(int H, int W) {
  Geometry g;
  g.wseg = W < CHUNK_POINTS ? W : CHUNK_POINTS;
  g.rows = W < CHUNK_POINTS ? CHUNK_POINTS / W : 1;
  g.nrc = ldc_cdiv(H, g.rows);
  g.ncc = ldc_cdiv(W, g.wseg);
  g.nchunk = static_cast<long long>(g.nrc) * g.ncc;
  return g;
}

struct MomArgs {
  const float* x;
  long long sb, sc, sr;
  double* part;  // [C][B][nchunk][NP]
  int B, H, W, rows, wseg, ncc, nchunk;
};

template <int V>  // V = 4: 16-byte loads (W % 4 == 0, aligned base and strides), V = 1: scalar
__global__ __launch_bounds__(TPB) void field_moments_kernel(MomArgs a) {
  __shared__ double red1[TPB / 64][2];
  __shared__ double red2[TPB / 64][2];
  const long long idx = blockIdx.x;  // = the record index: [c][b][chunk]
  const int chunk = static_cast<int>(idx % a.nchunk);
  const long long plane = idx / a.nchunk;
  const int b = static_cast<int>(plane % a.B);
  const long long c = plane / a.B;
  const int rc = chunk / a.ncc, cc = chunk - rc * a.ncc;
  const int h0 = rc * a.rows, w0 = cc * a.wseg;
  const int nrow = min(a.rows, a.H - h0), wseg = min(a.wseg, a.W - w0);
  const int n = nrow * wseg;  // <= CHUNK_POINTS
  const float* src = a.x + b * a.sb + c * a.sc + h0 * a.sr + w0;
  const bool flat = nrow == 1 || a.sr == wseg;  // the chunk's values are contiguous

  // out-of-range slots hold NaN: skipped like the data's own
  float v[PER_THREAD];
#pragma unroll
  for (int k = 0; k < PER_THREAD / V; ++k) {
    const int i = (k * TPB + static_cast<int>(threadIdx.x)) * V;  // V == 4: wseg % 4 == 0, the four values share a row
    bool in = i < n;
    long long off = i;
    if (in && !flat) {
      const int r = i / wseg;
      off = r * a.sr + (i - r * wseg);
    }
    if constexpr (V == 4) {
      f32x4 q = {NAN, NAN, NAN, NAN};
      if (in) q = *reinterpret_cast<const f32x4*>(src + off);
#pragma unroll
      for (int j = 0; j < 4; ++j) v[4 * k + j] = q[j];
    } else {
      v[k] = in ? src[off] : NAN;
    }
  }

  // pass 1: count and sum -> the pivot
  double cnt = 0.0, sum = 0.0;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    const bool ok = v[k] == v[k];
    cnt += ok ? 1.0 : 0.0;
    sum += ok ? static_cast<double>(v[k]) : 0.0;
  }
  cnt = wave_sum(cnt);
  sum = wave_sum(sum);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red1[wave][0] = cnt;
    red1[wave][1] = sum;
  }
  __syncthreads();
  const double N = (red1[0][0] + red1[1][0]) + (red1[2][0] + red1[3][0]);  // every thread: the same four values in the same order
  const double S = (red1[0][1] + red1[1][1]) + (red1[2][1] + red1[3][1]);
  const double K = N > 0.0 ? S / N : 0.0;

  // pass 2: deviations from the pivot
  double s = 0.0, q = 0.0;
#pragma unroll
  for (int k = 0; k < PER_THREAD; ++k) {
    const bool ok = v[k] == v[k];
    const double d = ok ? static_cast<double>(v[k]) - K : 0.0;
    s += d;
    q = fma(d, d, q);
  }
  s = wave_sum(s);
  q = wave_sum(q);
  if ((threadIdx.x & 63) == 0) {
    red2[wave][0] = s;
    red2[wave][1] = q;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const double st = (red2[0][0] + red2[1][0]) + (red2[2][0] + red2[3][0]);
    const double qt = (red2[0][1] + red2[1][1]) + (red2[2][1] + red2[3][1]);
    double mean = 0.0, m2 = 0.0;  // an empty chunk: a record that adds nothing
    if (N > 0.0) {
      mean = K + st / N;
      m2 = qt - st * st / N;
      if (m2 < 0.0) m2 = 0.0;  // q >= s^2 / n up to rounding (a NaN stays)
    }
    double* rec = a.part + idx * NP;
    rec[0] = N;
    rec[1] = mean;
    rec[2] = m2;
  }
}

// one wave per channel: the channel's B * nchunk records are contiguous
__global__ __launch_bounds__(64) void field_moments_finish_kernel(const double* __restrict__ part, long long nrec, double* __restrict__ state,
                                                                  int accumulate) {
  const int c = blockIdx.x;
  const double* src = part + c * nrec * NP;
  double n = 0.0, t0 = 0.0;
  for (long long k = threadIdx.x; k < nrec; k += 64) {
    const double ni = src[k * NP];
    n += ni;
    t0 = fma(ni, src[k * NP + 1], t0);
  }
  n = wave_sum(n);
  t0 = wave_sum(t0);
  const double K = n > 0.0 ? t0 / n : 0.0;
  double t = 0.0, u = 0.0;
  for (long long k = threadIdx.x; k < nrec; k += 64) {
    const double ni = src[k * NP], d = src[k * NP + 1] - K, nd = ni * d;
    t += nd;
    u += fma(nd, d, src[k * NP + 2]);
  }
  t = wave_sum(t);
  u = wave_sum(u);
  if (threadIdx.x != 0) return;
  double mean = NAN, m2 = NAN;  // no valid value: numpy's nanmean
  if (n > 0.0) {
    mean = K + t / n;
    m2 = u - t * t / n;
    if (m2 < 0.0) m2 = 0.0;
  }
  double* st = state + 3 * c;
  if (accumulate) {
    const double na = st[0];
    if (na > 0.0) {  // anything else (0, NaN: nothing accumulated yet) is replaced by the batch
      if (!(n > 0.0)) return;
      const double ma = st[1], tot = na + n, delta = mean - ma;
      mean = ma + delta * (n / tot);
      m2 = (st[2] + m2) + delta * delta * (na * (n / tot));
      n = tot;
    }
  }
  st[0] = n;
  st[1] = mean;
  st[2] = m2;
}

constexpr long long MAX_RECORDS = (1ll << 24) - 1;  // grid.x * TPB threads of the first launch stay below 2^32

// total records, or -1 when the launch geometry cannot hold them
inline long long record_count(int B, int C, int H, int W) {
  const long long per_plane = geometry(H, W).nchunk;  // < 2^62
  if (per_plane > MAX_RECORDS) return -1;
  const long long per_channel = per_plane * B;
  if (per_channel > MAX_RECORDS || per_channel * C > MAX_RECORDS) return -1;
  return per_channel * C;
}

}  // namespace

extern "C" long long ldc_field_moments_workspace_bytes(int B, int C, int H, int W) {
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0) return 0;
  const long long nrec = record_count(B, C, H, W);
  return nrec < 0 ? 0 : nrec * NP * static_cast<long long>(sizeof(double));
}

extern "C" int ldc_field_moments(const float* x, long long batch_stride, long long channel_stride, long long row_stride, int B, int C, int H,
                                 int W, double* state, int accumulate, void* workspace, long long workspace_bytes, void* stream) {
  LDC_CHECK_PTR(x);
  LDC_CHECK_PTR(state);
  LDC_CHECK_PTR(workspace);
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || row_stride < W) return LDC_ERR_ARG;
  const long long nrec = record_count(B, C, H, W);
  if (nrec < 0) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < nrec * NP * static_cast<long long>(sizeof(double))) return LDC_ERR_ARG;
  LDC_CHECK_ALIGN16(workspace);
  if ((reinterpret_cast<uintptr_t>(state) & 7u) != 0 || (reinterpret_cast<uintptr_t>(x) & 3u) != 0) return LDC_ERR_ALIGN;
  const Geometry g = geometry(H, W);
  MomArgs a{x, batch_stride, channel_stride, row_stride, static_cast<double*>(workspace), B, H, W, g.rows, g.wseg, g.ncc, static_cast<int>(g.nchunk)};
  const bool vec = W % 4 == 0 && ldc_aligned16(x) && batch_stride % 4 == 0 && channel_stride % 4 == 0 && row_stride % 4 == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(field_moments_kernel<4>, dim3(static_cast<unsigned>(nrec)), dim3(TPB), 0, s, a);
  else hipLaunchKernelGGL(field_moments_kernel<1>, dim3(static_cast<unsigned>(nrec)), dim3(TPB), 0, s, a);
  const int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(field_moments_finish_kernel, dim3(C), dim3(64), 0, s, a.part, nrec / C, state, accumulate);
  return ldc_launch_status();
}
