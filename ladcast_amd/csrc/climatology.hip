// Day-of-year climatology from raw frames (no counterpart in the reference, which reads a ready-made zarr climatology): the table
// (day of year, hour, channel, point) that evaluate_ens_gpu loads as --climatology_path, built from a stream of fp32 frames.
//   ldc_climatology_accumulate: the raw state per slot (= day * n_hours + hour) and point is the count n of the non-NaN samples (int)
//     and their sum s (fp64).  A thread owns V consecutive points of one row (V = 4: 16-byte loads of x and of count, two 16-byte
//     read-modify-writes of sum; V = 1: scalar) and walks the B frames of the batch in order: slot = slots[b] (outside [0, n_slots): the
//     frame is skipped), s[slot] += x, n[slot] += 1 where x is not NaN.  One thread, program order: two frames of a batch that share a
//     slot add in frame order, and the state after a dataset is the same bits however the frames were cut into batches.  A group of
//     values that is all NaN writes nothing.
//   ldc_climatology_smooth: clim[d] = (sum_k g_k s[(d + k) mod n_days]) / (sum_k g_k n[(d + k) mod n_days]), k = -r .. r, per hour and
//     point: the weighted mean of all samples of the window, NaN where the denominator is 0.  A workgroup of 512 threads takes a tile of
//     TILE = 32 consecutive points of one hour and stages their whole day column - n_days entries of s (8 B) and n (4 B) per point - and
//     the window's weights in LDS; every state element is read from memory exactly once per launch.  LDS: n_days * (32 * 12 + 8) =
//     n_days * 392 bytes plus 128 bytes of zero weights after the window (dynamic) and 128 bytes of counters (static): 366 days ->
//     143,728 bytes (140.4 KiB) of the CU's 160 KiB (163,840 bytes), one workgroup per CU, two waves per SIMD; the capacity is
//     (163,840 - 256) / 392 = 417 days.  A 64-point tile would need 280 KiB at 366 days; a 32-point row is 256 B of s, 128 B of n and
//     128 B of out: whole cache lines when points % 32 == 0 (production: 12 x 121 x 240 = 32 x 10890).
//     Thread (p = tid % 32, g = tid / 32) stages the days g, g + 16, ... of point p, eight days (16 loads) in flight per thread - loads
//     that each wait for their own LDS write leave a workgroup with one round trip to memory per day - and then produces the outputs
//     of point p for the day chunks g, g + 16, ... of R = 8 consecutive days: it walks the R + window - 1 input days of a chunk once
//     (one LDS read of s and n each) and feeds each into the R accumulator pairs, the R most recent weights held in registers in a ring
//     indexed statically (the loop is unrolled by R): an LDS read per 8 multiply-adds instead of one each, which would bind the kernel
//     on LDS bandwidth.  The first and the last R - 1 input days of a chunk, which only some of its outputs read, take their weights
//     from 2 (R - 1) registers loaded once per thread, so no multiply-add is predicated (a window shorter than R days runs a
//     predicated loop instead: predicating the ragged blocks of the 61-day window cost as much as all its whole blocks).  Each output sums its window in the order k = -r .. r with fma(g_k, s, acc); the quotient is rounded to fp64,
//     then once to fp32.
//     n_empty[c]: the outputs of channel c whose denominator is 0, counted per point in LDS, then one integer atomicAdd per workgroup
//     and channel.
// All arithmetic is fp64 (an fp32 value and a count are exact doubles); nothing is contracted (built with -ffp-contract=off, fma where
// written).  No float atomics: the same call sequence gives the same bits.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef int i32x4 __attribute__((ext_vector_type(4)));

constexpr int TPB = 256;

struct AccArgs {
  const float* x;
  long long sb, sc, sr;
  const int* slots;
  double* sum;   // [n_slots][C][H][W]
  int* count;    // [n_slots][C][H][W]
  long long total;  // threads with work: C * H * ceil(W / V)
  int B, C, H, W, n_slots;
};

template <int V>  // V = 4: 16-byte accesses (W % 4 == 0, aligned bases and strides), V = 1: scalar
__global__ __launch_bounds__(TPB) void climatology_accumulate_kernel(AccArgs a) {
  const long long t = static_cast<long long>(blockIdx.x) * TPB + threadIdx.x;
  if (t >= a.total) return;
  const int wv = a.W / V;
  const int w = static_cast<int>(t % wv) * V;
  const long long row = t / wv;  // c * H + h
  const int h = static_cast<int>(row % a.H);
  const long long c = row / a.H;
  const float* src = a.x + c * a.sc + h * a.sr + w;
  const long long plane = static_cast<long long>(a.C) * a.H * a.W;
  const long long off = row * a.W + w;
  for (int b = 0; b < a.B; ++b) {
    const int slot = a.slots[b];
    if (slot < 0 || slot >= a.n_slots) continue;
    double* s = a.sum + slot * plane + off;
    int* n = a.count + slot * plane + off;
    if constexpr (V == 4) {
      const f32x4 q = *reinterpret_cast<const f32x4*>(src + b * a.sb);
      const bool ok0 = q[0] == q[0], ok1 = q[1] == q[1], ok2 = q[2] == q[2], ok3 = q[3] == q[3];
      if (!(ok0 || ok1 || ok2 || ok3)) continue;
      f64x2 s0 = *reinterpret_cast<f64x2*>(s), s1 = *reinterpret_cast<f64x2*>(s + 2);
      i32x4 k = *reinterpret_cast<i32x4*>(n);
      s0[0] = ok0 ? s0[0] + static_cast<double>(q[0]) : s0[0];
      s0[1] = ok1 ? s0[1] + static_cast<double>(q[1]) : s0[1];
      s1[0] = ok2 ? s1[0] + static_cast<double>(q[2]) : s1[0];
      s1[1] = ok3 ? s1[1] + static_cast<double>(q[3]) : s1[1];
      k[0] += ok0 ? 1 : 0;
      k[1] += ok1 ? 1 : 0;
      k[2] += ok2 ? 1 : 0;
      k[3] += ok3 ? 1 : 0;
      *reinterpret_cast<f64x2*>(s) = s0;
      *reinterpret_cast<f64x2*>(s + 2) = s1;
      *reinterpret_cast<i32x4*>(n) = k;
    } else {
      const float v = src[b * a.sb];
      if (v == v) {
        *s += static_cast<double>(v);
        *n += 1;
      }
    }
  }
}

constexpr int TILE = 32;                 // points per workgroup
constexpr int SM_TPB = 512;              // two waves per SIMD: LDS latency of one hides behind the other's multiply-adds
constexpr int DGROUPS = SM_TPB / TILE;   // 16 threads per point, each on its own days
constexpr int R = 8;                     // consecutive output days per chunk (accumulators in registers)
constexpr int G_PAD = 2 * R;             // zero weights after the window: a block of R input days reads its weights unconditionally
constexpr int LDS_PER_DAY = TILE * 12 + 8;  // s, n of the tile and one weight
constexpr int LDS_FIXED = G_PAD * 8 + TILE * 4;  // the weight padding (dynamic) and the per-point empty counters (static)
constexpr int LDS_BYTES = 160 * 1024;       // per CU (and per workgroup) on gfx950
constexpr int MAX_DAYS = (LDS_BYTES - LDS_FIXED) / LDS_PER_DAY;  // 417
static_assert(MAX_DAYS >= 366, "the production year must fit");

struct SmoothArgs {
  const double* sum;
  const int* count;
  const double* weights;
  float* out;
  long long* n_empty;
  long long points, plane;
  int window, n_days, n_hours, tiles;
};

// stage days d, d + DGROUPS, ... of one point while U of them are left: all 2 U loads are issued before the first LDS write waits
template <int U>
__device__ __forceinline__ void stage_days(int& d, int n_days, const double* __restrict__ gs, const int* __restrict__ gn, long long day_stride,
                                           double* s, int* n) {
  for (; d + (U - 1) * DGROUPS < n_days; d += U * DGROUPS) {
    double sv[U];
    int nv[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      sv[u] = gs[(d + u * DGROUPS) * day_stride];
      nv[u] = gn[(d + u * DGROUPS) * day_stride];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      s[(d + u * DGROUPS) * TILE] = sv[u];
      n[(d + u * DGROUPS) * TILE] = nv[u];
    }
  }
}

// The chunk's outputs i = 0 .. R - 1 (days d0 + i) read input day jj (relative to day d0 - r) with weight g[jj - i], 0 <= jj - i < window.

// the next input day of the column: its sum and its count as doubles
__device__ __forceinline__ void next_day(int& idx, int n_days, const double* __restrict__ s, const int* __restrict__ n, double& v, double& c) {
  v = s[idx * TILE];
  c = static_cast<double>(n[idx * TILE]);
  idx = idx + 1 == n_days ? 0 : idx + 1;
}

// window < R: every multiply-add is predicated (blocks of R input days; the weight ring as in smooth_chunk)
__device__ __forceinline__ void smooth_chunk_short(int window, int n_days, int idx, const double* __restrict__ s, const int* __restrict__ n,
                                                   const double* __restrict__ g, double (&acc_s)[R], double (&acc_n)[R]) {
  double ring[R];
#pragma unroll
  for (int i = 0; i < R; ++i) ring[i] = 0.0;
  for (int q = 0; q * R < R + window - 1; ++q) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      const int jj = q * R + u;
      ring[u] = g[jj];  // zero from index window on, and never used there
      double v, c;
      next_day(idx, n_days, s, n, v, c);
#pragma unroll
      for (int i = 0; i < R; ++i) {
        if (jj - i >= 0 && jj - i < window) {
          acc_s[i] = fma(ring[(u - i + R) % R], v, acc_s[i]);  // g[jj - i], loaded i steps ago
          acc_n[i] = fma(ring[(u - i + R) % R], c, acc_n[i]);
        }
      }
    }
  }
}

// window >= R: no multiply-add is predicated.  Head, input days 0 .. R - 2: output i <= jj, weight gh[jj - i] = g[jj - i].  Middle, input
// days R - 1 .. window - 1: every output, the R most recent weights in a ring indexed statically (steps in blocks of R; the last block
// stops early).  Tail, input days window + t, t = 0 .. R - 2: output i > t, weight gt[i - t - 1] = g[window - (i - t)].
__device__ __forceinline__ void smooth_chunk(int window, int n_days, int idx, const double* __restrict__ s, const int* __restrict__ n,
                                             const double* __restrict__ g, const double (&gh)[R - 1], const double (&gt)[R - 1],
                                             double (&acc_s)[R], double (&acc_n)[R]) {
  double v, c;
#pragma unroll
  for (int u = 0; u < R - 1; ++u) {
    next_day(idx, n_days, s, n, v, c);
#pragma unroll
    for (int i = 0; i <= u; ++i) {
      acc_s[i] = fma(gh[u - i], v, acc_s[i]);
      acc_n[i] = fma(gh[u - i], c, acc_n[i]);
    }
  }
  double ring[R];  // ring[(u - i) mod R] = the weight of output i at step u of a block: ring[j] = g[j - 1] before the first block
  ring[0] = 0.0;
#pragma unroll
  for (int j = 1; j < R; ++j) ring[j] = gh[j - 1];
  const int nmid = window - (R - 1);
  int jj = R - 1;
  for (int b = 0; b < nmid / R; ++b, jj += R) {
#pragma unroll
    for (int u = 0; u < R; ++u) {
      ring[u] = g[jj + u];
      next_day(idx, n_days, s, n, v, c);
#pragma unroll
      for (int i = 0; i < R; ++i) {
        acc_s[i] = fma(ring[(u - i + R) % R], v, acc_s[i]);
        acc_n[i] = fma(ring[(u - i + R) % R], c, acc_n[i]);
      }
    }
  }
  const int left = nmid % R;
#pragma unroll
  for (int u = 0; u < R - 1; ++u) {
    if (u < left) {
      ring[u] = g[jj + u];
      next_day(idx, n_days, s, n, v, c);
#pragma unroll
      for (int i = 0; i < R; ++i) {
        acc_s[i] = fma(ring[(u - i + R) % R], v, acc_s[i]);
        acc_n[i] = fma(ring[(u - i + R) % R], c, acc_n[i]);
      }
    }
  }
#pragma unroll
  for (int t = 0; t < R - 1; ++t) {
    next_day(idx, n_days, s, n, v, c);
#pragma unroll
    for (int i = t + 1; i < R; ++i) {
      acc_s[i] = fma(gt[i - t - 1], v, acc_s[i]);
      acc_n[i] = fma(gt[i - t - 1], c, acc_n[i]);
    }
  }
}

__global__ __launch_bounds__(SM_TPB) void climatology_smooth_kernel(SmoothArgs a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char clim_smem[];
  __shared__ int empty[TILE];
  double* s = reinterpret_cast<double*>(clim_smem);                    // [n_days][TILE]
  double* g = s + static_cast<size_t>(a.n_days) * TILE;                // [n_days + G_PAD] (window used, zeros after it)
  int* n = reinterpret_cast<int*>(g + a.n_days + G_PAD);               // [n_days][TILE]
  const int tid = threadIdx.x, p = tid & (TILE - 1), dg = tid / TILE;
  const int hour = blockIdx.x / a.tiles, tile = blockIdx.x - hour * a.tiles;
  const long long p0 = static_cast<long long>(tile) * TILE;
  const bool in = p0 + p < a.points;

  const long long day_stride = a.n_hours * a.points;
  const long long base = hour * a.points + p0 + p;
  int d = dg;
  if (in) {
    stage_days<8>(d, a.n_days, a.sum + base, a.count + base, day_stride, s + p, n + p);
    stage_days<4>(d, a.n_days, a.sum + base, a.count + base, day_stride, s + p, n + p);
    stage_days<2>(d, a.n_days, a.sum + base, a.count + base, day_stride, s + p, n + p);
    stage_days<1>(d, a.n_days, a.sum + base, a.count + base, day_stride, s + p, n + p);
  } else {  // a lane past the last point computes on zeros and stores nothing
    for (; d < a.n_days; d += DGROUPS) {
      s[d * TILE + p] = 0.0;
      n[d * TILE + p] = 0;
    }
  }
  for (int k = tid; k < a.window + G_PAD; k += SM_TPB) g[k] = k < a.window ? a.weights[k] : 0.0;
  if (tid < TILE) empty[tid] = 0;
  __syncthreads();

  const int r = (a.window - 1) / 2;
  const int nchunk = (a.n_days + R - 1) / R;
  const bool longw = a.window >= R;
  double gh[R - 1], gt[R - 1];  // the first and the last R - 1 weights
#pragma unroll
  for (int m = 0; m < R - 1; ++m) {
    gh[m] = longw ? g[m] : 0.0;
    gt[m] = longw ? g[a.window - 1 - m] : 0.0;
  }
  int my_empty = 0;
  for (int chunk = dg; chunk < nchunk; chunk += DGROUPS) {
    const int d0 = chunk * R;
    int idx = d0 - r;  // > -n_days: window <= n_days
    if (idx < 0) idx += a.n_days;
    double acc_s[R], acc_n[R];
#pragma unroll
    for (int i = 0; i < R; ++i) acc_s[i] = acc_n[i] = 0.0;
    if (longw) smooth_chunk(a.window, a.n_days, idx, s + p, n + p, g, gh, gt, acc_s, acc_n);
    else smooth_chunk_short(a.window, a.n_days, idx, s + p, n + p, g, acc_s, acc_n);
#pragma unroll
    for (int i = 0; i < R; ++i) {
      const int d = d0 + i;
      if (d < a.n_days && in) {
        const bool none = acc_n[i] == 0.0;
        a.out[d * day_stride + base] = none ? NAN : static_cast<float>(acc_s[i] / acc_n[i]);
        my_empty += none ? 1 : 0;
      }
    }
  }
  if (a.n_empty == nullptr) return;
  if (my_empty != 0) atomicAdd(&empty[p], my_empty);
  __syncthreads();
  if (tid != 0) return;
  // the tile's points in order: one add per channel the tile touches
  const int np = static_cast<int>(min(static_cast<long long>(TILE), a.points - p0));
  long long c = p0 / a.plane, next = (c + 1) * a.plane - p0;  // first tile-relative point of channel c + 1
  long long run = 0;
  for (int k = 0; k < np; ++k) {
    if (k == next) {
      if (run != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.n_empty + c), static_cast<unsigned long long>(run));
      run = 0;
      ++c;
      next += a.plane;
    }
    run += empty[k];
  }
  if (run != 0) atomicAdd(reinterpret_cast<unsigned long long*>(a.n_empty + c), static_cast<unsigned long long>(run));
}

inline bool misaligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) != 0; }

constexpr long long MAX_ELEMS = 1ll << 62;

}  // namespace

extern "C" int ldc_climatology_accumulate(const float* x, long long batch_stride, long long channel_stride, long long row_stride, int B, int C,
                                          int H, int W, const int* slots, int n_slots, double* sum, int* count, void* stream) {
  LDC_CHECK_PTR(x);
  LDC_CHECK_PTR(slots);
  LDC_CHECK_PTR(sum);
  LDC_CHECK_PTR(count);
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || n_slots <= 0 || row_stride < W) return LDC_ERR_ARG;
  if (misaligned(x, 4) || misaligned(slots, 4) || misaligned(count, 4) || misaligned(sum, 8)) return LDC_ERR_ALIGN;
  const bool vec = W % 4 == 0 && ldc_aligned16(x) && ldc_aligned16(sum) && ldc_aligned16(count) && batch_stride % 4 == 0 &&
                   channel_stride % 4 == 0 && row_stride % 4 == 0;
  const long long rows = static_cast<long long>(C) * H;  // < 2^62
  if (rows > INT_MAX) return LDC_ERR_UNSUPPORTED;
  const long long total = rows * (vec ? W / 4 : W), blocks = (total + TPB - 1) / TPB;
  if (blocks > INT_MAX || rows * W > MAX_ELEMS / n_slots) return LDC_ERR_UNSUPPORTED;
  AccArgs a{x, batch_stride, channel_stride, row_stride, slots, sum, count, total, B, C, H, W, n_slots};
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(climatology_accumulate_kernel<4>, dim3(static_cast<unsigned>(blocks)), dim3(TPB), 0, s, a);
  else hipLaunchKernelGGL(climatology_accumulate_kernel<1>, dim3(static_cast<unsigned>(blocks)), dim3(TPB), 0, s, a);
  return ldc_launch_status();
}

extern "C" int ldc_climatology_smooth(const double* sum, const int* count, const double* weights, int window, int n_days, int n_hours, int C,
                                      long long plane, float* out, long long* n_empty, void* stream) {
  LDC_CHECK_PTR(sum);
  LDC_CHECK_PTR(count);
  LDC_CHECK_PTR(weights);
  LDC_CHECK_PTR(out);
  if (n_days <= 0 || n_hours <= 0 || C <= 0 || plane <= 0 || window < 1 || window % 2 == 0 || window > n_days) return LDC_ERR_ARG;
  if (misaligned(sum, 8) || misaligned(weights, 8) || misaligned(count, 4) || misaligned(out, 4) || (n_empty != nullptr && misaligned(n_empty, 8)))
    return LDC_ERR_ALIGN;
  if (n_days > MAX_DAYS || plane > MAX_ELEMS / C) return LDC_ERR_UNSUPPORTED;
  const long long points = plane * C, tiles = (points + TILE - 1) / TILE;
  if (tiles * n_hours > INT_MAX || points > MAX_ELEMS / n_days / n_hours) return LDC_ERR_UNSUPPORTED;
  static const bool attr_set = [] {  // once per process; thread-safe (C++11 static initialisation)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(climatology_smooth_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                              MAX_DAYS * LDS_PER_DAY + G_PAD * 8);
    return true;
  }();
  (void)attr_set;
  SmoothArgs a{sum, count, weights, out, n_empty, points, plane, window, n_days, n_hours, static_cast<int>(tiles)};
  hipLaunchKernelGGL(climatology_smooth_kernel, dim3(static_cast<unsigned>(tiles * n_hours)), dim3(SM_TPB), static_cast<size_t>(n_days) * LDS_PER_DAY + G_PAD * 8,
                     static_cast<hipStream_t>(stream), a);
  return ldc_launch_status();
}
