// Paired block-bootstrap comparison of two scored rollouts (no counterpart in the reference): a, b hold the scores of two runs at N
// paired initial times for K series (element (i, k) at i * ld + k); draws holds R replicates of D resampled initial times.  Per series:
// the point estimates of both runs, of their difference and of their ratio, percentile intervals of the difference and of the ratio
// over the replicates, and the sign counts a two-sided p-value is made of (include/ladcast_hip.h states every definition).
//
// Three launches behind one memset:
//   bootstrap_weights_kernel: draws -> multiplicities.  Wt[i][r] (int, [N][RS], RS = R + 1 rounded up to 4) = how often replicate r
//     drew initial time i: one integer atomicAdd per draw into the zeroed table (integers: the order does not matter).  Column R is all
//     ones - the "replicate" that takes every pair once - so the point estimates come out of the same product as the replicates.
//   bootstrap_sums_kernel: the replicate sums are the matrix product Wt^T . X with X = (a, b, 1) where the pair is valid and (0, 0, 0)
//     where it is not.  A workgroup of 256 threads owns a tile of 64 replicates x 64 series and walks the initial times in chunks of
//     16: the chunk of Wt (64 consecutive ints per time: whole 256-byte rows) and of a / b (64 consecutive floats per time) is staged
//     in LDS as doubles (4 x 8 KiB), so every staged row of X is reused by 64 replicates and every row of Wt by 64 series - a gather
//     that walks draws per series moves R * D * K values with no reuse at all.  Thread (tr = tid % 16, tk = tid / 16) holds the
//     4 x 4 register tile of replicates 4 tr .. 4 tr + 3 and series 4 tk .. 4 tk + 3: three fp64 accumulators each (sum of a, sum of b,
//     valid draws), 16 LDS doubles read per 48 fused multiply-adds.  A multiplicity times an fp32 value is exact in fp64, so fma gives
//     the bits of multiply-then-add.  The sums go out series-major ([K][RS]: 16 lanes write 512 contiguous bytes of a series), the
//     count as int.  32 KiB of LDS, 148 VGPRs and 4 waves per workgroup: three workgroups per CU hide each other's staging.
//   bootstrap_select_kernel: one workgroup of 1024 threads per series reads its R sums contiguously, forms theta (S / m, or its square
//     root) of both runs, d* = b* - a* and q* = b* / a*, counts the used replicates and the signs of d*, and sorts first the finite d*
//     and then the finite q* in LDS: a bitonic network over P = the power of two >= R keys of 8 bytes (R <= 16384: 128 KiB of the
//     CU's 160 KiB), the doubles mapped to integers whose order is the doubles' (and -0 < +0, so the selected bits do not depend on
//     the network); the values left out sort last.  The two ranks are read straight from the sorted keys.
// All arithmetic is fp64 with the default, correctly rounded division and square root; nothing is contracted (built with
// -ffp-contract=off, fma where written).  No float atomics: the same inputs give the same bits.
#include <limits.h>
#include <math.h>

#include "common.h"

namespace {

constexpr int MAX_R = 16384;            // keys of one series in LDS: 128 KiB
constexpr int TR = 64, TK = 64, TI = 16;  // tile of the product: replicates x series, initial times per staged chunk
constexpr int SUMS_TPB = 256;
constexpr int RR = 4, RK = 4;           // register tile per thread
static_assert((TR / RR) * (TK / RK) == SUMS_TPB, "one register tile per thread");
constexpr int SEL_TPB = 1024;
constexpr int W_TPB = 256;
constexpr long long KEY_LAST = LLONG_MAX;  // a replicate that is left out: after every finite value

struct Layout {  // of the workspace
  long long rs;      // row stride of Wt and of the sums: R + 1 rounded up to 4
  long long off_sa, off_sb, off_m, bytes;
};

inline Layout layout(int N, int K, int R) {
  Layout l;
  l.rs = (static_cast<long long>(R) + 1 + 3) / 4 * 4;
  const long long w_bytes = (static_cast<long long>(N) * l.rs * 4 + 255) / 256 * 256;
  const long long s_bytes = static_cast<long long>(K) * l.rs * 8;  // a multiple of 32
  l.off_sa = w_bytes;
  l.off_sb = l.off_sa + s_bytes;
  l.off_m = l.off_sb + s_bytes;
  l.bytes = l.off_m + static_cast<long long>(K) * l.rs * 4;
  return l;
}

struct WeightArgs {
  const int* draws;
  int* wt;
  long long rs, total;  // total = R * D
  int N, R, D;
};

__global__ __launch_bounds__(W_TPB) void bootstrap_weights_kernel(WeightArgs a) {
  const long long t = static_cast<long long>(blockIdx.x) * W_TPB + threadIdx.x;
  if (t < a.total) {
    const int r = static_cast<int>(t / a.D);
    const int i = a.draws[t];  // in [0, N) by the caller's contract; anything else is dropped, never written through
    if (static_cast<unsigned>(i) < static_cast<unsigned>(a.N)) atomicAdd(a.wt + i * a.rs + r, 1);
  }
  if (t < a.N) a.wt[t * a.rs + a.R] = 1;  // nobody else writes column R
}

struct SumArgs {
  const float* a;
  const float* b;
  const int* wt;
  double* sa;
  double* sb;
  int* m;
  long long ld, rs;
  int N, K, RT;  // RT = R + 1 columns of Wt in use
};

__global__ __launch_bounds__(SUMS_TPB) void bootstrap_sums_kernel(SumArgs g) {
  __shared__ __attribute__((aligned(16))) double ws[TI][TR];
  __shared__ __attribute__((aligned(16))) double xa[TI][TK];
  __shared__ __attribute__((aligned(16))) double xb[TI][TK];
  __shared__ __attribute__((aligned(16))) double xv[TI][TK];
  const int tid = threadIdx.x;
  const long long k0 = static_cast<long long>(blockIdx.x) * TK;
  const int r0 = blockIdx.y * TR;
  const int tr = tid % (TR / RR), tk = tid / (TR / RR);
  // staging: thread -> column c of rows i0 + q, q = tid / 64 + 4 u
  const int sc = tid % 64, sq = tid / 64;
  const bool r_in = r0 + sc < g.RT, k_in = k0 + sc < g.K;

  double acc_a[RR][RK], acc_b[RR][RK], acc_v[RR][RK];
#pragma unroll
  for (int p = 0; p < RR; ++p)
#pragma unroll
    for (int q = 0; q < RK; ++q) acc_a[p][q] = acc_b[p][q] = acc_v[p][q] = 0.0;

  for (int i0 = 0; i0 < g.N; i0 += TI) {
    int wv[TI / 4];
    float av[TI / 4], bv[TI / 4];
    bool ok[TI / 4];
#pragma unroll
    for (int u = 0; u < TI / 4; ++u) {
      const int i = i0 + sq + 4 * u;
      const bool i_in = i < g.N;
      wv[u] = (i_in && r_in) ? g.wt[i * g.rs + r0 + sc] : 0;
      ok[u] = i_in && k_in;
      av[u] = ok[u] ? g.a[i * g.ld + k0 + sc] : 0.f;
      bv[u] = ok[u] ? g.b[i * g.ld + k0 + sc] : 0.f;
    }
    __syncthreads();  // the previous chunk has been read
#pragma unroll
    for (int u = 0; u < TI / 4; ++u) {
      const int q = sq + 4 * u;
      const bool valid = ok[u] && isfinite(av[u]) && isfinite(bv[u]);
      ws[q][sc] = static_cast<double>(wv[u]);
      xa[q][sc] = valid ? static_cast<double>(av[u]) : 0.0;
      xb[q][sc] = valid ? static_cast<double>(bv[u]) : 0.0;
      xv[q][sc] = valid ? 1.0 : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int q = 0; q < TI; ++q) {
      double w[RR], va[RK], vb[RK], vv[RK];
#pragma unroll
      for (int p = 0; p < RR; ++p) w[p] = ws[q][RR * tr + p];
#pragma unroll
      for (int s = 0; s < RK; ++s) {
        va[s] = xa[q][RK * tk + s];
        vb[s] = xb[q][RK * tk + s];
        vv[s] = xv[q][RK * tk + s];
      }
#pragma unroll
      for (int p = 0; p < RR; ++p)
#pragma unroll
        for (int s = 0; s < RK; ++s) {
          acc_a[p][s] = fma(w[p], va[s], acc_a[p][s]);
          acc_b[p][s] = fma(w[p], vb[s], acc_b[p][s]);
          acc_v[p][s] = fma(w[p], vv[s], acc_v[p][s]);
        }
    }
  }
#pragma unroll
  for (int s = 0; s < RK; ++s) {
    const long long k = k0 + RK * tk + s;
    if (k >= g.K) continue;
#pragma unroll
    for (int p = 0; p < RR; ++p) {
      const int r = r0 + RR * tr + p;
      if (r >= g.RT) continue;
      g.sa[k * g.rs + r] = acc_a[p][s];
      g.sb[k * g.rs + r] = acc_b[p][s];
      g.m[k * g.rs + r] = static_cast<int>(acc_v[p][s]);  // an exact integer <= D
    }
  }
}

// doubles -> integers of the same order (IEEE totalOrder: -0 before +0), and back
__device__ __forceinline__ long long order_key(double x) {
  const long long u = __double_as_longlong(x);
  return u ^ ((u >> 63) & LLONG_MAX);
}
__device__ __forceinline__ double key_value(long long k) { return __longlong_as_double(k ^ ((k >> 63) & LLONG_MAX)); }

__device__ __forceinline__ double theta(double s, int m, int kind) {
  const double mean = s / static_cast<double>(m);
  return kind == 1 ? sqrt(mean) : mean;
}

// ascending bitonic network over the P keys (P a power of two); ends with a barrier
__device__ __forceinline__ void sort_keys(long long* keys, int P, int tid) {
  __syncthreads();
  for (int k2 = 2; k2 <= P; k2 <<= 1) {
    for (int j = k2 >> 1; j > 0; j >>= 1) {
      for (int t = tid; t < P / 2; t += SEL_TPB) {
        const int i = 2 * t - (t & (j - 1));  // bit j of i is clear
        const int l = i + j;
        const long long x = keys[i], y = keys[l];
        if ((x > y) == ((i & k2) == 0)) {
          keys[i] = y;
          keys[l] = x;
        }
      }
      __syncthreads();
    }
  }
}

struct SelectArgs {
  const double* sa;
  const double* sb;
  const int* m;
  double* stats;
  int* counts;
  long long rs;
  int R, P, kind, tail_ppm;
};

__global__ __launch_bounds__(SEL_TPB) void bootstrap_select_kernel(SelectArgs g) {
  extern __shared__ __attribute__((aligned(16))) unsigned char boot_smem[];
  __shared__ int cnt[4];  // n_used, n_le0, n_ge0, finite ratios
  long long* keys = reinterpret_cast<long long*>(boot_smem);
  const int tid = threadIdx.x;
  const long long row = static_cast<long long>(blockIdx.x) * g.rs;
  const double* sa = g.sa + row;
  const double* sb = g.sb + row;
  const int* m = g.m + row;
  if (tid < 4) cnt[tid] = 0;
  __syncthreads();

  double lohi[4];
  for (int pass = 0; pass < 2; ++pass) {  // 0: the differences, 1: the ratios
    int used = 0, le0 = 0, ge0 = 0;
    for (int r = tid; r < g.P; r += SEL_TPB) {
      long long key = KEY_LAST;
      const int mr = r < g.R ? m[r] : 0;
      if (mr > 0) {
        const double as = theta(sa[r], mr, g.kind), bs = theta(sb[r], mr, g.kind);
        const double v = pass == 0 ? bs - as : bs / as;
        if (isfinite(v)) {
          key = order_key(v);
          ++used;
          le0 += v <= 0.0 ? 1 : 0;
          ge0 += v >= 0.0 ? 1 : 0;
        }
      }
      keys[r] = key;
    }
    used = wave_sum(used);
    le0 = wave_sum(le0);
    ge0 = wave_sum(ge0);
    if ((tid & 63) == 0) {  // integers: the order of the adds does not matter
      if (pass == 0) {
        atomicAdd(&cnt[0], used);
        atomicAdd(&cnt[1], le0);
        atomicAdd(&cnt[2], ge0);
      } else {
        atomicAdd(&cnt[3], used);
      }
    }
    sort_keys(keys, g.P, tid);  // its first barrier publishes keys and cnt
    const int n = cnt[pass == 0 ? 0 : 3];
    if (n > 0) {
      const int lo = static_cast<int>(static_cast<long long>(g.tail_ppm) * n / 1000000);
      lohi[2 * pass] = key_value(keys[lo]);
      lohi[2 * pass + 1] = key_value(keys[n - 1 - lo]);
    } else {
      lohi[2 * pass] = lohi[2 * pass + 1] = NAN;
    }
    __syncthreads();  // the keys are rewritten by the next pass
  }
  if (tid != 0) return;
  const int n_valid = m[g.R];
  double a_hat = NAN, b_hat = NAN;
  if (n_valid > 0) {
    a_hat = theta(sa[g.R], n_valid, g.kind);
    b_hat = theta(sb[g.R], n_valid, g.kind);
  }
  double* st = g.stats + static_cast<long long>(blockIdx.x) * 8;
  st[0] = a_hat;
  st[1] = b_hat;
  st[2] = b_hat - a_hat;
  st[3] = b_hat / a_hat;
  st[4] = lohi[0];
  st[5] = lohi[1];
  st[6] = lohi[2];
  st[7] = lohi[3];
  int* ct = g.counts + static_cast<long long>(blockIdx.x) * 4;
  ct[0] = n_valid;
  ct[1] = cnt[0];
  ct[2] = cnt[1];
  ct[3] = cnt[2];
}

inline bool misaligned(const void* p, unsigned bytes) { return (reinterpret_cast<uintptr_t>(p) & (bytes - 1u)) != 0; }

inline bool sizes_served(int N, int R, int D) {
  if (R > MAX_R) return false;
  const long long total = static_cast<long long>(R) * D;
  return ((total > N ? total : N) + W_TPB - 1) / W_TPB <= INT_MAX;  // the grid of the weights launch
}

}  // namespace

extern "C" int ldc_paired_bootstrap_max_replicates(void) { return MAX_R; }

extern "C" long long ldc_paired_bootstrap_workspace_bytes(int N, int K, int R, int D) {
  if (N <= 0 || K <= 0 || R <= 0 || D <= 0 || !sizes_served(N, R, D)) return 0;
  return layout(N, K, R).bytes;
}

extern "C" int ldc_paired_bootstrap(const float* a, const float* b, long long ld, int N, int K, const int* draws, int R, int D, int kind,
                                    int tail_ppm, double* stats, int* counts, void* workspace, long long workspace_bytes, void* stream) {
  LDC_CHECK_PTR(a);
  LDC_CHECK_PTR(b);
  LDC_CHECK_PTR(draws);
  LDC_CHECK_PTR(stats);
  LDC_CHECK_PTR(counts);
  LDC_CHECK_PTR(workspace);
  if (N <= 0 || K <= 0 || R <= 0 || D <= 0 || ld < K || kind < 0 || kind > 1 || tail_ppm < 0 || tail_ppm >= 500000) return LDC_ERR_ARG;
  if (!sizes_served(N, R, D)) return LDC_ERR_UNSUPPORTED;
  const Layout l = layout(N, K, R);
  if (workspace_bytes < l.bytes) return LDC_ERR_ARG;
  if (misaligned(a, 4) || misaligned(b, 4) || misaligned(draws, 4) || misaligned(counts, 4) || misaligned(stats, 8) || !ldc_aligned16(workspace))
    return LDC_ERR_ALIGN;
  hipStream_t s = static_cast<hipStream_t>(stream);
  unsigned char* ws = static_cast<unsigned char*>(workspace);
  int* wt = reinterpret_cast<int*>(ws);
  double* sa = reinterpret_cast<double*>(ws + l.off_sa);
  double* sb = reinterpret_cast<double*>(ws + l.off_sb);
  int* m = reinterpret_cast<int*>(ws + l.off_m);
  static const bool attr_set = [] {  // once per process; thread-safe (C++11 static initialisation)
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(bootstrap_select_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, MAX_R * 8);
    return true;
  }();
  (void)attr_set;
  if (hipMemsetAsync(wt, 0, static_cast<size_t>(N) * l.rs * 4, s) != hipSuccess) return ldc_launch_status();

  const long long total = static_cast<long long>(R) * D;
  const long long w_threads = total > N ? total : N;
  WeightArgs wa{draws, wt, l.rs, total, N, R, D};
  hipLaunchKernelGGL(bootstrap_weights_kernel, dim3(static_cast<unsigned>((w_threads + W_TPB - 1) / W_TPB)), dim3(W_TPB), 0, s, wa);

  SumArgs sm{a, b, wt, sa, sb, m, ld, l.rs, N, K, R + 1};
  hipLaunchKernelGGL(bootstrap_sums_kernel, dim3(static_cast<unsigned>((K + TK - 1) / TK), static_cast<unsigned>((R + 1 + TR - 1) / TR)), dim3(SUMS_TPB),
                     0, s, sm);

  int P = 1;
  while (P < R) P <<= 1;
  SelectArgs se{sa, sb, m, stats, counts, l.rs, R, P, kind, tail_ppm};
  hipLaunchKernelGGL(bootstrap_select_kernel, dim3(static_cast<unsigned>(K)), dim3(SEL_TPB), static_cast<size_t>(P) * 8, s, se);
  return ldc_launch_status();
}
