// Zonal power spectra of a decoded ensemble: power per longitudinal wavenumber of the members, of the ensemble
// mean and of the truth, per (channel, lead time).  Not in the reference (ladcast/evaluate/utils.py stops at CRPS and ACC).
// Addressing is that of ldc_rollout_reliability (reliability.hip): forecast by member / lead / channel strides, optional fused inverse
// normalisation (inv_norm, ensemble_common.h), truth as a table of planes with a slot per lead time, output columns at l_off.
// row_weight[H] >= 0 replaces the latitude weight: a row whose weight is not > 0 is never read.
// Per row of W points (half = W / 2, K = half + 1 bins), for each of the M + 2 sequences y (members in order, ensemble mean m, truth t):
//   mu  = (sum_j y_j) / W                 pair sums y_p + y_{W-p} per lane in index order, wave butterfly
//   e_p = (y_p - mu) + (y_{W-p} - mu), o_p = (y_p - mu) - (y_{W-p} - mu) for 0 < p < half;  e_0 = y_0 - mu, e_half = y_half - mu, o = 0
//   Re_k = sum_{p = 0 .. half} e_p cos(2 pi p k / W),  Im_k = sum_p o_p sin(2 pi p k / W)    explicit fmaf in p order, k = 1 .. half
//   |Y_k|^2 = Re^2 + Im^2 in fp64 (exact products);  k = 0: (W mu)^2, i.e. P_0 = mu^2: the pivot, P_k for k >= 1 does not see mu
// The twiddles come from one W-entry table per launch: sincospi in fp64, rounded to fp32; entry (p k) mod W is tracked by addition.
// m_j = (x_0j + ... + x_{M-1,j}) / M in fp32 in member order, as reliability.hip forms its mean.  A row with a NaN among its M members or
// its truth (after the inverse normalisation) is left out and counted.
// Mapping: one wave per workgroup, RPW consecutive rows per workgroup.  Lane t owns bins k = 1 + t + 64 b, b < KB = ceil(half / 64), and 8
// sequences at a time: (e_p, o_p) of the 8 sequences lie in LDS as [p][2][8] and are read by every lane at the same address (b128
// broadcasts, no bank conflict); one twiddle gather per (p, bin) serves 16 fmaf.  Sums over members and rows per bin: fp64 in the lane, in
// order; the workgroups' records are merged in index order by the finish launch.  No atomics: run-to-run bit-equal.
// Built with -ffp-contract=off: the only fused operations are the explicit fmaf of the transform.
#include <math.h>

#include "ensemble_common.h"

namespace {

constexpr int WAVE = 64;
constexpr int RPW = 8;          // rows per workgroup (one record each workgroup)
constexpr int SB = 8;           // sequences per register block
constexpr int MAX_M = 1024;
constexpr int MAX_W = 512;
constexpr long long TABLE_BYTES = MAX_W * 2 * sizeof(float);  // front of the workspace: the twiddle table

constexpr int rec_doubles(int K) { return 2 + 3 * K; }  // sum of weights; (n_invalid, n_valid) as two int32; [3][K] sums

struct SpecArgs {
  RolloutView v;        // no climatology; lat_w holds row_weight
  const float2* table;  // [W] (cos, sin)(2 pi i / W)
  double* rec;          // [L][C][nrec][rec_doubles(K)]
  int nrec;
};

__global__ void spectrum_table_kernel(float2* __restrict__ table, int W) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= W) return;
  double s, c;
  sincospi(static_cast<double>(2 * i) / static_cast<double>(W), &s, &c);
  table[i] = make_float2(static_cast<float>(c), static_cast<float>(s));
}

// KB: bins per lane; serves W <= 128 KB
template <int KB, bool INV>
__global__ __launch_bounds__(WAVE) void spectrum_kernel(SpecArgs a) {
  constexpr int WMAX = 128 * KB;
  constexpr int NQ = 2 * KB;  // points per lane
  constexpr int PQ = KB + 1;  // fold pairs p = 0 .. half per lane
  __shared__ float2 s_tw[WMAX];
  __shared__ float s_mean[WMAX];
  __shared__ __attribute__((aligned(16))) float s_eo[WMAX / 2 + 1][2][SB];
  const int c = blockIdx.y, l = blockIdx.z, t = threadIdx.x;
  const int M = a.v.M, W = a.v.W, half = W >> 1, K = half + 1;
  const float Mf = static_cast<float>(M), Wf = static_cast<float>(W);
  const float* fbase = view_forecast(a.v, c, l);
  const float* tbase = view_truth(a.v, c, l);
  const InvNorm nrm = view_norm<INV>(a.v, c);
  for (int i = t; i < W; i += WAVE) s_tw[i] = a.table[i];
  int kk[KB];  // the lane's bins; 0: none (the table's entry 0 is read, nothing is kept)
#pragma unroll
  for (int b = 0; b < KB; ++b) {
    const int k = 1 + t + WAVE * b;
    kk[b] = k <= half ? k : 0;
  }
  double tot[KB][3], tot0[3] = {0.0, 0.0, 0.0}, wsum = 0.0;
#pragma unroll
  for (int b = 0; b < KB; ++b) tot[b][0] = tot[b][1] = tot[b][2] = 0.0;
  int n_invalid = 0, n_valid = 0;
  const int nblk = (M + 2 + SB - 1) / SB;

  const int h1 = min((static_cast<int>(blockIdx.x) + 1) * RPW, a.v.H);
  for (int h = blockIdx.x * RPW; h < h1; ++h) {
    const float w = a.v.lat_w[h];
    if (!(w > 0.f)) continue;  // not read at all
    const float* frow = fbase + static_cast<long long>(h) * W;
    const float* trow = tbase + static_cast<long long>(h) * W;
    // the ensemble mean of the row and its validity
    float sum[NQ];
    bool bad = false;
#pragma unroll
    for (int q = 0; q < NQ; ++q) sum[q] = 0.f;
    for (int i = 0; i < M; ++i) {
#pragma unroll
      for (int q = 0; q < NQ; ++q) {
        const int j = t + WAVE * q;
        if (j < W) {
          const float v = load_member<INV>(frow + j, i, a.v.fc_ms, nrm);
          sum[q] += v;
          bad = bad || (v != v);
        }
      }
    }
    __syncthreads();  // the readers of s_mean of the row before are done
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
      const int j = t + WAVE * q;
      if (j < W) {
        s_mean[j] = sum[q] / Mf;
        const float tv = trow[j];
        bad = bad || (tv != tv);
      }
    }
    if (__syncthreads_or(bad ? 1 : 0)) {
      ++n_invalid;
      continue;
    }
    ++n_valid;
    double acc[KB][3], acc0[3] = {0.0, 0.0, 0.0};
#pragma unroll
    for (int b = 0; b < KB; ++b) acc[b][0] = acc[b][1] = acc[b][2] = 0.0;
    for (int blk = 0; blk < nblk; ++blk) {
      // sequence q: member q < M, the ensemble mean (M), the truth (M + 1), nothing beyond
      auto value = [&](int q, int j) -> float {
        if (q < M) return load_member<INV>(frow + j, q, a.v.fc_ms, nrm);
        if (q == M) return s_mean[j];
        if (q == M + 1) return trow[j];
        return 0.f;
      };
      float ya[PQ][SB], yb[PQ][SB], mu[SB];
#pragma unroll
      for (int s = 0; s < SB; ++s) {
        const int q = blk * SB + s;
        float part = 0.f;
#pragma unroll
        for (int r = 0; r < PQ; ++r) {
          const int p = t + WAVE * r;
          ya[r][s] = p <= half ? value(q, p) : 0.f;
          yb[r][s] = (p > 0 && p < half) ? value(q, W - p) : 0.f;
          part += ya[r][s] + yb[r][s];
        }
        mu[s] = wave_sum(part) / Wf;
      }
      __syncthreads();  // the bin loop of the block before has read s_eo
#pragma unroll
      for (int r = 0; r < PQ; ++r) {
        const int p = t + WAVE * r;
        if (p <= half) {
          const bool paired = p > 0 && p < half;
          float e[SB], o[SB];
#pragma unroll
          for (int s = 0; s < SB; ++s) {
            const float ra = ya[r][s] - mu[s];
            const float rb = yb[r][s] - mu[s];
            e[s] = paired ? ra + rb : ra;
            o[s] = paired ? ra - rb : 0.f;
          }
          float4* dst = reinterpret_cast<float4*>(&s_eo[p][0][0]);
          dst[0] = make_float4(e[0], e[1], e[2], e[3]);
          dst[1] = make_float4(e[4], e[5], e[6], e[7]);
          dst[2] = make_float4(o[0], o[1], o[2], o[3]);
          dst[3] = make_float4(o[4], o[5], o[6], o[7]);
        }
      }
      __syncthreads();
      float re[KB][SB], im[KB][SB];
      int idx[KB];
#pragma unroll
      for (int b = 0; b < KB; ++b) {
        idx[b] = 0;
#pragma unroll
        for (int s = 0; s < SB; ++s) re[b][s] = im[b][s] = 0.f;
      }
      for (int p = 0; p <= half; ++p) {
        const float4* src = reinterpret_cast<const float4*>(&s_eo[p][0][0]);
        const float4 e0 = src[0], e1 = src[1], o0 = src[2], o1 = src[3];
        const float e[SB] = {e0.x, e0.y, e0.z, e0.w, e1.x, e1.y, e1.z, e1.w};
        const float o[SB] = {o0.x, o0.y, o0.z, o0.w, o1.x, o1.y, o1.z, o1.w};
#pragma unroll
        for (int b = 0; b < KB; ++b) {
          const float2 tw = s_tw[idx[b]];
#pragma unroll
          for (int s = 0; s < SB; ++s) {
            re[b][s] = __builtin_fmaf(e[s], tw.x, re[b][s]);
            im[b][s] = __builtin_fmaf(o[s], tw.y, im[b][s]);
          }
          idx[b] += kk[b];
          idx[b] -= idx[b] >= W ? W : 0;
        }
      }
#pragma unroll
      for (int s = 0; s < SB; ++s) {
        const int q = blk * SB + s;
        const int plane = q < M ? 0 : q - M + 1;  // wave-uniform
        if (plane > 2) break;
        const double y0 = static_cast<double>(mu[s]) * static_cast<double>(Wf);
        acc0[plane] += y0 * y0;
#pragma unroll
        for (int b = 0; b < KB; ++b) {
          const double r = static_cast<double>(re[b][s]), i = static_cast<double>(im[b][s]);
          acc[b][plane] += r * r + i * i;
        }
      }
    }
    const double wd = static_cast<double>(w);
    wsum += wd;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) {
      tot0[pl] += wd * acc0[pl];
#pragma unroll
      for (int b = 0; b < KB; ++b) tot[b][pl] += wd * acc[b][pl];
    }
  }
  double* rec = a.rec + ((static_cast<long long>(l) * a.v.C + c) * a.nrec + blockIdx.x) * rec_doubles(K);
  if (t == 0) {
    rec[0] = wsum;
    reinterpret_cast<int*>(rec + 1)[0] = n_invalid;
    reinterpret_cast<int*>(rec + 1)[1] = n_valid;
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) rec[2 + pl * K] = tot0[pl];
  }
#pragma unroll
  for (int b = 0; b < KB; ++b)
    if (kk[b] > 0) {
#pragma unroll
      for (int pl = 0; pl < 3; ++pl) rec[2 + pl * K + kk[b]] = tot[b][pl];
    }
}

// One workgroup per (channel, lead time): grid (C, L).  out [3][C][L_total][K]; n_invalid [C][L_total]; columns l_off .. l_off + L - 1.
__global__ __launch_bounds__(256) void spectrum_finish_kernel(const double* __restrict__ recs, int nrec, int M, int C, int W,
                                                              float* __restrict__ out, int* __restrict__ n_invalid, int L_total, int l_off) {
  const int c = blockIdx.x, l = blockIdx.y;
  const int half = W >> 1, K = half + 1, RD = rec_doubles(K);
  const double* base = recs + (static_cast<long long>(l) * C + c) * nrec * RD;
  const long long col = static_cast<long long>(c) * L_total + l_off + l;
  const long long plane = static_cast<long long>(C) * L_total * K;
  const double W2 = static_cast<double>(W) * static_cast<double>(W);
  for (int k = threadIdx.x; k < K; k += blockDim.x) {
    double wsum = 0.0, s0 = 0.0, s1 = 0.0, s2 = 0.0;
    int valid = 0;
    for (int r = 0; r < nrec; ++r) {
      const double* src = base + static_cast<long long>(r) * RD;
      wsum += src[0];
      valid += reinterpret_cast<const int*>(src + 1)[1];
      s0 += src[2 + k];
      s1 += src[2 + K + k];
      s2 += src[2 + 2 * K + k];
    }
    const double sk = (k == 0 || k == half) ? 1.0 : 2.0;
    const float nanv = __builtin_nanf("");
    float* o = out + col * K + k;
    o[0] = valid > 0 ? static_cast<float>(sk * s0 / (static_cast<double>(M) * W2 * wsum)) : nanv;
    o[plane] = valid > 0 ? static_cast<float>(sk * s1 / (1.0 * W2 * wsum)) : nanv;
    o[2 * plane] = valid > 0 ? static_cast<float>(sk * s2 / (1.0 * W2 * wsum)) : nanv;
  }
  if (threadIdx.x == 0) {
    int inv = 0;
    for (int r = 0; r < nrec; ++r) inv += reinterpret_cast<const int*>(base + static_cast<long long>(r) * RD + 1)[0];
    n_invalid[col] = inv;
  }
}

template <bool INV>
void launch_spectrum(const SpecArgs& a, dim3 grid, hipStream_t s) {
  const int W = a.v.W;
  if (W <= 128) hipLaunchKernelGGL((spectrum_kernel<1, INV>), grid, dim3(WAVE), 0, s, a);
  else if (W <= 256) hipLaunchKernelGGL((spectrum_kernel<2, INV>), grid, dim3(WAVE), 0, s, a);
  else if (W <= 384) hipLaunchKernelGGL((spectrum_kernel<3, INV>), grid, dim3(WAVE), 0, s, a);
  else hipLaunchKernelGGL((spectrum_kernel<4, INV>), grid, dim3(WAVE), 0, s, a);
}

bool served(int M, int C, int L, int H, int W) {
  return M <= MAX_M && C <= 65535 && L <= 65535 && (W & 1) == 0 && W >= 4 && W <= MAX_W && static_cast<long long>(H) * W <= (1ll << 24);
}

}  // namespace

extern "C" long long ldc_rollout_spectrum_workspace_bytes(int M, int C, int L, int H, int W) {
  if (M <= 0 || C <= 0 || L <= 0 || H <= 0 || W <= 0 || !served(M, C, L, H, W)) return 0;
  const long long nrec = (static_cast<long long>(H) + RPW - 1) / RPW;
  return TABLE_BYTES + static_cast<long long>(L) * C * nrec * rec_doubles(W / 2 + 1) * static_cast<long long>(sizeof(double));
}

extern "C" int ldc_rollout_spectrum(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                                    const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                                    long long truth_channel_stride, const int* truth_slot, const float* row_weight, int M, int C, int L, int H,
                                    int W, float* out, int* n_invalid, int L_total, int l_off, void* workspace, long long workspace_bytes,
                                    void* stream) {
  SpecArgs a{};
  if (ldc_rollout_view(&a.v, forecast, member_stride, lead_stride, channel_stride, mean, std_, target_std, truth, truth_slot_stride,
                       truth_channel_stride, truth_slot, nullptr, 0, 0, nullptr, row_weight, M, C, L, H, W, L_total, l_off) != LDC_OK)
    return LDC_ERR_ARG;
  LDC_CHECK_PTR(out);
  LDC_CHECK_PTR(n_invalid);
  LDC_CHECK_PTR(workspace);
  if (!served(M, C, L, H, W)) return LDC_ERR_UNSUPPORTED;
  if (workspace_bytes < ldc_rollout_spectrum_workspace_bytes(M, C, L, H, W)) return LDC_ERR_ARG;
  LDC_CHECK_ALIGN16(workspace);
  float2* table = static_cast<float2*>(workspace);
  a.table = table;
  a.rec = reinterpret_cast<double*>(static_cast<char*>(workspace) + TABLE_BYTES);
  a.nrec = ldc_cdiv(H, RPW);
  hipStream_t s = static_cast<hipStream_t>(stream);
  hipLaunchKernelGGL(spectrum_table_kernel, dim3(ldc_cdiv(W, 256)), dim3(256), 0, s, table, W);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  dim3 grid(a.nrec, C, L);
  if (mean != nullptr) launch_spectrum<true>(a, grid, s);
  else launch_spectrum<false>(a, grid, s);
  st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(spectrum_finish_kernel, dim3(C, L), dim3(256), 0, s, a.rec, a.nrec, M, C, W, out, n_invalid, L_total, l_off);
  return ldc_launch_status();
}
