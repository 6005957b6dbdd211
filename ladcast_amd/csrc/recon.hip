// DC-AE reconstruction evaluation (reference: ladcast/evaluate/evaluate_encdec_model.py): the batch preprocessing and the scores
// of a reconstruction against its target, each in one pass.
//   ldc_recon_preprocess = weather_dataset_preprocess_batch (dataloader/weather_dataset.py:203-224): crop_south_pole and
//     incl_sur_pressure=False are a row offset and a smaller channel count of the strided input, (x - mean_c) / std_c with a real
//     subtraction and a correctly rounded division (bit-equal to torch), NaN -> -2 in the SST channel + the uint8 mask of where.
//   ldc_recon_scores = process_tensor_for_loss (metric/utils.py:20-63) + LpLoss.rel with a weight (metric/loss.py:73-102) + the
//     un-normalise / mse_loss / latitude-weighted mean block of evaluate_encdec_model.py:211-231, ~12 torch passes over (B, Cp, H, W):
//       num[b][c] = sum (w_h (p - t))^2, den[b][c] = sum (w_h t)^2, rel = sqrt(num) / sqrt(den)      (the weight enters squared)
//       lw_mse[c] = mean_{b,h,w} w_h ((p sigma_c + mu_c) - (t sigma_c + mu_c))^2                      (masked points stay, as zeros)
//     The target's static channels are read from `static_` (the reference's torch.cat is never made).  The physical-unit difference
//     rounds as torch's fp32 ops do - multiply, add, multiply, add, subtract, square, multiply, nothing contracted (this file is
//     built with -ffp-contract=off and the chain is written with the _rn intrinsics) - so a point value is bit-equal to the
//     reference's and only the order of the sums differs.
// B * Cp planes are too few for 256 CUs at B = 1-2: a plane is cut into chunks of whole rows (~1024 points), one workgroup each,
// whose three partial sums go to the caller's workspace; a second small launch adds them in a fixed order (no float atomics: two
// calls give the same bits).
#include <math.h>

#include "common.h"

namespace {

constexpr int TPB = 256;
constexpr int CHUNK_POINTS = 1024;  // points per workgroup of the scores kernel (whole rows; one row when W is larger)
constexpr int NP = 4;               // floats per partial record: num, den, lw, pad

__host__ __device__ inline int chunk_rows(int W) { return W >= CHUNK_POINTS ? 1 : CHUNK_POINTS / W; }

struct PreArgs {
  const float* x;
  long long sb, sc, sr;
  const float *mean, *std_;
  float* out;
  unsigned char* mask;
  int C, H, W, sst;
};

template <int V>  // V = 4: 16-byte loads / stores (W % 4 == 0, aligned bases and strides), V = 1: scalar
__global__ __launch_bounds__(TPB) void recon_preprocess_kernel(PreArgs a) {
  const int c = blockIdx.y, b = blockIdx.z;
  const long long HW = static_cast<long long>(a.H) * a.W;
  const long long e = (static_cast<long long>(blockIdx.x) * TPB + threadIdx.x) * V;
  if (e >= HW) return;
  const int h = static_cast<int>(e / a.W), w = static_cast<int>(e - static_cast<long long>(h) * a.W);
  const float* src = a.x + b * a.sb + c * a.sc + h * a.sr + w;
  float* dst = a.out + (static_cast<long long>(b) * a.C + c) * HW + e;
  const float mu = a.mean[c], sd = a.std_[c];
  float v[V];
  if constexpr (V == 4) {
    const f32x4 q = *reinterpret_cast<const f32x4*>(src);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = q[i];
  } else {
    v[0] = src[0];
  }
  const bool sst = c == a.sst;
#pragma unroll
  for (int i = 0; i < V; ++i) {
    float y = __fdiv_rn(__fsub_rn(v[i], mu), sd);
    if (sst) {
      const bool nan = y != y;  // torch.isnan of the NORMALISED value, as the reference takes it
      a.mask[static_cast<long long>(b) * HW + e + i] = nan ? 1 : 0;
      if (nan) y = -2.0f;
    }
    v[i] = y;
  }
  if constexpr (V == 4) {
    f32x4 q;
#pragma unroll
    for (int i = 0; i < 4; ++i) q[i] = v[i];
    *reinterpret_cast<f32x4*>(dst) = q;
  } else {
    dst[0] = v[0];
  }
}

struct ScoreArgs {
  const float *pred, *target, *stat;
  long long stat_bs;
  const unsigned char* mask;
  const float *lat_w, *mean, *std_;
  float* part;  // [B * Cp][nchunk][NP]
  int C, Cp, H, W, sst, nchunk, rows;
};

struct Acc {
  float num, den, lw;
};

__device__ __forceinline__ void add_point(Acc& s, float p, float t, bool masked, float w, float sd, float mu) {
  if (masked) p = t = -2.0f;
  const float wd = __fmul_rn(w, __fsub_rn(p, t)), wt = __fmul_rn(w, t);
  s.num = __fadd_rn(s.num, __fmul_rn(wd, wd));
  s.den = __fadd_rn(s.den, __fmul_rn(wt, wt));
  const float e = __fsub_rn(__fadd_rn(__fmul_rn(p, sd), mu), __fadd_rn(__fmul_rn(t, sd), mu));
  s.lw = __fadd_rn(s.lw, __fmul_rn(__fmul_rn(e, e), w));
}

template <int V>
__global__ __launch_bounds__(TPB) void recon_scores_kernel(ScoreArgs a) {
  __shared__ float red[TPB / 64][3];
  const int plane = blockIdx.y, chunk = blockIdx.x;
  const int b = plane / a.Cp, c = plane - b * a.Cp;
  const long long HW = static_cast<long long>(a.H) * a.W;
  const int h0 = chunk * a.rows, nrow = min(a.rows, a.H - h0);
  const long long e0 = static_cast<long long>(h0) * a.W;
  const int n = nrow * a.W;  // points of this chunk (< 2^31: one row, or at most CHUNK_POINTS)
  const float* p = a.pred + static_cast<long long>(plane) * HW + e0;
  const float* t = (c < a.C ? a.target + (static_cast<long long>(b) * a.C + c) * HW : a.stat + b * a.stat_bs + (c - a.C) * HW) + e0;
  const unsigned char* m = (a.mask != nullptr && c == a.sst) ? a.mask + b * HW + e0 : nullptr;
  const float sd = a.std_[c], mu = a.mean[c];
  Acc s{0.f, 0.f, 0.f};
  for (int i = threadIdx.x * V; i < n; i += TPB * V) {
    const float w = a.lat_w[h0 + i / a.W];  // V == 4: W % 4 == 0, the four points share a row
    if constexpr (V == 4) {
      const f32x4 pv = *reinterpret_cast<const f32x4*>(p + i), tv = *reinterpret_cast<const f32x4*>(t + i);
      const unsigned mk = m ? *reinterpret_cast<const unsigned*>(m + i) : 0u;
#pragma unroll
      for (int j = 0; j < 4; ++j) add_point(s, pv[j], tv[j], ((mk >> (8 * j)) & 0xffu) != 0u, w, sd, mu);
    } else {
      add_point(s, p[i], t[i], m != nullptr && m[i] != 0, w, sd, mu);
    }
  }
  // fixed order: lanes by butterfly, then the four wave totals
  const float r0 = wave_sum(s.num), r1 = wave_sum(s.den), r2 = wave_sum(s.lw);
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[wave][0] = r0;
    red[wave][1] = r1;
    red[wave][2] = r2;
  }
  __syncthreads();
  if (threadIdx.x < 3) {
    const int i = threadIdx.x;
    a.part[(static_cast<long long>(plane) * a.nchunk + chunk) * NP + i] = (red[0][i] + red[1][i]) + (red[2][i] + red[3][i]);
  }
}

// one wave per channel: per batch element, lane j adds the chunk records j, j + 64, ... in order, then a fixed butterfly
__global__ __launch_bounds__(64) void recon_scores_finish_kernel(const float* __restrict__ part, int nchunk, int B, int Cp, float npoints,
                                                                 float* __restrict__ rel, float* __restrict__ abs_norm,
                                                                 float* __restrict__ lw_mse) {
  const int c = blockIdx.x;
  float lw = 0.f;
  for (int b = 0; b < B; ++b) {
    const float* src = part + (static_cast<long long>(b) * Cp + c) * nchunk * NP;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int k = threadIdx.x; k < nchunk; k += 64) {
      s0 += src[k * NP];
      s1 += src[k * NP + 1];
      s2 += src[k * NP + 2];
    }
    s0 = wave_sum(s0);
    s1 = wave_sum(s1);
    lw += wave_sum(s2);
    if (threadIdx.x == 0) {
      const float nrm = sqrtf(s0);
      rel[b * Cp + c] = nrm / sqrtf(s1);  // den == 0: inf, or NaN when num == 0 too, as the reference's division gives
      if (abs_norm) abs_norm[b * Cp + c] = nrm;
    }
  }
  if (threadIdx.x == 0) lw_mse[c] = lw / npoints;
}

}  // namespace

extern "C" int ldc_recon_preprocess(const float* x, long long batch_stride, long long channel_stride, long long row_stride, int B,
                                    int C, int H, int W, const float* mean, const float* std_, int sst_channel, float* out,
                                    unsigned char* nan_mask, void* stream) {
  LDC_CHECK_PTR(x);
  LDC_CHECK_PTR(mean);
  LDC_CHECK_PTR(std_);
  LDC_CHECK_PTR(out);
  if (B <= 0 || C <= 0 || H <= 0 || W <= 0 || row_stride < W || sst_channel >= C) return LDC_ERR_ARG;
  if (sst_channel >= 0) LDC_CHECK_PTR(nan_mask);
  if (B > 65535 || C > 65535) return LDC_ERR_UNSUPPORTED;
  PreArgs a{x, batch_stride, channel_stride, row_stride, mean, std_, out, nan_mask, C, H, W, sst_channel < 0 ? -1 : sst_channel};
  const long long HW = static_cast<long long>(H) * W;
  const bool vec = W % 4 == 0 && ldc_aligned16(x) && ldc_aligned16(out) && batch_stride % 4 == 0 && channel_stride % 4 == 0 && row_stride % 4 == 0;
  hipStream_t s = static_cast<hipStream_t>(stream);
  if (vec) hipLaunchKernelGGL(recon_preprocess_kernel<4>, dim3(ldc_cdiv(HW / 4, TPB), C, B), dim3(TPB), 0, s, a);
  else hipLaunchKernelGGL(recon_preprocess_kernel<1>, dim3(ldc_cdiv(HW, TPB), C, B), dim3(TPB), 0, s, a);
  return ldc_launch_status();
}

extern "C" long long ldc_recon_scores_workspace_bytes(int B, int Cp, int H, int W) {
  if (B <= 0 || Cp <= 0 || H <= 0 || W <= 0) return 0;
  return static_cast<long long>(B) * Cp * ldc_cdiv(H, chunk_rows(W)) * NP * static_cast<long long>(sizeof(float));
}

extern "C" int ldc_recon_scores(const float* pred, const float* target, const float* static_, long long static_batch_stride,
                                const unsigned char* nan_mask, const float* lat_weight, const float* mean, const float* std_, int B,
                                int C, int S, int H, int W, int sst_channel, float* rel, float* abs_norm, float* lw_mse,
                                void* workspace, long long workspace_bytes, void* stream) {
  LDC_CHECK_PTR(pred);
  LDC_CHECK_PTR(target);
  LDC_CHECK_PTR(lat_weight);
  LDC_CHECK_PTR(mean);
  LDC_CHECK_PTR(std_);
  LDC_CHECK_PTR(rel);
  LDC_CHECK_PTR(lw_mse);
  LDC_CHECK_PTR(workspace);
  if (B <= 0 || C <= 0 || S < 0 || H <= 0 || W <= 0) return LDC_ERR_ARG;
  if (S > 0) LDC_CHECK_PTR(static_);
  const int Cp = C + S;
  const long long HW = static_cast<long long>(H) * W;
  if (static_cast<long long>(B) * Cp > 65535 || B * HW >= (1ll << 24)) return LDC_ERR_UNSUPPORTED;  // grid.y; the fp32 point count
  if (workspace_bytes < ldc_recon_scores_workspace_bytes(B, Cp, H, W)) return LDC_ERR_ARG;
  LDC_CHECK_ALIGN16(workspace);
  ScoreArgs a{};
  a.pred = pred;
  a.target = target;
  a.stat = static_;
  a.stat_bs = static_batch_stride;
  a.mask = (nan_mask != nullptr && sst_channel >= 0 && sst_channel < Cp) ? nan_mask : nullptr;
  a.lat_w = lat_weight;
  a.mean = mean;
  a.std_ = std_;
  a.part = static_cast<float*>(workspace);
  a.C = C; a.Cp = Cp; a.H = H; a.W = W;
  a.sst = sst_channel;
  a.rows = chunk_rows(W);
  a.nchunk = ldc_cdiv(H, a.rows);
  // 16-byte loads: every plane and every chunk of whole rows starts on a 16-byte boundary (the mask: on a 4-byte one)
  const bool vec = W % 4 == 0 && ldc_aligned16(pred) && ldc_aligned16(target) && (S == 0 || (ldc_aligned16(static_) && static_batch_stride % 4 == 0)) &&
                   (a.mask == nullptr || (reinterpret_cast<uintptr_t>(a.mask) & 3u) == 0);
  hipStream_t s = static_cast<hipStream_t>(stream);
  dim3 grid(a.nchunk, B * Cp);
  if (vec) hipLaunchKernelGGL(recon_scores_kernel<4>, grid, dim3(TPB), 0, s, a);
  else hipLaunchKernelGGL(recon_scores_kernel<1>, grid, dim3(TPB), 0, s, a);
  int st = ldc_launch_status();
  if (st != LDC_OK) return st;
  hipLaunchKernelGGL(recon_scores_finish_kernel, dim3(Cp), dim3(64), 0, s, a.part, a.nchunk, B, Cp, static_cast<float>(B * HW), rel,
                     abs_norm, lw_mse);
  return ldc_launch_status();
}
