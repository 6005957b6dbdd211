// The EDM denoising objective around the model forward (reference: train_AR.py:873-1032 without the backward pass), with one noise level
// PER SAMPLE: noising + input preconditioning, output preconditioning, and the weighted squared error reduced to one value per (H, W) plane.
// Built with -ffp-contract=off (as sampler.hip): every product, sum and difference rounds to fp32 where torch's elementwise kernels
// round, so `noisy`, `x_in` and `denoised` are bit-identical to the reference's tensor expressions.  The per-sample coefficients are
// fp32 device vectors the host computed with the reference's own fp32 tensor arithmetic (schedulers: `edm_coefficients`).
// Not tuned: each kernel makes one pass over its data with scalar loads (a 450-element plane starts on a 16-byte boundary only every
// other plane); next to the forward between them they are noise.
#include "common.h"

namespace {

// noisy = clean + noise * sigma_b (two roundings); x_in = noisy * c_in_b.  noise == nullptr: noisy = clean (precondition_inputs alone).
__global__ void edm_noise_inputs_kernel(const float* __restrict__ clean, const float* __restrict__ noise,
                                        const float* __restrict__ sigma, const float* __restrict__ c_in, float* __restrict__ noisy,
                                        float* __restrict__ x_in, long long n_per_sample, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long b = i / n_per_sample;
  float v = clean[i];
  if (noise != nullptr) {
    const float s = noise[i] * sigma[b];
    v = v + s;
  }
  if (noisy != nullptr) noisy[i] = v;
  if (x_in != nullptr) x_in[i] = v * c_in[b];
}

// denoised = c_skip_b * noisy + c_out_b * F (three roundings, the order of precondition_outputs) on (B, C, T, plane) views of tensors
// with `*_frames` frames: row (b, c) of a view is T * plane contiguous elements at (b * C + c) * frames * plane
__global__ void edm_denoise_kernel(const float* __restrict__ noisy, const float* __restrict__ F, const float* __restrict__ c_skip,
                                   const float* __restrict__ c_out, float* __restrict__ denoised, int C, long long run,
                                   long long noisy_row, long long f_row, long long den_row, long long n) {
  const long long i = static_cast<long long>(blockIdx.x) * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const long long row = i / run, j = i - row * run;
  const long long b = row / C;
  const float a = c_skip[b] * noisy[row * noisy_row + j];
  const float g = c_out[b] * F[row * f_row + j];
  denoised[row * den_row + j] = a + g;
}

// One wave per (b, c, t) plane.  Lane l takes elements l, l + 64, ... of the plane in that order into its own fp64 sum; the 64 sums go
// through the xor butterfly (a fixed tree: both operands of every add are the same values in every lane, so all lanes end with the same
// bits); one fp64 division by the plane size, one rounding to fp32.  No atomics, nothing that depends on which wave runs when.
constexpr int LOSS_WAVES = 4;

__global__ void __launch_bounds__(64 * LOSS_WAVES)
    edm_denoise_loss_kernel(const float* __restrict__ noisy, const float* __restrict__ F, const float* __restrict__ target,
                            const float* __restrict__ c_skip, const float* __restrict__ c_out, const float* __restrict__ weight,
                            const float* __restrict__ lat_weight, float* __restrict__ table, float* __restrict__ denoised,
                            long long planes, int planes_per_sample, int W, int plane) {
  const int lane = threadIdx.x & 63;
  const long long pl = static_cast<long long>(blockIdx.x) * LOSS_WAVES + (threadIdx.x >> 6);
  if (pl >= planes) return;  // wave-uniform
  const long long b = pl / planes_per_sample;
  const float cs = c_skip[b], co = c_out[b], wb = weight[b];
  const long long base = pl * plane;
  double acc = 0.0;
  for (int p = lane; p < plane; p += 64) {
    const float a = cs * noisy[base + p];
    const float g = co * F[base + p];
    const float d = a + g;
    if (denoised != nullptr) denoised[base + p] = d;
    const float e = d - target[base + p];
    const float q = e * e;
    float w = wb;
    if (lat_weight != nullptr) w = lat_weight[p / W] * wb;
    const float term = w * q;
    acc += static_cast<double>(term);
  }
  acc = wave_sum(acc);
  if (lane == 0) table[pl] = static_cast<float>(acc / static_cast<double>(plane));
}

}  // namespace

extern "C" int ldc_edm_noise_inputs(const float* clean, const float* noise, const float* sigma, const float* c_in, float* noisy,
                                    float* x_in, int B, long long n_per_sample, void* stream) {
  LDC_CHECK_PTR(clean);
  if (noise != nullptr && sigma == nullptr) return LDC_ERR_ARG;
  if (x_in != nullptr && c_in == nullptr) return LDC_ERR_ARG;
  if (noisy == nullptr && x_in == nullptr) return LDC_ERR_ARG;
  if (B <= 0 || n_per_sample <= 0) return LDC_ERR_ARG;
  const long long n = static_cast<long long>(B) * n_per_sample;
  if ((n + 255) / 256 > 0x7fffffffLL) return LDC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(edm_noise_inputs_kernel, dim3(ldc_cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), clean, noise,
                     sigma, c_in, noisy, x_in, n_per_sample, n);
  return ldc_launch_status();
}

extern "C" int ldc_edm_denoise(const float* noisy, const float* F, const float* c_skip, const float* c_out, float* denoised, int B,
                               int C, int T, int plane, int noisy_frames, int f_frames, int denoised_frames, void* stream) {
  LDC_CHECK_PTR(noisy);
  LDC_CHECK_PTR(F);
  LDC_CHECK_PTR(c_skip);
  LDC_CHECK_PTR(c_out);
  LDC_CHECK_PTR(denoised);
  if (B <= 0 || C <= 0 || T <= 0 || plane <= 0) return LDC_ERR_ARG;
  if (noisy_frames < T || f_frames < T || denoised_frames < T) return LDC_ERR_ARG;
  const long long run = static_cast<long long>(T) * plane;
  const long long n = static_cast<long long>(B) * C * run;
  if ((n + 255) / 256 > 0x7fffffffLL) return LDC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(edm_denoise_kernel, dim3(ldc_cdiv(n, 256)), dim3(256), 0, static_cast<hipStream_t>(stream), noisy, F, c_skip,
                     c_out, denoised, C, run, static_cast<long long>(noisy_frames) * plane, static_cast<long long>(f_frames) * plane,
                     static_cast<long long>(denoised_frames) * plane, n);
  return ldc_launch_status();
}

extern "C" int ldc_edm_denoise_loss(const float* noisy, const float* F, const float* target, const float* c_skip, const float* c_out,
                                    const float* weight, const float* lat_weight, float* table, float* denoised, int B, int C, int T,
                                    int H, int W, void* stream) {
  LDC_CHECK_PTR(noisy);
  LDC_CHECK_PTR(F);
  LDC_CHECK_PTR(target);
  LDC_CHECK_PTR(c_skip);
  LDC_CHECK_PTR(c_out);
  LDC_CHECK_PTR(weight);
  LDC_CHECK_PTR(table);
  if (B <= 0 || C <= 0 || T <= 0 || H <= 0 || W <= 0) return LDC_ERR_ARG;
  const long long plane = static_cast<long long>(H) * W;
  const long long per_sample = static_cast<long long>(C) * T;
  const long long planes = static_cast<long long>(B) * per_sample;
  if (plane > 0x7fffffffLL || per_sample > 0x7fffffffLL || (planes + LOSS_WAVES - 1) / LOSS_WAVES > 0x7fffffffLL) return LDC_ERR_UNSUPPORTED;
  hipLaunchKernelGGL(edm_denoise_loss_kernel, dim3(ldc_cdiv(planes, LOSS_WAVES)), dim3(64 * LOSS_WAVES), 0,
                     static_cast<hipStream_t>(stream), noisy, F, target, c_skip, c_out, weight, lat_weight, table, denoised, planes,
                     static_cast<int>(per_sample), W, static_cast<int>(plane));
  return ldc_launch_status();
}
