// Derived fields that need horizontal derivatives: relative vorticity and divergence of a wind (u, v) on a
// latitude-longitude grid, from de-normalised channels of a decoded batch or of a truth / climatology table, written as new planes.  The
// sibling of derive_kernel (derive.hip), which is point-wise over a flat HW: this one needs H and W, the longitude wrap, the row neighbours
// and a rule for a pole row.  The definition is stated once, in include/ladcast_hip.h at ldc_derive_sphere; the host makes the per-row
// constants in float64 (ladcast_amd/evaluate/derived.py: sphere_row_tables), so kernel and host reference share their bits.
// Built with -ffp-contract=off: every double operation rounds on its own, in the order the header states.
#include "ensemble_common.h"

namespace {

constexpr int kWaves = 4;  // rows per workgroup: one wave owns one row
constexpr int kThreads = 64 * kWaves;

struct SphereLaunch {  // launch argument
  const float* src;
  long long outer_stride, lead_stride, channel_stride;
  const int* slot;
  const float* mean;
  const float* sd;
  float target_std;
  int H, W, row_blocks;  // row_blocks = ceil(H / kWaves): blockIdx.x = field * row_blocks + row block
  const double* tab;     // [4][H]: c, q, r, pc
  double k;
  float* out;
  long long out_outer_stride, out_lead_stride, out_channel_stride;
  int ch_a[LDC_DERIVE_MAX_FIELDS], ch_b[LDC_DERIVE_MAX_FIELDS];  // per field: the channels of a and b
  unsigned char neg_a[LDC_DERIVE_MAX_FIELDS];                    // divergence: a = -v
};

// one loaded value -> de-normalised in fp32 as the scorers do, negated where a = -v (exact), widened
__device__ __forceinline__ double widen(float v, bool inv, const InvNorm& n, bool neg) {
  if (inv) v = inv_norm(v, n);
  return static_cast<double>(neg ? -v : v);
}

// Wave w of a workgroup owns row j = row block * kWaves + w of one (field, lead, outer); its lanes walk the row V longitudes at a time.
// The i +- 1 and j +- 1 neighbours are read through the caches: every value of a is read by the rows above and below it, every value of b
// by its own row only, and the four rows of a workgroup request six distinct rows of a between them.  A pole row (r[j] == 0) is a branch of the wave that owns it.  V == 4: 16-byte loads and stores, chosen by the host when
// W % 4 == 0 (every row then starts on the 16-byte grid) and the bases and strides keep 16-byte alignment.
template <int V>
__global__ __launch_bounds__(kThreads) void sphere_kernel(SphereLaunch p) {
  const int lane = threadIdx.x & 63;
  const int f = blockIdx.x / p.row_blocks;
  const int j = (blockIdx.x - f * p.row_blocks) * kWaves + (threadIdx.x >> 6);
  const int H = p.H, W = p.W;
  if (j >= H) return;  // wave-uniform
  const int l = blockIdx.y, o = blockIdx.z;
  const long long sl = p.slot != nullptr ? p.slot[l] : l;
  const float* s = p.src + o * p.outer_stride + sl * p.lead_stride;
  const int ca = p.ch_a[f], cb = p.ch_b[f];
  const bool neg = p.neg_a[f] != 0, inv = p.mean != nullptr;
  InvNorm na = {}, nb = {};
  if (inv) {
    na = make_inv_norm(p.target_std, p.sd, p.mean, ca);
    nb = make_inv_norm(p.target_std, p.sd, p.mean, cb);
  }
  const float* pa = s + ca * p.channel_stride;
  const float* pb = s + cb * p.channel_stride;
  float* dst = p.out + o * p.out_outer_stride + l * p.out_lead_stride + f * p.out_channel_stride + static_cast<long long>(j) * W;
  const double* c = p.tab;
  const double rj = p.tab[2LL * H + j];
  if (rj == 0.0) {  // a pole row: the mean of a along the adjacent latitude circle times the cap factor, the same value at every longitude
    const int jp = j == 0 ? 1 : j - 1;
    const float* row = pa + static_cast<long long>(jp) * W;
    double acc = 0.0;
    for (int i = lane; i < W; i += 64) acc += widen(row[i], inv, na, neg);
    acc = wave_sum(acc);  // the xor butterfly 32 .. 1: every lane ends with the same bits
    const float v = static_cast<float>(acc / static_cast<double>(W) * p.tab[3LL * H + j]);
    for (int i = lane; i < W; i += 64) dst[i] = v;
    return;
  }
  const int jn = j + 1 < H ? j + 1 : H - 1, js = j > 0 ? j - 1 : 0;
  const double cn = c[jn], cs = c[js], qj = p.tab[static_cast<long long>(H) + j], k = p.k;
  const float* rb = pb + static_cast<long long>(j) * W;
  const float* rn = pa + static_cast<long long>(jn) * W;
  const float* rs = pa + static_cast<long long>(js) * W;
  for (int i = lane * V; i < W; i += 64 * V) {
    float bv[V + 2], an[V], as[V];  // bv: b[j][i - 1 .. i + V], wrapped
    if constexpr (V == 4) {
      const f32x4 tb = *reinterpret_cast<const f32x4*>(rb + i), tn = *reinterpret_cast<const f32x4*>(rn + i),
                  ts = *reinterpret_cast<const f32x4*>(rs + i);
      bv[1] = tb.x, bv[2] = tb.y, bv[3] = tb.z, bv[4] = tb.w;
      an[0] = tn.x, an[1] = tn.y, an[2] = tn.z, an[3] = tn.w;
      as[0] = ts.x, as[1] = ts.y, as[2] = ts.z, as[3] = ts.w;
    } else {
      bv[1] = rb[i], an[0] = rn[i], as[0] = rs[i];
    }
    bv[0] = rb[i == 0 ? W - 1 : i - 1];
    bv[V + 1] = rb[i + V == W ? 0 : i + V];
    double b[V + 2];
#pragma unroll
    for (int u = 0; u < V + 2; ++u) b[u] = widen(bv[u], inv, nb, false);
    float res[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
      const double dl = (b[u + 2] - b[u]) * k;
      const double dp = (widen(an[u], inv, na, neg) * cn - widen(as[u], inv, na, neg) * cs) * qj;
      res[u] = static_cast<float>((dl - dp) * rj);
    }
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(dst + i) = f32x4{res[0], res[1], res[2], res[3]};
    else dst[i] = res[0];
  }
}

}  // namespace

extern "C" int ldc_sizeof_sphere_desc(void) { return static_cast<int>(sizeof(ldc_sphere_desc)); }

extern "C" int ldc_derive_sphere(const float* src, long long outer_stride, long long lead_stride, long long channel_stride, const int* slot,
                                 const float* mean, const float* std_, float target_std, int n_outer, int L, int C, int H, int W,
                                 const double* row_tables, double k, const ldc_sphere_desc* desc, int D, float* out,
                                 long long out_outer_stride, long long out_lead_stride, long long out_channel_stride, void* stream) {
  LDC_CHECK_PTR(src);
  LDC_CHECK_PTR(row_tables);
  LDC_CHECK_PTR(desc);
  LDC_CHECK_PTR(out);
  if ((mean != nullptr) != (std_ != nullptr)) return LDC_ERR_ARG;
  if (n_outer <= 0 || L <= 0 || C <= 0 || H < 2 || W < 3 || D < 1 || D > LDC_DERIVE_MAX_FIELDS) return LDC_ERR_ARG;
  if (outer_stride < 0 || lead_stride < 0 || channel_stride < 0 || out_outer_stride < 0 || out_lead_stride < 0 || out_channel_stride < 0)
    return LDC_ERR_ARG;
  SphereLaunch p = {};
  for (int f = 0; f < D; ++f) {
    const int u = desc[f].ch[0], v = desc[f].ch[1];
    if (desc[f].kind != LDC_SPHERE_VORTICITY && desc[f].kind != LDC_SPHERE_DIVERGENCE) return LDC_ERR_ARG;
    if (u < 0 || u >= C || v < 0 || v >= C) return LDC_ERR_ARG;
    const bool div = desc[f].kind == LDC_SPHERE_DIVERGENCE;
    p.ch_a[f] = div ? v : u;
    p.ch_b[f] = div ? u : v;
    p.neg_a[f] = div ? 1 : 0;
  }
  const long long row_blocks = (static_cast<long long>(H) + kWaves - 1) / kWaves;
  if (L > 65535 || n_outer > 65535 || row_blocks * D > 2147483647LL) return LDC_ERR_UNSUPPORTED;
  const auto mult4 = [](long long v) { return (v & 3) == 0; };
  const bool vec = mult4(W) && ldc_aligned16(src) && ldc_aligned16(out) && mult4(outer_stride) && mult4(lead_stride) && mult4(channel_stride) &&
                   mult4(out_outer_stride) && mult4(out_lead_stride) && mult4(out_channel_stride);
  p.src = src, p.outer_stride = outer_stride, p.lead_stride = lead_stride, p.channel_stride = channel_stride;
  p.slot = slot, p.mean = mean, p.sd = std_, p.target_std = target_std;
  p.H = H, p.W = W, p.row_blocks = static_cast<int>(row_blocks);
  p.tab = row_tables, p.k = k, p.out = out;
  p.out_outer_stride = out_outer_stride, p.out_lead_stride = out_lead_stride, p.out_channel_stride = out_channel_stride;
  const dim3 grid(static_cast<unsigned>(p.row_blocks) * D, L, n_outer);
  if (vec) hipLaunchKernelGGL(sphere_kernel<4>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), p);
  else hipLaunchKernelGGL(sphere_kernel<1>, grid, dim3(kThreads), 0, static_cast<hipStream_t>(stream), p);
  return ldc_launch_status();
}
