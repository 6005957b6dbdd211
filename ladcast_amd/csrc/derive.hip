// Derived fields of a decoded batch or of a truth / climatology table: wind speed, differences, vertical shear,
// computed from de-normalised channels and written as new planes, so that every scorer verifies them as channels.  The sibling of
// track_gather_kernel (track.hip): that one copies channels out with the inverse normalisation, this one computes new planes from them.
// Built with -ffp-contract=off: the difference must round as a subtraction of the de-normalised planes does.
#include <math.h>

#include "ensemble_common.h"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxPlanes = 16;  // distinct source channels per launch; a field list that needs more is cut into several launches

struct DeriveLaunch {  // launch argument: the fields of one launch and the distinct source channels they read
  int n_planes, n_fields, field0;  // field0: the first field's index in the caller's list = its output channel
  int plane[kMaxPlanes];           // source channel of each staged plane
  int kind[LDC_DERIVE_MAX_FIELDS];
  unsigned char in[LDC_DERIVE_MAX_FIELDS][4];  // per field: which staged plane each input is
};

__device__ __forceinline__ float derive_one(int kind, float a, float b, float c, float d) {
  if (kind == LDC_DERIVE_DIFF) return a - b;
  double x = a, y = b;
  if (kind == LDC_DERIVE_SHEAR) {
    x -= static_cast<double>(c);
    y -= static_cast<double>(d);
  }
  return static_cast<float>(sqrt(x * x + y * y));  // the squares are exact in double; sum, root and the cast round once each
}

// One thread holds V consecutive points of one (outer, lead) pair.  Every distinct source plane is loaded once, de-normalised and parked in
// the thread's own LDS column (the plane index is a run-time value: registers would go to scratch); the fields then read their inputs from
// there.  No thread reads another's column, so there is no barrier.  V == 4: 16-byte loads and stores, chosen by the host when HW % 4 == 0
// and every plane base is 16-byte aligned.
template <int V>
__global__ __launch_bounds__(kThreads) void derive_kernel(const float* __restrict__ src, long long outer_stride, long long lead_stride,
                                                          long long channel_stride, const int* __restrict__ slot,
                                                          const float* __restrict__ mean, const float* __restrict__ sd, float target_std,
                                                          long long HW, DeriveLaunch f, float* __restrict__ out,
                                                          long long out_outer_stride, long long out_lead_stride,
                                                          long long out_channel_stride) {
  extern __shared__ float stage[];  // [n_planes][kThreads][V]
  const long long p = (static_cast<long long>(blockIdx.x) * kThreads + threadIdx.x) * V;
  if (p >= HW) return;
  const int l = blockIdx.y, o = blockIdx.z;
  const long long sl = slot != nullptr ? slot[l] : l;
  const float* s = src + o * outer_stride + sl * lead_stride + p;
  float* mine = stage + threadIdx.x * V;
#pragma unroll 4
  for (int u = 0; u < f.n_planes; ++u) {
    const int c = f.plane[u];
    const float* q = s + c * channel_stride;
    float v[V];
    if constexpr (V == 4) {
      const f32x4 t = *reinterpret_cast<const f32x4*>(q);
      v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
      v[0] = q[0];
    }
    if (mean != nullptr) {
      const InvNorm n = make_inv_norm(target_std, sd, mean, c);
#pragma unroll
      for (int i = 0; i < V; ++i) v[i] = inv_norm(v[i], n);
    }
    float* w = mine + static_cast<long long>(u) * kThreads * V;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(w) = f32x4{v[0], v[1], v[2], v[3]};
    else w[0] = v[0];
  }
  float* dst = out + o * out_outer_stride + l * out_lead_stride + f.field0 * out_channel_stride + p;
  for (int k = 0; k < f.n_fields; ++k) {
    const int kind = f.kind[k];
    const float* a = mine + f.in[k][0] * kThreads * V;
    const float* b = mine + f.in[k][1] * kThreads * V;
    const float* c = mine + f.in[k][2] * kThreads * V;  // DIFF, SPEED: inputs 2 and 3 name plane 0 and are not used
    const float* d = mine + f.in[k][3] * kThreads * V;
    float r[V];
#pragma unroll
    for (int i = 0; i < V; ++i) r[i] = derive_one(kind, a[i], b[i], c[i], d[i]);
    float* w = dst + k * out_channel_stride;
    if constexpr (V == 4) *reinterpret_cast<f32x4*>(w) = f32x4{r[0], r[1], r[2], r[3]};
    else w[0] = r[0];
  }
}

int inputs_of(int kind) { return kind == LDC_DERIVE_SHEAR ? 4 : (kind == LDC_DERIVE_SPEED || kind == LDC_DERIVE_DIFF) ? 2 : 0; }

}  // namespace

extern "C" int ldc_sizeof_derive_desc(void) { return static_cast<int>(sizeof(ldc_derive_desc)); }

extern "C" int ldc_derive_fields(const float* src, long long outer_stride, long long lead_stride, long long channel_stride, const int* slot,
                                 const float* mean, const float* std_, float target_std, int n_outer, int L, int C, long long HW,
                                 const ldc_derive_desc* desc, int D, float* out, long long out_outer_stride, long long out_lead_stride,
                                 long long out_channel_stride, void* stream) {
  LDC_CHECK_PTR(src);
  LDC_CHECK_PTR(desc);
  LDC_CHECK_PTR(out);
  if ((mean != nullptr) != (std_ != nullptr)) return LDC_ERR_ARG;
  if (n_outer <= 0 || L <= 0 || C <= 0 || HW <= 0 || D < 1 || D > LDC_DERIVE_MAX_FIELDS) return LDC_ERR_ARG;
  if (outer_stride < 0 || lead_stride < 0 || channel_stride < 0 || out_outer_stride < 0 || out_lead_stride < 0 || out_channel_stride < 0)
    return LDC_ERR_ARG;
  for (int k = 0; k < D; ++k) {
    const int n = inputs_of(desc[k].kind);
    if (n == 0) return LDC_ERR_ARG;
    for (int j = 0; j < n; ++j)
      if (desc[k].ch[j] < 0 || desc[k].ch[j] >= C) return LDC_ERR_ARG;
  }
  const auto mult4 = [](long long v) { return (v & 3) == 0; };
  const bool vec = mult4(HW) && ldc_aligned16(src) && ldc_aligned16(out) && mult4(outer_stride) && mult4(lead_stride) && mult4(channel_stride) &&
                   mult4(out_outer_stride) && mult4(out_lead_stride) && mult4(out_channel_stride);
  const int V = vec ? 4 : 1;
  const long long blocks = (HW / V + kThreads - 1) / kThreads;
  if (blocks > 2147483647LL || L > 65535 || n_outer > 65535) return LDC_ERR_UNSUPPORTED;
  // the launches: fields in order, a new launch where the next field's channels would not fit the kMaxPlanes staged planes any more
  int k = 0;
  while (k < D) {
    DeriveLaunch f = {};
    f.field0 = k;
    for (; k < D; ++k) {
      const int n = inputs_of(desc[k].kind);
      int idx[4] = {0, 0, 0, 0}, planes = f.n_planes;
      bool fits = true;  // a field needs at most 4 planes: an empty launch always has room
      for (int j = 0; j < n && fits; ++j) {
        int u = 0;
        while (u < planes && f.plane[u] != desc[k].ch[j]) ++u;
        if (u == planes) {
          if (planes == kMaxPlanes) fits = false;
          else f.plane[planes++] = desc[k].ch[j];
        }
        idx[j] = u;
      }
      if (!fits) break;
      f.n_planes = planes;
      f.kind[f.n_fields] = desc[k].kind;
      for (int j = 0; j < 4; ++j) f.in[f.n_fields][j] = static_cast<unsigned char>(idx[j]);
      ++f.n_fields;
    }
    const dim3 grid(static_cast<unsigned>(blocks), L, n_outer);
    const size_t lds = static_cast<size_t>(f.n_planes) * kThreads * V * sizeof(float);
    if (vec)
      hipLaunchKernelGGL(derive_kernel<4>, grid, dim3(kThreads), lds, static_cast<hipStream_t>(stream), src, outer_stride, lead_stride,
                         channel_stride, slot, mean, std_, target_std, HW, f, out, out_outer_stride, out_lead_stride, out_channel_stride);
    else
      hipLaunchKernelGGL(derive_kernel<1>, grid, dim3(kThreads), lds, static_cast<hipStream_t>(stream), src, outer_stride, lead_stride,
                         channel_stride, slot, mean, std_, target_std, HW, f, out, out_outer_stride, out_lead_stride, out_channel_stride);
    const int st = ldc_launch_status();
    if (st != LDC_OK) return st;
  }
  return LDC_OK;
}
