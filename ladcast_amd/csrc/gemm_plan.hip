// Host planner of the grouped GEMMs: which kernel instance runs a group (LDS-DMA ring kernel of gemm_bf16x3_v3.hip | register-staged
// stream-K kernel of gemm_streamk.hip, tile height, one launch or one per problem) and how each launch's (tile, k-step) units are cut
// over the CUs.  Pure host code that never touches a data pointer beyond its NULL / alignment checks: the entry points plan, then run
// the plan; ldc_gemm_grouped_plan returns the same plan without launching (the GEMM's counterpart of ldc_sphere_conv_plan).
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "common.h"

namespace {

constexpr int BN = 128, BK = 32;  // tile width and k-step of every grouped kernel
constexpr int MAXP = LDC_GEMM_MAX_PROBLEMS;
constexpr int LDC_SPLIT_GROUP = -100;  // internal: "launch this group's problems one by one" (plan_ring_split)

int plan_ring(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, const void* workspace, long long workspace_bytes,
              int bm, int terms, const ldc_conv_params* cp, bool may_split_group, ldc_gemm_launch_plan* out) {
  const bool conv = cp != nullptr;
  const int SLOT_FLOATS = bm * BN;
  constexpr int CUS = 256;  // one workgroup per CU
  long long U = 0, tiles = 0;
  for (int i = 0; i < n; ++i) {
    const ldc_gemm_problem& q = problems[i];
    LDC_CHECK_PTR(q.A);
    LDC_CHECK_PTR(q.W);
    LDC_CHECK_PTR(q.C);
    const ldc_gemm_desc& d = q.d;
    if (d.M <= 0 || d.N <= 0 || d.K <= 0 || d.batch <= 0) return LDC_ERR_ARG;
    if (d.K % (terms == 1 ? 2 * BK : BK)) return LDC_ERR_UNSUPPORTED;  // a 128-byte k-step: 64 plain-bf16 / 32 split / 32 fp32 values
    if (terms == 0) {  // exact fp32: plain fp32 rows in, fp32 rows out, a contiguous [N][K] weight
      if (d.flags != 0 || d.ldw != d.K) return LDC_ERR_UNSUPPORTED;
    } else {
      if (!(d.flags & LDC_GEMM_A_SPLIT)) return LDC_ERR_UNSUPPORTED;
    }
    LDC_CHECK_ALIGN16(q.A);
    LDC_CHECK_ALIGN16(q.W);
    if (terms == 0) {
      if ((d.lda & 3) || (d.a_bs & 3)) return LDC_ERR_UNSUPPORTED;  // the caller falls back to the register-staged kernel
    } else {
      if ((d.lda & 7) || (d.a_bs & 7) || (reinterpret_cast<unsigned long long>(q.A) & 31ull)) return LDC_ERR_ALIGN;
    }
    if (d.act < LDC_ACT_NONE || d.act > LDC_ACT_RELU) return LDC_ERR_UNSUPPORTED;
    ldc_gemm_problem_plan& P = out->pr[i];
    {
      auto al16 = [](const void* q_) { return (reinterpret_cast<unsigned long long>(q_) & 15ull) == 0; };
      bool v4 = (d.N % 4 == 0) && (d.ldc % 4 == 0) && (d.c_bs % 4 == 0) && al16(q.C);
      if (q.bias) v4 = v4 && al16(q.bias);
      if (q.gate) v4 = v4 && al16(q.gate) && (d.gate_bs % 4 == 0);
      if (q.R) v4 = v4 && al16(q.R) && (d.ldr % 4 == 0) && (d.r_bs % 4 == 0);
      P.vec4 = v4 ? 1 : 0;
      P.c_split = (terms != 0 && (d.flags & LDC_GEMM_C_SPLIT)) ? (terms == 3 ? LDC_FMT_SPLIT : LDC_FMT_BF16) : 0;
      // operand rows out: N % 4 == 0 (v4), the pad half of a last half-filled 8-column group is zeroed
      if (P.c_split && !(v4 && d.ldc % 8 == 0 && d.ldc >= ((d.N + 7) & ~7) &&
                         d.c_bs % 8 == 0 && (reinterpret_cast<unsigned long long>(q.C) & 31ull) == 0))
        return LDC_ERR_ALIGN;
    }
    if (epi != nullptr && epi[i].heads > 0) {
      const ldc_qkv_epilogue& e = epi[i];
      auto al16 = [](const void* q_) { return (reinterpret_cast<unsigned long long>(q_) & 15ull) == 0; };
      if (d.N != 3 * e.heads * BN || d.act != LDC_ACT_NONE || q.gate != nullptr || q.R != nullptr) return LDC_ERR_ARG;
      if ((e.wq == nullptr) != (e.wk == nullptr) || e.reserved != nullptr || e.rope_row0 < 0) return LDC_ERR_ARG;
      if (terms == 0) {  // plain fp32 rows out
        if ((d.ldc & 3) || (d.c_bs & 3) || !al16(q.C)) return LDC_ERR_ALIGN;
      } else {
        if ((d.ldc & 7) || (d.c_bs & 7) || (reinterpret_cast<unsigned long long>(q.C) & 31ull)) return LDC_ERR_ALIGN;
      }
      if (!al16(e.wq) || !al16(e.wk) || !al16(e.rope) || (q.bias && !al16(q.bias))) return LDC_ERR_ALIGN;
      P.qkv_heads = e.heads;
      P.rope_row0 = e.rope_row0;
      P.qk_w[0] = e.wq;
      P.qk_w[1] = e.wk;
      P.rope_cs = e.rope;
      P.eps = e.eps;
      P.qscale = e.qscale != 0.f ? e.qscale : 0.08838834764831845f * 1.4426950408889634f;
    }
    P.tm = ldc_cdiv(d.M, bm);
    P.tn = ldc_cdiv(d.N, BN);
    P.kt = d.K / (terms == 1 ? 2 * BK : BK);
    P.unit0 = U;
    P.tile0 = tiles;
    {
      // super-row height: an XCD's share is ~T8 = tiles / 8 consecutive tiles = rm row panels x T8 / rm column panels; per k-step
      // it pulls rm * BM + (T8 / rm) * BN operand rows through the fabric -> minimum at rm = sqrt(T8 * BN / BM); super-rows of
      // (nearly) equal height.  Only when the activation panel is what the one-super-row order over-fetches (every XCD streams all
      // of A): measured (profiles/r02_c_gemm_tile_order_ab.log) 2250 x 1536 x 7680 -3.4 % time / -31 % fabric
      // bytes and 18000 x 1536 x 7680 -10 %, but +3 % on 2250 x 4608 / 10752 x 1536, whose 14 MB A panel stays cached anyway.
      // LDC_BF16X3_RM (measurement aid, read per call): force it; 0 = one super-row
      P.rm = P.tm;
      // (a conv's taps re-read the same pixels: its panel is M x ldx, and neighbouring row tiles share their halo rows)
      const double a_bytes = conv ? static_cast<double>(d.M) * d.lda * 4.0 : static_cast<double>(d.batch) * d.M * d.K * 4.0;
      if (a_bytes >= 48e6) {
        const double t8 = static_cast<double>(d.batch) * P.tm * P.tn / 8.0;
        const double want = sqrt(t8 * BN / bm);
        int nsr = static_cast<int>(P.tm / (want > 1.0 ? want : 1.0) + 0.5);
        if (nsr < 1) nsr = 1;
        if (nsr > P.tm) nsr = P.tm;
        P.rm = ldc_cdiv(P.tm, nsr);
      }
      if (const char* e = LDC_AB_GETENV("LDC_BF16X3_RM")) {
        const int f = atoi(e);
        if (f >= 0) P.rm = (f == 0 || f > P.tm) ? P.tm : f;
      }
    }
    const long long t = static_cast<long long>(d.batch) * P.tm * P.tn;
    tiles += t;
    U += t * P.kt;
  }
  if (tiles > LDC_GEMM_COUNTER_BYTES / 4 - 16) return LDC_ERR_UNSUPPORTED;  // in-launch reduction only; last 64 B: zero page
  const long long slot_bytes = SLOT_FLOATS * static_cast<long long>(sizeof(float));
  // grid size: (phase-aligned divisor of tiles * s when every problem has the same k-depth)
  long long G = CUS;
  {
    bool same_kt = true;
    for (int i = 1; i < n; ++i) same_kt = same_kt && (out->pr[i].kt == out->pr[0].kt);
    long long best = 0;
    if (same_kt) {
      const int kt = out->pr[0].kt;
      // more workgroups win unless they are bought with many more pieces per tile (a hand-off each): 2 % per extra split factor.
      // 288 tiles x 320 k-steps (the 1.6B model's single-block out projection): 192 ranges at s = 2, 240 at s = 5 - 279 -> 269 us
      double best_score = 0.0;
      for (int sfac = 1; sfac <= 8; ++sfac) {
        if (kt % sfac || (sfac > 1 && kt / sfac < 8)) continue;  // whole tiles (sfac 1) at any depth
        const long long items = tiles * sfac;
        long long gd = items < CUS ? items : CUS;
        while (gd > 1 && items % gd) --gd;
        const double score = static_cast<double>(gd) * (1.0 - 0.02 * (sfac - 1));
        if (score > best_score) {
          best_score = score;
          best = gd;
        }
      }
    }
    long long few = 0;  // few tiles (the 84-column output head: 15 tiles): aligned split-K over more workgroups
    if (same_kt && best < 160) {
      const int kt = out->pr[0].kt;
      for (int sfac = 8; sfac >= 2; --sfac)
        if (kt % sfac == 0 && kt / sfac >= 8 && tiles * sfac <= CUS) {
          few = tiles * sfac;
          break;
        }
    }
    // Round 4: a GROUP whose tile count has no k-aligned cut onto >= 160 workgroups (1.6B dual blocks: (15 + 4) x 16 = 304 tiles of
    // k-depth 2^j - every aligned grid is a multiple of 19 that divides 304 s: 152) used to take the unaligned ranges below, which cost
    // the split modes 40 % (out / down projection of the 1.6B dual block: 205 / 213 TFLOP/s).  Its problems one by one cut well
    // (pred: 240 tiles = 240 workgroups; cond: 64 tiles x 4 k-pieces = 256): the dispatcher launches them separately.
    if (may_split_group && terms != 0 && n > 1 && best < 160 && few == 0) return LDC_SPLIT_GROUP;
    if (best >= 160) {
      G = best;
    } else if (few > 0) {
      G = few;  // measured on 1800 x 84 x 1536: 24.7 us at the stream-K default (36 ranges), 18.0 at 90
    } else {
      const double kt_avg = static_cast<double>(U) / static_cast<double>(tiles);
      long long umin = static_cast<long long>(sqrt(kt_avg * 8.0) + 0.5);
      if (umin < 1) umin = 1;
      const long long gmax = U / umin > 0 ? U / umin : 1;
      if (gmax < G) G = gmax;
    }
  }
  if (terms == 0) {  // (the DCAE's fp32 convs too: 8.09 / 8.83 -> 7.73 / 8.41 ms per frame, profiles/r04_l_dcae_unit_ranges_ab.txt; the split modes lose 10 % with it)
    // exact fp32 (round 4): ALWAYS one unit range per CU, cut wherever U / 256 falls.  The fp32 k-step is matrix-pipe bound (5x the split
    // kernel's MFMA time per k-step), so the L2 lockstep that made unaligned ranges 40 % slower in the split mode does not matter here and
    // the chip is not at its power cap: idle CUs cost their full share.  375M in fp32 mode, same box: 111.3 -> 118.5 TFLOP/s per GEMM launch,
    // 2.82 -> 2.96 member-steps/s (aligned 240 / 248 ranges: 111.6 / 115.0; profiles/r04_k_fp32_unit_ranges.txt)
    if (U >= 4 * CUS) G = CUS;
  }
  static const char* const force_g = LDC_AB_GETENV("LDC_BF16X3_G");  // measurement aid (read once): force the number of unit ranges
  if (force_g) {
    const long long g_ = atoll(force_g);
    if (g_ > 0 && g_ <= CUS) G = g_;
  }
  if (U < G) G = U;
  if (workspace == nullptr) return LDC_ERR_ARG;
  if (workspace_bytes < LDC_GEMM_COUNTER_BYTES + 2 * slot_bytes) return LDC_ERR_ARG;
  {
    const long long fit = (workspace_bytes - LDC_GEMM_COUNTER_BYTES) / (2 * slot_bytes);
    if (fit < G) G = fit;
  }
  LDC_CHECK_ALIGN16(workspace);
  if (U >= (1LL << 31)) return LDC_ERR_UNSUPPORTED;  // 32-bit unit arithmetic in the kernel
#ifdef LDC_AB_BUILD
  {  // A/B build only: LDC_GEMM_DEBUG_G=1 prints every launch's cut (n problems, tiles, k-depth, tile rows, unit ranges, units per range)
    static const bool dbg = getenv("LDC_GEMM_DEBUG_G") != nullptr;
    if (dbg)
      fprintf(stderr, "ldc_gemm cut: terms %d conv %d n %d tiles %lld kt0 %d BM %d G %lld U %lld %s\n", terms, int(conv), n, tiles, out->pr[0].kt, bm, G, U,
              (U % G == 0 && (U / G) % out->pr[0].kt == 0) ? "whole tiles" : (U % G == 0 ? "equal ranges" : "UNALIGNED"));
  }
#endif
  out->G = static_cast<int>(G);
  out->U = U;
  out->upg = static_cast<unsigned>(U / G);
  out->urem = static_cast<unsigned>(U % G);
  out->tiles = tiles;
  return LDC_OK;
}

// the register-staged stream-K kernels (gemm_streamk.hip): 128-row tiles, 2 workgroups per CU, unit range g = [g U / G, (g + 1) U / G)
int plan_regstage(const ldc_gemm_problem* problems, int n, const void* workspace, long long workspace_bytes, bool split_bf16,
                  ldc_gemm_launch_plan* out) {
  constexpr int BM = 128, SLOT_FLOATS = BM * BN;
  LDC_CHECK_PTR(problems);
  if (n <= 0 || n > MAXP) return LDC_ERR_ARG;
  long long U = 0, tiles = 0;
  for (int i = 0; i < n; ++i) {
    const ldc_gemm_problem& q = problems[i];
    LDC_CHECK_PTR(q.A);
    LDC_CHECK_PTR(q.W);
    LDC_CHECK_PTR(q.C);
    const ldc_gemm_desc& d = q.d;
    if (d.M <= 0 || d.N <= 0 || d.K <= 0 || d.batch <= 0) return LDC_ERR_ARG;
    LDC_CHECK_ALIGN16(q.A);
    LDC_CHECK_ALIGN16(q.W);
    if ((d.K & 3) || (d.lda & 3) || (d.a_bs & 3)) return LDC_ERR_ALIGN;
    if (split_bf16 ? (d.K & 7) != 0 : (d.ldw & 3) != 0) return LDC_ERR_ALIGN;
    if (d.act < LDC_ACT_NONE || d.act > LDC_ACT_RELU) return LDC_ERR_UNSUPPORTED;
    if ((d.flags & ~LDC_GEMM_F32_REGSTAGE) != 0) return LDC_ERR_UNSUPPORTED;  // split activation formats: the LDS-DMA bf16x3 kernel only (K % 32 == 0)
    ldc_gemm_problem_plan& P = out->pr[i];
    P.tm = ldc_cdiv(d.M, BM);
    P.tn = ldc_cdiv(d.N, BN);
    P.kt = ldc_cdiv(d.K, BK);
    P.rm = P.tm;
    P.unit0 = U;
    P.tile0 = tiles;
    const long long t = static_cast<long long>(d.batch) * P.tm * P.tn;
    tiles += t;
    U += t * P.kt;
  }
  if (tiles > LDC_GEMM_COUNTER_BYTES / 4 - 16) return LDC_ERR_UNSUPPORTED;  // one hand-off counter per tile (1 MiB block: 262 128 tiles)
  const long long slot_bytes = SLOT_FLOATS * static_cast<long long>(sizeof(float));
  long long G = 512;
  {
    // Balance k-steps per workgroup against slabs per split tile: time ~ (U/G) t_unit + (kt G/U) t_slab is
    // smallest at U/G = sqrt(kt t_slab / t_unit); t_slab / t_unit ~ 2 (fp32 units) or ~ 7 (bf16x3 units).
    const double kt_avg = static_cast<double>(U) / static_cast<double>(tiles);
    long long umin = static_cast<long long>(sqrt(kt_avg * (split_bf16 ? 7.0 : 2.0)) + 0.5);
    if (umin < 1) umin = 1;
    const long long gmax = U / umin > 0 ? U / umin : 1;
    if (gmax < G) G = gmax;
  }
  if (U < G) G = U;
  if (workspace == nullptr || workspace_bytes < LDC_GEMM_COUNTER_BYTES + 2 * slot_bytes) return LDC_ERR_ARG;
  {
    const long long fit = (workspace_bytes - LDC_GEMM_COUNTER_BYTES) / (2 * slot_bytes);
    if (fit < G) G = fit;  // not enough scratch for 2 slabs per workgroup: shrink the grid to what fits
  }
  LDC_CHECK_ALIGN16(workspace);
  out->G = static_cast<int>(G);
  out->U = U;
  out->upg = static_cast<unsigned>(U / G);
  out->urem = static_cast<unsigned>(U % G);
  out->tiles = tiles;
  return LDC_OK;
}

// exact-fp32 group on the ring kernel (terms = 0); LDC_ERR_UNSUPPORTED -> plan_group takes the register-staged stream-K kernel instead
// (K % 32 != 0, strided weights, unaligned rows)
int plan_ring_f32(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, const void* workspace, long long workspace_bytes,
                  ldc_gemm_group_plan* g) {
  LDC_CHECK_PTR(problems);
  if (n <= 0 || n > MAXP) return LDC_ERR_ARG;
  for (int i = 0; i < n; ++i)  // the caller's choice (include/ladcast_hip.h): this launch stays on the register-staged kernel
    if (problems[i].d.flags & LDC_GEMM_F32_REGSTAGE) return LDC_ERR_UNSUPPORTED;
  auto al16 = [](const void* q_) { return q_ != nullptr && (reinterpret_cast<unsigned long long>(q_) & 15ull) == 0; };
  // what the register-staged kernel accepts and this one does not goes there, not back to the caller as an error
  if (!al16(workspace) || workspace_bytes < LDC_GEMM_COUNTER_BYTES + 2ll * 256 * BN * static_cast<long long>(sizeof(float)))
    return LDC_ERR_UNSUPPORTED;
  for (int i = 0; i < n; ++i) {
    const ldc_gemm_desc& d = problems[i].d;
    if (d.M <= 0 || d.N <= 0 || d.K <= 0 || d.batch <= 0) return LDC_ERR_ARG;
    if (!al16(problems[i].A) || !al16(problems[i].W)) return LDC_ERR_UNSUPPORTED;
  }
  // 128-row tiles only: a tile is 2.7x the split kernel's MFMA time, so balance matters more than the halved W traffic per FLOP of
  // the 256-row tile (375M model in fp32 mode, same box: 113.6 TFLOP/s against 111.0 with 256 rows forced; profiles/r03_j_*)
  g->bm[0] = 128;
#ifdef LDC_AB_BUILD
  static const char* const force_bm = getenv("LDC_F32_RING_BM");  // A/B build only: 256-row tiles for the exact-fp32 GEMMs
  if (force_bm && atoi(force_bm) == 256) g->bm[0] = 256;
#endif
  g->count[0] = n;
  return plan_ring(problems, epi, n, workspace, workspace_bytes, g->bm[0], 0, nullptr, false, &g->launch[0]);
}

// split-bf16 / single-term group on the ring kernel; LDC_ERR_UNSUPPORTED when a problem does not fit it (plan_group takes the
// register-staged kernel instead)
int plan_ring_split(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, const void* workspace, long long workspace_bytes,
                    ldc_gemm_group_plan* g) {
  LDC_CHECK_PTR(problems);
  if (n <= 0 || n > MAXP) return LDC_ERR_ARG;
  // half-height tiles while 256-row tiles would not fill the chip twice over (both heights run 8 waves here, so the
  // half-height tile costs no MFMA efficiency, only twice the W traffic per FLOP); LDC_BF16X3_BM forces one
  static const char* const force_thr = LDC_AB_GETENV("LDC_BF16X3_SMALL_TILES");  // measurement aid, read once: the cross-over below
  static const char* const force_bm = LDC_AB_GETENV("LDC_BF16X3_BM");  // measurement aid, read once
  auto tiles256 = [](const ldc_gemm_desc& d) { return static_cast<long long>(d.batch) * ldc_cdiv(d.M, 256) * ldc_cdiv(d.N, BN); };
  auto tile_rows = [](long long t256) {
    if (force_bm) return atoi(force_bm) == 128 ? 128 : 256;
    return t256 < (force_thr ? atoll(force_thr) : 400) ? 128 : 256;  // measured cross-over on the 375M model launches (tools/gemm_sustained.py, both heights forced)
  };
  long long group256 = 0;
  for (int i = 0; i < n; ++i) {
    const ldc_gemm_desc& d = problems[i].d;
    if (d.M <= 0 || d.N <= 0 || d.batch <= 0) return LDC_ERR_ARG;
    if (!(d.flags & LDC_GEMM_A_SPLIT)) return LDC_ERR_UNSUPPORTED;
    if (((d.flags ^ problems[0].d.flags) & LDC_GEMM_BF16_1TERM) != 0) return LDC_ERR_ARG;  // one arithmetic per launch
    group256 += tiles256(d);
  }
  g->terms = (problems[0].d.flags & LDC_GEMM_BF16_1TERM) != 0 ? 1 : 3;
  g->bm[0] = tile_rows(group256);
  g->count[0] = n;
  const int st = plan_ring(problems, epi, n, workspace, workspace_bytes, g->bm[0], g->terms, nullptr, true, &g->launch[0]);
  if (st != LDC_SPLIT_GROUP) return st;
  // (no partial output on a bad argument: plan_ring returns LDC_SPLIT_GROUP only after it has validated EVERY problem of the group - the
  // per-problem checks run before the cut is chosen - and every single launch is planned, workspace checks included, before anything
  // is queued)
  g->launches = n;
  for (int i = 0; i < n; ++i) {  // the group has no good aligned cut: its problems one after the other (independent; same stream)
    g->first[i] = i;
    g->count[i] = 1;
    g->bm[i] = tile_rows(tiles256(problems[i].d));
    g->launch[i] = ldc_gemm_launch_plan{};
    const int sti = plan_ring(problems + i, epi ? epi + i : nullptr, 1, workspace, workspace_bytes, g->bm[i], g->terms, nullptr, false, &g->launch[i]);
    if (sti != LDC_OK) return sti;
  }
  return LDC_OK;
}

// the plan of one call of a grouped entry point: ldc_gemm_grouped (split_bf16 = false) | ldc_gemm_grouped_bf16x3, or with `qkv` their
// fused-QKV forms, whose epilogue exists on the ring kernel only (LDC_ERR_UNSUPPORTED goes back to the caller)
int plan_group(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, bool qkv, int n, const void* workspace,
               long long workspace_bytes, bool split_bf16, ldc_gemm_group_plan* g) {
  *g = ldc_gemm_group_plan{};
  g->kernel = LDC_GEMM_KERNEL_RING;
  g->launches = 1;
  if (qkv) LDC_CHECK_PTR(epi);
  // Exact fp32 (round 3): the LDS-DMA ring kernel with fp32 operand rows and the fp32 matrix instruction where the shapes allow
  // (K % 32 == 0, contiguous weights, 16-byte rows).  Split bf16: pre-split activations (LDC_GEMM_A_SPLIT) and K % 32 == 0 - every launch
  // of the models: the 16x16x32 ring kernel.  Anything else (fp32 activations, K % 32 != 0): the register-staged kernel, which splits in
  // its loop.  A/B build only: LDC_BF16X3_KERNEL=regstage forces the register-staged kernel.
  int force = 0;
#ifdef LDC_AB_BUILD
  static const int force_env = [] {
    const char* e = getenv("LDC_BF16X3_KERNEL");
    return (e != nullptr && strcmp(e, "regstage") == 0) ? 1 : 0;
  }();
  force = split_bf16 && !qkv ? force_env : 0;
#endif
  if (force == 0) {
    const int st = split_bf16 ? plan_ring_split(problems, epi, n, workspace, workspace_bytes, g)
                              : plan_ring_f32(problems, epi, n, workspace, workspace_bytes, g);
    if (st != LDC_ERR_UNSUPPORTED || qkv) return st;
  }
  g->kernel = LDC_GEMM_KERNEL_REGSTAGE;
  g->terms = split_bf16 ? 3 : 0;
  g->launches = 1;
  g->count[0] = n;
  g->bm[0] = 128;
  g->launch[0] = ldc_gemm_launch_plan{};
  return plan_regstage(problems, n, workspace, workspace_bytes, split_bf16, &g->launch[0]);
}

int run_group(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, bool qkv, int n, void* workspace, long long workspace_bytes,
              bool split_bf16, void* stream) {
  ldc_gemm_group_plan g;
  const int st = plan_group(problems, epi, qkv, n, workspace, workspace_bytes, split_bf16, &g);
  if (st != LDC_OK) return st;
  if (g.kernel == LDC_GEMM_KERNEL_REGSTAGE) return ldc_gemm_regstage_launch(problems, n, g.launch[0], split_bf16, workspace, stream);
  for (int l = 0; l < g.launches; ++l) {
    const int sl = ldc_gemm_ring_launch(problems + g.first[l], g.count[l], g.launch[l], g.bm[l], g.terms, nullptr, workspace, stream);
    if (sl != LDC_OK) return sl;
  }
  return LDC_OK;
}

}  // namespace

int ldc_gemm_plan_ring(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, const void* workspace, long long workspace_bytes,
                       int bm, int terms, const ldc_conv_params* cp, ldc_gemm_launch_plan* out) {
  *out = ldc_gemm_launch_plan{};
  return plan_ring(problems, epi, n, workspace, workspace_bytes, bm, terms, cp, false, out);
}

extern "C" int ldc_gemm_grouped(const ldc_gemm_problem* problems, int n, void* workspace, long long workspace_bytes, void* stream) {
  return run_group(problems, nullptr, false, n, workspace, workspace_bytes, false, stream);
}

extern "C" int ldc_gemm_grouped_bf16x3(const ldc_gemm_problem* problems, int n, void* workspace, long long workspace_bytes, void* stream) {
  return run_group(problems, nullptr, false, n, workspace, workspace_bytes, true, stream);
}

// exact-fp32 QKV projection with per-head RMSNorm + rotary embedding as its epilogue, plain fp32 rows out (include/ladcast_hip.h);
// LDC_ERR_UNSUPPORTED (K % 32 != 0, strided weights, unaligned rows): run ldc_gemm_grouped and ldc_qk_rmsnorm_rope instead
extern "C" int ldc_gemm_grouped_qkv_f32(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, void* workspace,
                                        long long workspace_bytes, void* stream) {
  return run_group(problems, epi, true, n, workspace, workspace_bytes, false, stream);
}

// QKV projection with the attention operand rows as output (include/ladcast_hip.h); only the ring kernel has that epilogue:
// LDC_ERR_UNSUPPORTED (K % 32 != 0, fp32 activations) means "run the plain GEMM and ldc_attn_qkv_prepare_split instead"
extern "C" int ldc_gemm_grouped_bf16x3_qkv(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, void* workspace,
                                           long long workspace_bytes, void* stream) {
  return run_group(problems, epi, true, n, workspace, workspace_bytes, true, stream);
}

extern "C" int ldc_sizeof_gemm_plan(void) { return static_cast<int>(sizeof(ldc_gemm_plan)); }

extern "C" int ldc_gemm_grouped_plan(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, int split_bf16,
                                     long long workspace_bytes, ldc_gemm_plan* out) {
  LDC_CHECK_PTR(out);
  alignas(16) static const char any_workspace[16] = {};  // the query has no workspace: every 16-byte aligned address plans alike
  ldc_gemm_group_plan g;
  const int st = plan_group(problems, epi, epi != nullptr, n, any_workspace, workspace_bytes, split_bf16 != 0, &g);
  *out = ldc_gemm_plan{};
  if (st != LDC_OK) return st;
  out->kernel = g.kernel;
  out->terms = g.terms;
  out->launches = g.launches;
  for (int l = 0; l < g.launches; ++l) {
    const ldc_gemm_launch_plan& L = g.launch[l];
    out->tile_rows[l] = g.bm[l];
    out->workgroups[l] = L.G;
    out->units[l] = L.U;
    out->tiles[l] = L.tiles;
    out->units_per_group[l] = static_cast<int>(L.upg);
    out->units_rem[l] = static_cast<int>(L.urem);
    for (int i = 0; i < g.count[l]; ++i) {
      const ldc_gemm_problem_plan& P = L.pr[i];
      const int p = g.first[l] + i;
      out->tile_rows_m[p] = P.tm;
      out->tile_cols_n[p] = P.tn;
      out->k_steps[p] = P.kt;
      out->super_row[p] = P.rm;
    }
  }
  return LDC_OK;
}
