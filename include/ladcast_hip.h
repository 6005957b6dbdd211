/* ladcast_hip.h -- C ABI of libladcast_hip.so (MI355X / gfx950 HIP kernels for the
 * LaDCast autoregressive latent-diffusion rollout).
 *
 * The reference (tonyzyl/ladcast) is pure Python and has NO FFI: its plug-in surface
 * is Python duck typing (pipeline API, diffusers-style model/scheduler surface,
 * attention-processor protocol).  This header is therefore
 * build-defined.  Each entry point names the reference code it replaces
 * (file:line under the reference tree) so a maintainer can see which torch ops
 * the call stands in for.  INTEGRATION.md shows the ctypes binding.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer borrowed from the caller (the caller --
 *     normally torch -- owns all memory; the library never allocates);
 *   - `stream` is a hipStream_t passed as void* (0 = default stream); all work is
 *     enqueued on it, nothing synchronises the host; safe under hipGraph capture;
 *   - return value: 0 on success, LDC_ERR_* (<0) on bad arguments, or
 *     -(1000 + hipError_t) if the launch failed.  Nothing throws across the ABI;
 *   - all matrices are row-major fp32 unless stated; "ld*" are row strides in
 *     ELEMENTS; float4 paths need pointers 16-byte aligned and K, ld* % 4 == 0;
 *   - no global mutable state: reentrant per stream.
 */
#ifndef LADCAST_HIP_H
#define LADCAST_HIP_H

#ifdef __cplusplus
extern "C" {
#endif

#define LDC_ABI_VERSION 5

#define LDC_OK 0
#define LDC_ERR_ARG (-1)       /* null pointer / non-positive size */
#define LDC_ERR_ALIGN (-2)     /* pointer or stride breaks the 16-byte rule */
#define LDC_ERR_UNSUPPORTED (-3)

enum ldc_act { LDC_ACT_NONE = 0, LDC_ACT_SILU = 1, LDC_ACT_GELU_TANH = 2, LDC_ACT_RELU = 3 };
/* `act_in` of ldc_linear_small / _grouped / _mod only: x holds ONE timestep per row (x_rows floats, any alignment) and the input
 * row is its 256-wide sinusoidal embedding [cos(t f_k) | sin(t f_k)], f_k = exp(-ln(1e4) k / 128) (K must be 256): diffusers
 * Timesteps(256, flip_sin_to_cos=True, downscale_freq_shift=0) fused into the TimestepEmbedding's first Linear
 * (models/LaDCast_3D_model.py:362-364,673); same values as ldc_timestep_embedding. */
#define LDC_ACT_IN_TIMESTEP_SINCOS 16

int ldc_abi_version(void);
/* name of the code-object architecture the library was built for ("gfx950") */
const char* ldc_build_arch(void);

/* ---------------------------------------------------------------------------
 * Dense contraction  C[b] = epilogue(A[b] . W^T)        (fp32 MFMA, exact fp32)
 *   A[b]: M x K (lda), W: N x K (ldw, shared by all batches), C[b]: M x N (ldc)
 *   v = acc + bias[n]; v = act(v); v *= gate[b*gate_bs + n]; v += R[b][m*ldr + n]
 *   (bias / gate / R may be NULL).  R may alias C.
 * Replaces nn.Linear + activation + gated residual on the token streams:
 *   models/LaDCast_3D_model.py:92-94,175-177,214,219 (q/k/v, added q/k/v, to_out,
 *   to_add_out), :271-276,503-512,558-563 (FeedForward + gate), :422-424,442,
 *   460-462 (proj_mlp / proj_out of the single block), :1045 (proj_out),
 *   models/embeddings.py:52-58 (k=1 Conv3d patch embed), and the NHWC 1x1 convs /
 *   Linear layers of models/DCAE.py:129-131,142-144,286,296.
 * ------------------------------------------------------------------------- */
typedef struct ldc_gemm_desc {
  int M, N, K, batch;
  int lda, ldw, ldc, ldr;
  long long a_bs, c_bs, r_bs; /* batch strides (elements) */
  int gate_bs;                /* batch stride of gate (elements) */
  int act;                    /* enum ldc_act */
  int flags;                  /* LDC_GEMM_* bits below; 0 = plain fp32 A and C */
  int reserved;               /* 0 */
} ldc_gemm_desc;
/* Split-bf16 activation format (only ldc_gemm_grouped_bf16x3 takes these; every other entry rejects them):
 * columns 8c..8c+7 of a row occupy the SAME 32 bytes as 8 floats would, holding [hi x8 | lo x8] bf16
 * (hi = bf16(x), lo = bf16(x - hi)), so every pointer / stride / column offset that is a multiple of 8
 * elements addresses the same data in both formats.
 *   LDC_GEMM_A_SPLIT  A is in that format (made by a producer kernel that split it once) instead of fp32:
 *                     the GEMM then skips its own split of every A fragment; results are bit-identical.
 *   LDC_GEMM_C_SPLIT  C is written in that format (after bias / activation / gate / residual). */
#define LDC_GEMM_A_SPLIT 1
#define LDC_GEMM_C_SPLIT 2
/*   LDC_GEMM_BF16_1TERM  single-term bf16 contraction bf16(A).bf16(W) (fp32 accumulate): the "bf16" mixed-precision mode
 *                     (BASELINE configs[4] "fp16/bf16 mixed"; what torch.autocast(bfloat16) does to an nn.Linear's
 *                     operands, the reference's fp32 islands - models/LaDCast_3D_model.py:953, models/DCAE.py:162,180 -
 *                     never reach a GEMM here).  In this mode the operands are PLAIN bf16 ROWS (LDC_FMT_BF16): a row of
 *                     K values occupies the first 2 K bytes of the 4 K bytes its fp32 row would (same pointers, same
 *                     strides, half the bytes moved); LDC_GEMM_A_SPLIT (required) then means "A is in that format" and
 *                     LDC_GEMM_C_SPLIT "write C in that format"; W comes from ldc_pack_weight_bf16 ([N][K] bf16).
 *                     K % 64 == 0; all problems of one call must agree.  Measured 3.2e-3 rel-L2 per 375M forward instead of 6e-6
 *                     (stated tolerance 7e-3 = measured x 2; the table of all stated tolerances is ladcast_amd/precision.py). */
#define LDC_GEMM_BF16_1TERM 4
/*   LDC_GEMM_F32_REGSTAGE  (ldc_gemm_grouped, exact-fp32 problems only) keep the launch on the register-staged stream-K kernel
 *                     (v_mfma_f32_32x32x2_f32) even where the LDS-DMA ring kernel would serve it (K % 32 == 0, contiguous weights,
 *                     16-byte rows): the second exact-fp32 implementation as a caller's choice - cross-checks, and shapes a caller
 *                     knows to be launch-bound.  Same results to fp32 rounding (another summation order). */
#define LDC_GEMM_F32_REGSTAGE 8
/* activation formats of the producers' `out_split` / `x_fmt` arguments: fp32, split-bf16 groups (LDC_GEMM_A_SPLIT), plain bf16 rows */
#define LDC_FMT_F32 0
#define LDC_FMT_SPLIT 1
#define LDC_FMT_BF16 2
int ldc_sizeof_gemm_desc(void);
int ldc_gemm_bias_act(const float* A, const float* W, const float* bias, const float* gate,
                      const float* R, float* C, const ldc_gemm_desc* d, void* stream);

/* Same contraction for up to LDC_GEMM_MAX_PROBLEMS independent problems in ONE persistent launch
 * with stream-K scheduling (work = (tile, 32-deep k-step) units cut into equal contiguous ranges);
 * tiles whose K range was split are summed INSIDE the launch by the piece that arrives last, in
 * workgroup order (bitwise reproducible; no second launch since ABI 2).  Problems with K % 32 == 0,
 * ldw == K, lda % 4 == 0 and 16-byte aligned A / W run on the LDS-DMA ring kernel (fp32 operand rows,
 * v_mfma_f32_16x16x4_f32, one workgroup per CU); the others - same results up to the summation
 * order - on the register-staged kernel (2 workgroups per CU).  Exact fp32 products either way.  Built for the
 * small grids of the AR transformer (e.g. the pred- and cond-stream projections of a dual block,
 * models/LaDCast_3D_model.py:92-94,175-177,558-563).  `workspace` is caller-owned device scratch of
 * at least ldc_gemm_grouped_workspace_bytes() bytes (16-byte aligned), initialised ONCE with
 * ldc_gemm_grouped_workspace_init (zeroes the tile-arrival counters in its first MiB; every call
 * leaves them zero) and then reused by the calls of ONE stream.  C of one problem must not overlap
 * A/R of another problem of the same call. */
#define LDC_GEMM_MAX_PROBLEMS 4
typedef struct ldc_gemm_problem {
  const float* A;
  const float* W;
  const float* bias;
  const float* gate;
  const float* R;
  float* C;
  ldc_gemm_desc d;
} ldc_gemm_problem;
int ldc_sizeof_gemm_problem(void);
long long ldc_gemm_grouped_workspace_bytes(void);
int ldc_gemm_grouped_workspace_init(void* workspace, long long workspace_bytes, void* stream);
int ldc_gemm_grouped(const ldc_gemm_problem* problems, int n, void* workspace, long long workspace_bytes,
                     void* stream);

/* Split-bf16 ("bf16x3") form of ldc_gemm_grouped: same problems / epilogue / scheduling, but every
 * problem's W points to weights pre-split by ldc_pack_weight_bf16x2 ([N][K/8][hi x8 | lo x8] bf16,
 * N*K*4 bytes; d.ldw is ignored, K % 8 == 0) and the contraction is Ah.Wh + Ah.Wl + Al.Wh on the bf16
 * matrix cores with fp32 accumulation (hi = bf16(x), lo = bf16(x - hi); activations are split on
 * load).  Error vs exact fp32: ~4e-6 rel-L2 per model forward. */
int ldc_gemm_grouped_bf16x3(const ldc_gemm_problem* problems, int n, void* workspace, long long workspace_bytes,
                            void* stream);
int ldc_pack_weight_bf16x2(const float* W, void* out, int N, int K, int ldw, void* stream);
/* fp32 [N][K] (row stride ldw) -> plain bf16 [N][K] (2 N K bytes), the W operand of the LDC_GEMM_BF16_1TERM mode */
int ldc_pack_weight_bf16(const float* W, void* out, int N, int K, int ldw, void* stream);

/* Small-M linear (M = rows <= 64): y[r] = act_out(W . act_in(x[r % x_rows]) + bias)
 *                                           + add[r % add_rows]
 * HBM-bound weight streaming; replaces the timestep / text / AdaLN projection
 * Linears on (B, D) vectors: diffusers TimestepEmbedding, PixArtAlphaTextProjection,
 * AdaLayerNormZero/-Single/-Continuous .linear and HunyuanVideoAdaNorm.linear
 * (models/LaDCast_3D_model.py:224-238,362-364,441,524-529,673-678,1044).
 * Two kernels, chosen from (rows, N, K) only: up to 8 rows, or N < 4096, or K % 64 != 0 -> the VALU kernel (W streamed once per 8 rows);
 * more rows on a wide output (the AdaLN modulation of a sampler chunk's conditioning batch: 20 rows per member x 38 D) -> exact-fp32
 * products on v_mfma_f32_16x16x4_f32 (W streamed once per 32 rows).  Same formula, different summation order (fp32 rounding); inside either
 * kernel a row's result does not depend on the other rows of the launch. */
int ldc_linear_small(const float* x, int x_rows, const float* W, const float* bias,
                     const float* add, int add_rows, float* y, int rows, int N, int K,
                     int act_in, int act_out, void* stream);

/* ldc_linear_small followed by y = y * (1 + mod[r % mod_rows][n]) + mod[r % mod_rows][N + n] (mod: [mod_rows][2 N]): the
 * time-elapsed modulation of the conditioning embedding, temb * (1 + scale) + shift (models/LaDCast_3D_model.py:958-969), as the
 * epilogue of the text embedder's second Linear; always the VALU kernel: bit-identical to ldc_linear_small + ldc_temb_modulate where that
 * takes the VALU kernel too (see above). */
int ldc_linear_small_mod(const float* x, int x_rows, const float* W, const float* bias, const float* add, int add_rows,
                         const float* mod, int mod_rows, float* y, int rows, int N, int K, int act_in, int act_out,
                         void* stream);

/* Up to LDC_LINEAR_SMALL_MAX_GROUPED independent small linears (same formula, the per-output arithmetic of
 * ldc_linear_small's VALU kernel: results are bit-identical to single launches that take that kernel) in ONE launch: the two MLPs of
 * CombinedTimestepTextProjEmbeddings (timestep_embedder / text_embedder, used twice per forward:
 * models/LaDCast_3D_model.py:362-364,953-969) have independent first and second layers.  No problem's y may be
 * another problem's x / add / y (LDC_ERR_ARG). */
#define LDC_LINEAR_SMALL_MAX_GROUPED 4
typedef struct ldc_linear_small_problem {
  const float* x;    /* [x_rows][K] */
  const float* W;    /* [N][K] */
  const float* bias; /* [N] or NULL */
  const float* add;  /* [add_rows][N] or NULL */
  float* y;          /* [rows][N] */
  int x_rows, add_rows, rows, N, K, act_in, act_out, reserved;
} ldc_linear_small_problem;
int ldc_linear_small_grouped(const ldc_linear_small_problem* problems, int n, void* stream);

/* ---------------------------------------------------------------------------
 * Attention   O = softmax(Q K^T / sqrt(128) + key_bias) V   per (batch, head)
 *   Q,K,V: token-major [B][S][H][128] views with row stride ld_qkv and batch stride
 *   qkv_bs (so they can be column slices of one fused QKV buffer);
 *   O: [B][S][H*128] with row stride ldo, batch stride o_bs;
 *   key_bias: NULL, or [S] floats added to every query's score of that key - the float
 *   attention mask of `scale_attn_by_lat` (models/LaDCast_3D_model.py:683-693,873-882:
 *   a (1, 1, 1, keys) tensor, i.e. a function of the key alone).
 * Replaces F.scaled_dot_product_attention at models/LaDCast_3D_model.py:199-203
 * (incl. the transpose/flatten back to [B, N, C]).  head_dim must be 128.
 * ------------------------------------------------------------------------- */
int ldc_attn_fwd(const float* Q, const float* K, const float* V, float* O, int B, int S, int H,
                 int ld_qkv, long long qkv_bs, int ldo, long long o_bs, const float* key_bias, void* stream);
/* (ABI 4) the same with a workspace of ldc_attn_fwd_workspace_bytes() bytes (16-byte aligned, ZERO-FILLED ONCE by the caller, one per
 * stream: the launch leaves its counters zero).  With it, a launch whose query blocks x heads x batch do not fill whole rounds of the 256
 * CUs is cut into one contiguous range of (unit, key tile) items per CU - 216 units (one member of the 375M model) take 0.84 of a round,
 * 288 / 432 units 1.13 / 1.69 rounds instead of two; pieces of a unit meet through write-through slabs and are combined by the last
 * arriver in range order (bitwise reproducible).  workspace == NULL (or too small): the one-unit-per-workgroup grids of ldc_attn_fwd. */
long long ldc_attn_fwd_workspace_bytes(void);
int ldc_attn_fwd_ws(const float* Q, const float* K, const float* V, float* O, int B, int S, int H, int ld_qkv, long long qkv_bs,
                    int ldo, long long o_bs, const float* key_bias, void* workspace, long long workspace_bytes, void* stream);
/* Fewer queries than keys: the queries are the first Sq of the S token rows (1 <= Sq <= S), keys and values are all S rows.  Rows
 * [0, Sq) of O are written, rows >= Sq of O are not touched.  For a caller whose last Sq.. rows are only needed as keys / values - the
 * last single-stream block of the model, whose conditioning rows no later layer reads.  Work units are query blocks of Sq x heads x
 * batch, and every choice made from the unit count (balanced cut, wave groups) is made from that number, so the results of rows [0, Sq)
 * agree with the full call's to fp32 rounding, not bit for bit.  Sq == S is exactly ldc_attn_fwd / ldc_attn_fwd_ws (same bits); the
 * workspace is the same one. */
int ldc_attn_fwd_qrows(const float* Q, const float* K, const float* V, float* O, int B, int S, int Sq, int H, int ld_qkv,
                       long long qkv_bs, int ldo, long long o_bs, const float* key_bias, void* stream);
int ldc_attn_fwd_ws_qrows(const float* Q, const float* K, const float* V, float* O, int B, int S, int Sq, int H, int ld_qkv,
                          long long qkv_bs, int ldo, long long o_bs, const float* key_bias, void* workspace, long long workspace_bytes,
                          void* stream);
/* The same with the deferred-rescale threshold given by the caller (tests, measurements).  The kernel keeps, per query, the maximum that
 * was applied to its O and l accumulators, and rescales them only when a key tile's maximum exceeds it by more than rescale_thr (log2
 * units, 0 .. 64; probabilities are then at most 2^rescale_thr).  ldc_attn_fwd_ws_qrows is this call with the library's threshold (8);
 * 0 makes the accumulators follow every new maximum.  Results agree to fp32 rounding whatever the threshold. */
int ldc_attn_fwd_ws_qrows_thr(const float* Q, const float* K, const float* V, float* O, int B, int S, int Sq, int H, int ld_qkv,
                              long long qkv_bs, int ldo, long long o_bs, const float* key_bias, void* workspace,
                              long long workspace_bytes, float rescale_thr, void* stream);

/* (ABI 2: the second-generation split attention - ldc_attn_pack_bf16x3 / ldc_attn_fwd_packed_bf16x3 / ldc_attn_packed_bytes, a
 * pack pass writing LDS tile images + the attention on them - was removed; ldc_attn_qkv_prepare_split / the fused QKV epilogue +
 * ldc_attn_fwd_split below serve every caller it had.)
 *
 * `flags` of ldc_attn_fwd_split is a bit set: LDC_ATTN_OUT_SPLIT = O is written in the split activation format of LDC_GEMM_A_SPLIT (ldo, o_bs
 * multiples of 8); LDC_ATTN_BF16_1TERM = single-term bf16 products (Qh.Kh, Ph.Vh; fp32 scores, softmax and accumulation):
 * the attention of the "bf16" mixed-precision mode (see LDC_GEMM_BF16_1TERM). */
#define LDC_ATTN_OUT_SPLIT 1
#define LDC_ATTN_BF16_1TERM 2
#define LDC_ATTN_OUT_BF16 4 /* ldc_attn_fwd_split only: O as plain bf16 rows (LDC_FMT_BF16) */

/* Split-bf16 attention on ROW-MAJOR operand rows (third generation; no packed copy of the operands):
 *   Q, K, V are views into a fused [B][S][3][H][128]-float buffer (row stride ld_qkv, batch stride qkv_bs, in floats) whose
 *   512 bytes per (token, head) hold, instead of 128 floats,
 *     q, k: 16 groups of 8 head-dim values, each [hi x8 | lo x8] bf16 (the LDC_GEMM_A_SPLIT format), with the per-head
 *           RMSNorm + rotary embedding already applied and q multiplied by log2(e) / sqrt(128);
 *     v   : [hi x128 | lo x128] bf16.
 *   Producers: the QKV projection itself (ldc_gemm_grouped_bf16x3_qkv below: GEMM epilogue) or, from an fp32 buffer in place,
 *   ldc_attn_qkv_prepare_split (token rows [0, split_row) use wq0 / wk0 / cos0 / sin0, rows [split_row, S) use wq1 / wk1 / cos1 / sin1 with table row = row - split_row; NULL weights = no norm, NULL tables = no RoPE).
 *   ldc_attn_fwd_split: O = softmax(q.k^T) v per (batch, head); `flags`: the bit set above.
 * Replaces attn.norm_q/norm_k/norm_added_q/norm_added_k + apply_rotary_emb + F.scaled_dot_product_attention,
 * models/LaDCast_3D_model.py:103-169,183-203. */
/* The QKV projection with those operand rows as its OUTPUT: ldc_gemm_grouped_bf16x3 (pre-split activations, K % 32 == 0) whose
 * epilogue, for every problem i with epi[i].heads > 0 (N = 3 * heads * 128, C = the fused buffer, no act / gate / residual), adds
 * the bias, applies RMSNorm(128, eps) * wq | wk and the rotary embedding (compact table, row = rope_row0 + m; NULL = none) to the q and k
 * heads, multiplies q by qscale (0 = log2(e) / sqrt(128)) and writes the split rows - to_q/to_k/to_v (+ add_*_proj), norm_q/k,
 * apply_rotary_emb of models/LaDCast_3D_model.py:92-169,175-190 in one launch.  Problems with heads == 0 get the ordinary epilogue.
 * LDC_ERR_UNSUPPORTED: shape not served by that kernel - run the plain GEMM, then ldc_attn_qkv_prepare_split. */
typedef struct ldc_qkv_epilogue {
  const float* wq;   /* [128] */
  const float* wk;   /* [128] */
  const float* rope; /* [rows][64][2] = (cos_i, sin_i) of rotary pair i: the compact form of the reference's [rows][128] cos / sin
                        tables, which hold every value twice (repeat_interleave(2)); NULL = no rotary embedding */
  const float* reserved; /* NULL */
  float eps, qscale;
  int heads, rope_row0;
} ldc_qkv_epilogue;
int ldc_sizeof_qkv_epilogue(void);
int ldc_gemm_grouped_bf16x3_qkv(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, void* workspace,
                                long long workspace_bytes, void* stream);
/* (ABI 4) exact-fp32 counterpart: the same grouped launch on fp32 operands (ldc_gemm_grouped's problems, flags 0) where problem i with
 * epi[i].heads > 0 is a QKV projection whose epilogue applies bias -> per-head RMSNorm * weight -> adjacent-pair rotary embedding to the q
 * and k heads (v: bias only) and writes PLAIN fp32 rows - what ldc_qk_rmsnorm_rope does in place afterwards, without its launches and its
 * round trip (pass qscale = 1: ldc_attn_fwd scales q itself).  LDC_ERR_UNSUPPORTED (K % 32 != 0, strided weights, rows not 16-byte
 * aligned): run ldc_gemm_grouped + ldc_qk_rmsnorm_rope. */
int ldc_gemm_grouped_qkv_f32(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epi, int n, void* workspace,
                             long long workspace_bytes, void* stream);
/* (added since ABI 5, version unchanged) What a grouped call would run, without running it: ldc_gemm_grouped_plan returns the status
 * ldc_gemm_grouped (split_bf16 = 0) | ldc_gemm_grouped_bf16x3 (1) would return for `problems` with a 16-byte aligned workspace of
 * `workspace_bytes` - with epilogues != NULL: ldc_gemm_grouped_qkv_f32 | ldc_gemm_grouped_bf16x3_qkv - and on LDC_OK fills `out`.  It
 * launches nothing and reads no data pointer: A / W / C / bias / ... are checked for NULL and alignment exactly as by the launch, so
 * any addresses with the caller's alignment plan like the caller's buffers.  The same host code plans the launches themselves.
 *   kernel    LDC_GEMM_KERNEL_RING: gemm_bf16x3_v3_kernel<tile_rows, terms, false> | LDC_GEMM_KERNEL_REGSTAGE: gemm_streamk_kernel
 *             (terms 0) / gemm_streamk_bf16x3_kernel (terms 3), 128-row tiles
 *   terms     0 exact fp32 | 1 single-term bf16 | 3 split bf16
 *   launches  1, or n: a split-mode group without a k-aligned cut runs its problems one by one (launch l = problem l)
 *   per launch l: tile_rows (128 | 256), workgroups, units (= (tile, k-step) pairs), tiles, and the cut: workgroup g runs units
 *             [g units_per_group + min(g, units_rem), ...) (the register-staged kernels cut at g units / workgroups instead)
 *   per problem p: its tile grid tile_rows_m x tile_cols_n (x batch), k_steps per tile, and super_row: the ring kernel walks the tiles in
 *             bands of that many row tiles (= tile_rows_m: one band) */
#define LDC_GEMM_KERNEL_RING 0
#define LDC_GEMM_KERNEL_REGSTAGE 1
typedef struct ldc_gemm_plan {
  int kernel, terms, launches, reserved;
  int tile_rows[LDC_GEMM_MAX_PROBLEMS], workgroups[LDC_GEMM_MAX_PROBLEMS];
  long long units[LDC_GEMM_MAX_PROBLEMS], tiles[LDC_GEMM_MAX_PROBLEMS];
  int units_per_group[LDC_GEMM_MAX_PROBLEMS], units_rem[LDC_GEMM_MAX_PROBLEMS];
  int tile_rows_m[LDC_GEMM_MAX_PROBLEMS], tile_cols_n[LDC_GEMM_MAX_PROBLEMS], k_steps[LDC_GEMM_MAX_PROBLEMS], super_row[LDC_GEMM_MAX_PROBLEMS];
} ldc_gemm_plan;
int ldc_sizeof_gemm_plan(void);
int ldc_gemm_grouped_plan(const ldc_gemm_problem* problems, const ldc_qkv_epilogue* epilogues, int n, int split_bf16,
                          long long workspace_bytes, ldc_gemm_plan* out);
int ldc_attn_qkv_prepare_split(float* Q, float* K, float* V, int B, int S, int H, int ld_qkv, long long qkv_bs, int split_row,
                               const float* wq0, const float* wk0, const float* cos0, const float* sin0, const float* wq1,
                               const float* wk1, const float* cos1, const float* sin1, float eps, void* stream);
/* workspace (ABI 3): bytes ldc_attn_fwd_split can use for this call shape (0: none needed).  When query blocks x heads x batch exceed the
 * 256 CUs by at most half a round (the 1.6B model: 16 heads x 18 query blocks of 128 = 288 units), the kernel runs one persistent
 * workgroup per CU - its whole units first, then ONE key slice of a left-over unit - and a second small launch merges the slices'
 * (O, m, l) in slice order (bitwise reproducible): 288 units take ~1.13 rounds instead of two uneven ones.  workspace == NULL (or too
 * small) is legal: the call then runs the plain one-unit-per-workgroup grids. */
long long ldc_attn_fwd_split_workspace_bytes(int B, int S, int H);
/* upper bound of the above over every call shape (17.8 MB): allocate this once per stream when launches are captured into hipGraphs -
 * a workspace that is replaced by a larger one later leaves the captured launches writing through a dangling pointer */
long long ldc_attn_fwd_split_workspace_max_bytes(void);
int ldc_attn_fwd_split(const float* Q, const float* K, const float* V, float* O, int B, int S, int H, int ld_qkv,
                       long long qkv_bs, int ldo, long long o_bs, const float* key_bias, int flags, void* workspace,
                       long long workspace_bytes, void* stream);
/* key_bias: as ldc_attn_fwd's, but 32 * ceil(S / 32) floats (16-byte aligned; entries past S are ignored). */
/* Fewer queries than keys, as ldc_attn_fwd_qrows: queries = token rows [0, Sq), keys / values = all S rows, rows >= Sq of O untouched (in
 * every output format).  The units - and with them the choice of the persistent form and the workspace it asks for - are query blocks of
 * Sq x heads x batch.  Sq == S is exactly ldc_attn_fwd_split / ldc_attn_fwd_split_workspace_bytes. */
long long ldc_attn_fwd_split_qrows_workspace_bytes(int B, int S, int Sq, int H);
int ldc_attn_fwd_split_qrows(const float* Q, const float* K, const float* V, float* O, int B, int S, int Sq, int H, int ld_qkv,
                             long long qkv_bs, int ldo, long long o_bs, const float* key_bias, int flags, void* workspace,
                             long long workspace_bytes, void* stream);

/* In-place per-head RMSNorm(128, eps, weight) on q and k followed by the
 * adjacent-pair rotary embedding (cos/sin tables [rows][128], NULL = no RoPE),
 * for token rows [row0, row0+rows) of every batch of a fused QKV buffer.
 * Replaces attn.norm_q/norm_k/norm_added_q/norm_added_k + apply_rotary_emb,
 * models/LaDCast_3D_model.py:103-169,183-186. */
int ldc_qk_rmsnorm_rope(float* q, float* k, int B, int row0, int rows, int H, int ld, long long bs,
                        const float* wq, const float* wk, float eps, const float* cos_tab,
                        const float* sin_tab, void* stream);

/* Row LayerNorm (no affine inside) followed by y = n * mul + add with
 *   mode 0: mul = 1 + scale[b][c], add = shift[b][c]   (AdaLN modulate)
 *   mode 1: mul = scale[c],        add = shift[c]      (plain affine LayerNorm)
 * x: [B][rows][D] (ldx, x_bs) -> y (ldy, y_bs); mod_bs = batch stride of scale/shift.
 * Replaces AdaLayerNormZero/-Single/-Continuous .norm + modulation, nn.LayerNorm,
 * models/LaDCast_3D_model.py:257,270,287,299,441,502,507,524-529,546-555,1044. */
int ldc_layernorm_mod(const float* x, float* y, int B, int rows, int D, int ldx, long long x_bs,
                      int ldy, long long y_bs, const float* scale, const float* shift, int mod_bs,
                      int mode, float eps, int out_split, void* stream);
/* out_split != 0: y is written in the split activation format of LDC_GEMM_A_SPLIT (the consumer GEMM then
 * does not split it again); D, ldy, y_bs multiples of 8. */
/* The same over two row segments in one launch: rows [0, split_row) use scale / shift, rows [split_row, rows)
 * use scale2 / shift2 (same mode, eps and mod_bs).  One call per dual block norm instead of one per stream:
 * norm1 + norm1_context (models/LaDCast_3D_model.py:524-529) and norm2 + norm2_context (:546-555) when the
 * two token streams are adjacent rows of one buffer.  Row results are those of ldc_layernorm_mod, bit for bit. */
int ldc_layernorm_mod2(const float* x, float* y, int B, int rows, int D, int ldx, long long x_bs,
                       int ldy, long long y_bs, const float* scale, const float* shift, int split_row,
                       const float* scale2, const float* shift2, int mod_bs, int mode, float eps,
                       int out_split, void* stream);

/* y[b][c] = mean over rows of x[b][r][c]   (hidden_states.mean(dim=1),
 * models/LaDCast_3D_model.py:382,955) */
int ldc_mean_rows(const float* x, float* y, int B, int rows, int D, int ldx, long long x_bs, void* stream);
/* The same mean (bit-identical y) that also writes x in the split activation format of LDC_GEMM_A_SPLIT to
 * x_split (row stride lds, batch stride s_bs, in floats; D % 8 == 0), so that the Linear consuming x
 * (context_refiner.proj_in, models/LaDCast_3D_model.py:362-380) takes the pre-split GEMM kernel. */
int ldc_mean_rows_split(const float* x, float* y, float* x_split, int B, int rows, int D, int ldx,
                        long long x_bs, int lds, long long s_bs, int fmt /* LDC_FMT_SPLIT | LDC_FMT_BF16 */, void* stream);

/* out[b][r][c] = resid[b][r][c] + gate[b][c] * y[b][r][c]  (refiner gated residual on the
 * projection-less attention output, models/LaDCast_3D_model.py:296-297) */
int ldc_gate_residual(const float* resid, const float* y, const float* gate, float* out, int B,
                      int rows, int D, int ld_res, long long res_bs, int ld_y, long long y_bs,
                      int gate_bs, void* stream);
/* ldc_gate_residual in place (resid += gate * y) followed by out = LayerNorm(resid; eps) * weight + bias (out_split: written in
 * the LDC_GEMM_A_SPLIT format) in ONE launch: the refiner block's gated attention residual + norm2
 * (models/LaDCast_3D_model.py:296-300); bit-identical to ldc_gate_residual + ldc_layernorm_mod(mode 1). */
int ldc_gate_residual_layernorm(float* resid, const float* y, const float* gate, float* out, int B, int rows, int D, int ld_res,
                                long long res_bs, int ld_y, long long y_bs, int gate_bs, int ld_out, long long out_bs,
                                const float* weight, const float* bias, float eps, int out_split, void* stream);

/* Layout changes between the reference's channel-major latents (B, C, T*H*W) and
 * token-major (B, T*H*W, ld) (models/embeddings.py:56-59 flatten/transpose and
 * models/LaDCast_3D_model.py:1047-1062 un-patchify; also NCHW <-> NHWC for the DCAE).
 * Columns [C, fill_cols) of the token-major output are zero-filled (fill_cols <= ldo; lets two
 * calls concatenate channels into one padded row). */
int ldc_chan_to_token(const float* in, float* out, int B, int C, int N, int ldo, int fill_cols, void* stream);
/* out_split != 0: the token rows are written in the split activation format of LDC_GEMM_A_SPLIT
 * (fill_cols, ldo multiples of 8; out 32-byte aligned). */
int ldc_chan_to_token_split(const float* in, float* out, int B, int C, int N, int ldo, int fill_cols,
                            int out_split, void* stream);
int ldc_token_to_chan(const float* in, float* out, int B, int C, int N, int ldi, void* stream);

/* Sinusoidal timestep embedding [cos | sin], 256 wide (diffusers Timesteps(256,
 * flip_sin_to_cos=True, shift=0); models/LaDCast_3D_model.py:362-364,673). */
int ldc_timestep_embedding(const float* t, float* out, int n, void* stream);

/* temb[b][c] = temb[b][c] * (1 + te[b % te_rows][c]) + te[b % te_rows][D + c]
 * (time-elapsed scale/shift, models/LaDCast_3D_model.py:966-969) */
int ldc_temb_modulate(float* temb, const float* te, int B, int D, int te_rows, void* stream);

/* Per-channel affine on (outer, C, inner): forward (x-mean[c])/std[c]*t, inverse
 * x/t*std[c]+mean[c]  (dataloader/utils.py:223-240). */
int ldc_chan_affine(const float* x, float* y, const float* mean, const float* std_, float target_std,
                    long long outer, int C, long long inner, int inverse, void* stream);

/* ---------------------------------------------------------------------------
 * Sampler state updates (pipelines/edm_sampler.py:60-113; fp64 state, fp32 model I/O)
 * and the DPM-Solver++(2M) step of diffusers.EDMDPMSolverMultistepScheduler.step
 * (used by pipelines/pipeline_AR.py:100-102).  Scalars are computed on the host
 * in fp32 exactly as the scheduler does and passed here widened to double.
 * ------------------------------------------------------------------------- */
int ldc_edm_scale_f64_to_f32(const double* x, double c_in, float* out, long long n, void* stream);
int ldc_edm_init_state(const float* noise, double sigma0, double* x, long long n, void* stream);
/* stochastic churn of the non-deterministic sampler (pipelines/edm_sampler.py:67-76): x_hat = x_cur + coef * noise (fp64),
 * coef = sqrt(t_hat^2 - t_cur^2) * S_noise computed in fp32 on the host as the reference does */
int ldc_edm_churn(const double* x_cur, const double* noise, double coef, double* x_hat, long long n, void* stream);
/* den = c_skip*x + c_out*F; d = (x-den)/t_hat; x_next = x + dt*d */
int ldc_edm_euler(const double* x_hat, const float* F, double c_skip, double c_out, double t_hat,
                  double dt, double* x_next, double* d_cur, long long n, void* stream);
/* den = c_skip*x_next + c_out*F; d' = (x_next-den)/t_next; x_next = x_hat + dt*(0.5 d_cur + 0.5 d') */
int ldc_edm_heun(const double* x_hat, double* x_next, const float* F, const double* d_cur,
                 double c_skip, double c_out, double t_next, double dt, long long n, void* stream);
int ldc_f64_to_f32(const double* x, float* y, long long n, void* stream);
/* x0 = c_skip*sample + c_out*F; order 1: prev = a*sample - b*x0;
 * order 2: prev = a*sample - b*x0 - (0.5*b) * (inv_r0 * (x0 - m1))   (all fp32) */
int ldc_dpm_step(const float* sample, const float* F, const float* m1, float* x0, float* prev,
                 float c_skip, float c_out, float a, float b, float inv_r0, int order, long long n,
                 void* stream);
/* One solver step of the scheduler classes the reference's pipeline loop names (pipelines/pipeline_AR.py:19-21,100-102:
 * diffusers DDIMScheduler.step / DDPMScheduler.step, v0.32.1) as one fused fp32 kernel; coefficients are the host's fp32 0-dim
 * tensor arithmetic, widened nowhere.  prediction_type: 0 epsilon, 1 sample, 2 v_prediction; clip_range <= 0: no clamp of x0;
 * noise == NULL: no noise term (DDIM eta = 0; DDPM at t = 0).
 *   x0 = (s - sqrt_beta_t F) / sqrt_alpha_t | F | sqrt_alpha_t s - sqrt_beta_t F   (clamped)
 *   ldc_ddim_step: prev = sqrt_alpha_prev x0 + dir_coef eps [+ std_dev noise], eps = F | (s - sqrt_alpha_t x0)/sqrt_beta_t |
 *                  sqrt_alpha_t F + sqrt_beta_t s  (use_clipped_model_output: eps re-derived from the clamped x0)
 *   ldc_ddpm_step: prev = x0_coef x0 + sample_coef s [+ std_dev noise] */
int ldc_ddim_step(const float* sample, const float* F, const float* noise, float* x0, float* prev, float sqrt_alpha_t,
                  float sqrt_beta_t, float sqrt_alpha_prev, float dir_coef, float std_dev, float clip_range,
                  int prediction_type, int use_clipped_model_output, long long n, void* stream);
int ldc_ddpm_step(const float* sample, const float* F, const float* noise, float* x0, float* prev, float sqrt_alpha_t,
                  float sqrt_beta_t, float x0_coef, float sample_coef, float std_dev, float clip_range, int prediction_type,
                  long long n, void* stream);
int ldc_scale_f32(const float* x, float s, float* y, long long n, void* stream);
/* out = a*x + b*y (fp32): scheduler.precondition_outputs (c_skip*sample + c_out*F) and
 * add_noise (x0 + sigma*noise) on whole tensors */
int ldc_axpby_f32(const float* x, float a, const float* y, float b, float* out, long long n, void* stream);

/* ---------------------------------------------------------------------------
 * The EDM denoising objective around the forward, one noise level PER SAMPLE (train_AR.py:873-1032 without the backward
 * pass).  Tensors: contiguous fp32 (B, C, T, H, W); sample of element i: i / n_per_sample; latitude row: (i / W) % H.
 * sigma / c_in / c_skip / c_out / weight: fp32 device vectors [B] the host computed with the reference's fp32 tensor
 * expressions.  No product-sum is contracted: noisy, x_in and denoised are bit-identical to torch's elementwise results.
 * LDC_ERR_ARG: a null pointer or a non-positive size; LDC_ERR_UNSUPPORTED: more blocks than a grid holds.
 * ------------------------------------------------------------------------- */
/* noisy = clean + noise * sigma_b (a product, then a sum); x_in = noisy * c_in_b.  One launch for the batch.
 * noise == NULL: noisy = clean (precondition_inputs of an already noised tensor; sigma unused).  noisy or x_in may be NULL
 * (not both): that output is not written (c_in unused without x_in). */
int ldc_edm_noise_inputs(const float* clean, const float* noise, const float* sigma, const float* c_in, float* noisy,
                         float* x_in, int B, long long n_per_sample, void* stream);
/* denoised = c_skip_b * noisy + c_out_b * F (three roundings: scheduler.precondition_outputs) on (B, C, T, plane) views that
 * may be T-slices of larger tensors: `*_frames` = frames of the tensor the view was sliced from (>= T), i.e. its channel
 * stride is frames * plane and its batch stride C * frames * plane; the pointer is the view's first element. */
int ldc_edm_denoise(const float* noisy, const float* F, const float* c_skip, const float* c_out, float* denoised, int B,
                    int C, int T, int plane, int noisy_frames, int f_frames, int denoised_frames, void* stream);
/* table[b][c][t] = mean over the (H, W) plane of  w * ((c_skip_b * noisy + c_out_b * F) - target)^2,  w = weight_b, or
 * (lat_weight[h] * weight_b) with lat_weight [H] (NULL: none): every term in fp32 in that order, summed in fp64 in a fixed
 * order (one wave per plane, fixed lane assignment, butterfly; no atomics - two launches give the same bits), divided and
 * rounded once to fp32.  denoised (NULL: not written): the preconditioned output, as ldc_edm_denoise. */
int ldc_edm_denoise_loss(const float* noisy, const float* F, const float* target, const float* c_skip, const float* c_out,
                         const float* weight, const float* lat_weight, float* table, float* denoised, int B, int C, int T,
                         int H, int W, void* stream);

/* ---------------------------------------------------------------------------
 * DCAE encoder / decoder (models/DCAE.py, models/sphere_conv.py) in NHWC layout
 * ([B][H][W][C], channel stride 1, pixel stride ld*).
 * ------------------------------------------------------------------------- */
/* Dense SphereConv2d (stride 1, ksize 3 or 5, even W) as an implicit GEMM on the fp32 MFMA:
 *   Y[pix][co] = act(bias[co] + sum_{ky,kx,ci} Wt[co][(ky*ks+kx)*cin + ci] * X[src(pix,ky,kx)][ci]) (+ R[pix][co])
 * with the reference's pole padding / kernel-row flip (models/sphere_conv.py:62-129,174-192).
 * Wt is the conv weight repacked [cout][ks*ks][cin] (cin % 4 == 0, zero-padded if needed). */
int ldc_sphere_conv_nhwc(const float* X, const float* Wt, const float* bias, const float* R, float* Y, int B,
                         int H, int W, int cin, int ldx, int cout, int ldy, int ldr, int ksize, int act,
                         void* stream);
/* Depthwise SphereConv2d, weights [ks*ks][C]; glu != 0: y[c] = d[c] * silu(d[c + C/2]) for c < C/2
 * (GLUMBConv conv_depth + gate, models/DCAE.py:287-295,311-313; multiscale proj_in, :77-85). */
int ldc_sphere_dwconv_nhwc(const float* x, const float* wt, const float* bias, float* y, int B, int H, int W,
                           int C, int ldx, int ldy, int ksize, int glu, void* stream);
/* Grouped 1x1 conv with 32 channels per group, weights [groups*32][32] (models/DCAE.py:86-88). */
int ldc_grouped_conv1x1_nhwc(const float* x, const float* wt, float* y, long long M, int groups, int ldx, int ldy,
                             void* stream);
/* ReLU linear attention over consecutive 96-channel groups (q|k|v = 32|32|32) of qkv[B][P][ldq];
 * y[B][P][groups*32] (models/DCAE.py:158-175,239-253; fp32, eps 1e-15). */
int ldc_relu_linear_attn_nhwc(const float* qkv, float* y, int B, int P, int groups, int ldq, int ldy, float eps,
                              void* workspace, long long workspace_bytes, void* stream);
/* Both contractions on the fp32 matrix core (exact fp32 products).  P >= 1024 and `workspace` >= ldc_relu_linear_attn_workspace_bytes(B, P,
 * groups) bytes (16-byte aligned; 0 bytes for P < 1024): two launches over 128-pixel slices - partial KV matrices (33 x 32 per slice) to the workspace,
 * then KV = the partials added in slice order and the output of the same pixels; the order only depends on P, so a frame's result
 * does not depend on the batch it is in (bitwise reproducible).  With a NULL / smaller workspace: one launch, a 16-wave workgroup
 * per (batch, group), partials added in wave order - the same result up to fp32 rounding. */
long long ldc_relu_linear_attn_workspace_bytes(int B, int P, int groups);
/* y = act(RMSNorm_C(x) * w + b (+ resid)) per pixel row (models/DCAE.py:259-260,317-322,371-377,729-730). */
int ldc_rmsnorm_rows(const float* x, const float* w, const float* b, const float* resid, float* y, long long rows,
                     int C, int ldx, int ldr, int ldy, float eps, int act, void* stream);
/* DCDownBlock2d tail: pixel_unshuffle(cv) + channel-group-mean(pixel_unshuffle(x)) (models/DCAE.py:477-490).
 * cv: [B][2*H2][2*W2][cout/4], x: [B][2*H2][2*W2][cin], y: [B][H2][W2][cout]. */
int ldc_pixel_unshuffle_shortcut(const float* cv, const float* x, float* y, int B, int H2, int W2, int cout, int cin,
                                 void* stream);
/* DCUpBlock2d tail: pixel_shuffle(cv) + pixel_shuffle(repeat_interleave(x)) (models/DCAE.py:526-532).
 * cv: [B][H][W][4*cout], x: [B][H][W][cin], y: [B][2H][2W][cout]. */
int ldc_pixel_shuffle_shortcut(const float* cv, const float* x, float* y, int B, int H, int W, int cout, int cin,
                               void* stream);
/* Channel regroup of [M][cin] -> [M][cout]: group mean (cin > cout; encoder out shortcut, models/DCAE.py:624-627)
 * or repeat_interleave (cin < cout; decoder in shortcut, :720-722). */
int ldc_chan_regroup(const float* x, float* y, long long M, int cin, int cout, void* stream);

/* ldc_sphere_conv_nhwc (dense SphereConv2d, same contract) on PRE-SPLIT activations (the DCAE's `bf16x3` path since round 2; round 1's
 * fp32-rows-in entry point ldc_sphere_conv_nhwc_bf16x3 left the ABI in version 3 - it left the tree with round 1's kernel in round 6): X holds NHWC rows in the split format
 * (in_fmt = LDC_FMT_SPLIT: columns 8g..8g+7 in 32 bytes [hi x8 | lo x8]; ldx % 8 == 0, ldx >= cin rounded up to 8, pad columns
 * zero), written by the producers below, so the conv's main loop is the pre-split GEMM kernel (gemm_bf16x3_v3.hip: 16x16x32 MFMA, no
 * VALU in the loop) with the sphere gather as per-lane LDS-DMA source addresses.  Wp: ldc_pack_weight_bf16x2 of the tap-major weight
 * [cout][k*k][cin_p], cin_p = 32 * 2^j >= cin with zeros behind cin.  out_fmt: LDC_FMT_F32 (Y fp32 rows) or LDC_FMT_SPLIT (Y split rows for the next conv, ldy % 8 == 0,
 * ldy >= cout rounded up to 8; cout % 4 == 0, the pad half of a last half-filled group is written as zeros).  cin % 8 need not
 * hold (252: the last group's pad columns are zero in X and in Wp).  ksize 1 / 3 / 5.
 * in_fmt = LDC_FMT_BF16 is the single-term `bf16` mode of the same conv (see LDC_GEMM_BF16_1TERM): X plain bf16 rows (same ldx, in
 * floats), Wp = ldc_pack_weight_bf16 of the [cout][k*k][cin rounded up to 64 * 2^j] tap-major weight, out_fmt LDC_FMT_F32 | LDC_FMT_BF16.
 * in_fmt = LDC_FMT_F32 (ABI 3) is the EXACT-fp32 conv on the same kernel (v_mfma_f32_16x16x4_f32 on plain fp32 operand rows, the conv
 * gather unchanged): X plain fp32 rows (ldx % 4 == 0, cin % 4 == 0), Wp the plain fp32 [cout][k*k][cin rounded up to 32 * 2^j]
 * tap-major weight with zeros behind cin, out_fmt LDC_FMT_F32 - what AutoencoderDC runs in its fp32 mode (ldc_sphere_conv_nhwc, the
 * tile-per-workgroup kernel, stays for channel counts that are no multiple of 4 and as the second implementation in the tests).
 * Replaces models/sphere_conv.py:62-192 + the nn.Conv2d / nn.Linear 1x1 layers of models/DCAE.py:96-324. */
int ldc_sphere_conv_nhwc_split(const float* X, const void* Wp, const float* bias, const float* R, float* Y, int B, int H, int W,
                               int cin, int ldx, int cout, int ldy, int ldr, int ksize, int act, int in_fmt, int out_fmt,
                               void* workspace, long long workspace_bytes, void* stream);
/* ABI 4: 3 x 3 convs in the split-bf16 / bf16 formats run a second kernel where the shape fills its tiles (conv_halo.hip): a workgroup
 * owns a TH x TW pixel tile and DMAs the tile's (TH + 2) x (TW + 2) halo image into LDS once per channel chunk - sphere padding folded
 * into the source addresses - instead of once per (tap, chunk); same arguments, same arithmetic per output element (k order: chunk-major
 * instead of tap-major, so results differ from the gathered kernel in the last bits of the fp32 accumulation only).
 * ldc_sphere_conv_plan tells which kernel a call shape gets: returns 1 and the tile (rows = TH x TW: 128 | 256; width TW) for the
 * halo-staged kernel, 0 for the gathered one (ksize != 3, fp32 rows, images that would leave most of the tiles' rows empty).  The plan
 * assumes the caller passes the full grouped-GEMM workspace (ldc_gemm_grouped_workspace_bytes): shapes that put two workgroups on a
 * tile need LDC_GEMM_COUNTER_BYTES + 2 * tiles * 128 KiB of it, and a call with less runs the gathered kernel whatever the plan says.
 * Both kernels validate alike: X 32-byte / Wp and workspace 16-byte aligned, ldx % 8 == 0 (LDC_ERR_ALIGN), act in range
 * (LDC_ERR_UNSUPPORTED), ldr >= cout when R is given (LDC_ERR_ARG). */
int ldc_sphere_conv_plan(int B, int H, int W, int cin, int cout, int ksize, int in_fmt, int* tile_rows, int* tile_w);
/* Producers of operand rows.  `ys` = operand copy in format `fmt` (LDC_FMT_SPLIT | LDC_FMT_BF16; lds % 8 == 0, >= C rounded up to
 * 8, 32-byte aligned; pad columns zeroed), `y` = fp32 copy (the residual stream / inputs of depthwise convs); either may be NULL,
 * not both. */
int ldc_rmsnorm_rows_split(const float* x, const float* w, const float* b, const float* resid, float* y, float* ys, long long rows,
                           int C, int ldx, int ldr, int ldy, int lds, int fmt, float eps, int act, void* stream);
int ldc_pixel_unshuffle_shortcut_split(const float* cv, const float* x, float* y, float* ys, int B, int H2, int W2, int cout,
                                       int cin, int lds, int fmt, void* stream);
int ldc_pixel_shuffle_shortcut_split(const float* cv, const float* x, float* y, float* ys, int B, int H, int W, int cout, int cin,
                                     int lds, int fmt, void* stream);
/* ABI 4: `cv` of ldc_pixel_shuffle_shortcut_split may be NULL - y is then the block's shortcut term alone,
 * pixel_shuffle(x.repeat_interleave(4 cout / cin, dim=1), 2) (models/DCAE.py:526-530), which the interpolate form of the up block adds to
 * its conv as the residual operand R.  ldc_upsample_nearest2x_rows: F.interpolate(scale_factor=2, mode="nearest") on NHWC rows
 * (models/DCAE.py:519-522, upsample_block_type = "interpolate"): y[b, 2h+i, 2w+j, :] = x[b, h, w, :], as fp32 rows (y, ldy) and / or operand
 * rows (ys, lds, fmt) for the conv that follows; C % 4 == 0. */
int ldc_upsample_nearest2x_rows(const float* x, float* y, float* ys, int B, int H, int W, int C, int ldx, int ldy, int lds, int fmt, void* stream);
/* ABI 5 (round 6): the DC-AE family's `layers_per_block[0] == 0` form (models/DCAE.py:559-579,702-712: no stage at full resolution - the encoder's
 * conv_in is a DCDownBlock2d and the decoder's conv_out a DCUpBlock2d, both WITHOUT shortcut).  `x` of ldc_pixel_unshuffle_shortcut_split may be
 * NULL: y = pixel_unshuffle(cv) alone.  ldc_pixel_shuffle_to_chan: pixel_shuffle of the conv's NHWC rows cv [B][H][W][4 cout] written straight as
 * the NCHW result out [B][keep][2H][2W], the first `keep` <= cout channels (any cout: field counts need not be multiples of 4). */
int ldc_pixel_shuffle_to_chan(const float* cv, float* out, int B, int H, int W, int cout, int keep, void* stream);
int ldc_split_rows(const float* x, float* ys, long long rows, int C, int ldx, int lds, int fmt, void* stream);
/* ldc_sphere_dwconv_nhwc / ldc_relu_linear_attn_nhwc with the output format as an argument (LDC_FMT_F32 | _SPLIT | _BF16). */
int ldc_sphere_dwconv_nhwc_fmt(const float* x, const float* wt, const float* bias, float* y, int B, int H, int W, int C, int ldx,
                               int ldy, int ksize, int glu, int out_fmt, void* stream);
int ldc_relu_linear_attn_nhwc_fmt(const float* qkv, float* y, int B, int P, int groups, int ldq, int ldy, float eps, int out_fmt,
                                  void* workspace, long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Ensemble scoring of one lead time of a decoded forecast:
 *   forecast [M members][C][H*W] with member / channel strides in elements (the H*W plane contiguous), so a
 *   `[:, :, t]` slice of the reference's (ens, C, T, H, W) array needs no copy; truth / clim [C][H*W] with a channel
 *   stride (clim NULL = no ACC); lat_weight [H]; M <= 64.
 *   out [5][C] = ens_acc, ens_mse, crps_spread, crps_skill, crps, each the (nan)mean over the grid of the
 *   latitude-weighted point values; channel `nan_channel` (the SST channel, NaN over land) uses nanmean, the others
 *   mean (-1 = none); ACC always nanmean.  skill_map / spread_map: optional [C][H*W] unweighted point values.
 * Replaces pointwise_crps_skill / pointwise_crps_spread / get_crps / get_acc (ladcast/evaluate/utils.py:51-149) and
 * the per-lead-time block of ladcast/evaluate/evaluate_ens_gpu.py:339-425; one pass over the forecast.
 * workspace: ldc_ensemble_scores_workspace_bytes(C, H, W) bytes of device scratch.
 * ------------------------------------------------------------------------- */
long long ldc_ensemble_scores_workspace_bytes(int C, int H, int W);
int ldc_ensemble_scores(const float* forecast, long long member_stride, long long channel_stride,
                        const float* truth, long long truth_channel_stride, const float* clim,
                        long long clim_channel_stride, const float* lat_weight, int M, int C, int H, int W,
                        int nan_channel, float* out, float* skill_map, float* spread_map, void* workspace,
                        long long workspace_bytes, void* stream);
/* Every lead time of a decode batch of a rollout in one launch (additive under ABI 5): the driver of
 * ladcast/evaluate/evaluate_ens_gpu.py:268-425 scores each decoder output where it lies.  Same point body, arms (M <= 64) and reduction
 * order as ldc_ensemble_scores: column l of `out` holds the bits ldc_ensemble_scores gives for lead time l.
 *   forecast: value (member m, lead l, channel c, point p) at forecast[m*member_stride + l*lead_stride + c*channel_stride + p] (elements;
 *     the H*W plane contiguous): the reference's (ens, C, T, H, W) array, or the decoder's frame-major output for a batch laid out
 *     lead-major then member, (L*ens, C, H, W): lead_stride = ens*C*HW, member_stride = C*HW, channel_stride = HW.
 *   mean / std_ [C] device vectors, target_std: the inverse normalisation of decode_latent_ens fused into the load - every forecast
 *     value becomes (x / target_std) * std_[c] + mean[c], each operation rounded on its own in the order of ldc_chan_affine(inverse=1)
 *     and ldc_track_gather (bit-equal to de-normalising first).  mean == NULL: the forecast is in physical units already.  Truth and
 *     climatology are never transformed.
 *   truth / clim: tables of planes with one slot per lead time.  Lead l, channel c reads the plane at
 *     truth + truth_slot[l]*truth_slot_stride + c*truth_channel_stride (likewise clim; clim == NULL = no ACC).  truth_slot / clim_slot
 *     are DEVICE int arrays [L]; their values are the caller's responsibility (not checked on the device).  A (C, T, H, W) tensor is
 *     slot_stride = HW, channel_stride = T*HW, slots 0..L-1; a resident (N, C, H, W) table is slot_stride = C*HW, channel_stride = HW.
 *   out [5][C][L_total] = ens_acc, ens_mse, crps_spread, crps_skill, crps; columns l_off .. l_off + L - 1 are written, the others are
 *     left alone, so successive launches fill the five (C, total_num_steps) arrays of one initial time.  nan_channel as above.  No
 *     point maps.
 * LDC_ERR_ARG: a null or non-positive argument, a workspace smaller than ldc_rollout_scores_workspace_bytes(C, L, H, W), or
 * l_off + L > L_total; LDC_ERR_UNSUPPORTED: M > 64, C > 65535 or L > 65535. */
long long ldc_rollout_scores_workspace_bytes(int C, int L, int H, int W);
int ldc_rollout_scores(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                       const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                       long long truth_channel_stride, const int* truth_slot, const float* clim, long long clim_slot_stride,
                       long long clim_channel_stride, const int* clim_slot, const float* lat_weight, int M, int C, int L, int H,
                       int W, int nan_channel, float* out, int L_total, int l_off, void* workspace, long long workspace_bytes,
                       void* stream);
/* The three scores of the reference's validation hook (ladcast/train_AR.py:281-312) for every lead time of a decode batch in one launch
 * (additive under ABI 5).  Addressing of forecast, inverse normalisation, truth table, lat_weight, out columns and workspace exactly as
 * ldc_rollout_scores; there is no climatology and no nanmean channel: every average is a plain mean, so one NaN among a point's members
 * or in its truth makes all three scores of that (channel, lead time) NaN and leaves every other one alone.
 *   out [3][C][L_total] = ens_mse, single_mse, crps:
 *     ens_mse    = mean_hw[(mean_i x_i - t)^2 w(lat)]
 *     single_mse = mean_{i,hw}[(x_i - t)^2 w(lat)]   (sum over the members in member order, / M, per point)
 *     crps       = mean_hw[(skill - spread / 2) w(lat)]
 *   Same point body, arms (M <= 64) and reduction order as ldc_rollout_scores: ens_mse and crps hold the bits its `ens_mse` and `crps`
 *   give with clim == NULL and nan_channel == -1; at M == 1 single_mse holds the bits of ens_mse.  No float atomics: run-to-run bit-equal.
 * Errors as ldc_rollout_scores, with ldc_validation_scores_workspace_bytes(C, L, H, W). */
long long ldc_validation_scores_workspace_bytes(int C, int L, int H, int W);
int ldc_validation_scores(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                          const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                          long long truth_channel_stride, const int* truth_slot, const float* lat_weight, int M, int C, int L, int H,
                          int W, float* out, int L_total, int l_off, void* workspace, long long workspace_bytes, void* stream);
/* Ensemble reliability for every lead time of a decode batch in one launch (additive under ABI 5; reliability.hip):
 * spread-skill ratio and rank histogram.  Not in the reference.  Addressing of forecast, inverse normalisation, truth table, lat_weight,
 * out columns and nan_channel exactly as ldc_rollout_scores; no climatology.  There is no sort, so 1 <= M <= 1024.
 * Per point, members x_i in member order: mean = sum_i x_i / M, se = (mean - t)^2, var = sum_i (x_i - mean)^2 / (M - 1) (two-pass;
 * M == 1: NaN), rank bin = #{x_i < t} + (#{x_i == t} >> 1) in 0 .. M (ties: deterministic mid-rank).  A point is valid for the histogram
 * when no member and not the truth is NaN; +-inf are ordinary ordered values.
 *   out [3][C][L_total] = ens_mse = <w se>, ens_var = <w var>, ssr = sqrt((M + 1) / M) * sqrt(ens_var / ens_mse); each average is a plain
 *     mean (one NaN point -> NaN) except in channel nan_channel (nanmean over the points where the value is not NaN).  For M <= 64 ens_mse
 *     holds the bits of ldc_rollout_scores' ens_mse.
 *   hist_count  [C][L_total][M + 1] int32: valid points per rank bin
 *   hist_weight [C][L_total][M + 1] fp32: sum of w over the valid points per bin, in a fixed order
 *   n_invalid   [C][L_total] int32: points left out of the histogram
 *   Columns l_off .. l_off + L - 1 of every output are written, the others left alone.  No float atomics: run-to-run bit-equal.
 * workspace: ldc_rollout_reliability_workspace_bytes(M, C, L, H, W) bytes of device scratch (0 for arguments the call refuses).
 * LDC_ERR_ARG: a null or non-positive argument (M <= 0 among them), a workspace that is too small, or l_off + L > L_total;
 * LDC_ERR_UNSUPPORTED: M > 1024, C > 65535, L > 65535 or H * W > 2^24.  Nothing is launched on an error. */
long long ldc_rollout_reliability_workspace_bytes(int M, int C, int L, int H, int W);
int ldc_rollout_reliability(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                            const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                            long long truth_channel_stride, const int* truth_slot, const float* lat_weight, int M, int C, int L, int H,
                            int W, int nan_channel, float* out, int* hist_count, float* hist_weight, int* n_invalid, int L_total,
                            int l_off, void* workspace, long long workspace_bytes, void* stream);
/* Zonal power spectra for every lead time of a decode batch in one launch (additive under ABI 5; spectrum.hip):
 * power per longitudinal wavenumber of the members, of the ensemble mean and of the truth.  Not in the reference.  Addressing of
 * forecast, inverse normalisation (mean == NULL: physical units), truth table and out columns exactly as ldc_rollout_reliability; no
 * climatology and no nan_channel.  row_weight [H] fp32 on the device replaces the latitude weight and must be >= 0 (the call cannot
 * check device memory: a negative or NaN weight is treated as 0).  A row of weight 0 is not read: NaN or inf there has no effect.
 * Definitions, per row of W points with positive weight, x_i the de-normalised members, t the truth, m_j = (sum_i x_ij) / M summed in
 * member order in fp32 (as ldc_rollout_reliability), K = W / 2 + 1, and for a real sequence y:
 *     Y_k = sum_j y_j exp(-2 pi i j k / W),  P_k(y) = s_k |Y_k|^2 / W^2,  s_0 = s_{W/2} = 1, s_k = 2 otherwise: sum_k P_k = mean_j y_j^2
 *   P_0 is the square of the row mean (pair sums in index order, then a butterfly); the bins k >= 1 are transformed from the residual
 *   y_j - mean, folded by the real-input symmetry, with twiddles from one W-entry table per launch (fp64 sincospi rounded to fp32) and
 *   explicit fused multiply-adds in index order; |Y_k|^2 and every sum over members and rows are fp64.
 * Validity: a row is valid when none of its (M + 1) W member and truth values is NaN after the inverse normalisation; +-inf are
 *   ordinary values (they give inf or NaN power).  Invalid rows are left out of every average and counted.
 *   out [3][C][L_total][K] fp32 = spec_members = <(1 / M) sum_i P_k(x_i)>, spec_mean = <P_k(m)>, spec_truth = <P_k(t)>, with
 *     <.> = sum_h w_h (.) / sum_h w_h over the valid rows of that (c, l); no valid row: NaN in all 3 K values.  At M == 1 spec_members
 *     and spec_mean are equal bit for bit.
 *   n_invalid [C][L_total] int32: rows of positive weight left out.
 *   Columns l_off .. l_off + L - 1 of both outputs are written, the others left alone.  No atomics: run-to-run bit-equal.
 * workspace: ldc_rollout_spectrum_workspace_bytes(M, C, L, H, W) bytes of device scratch, 16-byte aligned (0 for arguments the call
 *   refuses).
 * LDC_ERR_ARG: a null or non-positive argument, l_off + L > L_total or a workspace that is too small; LDC_ERR_UNSUPPORTED: M > 1024,
 * W odd, W < 4, W > 512, H * W > 2^24, C > 65535 or L > 65535; LDC_ERR_ALIGN: workspace not 16-byte aligned.  Nothing is launched on
 * an error. */
long long ldc_rollout_spectrum_workspace_bytes(int M, int C, int L, int H, int W);
int ldc_rollout_spectrum(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                         const float* mean, const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                         long long truth_channel_stride, const int* truth_slot, const float* row_weight, int M, int C, int L, int H,
                         int W, float* out, int* n_invalid, int L_total, int l_off, void* workspace, long long workspace_bytes,
                         void* stream);
/* Ensemble products for every lead time of a decode batch in one launch (additive under ABI 5; products.hip):
 * per grid point the ensemble mean, spread, range, quantiles and probabilities of exceeding a threshold.  Not in the reference.  There
 * is no truth.  Addressing of forecast, inverse normalisation (mean == NULL: physical units; mean / std_ indexed by the ORIGINAL
 * channel) and output columns exactly as ldc_rollout_scores; pointwise, so no workspace.
 * channels: optional device int32 [Cs], indices into the C channels in any order; NULL: all channels (Cs must equal C).  The outputs
 *   hold Cs channels in list order.  The indices are the caller's responsibility (the call cannot read device memory).
 * Per point, the M members x_i in member order after the inverse normalisation:
 *   stats [4][Cs][L_total][H][W] = mean, std, min, max: mean = (sequential fp32 sum) / M; std = sqrt(sum_i (x_i - mean)^2 / (M - 1)),
 *     two-pass (M == 1: NaN), the variance of ldc_rollout_reliability
 *   quant [Q][Cs][L_total][H][W], Q = desc->n_quant <= LDC_PRODUCTS_MAX_QUANTILES: quantile k is given as (q_lo[k], q_t[k]), which the
 *     host derives from q in [0, 1] in float64: pos = q (M - 1), lo = min(floor(pos), M - 1), t = float(pos - lo).  With the sorted
 *     members x_(0) <= ... <= x_(M-1): x_(lo) untouched when t == 0, else a + (b - a) * t, a = x_(lo), b = x_(min(lo + 1, M - 1)), three
 *     fp32 operations without contraction (numpy's method="linear").  0 <= q_lo <= M - 1 and 0 <= q_t <= 1 are checked.
 *   exceed [P][Cs][L_total][H][W], P = desc->n_thr <= LDC_PRODUCTS_MAX_THRESHOLDS: thr [P][Cs] fp32 on the device, in physical units;
 *     thr_dir[k] = +1: #{x_i > thr} / M, -1: #{x_i < thr} / M.  A NaN threshold makes that (k, channel) plane NaN.
 *   A point with a NaN member is NaN in every output; +-inf are ordinary ordered values (IEEE arithmetic).
 *   Each output pointer is optional: NULL = not computed, not written.  Columns l_off .. l_off + L - 1 are written, the others left alone.
 * With quantiles the members are sorted in registers: M <= 64.  Without (Q == 0 or quant == NULL): 1 <= M <= 1024.
 * LDC_ERR_ARG: a null forecast or desc, a non-positive size (M <= 0 among them), l_off + L > L_total, channels == NULL with Cs != C,
 * more quantiles or thresholds than the caps, a (q_lo, q_t) out of range, a direction that is not +-1, thr == NULL with thresholds, or
 * no output at all; LDC_ERR_UNSUPPORTED: M > 1024, M > 64 with quantiles, Cs > 65535, L > 65535 or H * W > 2^24.  Nothing is launched
 * on an error. */
#define LDC_PRODUCTS_MAX_QUANTILES 16
#define LDC_PRODUCTS_MAX_THRESHOLDS 8
typedef struct ldc_products_desc {
  int n_quant; /* Q */
  int n_thr;   /* P */
  int q_lo[LDC_PRODUCTS_MAX_QUANTILES];
  float q_t[LDC_PRODUCTS_MAX_QUANTILES];
  int thr_dir[LDC_PRODUCTS_MAX_THRESHOLDS];
} ldc_products_desc;
int ldc_sizeof_products_desc(void);
int ldc_rollout_products(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride,
                         const float* mean, const float* std_, float target_std, const int* channels, int M, int C, int Cs, int L, int H,
                         int W, const ldc_products_desc* desc, const float* thr, float* stats, float* quant, float* exceed, int L_total,
                         int l_off, void* stream);
/* Verification of threshold events for every lead time of a decode batch in one launch (additive under ABI 5; events.hip, DESIGN.md
 * section 8.4): per (event, lead time) the joint histogram of "how many of the M members show the event" against "did the truth show
 * it", counted and latitude-weighted - the sufficient statistic of the Brier score and its decomposition, the reliability diagram and
 * the ROC curve (ladcast_amd.evaluate.event_scores derives them on the host).  Not in the reference.  Addressing of forecast, inverse
 * normalisation (mean == NULL: physical units), truth table, lat_weight and output columns exactly as ldc_rollout_reliability; the
 * optional climatology table (clim, clim_slot_stride, clim_channel_stride, clim_slot: a DEVICE int array [L]) exactly as
 * ldc_rollout_scores.  1 <= M <= 1024.
 * desc: HOST descriptor of the E = n_events <= LDC_EVENTS_MAX events, read and checked in full by the call.  Event e looks at channel
 *   c = channel[e] of the C channels; several events may share a channel.
 * Per grid point of event e, the members x_i in member order after the inverse normalisation, truth t, climatology a:
 *   u_i = x_i, v = t                 (anomaly[e] == 0)
 *   u_i = x_i - a, v = t - a         (anomaly[e] == 1: one fp32 subtraction each; needs clim)
 *   n = #{i : u_i > thr[e]} in 0 .. M and o = (v > thr[e]) in {0, 1} for dir[e] == +1; `<` in place of `>` for dir[e] == -1
 *   the point is valid when no member, not the truth and (anomaly[e] == 1) not the climatology is NaN; +-inf are ordinary ordered values
 *   hist_count  [E][L_total][M + 1][2] int32: valid points per (n, o)
 *   hist_weight [E][L_total][M + 1][2] fp32: sum of lat_weight over those points, in a fixed order
 *   n_invalid   [E][L_total] int32: points left out
 *   Columns l_off .. l_off + L - 1 of every output are written, the others left alone.  No float atomics: run-to-run bit-equal.
 * workspace: ldc_rollout_events_workspace_bytes(M, E, L, H, W) bytes of device scratch (0 for arguments the call refuses).
 * LDC_ERR_ARG: a null or non-positive argument, n_events outside 1 .. LDC_EVENTS_MAX, a channel outside 0 .. C - 1, a direction that is
 * not +-1, an anomaly that is not 0 / 1, anomaly == 1 with clim == NULL, clim without clim_slot, a NaN threshold, l_off + L > L_total or
 * a workspace that is too small; LDC_ERR_UNSUPPORTED: M > 1024, L > 65535 or H * W > 2^24.  Nothing is launched on an error. */
#define LDC_EVENTS_MAX 32
typedef struct ldc_events_desc {
  int n_events;                /* E */
  int channel[LDC_EVENTS_MAX]; /* index into the C channels */
  int dir[LDC_EVENTS_MAX];     /* +1: value > thr, -1: value < thr */
  int anomaly[LDC_EVENTS_MAX]; /* 1: value is x - clim (needs clim), 0: value is x */
  float thr[LDC_EVENTS_MAX];   /* physical units (of the anomaly where anomaly == 1) */
} ldc_events_desc;
int ldc_sizeof_events_desc(void);
long long ldc_rollout_events_workspace_bytes(int M, int E, int L, int H, int W);
int ldc_rollout_events(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride, const float* mean,
                       const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                       long long truth_channel_stride, const int* truth_slot, const float* clim, long long clim_slot_stride,
                       long long clim_channel_stride, const int* clim_slot, const float* lat_weight, int M, int C, int L, int H, int W,
                       const ldc_events_desc* desc, int* hist_count, float* hist_weight, int* n_invalid, int L_total, int l_off,
                       void* workspace, long long workspace_bytes, void* stream);
/* Neighbourhood verification of the same threshold events for every lead time of a decode batch (additive under ABI 5; fss.hip,
 * DESIGN.md section 8.6): the additive sufficient statistics of the fractions skill score (Roberts & Lean 2008) per (event,
 * neighbourhood radius, lead time).  ladcast_amd.evaluate.fss_scores derives the scores on the host in float64; sums of several initial
 * times add.  Not in the reference.  Every argument up to desc exactly as ldc_rollout_events, and the classification of a grid point q
 * of event e - n(q) in 0 .. M, o(q) in {0, 1}, valid(q) - is the one documented there (one shared device function).  1 <= M <= 1024.
 * radii: HOST array of S <= LDC_FSS_SCALES_MAX radii r >= 0 in GRID POINTS (copied into the launch); the window is (2 r + 1) x (2 r + 1)
 *   points: rows i - r .. i + r clipped to 0 .. H - 1, columns j - r .. j + r modulo W (longitude is periodic).  Its width in
 *   kilometres shrinks towards the poles; nothing corrects for that.
 * Over the valid points of the window of centre p = (i, j), exact integers:  N = #valid, Sn = sum n(q), So = sum o(q).  A centre
 * contributes when p itself is valid (N >= 1): land centres of SST are not scored, land neighbours enter neither fraction.  Per
 * contributing centre, fp64, every operation rounded on its own, w = double(lat_weight[i]):
 *   Pf = double(Sn) / (double(M) * double(N)),  Po = double(So) / double(N),  a = w * Pf,  b = w * Po,  d = Pf - Po
 *   fss_sums  [E][S][L_total][6] fp64: the sums over the contributing centres of  w, a, b, a * Pf, b * Po, (w * d) * d  - all
 *     non-negative; FSS = 1 - s5 / (s3 + s4).  r = 0 makes s5 the numerator of the Brier score of ldc_rollout_events.
 *   n_invalid [E][L_total] int32: the centres left out, equal to ldc_rollout_events' n_invalid.
 *   Columns l_off .. l_off + L - 1 of both outputs are written, the others left alone.  No atomics: run-to-run bit-equal.
 * workspace: ldc_rollout_fss_workspace_bytes(M, E, S, L, H, W) bytes of device scratch, 8-byte aligned (0 for arguments the call
 *   refuses): 16 bytes per point and (event, lead time) - a packed word and a summed-area table entry of three uint32 - plus the
 *   workgroup records.
 * LDC_ERR_ARG: everything ldc_rollout_events refuses, radii == NULL, S outside 1 .. LDC_FSS_SCALES_MAX, a negative radius, a window
 * with 2 r + 1 > W (it would meet itself; 2 r + 1 >= H is served: every row) or a workspace that is too small; LDC_ERR_UNSUPPORTED:
 * M > 1024, L > 65535, H * W > 2^24 or M * H * W > 2^31 (Sn is held in uint32); LDC_ERR_ALIGN: workspace or fss_sums not 8-byte
 * aligned.  Nothing is launched on an error. */
#define LDC_FSS_SCALES_MAX 16
long long ldc_rollout_fss_workspace_bytes(int M, int E, int S, int L, int H, int W);
int ldc_rollout_fss(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride, const float* mean,
                    const float* std_, float target_std, const float* truth, long long truth_slot_stride, long long truth_channel_stride,
                    const int* truth_slot, const float* clim, long long clim_slot_stride, long long clim_channel_stride,
                    const int* clim_slot, const float* lat_weight, int M, int C, int L, int H, int W, const ldc_events_desc* desc,
                    const int* radii, int S, double* fss_sums, int* n_invalid, int L_total, int l_off, void* workspace,
                    long long workspace_bytes, void* stream);
/* Regional ensemble scores for every lead time of a decode batch in one launch (additive under ABI 5; regional.hip, DESIGN.md section
 * 8.5): for up to 32 regions that may overlap, the additive sufficient statistics of bias, RMSE, spread, spread-skill ratio, CRPS and
 * ACC per (region, channel, lead time).  ladcast_amd.evaluate.regional_scores derives the scores on the host in float64; sums of several
 * initial times add.  Not in the reference.  Addressing of forecast, inverse normalisation (mean == NULL: physical units), truth and
 * climatology tables (clim == NULL: no ACC terms), lat_weight and output columns exactly as ldc_rollout_scores.  1 <= M <= 64.
 * region_mask: DEVICE uint32 [H * W]; bit r of word p says that point p belongs to region r, r < R <= 32 (bits >= R are ignored).
 *   Regions may overlap, be empty, or leave points uncovered.  A point with no bit below R is not read: NaN or inf there has no effect.
 * Per point, all fp32, the members x_i in member order after the inverse normalisation, truth t, weight w = lat_weight[row],
 * climatology a, each value formed as the kernel that already has it forms it:
 *   mean = (x_0 + ... + x_{M-1}) / M (sequential), e = mean - t, se = e * e                    (ldc_rollout_scores)
 *   var = sum_i (x_i - mean)^2 / (M - 1), two-pass in member order; M == 1: 0                  (ldc_rollout_reliability)
 *   skill = sum_i |t - x_i| / M;  spread = 2 / (M (M - 1)) * sum_i (2 i - M - 1) x_(i) over the sorted members; M == 1: 0
 *   fa = mean - a, ta = t - a, and the fp32 products fa * ta, fa * fa, ta * ta
 * Validity: a point is valid when no member and not the truth is NaN, ACC-valid when it is valid and a is not NaN; +-inf are ordinary
 *   values (the sums then follow IEEE).  Unlike ldc_rollout_scores there is no mean / nanmean distinction and no nan_channel: in EVERY
 *   channel the invalid points are left out and counted, so SST over land drops out by itself and one bad point does not make a
 *   regional score NaN.
 *   sums   [R][C][L_total][10] fp64: over the region's valid points  sum w, sum w e, sum w se, sum w var, sum w skill, sum w spread;
 *     over its ACC-valid points  sum w, sum w fa ta, sum w fa^2, sum w ta^2 (these four are zeros when clim == NULL).  Every term is
 *     double(w) * double(v), which is exact: the only rounding behind the fp32 point values is that of the fp64 additions.
 *   counts [R][C][L_total][3] int32: the valid points of the region, the invalid ones, the ACC-valid ones.
 *   Columns l_off .. l_off + L - 1 of both outputs are written, the others left alone.  No atomics: run-to-run bit-equal, and the sums
 *   of region r do not depend on R or on the other regions (one region passed alone gives the bits it gives among 31 others).
 * workspace: ldc_rollout_regional_workspace_bytes(M, R, C, L, H, W) bytes of device scratch, 8-byte aligned (0 for arguments the call
 *   refuses): 1.5 bytes per point and (channel, lead time), whatever R is.
 * LDC_ERR_ARG: a null or non-positive argument (R <= 0 among them), clim without clim_slot, mean without std_, l_off + L > L_total or a
 * workspace that is too small; LDC_ERR_UNSUPPORTED: M > 64, R > 32, C > 65535, L > 65535 or H * W > 2^24; LDC_ERR_ALIGN: workspace or
 * sums not 8-byte aligned.  Nothing is launched on an error. */
long long ldc_rollout_regional_workspace_bytes(int M, int R, int C, int L, int H, int W);
int ldc_rollout_regional(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride, const float* mean,
                         const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                         long long truth_channel_stride, const int* truth_slot, const float* clim, long long clim_slot_stride,
                         long long clim_channel_stride, const int* clim_slot, const float* lat_weight, const unsigned* region_mask, int R,
                         int M, int C, int L, int H, int W, double* sums, int* counts, int L_total, int l_off, void* workspace,
                         long long workspace_bytes, void* stream);
/* Energy score of a decoded ensemble for every lead time of a decode batch (additive under ABI 5; energy.hip): the
 * multivariate generalisation of the CRPS, ES = mean_i ||x_i - t|| - 1/2 mean_{i,j} ||x_i - x_j|| with ||.|| the latitude-weighted RMS
 * norm of a whole field, per (channel, lead time) and per group of channels.  It tells an ensemble of coherent fields from one whose
 * members are the right marginal distribution shuffled point by point, which no pointwise score can.  Not in the reference.  Addressing
 * of forecast, inverse normalisation (mean == NULL: physical units), truth table, lat_weight and output columns exactly as
 * ldc_rollout_regional.  1 <= M <= 256.
 * Per (channel c, lead l), vectors y_0 .. y_{M-1} the members after the inverse normalisation and y_M the truth:
 *   a point p is valid when no member and not the truth is NaN; invalid points contribute nothing and are counted; +-inf are ordinary
 *   values (inf - inf makes the affected entries NaN, as IEEE says)
 *   D2[a][b] = sum over valid p of double(w_p) * double(sq), d = y_a[p] - y_b[p] (one fp32 subtraction), sq = d * d (one fp32 product),
 *     w_p = lat_weight[row(p)]; the product is exact: the only roundings are the two fp32 operations and the fp64 additions.  D2 is
 *     symmetric (entry (b, a) holds the bits of (a, b)) and its diagonal is written as 0 whatever the values are.
 *   Wv = sum over valid p of double(w_p);  norm(a, b) = sqrt(D2[a][b] / Wv) in fp64 (IEEE sqrt and divide)
 *   skill = (sum_i norm(i, M)) / M;  spread = (sum_{i != j} norm(i, j)) / (M M);  spread_fair = the same sum / (M (M - 1)), 0 at M == 1;
 *   the sums run sequentially in (i, j) lexicographic order;  es = skill - 0.5 spread;  es_fair = skill - 0.5 spread_fair;  the four
 *   are NaN when Wv == 0.  For a single valid point es_fair is the CRPS of that point.
 * Groups (0 <= G <= 32, may overlap): group_mask DEVICE uint32 [C], bit g of word c says that channel c belongs to group g (bits >= G
 *   are ignored); inv_scale2 DEVICE fp64 [C] = 1 / scale_c^2.  D2_g[a][b] = sum over c in g, ascending, of D2_c[a][b] * inv_scale2[c]
 *   (each product rounded), Wv_g = sum over c in g of Wv_c, and the same five quantities follow; a group without a channel is NaN.
 *   energy       [5][C][L_total] fp64: es, es_fair, skill, spread, Wv
 *   energy_group [5][G][L_total] fp64: the same per group; NULL if and only if G == 0 (group_mask and inv_scale2 are then not read)
 *   n_invalid    [C][L_total] int32: the invalid points
 *   dist2        [C][L_total][M + 1][M + 1] fp64: D2, for diagnostics; NULL: not written
 *   Columns l_off .. l_off + L - 1 are written, the others left alone.  No atomics: the fp64 additions run in an order that depends on
 *   H, W and M only, so two runs give the same bits and a column's bits do not depend on C, L, L_total, l_off, the strides, G, the other
 *   channels or dist2.
 * workspace: ldc_rollout_energy_workspace_bytes(M, C, G, L, H, W) bytes of device scratch, 8-byte aligned (0 for arguments the call
 *   refuses).  With NB = ceil((M + 1) / 4) it holds, per (channel, lead time), ceil(H W / 4096) + 1 records of NB (NB + 1) / 2 blocks
 *   of 16 fp64 - the partial matrices of the point chunks and their total.  That term, 4 (M + 1)^2 bytes per record to leading order
 *   (268 KiB at M = 256, 2.4 MB per (channel, lead time) on a 120 x 240 grid), is what bounds M at 256.
 * LDC_ERR_ARG: a null or non-positive argument, G < 0, G > 0 without group_mask / inv_scale2 / energy_group, energy_group with G == 0,
 * mean without std_, l_off + L > L_total or a workspace that is too small; LDC_ERR_UNSUPPORTED: M > 256, G > 32, C > 65535, L > 65535
 * or H * W > 2^24; LDC_ERR_ALIGN: workspace, energy, energy_group, dist2 or inv_scale2 not 8-byte aligned.  Nothing is launched on an
 * error. */
long long ldc_rollout_energy_workspace_bytes(int M, int C, int G, int L, int H, int W);
int ldc_rollout_energy(const float* forecast, long long member_stride, long long lead_stride, long long channel_stride, const float* mean,
                       const float* std_, float target_std, const float* truth, long long truth_slot_stride,
                       long long truth_channel_stride, const int* truth_slot, const float* lat_weight, const unsigned* group_mask,
                       const double* inv_scale2, int G, int M, int C, int L, int H, int W, double* energy, double* energy_group,
                       int* n_invalid, double* dist2, int L_total, int l_off, void* workspace, long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Tropical-cyclone tracking through a decoded ensemble (track.hip).  Replaces the reference's tracker,
 * ladcast/evaluate/track.py:151-335 (round_to_grid / select_box / find_local_minimum / track_first_n_steps), run on the
 * xarray dataset that ladcast/pipelines/utils.py:83-246 (latent_ens_to_xarr) decodes into: the decoded frames stay on the
 * device, only the tracker's channels are gathered, the ensemble mean is taken on the device and every track runs in one
 * launch.  The grid is two ASCENDING fp64 coordinate arrays built on the host exactly as the reference builds them
 * (lat = np.arange(-88.5, 90 + 1e-6, 1.5), 120 rows; lon = np.arange(0, 358.5 + 1e-6, 1.5), 240 columns); fields are fp32
 * [H][W] planes, row = latitude.  Box bounds are index ranges found by comparing against those arrays, and the coordinate
 * arithmetic rounds as Python's float ops do (Python's `%` included).  H, W <= LDC_TRACK_MAX_GRID.  Any strictly ascending
 * finite grid is served (regional, irregular, one row or column, 0 and 360 both present); a non-finite centre finds nothing.
 * The distance key that picks the closest surviving minimum, (la - lat0)**2 + ((lo - lon0 + 180) % 360 - 180)**2 in the
 * reference, is computed as d * d, each product correctly rounded.  It equals the reference bit for bit whenever the
 * coordinate differences square exactly (the default grid; any dyadic grid and centre).  Otherwise CPython's pow(d, 2) can
 * differ from d * d by one rounding per term, which can decide only between candidates whose keys are within 2 ulp of each
 * other; candidates with equal keys keep the reference's visiting order (rows ascending, then columns ascending, the small
 * longitudes of a box that wraps first).
 * ------------------------------------------------------------------------- */
#define LDC_TRACK_MAX_CHANNELS 8
#define LDC_TRACK_MAX_BOXES 8 /* entries of inner_box_sizes */
#define LDC_TRACK_MAX_INNER 30 /* degrees, per inner box size */
#define LDC_TRACK_MAX_GRID 1024
/* Channel gather with the inverse normalisation of decode_latent_ens (pipelines/utils.py:51-80):
 *   out[b][t_off + t][k][p] = (x[b*sb + t*st + channels[k]*sc + p] / target_std) * std[channels[k]] + mean[channels[k]]
 * for b < B, t < T, k < n_ch, p < HW; out is (B, T_total, n_ch, HW), so decoding in frame batches fills one buffer.  x is the
 * decoder's output in any layout with a contiguous HW plane: (B, C, T, HW) or the frame-major (B*T, C, HW) the decoder returns.
 * Same operations in the same order as ldc_chan_affine(inverse=1): bit-equal to decode_latent_ens(...)[:, channels].
 * `channels` is a HOST array of n_ch <= LDC_TRACK_MAX_CHANNELS indices (copied into the launch); mean / std are device vectors
 * indexed by channel.  LDC_ERR_UNSUPPORTED when n_ch is above its cap, B > 65535 or T * n_ch > 65535 (nothing is launched). */
int ldc_track_gather(const float* x, long long sb, long long st, long long sc, int B, int T, long long HW, const int* channels,
                     int n_ch, const float* mean, const float* std_, float target_std, float* out, int T_total, int t_off,
                     void* stream);
/* Derived fields (additive under ABI 5; derive.hip): new planes computed from de-normalised channels, the
 * sibling of ldc_track_gather.  Value (outer o, lead l, channel c, point p) of the source is
 *   x = src[o*outer_stride + (slot ? slot[l] : l)*lead_stride + c*channel_stride + p],  o < n_outer, l < L, c < C, p < HW
 * with a contiguous HW plane: the decoder's output (outer = member, any layout the scorers' forecast accepts), or a truth /
 * climatology table (n_outer = 1, slot a DEVICE int array [L]; the kernel trusts the slots).  mean / std_ (device vectors [C]) and
 * target_std de-normalise it exactly as the scorers do, (x / target_std) * std_[c] + mean[c], the division skipped for
 * target_std == 1; mean == NULL (then std_ == NULL too): the source is physical already and its bits are taken as they are.
 * desc: HOST array of D <= LDC_DERIVE_MAX_FIELDS fields, copied into the launch.  With a, b, c, d the de-normalised channels
 * ch[0 .. 3] of a field (a channel may appear in several fields and twice in one):
 *   LDC_DERIVE_DIFF   a - b, one fp32 subtraction: bit-equal to subtracting the de-normalised planes
 *   LDC_DERIVE_SPEED  (float)sqrt((double)a*a + (double)b*b)
 *   LDC_DERIVE_SHEAR  (float)sqrt(x*x + y*y), x = (double)a - c, y = (double)b - d
 * in double the squares are exact and neither overflow nor underflow; the sum and the root round once each, the cast once more.  A
 * NaN input gives NaN, inf follows IEEE.  Field k is written to out[o*out_outer_stride + l*out_lead_stride + k*out_channel_stride + p]:
 * the tail channels of a larger tensor, or a tensor of its own.  out must not overlap the planes that are read.
 * Every distinct source plane is read once per launch; fields are served in order, at most 16 distinct source channels per launch
 * (D = 16 SHEAR fields of 64 different channels take four launches).  16-byte loads and stores when HW % 4 == 0 and src, out and the
 * six strides keep 16-byte alignment; a scalar path otherwise.  No atomics, no workspace.
 * LDC_ERR_ARG: a null src / desc / out, mean without std_ or the reverse, a non-positive size, a negative stride, D outside
 * 1 .. LDC_DERIVE_MAX_FIELDS, an unknown kind, a channel outside 0 .. C - 1; LDC_ERR_UNSUPPORTED: L or n_outer above 65535.  Nothing is
 * launched on an error. */
#define LDC_DERIVE_MAX_FIELDS 16
#define LDC_DERIVE_SPEED 0 /* ch[0 .. 1] = a, b */
#define LDC_DERIVE_DIFF 1  /* ch[0 .. 1] = a, b */
#define LDC_DERIVE_SHEAR 2 /* ch[0 .. 3] = a, b, c, d */
typedef struct ldc_derive_desc {
  int kind;
  int ch[4]; /* indices into the C channels; entries the kind does not use are ignored */
} ldc_derive_desc;
int ldc_sizeof_derive_desc(void);
int ldc_derive_fields(const float* src, long long outer_stride, long long lead_stride, long long channel_stride, const int* slot,
                      const float* mean, const float* std_, float target_std, int n_outer, int L, int C, long long HW,
                      const ldc_derive_desc* desc, int D, float* out, long long out_outer_stride, long long out_lead_stride,
                      long long out_channel_stride, void* stream);
/* Derived fields that need horizontal derivatives (additive under ABI 5; sphere_derive.hip): relative vorticity
 * and divergence of a wind (u, v) = channels ch[0], ch[1] on a latitude-longitude grid, rows j < H at latitude phi_j, columns i < W at
 * longitude 2 pi i / W (a full periodic circle).  Source addressing, slot, mean / std_ / target_std and the three out strides mean
 * exactly what they mean for ldc_derive_fields, with HW = H * W and a contiguous (H, W) plane.  With
 *   LDC_SPHERE_VORTICITY   (a, b) = (u, v)
 *   LDC_SPHERE_DIVERGENCE  (a, b) = (-v, u)      D(u, v) = zeta(-v, u): one code path, the negation is exact
 * de-normalised in fp32 and widened to double, jn = min(j + 1, H - 1), js = max(j - 1, 0), ie = (i + 1) mod W, iw = (i - 1 + W) mod W:
 *   r[j] != 0:  dl = (b[j][ie] - b[j][iw]) * k;  dp = (a[jn][i] * c[jn] - a[js][i] * c[js]) * q[j];  out = (float)((dl - dp) * r[j])
 *   r[j] == 0:  out = (float)((sum_i a[jp][i]) / W * pc[j]) for every i, jp = 1 for j == 0, else j - 1       (a pole row)
 * every operation an IEEE double operation in this order (the file is built with -ffp-contract=off), one rounding to fp32.
 * row_tables: DEVICE fp64 [4][H] = c, q, r, pc, made by the host (ladcast_amd.evaluate.derived.sphere_row_tables): c = cos phi (0 on a
 * pole row), q = 1 / (phi[jn] - phi[js]), r = 1 / (R c) (0 on a pole row: that marks it), pc = the polar-cap factor; k = W / (4 pi).
 * The kernel trusts the table.  One wave owns one row; a pole row's sum is taken by its wave: lane l adds elements l, l + 64, ... in
 * double, then the xor butterfly 32 .. 1 - a fixed order, the same call gives the same bits.  A NaN input gives NaN at exactly the
 * points whose stencil reads it (a whole pole row for a NaN anywhere in row jp); inf follows IEEE.  out must not overlap the planes
 * that are read.  16-byte loads and stores when W % 4 == 0 and src, out and the six strides keep 16-byte alignment; a scalar path
 * otherwise.  No atomics, no workspace, no scratch.
 * LDC_ERR_ARG: a null src / row_tables / desc / out, mean without std_ or the reverse, a non-positive size, H < 2, W < 3, a negative
 * stride, D outside 1 .. LDC_DERIVE_MAX_FIELDS, an unknown kind, a channel outside 0 .. C - 1; LDC_ERR_UNSUPPORTED: L or n_outer above
 * 65535.  Nothing is launched on an error. */
#define LDC_SPHERE_VORTICITY 0
#define LDC_SPHERE_DIVERGENCE 1
typedef struct ldc_sphere_desc {
  int kind;
  int ch[2]; /* u, v: indices into the C channels */
} ldc_sphere_desc;
int ldc_sizeof_sphere_desc(void);
int ldc_derive_sphere(const float* src, long long outer_stride, long long lead_stride, long long channel_stride, const int* slot,
                      const float* mean, const float* std_, float target_std, int n_outer, int L, int C, int H, int W,
                      const double* row_tables, double k, const ldc_sphere_desc* desc, int D, float* out,
                      long long out_outer_stride, long long out_lead_stride, long long out_channel_stride, void* stream);
/* out[i] = np.nanmean over e < E of x[e*member_stride + i], i < n (fp32, the reference's ds.mean(dim="idx")): NaNs skipped, the
 * sum taken in member order, one division by the count (NaN where every member is NaN). */
int ldc_track_nanmean(const float* x, long long member_stride, int E, long long n, float* out, void* stream);
/* track_first_n_steps for n_tracks tracks, one wave each, every step and every inner box size in one launch.
 *   track e, frame f: the MSLP plane at fields + e*track_stride + f*frame_stride + mslp_off, the Z700 plane at ... + z_off;
 *   frame f = lead 6 h * f, frame 0 the initial condition (read by no step).
 *   lat0 / lon0 [n_tracks]: the start, already round_to_grid'ed on the host (lon0 may be 360.0).
 *   inner_box_sizes: HOST array of n_boxes <= LDC_TRACK_MAX_BOXES sizes, each in [0, LDC_TRACK_MAX_INNER] degrees.
 *   enforce_msl = 0: lsm [H][W] (land-sea mask, nearest lookup with pandas' rule) picks MSLP (< 0.5) or not, then Z700 if MSLP
 *   did not move the track; z_off >= 0 and lsm are required.  enforce_msl != 0: MSLP only (lsm, z_off unused).
 *   out_lat / out_lon [n_tracks][n_steps + 1] fp64: the track, step 0 = the start.
 *   out_code [n_tracks][n_steps]: per step 0 = stayed (the reference warns), 1 + k = moved on MSLP with box k,
 *   1 + n_boxes + k = moved on Z700 with box k.
 * LDC_ERR_UNSUPPORTED when n_boxes or an inner size is above its cap (nothing is launched). */
int ldc_track_storms(const float* fields, long long track_stride, long long frame_stride, long long mslp_off, long long z_off,
                     const float* lsm, const double* lat, int H, const double* lon, int W, const double* lat0,
                     const double* lon0, int n_tracks, int n_steps, const int* inner_box_sizes, int n_boxes, int enforce_msl,
                     double* out_lat, double* out_lon, int* out_code, void* stream);
/* A batch of single find_local_minimum calls (track.py:173-238), so the search can be pinned apart from the track loop:
 * query q searches the plane fields + field_idx[q]*field_stride around (lat0[q], lon0[q]) with inner size inner[q] (device arrays).
 * found[q] = 1 -> (out_lat, out_lon, out_val)[q] = the reference's (la, lo, v); 0 -> the reference returns None;
 * LDC_ERR_UNSUPPORTED -> inner[q] outside [0, LDC_TRACK_MAX_INNER], not searched (the host binding refuses those before launch). */
int ldc_track_local_min(const float* fields, long long field_stride, const int* field_idx, const double* lat, int H,
                        const double* lon, int W, const double* lat0, const double* lon0, const int* inner, int n_queries,
                        int* found, double* out_lat, double* out_lon, float* out_val, void* stream);

/* ---------------------------------------------------------------------------
 * DC-AE reconstruction evaluation (recon.hip; reference ladcast/evaluate/evaluate_encdec_model.py).  Additive: ABI 5.
 * Preprocessing of a raw batch, weather_dataset_preprocess_batch (dataloader/weather_dataset.py:203-224), in one pass:
 *   out[b][c][h][w] = (x[b*batch_stride + c*channel_stride + h*row_stride + w] - mean[c]) / std_[c], b < B, c < C, h < H, w < W -
 *   a real subtraction and a correctly rounded division, bit-equal to torch.  crop_south_pole is the caller's row offset into x,
 *   incl_sur_pressure=False a C one smaller than the frames hold: no copy.  out is contiguous (B, C, H, W).
 *   In channel sst_channel a NaN result becomes -2 and nan_mask (B, H, W), uint8, records where (1 / 0, every point written);
 *   sst_channel = -1: no channel is treated, nan_mask may be NULL and is not written.  mean / std_: device vectors [C].
 *   16-byte loads and stores when W % 4 == 0 and x, out and the three strides keep 16-byte alignment; a scalar path otherwise. */
int ldc_recon_preprocess(const float* x, long long batch_stride, long long channel_stride, long long row_stride, int B, int C,
                         int H, int W, const float* mean, const float* std_, int sst_channel, float* out,
                         unsigned char* nan_mask, void* stream);
/* Scores of a reconstruction pred (B, Cp, H, W) against target (B, C, H, W) followed by the static channels static_
 * (S planes per batch element, static_batch_stride elements apart - 0 broadcasts one set; S = 0: static_ may be NULL), Cp = C + S,
 * all contiguous fp32.  Replaces process_tensor_for_loss (metric/utils.py:20-63), LpLoss.rel with a weight (metric/loss.py:73-102)
 * and the un-normalise / mse_loss / latitude-weighted mean of evaluate_encdec_model.py:211-231.  With p and t forced to -2 where
 * nan_mask (B, H, W; NULL = none) is set in channel sst_channel, w = lat_weight[h], mean / std_ device vectors [Cp]:
 *   rel[b][c]      = sqrt(sum_hw (w (p - t))^2) / sqrt(sum_hw (w t)^2)     (the weight enters squared; a zero target plane gives
 *                    inf, or NaN when the numerator is zero too - no clamp)
 *   abs_norm[b][c] = the numerator of rel (optional, NULL = not written: LpLoss.abs)
 *   lw_mse[c]      = mean_bhw w ((p std_[c] + mean[c]) - (t std_[c] + mean[c]))^2, every product and sum rounded on its own as
 *                    torch's fp32 ops are (multiply, add, multiply, add, subtract, square, multiply); masked points count as zeros
 * Point values are bit-equal to the reference's; sums are fp32 in a fixed order (two calls: same bits).  B * Cp <= 65535,
 * B * H * W < 2^24 (LDC_ERR_UNSUPPORTED).  workspace: ldc_recon_scores_workspace_bytes(B, Cp, H, W) bytes, 16-byte aligned, no
 * initialisation needed.  16-byte loads when W % 4 == 0 and the bases are aligned; a scalar path otherwise. */
long long ldc_recon_scores_workspace_bytes(int B, int Cp, int H, int W);
int ldc_recon_scores(const float* pred, const float* target, const float* static_, long long static_batch_stride,
                     const unsigned char* nan_mask, const float* lat_weight, const float* mean, const float* std_, int B, int C,
                     int S, int H, int W, int sst_channel, float* rel, float* abs_norm, float* lw_mse, void* workspace,
                     long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Dataset statistics (moments.hip; reference ladcast/preprocecss/compute_mean_std_era5.py, and the latent statistics JSON the
 * reference ships without code).  Additive: ABI 5.
 * Per channel c < C, over all non-NaN values of x[b*batch_stride + c*channel_stride + h*row_stride + w], b < B, h < H, w < W (fp32;
 * strided as in ldc_recon_preprocess: the south-pole crop is the caller's row offset, a dropped channel a smaller C, no copy):
 *   state[c] = { n, mean, M2 } (fp64): the count, the mean and the sum of squared deviations from the mean; the population
 *   variance is M2 / n.  Only NaN is skipped (+-inf is a value like any other and makes the channel's mean and M2 inf / NaN).
 *   accumulate == 0: the state is overwritten, whatever it held.  accumulate != 0: the batch's moments are merged into it by Chan's
 *   pairwise update (a state with n == 0, or n not a positive number, is replaced; a batch without a valid value leaves it alone),
 *   so a dataset streamed in batches of any size gives the statistics of the whole.  A channel that never saw a valid value has
 *   n = 0 and mean = M2 = NaN (numpy's nanmean).
 * All arithmetic is fp64.  A plane is cut into chunks of <= 4096 values, each reduced around its own mean as pivot (corrected two-pass,
 * the values held in registers: one pass over memory); the chunk records (n, mean, M2) go to the workspace and a second launch merges a
 * channel's records in index order, again around their mean, and then into the state.  No float atomics: the same call sequence gives
 * the same bits.  The mean of one call is within about one fp64 ulp of |mean| plus ~2^-48 of the standard deviation, M2 within ~2^-47
 * relative; each accumulate adds up to half an ulp of |mean|.  A constant channel gives M2 = 0 exactly (while n * |value| is exact in
 * fp64: fewer than 2^29 values per call).
 * 16-byte loads when W % 4 == 0 and x and the three strides keep 16-byte alignment; a scalar path otherwise.
 * LDC_ERR_ARG: a null pointer, a non-positive size, row_stride < W, or a workspace smaller than
 * ldc_field_moments_workspace_bytes(B, C, H, W); LDC_ERR_ALIGN: workspace not 16-byte, state not 8-byte or x not 4-byte aligned;
 * LDC_ERR_UNSUPPORTED: more than 2^24 - 1 chunk records, B * C * ceil(H / rows) * ceil(W / 4096) with rows = max(1, 4096 / W) (the
 * grid of the first launch; ldc_field_moments_workspace_bytes returns 0 then).  Nothing is launched or written on an error.
 * workspace: 32 bytes per record, no initialisation needed. */
long long ldc_field_moments_workspace_bytes(int B, int C, int H, int W);
int ldc_field_moments(const float* x, long long batch_stride, long long channel_stride, long long row_stride, int B, int C, int H,
                      int W, double* state, int accumulate, void* workspace, long long workspace_bytes, void* stream);

/* ---------------------------------------------------------------------------
 * Day-of-year climatology from raw frames (climatology.hip; the reference reads a ready-made climatology and has no code that makes
 * one).  Additive: ABI 5.  The table evaluate_ens_gpu reads as --climatology_path: (day of year, hour, channel, row, column).
 *
 * Accumulate.  x[b*batch_stride + c*channel_stride + h*row_stride + w], b < B, c < C, h < H, w < W (fp32; strided as in
 * the field moments above: a row crop is the caller's row offset, a channel block a channel offset and a smaller C, no copy).
 * slots: device int[B]; frame b belongs to slot slots[b]; an entry outside [0, n_slots) skips the frame (nothing of it is read or
 * written).  sum: dense double[n_slots][C][H][W], count: dense int[n_slots][C][H][W], both zero-filled ONCE by the caller before the
 * first call and then only passed on from call to call.  For every non-NaN value (only NaN is skipped; +-inf is a value):
 *   sum[slot][c][h][w] += x (fp64),  count[slot][c][h][w] += 1
 * in frame order b = 0 .. B - 1, one thread per point: two frames of a batch that share a slot add in frame order, and the state
 * after a dataset holds the same bits however its frames were cut into batches.  Elements no valid value falls on are not written.
 * 16-byte loads of x and count and 16-byte read-modify-writes of sum when W % 4 == 0 and x, sum, count and the three strides keep
 * 16-byte alignment; a scalar path otherwise.
 * LDC_ERR_ARG: a null pointer, a non-positive size (B, C, H, W, n_slots) or row_stride < W; LDC_ERR_ALIGN: x, slots or count not
 * 4-byte or sum not 8-byte aligned; LDC_ERR_UNSUPPORTED: C * H above 2^31 - 1, more than 2^31 - 1 workgroups of 256 threads (one
 * thread per 4 points, or per point on the scalar path) or a state of 2^62 elements or more.
 *
 * Smooth.  sum and count viewed as [n_days][n_hours][points], points = C * plane (plane = H * W of the accumulate call, n_slots =
 * n_days * n_hours, slot = day * n_hours + hour); weights: device double[window], window odd, the weight of day offset
 * k - (window - 1) / 2 at index k; out: float[n_days][n_hours][points], every element written:
 *   out[d][h][p] = (sum_k weights[k] sum[(d + k - r) mod n_days][h][p]) / (sum_k weights[k] count[(d + k - r) mod n_days][h][p]),
 *   r = (window - 1) / 2: the weighted mean of all samples in the window, each weighted by its day offset; the day axis is circular,
 *   hours are never mixed.  Both sums run over k = 0 .. window - 1 in order as fp64 fused multiply-adds, the quotient is rounded to
 *   fp64 and then once to fp32.  NaN where the denominator is 0.  window = 1, weights = {1}: the plain mean of each slot.
 * n_empty (optional, NULL = not counted): long long[C], zero-filled by the caller; the kernel ADDS per channel the number of
 * (day, hour, point) outputs whose denominator is 0 (integer atomics, at most one per workgroup and channel).
 * sum, count and weights are only read.  A workgroup stages the whole day column of 32 consecutive points of one hour in LDS
 * (392 bytes per day), so every state element is read from memory once per launch; n_days <= 417 (160 KiB of LDS).
 * LDC_ERR_ARG: a null pointer (n_empty excepted), a non-positive size (n_days, n_hours, C, plane), window < 1, window even or
 * window > n_days; LDC_ERR_ALIGN: sum, weights or n_empty not 8-byte, count or out not 4-byte aligned; LDC_ERR_UNSUPPORTED:
 * n_days > 417, more than 2^31 - 1 workgroups (n_hours * ceil(points / 32)) or a table of 2^62 elements or more.
 *
 * Both: nothing is launched or written on an error.  No float atomics: the same call sequence gives the same bits. */
int ldc_climatology_accumulate(const float* x, long long batch_stride, long long channel_stride, long long row_stride, int B, int C,
                               int H, int W, const int* slots, int n_slots, double* sum, int* count, void* stream);
int ldc_climatology_smooth(const double* sum, const int* count, const double* weights, int window, int n_days, int n_hours, int C,
                           long long plane, float* out, long long* n_empty, void* stream);

/* ---------------------------------------------------------------------------
 * Paired block-bootstrap comparison of two scored runs (bootstrap.hip; no counterpart in the reference).  Additive: ABI 5.
 *
 * a, b: the scores of runs A and B, fp32, N paired initial times by K series, element (i, k) at [i*ld + k], ld >= K (a slice of the
 * series of a wider array is passed without a copy).  draws: device int[R][D], R replicates of D resampled initial times, every
 * value in [0, N) (the caller's contract; a value outside is dropped, never written through).  The resampling scheme is the host's.
 * kind: 0 = mean, theta = S / m;  1 = root mean, theta = sqrt(S / m) (RMSE from per-time MSE).  tail_ppm: the tail probability of
 * the interval on each side in parts per million (25000: a 95 % interval), 0 <= tail_ppm < 500000.
 *
 * Per series k.  Pair i is valid when a[i,k] and b[i,k] are both finite; invalid pairs are skipped everywhere.
 *   n_valid = the valid pairs;  a_hat, b_hat = theta over them;  diff_hat = b_hat - a_hat;  ratio_hat = b_hat / a_hat.
 *   Replicate r: SA_r, SB_r = the fp64 sums over its valid draws, m_r their number; m_r == 0: the replicate is unused.  Otherwise
 *   a*_r, b*_r = theta of the sums, d*_r = b*_r - a*_r, q*_r = b*_r / a*_r.
 *   n_used = the replicates with m_r > 0 and finite d*_r;  n_le0 / n_ge0 = those of them with d* <= 0 / d* >= 0.
 *   Interval of diff: the n_used finite d* sorted ascending, lo = (tail_ppm * n_used) / 1000000 (64-bit integer division),
 *   hi = n_used - 1 - lo, diff_lo = sorted[lo], diff_hi = sorted[hi]; no interpolation.  Interval of ratio: the same over the finite
 *   q*, with their own count.  (The order is that of the values, -0 before +0.)
 *   stats[k] = { a_hat, b_hat, diff_hat, ratio_hat, diff_lo, diff_hi, ratio_lo, ratio_hi } (double[K][8]);
 *   counts[k] = { n_valid, n_used, n_le0, n_ge0 } (int[K][4]).  n_valid == 0: the four estimates are NaN; no finite d* (q*): the
 *   interval of diff (ratio) is NaN.  ratio_hat is the quotient as it comes (a_hat == 0: +-inf or NaN).
 * Sums are fp64 in any order (a multiplicity times an fp32 value is exact): each within D * 2^-53 * sum |terms| of the exact sum;
 * division and square root are correctly rounded.  No float atomics: the same inputs give the same bits.
 *
 * Three launches behind a memset: draws -> multiplicities W[r][i]; the replicate sums as the tiled product W . (a, b, valid) with fp64
 * FMA, written series-major; one workgroup per series forms d* / q*, sorts them in LDS and reads the ranks.
 * R <= ldc_paired_bootstrap_max_replicates() = 16384 (the keys of a series fill 128 KiB of LDS).
 * workspace: ldc_paired_bootstrap_workspace_bytes(N, K, R, D) bytes (0: the sizes are not served), 16-byte aligned, no initialisation:
 *   4 N RS rounded up to 256, plus 20 K RS, RS = R + 1 rounded up to 4.
 * LDC_ERR_ARG: a null pointer, a non-positive size, ld < K, kind outside {0, 1}, tail_ppm outside [0, 500000) or a workspace that is
 * too small; LDC_ERR_UNSUPPORTED: R above the cap, or more than 2^31 - 1 workgroups of 256 draws (R * D); LDC_ERR_ALIGN: a, b, draws or counts not 4-byte, stats
 * not 8-byte or workspace not 16-byte aligned.  Nothing is launched or written on an error. */
int ldc_paired_bootstrap_max_replicates(void);
long long ldc_paired_bootstrap_workspace_bytes(int N, int K, int R, int D);
int ldc_paired_bootstrap(const float* a, const float* b, long long ld, int N, int K, const int* draws, int R, int D, int kind,
                         int tail_ppm, double* stats, int* counts, void* workspace, long long workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* LADCAST_HIP_H */
