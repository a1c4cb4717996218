/* libmintime_hip.so -- C ABI of the MI355X-native MINTIME hot path.
 *
 * The reference (davide-coccomini/MINTIME...) is pure Python on PyTorch and has NO FFI / plugin layer
 * (SURVEY.md §8b); its "operator API" for this path is the nn.Module surface
 *   models/efficientnet/efficientnet_pytorch/model.py:267  EfficientNet.forward
 *   models/size_invariant_timesformer.py:224               SizeInvariantTimeSformer.forward
 * and the tensor ops those call.  Each entry point below replaces the group of reference ops cited
 * next to it.  The Python host (package dir `mintime-..._amd/`) binds these with ctypes; a reference
 * maintainer would bind them the same way.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (fp32 unless stated; masks uint8; indices int32/int64)
 *   - every function enqueues on `stream` (a hipStream_t passed as void*), never synchronises,
 *     never allocates; scratch comes from the caller
 *   - return 0 on success, negative on error; mt_last_error() gives a thread-local message
 *   - re-entrant: launches go to the caller's stream on the current device; the only process-wide state are two switches
 *     (mt_gemm_set_split, mt_set_deterministic; since 122 also the arithmetic tier, mt_gemm_set_precision) and, with the latter on, the per-stream workspace described there
 */
#ifndef MINTIME_HIP_H
#define MINTIME_HIP_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define MT_VERSION 123

int mt_version(void);
const char* mt_last_error(void);

/* ------------------------------------------------------------------------------------------------
 * Deterministic mode (reference train.py:110 `cudnn.deterministic = True`).  Off by default (MT_DETERMINISTIC=1 in the environment
 * turns it on at load time).  With the switch on no floating-point atomic is issued anywhere in the training step: partial sums go
 * through logs / split-K slabs in a per-stream workspace OWNED BY THE LIBRARY (the one exception to "never allocates": grown with
 * hipMalloc on first use, which may synchronise) and are added in a fixed order, so the same inputs and state give bit-identical
 * gradients run after run.  Slower (the bench line's `deterministic` leg has the cost).  Returns 0 / the current setting.
 * mt_det_bn_sums: BatchNorm sums in fixed order from a stored tensor x [rows][C] into stats[0 .. 2C) (fp64, +=): mode 0 = sum x,
 * sum x^2 (forward batch statistics); mode 1 = sum x, sum x * (z - mean) * invstd (backward; mean_invstd = [2][C]).  The engines call
 * it instead of the producers' fused statistics when the switch is on (round 4's engines; kept as an entry point, no longer on the path).
 * BatchNorm statistics without the second pass (EfficientNet since version 115): every entry point that takes a BatchNorm accumulator
 * (`double* stats, int slots`, or `stats` / `stats_slots` of a GEMM descriptor) accepts a NEGATIVE slot count: |slots| accumulators,
 * each held as two 64-bit INTEGER limbs |slots| * 2 * C doubles apart (stats must hold 2 * |slots| * 2 * C zeroed doubles): a block's
 * fp32 partial v adds trunc(v) to limb 0 and round((v - trunc(v)) * 2^44) to limb 1 with integer atomics.  Integer addition is
 * associative, so the sums are the same bits whatever order the blocks arrive in; mt_bn_finalize / mt_bn_bwd_finalize decode the limbs
 * when given the same negative count.
 */
int mt_set_deterministic(int on);
int mt_get_deterministic(void);
/* Frees the deterministic mode's workspaces of `stream` on the current device (synchronises that stream): call before destroying a
 * stream that ran deterministic launches.  The workspaces never grow under stream capture (the entry point fails instead). */
int mt_det_release(void* stream);
int mt_det_bn_sums(const float* x, const float* z, const float* mean_invstd, int64_t rows, int C, int mode, double* stats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Dense contraction family (fp32 MFMA).  Replaces every nn.Linear / 1x1 Conv2d / their autograd:
 *   size_invariant_timesformer.py:111,144 (to_qkv, to_out), :69-74 (FeedForward), :228 (to_patch_embedding)
 *   efficientnet_pytorch/model.py:98,116,286 (_expand_conv, _project_conv, _conv_head)
 * ------------------------------------------------------------------------------------------------ */
typedef struct { int gin, gout, off; } mt_rowmap;   /* row' = (r/gin)*gout + off + r%gin ; gin==0: identity */

enum { MT_OP_NT = 0,    /* C[M,N] = A[M,K] * B[N,K]^T      forward (torch weight layout)             */
       MT_OP_NN = 1,    /* C[M,N] = A[M,K] * B[K,N]        dgrad                                      */
       MT_OP_TN = 2 };  /* C[M,N] = A[K,M]^T * B[K,N]      wgrad (split-K + fp32 atomics, C pre-zeroed) */

enum { MT_PRO_NONE = 0, MT_PRO_BN_SWISH_GATE = 1, MT_PRO_BN_SWISH = 2, MT_PRO_AFFINE = 3,
       MT_PRO_BN_BWD = 4,
       MT_PRO_IM2COL = 5 };  /* A := act(affine(x[n, oh*s+kh-p, ow*s+kw-p, ci])) gathered from an NHWC image (conv_* fields):
                                dense k x k / strided 1x1 convolution as a GEMM with M = N*Ho*Wo, K = k*k*C (padded to %4) */  /* A := ka[c]*A + kb[c]*A2 + kc[c]  (BatchNorm backward folded into the load; ka,kb,kc = scale,shift,gate) */
enum { MT_BPRO_NONE = 0, MT_BPRO_BN_SWISH_GATE = 1, MT_BPRO_IM2COL = 2 };  /* TN only: B := swish(B*b_scale[n]+b_shift[n]) * b_gate[(k/b_hw)*N+n] */
enum { MT_EPI_STORE = 0, MT_EPI_BIAS_RES = 1, MT_EPI_GEGLU = 2, MT_EPI_STATS = 3, MT_EPI_ATOMIC = 4,
       MT_EPI_GEGLU_BWD = 5, MT_EPI_ACCUM = 6,
       /* MBConv backward around the squeeze-excite stage (autograd of efficientnet_pytorch/model.py:108-117), NN + BN_BWD only.
          The GEMM result da = dz_p . W_project is consumed in the accumulators and never stored; C2 = the depthwise conv's raw
          output z_d [M,N], u = z_d*e_scale[n] + e_shift[n], img = m / e_hw:
            SE_RED:  C[img,n] += sum_rows da * swish(u)                    (d gate, fp32 atomics, C [M/e_hw, N] zero-filled)
            ACT_BWD: C[m,n] = (da*e_gate[img,n] + e_dpool[img,n]/e_hw) * swish'(u)   and the BatchNorm-backward sums of it:
                     stats[..][0][n] += C, stats[..][1][n] += C * (z_d - e_mi[n]) * e_mi[N+n]                              */
       MT_EPI_SE_RED = 7, MT_EPI_ACT_BWD = 8 };

typedef struct {
  int op, prologue, epilogue;
  const float* A; const float* B; float* C;
  int M, N, K;                      /* GEGLU: N = full width of the weight (2*n_half)                   */
  int64_t lda, ldb, ldc;
  mt_rowmap a_map, b_map, c_map;
  const float* bias;
  const float* R; int64_t ldr;      /* residual (BIAS_RES)                                               */
  const float* scale; const float* shift; const float* gate; int hw;   /* prologue vectors               */
  float* C2; int64_t ldc2;          /* GEGLU: optional pre-activation store, row = (a_0,g_0,a_1,g_1,...) -- private
                                       to the GEGLU / GEGLU_BWD pair; GEGLU_BWD: those pre-activations (ldc2 even)        */
  double* stats; int stats_slots;   /* STATS: [slots][2][N] fp64 accumulators (sum, sum of squares)      */
  int n_half;
  int split_k;                      /* TN: number of K splits; <= 0 picks one that fills the chip        */
  const float* A2;                  /* BN_BWD prologue: second source, same layout as A                  */
  int b_prologue; const float* b_scale; const float* b_shift; const float* b_gate; int b_hw;
  /* im2col prologues: the gathered operand (A of NT with MT_PRO_IM2COL and STORE / STATS; B of TN with MT_BPRO_IM2COL, BN_BWD on A
     and ATOMIC) is a dense NHWC image [n][conv_H][conv_W][conv_C] without a leading dimension.  Its virtual matrix has one row per
     output pixel (n, oh, ow), oh < conv_Ho, ow < conv_Wo (taken as given: a window may hang over the bottom / right edge), and one
     column per (kh, kw, ci); it is exactly zero where the tap lies outside the image (the padding passes through neither the affine
     scale / shift, resp. b_scale / b_shift, nor the activation) and in the columns from k*k*C up to the contraction width (K of NT,
     N of TN), which must be at least k*k*C.  conv_pad is the one leading pad of both axes; conv_act: 0 none, 2 relu. */
  int conv_H, conv_W, conv_C, conv_Ho, conv_Wo, conv_k, conv_stride, conv_pad, conv_act;
  int conv_src_u8;                  /* im2col source image is uint8 (raw crops, conv_C % 4 != 0) instead of fp32  */
  float* col_sum;                   /* GEGLU_BWD: optional [2*n_half] column sums of the stored gradient (= d bias of the
                                       Linear that produced the pre-activations), atomically accumulated; caller zero-fills */
  const void* b_planes;             /* NT only, optional: B pre-split by mt_split_planes (three bf16 planes, each [N][K] with B's
                                       ldb).  The split-operand loop then streams B by DMA instead of splitting it per tile;
                                       every other path ignores the field and reads B.  B must still be valid.             */
  int64_t b_plane_stride;           /* elements between planes */
  const float* e_scale; const float* e_shift;   /* SE_RED / ACT_BWD: BatchNorm affine of z_d [N]                            */
  const float* e_gate; const float* e_dpool;    /* ACT_BWD: squeeze-excite gate and pooled-gradient rows [M/e_hw, N]         */
  const float* e_mi; int e_hw;                  /* ACT_BWD: mean | invstd [2][N]; rows per image                             */
} mt_gemm_desc;

int mt_gemm(const mt_gemm_desc* d, void* stream);

/* Matrix pipe of the prologue-free contractions (the TimeSformer's Linear layers and their gradients).
 *   1 (default; MT_GEMM_SPLIT=0 in the environment starts at 0): split-operand fp32 -- every fp32 operand value is split exactly
 *     into three bf16 pieces and the six leading piece products are accumulated in fp32 on v_mfma_f32_32x32x16_bf16
 *     (csrc/gemm_split.hpp); error against fp64 equal to the fp32 MFMA pipe's (tests/test_gpu_gemm.py), 6/16 of its matrix time.
 *   0: v_mfma_f32_32x32x2_f32 everywhere.
 * Process-wide; returns the previous setting.  Inputs, outputs and accumulators are fp32 either way. */
int mt_gemm_set_split(int on);
int mt_gemm_get_split(void);

/* Arithmetic tier of the bf16-pipe contractions: everything on mt_gemm_planes and the split-operand loop of mt_gemm.
 *   MT_PRECISION_HIGHEST (default): the six leading piece products of the three-piece split, fp32-level error.
 *   MT_PRECISION_HIGH: the three products a0 b0 + a0 b1 + a1 b0 of the first two pieces of the SAME split (the "bf16x3" of
 *     torch.set_float32_matmul_precision("high"); gfx950 has no TF32).  About 16 mantissa bits per operand:
 *     |error| <= 3.1 * 2^-16 * sum|a||b| plus the fp32 accumulation error.  Half the matrix instructions; the plane loop reads two of
 *     an operand's three planes (producers still write all three: one plane tensor serves both tiers).
 * Accumulators, layouts, epilogues, the balanced accumulators and deterministic mode are the same at both tiers.  With
 * mt_gemm_set_split(0) the tier has no effect on mt_gemm: the fp32 pipe is exact (mt_gemm_planes has no fp32-pipe form and follows
 * the tier).  Not covered (fp32 MFMA at either tier): the attention cores, contractions with K < 512 or an operand prologue the split
 * loop does not take, the depthwise / squeeze-excite / stem kernels and the 3-D convolutions.
 * Process-wide and read when a call is DISPATCHED: a recorded launch plan replays at the tier current at replay.
 * mt_gemm_set_precision returns the previous level; an unknown level returns MT_ERR_ARG = -1 (mt_last_error() says why) and changes
 * nothing.  MT_MATMUL_PRECISION=highest|high in the environment sets the initial level; any other value keeps highest and is
 * reported through mt_last_error() by the first mt_gemm_get_precision(). */
#define MT_PRECISION_HIGHEST 0
#define MT_PRECISION_HIGH 1
int mt_gemm_set_precision(int level);
int mt_gemm_get_precision(void);

/* planes[p][i], p = 0..2: the exact three-piece bf16 split of src[i] (x = x0 + x1 + x2, round-to-nearest at each level) that the
 * split-operand loop computes on the fly -- done once for operands that many launches share (weights: once per optimizer step).
 * planes: 3 * n bf16 values, 16-byte aligned; plane stride n. */
int mt_split_planes(const float* src, void* planes, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Plane-operand contractions (csrc/gemm_planes.hpp): the TimeSformer's Linear layers and their gradients
 * (size_invariant_timesformer.py:60-76, 111, 144 and their autograd) with BOTH operands pre-split.
 *
 * A "plane tensor" of an fp32 matrix X [rows][cols] is its exact three-piece bf16 split X = P0 + P1 + P2 (round-to-nearest at each
 * level -- the pieces mt_gemm's split-operand loop computes on the fly) stored as
 *     planes[3][Rp/32][Cp/16][32][16] bf16,   Rp = rows rounded up to 32, Cp = cols rounded up to 16, padding = zeros,
 * i.e. 1 KB blocks of 32 rows x 16 columns; mt_planes_elems(rows, cols) = Rp * Cp is the plane stride in elements.  The producer
 * of a tensor writes its planes once (mt_layernorm_fwd / mt_layernorm_bwd_rows / mt_attn_fwd / mt_attn_bwd / the GEGLU epilogues
 * below / mt_split_planes_blk); forward, data-gradient and weight-gradient GEMMs all read the same planes by LDS-DMA, the first
 * along the columns, the other two along the rows (LDS transpose-reads).  fp32 in, fp32 out, fp32 accumulation:
 * NT / NN results are bit-identical to mt_gemm's split-operand loop on the same fp32 operands.
 * ------------------------------------------------------------------------------------------------ */
int64_t mt_planes_elems(int rows, int cols);

/* planes of src [rows][cols] (row-major, leading dimension ld). */
int mt_split_planes_blk(const float* src, int64_t ld, int rows, int cols, void* planes, void* stream);

/* Many contiguous matrices in one launch (the Linear weights, once per optimizer step).  items: device array of
 * { const float* src; void* planes; int64_t rows, cols, first; } with first = running sum of (Rp/32)*(Cp/16) over the items before;
 * total_blocks = that sum over all items. */
int mt_split_planes_blk_multi(const void* items, int count, int64_t total_blocks, void* stream);

/* planes of dz = ka * du + kb * z + kc  (du, z [rows][C] fp32, kabc = [3][C]: the BatchNorm-backward affine of mt_bn_bwd_finalize):
 * the operand a 1x1 convolution's data- AND weight-gradient GEMMs share, written once (Xception's pointwise convolutions,
 * reference models/xception.py:17-27 under autograd). */
int mt_bn_bwd_apply_planes(const float* du, const float* z, const float* kabc, void* planes, int rows, int C, void* stream);

typedef struct {
  int op;                           /* MT_OP_NT: C = A[M,K] B[N,K]^T ; MT_OP_NN: C = A[M,K] B[K,N] ; MT_OP_TN: C += A[K,M]^T B[K,N]        */
  int epilogue;                     /* NT: STORE, BIAS_RES, GEGLU, STATS ; NN: STORE, GEGLU_BWD ; TN: ATOMIC (C pre-zeroed, split-K)       */
  int M, N, K;                      /* GEGLU: N = 2 * n_half ; GEGLU_BWD: N = n_half                                                       */
  const void* a_planes;             /* plane tensor of A as stored ([M][K], TN: [K][M])                                                    */
  const void* b_planes;             /* plane tensor of B as stored (NT: [N][K], NN / TN: [K][N])                                           */
  float* C; int64_t ldc;            /* fp32 result (may be NULL for the GEGLU pair when c_planes is given)                                 */
  const float* bias;
  const float* R; int64_t ldr;      /* BIAS_RES residual                                                                                   */
  float* C2; int64_t ldc2;          /* GEGLU: optional pre-activation store (a_0,g_0,a_1,g_1,...); GEGLU_BWD: those pre-activations        */
  int n_half;
  float* col_sum;                   /* GEGLU_BWD: optional [2*n_half] column sums of the gradient (bias gradient), caller zero-fills       */
  void* c_planes;                   /* GEGLU: plane tensor of h [M][n_half]; GEGLU_BWD: of du [M][2*n_half]; NULL: fp32 output only        */
  int split_k;                      /* TN: number of K ranges; <= 0 picks one                                                               */
  void* sk_workspace;               /* NT / NN, optional: mt_gemm_planes_workspace_bytes() of device memory, 256-byte aligned, ZERO-FILLED   */
  int64_t sk_workspace_bytes;       /* once by the caller and lent to every launch of ONE stream (launches leave it zero-filled again).    */
                                    /* With it the launch runs stream-K: a persistent grid shares the (tile, k-step) list evenly instead of */
                                    /* one block per tile -- same result up to the association of a split tile's partial sums, which is     */
                                    /* fixed (bit-reproducible run to run).  NULL: one block per output tile.                               */
  double* stats; int stats_slots;   /* NT + MT_EPI_STATS (a 1x1 convolution with train-mode BatchNorm): column sums and sums of squares     */
                                    /* of the stored result into [slots][2][N] fp64 accumulators, like mt_gemm                              */
} mt_gemm_planes_desc;

/* Limit: an operand's three planes (padded rows x padded columns x 6 bytes) must stay under 4 GB -- the loop reaches them by 32-bit
 * byte offsets from one base -- or the call returns MT_ERR_UNSUPPORTED (before round 6's end it wrapped silently).                      */
int mt_gemm_planes(const mt_gemm_planes_desc* d, void* stream);

/* nn.Dropout inside the TimeSformer (size_invariant_timesformer.py:66-70 between GEGLU and net.3, :98-101 behind to_out.0), train mode
 * with attn-dropout / ff-dropout > 0 (the shipped YAML uses 0: these passes run only then).  m = keep / (1 - p), an fp32 tensor the
 * caller draws.  mt_mul_planes: planes of x * m ([rows][cols]; optionally the fp32 product too); mt_mul_add: out = r + y * m;
 * mt_geglu_bwd: du = [dh m gelu(g) | dh m a gelu'(g)] from the forward's interleaved pre-activations u = (a_0, g_0, a_1, g_1, ...),
 * as planes [rows][2 n_half] and optionally fp32 (m may be NULL). */
int mt_mul_planes(const float* x, const float* m, void* planes, float* out, int rows, int cols, void* stream);
int mt_mul_add(const float* y, const float* m, const float* r, float* out, int64_t n, void* stream);
int mt_geglu_bwd(const float* dh, const float* m, const float* u, void* du_planes, float* du, int rows, int n_half, void* stream);
int64_t mt_gemm_planes_workspace_bytes(void);
/* Persistent form of the fp32-output NT / NN plane GEMMs (MT_EPI_STORE, MT_EPI_BIAS_RES) with more tiles than resident block slots:
 * blocks_per_cu resident blocks per CU walk their XCD's share of the tile list and issue the next tile's first DMA stage before the
 * current tile's epilogue.  Same sums in the same order (bit-identical results).  0 = one block per tile (default; MT_PLANES_PERSIST
 * sets the initial value).  Process-wide like mt_gemm_set_split; returns the previous setting. */
int mt_gemm_planes_set_persist(int blocks_per_cu);

/* ------------------------------------------------------------------------------------------------
 * Size-Invariant TimeSformer forward, non-GEMM pieces
 * ------------------------------------------------------------------------------------------------ */

/* nn.LayerNorm over the last dim (size_invariant_timesformer.py:18-26).  stats (optional) [rows,2] = mean, rstd.
 * y (fp32) and / or y_planes (plane tensor of y [rows][dim], dim % 16 == 0; see mt_gemm_planes) -- at least one. */
int mt_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* stats,
                     int rows, int dim, float eps, void* y_planes, void* stream);

/* cls token + positional + size embeddings (:231-248), in place on x [B, 1+F*n, dim] whose rows 1.. hold the
 * patch-embedding output.  positions int64 [B,1+F*n] (NULL: the token index); sizes int32 [B,F] (NULL size_emb: enable-size-emb False -- sizes is then not read,
 * whatever it holds). */
int mt_embed_fwd(float* x, const float* cls, const float* pos_emb, const float* size_emb,
                 const int64_t* positions, const int32_t* sizes, int B, int F, int n, int dim, int pos_rows, int size_rows,
                 int* err_flag, void* stream);
/* pos_rows / size_rows = rows of the two tables.  nn.Embedding raises on an out-of-range index; here such an index is clamped
 * into the table (no out-of-bounds access, forward or backward) and *err_flag (optional, device int32, sticky) gets bit 0
 * (positions) / bit 1 (size_embedding) set, which the host checks at its next synchronisation point. */

/* Divided attention core (:80-87 attn(), :112-141 of Attention.forward) on the QKV GEMM output
 * qkv [B, 1+F*n, 3*H*64] -> out [B, 1+F*n, H*64] (merged heads).  mode 0 = time (identity-masked), 1 = space,
 * 2 = the cls query only (out row 0 of each clip; what the LAST layer's space attention needs when only the cls token is read
 * afterwards -- the optional dead-row pruning of tsf_engine.py; mt_attn_bwd mode 2 is its adjoint: dk / dv of all keys, dq of row 0).
 * mask uint8 [B,F], ident uint8 [B,F,F]; cls_att (optional) [(B*H), 1+F*n] = the cls query's probabilities.
 * out_planes (optional, mode 0 / 1): plane tensor of out [B*(1+F*n)][H*64] (mt_gemm_planes), written by the same kernels -- the
 * operand of the out-projection and of its weight gradient; out may then be NULL.
 * n (patches per frame) = 1 .. 100: cls + n <= 64 keys run the 2 x 2-tile space kernels, 64 <= n <= 100 the query-walking ones;
 * any other n returns MT_ERR_UNSUPPORTED before anything is launched (no output is written). */
int mt_attn_fwd(const float* qkv, float* out, float* cls_att, const uint8_t* mask, const uint8_t* ident,
                int B, int H, int F, int n, int mode, float scale, void* out_planes, void* stream);

/* to_out: LayerNorm + Linear(dim, classes) on the cls row x[:,0] (:270-276). x [B,N,dim] -> logits [B,classes]. */
int mt_head_fwd(const float* x, const float* gamma, const float* beta, const float* w, const float* bias,
                float* logits, int B, int N, int dim, int classes, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EfficientNet-B0 forward, everything except the 1x1 convolutions (those are mt_gemm on NHWC rows).
 * Activations are NHWC fp32.  Tensors between kernels hold the RAW conv output z; consumers apply
 * swish(z*scale[c]+shift[c]) on load.  `stats` = [slots][2][C] fp64 accumulators (sum, sum of squares),
 * zeroed by the caller; pass NULL when batch statistics are not needed (eval).
 * ------------------------------------------------------------------------------------------------ */

/* _conv_stem: 3x3 stride-2 TF-SAME conv 3->32 (model.py:173,276; utils.py:248-276) + the BatchNorm batch statistics of its output
 * (stats [slots][2][32] fp64, accumulated; NULL = none).  x [N,H,W,3] fp32 or (x_is_u8) uint8 -> z [N,ceil(H/2),ceil(W/2),32];
 * w in torch layout [32,3,3,3]; W <= 512.  Streaming MFMA kernel (stem_fwd.hip): one output row per block and pass. */
int mt_stem_conv_fwd(const void* x, int x_is_u8, const float* w, float* z, double* stats, int slots, int N, int H, int W,
                     void* stream);
/* The same kernel without padding (Conv2d(3, 32, 3, 2, 0): Xception's conv1, xception.py:135): z [N,(H-3)/2+1,(W-3)/2+1,32]. */
int mt_stem_conv_fwd_valid(const void* x, int x_is_u8, const float* w, float* z, double* stats, int slots, int N, int H, int W,
                           void* stream);

/* Depthwise conv (k 3|5, stride 1|2, TF-SAME padding; for k3 s1 that is pad 1) applied to act(zin*scale+shift);
 * act 1 = swish: EfficientNet _depthwise_conv on swish(bn(z)) (model.py:98-103);
 * act 2 = relu / 0 = none: Xception SeparableConv2d.conv1 (xception.py:21,25).  w torch layout [C,1,k,k]. */
int mt_dwconv_fwd(const float* zin, const float* scale, const float* shift, const float* w, float* zout,
                  double* stats, int slots, int N, int H, int W, int C, int k, int stride, int act, void* stream);
/* The same convolution with the output written as a plane tensor ([N*Ho*Wo rows][C columns], mt_planes_elems; padding zeroed) and
 * nowhere else: Xception's SeparableConv2d (xception.py:17-27) feeds its depthwise output to the pointwise convolution only, which
 * runs on mt_gemm_planes -- the fp32 tensor and the mt_split_planes_blk pass over it are not needed. */
int mt_dwconv_fwd_planes(const float* zin, const float* scale, const float* shift, const float* w, void* planes, int N, int H,
                         int W, int C, int k, int stride, int act, void* stream);

/* nn.BatchNorm2d bookkeeping (model.py:51-52,62,72,86,174,202): training!=0 -> batch statistics from `stats`
 * (count = N*H*W), running-stat update with `momentum` (unbiased variance); else running statistics.
 * Emits scale = gamma*invstd, shift = beta - mean*scale, and mean_invstd [2][C] (optional, for backward). */
int mt_bn_finalize(const double* stats, int slots, double count, const float* gamma, const float* beta,
                   float* running_mean, float* running_var, float* scale, float* shift, float* mean_invstd,
                   int C, float eps, float momentum, int training, void* stream);

/* squeeze: mean_hw swish(bn(z)) (model.py:104-108), computed as `parts` pixel slices per image so that small batches still
 * fill the chip: partial[n, part, c] (already divided by HW); parts = mt_se_pool_parts(N, HW, C).  No atomics. */
int mt_se_pool_parts(int N, int HW, int C);
int mt_se_pool_fwd(const float* z, const float* scale, const float* shift, float* partial, int N, int HW, int C, int parts,
                   void* stream);

/* excite: pooled = sum of the slices (written to `pooled` [N,C] when not NULL: kept for backward);
 * gate = sigmoid(_se_expand(swish(_se_reduce(pooled)))) (model.py:109-112). w1 [CS,C], w2 [C,CS];
 * hidden [N,CS] (required: the hand-over between the kernel pair) receives the pre-activation of the squeeze layer, which backward keeps.
 * CS = 1 .. 48 like mt_se_bwd (any other width: MT_ERR_UNSUPPORTED before anything is launched). */
int mt_se_gate_fwd(const float* partial, int parts, const float* w1, const float* b1, const float* w2, const float* b2,
                   float* pooled, float* gate, float* hidden, int N, int C, int CS, void* stream);

/* y = act(z*scale+shift) * rowscale[row / rows_per_group] (+ res): _bn2 + drop_connect + identity skip
 * (model.py:117-127, utils.py:129-154; act=0) and head _bn1+swish (model.py:286; act=1). rowscale may be NULL. */
int mt_bn_act_fwd(const float* z, const float* scale, const float* shift, const float* res, float* y,
                  int64_t rows, int C, int act, const float* rowscale, int rows_per_group, void* stream);

/* Attention explainability post-process (utils.py:68-96 aggregate_attentions): out [3][F] = softmax over frame chunks of
 * scale_factor * mean over the chunk's tokens of max over (batch*heads) of the cls attention; rows space / time / combined.
 * space_att, time_att: [(B*H), N] as returned by mt_attn_fwd's cls_att. */
int mt_attn_aggregate(const float* space_att, const float* time_att, float* out, int BH, int N, int F,
                      float scale_factor, void* stream);

/* Input-sequence builder (next-row f1): the side inputs of SizeInvariantTimeSformer.forward for a batch of clips, built in HBM
 * from the compact description a loader produces.  Replaces the list-building code of deepfakes_dataset.py:259-287 (size
 * buckets via SIZE_EMB_DICT :30-31, padded slots), :315-321 (identities_mask), :324-329 (temporal positions) and
 * predict.py:285-309,335-347.  Inputs (device, int32): slots[B][max_identities] = slots per identity in slot order (0 = unused),
 * valid[B][max_identities] = faces actually present (<= slots; the rest of the identity's slots are padding), frames[B][F] =
 * video-frame number per slot (ignored at padded slots: they take the largest frame number seen so far, :271-275),
 * ratio[B][F] = int(face_area*100/video_area) per slot (0..100).  Outputs: mask [B][F] u8, identities_mask [B][F][F] u8,
 * size_embedding [B][F] int32 (bucket 1..20, 0 = padding), positions [B][1+F*num_patches] int64.
 * mask_mode 0 = the dataset's behaviour (mask all ones: its padding test at :281 runs after the list was already extended),
 * mask_mode 1 = predict.py:304 (padded slots masked out). */
int mt_build_clip_inputs(const int* slots, const int* valid, const int* frames, const int* ratio, unsigned char* mask,
                         unsigned char* identities_mask, int* size_embedding, int64_t* positions, int B, int F,
                         int num_patches, int max_identities, int mask_mode, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Size-Invariant TimeSformer backward, non-GEMM pieces.  The reference derives these through torch autograd
 * from the same source lines as the forward entry points; here they are explicit adjoint kernels.
 * ------------------------------------------------------------------------------------------------ */

/* LayerNorm adjoint. dx (+)= LN'(dy) (accumulate!=0 adds into dx: the residual stream's gradient);
 * dgamma/dbeta are accumulated atomically (caller zero-fills). stats = [rows,2] mean,rstd saved by the forward.
 * dx_colsum (optional, [dim], atomically accumulated): column sums of the UPDATED dx rows -- the bias gradient of the Linear
 * whose output gradient dx is next (to_out.0.bias / net.3.bias / to_patch_embedding.bias), which the reference gets from
 * autograd's sum over rows; rows with row % skip_period == 0 are left out when skip_period > 0 (the cls rows, which the patch
 * embedding does not produce, :231-232).
 * dx_in (optional): with accumulate != 0 the sum is dx = LN'(dy) + dx_in instead of in place (NULL = dx itself), so that the
 * previous value of the residual-stream gradient stays readable (deferred weight gradients, tsf_backward.py). */
int mt_layernorm_bwd(const float* dy, const float* x, const float* stats, const float* gamma, float* dx,
                     float* dgamma, float* dbeta, int rows, int dim, int accumulate, float* dx_colsum, int skip_period,
                     const float* dx_in, void* stream);
/* The same LayerNorm backward split by queue: mt_layernorm_bwd_rows writes only dx = LN'(dy) + dx_in (few registers, no LDS: it
 * co-resides with the weight-gradient GEMMs instead of waiting for their blocks to end) and mt_layernorm_bwd_cols accumulates the
 * parameter gradients (dgamma, dbeta, and dx_colsum = column sums of dx_new, rows with r % skip_period == 0 left out when
 * skip_period > 0) -- meant for the weight-gradient stream. */
int mt_layernorm_bwd_rows(const float* dy, const float* x, const float* stats, const float* gamma, float* dx, const float* dx_in,
                          int rows, int dim, void* dx_planes, void* stream);   /* dx_planes (optional): plane tensor of the new dx */
int mt_layernorm_bwd_cols(const float* dy, const float* x, const float* stats, const float* dx_new, float* dgamma, float* dbeta,
                          float* dx_colsum, int skip_period, int rows, int dim, void* stream);

/* (autograd of PreNorm's nn.LayerNorm, size_invariant_timesformer.py:18-26, as above.)  The rows kernel with the parameter-gradient
 * sums folded in: besides dx (and its planes) every block stores one row of
 * partials[blocks][3][dim] = its rows' column sums of dy * xhat, dy and dx_new (rows with r % skip_period == 0 left out of the
 * third when skip_period > 0); blocks = mt_layernorm_bwd_rows_blocks(rows).  mt_layernorm_bwd_cols_reduce adds the block rows,
 * in block order (a fixed summation order: deterministic as it is), into dgamma, dbeta and dx_colsum (NULL = skipped) -- 6 MB read at
 * B = 32 instead of the 75 MB mt_layernorm_bwd_cols re-reads.  dim <= 512. */
int mt_layernorm_bwd_rows_blocks(int rows);
int mt_layernorm_bwd_rows_sums(const float* dy, const float* x, const float* stats, const float* gamma, float* dx, const float* dx_in,
                               int rows, int dim, void* dx_planes, float* partials, int skip_period, void* stream);
int mt_layernorm_bwd_cols_reduce(const float* partials, int blocks, int dim, float* dgamma, float* dbeta, float* dx_colsum,
                                 void* stream);
/* mt_layernorm_bwd_rows_sums with a SPARSE residual gradient: dx_res [rows / period][dim] belongs to the rows r % period == 0
 * (row r takes dx_res[r / period]); every other row takes none, dx = LN'(dy).  Same dx, dx_planes and partials as the dense form fed
 * a [rows][dim] tensor that is zero off those rows.  The last layer with its dead rows pruned: the head reads x[:, 0] only (:270-276),
 * so below that layer's space attention the residual stream's gradient lives on the cls rows (period = 1 + F*n) alone.
 * rows % period == 0, dim <= 512; anything else returns an error before anything is launched. */
int mt_layernorm_bwd_rows_sums_sparse(const float* dy, const float* x, const float* stats, const float* gamma, float* dx,
                                      const float* dx_res, int period, int rows, int dim, void* dx_planes, float* partials,
                                      int skip_period, void* stream);

/* out[n] += sum_m A[map(m)*lda + n]   (bias gradients). */
int mt_colsum(const float* A, int64_t lda, mt_rowmap map, int M, int N, float* out, void* stream);

/* adjoint of mt_head_fwd; writes dx[:,0,:] (dx must be zero elsewhere), accumulates the four parameter grads. */
int mt_head_bwd(const float* dlogits, const float* x, const float* gamma, const float* beta, const float* w,
                float* dx, float* dgamma, float* dbeta, float* dw, float* dbias, int B, int N, int dim, int classes,
                float eps, void* stream);

/* adjoint of mt_embed_fwd: scatter-adds into dcls [dim], dpos_emb, dsize_emb (zero-filled by the caller). */
int mt_embed_bwd(const float* dx, float* dcls, float* dpos_emb, float* dsize_emb, const int64_t* positions,
                 const int32_t* sizes, int B, int F, int n, int dim, int pos_rows, int size_rows, void* stream);

/* adjoint of mt_attn_fwd: dout [B,N,H*64] -> dqkv [B,N,3*H*64] (modes 0 / 1: fully written). Probabilities are recomputed from qkv.
 * mode 2 reads row 0 of dout only and writes dk / dv of every row and dq of row 0 of each clip; the dq section (columns [0, H*64)) of
 * the patch rows is NOT written and keeps what it held -- a caller that reads it zero-fills it first.
 * dqkv_planes (optional, mode 0 / 1): the result as a plane tensor [B*N][3*H*64] (operand of the QKV layer's data and weight
 * gradients).  dqkv is then working memory: its patch rows are left holding the cls query's contribution only.
 * n = 1 .. 100 like mt_attn_fwd (any other n: MT_ERR_UNSUPPORTED, nothing written).  One wavefront owns a whole (b, head, frame) /
 * (b, head, patch) group at every n: patch rows have one writer, the cls key's row takes atomics or, in deterministic mode, a
 * fixed-order reduction with one rank per group. */
int mt_attn_bwd(const float* qkv, const float* dout, float* dqkv, const uint8_t* mask, const uint8_t* ident,
                int B, int H, int F, int n, int mode, float scale, void* dqkv_planes, void* stream);
/* The cls query's adjoint (mt_attn_bwd mode 2; autograd of :80-87 / :112-141 for the query x[:, 0] that the head reads, :270-276) with
 * the COMPLETE plane tensor of dqkv [B*N][3*H*64] as its only output: dk / dv of every key, dq of the cls row, exact zeros in the dq
 * section of every patch row and in the padding rows (rows rounded up to 32) -- what mt_split_planes_blk makes of mode 2's result in
 * a zero-filled dqkv, without the fill, the fp32 tensor or the split pass.  Reads row 0 of each clip of dout [B,N,H*64].  One block
 * per (clip, head), no atomics: the same bits on every run.  n = 1 .. 100 and a 16-byte aligned plane tensor, else an error and
 * nothing written. */
int mt_attn_bwd_cls_planes(const float* qkv, const float* dout, const uint8_t* mask, int B, int H, int F, int n, float scale,
                           void* dqkv_planes, void* stream);

/* ------------------------------------------------------------------------------------------------
 * EfficientNet-B0 backward, everything except the 1x1-convolution dgrad/wgrad (mt_gemm with the BN_BWD prologue).
 * BatchNorm backward is three steps: a producer accumulates sums[2][C] = (sum du, sum du*xhat) into fp64 slots;
 * mt_bn_bwd_finalize turns them into kabc[3][C] so that dz = ka*du + kb*z + kc; consumers apply that on load.
 * ------------------------------------------------------------------------------------------------ */

/* du = (din [*gate[n,c] + dpool[n,c]/hw] [*rowscale[n]]) * (act ? swish'(z*scale+shift) : 1), written to dout when
 * non-NULL (in place allowed), plus the BN sums.  Adjoint of swish/_bn* + SE scaling + drop_connect (model.py:100-127). */
int mt_bn_act_bwd(const float* din, const float* z, const float* scale, const float* shift,
                  const float* mean_invstd, const float* gate, const float* dpool, const float* rowscale,
                  float* dout, double* stats, int slots, int64_t rows, int C, int hw, int act, void* stream);

/* training != 0: batch-statistics BN adjoint; else running-statistics (kb = kc = 0). dgamma/dbeta accumulate. */
int mt_bn_bwd_finalize(const double* stats, int slots, double count, const float* gamma, const float* mean_invstd,
                       float* kabc, float* dgamma, float* dbeta, int C, int training, void* stream);

/* Squeeze-excite adjoint (model.py:104-113): from da = d(gated tensor) computes dgate, the two 1x1-conv weight/bias
 * grads (accumulated) and dpooled [N,C] (the pooling path's contribution to d(activated tensor)).
 * parts & 1: the reduction and the per-image adjoint (dgate, dpre2, dhid, dpooled -- what the data path waits for);
 * parts & 2: the weight / bias gradients from dpre2, dhid (independent of the data path: may run on another stream);
 * parts & 4: the per-image adjoint only (dgate given, e.g. reduced by mt_gemm's MT_EPI_SE_RED; da / z / scale / shift unused).
 * scratch (parts & 5): mt_se_scratch_floats(N, C, CS) floats of workspace (per-slab partial sums of the squeeze gradient). */
int mt_se_scratch_floats(int N, int C, int CS);
int mt_se_bwd(const float* da, const float* z, const float* scale, const float* shift, const float* gate,
              const float* hidden, const float* pooled, const float* w1, const float* w2, float* dgate,
              float* dpre2, float* dhid, float* dpooled, float* dw1, float* db1, float* dw2, float* db2, int N,
              int HW, int C, int CS, int parts, float* scratch, void* stream);

/* Depthwise-conv adjoint: dz = ka*du+kb*z+kc (virtual, output side).  parts&1: dw (accumulated, torch layout
 * [C,1,k,k]); parts&2: du_in = d(input pre-activation) = dgrad * swish'(bn_in(zin)), plus the input-side BN sums.
 * The two parts are independent kernels (the host runs the weight part on a second stream). */
int mt_dwconv_bwd(const float* du, const float* z, const float* kabc, const float* w, const float* zin,
                  const float* scale_in, const float* shift_in, const float* mean_invstd_in, float* du_in,
                  double* stats_in, int slots, float* dw, int N, int H, int W, int C, int k, int stride,
                  int parts, int act, const float* res_pre, const float* res_post, void* stream);
/* act as in mt_dwconv_fwd; stats_in/mean_invstd_in may both be NULL.  du_in = (dgrad + res_pre) * act'(.) + res_post: gradients of
 * other consumers of the activated (res_pre) or raw (res_post) input tensor (Xception skip paths), either may be NULL. */
/* The same with res_pre / res_post given at half resolution, [N, ceil(H/2), ceil(W/2), C]: the gradient that a stride-2 1x1
 * convolution (Xception's skip path, xception.py:36-40) sends to the even (ih, iw) positions of its input; stride must be 1. */
int mt_dwconv_bwd_res2(const float* du, const float* z, const float* kabc, const float* w, const float* zin,
                       const float* scale_in, const float* shift_in, const float* mean_invstd_in, float* du_in,
                       double* stats_in, int slots, float* dw, int N, int H, int W, int C, int k, int stride,
                       int parts, int act, const float* res_pre, const float* res_post, void* stream);

/* _conv_stem weight gradient (accumulated, torch layout [32,3,3,3]); x [N,H,W,3].  H and W of different parity (TF-SAME would pad
 * the two axes differently in front) are MT_ERR_UNSUPPORTED, as in mt_stem_conv_fwd. */
int mt_stem_conv_wgrad(const float* du, const float* z, const float* kabc, const void* x, int x_is_u8, float* dw, int N,
                       int H, int W, void* stream);   /* x fp32 or (x_is_u8) uint8 */
/* ... of the unpadded stride-2 3x3 convolution (Xception's conv1); du, z [N,(H-3)/2+1,(W-3)/2+1,32]. */
int mt_stem_conv_wgrad_valid(const float* du, const float* z, const float* kabc, const void* x, int x_is_u8, float* dw, int N,
                             int H, int W, void* stream);

/* _conv_stem data gradient = the gradient w.r.t. the crops (replaces torch autograd through _conv_stem, reference
 * efficientnet_pytorch/model.py:173,276): dx [N,H,W,3] fp32, OVERWRITTEN (every element is written);
 * dx[n,ih,iw,ci] = sum_{kh,kw,co} dz[n,oh,ow,co] * w[co,ci,kh,kw] over the taps with ih+pb-kh = 2 oh, iw+pb-kw = 2 ow, dz = ka*du+kb*z+kc,
 * pb = the forward's leading TF-SAME pad.  du, z [N*Ho*Wo,32] 16-byte aligned, kabc [3][32], w [32,3,3,3].  Limits as mt_stem_conv_fwd:
 * W <= 512, H and W need the same leading pad.  One writer per element, no atomics: bit-identical from run to run. */
int mt_stem_conv_dgrad(const float* du, const float* z, const float* kabc, const float* w, float* dx, int N, int H, int W,
                       void* stream);
/* ... of the unpadded stride-2 3x3 convolution (replaces torch autograd through Xception's conv1, reference xception.py:161-170);
 * du, z [N,(H-3)/2+1,(W-3)/2+1,32], H, W >= 3.  Input rows / columns that no tap reaches (the last one of an even H / W) come out 0. */
int mt_stem_conv_dgrad_valid(const float* du, const float* z, const float* kabc, const float* w, float* dx, int N, int H, int W,
                             void* stream);

/* Weight gradient of a 1x1 convolution with few channels and very many rows (MBConv expand / project convs of stages 1-4,
 * efficientnet_pytorch/model.py:93-104 under train.py:371):  dw[Cout,Cin] += sum_r (ka*du+kb*z+kc)[r,Cout] * a[r,Cin] with
 * a = x, or (gate != NULL) swish(sc*x+sh)*gate[r/hw].  The whole (32-padded) result stays in MFMA accumulators while the rows
 * stream through; mt_conv1x1_wgrad_supported says whether a shape has an instance (otherwise use mt_gemm, MT_OP_TN). */
int mt_conv1x1_wgrad_supported(int Cout, int Cin);
/* Data AND weight gradient of an expand conv (z = x . W^T, W [Cout, Cin], Cin <= 32) in ONE streaming pass over du (skinny_bwd.hip):
 * with dz = ka*du + kb*z + kc (BatchNorm backward of _bn0): dx[rows, Cin] = dz . W (+ res), dw[Cout, Cin] += dz^T . x.  z is not an
 * argument: it is linear in x, so its share is folded into two Cin x Cin matrices (W^T diag(kb) W and x^T x) inside the kernel.
 * Replaces mt_conv1x1_rows (mode 2) + mt_conv1x1_wgrad on the same tensors: 1 instead of 4 passes over the expanded activations. */
int mt_conv1x1_bwd_fused_supported(int Cout, int Cin);
/* Squeeze-excite stage of the MBConv reverse walk for the early blocks without the project conv's data gradient in memory
 * (skinny_se.hip): da = (ka*du_p + kb*z_p + kc) . W_p is rebuilt from the NARROW gradient inside two streaming passes over z_d:
 *   mode 0: dgate[rows / hw, C] += sum_rows da * swish(z_d*scale + shift)                     (zero-filled by the caller)
 *   mode 1: du_d = (da*gate + dpooled/hw) * swish'(z_d*scale + shift), plus its BatchNorm-backward sums (stats like MT_EPI_STATS,
 *           second sum = du_d * (z_d - mean) * invstd)
 * Replaces mt_conv1x1_rows (mode 2) + the reduction of mt_se_bwd + mt_bn_act_bwd: 3 instead of 6 passes over the expanded tensor.
 * w_p [Co, C] (Co <= 32; C = 32 / 96 / 144), hw % 64 == 0, rows > 0 and rows % hw == 0 (else MT_ERR_ARG).  Read as float4, so 16-byte aligned
 * (else MT_ERR_ARG): du_p, z_p, kabc_p, z_d, scale_d, shift_d, and in mode 1 gate, dpooled, mean_invstd_d, du_d.  stats [|slots|][2][C]; a
 * negative slot count selects the integer-limb accumulators (see mt_set_deterministic above). */
int mt_se_stage_fused_supported(int Co, int C, int hw);
int mt_se_stage_fused(const float* du_p, const float* z_p, const float* kabc_p, const float* w_p, const float* z_d,
                      const float* scale_d, const float* shift_d, int mode, float* dgate, const float* gate, const float* dpooled,
                      const float* mean_invstd_d, float* du_d, double* stats, int slots, int64_t rows, int Co, int C, int hw,
                      void* stream);
/* mt_conv1x1_bwd_fused: rows > 0 (else MT_ERR_ARG); du, kabc, x, res, dx 16-byte aligned (else MT_ERR_ARG). */
int mt_conv1x1_bwd_fused(const float* du, const float* kabc, const float* x, const float* w, const float* res, float* dx,
                         float* dw, int64_t rows, int Cout, int Cin, void* stream);
/* mt_conv1x1_wgrad: rows > 0 (else MT_ERR_ARG); du, z, kabc, x and (when given) gate 16-byte aligned (else MT_ERR_ARG); hw may be
 * any positive value, also above rows (gate then holds one image). */
int mt_conv1x1_wgrad(const float* du, const float* z, const float* kabc, const float* x, const float* sc, const float* sh,
                     const float* gate, int hw, float* dw, int64_t rows, int Cout, int Cin, void* stream);
/* The same weight gradient for the WIDE project convolutions of the late stages (65-320 output x 224-2048 expanded channels, the gate
 * form only: sc, sh, gate required; hw >= 32): the result is cut into 128-column slabs, one block per (slab, row range), load / transform
 * wavefronts feeding MFMA wavefronts through double-buffered LDS (wide_wgrad.hip).  Replaces mt_gemm (MT_OP_TN with both operand
 * prologues), which re-applied the transforms per fragment read.  rows > 0 and hw >= 32 (else MT_ERR_ARG); du, z, kabc, x, sc, sh, gate
 * 16-byte aligned (else MT_ERR_ARG). */
int mt_conv1x1_wgrad_wide_supported(int Cout, int Cin);
int mt_conv1x1_wgrad_wide(const float* du, const float* z, const float* kabc, const float* x, const float* sc, const float* sh,
                          const float* gate, int hw, float* dw, int64_t rows, int Cout, int Cin, void* stream);

/* 1x1 convolution with few channels and very many rows as a streaming kernel (MBConv expand / project convs of stages 1-4 and
 * their data gradients, efficientnet_pytorch/model.py:93-118): out[rows,Cout] = a[rows,Cin] . W^T (+ res), with
 *   amode 0: a = x;   1: a = swish(c0*x + c1) * c2[row / hw]  (c2 = SE gate [rows/hw, Cin]);   2: a = c0*x + c1*x2 + c2 (BatchNorm backward).
 * w is [Cout, ldw] (w_transposed = 0) or the forward weight [Cin, ldw] used transposed (w_transposed = 1, data gradient).
 * stats (optional) receives the BatchNorm sums of `out` like MT_EPI_STATS.  mt_conv1x1_rows_supported tells whether this kernel is
 * the measured better choice for a channel pair and mode (otherwise use mt_gemm); mt_conv1x1_rows itself runs every pair that has an
 * instance (Cin % 4 == 0 and (ceil(Cin/32), ceil(Cout/32)) one of (1,1) (1,3) (1,5) (3,1)) in every mode.  rows > 0 (else MT_ERR_ARG);
 * x, x2 and, in amode 1, c2 are read as float4: 16-byte aligned (else MT_ERR_ARG).  stats [|slots|][2][Cout]; a negative slot count
 * selects the integer-limb accumulators (see mt_set_deterministic above). */
int mt_conv1x1_rows_supported(int Cin, int Cout, int amode);
int mt_conv1x1_rows(const float* x, const float* x2, const float* w, int ldw, int w_transposed, const float* c0, const float* c1,
                    const float* c2, int hw, int amode, const float* res, float* out, double* stats, int slots, int64_t rows,
                    int Cin, int Cout, void* stream);

/* dst_i [cols_i, rows_i] = src_i [rows_i, cols_i]^T for `count` matrices in one launch (the TimeSformer's transposed Linear weights,
 * tsf_engine.py: data gradients in the k-contiguous NT form; replaces 54 torch copy kernels per step).  items: device array of
 * { const float* src; float* dst; int64 rows; int64 cols; int64 tile0 } with tile0 = running count of 32 x 32 tiles. */
int mt_transpose_multi(const void* items, int count, int64_t total_tiles, void* stream);
/* ------------------------------------------------------------------------------------------------
 * Training-step ends (next-row f4).
 * mt_bce_logits: torch.nn.BCEWithLogitsLoss(pos_weight)(logits, labels) with mean reduction (train.py:261,367-368) and its
 *   gradient in one launch: loss[1], dlogits[n] (may be NULL) = d loss / d logits.
 * mt_sgd_multi: torch.optim.SGD(lr, weight_decay) (train.py:186,378; no momentum) over many tensors in one launch:
 *   p -= lr * (g + weight_decay * p).  items = device array of {float* p; const float* g; int64 n; int64 block0} sorted by
 *   block0 = index of the tensor's first 4096-element block; total_blocks = sum over tensors of ceil(n / 4096).
 * ------------------------------------------------------------------------------------------------ */
int mt_bce_logits(const float* logits, const float* labels, float pos_weight, float* loss, float* dlogits, int n, void* stream);
int mt_sgd_multi(const void* items, int count, int64_t total_blocks, float lr, float weight_decay, void* stream);
/* mt_adam_multi: torch.optim.Adam (decoupled_weight_decay = 0: L2 term added to the gradient) / torch.optim.AdamW
 *   (decoupled_weight_decay = 1: p *= 1 - lr*wd first) over many tensors in one launch (train.py:187-190, :378; amsgrad off).
 *   items = device array of {float* p; const float* g; float* m; float* v; int64 n; int64 block0} sorted by block0 (as above).
 *   step_size = lr / (1 - beta1^t), bias_correction2_sqrt = sqrt(1 - beta2^t) for the step count t of this call. */
int mt_adam_multi(const void* items, int count, int64_t total_blocks, float lr, float weight_decay, double beta1, double beta2,
                  float eps, float step_size, float bias_correction2_sqrt, int decoupled_weight_decay, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Epoch metrics (next-row f5; csrc/metrics.hip).  The reference moves the logits to the host every step and counts there.
 * mt_metrics_update: one step's share of check_correct (utils.py:32-57 as called at train.py:367-374, :434-441, test.py:267-277) and of
 *   `total_loss += round(loss.item(), 2)` (train.py:370, test.py:270), accumulated into device state; one launch of one block, no
 *   atomics (launches on one stream are serialised: one writer), no host read.  logits [n] fp32; labels [n] fp32, 0 or 1 (non-zero = 1);
 *   loss [1] fp32 or NULL; mc_labels [n] fp32 or NULL (test.py's multiclass_labels: may be NaN).
 *   Predicted class = logit > 0.  The reference's round(fp32 sigmoid(logit)) differs only for 0 < logit <~ 1.2e-7, where fp32 sigmoid is
 *   exactly 0.5 and rounds to 0; logit == 0 and a NaN logit are class 0 under both.
 *   counts [8] int64 += { n_seen, tp, fp, tn, fn, steps, stored, overflow }: correct = tp + tn, positive_class = tp + fp,
 *   negative_class = tn + fn.  loss_sums [2] fp64 += { loss, rint(loss * 100) / 100 } in call order (required when loss is given).
 *   mc_errors [9] int64 (test.py:219; required with mc_labels): [c] += 1 per misclassified sample whose class is an integer in 0..8;
 *   NaN and any other value are skipped (utils.py:44).  Every (logit, label) is appended to store_scores / store_labels [capacity] at
 *   the position counts[6], which the kernel reads from the state (no host-side dependence on earlier calls: capturable in a graph);
 *   what does not fit is dropped and counts[7] is set to 1 -- the counters still count every sample.  The caller zeroes the state.
 * mt_metrics_auc: the exact area under the ROC curve of the first n stored samples (test.py:280-282 metrics.roc_curve + metrics.auc),
 *   as integers: out [4] uint64 = { gt, eq, n_pos, n_neg } with gt / eq = the number of (positive i, negative j) pairs with
 *   score_i > / == score_j, so AUC = (2 gt + eq) / (2 n_pos n_neg) -- equal, in real arithmetic, to the trapezoid area with half
 *   credit for ties.  NaN scores take part in no pair and in neither class count.  It ranks the logits where the reference ranks fp32
 *   sigmoid(logit): they differ only where distinct logits collapse to one sigmoid value (from about |logit| > 16.6, or closer than
 *   an ulp).  Tiled all-pairs count, one block partial each, summed by a second launch in index order; no atomics.
 *   partials: 4 * ceil(n / 256) uint64 of scratch.  n = 0 writes zeros; n > 2^24 returns MT_ERR_UNSUPPORTED (nothing launched).
 * ------------------------------------------------------------------------------------------------ */
int mt_metrics_update(const float* logits, const float* labels, const float* loss, const float* mc_labels, int64_t* counts,
                      double* loss_sums, int64_t* mc_errors, float* store_scores, unsigned char* store_labels, int64_t capacity,
                      int n, void* stream);
int mt_metrics_auc(const float* store_scores, const unsigned char* store_labels, int64_t n, uint64_t* partials, uint64_t* out,
                   void* stream);

/* ------------------------------------------------------------------------------------------------
 * Identity clustering (next-row f6; csrc/identity.hip).  The reference copies a video's FaceNet embeddings to the host, takes
 * np.dot(E, E.T) (preprocessing/cluster_faces.py:96, predict.py:162) and hands it to _generate_connected_components
 * (preprocessing/utils.py:16-29, called at cluster_faces.py:101 and predict.py:167 with threshold 0.45): a Python double loop over all
 * n^2 entries that adds the edge (i, j) to a networkx graph wherever i != j and similarities[i, j] > threshold, then lists the
 * connected components.  The rule, for one video with faces 0..n-1:
 *   similarity  s_ij = sum_k e_ik * e_jk in fp32, no normalisation, ascending k as one fma chain (v_mfma_f32_32x32x2_f32): s_ij and
 *               s_ji are the same bits;
 *   edge        i -- j iff i != j and s_ij > threshold (strict; a NaN similarity is no edge); never across videos;
 *   label       -1 for a face without an edge (the reference never adds it to the graph: the dataset's discarded faces); otherwise the
 *               0-based rank of its connected component among the video's components ordered by smallest member -- the order in
 *               which nx.connected_components yields them for that graph (networkx keeps nodes in insertion order, and the loop
 *               first touches a component at the row of its smallest member when the matrix is symmetric, as a Gram matrix is).
 * A batch is ragged: offsets [V + 1] int32 (device), video v owns rows offsets[v] .. offsets[v + 1] - 1 of the T rows.
 * Limits, checked before anything is launched or written: 1 <= max_faces <= 4096 (a video's labels live in LDS) and 1 <= D <= 2048,
 * else MT_ERR_UNSUPPORTED; V >= 1, T >= 0.  A video with 0 faces is legal (no tile, n_identities = 0).
 * err_flag (optional, device int32, sticky, as in mt_embed_fwd): bit 0 = a video has more than max_faces faces -- it is treated as
 * truncated to its first max_faces (the faces past them are labelled -1) and no access leaves the T rows or the W words; bit 1 = the
 * label loop hit its trip bound (cannot happen on a symmetric adjacency; a defect must not become a hang); bit 2 = offsets outside
 * [0, T] (that video is skipped).
 * mt_identity_adjacency: adj [T][W] uint32, W = ceil(max_faces / 32): bit j & 31 of word j >> 5 of row offsets[v] + i is the edge
 *   i -- j of video v; the bits past a video's faces are written as zero and every row of a (truncated) video is written whole.
 *   32 x 32 tiles of each video's Gram matrix, one wavefront each, compared in the accumulator registers and packed with wave ballots;
 *   no [n, n] float matrix is written.  Both triangles are computed, with the same k order: adj is symmetric.  Block b is a tile of
 *   the video with tile_prefix[v] <= b < tile_prefix[v + 1], tile_prefix [V + 1] int32 (device) = running sum of
 *   ceil(min(n_v, max_faces) / 32)^2, total_tiles = its last entry = the grid.
 * mt_identity_adjacency_sim: the same bit matrix, [n][ceil(n / 32)], from a ready similarity matrix sim [n, n] fp32 of ONE video (the
 *   reference function's own argument; need not be symmetric): i -- j iff i != j and (sim[i][j] > threshold or sim[j][i] > threshold)
 *   -- the reference visits both orders and its graph is undirected.  n <= 4096.  source [n] int32: 1 where row i itself holds an
 *   entry above the threshold.  For an asymmetric matrix the reference's loop first touches a component at its smallest SOURCE, not
 *   at its smallest member, and that decides the order in which the components are listed.
 * mt_identity_components: one block per video over adj (row pitch W = ceil(max_faces / 32), which must be symmetric): labels [T] int32
 *   as above, n_identities [V] int32, sizes [T] int32 or NULL: sizes[offsets[v] + k] = members of identity k of video v, 0 for
 *   k >= n_identities[v].  source [T] int32 or NULL: with it, components are ranked by their smallest member that is a source (the
 *   order of the reference on an asymmetric matrix); NULL ranks by smallest member.  Minimum-label propagation + pointer jumping until a round changes nothing, at most n + 1 rounds; the
 *   result is the unique minimum-member labelling whatever the schedule.  Integer atomics only.
 * ------------------------------------------------------------------------------------------------ */
int mt_identity_adjacency(const float* emb, const int* offsets, const int* tile_prefix, int V, int T, int D, int total_tiles,
                          int max_faces, float threshold, uint32_t* adj, int* err_flag, void* stream);
int mt_identity_adjacency_sim(const float* sim, int n, float threshold, uint32_t* adj, int* source, void* stream);
int mt_identity_components(const uint32_t* adj, const int* offsets, const int* source, int V, int T, int max_faces, int* labels,
                           int* n_identities, int* sizes, int* err_flag, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Xception (config 5 extractor, reference models/xception.py).  Dense convolutions are mt_gemm with the IM2COL
 * prologue; separable convolutions are mt_dwconv_* (act 0/2) + mt_gemm; the rest:
 * ------------------------------------------------------------------------------------------------ */

/* torch conv weight [Co,Ci,k,k] -> GEMM operand out[r][(kh,kw,c)] with row pitch ld (zero padded, ld %% 4 == 0).
 * transpose 0: rows = Co (forward / wgrad layout); 1: rows = Ci with the kernel flipped (data-gradient convolution). */
int mt_conv_weight_pack(const float* w, float* out, int Co, int Ci, int k, int ld, int transpose, void* stream);
/* dw[co][ci][kh][kw] += dwp[co][(kh,kw,ci)] */
int mt_conv_weight_unpack_grad(const float* dwp, float* dw, int Co, int Ci, int k, int ld, void* stream);

/* Block tail (xception.py:64-79): y = MaxPool2d(3,2,1)(z*scale+shift) + (zs*scale_s+shift_s); z [N,H,W,C], zs,y [N,Ho,Wo,C]. */
int mt_maxpool_add_fwd(const float* z, const float* scale, const float* shift, const float* zs, const float* scale_s,
                       const float* shift_s, float* y, int N, int H, int W, int C, void* stream);
/* du (pre-zeroed, [N,H,W,C]) += dy routed to each window's arg-max of z*scale+shift. */
int mt_maxpool_bwd(const float* dy, const float* z, const float* scale, const float* shift, float* du, int N, int H,
                   int W, int C, void* stream);
/* The block tail with the adjoint's routing recorded (training): also writes arg [N,Ho,Wo,C] uint8 = the window position kh*3+kw of each
 * window's arg-max (first maximum in row-major order, like torch; 255 = none) and zmax = the raw z there.  The BatchNorm-backward sums of
 * the pooled unit are then sums over the POOLED tensors (S1 = sum dy, S2 = sum dy * xhat(zmax): mt_bn_act_bwd on dy / zmax), and the
 * routed gradient is a gather with one writer per element -- no zero fill, no atomics, bit-identical run to run:
 *   mt_maxpool_bwd_arg: du [N,H,W,C] = dy routed (every element written);
 *   mt_maxpool_bn_bwd_apply_planes: dz = ka*du + kb*z + kc with du routed on the fly, written as a plane tensor (mt_gemm_planes operand);
 *     du never exists in memory (replaces zero fill + mt_maxpool_bwd + the full-resolution sums pass + mt_bn_bwd_apply_planes). */
int mt_maxpool_add_fwd_arg(const float* z, const float* scale, const float* shift, const float* zs, const float* scale_s,
                           const float* shift_s, float* y, uint8_t* arg, float* zmax, int N, int H, int W, int C, void* stream);
int mt_maxpool_bwd_arg(const float* dy, const uint8_t* arg, float* du, int N, int H, int W, int C, void* stream);
int mt_maxpool_bn_bwd_apply_planes(const float* dy, const uint8_t* arg, const float* z, const float* kabc, void* planes, int N, int H,
                                   int W, int C, void* stream);
/* dz = ka*du + kb*z + kc materialised (dense conv2's data gradient is itself an im2col GEMM over dz). */
int mt_bn_bwd_apply(const float* du, const float* z, const float* kabc, float* dz, int64_t rows, int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Operand-plane producers for EfficientNet-B0's late stages (model.py:89-128; csrc/effnet_planes.hip): the MBConv 1x1 convolutions of
 * the 14 x 14 / 7 x 7 stages and the head on mt_gemm_planes.
 * mt_bn_act_fwd_planes: mt_bn_act_fwd (block output y = act(z * scale + shift) [* rowscale[row / rows_per_group]] [+ res]) that also
 *   writes y as a plane tensor -- the next expand convolution's operand (forward and weight gradient).
 * mt_bn_swish_gate_planes: the project convolution's operand swish(z * scale[c] + shift[c]) * gate[(row / hw) * C + c] (model.py:104-116:
 *   _bn1, swish, squeeze-excite gate) as a plane tensor.
 * ------------------------------------------------------------------------------------------------ */
int mt_bn_act_fwd_planes(const float* z, const float* scale, const float* shift, const float* res, float* y, int rows, int C, int act,
                         const float* rowscale, int rows_per_group, void* y_planes, void* stream);
int mt_bn_swish_gate_planes(const float* z, const float* scale, const float* shift, const float* gate, int hw, void* planes, int rows,
                            int C, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Baseline head (reference models/baseline.py:15-37, `--model 0`): AdaptiveAvgPool2d(1) -> Linear(dim, mlp) -> Linear(mlp, 1) over
 * per-crop features, for num-classes 1 only (csrc/baseline.hip).  With one class and no nonlinearity between the Linears the head is
 * the vector v = W1^T w2 and the scalar c0 = w2 . b1 + b2:  logit_i = mean_p(x_i[p, :]) . v + c0.  No GEMM runs and no atomic is
 * issued: every sum is in a fixed order, so the results are the same bits run after run (deterministic mode or not).
 * Shapes: x holds n crops of C channels and hw pixels, layout 0 = NHWC (x[i][p][c], the extractors' own output) or 1 = NCHW
 * (x[i][c][p]); W1 [m][C], b1 [m], w2 [m] (the single row of the second Linear's weight), b2 [1].  C % 4 == 0, n <= 65535,
 * C * hw < 2^31; offsets past one crop are 64-bit.  x, dx, vc, work, W1 and dW1 are 16-byte aligned.
 * mt_baseline_head_fwd: vc [C + 1] = (v, c0) (kept for the backward); pooled [n][C] = the mean features (NULL: not written -- an
 *   inference forward); part = scratch of n * ceil(C / 256) floats; logits [n].
 * mt_baseline_head_bwd: from dlogits [n] = dL/dlogit, the gradients whose pointer is not NULL: dW1 [m][C], db1 [m], dW2 [m], db2 [1]
 *   (these need pooled, W1, b1, w2 and work = scratch of (ceil(n / 32) + 1) * (C + 4) floats) and dx = dlogit_i v / hw broadcast over
 *   the crop's pixels, written in `layout` (the input's).  Nothing is launched for a NULL output.
 * ------------------------------------------------------------------------------------------------ */
int mt_baseline_head_fwd(const float* x, int layout, int n, int hw, int C, int m, const float* w1, const float* b1, const float* w2,
                         const float* b2, float* vc, float* pooled, float* part, float* logits, void* stream);
int mt_baseline_head_bwd(const float* dlogits, const float* pooled, const float* vc, int n, int hw, int C, int m, const float* w1,
                         const float* b1, const float* w2, float* dw1, float* db1, float* dw2, float* db2, float* dx, int layout,
                         float* work, void* stream);

/* ------------------------------------------------------------------------------------------------
 * SlowFast R50 (pytorchvideo slowfast_r50, reference train.py:143-147 / test.py:121-125, `--model 2`; csrc/conv3d.hip, slowfast.hip).
 * Activations are channels-last rows: [N][T][H][W] rows of C floats with a row pitch (ld*, in floats), so a pathway's channel slice of
 * a concatenated tensor is addressed in place.  No entry point issues an atomic and every sum runs in a fixed order: the results are
 * the same bits run after run, deterministic mode or not.  Offsets are 64-bit (no 4 GB operand limit).
 *
 * mt_conv3d_*: Conv3d as an implicit GEMM on v_mfma_f32_32x32x2_f32, any (kt, kh, kw) kernel, per-axis stride and padding;
 *   C % 4 == 0, K % 4 == 0, pitches % 4 == 0 (the 3-channel stems take a 4th, zero, channel: mt_sf_ingest writes it).
 *   fwd:   y[m][co] (+)= sum pro(x)[in(m, tap)][ci] * w[co][tap][ci]  (w = torch weight permuted to [K][kt][kh][kw][C]);
 *          pro(v) = relu(v * scale[ci] + shift[ci]) when scale is given (BatchNorm + ReLU of the producer; padding stays zero);
 *          part != NULL: BatchNorm sums of y, stats [2][K] fp64 (sum, sum of squares; written, slot count 1 for mt_bn_finalize);
 *          part holds mt_conv3d_part_floats(d) floats.
 *   dgrad: dx[r][ci] (+)= sum dy[out(r, tap)][co] * wt[tap][co][ci]  (wt = weight permuted to [kt][kh][kw][K][C]); a gather, so
 *          every stride works without atomics.  dx is the gradient of pro(x) (the caller applies the BatchNorm-ReLU adjoint).
 *   wgrad: dw[co][tap][ci] = sum_m dy[m][co] * pro(x)[in(m, tap)][ci]  (written); split over rows into ws and added in split order.
 *          splits: any count from 1 (mt_conv3d_wgrad_splits(d) is the planner's choice, not a requirement), with ws of
 *          splits * K * taps * C floats for splits > 1 (else ws may be NULL).  The rows are dealt in equal parts rounded up to whole
 *          steps of 16, so only the first nsplit <= splits slabs of ws are used; one part (nsplit == 1) writes dw directly.
 * mt_sf_bn_relu_fwd: y = relu(z * scale + shift + r), r = res * rscale + rshift (rscale given), res, or 0 (res NULL).
 * mt_sf_bn_relu_bwd_stats / _apply: the BatchNorm(+ReLU) adjoint.  du = g * mask with mask = (z * scale + shift > 0) when scale is
 *   given, (m > 0) when m is given, else 1.  stats [2][C] (fp64, written) = (sum du, sum du * (z - mean) * invstd) for
 *   mt_bn_bwd_finalize (slots 1, count = rows); part holds mt_sf_bn_bwd_part_floats(rows, C) floats.  apply: out (+)= ka du + kb z + kc
 *   (kabc given) or du.
 * mt_sf_maxpool_fwd / _bwd: MaxPool3d((1,3,3), (1,2,2), (0,1,1)) over relu(z * scale + shift) (z [NT][H][W][C]), first maximum in
 *   window order, arg = h * W + w (int32 [rows out][C]); out has pitch ldo.  bwd: din [NT][H][W][C] (written) as a gather.
 * mt_sf_head_*: ResNetBasicHead of both pathways.  pool: d[b][p][coff + c] = mult * mean of feat over window p (AvgPool3d stride 1,
 *   p row-major over the (T-kt+1, H-kh+1, W-kw+1) grid; mult = dropout keep / (1 - p) multipliers, NULL = none).  proj: logits[b][j] =
 *   bias[j] + mean_p W[j] . d[b][p] (Linear at every window, AdaptiveAvgPool3d(1)).  bwd: dW (+=), db (+=), dpool = mult * dd.
 *   dfeat: the window pooling's adjoint (written, pitch ldf).
 * mt_sf_ingest: frame j of fidx (int32 [Tout]) -> (v(src[b][fidx[j]][h][w][c]), c < 3; 0) as 4 floats, into out [B][Tsplit][H][W][4]
 *   for j < Tsplit, else out2 [B][Tout - Tsplit][H][W][4]; v = (u / 255 - 0.45) / 0.225 (normalize) or u; src uint8 (is_u8) or fp32
 *   with element strides (b, f, h, w, c).  Both pathways in one launch: reference utils.py:166-186 (UniformTemporalSubsample, /255,
 *   Normalize, PackPathway).
 * mt_sf_ingest_bwd: the ingest's adjoint, dsrc[b][f][h][w][c] = k * sum over the output frames j with fidx[j] == f of
 *   dout_j[b][.][h][w][c], c < 3 (dout_j in dout [B][Tsplit][H][W][4] for j < Tsplit, else in dout2; the 4th channel is not read);
 *   k = 1 / (255 * 0.225) (normalize) or 1.  The inverse map comes CSR style: start (int32 [F + 1]) and jlist (int32 [Tout], j
 *   ascending inside a frame): frame f sums jlist[start[f] .. start[f+1]) in that order, a frame nobody selected gets exact 0.
 *   dsrc is fp32 with the element strides (b, f, h, w, c) of mt_sf_ingest's src; written, one writer per element.
 * mt_sf_ingest_resize (csrc/sf_resize.hip): mt_sf_ingest with the reference's two spatial steps between Normalize and PackPathway:
 *   ShortSideScale (bilinear, align_corners = False, no antialiasing) of the Hs x Ws source frames to Hr x Wr and CenterCropVideo to
 *   the window [top, top + Ho) x [left, left + Wo).  out [B][Tsplit][Ho][Wo][4] / out2 [B][Tout - Tsplit][Ho][Wo][4], 4th channel 0.
 *   The caller gives the taps of the WINDOW's rows and columns (window index d <-> resized index top + d, left + d): hidx (int32
 *   [2][Ho]: source rows i0, then i1) and hlam (fp32 [Ho]); widx ([2][Wo]) and wlam ([Wo]) likewise.  Per channel, with
 *   v = (u / 255 - 0.45) / 0.225 (normalize) or u taken of every tap BEFORE the interpolation (the reference's order):
 *     out = (1 - hlam) ((1 - wlam) v[i0h][i0w] + wlam v[i0h][i1w]) + hlam ((1 - wlam) v[i1h][i0w] + wlam v[i1h][i1w])
 *   Table indices are clamped to the source frame before they address it.  Hr, Wr, top, left only say what the tables were made
 *   for: a window outside the resized frame returns MT_ERR_ARG.
 * mt_sf_ingest_resize_bwd: its exact adjoint as a gather, dsrc as mt_sf_ingest_bwd's (fp32, the source's strides, written, one writer
 *   per element, k as there):  dsrc[b][f][hs][ws][c] = k * sum hwt[r] * wwt[q] * dout_j[b][.][hout[r]][wout[q]][c]  over the output
 *   frames j = jlist[fstart[f] .. fstart[f+1]), the row references r in [hstart[hs], hstart[hs+1]) and the column references q in
 *   [wstart[ws], wstart[ws+1]), in that nesting and in list order.  hstart (int32 [Hs + 1]), hout (int32: window row) and hwt
 *   (fp32: 1 - hlam for a reference as i0, hlam as i1; a clamped edge with i1 == i0 lists both) are the inverse of hidx / hlam, CSR
 *   style; wstart, wout, wwt likewise.  A frame nobody selected, a pixel outside the window's footprint and any element no tap
 *   references get exact 0.
 *   Both: MT_ERR_ARG for a null pointer, an empty shape or a window outside the resized frame; MT_ERR_UNSUPPORTED, before any
 *   launch, for packed buffers that are not 16-byte aligned (and for more than 65535 clips or frames).
 * mt_sf_stem_dgrad: the stems' data gradient down to the clip (csrc/sf_stem_dgrad.hip), with Ho = (H-1)/2 + 1, Wo = (W-1)/2 + 1:
 *   dx[n][t][h][w][c] = sum_{dt,kh,kw,co} dz[n][t + kt/2 - dt][(h+3-kh)/2][(w+3-kw)/2][co] * w[co][c][dt][kh][kw] over the taps with
 *   even h+3-kh and w+3-kw and a dz index on the grid.  dz [N][T][Ho][Wo] rows of K floats, pitch ldz (% 4 == 0), 16-byte aligned;
 *   wt = the weight repacked by the host to [kt*K][160]: row dt*K + co, column (kh*7 + kw)*3 + c, columns 147..159 zero;
 *   dx [N][T][H][W][4], 16-byte aligned, written (4th channel 0).  (kt, K) = (1, 64) (slow stem) or (5, 8) (fast stem), any N, T, H,
 *   W >= 1; anything else returns MT_ERR_UNSUPPORTED before a launch.  A gather on v_mfma_f32_32x32x2_f32: no atomics.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int N, T, H, W, C;                      /* input grid and channels */
  int To, Ho, Wo, K;                      /* output grid and channels */
  int kt, kh, kw, st, sh, sw, pt, ph, pw; /* kernel, stride, padding per axis */
  int64_t ldx, ldy;                       /* row pitches (floats) of the input and output rows */
} mt_conv3d_desc;
int64_t mt_conv3d_part_floats(const mt_conv3d_desc* d);
int mt_conv3d_wgrad_splits(const mt_conv3d_desc* d);
int mt_conv3d_fwd(const mt_conv3d_desc* d, const float* x, const float* scale, const float* shift, const float* w, float* y, int accumulate,
                  float* part, double* stats, void* stream);
int mt_conv3d_dgrad(const mt_conv3d_desc* d, const float* dy, const float* wt, float* dx, int accumulate, void* stream);
int mt_conv3d_wgrad(const mt_conv3d_desc* d, const float* x, const float* scale, const float* shift, const float* dy, float* dw, float* ws,
                    int splits, void* stream);
int mt_sf_bn_relu_fwd(const float* z, int64_t ldz, const float* scale, const float* shift, const float* res, int64_t ldr,
                      const float* rscale, const float* rshift, float* y, int64_t ldy, int64_t rows, int C, void* stream);
int64_t mt_sf_bn_bwd_part_floats(int64_t rows, int C);
int mt_sf_bn_relu_bwd_stats(const float* g, int64_t ldg, const float* z, int64_t ldz, const float* scale, const float* shift, const float* m,
                            int64_t ldm, const float* mean_invstd, float* part, double* stats, int64_t rows, int C, void* stream);
int mt_sf_bn_relu_bwd_apply(const float* g, int64_t ldg, const float* z, int64_t ldz, const float* scale, const float* shift, const float* m,
                            int64_t ldm, const float* kabc, float* out, int64_t ldo, int accumulate, int64_t rows, int C, void* stream);
int mt_sf_maxpool_fwd(const float* z, const float* scale, const float* shift, float* out, int64_t ldo, int* arg, int64_t NT, int H, int W,
                      int C, void* stream);
int mt_sf_maxpool_bwd(const float* dout, int64_t ldd, const int* arg, float* din, int64_t NT, int H, int W, int C, void* stream);
int mt_sf_head_pool(const float* feat, int64_t ldf, const float* mult, float* d, int B, int T, int H, int W, int C, int kt, int kh, int kw,
                    int coff, int CT, void* stream);
int mt_sf_head_proj(const float* d, const float* w, const float* bias, float* logits, int B, int P, int CT, int J, void* stream);
int mt_sf_head_bwd(const float* g, const float* d, const float* w, const float* mult, float* dw, float* db, float* dpool, int B, int P, int CT,
                   int J, void* stream);
int mt_sf_head_dfeat(const float* dpool, float* dfeat, int64_t ldf, int B, int T, int H, int W, int C, int kt, int kh, int kw, int coff,
                     int CT, void* stream);
int mt_sf_ingest(const void* src, int is_u8, int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc, const int* fidx, int Tout,
                 int Tsplit, int B, int H, int W, int normalize, float* out, float* out2, void* stream);
int mt_sf_ingest_bwd(const float* dout, const float* dout2, const int* start, const int* jlist, int F, int Tout, int Tsplit, int B, int H,
                     int W, int normalize, float* dsrc, int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc, void* stream);
int mt_sf_ingest_resize(const void* src, int is_u8, int64_t sb, int64_t sf, int64_t sh, int64_t sw, int64_t sc, const int* fidx, int Tout,
                        int Tsplit, int B, int Hs, int Ws, const int* hidx, const float* hlam, const int* widx, const float* wlam, int Hr,
                        int Wr, int top, int left, int Ho, int Wo, int normalize, float* out, float* out2, void* stream);
int mt_sf_ingest_resize_bwd(const float* dout, const float* dout2, const int* fstart, const int* jlist, int F, int Tout, int Tsplit, int B,
                            int Hs, int Ws, const int* hstart, const int* hout, const float* hwt, const int* wstart, const int* wout,
                            const float* wwt, int Hr, int Wr, int top, int left, int Ho, int Wo, int normalize, float* dsrc, int64_t sb,
                            int64_t sf, int64_t sh, int64_t sw, int64_t sc, void* stream);
int mt_sf_stem_dgrad(const float* dz, int64_t ldz, const float* wt, float* dx, int N, int T, int H, int W, int kt, int K, void* stream);

/* ------------------------------------------------------------------------------------------------
 * FaceNet InceptionResnetV1, inference only (the embedder in front of the identity clustering: reference predict.py:150-158,
 * preprocessing/cluster_faces.py:84-92; csrc/facenet.hip).  Activations are channels-last rows, [N][H][W] rows of C floats with a row
 * pitch (ld*, in floats), so a branch's last convolution and the pooling branches write their channel slice of the concatenation
 * buffer in place.  BatchNorm is folded into the weights and a bias by the caller.  No entry point issues an atomic; every sum runs in
 * an order fixed by the layer's own geometry (C, K, kh, kw, Ho, Wo, stride, padding) and NEVER by N: a face's rows are the same bits
 * whoever shares its batch.  Row offsets are 64-bit; row counts stay below 2^31.
 *
 * mt_conv2d_fwd: Conv2d as an implicit GEMM on v_mfma_f32_32x32x2_f32, any (kh, kw), per-axis stride and padding.
 *     conv[m][co] = sum_{tap, ci} x[in(m, tap)][ci] * w[co][tap][ci]      (w = torch weight permuted to [K][kh][kw][C]; zero padding)
 *     y = act(conv + bias)                        res == NULL
 *     y = act(res + res_scale * (conv + bias))    res given (rows of K floats, pitch ldr): the Inception-ResNet block tail
 *   act 0 = none, 1 = ReLU; bias [K] or NULL.  One block owns a 64 x 64 output tile and walks the whole reduction in ascending
 *   (tap, ci) order, 32 per step, each step 16 MFMAs of depth 2: the result is a chain of fused multiply-adds with one rounding per
 *   product, |y - exact| <= (kh kw C + 4) 2^-24 (|res| + |res_scale| (sum |x w| + |bias|)) to first order.
 *   C % 4 == 0, K % 4 == 0, pitches % 4 == 0 and >= the widths, x and w 16-byte aligned, else MT_ERR_UNSUPPORTED (the 3-channel stem
 *   takes a 4th, zero, channel: mt_face_ingest writes it).  Ho, Wo must equal floor((in + 2 p - k) / s) + 1, else MT_ERR_ARG.
 *   Nothing is launched or written on an error.  y may alias neither x nor res.
 * mt_face_ingest: src [T][H][W][3] uint8 (is_u8) or fp32 with ELEMENT strides (st, sh, sw, sc) -- a channels-last crop array, or
 *   the NCHW tensor of the reference's call -- -> out [T][H][W][4] fp32, 16-byte aligned: (u - 127.5) / 128 (standardize; both steps
 *   are exact for uint8) or u, the 4th channel 0.
 * mt_maxpool2d_fwd: MaxPool2d(k = 3, s = 2, p = 0) of x [N][H][W] rows (pitch ldx) into y [N][Ho][Wo] rows (pitch ldy), C % 4 == 0,
 *   both 16-byte aligned; any other (k, s, p) returns MT_ERR_UNSUPPORTED.
 * mt_avgpool_rows: y[n][c] = (x[n*rows][c] + ... + x[n*rows + rows - 1][c]) / rows, added in that order (AdaptiveAvgPool2d(1)).
 * mt_l2_normalize_rows: y[r] = x[r] / max(||x[r]||_2, eps) (F.normalize); a zero row stays zero.  One wavefront per row, the sum of
 *   squares as 64 strided chains joined by a fixed butterfly.
 * ------------------------------------------------------------------------------------------------ */
typedef struct {
  int N, H, W, C;                 /* input grid and channels */
  int Ho, Wo, K;                  /* output grid and channels */
  int kh, kw, sh, sw, ph, pw;     /* kernel, stride, padding per axis */
  int act;                        /* 0 none, 1 ReLU */
  float res_scale;                /* multiplies conv + bias when res is given */
  int64_t ldx, ldy, ldr;          /* row pitches (floats) of x, y and res */
} mt_conv2d_desc;
int mt_conv2d_fwd(const mt_conv2d_desc* d, const float* x, const float* w, const float* bias, const float* res, float* y, void* stream);
int mt_face_ingest(const void* src, int is_u8, int64_t st, int64_t sh, int64_t sw, int64_t sc, int T, int H, int W, int standardize,
                   float* out, void* stream);
int mt_maxpool2d_fwd(const float* x, int64_t ldx, float* y, int64_t ldy, int N, int H, int W, int C, int k, int s, int p, void* stream);
int mt_avgpool_rows(const float* x, int64_t ldx, float* y, int64_t ldy, int N, int rows, int C, void* stream);
int mt_l2_normalize_rows(const float* x, int64_t ldx, float* y, int64_t ldy, int64_t rows, int D, float eps, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Face crops for the embedder (csrc/face_crops.hip): what the reference does on the host, one face at a time, between the detector
 * and InceptionResnetV1 -- the crop rule of predict.py:103-140 (= preprocessing/extract_crops.py:75-113) and preprocess_images
 * (preprocessing/utils.py:32-34), torchvision Resize([128, 128]) of a PIL image = Pillow's Image.resize(BILINEAR), antialiased.
 *
 * mt_face_rects: boxes [T][4] fp32 (xmin, ymin, xmax, ymax; half-resolution frame coordinates) -> rects [T][4] int32
 *   (x0, y0, w, h) in the H x W frame, valid [T] bytes.  One thread per face, integers only:
 *     every coordinate is doubled and truncated toward zero (it may be negative); bw, bh = the box's width and height;
 *     padding pw = floor(bw / 3), ph = floor(bh / 3) (floor, also of a negative);
 *     the padded spans sw = (xmax + pw) - max(xmin - pw, 0), sh likewise; the LONGER span's padding is reduced by
 *     trunc((longer - shorter) / 2), which squares the window while it is inside the frame (on a tie pw takes the zero);
 *     window = rows max(ymin - ph, 0) .. ymax + ph, columns max(xmin - pw, 0) .. xmax + pw, the far ends cut at H and W;
 *     if that window (cut by an edge) is not square, the longer side loses d = trunc(|h - w| / 2) at BOTH ends when d > 0; when
 *     d == 0 (sides one apart) a taller window drops its FIRST row, a wider one its LAST column.  The result may stay one off square.
 *   valid = 0, rect = (0, 0, 0, 0) and *err += 1 (sticky device int32 counter, NULL allowed) when the window is empty, when a far
 *   end is negative (a Python slice would wrap around), when a side is longer than 4096, when frame_index[t] is outside [0, N), or
 *   when a coordinate is not finite or beyond 2^29.  H, W >= 1, N >= 1, T >= 0.
 *
 * mt_crop_resize_u8: T source windows of any size -> out [T][OH][OW][3] uint8, one launch, no host read.  The source is either
 *   frames  src = [N][H][W][3] uint8 with rects / frame_index / valid as mt_face_rects leaves them (crops == NULL), or
 *   packed  src = a byte buffer of src_bytes bytes, crops [T][4] int64 = (byte offset, row pitch in bytes, w, h) of ready RGB crops.
 *   A face whose entry is not valid, or does not lie inside the source, or has a side outside 1..4096 comes out all zeros; the
 *   latter two also set bit 0 of err[1] (err = device int32 [2] or NULL; err[0] is mt_face_rects' counter).
 *   Per axis, in IEEE double without contraction (in = window side, out = output side):
 *     scale = in / out, fs = max(scale, 1), support = fs, ksize = 2 ceil(support) + 1; for output index i:
 *     center = (i + 0.5) scale, first = max((int)(center - support + 0.5), 0), n = min((int)(center + support + 0.5), in) - first,
 *     w_j = max(1 - |(j + first - center + 0.5) / fs|, 0) for j < n, summed in index order, each divided by the sum,
 *     k_j = (int)(w_j 2^22 + 0.5);  a pass is  clip((2^21 + sum_j pixel_j k_j) >> 22, 0, 255)  in int32.
 *     (Pillow's C multiplies by 1.0 / fs where this divides by fs; the k_j of the two forms are equal wherever they were compared:
 *     every in of 1..4096 at out = 1, 2, 3, 96, 128, 160, 256.)
 *   The horizontal pass runs first into uint8, the vertical pass over that -- except, as Image.resize itself does, for a window more
 *   than 100 times as tall as wide with OH < h, which is resized vertically first.  1 <= OH, OW <= 256, T <= 65535 (grid.y), else
 *   MT_ERR_UNSUPPORTED before anything is launched.  max_w: an upper bound of the window widths (<= 4096) known to the host; it
 *   sizes the x coefficient table in LDS, never the result (a window whose table would not fit counts as outside the source).  A
 *   face's bytes do not depend on the batch.  Grid = (8 bands of output rows, T); a block walks its band in sub-bands whose
 *   horizontal-pass rows fit its LDS tile.
 * ------------------------------------------------------------------------------------------------ */
int mt_face_rects(const float* boxes, const int* frame_index, int T, int N, int H, int W, int* rects, unsigned char* valid, int* err,
                  void* stream);
int mt_crop_resize_u8(const unsigned char* src, int64_t src_bytes, int N, int H, int W, const int* rects, const int* frame_index,
                      const unsigned char* valid, const int64_t* crops, int T, int max_w, int OH, int OW, unsigned char* out,
                      int* err, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MTCNN face detector, inference only (csrc/mtcnn.hip): what the reference's FacenetDetector runs in front of everything else,
 * facenet_pytorch's MTCNN(thresholds, margin = 0).detect(frames, landmarks = False) (preprocessing/face_detector.py:38-56), from the
 * uint8 frames [N][H][W][3] to boxes without a host read.  UNCHECKED against the package or a checkpoint: facenet_pytorch is not
 * available where this was written; networks, key names and post-processing are restated by hand from its published source.
 *
 * Records.  Every list holds records of 12 floats: x1 y1 x2 y2 score reg[4] key 0 0 (key: int32 bits).  Lists are segments
 * [segs][cap] of records with a device int32 count per segment; a count above cap means the list overflowed and every reader
 * clamps it.  key = level << 24 | (y Wm + x) names the P-Net map position the box came from.
 * Defined deviations from the package: (a) equal scores in an NMS order are broken by key ascending (the package: an unstable sort);
 * (b) NMS runs per image on the coordinates themselves (torchvision offsets every box by image * (max + 1) first); (c) a stage-2/3
 * window without a pixel (ey <= y - 1 or ex <= x - 1) gets no score and is dropped (the package fails on it); (d) lists have
 * capacities, and an overflow sets a bit of the sticky device word `err` and drops what does not fit, nothing is written outside.
 *
 * area_resize(in -> out), per axis: output cell i averages source indices floor(i in / out) .. ceil((i + 1) in / out) - 1
 *   (F.interpolate(mode = "area")); a pixel is (sum / count - 127.5) * 0.0078125 with an exact integer sum and one fp32 division.
 *
 * mt_mtcnn_pnet: ONE pyramid level of N frames, fused: the level (Hs x Ws = int(H s + 1) x int(W s + 1), at least 12 x 12) is
 *   resampled tile by tile into LDS and P-Net runs on it there -- conv1 3->10 k3, PReLU, MaxPool(2, 2, ceil_mode), conv2 10->16 k3,
 *   PReLU, conv3 16->32 k3, PReLU, conv4_1 (2, softmax, prob = channel 1) and conv4_2 (4 = reg); map Hm = ceil((Hs - 2) / 2) - 4.
 *   One block = 16 x 16 map positions, 256 threads, 59 KB of LDS.  Every output is bias + a chain of fused multiply-adds in
 *   ascending (ky, kx, ci) order: a function of the layer alone, never of N, the tile or the level size; to first order
 *   |y - exact| <= (n + 1) 2^-24 sum |x w| per layer of reduction length n, on top of the error its inputs carry.
 *   weights: 6632 floats -- w1 [3][3][3][10], b1, a1 (PReLU), w2 [3][3][10][16], b2, a2, w3 [3][3][16][32], b3, a3,
 *   w4 [32][6] (conv4_1 then conv4_2), b4 -- i.e. every filter as [ky][kx][ci][co].
 *   A position with prob >= thr is appended to segment n * levels + level of rec (cap records each) through one LDS counter per
 *   block and one integer atomic per block on counts[]; box = floor((2x + 1) / scale), floor((2y + 1) / scale),
 *   floor((2x + 12) / scale), floor((2y + 12) / scale), fp32 with a correctly rounded division.  The append order is not defined;
 *   overflow sets bit 0 of *err.  dbg_level [N][Hs][Ws][3] and dbg_maps [N][5][Hm][Wm] (prob, reg0..3), NULL outside the tests,
 *   additionally receive the level and the maps.  counts are NOT cleared here.
 * mt_mtcnn_nms: greedy NMS of `segs` ragged segments, one wavefront each, cap_in <= 1024.  Rows with score < 0 are dropped first.
 *   Order: score descending, key ascending.  form 0 (torchvision): area = (x2 - x1)(y2 - y1), inter = max(0, xx2 - xx1) max(0, yy2 -
 *   yy1), a box goes when inter / (a_kept + a - inter) > thr.  form 1 (the package's numpy form, method Min): + 1 on every
 *   difference, inter / min(a_kept, a) > thr.  Products and the division are rounded on their own (no fused multiply-add, no
 *   reciprocal), so decisions are those of fp32 CPU arithmetic.  The kept records of segment g are written, in kept order, to
 *   segment g / group of rec_out: group == 1 at its start with count_out[g] = kept; group > 1 appended at
 *   atomicAdd(count_out[g / group], kept), so the caller clears count_out and the order among the group's members is not defined.
 *   What does not fit cap_out is dropped and sets err_bit (a mask) in *err.  picks [segs][cap_in] or NULL: the input rows kept, in
 *   order, then -1.
 * mt_mtcnn_boxes: one thread per record, every operation rounded on its own, in this order.  mode 1 (stage 1): w = x2 - x1,
 *   h = y2 - y1; x1 += r0 w, y1 += r1 h, x2 += r2 w, y2 += r3 h; rerec.  mode 2 (stage 2): the same with w, h + 1 (bbreg); rerec.
 *   mode 3 (stage 3): bbreg, no rerec.  mode 0: nothing.  rerec: l = max(w, h) of the new box; x1 += 0.5 w - 0.5 l, y1 += 0.5 h -
 *   0.5 l, x2 = x1 + l, y2 = y1 + l.  Then, if win [segs][cap][4] int32 is given, pad: truncate toward zero; x = max(x1, 1),
 *   y = max(y1, 1), ex = min(x2, W), ey = min(y2, H), stored as (x, y, ex, ey); rows past the count get zeros.
 * mt_mtcnn_crop: window rows y-1 .. ey-1, columns x-1 .. ex-1 of frame `seg` -> out [N * cap][S][S][4] fp32, area_resize'd and
 *   normalised, 4th channel 0 (the input rows of mt_conv2d_fwd).  Rows past the count and windows without a pixel come out zero.
 * mt_mtcnn_prelu_pool: y = MaxPool(k, s, ceil_mode)(PReLU(x)) of channels-last rows x [rows][H][W][C], one slope per channel,
 *   C % 4 == 0, k in 1..3 (k = 1: PReLU alone).  counts != NULL: row r is skipped unless r % cap < counts[r / cap].
 * mt_mtcnn_score: head [segs * cap][ldh] = logits 0, 1 and reg 0..3 (the two dense heads stacked along K) -> rec: score =
 *   softmax(logits)[1] if it is > thr (strict) and the row's window holds a pixel, else -1; reg.
 * mt_mtcnn_finalize: the per-image lists rec [N][cap] -> boxes [max_faces][4], probs, frame_index (-1 on unused rows), *count,
 *   image_counts [N], image-major; rows that do not fit set err_bit in *err.  N <= 4096.
 * No entry point issues a floating-point atomic.  Nothing is launched or written on an argument error.
 * ------------------------------------------------------------------------------------------------ */
int mt_mtcnn_pnet(const unsigned char* frames, int N, int H, int W, int Hs, int Ws, float scale, int level, int levels,
                  const float* weights, float thr, float* rec, int* counts, int cap, int* err, float* dbg_level, float* dbg_maps,
                  void* stream);
int mt_mtcnn_nms(const float* rec_in, const int* count_in, int segs, int cap_in, int group, int form, float thr, float* rec_out,
                 int* count_out, int cap_out, int* picks, int* err, int err_bit, void* stream);
int mt_mtcnn_boxes(float* rec, const int* counts, int segs, int cap, int mode, int H, int W, int* win, void* stream);
int mt_mtcnn_crop(const unsigned char* frames, int N, int H, int W, const int* win, const int* counts, int cap, int S, float* out,
                  void* stream);
int mt_mtcnn_prelu_pool(const float* x, float* y, const float* slope, int64_t rows, int H, int W, int C, int k, int s, const int* counts,
                        int cap, void* stream);
int mt_mtcnn_score(const float* head, int ldh, float* rec, const int* win, const int* counts, int segs, int cap, int H, int W, float thr,
                   void* stream);
int mt_mtcnn_finalize(const float* rec, const int* counts, int N, int cap, int max_faces, float* boxes, float* probs, int* frame_index,
                      int* count, int* image_counts, int* err, int err_bit, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Launch plans (the caller side of the step: reference train.py:332-378, the Python loop that issues every op).
 * A plan holds the SEQUENCE of entry-point calls of one phase (EfficientNet forward, TimeSformer forward, TimeSformer backward,
 * EfficientNet backward) so that the host issues a phase with one call instead of hundreds through its FFI.
 *   mt_plan_record_begin .. mt_plan_record_end   every call the CALLING THREAD makes in between to an entry point of this header
 *       that takes a `stream` (and to mt_plan_fork) is executed as usual AND appended to the plan with its argument values:
 *       pointers, shapes, scalars, descriptors (copied), the stream.
 *   mt_plan_run     re-issues the recorded calls in order, on the streams they were recorded on.  The caller guarantees what it
 *       guarantees for the calls themselves -- every buffer alive at the recorded address -- and that the recording thread's
 *       stream order is a valid order (cross-stream dependencies are part of the plan through mt_plan_fork).
 *       probe_mask: bit t set = bracket every call tagged t with timing events on its own stream (mt_plan_probe_read).
 *   mt_plan_fork    `to_stream` waits for everything enqueued so far on `from_stream` (event record + wait); recorded when recording.
 *   mt_plan_tag     tags the NEXT recorded call of this thread with tag 1..31 and a work figure (bytes or flops).
 *   mt_plan_probe_read   waits for the probe events of `tag`, returns launches / summed milliseconds / summed work, and clears them.
 *   mt_memset_async / mt_copy_async   hipMemsetAsync / device-to-device hipMemcpyAsync as entry points, so a plan can hold them.
 * A plan is bound to the device that was current at mt_plan_create.  Not thread-safe per plan; different plans are independent.
 * ------------------------------------------------------------------------------------------------ */
typedef struct mt_plan mt_plan;
int mt_plan_create(mt_plan** out);
int mt_plan_destroy(mt_plan* plan);
int mt_plan_record_begin(mt_plan* plan);
int mt_plan_record_end(mt_plan* plan);
int mt_plan_size(const mt_plan* plan);
int mt_plan_tag(int tag, double work);
int mt_plan_fork(void* from_stream, void* to_stream);
int mt_plan_run(mt_plan* plan, unsigned probe_mask);
int mt_plan_probe_read(mt_plan* plan, int tag, int* launches, double* ms, double* work);
int mt_memset_async(void* p, int value, int64_t bytes, void* stream);
int mt_copy_async(void* dst, const void* src, int64_t bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif
