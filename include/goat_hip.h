/*
 * goat_hip.h — C ABI of libgoat_hip.so: hand-written gfx950 (CDNA4) kernels for GOAT's cross-modal
 * transformer forward/backward (VLN-GOAT pre-training / fine-tuning hot path).
 *
 * The reference (CrystalSixone/VLN-GOAT) is pure PyTorch: it has NO native interface for this path
 * (SURVEY.md §2.1).  Each entry point below therefore replaces a *PyTorch eager op sequence* of the
 * reference; the sequence is cited as file:line (P/ = pretrain_src/, M/ = map_nav_src/).  A maintainer
 * binds these with ctypes; `vln-goat_amd/_lib.py` is that binding.
 *
 * Conventions
 *   - plain C, raw device pointers, explicit sizes/strides (in ELEMENTS), no ownership transfer;
 *   - `stream` is a hipStream_t; every call is stream-ordered, never synchronises, never allocates
 *     (hipGraph-capturable);
 *   - dtype: GOAT_F32 = 0 (exact-f32 MFMA path), GOAT_BF16 = 1 (bf16 storage, f32 accumulate);
 *   - parameters (bias, LayerNorm gamma/beta) and statistics are always float32;
 *   - return 0 on success, negative on invalid argument / unsupported shape (GOAT_E_*), or the positive
 *     hipError_t of a failed launch.  No global state except lazily-set kernel attributes.
 */
#ifndef GOAT_HIP_H
#define GOAT_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GOAT_F32 0
#define GOAT_BF16 1

#define GOAT_E_ARG (-1)    /* null pointer / bad enum */
#define GOAT_E_SHAPE (-2)  /* unsupported shape or alignment */

/* epilogues of goat_gemm_nt */
#define GOAT_EPI_NONE 0       /* C = A·Bᵀ (+bias) */
#define GOAT_EPI_GELU 1       /* u = A·Bᵀ+bias ; aux<-u (if aux) ; C = erf-gelu(u)   P/model/Bert_backbone.py:41-47,345-357 */
#define GOAT_EPI_RELU 2       /* same with relu                                   P/model/pretrain_goat.py:32-35 */
#define GOAT_EPI_MUL_DGELU 3  /* C = (A·Bᵀ) * gelu'(aux)   (backward of the GELU epilogue) */
#define GOAT_EPI_MUL_DRELU 4  /* C = (A·Bᵀ) * [aux>0] */
#define GOAT_EPI_ACCUM 5      /* C += A·Bᵀ  (float32 C only, no bias): weight gradients accumulated in place into the
                                flat gradient arena, i.e. autograd's `param.grad += dW` without the temporary */

/* library/version probe: returns 100*major+minor */
int goat_version(void);

/* C[M,N] = epilogue(A[M,K] · B[N,K]ᵀ + bias[N]).  Both operands K-contiguous ("NT"), which is
 * torch.nn.Linear's layout: replaces F.linear / addmm (P/model/Bert_backbone.py:170-172,302,348,362;
 * nn.MultiheadAttention in_proj/out_proj P/model/transformer.py:137; heads P/model/pretrain_goat.py:18-35).
 * Also used for dgrad (B = Wᵀ shadow) and wgrad (A = dYᵀ, B = Xᵀ, split_k>1, out f32).
 *   dtype_in : element type of A, B, aux        dtype_out: element type of C (GOAT_F32 allowed with bf16 in)
 *   K and lda/ldb must be multiples of 16 bytes worth of elements (8 bf16 / 4 f32); bases 16-B aligned.
 *   split_k>1 : K is split over gridDim.y and partial tiles are atomically added into C (requires
 *               dtype_out==GOAT_F32, epilogue NONE, bias NULL; C must hold the value to accumulate onto — also when
 *               K is a single K-tile and nothing is left to split: a split_k>1 launch always ADDS into C).
 */
int goat_gemm_nt(void* stream, int dtype_in, int dtype_out,
                 const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                 int M, int N, int K, const float* bias, int epilogue,
                 void* aux, int64_t ldaux, int split_k);

#define GOAT_GEMM_8WAVES 0x100   /* flag in goat_gemm_bf16's nstage argument: run the 128-row tile with eight waves */
#define GOAT_GEMM_PP 0x200       /* flag in nstage: the "ping-pong" main loop (csrc/gemm5_tile.hpp) — two groups of four waves half a
                                    K-tile out of phase, one feeding the matrix pipe while the other loads; tiles 256x256, 192x256 (K-contiguous
                                    A only), 128x256, 256x128, 128x128, nstage 2; same operands, epilogues and (bit-identical) results */
#define GOAT_GEMM_PERSIST 0x400  /* flag in nstage, with GOAT_GEMM_PP: one workgroup per CU walks the tiles of its XCD's chunk and requests the next
                                    tile's first K-tile before the current tile's epilogue (bf16 results, unsplit, K-contiguous A; bit-identical
                                    results; pays when the problem has more tiles than the chip has CUs, e.g. per-rank batch 256) */

/* Pipelined bf16 GEMM with direct-to-LDS (LDS-DMA) operand staging, all operand layouts (csrc/gemm2.hip):
 *   C[M,N] = epilogue( op(A) · op(B)ᵀ + bias ),  contraction length Kc
 *   trans_a=0: A is [M,Kc] (Kc contiguous) ; trans_a=1: A is [Kc,M] (M contiguous)   (same for B with N)
 *   (0,0) forward y = x·Wᵀ  (F.linear) ; (0,1) dgrad dx = dy·W ; (1,1) wgrad dW = dyᵀ·x  — the autograd of
 *   every nn.Linear on the path (P/model/Bert_backbone.py:170-172,302,348,362; P/model/transformer.py:137-140).
 * bf16 inputs; dtype_out GOAT_BF16 or GOAT_F32 (F32 only with GOAT_EPI_NONE); the activation-derivative epilogues take no bias.  K-contiguous operands need
 * Kc % 64 == 0 (transposed operands: any Kc, the tail is zero-filled by the buffer bounds check); lda/ldb
 * multiples of 8, bases 16-B aligned, each operand < 2 GiB.  split_k>1: f32 atomic accumulation into C (split_k is clamped to the
 * number of K-tiles; with one K-tile the launch runs unsplit and still adds into C).
 * bm: 64, 128 (four waves) or 256 (eight waves sharing one B tile: 25 % fewer L2->LDS bytes per flop, nstage <= 3; for
 * M >= 2048) — the M-tile; 64 fills the chip on small-M problems.  bm 128 with nstage | GOAT_GEMM_8WAVES: the 128-row tile
 * on eight waves (32x64 wave patches; twice the waves issue the tile's LDS-DMA).  nstage: 2..4 LDS ring stages (2 = most
 * workgroups per CU, 3-4 = deeper prefetch for long/cold contractions).
 * colsum (trans_a only, may be NULL): colsum[m] += sum_k A[k,m] (float32, atomic; caller zero-fills) — the bias
 * gradient of the Linear, accumulated from the A fragments the wgrad already holds in registers. */
int goat_gemm_bf16(void* stream, int trans_a, int trans_b, int dtype_out,
                   const void* A, int64_t lda, const void* B, int64_t ldb, void* C, int64_t ldc,
                   int M, int N, int Kc, const float* bias, int epilogue,
                   void* aux, int64_t ldaux, int split_k, int bm, int nstage, float* colsum);
/* Does this build have that configuration?  0, or GOAT_E_ARG where goat_gemm_bf16 would refuse the same seven arguments whatever the
 * operands (tile = its bm argument).  The lookup goat_gemm_bf16 itself performs before it launches; takes no pointer, touches no device. */
int goat_gemm_bf16_query(int trans_a, int trans_b, int dtype_out, int epilogue, int split_k, int tile, int nstage);
/* colsum[c] += sum_r x[r,c] (float32, atomic; caller zero-fills): bias gradient of a Linear. */
int goat_colsum(void* stream, int dtype, const void* x, int64_t ld, int R, int C, float* colsum);

/* Weight (and bias) gradient of a Linear with K <= 16 input features — the 7- / 14-wide position Linears
 * (P/model/vilmodel_goat.py:300-303,406,475): dw[n, k] += sum_r dy[r, n] x[r, k], dbias[n] += sum_r dy[r, n] (dbias may be NULL).
 * dy [rows, N] and x [rows, ld_x] in `dtype`, row strides in elements; x rows padded to whole 16-byte chunks and 16-byte aligned; dw float32 [N, K] with row stride ld_dw; both outputs are
 * ADDED to (float atomics: gradient-arena slices cleared at step start, or zero-filled by the caller). */
int goat_wgrad_smallk(void* stream, int dtype, const void* dy, int64_t ld_dy, const void* x, int64_t ld_x, int rows, int N, int K,
                      float* dw, int64_t ld_dw, float* dbias);

/* out[c, r] = in[r, c] for r<R, c<C; out columns R..ld_out-1 are zero-filled (so the result can feed
 * goat_gemm_nt as a K-padded operand).  If colsum!=NULL, colsum[c] += sum_r in[r,c] (float32, atomic):
 * that is the bias gradient of a Linear (autograd of P/model/Bert_backbone.py:302 et al.). */
int goat_transpose(void* stream, int dtype, const void* in, int64_t ld_in, void* out, int64_t ld_out,
                   int R, int C, float* colsum);

/* z = residual + dropout_p(x) ; y = LayerNorm(z)*gamma+beta.   BertSelfOutput/BertOutput
 * (P/model/Bert_backbone.py:306-310,366-370), RobertaEmbeddings LN (:115-116), pre-LN norms
 * (P/model/transformer.py:174,178).  residual may be NULL; p may be 0.  z_out may be NULL when
 * residual==NULL and p==0 (then z==x).  mean/rstd: float32[M] saved for backward.
 * Dropout keep-mask for flat element index i is hash(seed + *rng_dev, offset+i) (see csrc/common.hpp);
 * rng_dev (device uint64, may be NULL) lets a captured hipGraph draw fresh masks on every replay. */
int goat_ln_fwd(void* stream, int dtype, const void* x, const void* residual,
                const float* gamma, const float* beta, float eps,
                float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev,
                void* y, void* z_out, float* mean, float* rstd, int M, int H);

/* backward of goat_ln_fwd.  dz = LN-backward(dy + dy2) ; d_res<-dz (if non-NULL) ; dx<-dz*mask/(1-p) (if non-NULL).
 * dy2 (may be NULL): a second upstream gradient of y, summed on load.  In the post-LN blocks y feeds both the next
 * sub-layer's first Linear and the next LayerNorm's residual input; the two gradients arrive separately
 * (hipops.layer_norm(fork=True)) and autograd's add kernel between them is not needed.
 * dgamma/dbeta: float32[H], overwritten (accumulate=0) or added to (accumulate=1: gradient-arena slices).
 * ws == NULL (default): every block adds its column partials to dgamma / dbeta with float atomics — one launch, summation
 *   order not reproducible (accumulate=0 clears the two vectors with a memset node first).
 * ws != NULL: float32 scratch of goat_ln_bwd_ws_floats(H) elements for per-block column partials; a second tiny kernel
 *   reduces them — no atomics, deterministic (round-1 behaviour: 43 extra launches per pre-training step).
 * accumulate == 2 (ws required, goat_ln_bwd_nparts(M) * 2 * H floats): the per-block partials are LEFT in ws and nothing is
 *   written to dgamma / dbeta; the caller sums the partials of many LayerNorm calls into their gradient vectors with ONE
 *   goat_ln_reduce_batched launch when the backward pass ends (the column reduction is 40 % of this kernel's time at the GOAT
 *   row counts; deterministic).
 * dx_add (may be NULL; same shape / dtype as dx): added to dx on store — the gradient that reaches the LayerNorm's INPUT through
 *   its other consumer (the skip connection around a pre-LN sub-layer, P/model/transformer.py:170-182), so autograd launches no
 *   add kernel for that junction (hipops.layer_norm(fork_in=True)).
 *   accumulate | GOAT_LN_ADD_BEFORE: dx_add is instead the gradient that reaches the PRE-NORM SUM z = residual + dropout(x) through
 *   its other consumer and joins before the residual / dropout split: d_res <- dz + dx_add, dx <- (dz + dx_add) * mask / (1 - p).
 *   With it one goat_ln_fwd / goat_ln_bwd pair serves "src = skip + dropout(a); n = LayerNorm(src)" of a pre-LN block, where src
 *   itself continues as the next skip connection (hipops.layer_norm(z_out=True)).
 * Kernels: bf16 rows of H = 768 (every LayerNorm of the model at its hidden size) run ln_bwd768_kernel (round 6: 8-byte chunks, rows in
 *   flight packed as bf16, <= 128 VGPRs); other widths and float32 run the generic ln_bwd_kernel.  Same grid, same partial rows
 *   (goat_ln_bwd_nparts), same semantics; GOAT_LN_BWD_GENERIC=1 in the environment selects the generic kernel everywhere (A/B, tests). */
#define GOAT_LN_ADD_BEFORE 4
typedef struct goat_ln_partial {
  const float* ws;         /* partials written by goat_ln_bwd(..., accumulate = 2): [nparts][2][H] float32 */
  float* dgamma;           /* float32[H], ADDED to */
  float* dbeta;
  int32_t nparts;          /* goat_ln_bwd_nparts(M) of that call */
  int32_t reserved;
} goat_ln_partial;
int goat_ln_bwd_ws_floats(int H);
int goat_ln_bwd_nparts(int M);
/* entries with the same dgamma (a LayerNorm applied several times in one backward pass) must share dbeta; they are summed by one
 * writer in call order. */
int goat_ln_reduce_batched(void* stream, const goat_ln_partial* entries, int n, int H);
int goat_ln_bwd(void* stream, int dtype, const void* dy, const void* dy2, const void* z,
                const float* gamma, const float* mean, const float* rstd,
                float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev,
                void* dx, void* d_res, float* dgamma, float* dbeta, float* ws, int M, int H, int accumulate,
                const void* dx_add);
/* The same pair with dropout on the LayerNorm's OUTPUT as well: y = dropout_{p_out}(LayerNorm(z)) (the embedding blocks,
 * P/model/Bert_backbone.py:108-110, P/model/vilmodel_goat.py:228-237: `dropout(layer_norm(x))`), mask from counter offset_out of the
 * same seed; the backward masks dy (+ dy2) the same way before anything else.  post_add (may be NULL; shape / dtype of y): a second
 * summand behind the norm, y = dropout_{p_out}(LayerNorm(z) + post_add) — the image embedding block's normalised view features plus
 * normalised location features (P/model/vilmodel_goat.py:340-344); its gradient (the masked dy) is written to d_post.
 * p_out == 0 and post_add == NULL: exactly goat_ln_fwd / goat_ln_bwd. */
int goat_ln_fwd_do(void* stream, int dtype, const void* x, const void* residual, const float* gamma, const float* beta, float eps,
                   float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev, void* y, void* z_out, float* mean, float* rstd,
                   int M, int H, float p_out, uint64_t offset_out, const void* post_add);
int goat_ln_bwd_do(void* stream, int dtype, const void* dy, const void* dy2, const void* z, const float* gamma, const float* mean,
                   const float* rstd, float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev, void* dx, void* d_res,
                   float* dgamma, float* dbeta, float* ws, int M, int H, int accumulate, const void* dx_add, float p_out,
                   uint64_t offset_out, void* d_post);

/* y = residual + dropout_p(x)  (residual may be NULL, y may alias x).  nn.Dropout + pre-LN residual adds
 * (P/model/transformer.py:177,181; P/model/vilmodel_goat.py:316). n = element count. */
int goat_dropout_add_fwd(void* stream, int dtype, const void* x, const void* residual, void* y,
                         int64_t n, float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev);
/* dx = dy * mask/(1-p) with the same (seed, offset). */
int goat_dropout_bwd(void* stream, int dtype, const void* dy, void* dx,
                     int64_t n, float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev);

/* dx = dropmask_p(dy) * act'(u), act = GOAT_EPI_GELU | GOAT_EPI_RELU: backward of h = dropout_p(act(u)),
 * the inner activation (+dropout) of the panorama encoder FFN (P/model/transformer.py:179) and of the small heads. */
int goat_act_bwd(void* stream, int dtype, const void* dy, const void* u, void* dx, int64_t n, int act,
                 float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev);

/* Masked multi-head attention, head_dim fixed at 64.
 *   O[b,q,h,:] = dropout_p(softmax_k(scale * Q[b,q,h,:]·K[b,k,h,:] + kmask[b,k] + bias[b,q,k])) · V[b,k,h,:]
 * Replaces BertSelfAttention.forward (P/model/Bert_backbone.py:246-290; additive -10000 masks P/model/ops.py:25-34,
 * graph_sprels bias :690-691) and F.multi_head_attention_forward with key_padding_mask (-inf)
 * (P/model/transformer.py:172-176).  Q/K/V/O are [B, L, nh*64] views with explicit row and batch strides
 * (so q,k,v may be slices of one fused QKV projection, or — round 6 — K|V columns of a projection BANK that holds every layer's
 * cross-attention K|V of one attended sequence: row stride n_layers * 2 * nh * 64; hipops.linear_bank).  kmask: float32 [B,Lk] additive or NULL;
 * bias: float32 [B,Lq,Lk] additive or NULL.  lse: float32 [B,nh,Lq] saved for backward.
 * Lk <= 256.  Rows whose keys are all -inf produce zeros.
 * Dropout bits are a function of (seed + *rng_dev, offset, b, h, q, key) and of the dtype only — never of which kernel family
 * (LDS-staged / streaming) served the call — so goat_attn_bwd regenerates goat_attn_fwd's mask for every shape. */
int goat_attn_fwd(void* stream, int dtype,
                  const void* Q, int64_t q_rs, int64_t q_bs,
                  const void* K, int64_t k_rs, int64_t k_bs,
                  const void* V, int64_t v_rs, int64_t v_bs,
                  void* O, int64_t o_rs, int64_t o_bs,
                  const float* kmask, const float* bias, float* lse,
                  int B, int nh, int Lq, int Lk, float scale,
                  float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev);

/* backward of goat_attn_fwd.  dQ/dK/dV share the stride convention; dbias: float32 [B,Lq,Lk] or NULL,
 * ACCUMULATED (atomic; caller zero-fills) with the sum over heads of dS (the gradient of `bias`; feeds sprel_linear's 1->1 Linear,
 * P/model/vilmodel_goat.py:496-497). */
int goat_attn_bwd(void* stream, int dtype,
                  const void* Q, int64_t q_rs, int64_t q_bs,
                  const void* K, int64_t k_rs, int64_t k_bs,
                  const void* V, int64_t v_rs, int64_t v_bs,
                  const void* O, int64_t o_rs, int64_t o_bs,
                  const void* dO, int64_t do_rs, int64_t do_bs,
                  void* dQ, int64_t dq_rs, int64_t dq_bs,
                  void* dK, int64_t dk_rs, int64_t dk_bs,
                  void* dV, int64_t dv_rs, int64_t dv_bs,
                  const float* kmask, const float* bias, const float* lse, float* dbias,
                  int B, int nh, int Lq, int Lk, float scale,
                  float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev);

/* goat_attn_fwd / goat_attn_bwd for 1 <= Lk <= 512 (RxR-length instructions: max_txt_len 300, at most max_position_embeddings - 2 = 512
 * tokens): same arguments, same meaning of every output, same dropout bits.  The forward streams the keys in tiles of 32 with a running
 * row maximum / row sum (csrc/attention_long.hip) instead of holding the score row-block in registers; the backward runs goat_attn_bwd's
 * general dQ and dK|dV kernels with all K rows in LDS.  GOAT_E_SHAPE for Lk > 512 or a stride / base that is not 16-byte aligned
 * (O included: the output rows are written in 4-element vectors).  goat_attn_fwd / goat_attn_bwd keep their Lk <= 256 contract. */
int goat_attn_long_fwd(void* stream, int dtype,
                       const void* Q, int64_t q_rs, int64_t q_bs,
                       const void* K, int64_t k_rs, int64_t k_bs,
                       const void* V, int64_t v_rs, int64_t v_bs,
                       void* O, int64_t o_rs, int64_t o_bs,
                       const float* kmask, const float* bias, float* lse,
                       int B, int nh, int Lq, int Lk, float scale,
                       float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev);
int goat_attn_long_bwd(void* stream, int dtype,
                       const void* Q, int64_t q_rs, int64_t q_bs,
                       const void* K, int64_t k_rs, int64_t k_bs,
                       const void* V, int64_t v_rs, int64_t v_bs,
                       const void* O, int64_t o_rs, int64_t o_bs,
                       const void* dO, int64_t do_rs, int64_t do_bs,
                       void* dQ, int64_t dq_rs, int64_t dq_bs,
                       void* dK, int64_t dk_rs, int64_t dk_bs,
                       void* dV, int64_t dv_rs, int64_t dv_bs,
                       const float* kmask, const float* bias, const float* lse, float* dbias,
                       int B, int nh, int Lq, int Lk, float scale,
                       float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev);

/* One step of KV-cached decoding (csrc/decode.hip): the speaker's word-by-word loop (M/r2r/transpeaker.py:292-322, which re-runs the
 * decoder of M/models/transpeaker_model.py:200-230 over the whole prefix for every word) as a fixed-shape computation whose position
 * lives in DEVICE memory, so that one captured hipGraph serves every step.
 *
 * goat_attn_decode_fwd: cache append + single-query attention, head_dim 64.  Let t = *pos_dev.  KVnew[b] (this step's K|V projection
 * row, [B, 2*nh*64], dense) is copied into cache[b, t]; then
 *   O[b,h,:] = dropout_p(softmax_{k<=t}(scale * Q[b,h,:]·K[b,k,h,:] + kmask[b,k])) · V[b,k,h,:]
 * Q, O: [B, nh*64] dense.  cache: [B, Lmax, 2*nh*64] as K|V columns (K of head h at column h*64, V at nh*64 + h*64) with row stride
 * c_rs and batch stride c_bs in elements.  kmask: float32 [B, Lmax] additive or NULL.  Keys k > t are never read: the cache tail (and
 * the kmask tail) may hold anything, NaN included.  A row whose visible keys all carry -1e9 comes out uniform over the t+1 visible keys
 * (the reference's masked_fill(-1e9) before the softmax, M/models/transpeaker_model.py:91-119); all -inf gives zeros.
 * Dropout bits are a function of (seed + *rng_dev, offset, b, h, key) only (HeadRng of csrc/common.hpp), the same for both dtypes.
 * 1 <= Lmax <= 512.  GOAT_E_SHAPE: Lmax outside that range, c_rs / c_bs not a multiple of the 16-byte chunk (4 f32 / 8 bf16 elements),
 * c_rs < 2*nh*64, or a base pointer that is not 16-byte aligned.  GOAT_E_ARG: null Q / KVnew / cache / O / pos_dev, bad dtype, p outside
 * [0, 1).  A t outside [0, Lmax) read on the device makes every workgroup return without touching memory. */
int goat_attn_decode_fwd(void* stream, int dtype, const void* Q, const void* KVnew,
                         void* cache, int64_t c_rs, int64_t c_bs, void* O,
                         const float* kmask, const int32_t* pos_dev,
                         int B, int nh, int Lmax, float scale,
                         float p, uint64_t seed, uint64_t offset, const uint64_t* rng_dev);

/* goat_decode_select: the next word of every row and the loop state in one launch — the logits[:, unk] = -inf, argmax / Categorical
 * sample, pad-after-<EOS> and `ended` bookkeeping of M/r2r/transpeaker.py:303-322.  logits: float32 [B, ld], V <= ld valid columns.
 * Let t = *pos_dev.  Per row: the column `unk` is never chosen; greedy (sampling == 0) takes the arg-max, a tie going to the LOWEST
 * index (NaN counts as -inf); sampling != 0 draws from softmax(logits) by Gumbel-max over the counter hash of csrc/common.hpp, a
 * function of (seed + *rng_dev, offset, b, column); a row with ended[b] != 0 gets `pad`.  The word goes to words[b, t+1]
 * (int64 [B, Lmax]); kmask[b, t+1] (float32 [B, Lmax]) becomes -1e9 if the word is `pad`, else 0; a row that emits `eos` gets
 * ended[b] = 1 and end_step[b] = t.  Then *pos_dev = t + 1 and *n_live = the number of rows not yet ended.  A t outside [0, Lmax - 1)
 * read on the device: nothing is touched.  GOAT_E_ARG: a null pointer (rng_dev may be NULL); GOAT_E_SHAPE: V < 2, ld < V, Lmax < 2. */
int goat_decode_select(void* stream, const float* logits, int64_t ld, int B, int V, int Lmax,
                       int unk, int eos, int pad, int sampling,
                       uint64_t seed, uint64_t offset, const uint64_t* rng_dev,
                       int32_t* pos_dev, int64_t* words, float* kmask, uint8_t* ended, int32_t* end_step, int32_t* n_live);

/* Back-translation on the device (csrc/backtrans.hip): the self-training rollout of M/r2r/agent.py:457-474 (driven by
 * M/r2r/main_nav.py:194-249 under --use_transpeaker) between the speaker's decode loop and the agent's walk.
 *
 * goat_retok_rows: decoded speaker words -> the agent's padded txt_ids / txt_masks rows; one workgroup per row, integers only.  What the
 * reference does on the host per sentence: speaker.tok.shrink (M/utils/data.py:373-398), decode_sentence (:362-371), the agent's
 * tokenizer on the joined string, `[:max_instr_len]` (M/r2r/agent.py:934) and the zero padding of _language_variable (:38-65).
 *   words      int64 [B, ldw] (DecodeState.words: columns behind the newest word hold `pad`).
 *   width      >= 2: that many columns of every row.  0: derived from the decode state as speaker.infer_batch_cached cuts its result,
 *              *n_live > 0 ? *pos_dev + 1 : max_b(ended[b] ? end_step[b] : -1) + 2; every workgroup forms the maximum itself.  ended
 *              uint8 [B], end_step int32 [B], pos_dev / n_live int32 [1] are read only then and may be NULL otherwise.
 *   per row    (1) shrink: w[i] is kept for i < width - 1 where w[i] != w[i + 1] — the last column is always dropped, a run collapses to
 *              its last element, a trailing run disappears; (2) end = index of the first `eos` among the kept words, or their number if
 *              that index is 0 (none, or `eos` first); (3) start = 1 if more than one word is kept and the first is `bos`, else 0;
 *              (4) the sentence is kept[start:end] up to the first `pad`; (5) word j expands to ids[start_tab[w] .. start_tab[w + 1]) of the
 *              `first_*` table for the sentence-initial word and of the `rest_*` table for every later one (a byte-level BPE encodes
 *              "walk" and " walk" differently; a word may expand to nothing); int32 CSR arrays, V + 1 starts each;
 *              (6) out_ids[b] = ([agent_bos] + ids + [agent_eos])[:max_len], then fill_id up to ldo; out_mask[b, j] = j < lens[b] (one
 *              byte per slot, the layout of a bool tensor); lens[b] = min(max_len, 2 + number of ids).
 *   status     int32 [B], written by every launch: 0, or GOAT_RETOK_E_WIDTH (the width, given or derived, is < 2 or > ldw — the
 *              reference raises on a one-column row), GOAT_RETOK_E_WORD (a word of the first `width` columns outside [0, V)),
 *              GOAT_RETOK_E_EMPTY (the whole row is one run, nothing is kept: the reference's np.argmax raises on the empty list).  Such
 *              a row gets lens 0, fill_id everywhere and a zero mask.
 * GOAT_E_ARG: a null pointer (the four state pointers only with width == 0).  GOAT_E_SHAPE: ldw outside 1..512, width outside 0..512,
 * max_len outside 2..512 or > ldo, B outside 1..1024, V < 1.  Both are returned before any launch. */
#define GOAT_RETOK_E_WIDTH 1
#define GOAT_RETOK_E_WORD 2
#define GOAT_RETOK_E_EMPTY 4
int goat_retok_rows(void* stream, const int64_t* words, int64_t ldw, const uint8_t* ended, const int32_t* end_step,
                    const int32_t* pos_dev, const int32_t* n_live, int width, int B, int V, int bos, int eos, int pad,
                    const int32_t* first_start, const int32_t* first_ids, const int32_t* rest_start, const int32_t* rest_ids,
                    int agent_bos, int agent_eos, int64_t fill_id, int max_len, int64_t* out_ids, uint8_t* out_mask,
                    int64_t ldo, int32_t* lens, int32_t* status);

/* goat_scale_cols: out[r, c] = x[r, c] * noise[c] for c < D over `rows` rows of leading dimension ld (GOAT_F32 / GOAT_BF16; noise is
 * float32 [D]): the shared environment-dropout mask `noise = drop_env(ones(feature_size))` of M/r2r/agent.py:459 multiplied into the
 * image columns of the speaker's inputs (M/r2r/transpeaker.py:272-278) and into every view feature of the agent's panoramas
 * (M/r2r/agent.py:86-148,541).  One float32 multiply per element, rounded once to the storage type.  Columns D..ld-1 are not touched
 * when out == x and copied bit for bit otherwise.  16-byte chunks when x, out and noise are 16-byte aligned and ld is a multiple of the
 * chunk (4 f32 / 8 bf16 elements), single elements otherwise; D needs no alignment.  x and out either coincide or do not overlap.
 * GOAT_E_ARG: a null pointer, a bad dtype; GOAT_E_SHAPE: rows < 1, D < 1, ld < D, a base that is not element-aligned. */
int goat_scale_cols(void* stream, int dtype, const void* x, void* out, const float* noise, int64_t rows, int64_t ld, int D);

/* k-means over the pooled front-door features and the draw of the FACL dictionaries (csrc/kmeans.hip): what M/utils/data.py:403-480
 * (KMeansPicker: sklearn KMeans per modality, np.random.choice per cluster) does on the host.  Shared limits: X is [N, ld_x] in
 * GOAT_F32 or GOAT_BF16 with N >= 1, D a multiple of 8 (>= 8), ld_x >= D, 16-byte aligned rows; 1 <= K <= 256; C is float32 [K, D],
 * contiguous and 16-byte aligned.  GOAT_E_ARG: a null pointer that is not marked nullable, or a bad dtype; GOAT_E_SHAPE: the rest.
 *
 * goat_kmeans_assign: labels[i] = argmin_k (||c_k||² - 2 x_i·c_k), a tie going to the LOWEST k, a NaN score counting as +inf;
 * mind2[i] (nullable) = max(0, ||x_i||² + that minimum); *changed (nullable) += the number of rows whose new label differs from what
 * labels[i] held before the write.  All arithmetic is float32 (f32-input MFMA; bf16 rows are promoted, nothing is rounded to bf16). */
int goat_kmeans_assign(void* stream, int dtype, const void* X, int64_t ld_x, const float* C,
                       int32_t* labels, float* mind2, int32_t* changed, int N, int D, int K);

/* goat_kmeans_csr: labels int32 [N] -> start int32 [K+1] (prefix sums of the cluster sizes) and order int32 [N] (row indices grouped
 * by cluster, ascending inside each cluster: a stable counting sort).  A label outside [0, K) is skipped: start[K] < N then and the
 * tail of `order` is not written. */
int goat_kmeans_csr(void* stream, const int32_t* labels, int32_t* start, int32_t* order, int N, int K);

/* goat_kmeans_centres: C[k] = mean of the rows X[order[start[k] .. start[k+1])], float32 accumulation in an order that depends on
 * (order, start) alone (no atomics: two runs give the same bits).  The row of an empty cluster is left untouched. */
int goat_kmeans_centres(void* stream, int dtype, const void* X, int64_t ld_x, const int32_t* order, const int32_t* start,
                        float* C, int N, int D, int K);

/* goat_kmeans_pick: picked[k] = order[start[k] + floor(u_k * n_k)], n_k = start[k+1] - start[k], u_k = h / 2^32 with h the 32 bits
 * the counter hash of csrc/common.hpp gives for (seed + *rng_dev, offset + k) (rng_dev nullable), taken by multiply-high;
 * out[b, k, :] = X[picked[k], :] for every b < B (out: [B, K, D] contiguous, the dtype of X, 16-byte aligned).  An empty cluster gives
 * picked[k] = -1 and zero rows. */
int goat_kmeans_pick(void* stream, int dtype, const void* X, int64_t ld_x, const int32_t* order, const int32_t* start,
                     void* out, int32_t* picked, int N, int D, int K, int B,
                     uint64_t seed, uint64_t offset, const uint64_t* rng_dev);

/* Running per-slot means of picked rows: the BACL dictionaries (csrc/zdict.hip), what M/r2r/agent.py:713-848 (update_z_dict) and
 * M/do_utils/do_intervention.py:109-148 do with per-row numpy appends and np.mean on the host.  The state is sum / comp float32 [K, D]
 * and count int32 [K], all zero at the start; 1 <= K <= 65535, D a multiple of 8 (>= 8), sum / comp 16-byte aligned.
 * GOAT_E_ARG: a null pointer that is not marked nullable, or a bad dtype; GOAT_E_SHAPE: the rest.
 *
 * goat_dict_accumulate: X is [R, ld_x] in GOAT_F32 or GOAT_BF16 (R >= 1, ld_x >= D and a multiple of the 16-byte chunk, 16-byte
 * aligned base); rows int32 [P] (P >= 1) are row indices into X grouped by slot, slot k owning rows[start[k] .. start[k+1]) with
 * start int32 [K+1].  The rows of a slot are added in float32 in pieces of at most 64 rows and every piece sum is folded into the
 * pair (sum[k], comp[k]) with a compensated (two-sum) step, so that sum + comp stays accurate over any number of launches; count[k]
 * grows by the number of rows used.  A row index outside [0, R) adds nothing and is not counted; a slot without rows in this launch
 * keeps its pair and its count bit for bit.  No atomics: one writer per (slot, column), the order of the additions depends on the
 * arguments alone. */
int goat_dict_accumulate(void* stream, int dtype, const void* X, int64_t ld_x, int64_t R,
                         const int32_t* rows, const int32_t* start,
                         float* sum, float* comp, int32_t* count, int P, int D, int K);

/* goat_dict_finish: feats[k] = (sum[k] + comp[k]) / count[k] (float32 [K, D], nullable); the same values converted to out_dtype in
 * every out[b, k, :] (out: [B, K, D], nullable); out_pz[b, k] = count[k] / sum of all counts, formed on the device in float64 and
 * rounded once to float32, then to out_dtype (out_pz: [B, K], nullable).  A slot with count 0 gives zeros.  feats and out are 16-byte
 * aligned; B >= 1.  With all three outputs NULL nothing is launched. */
int goat_dict_finish(void* stream, int out_dtype, const float* sum, const float* comp, const int32_t* count,
                     float* feats, void* out, void* out_pz, int B, int D, int K);

/* Softmax cross-entropy (reduction none) on float32 logits [M, ld] with N valid columns (ld >= N may be padded):
 * loss[m] = logsumexp(logits[m,:N]) - logits[m,target[m]], lse saved.  Replaces F.cross_entropy on the 576 x 50265
 * MLM scores (P/model/pretrain_goat.py:213-215).  Backward writes dlogits (GOAT_BF16 or GOAT_F32) with row stride
 * ld_out, zeros in the padding columns [N, ld_out), ready to be the K-padded operand of the decoder's dgrad/wgrad.
 * A negative target marks an ignored row (loss 0, zero gradient): the padding rows of a shape-bucketed static batch.
 * A target >= N (compared as the int64 it is, in both directions) gives a NaN loss and NaN in dlogits[m, :N]; nothing is read out of
 * bounds. */
int goat_ce_fwd(void* stream, const float* logits, int64_t ld, int M, int N, const int64_t* targets,
                float* loss, float* lse);
int goat_ce_bwd(void* stream, int dtype_out, const float* logits, int64_t ld, int M, int N,
                const int64_t* targets, const float* lse, const float* dloss, void* dlogits, int64_t ld_out);

/* Adaptive panorama fusion: w = softmax_v(tanh(x[n,v,:]·a + a0)) over ALL V slots (no mask);
 * fused[n,:] = sum_v w_v x[n,v,:]    (P/model/vilmodel_goat.py:354-361).  a: float32[H], a0: float32[1].
 * wsave: float32 [N,V] softmax weights saved for backward. */
int goat_pano_fusion_fwd(void* stream, int dtype, const void* x, const float* a, const float* a0,
                         void* fused, float* wsave, int N, int V, int H);
/* backward: dx (overwritten), da/da0 float32 accumulated atomically. */
int goat_pano_fusion_bwd(void* stream, int dtype, const void* x, const float* a, const float* a0,
                         const float* wsave, const void* dfused, void* dx, float* da, float* da0,
                         int N, int V, int H);

/* Row gather / segment mean:  out[i,:] = scale[i] * sum_{j in [start[i],start[i+1])} src[idx[j],:]
 * (idx = -1 contributes zero).  One launch replaces the host triple loop of
 * GlobalMapEncoder._aggregate_gmap_features (P/model/vilmodel_goat.py:438-460), the [stop]-token
 * concat/pad of vp_input_embedding (:377-391) and pad_tensors_wgrad (P/model/ops.py:46-68).
 * idx/start are int32 device arrays built once per batch on the host from the string ids.
 * tok_w (may be NULL): a weight per index entry, out[i] = scale[i] * sum_j tok_w[j] src[idx[j]].  With the INVERSE index of a
 * gather (graphmap.inverse_index: for every source row the segments that read it, tok_w = their scales) this same entry point is
 * the gather's backward pass — one writer per row, results in the activation dtype, no zero fill / atomics / cast. */
int goat_gather_segmean_fwd(void* stream, int dtype, const void* src, int64_t src_rows,
                            const int32_t* idx, const int32_t* start, const float* scale,
                            void* out, int n_out, int H, const float* tok_w);
/* backward: dsrc[idx[j],:] += scale[i]*dout[i,:]  (float atomics into float32 dsrc32 [src_rows,H]). */
int goat_gather_segmean_bwd(void* stream, int dtype, const void* dout,
                            const int32_t* idx, const int32_t* start, const float* scale,
                            float* dsrc32, int n_out, int H);

/* Grouped weight gradients: n <= 48 independent problems dW_i[n_out,n_in] (float32) = dY_i[rows,n_out]^T · X_i[rows,n_in]
 * (bf16 operands, any row count — the contraction tail is zero-filled) in ONE launch of the goat_gemm_bf16 tile
 * kernel, unsplit.  The autograd of the several nn.Linear of a transformer block (P/model/Bert_backbone.py:170-172,302,
 * 348,362) produces weight gradients of 36-144 tiles each; together they fill the 256 CUs without the split-K atomics
 * and zero fills a single small problem needs.  accumulate != 0: dW += ...; dbias (may be NULL): float32 [n_out],
 * += column sums of dY (atomic; the caller clears it).  ld_* in elements; ld_dy, ld_x multiples of 8, bases 16-B aligned.
 * bm 64 | 128, nstage 2..4 (| GOAT_GEMM_8WAVES with bm 128) as in goat_gemm_bf16. */
typedef struct goat_wgrad_problem {
  const void* dy; int64_t ld_dy;
  const void* x; int64_t ld_x;
  float* dw; int64_t ld_dw;
  float* dbias;
  int rows, n_out, n_in;
  int accumulate;
} goat_wgrad_problem;
int goat_wgrad_grouped(void* stream, const goat_wgrad_problem* probs, int n, int bm, int nstage);
/* Contraction-balanced form of the same launch (round 5).  goat_wgrad_grouped gives every output tile a workgroup, so a group is
 * whole rounds of tiles over the CUs plus a tail, and a group that mixes contraction lengths (panorama rows beside text rows) ends
 * with most CUs idle.  Here ONE workgroup per CU takes an equal, contiguous share of the group's K-tile iterations; a tile cut by a
 * share boundary is summed through `workspace` in a fixed order (deterministic; differs from goat_wgrad_grouped by float32
 * summation order only).  Ping-pong tiles only: bm = 256 | 256 << 16, 128 | 256 << 16, 256 | 128 << 16 (as goat_wgrad_grouped's bm).
 * workspace: goat_wgrad_balanced_ws_bytes(bm) bytes, 256-byte aligned, ZEROED once by the caller before the first launch (the kernel
 * leaves its flags zero), and not shared by launches that may run concurrently (one per stream).  GOAT_E_SHAPE when the group has
 * fewer K-tile iterations than the device has CUs (use goat_wgrad_grouped). */
int goat_wgrad_grouped_balanced(void* stream, const goat_wgrad_problem* probs, int n, int bm, void* workspace,
                                int64_t workspace_bytes);
int goat_wgrad_balanced_ws_bytes(int bm);   /* < 0: bm is not one of the tiles above */
/* 0, or GOAT_E_ARG where goat_wgrad_grouped would refuse (bm, nstage) whatever the problems: its own lookup, no pointer, no device. */
int goat_wgrad_grouped_query(int tile, int nstage);

/* Embedding tables (float32 masters):  out[r,:] = word[ids[r],:] + type[type_ids ? type_ids[r] : 0,:] + pos[r % L,:]
 * cast to `dtype` — the three nn.Embedding lookups and two adds of BertEmbeddings.forward
 * (P/model/Bert_backbone.py:98-113; the reference's position ids are arange(L) for every sample), and with
 * type_tab = pos_tab = NULL the single lookup of gmap_step_embeddings (P/model/vilmodel_goat.py:474) /
 * nav_type_embedding.  ids/type_ids are int64 [rows] (torch LongTensor).  An id outside [0,vocab) sets bit 0 of
 * *err_flag (if given) and reads row 0 instead of faulting. */
int goat_embed_fwd(void* stream, int dtype, const float* word, const int64_t* ids, const float* type_tab,
                   const int64_t* type_ids, const float* pos_tab, int L, void* out, int rows, int H, int vocab,
                   int* err_flag);
/* backward: scatter-add of dout[rows,H] into the PRE-ZEROED float32 table gradients (float atomics).  Any of
 * dword / dtype_tab / dpos may be NULL.  Rows with ids[r] == word_pad and positions l == pos_pad contribute
 * nothing (nn.Embedding(padding_idx) semantics, Bert_backbone.py:85-87; pass -1 for "no padding row").
 * dtype_tab is only written when type_ids != NULL: the all-zero-type case is a column sum (goat_colsum). */
int goat_embed_bwd(void* stream, int dtype, const void* dout, const int64_t* ids, const int64_t* type_ids, int L,
                   float* dword, float* dtype_tab, float* dpos, int rows, int H, int vocab, int word_pad, int pos_pad);

/* ---- causal-learning heads (csrc/causal.hip) -------------------------------------------------------------------
 * tanh-attention pooling of the CFP heads: a = softmax_l(tanh(x[b,l,:])·w) over ALL L <= 256 slots (no padding mask,
 * as the reference), out[b,:] = tanh(sum_l a_l x[b,l,:])   (P/model/pretrain_goat.py:502-515,
 * M/models/vilmodel_GOAT.py:909-922).  x [B,L,H] in `dtype`; w float32 [H]; out float32 [B,H]; attn float32 [B,L] (saved).
 * slot_mask (float32 [B,L], may be NULL): added to the scores before the softmax — 0 / -inf.  NULL = the reference: every slot
 * of the batch's padded width takes part.  A shape-bucketed static batch is padded BEYOND that width; the mask removes exactly
 * those extra slots, so the pooled vector is what the reference computes on the batch's own padding. */
int goat_attn_pool_fwd(void* stream, int dtype, const void* x, const float* w, float* out, float* attn, float* ws, int B,
                       int L, int H, const float* slot_mask);   /* ws: float32 scratch of B*L elements */
/* backward: dx [B,L,H] (dtype) overwritten; dw float32 [H] accumulated (atomics; caller zero-fills); ws: float32 scratch
 * of B*L elements.  H % 4 == 0. */
int goat_attn_pool_bwd(void* stream, int dtype, const void* x, const float* w, const float* attn, const float* out,
                       const float* dout, void* dx, float* dw, float* ws, int B, int L, int H);

/* "door" gate of BACL type_2 / FACL: s = sigmoid(aug·wa + ba + ori·wo + bo) per row, out = s*aug + (1-s)*ori
 * (P/model/vilmodel_goat.py:137-143; M/models/vilmodel_GOAT.py:147-153, 548-552: two nn.Linear(H,1) + nn.Sigmoid).
 * aug/ori/out [rows,H] in `dtype`; wa/wo float32 [H]; ba/bo float32 device scalars; gate float32 [rows] (saved). */
int goat_door_gate_fwd(void* stream, int dtype, const void* aug, const void* ori, const float* wa, const float* wo,
                       const float* ba, const float* bo, void* out, float* gate, int rows, int H);
/* backward: daug/dori overwritten; dwa/dwo float32 [H] and dbias float32 [1] accumulated (caller zero-fills);
 * dbias is the gradient of BOTH biases; dbias2 (may be NULL) receives the same sum — the second bias' own gradient slice.  H <= 1024. */
int goat_door_gate_bwd(void* stream, int dtype, const void* aug, const void* ori, const float* wa, const float* wo,
                       const float* gate, const void* dout, void* daug, void* dori, float* dwa, float* dwo, float* dbias,
                       int rows, int H, float* dbias2);

/* probability-weighted dictionary sum of BACL type_1: out[b,:] = sum_k p[b,k] z[b,k,:]
 * (P/model/vilmodel_goat.py:115-118; M/models/vilmodel_GOAT.py:246-249).  z float32 [B,K,H], p float32 [B,K];
 * out in dtype_out.  backward: dz = p (x) dout, dp = z·dout; either may be NULL. */
int goat_dict_wsum_fwd(void* stream, int dtype_out, const float* z, const float* p, void* out, int B, int K, int H);
int goat_dict_wsum_bwd(void* stream, int dtype_dout, const void* dout, const float* z, const float* p, float* dz, float* dp,
                       int B, int K, int H);

/* ---- fused optimizer step on the gradient arena ------------------------------------------------------------
 * The reference's update (P/train_r2r_goat.py:349-366): grad-norm clip 5.0 over every parameter that has a gradient
 * (torch.nn.utils.clip_grad_norm_), then HF-style AdamW (P/optim/adamw.py:53-110): m = b1 m + (1-b1) g; v = b2 v + (1-b2) g^2;
 * p -= step_size * m / (sqrt(v) + eps) with step_size = lr * sqrt(1-b2^t) / (1-b1^t) (t = that PARAMETER's own step count);
 * then the decoupled decay applied AFTER the update, p -= lr * weight_decay * p (weight_decay 0 for names containing
 * "bias" / "LayerNorm.weight", P/optim/misc.py:13-23); parameters without a gradient in this step are skipped entirely.
 * Here: gradients live in ONE float32 arena (dp.GradArena), the moments in two arenas of the same layout, the parameters
 * stay the model's own float32 tensors.
 *   goat_grad_sqnorm : *out_sq += sum of g^2 over the element ranges [begin, end) of `ranges` (int64 pairs, device memory)
 *   goat_adamw_step  : one launch over `nchunks` chunks (<= 65536 elements each; chunk c = {tensor index, first element}
 *                      int32 pairs in device memory) of the tensors described by `tensors` (device memory).  The clip
 *                      coefficient min(1, max_norm / (sqrt(*sq_norm) + 1e-6)) is computed in the kernel from the device
 *                      scalar goat_grad_sqnorm produced (max_norm <= 0: no clipping), so the step needs no host
 *                      synchronisation.  shadow0 / shadow1 / shadow_f32 (optional): the copies of the parameter the GEMMs read
 *                      (bf16 operand "shadows", the float32 image inside a concatenated QKV bias) refreshed in the same
 *                      pass AT THEIR ADDRESSES — a captured hipGraph that reads them sees the updated weights.  16-byte
 *                      accesses where every address of the tensor allows (gradient, moments, parameter, copies), scalar
 *                      ones elsewhere; a chunk whose first element lies outside its tensor is skipped.  (Both as in
 *                      goat_optim_step below: the two kernels share one walk over the chunk.) */
typedef struct goat_adamw_tensor {
  float* param;            /* float32 master weights */
  void* shadow0;           /* bf16 copy, same element order, or NULL */
  void* shadow1;           /* second bf16 copy (e.g. inside a row-concatenated QKV shadow), or NULL */
  int64_t arena_off;       /* first element of this tensor in the gradient / moment arenas */
  int64_t numel;
  float step_size;         /* lr * sqrt(1 - b2^t) / (1 - b1^t) for this tensor's step count t (or lr without bias correction) */
  float decay;             /* lr * weight_decay (0: no decay) */
  float* shadow_f32;       /* float32 copy, same element order (a member of a concatenated bias), or NULL */
  int32_t cols;            /* > 0: shadow0 is a row-padded image — element i goes to (i / cols) * ld0 + i % cols */
  int32_t ld0;             /*      (the K-padded bf16 copies of the 7- / 14-wide position Linears) */
} goat_adamw_tensor;
int goat_grad_sqnorm(void* stream, const float* arena, const int64_t* ranges, int n_ranges, float* out_sq);
int goat_adamw_step(void* stream, const float* grad_arena, float* exp_avg, float* exp_avg_sq, const goat_adamw_tensor* tensors,
                    const int32_t* chunks, int nchunks, float beta1, float beta2, float eps, float max_norm,
                    const float* sq_norm);

/* ---- the fine-tuning update on the gradient arena (SURVEY a-19, config 4) ------------------------------------------------------
 * The reference's iteration ends with optim_step (M/r2r/agent.py:414-420; M/r2r/agent_base.py:105-123 build, :160-200 loop):
 * clip_grad_norm_(vln_bert.parameters(), 40.) and torch.optim.{AdamW | Adam | RMSprop | SGD}(params, lr = args.lr).step() with torch's
 * default hyper-parameters, optionally under a learning-rate schedule (agent_base.py:125-128); the optimizer state is saved / resumed
 * with --save_optimizer / --resume_optimizer (agent_base.py:205-253).  g = gradient * clip coefficient; torch's single-tensor forms:
 *   GOAT_OPT_ADAMW   : p *= 1 - lr*wd;  m = lerp(m, g, 1-b1);  v = b2 v + (1-b2) g^2;  p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps)
 *                      with bc1 = 1 - b1^t, bc2 = 1 - b2^t, t = *step + 1                (torch defaults: 0.9 / 0.999, 1e-8, wd 1e-2)
 *   GOAT_OPT_ADAM    : the same without the first line; wd != 0 (default 0): g += wd*p before the moments
 *   GOAT_OPT_RMSPROP : v = a v + (1-a) g^2;  p -= lr * g / (sqrt(v) + eps)                (a = hyper->beta1; 0.99, 1e-8; v = exp_avg_sq)
 *   GOAT_OPT_SGD     : p -= lr * g                                                        (wd as for Adam in both)
 * One launch over the chunk table of goat_adamw_step (chunk c = {tensor index, first element}, <= 65536 elements), 16-byte accesses
 * where the addresses allow, the operand copies (shadow0 / shadow1 bf16, shadow_f32, the cols / ld0 row-padded form) refreshed in the
 * same pass at their addresses.  EVERYTHING that changes from step to step is read from device memory — `hyper` (doubles: 1 - b^t,
 * lr / bc1 and 1 - lr*wd are formed in double and rounded to float once, as torch forms them on the host), the int64 counter `step`
 * (= completed steps) and the squared norm goat_grad_sqnorm accumulated into *sq_norm — so the step can be part of a captured
 * hipGraph: a replay picks up a new learning rate or gradient without a host argument.  Clip coefficient as in goat_adamw_step,
 * min(1, max_norm / (sqrt(*sq_norm) + 1e-6)); hyper->max_norm <= 0: no clipping.  exp_avg may be NULL for RMSprop / SGD, exp_avg_sq
 * for SGD.
 *   goat_optim_advance : the step's stream-ordered tail, ONE thread: *step += 1, *last_sq = *sq_norm, *sq_norm = 0 (the next
 *                        goat_grad_sqnorm accumulates from zero).  The update kernel's workgroups all read these and never write them. */
#define GOAT_OPT_ADAMW 0
#define GOAT_OPT_ADAM 1
#define GOAT_OPT_RMSPROP 2
#define GOAT_OPT_SGD 3
typedef struct goat_optim_tensor {
  float* param;            /* float32 master weights */
  void* shadow0;           /* bf16 copy, same element order (or the row-padded image when cols > 0), or NULL */
  void* shadow1;           /* second bf16 copy, or NULL */
  float* shadow_f32;       /* float32 copy, same element order, or NULL */
  int64_t arena_off;       /* first element of this tensor in the gradient / moment arenas */
  int64_t numel;
  int32_t cols;            /* > 0: shadow0 is a row-padded image — element i goes to (i / cols) * ld0 + i % cols */
  int32_t ld0;
} goat_optim_tensor;
typedef struct goat_optim_hyper {
  double lr, beta1, beta2, eps, weight_decay, max_norm;      /* beta1 = alpha for RMSprop */
} goat_optim_hyper;
int goat_optim_step(void* stream, int algo, const float* grad_arena, float* exp_avg, float* exp_avg_sq,
                    const goat_optim_tensor* tensors, const int32_t* chunks, int nchunks, const goat_optim_hyper* hyper,
                    const int64_t* step, const float* sq_norm);
int goat_optim_advance(void* stream, int64_t* step, float* sq_norm, float* last_sq);

/* Tail of the single-action-prediction head, one launch per direction (csrc/causal.hip).  gs [B,G] / ls [B,W]: raw scores of the
 * global / local heads (dtype GOAT_BF16 | GOAT_F32); fwl [B]: fusion logit (fw = sigmoid(fwl) when fw_sigmoid, fwl itself otherwise;
 * NULL: fw = 0.5).  Masks (bytes, any may be NULL): gvis 1 = visited, gvalid 0 = beyond the map, glens map lengths, lmask 1 = masked
 * (1 = valid when lmask_is_valid).  M [B,G,W] float32 logit-fusion matrix (NULL: none).  Outputs float32:
 *   gl = mask(gs * fw), ll = mask(ls * (1 - fw)), fused = gl + M · zero-filled(ll) (+ ll[0] on column 0 when add_stop),
 *   loss[b] = CE(gl, ga) + CE(ll, la) + CE(fused, ga) when loss != NULL (negative label: 0; a label >= G for ga, >= W for la,
 *   compared as the int64 it is: 0 as well, in the loss and in the gradients), lse [B,3] saved for the backward.
 * Replaces the reference's elementwise / masked_fill / bmm / log_softmax chain: P/model/pretrain_goat.py:375-413 (pre-training),
 * M/models/vilmodel_GOAT.py:803-839 (fine-tuning: add_stop = 1, lmask = vp_nav_masks with lmask_is_valid = 1).
 * Backward: upstream dloss [B] (with the labels) and / or dgl, dll, dfused (NULL = zero) -> dgs, dls (dtype), dfwl (when fwl). */
int goat_sap_fuse_fwd(void* stream, int dtype, const void* gs, const void* ls, const void* fwl, int fw_sigmoid,
                      const uint8_t* gvis, const uint8_t* gvalid, const int64_t* glens, const uint8_t* lmask, int lmask_is_valid,
                      const float* M, int add_stop, const int64_t* ga, const int64_t* la, float* gl, float* ll, float* fused,
                      float* loss, float* lse, int B, int G, int W);
int goat_sap_fuse_bwd(void* stream, int dtype, const void* gs, const void* ls, const void* fwl, int fw_sigmoid,
                      const uint8_t* gvis, const uint8_t* gvalid, const int64_t* glens, const uint8_t* lmask, int lmask_is_valid,
                      const float* M, int add_stop, const int64_t* ga, const int64_t* la, const float* gl, const float* ll,
                      const float* fused, const float* lse, const float* dloss, const float* dgl, const float* dll,
                      const float* dfused, void* dgs, void* dls, void* dfwl, int B, int G, int W);
/* CFP contrastive losses (P/model/pretrain_goat.py:519-534): loss[i] = sum over x in {gmap, vp, fused} of
 * 1/2 [CE(x_loc[i]·txt_allᵀ/τ, t_i) + CE(txt_loc[i]·x_allᵀ/τ, t_i)], t_i = target0 + i.  x_loc / x_all: arrays of 3 device
 * pointers ([Bl,H] / [Ba,H] float32; all = loc on one rank, the all-gathered rows under data parallelism); loss [Bl] is
 * ADDED to (one writer per sample: deterministic); prob: [6,Bl,Ba] float32 scratch the backward reads.
 * Backward: gradients are ADDED to dx_loc[k] / dx_all[k] / dtxt_loc / dtxt_all (any may be NULL; loc and all pointers may
 * alias on one rank).  Every output element has one writer that sums its contributions in a fixed order — no atomics, so a
 * captured or phased step reproduces the eager one bit for bit.  Replaces ~70 ATen launches of the torch formulation. */
int goat_infonce_fwd(void* stream, const float* const* x_loc, const float* const* x_all, const float* txt_loc,
                     const float* txt_all, float* loss, float* prob, int Bl, int Ba, int H, int target0, float temperature);
int goat_infonce_bwd(void* stream, const float* const* x_loc, const float* const* x_all, const float* txt_loc,
                     const float* txt_all, const float* dloss, const float* prob, float* const* dx_loc, float* const* dx_all,
                     float* dtxt_loc, float* dtxt_all, int Bl, int Ba, int H, int target0, float temperature);

/* Debug/probe helper used by tests: fills out[64*4] with the element indices returned by
 * ds_read_b64_tr_b16 when lane l points at elements 4l..4l+3 of an LDS array holding 0,1,2,... */
int goat_probe_tr16(void* stream, uint16_t* out);

/* Linear(H, 1) — the last layer of ClsPrediction (P/model/pretrain_goat.py:27-38: the global / local action scores, the fusion logit, the
 * object scores): y[m] = x[m,:] . w + b (w: float32 [H], rounded to the activation dtype as the GEMM path's shadow weight; b: float32 [1] or
 * NULL; float32 accumulation; y in `dtype`).  H a multiple of 8, <= 1024. */
int goat_rowdot_fwd(void* stream, int dtype, const void* x, const float* w, const float* b, void* y, int M, int H);
/* backward: dx[m,:] = dy[m] w (NULL: skipped); dw[H] += sum_m dy[m] x[m,:], db[1] += sum_m dy[m] (float32 atomics: the caller clears or
 * accumulates).  NULL dw: db must be NULL too (GOAT_E_ARG otherwise: the kernel has no bias-only form). */
int goat_rowdot_bwd(void* stream, int dtype, const void* x, const float* w, const void* dy, void* dx, float* dw, float* db, int M, int H);

/* CFP fused vector (P/model/pretrain_goat.py:486-499 with the glocal fusion weight of :393-399): w = sigmoid(fwl[b]) (fwl: the
 * output of sap_fuse_linear, [B] in dtype_fwl); fo[b,:] = go[b,:] * w + vo[b,:] * (1 - w) (float32 [B,H]); fw[b] = w saved for backward.
 * Replaces sigmoid, two muls, rsub, add (and their ~10 backward launches) on [B,768] tensors. */
int goat_cfp_mix_fwd(void* stream, int dtype_fwl, const float* go, const float* vo, const void* fwl, float* fo, float* fw, int B, int H);
/* backward: dgo = dfo * w, dvo = dfo * (1 - w) (accumulate != 0: ADDED to what dgo / dvo hold — the InfoNCE gradients of the same vectors),
 * dfwl[b] = w (1 - w) sum_h dfo (go - vo) in dtype_fwl. */
int goat_cfp_mix_bwd(void* stream, int dtype_fwl, const float* go, const float* vo, const float* fw, const float* dfo, float* dgo,
                     float* dvo, void* dfwl, int B, int H, int accumulate);

/* ---- glue of the captured steps (csrc/glue.hip) -------------------------------------------------------------------------
 * out[numel] = sum_i srcs[i][numel] (n <= 8 tensors of `dtype`, float32 accumulation, ONE rounding): the gradient of a tensor with
 * several consumers — replaces the k - 1 pairwise `add` launches of torch's autograd engine (AccumulateGrad-free fan-in: the text
 * states read by every cross-modal layer, P/model/vilmodel_goat.py:163-199; LayerNorm outputs with two consumers,
 * P/model/Bert_backbone.py:304-310).  srcs is a HOST array of device pointers (16-B aligned); out may alias srcs[0]. */
int goat_add_n(void* stream, int dtype, const void* const* srcs, int n, void* out, int64_t numel);
/* n <= 16 byte ranges (16-B aligned, multiples of 16 bytes) cleared by one launch — optimizer.zero_grad() of the reference
 * (P/train_r2r_goat.py:301-363) over the gradient arena's per-task ranges.  ptrs / nbytes are HOST arrays. */
int goat_zero_ranges(void* stream, void* const* ptrs, const int64_t* nbytes, int n);

/* ---- validation metrics (csrc/navmetrics.hip) ----------------------------------------------------------------------------
 * Every per-trajectory score of the reference's `eval_metrics` (M/r2r/env.py:452-490 `_eval_item`, M/r2r/eval_utils.py `cal_dtw` /
 * `cal_cls`) for N items in one launch, one 64-thread workgroup per item.  out[N, GOAT_NAV_METRICS_COLS] float64, columns:
 *   0 nav_error   1 oracle_error   2 trajectory_steps   3 trajectory_lengths   4 gt_lengths   5 success   6 oracle_success   7 spl
 *   8 DTW   9 nDTW   10 SDTW   11 CLS
 * dist: the shortest-distance tables of n_scans scans, each a packed row-major [n_s, n_s] float64 block at dist + scan_off[s] with
 * n_s = scan_n[s]; item_scan[N]: the table of every item.  pred / ref: node indices of the flattened predicted path and of the
 * ground-truth path in CSR form (item i owns pred[pred_start[i] : pred_start[i + 1]], P_i nodes, and likewise R_i nodes of ref).
 * success = nav_error < margin (strict), spl = success * gt_len / max(traj_len, gt_len, 0.01), nDTW = exp(-DTW / (margin * R)),
 * SDTW = success * nDTW, CLS as cal_cls (a one-node reference path gives 0 / 0 = NaN, as there).  With goal / goal_start (CSR of
 * goal nodes per item; both NULL = the rule above) columns 5 and 6 follow M/reverie/env.py:543-549: the last node / any node of the
 * predicted path is one of the item's goal nodes.  All arithmetic is IEEE float64 without contraction; DTW is computed by
 * anti-diagonals with the reference's own add per cell (bit-identical to its matrix); columns 3, 4, 7, 9, 10, 11 hold sums whose order
 * differs from numpy's.  max_ref >= max_i R_i sizes the LDS (three diagonals): 1 <= max_ref <= 2047; P_i is not capped.
 * PRECONDITION (the entry cannot read device memory): every node index is in [0, n_s) of its item's scan, every goal index too, the
 * CSR starts are non-decreasing and inside their arrays, P_i >= 1 and 1 <= R_i.  The kernel writes a row of NaN for an item whose
 * scan id is outside [0, n_scans), whose P_i or R_i is < 1 or whose R_i exceeds max_ref; it cannot check node indices.
 * GOAT_E_ARG: a null pointer other than stream / goal / goal_start, or exactly one of goal / goal_start given;
 * GOAT_E_SHAPE: N < 1, n_scans < 1, max_ref < 1 or max_ref > 2047.  Both are returned before any launch. */
#define GOAT_NAV_METRICS_COLS 12
int goat_nav_metrics(void* stream, const double* dist, const int64_t* scan_off, const int32_t* scan_n, int n_scans,
                     const int32_t* item_scan, const int32_t* pred, const int32_t* pred_start, const int32_t* ref,
                     const int32_t* ref_start, const int32_t* goal, const int32_t* goal_start, int N, int max_ref, double margin,
                     double* out);

/* ---- validation statistics of the pre-training tasks (csrc/valstats.hip) -----------------------------------------------------------
 * The sums behind the reference's validate_mlm / _mrc / _sap / _cfp (P/train_r2r_goat.py:438-583) and validate_og
 * (P/train_reverie_goat.py:587-612) without a host read per batch: goat_val_rows / goat_val_cfp write one loss and one hit per row,
 * goat_val_reduce adds their sums into a float64 slot the caller reads once per loader.  Plain stores, no atomics, no waiting
 * between workgroups: every sum has one writer and a fixed order, so two runs give the same bits (the reference's sums come out of
 * float32 atomics).  Every entry returns GOAT_E_ARG / GOAT_E_SHAPE before any launch.
 *
 * goat_val_rows: logits float32 [M, ld] with N valid columns, ANY ld >= N and a base that needs float alignment only (16-byte loads
 * where a row allows them; goat_ce_fwd demands ld % 4 == 0 and a 16-byte base, the [B, G] logits of sap / og have neither).  Each
 * logit is read once.  Exactly one of `labels` (int64 [M]) and `soft` (float32 [M, ld_soft]) is non-null:
 *   hard: row_loss[m] = logsumexp(row) - row[label], row_hit[m] = (argmax(row) == label): F.cross_entropy(reduction='sum') and
 *         `scores.max(dim=-1)[1] == labels` (P/train_r2r_goat.py:449-451, :509-514; P/train_reverie_goat.py:597-599), row by row.
 *         label < 0: an ignored row, loss 0, hit 0, not counted by goat_val_reduce.  label >= N: NaN loss, hit 0 (goat_ce_fwd's rule).
 *   soft: row_loss[m] = sum_n xlogy(t, t) - t * log_softmax(row)[n] (F.kl_div(log_softmax, t, reduction='sum'), P/train_r2r_goat.py:
 *         481-482; a zero target contributes 0), row_hit[m] = (argmax(row) == argmax(t)) (compute_accuracy_for_soft_targets, :466-470).
 * Every argmax is the lowest index among the maxima.  -inf logits (masked slots) are skipped; a row of only -inf gives a NaN loss as
 * torch does (its argmax is 0); a NaN logit gives a NaN loss and hit 0.  row_loss float32 [M], row_hit int32 [M].
 * GOAT_E_ARG: null logits / row_loss / row_hit, both or neither of labels / soft; GOAT_E_SHAPE: M < 1, N < 1, ld < N, ld_soft < N. */
int goat_val_rows(void* stream, const float* logits, int64_t ld, int M, int N, const int64_t* labels, const float* soft,
                  int64_t ld_soft, float* row_loss, int32_t* row_hit);
/* validate_cfp (P/train_r2r_goat.py:540-565): x is a HOST array of 3 device pointers (gmap, vp, fused), all operands float32 [B, H]
 * packed.  row_loss[k, i] = 1/2 [CE(x_k[i]·txtᵀ/τ, i) + CE(txt[i]·x_kᵀ/τ, i)], row_hit[k, i] = (argmax_j x_k[i]·txt[j] == i) (image to
 * text only, as the reference counts it; lowest index among the maxima); dots are float32 accumulations as in goat_infonce_fwd.
 * row_loss float32 [3, B], row_hit int32 [3, B].  One workgroup per (k, i) holds both score rows in LDS: B <= GOAT_VAL_CFP_MAX_B.
 * GOAT_E_ARG: a null pointer (x, any x[k], txt, row_loss, row_hit); GOAT_E_SHAPE: B < 1, B > 1024, H < 1, temperature not > 0. */
#define GOAT_VAL_CFP_MAX_B 1024
int goat_val_cfp(void* stream, const float* const* x, const float* txt, int B, int H, float temperature, float* row_loss,
                 int32_t* row_hit);
/* One workgroup: acc[0] += sum_m row_loss[m] (float64, strided partials in ascending order, then a fixed tree), acc[1] += sum_m
 * row_hit[m], acc[2] += the number of rows with labels[m] >= 0 (labels NULL: M).  acc: one float64 [3] slot of a caller-owned
 * [n_slots, 3] tensor; counts stay exact in a double.  Launches on one stream run in order, so a slot has one writer at a time.
 * GOAT_E_ARG: null row_loss / row_hit / acc; GOAT_E_SHAPE: M < 1. */
int goat_val_reduce(void* stream, const float* row_loss, const int32_t* row_hit, const int64_t* labels, int M, double* acc);

/* ---- the navigator of a policy-driven walk on the device (csrc/navstate.hip, csrc/navstate_core.hpp) --------------------------------
 * A sampled (M/r2r/agent.py:596-690, feedback = 'sample') or argmax (:601-672) walk without host tables: goat_nav_step for index t
 * does what EpisodePlanner.advance() of step t - 1 followed by build_step() of step t do on the host (vln-goat_amd/episodes.py:245-357;
 * the map of M/models/graph_utils.py:43-144, the builders of M/r2r/agent.py:82-347, the fusion matrix of M/models/vilmodel_GOAT.py:
 * 790-806) and writes the step's tables at the addresses the captured step graph reads.  t = 0 builds only; t = T advances only.
 *   scan_tab   device int64 [14]: addresses of the static scan tables in the order navdev.ScanTables packs them (positions float64
 *              [NV, 3]; candidate CSR start int32 [NV + 1], neighbour, pointId int32 [NC], normalized heading / elevation float64
 *              [NC, 2], edge length float64 [NC]; feature row, scan of a viewpoint int32 [NV]; first viewpoint, size int32 [S], offset
 *              int64 [S] and values float64 of the scans' all-pairs shortest distances; view_angle_feature_table float32 [36, 36, A];
 *              heading / elevation of the 36 views float64 [36, 2]).  Viewpoints are numbered across the scans of the table.
 *   step_tab   device int64 [21]: addresses of the tables of step t in the order feat_idx, feat_start, loc_fts, nav_types, view_lens,
 *              gmap_step_ids, gmap_pos_fts, gmap_pair_dists, gmap_visited_masks, gmap_masks, vp_pos_fts, vp_masks, vp_nav_masks,
 *              nav_fusion, target, csr_idx, csr_start, csr_scale, inv_idx, inv_start, inv_w, in the dtypes and shapes of
 *              EpisodePlanner.build_step at map width G and panorama width W (int32 index tables, int64 ids / types / lens / target,
 *              1-byte bool masks, float32 features).  Every element, padding included, is written.  NULL when t == T.
 *   si, sd     the private state: B blocks of goat_nav_state_ints(T, W, cap) int32 and of cap * cap + cap float64 (distance matrix with
 *              the reference's 95959595 default, stop scores).
 *   log        the read-back block: actions int32 [T, B], alive flags [T, B], then B blocks of goat_nav_log_ints(T, cap) int32: a header
 *              (word 2 ended, 5 status, 6 its step, 11 live steps, 16 hops, 17 / 18 start and length of the backtrack), T + 2 hop
 *              starts and the hop log (viewpoint numbers).
 *   ws         int32 workspace of 2 (B + 1) + T (B W + B) + B + 1 words; the last one holds the number of episodes still walking when
 *              step t begins (for a caller that wants to stop early; reading it synchronises).
 *   act        the action of step t - 1 (NULL at t = 0).  mode 0 (sample): the step's probabilities float32 [B, G_prev] with u float64
 *              [T, B]: SampledEpisode.sample, a serial float64 cumulative sum in slot order, u * c[-1] clamped to nextafter(c[-1], 0),
 *              the first slot whose cumulative mass exceeds it.  mode 1 (argmax): float32 [3, B] (action, stop score, best object);
 *              the stop scores of live episodes are kept per node and an ending episode appends the path to the first maximum in visit
 *              order.  mode 2 (forced): int32 [T, B].
 * Status words (sticky, first wins): 1 a map larger than the step's bucket G or than cap, 2 a panorama wider than W, 3 an action that
 * is not a selectable node, 4 a hop log or path stack that overflowed.  The kernel clamps and goes on; nothing faults.
 * One workgroup per episode plus one workgroup for the batch-wide compact CSRs; plain stores, no atomics; float64 sums and
 * comparisons are single IEEE operations (contraction off), so decisions, map distances and labels equal the host's bit for bit; the
 * angle features go through the device's sin / cos / asin.
 * PRECONDITION (the entry cannot read device memory): the address tables point at tensors of the stated sizes; ep holds valid numbers.
 * GOAT_E_ARG: a null pointer (act / u where the mode and t need them, step_tab for t < T), a mode outside 0..2;
 * GOAT_E_SHAPE: B, T, W, cap, G, G_prev of zero or above GOAT_NAV_MAX_*, G < 2 or G > cap + 2, t outside [0, T], A not a multiple of
 * 4 in [4, 64].
 * Both are returned before any launch. */
#define GOAT_NAV_MAX_B 1024
#define GOAT_NAV_MAX_T 64
#define GOAT_NAV_MAX_G 256
#define GOAT_NAV_MAX_W 64
#define GOAT_NAV_MAX_CAP 254
/* goat_nav_reset: start_walk (vln-goat_amd/nav_inputs.py:223-230) for B episodes: ep int32 [B, 4] = scan, start viewpoint, start view
 * index, goal viewpoint.  Clears state and log, then the first update_graph. */
/* sizes of one episode's blocks in int32 words (values, not status codes; 0 for sizes outside the limits above) */
int goat_nav_state_ints(int T, int W, int cap);
int goat_nav_log_ints(int T, int cap);
int goat_nav_reset(void* stream, const int64_t* scan_tab, int32_t* si, double* sd, int32_t* log, const int32_t* ep, int B, int T, int W,
                   int cap);
int goat_nav_step(void* stream, const int64_t* scan_tab, const int64_t* step_tab, int32_t* si, double* sd, int32_t* log, int32_t* ws,
                  const void* act, const double* u, int mode, int t, int B, int T, int G_prev, int G, int W, int A, int cap,
                  int64_t ignoreid);

/* goat_nav_ndtw: the DAgger label of the nDTW expert (csrc/navexpert_core.hpp) for step t < T, launched behind goat_nav_step(t) on the
 * same state: `_teacher_action` under expert_policy = 'ndtw' (M/r2r/agent.py:330-346, what the RxR scripts set) with `cal_dtw`
 * (M/r2r/eval_utils.py:6-26).  Per selectable unvisited map slot g >= 2 the DTW between (walked path + shortest path from the current
 * viewpoint to the slot's node) and the episode's ground-truth path; the first slot whose DTW is strictly smallest is written to the
 * step's `target` over the shortest-path label goat_nav_step put there (ignoreid for an ended episode or without a candidate, 0 on the
 * goal).  The kernel orders by DTW, not by -nDTW = -exp(-DTW / (3 R)): exp is monotone, so the two agree except where rounding maps two
 * DTWs to one double.  Every cell is cost + min(up, left, diag) in float64 in cal_dtw's order, rows filled serially (no scan across
 * lanes), so the labels equal nav_inputs.teacher_action(expert_policy='ndtw') exactly.
 *   scan_tab   as goat_nav_step, with a 15th address: the predecessor matrices int32 of the scans' all-pairs shortest paths
 *              (ScanGraph.shortest()[1], scan-local indices) at the offsets of the distances.  goat_nav_step reads the first 14 only.
 *   ref        int32 [B, max_ref + 1]: the length R of an episode's ground-truth path (1 <= R <= max_ref), then its viewpoint numbers.
 *   xd         float64, B blocks of goat_nav_expert_doubles(cap, max_ref): the DTW row behind the last folded node of the walked path and
 *              one working row per map node.  The fold counter is header word 21 of the episode's log block, cleared by goat_nav_reset.
 * One workgroup of 256 threads per episode; the walked path is folded forward by the hops logged since the last call (thread 0), then
 * one thread per candidate.  A predecessor chain that does not reach the current viewpoint sets status word 4.
 * GOAT_E_ARG: a null pointer; GOAT_E_SHAPE: B, T, W, cap outside the limits above, max_ref < 1 or > GOAT_NAV_MAX_REF, t outside [0, T).
 * Both are returned before any launch.  goat_nav_expert_doubles is a value (0 for sizes outside the limits). */
#define GOAT_NAV_MAX_REF 64
int goat_nav_expert_doubles(int cap, int max_ref);
int goat_nav_ndtw(void* stream, const int64_t* scan_tab, const int64_t* step_tab, int32_t* si, double* sd, int32_t* log,
                  const int32_t* ref, double* xd, int t, int B, int T, int W, int cap, int max_ref, int64_t ignoreid);

/* goat_nav_obj_*: goat_nav_reset / goat_nav_step for a REVERIE / SOON walk (M/reverie/agent_obj_goat.py:180-436), whose panoramas carry
 * up to O object tokens behind their W views (WT = W + O).  The step differs from goat_nav_step where EpisodePlanner.build_step branches
 * on its objects: the pool rows of a step are B * WT + B; loc_fts [B, WT, A + 3] and nav_types [B, WT] hold, behind the view_len views,
 * [angle_feature(direction - the snapped view's angles) | box] and type 2 per object; vp_masks, vp_nav_masks, vp_pos_fts and nav_fusion
 * are WT + 2 wide; gmap_masks[:, 1] stays true (the REVERIE builder keeps [MEM] selectable; choosing it is still status 3); the label
 * is the shortest-path expert's.  The same two launches: one workgroup per episode, one for the batch-wide tables.
 *   obj_tab    device int64 [5]: addresses of the static object tables in the order navdev.ObjectTables packs them, indexed by the
 *              viewpoint numbers of scan_tab: object CSR start int32 [NV + 1], first row of the viewpoint in ObjectStore.table int32
 *              [NV] (its rows are contiguous), and per object direction float64 [N, 2], box float32 [N, 3] (h / 480, w / 640, their
 *              float32 product), category int64 [N].
 *   step_tab   as goat_nav_step at panorama width WT (feat_idx / feat_start stay [B * W] / [B * W + 1]).
 *   ostep_tab  device int64 [10]: obj_idx int32 [B * O], obj_start int32 [B * O + 1], reverie_obj_lens int64 [B], reverie_obj_names
 *              int64 [B, O], vp_obj_masks bool [B, WT + 2], obj_target int64 [B] (slot of the target object on one of the episode's
 *              goal viewpoints, else ignoreid), ocat_idx int32 [B * WT], ocat_start int32 [B * WT + 1], ocat_inv_idx int32 [B * WT],
 *              ocat_inv_start int32 [B * W + B * O + 1].  Every element, padding included, is written.  NULL when t == T.
 *   goal       int32 [B, max_end, 2]: per episode its goal viewpoints (-1: unused pair) and the index of the target object among each
 *              one's objects (-1: not there).  Read every step; not copied into the state.
 *   si         B blocks of goat_nav_obj_state_ints(T, W, O, cap) int32; sd and log as goat_nav_step.  Header words 22 / 23 of a log
 *              block: 1 + the viewpoint of the best stop node at the forced end of an argmax walk (0: no node was scored) and its best
 *              object (row 2 of act, recorded per scored node; -1 where the viewpoint has no objects: the row is not read there).
 *   ws         int32 workspace of 2 (B + 1) + T (B WT + B) + B + 1 + (B + 1) words; the live count is word 2 (B + 1) + T (B WT + B) + B.
 * Status word 5: a viewpoint with more than O objects (clamped).
 * GOAT_E_ARG: a null pointer (as goat_nav_step; obj_tab, goal; ostep_tab for t < T); GOAT_E_SHAPE: O < 1 or > GOAT_NAV_MAX_O, max_end
 * outside 1..GOAT_NAV_MAX_END, and everything goat_nav_step rejects.  Both are returned before any launch.  goat_nav_obj_state_ints is a
 * value (0 outside the limits).  The read-back block keeps the size goat_nav_log_ints(T, cap). */
#define GOAT_NAV_MAX_O 64
#define GOAT_NAV_MAX_END 64
int goat_nav_obj_state_ints(int T, int W, int O, int cap);
int goat_nav_obj_reset(void* stream, const int64_t* scan_tab, int32_t* si, double* sd, int32_t* log, const int32_t* ep, int B, int T,
                       int W, int O, int cap);
int goat_nav_obj_step(void* stream, const int64_t* scan_tab, const int64_t* obj_tab, const int64_t* step_tab, const int64_t* ostep_tab,
                      int32_t* si, double* sd, int32_t* log, int32_t* ws, const void* act, const double* u, const int32_t* goal, int mode,
                      int t, int B, int T, int G_prev, int G, int W, int O, int max_end, int A, int cap, int64_t ignoreid);

#ifdef __cplusplus
}
#endif
#endif /* GOAT_HIP_H */
