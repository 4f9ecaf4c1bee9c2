/* polus_hip.h — C ABI of libpolus_hip.so, the MI355X (gfx950) kernel library behind the
 * Polus training hot path.
 *
 * The reference (bioinformatics-ua/polus @ 0.2.1) has NO native interface: every numeric
 * instruction of `BaseTrainer.train_step` (polus/training.py:150-193) is executed by
 * third-party wheels (TensorFlow/Keras, HuggingFace TF-BERT, tensorflow-addons, Horovod).
 * Each entry point below therefore cites the reference call site whose arithmetic it
 * replaces.  Conventions:
 *   - every function returns 0 on success; on failure a non-zero code and a thread-local
 *     message from polus_last_error();
 *   - every pointer is a caller-owned DEVICE pointer (HBM) unless the name says host;
 *     nothing is allocated inside a call — scratch is passed as (workspace, bytes) and
 *     sized with the matching *_workspace_bytes();
 *   - every launch goes to the caller's stream (`void* stream` is a hipStream_t);
 *     no call synchronises;
 *   - activations are row-major [rows, features]; Dense weights are [out, in]
 *     (PyTorch layout — the reference loads its BERT weights `from_pt=True`,
 *     polus/models.py:229);
 *   - `dtype` selects the activation/weight element type: POLUS_F32 (exact-f32 MFMA,
 *     the parity path) or POLUS_BF16 (bf16 MFMA inputs, f32 accumulation).  Biases,
 *     LayerNorm parameters, statistics, losses, gradients of parameters and optimizer
 *     state are always f32.
 */
#ifndef POLUS_HIP_H
#define POLUS_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define POLUS_ABI_VERSION 1

enum { POLUS_OK = 0, POLUS_ERR_INVALID = 1, POLUS_ERR_HIP = 2, POLUS_ERR_WORKSPACE = 3 };
enum { POLUS_F32 = 0, POLUS_BF16 = 1 };
/* operand storage for polus_gemm: K_CONTIG = [rows][K] (K fastest), K_STRIDED = [K][rows] */
enum { POLUS_K_CONTIG = 0, POLUS_K_STRIDED = 1 };
enum { POLUS_ACT_NONE = 0, POLUS_ACT_GELU = 1, POLUS_ACT_SWISH = 2, POLUS_ACT_RELU = 3, POLUS_ACT_TANH = 4 };
/* polus_gemm flags */
enum {
    POLUS_GEMM_ACCUM_C = 1,  /* C += result (gradient accumulation)                         */
    POLUS_GEMM_ACT_FWD = 2,  /* aux[m][n] = v (pre-activation, if aux != NULL); C = act(v)   */
    POLUS_GEMM_ACT_BWD = 4,  /* C = v * act'(aux[m][n])                                      */
    POLUS_GEMM_DROPOUT = 8   /* polus_gemm_dropout only: v = keep(seed, m*N+n) ? v/(1-p) : 0   */
};

const char* polus_last_error(void);
int polus_abi_version(void);
/* host out-params; arch is a NUL-terminated gcnArchName prefix (e.g. "gfx950") */
int polus_device_info(int* n_cu, int* lds_bytes_per_cu, char* arch, int arch_len);
/* The POLUS_* tuning switches of the library are read from the environment once, at the first call
 * that needs one; this re-reads them (A/B tools and tests that flip a switch inside one process). */
int polus_reload_env(void);
/* POLUS_GEMM_RESERVE_CUS (CUs the GEMM tile-shape choice and the persistent grids leave to concurrent RCCL channel
 * kernels) applies only while this is on (default on).  The data-parallel trainer switches it on for backward, where the
 * bucketed exchange runs beside the GEMMs, and off for the forward pass. */
int polus_set_reserve_active(int on);
/* Per-step scalars from device memory, for steps replayed from a captured HIP graph (the kernel arguments of a
 * replay are frozen).  `dev_block16` points to 16 bytes in HBM, {uint32 salt; float lr; float lr_t; uint32 0},
 * that the caller rewrites before each replay; NULL unregisters.  While a block is registered
 *   - every dropout site uses seed_eff = mix(seed + salt), mix(x) = (x ^ x >> 15) * 0x2C1B3C6D (uint32), so the
 *     caller passes the step-independent part as `seed` and the step term as `salt` (the eager path passes
 *     mix(step-independent + step term) as `seed`: identical masks either way);
 *   - polus_adam_step takes lr and lr_t from the block instead of its arguments.
 * Process-wide (one process drives one GPU). */
int polus_set_dynamic_params(const void* dev_block16);

/* ---- GEMM (HF Dense layers + their gradients; tape.gradient at polus/training.py:185)
 * C[M,N] = epilogue(alpha * A_op[M,K] . B_op[K,N]).
 *   a_layout: K_CONTIG  -> A stored [M][K] (lda = row stride), K_STRIDED -> stored [K][M]
 *   b_layout: K_CONTIG  -> B stored [N][K] (ldb),              K_STRIDED -> stored [K][N]
 *   forward  Y = X W^T        : A=X (K_CONTIG), B=W[out,in] (K_CONTIG)
 *   dX = dY W                 : A=dY (K_CONTIG), B=W[out,in] (K_STRIDED)
 *   dW = dY^T X               : A=dY (K_STRIDED), B=X (K_STRIDED), c_dtype = POLUS_F32
 * epilogue order: v = alpha*acc; v += bias[n]; ACT_FWD: aux=v, v=act(v); ACT_BWD: v*=act'(aux);
 *                 v += resid[m][n]; ACCUM_C: v += C[m][n]; C = v.
 * c_dtype is the element type of C / resid / aux... C only: resid and aux use `dtype`.
 * split_k > 1 writes f32 partial slabs to `workspace` and reduces them in a second,
 * order-fixed kernel (bitwise reproducible).  With bf16 K-contiguous operands and a bf16 C the reduce
 * applies the whole epilogue (residual, activation forward / backward, dropout); otherwise only
 * bias / ACCUM_C epilogues are allowed with split_k > 1.
 * polus_gemm_auto_split: the number of K slices the library recommends for a bf16 Dense GEMM of this size
 * (1 = none; a tuning query with no counterpart in the reference, whose Dense layers are Keras / HF calls):
 * > 1 only for about two thousand tokens and fewer, where even its 128 x 128 tile leaves most of the chip idle. */
size_t polus_gemm_workspace_bytes(int M, int N, int split_k);
int polus_gemm_auto_split(int M, int N, int K);
int polus_gemm(int dtype, int a_layout, int b_layout, int c_dtype,
               const void* A, long lda, const void* B, long ldb, void* C, long ldc,
               int M, int N, int K, float alpha,
               const float* bias, const void* resid, long ldr, void* aux, long ldaux,
               int act, int flags, int split_k, void* workspace, size_t workspace_bytes,
               void* stream);

/* polus_gemm with inverted dropout in the epilogue, applied after bias/activation and before the
 * residual add (HF TFBertSelfOutput / TFBertOutput: dropout(dense(x)) + residual).  The mask is a
 * pure function of (seed, m*N + n); polus_dropout_mask reproduces it. */
int polus_gemm_dropout(int dtype, int a_layout, int b_layout, int c_dtype,
                       const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                       int M, int N, int K, float alpha,
                       const float* bias, const void* resid, long ldr, void* aux, long ldaux,
                       int act, int flags, int split_k, void* workspace, size_t workspace_bytes,
                       float drop_p, uint32_t seed, void* stream);
/* polus_gemm_route (host only: no HIP call, no pointer dereferenced) reports what polus_gemm (drop_p == 0) or
 * polus_gemm_dropout (drop_p > 0) would run for these arguments under the current switches.  The pointers count for their
 * alignment alone (any integer address; NULL = absent for bias / resid / aux).  It fails where those calls fail in validation
 * (the workspace aside), with the same message.  out[POLUS_GEMM_ROUTE_INTS]:
 *   [0] kernel: 0 general 128 x 128, 1 ring 256 x 128, 2 ring 128 x 128, 3 ring 256 x 128 with dropout, 4 ping-pong one
 *       workgroup per tile, 5 ping-pong persistent
 *   [1] tile width   [2] compile-time epilogue class 0..3 (alpha / bias, activation forward, residual (+ dropout),
 *       activation backward), -1 = run-time epilogue   [3] dropout   [4] K slices launched
 *   [5] reduce after the slices: 0 none, 1 plain (alpha, bias, ACCUM_C), 2 with the whole epilogue
 *   [6] workgroups of the persistent ping-pong form, else 0
 *   [7] a_vec [8] b_vec: whole aligned 16-byte operand chunks   [9] epi_vec: 4-wide epilogue accesses   [10] epi_vec16: 16-byte
 *       epilogue accesses   [11] kernel 0 runs its whole-chunk instantiation (a_vec and b_vec) */
#define POLUS_GEMM_ROUTE_INTS 12
int polus_gemm_route(int dtype, int a_layout, int b_layout, int c_dtype,
                     const void* A, long lda, const void* B, long ldb, void* C, long ldc,
                     int M, int N, int K, float alpha,
                     const float* bias, const void* resid, long ldr, void* aux, long ldaux,
                     int act, int flags, int split_k, float drop_p, int* out);
/* y[i] = keep(seed, i) ? x[i]/(1-p) : 0 (tf.keras.layers.Dropout; apply the same call to dy for backward) */
int polus_dropout(int dtype, const void* x, void* y, int64_t n, float drop_p, uint32_t seed, void* stream);
/* mask[i] = 1 if element i is kept (i = idx0 .. idx0+n-1): the reference for every dropout site */
int polus_dropout_mask(uint32_t seed, float drop_p, uint32_t idx0, int64_t n, uint8_t* mask, void* stream);

/* ---- Dense backward for the parameters (the dW/db part of tape.gradient, polus/training.py:185):
 * dW[n_out, n_in] (+)= dY[T, n_out]^T . X[T, n_in]  (f32) and, if db != NULL, db[n_out] (+)= column
 * sums of dY — one pass over dY (on the bf16 ring kernel the column sums ride on the matrix pipe).
 * Deterministic split-K over T. */
size_t polus_dense_bwd_params_workspace_bytes(int T, int n_out, int n_in, int split_k);
int polus_dense_bwd_params(int dtype, const void* dY, long lddy, const void* X, long ldx,
                           float* dW, long lddw, float* db, int T, int n_out, int n_in,
                           int accumulate, int split_k, void* workspace, size_t workspace_bytes,
                           void* stream);

/* Host only, like polus_gemm_route: out[0] = 1 the ring kernel (column sums on the matrix pipe), 0 polus_gemm + polus_colsum;
 * out[1] = K slices launched. */
int polus_dense_bwd_params_route(int dtype, const void* dY, long lddy, const void* X, long ldx,
                                 float* dW, long lddw, float* db, int T, int n_out, int n_in, int split_k, int* out);

/* The same for up to POLUS_MAX_GROUP (8) Dense layers in ONE launch -- the four weight gradients of
 * an encoder layer (the per-variable MatMul grads tape.gradient emits for one TFBertLayer,
 * polus/training.py:185 through polus/models.py:205-213): the concatenated tile lists fill the chip
 * with 2-3 K-splits instead of 7-28 per matrix.  All problems share T and `accumulate`; split_k > 0
 * applies to every problem, split_k <= 0 lets the library choose per problem so that the launch is
 * one full round of workgroup slots; db may be NULL per problem.  Falls back to one call per problem when a shape does not fit the
 * grouped kernel. */
typedef struct polus_dw_problem {
    const void* dY; long lddy;     /* [T, n_out] */
    const void* X;  long ldx;      /* [T, n_in]  */
    float* dW; long lddw;          /* [n_out, n_in] f32 */
    float* db;                     /* [n_out] f32 or NULL */
    int n_out, n_in;
} polus_dw_problem;
size_t polus_dense_bwd_params_grouped_workspace_bytes(int n, const polus_dw_problem* problems, int T, int split_k);
int polus_dense_bwd_params_grouped(int dtype, int n, const polus_dw_problem* problems, int T, int accumulate,
                                   int split_k, void* workspace, size_t workspace_bytes, void* stream);

/* Host only, like polus_gemm_route: out[0] = 0 one call per problem, 1 ring grouped, 2 ping-pong grouped with an even
 * split, 3 ping-pong stream-K; out[1] = 1 when every slab reduction and bias gradient of the group takes one launch;
 * out[2 + k] = K slices of problem k (stream-K: its slots per tile).  out holds 2 + n ints. */
int polus_dense_bwd_params_grouped_route(int dtype, int n, const polus_dw_problem* problems, int T, int split_k, int* out);

/* ---- Dense layers with at most 8 output units (a token-classification head, polus/ner/models.py:26-44; the Dense(10) that ends
 * tutorials/classifier_example.py:44-48 has C = 10 and stays on polus_gemm + polus_dense_bwd_params): y = x W^T + b, W [C][H]
 * row-major in `dtype`.  HBM-bound, one wave per row, no matrix
 * pipe: a 128-wide MFMA tile would compute 97 % padding.  polus_dense_thin_supported: 1 when (dtype, H, C) fits (C <= 8,
 * H a multiple of 16 bytes of elements, H <= 1024).  forward: y [rows][C] in y_dtype (f32 or dtype).  backward: dy [rows][C] in
 * dy_dtype (f32 or dtype); dx [rows][H] in dtype or NULL; dW [C][H] and db [C] (or NULL) f32, (+)= when accumulate; sums in a fixed
 * order (bitwise reproducible); workspace from polus_dense_thin_bwd_workspace_bytes. */
int polus_dense_thin_supported(int dtype, int H, int C);
int polus_dense_thin_fwd(int dtype, const void* x, long ldx, const void* W, long ldw, const float* bias,
                         int y_dtype, void* y, long ldy, int rows, int H, int C, void* stream);
size_t polus_dense_thin_bwd_workspace_bytes(int dtype, int rows, int H, int C);
int polus_dense_thin_bwd(int dtype, const void* x, long ldx, int dy_dtype, const void* dy, long lddy,
                         const void* W, long ldw, void* dx, long lddx, float* dW, long lddw, float* db,
                         int rows, int H, int C, int accumulate, void* workspace, size_t workspace_bytes, void* stream);

/* ---- fused scaled-dot-product attention (HF TFBertSelfAttention as driven by
 * TFBertSplited.call, polus/models.py:201-216, with the additive key mask
 * (1-m)*-10000 of polus/models.py:175-195).
 * qkv   [B*S, 3H] fused projections, row blocks Q | K | V, head h at columns h*64..h*64+63
 * mask  [B, S] int32 {0,1} (NULL = all ones)
 * ctx   [B*S, H]; lse [B, A, S] f32 = log-sum-exp of the masked, scaled scores
 * head_dim must be 64.  Backward recomputes the probabilities from lse; dqkv [B*S, 3H].
 * drop_p > 0: inverted dropout of the probabilities after the softmax (HF attention_probs_dropout),
 * mask = keep(seed, ((b*A+h)*S+q)*S+key), regenerated in backward.
 * workspace for bwd: B*A*S floats (row dot products dO.O), plus S/256 f32 dQ slabs of [B*S, H] for
 * S = 512 .. 2048 in whole 256-key blocks (key-resident one-pass backward).  The query is an upper bound over
 * every kernel route: it depends on the shape alone, not on dtype or on a POLUS_* switch.
 * polus_attention_route (host only, no HIP call) reports the kernels a call would run under the current
 * switches: *fwd = 1 LDS-DMA 4 waves, 2 LDS-DMA 8 waves, 3 wide bf16 8 waves, 4 wide f32 4 waves; *bwd = 1 one pass
 * 4 waves, 2 one pass 8 waves, 3 one pass 64-key blocks, 4 key-resident one block, 5 key-resident with dQ slabs,
 * 6 two kernels bf16, 7 two kernels f32.  Fails on a bad dtype or S < 1. */
int polus_attention_route(int dtype, int S, int* fwd, int* bwd);
int polus_attention_fwd(int dtype, const void* qkv, const int32_t* mask, void* ctx, float* lse,
                        int B, int S, int n_heads, int head_dim, float drop_p, uint32_t seed, void* stream);
size_t polus_attention_bwd_workspace_bytes(int B, int S, int n_heads);
int polus_attention_bwd(int dtype, const void* qkv, const int32_t* mask, const void* ctx,
                        const void* dctx, const float* lse, void* dqkv,
                        int B, int S, int n_heads, int head_dim, float drop_p, uint32_t seed,
                        void* workspace, size_t workspace_bytes, void* stream);

/* ---- LayerNorm over the feature axis, eps inside the sqrt, biased variance
 * (HF TFBertSelfOutput/TFBertOutput/TFBertEmbeddings LayerNorm, eps 1e-12).
 * fwd: y = (x-mean)*rstd*gamma+beta; mean/rstd [rows] f32 are saved for backward.
 * bwd: dx; dgamma/dbeta [H] f32 (+= when accumulate); if dbias != NULL also
 *      dbias[H] (+)= column sums of dx (the bias gradient of the Dense that produced x).
 *      When x = dropout(dense) + residual (drop_p > 0, mask index row*H+col as in polus_gemm_dropout):
 *      dx_masked = dx * mask/(1-p) is the gradient the Dense sees, and dbias sums dx_masked.
 *      With dgamma = dbeta = NULL the call stops after the main kernel and leaves the per-workgroup partial sums in
 *      `workspace` (dbias non-NULL still requests the bias sums); polus_layernorm_bwd_finalize then reduces them -- on any
 *      stream ordered behind the first call (the training step queues it behind the layer's weight-gradient launch on the
 *      side stream, off the critical path).  Same kernels in the same order: same bits. */
size_t polus_layernorm_bwd_workspace_bytes(int rows, int H);
int polus_layernorm_fwd(int dtype, const void* x, const float* gamma, const float* beta,
                        void* y, float* mean, float* rstd, int rows, int H, float eps, void* stream);
int polus_layernorm_bwd(int dtype, const void* dy, const void* x, const float* gamma,
                        const float* mean, const float* rstd, void* dx,
                        float* dgamma, float* dbeta, float* dbias, int accumulate,
                        int rows, int H, void* dx_masked, float drop_p, uint32_t seed,
                        void* workspace, size_t workspace_bytes, void* stream);
int polus_layernorm_bwd_finalize(void* workspace, size_t workspace_bytes, int rows, int H, float* dgamma, float* dbeta,
                                 float* dbias, int accumulate, void* stream);

/* ---- embeddings: word[ids] + pos[s] + type[tt] -> LayerNorm (HF TFBertEmbeddings; TF gather
 * has no padding_idx, so row 0 receives its gradient).  Tables and their gradients are f32.
 * bwd recomputes the pre-LN sum; gword rows are accumulated with f32 atomics unless
 * `deterministic`, in which case duplicates are summed in index order by one owner wave.
 * drop_p in [0, 1); drop_p > 0 drops elements of y, mask index row*H+col as above, and needs B*S*H < 2^32. */
size_t polus_embed_bwd_workspace_bytes(int B, int S, int H);
int polus_embed_ln_fwd(int dtype, const int32_t* ids, const int32_t* type_ids,
                       const float* word, const float* pos, const float* type,
                       const float* gamma, const float* beta, void* y, float* mean, float* rstd,
                       int B, int S, int H, int vocab, int max_pos, int type_vocab, float eps,
                       float drop_p, uint32_t seed, void* stream);
int polus_embed_ln_bwd(int dtype, const void* dy, const int32_t* ids, const int32_t* type_ids,
                       const float* word, const float* pos, const float* type, const float* gamma,
                       const float* mean, const float* rstd,
                       float* gword, float* gpos, float* gtype, float* ggamma, float* gbeta,
                       int accumulate, int deterministic,
                       int B, int S, int H, int vocab, int max_pos, int type_vocab,
                       float drop_p, uint32_t seed,
                       void* workspace, size_t workspace_bytes, void* stream);

/* polus_rowwise_route (host only, no HIP call) reports what the LayerNorm and embedding calls above would run for `rows`
 * rows of H features (rows = B*S for the embedding) under the current switches, from the functions their launchers call.
 * out[POLUS_ROWWISE_ROUTE_INTS]:
 *   [0] LayerNorm kernels: 1 f32 a wave per row, 2 bf16 a wave per row, 3 bf16 a half-wave per row
 *   [1] workgroups of polus_layernorm_fwd
 *   [2] workgroups of polus_layernorm_bwd given a 16-byte aligned dx_masked (one that is not takes route 2 where [0] says 3)
 *   [3] finalize launches after the LayerNorm backward: 1, or 2 above POLUS_LN_FIN_SINGLE workgroups
 *   [4] word-table scatter of polus_embed_ln_bwd: 1..4 atomic with runs combined, that many 256-feature chunks; 5 atomic, any H;
 *       6 owner (`deterministic`)
 *   [5] workgroups of the embedding forward   [6] workgroups of the embedding's LayerNorm backward (its finalize is always one launch)
 * Fails on a bad dtype, rows < 1, or an H that is no multiple of 4 in [4, 2048]. */
#define POLUS_ROWWISE_ROUTE_INTS 7
int polus_rowwise_route(int dtype, int rows, int H, int deterministic, int* out);

/* ---- column sums out[c] (+)= sum_r x[r][c]  (bias gradients) */
size_t polus_colsum_workspace_bytes(int rows, int cols);
int polus_colsum(int dtype, const void* x, long ldx, int rows, int cols, float* out, int accumulate,
                 void* workspace, size_t workspace_bytes, void* stream);

/* ---- losses.  logits are f32 [rows, C] (ld = ldl); dlogits is written in `dtype` (ld = lddl)
 * already divided by `rows` (tf.reduce_mean over every leading dim); loss is one f32.
 * softmax_xent: Keras SparseCategoricalCrossentropy(from_logits=True)
 *   (tutorials/classifier_example.py:55); class_weights != NULL gives polus/losses.py:5-18
 *   with one-hot targets (weight = class_weights[label]).
 * sigmoid_xent: polus/losses.py:21-41, y_true f32 multi-hot [rows, C]. */
size_t polus_loss_workspace_bytes(int rows);
int polus_softmax_xent(int dtype, const float* logits, long ldl, const int32_t* labels,
                       const float* class_weights, float* loss, void* dlogits, long lddl,
                       int rows, int C, void* workspace, size_t workspace_bytes, void* stream);
int polus_sigmoid_xent(int dtype, const float* logits, long ldl, const float* y_true, long ldy,
                       const float* class_weights, float negative_weight, float* loss,
                       void* dlogits, long lddl, int rows, int C,
                       void* workspace, size_t workspace_bytes, void* stream);

/* ---- softmax cross-entropy over rows of any width with ignored rows (xent_wide.hip): the masked-LM objective of the
 * original BERT recipe (HF BertForMaskedLM: CrossEntropyLoss(ignore_index = -100) over [rows, vocab]); the reference has no
 * pre-training step, its users start from checkpoints made by this objective.  One workgroup per row.
 *   logits [rows, V] in `dtype` (f32 or bf16), row stride ldl; labels int32 [rows]; dlogits in `dtype`, row stride lddl.
 *   label < 0: the row is ignored (0 to the loss, a zero dlogits row).  label >= V: ignored as well and counted in
 *   stats[1] (as polus_confusion_matrix counts `rejected`).  stats (device int32 [2], may be NULL) = {counted, rejected}.
 *   loss = sum over counted rows of (lse(row) - x[label]) / max(counted, 1); dlogits = (softmax - onehot) / max(counted, 1).
 *   dlogits may be the logits buffer itself (then lddl == ldl); any other overlap is undefined.
 * All arithmetic f32, expf / logf, gradient as exp((x - max) - log(sum)).  A row of at most 128 KiB is staged in LDS (one
 * HBM read, one write per element); a wider one is streamed (online max / sum, then a second read).  16-byte accesses
 * when logits, dlogits and both strides in bytes are multiples of 16, single elements otherwise: same results to the
 * last bit on the staged path.  No atomics; per-row losses are added in index order: bitwise reproducible.
 * polus_softmax_xent_wide_route (host only: no HIP call, no pointer dereferenced; the pointers count for their alignment)
 * reports what the call would run and fails where its validation fails: out[0] 0 staged / 1 streaming, out[1] 1 = 16-byte
 * accesses, out[2] dynamic LDS bytes. */
#define POLUS_XENT_WIDE_ROUTE_INTS 3
size_t polus_softmax_xent_wide_workspace_bytes(int rows);
int polus_softmax_xent_wide_route(int dtype, const void* logits, long ldl, const void* dlogits, long lddl,
                                  int rows, int V, int* out);
int polus_softmax_xent_wide(int dtype, const void* logits, long ldl, const int32_t* labels, float* loss,
                            void* dlogits, long lddl, int32_t* stats, int rows, int V,
                            void* workspace, size_t workspace_bytes, void* stream);
/* y[i] = x[idx[i]] for i < n where 0 <= idx[i] < rows, a zero row otherwise; x [rows, H] and y [n, H] in `dtype` with free
 * row strides (>= H), y != x.  Every element of y[0..n) is written.  Picks the masked positions out of [B S, H]; with the
 * inverse map it is also the scatter of the backward pass: deterministic, no atomics.
 * polus_inverse_map: inv[j] (int32 [rows]) = the LAST i < n with idx[i] == j, or -1; entries of idx outside [0, rows) are
 * skipped.  One workgroup; for index lists of a few thousand entries. */
int polus_gather_rows(int dtype, const void* x, long ldx, const int32_t* idx, void* y, long ldy,
                      int n, int rows, int H, void* stream);
int polus_inverse_map(const int32_t* idx, int n, int32_t* inv, int rows, void* stream);

/* ---- linear-chain CRF (polus/layers.py:58-126; tensorflow-addons crf_log_likelihood /
 * crf_decode restated).  potentials f32 [B,S,C]; tags int32 [B,S]; lengths int32 [B];
 * trans f32 [C,C] (already masked by the caller, polus/layers.py:58-63);
 * sample_w f32 [B] or NULL.  loss = mean_b(-ll_b * w_b).  dpot in `dtype`, dtrans f32 [C,C].
 * C <= 16: one thread per sequence; 17 <= C <= 128: one workgroup per sequence (crf.hip).
 * lengths outside [0, S] and tags outside [0, C) are clamped; tags at and past a sequence's length are
 * not read; dpot rows at and past it are written as zeros; the workspace need not be initialised.
 * Both paths agree with the float64 definition for any finite f32 potentials and transitions (masked
 * ones at -10000 included), however far apart, within the bounds recorded in tests/crf_cases.py. */
size_t polus_crf_workspace_bytes(int B, int S, int C);
int polus_crf_nll(int dtype, const float* potentials, const int32_t* tags, const int32_t* lengths,
                  const float* trans, const float* sample_w, float* loss, void* dpot,
                  float* dtrans, int accumulate, int B, int S, int C,
                  void* workspace, size_t workspace_bytes, void* stream);
int polus_crf_viterbi(const float* potentials, const int32_t* lengths, const float* trans,
                      int32_t* out_tags, int B, int S, int C,
                      void* workspace, size_t workspace_bytes, void* stream);

/* ---- token-level late interaction (ColBERT MaxSim) for dense retrieval.  The reference types the document
 * representation `# B, E or B, L, E` (polus/ir/training.py:51,63,98) and leaves the scoring of token vectors
 * to the user's `compute_scores`; these are its forward and backward (maxsim.hip).
 * Q [B,Lq,E] and D [N,Ld,E] in `dtype`, contiguous, 16-byte aligned; qmask int32 [B,Lq] and dmask int32 [N,Ld],
 * NULL = all ones; a token is valid where its mask is non-zero.
 *   score[b*lds + c]  = sum over valid i of max over valid j of <Q[b,i], D[c,j]>   (f32, lds >= N)
 *   argmax[b][c][i]   = the winning j (int32 [B,N,Lq]); ties go to the lowest j as computed; -1 for an invalid
 *                       query token or a document without a valid token (such a term adds 0).
 * bf16: v_mfma_f32_16x16x32_bf16 with f32 accumulation; f32: exact-f32 v_mfma_f32_16x16x4_f32 in a fixed k order.
 * Backward, from dscore f32 (row stride lds) and the forward's argmax, f32 sums rounded once to `dtype`:
 *   dQ[b,i] = sum over c ascending of dscore[b,c] * D[c, argmax[b,c,i]]
 *   dD[c,j] = sum over (b,i) ascending with argmax[b,c,i] == j of dscore[b,c] * Q[b,i]
 * Every element of dQ and dD is written (0 where nothing lands); no atomics, bitwise reproducible; no workspace.
 * Limits (refused before any launch): E a multiple of 32 in [32, 256]; 1 <= Lq, Ld <= 512; B, N <= 65535;
 * B*N*Lq < 2^31. */
int polus_maxsim_fwd(int dtype, const void* Q, const void* D, const int32_t* qmask, const int32_t* dmask,
                     float* score, long lds, int32_t* argmax, int B, int N, int Lq, int Ld, int E, void* stream);
/* The forward without the argmax, for scoring a corpus (polus_amd/ir/search.py): the same kernel body with the
 * argmax stores compiled out, so score is bit for bit what polus_maxsim_fwd writes for the same inputs, and 4*B*N*Lq
 * bytes less leave the chip.  Limits: those of polus_maxsim_fwd without B*N*Lq < 2^31 (that one is the argmax's). */
int polus_maxsim_scores(int dtype, const void* Q, const void* D, const int32_t* qmask, const int32_t* dmask,
                        float* score, long lds, int B, int N, int Lq, int Ld, int E, void* stream);
int polus_maxsim_bwd(int dtype, const void* Q, const void* D, const float* dscore, long lds,
                     const int32_t* argmax, void* dQ, void* dD, int B, int N, int Lq, int Ld, int E, void* stream);
/* Re-ranking (rerank.hip): every query scores its own list of candidate documents, the second stage of a two-stage
 * search.  Q [B,Lq,E], qmask [B,Lq] as above; D [N,Ld,E] and dmask int32 [N,Ld] (NULL = all ones) hold the whole
 * stored corpus; cand int32 [B,C], row stride ldc >= C, names documents of D; score f32 [B,C], row stride lds >= C.
 *   score[b*lds + c] = the MaxSim score of query b and document cand[b*ldc + c], bit for bit what polus_maxsim_scores
 *                      writes for that pair (the same fragments and MFMAs in ascending k, the same summation tree and
 *                      tile order): a document without a valid token and a query without one score 0.0;
 *                    = -inf where cand[b*ldc + c] < 0 or >= N: the entry is absent and nothing of it is dereferenced
 *                      (-inf is what polus_topk_merge and polus_topk_merge_ids drop).
 * Columns of score past C are not written.  One workgroup per (query, block of candidates); a wave keeps the query's
 * tiles in registers and streams its own documents from global memory, skipping the 16-token tiles behind a
 * document's last valid token (masked tokens never win, so the bits do not change); queries of more tiles than a
 * wave holds take rounds over the document.  Document addresses are 64-bit.  No LDS, no atomics, no workspace;
 * bitwise reproducible.  Memory-bound: each candidate's valid tiles are read once per query.
 * Limits (refused before any launch): dtype f32 or bf16; E a multiple of 32 in [32, 256]; 1 <= Lq, Ld <= 512;
 * 1 <= B <= 65535; 1 <= C <= 65535; 1 <= N <= 2^31 - 1; ldc >= C; lds >= C; Q, D, cand, score non-null; Q and D
 * 16-byte aligned. */
int polus_maxsim_rerank(int dtype, const void* Q, const void* D, const int32_t* qmask, const int32_t* dmask,
                        const int32_t* cand, long ldc, float* score, long lds,
                        int B, int C, int N, int Lq, int Ld, int E, void* stream);
/* ---- FP8 token index (maxsim_fp8.hip): document token vectors stored as OCP e4m3fn codes (not fnuz) with one f32
 * scale per token, an exact power of two, 8 + E bytes per token with the int32 mask against 4 + 2E in bf16.
 * Quantiser, per row x[0..E), integers only:
 *   amax = max |x_k| = m * 2^k with m in [0.5, 1) (frexp);   e = max(k - 9 + (m > 0.875), -100), e = 0 if amax == 0;
 *   scale = 2^e;   code_k = e4m3fn(x_k / 2^e), round to nearest even.
 * e is the smallest exponent with amax / 2^e <= 448, so nothing saturates and a non-zero row's largest code lies in
 * (224, 448] unless the clamp at -100 holds it lower.  Contract: finite x with amax <= 2^100.  A NaN element is
 * ignored by amax and becomes a NaN code; an infinite or larger amax gives unspecified codes and scale.  No input makes
 * the kernel touch memory outside its rows.
 * Dequantisation is y = T(code) * scale: an e4m3 value has at most 4 significant bits, so both steps are exact in f32
 * and in bf16 (as long as code * scale stays a normal number of T, which scale >= 2^-100 guarantees).
 * x, y [rows, E] in `dtype` (f32 or bf16), codes uint8 [rows, E], scale f32 [rows]; one wave per row.
 * Limits (refused before any launch): rows >= 1; E a multiple of 4 in [4, 256]; non-null pointers; x / y and codes
 * 16-byte aligned. */
int polus_fp8_quantize_rows(int dtype, const void* x, uint8_t* codes, float* scale, int rows, int E, void* stream);
int polus_fp8_dequantize_rows(int dtype, const uint8_t* codes, const float* scale, void* y, int rows, int E,
                              void* stream);
/* polus_maxsim_scores and polus_maxsim_rerank over an FP8 corpus: codes uint8 [N,Ld,E] and scale f32 [N,Ld] stand in
 * for D; Q stays in `dtype` (f32 or bf16), every other argument and every word of the counterpart's contract holds
 * (masks, strides, -inf for absent candidates with nothing dereferenced, columns past N / C not written, tiles behind
 * a document's last valid token skipped, the resident-query and the rounds route).  The code bytes are converted to
 * `dtype` in registers and fed to the counterpart's fragments and MFMAs in the same k order; an accumulator row (a
 * document token) is multiplied by its token's scale before the mask and the max; the reduction is the counterpart's.
 * A power-of-two scale commutes with every rounding of the sum, so
 *   polus_maxsim_scores_fp8(Q, codes, scale) is bit for bit polus_maxsim_scores(Q, D) with D = T(codes) * scale,
 *   polus_maxsim_rerank_fp8 is bit for bit polus_maxsim_scores_fp8 of each (query, candidate) pair,
 * provided no product or partial sum under- or overflows f32 (scales of a unit-norm or N(0,1) corpus are ~2^-8).
 * All quantisation error therefore sits in polus_fp8_quantize_rows.  Memory-bound like the counterparts, on half the
 * document bytes.
 * Limits (refused before any launch): those of the counterpart, with codes 16-byte aligned and scale non-null. */
int polus_maxsim_scores_fp8(int dtype, const void* Q, const uint8_t* codes, const float* scale, const int32_t* qmask,
                            const int32_t* dmask, float* score, long lds, int B, int N, int Lq, int Ld, int E,
                            void* stream);
int polus_maxsim_rerank_fp8(int dtype, const void* Q, const uint8_t* codes, const float* scale, const int32_t* qmask,
                            const int32_t* dmask, const int32_t* cand, long ldc, float* score, long lds,
                            int B, int C, int N, int Lq, int Ld, int E, void* stream);
/* ---- Residual-compressed token index (residual.hip; ColBERTv2): a document token is stored as the 16-bit id of its
 * nearest centroid plus nbits = 1, 2 or 4 bits per dimension that name a bucket of its residual: 2 + E*nbits/8 bytes
 * per token, 38 at E = 128 and nbits = 2 with the int32 mask, against 260 in bf16 and 136 in FP8.
 * A codec is
 *   centroids [K, E] in `dtype` (f32 or bf16), 1 <= K <= 65535;   nbits in {1, 2, 4};
 *   cutoffs f32 [2^nbits - 1], non-decreasing;   weights f32 [2^nbits];
 * a token is
 *   code   uint16: its centroid.  Any code >= K means "no token", 0xFFFF among them, as in polus_centroid_scores;
 *   packed uint8 [E*nbits/8].
 * Rules, per element k of a row with code < K:
 *   residual   r_k = f32(x_k) - f32(centroids[code][k]), one f32 subtraction;
 *   bucket     bucket_k = the number of cutoffs c_j with r_k > c_j (IEEE comparison): a residual equal to a cutoff goes
 *              to the lower bucket, NaN to bucket 0, +inf to the top bucket (unless a cutoff is +inf itself);
 *   packing    element k sits in byte k*nbits/8 (integer division) at bits [nbits*(k mod 8/nbits), +nbits), least
 *              significant first: at nbits = 2 byte 0 holds elements 0..3, element 0 in bits 0-1;
 *   decode     y_k = T(f32(centroids[code][k]) + weights[bucket_k]): one f32 addition, then one round-to-nearest-even
 *              conversion to `dtype` (none for f32).
 * A row with code >= K: its packed bytes are all zero on compress and its y is all (+0) zeros on decode, and nothing of
 * centroids is dereferenced for it.  Cutoffs and weights are taken as given (the cutoffs' order is not checked here).
 * x, y [rows, E]; codes uint16 [rows]; packed uint8 [rows, E*nbits/8]; one thread per 8 elements; no workspace, no
 * atomics, bitwise reproducible.
 * Limits (refused before any launch): dtype f32 or bf16; nbits 1, 2 or 4; E a multiple of 32 in [32, 256];
 * 1 <= K <= 65535; rows >= 1; non-null pointers; x / y and centroids 16-byte aligned, packed 4-byte aligned. */
int polus_residual_compress(int dtype, const void* x, const uint16_t* codes, const void* centroids, int K,
                            const float* cutoffs, int nbits, uint8_t* packed, int rows, int E, void* stream);
int polus_residual_decompress(int dtype, const uint16_t* codes, const uint8_t* packed, const void* centroids, int K,
                              const float* weights, int nbits, void* y, int rows, int E, void* stream);
/* polus_maxsim_rerank over a residual-compressed corpus: codes uint16 [N,Ld] and packed uint8 [N,Ld,E*nbits/8] with the
 * codec's centroids [K,E] (in `dtype`, like Q) and weights stand in for D; every other argument and every word of
 * polus_maxsim_rerank's contract holds (masks, strides, -inf for absent candidates with nothing dereferenced, columns
 * past C not written, tiles behind a document's last valid token skipped, the resident-query and the rounds route, the
 * same documents per wave).  A lane reads its row's code (the document's codes are loaded a document ahead, like its
 * mask), its nbits bytes of residual bits per 32-wide k-step and the matching 8 elements of the centroid row, and forms
 * T(c + weights[bucket]) in registers with the decoder's own arithmetic; the fragments go to polus_maxsim_rerank's
 * MFMAs in the same k order and its reduction follows.  So
 *   polus_maxsim_rerank_res(Q, codes, packed, ...) is bit for bit polus_maxsim_rerank(Q, D) with
 *   D = polus_residual_decompress(codes, packed, ...),
 * and the quantiser holds all of the error.  A token with code >= K reads centroid 0 as a stand-in and counts as a row of
 * zeros, as in D.  The weights stay in registers; no LDS, no barrier, no atomics, no workspace.  The centroid rows
 * (2E bytes per decoded token in bf16) come through L2 / Infinity Cache.
 * Limits (refused before any launch): those of polus_maxsim_rerank and of the codec above; Q and centroids 16-byte
 * aligned, packed 4-byte aligned; codes, packed, centroids, weights non-null. */
int polus_maxsim_rerank_res(int dtype, const void* Q, const uint16_t* codes, const uint8_t* packed,
                            const void* centroids, int K, const float* weights, int nbits, const int32_t* qmask,
                            const int32_t* dmask, const int32_t* cand, long ldc, float* score, long lds,
                            int B, int C, int N, int Lq, int Ld, int E, void* stream);
/* Row L2 normalisation, torch.nn.functional.normalize(x, dim=-1, eps) (ColBERT's cosine): x, y [rows,E] in
 * `dtype` (E <= 256), rnorm f32 [rows].  Forward (f32 arithmetic): y = x / max(|x|, eps), rnorm = 1 / max(|x|, eps).
 * Backward: dx = (dy - y <y, dy>) * rnorm where |x| > eps, dy / eps otherwise.  One wave per row. */
int polus_l2norm_fwd(int dtype, const void* x, void* y, float* rnorm, int rows, int E, float eps, void* stream);
int polus_l2norm_bwd(int dtype, const void* y, const float* rnorm, const void* dy, void* dx, int rows, int E,
                     float eps, void* stream);

/* ---- tuple scoring for retrieval distillation (tuples.hip): query b is scored against its OWN n documents only (an
 * n-way tuple: the positive and n - 1 negatives, with a teacher's scores for them), not against all N = B n of the step.
 * The N documents sit in one contiguous buffer; `layout` names the row of document (b, j):
 *   0, slot-major:  j*B + b  (what the retrieval trainers build: positives first, then negative block i);
 *   1, query-major: b*n + j.
 * MaxSim tuples.  Q [B,Lq,E], D [B*n,Ld,E] in `dtype`, contiguous, 16-byte aligned; qmask int32 [B,Lq], dmask int32
 * [B*n,Ld], NULL = all ones.
 *   score[b*lds + j] = MaxSim(Q[b], D[doc(b,j)])  (f32, lds >= n);
 *   argmax int32 [B,n,Lq]: the winning document token, lowest j on ties, -1 for an invalid query token or a document
 *   without a valid token.
 * score and argmax are bit for bit what polus_maxsim_fwd writes for the pair (b, doc(b,j)): the same fragments, MFMAs in
 * ascending k, the same running (value, j) pick, the same xor-shuffle sum of a tile's 16 maxima, tiles added in ascending
 * order.  One wave per pair keeps the query's tiles in registers and streams the document from global memory (no LDS,
 * no barrier), skipping the tiles behind its last valid token; queries of more tiles than a wave holds take rounds.
 * Backward, from dscore f32 [B,n] (row stride lds) and the forward's argmax:
 *   dQ[b,i]         = sum over j ascending of dscore[b,j] * D[doc(b,j), argmax[b,j,i]]
 *   dD[doc(b,j), t] = sum over i ascending with argmax[b,j,i] == t of dscore[b,j] * Q[b,i]
 * f32 fmaf chains in that order from +0, rounded once to `dtype`; every element of dQ and dD is written (0 where nothing
 * lands); no atomics, no workspace, bitwise reproducible.  Order and arithmetic are polus_maxsim_bwd's, so the results
 * equal what it gives for a B x N dscore that is zero outside the tuple entries and the all-pairs argmax.
 * Limits (refused before any launch): dtype f32 or bf16; E a multiple of 32 in [32, 256]; 1 <= Lq, Ld <= 512;
 * 1 <= B <= 65535; 1 <= n <= 65535; B*n <= 2^31 - 1; B*n*Lq < 2^31; lds >= n; layout 0 or 1; forward: Q and D 16-byte
 * aligned; no null pointer but the masks. */
int polus_maxsim_tuples_fwd(int dtype, const void* Q, const void* D, const int32_t* qmask, const int32_t* dmask,
                            float* score, long lds, int32_t* argmax, int B, int n, int layout, int Lq, int Ld, int E,
                            void* stream);
int polus_maxsim_tuples_bwd(int dtype, const void* Q, const void* D, const float* dscore, long lds,
                            const int32_t* argmax, void* dQ, void* dD, int B, int n, int layout, int Lq, int Ld, int E,
                            void* stream);
/* Dot tuples, for single vectors ([CLS] embeddings, SPLADE representations over the vocabulary): q [B,W] (row stride
 * ldq) and d [B*n,W] (row stride ldd) in `dtype`, the same `layout`.
 *   score[b*lds + j] = sum_w q[b,w] * d[doc(b,j),w], f32.  Order: a row is cut into chunks of 16 / sizeof(dtype)
 *   elements; one wave per pair, lane l takes chunks l, l + 64, ... and adds their elements in ascending w to one fmaf
 *   chain from +0; the 64 lane sums meet in the xor-shuffle tree 32, 16, .., 1.
 *   dq[b]        = sum over j ascending of dscore[b,j] * d[doc(b,j)]   (fmaf chain from +0, rounded once; stride lddq)
 *   dd[doc(b,j)] = dscore[b,j] * q[b]                                  (one product, rounded once; stride lddd)
 * Every element of dq and dd is written.  Whole chunks move as 16-byte accesses when every row pointer involved and
 * every row stride in bytes is a multiple of 16, element by element otherwise: the same bits either way.
 * Limits: W >= 1; 1 <= B, n <= 65535; B*n <= 2^31 - 1; lds >= n; row strides >= W; layout 0 or 1. */
int polus_dot_tuples_fwd(int dtype, const void* q, long ldq, const void* d, long ldd, float* score, long lds,
                         int B, int n, int layout, int W, void* stream);
int polus_dot_tuples_bwd(int dtype, const void* q, long ldq, const void* d, long ldd, const float* dscore, long lds,
                         void* dq, long lddq, void* dd, long lddd, int B, int n, int layout, int W, void* stream);
/* Distillation losses over tuple scores: student and teacher f32 [rows,n] (row strides lds, ldt), loss f32 [1],
 * dstudent f32 [rows,n] (row stride ldd), every element written.  A column whose teacher score is -inf (what
 * polus_maxsim_rerank writes for a missing candidate) is absent: left out of every sum, gradient 0, its student value
 * never used.  f32 arithmetic, one wave per row, per-row results added in index order by a second kernel: no atomics,
 * bitwise reproducible.
 * polus_distill_kl, over the present columns of a row: p = softmax(teacher), s = log_softmax(student), each with its
 *   own maximum subtracted; loss = sum over rows of sum_j p_j (log p_j - s_j) / rows; dstudent = (softmax(student) - p)
 *   / rows; a row without a present column adds 0 and gets a zero row.
 * polus_margin_mse: column 0 is the positive; with m present negatives j >= 1 in a row whose column 0 is present and
 *   M = the sum of m over those rows, loss = sum over them of ((s_0 - s_j) - (t_0 - t_j))^2 / max(M, 1) and dstudent its
 *   exact gradient; a row whose column 0 is absent contributes nothing and gets a zero row.
 * Limits: rows >= 1; 1 <= n <= 1024; row strides >= n; workspace >= polus_distill_workspace_bytes(rows) (host only). */
size_t polus_distill_workspace_bytes(int rows);
int polus_distill_kl(const float* student, long lds, const float* teacher, long ldt, float* loss, float* dstudent,
                     long ldd, int rows, int n, void* workspace, size_t workspace_bytes, void* stream);
int polus_margin_mse(const float* student, long lds, const float* teacher, long ldt, float* loss, float* dstudent,
                     long ldd, int rows, int n, void* workspace, size_t workspace_bytes, void* stream);

/* ---- cross-encoder pair rows (pairs.hip; HF BertTokenizer(q, d, truncation="only_second", padding="max_length")
 * restated over token ids): a reranker scores pairs `[CLS] query [SEP] document [SEP]`, built here on the device from
 * query rows, document rows and a candidate table.  Integers only: every result is exact.
 * Inputs.  q_ids, qmask int32 [B, Lq] (row strides ldq, ldqm); d_ids, dmask int32 [N, Ld] (row strides ldd, lddm); a
 *   NULL mask is all ones.  cand int32 [B, n], row stride ldc.
 * Valid tokens.  The valid tokens of a row are those whose mask is non-zero, in order: holes and left padding are
 *   compacted away.
 * Stripping.  Of a query's valid tokens the first q_head and the last q_tail are dropped, of a document's the first
 *   d_head and the last d_tail; each count is in 0..8, and dropping more than there are leaves none.  1/1 takes the
 *   [CLS] and [SEP] off HF-tokenised inputs, 0/0 uses raw ids as they are.  nq, nd = what is left.
 * Truncation.  nq' = min(nq, max_q), nd' = min(nd, S - 3 - nq'), the FIRST tokens of each (HF's only_second).
 *   S >= max_q + 3 is required.
 * Pair index.  Pair p has query b = p / n and document cand[b*ldc + p % n].  Output row r is pair rows[r] (int32 [R]),
 *   or pair r when rows is NULL; the same p may appear more than once in rows.  A value of rows outside [0, B*n) is
 *   the caller's error: it is not detected and reads out of bounds.
 * Output row.  cls, q'.., sep, d'.., sep, then pad up to S.  token_type_ids is 0 through the first sep, 1 through the
 *   second and 0 on padding; attention_mask is 1 on the length = nq' + nd' + 3 real tokens and 0 behind them.
 * Missing candidates.  A candidate id outside [0, N) gives the empty-document pair `cls q' sep sep` (length nq' + 3); no
 *   document memory is read for it.  No row comes out fully masked: length >= 3.
 * Writes.  Every element of the S columns of input_ids, token_type_ids and attention_mask (int32 [R, S], one row
 *   stride ldo >= S) is written, and nothing beyond column S - 1.
 * polus_pair_lengths writes only length int32 [R], from the same arguments (the host plans buckets from it).
 * polus_pair_pack writes the three outputs and length (NULL: not written).  One wave per output row; compaction by
 *   __ballot and a popcount prefix over 64-token steps; plain stores, no LDS, no atomics, no workspace.
 * polus_pair_scatter_scores, for DISTINCT rows: out[b*ldo + j] = s[r] when the candidate of pair rows[r] = b*n + j
 *   exists and -inf when it does not (what polus_maxsim_rerank writes and polus_distill_kl reads as "absent"); s f32
 *   [R]; entries of out (f32 [B, n], row stride ldo) that rows does not name are left alone.
 * Limits (refused before any launch): no null pointer but the masks, rows and polus_pair_pack's length; R, B, n, N,
 *   Lq, Ld >= 1; B*n <= 2^31 - 1; row strides >= the widths; strips in 0..8; max_q >= 0; S >= max_q + 3. */
int polus_pair_lengths(const int32_t* qmask, long ldqm, const int32_t* dmask, long lddm, const int32_t* cand, long ldc,
                       const int32_t* rows, int R, int B, int n, int N, int Lq, int Ld, int q_head, int q_tail,
                       int d_head, int d_tail, int max_q, int S, int32_t* length, void* stream);
int polus_pair_pack(const int32_t* q_ids, long ldq, const int32_t* qmask, long ldqm, const int32_t* d_ids, long ldd,
                    const int32_t* dmask, long lddm, const int32_t* cand, long ldc, const int32_t* rows, int R, int B,
                    int n, int N, int Lq, int Ld, int q_head, int q_tail, int d_head, int d_tail, int max_q, int S,
                    int cls, int sep, int pad, int32_t* input_ids, int32_t* token_type_ids, int32_t* attention_mask,
                    long ldo, int32_t* length, void* stream);
int polus_pair_scatter_scores(const float* s, const int32_t* rows, const int32_t* cand, long ldc, int R, int B, int n,
                              int N, float* out, long ldo, void* stream);

/* ---- exact running top-k of score rows, for corpus search (topk.hip).  scores f32 [rows, n], row stride lds >= n;
 * column c is the document with id id0 + c.  top_val f32 and top_id int32, contiguous [rows, k], hold the running
 * state and are rewritten.  Per row:
 *   candidates = the entries of the incoming state with id >= 0, plus (scores[r][c], id0 + c) for c < n; with
 *                init != 0 the incoming state is ignored and never read;
 *   dropped    = candidates whose score is NaN or -inf (-inf is how a caller masks a document out);
 *   order      = score descending by IEEE comparison (-0.0 equals +0.0 and either may come back as +0.0), ties to the
 *                lower id;
 *   output     = the best k candidates in that order; when fewer than k remain the tail is (-inf, -1).
 * With init == 0 the state must come from an earlier call and its ids must be disjoint from the chunk's: duplicates
 * are not detected.  The result is exact: a corpus merged in any chunking gives bit for bit the result of one call
 * over the whole row.  One workgroup per row keeps the top k and a candidate buffer as 64-bit keys (orderable score
 * bits, then the complemented id: a total order) in LDS and bitonic-sorts them when the buffer fills; no float
 * atomics, bitwise reproducible, no workspace.  Memory-bound: one read of 4*rows*n bytes.
 * Limits (refused before any launch): 1 <= k <= 1024; rows >= 1; n >= 1; id0 >= 0; id0 + n <= 2^31 - 1; lds >= n;
 * non-null pointers. */
int polus_topk_merge(const float* scores, long lds, int rows, int n, int32_t id0,
                     float* top_val, int32_t* top_id, int k, int init, void* stream);
/* polus_topk_merge over columns that carry their own ids (the scores of polus_maxsim_rerank): column c of row r is the
 * document ids[r*ldi + c] (int32 [rows, n], row stride ldi >= n; rows need no alignment beyond 4 bytes), and a column
 * whose id is negative is dropped whatever its score.  Everything else is the contract above: NaN and -inf dropped,
 * score descending by IEEE comparison, ties to the lower ID (not the lower column), (-inf, -1) padding, `init`, exact and
 * independent of the chunking and of the column order, no float atomics, no workspace.  That guarantee is for rows
 * whose ids, together with the incoming state's, are distinct.  A duplicate id is not detected: each copy competes as
 * an entry of its own and may come back beside the others, but a copy whose (score, id) equals the k-th entry held
 * when its tile is read is passed over, so how many copies of an id return can depend on the chunking and the column
 * order.  Entries of other ids that rank above every copy are not affected.
 * Limits (refused before any launch): 1 <= k <= 1024; rows >= 1; n >= 1; lds >= n; ldi >= n; non-null pointers. */
int polus_topk_merge_ids(const float* scores, long lds, const int32_t* ids, long ldi, int rows, int n,
                         float* top_val, int32_t* top_id, int k, int init, void* stream);

/* ---- centroid-pruned search of a token index (centroid.hip; ColBERTv2 / PLAID candidate generation).  Every stored
 * document token is replaced by the id of its nearest centroid, an unsigned 16-bit code; 0xFFFF means "no token"
 * (masked or padding), and any other code >= K is absent too: nothing is dereferenced for it.
 *
 * polus_centroid_scores, the approximate MaxSim by table look-ups:
 *   table  f32 [K, >= B*Lq], row stride ldt:  table[c*ldt + b*Lq + i] = <centroid c, Q[b,i]>   (one polus_gemm)
 *   qmask  int32 [B, Lq] or NULL (all ones);  codes uint16 [N, Ld] contiguous;  score f32 [B, N], row stride lds >= N
 *   score[b*lds + n] = sum over valid i of  max over present j of  table[codes[n,j]*ldt + b*Lq + i]
 * A query token without a present document token adds 0.0, so an empty document and an empty query score 0.0 as in
 * polus_maxsim_scores.  Columns of score past N are not written.  The table is assumed finite.  The max is exact; the
 * sum over i is f32 in an order fixed by Lq alone (a lane's query tokens i, i + 64, ... ascending, then one xor-shuffle
 * tree over the wave), so the bits of score[b, n] depend on that (query, document) pair only: not on B, N, the other
 * queries and documents of the launch, the chunking of a corpus, or the route.  No atomics, no workspace, bitwise
 * reproducible.  One workgroup per (query, contiguous range of documents, sized so that a launch has about four
 * workgroups per CU and a range at least 4 documents per wave); a wave owns a pair from its first look-up to the store.
 * Two routes, chosen from Lq and K alone:
 *   1 LDS-resident: the workgroup (1024 threads) copies the query's [K, Lq] slice of the table into dynamic LDS, rows
 *     packed at a stride of Lq floats without padding, plus one row of -inf that absent codes read:
 *     LDS bytes = (K + 1) * Lq * 4, and the route is taken iff that is <= 163840 (160 KiB, one CU's LDS; K <= 1279 at
 *     Lq = 32).  A step of a wave reads whole contiguous rows: one row (Lq > 32), two (17 .. 32) or 64 / P rows of
 *     P = 2^ceil(log2 Lq) floats (Lq <= 16).
 *   2 global gather: 256 threads, the same loop with the rows read from global memory (L2 / Infinity Cache resident in
 *     practice); serves every K * Lq too large for LDS.
 * polus_centroid_scores_route (host only, no HIP call) reports out[0] = the route (1 or 2) and out[1] = the dynamic LDS
 * bytes of route 1 (0 for route 2); it applies the shape limits below.
 * Limits (refused before any launch): 1 <= Lq, Ld <= 512; 1 <= K <= 65535; 1 <= B, N <= 65535; ldt >= B*Lq; lds >= N;
 * table, codes, score non-null. */
#define POLUS_CENTROID_ROUTE_INTS 2
int polus_centroid_scores_route(int B, int N, int Lq, int Ld, int K, int* out);
int polus_centroid_scores(const float* table, long ldt, const int32_t* qmask, const uint16_t* codes,
                          float* score, long lds, int B, int N, int Lq, int Ld, int K, void* stream);
/* The nearest centroid of each row of a similarity matrix (tokens x centroids^T from polus_gemm):
 *   sim f32 [rows, K], row stride lds >= K;  mask int32 [rows] or NULL;  codes uint16 [rows]
 *   codes[r] = 0xFFFF where mask[r] == 0, else the first (lowest) c that maximises sim[r, c] by IEEE comparison
 *              (-0.0 equals +0.0).  A NaN never wins; a row of NaN only gives 0.
 * One wave per row, 16-byte reads where the row is 16-byte aligned (4-byte reads otherwise); candidates are ordered by
 * (value descending, column ascending), a total order, so the result does not depend on how lanes split the row.
 * Limits (refused before any launch): rows >= 1; 1 <= K <= 65535; lds >= K; sim, codes non-null. */
int polus_centroid_codes(const float* sim, long lds, const int32_t* mask, uint16_t* codes, int rows, int K, void* stream);
/* One spherical k-means update:
 *   x [T, E] in `dtype` (f32 / bf16);  codes uint16 [T];  prev, out [K, E] in `dtype` (out must not alias prev);
 *   counts int32 [K]
 *   sum_k     = f32 sum of x[t] over the t with codes[t] == k;   counts[k] = how many such t
 *   out[k]    = sum_k / |sum_k|, rounded once to `dtype`, if counts[k] > 0 and |sum_k| > eps;   prev[k] otherwise
 * Codes >= K (0xFFFF among them) belong to no centroid and are skipped.  One workgroup of 4 waves per centroid scans the
 * code array: wave w adds the rows of tokens [w*ceil(T/4), (w+1)*ceil(T/4)) in ascending t, the four partials are added
 * as (w0 + w1) + (w2 + w3); |sum_k|^2 is an f32 sum over the features in a fixed tree.  No atomics, no workspace, bitwise
 * reproducible.  Index-build time work: K reads of the code array.
 * Limits (refused before any launch): dtype f32 or bf16; E a multiple of 32 in [32, 256]; T >= 1; 1 <= K <= 65535;
 * non-null pointers. */
int polus_centroid_update(int dtype, const void* x, const uint16_t* codes, const void* prev, void* out,
                          int32_t* counts, int T, int K, int E, float eps, void* stream);
/* polus_centroid_scores over a candidate list per query (the probed search, ivf.hip below):
 *   cand int32 [B, C], row stride ldc >= C;  score f32 [B, C], row stride lds >= C;  codes uint16 [N, Ld] as above
 *   score[b*lds + c] = the bits polus_centroid_scores gives the pair (b, cand[b*ldc + c]): the same kernel body, lane
 *                      mapping and summation order on either route, the document index alone taken from cand.
 *   cand[b, c] < 0 or >= N:  score = -inf and nothing is read for it (-inf is what polus_topk_merge_ids drops).
 * A repeated id is scored once per copy.  Columns of score past C are not written.  No atomics, no workspace, bitwise
 * reproducible.  The routes are polus_centroid_scores' (polus_centroid_scores_route with N = C).
 * Limits (refused before any launch): 1 <= Lq, Ld <= 512; 1 <= K <= 65535; 1 <= B, C <= 65535; N >= 1; ldt >= B*Lq;
 * ldc >= C; lds >= C; table, codes, cand, score non-null. */
int polus_centroid_scores_ids(const float* table, long ldt, const int32_t* qmask, const uint16_t* codes,
                              const int32_t* cand, long ldc, float* score, long lds, int B, int C, int N, int Lq, int Ld,
                              int K, void* stream);

/* ---- inverted centroid lists and probed candidate generation for a token index (ivf.hip; the first step of PLAID,
 * ColBERTv2's retrieval: no counterpart in the reference).  The list of centroid c names the documents that hold at
 * least one present token coded c; a query probes the lists of the nprobe centroids nearest to each of its tokens, the
 * union of those lists is its candidate set, and polus_centroid_scores_ids scores only that set.
 *
 * The lists, in CSR form:  offsets int32 [K + 1], offsets[0] = 0, offsets[K] = P, the number of (centroid, document)
 * pairs;  docs int32 [P];  docs[offsets[c] .. offsets[c+1]) holds the ids of the documents of centroid c, each exactly
 * once however many of its tokens share c.  THE ORDER OF THE IDS INSIDE ONE LIST IS UNSPECIFIED (it follows the order
 * in which workgroups reach a cursor and may differ from run to run); the lists as SETS, counts and offsets are exact
 * and reproducible (integer arithmetic).  Nothing downstream depends on the order: a list is only ever OR-ed into a
 * bitmap.  codes uint16 [N, Ld] contiguous are polus_centroid_scores'; a code >= K (0xFFFF among them) is no token.
 * The caller owns every buffer; nothing is allocated here.  Built in three steps:
 *   polus_ivf_count:    counts int32 [K] (zeroed by the call itself): counts[c] = documents with a present token c.
 *                       One wave per document: its codes go to LDS, a token counts iff no earlier token of the document
 *                       has its code, and each such token adds 1 to its centroid's counter (int32 vector atomics).
 *   polus_ivf_offsets:  the exclusive scan of counts, one workgroup, 64-bit sums.  P >= 2^31 cannot be addressed: then
 *                       offsets[K] = -1 and offsets[0 .. K) are unspecified; the caller reads offsets[K] (it needs P to
 *                       allocate docs) and must refuse a negative value.
 *   polus_ivf_fill:     cursor int32 [K] is scratch (zeroed by the call itself, meaningless afterwards).  The same walk
 *                       as count; a counted token takes slot = cursor[c]++ and stores its document id at
 *                       docs[offsets[c] + slot], only if that index is < offsets[c+1] and < P: offsets that belong to
 *                       other codes lose entries, they never write out of range.
 * polus_ivf_mark, the candidate set as a bitmap:
 *   probes int32 [B*Lq, nprobe], row stride ldp >= nprobe (the ids polus_topk_merge leaves: -1 padded);  qmask int32
 *   [B, Lq] or NULL (all ones);  bitmap uint32 [B, W], W = ceil(N / 32), row stride ldb >= W words.
 *   The call first clears the W words of every row (words past W are not touched), then sets bit d & 31 of word
 *   d >> 5 of row b for every d in the list of every probe (b, i, p) with qmask[b, i] != 0 and 0 <= probe < K.  Any
 *   other probe value is skipped and nothing is dereferenced for it.  A list position outside [0, P) is not read, a
 *   list entry outside [0, N) is not written through, so stale or foreign lists cannot fault; bits >= N of the last
 *   word stay 0.  The result is a set: exact, independent of scheduling and of the order inside the lists (int32 vector
 *   atomic OR, skipped where the bit is seen set).  Work is spread by list ENTRIES, not by lists: a query's probes are
 *   taken 256 at a time, their list lengths are prefix-summed in LDS, and the entries of the tile are dealt out evenly
 *   to the query's workgroups (a binary search finds an entry's list), so one centroid that holds most of the corpus
 *   costs no more than many small ones.
 * polus_ivf_compact, the bitmap as ascending ids:
 *   count int32 [B]: count[b] = the set bits of row b among bits [0, N), the full number also when it exceeds cap.
 *   cand int32 [B, cap] (row stride ldc >= cap) or NULL: cand[b, 0 .. min(count[b], cap)) = the set positions in
 *   ascending order, the rest of the row up to cap = -1.  cand == NULL (cap ignored) is the count-only call that sizes
 *   the buffer.  One workgroup per row: popcounts and a prefix sum over the words, no atomics, deterministic.
 * Limits (refused before any launch): 1 <= Ld <= 512; 1 <= K <= 65535; N >= 1; B >= 1; 1 <= Lq <= 512;
 * 1 <= nprobe <= 1024; 0 <= P < 2^31; cap >= 1 with cand; ldp >= nprobe; ldb >= ceil(N/32); ldc >= cap; non-null
 * pointers (qmask and cand may be NULL; docs may be NULL when P = 0). */
int polus_ivf_count(const uint16_t* codes, int N, int Ld, int K, int32_t* counts, void* stream);
int polus_ivf_offsets(const int32_t* counts, int K, int32_t* offsets, void* stream);
int polus_ivf_fill(const uint16_t* codes, int N, int Ld, int K, const int32_t* offsets, int P, int32_t* cursor,
                   int32_t* docs, void* stream);
int polus_ivf_mark(const int32_t* probes, long ldp, const int32_t* qmask, const int32_t* offsets, const int32_t* docs,
                   int P, int K, int N, uint32_t* bitmap, long ldb, int B, int Lq, int nprobe, void* stream);
int polus_ivf_compact(const uint32_t* bitmap, long ldb, int B, int N, int32_t* cand, long ldc, int cap, int32_t* count,
                      void* stream);

/* ---- learned sparse retrieval, SPLADE (splade.hip; no counterpart in the reference, whose first stages are dense).
 * A text becomes one non-negative vector over the vocabulary, rep[v] = max over its valid tokens s of
 * log(1 + relu(logit[s, v])), from the masked-LM logits of all its tokens.  log1p is monotone: the maximum is taken
 * over the stored values and log1pf is applied once.
 *
 * polus_splade_pool_fwd:
 *   logits [B*S, V] in `dtype` (f32 or bf16), row stride ldl;  mask int32 [B, S] contiguous, NULL = every token valid
 *   rep, xmax f32 [B, V] (row strides ldr, ldx);  arg int32 [B, V] (row stride lda)
 *   per (b, v):  m = the maximum of logits[b*S + s, v] over the s with mask[b, s] != 0, arg = the lowest s attaining m;
 *                no valid token or m <= 0:  rep = 0, xmax = 0, arg = -1;   otherwise rep = log1pf(m), xmax = m.
 *   Comparisons are `>`: a NaN never wins (a column of NaN gives (0, 0, -1)).  One read of the valid rows of logits, a
 *   masked row is not read at all; columns past V of the outputs are not written.
 * polus_splade_pool_bwd:
 *   dlogits[b*S + s, v] = (s == arg[b, v]) ? T(drep[b, v] / (1 + xmax[b, v])) : 0 for EVERY s < S, masked rows included:
 *   IEEE f32 addition and division, rounded once to `dtype`.  Columns past V of a row are not touched.  Nothing of the
 *   logits is read, so dlogits may be the logits buffer of the forward pass.  Write-only traffic but for the three
 *   [B, V] inputs.
 * Both: a lane owns one 16-byte chunk of columns of one sequence and walks its S rows; grid (chunks / 256, B).  16-byte
 * accesses of logits / dlogits where the pointer and ldl * sizeof(T) are multiples of 16, single elements otherwise and
 * for the columns behind the last whole chunk; 16-byte accesses of the [B, V] arrays where all three are 16-byte
 * aligned with strides that are multiples of 4.  The results are the same bits on every access route.  No atomics, no
 * workspace, no scratch, bitwise reproducible.
 * Limits (refused before any launch): dtype f32 or bf16; 1 <= B <= 65535; S >= 1; V >= 1; every row stride >= V;
 * non-null pointers (mask aside), each aligned to its element.
 *
 * polus_flops_reg, the FLOPS sparsity regulariser of SPLADE over the rows [0, rows) of rep (f32, row stride ldr):
 *   colmean[v] = (sum over b of rep[b, v]) / rows;   value = lambda * sum over v of colmean[v]^2
 *   loss[0] = value, or loss[0] += value with loss_accumulate != 0 (device f32; this is how a trainer adds the
 *   regulariser to its loss without a host round trip);
 *   drep != NULL:  drep[b, v] += (lambda * (2 / rows)) * colmean[v]  for b < rows, v < V  (f32, row stride lddr).
 * Queries and documents take one call each, on their own rows and with their own lambda.  Order: a column is summed in
 * ascending b by one lane; lane l of workgroup k (one wave) holds columns 256 k + 4 l .. + 3 and adds their four
 * squares in ascending v, a wave's 64 sums go through one xor-shuffle tree into workspace[k], and a second launch adds
 * the ceil(V / 256) partials in index order.  The order does not depend on alignment (which only selects 16-byte or
 * 4-byte accesses).  No atomics, bitwise reproducible.
 * Limits (refused before any launch): rows >= 1; V >= 1; ldr >= V; lddr >= V with drep; rep, loss non-null;
 * drep != rep; workspace >= polus_flops_reg_workspace_bytes(V) (host only).
 *
 * polus_sparse_scores, sparse documents against dense queries (the search of a SPLADE index):
 *   q f32 [B, V] (row stride ldq): the queries' representations, dense;
 *   ids int32 and w f32 [N, M] (row strides ldi, ldw): the M (term, weight) pairs kept per document;
 *   score[b*lds + n] = sum over m with 0 <= ids[n, m] < V of  w[n, m] * q[b, ids[n, m]]
 * An id outside [0, V), -1 included, is skipped: its weight is read, nothing of q is dereferenced for it.  A term
 * that occurs twice counts twice.  One workgroup (16 waves) per (query, contiguous range of documents, sized so that
 * a launch has about four workgroups per CU and a range at least 8 documents per wave) copies the query row into
 * dynamic LDS, V * 4 bytes rounded up to 16, which is all the LDS the kernel uses: V * 4 <= 163840 (160 KiB, one CU's
 * LDS), i.e. V <= 40960; V = 30522 takes 122088 bytes.  A wider vocabulary is refused: there is no global-memory
 * route.  A wave owns a document (and works on eight of its documents at a time, to have their loads in flight
 * together; a document's arithmetic does not depend on the others).  Summation order: lane l runs p = fmaf(w[n, m], q[b, ids[n, m]], p) from p = 0 over
 * m = l, l + 64, l + 128, ... in ascending m (skipped terms leave p as it is), then the 64 lane sums are added by the
 * xor-shuffle tree with offsets 32, 16, 8, 4, 2, 1.  The bits of an entry therefore depend on the query row, the
 * document's row and M alone: not on B, N, the range of documents of the launch, the grid or the device.  Columns of
 * score past N are not written.  No atomics, no workspace, bitwise reproducible.
 * Limits (refused before any launch): 1 <= M <= 1024 (what polus_topk_merge can keep); B >= 1; N >= 1 (documents are
 * addressed with 64 bits); V >= 1 and V * 4 <= 163840; ldq >= V; ldi, ldw >= M; lds >= N; B * ceil(N / range) < 2^31;
 * non-null pointers. */
int polus_splade_pool_fwd(int dtype, const void* logits, long ldl, const int32_t* mask, float* rep, long ldr,
                          float* xmax, long ldx, int32_t* arg, long lda, int B, int S, int V, void* stream);
int polus_splade_pool_bwd(int dtype, const float* drep, long lddr, const float* xmax, long ldx, const int32_t* arg,
                          long lda, void* dlogits, long lddl, int B, int S, int V, void* stream);
size_t polus_flops_reg_workspace_bytes(int V);
int polus_flops_reg(const float* rep, long ldr, int rows, int V, float lambda, float* loss, int loss_accumulate,
                    float* drep, long lddr, void* workspace, size_t workspace_bytes, void* stream);
int polus_sparse_scores(const float* q, long ldq, const int32_t* ids, long ldi, const float* w, long ldw,
                        float* score, long lds, int B, int N, int M, int V, void* stream);

/* ---- lexical retrieval, BM25 over token ids (bm25.hip; no counterpart in the reference, which has no lexical stage).
 * A document is the bag of its token ids; the index keeps per document M (term, count) pairs, the document length and
 * the corpus statistics, and derives f32 weights from them, so that polus_sparse_scores over (q, terms, w) is the BM25
 * score.  Integers only in polus_bm25_term_counts: every result is exact.
 *
 * polus_bm25_term_counts:
 *   ids int32 [n, L] (row stride ldi);  mask int32 [n, L] (row stride ldm) or NULL = every token valid
 *   terms, tf int32 [n, M] (row strides ldt, ldf);  doc_len int32 [n]
 *   df int32 [V] or NULL, ACCUMULATED;  stats int64 [3] or NULL, ACCUMULATED (zero both to start)
 *   Valid tokens.  The valid tokens of a row are those whose mask is non-zero, in order.
 *   Stripping.  A row with at most head + tail valid tokens is empty; otherwise its first `head` and last `tail` valid
 *     tokens are dropped (polus_pair_pack's rule: 1/1 takes the [CLS] and [SEP] off HF-tokenised rows).
 *   Rejection.  A remaining token whose id lies outside [0, V) is dropped and adds 1 to stats[1].
 *   doc_len[r] = the number of tokens that remain; it is also added to stats[2].
 *   Terms.  Let u be the number of distinct remaining ids, ordered by (count descending, id ascending).  Slot s <
 *     min(u, M) holds the s-th of them: terms[r, s] = the id, tf[r, s] = its count.  Every further slot s < M is written
 *     as (-1, 0).  u > M adds 1 to stats[0] (a truncated document).  Nothing beyond column M - 1 is written.
 *   df[t] += 1 for every distinct remaining id t of the row, kept in a slot or not (int32 atomics); with df == NULL
 *     (queries) that step is skipped.
 *   One workgroup per document (grid-stride): ids into LDS as 64-bit keys, bitonic sort, run heads by neighbour
 *   compares, run lengths by a binary search, a second sort of (count, id) keys; 16 KiB of LDS for every V.  stats
 *   receives three int64 atomic adds per workgroup.  Sums of integers are exact in any order: bitwise reproducible.  No
 *   float atomics, no workspace.
 *   Limits (refused before any launch): 1 <= L <= 2048; 1 <= M <= 1024; n >= 1; V >= 1; 0 <= head, tail <= 8; ldi >= L;
 *     ldm >= L with a mask; ldt, ldf >= M; ids, terms, tf, doc_len non-null.
 *
 * polus_bm25_weights:  w f32 [n, M] (row stride ldw) from tf int32 [n, M] (row stride ldf), doc_len int32 [n] and three
 *   f32 constants (BM25Index.refresh: c0 = k1 (1 - b), c1 = k1 b / avgdl, k1p1 = k1 + 1):
 *     K_r     = fl(fl(c1 * f32(doc_len[r])) + c0)
 *     w[r, m] = tf[r, m] > 0 ? fl(fl(f32(tf[r, m]) * k1p1) / fl(f32(tf[r, m]) + K_r)) : +0.0f
 *   Every fl is one IEEE f32 rounding to nearest even, the division is correctly rounded and nothing is contracted into
 *   an fma: NumPy float32 arithmetic gives the same bits.  Nothing beyond column M - 1 is written.  One wave per row.
 *   Limits (refused before any launch): n >= 1; 1 <= M <= 1024; ldf, ldw >= M; non-null pointers.
 *
 * polus_bm25_query:  the dense query rows polus_sparse_scores reads.  q f32 [B, V] (row stride ldq), EVERY element of
 *   the V columns written; terms, tf int32 [B, M] (row strides ldt, ldf) as polus_bm25_term_counts leaves them; idf f32 [V]:
 *     q[b, terms[b, m]] = fl(f32(tf[b, m]) * idf[terms[b, m]])  for the slots with 0 <= terms[b, m] < V;  0.0 elsewhere.
 *   The terms of a row must be distinct (plain stores; of a repeated term one slot's value remains).  One workgroup per
 *   row: fill, barrier, scatter.
 *   Limits (refused before any launch): B >= 1; 1 <= M <= 1024; V >= 1 and V * 4 <= 163840 (polus_sparse_scores' limit
 *     on the row); ldt, ldf >= M; ldq >= V; non-null pointers. */
int polus_bm25_term_counts(const int32_t* ids, long ldi, const int32_t* mask, long ldm, int n, int L, int V, int head,
                           int tail, int32_t* terms, long ldt, int32_t* tf, long ldf, int M, int32_t* doc_len,
                           int32_t* df, int64_t* stats, void* stream);
int polus_bm25_weights(const int32_t* tf, long ldf, const int32_t* doc_len, float* w, long ldw, int n, int M, float c0,
                       float c1, float k1p1, void* stream);
int polus_bm25_query(const int32_t* terms, long ldt, const int32_t* tf, long ldf, const float* idf, float* q, long ldq,
                     int B, int M, int V, void* stream);

/* ---- block-inverted postings and term-at-a-time search (postings.hip; no counterpart in the reference).  The inverted
 * route of the two lexical first stages, beside the forward route above: polus_sparse_scores reads every slot of
 * every document for every query, Q * N * M * 8 bytes; a search over postings reads only the lists of the query's
 * terms.  It also has no limit on V beyond int32, since no dense query row has to fit in LDS.
 *
 * Blocks.  The N documents are cut into blocks of block_docs consecutive ids; block_docs is a power of two in
 * [64, 32768], the last block may be partial, nblk = ceil(N / block_docs).
 * Postings.  A posting is a triple (term t, document d, weight w) taken from a forward slot (ids[d, m], w[d, m]) of
 * ids int32 / w f32 [N, M] (row strides ldi, ldw).  A slot is a posting iff 0 <= id < V and w != 0: a NaN weight counts,
 * +0.0 and -0.0 do not (SPLADE's zero-weight filler slots would otherwise give the lowest term ids a list of N
 * entries each).  PRECONDITION: the ids in one document's slots are distinct (polus_bm25_term_counts and
 * polus_topk_merge guarantee it); with duplicates the result is unspecified, but nothing faults.
 * Storage, per block in CSR form over the terms:
 *   offsets  int32 [nblk, V + 1] contiguous;  offsets[b, 0] = 0;  offsets[b, V] = the block's posting count,
 *            <= block_docs * M <= 2^25.
 *   base     int64 [nblk + 1]: the exclusive scan of the block totals;  base[nblk] = P.  P may exceed 2^31, so every
 *            posting index is 64-bit.
 *   post_doc uint16 [P]: the document id local to its block, d - b * block_docs.
 *   post_w   f32 [P]: the weight.
 *   The list of (b, t) is the positions base[b] + offsets[b, t] .. base[b] + offsets[b, t + 1].  THE ORDER INSIDE A LIST
 *   IS UNSPECIFIED (a posting takes the slot an atomic cursor hands it); the lists as SETS, the counts, the offsets and
 *   the base are exact and reproducible.  Nothing downstream depends on the order (the score rule below).
 * Query lists.  q_terms int32 [Q, cap], q_w f32 [Q, cap] (row strides ldt, ldw), q_count int32 [Q]: row q's entries
 *   0 .. min(q_count[q], cap) are in ascending term id, the rest of the row is (-1, 0.0).
 * THE SCORE RULE.  For query q and document d:  acc = +0.0f;  the entries j = 0 .. min(q_count[q], cap) - 1 are taken in
 *   that order;  an entry with q_terms[q, j] outside [0, V) is skipped;  if d's block holds a posting (t, d, w) for
 *   t = q_terms[q, j], then  acc = fl(acc + fl(q_w[q, j] * w)):  one rounding for the product and one for the sum, no
 *   fma.  NumPy float32 arithmetic reproduces these bits.  A document with no matching term scores +0.0 (and is still
 *   ranked, as on the forward route).  An entry whose term repeats an earlier one counts again.
 *
 * The caller owns every buffer; nothing is allocated here; limits are refused on the host before any launch; integer
 * atomics are int32 vector atomics; there are NO floating-point atomics: the score rule fixes the order of the sums.
 *
 * polus_postings_count:   counts int32 [nblk, V] contiguous, zeroed by the call itself;  counts[b, t] = the postings of
 *   term t in block b.  One thread per forward slot, one int32 add per posting.
 * polus_postings_offsets: offsets[b, :] = the exclusive scan of counts[b, :] (one workgroup per block, 64-bit sums,
 *   a negative count reads as 0), then base = the int64 exclusive scan of the block totals (one workgroup): two launches.
 * polus_postings_fill:    cursor int32 [nblk, V] is scratch, zeroed by the call itself, meaningless afterwards (it may be
 *   the counts buffer, which is no longer needed).  The same walk as count;  a posting takes slot = cursor[b, t]++ and
 *   is stored at base[b] + offsets[b, t] + slot only if offsets[b, t] + slot < offsets[b, t + 1] and the position lies in
 *   [0, P): foreign or stale offsets lose entries, they never write out of range.  P = 0 is legal (nothing is stored;
 *   post_doc and post_w may be NULL).
 * polus_sparse_compact_rows:  a dense row q[r, 0 .. V) (f32, row stride ldq) becomes a query list: entry v is kept iff
 *   q[r, v] != 0 (NaN kept, +-0.0 dropped), in ascending v, with weight q[r, v].  q_count[r] = the FULL number of kept
 *   entries even when it exceeds cap; entries past cap are dropped; the rest of the row up to cap is (-1, 0.0); nothing
 *   past column cap - 1 is written.  One workgroup per row, __ballot and popcount prefix, no atomics.  No limit on V
 *   beyond int32; rows need no alignment beyond 4 bytes.
 * polus_bm25_query_lists:  terms, tf int32 [Q, M] (row strides ldt, ldf) as polus_bm25_term_counts leaves a query (distinct
 *   ids ordered by count, -1 in unused slots);  the query list q_terms / q_w [Q, M] (row strides ldt2, ldw; cap = M) in
 *   ascending id with weight fl(f32(tf) * idf[t]), polus_bm25_query's arithmetic;  ids outside [0, V) are dropped;
 *   q_count[r] = the kept entries.  One workgroup per row; an entry's place is the number of kept entries with a
 *   smaller id (of equal ids, the lower slot first), counted through LDS.  No dense [Q, V] row is made, so
 *   polus_bm25_query's limit on V is not involved.
 * polus_postings_scores:  one workgroup per (query, block) for the blocks blk0 .. blk0 + nblk_launch.  An f32
 *   accumulator of block_docs entries sits in dynamic LDS (at most 128 KiB of a CU's 160) and is zeroed first; the
 *   query's entries are walked in order; for each one the threads stride over the list of (block, term) and do a plain
 *   load-add-store on acc[post_doc] (the documents of one list are distinct: no two threads share an address); a
 *   barrier separates the terms (an empty list, which is uniform over the workgroup, skips it).  At the end acc goes
 *   out coalesced:  score[q * lds + (b - blk0) * block_docs + local]  for the documents b * block_docs + local < N only.
 *   Bounds: a list is clamped to positions [0, P) before it is read; a local id >= the documents of its block is not
 *   accumulated; so stale or foreign postings cannot fault or write outside the row.
 * Limits (refused before any launch): N >= 1; 1 <= M <= 1024; 1 <= V < 2^31 - 1; block_docs a power of two in
 * [64, 32768]; nblk >= 1; P >= 0; Q >= 1; cap >= 1; 0 <= blk0, nblk_launch >= 1, blk0 + nblk_launch <= nblk;
 * Q * nblk_launch < 2^31; ldi, ldw >= M; ldq >= V; list row strides >= cap (>= M for polus_bm25_query_lists);
 * lds >= the documents of the launch; non-null pointers (post_doc and post_w may be NULL when P = 0). */
int polus_postings_count(const int32_t* ids, long ldi, const float* w, long ldw, int N, int M, int V, int block_docs,
                         int32_t* counts, void* stream);
int polus_postings_offsets(const int32_t* counts, int nblk, int V, int32_t* offsets, int64_t* base, void* stream);
int polus_postings_fill(const int32_t* ids, long ldi, const float* w, long ldw, int N, int M, int V, int block_docs,
                        const int32_t* offsets, const int64_t* base, long P, int32_t* cursor, uint16_t* post_doc,
                        float* post_w, void* stream);
int polus_sparse_compact_rows(const float* q, long ldq, int Q, int V, int cap, int32_t* q_terms, long ldt, float* q_w,
                              long ldw, int32_t* q_count, void* stream);
int polus_bm25_query_lists(const int32_t* terms, long ldt, const int32_t* tf, long ldf, const float* idf, int Q, int M,
                           int V, int32_t* q_terms, long ldt2, float* q_w, long ldw, int32_t* q_count, void* stream);
int polus_postings_scores(const int32_t* q_terms, long ldt, const float* q_w, long ldw, const int32_t* q_count, int cap,
                          const int32_t* offsets, const int64_t* base, const uint16_t* post_doc, const float* post_w,
                          long P, int V, int block_docs, int blk0, int nblk_launch, int N, float* score, long lds, int Q,
                          void* stream);

/* ---- hard-negative mining (mine.hip): k negatives per query sampled from a ranked candidate list, the step between a
 * first-stage search and the (question, positive, negatives) tuples of the trainers.  Integers only: exact.
 *   cand int32 [Q, C] (row stride ldc), in rank order, ids distinct within a row (as a search returns them)
 *   score f32 [Q, C] (row stride lds) or NULL;  exclude int32 [Q, P] (row stride lde), NULL allowed when P == 0
 *   neg int32 [Q, k] contiguous;  neg_col int32 [Q, k] contiguous or NULL;  n_pool int32 [Q]
 * Pool.  The pool of row r is the columns c >= skip_top, in column order, with cand[r, c] >= 0, cand[r, c] not equal to
 *   any non-negative entry of exclude[r, :], and, when score is given, score[r, c] > min_score (a NaN fails;
 *   min_score = 0 removes the documents that share no term with a BM25 query).  R = the pool's size; n_pool[r] = R.
 * R <= k.  neg[r, j] = the id of pool position j for j < R and -1 for R <= j < k.
 * R > k.   With lo_j = floor(j R / k) and hi_j = floor((j + 1) R / k) in 64-bit integers, neg[r, j] = the id at pool
 *   position lo_j + polus_hash32(seed, r k + j) mod (hi_j - lo_j), where polus_hash32(seed, idx) is the murmur3
 *   finaliser of idx * 0x9E3779B1 + seed (uint32 arithmetic; the dropout mask's hash) and r k + j is taken mod 2^32.
 *   One draw per rank stratum: the negatives come out in rank order, are distinct and span the whole depth.
 * neg_col[r, j] = the column neg[r, j] came from, -1 where neg is -1.
 * One wave per query, two sweeps over the columns in 64-column steps (count, then place by __ballot and popcount);
 * plain stores to distinct addresses, no LDS, no atomics, no workspace, bitwise reproducible.
 * Limits (refused before any launch): Q, C >= 1; 1 <= k <= 1024; 0 <= P <= 1024; skip_top >= 0; Q k < 2^32; ldc >= C;
 *   lds >= C with scores; lde >= P and exclude non-null when P > 0; cand, neg, n_pool non-null. */
int polus_mine_negatives(const int32_t* cand, long ldc, const float* score, long lds, const int32_t* exclude, long lde,
                         int Q, int C, int P, int skip_top, float min_score, int k, uint32_t seed, int32_t* neg,
                         int32_t* neg_col, int32_t* n_pool, void* stream);

/* ---- rank fusion (fuse.hip; no counterpart in the reference): L ranked lists per query, as L searches return them,
 * joined by document id and fused by reciprocal rank (RRF), CombSUM, or CombSUM over min-max normalised scores.
 *   ids int32 [L, Q, C] (list stride lsi, row stride ldi);  scores f32 [L, Q, C] (lss, lds) or NULL (rrf only)
 *   weights: a HOST array f32 [L], read during the call, or NULL = all 1.0f;  rrf_k: the constant of RRF (60 in the paper)
 *   out_id int32 and out_val f32 [Q, L*C] (row strides ldoi, ldov);  count int32 [Q]
 * Kept.  Entry (l, r, c) is kept iff 0 <= ids[l, r, c] < n_docs and, when scores is given, scores[l, r, c] is finite
 *   (NaN and +-inf are dropped; -inf is how polus_maxsim_rerank marks a missing candidate).  Every other entry is skipped
 *   and nothing is indexed by it.
 * Rank.  rank(l, r, c) = 1 + the number of kept entries of list row (l, r) at columns below c.  A dropped entry takes no
 *   rank.  A list is taken in the order given and never re-sorted.
 * Contribution of a kept entry with score s and weight w = weights[l], in f32, every fl one IEEE rounding to nearest
 *   even, the division correctly rounded, nothing contracted into an fma (as polus_bm25_weights: NumPy float32 arithmetic
 *   gives the same bits):
 *     mode POLUS_FUSE_RRF     fl(w / fl(rrf_k + f32(rank)))
 *     mode POLUS_FUSE_SUM     fl(w * s)
 *     mode POLUS_FUSE_MINMAX  fl(w * fl(fl(s - lo) / fl(hi - lo))),  lo and hi the minimum and maximum, by IEEE
 *                             comparison, of the kept scores of list row (l, r);  hi == lo (a list row with one kept
 *                             entry among them):  fl(w * 1.0f) for each of its kept entries.
 *   Precondition of MINMAX: hi - lo is finite.  -0.0 equals +0.0 under IEEE comparison: where the minimum of a list row
 *   is a zero present with both signs, which of the two is lo, and with it the sign of a zero contribution, is
 *   unspecified.  A document absent from a list gets nothing from it (so the worst document present also gets 0: the
 *   usual reading of CombSUM over min-max scores).
 * Fused score of a document = its contributions added left to right in (list, column) order, the first taken as it is:
 *   fl(fl(c_1 + c_2) + c_3) ...  A repeated id inside one list row is not detected: every copy takes its own rank and
 *   contributes, in column order (searches return no such rows; the rule keeps the result defined).
 * Output.  count[r] = the number of distinct kept ids of row r;  out_id[r, 0 .. count[r]) = those ids ASCENDING and
 *   out_val[r, 0 .. count[r]) their fused scores;  columns count[r] .. L*C - 1 are (-1, -inf).  Nothing beyond column
 *   L*C - 1 is written.  This is the candidate row polus_ivf_compact hands out and what polus_topk_merge_ids and
 *   polus_maxsim_rerank accept (a negative id is a missing candidate there).  Ids and counts are exact, the values are
 *   the bits of the rule above whatever Q, the grid or the device.
 * One workgroup per query (grid-stride): every list row read once in 64-column steps (kept flags by __ballot, ranks by
 * popcount prefix, lo / hi by wave reduction), contributions and 64-bit keys id << 13 | (l C + c) in 48 KiB of LDS, one
 * bitonic sort of the keys, run heads found by neighbour compares add their run in order and are compacted by ballot
 * and popcount.  No atomics, no workspace, bitwise reproducible.
 * Limits (refused before any launch): 1 <= L <= 8; Q >= 1; C >= 1; L*C <= 4096; 1 <= n_docs <= 2^31 - 1; ldi, lds >= C;
 *   with L > 1, lsi >= (Q - 1) ldi + C and lss >= (Q - 1) lds + C (the extent of one list); ldoi, ldov >= L*C; scores
 *   non-null for SUM and MINMAX; rrf_k finite and >= 0 for RRF; weights finite; mode one of the three; ids, out_id,
 *   out_val, count non-null. */
#define POLUS_FUSE_RRF 0
#define POLUS_FUSE_SUM 1
#define POLUS_FUSE_MINMAX 2
int polus_fuse_lists(const int32_t* ids, long lsi, long ldi, const float* scores, long lss, long lds, int L, int Q, int C,
                     int n_docs, int mode, const float* weights, float rrf_k, int32_t* out_id, long ldoi, float* out_val,
                     long ldov, int32_t* count, void* stream);

/* ---- product quantisation of single ([CLS]) vectors and its asymmetric-distance scan (pq.hip; Jegou, Douze, Schmid:
 * "Product quantization for nearest neighbor search", 2011; no counterpart in the reference).
 *
 * Format.  A vector of E = m * dsub elements is cut into m consecutive sub-vectors of dsub elements.  The codebook is
 * f32 [m, ksub, dsub], contiguous: codebook[(j*ksub + c)*dsub + t] is element t of codeword c of sub-space j.  A stored
 * vector is m bytes uint8, byte j naming a codeword of sub-space j.  A byte >= ksub (a foreign or stale code) is never
 * out of bounds anywhere: see each function.
 * Arithmetic.  Every f32 operation below is one IEEE rounding, never an fma, in the order stated, so NumPy float32
 * reproduces every bit (tests/pq_ref.py).  bf16 inputs are widened to f32 first (exact).
 * Limits of every function (refused before any launch, with a message): m a multiple of 4 in [4, 160]; 1 <= ksub <= 256;
 * 1 <= dsub <= 32; row counts >= 1 (Q and N of the scan also <= 65535); every leading dimension at least the row
 * width; dtype f32 or bf16; non-null pointers.
 *
 * polus_pq_encode:  x [rows, E] in `dtype`, row stride ldx >= E;  codes uint8 [rows, m], row stride ldc >= m
 *   dist(c)     = sum over t = 0 .. dsub-1, ascending, from +0.0, of  fl(fl(x_t - cb_t) * fl(x_t - cb_t))
 *   codes[r, j] = the lowest c < ksub that minimises dist by IEEE comparison, a NaN distance counting as +inf: a NaN
 *                 never wins over a number, and a sub-vector whose distances are all NaN (or +inf) gets code 0.
 *   The result depends on that sub-vector and the codebook only.  One thread per (row, sub-space), the sub-space's
 *   codewords in LDS.
 * polus_pq_update, one Lloyd update:  x [T, E] in `dtype`, row stride ldx;  codes uint8 [T, m], row stride ldc;  prev, out
 *   f32 [m, ksub, dsub] (out must not alias prev);  counts int32 [m, ksub]
 *   counts[j, c] = the number of rows t with codes[t, j] == c (codes >= ksub belong to no codeword and are skipped)
 *   out[j, c, :] = fl(sum / f32(counts[j, c])), one division per element, where counts[j, c] > 0;  prev[j, c, :] otherwise
 *   The sum is f32 in an order that is a function of T alone: with P = ceil(T / 64), partial l = 0 .. 63 adds, from +0.0,
 *   the sub-vectors of the rows t in [l*P, min((l+1)*P, T)) whose code is c, in ascending t; then six rounds
 *   p_l = fl(p_l + p_(l xor o)) for o = 32, 16, 8, 4, 2, 1 (every l at once) leave the sum in every p_l.  One wave per
 *   (j, c), lane l holding partial l.  No atomics, no workspace, bitwise reproducible.  Index-build time work: m * ksub
 *   reads of a code column.
 * polus_pq_decode:  y [rows, E] in `dtype`, row stride ldy >= E
 *   y[r, j*dsub + t] = codebook[j, codes[r, j], t] rounded once to `dtype`;  a code >= ksub decodes to zeros.
 * polus_pq_lut, the table of one search:  q [Q, E] in `dtype`, row stride ldq >= E;  lut f32 [Q, m, ksub], contiguous
 *   lut[b, j, c] = sum over t = 0 .. dsub-1, ascending, from +0.0, of  fl(q[b, j*dsub + t] * codebook[j, c, t])
 * polus_pq_scores, the scan:  lut as above;  codes uint8 [N, m], row stride ldc;  score f32 [Q, N], row stride lds >= N
 *   score[b, n] = sum over j = 0 .. m-1, ascending, from +0.0, of  lut[b, j, codes[n, j]]
 *   A byte >= ksub reads -inf, so its document scores -inf (or NaN beside a +inf or NaN entry), which polus_topk_merge
 *   drops.  The table may hold NaN and +-inf; they propagate by IEEE rules.  Columns past N and rows past Q of score are
 *   not written.  The bits of a pair depend on that query's table and that document's codes only: not on Q, N, the
 *   chunking of a corpus or how many queries a workgroup serves.  No atomics, no workspace.
 *   One workgroup (1024 threads) serves qt consecutive queries and a contiguous range of documents.  It copies the qt
 *   tables into dynamic LDS interleaved as [m][256][qt] floats, every sub-space padded to 256 entries with -inf:
 *   qt * m * 1024 bytes.  A thread owns a document from its first look-up to the store: it reads the m code bytes in
 *   16-byte pieces (codes, ldc and m multiples of 16), else in 4-byte pieces (multiples of 4), else byte by byte, and
 *   one LDS read of 4 * qt bytes per code fetches the entry of all qt queries.  qt is the largest of 4, 2, 1 that is
 *   <= Q and keeps qt * m * 1024 <= 163840 (one CU's LDS: m = 160 at qt = 1 fills it, whence the limit on m); the last
 *   group of a Q that is no multiple of qt repeats query Q - 1 in its spare slots and stores nothing for them.
 * polus_pq_scores_route (host only, no HIP call) applies the limits and reports out[0] = qt, out[1] = the dynamic LDS
 * bytes. */
#define POLUS_PQ_ROUTE_INTS 2
int polus_pq_encode(int dtype, const void* x, long ldx, const float* codebook, uint8_t* codes, long ldc, int rows, int m,
                    int ksub, int dsub, void* stream);
int polus_pq_update(int dtype, const void* x, long ldx, const uint8_t* codes, long ldc, const float* prev, float* out,
                    int32_t* counts, int T, int m, int ksub, int dsub, void* stream);
int polus_pq_decode(const uint8_t* codes, long ldc, const float* codebook, int dtype, void* y, long ldy, int rows, int m,
                    int ksub, int dsub, void* stream);
int polus_pq_lut(int dtype, const void* q, long ldq, const float* codebook, float* lut, int Q, int m, int ksub, int dsub,
                 void* stream);
int polus_pq_scores(const float* lut, const uint8_t* codes, long ldc, float* score, long lds, int Q, int N, int m, int ksub,
                    void* stream);
int polus_pq_scores_route(int Q, int N, int m, int ksub, int* out);

/* ---- IVF-PQ of single ([CLS]) vectors (ivfpq.hip; Jegou, Douze, Schmid 2011, "IVFADC", the layout of FAISS' IVFPQ, here
 * for inner products; no counterpart in the reference).  A coarse quantiser of K centroids splits the corpus into K
 * lists; a document is stored as the id of its centroid and the product-quantisation codes of its RESIDUAL against that
 * centroid, and a query scores only the documents of the lists it probes.
 *
 * Format.  Per document one unsigned 16-bit coarse code coarse[n], the id of its centroid; a value >= K (0xFFFF among
 * them) is "no list".  Beside it m bytes uint8 of PQ codes, the format and limits of the section above (m a multiple of 4
 * in [4, 160]; 1 <= ksub <= 256; 1 <= dsub <= 32; E = m * dsub), naming the codewords of the residual's sub-vectors.  The
 * coarse centroids are [K, E], contiguous, in the index's dtype (f32 or bf16); 1 <= K <= 65535.
 * Arithmetic.  As above: every f32 operation is one IEEE rounding, never an fma, in the order stated, so NumPy float32
 * reproduces every bit (tests/ivfpq_ref.py); bf16 inputs are widened to f32 first (exact).
 *
 * polus_ivfpq_residual:  x [rows, E] in `dtype`, row stride ldx >= E;  cent [K, E] in `dtype`;  coarse uint16 [rows];
 *   r f32 [rows, E], row stride ldr >= E
 *   r[t, e] = fl(f32(x[t, e]) - f32(cent[coarse[t], e])), one rounding;  a row whose coarse code is >= K gives zeros and
 *   reads no centroid.  The centroid is the one STORED in the index's dtype, so that <q, cent> from polus_gemm over the
 *   same array and the stored residual refer to the same vector.  One thread per output.  1 <= E <= 5120.
 * polus_ivfpq_coarse_update, one Lloyd step on whole vectors:  x [T, E] in `dtype`, row stride ldx;  coarse uint16 [T];
 *   prev, out [K, E] in `dtype`, contiguous (out must not overlap prev);  counts int32 [K]
 *   counts[k] = the number of rows t with coarse[t] == k (codes >= K belong to no centroid and are skipped)
 *   out[k, :] = fl(sum / f32(counts[k])), one division per element, rounded once to `dtype`, where counts[k] > 0;
 *               prev[k, :] otherwise
 *   The sum follows polus_pq_update's order rule, a function of T alone: with P = ceil(T / 64), partial l = 0 .. 63 adds,
 *   from +0.0, the rows t in [l*P, min((l+1)*P, T)) whose code is k, in ascending t; then six rounds
 *   p_l = fl(p_l + p_(l xor o)) for o = 32, 16, 8, 4, 2, 1.  One workgroup of 4 waves per centroid, lane l holding partial
 *   l for 16 features at a time.  No atomics, no workspace, bitwise reproducible.  Index-build time work: every
 *   wave reads the code array once per 64 features, E / 16 reads per centroid.  1 <= E <= 5120.
 * polus_ivfpq_scores_ids, the scan over candidate lists:  lut f32 [Q, m, ksub], contiguous (polus_pq_lut of the queries
 *   with the RESIDUAL codebook);  cdot f32 [Q, K], row stride ldd >= K, cdot[b, c] = <q_b, cent_c>, an input (one
 *   polus_gemm);  coarse uint16 [N];  codes uint8 [N, m], row stride ldc;  cand int32 [Q, C], row stride ldcand >= C, or
 *   NULL;  score f32 [Q, C], row stride lds >= C
 *   n           = cand[b, c], or c where cand == NULL (then C must equal N: the exhaustive route, for which the caller
 *                 offsets coarse and codes per chunk of a corpus)
 *   acc         = sum over j = 0 .. m-1, ascending, from +0.0, of  lut[b, j, codes[n, j]]     (polus_pq_scores' rule)
 *   score[b, c] = fl(cdot[b, coarse[n]] + acc), one more rounding
 *   coarse[n] >= K: score = -inf and nothing is read from cdot for it.  A code byte >= ksub reads -inf through the
 *   table's padding, as in polus_pq_scores.  n outside [0, N): score = -inf and nothing is read for it (-inf is what
 *   polus_topk_merge_ids drops).  A repeated id is scored once per copy.  Columns past C are not written.  lut and cdot
 *   may hold NaN and +-inf; they propagate by IEEE rules.  The bits of a score depend on its (query, document) pair
 *   only: not on Q, C, the order of the candidates, the chunking or the route.  No atomics, no workspace.
 *   One workgroup (1024 threads) serves one query and a contiguous range of its candidate columns.  It copies that
 *   query's table into dynamic LDS as [m][256] floats, every sub-space padded to 256 entries with -inf: m * 1024 bytes,
 *   polus_pq_scores' layout at qt = 1 (candidate lists differ per query, so no code byte serves two queries).  A thread
 *   owns a candidate from its first look-up to the store; it reads the code row at codes + n * ldc in 16-byte pieces
 *   (codes, ldc and m multiples of 16), else in 4-byte pieces (multiples of 4), else byte by byte.  Each query's columns
 *   are spread over the CUs (two workgroups per CU where two tables fit its LDS), at least 256 columns a workgroup.
 *   Limits (refused before any launch): the PQ limits; 1 <= Q, C <= 65535; N >= 1; 1 <= K <= 65535; ldd >= K; ldc >= m;
 *   ldcand >= C; lds >= C; C == N without cand; non-null pointers except cand.
 * polus_ivfpq_scores_ids_route (launches nothing) applies the scan's shape limits and reports out[0] = the dynamic LDS
 * bytes and out[1] = the columns per workgroup, which follow the CU count of the current device (256 without one). */
#define POLUS_IVFPQ_ROUTE_INTS 2
int polus_ivfpq_scores_ids(const float* lut, const float* cdot, long ldd, const uint16_t* coarse, const uint8_t* codes,
                           long ldc, const int32_t* cand, long ldcand, float* score, long lds, int Q, int C, int N, int m,
                           int ksub, int K, void* stream);
int polus_ivfpq_scores_ids_route(int Q, int C, int m, int ksub, int* out);
int polus_ivfpq_residual(int dtype, const void* x, long ldx, const void* cent, const uint16_t* coarse, float* r, long ldr,
                         int rows, int K, int E, void* stream);
int polus_ivfpq_coarse_update(int dtype, const void* x, long ldx, const uint16_t* coarse, const void* prev, void* out,
                              int32_t* counts, int T, int K, int E, void* stream);

/* ---- refine: exact re-scoring of per-query candidate ids against stored single ([CLS]) vectors (refine.hip; the second
 * stage of FAISS' IndexRefine and of ScaNN's reordering, and the bi-encoder rerank behind a lexical first stage; no
 * counterpart in the reference).  A compressed index proposes R > k candidates, this kernel scores those R against better
 * vectors, polus_topk_merge_ids keeps the best k.
 *
 * polus_cls_rerank:  Q [B, E] in `dtype` (f32 or bf16), row stride ldq >= E;  D [N, E] in `dtype`, row stride ldd >= E;
 *   cand int32 [B, C], row stride ldcand >= C;  score f32 [B, C], row stride lds >= C
 *   n           = cand[b, c]
 *   score[b, c] = <Q[b], D[n]> by the rule below          for n in [0, N)
 *               = -inf, and nothing is read for it          for n outside [0, N)   (-inf is what polus_topk_merge_ids drops;
 *                                                           the contract of polus_maxsim_rerank and polus_ivfpq_scores_ids)
 *   Columns past C are not written.  A repeated id is scored once per copy.  Document addresses are 64-bit.  Q and D may
 *   hold NaN and +-inf; they propagate by IEEE rules.  No atomics, no workspace, no LDS; bitwise reproducible.
 * Arithmetic.  bf16 is widened to f32 (exact).  Every f32 operation is one IEEE rounding, never an fma, so NumPy float32
 *   reproduces every bit (tests/refine_ref.py).  The order is a function of E alone: the features are taken in groups of 8
 *   consecutive ones; partial l = 0 .. 63 adds, from +0.0 and in ascending e, fl(q_e * d_e) for every e with
 *   (e div 8) mod 64 == l; then six rounds p_l = fl(p_l + p_(l xor o)) for o = 32, 16, 8, 4, 2, 1 (the xor order of
 *   polus_pq_update); the score is p_0.  The bits of a score depend on its (query, document) pair only: not on B, C, the
 *   column it stands in, ldcand, the chunking of a search, or how many candidates a wave or a workgroup handles.
 * polus_cls_rerank_fp8:  the same call with codes uint8 [N, E] (OCP e4m3fn, row stride ldd >= E) and scale f32 [N] in place
 *   of D; Q stays in `dtype`.  The sum runs over fl(f32(q_e) * f32(code_e)) in the same order, then
 *   score = fl(scale[n] * sum), one more rounding.  A power-of-two scale commutes with every rounding, so
 *     polus_cls_rerank_fp8(Q, codes, scale) is bit for bit polus_cls_rerank(Q, D) with D = T(codes) * scale,
 *   provided no product or partial sum under- or overflows f32 (scales of a unit-norm or N(0,1) corpus are ~2^-8).  All
 *   quantisation error therefore sits in polus_cls_fp8_quantize.
 * Kernel.  One workgroup of 4 waves per (query, contiguous range of candidate columns); a wave owns a candidate, so its id
 *   is wave-uniform.  Lane l holds the query's groups l, l + 64, ... in registers for the whole launch and reads the same
 *   groups of a row, 16 bytes (bf16), 32 (f32) or 8 (codes) at a time; the rows of a wave's next candidates are requested
 *   before the current ones are reduced (8 rows in flight per wave at E <= 1024, 4 up to 2048, 2 above).  The cross-lane
 *   rounds use DPP, swizzles and one bpermute.  The column range of a workgroup follows B * C and the CU count of the
 *   current device (about 16 waves per CU over the launch, 1 .. 64 columns a wave), so one query with 1000 candidates
 *   still occupies 250 workgroups.  A gather of whole rows: bound by memory latency, not by arithmetic.
 * Limits (refused before any launch): dtype f32 or bf16; E a multiple of 16 in [16, 5120]; 1 <= B, C <= 65535;
 *   1 <= N <= 2^31 - 1; ldq, ldd >= E; ldcand, lds >= C; non-null pointers; Q and D / codes 16-byte aligned, and row strides
 *   that keep every row 16-byte aligned (ldq and ldd multiples of 4 in f32, of 8 in bf16; ldd a multiple of 16 for codes).
 *
 * polus_cls_fp8_quantize / polus_cls_fp8_dequantize:  the quantiser of polus_fp8_quantize_rows, word for word (the integer
 *   rule for the exponent, one power-of-two scale per row, nothing saturates, a NaN element ignored by amax and kept as a
 *   NaN code, a zero row with e = 0; the same device code, csrc/fp8_common.h), over whole rows:  x, y [rows, E] in
 *   `dtype`, contiguous;  codes uint8 [rows, E], contiguous;  scale f32 [rows].  One wave per row, two passes over it.
 *   Limits (refused before any launch): dtype f32 or bf16; rows >= 1; E a multiple of 16 in [16, 5120]; non-null
 *   pointers; x / y and codes 16-byte aligned. */
int polus_cls_rerank(int dtype, const void* Q, long ldq, const void* D, long ldd, const int32_t* cand, long ldcand,
                     float* score, long lds, int B, int C, int N, int E, void* stream);
int polus_cls_rerank_fp8(int dtype, const void* Q, long ldq, const uint8_t* codes, long ldd, const float* scale,
                         const int32_t* cand, long ldcand, float* score, long lds, int B, int C, int N, int E, void* stream);
int polus_cls_fp8_quantize(int dtype, const void* x, uint8_t* codes, float* scale, int rows, int E, void* stream);
int polus_cls_fp8_dequantize(int dtype, const uint8_t* codes, const float* scale, void* y, int rows, int E, void* stream);

/* ---- argmax over the last axis (PolusClassifier.inference, polus/models.py:148-150) */
int polus_argmax(const float* x, long ldx, int32_t* out, int rows, int C, void* stream);

/* ---- confusion matrix of the validation path (polus/metrics.py:51-66, tf.math.confusion_matrix):
 * cm[row_idx[i]][col_idx[i]] += 1 for i < n; cm is int32 [C, C] on the device and is ACCUMULATED into
 * (zero it to start); C <= 128.  Integer atomics: exact.  A pair with an index outside [0, C) adds nothing to cm
 * and 1 to *rejected (device int32, accumulated; may be null): tf.math.confusion_matrix raises on such input, the
 * caller decides (polus_amd/metrics.py raises in evaluate()). */
int polus_confusion_matrix(const int32_t* row_idx, const int32_t* col_idx, int64_t n, int C,
                           int32_t* cm, int32_t* rejected, void* stream);

/* ---- BIO span decoding and strict entity matching over tag tensors (bio.hip; polus/ner/bio.py decode_bio with
 * allow_errors=True as documented, polus/ner/utils.py eval_list_of_entity_sets).  tags int32 [B, S], row stride >= S.
 * scheme int32 [C]: -1 for an outside tag (O, PAD, ...), else 2 * type + (1 for I-, 0 for B-).  mask int32 [B, S]
 * (NULL = every token kept): a token with mask 0 is removed before decoding, so the kept tokens on either side of it
 * are neighbours, and its tag is never interpreted.  For a kept token j with previous kept token p of the row:
 *   in an entity   iff scheme[tag] != -1; a tag outside [0, C) decodes as outside and is counted as rejected;
 *   starts one     iff it is B-x, or I-x and p is absent, outside (counted as inside_tag_after_other_tag) or of
 *                  another type (inside_tag_with_different_entity_type);
 *   ends one       iff it is in one and the next kept token is absent, outside or a start.
 * An entity is (row, start column, last column + 1, type); it never continues into the next row.
 *
 * polus_bio_entity_counts decodes tags_a and tags_b under one mask and ACCUMULATES (zero them to start)
 *   counts int32 [T, 3]: per type (entities in both with the same row, start, end and type; entities of a; of b);
 *   stats int32 [6]: kept tokens, rejected values (each tensor counted on its own), inside_tag_after_other_tag and
 *                    inside_tag_with_different_entity_type of a, then the same two of b.
 * polus_bio_spans writes a row's entities as (start, end_exclusive, type) in order of start into spans int32
 * [B, M, 3] (contiguous) and their number into count int32 [B]: the true number even above M, of which only the first
 * M are written; slots behind min(count, M) are not touched.  *rejected (device int32, may be null) is accumulated.
 * One wave per row, lanes over 64 tokens per step, all flags as 64-bit ballot masks with a small carry between steps;
 * per-type counts through an LDS histogram and integer atomics: exact, independent of launch order; span order from
 * a popcount prefix of the start mask.  No workspace.  Memory-bound: every tag and mask element is read once.
 * Limits (refused before any launch): 0 < C <= 256; 0 < T <= 128; S >= 1; M >= 1; row strides >= S; non-null tags,
 * scheme and outputs.  B == 0 returns POLUS_OK without a launch.  The contents of scheme are the caller's to check
 * (polus_amd/ner/bio.py check_scheme); a code naming a type >= T decodes as outside. */
int polus_bio_entity_counts(const int32_t* tags_a, long lda, const int32_t* tags_b, long ldb,
                            const int32_t* mask, long ldm, const int32_t* scheme, int C, int T, int B, int S,
                            int32_t* counts, int32_t* stats, void* stream);
int polus_bio_spans(const int32_t* tags, long ldt, const int32_t* mask, long ldm, const int32_t* scheme, int C,
                    int B, int S, int32_t* spans, int M, int32_t* count, int32_t* rejected, void* stream);

/* ---- optimizer (optimizer.apply_gradients, polus/training.py:191): Keras Adam /
 * HF AdamWeightDecay over a flat f32 arena.  `seg` is a device table of int64 triples
 * (begin, end, flags) covering [0,n) in chunks; flags bit0 = apply weight decay,
 * bit1 = write a bf16 copy of the updated value to shadow[i] (GEMM weights).
 *   p -= lr*wd*p (decayed tensors) ; m,v update ; p -= lr_t * m / (sqrt(v)+eps)
 * g is multiplied by grad_scale and, if clip_scale != NULL, by *clip_scale (device). */
int polus_adam_step(float* p, const float* g, float* m, float* v, void* shadow_bf16,
                    const int64_t* seg, int n_seg, int64_t n,
                    float lr, float lr_t, float beta1, float beta2, float eps, float weight_decay,
                    float grad_scale, const float* clip_scale, void* stream);
/* sum of squares of g[0..n) -> *out (deterministic two-stage); polus_sqnorm_segments sums only the
 * windows [seg[3k], seg[3k+1]) of g (the polus_adam_step segment table: the variables actually being
 * updated; workspace >= 4096 bytes); then polus_clip_scale writes
 * min(1, clip_norm / sqrt(sum_k sqnorm[k] * grad_scale^2)) -- tf.clip_by_global_norm over n_terms partial
 * sums (one per parameter arena). */
size_t polus_sqnorm_workspace_bytes(int64_t n);
int polus_sqnorm(const float* g, int64_t n, float* out, void* workspace, size_t workspace_bytes, void* stream);
int polus_sqnorm_segments(const float* g, const int64_t* seg, int n_seg, float* out,
                          void* workspace, size_t workspace_bytes, void* stream);
int polus_clip_scale(const float* sqnorm, int n_terms, float grad_scale, float clip_norm, float* out_scale, void* stream);
/* f32 -> bf16 copy (shadow weights refresh after load / broadcast) and bf16/f32 casts */
int polus_cast(int src_dtype, const void* src, int dst_dtype, void* dst, int64_t n, void* stream);
/* dst[cols][rows] = src[rows][cols]^T for bf16 (transposed weight shadow read by dX = dY . W) */
int polus_transpose_bf16(const void* src, void* dst, int rows, int cols, void* stream);
/* Many matrices at once: matrix s lives at element offset segs[4s] of BOTH src_base and dst_base
 * (rows segs[4s+1], cols segs[4s+2]); segs[4s+3] = index of its first 64x64 tile in the launch
 * (ascending), total_tiles = sum of tiles.  `segs_dev` is a device array of 4*nseg int64.  Both bases must be
 * 8-byte aligned and every offset a multiple of 4 elements (matrices of 4k x 4l move 8 bytes per access).  Used
 * once per optimizer step to refresh the transposed bf16 weight shadows that dX = dY.W reads
 * (replaces the implicit transpose inside tape.gradient's MatMul grad, polus/training.py:185). */
int polus_transpose_bf16_batched(const void* src_base, void* dst_base, const void* segs_dev, int nseg,
                                 int total_tiles, void* stream);
/* du = dy * act'(u) elementwise (activation gradient of a Dense whose dY is not produced by
 * a polus_gemm epilogue) */
int polus_act_bwd(int dtype, const void* dy, const void* u, void* du, int64_t n, int act, void* stream);
/* y = a*x elementwise, f32 (gradient averaging when the comm backend lacks AVG) */
int polus_scale(float* x, float a, int64_t n, void* stream);

/* ---- data-parallel collectives over RCCL / xGMI: the device side of the six Horovod touch points of the
 * reference -- hvd.init (polus/__init__.py:109-122), hvd.DistributedGradientTape's gradient averaging
 * (polus/training.py:182-185) and hvd.broadcast_variables (polus/training.py:210-211).
 * One communicator per process (one process per GPU).  Rank 0 draws a 128-byte id with polus_comm_unique_id and
 * hands it to the other ranks over any host channel (the Python side uses the torchrun TCP store); every rank
 * then calls polus_comm_init(rank, world, id).  Collectives are queued on `stream` and return immediately; buffers
 * are device pointers; `dtype` is POLUS_F32 or POLUS_BF16 (bf16 = half the bytes on the links, sums rounded to bf16).
 *   allreduce_sum      buf[count] := sum over ranks (in place); the 1/world factor is folded into polus_adam_step
 *   reduce_scatter_sum recv[recv_count] := rank's slice of the sum of send[world * recv_count]
 *   all_gather         recv[world * send_count] := concatenation of every rank's send[send_count]
 *   broadcast          buf[bytes] := root's buf
 * group_start / group_end bracket several collectives into one RCCL launch. */
#define POLUS_COMM_ID_BYTES 128
int polus_comm_unique_id(void* out_id128);
int polus_comm_init(void** comm, int rank, int world, const void* unique_id128);
int polus_comm_destroy(void* comm);
/* what RCCL itself says about the communicator: ranks it spans, this rank, the HIP device it is bound to
 * (ncclCommCount / ncclCommUserRank / ncclCommCuDevice) -- bench.py prints n_ranks as `rccl_ranks` */
int polus_comm_info(void* comm, int* n_ranks, int* rank, int* device);
int polus_comm_broadcast(void* comm, void* buf, size_t bytes, int root, void* stream);
int polus_comm_allreduce_sum(void* comm, void* buf, size_t count, int dtype, void* stream);
int polus_comm_reduce_scatter_sum(void* comm, const void* send, void* recv, size_t recv_count, int dtype, void* stream);
int polus_comm_all_gather(void* comm, const void* send, void* recv, size_t send_count, int dtype, void* stream);
int polus_comm_group_start(void);
int polus_comm_group_end(void);

#ifdef __cplusplus
}
#endif
#endif /* POLUS_HIP_H */
