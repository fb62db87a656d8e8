/*
 * dwamd.h -- C ABI of libdwamd.so: the MI355X (gfx950 / CDNA4) kernels of the Whisper distillation hot path.
 *
 * The reference (huggingface/distil-whisper) has no FFI layer of its own: its hot path calls the Python surface
 * of `transformers` (WhisperFeatureExtractor + WhisperForConditionalGeneration) which dispatches to ATen/rocBLAS/
 * MIOpen kernels.  Each entry point below names the reference site it replaces (paths relative to the reference
 * tree `training/`, `TF:` = transformers/models/whisper of the pinned transformers==5.15.0).
 *
 * Conventions
 *   - every function returns 0 on success, a hipError_t value (>0) if a launch failed, or a negative DW_E* code
 *     for an invalid argument; nothing throws across this boundary;
 *   - the caller owns every buffer (device pointers from its own allocator); kernels never allocate;
 *   - `stream` is a hipStream_t passed as void*; all work is enqueued asynchronously on it, no host sync inside;
 *   - bf16 = 16-bit brain float (the upper half of an IEEE binary32), row-major everywhere, "ld" = leading
 *     dimension in ELEMENTS;
 *   - re-entrant: may be called from the Python main thread (forward) and the autograd engine thread (backward).
 */
#ifndef DWAMD_H
#define DWAMD_H
#include <stdint.h>
#ifdef __cplusplus
extern "C" {
#endif

#define DW_OK 0
#define DW_EINVAL (-1)  /* bad argument (alignment, K %% 64, null pointer ...) */
#define DW_EUNSUP (-2)  /* unsupported shape (e.g. head_dim != 64)            */

#define DW_F32 0
#define DW_BF16 1

int dw_version(void);

/* ---- a1: log-mel front end --------------------------------------------------------------------------------------
 * Replaces WhisperFeatureExtractor._torch_extract_fbank_features (TF:feature_extraction_whisper.py:135-168), called
 * from run_distillation.py:1176,1234 and run_eval.py:628-642.
 * audio [batch][n_samples] f32 (n_samples = 480000), hann window 400 (periodic), hop 160, reflect-pad centre STFT,
 * power spectrum, mel_filters [201][n_mels] f32 (HF layout), log10(clamp 1e-10), max(x, clipmax-8), (x+4)/4.
 * out [batch][n_mels][n_frames] f32 with n_frames = n_samples/160.  twiddle [400][2] f32 = (cos, sin)(2*pi*i/400),
 * window [400] f32; clipmax [batch] f32 scratch (overwritten).
 * n_samples >= 400 and a multiple of 160, 1 <= n_mels <= 256, n_mels * n_frames a multiple of 4 and `out` 16-byte aligned (the
 * normalisation pass moves four floats per lane); DW_EINVAL otherwise, before any launch. */
int dw_logmel(const float* audio, int batch, int n_samples, const float* mel_filters, int n_mels,
              const float* twiddle, const float* window, float* out, float* clipmax, void* stream);

/* ---- a3/a4/a5/a6: dense projections on the bf16 MFMA ------------------------------------------------------------
 * Replaces nn.Linear / nn.Conv1d (after im2col) forward+backward GEMMs (TF:modeling_whisper.py:279-282, 375-376,
 * 444-445, 566-567, 970).   C[M,N] = epilogue( op(A)[M,K] . op(B)[K,N] ), fp32 accumulation.
 *   trans_a = 0: A stored [M][lda] (K contiguous)      trans_a = 1: A stored [K][lda] (M contiguous)
 *   trans_b = 0: B stored [N][ldb] (K contiguous, i.e. the nn.Linear weight layout)
 *   trans_b = 1: B stored [K][ldb] (N contiguous)
 * Requirements: K %% 64 == 0 (pad with zeros), lda/ldb multiples of 8, base pointers 16-byte aligned.
 * Epilogue, in this order (each step optional):
 *   v = acc + bias[n]                      (bias f32 [N])
 *   Z[m][n] = bf16(v)                      (z_out, ldz; the pre-activation kept for backward)
 *   v = gelu(round_bf16(v))                (act == 1; exact erf GELU on the bf16-rounded value, as autocast does)
 *   v = v * gelu'(Zin[m][n])               (zgrad_in bf16, ldzg: fused GELU backward)
 *   v = (round_res ? round_bf16(v) : v) + R[m %% r_row_mod or m][n]     (residual R, f32 or bf16, ldr)
 *   C[m][n] = v as f32 or bf16             (c_dtype, ldc)
 * R may alias C (in-place accumulation: every element is read and written by the same lane). */
typedef struct DwGemm {
    const void* a;      /* bf16 */
    const void* b;      /* bf16 */
    void* c;            /* f32 or bf16 */
    const float* bias;  /* f32 [N] or NULL */
    void* z_out;        /* bf16 or NULL */
    const void* zgrad_in; /* bf16 or NULL */
    const void* r;      /* residual or NULL */
    int64_t lda, ldb, ldc, ldz, ldzg, ldr;
    int32_t m, n, k;
    int32_t trans_a, trans_b;
    int32_t act;        /* 0 none, 1 gelu */
    int32_t c_dtype;    /* DW_F32 / DW_BF16 */
    int32_t r_dtype;    /* DW_F32 / DW_BF16 */
    int32_t r_row_mod;  /* 0: R row = m; >0: R row = m %% r_row_mod (positional table broadcast) */
    int32_t round_res;  /* 1: round v to bf16 before adding R (autocast semantics) */
    int32_t tile;       /* 0 auto, 128 or 256: force the block tile; 16: the skinny-M (m <= 64) weight-streaming kernel;
                           129 (probing): like 0 for outputs below two rounds of 256-row tiles, refused for k-major A / split K */
    int32_t split_k;    /* > 1: the K range is cut into that many slices, combined either by atomic_acc or by
                           storing fp32 partials at c + slice * slice_stride (then call dw_reduce_slices) */
    int32_t atomic_acc; /* 1: C (f32, plain epilogue) += result with float atomics (gradient accumulation) */
    int64_t slice_stride; /* elements between the partial outputs of consecutive K slices (split_k > 1, no atomics) */
    /* Decode-step fusions, honoured by the skinny-M kernel only (m <= 32 for ln_x, m <= 64 for kv_out; any other launch
     * with these fields set is rejected with DW_EINVAL).  All zero = off. */
    const void* ln_x;        /* A = bf16(LayerNorm(ln_x)) computed on load over the K columns (`a` is ignored; k <= 1280):
                                the LayerNorm in front of a projection (TF:modeling_whisper.py:459, 474, 491) */
    const float* ln_gamma;   /* f32 [k] */
    const float* ln_beta;    /* f32 [k] */
    void* kv_out;            /* bf16 K/V cache: output columns >= kv_split of row m are stored at
                                kv_out[((m / kv_rows_per_batch) * kv_batch_pitch + kv_row0 + m % kv_rows_per_batch) * kv_ld
                                       + (n - kv_split)] instead of C (the in-place cache append of
                                TF:modeling_whisper.py:312-335); requires a bf16 output without activation / residual */
    int64_t ld_lnx, kv_ld;
    int32_t ln_x_dtype;      /* DW_F32 / DW_BF16 */
    int32_t kv_split, kv_rows_per_batch, kv_batch_pitch, kv_row0;
    float ln_eps;
    int32_t z_is_gelu_grad;  /* 1: z_out (with act = 1) receives gelu'(z) in fp16 instead of z in bf16, and zgrad_in is read as
                                such: the backward epilogue multiplies by the stored derivative instead of evaluating it
                                (same bytes; the derivative is rounded to 11 bits where the reference keeps fp32) */
    float* colsum_out;       /* f32 [N] or NULL: the column sums of the stored C (as rounded to its dtype) are ADDED to it with
                                float atomics -- the bias gradient of the Linear whose output gradient this GEMM produces
                                (dX of fc2 -> fc1.bias), without a separate pass over C.  Tile kernels only, no K slices. */
} DwGemm;
int dw_gemm_bf16(const DwGemm* g, void* stream);
/* out[i] (+)= sum over slices of part[s*stride + i]; n, stride multiples of 4 (split-K combination, deterministic). */
int dw_reduce_slices(const float* part, int64_t stride, int slices, float* out, int64_t n, int accumulate, void* stream);
/* The same over [rows][cols] matrices whose rows are ld_part (slabs, slice_stride elements apart) / ld_out elements apart. */
int dw_reduce_slices_ld(const float* part, int64_t slice_stride, int64_t ld_part, int slices, float* out, int64_t ld_out,
                        int rows, int cols, int accumulate, void* stream);
/* Grouped weight gradients: C_i (+)= A_i^T . B_i for 1 <= count <= DW_WGRAD_GROUP_MAX problems in ONE launch, one 320 x 256 output
 * tile per workgroup, no K slices and nothing to combine -- the weight matrices of a layer together fill one round of the CUs where
 * each alone needs a split of k (csrc/gemm_wgrad_group.hip).  All problems share the contraction length k (the token rows); both
 * operands are k-major bf16 as for dw_gemm_bf16 with trans_a && trans_b: a [k][lda] holds the m_i columns, b [k][ldb] the n_i.
 * accumulate = 0: c_i is stored (whatever it held); 1: c_i += the product (every element read and written once by the same lane).
 * Every output element is one fp32 chain over k in ascending order: deterministic, the same bits from every launch.
 * DW_EINVAL, before any launch and with nothing written, unless: every m_i %% 320 == 0 and n_i %% 256 == 0 (both > 0); k > 0 and
 * k %% 64 == 0; the tiles of the group sum(m_i / 320 * n_i / 256) number at most the CUs the persistent GEMMs occupy (256, or
 * dw_debug_set key 9); k * lda_i * 2 and k * ldb_i * 2 are below 2^31 - 1 (31-bit buffer offsets); a_i, b_i and c_i are 16-byte
 * aligned, lda_i and ldb_i multiples of 8 with lda_i >= m_i and ldb_i >= n_i, ldc_i a multiple of 4 with ldc_i >= n_i. */
#define DW_WGRAD_GROUP_MAX 4
typedef struct DwWgradProblem {
    const void* a;   /* bf16 [k][lda] */
    const void* b;   /* bf16 [k][ldb] */
    float* c;        /* f32 [m][ldc] */
    int64_t lda, ldb, ldc;
    int32_t m, n;
} DwWgradProblem;
int dw_wgrad_group(const DwWgradProblem* problems, int count, int k, int accumulate, void* stream);

/* ---- LayerNorm (TF:modeling_whisper.py:371,377,434,443,446,573,682), eps 1e-5, statistics in f32 ---------------
 * x [rows][cols] f32 or bf16 (x_dtype), y bf16 [rows][cols]; mean/rstd f32 [rows] (may be NULL for inference). */
int dw_layernorm_fwd(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, float* mean,
                     float* rstd, int rows, int cols, float eps, void* stream);
/* dx = LN'(dy); if accumulate: dres[rows][cols] (f32) += dx else dres = dx.  dgamma/dbeta f32 [cols] are ADDED to
 * (zero them first).  Optional fused outputs: dres_lowp (bf16 [rows][cols]) = bf16(dres) -- the gradient the
 * next residual branch's GEMMs consume -- and dres_colsum (f32 [cols], ADDED to) = its column sums = the bias gradient
 * of that branch's output projection.  The three column sums are taken in float64 in a fixed order (the same inputs give
 * the same bits) through `sums`: caller-owned, 8-byte aligned, at least dw_layernorm_bwd_ws_bytes(rows, cols) bytes, any
 * content; it must stay untouched until the work queued on `stream` has run. */
int dw_layernorm_bwd_ws_bytes(int rows, int cols);
int dw_layernorm_bwd(const void* dy_bf16, const void* x, int x_dtype, const float* mean, const float* rstd,
                     const float* gamma, float* dres, int accumulate, float* dgamma, float* dbeta, void* dres_lowp,
                     float* dres_colsum, int rows, int cols, void* sums, int64_t sums_bytes, void* stream);
/* The same two with row pitches in elements (>= cols, multiples of 4; 8 for bf16 x): activation buffers whose rows are padded
 * by 128 bytes so that the 128-byte pieces a GEMM tile reads from 256-320 consecutive rows do not fall on two of an XCD's sixteen
 * L2 channels (rows 2 560 / 10 240 bytes apart do; engine.row_pad, tools/gemm_stride_probe.py). */
int dw_layernorm_fwd_ld(const void* x, int x_dtype, const float* gamma, const float* beta, void* y, float* mean,
                        float* rstd, int rows, int cols, float eps, int64_t ldx, int64_t ldy, void* stream);
int dw_layernorm_bwd_ld(const void* dy_bf16, const void* x, int x_dtype, const float* mean, const float* rstd,
                        const float* gamma, float* dres, int accumulate, float* dgamma, float* dbeta, void* dres_lowp,
                        float* dres_colsum, int rows, int cols, int64_t lddy, int64_t ldx, int64_t lddres,
                        int64_t ldlowp, void* sums, int64_t sums_bytes, void* stream);

/* ---- attention core (TF:modeling_whisper.py:215-238 / integrations/sdpa_attention.py), head_dim 64 --------------
 * q [B*Lq rows], k,v [B*Lk rows]: bf16, head h of a row at element offset h*64, row strides ldq/ldk/ldv/ldo
 * (elements).  o bf16 same addressing with ldo; lse f32 [B][H][Lq] (natural-log logsumexp of scale*q.k).
 * softmax(scale * q k^T [+ causal mask]) v; the reference pre-scales q by 0.125 and passes scaling=1.0, which is
 * bit-identical to scale=0.125 here (power of two). */
int dw_attn_fwd(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Lq, int Lk,
                int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int causal, float scale, void* stream);
/* Same kernel with explicit batch pitches (rows between consecutive batches of q/o and of k/v): reads a padded KV
 * cache in place during greedy decoding (TF:modeling_whisper.py:312-335 EncoderDecoderCache).  lse may be NULL.
 * causal: 0 none, 1 query i sees keys <= i, 2 bottom-right aligned (query i sees keys <= i + Lk - Lq: several new
 * queries against a longer cache -- the multi-token verify step of speculative decoding, run_eval.py:578-599).
 * The rule holds at Lq == 1 too: with causal 1 the single query is query 0 and attends to key 0 only, whatever Lk is
 * (a single query against a whole cache is causal 0 or 2). */
int dw_attn_fwd_ex(const void* q, const void* k, const void* v, void* o, float* lse, int B, int H, int Lq, int Lk,
                   int64_t ldq, int64_t ldk, int64_t ldv, int64_t ldo, int64_t q_batch_rows, int64_t kv_batch_rows,
                   int causal, float scale, void* stream);
/* Forward over RAGGED batches of packed rows (forward-only passes: the frozen teacher's decoder over the live positions of a
 * batch, run_distillation.py:1472-1480 with the dead decoder positions left out; no lse).  n_seq sequences; sequence i has
 * q_len[i] (1 <= q_len[i] <= max_q) queries at rows q_start[i], q_start[i] + 1, ... of q / o (int32 arrays on the device).
 * Self-attention: kv_start = q_start and kv_len = q_len -- keys / values are rows of the same packed buffers (causal 0 / 1).
 * Cross-attention: kv_start = kv_len = NULL -- k / v are [kv_batches][kv_batch_rows] rectangles with Lk valid rows each and
 * sequence i reads batch min(i, kv_batches - 1) (n_seq may exceed kv_batches by filler sequences whose results are unused).
 * Same arithmetic per query as dw_attn_fwd over the rectangular layout (bit-identical rows). */
int dw_attn_fwd_varlen(const void* q, const void* k, const void* v, void* o, int n_seq, int H, int max_q, int Lk, int64_t ldq,
                       int64_t ldk, int64_t ldv, int64_t ldo, const int32_t* q_start, const int32_t* q_len,
                       const int32_t* kv_start, const int32_t* kv_len, int kv_batches, int64_t kv_batch_rows, int causal,
                       float scale, void* stream);
/* delta: caller-owned f32 scratch of 2*B*H*Lq elements (the dQ kernel stores -rowsum(dO*O) and -lse/scale of its queries
 * there; the dK/dV kernel, launched behind it, starts its accumulators from them).  dq/dk/dv bf16 with row strides
 * lddq/lddk/lddv. */
int dw_attn_bwd(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                float* delta, void* dq, void* dk, void* dv, int B, int H, int Lq, int Lk, int64_t ldq, int64_t ldk,
                int64_t ldv, int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, int causal,
                float scale, void* stream);
/* The same, plus (optional, may be NULL) the bias gradients of the projections that produced q and v: dq_colsum /
 * dv_colsum f32 [B][H*64] receive (ADDED with float atomics) the PER-BATCH-ROW column sums of the dq / dv matrices as
 * stored, from the kernels that write dq / dv instead of a separate pass over them; the caller adds the B partial rows
 * (dw_reduce_slices) into q_proj.bias.grad / v_proj.bias.grad.  Per batch row because every 32-row wave tile of a
 * (batch, head) adds to the same 64 addresses: one [H*64] target for the whole batch serialises 1 500 atomics per
 * address and cost more than the pass it replaced.  (k_proj has no bias, TF:modeling_whisper.py:279.) */
int dw_attn_bwd_ex(const void* q, const void* k, const void* v, const void* o, const void* d_o, const float* lse,
                   float* delta, void* dq, void* dk, void* dv, int B, int H, int Lq, int Lk, int64_t ldq, int64_t ldk,
                   int64_t ldv, int64_t ldo, int64_t lddo, int64_t lddq, int64_t lddk, int64_t lddv, int causal,
                   float scale, float* dq_colsum, float* dv_colsum, void* stream);

/* ---- a7: fused CE + temperature-KL distillation loss (run_distillation.py:1453-1462, 1486-1493 and
 * TF:modeling_whisper.py:1083-1087).  s/t logits bf16 [rows][ld] (V valid columns), labels int64 [rows] (-100 =
 * ignore).  losses f32[4] = {ce, kl*T^2, 0.8-weighted total, n_valid}.  If dlogits != NULL the gradient of
 * grad_scale * total w.r.t. the student logits is written there (bf16 [rows][ld], may alias s_logits; columns
 * V..ld-1 are zeroed).  row_ce/row_kl f32 [rows] scratch; counts int32[2] scratch. */
int dw_distill_loss(const void* s_logits, const void* t_logits, const int64_t* labels, int rows, int V, int64_t ld,
                    float temperature, float ce_weight, float kl_weight, float grad_scale, float* losses,
                    void* dlogits, float* row_ce, float* row_kl, int32_t* counts, void* stream);
/* The same with the mix {ce_weight, kl_weight} read from DEVICE memory (`weights`: f32[2]) by the gradient pass and the
 * total: for a caller whose weights are device scalars -- the upstream gradients autograd hands to the reference's own loss
 * lines `0.8 * ce_loss + kl_weight * kl_loss` (run_distillation.py:1486-1493) when they run over the drop-in modules' lazy
 * logits (distil_whisper_amd.modeling.LazyLogits) -- no host round trip, graph-capturable. */
int dw_distill_loss_w(const void* s_logits, const void* t_logits, const int64_t* labels, int rows, int V, int64_t ld,
                      float temperature, const float* weights, float grad_scale, float* losses, void* dlogits,
                      float* row_ce, float* row_kl, int32_t* counts, void* stream);

/* ---- Stored top-k teacher targets (offline distillation; the format is stated here and nowhere else) -------------------------
 * For one label position -- one row z of teacher logits, bf16, V valid columns --, a temperature T > 0 and 1 <= k <= 64, k < V:
 *   K        the k columns with the largest z; equal values go to the LOWER column (-0 counts as +0); stored in order of value
 *            descending, then column ascending.  bf16 widens exactly: the selection is exact and has one right answer
 *   logp[j]  = z[K_j] / T - logsumexp(z / T) over all V columns, fp32
 *   rest     = sum over c not in K of exp(z[c] / T - lse), fp32: summed over the tail term by term, never 1 - sum exp(logp);
 *              exactly 0 when every tail term underflows.  (Computed as sum_{c not in K} e_c / sum_c e_c, e_c = exp((z[c] - max z) / T),
 *              and logp[j] as (z[K_j] - max z) / T - log sum_c e_c: the same numbers without a rounded lse inside an exponent.)
 * A batch: idx int32 [B, Td, k], logp float32 [B, Td, k], rest float32 [B, Td], with the temperature and V they were made at;
 * targets are bound to that temperature.
 *
 * dw_logits_topk: logits bf16 [rows][ld] -> idx [rows][k], logp [rows][k], rest [rows].  One launch, one workgroup per row; no
 * floating-point atomics: equal inputs give equal bits.  Checked before the launch, in this order:
 *   DW_EINVAL  a null pointer; logits not 8-byte, idx / logp / rest not 4-byte aligned; rows < 1, V < 1, ld < V, ld not a multiple
 *              of 4, temperature not in (0, FLT_MAX]; k < 1 or k >= V
 *   DW_EUNSUP  V > 53 248 (thirteen 4-column chunks per lane), k > 64
 * A refused call launches nothing and writes nothing. */
int dw_logits_topk(const void* logits, int rows, int V, int64_t ld, float temperature, int k, int32_t* idx, float* logp,
                   float* rest, void* stream);
/* dw_distill_loss with the teacher row replaced by its stored targets (idx / logp int32 / f32 [rows][k], rest f32 [rows], made at
 * `temperature`): the KL divergence of the two distributions with the columns outside K merged into one bucket.  It never exceeds
 * the dense KL and equals it, gradient included, when rest == 0.  Per row, q = softmax(z_s / T), p_j = exp(logp[j]), r = rest:
 *   ce      the dense kernel's term, counted where label != -100
 *   row_kl  = sum_j p_j (logp[j] - log q_{K_j}) + r (log r - log qR)     (second term 0 when r == 0; counted where label >= 0;
 *             stored like the dense kernel's row_kl: T^2 enters with the mean, losses[1] = sum(row_kl) / n * T^2)
 *   qR      = sum over c not in K of q_c, accumulated over the non-members themselves (a membership bitmap of V bits in LDS), never
 *             "whole minus the members".  With e_c = exp((z_c - max z) / T): qR = max(sum_{c not in K} e_c, FLT_MIN) / sum_c e_c --
 *             the tail sum is clamped from below by FLT_MIN = 2^-126, so a row whose student tail underflows stays finite
 *   the KL part of the gradient, in the place of softmax(z_s/T) - softmax(z_t/T): q_c - p_c for c in K, q_c (1 - r / qR) otherwise
 * losses, dlogits (may alias s_logits; columns V..ld-1 zeroed), row_ce / row_kl / counts, grad_scale and the all-ignored batch (NaN
 * means, a zero gradient, losses[3] = 0) are dw_distill_loss's.  A row whose label excludes it from both sums (-100, or any other
 * negative label) is not looked at: whatever idx / logp / rest hold there changes nothing and is not dereferenced.  In a counted
 * row the k indices are distinct columns of [0, V) (the caller's promise; an index outside that range is skipped).
 * Checked before any launch: DW_EINVAL as dw_distill_loss (s_logits / dlogits 16-byte aligned, ld a multiple of 8), a null or not
 * 4-byte aligned idx / logp / rest, k < 1 or k >= V; then DW_EUNSUP for V > 53 248 or k > 64.  Nothing is written then. */
int dw_distill_loss_topk(const void* s_logits, const int32_t* idx, const float* logp, const float* rest, int k,
                         const int64_t* labels, int rows, int V, int64_t ld, float temperature, float ce_weight, float kl_weight,
                         float grad_scale, float* losses, void* dlogits, float* row_ce, float* row_kl, int32_t* counts,
                         void* stream);
/* The same with the mix read from device memory, as dw_distill_loss_w. */
int dw_distill_loss_topk_w(const void* s_logits, const int32_t* idx, const float* logp, const float* rest, int k,
                           const int64_t* labels, int rows, int V, int64_t ld, float temperature, const float* weights,
                           float grad_scale, float* losses, void* dlogits, float* row_ce, float* row_kl, int32_t* counts,
                           void* stream);

/* ---- embeddings (TF:modeling_whisper.py:675-676, 736-762) ------------------------------------------------------
 * out[b*T+t][:] = tok[ids[b*T+t]][:] + pos[t][:]; tables f32 or bf16 (tab_dtype); out f32 or bf16.
 * D a multiple of 4; tok, pos and out aligned to four of their elements (8 bytes for bf16, 16 for f32), DW_EINVAL otherwise.
 * 0 <= ids < rows of tok is the caller's promise. */
int dw_embed_fwd(const int64_t* ids, const void* tok, const void* pos, int tab_dtype, void* out, int out_dtype,
                 int B, int T, int D, void* stream);
/* dtok[ids[r]] += dx[r] (atomic f32), dpos[t] += sum_b dx[b*T+t] (skipped if dpos NULL). */
int dw_embed_bwd(const float* dx, const int64_t* ids, float* dtok, float* dpos, int B, int T, int D, void* stream);

/* ---- conv front end helpers (TF:modeling_whisper.py:566-567, 618-625) ------------------------------------------
 * conv1 (k3,p1,s1) and conv2 (k3,p1,s2) run as im2col + dw_gemm_bf16 with W' [D][3*C] (W'[d][k*C+c] = W[d][c][k]).
 * im2col_mel: mel f32 [B][C][T] -> xcol bf16 [B*T][kpad], xcol[(b,t)][k*C+c] = mel[b][c][t+k-1], zero padded. */
int dw_im2col_mel(const float* mel, void* xcol, int B, int C, int T, int kpad, void* stream);
/* im2col_s2: a bf16 [B*T][C] -> xcol bf16 [B*T/2][3*C], xcol[(b,t)][k*C+c] = a[b][2t+k-1][c].
 * T even, C a multiple of 8, a and xcol 16-byte aligned (eight bf16 per lane); DW_EINVAL otherwise. */
int dw_im2col_s2(const void* a, void* xcol, int B, int T, int C, void* stream);
/* col2im_s2 + GELU backward: dz[b][r][c] = gelu'(z[b][r][c]) * sum_{2t+k-1=r} dxcol[(b,t)][k*C+c].
 * T even, C a multiple of 8, dxcol, z and dz 16-byte aligned (eight bf16 per lane); DW_EINVAL otherwise. */
int dw_col2im_s2_gelu_bwd(const void* dxcol, const void* z, void* dz, int B, int T, int C, void* stream);
/* dz = bf16(dy) * gelu'(z): backward of the GELU after conv2 (dy f32 or bf16, z/dz bf16, n %% 4 == 0).
 * z, dz and a bf16 dy 8-byte aligned, an f32 dy 16-byte aligned (four elements per lane); DW_EINVAL otherwise. */
int dw_gelu_bwd(const void* dy, int dy_dtype, const void* z, void* dz, int64_t n, void* stream);
/* conv weight <-> GEMM weight layouts: w [D][C][3] f32 <-> wp [D][kpad] (bf16 pack / f32 grad unpack-accumulate). */
int dw_pack_conv_weight(const float* w, void* wp_bf16, int D, int C, int kpad, void* stream);
int dw_unpack_conv_grad(const float* gwp, float* gw, int D, int C, int kpad, int accumulate, void* stream);

/* ---- small streaming kernels -----------------------------------------------------------------------------------*/
int dw_cast_f32_bf16(const float* x, void* y, int64_t n, void* stream);
int dw_cast_bf16_f32(const void* x, float* y, int64_t n, void* stream);
/* out[n] (+)= sum_r x[r][n], x bf16 [rows][ld] (bias gradients). */
int dw_colsum_bf16(const void* x, int64_t ld, int rows, int cols, float* out, int accumulate, void* stream);
/* Rows through an index list (int32, device): gather (scatter = 0) dst[i][:] = src[idx[i]][:], scatter dst[idx[i]][:] =
 * src[i][:], i < n; row_bytes and both pitches multiples of 16.  The padding-free decoder pass keeps [live rows][D]
 * activations between the attention calls -- the reference computes all 448 padded positions of every row of the batch
 * (collator, run_distillation.py:405-478; decoder, TF:modeling_whisper.py:690-795). */
int dw_move_rows(const void* src, int64_t src_pitch_bytes, void* dst, int64_t dst_pitch_bytes, const int32_t* idx, int n,
                 int row_bytes, int scatter, void* stream);
/* y = a (bf16/f32) + b (bf16/f32) elementwise into f32 or bf16 */
int dw_add(const void* a, int a_dtype, const void* b, int b_dtype, void* y, int y_dtype, int64_t n, void* stream);

/* ---- a9: global-norm clip + AdamW (run_distillation.py:1377-1407, 1611-1614; torch.optim.AdamW semantics) -------
 * sumsq: out[0] += sum(g^2) (zero it first).  adamw: clip = min(1, max_norm/(sqrt(sumsq[0])+1e-6)) (max_norm <= 0
 * disables), g' = g*clip*grad_mul; p *= 1-lr*wd; m,v update; p -= lr/bc1 * m/(sqrt(v)/sqrt(bc2)+eps); the bf16
 * shadow copy used by the GEMMs is refreshed in the same pass (shadow may be NULL). */
#define DW_SUMSQ_PARTIALS 2048
/* partials: caller-owned scratch of DW_SUMSQ_PARTIALS floats.  Two deterministic stages (per-block partials, then one
 * block adds them in a fixed order; no float atomics): data-parallel replicas must derive bit-identical clip
 * coefficients from their bit-identical all-reduced gradients. */
int dw_sumsq_f32(const float* g, int64_t n, float* out, float* partials, void* stream);
int dw_adamw(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, const float* sumsq,
             float max_norm, float grad_mul, double lr, double beta1, double beta2, double eps, double weight_decay,
             int step, void* stream);
/* The same update with the optimizer's scalar state RESIDENT ON THE DEVICE, so that one whole training step (forward,
 * backward, clip, AdamW) is a fixed launch sequence that can be captured in a HIP graph and replayed: nothing the host
 * passes by value changes from step to step.  state: 8 doubles, caller-owned: [0] lr (the host rewrites it before a step
 * when an LR scheduler runs: get_scheduler, run_distillation.py:1410-1415), [1] number of optimizer steps taken so far,
 * [2] beta1, [3] beta2, [4..6] written by dw_adam_tick for the update kernels of this step, [7] unused.
 * dw_adam_tick: once per optimizer step before the dw_adamw_dev calls of that step: advances state[1] and derives
 * lr/(1-beta1^step), sqrt(1-beta2^step).  gate (optional, f32 device scalar): when *gate <= 0 the whole step is skipped
 * (nothing advances, no parameter changes) -- the trainer passes the loss kernel's n_valid so that a batch without a
 * single label does not move the weights by momentum / weight decay alone. */
int dw_adam_tick(double* state, const float* gate, void* stream);
int dw_adamw_dev(float* p, const float* g, float* m, float* v, void* shadow_bf16, int64_t n, const float* sumsq,
                 float max_norm, float grad_mul, const double* state, double eps, double weight_decay, void* stream);

/* ---- a10b: training-mode dropout of the student ------------------------------------------------------------------
 * Replaces nn.functional.dropout at the row-local sites of TF:modeling_whisper.py: the embeddings (WhisperEncoder.forward
 * 625, WhisperDecoder.forward 763: `dropout`), the three residual branches of a layer (WhisperEncoderLayer 398 / 406,
 * WhisperDecoderLayer 479 / 493 / 502: `dropout`) and the GELU output of fc1 (404 / 500: `activation_dropout`); run_distillation.py sets them on the student config (the `--dropout` family of the Flax recipe).
 * Mask: one bit per element, byte b of row r covers columns 8b .. 8b+7 (bit j = column 8b+j), row pitch cols/8 bytes;
 * cols %% 8 == 0.  Element e = row*cols + col keeps its value iff word (e & 3) of Philox4x32-10(counter = (e >> 2, site,
 * step_lo, step_hi), key = seed) >= thr, thr = min(2^32-1, round(p * 2^32)); rows*cols < 2^34 (else DW_EUNSUP).  `step` is
 * a 64-bit counter in DEVICE memory (dw_dropout_tick advances it), so a replayed HIP graph draws fresh masks.
 * dw_dropout_fwd: out = residual + m * t with t = u * scale, rounded to bf16 when u is bf16 (scale = 1/(1-p)); residual
 *   may be NULL; u / residual / out are bf16 or f32 with row pitches ldu / ldr / ldo in elements (16-byte aligned rows);
 *   out may alias u or residual (same dtype and pitch: every element is read and written by the same lane); mask is written.
 * dw_dropout_bwd: out = m * t with t = dy * scale, rounded to bf16 when dy is bf16; reads the mask; may run in place. */
int dw_dropout_fwd(const void* u, int u_dtype, int64_t ldu, const void* residual, int r_dtype, int64_t ldr, void* out,
                   int out_dtype, int64_t ldo, uint8_t* mask, int rows, int cols, uint32_t thr, float scale, uint64_t seed,
                   int site, const uint64_t* step, void* stream);
int dw_dropout_bwd(const void* dy, int dy_dtype, int64_t lddy, const uint8_t* mask, void* out, int out_dtype, int64_t ldo,
                   int rows, int cols, float scale, void* stream);
int dw_dropout_tick(uint64_t* step, void* stream);

/* ---- a10c: SpecAugment of the training forward ------------------------------------------------------------------
 * TF:modeling_whisper.py _compute_mask_indices / WhisperModel._mask_input_features (`apply_spec_augment`, `mask_time_*`,
 * `mask_feature_*`): spans of `mask_length` positions are zeroed along the time axis (features[b, :, t]) and / or the
 * feature axis (features[b, f, :]) of the fp32 log-mel features [B][n_mels][T].  ONE launch draws both masks of every row
 * and applies them; out == in is the in-place form (only the zeros are stored), otherwise out = masked copy of in.
 * An axis with mask_*_prob <= 0 is not masked (and its length is not checked).  Per axis (time: axis_len = T, len_b =
 * lengths[b] clamped to [0, T], or T when lengths is NULL; feature: axis_len = len_b = n_mels), in double precision:
 *   epsilon = word 0 of Philox4x32-10(counter = (0, site, step_lo, step_hi), key = seed) * 2^-32, one per axis and call;
 *   n(len)  = (int)(prob * len / mask_length + epsilon); = max(n, min_masks); = axis_len / mask_length if n * mask_length >
 *             axis_len; = max(len - (mask_length - 1), 0) if that is smaller;  n_b = n(len_b), max_n = n(axis_len);
 *   max_n == 0: no position of any row is masked.  n_b == 0 < max_n: position axis_len - 1 of row b alone is masked (the
 *   reference's dummy index).  Otherwise n_b distinct starts are drawn from [0, M), M = len_b - (mask_length - 1), by Floyd's
 *   subset algorithm: for w = 0 .. n_b - 1, j = M - n_b + w, t = (r_w * (j + 1)) >> 32, take j if t was taken before, where
 *   r_w is word (w & 3) of Philox4x32-10(counter = (((b + 1) << 16) | (w >> 2), site, step_lo, step_hi), key = seed); the
 *   mask is the union of [start, start + mask_length).
 * site = DW_SPEC_SITE_TIME / DW_SPEC_SITE_FEATURE, above every site of dw_dropout_fwd (< 512), so dropout's masks do not
 * depend on SpecAugment; `step` is dropout's device-resident counter (dw_dropout_tick).  time_mask uint8 [B][T] and feat_mask
 * uint8 [B][n_mels] (1 = zeroed) are written when not NULL.  DW_EINVAL: null in / out / step, mask_length < 1 or > axis_len
 * of an active axis; DW_EUNSUP: B > 65534, T or n_mels > 16384. */
#define DW_SPEC_SITE_TIME 512u
#define DW_SPEC_SITE_FEATURE 513u
int dw_spec_augment(const float* in, float* out, int B, int n_mels, int T, const int32_t* lengths, double mask_time_prob,
                    int mask_time_length, int mask_time_min_masks, double mask_feature_prob, int mask_feature_length,
                    int mask_feature_min_masks, uint64_t seed, const uint64_t* step, uint8_t* time_mask, uint8_t* feat_mask,
                    void* stream);

/* ---- a11: token selection of one greedy-decoding step for the whole batch (TF:generation/logits_process.py processors
 * MinNewTokensLength, SuppressTokensAtBegin, SuppressTokens, WhisperTimeStamp as installed by
 * TF:models/whisper/generation_whisper.py:1774-1812, then argmax and the EOS / pad bookkeeping of GenerationMixin).
 * logits bf16 [B][ld] (V valid columns); suppress / begin_suppress: uint8 [V] masks (1 = never sampled) or NULL,
 * begin_suppress applies when first != 0; no_eos != 0 masks eos (min_new_tokens not reached); forced != 0: position n is
 * still inside the forced prefix (cur = tokens[b][n], nothing else happens).  Timestamp rules: ts_begin =
 * no_timestamps_token_id + 1 (< 0 disables), max_initial = max_initial_timestamp_index (< 0 none), begin_index = length
 * of the forced prefix.  tokens int64 [B][tok_ld]: history in [0, n), the selected token is written to [n]; cur int64 [B]
 * receives it as well; done uint8 [B] in/out (finished rows get `fill`); eos < 0 disables the bookkeeping. */
int dw_greedy_select(const void* logits, int B, int V, int64_t ld, const uint8_t* suppress,
                     const uint8_t* begin_suppress, int first, int no_eos, int forced, int ts_begin, int max_initial,
                     int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos, int fill, uint8_t* done,
                     int64_t* cur, void* stream);
/* The same step with the two history-dependent default processors of GenerationMixin in front of the rules above (TF
 * `_get_logits_processor` order): RepetitionPenaltyLogitsProcessor -- the logit v of every id in tokens[b][0, n) (the decoder
 * prompt included) becomes v < 0 ? v * repetition_penalty : v / repetition_penalty, once per id -- and
 * NoRepeatNGramLogitsProcessor -- an id that would complete an n-gram of size no_repeat_ngram the row already holds is
 * never selected (0 = off).  repetition_penalty must be finite and > 0 (1.0 = off), no_repeat_ngram >= 0, V <= 65536 (the
 * history bitmaps of the workgroup); with 1.0 and 0 it selects what dw_greedy_select selects. */
int dw_greedy_select_history(const void* logits, int B, int V, int64_t ld, const uint8_t* suppress,
                             const uint8_t* begin_suppress, int first, int no_eos, int forced, int ts_begin, int max_initial,
                             int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos, int fill, uint8_t* done,
                             int64_t* cur, float repetition_penalty, int no_repeat_ngram, void* stream);
/* dw_greedy_select_history with GenerationMixin's SequenceBiasLogitsProcessor and NoBadWordsLogitsProcessor
 * (`generate(sequence_bias=, bad_words_ids=)`) in the same launch.  The table holds S <= 1024 sequences of 1..32 token ids in
 * [0, V): sequence s is bias_tok[bias_off[s], bias_off[s + 1]) (int32, device memory) with the bias bias_val[s] (f32; -inf =
 * a bad word) for the column of its last token.  The entries must be ordered by that column, ascending; within a column their
 * order is the order in which their biases are summed.  A one-token sequence always counts; a longer one is ignored when it is
 * longer than the history (bias_off[s + 1] - bias_off[s] > n) and counts otherwise iff the last len - 1 tokens of
 * tokens[b][0, n) equal its prefix.  The biases that count for a column are summed first (fp32, table order; no atomics on
 * floats) and the sum is added to the logit once, in front of the repetition penalty; a column whose sum is -inf is never
 * selected.  S = 0 (the pointers may be NULL) selects what dw_greedy_select_history selects.  The contents of the table are
 * not checked (decoding.sequence_bias_table builds and validates it). */
int dw_greedy_select_bias(const void* logits, int B, int V, int64_t ld, const uint8_t* suppress,
                          const uint8_t* begin_suppress, int first, int no_eos, int forced, int ts_begin, int max_initial,
                          int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos, int fill, uint8_t* done,
                          int64_t* cur, float repetition_penalty, int no_repeat_ngram, const int* bias_tok,
                          const int* bias_off, const float* bias_val, int S, void* stream);
/* The sampled step (`generate(do_sample=True, temperature=, top_k=, top_p=)`: TF:generation/utils.py `_get_logits_processor` +
 * `_sample`; the fallback passes of TF:generation_whisper.py `generate_with_fallback`, run_eval.py:690-739) in one launch.  The
 * processed score of every column is the one dw_greedy_select_history judges (excluded = -inf); then, in the reference's order,
 * TemperatureLogitsWarper (s / temperature), TopKLogitsWarper (top_k <= 0: off; else columns below the min(top_k, V)-th largest of
 * all V scores are removed, ties at the threshold stay), TopPLogitsWarper (top_p >= 1: off; else a column is removed iff the
 * softmax probability of all columns with a score <= its own is <= 1 - top_p; the largest always stays.  The reference removes a
 * prefix of an ascending sort and so splits the group of equal scores at the boundary in an order that depends on the device's
 * sort; this entry keeps that group whole), and the draw: argmax over the surviving columns of softmax(s)[c] / noise[b][c], equal
 * quotients to the smaller column.  noise f32 [B][noise_ld]: Exponential(1) variates -- with `noise.exponential_(1, generator)`
 * on a contiguous [B, V] tensor the token is the one torch.multinomial(softmax(s), 1, generator) draws.  A position inside the
 * forced prefix is not sampled (there is no `forced`).  temperature finite and > 0, top_k >= 0, 0 < top_p <= 1, V <= 65536;
 * equal inputs give equal tokens (no floating-point atomics). */
int dw_sample_select(const void* logits, int B, int V, int64_t ld, const uint8_t* suppress,
                     const uint8_t* begin_suppress, int first, int no_eos, int ts_begin, int max_initial,
                     int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos, int fill, uint8_t* done,
                     int64_t* cur, float repetition_penalty, int no_repeat_ngram, float temperature, int top_k,
                     float top_p, const float* noise, int64_t noise_ld, void* stream);

/* ---- beam search: one token step of `generate(num_beams=k)` (TF:generation/utils.py `_beam_search`; csrc/beam.hip).
 * dw_beam_candidates: for each of the R = B * k beam rows, in fp32: lse = log-sum-exp over all V raw logits (the reference takes
 * log_softmax before its processors and does not renormalise), lp[c] = logits[c] - lse where the rules of dw_greedy_select allow
 * column c (no_eos, begin_suppress when first != 0, suppress, the timestamp rules from the row's own history tokens[r][0, n),
 * the timestamp mass rule), -inf elsewhere; the row's K = 2k largest lp[c] + run_scores[r] go to cand_val / cand_tok [R][K],
 * ordered by value descending, then column ascending; with fewer than K allowed columns the rest is (-inf, eos).  logits bf16
 * [R][ld] as in dw_greedy_select; eos in [0, V).  K <= 32 and V <= 65536, else DW_EUNSUP.  stop: device word; non-zero = the
 * search has ended, nothing is written. */
int dw_beam_candidates(const void* logits, int R, int V, int64_t ld, const uint8_t* suppress, const uint8_t* begin_suppress,
                       int first, int no_eos, int ts_begin, int max_initial, const int64_t* tokens, int64_t tok_ld, int n,
                       int begin_index, int eos, const float* run_scores, int K, float* cand_val, int32_t* cand_tok,
                       const int32_t* stop, void* stream);
/* dw_beam_update: the bookkeeping of the step whose candidates dw_beam_candidates wrote, for the whole batch (one workgroup
 * decides, a row-parallel launch moves the token rows).  Per utterance: the k * K candidates merged into the top K by (value
 * descending, flat index beam * V + token ascending); hits = EOS or cur + 1 >= max_length; the k best open continuations become
 * running_out / run_scores / src_rows (int64 [R]: the row each new beam continues, for the caller's K/V gather) / next_tok (int64
 * [R]: the next step's input); hits among the first k are merged into sequences_out / beam_scores / finished / lengths (int32:
 * generated tokens) with score value / fin_div; the early-stopping heuristic (early_stopping 0 = False, 1 = True, 2 = "never")
 * with best running score / hyp_div updates unsat (uint8 [B]); the loop condition goes to *stop (1 = ended).  fin_div =
 * (cur + 1 - prompt_len) ^ length_penalty and hyp_div = hyp_len ^ length_penalty come from the host.  Equal scores: the lower
 * index wins.  running / sequences int64 [R][tok_ld]; in and out must be different buffers and every buffer holds the pad token
 * beyond its hypotheses; columns [0, cur] are written.  With *stop set on entry the state is left as it is: out = in, src_rows =
 * identity, next_tok untouched.  plan: int32 [4 * R] scratch.  k <= 16, V <= 65536, B * k <= 65535, else DW_EUNSUP. */
int dw_beam_update(const float* cand_val, const int32_t* cand_tok, int B, int k, int V, int cur, int prompt_len, int max_length,
                   int eos, int early_stopping, float fin_div, float hyp_div, const int64_t* running_in, int64_t* running_out,
                   const int64_t* sequences_in, int64_t* sequences_out, int64_t tok_ld, float* run_scores, float* beam_scores,
                   uint8_t* finished, int32_t* lengths, uint8_t* unsat, int32_t* stop, int64_t* src_rows, int64_t* next_tok,
                   int32_t* plan, void* stream);

/* ---- speculative (assisted) greedy decoding: the selection and the bookkeeping of one round (TF:generation/utils.py
 * `_assisted_decoding`, greedy; reached from run_eval.py:578-599, 706-707 `assistant_model=`; csrc/assist.hip).
 * dw_assist_pick: the token the rules of dw_greedy_select pick at n consecutive positions of every row, without the EOS / pad
 * bookkeeping.  logits bf16, V valid columns (ld >= V, a multiple of 4; base 8-byte aligned): the row at element offset
 * (b * batch_rows + j) * ld predicts tokens[b][L + j], j < n (batch_rows >= n).  tokens int64 [B][tok_ld]: position (b, j) is
 * judged against the history tokens[b][0, L + j) -- for j > 0 it includes the drafts at [L, L + j), which must be in place --
 * with begin_index = the decoder prompt length (1 <= begin_index <= L), begin_suppress at L + j == begin_index only, eos masked
 * while L + j - begin_index < min_new, ts_begin / max_initial / suppress as in dw_greedy_select, the timestamp mass rule
 * included; among equal scores the lower column wins.  own int64 [B][own_ld] (own_ld >= n) receives the tokens.  store != 0
 * (n == 1 only; the assistant's draft step): the token also goes to tokens[b][L] and cur[b] (int64 [B]).  No `done`: a draft
 * continues past an EOS it drafted.  One workgroup per (j, b); any V that dw_greedy_select takes; B <= 65535. */
int dw_assist_pick(const void* logits, int B, int n, int V, int64_t ld, int64_t batch_rows, const uint8_t* suppress,
                   const uint8_t* begin_suppress, int min_new, int ts_begin, int max_initial, int64_t* tokens, int64_t tok_ld,
                   int L, int begin_index, int eos, int64_t* own, int64_t own_ld, int store, int64_t* cur, void* stream);
/* dw_assist_accept: with own [B][own_ld] from dw_assist_pick(n = k + 1) and the k drafts at tokens[b][L, L + k): m_b = the number
 * of leading j < k with own[b][j] == tokens[b][L + j] (k for a row whose done[b] is set), n_ok = min over b (0 when k == 0); then
 * for j = 0 .. n_ok in order: c = done[b] ? fill : own[b][j]; tokens[b][L + j] = c; done[b] |= (c == eos).  eos < 0: no `done`
 * handling (done may be NULL).  result int32 [2] = {n_ok, eos >= 0 and every row done}.  Positions behind L + n_ok keep what
 * they hold.  One workgroup, one thread per row: B <= 1024 and k <= 1024, else DW_EUNSUP (the caller keeps its torch step). */
int dw_assist_accept(const int64_t* own, int64_t own_ld, int64_t* tokens, int64_t tok_ld, int B, int L, int k, int eos, int fill,
                     uint8_t* done, int32_t* result, void* stream);
/* Per-row acceptance: every row keeps its own length len[b] (int32 [B], device memory that the host never reads), so a rejected
 * draft of one row costs the other rows nothing; the decoder passes of such a round are dw_decode_step_rows.
 * dw_assist_pick_rows: dw_assist_pick with the host's L replaced by the device's len[b] + j0: the row at element offset
 * (b * batch_rows + j) * ld predicts tokens[b][len[b] + j0 + j] from the history tokens[b][0, len[b] + j0 + j); begin_suppress
 * where that index == begin_index, eos masked while it is < begin_index + min_new, every rule as in dw_assist_pick (the same
 * calls into select_rules.h).  len[b] >= begin_index (smaller values are read as begin_index).  store != 0 (n == 1; the
 * assistant's draft step number j0 of the round): the token also goes to tokens[b][len[b] + j0] and cur[b].  A position
 * >= tok_ld (a row that has ended at the end of the buffer) is not judged: own[b][j] = 0, nothing else is written.  tok_ld >
 * begin_index.  One workgroup per (j, b); B <= 65535. */
int dw_assist_pick_rows(const void* logits, int B, int n, int V, int64_t ld, int64_t batch_rows, const uint8_t* suppress,
                        const uint8_t* begin_suppress, int min_new, int ts_begin, int max_initial, int64_t* tokens, int64_t tok_ld,
                        const int32_t* len, int j0, int begin_index, int eos, int64_t* own, int64_t own_ld, int store,
                        int64_t* cur, void* stream);
/* dw_assist_accept_rows: with own [B][own_ld] from dw_assist_pick_rows(n = k + 1, j0 = 0) and row b's drafts at tokens[b][len[b],
 * len[b] + k).  A row is live when done[b] == 0 and len[b] < total; for a live row with kb = min(k, total - 1 - len[b]) drafts
 * offered (the caller sizes k so that kb == k): m_b = the number of leading j < kb with own[b][j] == tokens[b][len[b] + j]; for
 * j = 0 .. m_b in order c = own[b][j], tokens[b][len[b] + j] = c, and the row ends there when c == eos (eos < 0: never); len[b]
 * becomes the index behind the last token written, and the row also ends when that reaches `total`.  A row that has ended, in
 * this call or before, has tokens[b][len[b] .. min(old len[b] + k, total - 1)] = fill (the drafts behind its end), done[b] = 1
 * and is parked: pos_target[b] = pos_assistant[b] = 0.  A row still live: done[b] = 0, pos_target[b] = len[b] - 1 and
 * pos_assistant[b] = len[b] - 2, the positions from which the next round's passes re-feed it (the target's cache is valid below
 * len - 1, the assistant's below len - 2).  done uint8 [B] in/out (required, also for eos < 0).  result int32 [4] = {drafts
 * accepted, summed over the rows live on entry: min(tokens written, m_b); drafts offered to them: the sum of kb; 1 when no row is
 * live on return; the largest len among the rows live on return, 0 when there is none}.  tok_ld >= total >= 2.  One workgroup, one
 * thread per row: B <= 1024 and k <= 1024, else DW_EUNSUP. */
int dw_assist_accept_rows(const int64_t* own, int64_t own_ld, int64_t* tokens, int64_t tok_ld, int B, int k, int total, int eos,
                          int fill, int32_t* len, uint8_t* done, int32_t* pos_target, int32_t* pos_assistant, int32_t* result,
                          void* stream);

/* ---- a11: one decoder pass of cached greedy decoding as ONE call (the `decode_step` entry of SURVEY.md 8b).
 * Replaces `WhisperDecoder.forward` + `proj_out` on the cache branch (TF:modeling_whisper.py:690-795, 312-335, 1080)
 * as reached from `generate` (run_eval.py:739, run_distillation.py:1524-1528, run_pseudo_labelling.py:861-996).
 * Every launch of the pass is enqueued on `stream`; nothing is allocated, nothing synchronises (HIP-graph capturable).
 * All matrices bf16 in nn.Linear layout [out][in]; biases and LayerNorm parameters f32; q scaling 0.125 is applied
 * inside attention.  The caller owns every buffer (weights, caches, workspace). */
typedef struct DwDecoderLayer {
    const float *ln1_g, *ln1_b;  /* self_attn_layer_norm */
    const void* wqkv;            /* [3D][D]: q_proj | k_proj | v_proj weights stacked */
    const float* bqkv;           /* [3D] (the k part is zero: k_proj has no bias) */
    const void* wo;  const float* bo;    /* self_attn.out_proj */
    const float *ln2_g, *ln2_b;  /* encoder_attn_layer_norm */
    const void* wq;  const float* bq;    /* encoder_attn.q_proj */
    const void* wo2; const float* bo2;   /* encoder_attn.out_proj */
    const float *ln3_g, *ln3_b;  /* final_layer_norm */
    const void* w1;  const float* b1;    /* fc1 [ffn][D] */
    const void* w2;  const float* b2;    /* fc2 [D][ffn] */
    void* self_kv;               /* bf16 [batch][max_len][2D]: K | V of the generated prefix, appended in place */
    const void* cross_kv;        /* bf16 [batch*src_len][2D]: K | V of the encoder states (projected once per batch); rows
                                    DwDecodeStep.cross_kv_ld elements apart.  Not read (may be NULL) at cross_kv_fmt = 1 */
    const void *cross_k8, *cross_v8;   /* cross_kv_fmt = 1: codes uint8 [batch][heads][src_len][64] ("FP8 cross-attention K/V" below) */
    const float* cross_scale;    /* cross_kv_fmt = 1: float [batch][2][D], K's column scales then V's */
} DwDecoderLayer;
typedef struct DwDecodeStep {
    int32_t batch, n_new;        /* n_new new positions per sequence (1 = token step; > 1 = prefill / verify pass) */
    int32_t d_model, heads, ffn, n_layers;
    int32_t src_len, max_len;    /* encoder positions (1500); capacity of the self-attention cache */
    int32_t t;                   /* position of the first new token = number of cached positions */
    int32_t vocab, ldv;          /* LM-head rows used / padded (multiple of 16) = row pitch of logits */
    int32_t stream_dtype;        /* residual stream and embedding tables: DW_F32 (autocast student) or DW_BF16 */
    int32_t cross_kv_ld;         /* row pitch of every layer's cross_kv in elements; 0 = 2 * d_model.  (Rows padded by 128 bytes
                                    stream faster: the 128-byte K / V pieces of a head in consecutive 5 120-byte rows fall on four
                                    of an XCD's sixteen L2 channels -- 29.8 -> 26.4 us per layer at batch 16.) */
    const int64_t* ids;          /* [batch][n_new] */
    const void* tok_emb;         /* [vocab..][D] */
    const void* pos_emb;         /* [max_target_positions][D] (row t .. t+n_new-1 are used) */
    const float *lnf_g, *lnf_b;  /* decoder.layer_norm */
    const void* lm_head;         /* bf16 [ldv][D] (tied embedding, zero-padded rows) */
    const DwDecoderLayer* layers;
    void *x, *h, *qkv, *o, *a;   /* workspace, rows = batch*n_new: x [rows][D] stream dtype; h, o [rows][D], qkv
                                    [rows][3D], a [rows][ffn] bf16 */
    void* logits;                /* out: bf16 [rows][ldv] */
    int32_t cross_kv_fmt;        /* 0: the cross-attention reads DwDecoderLayer.cross_kv (bf16) -- the pass as it always was.
                                    1: it reads cross_k8 / cross_v8 / cross_scale through dw_decode_attn_proj_kv8, for every layer;
                                    every other launch of the pass is unchanged.  Only the token step has that kernel: n_new > 1,
                                    dw_decode_step_rows, a d_model outside 384 / 512 / 768 / 1024 / 1280, src_len > 8192 or
                                    dw_debug_set key 7 bit 3 set are DW_EUNSUP, a NULL cross_k8 / cross_v8 / cross_scale / bq /
                                    ln2_g / ln2_b of any layer, a cross_k8 / cross_v8 not 16-byte or a cross_scale not 4-byte aligned,
                                    and any other value of the field DW_EINVAL, before any launch. */
} DwDecodeStep;
int dw_decode_step(const DwDecodeStep* d, void* stream);
/* dw_decode_step_rows: the same pass with row b of the batch starting at position row_t[b] instead of d->t (which is ignored):
 * its n_new tokens take the position embeddings row_t[b] + j, their K / V are written to rows row_t[b] + j of the row's
 * self-attention cache, query j sees the keys [0, row_t[b] + j]; cross-attention, LayerNorms, GEMMs and the LM head are the
 * launches of dw_decode_step.  Cache rows of a sequence below row_t[b] must be valid; rows outside [row_t[b], row_t[b] + n_new)
 * are not written.  row_t: int32 [batch] in DEVICE memory, read by the kernels and never by the host (speculative decoding with
 * per-row acceptance writes it in dw_assist_accept_rows); max_t: a host bound, row_t[b] <= max_t and max_t + n_new <= max_len,
 * used for launch and LDS sizing only -- the kernels read an entry outside [0, max_t] as the nearer end of that range, so no
 * entry can address past the row's cache.  Three launches differ from dw_decode_step: the embedding, the K/V append (the QKV GEMM
 * runs without its fused append) and the self-attention, a kernel for few queries against per-row key counts: n_new <= 32 and
 * n_new * (64 + max_t + n_new) * 4 + 8320 <= 65536 bytes of LDS (n_new = 6 at any max_len <= 2000), batch <= 65535, else
 * DW_EUNSUP.  DW_EINVAL: what dw_decode_step refuses, a null or misaligned row_t, max_t < 0, max_t + n_new > max_len.  Refused
 * calls launch nothing.  Nothing is allocated, nothing synchronises. */
int dw_decode_step_rows(const DwDecodeStep* d, const int32_t* row_t, int32_t max_t, void* stream);
/* dw_decode_attn_proj: the token step's attention with its projection inside, alone -- the one launch dw_decode_step makes for a
 * layer's cross-attention (mode 0; dw_debug_set key 7 bit 3 clear) or self-attention (mode 1; bit 2 clear), through this very
 * function.  Per sequence b < B and head h < H (D = 64 * H), one workgroup:
 *   ln   = bf16(LayerNorm(x[b]; ln_g, ln_b, eps))                     x: [B] rows of D, x_dtype DW_F32 / DW_BF16, ldx elements apart
 *   mode 0:  q = bf16(w[h] . ln + bias[h])                            w bf16 [D][D], bias f32 [D]
 *            o[b][h] = softmax_j(scale * q . k[b][j][h]) v[b][j][h]   over the Lk keys j of k / v
 *   mode 1:  q, k_new, v_new the same way from w bf16 [3D][D] (q | k | v stacked), bias f32 [3D]; k_new | v_new are written to
 *            columns [0, D) | [D, 2D) of row t = Lk - 1 of sequence b in kv_app, and the softmax runs over the Lk - 1 rows of k / v
 *            in front of t and the new key, which is not read back from memory (Lk = 1: no key is read at all).
 * k, v: bf16, head h at element offset 64 * h, key j of sequence b at row b * kv_rows + j, rows ldkv elements apart (k and v are
 * usually two column offsets into one K | V buffer).  kv_app: bf16, same pitches (ldkv >= 2D), may be the buffer k points into;
 * ignored in mode 0.  o: bf16 [B][ldo].  fp32 sums over bf16 operands, P rounded to bf16 in front of the PV product.
 * Checked before any launch, in this order:
 *   DW_EINVAL  mode not 0 / 1; x_dtype not DW_F32 / DW_BF16; a null x, ln_g, ln_b, w, bias, k, v, o (kv_app in mode 1);
 *              B < 1, H < 1, Lk < 1, Lk > kv_rows;
 *              x, w, k, v, ln_g or ln_b not 16-byte aligned, ldx or ldkv not a multiple of 8 elements (the kernel issues 16-byte
 *              loads on all of them); bias not 4-byte, o / kv_app not 2-byte aligned
 *   DW_EUNSUP  B or H above 65535 (grid dimensions); D = 64 * H not one of 384 / 512 / 768 / 1024 / 1280 (the instantiations: a
 *              lane holds a weight row's fragments in registers); Lk > 8192 (one score per key in LDS)
 *   DW_EINVAL  ldx < D, ldo < D, ldkv < D (mode 1: < 2D)
 * A refused call launches nothing and writes nothing.  One launch on `stream`; nothing is allocated, nothing synchronises. */
int dw_decode_attn_proj(int mode, const void* x, int x_dtype, int64_t ldx, const float* ln_g, const float* ln_b, float eps,
                        const void* w, const float* bias, const void* k, const void* v, int64_t ldkv, int64_t kv_rows,
                        void* kv_app, void* o, int64_t ldo, int B, int H, int Lk, float scale, void* stream);
/* dw_decode_attn_proj_rows: mode 1 of dw_decode_attn_proj with sequence b at its own position: row_t int32 [B] in DEVICE memory
 * (the host never reads it; the kernel reads an entry outside [0, max_t] as the nearer end of that range), max_t the host's bound.
 * Sequence b writes k_new | v_new to row row_t[b] of its rows of kv_app and its softmax runs over row_t[b] + 1 keys; the workgroup
 * of (b, h) performs the arithmetic of the uniform kernel at Lk = row_t[b] + 1 in the same order, so o[b] and the appended row
 * are what dw_decode_attn_proj(mode 1, Lk = row_t[b] + 1) writes for that sequence, bit for bit.  LDS is sized by max_t + 1.
 * The refusals of dw_decode_attn_proj with Lk = max_t + 1, in front of the launch, and: DW_EINVAL for a null or misaligned row_t,
 * max_t < 0, max_t + 1 > kv_rows; DW_EUNSUP for max_t + 1 > 8192. */
int dw_decode_attn_proj_rows(const void* x, int x_dtype, int64_t ldx, const float* ln_g, const float* ln_b, float eps, const void* w,
                             const float* bias, const void* k, const void* v, int64_t ldkv, int64_t kv_rows, void* kv_app, void* o,
                             int64_t ldo, int B, int H, float scale, const int32_t* row_t, int32_t max_t, void* stream);
/* ---- FP8 cross-attention K/V (opt-in; the format is stated here and nowhere else) -------------------------------------------
 * Scope of a scale: one sequence b, one layer, one tensor (K or V), one column c < D, over the src_len rows j of that sequence.
 *   amax = max_j |x[b][j][c]|                                   over the bf16 values
 *   inv  = 448 / amax,  s = amax / 448                          two fp32 round-to-nearest divisions;  amax < 2^-100 (zero included):
 *                                                               inv = s = 1 -- the column counts as zero, its codes are signed zeros,
 *                                                               and 448 / amax is finite for every other column
 *   code = e4m3fn(x * inv)                                      fp32 product (not contracted with anything), rounded to nearest
 *                                                               even onto the OCP e4m3fn grid (4 exponent bits, bias 7, 3 mantissa
 *                                                               bits, subnormals of 2^-9, no infinities), saturated at +-448: never
 *                                                               a NaN code; the sign of a zero is kept
 *   value the kernels use = s * float(code)
 * The scales are per COLUMN: K's fold into the query and V's into the output once per workgroup, no scale is read per key, and an
 * outlier channel does not cost the other columns their precision.
 * Layout of a layer: codes head-major, uint8 [B][H][src_len][64] for K and for V (a (sequence, head) workgroup streams one
 * contiguous region whose 128-byte lines are wholly its own); scales float [B][2][D], K's D columns then V's.
 *
 * dw_cross_kv_quant: codes and scales of sequences [seq0, seq0 + n_seq) of a layer from the bf16 K | V rows the projection GEMM
 * writes: kv [n_seq * src_len][ld], K in columns [0, D), V in [D, 2D), D = 64 * H; row j of sequence seq0 + i is row i * src_len + j.
 * k8, v8, scales: the layer's whole buffers (sequence 0 first).  One launch, two sweeps (column maxima, then codes; the second reads
 * from L2).  Only the addressed sequences' codes and scales are written.  Checked before the launch, in this order:
 *   DW_EINVAL  a null kv, k8, v8 or scales;  seq0 < 0, n_seq < 1, src_len < 1, H < 1;
 *              kv not 16-byte aligned or ld not a multiple of 8 elements, k8 / v8 not 8-byte, scales not 4-byte aligned
 *   DW_EUNSUP  n_seq > 65535, H > 16384 (grid dimensions)
 *   DW_EINVAL  ld < 2D
 * A refused call launches nothing and writes nothing.  Nothing is allocated, nothing synchronises. */
int dw_cross_kv_quant(const void* kv, int64_t ld, void* k8, void* v8, float* scales, int seq0, int n_seq, int src_len, int H,
                      void* stream);
/* dw_decode_attn_proj_kv8: mode 0 of dw_decode_attn_proj over FP8 K/V, alone -- the launch dw_decode_step makes for a layer's
 * cross-attention at cross_kv_fmt = 1.  LayerNorm and q projection are those of dw_decode_attn_proj, sum for sum: q is the same
 * bf16 value, bit for bit.  With sK = kv_scale[b][0], sV = kv_scale[b][1], c = scale * log2(e):
 *   score_j = sum_d (q_d * c * sK_d) * float(k8[b][h][j][d])      fp32
 *   o[b][h][d] = bf16(sV_d * (sum_j bf16(P_j) * float(v8[b][h][j][d]) / sum_j P_j)),  P_j = exp2(score_j - max score)
 * k8, v8: uint8 [B][H][kv_rows][64], the first Lk rows of a head are read; kv_scale float [B][2][D]; o bf16 [B][ldo].
 * Checked before any launch, in this order:
 *   DW_EINVAL  x_dtype not DW_F32 / DW_BF16; a null x, ln_g, ln_b, w, bias, k8, v8, kv_scale, o; B < 1, H < 1, Lk < 1, Lk > kv_rows;
 *              x, w, k8, v8, ln_g or ln_b not 16-byte aligned, ldx not a multiple of 8 elements; bias or kv_scale not 4-byte, o
 *              not 2-byte aligned
 *   DW_EUNSUP  B or H above 65535; D = 64 * H not one of 384 / 512 / 768 / 1024 / 1280; Lk > 8192
 *   DW_EINVAL  ldx < D, ldo < D
 * A refused call launches nothing and writes nothing.  One launch on `stream`; nothing is allocated, nothing synchronises. */
int dw_decode_attn_proj_kv8(const void* x, int x_dtype, int64_t ldx, const float* ln_g, const float* ln_b, float eps, const void* w,
                            const float* bias, const void* k8, const void* v8, const float* kv_scale, int64_t kv_rows, void* o,
                            int64_t ldo, int B, int H, int Lk, float scale, void* stream);
/* dw_decode_token_rows: the token step (n_new == 1, else DW_EINVAL) with row b at position row_t[b] (row_t / max_t as for
 * dw_decode_step_rows): the launch sequence of dw_decode_step at n_new == 1 with two launches swapped -- the embedding takes the
 * position row per sequence, the self-attention with its projection and K/V append inside is dw_decode_attn_proj_rows.  With equal
 * positions the logits and caches are those of dw_decode_step, bit for bit.  Where D = 64 * heads has no such kernel, max_t + 1 >
 * 8192 or dw_debug_set key 7 has bit 2 set (the default: see there), the self-attention is that of dw_decode_step_rows (QKV GEMM,
 * append, attention over per-row key counts) and the pass is dw_decode_step_rows' own.  The step of continuous batching
 * (dw_slot_step below writes row_t and ids).  Nothing is allocated, nothing synchronises. */
int dw_decode_token_rows(const DwDecodeStep* d, const int32_t* row_t, int32_t max_t, void* stream);
/* dw_slot_step: the token selection of continuous batching (csrc/slots.hip), one 1024-thread workgroup per slot b < S.  Device
 * state per slot: tokens int64 [S][tok_ld], len (tokens held = the position this step fills), plen (prompt length = begin_index
 * of the rules), budget (plen + max_new_tokens, <= tok_ld), done, and the feed of the next pass row_t / cur (int64 [S]).
 * logits bf16 [S][ld]: row b is the output of the pass that fed cur[b] at position row_t[b].  With n = len[b]:
 *   done[b]                 the row is left alone; row_t[b] = 0, cur[b] = tokens[b][0] (parked at position 0)
 *   n < plen[b]             nxt = tokens[b][n] (teacher forcing)
 *   otherwise               nxt = the best allowed column of the row under suppress / begin_suppress (first = n == plen[b]),
 *                           min-new-tokens (EOS excluded while n - plen[b] < min_new) and the timestamp rules (ts_begin =
 *                           no_timestamps_token_id + 1, < 0: off; max_initial < 0: none) with the history tokens[b][0 .. n)
 *   then tokens[b][n] = nxt, len[b] = n + 1; a generated nxt that is `eos` or fills the budget (n + 1 >= budget[b]) sets done[b]
 *   and parks the slot, else row_t[b] = n, cur[b] = nxt.
 * A slot whose state no refill leaves behind (len < 1, len >= tok_ld, plen < 1) is set done and parked.  DW_EINVAL: a null or
 * misaligned pointer, S outside [1, 65535], tok_ld < 2, V < 1, ld < V, ld not a multiple of 4, logits not 8-byte aligned, the
 * timestamp rules without eos.  One launch; no argument depends on a position: with dw_decode_token_rows it replays from one HIP
 * graph. */
int dw_slot_step(const void* logits, int S, int V, int64_t ld, const uint8_t* suppress, const uint8_t* begin_suppress, int ts_begin,
                 int max_initial, int eos, int min_new, int64_t* tokens, int64_t tok_ld, int32_t* len, const int32_t* plen,
                 const int32_t* budget, uint8_t* done, int32_t* row_t, int64_t* cur, void* stream);
/* dw_slot_step_scores: dw_slot_step -- the same tokens and state, launch for launch -- which also keeps the two numbers the seek
 * loop's thresholds judge a window by.  lp_sum, nsp float [S]; nsp_pos int32 [S]; nsp_col: a column (< 0: nsp and nsp_pos are not
 * touched and may be null).  With n = len[b] before the step and row = the slot's logits row:
 *   done[b]                 neither number is touched
 *   a generated step        s = the processed row the pick judges: a column the rules exclude is -inf, and so is every text
 *                           column (c < ts_begin) when the timestamps' mass has taken the pick.
 *                           lp_sum[b] += s[nxt] - logsumexp(s), in fp32, an EOS included (no allowed column: nothing is added)
 *   n - 1 == nsp_pos[b]     nsp[b] = softmax(raw row)[nsp_col] when the step is forced (n < plen[b]), softmax(s)[nsp_col] when
 *                           it is generated.  No other forced step reads its logits.
 * The caller zeroes lp_sum[b] / nsp[b] when it fills a slot.  DW_EINVAL: as dw_slot_step; a null or misaligned lp_sum; nsp_col
 * >= V; nsp_col >= 0 with a null or misaligned nsp / nsp_pos.  A refused call launches nothing.  One launch. */
int dw_slot_step_scores(const void* logits, int S, int V, int64_t ld, const uint8_t* suppress, const uint8_t* begin_suppress,
                        int ts_begin, int max_initial, int eos, int min_new, int64_t* tokens, int64_t tok_ld, int32_t* len,
                        const int32_t* plen, const int32_t* budget, uint8_t* done, int32_t* row_t, int64_t* cur, float* lp_sum,
                        float* nsp, const int32_t* nsp_pos, int nsp_col, void* stream);

/* ---- token-level timestamps (TF:generation_whisper.py:241-381 `_extract_token_timestamps`, :43-61 `_median_filter`, :64-115
 * `_dynamic_time_warping`; reached from `generate(return_token_timestamps=True)`, TF:1146-1157).  The reference collects every
 * decoding step's eager cross-attention matrix and post-processes it on the host; here one teacher-forced decoder pass hands
 * the alignment layers' q / k projections to the first entry point and the rest stays on the device.
 *
 * dw_cross_attn_probs: probs[b][slot0 + i][l][0 .. Lk) = softmax over the Lk keys of scale * q[b*L + l, head heads[i]] .
 * k[b*kv_batch_rows + key, head heads[i]], i < n.  q bf16 [B*L rows][ldq], k bf16 [B][kv_batch_rows][ldk] (head h of a row at
 * element offset h*64; H = heads per row), heads int32 [n] ON THE DEVICE (an id outside [0, H) leaves its slot untouched),
 * probs f32 [B][n_total][L][ldp] -- the layers of one model fill one tensor, slot by slot.  fp32 softmax with the exact row
 * maximum.  ldq / ldk multiples of 8, ldp a multiple of 4 and >= Lk, 16-byte aligned bases, L <= 512, n_total <= 32. */
int dw_cross_attn_probs(const void* q, const void* k, const int32_t* heads, int n, float* probs, int B, int H, int L, int Lk,
                        int64_t ldq, int64_t ldk, int64_t kv_batch_rows, int n_total, int slot0, int64_t ldp, float scale,
                        void* stream);
/* dw_align_prepare (TF:341-365): for batch row b the token rows first_tok .. first_tok + n_tok[b] - 1 and the frame columns
 * 0 .. n_frames[b] - 1 of probs [B][n_heads][L][ldp] (n_tok / n_frames: int32 [B] on the device, clamped to L - first_tok /
 * max_frames): per (head, frame) column (w - mean) / std over the token axis (population std; a zero spread divides as IEEE
 * does), median of median_filter_width (odd, 1..9) along the frames with reflect padding -- unfiltered when n_frames[b] <=
 * width / 2 --, mean over the heads, negated -> cost f32 [B][L][ldc], rows 0 .. n_tok[b] - 1. */
int dw_align_prepare(const float* probs, int B, int n_heads, int L, int64_t ldp, int first_tok, const int32_t* n_tok,
                     const int32_t* n_frames, int max_frames, int median_filter_width, float* cost, int64_t ldc, void* stream);
/* dw_dtw (TF:64-115, 367-369): dynamic time warping over cost[b] (n_tok[b] x n_frames[b]) and its backtrace, one workgroup per
 * batch row -> first_frame int32 [B][L]: the frame index at which the path first reaches each token (`time_indices[jumps]`;
 * -1 where the reference's path reaches the token in its border column).  Same path as the reference function: one fp32
 * addition per cell, the same strict comparisons (ties, inf and NaN choose "left").  trace: caller-owned scratch, uint32
 * [B][L][trace_ld] with trace_ld >= ceil(max_frames / 16) (two bits per cell).  Rows with n_tok[b] == 0 and the entries behind
 * n_tok[b] are left as they are.  L <= 512. */
int dw_dtw(const float* cost, int B, int L, int64_t ldc, const int32_t* n_tok, const int32_t* n_frames, int max_frames,
           uint32_t* trace, int64_t trace_ld, int32_t* first_frame, void* stream);

/* ---- scores of finished sequences (TF:generation/utils.py `_sample`: the per-step `scores` -- logits after the processors -- and
 * `raw_logits` that `generate(output_scores=True / output_logits=True, return_dict_in_generate=True)` returns, and what
 * `compute_transition_scores` and `_retrieve_avg_logprobs`, TF:models/whisper/generation_whisper.py:1958-1975, read from them).
 * The logits come from ONE teacher-forced decoder pass over the finished sequences; this entry applies the processors of
 * dw_greedy_select to every (step, row) at once.  logits: DW_BF16 or DW_F32 (dtype), row (b, j) at element offset
 * (b * batch_rows + j) * ld, V valid columns (ld >= V, a multiple of 4; base 8- / 16-byte aligned) -- the row that predicts
 * tokens[b][begin_index + j], j < L.  tokens int64 [B][tok_ld], tok_ld >= begin_index + L; begin_index = length of the decoder
 * prompt.  suppress / begin_suppress: uint8 [V] masks or NULL (begin_suppress applies at j == 0 only); eos is masked while
 * j < min_new; ts_begin / max_initial / eos as in dw_greedy_select (ts_begin < 0: no timestamp rules).  Outputs, each may be NULL
 * (not all three): scores f32 [L][B][ld_scores] (ld_scores >= V, a multiple of 4, 16-byte aligned base): the logit itself where
 * the column is allowed, -inf where a rule masks it and in the pad columns; chosen f32 [B][L]: the processed score of
 * tokens[b][begin_index + j]; logprob f32 [B][L]: log_softmax of the processed row at that token (-inf when it is masked).
 * With suppress = begin_suppress = NULL, min_new = 0 and ts_begin < 0 nothing is masked: a widening copy of the raw logits.
 * One launch on `stream`; nothing is allocated, nothing synchronises.  B <= 65535. */
int dw_score_tokens(const void* logits, int dtype, int B, int L, int V, int64_t ld, int64_t batch_rows, const int64_t* tokens,
                    int64_t tok_ld, int begin_index, const uint8_t* suppress, const uint8_t* begin_suppress, int min_new,
                    int ts_begin, int max_initial, int eos, float* scores, int64_t ld_scores, float* chosen, float* logprob,
                    void* stream);

/* ---- self tests (diagnostics for bring-up; not on the hot path) --------------------------------------------------
 * Runs ds_read_b64_tr_b16 on a known LDS image: out int32 [64][4] = element ids received by each lane. */
int dw_selftest_tr16(int32_t* out, void* stream);
/* Tuning knobs for kernel A/B experiments and tests; not part of the hot path (defaults are the measured best).
 *   key 0   GEMM kernel choice (csrc/gemm.hip gemm_choose): 0 = the default rule; 1 = the reference kernels only (16-wave
 *           256 x 256 tile, 8-wave 128 x 128 tile for small grids); 2 = the default rule, and the 320 x 256 tile wherever it is
 *           eligible (row-major A, M % 320 == 0, N % 256 == 0, one K slice).  Every kernel gives bit-identical results.
 *   key 1   rasterisation strip width override (0 = rule);   key 6  strip L2 budget in 512 KiB units (default 4)
 *   key 9   persistent grid size in CUs (multiple of 8, default 256)
 *   key 10  dynamic per-XCD tile hand-out (default 1);   key 11  GEMM staging: bit 7 (128) requests the next tile's first
 *           operand tile before the epilogue at any K (the rule does so for K <= 1024); bit 4 (16) makes the 16x16x32
 *           kernels skip their epilogue (profiling: nothing is stored); other bits unused (default 1)
 *   key 4   single-query attention (Lq == 1): 1 = the streaming decode kernel (default), 0 = the tile kernel; other values
 *           are DW_EINVAL
 *   key 5   log-mel DFT on the matrix cores (default 1);   key 7  decode-step fusions off (bit 0 LayerNorm-on-load,
 *           bit 1 K/V append, bit 2 self-attention with its q / k / v projection inside, bit 3 cross-attention with its q
 *           projection inside; default 4)
 *   key 18  attention tile kernels take (tile, head, batch) in plain launch order instead of the XCD-aware order (default 0)
 *   key 21  LayerNorm kernels: bit 0 persistent fp32-input forward with next-row prefetch (bits 8-11: workgroups per CU),
 *           bit 1 backward with next-row / residual-gradient prefetch at two waves per SIMD (default 3; tools/ln_ab.py)
 *   key 22  wide row-major 256-row launches hand a partial last row block (<= 128 rows) to the 128-tile kernel when the full
 *           row blocks alone need one round of the CUs less (default 1; bit-identical)
 *   key 23  attention forward: threshold (in powers of two) by which a tile maximum must exceed the running reference of
 *           the online softmax before the reference moves (default 8; 0 = the exact running maximum, the A/B leg of
 *           tests/test_sharp_parity_gpu.py)
 *   key 25  outputs with fewer than two rounds of 256-row tiles (the decoders' M = 32 x live positions): kernel chosen by the
 *           rounds of the CUs it needs among 128 x 256 tiles in a three-stage operand ring (csrc/gemm_wp8_m128.hip), 256 x 256
 *           on 16x16x32 and 320 x 256 (default 1; 0 = the lock-step 128 x 128 kernel; bit-identical)
 * Every other key is DW_EINVAL (keys 3, 8, 15, 16, 17 and 26 selected experiment kernels that are retired: DESIGN_HISTORY.md).
 */
int dw_debug_set(int key, int value);

#ifdef __cplusplus
}
#endif
#endif
