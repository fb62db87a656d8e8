// Token scoring of finished sequences: the reference's logits processors applied to the logits of ONE teacher-forced decoder
// pass, for `generate(output_scores=True / output_logits=True)` and `compute_transition_scores`.
//
// Reference behaviour (third-party `transformers`, TF: = transformers/generation/): `_sample` (TF:utils.py) appends, per decoding
// step, `next_token_scores` (the logits after the processors) to `scores` and the untouched `next_token_logits` to `raw_logits`;
// the processors are MinNewTokensLengthLogitsProcessor, SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor and
// WhisperTimeStampLogitsProcessor (TF:logits_process.py, installed in that order by TF:models/whisper/generation_whisper.py:
// 1774-1812).  Consumers: `compute_transition_scores` (TF:utils.py) and the long-form code's `_retrieve_avg_logprobs`
// (TF:models/whisper/generation_whisper.py:1958-1975).
// Here the sequences are already decoded: step j of row b is a function of tokens[b][0 .. P + j) and of the logits row of
// position P - 1 + j, so every (step, row) pair is independent -- one 1024-thread workgroup each, no loop over steps.
//
// The rules are those of the kernels that pick the token during decoding, and they are implemented once, in select_rules.h
// (row_rules, rule_masks_of, column_allowed), with first = (j == 0), no_eos = (j < min_new) and begin_index = P;
// tests/test_generate_scores_gpu.py pins this kernel against greedy_select_kernel.  In prose, with tsb = the first timestamp id
// and the history h = tokens[b][P .. P + j) of the generated part:
//   * EOS is masked while j < min_new;  begin_suppress masks its columns at j == 0 only;  suppress masks its columns always;
//   * timestamp mode (ts_begin >= 0): <|notimestamps|> = tsb - 1 is masked always, and
//       j == 0                     only timestamps, at most max_initial steps in:   allowed [tsb, tsb + max_initial]
//       h ends text, timestamp     a timestamp or EOS must follow:                  allowed [eos, tsb) and the timestamps below
//       h ends timestamp, timestamp  (or j == 1 and h[0] is a timestamp)  text only:  allowed [0, tsb)
//       timestamps never decrease: with t = the last timestamp in h, timestamps below t are masked -- below t + 1 unless h ends
//       "text, timestamp" (a pair that is still open may be closed by the same value);
//   * the mass rule: if logsumexp over the allowed timestamp columns exceeds the best allowed text logit, every text column
//     (c < tsb) is masked.
// An allowed column keeps its logit (widened to fp32, which is exact for bf16); a masked one becomes -inf.
//
// Traffic: the fp32 `scores` write (L x B x ld_scores x 4 bytes) and the logits, half or as much, read ONCE: a row of up to
// 13 x 4096 columns -- every Whisper vocabulary -- stays in registers across the three reductions.  Measured
// (profiles/generate_scores_bench.json, V = 51 866, bf16): 2.2 TB/s, a third of the rate of a streaming copy, and 84 % of the
// time remains without the `scores` store -- the registers of the held row leave one workgroup per CU, so its loads, its
// reductions and its stores do not overlap with another's.  Plain kernel on the caller's stream: no allocation, no host
// synchronisation.
#include "common.h"
#include "select_rules.h"                            // SEL_NT and the rules
#include "../../include/dwamd.h"

#define SC_NPRE 13                                   // chunks of SEL_NT x 4 columns held in registers: 53 248 columns

struct ScoreP {
    const void* logits; long ld, batch_rows;
    const int64_t* tokens; long tok_ld;
    const uint8_t* suppress; const uint8_t* begin_suppress;
    float* scores; long ld_scores;
    float* chosen; float* logprob;
    int B, L, V, P, min_new, tb, max_initial, eos;
};

__device__ __forceinline__ f32x4 sc_ld4(const bf16* p) {
    const bf16x4 t = *(const bf16x4*)p;
    return f32x4{bf2f(t[0]), bf2f(t[1]), bf2f(t[2]), bf2f(t[3])};
}
__device__ __forceinline__ f32x4 sc_ld4(const float* p) { return *(const f32x4*)p; }

template <class T>
__global__ __launch_bounds__(SEL_NT) void score_tokens_kernel(const ScoreP p) {
    __shared__ float redf[SEL_NT / 64];
    __shared__ int redi[SEL_NT / 64];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int V = p.V, eos = p.eos;
    const int64_t* row_tok = p.tokens + (long)b * p.tok_ld;
    const int n = p.P + j;                          // position of the token this step chose
    const T* row = (const T*)p.logits + ((long)b * p.batch_rows + j) * p.ld;
    const int first = j == 0;
    const RowRules rr = row_rules(row_tok, n, p.P, p.tb, p.max_initial, V, eos, j < p.min_new, redi);
    const bool ts_mode = rr.ts_mode;
    const int tsb = rr.tsb;
    const uint8_t* suppress = p.suppress;
    const uint8_t* begin_suppress = first ? p.begin_suppress : nullptr;      // (so that word_masks asks nothing of an unused mask)
    const bool word_masks = (((uintptr_t)suppress | (uintptr_t)begin_suppress) & 3) == 0;
    // bit e of the result: column c0 + e is allowed (c0 a multiple of 4; columns at or behind V are not).  The condition is
    // column_allowed of select_rules.h, written out: called as a function, its chain is turned into selects before it reaches this
    // kernel, which then has 6 % more instructions and runs 1.4-3.7 % slower (profiles/select_rules_refactor.md).
    auto ok4 = [&](int c0) -> unsigned {
        const unsigned mask = rule_masks_of(suppress, begin_suppress, first, word_masks, c0, V);
        unsigned ok = 0;
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c0 + e;
            const bool a = c < V && !((mask >> (8 * e)) & 0xffu) && ((c >= rr.tlo && c < rr.thi) || (c >= rr.slo && c < rr.shi)) &&
                           c != rr.ban_eos && c != rr.ban_nots;
            ok |= (a ? 1u : 0u) << e;
        }
        return ok;
    };
    auto allowed = [&](int c) -> bool { return (ok4(c & ~3) >> (c & 3)) & 1u; };       // one column (0 <= c < V)
    const float NEG = -INFINITY;
    float* out = p.scores ? p.scores + ((long)j * p.B + b) * p.ld_scores : nullptr;
    const int width = p.scores ? (int)p.ld_scores : V;          // columns to cover (validated: ld_scores < 2^31)
    const int clast = (V - 1) & ~3;                  // last chunk that holds a logit (loads are clamped to it: ld >= V, ld % 4 == 0)
    float tmax = NEG, smax = NEG;                    // best allowed text logit / best allowed timestamp logit
    bool mask_text = false;
    float M, sum = 0.f;
    if (width <= SC_NPRE * SEL_NT * 4) {
        // ---- the row in registers: everything is requested before anything is judged ----
        // (chunk i starts at column i * 4096: a chunk wholly behind V is not loaded -- uniform over the workgroup; it holds
        // zeros that no allowed bit ever selects)
        f32x4 xr[SC_NPRE];
        unsigned long long okb = 0;                  // 4 bits per chunk
#pragma unroll
        for (int i = 0; i < SC_NPRE; ++i)
            xr[i] = i * SEL_NT * 4 < V ? sc_ld4(row + min(tid * 4 + i * SEL_NT * 4, clast)) : f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < SC_NPRE; ++i) {
            const int c0 = tid * 4 + i * SEL_NT * 4;
            const unsigned ok = c0 < V ? ok4(c0) : 0u;
            okb |= (unsigned long long)ok << (4 * i);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((ok >> e) & 1u) {
                    if (c0 + e < tsb) tmax = fmaxf(tmax, xr[i][e]); else smax = fmaxf(smax, xr[i][e]);
                }
        }
        tmax = block_max<SEL_NT>(tmax, redf);
        smax = block_max<SEL_NT>(smax, redf);
        if (ts_mode && smax > NEG) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < SC_NPRE; ++i) {
                const int c0 = tid * 4 + i * SEL_NT * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (((okb >> (4 * i + e)) & 1ull) && c0 + e >= tsb) s += __expf(xr[i][e] - smax);
            }
            s = block_sum<SEL_NT>(s, redf);
            mask_text = smax + __logf(s) > tmax;
        }
        M = mask_text ? smax : fmaxf(tmax, smax);
#pragma unroll
        for (int i = 0; i < SC_NPRE; ++i) {
            const int c0 = tid * 4 + i * SEL_NT * 4;
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool a = ((okb >> (4 * i + e)) & 1ull) && !(mask_text && c0 + e < tsb);
                y[e] = a ? xr[i][e] : NEG;
                if (a) sum += __expf(xr[i][e] - M);
            }
            if (out && c0 < width) *(f32x4*)(out + c0) = y;
        }
    } else {
        // ---- vocabularies beyond the register budget: the same three passes as loops over the row (L2 resident) ----
        for (int c0 = tid * 4; c0 < V; c0 += SEL_NT * 4) {
            const f32x4 x = sc_ld4(row + c0);
            const unsigned ok = ok4(c0);
#pragma unroll
            for (int e = 0; e < 4; ++e)
                if ((ok >> e) & 1u) {
                    if (c0 + e < tsb) tmax = fmaxf(tmax, x[e]); else smax = fmaxf(smax, x[e]);
                }
        }
        tmax = block_max<SEL_NT>(tmax, redf);
        smax = block_max<SEL_NT>(smax, redf);
        if (ts_mode && smax > NEG) {
            float s = 0.f;
            for (int c0 = (tsb & ~3) + tid * 4; c0 < V; c0 += SEL_NT * 4) {
                const f32x4 x = sc_ld4(row + c0);
                const unsigned ok = ok4(c0);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (((ok >> e) & 1u) && c0 + e >= tsb) s += __expf(x[e] - smax);
            }
            s = block_sum<SEL_NT>(s, redf);
            mask_text = smax + __logf(s) > tmax;
        }
        M = mask_text ? smax : fmaxf(tmax, smax);
        for (int c0 = tid * 4; c0 < width; c0 += SEL_NT * 4) {
            const f32x4 x = sc_ld4(row + min(c0, clast));
            const unsigned ok = c0 < V ? ok4(c0) : 0u;
            f32x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool a = ((ok >> e) & 1u) && !(mask_text && c0 + e < tsb);
                y[e] = a ? x[e] : NEG;
                if (a) sum += __expf(x[e] - M);
            }
            if (out) *(f32x4*)(out + c0) = y;
        }
    }
    if (!p.chosen && !p.logprob) return;             // (uniform)
    sum = block_sum<SEL_NT>(sum, redf);
    if (tid == 0) {
        const long tok = row_tok[n];
        float sc = NEG, lp = NEG;
        if (tok >= 0 && tok < V && allowed((int)tok) && !(mask_text && tok < tsb)) {
            sc = (float)row[tok];
            lp = sc - (M + logf(sum));               // (an allowed column exists: M is finite and sum >= 1)
        }
        if (p.chosen) p.chosen[(long)b * p.L + j] = sc;
        if (p.logprob) p.logprob[(long)b * p.L + j] = lp;
    }
}

extern "C" int dw_score_tokens(const void* logits, int dtype, int B, int L, int V, int64_t ld, int64_t batch_rows,
                               const int64_t* tokens, int64_t tok_ld, int begin_index, const uint8_t* suppress,
                               const uint8_t* begin_suppress, int min_new, int ts_begin, int max_initial, int eos,
                               float* scores, int64_t ld_scores, float* chosen, float* logprob, void* stream) {
    DW_CLEAR_ERR();
    if (!logits || !tokens || (!scores && !chosen && !logprob)) return DW_EINVAL;
    if (dtype != DW_F32 && dtype != DW_BF16) return DW_EINVAL;
    if (B <= 0 || B > 65535 || L <= 0 || V <= 0 || ld < V || (ld & 3) || batch_rows < L) return DW_EINVAL;
    if ((uintptr_t)logits & (dtype == DW_F32 ? 15 : 7)) return DW_EINVAL;
    if (begin_index < 0 || tok_ld < (int64_t)begin_index + L || min_new < 0 || eos >= V) return DW_EINVAL;
    if (ts_begin >= 0 && (eos < 0 || begin_index < 1 || ts_begin < 1 || ts_begin > V)) return DW_EINVAL;
    if (scores && (ld_scores < V || (ld_scores & 3) || ld_scores > 0x7ffffff0 || ((uintptr_t)scores & 15))) return DW_EINVAL;
    ScoreP p;
    p.logits = logits; p.ld = (long)ld; p.batch_rows = (long)batch_rows;
    p.tokens = tokens; p.tok_ld = (long)tok_ld;
    p.suppress = suppress; p.begin_suppress = begin_suppress;
    p.scores = scores; p.ld_scores = (long)ld_scores; p.chosen = chosen; p.logprob = logprob;
    p.B = B; p.L = L; p.V = V; p.P = begin_index; p.min_new = min_new; p.tb = ts_begin; p.max_initial = max_initial; p.eos = eos;
    const dim3 grid(L, B), block(SEL_NT);
    if (dtype == DW_F32) hipLaunchKernelGGL(score_tokens_kernel<float>, grid, block, 0, (hipStream_t)stream, p);
    else hipLaunchKernelGGL(score_tokens_kernel<bf16>, grid, block, 0, (hipStream_t)stream, p);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
