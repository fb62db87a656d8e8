// Token selection of batched greedy decoding: the reference's logits processors + argmax + EOS bookkeeping for one
// decoding step of a whole batch in ONE launch (what GenerationMixin._sample does in a dozen small torch kernels).
//
// Reference behaviour (third-party `transformers`, TF: = transformers/generation/):
//   MinNewTokensLengthLogitsProcessor, SuppressTokensAtBeginLogitsProcessor, SuppressTokensLogitsProcessor and
//   WhisperTimeStampLogitsProcessor (TF:logits_process.py; installed in that order by
//   TF:models/whisper/generation_whisper.py:1774-1812), then `argmax` and
//   `next = next * unfinished + pad * (1 - unfinished)` (TF:utils.py `_sample`), as reached from
//   run_distillation.py:1524-1528, run_eval.py:690-739 and run_pseudo_labelling.py:861-996.
// Every rule is a predicate on (column, row history), so nothing is materialised: one pass over the row of bf16 logits
// keeps the best allowed text token and the best allowed timestamp token, a second pass (timestamp mode only) sums the
// timestamp probability mass for the "timestamps together beat the best text token" rule.
// HBM-bound: B x V x 2 bytes read once (twice in timestamp mode; the row is L2 resident).  One 1024-thread workgroup
// per row; being a plain kernel on the launch stream it is captured into the per-position HIP graphs like the rest of
// the step (the torch implementation of the timestamp rules was not graph-safe).
// Sampling (dw_sample_select, further down) is the same launch with the warpers and the multinomial draw behind the rules:
// TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper (TF:logits_process.py, in TF:utils.py `_get_logits_processor`'s
// order), `softmax` + `torch.multinomial` of TF:utils.py `_sample`, as reached from run_eval.py:690-739 (temperature fallback).
#include "common.h"
#include "select_rules.h"                           // SEL_NT, Best / block_best, every logits rule and the greedy walk
#include "../../include/dwamd.h"

// dw_debug_set key 7 (A/B): bit 0 LayerNorm-on-load off, bit 1 K/V append fusion off, bit 2 / bit 3: the self- / cross-attention of
// the token step as separate projection + attention launches.  Default 4: measured at batch 16 (profiles/r5_decode_fusions.md) the
// cross-attention with its q projection inside saves 7.5 us per token step (2 launches fewer; 38.3 us against 13.6 + 30.8), the
// self-attention with its q / k / v projection inside LOSES 8.6 us -- its 320 workgroups each pull the head's 491 KB of weights
// through L2 (157 MB against the GEMV's 9.8 MB from HBM) for a 5 us attention.
int g_decode_fuse_off = 4;

#define NEG_BIG_D (-1.0e30f)

// HIST (dw_greedy_select_history): the two history-dependent default processors of GenerationMixin, which the reference runs in
// front of Whisper's own (TF `_get_logits_processor`): RepetitionPenaltyLogitsProcessor -- a column whose id occurs in
// tokens[b, 0:n] (decoder prompt included) takes v < 0 ? v * p : v / p, once however often it occurs -- and
// NoRepeatNGramLogitsProcessor -- a column that would complete an n-gram the row already holds is excluded.  Both are
// predicates on (column, row history) like the rest: the workgroup turns the <= 448 history tokens into two bitmaps in LDS
// (one bit per column: `seen`, `banned`, select_rules.h); a four-column chunk whose bits are all clear keeps the short path of
// the walk (greedy_pick, select_rules.h), which both instances share with assist_pick_kernel (assist.hip).
template <bool HIST>
__global__ __launch_bounds__(SEL_NT) void greedy_select_kernel(
    const bf16* logits, int V, long ld, const uint8_t* suppress, const uint8_t* begin_suppress, int first, int no_eos,
    int forced, int tb, int max_initial, int64_t* tokens, long tok_ld, int n, int begin_index, int eos, int fill,
    uint8_t* done, int64_t* cur, float rep_pen, int ngram) {
    __shared__ Best red[SEL_NT / 64];
    __shared__ float redf[SEL_NT / 64];
    __shared__ int redi[SEL_NT / 64];
    __shared__ unsigned seen[HIST ? SEL_HIST_V / 32 : 1], banned[HIST ? SEL_HIST_V / 32 : 1];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t* row_tok = tokens + (long)b * tok_ld;
    if (forced) {                                  // position n still belongs to the forced prefix (teacher forcing)
        if (tid == 0) cur[b] = row_tok[n];
        return;
    }
    const bf16* row = logits + (long)b * ld;
    if constexpr (HIST) build_history_bitmaps(row_tok, n, V, rep_pen, ngram, seen, banned);
    const RowRules rr = row_rules(row_tok, n, begin_index, tb, max_initial, V, eos, no_eos, redi);
    const Best pick = greedy_pick<HIST>(row, V, suppress, begin_suppress, first, rr, seen, banned, rep_pen, red, redf);
    if (tid == 0) {
        long nxt = pick.i == 0x7fffffff ? 0 : pick.i;
        if (eos >= 0) {
            if (done[b]) nxt = fill;
            if (nxt == eos) done[b] = 1;
        }
        row_tok[n] = nxt;
        cur[b] = nxt;
    }
}

extern "C" int dw_greedy_select(const void* logits, int B, int V, int64_t ld, const uint8_t* suppress,
                                const uint8_t* begin_suppress, int first, int no_eos, int forced, int ts_begin,
                                int max_initial, int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos,
                                int fill, uint8_t* done, int64_t* cur, void* stream) {
    DW_CLEAR_ERR();
    if (!tokens || !cur || B <= 0 || n < 1 || n >= tok_ld) return DW_EINVAL;
    if (!forced && (!select_args_ok(logits, V, ld, n, ts_begin, begin_index, eos) || (eos >= 0 && !done))) return DW_EINVAL;
    hipLaunchKernelGGL(greedy_select_kernel<false>, dim3(B), dim3(SEL_NT), 0, (hipStream_t)stream, (const bf16*)logits, V,
                       (long)ld, suppress, begin_suppress, first, no_eos, forced, ts_begin, max_initial, tokens,
                       (long)tok_ld, n, begin_index, eos, fill, done, cur, 1.0f, 0);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

extern "C" int dw_greedy_select_history(const void* logits, int B, int V, int64_t ld, const uint8_t* suppress,
                                        const uint8_t* begin_suppress, int first, int no_eos, int forced, int ts_begin,
                                        int max_initial, int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos,
                                        int fill, uint8_t* done, int64_t* cur, float repetition_penalty, int no_repeat_ngram,
                                        void* stream) {
    DW_CLEAR_ERR();
    if (!tokens || !cur || B <= 0 || n < 1 || n >= tok_ld) return DW_EINVAL;
    if (!(repetition_penalty > 0.f) || !(repetition_penalty <= 3.402823466e38f) || no_repeat_ngram < 0) return DW_EINVAL;
    if (!forced && (!select_args_ok(logits, V, ld, n, ts_begin, begin_index, eos) || V > SEL_HIST_V || (eos >= 0 && !done))) return DW_EINVAL;
    hipLaunchKernelGGL(greedy_select_kernel<true>, dim3(B), dim3(SEL_NT), 0, (hipStream_t)stream, (const bf16*)logits, V,
                       (long)ld, suppress, begin_suppress, first, no_eos, forced, ts_begin, max_initial, tokens,
                       (long)tok_ld, n, begin_index, eos, fill, done, cur, repetition_penalty, no_repeat_ngram);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// dw_greedy_select_bias: greedy_select_kernel<true> with GenerationMixin's SequenceBiasLogitsProcessor and
// NoBadWordsLogitsProcessor (`generate(sequence_bias=, bad_words_ids=)`: hot-word boosts and forbidden words) in the same single
// launch.  In the reference's list the first stands in front of the repetition penalty and the second behind the n-gram rule; a
// bad word is a bias of -inf, which no later processor brings back, so both are one table (select_rules.h BiasTable) applied in
// front: thread s tests sequence s against the tail of the row's history, the first entry of a column adds that column's
// biases up in table order, a -inf sum joins the `banned` bitmap and any other non-zero sum sets the column in a third bitmap,
// `biased`, which the walk reads like `seen`: a chunk with a bit set is judged column by column as penal?(x + bias), in the
// mass-rule pass as well.  Nothing is allocated, no other workgroup is waited for, the table is read-only device memory: the
// step is captured into the per-position graphs like the others.
// LDS: three bitmaps of 8 KB, the table's columns and sums 4 KB each, 256 B of reduction scratch: 33 024 B per workgroup.
__global__ __launch_bounds__(SEL_NT) void greedy_select_bias_kernel(
    const bf16* logits, int V, long ld, const uint8_t* suppress, const uint8_t* begin_suppress, int first, int no_eos,
    int forced, int tb, int max_initial, int64_t* tokens, long tok_ld, int n, int begin_index, int eos, int fill,
    uint8_t* done, int64_t* cur, float rep_pen, int ngram, const BiasTable table) {
    __shared__ Best red[SEL_NT / 64];
    __shared__ float redf[SEL_NT / 64];
    __shared__ int redi[SEL_NT / 64];
    __shared__ unsigned seen[SEL_HIST_V / 32], banned[SEL_HIST_V / 32], biased[SEL_HIST_V / 32];
    __shared__ int bcol[SEL_BIAS_S];
    __shared__ float bsum[SEL_BIAS_S];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t* row_tok = tokens + (long)b * tok_ld;
    if (forced) {                                  // position n still belongs to the forced prefix (teacher forcing)
        if (tid == 0) cur[b] = row_tok[n];
        return;
    }
    const bf16* row = logits + (long)b * ld;
    build_history_bitmaps(row_tok, n, V, rep_pen, ngram, seen, banned);
    build_bias_bitmaps(row_tok, n, V, table, banned, biased, bcol, bsum);
    const RowRules rr = row_rules(row_tok, n, begin_index, tb, max_initial, V, eos, no_eos, redi);
    const Best pick = greedy_pick<true, true>(row, V, suppress, begin_suppress, first, rr, seen, banned, rep_pen, red, redf, biased,
                                              bcol, bsum, table.S);
    if (tid == 0) {
        long nxt = pick.i == 0x7fffffff ? 0 : pick.i;
        if (eos >= 0) {
            if (done[b]) nxt = fill;
            if (nxt == eos) done[b] = 1;
        }
        row_tok[n] = nxt;
        cur[b] = nxt;
    }
}

extern "C" int dw_greedy_select_bias(const void* logits, int B, int V, int64_t ld, const uint8_t* suppress,
                                     const uint8_t* begin_suppress, int first, int no_eos, int forced, int ts_begin,
                                     int max_initial, int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos,
                                     int fill, uint8_t* done, int64_t* cur, float repetition_penalty, int no_repeat_ngram,
                                     const int* bias_tok, const int* bias_off, const float* bias_val, int S, void* stream) {
    DW_CLEAR_ERR();
    if (!tokens || !cur || B <= 0 || n < 1 || n >= tok_ld) return DW_EINVAL;
    if (!(repetition_penalty > 0.f) || !(repetition_penalty <= 3.402823466e38f) || no_repeat_ngram < 0) return DW_EINVAL;
    if (S < 0 || S > SEL_BIAS_S || (S > 0 && (!bias_tok || !bias_off || !bias_val))) return DW_EINVAL;
    if (!forced && (!select_args_ok(logits, V, ld, n, ts_begin, begin_index, eos) || V > SEL_HIST_V || (eos >= 0 && !done))) return DW_EINVAL;
    const BiasTable table = {bias_tok, bias_off, bias_val, S};
    hipLaunchKernelGGL(greedy_select_bias_kernel, dim3(B), dim3(SEL_NT), 0, (hipStream_t)stream, (const bf16*)logits, V,
                       (long)ld, suppress, begin_suppress, first, no_eos, forced, ts_begin, max_initial, tokens,
                       (long)tok_ld, n, begin_index, eos, fill, done, cur, repetition_penalty, no_repeat_ngram, table);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Sampled selection (dw_sample_select): `generate(do_sample=True, temperature=, top_k=, top_p=)` in the same single launch.
// Reference behaviour: TF:generation/utils.py `_get_logits_processor` (processors, then TemperatureLogitsWarper, TopKLogitsWarper,
// TopPLogitsWarper of TF:generation/logits_process.py, in that order) and `_sample` (`probs = softmax(scores)`,
// `torch.multinomial(probs, 1)`), as reached from run_eval.py:690-739 (`temperature=(0.0, 0.2, ..., 1.0)` fallback passes,
// TF:generation_whisper.py `generate_with_fallback`).
// For one draw per row torch.multinomial IS `argmax(probs / q)` with q = empty_like(probs).exponential_(1): the caller draws q
// (`noise`) with torch's generator, so the token is the reference's; everything else happens here.
//   1. the processed fp32 score of every column as greedy_select_kernel<true> judges it (excluded = -inf), mass rule included;
//   2. s / temperature, correctly rounded like the reference's IEEE division;
//   3. top-k: the k-th largest of all V scores by a radix select, columns with s < kth removed (ties stay);
//   4. top-p: a column is removed iff the probability of all columns with a score <= its own is <= 1 - top_p.  The reference
//      removes a prefix of an ascending sort, so it splits the group of equal scores that straddles the boundary in the order
//      its sort happens to give; this kernel keeps that group whole (a documented deviation);
//   5. the winner is argmax exp(s - max) / noise over the surviving columns, equal quotients to the smaller column (softmax's
//      common factor 1 / sum does not move the argmax);
//   6. EOS bookkeeping as in the greedy kernel.
// The row's scores stay in registers (NCH chunks of four columns per thread: 13 up to 53 248 columns, 16 up to 65 536).
// Both thresholds come from ONE search, `select_key`: the smallest 32-bit key K whose cumulative weight W(<= K) exceeds T, found
// eight bits at a time over a 256-bin LDS histogram of 64-bit integers.  Top-k: key = ~order(s), weight 1, T = k - 1.  Top-p: key
// = order(s), weight = exp(s - max) in 2^-32 fixed point, T = floor((1 - top_p) * Z).  Integer sums do not depend on the order
// of the adds, so no threshold depends on the arrival order of an atomic and equal inputs give equal tokens.  (Fixed point,
// rounded to nearest: 65 536 roundings of at most 2^-33 each sum to less than 8e-6 of the largest column's weight even if all
// fell the same way, and to ~2e-8 as the random walk they are; the fast exponential's own error is of the order 1e-7 relative.)
// LDS adds to one bin serialise, and the first digit of fp32 scores fills a handful of bins, so the searches first narrow the
// candidates with the per-thread extrema: the k-th largest of the 1024 thread maxima is a lower bound of the k-th largest score
// (k <= 1024); for top-p the 256-th largest thread maximum L is used when the mass below L fits into the budget (a peaked
// distribution, the usual case).  Otherwise every finite column is a candidate: correct, slower.
// ---------------------------------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned order_key(float v) {         // unsigned order == float order; -0 counts as +0
    const unsigned u = __float_as_uint(v + 0.0f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float key_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}
#define KEY_NEG_INF 0x007fffffu                                  // order_key(-inf): every finite score has a larger key

typedef unsigned long long u64;
struct SelScratch { u64 hist[256]; u64 wtot[4]; u64 base; unsigned digit; u64 red[SEL_NT / 64]; };

__device__ __forceinline__ u64 block_sum_u64(u64 x, u64* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) x += __shfl_xor(x, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = x;
    __syncthreads();
    u64 t = 0;
    for (int i = 0; i < SEL_NT / 64; ++i) t += red[i];
    return t;
}

// The smallest key K among the thread block's items with base + W(items <= K) > T.  `each(f)` calls f(key, weight) for every item
// of the calling thread; the caller guarantees base <= T < base + W(all items).
template <class Each>
__device__ __forceinline__ unsigned select_key(Each&& each, u64 base, u64 T, SelScratch* sc) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned prefix = 0;
#pragma unroll 1
    for (int shift = 24; shift >= 0; shift -= 8) {
        const unsigned pmask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        __syncthreads();
        if (tid < 256) sc->hist[tid] = 0;
        __syncthreads();
        each([&](unsigned key, u64 w) {
            if ((key & pmask) == prefix) atomicAdd(&sc->hist[(key >> shift) & 255u], w);
        });
        __syncthreads();
        u64 own = 0, incl = 0;
        if (tid < 256) {                           // inclusive scan of the 256 bins: within a wave, then across the four waves
            own = incl = sc->hist[tid];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const u64 y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            if (lane == 63) sc->wtot[tid >> 6] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < (tid >> 6); ++w) incl += sc->wtot[w];
            const u64 before = base + incl - own;
            if (before <= T && before + own > T) { sc->digit = (unsigned)tid; sc->base = before; }   // exactly one bin
        }
        __syncthreads();
        prefix |= sc->digit << shift;
        base = sc->base;
    }
    return prefix;
}

template <int NCH>
__global__ __launch_bounds__(SEL_NT) void sample_select_kernel(
    const bf16* logits, int V, long ld, const uint8_t* suppress, const uint8_t* begin_suppress, int first, int no_eos,
    int tb, int max_initial, int64_t* tokens, long tok_ld, int n, int begin_index, int eos, int fill,
    uint8_t* done, int64_t* cur, float rep_pen, int ngram, float temperature, int top_k, float top_p, const float* noise,
    long noise_ld) {
    __shared__ Best red[SEL_NT / 64];
    __shared__ float redf[SEL_NT / 64];
    __shared__ int redi[SEL_NT / 64];
    __shared__ unsigned seen[SEL_HIST_V / 32], banned[SEL_HIST_V / 32];
    __shared__ SelScratch sc;
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t* row_tok = tokens + (long)b * tok_ld;
    if (eos >= 0 && done[b]) {                     // a finished row takes `fill` whatever its logits say
        if (tid == 0) { row_tok[n] = fill; cur[b] = fill; if (fill == eos) done[b] = 1; }
        return;
    }
    const bf16* row = logits + (long)b * ld;
    // ---- history bitmaps and the row state of the rules (select_rules.h), as in greedy_select_kernel<true> ----
    build_history_bitmaps(row_tok, n, V, rep_pen, ngram, seen, banned);
    auto penal = [&](float v) -> float { return v < 0.f ? v * rep_pen : v / rep_pen; };
    const RowRules rr = row_rules(row_tok, n, begin_index, tb, max_initial, V, eos, no_eos, redi);
    const bool ts_mode = rr.ts_mode;
    const int tsb = rr.tsb;
    // ---- 1. processed scores into registers: slot 4 i + e holds column tid * 4 + i * 4096 + e (-inf: excluded or beyond V) ----
    const bool word_masks = (((uintptr_t)suppress | (uintptr_t)begin_suppress) & 3) == 0;
    auto masks_of = [&](int c0) -> unsigned { return rule_masks_of(suppress, begin_suppress, first, word_masks, c0, V); };
    float s[NCH * 4];
    float btv = -INFINITY, bsv = -INFINITY;            // best allowed text / timestamp score (mass rule)
    {
        const int clast = (V - 1) & ~3;
        bf16x4 xr[NCH];
        unsigned mr[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c0 = min(tid * 4 + i * SEL_NT * 4, clast);
            xr[i] = *(const bf16x4*)(row + c0);
            mr[i] = masks_of(c0);
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c0 = tid * 4 + i * SEL_NT * 4;
            const bool live = c0 < V;
            const unsigned mask = mr[i];
            unsigned sbits = 0, bbits = 0;
            if (live) { sbits = history_bits_of(seen, c0); bbits = history_bits_of(banned, c0); }
            const ChunkKind kind = classify_chunk(rr, mask, live, c0, V, sbits, bbits);
            if (kind.clean) {                          // the whole chunk inside one allowed interval, nothing masked or penalised
                float m = -INFINITY;
#pragma unroll
                for (int e = 0; e < 4; ++e) { s[4 * i + e] = bf2f(xr[i][e]); m = fmaxf(m, s[4 * i + e]); }
                if (kind.in_text) btv = fmaxf(btv, m); else bsv = fmaxf(bsv, m);
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int c = c0 + e;
                    const bool ok = column_allowed(rr, c0, e, V, mask, bbits, live);
                    float v = bf2f(xr[i][e]);
                    if ((sbits >> e) & 1u) v = penal(v);
                    v = ok ? v : -INFINITY;
                    s[4 * i + e] = v;
                    if (c < tsb) btv = fmaxf(btv, v); else bsv = fmaxf(bsv, v);
                }
            }
        }
    }
    // slot j holds column tid4 + off(j); a compare of that column with a uniform bound is written tid4 < bound - off(j), so that
    // no loop keeps 52 column numbers in registers
    const int tid4 = tid * 4;
    auto off = [](int j) -> int { return (j >> 2) * (SEL_NT * 4) + (j & 3); };
    // (a loop that compares its columns with a uniform bound takes its own copy of the bound through an empty asm: shared, or
    // hoisted out of the passes of a search, the 52 compare results would stay live in scalar registers and spill)
    auto fresh = [](auto x) { asm volatile("" : "+v"(x)); return x; };
    btv = block_max<SEL_NT>(btv, redf);
    bsv = block_max<SEL_NT>(bsv, redf);
    // the timestamp mass rule, as the greedy kernel decides it
    bool text_out = false;
    if (ts_mode && bsv > -INFINITY) {
        float sum = 0.f;
        const int t0 = fresh(tsb);
#pragma unroll
        for (int j = 0; j < NCH * 4; ++j)
            if (tid4 >= t0 - off(j) && s[j] > -INFINITY) sum += __expf(s[j] - bsv);
        sum = wave_sum(sum);
        __syncthreads();
        if ((tid & 63) == 0) redf[tid >> 6] = sum;
        __syncthreads();
        sum = 0.f;
        for (int i = 0; i < SEL_NT / 64; ++i) sum += redf[i];
        text_out = bsv + __logf(sum) > btv;
    }
    // ---- 2. temperature: s / temperature correctly rounded, as one double product per column.  (The product of s and the
    // double reciprocal is within 2^-52 of the quotient, and a quotient of two floats keeps 2^-50 from every rounding boundary
    // of fp32.)  From here on a score lives as its order key: integer compares, -0 and +0 share a key. ----
    const double rtemp = 1.0 / (double)temperature;
    const float smax = (float)((double)(text_out ? bsv : fmaxf(btv, bsv)) * rtemp);     // (rounding is monotone: the row's maximum)
    unsigned ky[NCH * 4];
    {
        const int t0 = text_out ? fresh(tsb) : 0;                                       // text columns: below t0
#pragma unroll
        for (int j = 0; j < NCH * 4; ++j) {
            ky[j] = tid4 < t0 - off(j) ? KEY_NEG_INF : order_key((float)((double)s[j] * rtemp));
            if ((j & 7) == 7) __builtin_amdgcn_sched_barrier(0);
        }
    }
    Best pick = {-INFINITY, 0x7fffffff};
    if (smax > -INFINITY) {                        // (uniform: a row with no allowed column yields 0)
        // the m-th largest of the per-thread maxima, or 0 when fewer than m threads hold a finite score
        auto mth_thread_max = [&](int m) -> unsigned {
            unsigned mk = 0;
#pragma unroll
            for (int j = 0; j < NCH * 4; ++j) mk = max(mk, ky[j]);
            const bool fin = mk > KEY_NEG_INF;
            if (m > SEL_NT || (int)block_sum_u64(fin ? 1 : 0, sc.red) < m) return 0u;
            return ~select_key([&](auto&& f) { if (fin) f(~mk, (u64)1); }, 0, (u64)(m - 1), &sc);
        };
        // ---- 3. top-k: the k-th largest score = the k-th smallest of the inverted keys ----
        if (top_k > 0) {
            const int k = min(top_k, V);
            int nfin = 0;
#pragma unroll
            for (int j = 0; j < NCH * 4; ++j) nfin += ky[j] > KEY_NEG_INF;
            if ((int)block_sum_u64((u64)nfin, sc.red) >= k) {       // (fewer than k finite scores: the k-th is -inf, nothing goes)
                unsigned lo = mth_thread_max(k);                       // candidates: finite scores with a key >= lo
                if (!lo) lo = KEY_NEG_INF + 1u;
                const unsigned kth = ~select_key([&](auto&& f) {
                    const unsigned l = fresh(lo), ones = fresh(0xffffffffu);
#pragma unroll
                    for (int j = 0; j < NCH * 4; ++j)
                        if (ky[j] >= l) f(ky[j] ^ ones, (u64)1);
                }, 0, (u64)(k - 1), &sc);
#pragma unroll
                for (int j = 0; j < NCH * 4; ++j) ky[j] = ky[j] < kth ? KEY_NEG_INF : ky[j];
            }
        }
        // ---- 4. top-p ----
        if (top_p < 1.0f) {
            // exp(s - max) in 2^-32 fixed point, rounded to nearest (-inf: 0; the maximum: 2^32 - 256, the largest float below
            // 2^32).  `zero` is a 0 the compiler cannot see through (`fresh`): every pass recomputes the weights, which hoisted
            // out of the passes would be 104 registers.
            auto weight = [&](unsigned key, float mx, unsigned zero) -> u64 {
                return (u64)(unsigned)__fmaf_rn(__expf(key_value(key ^ zero) - mx), 4294967040.0f, 0.5f);
            };
            unsigned lo = mth_thread_max(256);
            if (!lo) lo = KEY_NEG_INF + 1u;
            u64 Z, below;
            {
                const float mx = fresh(smax);
                const unsigned l = fresh(lo), zero = fresh(0u);
                u64 zt = 0, bl = 0;
#pragma unroll
                for (int j = 0; j < NCH * 4; ++j) {
                    const u64 w = weight(ky[j], mx, zero);
                    zt += w;
                    bl += ky[j] < l ? w : (u64)0;
                }
                Z = block_sum_u64(zt, sc.red);      // >= 2^32 - 256: the maximum weighs exp(0)
                below = block_sum_u64(bl, sc.red);
            }
            u64 R = (u64)((1.0 - (double)top_p) * (double)Z);
            R = R < Z - 1 ? R : Z - 1;              // (top_p > 0: the largest column always stays)
            if (below > R) { lo = KEY_NEG_INF + 1u; below = 0; }       // a flat distribution: every finite column is a candidate
            const unsigned cut = select_key([&](auto&& f) {           // the smallest score that stays
                const float mx = fresh(smax);
                const unsigned l = fresh(lo), zero = fresh(0u);
#pragma unroll
                for (int j = 0; j < NCH * 4; ++j)
                    if (ky[j] >= l) f(ky[j], weight(ky[j], mx, zero));
            }, below, R, &sc);
#pragma unroll
            for (int j = 0; j < NCH * 4; ++j) ky[j] = ky[j] < cut ? KEY_NEG_INF : ky[j];
        }
        // ---- 5. the draw: argmax exp(s - max) / noise.  (The reference divides softmax(s) by the noise; the common factor
        // 1 / sum does not move the argmax and is left out.)  The noise arrives in groups of four chunks, the next group
        // requested before this one is used; addresses are clamped instead of branched around. ----
        const float* nrow = noise + (long)b * noise_ld;
        const unsigned zero = fresh(0u);
        constexpr int G = 4, NG = (NCH + G - 1) / G;
        float q[2][G * 4];
        auto request = [&](int g, float* qb) {
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (g * G + u >= NCH) break;
                const int c0 = tid * 4 + (g * G + u) * SEL_NT * 4;
#pragma unroll
                for (int e = 0; e < 4; ++e) qb[4 * u + e] = nrow[min(c0 + e, V - 1)];
            }
        };
        request(0, q[0]);
#pragma unroll
        for (int g = 0; g < NG; ++g) {
            if (g + 1 < NG) request(g + 1, q[(g + 1) & 1]);
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int u = 0; u < G; ++u) {
                if (g * G + u >= NCH) break;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned key = ky[4 * (g * G + u) + e];
                    const float r = __fdividef(__expf(key_value(key ^ zero) - smax), q[g & 1][4 * u + e]);
                    if (key > KEY_NEG_INF && r > pick.v) { pick.v = r; pick.i = 4 * (g * G + u) + e; }   // (ascending: the first of equals)
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        if (pick.i != 0x7fffffff) pick.i = tid4 + off(pick.i);          // slot -> column
    }
    pick = block_best(pick, red);
    if (tid == 0) {
        long nxt = pick.i == 0x7fffffff ? 0 : pick.i;
        if (eos >= 0 && nxt == eos) done[b] = 1;
        row_tok[n] = nxt;
        cur[b] = nxt;
    }
}

extern "C" int dw_sample_select(const void* logits, int B, int V, int64_t ld, const uint8_t* suppress,
                                const uint8_t* begin_suppress, int first, int no_eos, int ts_begin, int max_initial,
                                int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos, int fill, uint8_t* done,
                                int64_t* cur, float repetition_penalty, int no_repeat_ngram, float temperature, int top_k,
                                float top_p, const float* noise, int64_t noise_ld, void* stream) {
    DW_CLEAR_ERR();
    if (!tokens || !cur || B <= 0 || n < 1 || n >= tok_ld) return DW_EINVAL;
    if (!(repetition_penalty > 0.f) || !(repetition_penalty <= 3.402823466e38f) || no_repeat_ngram < 0) return DW_EINVAL;
    if (!select_args_ok(logits, V, ld, n, ts_begin, begin_index, eos) || V > SEL_HIST_V || (eos >= 0 && !done)) return DW_EINVAL;
    if (!(temperature > 0.f) || !(temperature <= 3.402823466e38f) || top_k < 0 || !(top_p > 0.f) || !(top_p <= 1.f))
        return DW_EINVAL;
    if (!noise || noise_ld < V || ((uintptr_t)noise & 3)) return DW_EINVAL;
    auto kern = V <= 13 * SEL_NT * 4 ? sample_select_kernel<13> : sample_select_kernel<16>;
    hipLaunchKernelGGL(kern, dim3(B), dim3(SEL_NT), 0, (hipStream_t)stream, (const bf16*)logits, V, (long)ld, suppress,
                       begin_suppress, first, no_eos, ts_begin, max_initial, tokens, (long)tok_ld, n, begin_index, eos, fill,
                       done, cur, repetition_penalty, no_repeat_ngram, temperature, top_k, top_p, noise, (long)noise_ld);
    DW_CHECK_LAUNCH();
    return DW_OK;
}


// ---------------------------------------------------------------------------------------------------------------------
// Token step: attention with its projection inside (round 5).  One workgroup of 16 waves per (sequence, head), as in
// attn_decode_kernel (attention.hip); in front of the two passes over the keys the workgroup computes what the projection
// GEMV in front of the attention used to deliver for its head:
//   MODE 0 (cross-attention):  q_h = bf16(Wq[h] . bf16(LayerNorm(x_b)) + bq[h])                       (64 x D of weights)
//   MODE 1 (self-attention):   q_h, k_h, v_h from the fused QKV weight; k_h / v_h are appended to the cache row t of the
//                              sequence and enter the softmax from LDS (the row is not read back from memory)
// The weight rows of a head are shared by the `batch` workgroups of that head through L2; all 10 x 16-byte weight loads of a
// lane are requested at kernel entry and land while the row statistics are reduced.  What it removes is a dependent launch
// per attention (a kernel boundary costs ~5 us in the 20-launch token step, profiles/r4_decode_gap_histogram.md) and the
// q / k / v round trip through memory.  The passes over the keys request four key groups per lane before the first is used
// (64 KiB in flight per workgroup instead of 16: the single-load loop was a chain of HBM round trips).
// Same arithmetic as the separate launches: two-pass LayerNorm statistics, bf16 operands, fp32 sums (in another order than the
// MFMA GEMV's -- a q element may differ by one bf16 ulp), P rounded to bf16 in front of the PV product.
// ---------------------------------------------------------------------------------------------------------------------
// a row's position from the device array of the per-row passes (further down), clamped to the host's bound [0, max_t]
__device__ __forceinline__ int row_pos(const int32_t* row_t, long b, int max_t) { return min(max(row_t[b], 0), max_t); }
struct DecAttnP {
    const void* x; long ldx;                   // residual stream [B][D] (f32 or bf16)
    const float* ln_g; const float* ln_b; float eps;
    const bf16* w; const float* bias;          // MODE 0: Wq [D][D], bq [D];  MODE 1: Wqkv [3D][D], bqkv [3D]
    const bf16* k; const bf16* v;              // keys / values of batch 0, head 0 (row pitch ldkv, batch pitch kv_rows rows)
    long ldkv, kv_rows;
    bf16* kv_app;                              // MODE 1: the cache (K | V per row) -- row t of every sequence is written
    bf16* o; long ldo;
    int D, Lk, t;                              // Lk counts the new key in MODE 1 (= t + 1)
    float scale;
    const int32_t* row_t; int max_t;           // ROWS (MODE 1): sequence b stands at row_t[b] <= max_t; Lk = max_t + 1 places the LDS regions
};
template <bool XBF>
__device__ __forceinline__ void dec_ld_x8(const void* x, long off, float (&v)[8]) {
    if (XBF) {
        const bf16x8 t = *(const bf16x8*)((const bf16*)x + off);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = bf2f(t[e]);
    } else {
        const f32x4 a = *(const f32x4*)((const float*)x + off);
        const f32x4 b = *(const f32x4*)((const float*)x + off + 4);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3]; v[4] = b[0]; v[5] = b[1]; v[6] = b[2]; v[7] = b[3];
    }
}
constexpr int DEC_NW = 8;                      // waves per workgroup (two workgroups per CU at <= 128 registers)
// ROWS (MODE 1, dw_decode_attn_proj_rows): the sequence's own position from p.row_t in place of the uniform p.t / p.Lk -- the
// workgroup of (b, h) then does what the uniform kernel does at Lk = row_t[b] + 1, sum for sum; p.Lk = max_t + 1 only places the
// scratch regions behind the scores in LDS.
template <int MODE, bool XBF, int NI, bool ROWS = false>   // NI = D / 64: 64-column steps of a weight row (compile time: the fragments live in registers)
__global__ __launch_bounds__(64 * DEC_NW, 4) void attn_decode_proj_kernel(const DecAttnP p) {
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    // [Lk scores (x4) | NW x 64 partial outputs | NW | NW | NW (sums) | 64 q | 64 k_new | 64 v_new | D bf16 normalised row | D f32 row]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, b = blockIdx.z;
    constexpr int D = NI * 64;
    static_assert(!ROWS || MODE == 1, "per-row positions belong to the self-attention");
    const int Lk = ROWS ? __builtin_amdgcn_readfirstlane(row_pos(p.row_t, b, p.max_t)) + 1 : p.Lk;   // keys of this sequence
    const int t_app = ROWS ? Lk - 1 : p.t;
    float* sc = dsm;
    float* part = dsm + ((p.Lk + 3) & ~3);
    float* redm = part + DEC_NW * 64;
    float* redl = redm + DEC_NW;
    float* reds = redl + DEC_NW;
    float* qs = reds + DEC_NW;
    float* knew = qs + 64;
    float* vnew = knew + 64;
    bf16* lnb = (bf16*)(vnew + 64);
    float* xrow = (float*)(lnb + D);
    const float c = p.scale * 1.4426950408889634f;
    // ---- projection ----
    const int j = tid >> 3, l = tid & 7;                  // output j of the head (0..63), 8 lanes share it
    // All of a lane's weight fragments (20 x 16 bytes at D = 1280) are requested at kernel entry and land while the row statistics
    // are reduced.  (With 16 waves and a 64-register budget -- two 1024-thread workgroups per CU -- every split of the fragments
    // spilled, and a spilled fragment is a wait for its load in front of the reductions; eight waves at <= 128 registers keep the
    // same 64 KiB of key / value loads in flight per workgroup.)  The opaque touch of all fragments in dot() makes them live at one
    // point: without it the k / v passes become load -> wait -> use chains (twenty L2 round trips in a row).
    constexpr int NE = NI;
    bf16x8 wf[NI];
    const bf16* const wrow0 = p.w + (long)(h * 64 + j) * D + l * 8;
#pragma unroll
    for (int i = 0; i < NE; ++i) wf[i] = *(const bf16x8*)(wrow0 + i * 64);
    {
        // the row goes through LDS as fp32: nothing of it is held in registers across the two reductions, next to the 80 weight
        // registers of a lane
        if (tid < (D >> 3)) {
            float xv[8];
            dec_ld_x8<XBF>(p.x, (long)b * p.ldx + tid * 8, xv);
            *(f32x4*)(xrow + tid * 8) = f32x4{xv[0], xv[1], xv[2], xv[3]};
            *(f32x4*)(xrow + tid * 8 + 4) = f32x4{xv[4], xv[5], xv[6], xv[7]};
        }
        __syncthreads();
        const bool has = tid < (D >> 2);
        float s1 = 0.f;
        if (has) { const f32x4 a = *(const f32x4*)(xrow + tid * 4); s1 = (a[0] + a[1]) + (a[2] + a[3]); }
        const float mu = block_sum<64 * DEC_NW>(s1, reds) / (float)D;
        float s2 = 0.f;
        if (has) {
            const f32x4 a = *(const f32x4*)(xrow + tid * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float dd = a[e] - mu; s2 += dd * dd; }
        }
        const float rs = rsqrtf(block_sum<64 * DEC_NW>(s2, reds) / (float)D + p.eps);
        f32x4 g4 = {0.f, 0.f, 0.f, 0.f}, b4 = {0.f, 0.f, 0.f, 0.f};
        if (has) {                                        // (requested in front of the late fragments: the counter retires in order)
            g4 = *(const f32x4*)(p.ln_g + tid * 4);
            b4 = *(const f32x4*)(p.ln_b + tid * 4);
        }
        asm volatile("" : "+v"(g4), "+v"(b4));
#pragma unroll
        for (int i = NE; i < NI; ++i) wf[i] = *(const bf16x8*)(wrow0 + i * 64);
        if (has) {
            const f32x4 a = *(const f32x4*)(xrow + tid * 4);
            bf16x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = f2bf((a[e] - mu) * rs * g4[e] + b4[e]);
            *(bf16x4*)(lnb + tid * 4) = y;
        }
        __syncthreads();
    }
    auto dot = [&](bf16x8 (&wf)[NI]) __attribute__((always_inline)) -> float {
#pragma unroll
        for (int i = 0; i < NI; ++i) asm volatile("" : "+v"(wf[i]));
        float acc = 0.f;
#pragma unroll
        for (int i = 0; i < NI; ++i) {
            const bf16x8 a = *(const bf16x8*)(lnb + (i * 8 + l) * 8);
#pragma unroll
            for (int e = 0; e < 8; ++e) acc = fmaf(bf2f(wf[i][e]), bf2f(a[e]), acc);
        }
        acc += __shfl_xor(acc, 1);
        acc += __shfl_xor(acc, 2);
        acc += __shfl_xor(acc, 4);
        return acc;
    };
    {
        const float qa = dot(wf);
        if (l == 0) qs[j] = bf2f(f2bf(qa + p.bias[h * 64 + j])) * c;
    }
    if constexpr (MODE == 1) {
#pragma unroll
        for (int part_i = 1; part_i <= 2; ++part_i) {       // 1: k, 2: v
            const bf16* wrow = p.w + ((long)part_i * D + h * 64 + j) * D + l * 8;
#pragma unroll
            for (int i = 0; i < NI; ++i) wf[i] = *(const bf16x8*)(wrow + i * 64);
            const float a = dot(wf);
            if (l == 0) {
                const bf16 r = f2bf(a + p.bias[part_i * D + h * 64 + j]);
                (part_i == 1 ? knew : vnew)[j] = bf2f(r);
                p.kv_app[((long)b * p.kv_rows + t_app) * p.ldkv + (part_i - 1) * D + h * 64 + j] = r;
            }
        }
    }
    __syncthreads();
    // ---- attention over Lk keys: 8 lanes share a key (16 bytes = 8 head dimensions each) ----
    const int sub = lane >> 3, ds = (lane & 7) * 8;
    const bf16* K = p.k + (long)b * p.kv_rows * p.ldkv + h * 64 + ds;
    const bf16* V = p.v + (long)b * p.kv_rows * p.ldkv + h * 64 + ds;
    float qv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) qv[e] = qs[ds + e];
    const int nold = MODE == 1 ? Lk - 1 : Lk;        // keys that live in memory
    constexpr int UN = 8;                                // key groups requested ahead per lane
    float mx = NEG_BIG_D;
    for (int k0 = wave * 8; k0 < Lk; k0 += UN * DEC_NW * 8) {
        bf16x8 kr[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            int k = k0 + u * DEC_NW * 8 + sub;
            k = k < nold ? k : (nold > 0 ? nold - 1 : 0);
            kr[u] = nold > 0 ? ld_stream<2>((const bf16x8*)(K + (long)k * p.ldkv)) : bf16x8{};
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int k = k0 + u * DEC_NW * 8 + sub;
            float s = 0.f;
            if (MODE == 1 && k == nold) {
#pragma unroll
                for (int e = 0; e < 8; ++e) s = fmaf(qv[e], knew[ds + e], s);
            } else {
#pragma unroll
                for (int e = 0; e < 8; ++e) s = fmaf(qv[e], bf2f(kr[u][e]), s);
            }
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            s += __shfl_xor(s, 4);
            if (k < Lk) {
                if ((lane & 7) == 0) sc[k] = s;
                mx = fmaxf(mx, s);
            }
        }
    }
    mx = wave_max(mx);
    if (lane == 0) redm[wave] = mx;
    __syncthreads();
    mx = redm[0];
#pragma unroll
    for (int i = 1; i < DEC_NW; ++i) mx = fmaxf(mx, redm[i]);
    float o[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float lsum = 0.f;
    for (int k0 = wave * 8; k0 < Lk; k0 += UN * DEC_NW * 8) {
        bf16x8 vr[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            int k = k0 + u * DEC_NW * 8 + sub;
            k = k < nold ? k : (nold > 0 ? nold - 1 : 0);
            vr[u] = nold > 0 ? ld_stream<2>((const bf16x8*)(V + (long)k * p.ldkv)) : bf16x8{};
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int k = k0 + u * DEC_NW * 8 + sub;
            if (k < Lk) {
                const float pv = __builtin_amdgcn_exp2f(sc[k] - mx);
                lsum += pv;
                const float pb = round_bf16(pv);
                if (MODE == 1 && k == nold) {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = fmaf(pb, vnew[ds + e], o[e]);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) o[e] = fmaf(pb, bf2f(vr[u][e]), o[e]);
                }
            }
        }
    }
    lsum = (lane & 7) == 0 ? lsum : 0.f;
    lsum = wave_sum(lsum);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        o[e] += __shfl_xor(o[e], 8);
        o[e] += __shfl_xor(o[e], 16);
        o[e] += __shfl_xor(o[e], 32);
    }
    if (sub == 0) {
#pragma unroll
        for (int e = 0; e < 8; ++e) part[wave * 64 + ds + e] = o[e];
    }
    if (lane == 0) redl[wave] = lsum;
    __syncthreads();
    if (wave == 0) {
        float acc = 0.f, lt = 0.f;
#pragma unroll
        for (int i = 0; i < DEC_NW; ++i) { acc += part[i * 64 + lane]; lt += redl[i]; }
        p.o[(long)b * p.ldo + h * 64 + lane] = f2bf(acc / lt);
    }
}

template <int MODE, bool XBF, bool ROWS = false>
static int launch_decode_proj_ni(const DecAttnP& p, const dim3& grid, const dim3& block, size_t smem, hipStream_t s) {
    switch (p.D >> 6) {
#define DW_NI(n) case n: hipLaunchKernelGGL((attn_decode_proj_kernel<MODE, XBF, n, ROWS>), grid, block, smem, s, p); break;
        DW_NI(6) DW_NI(8) DW_NI(12) DW_NI(16) DW_NI(20)        // d_model 384 / 512 / 768 / 1024 / 1280
#undef DW_NI
        default: return DW_EINVAL;
    }
    DW_CHECK_LAUNCH();
    return DW_OK;
}
static bool decode_proj_dim_ok(int D) { return D == 384 || D == 512 || D == 768 || D == 1024 || D == 1280; }
// The one dispatch of attn_decode_proj_kernel (include/dwamd.h): decode_pass calls it for both of its attention blocks, the tests
// call it alone.  Every refusal comes before the launch.
// rows: the per-row entry (dw_decode_attn_proj_rows); Lk is then max_t + 1, so the refusals by Lk bound every row's key count.
static int decode_attn_proj(int mode, const void* x, int x_dtype, int64_t ldx, const float* ln_g, const float* ln_b, float eps,
                            const void* w, const float* bias, const void* k, const void* v, int64_t ldkv, int64_t kv_rows,
                            void* kv_app, void* o, int64_t ldo, int B, int H, int Lk, float scale, bool rows, const int32_t* row_t,
                            void* stream) {
    if (mode != 0 && mode != 1) return DW_EINVAL;
    if (rows && (mode != 1 || !row_t || ((uintptr_t)row_t & 3))) return DW_EINVAL;
    if (x_dtype != DW_F32 && x_dtype != DW_BF16) return DW_EINVAL;
    if (!x || !ln_g || !ln_b || !w || !bias || !k || !v || !o || (mode == 1 && !kv_app)) return DW_EINVAL;
    if (B <= 0 || H <= 0 || Lk < 1 || Lk > kv_rows) return DW_EINVAL;
    // 16-byte loads: the row of x, the weight fragments, the key / value groups, four floats of gamma / beta per lane
    if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)k | (uintptr_t)v | (uintptr_t)ln_g | (uintptr_t)ln_b) & 15) || (ldx & 7) || (ldkv & 7))
        return DW_EINVAL;
    if (((uintptr_t)bias & 3) || ((uintptr_t)o & 1) || (mode == 1 && ((uintptr_t)kv_app & 1))) return DW_EINVAL;
    if (B > 65535 || H > 65535 || !decode_proj_dim_ok(H * 64) || Lk > 8192) return DW_EUNSUP;
    const int D = H * 64;
    if (ldx < D || ldo < D || ldkv < (mode == 1 ? 2L * D : (long)D)) return DW_EINVAL;
    DecAttnP p = {};
    p.x = x; p.ldx = ldx; p.ln_g = ln_g; p.ln_b = ln_b; p.eps = eps;
    p.w = (const bf16*)w; p.bias = bias;
    p.k = (const bf16*)k; p.v = (const bf16*)v; p.ldkv = ldkv; p.kv_rows = kv_rows;
    p.kv_app = mode == 1 ? (bf16*)kv_app : nullptr; p.o = (bf16*)o; p.ldo = ldo;
    p.D = D; p.Lk = Lk; p.t = mode == 1 ? Lk - 1 : 0; p.scale = scale;
    p.row_t = row_t; p.max_t = Lk - 1;
    const size_t smem = ((((size_t)p.Lk + 3) & ~(size_t)3) + DEC_NW * 64 + 3 * DEC_NW + 3 * 64) * 4 + (size_t)p.D * 6;
    const dim3 grid(1, H, B), block(64 * DEC_NW);
    const hipStream_t s = (hipStream_t)stream;
    const bool xbf = x_dtype == DW_BF16;
    if (rows) return xbf ? launch_decode_proj_ni<1, true, true>(p, grid, block, smem, s) : launch_decode_proj_ni<1, false, true>(p, grid, block, smem, s);
    if (mode == 0 && xbf) return launch_decode_proj_ni<0, true>(p, grid, block, smem, s);
    if (mode == 0) return launch_decode_proj_ni<0, false>(p, grid, block, smem, s);
    if (xbf) return launch_decode_proj_ni<1, true>(p, grid, block, smem, s);
    return launch_decode_proj_ni<1, false>(p, grid, block, smem, s);
}
extern "C" int dw_decode_attn_proj(int mode, const void* x, int x_dtype, int64_t ldx, const float* ln_g, const float* ln_b, float eps,
                                   const void* w, const float* bias, const void* k, const void* v, int64_t ldkv, int64_t kv_rows,
                                   void* kv_app, void* o, int64_t ldo, int B, int H, int Lk, float scale, void* stream) {
    DW_CLEAR_ERR();
    return decode_attn_proj(mode, x, x_dtype, ldx, ln_g, ln_b, eps, w, bias, k, v, ldkv, kv_rows, kv_app, o, ldo, B, H, Lk, scale, false,
                            nullptr, stream);
}
// Mode 1 with sequence b at its own position row_t[b] (device int32 [B], clamped to [0, max_t] by the kernel; the host never reads
// it): the new K/V go to cache row row_t[b] and the softmax runs over row_t[b] + 1 keys.  The refusals of the uniform entry with
// Lk = max_t + 1, in front of the launch.
extern "C" int dw_decode_attn_proj_rows(const void* x, int x_dtype, int64_t ldx, const float* ln_g, const float* ln_b, float eps,
                                        const void* w, const float* bias, const void* k, const void* v, int64_t ldkv, int64_t kv_rows,
                                        void* kv_app, void* o, int64_t ldo, int B, int H, float scale, const int32_t* row_t,
                                        int32_t max_t, void* stream) {
    DW_CLEAR_ERR();
    if (max_t < 0 || (int64_t)max_t + 1 > kv_rows) return DW_EINVAL;
    return decode_attn_proj(1, x, x_dtype, ldx, ln_g, ln_b, eps, w, bias, k, v, ldkv, kv_rows, kv_app, o, ldo, B, H, max_t + 1, scale, true,
                            row_t, stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// One decoder pass of cached greedy decoding as ONE C call: every launch of `WhisperDecoder.forward` on the cache
// branch (TF:modeling_whisper.py:690-795 with 312-335; reached from `generate`, run_eval.py:739,
// run_distillation.py:1524-1528, run_pseudo_labelling.py:861-996) is enqueued on the caller's stream: embedding,
// per layer LayerNorm -> fused QKV GEMM -> K/V appended to the cache in place -> self-attention over the cached prefix
// -> out-proj + residual -> LayerNorm -> Q GEMM -> cross-attention over the static encoder K/V -> out-proj + residual
// -> LayerNorm -> FC1 + GELU -> FC2 + residual, then the final LayerNorm and the tied LM head.  n_new = 1 is the
// token step (skinny weight-streaming GEMMs, streaming single-query attention); n_new > 1 scores several new
// positions against the cache with the bottom-right aligned causal mask (prompt prefill, the verify pass of assisted
// decoding).  Nothing is allocated; no host synchronisation: the call can be captured into a HIP graph.

__global__ __launch_bounds__(256) void kv_append_kernel(const bf16* qkv, bf16* cache, int n_new, int t, int max_len,
                                                         int D, long nvec) {
    // cache[b][t + j][0 .. 2D) = qkv[b * n_new + j][D .. 3D)   (8 bf16 per thread)
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    const int per_row = (2 * D) >> 3;
    const long row = i / per_row;
    const int c = (int)(i - row * per_row) << 3;
    const long b = row / n_new;
    const int j = (int)(row - b * n_new);
    *(bf16x8*)(cache + ((b * max_len + t + j) * 2L * D) + c) = *(const bf16x8*)(qkv + row * 3L * D + D + c);
}

// ---------------------------------------------------------------------------------------------------------------------
// The cached pass at per-row positions (dw_decode_step_rows; the verify / catch-up / draft passes of speculative decoding with
// per-row acceptance, decoding._assisted_rounds_device_rows).  Row b of the batch stands at position row_t[b]: its n new tokens
// take the position embeddings row_t[b] + j, their K/V go to cache rows row_t[b] + j and query j sees the keys [0, row_t[b] + j].
// row_t is device memory that only these three kernels read; each clamps it to [0, max_t], the host's bound that the caller
// checked against the cache (max_t + n <= max_len): a stale or wild entry cannot reach past a row's own cache.
// ---------------------------------------------------------------------------------------------------------------------

// embed_fwd_kernel (elementwise.hip) with the position row taken per sequence: x[b * n + j] = tok[ids[b][j]] + pos[row_t[b] + j],
// the sum in fp32, rounded once where the stream is bf16.  BF: tables and stream bf16, else both f32 (DwDecodeStep.stream_dtype).
template <bool BF>
__global__ __launch_bounds__(256) void embed_rows_kernel(const int64_t* ids, const void* tok, const void* pos, void* out,
                                                         const int32_t* row_t, int max_t, int n, int D, long nvec) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    const int dv = D >> 2;
    const long row = i / dv;
    const int c = (int)(i - row * dv) * 4;
    const long b = row / n;
    const long t = row_pos(row_t, b, max_t) + (int)(row - b * n);
    const long id = ids[row];
    if (BF) {
        const bf16x4 x = *(const bf16x4*)((const bf16*)tok + id * D + c);
        const bf16x4 y = *(const bf16x4*)((const bf16*)pos + t * D + c);
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(bf2f(x[e]) + bf2f(y[e]));
        *(bf16x4*)((bf16*)out + row * D + c) = o;
    } else {
        const f32x4 a = *(const f32x4*)((const float*)tok + id * D + c);
        const f32x4 p = *(const f32x4*)((const float*)pos + t * D + c);
        *(f32x4*)((float*)out + row * D + c) = a + p;
    }
}

// kv_append_kernel with the first cache row taken per sequence: cache[b][row_t[b] + j][0 .. 2D) = qkv[b * n + j][D .. 3D)
__global__ __launch_bounds__(256) void kv_append_rows_kernel(const bf16* qkv, bf16* cache, const int32_t* row_t, int max_t,
                                                              int n_new, int max_len, int D, long nvec) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= nvec) return;
    const int per_row = (2 * D) >> 3;
    const long row = i / per_row;
    const int c = (int)(i - row * per_row) << 3;
    const long b = row / n_new;
    const int j = (int)(row - b * n_new);
    const long t = row_pos(row_t, b, max_t);
    *(bf16x8*)(cache + ((b * max_len + t + j) * 2L * D) + c) = *(const bf16x8*)(qkv + row * 3L * D + D + c);
}

// Cached self-attention of a few queries against a per-row key count: n <= AR_MAXQ queries of head h of sequence b (rows b * n + j
// of qkv, head_dim 64) over the sequence's cache rows [0, t0 + n), t0 = row_t[b]; query j sees the keys k <= t0 + j.  One
// workgroup of four waves per (head, sequence); the work is a few hundred keys, so the kernel is three short phases over LDS
// instead of tiles:
//   1. scores: eight lanes share a key (16 bytes = 8 head dimensions each, AR_UN key groups requested ahead), every query's dot
//      product against it from the fp32 q in LDS (bf16 q x scale x log2 e), s[j][k] to LDS;
//   2. softmax: wave w owns the queries j = w (mod 4): the maximum and the sum over the keys the query sees, P rounded to bf16 (as
//      the other attention kernels feed their PV product) back into LDS, a key behind the query's own position as 0;
//   3. PV: the same lane-to-key mapping over V, AR_JC queries per sweep in registers (8 dimensions x AR_JC accumulators), summed
//      over the key slots of a wave by shuffles and over the waves through LDS, divided by the sum, stored as bf16.
// Same arithmetic as attn_decode_proj_kernel above (fp32 dot products of bf16 operands, exp2, unrounded sum, rounded P); the order
// of the sums over the keys is this kernel's own.  LDS: n x 64 q + n x ldk scores + 4 x AR_JC x 64 partial outputs + n sums, ldk
// = max_t + n rounded up to 4 (attn_rows_smem; the caller refuses more than 64 KiB).
constexpr int AR_NT = 256, AR_NW = AR_NT / 64, AR_JC = 8, AR_UN = 4, AR_MAXQ = 32;
static size_t attn_rows_smem(int n, int ldk) { return ((size_t)n * 64 + (size_t)n * ldk + AR_NW * AR_JC * 64 + AR_MAXQ) * 4; }

__global__ __launch_bounds__(AR_NT) void attn_rows_kernel(const bf16* qkv, long ldq, const bf16* cache, long ldkv, long kv_rows,
                                                          const int32_t* row_t, int max_t, bf16* o, long ldo, int n, int ldk,
                                                          float scale) {
    extern __shared__ __attribute__((aligned(16))) float arsm[];
    float* qs = arsm;                                   // [n][64]
    float* sc = qs + n * 64;                            // [n][ldk]
    float* part = sc + (long)n * ldk;                   // [AR_NW][AR_JC][64]
    float* lsum = part + AR_NW * AR_JC * 64;            // [n]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.x, b = blockIdx.y;
    const int t0 = __builtin_amdgcn_readfirstlane(row_pos(row_t, b, max_t));
    const int Lk = t0 + n;                              // keys of the last query; <= max_t + n <= ldk
    const float c = scale * 1.4426950408889634f;
    if (tid < n * 8) {
        const int j = tid >> 3, d0 = (tid & 7) * 8;
        const bf16x8 q = *(const bf16x8*)(qkv + ((long)b * n + j) * ldq + h * 64 + d0);
#pragma unroll
        for (int e = 0; e < 8; ++e) qs[j * 64 + d0 + e] = bf2f(q[e]) * c;
    }
    __syncthreads();
    // ---- 1. scores ----
    const int sub = tid >> 3, ds = (tid & 7) * 8;       // key slot 0..31 of a sweep, head dimensions ds .. ds + 7
    const bf16* K = cache + (long)b * kv_rows * ldkv + h * 64 + ds;
    const bf16* V = K + (ldkv >> 1);                    // (K | V per cache row: V starts D = ldkv / 2 columns in)
    for (int k0 = 0; k0 < Lk; k0 += 32 * AR_UN) {
        bf16x8 kr[AR_UN];
#pragma unroll
        for (int u = 0; u < AR_UN; ++u) {
            const int k = min(k0 + u * 32 + sub, Lk - 1);
            kr[u] = *(const bf16x8*)(K + (long)k * ldkv);
        }
#pragma unroll
        for (int u = 0; u < AR_UN; ++u) {
            const int k = k0 + u * 32 + sub;
            float kf[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) kf[e] = bf2f(kr[u][e]);
            for (int j = 0; j < n; ++j) {
                const f32x4 qa = *(const f32x4*)(qs + j * 64 + ds), qb = *(const f32x4*)(qs + j * 64 + ds + 4);
                float s = 0.f;
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fmaf(qa[e], kf[e], s);
#pragma unroll
                for (int e = 0; e < 4; ++e) s = fmaf(qb[e], kf[4 + e], s);
                s += __shfl_xor(s, 1);
                s += __shfl_xor(s, 2);
                s += __shfl_xor(s, 4);
                if ((tid & 7) == 0 && k < Lk) sc[(long)j * ldk + k] = s;
            }
        }
    }
    __syncthreads();
    // ---- 2. softmax of query j over its t0 + j + 1 keys ----
    for (int j = wave; j < n; j += AR_NW) {
        float* row = sc + (long)j * ldk;
        const int nk = t0 + j + 1;
        float mx = NEG_BIG_D;
        for (int k = lane; k < nk; k += 64) mx = fmaxf(mx, row[k]);
        mx = wave_max(mx);
        float sum = 0.f;
        for (int k = lane; k < Lk; k += 64) {
            float p = 0.f;
            if (k < nk) {
                p = __builtin_amdgcn_exp2f(row[k] - mx);
                sum += p;
                p = round_bf16(p);
            }
            row[k] = p;
        }
        sum = wave_sum(sum);
        if (lane == 0) lsum[j] = sum;
    }
    __syncthreads();
    // ---- 3. PV, AR_JC queries per sweep over the keys ----
    for (int j0 = 0; j0 < n; j0 += AR_JC) {
        const int nj = min(AR_JC, n - j0);
        const int Lj = t0 + j0 + nj;                    // keys of the sweep's last query
        float acc[AR_JC][8];
#pragma unroll
        for (int jj = 0; jj < AR_JC; ++jj)
#pragma unroll
            for (int e = 0; e < 8; ++e) acc[jj][e] = 0.f;
        for (int k0 = 0; k0 < Lj; k0 += 32 * AR_UN) {
            bf16x8 vr[AR_UN];
#pragma unroll
            for (int u = 0; u < AR_UN; ++u) {
                const int k = min(k0 + u * 32 + sub, Lj - 1);
                vr[u] = *(const bf16x8*)(V + (long)k * ldkv);
            }
#pragma unroll
            for (int u = 0; u < AR_UN; ++u) {
                const int k = k0 + u * 32 + sub;
                if (k < Lj) {
                    float vf[8];
#pragma unroll
                    for (int e = 0; e < 8; ++e) vf[e] = bf2f(vr[u][e]);
#pragma unroll
                    for (int jj = 0; jj < AR_JC; ++jj) {
                        if (jj < nj) {
                            const float p = sc[(long)(j0 + jj) * ldk + k];
#pragma unroll
                            for (int e = 0; e < 8; ++e) acc[jj][e] = fmaf(p, vf[e], acc[jj][e]);
                        }
                    }
                }
            }
        }
#pragma unroll
        for (int jj = 0; jj < AR_JC; ++jj) {
            if (jj < nj) {                              // (uniform: every lane of the wave takes part in the shuffles)
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float a = acc[jj][e];
                    a += __shfl_xor(a, 8);
                    a += __shfl_xor(a, 16);
                    a += __shfl_xor(a, 32);
                    if (lane < 8) part[(wave * AR_JC + jj) * 64 + ds + e] = a;
                }
            }
        }
        __syncthreads();
        for (int i = tid; i < nj * 64; i += AR_NT) {
            const int jj = i >> 6, dcol = i & 63;
            float a = 0.f;
#pragma unroll
            for (int w = 0; w < AR_NW; ++w) a += part[(w * AR_JC + jj) * 64 + dcol];
            o[((long)b * n + j0 + jj) * ldo + h * 64 + dcol] = f2bf(a / lsum[j0 + jj]);
        }
        __syncthreads();
    }
}

// The pass of dw_decode_step (row_t == nullptr: every row starts at d->t) and of dw_decode_step_rows (row b starts at row_t[b] <=
// max_t, a device array the host never reads: `t` is then max_t and sizes launches only).  The rows pass swaps three launches --
// embedding, K/V append, self-attention (the *_rows kernels above) -- and keeps every other launch of the uniform pass.
// token_rows (dw_decode_token_rows, n_new == 1): the rows pass keeps the self-attention with its projection inside, at per-row positions.
static int decode_pass(const DwDecodeStep* d, const int32_t* row_t, int t, void* stream, bool token_rows = false) {
    const int B = d->batch, n = d->n_new, D = d->d_model, H = d->heads, F = d->ffn;
    if (B <= 0 || n <= 0 || D != H * 64 || (D & 63) || (F & 63) || d->n_layers <= 0 || d->src_len <= 0 || t < 0 ||
        t + n > d->max_len || d->ldv < d->vocab || (d->ldv & 15))
        return DW_EINVAL;
    if (d->stream_dtype != DW_F32 && d->stream_dtype != DW_BF16) return DW_EINVAL;
    const int rows = B * n;
    const long ldx = d->cross_kv_ld > 0 ? d->cross_kv_ld : 2L * D;        // row pitch of the cross-attention K | V
    if (ldx < 2L * D || (ldx & 7)) return DW_EINVAL;
    const int ldk = (t + n + 3) & ~3;                                     // rows pass: pitch of a query's scores in LDS
    const size_t rows_smem = attn_rows_smem(n, ldk);
    // FP8 cross-attention K/V (include/dwamd.h): only the token step's kernel reads them -- refused before anything is launched
    const bool kv8 = d->cross_kv_fmt == 1;
    if (d->cross_kv_fmt != 0 && !kv8) return DW_EINVAL;
    if (kv8) {
        if (n != 1 || (row_t && !token_rows) || !decode_proj_dim_ok(D) || (g_decode_fuse_off & 8) || d->src_len > 8192 || B > 65535)
            return DW_EUNSUP;
        for (int l = 0; l < d->n_layers; ++l) {
            const DwDecoderLayer& L = d->layers[l];
            if (!L.cross_k8 || !L.cross_v8 || !L.cross_scale || !L.bq || !L.ln2_g || !L.ln2_b) return DW_EINVAL;
            if ((((uintptr_t)L.cross_k8 | (uintptr_t)L.cross_v8) & 15) || ((uintptr_t)L.cross_scale & 3)) return DW_EINVAL;
        }
    }
    if (row_t) {                                                          // (refused before anything is launched)
        if (n > AR_MAXQ || B > 65535 || rows_smem > 65536) return DW_EUNSUP;
        for (int l = 0; l < d->n_layers; ++l) {
            const DwDecoderLayer& L = d->layers[l];
            if (!L.wqkv || !L.wo || !L.wq || !L.wo2 || !L.w1 || !L.w2 || !L.self_kv || (!kv8 && !L.cross_kv)) return DW_EINVAL;
        }
    }
    const size_t es = d->stream_dtype == DW_F32 ? 4 : 2;
    int rc = DW_OK;
    if (row_t) {
        const long nvec = (long)rows * (D >> 2);
        const dim3 grid((nvec + 255) / 256), block(256);
        if (d->stream_dtype == DW_BF16)
            hipLaunchKernelGGL(embed_rows_kernel<true>, grid, block, 0, (hipStream_t)stream, (const int64_t*)d->ids, d->tok_emb,
                               d->pos_emb, d->x, row_t, t, n, D, nvec);
        else
            hipLaunchKernelGGL(embed_rows_kernel<false>, grid, block, 0, (hipStream_t)stream, (const int64_t*)d->ids, d->tok_emb,
                               d->pos_emb, d->x, row_t, t, n, D, nvec);
        DW_CHECK_LAUNCH();
    } else {
        rc = dw_embed_fwd(d->ids, d->tok_emb, (const char*)d->pos_emb + (size_t)t * D * es, d->stream_dtype, d->x,
                          d->stream_dtype, B, n, D, stream);
    }
    if (rc != DW_OK) return rc;
    // With few rows the LayerNorm in front of a projection is computed inside the weight-streaming GEMM and the new
    // K/V go straight into the cache (DwGemm.ln_x / kv_out): 9 launches per layer instead of 13.
    // (the rows pass takes neither fusion that bakes a uniform position: the GEMM's kv_out / kv_row0 and the self-attention with
    // its projection inside)
    const bool fuse_ln = rows <= 32 && D <= 1280 && !(g_decode_fuse_off & 1);
    const bool fuse_kv = !row_t && rows <= 64 && !(g_decode_fuse_off & 2);
    // token step: the q (q / k / v) projection of a head is computed by the attention workgroup of that head
    const bool proj_ok = n == 1 && decode_proj_dim_ok(D);
    const bool proj_self = (!row_t || token_rows) && proj_ok && !(g_decode_fuse_off & 4) && t + 1 <= 8192;
    const bool proj_cross = proj_ok && !(g_decode_fuse_off & 8) && d->src_len <= 8192;
    auto gemm = [&](const void* a, long lda, const void* w, const float* bias, int N, int K, void* c, long ldc, int c_dtype,
                    int act, const void* r, const float* ln_g, const float* ln_b, void* kv) -> int {
        DwGemm g = {};
        g.a = a; g.b = w; g.c = c; g.bias = bias; g.r = r;
        g.lda = lda; g.ldb = K; g.ldc = ldc; g.ldr = ldc;
        g.m = rows; g.n = N; g.k = K;
        g.act = act; g.c_dtype = c_dtype; g.r_dtype = c_dtype; g.round_res = 1;
        if (ln_g) {                                   // a = the residual stream x, normalised on load
            g.a = nullptr; g.ln_x = a; g.ld_lnx = lda; g.ln_x_dtype = d->stream_dtype;
            g.ln_gamma = ln_g; g.ln_beta = ln_b; g.ln_eps = 1e-5f;
        }
        if (kv) {
            g.kv_out = kv; g.kv_ld = 2 * D; g.kv_split = D; g.kv_rows_per_batch = n; g.kv_batch_pitch = d->max_len;
            g.kv_row0 = t;
        }
        return dw_gemm_bf16(&g, stream);
    };
    auto ln = [&](const float* gam, const float* bet) -> int {
        return dw_layernorm_fwd(d->x, d->stream_dtype, gam, bet, d->h, nullptr, nullptr, rows, D, 1e-5f, stream);
    };
    for (int l = 0; l < d->n_layers; ++l) {
        const DwDecoderLayer& L = d->layers[l];
        if (!L.wqkv || !L.wo || !L.wq || !L.wo2 || !L.w1 || !L.w2 || !L.self_kv || (!kv8 && !L.cross_kv)) return DW_EINVAL;
        // ---- self-attention over the cached prefix ----
        if (proj_self && L.bqkv && L.ln1_g && L.ln1_b) {
            const bf16* kc0 = (const bf16*)L.self_kv;
            if ((rc = decode_attn_proj(1, d->x, d->stream_dtype, D, L.ln1_g, L.ln1_b, 1e-5f, L.wqkv, L.bqkv, kc0, kc0 + D, 2L * D,
                                       d->max_len, L.self_kv, d->o, D, B, H, t + 1, 0.125f, row_t != nullptr, row_t, stream)) != DW_OK)
                return rc;
        } else {
        if (fuse_ln) {
            rc = gemm(d->x, D, L.wqkv, L.bqkv, 3 * D, D, d->qkv, 3 * D, DW_BF16, 0, nullptr, L.ln1_g, L.ln1_b,
                      fuse_kv ? L.self_kv : nullptr);
        } else {
            if ((rc = ln(L.ln1_g, L.ln1_b)) != DW_OK) return rc;
            rc = gemm(d->h, D, L.wqkv, L.bqkv, 3 * D, D, d->qkv, 3 * D, DW_BF16, 0, nullptr, nullptr, nullptr,
                      fuse_kv ? L.self_kv : nullptr);
        }
        if (rc != DW_OK) return rc;
        const bf16* kc = (const bf16*)L.self_kv;
        if (row_t) {
            const long nvec = (long)rows * ((2 * D) >> 3);
            hipLaunchKernelGGL(kv_append_rows_kernel, dim3((nvec + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                               (const bf16*)d->qkv, (bf16*)L.self_kv, row_t, t, n, d->max_len, D, nvec);
            DW_CHECK_LAUNCH();
            hipLaunchKernelGGL(attn_rows_kernel, dim3(H, B), dim3(AR_NT), rows_smem, (hipStream_t)stream, (const bf16*)d->qkv,
                               3L * D, kc, 2L * D, (long)d->max_len, row_t, t, (bf16*)d->o, (long)D, n, ldk, 0.125f);
            DW_CHECK_LAUNCH();
        } else {
        if (!fuse_kv) {
            const long nvec = (long)rows * ((2 * D) >> 3);
            hipLaunchKernelGGL(kv_append_kernel, dim3((nvec + 255) / 256), dim3(256), 0, (hipStream_t)stream,
                               (const bf16*)d->qkv, (bf16*)L.self_kv, n, t, d->max_len, D, nvec);
            DW_CHECK_LAUNCH();
        }
        if ((rc = dw_attn_fwd_ex(d->qkv, kc, kc + D, d->o, nullptr, B, H, n, t + n, 3 * D, 2 * D, 2 * D, D, n, d->max_len,
                                 n > 1 ? 2 : 0, 0.125f, stream)) != DW_OK) return rc;
        }
        }
        if ((rc = gemm(d->o, D, L.wo, L.bo, D, D, d->x, D, d->stream_dtype, 0, d->x, nullptr, nullptr, nullptr)) != DW_OK)
            return rc;
        // ---- cross-attention over the static encoder K/V ----
        if (kv8) {
            if ((rc = dw_decode_attn_proj_kv8(d->x, d->stream_dtype, D, L.ln2_g, L.ln2_b, 1e-5f, L.wq, L.bq, L.cross_k8, L.cross_v8,
                                              L.cross_scale, d->src_len, d->o, D, B, H, d->src_len, 0.125f, stream)) != DW_OK) return rc;
        } else if (proj_cross && L.bq && L.ln2_g && L.ln2_b) {
            const bf16* kx0 = (const bf16*)L.cross_kv;
            if ((rc = dw_decode_attn_proj(0, d->x, d->stream_dtype, D, L.ln2_g, L.ln2_b, 1e-5f, L.wq, L.bq, kx0, kx0 + D, ldx, d->src_len,
                                          nullptr, d->o, D, B, H, d->src_len, 0.125f, stream)) != DW_OK) return rc;
        } else {
        if (fuse_ln) {
            rc = gemm(d->x, D, L.wq, L.bq, D, D, d->qkv, 3 * D, DW_BF16, 0, nullptr, L.ln2_g, L.ln2_b, nullptr);
        } else {
            if ((rc = ln(L.ln2_g, L.ln2_b)) != DW_OK) return rc;
            rc = gemm(d->h, D, L.wq, L.bq, D, D, d->qkv, 3 * D, DW_BF16, 0, nullptr, nullptr, nullptr, nullptr);
        }
        if (rc != DW_OK) return rc;
        const bf16* kx = (const bf16*)L.cross_kv;
        if ((rc = dw_attn_fwd_ex(d->qkv, kx, kx + D, d->o, nullptr, B, H, n, d->src_len, 3 * D, ldx, ldx, D, n,
                                 d->src_len, 0, 0.125f, stream)) != DW_OK) return rc;
        }
        if ((rc = gemm(d->o, D, L.wo2, L.bo2, D, D, d->x, D, d->stream_dtype, 0, d->x, nullptr, nullptr, nullptr)) != DW_OK)
            return rc;
        // ---- feed-forward ----
        if (fuse_ln) {
            rc = gemm(d->x, D, L.w1, L.b1, F, D, d->a, F, DW_BF16, 1, nullptr, L.ln3_g, L.ln3_b, nullptr);
        } else {
            if ((rc = ln(L.ln3_g, L.ln3_b)) != DW_OK) return rc;
            rc = gemm(d->h, D, L.w1, L.b1, F, D, d->a, F, DW_BF16, 1, nullptr, nullptr, nullptr, nullptr);
        }
        if (rc != DW_OK) return rc;
        if ((rc = gemm(d->a, F, L.w2, L.b2, D, F, d->x, D, d->stream_dtype, 0, d->x, nullptr, nullptr, nullptr)) != DW_OK)
            return rc;
    }
    if ((rc = dw_layernorm_fwd(d->x, d->stream_dtype, d->lnf_g, d->lnf_b, d->h, nullptr, nullptr, rows, D, 1e-5f,
                               stream)) != DW_OK) return rc;
    return gemm(d->h, D, d->lm_head, nullptr, d->ldv, D, d->logits, d->ldv, DW_BF16, 0, nullptr, nullptr, nullptr, nullptr);
}

static bool decode_desc_ok(const DwDecodeStep* d) {
    return d && d->ids && d->tok_emb && d->pos_emb && d->layers && d->lm_head && d->x && d->h && d->qkv && d->o && d->a && d->logits;
}

extern "C" int dw_decode_step(const DwDecodeStep* d, void* stream) {
    DW_CLEAR_ERR();
    if (!decode_desc_ok(d)) return DW_EINVAL;
    return decode_pass(d, nullptr, d->t, stream);
}

extern "C" int dw_decode_step_rows(const DwDecodeStep* d, const int32_t* row_t, int32_t max_t, void* stream) {
    DW_CLEAR_ERR();
    if (!decode_desc_ok(d) || !row_t || ((uintptr_t)row_t & 3)) return DW_EINVAL;
    return decode_pass(d, row_t, max_t, stream);
}

// The token step (n_new == 1) with row b at position row_t[b]: the launches of dw_decode_step with the embedding and the
// self-attention taken per row (embed_rows_kernel, attn_decode_proj_kernel<1, ., ., true>).  Where the width has no such kernel or
// dw_debug_set key 7 has the self-attention fusion off, the pass of dw_decode_step_rows.
extern "C" int dw_decode_token_rows(const DwDecodeStep* d, const int32_t* row_t, int32_t max_t, void* stream) {
    DW_CLEAR_ERR();
    if (!decode_desc_ok(d) || !row_t || ((uintptr_t)row_t & 3) || d->n_new != 1) return DW_EINVAL;
    return decode_pass(d, row_t, max_t, stream, true);
}
