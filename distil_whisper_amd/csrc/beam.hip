// Beam search: one token step of `generate(num_beams=k)` on the device (TF:generation/utils.py `_beam_search`, the vectorised
// algorithm that decoding.beam_search_decode restates in torch), as reached from run_eval.py:143, 693 and
// run_distillation.py:1428-1436.
//   dw_beam_candidates  one 1024-thread workgroup per beam row: log_softmax over the raw row, the logits rules of
//                       greedy_select_kernel<false> (select_rules.h), + the row's running score, the K = 2k best as
//                       (value, token) ordered by value descending, then column ascending.
//   dw_beam_update      the bookkeeping of the step for the whole batch in ONE workgroup (a wave per utterance, the state of an
//                       utterance lives in the lanes' registers): merge of the k x K candidates into the utterance's top K, the k
//                       best open continuations, the merge of finished hypotheses under the length penalty, the early-stopping
//                       heuristic and the loop condition, written to the device word `stop`.  It decides WHICH rows move; a second,
//                       row-parallel launch of the same call moves them (the rows are up to 3.5 KB each, R of them twice).
// Nothing here waits for another workgroup, allocates or synchronises with the host.  Once `stop` is set both entries leave the
// state as it is (the row copy becomes the identity), so the host may read `stop` every few steps only.
// Ties: equal values go to the lower flat index beam * V + token (torch.topk leaves the order of equal scores unspecified).
#include "common.h"
#include "select_rules.h"
#include "../../include/dwamd.h"

#define BEAM_MAX_K 16                               // beams per utterance; K = 2k candidates per row
#define BEAM_NEG (-1.0e9f)                          // the reference's "minus infinity" of beam scores

// NCH chunks of four columns per thread: 13 up to 53 248 columns (every Whisper vocabulary), 16 up to 65 536.
template <int NCH>
__global__ __launch_bounds__(SEL_NT) void beam_candidates_kernel(
    const bf16* logits, int V, long ld, const uint8_t* suppress, const uint8_t* begin_suppress, int first, int no_eos, int tb,
    int max_initial, const int64_t* tokens, long tok_ld, int n, int begin_index, int eos, const float* run_scores, int K,
    float* cand_val, int32_t* cand_tok, const int32_t* stop) {
    __shared__ Best red[SEL_NT / 64];
    __shared__ float redf[SEL_NT / 64];
    __shared__ double redd[SEL_NT / 64];
    __shared__ int redi[SEL_NT / 64];
    if (*stop) return;                              // (uniform)
    const int b = blockIdx.x, tid = threadIdx.x;
    const int64_t* row_tok = tokens + (long)b * tok_ld;
    const bf16* row = logits + (long)b * ld;
    const RowRules rr = row_rules(row_tok, n, begin_index, tb, max_initial, V, eos, no_eos, redi);
    const bool word_masks = (((uintptr_t)suppress | (uintptr_t)begin_suppress) & 3) == 0;
    // ---- the row into registers as it is stored (bf16, slot 4 i + e holds column tid * 4 + i * 4096 + e) with one bit per slot:
    // the rules allow the column.  The fp32 scores replace it only at the end (a 1024-thread workgroup has 128 registers a lane) ----
    const int tid4 = tid * 4;
    auto col_of = [&](int j) -> int { return tid4 + (j >> 2) * (SEL_NT * 4) + (j & 3); };
    bf16x4 xr[NCH];
    unsigned long long okbits = 0, inbits = 0;          // bit j: slot j is allowed / inside the row
    float raw_max = -INFINITY, btv = -INFINITY, bsv = -INFINITY;   // row maximum; best allowed text / timestamp logit (mass rule)
    {
        const int clast = (V - 1) & ~3;
        unsigned mr[NCH];
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c0 = min(tid4 + i * SEL_NT * 4, clast);
            xr[i] = *(const bf16x4*)(row + c0);
            mr[i] = rule_masks_of(suppress, begin_suppress, first, word_masks, c0, V);
        }
#pragma unroll
        for (int i = 0; i < NCH; ++i) {
            const int c0 = tid4 + i * SEL_NT * 4;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int c = c0 + e;
                if (c >= V) continue;
                const float x = bf2f(xr[i][e]);
                inbits |= 1ull << (4 * i + e);
                raw_max = fmaxf(raw_max, x);
                if (column_allowed(rr, c0, e, V, mr[i])) {
                    okbits |= 1ull << (4 * i + e);
                    if (c < rr.tsb) btv = fmaxf(btv, x); else bsv = fmaxf(bsv, x);
                }
            }
        }
    }
    raw_max = block_max<SEL_NT>(raw_max, redf);
    btv = block_max<SEL_NT>(btv, redf);
    bsv = block_max<SEL_NT>(bsv, redf);
    // ---- log-sum-exp over ALL V raw logits (the reference takes log_softmax before its processors and does not renormalise):
    // fp32 terms, summed per thread in fp32 (<= 64 terms) and across the workgroup in double ----
    auto block_sum = [&](float part) -> float {
        double d = (double)part;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
        __syncthreads();
        if ((tid & 63) == 0) redd[tid >> 6] = d;
        __syncthreads();
        double t = 0.0;
        for (int i = 0; i < SEL_NT / 64; ++i) t += redd[i];
        return (float)t;
    };
    float part = 0.f;
#pragma unroll
    for (int j = 0; j < NCH * 4; ++j)
        if ((inbits >> j) & 1ull) part += __expf(bf2f(xr[j >> 2][j & 3]) - raw_max);
    const float logsum = logf(block_sum(part));
    // ---- the timestamp mass rule, as greedy_select_kernel decides it (the comparison is shift invariant) ----
    bool text_out = false;
    if (rr.ts_mode && bsv > -INFINITY) {
        float ps = 0.f;
#pragma unroll
        for (int j = 0; j < NCH * 4; ++j)
            if (((okbits >> j) & 1ull) && col_of(j) >= rr.tsb) ps += __expf(bf2f(xr[j >> 2][j & 3]) - bsv);
        text_out = bsv + __logf(block_sum(ps)) > btv;
    }
    // ---- accumulated scores, with torch's roundings: ((x - max) - log(sum)) + running; excluded columns -inf ----
    const float run = run_scores[b];
    float s[NCH * 4];
    Best mine = {-INFINITY, 0x7fffffff};
#pragma unroll
    for (int j = 0; j < NCH * 4; ++j) {
        const bool ok = ((okbits >> j) & 1ull) && !(text_out && col_of(j) < rr.tsb);
        const float v = ok ? __fadd_rn(__fsub_rn(__fsub_rn(bf2f(xr[j >> 2][j & 3]), raw_max), logsum), run) : -INFINITY;
        s[j] = v;
        if (v > mine.v) { mine.v = v; mine.i = col_of(j); }                 // (ascending columns: the first of equals)
    }
    // ---- the K largest, one workgroup reduction each; the owner of a winner drops it and rescans its slots ----
    for (int q = 0; q < K; ++q) {
        const Best w = block_best(mine, red);
        if (tid == 0) {
            cand_val[(long)b * K + q] = w.v;
            cand_tok[(long)b * K + q] = w.i == 0x7fffffff ? eos : w.i;
        }
        if (w.i != 0x7fffffff && ((w.i & (SEL_NT * 4 - 1)) >> 2) == tid) {
            const int slot = ((w.i / (SEL_NT * 4)) << 2) | (w.i & 3);
            mine.v = -INFINITY; mine.i = 0x7fffffff;
#pragma unroll
            for (int j = 0; j < NCH * 4; ++j) {
                if (j == slot) s[j] = -INFINITY;
                if (s[j] > mine.v) { mine.v = s[j]; mine.i = col_of(j); }
            }
        }
    }
}

extern "C" int dw_beam_candidates(const void* logits, int R, int V, int64_t ld, const uint8_t* suppress,
                                  const uint8_t* begin_suppress, int first, int no_eos, int ts_begin, int max_initial,
                                  const int64_t* tokens, int64_t tok_ld, int n, int begin_index, int eos, const float* run_scores,
                                  int K, float* cand_val, int32_t* cand_tok, const int32_t* stop, void* stream) {
    DW_CLEAR_ERR();
    if (!tokens || !run_scores || !cand_val || !cand_tok || !stop) return DW_EINVAL;
    if (R <= 0 || K < 2 || (K & 1) || n < 1 || n > tok_ld || eos < 0 || eos >= V) return DW_EINVAL;
    if (!select_args_ok(logits, V, ld, n, ts_begin, begin_index, eos)) return DW_EINVAL;
    if (K > 2 * BEAM_MAX_K || V > 16 * SEL_NT * 4) return DW_EUNSUP;
    auto kern = V <= 13 * SEL_NT * 4 ? beam_candidates_kernel<13> : beam_candidates_kernel<16>;
    hipLaunchKernelGGL(kern, dim3(R), dim3(SEL_NT), 0, (hipStream_t)stream, (const bf16*)logits, V, (long)ld, suppress,
                       begin_suppress, first, no_eos, ts_begin, max_initial, tokens, (long)tok_ld, n, begin_index, eos, run_scores,
                       K, cand_val, cand_tok, stop);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// dw_beam_update: lines `src_beam, tok = ...` through `unsat = ...` of decoding.beam_step_torch, value for value.  Every float
// operation is the single correctly rounded one torch performs (no contraction), so scores agree bit for bit given equal
// candidates.  Wave w handles utterances w, w + 16, ...: lane j < K holds merged candidate j, lane j < k the old hypothesis j.
// plan (int32 [4][R]) tells the row copy what to move: [0] source row of running, [1] token written at `cur` (-1: the source's),
// [2] source row of sequences (< R: the old sequences, else R + row of running), [3] token at `cur`.
// ---------------------------------------------------------------------------------------------------------------------
#define BEAM_UP_NT 1024
__global__ __launch_bounds__(BEAM_UP_NT) void beam_update_kernel(
    const float* cand_val, const int32_t* cand_tok, int B, int k, int V, int cur, int P, int max_length, int eos, int early,
    float fin_div, float hyp_div, float* run_scores, float* beam_scores, uint8_t* finished, int32_t* lengths, uint8_t* unsat,
    int32_t* stop, int64_t* src_rows, int64_t* next_tok, int32_t* plan) {
    __shared__ int flags[BEAM_UP_NT / 64][3];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int K = 2 * k, R = B * k;
    if (*stop) {                                    // (uniform) finished earlier: the state stays, every row maps to itself
        for (int r = tid; r < R; r += BEAM_UP_NT) {
            src_rows[r] = r;
            plan[r] = r; plan[R + r] = -1; plan[2 * R + r] = r; plan[3 * R + r] = -1;
        }
        return;
    }
    const bool last = cur + 1 >= max_length;
    int any_unsat = 0, all_fin = 1, all_hits = 1;
    for (int u = wave; u < B; u += BEAM_UP_NT / 64) {
        // ---- this utterance's top K of its k x K candidates: (value descending, flat index ascending, position ascending) ----
        const int nc = k * K;                        // <= 512: eight per lane
        float cv[8]; int cf[8];
        unsigned taken = 0;
#pragma unroll
        for (int e = 0; e < 8; ++e) {
            const int pos = lane + 64 * e;
            const bool in = pos < nc;
            cv[e] = in ? cand_val[(long)u * nc + pos] : -INFINITY;
            cf[e] = in ? (pos / K) * V + cand_tok[(long)u * nc + pos] : 0x7fffffff;
            if (!in) taken |= 1u << e;
        }
        float top_lp = -INFINITY; int top_flat = 0;
        for (int q = 0; q < K; ++q) {
            float bv = 0.f; int bf = 0x7fffffff, bp = 0x7fffffff;          // bp == 0x7fffffff: nothing yet
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                if ((taken >> e) & 1u) continue;
                const int pos = lane + 64 * e;
                if (bp == 0x7fffffff || cv[e] > bv || (cv[e] == bv && (cf[e] < bf || (cf[e] == bf && pos < bp)))) {
                    bv = cv[e]; bf = cf[e]; bp = pos;
                }
            }
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                const float ov = __shfl_xor(bv, o); const int of = __shfl_xor(bf, o), op = __shfl_xor(bp, o);
                if (op != 0x7fffffff && (bp == 0x7fffffff || ov > bv || (ov == bv && (of < bf || (of == bf && op < bp))))) {
                    bv = ov; bf = of; bp = op;
                }
            }
            if ((bp & 63) == lane) taken |= 1u << (bp >> 6);               // (nc >= K: every round finds one)
            if (lane == q) { top_lp = bv; top_flat = bf; }
        }
        const bool cand = lane < K;
        const int src_beam = cand ? top_flat / V : 0, tok = cand ? top_flat % V : 0;
        const bool hits = cand && (tok == eos || last);
        // ---- open beams carried on: the k best of open_lp ----
        const float open_lp = hits ? __fadd_rn(top_lp, BEAM_NEG) : top_lp;
        int rank_open = 0;
        for (int i = 0; i < K; ++i) {
            const float o = __shfl(open_lp, i);
            rank_open += (o > open_lp || (o == open_lp && i < lane)) ? 1 : 0;
        }
        // ---- old state of the utterance (read before anything of it is written) ----
        const bool old = lane < k;
        const float old_sc = old ? beam_scores[u * k + lane] : -INFINITY;
        const bool old_fin = old ? finished[u * k + lane] != 0 : true;
        const int old_len = old ? lengths[u * k + lane] : 0;
        const bool unsat_old = unsat[u] != 0;
        const bool all_fin_old = __all(old_fin);
        // ---- finished hypotheses: only the best k continuations may finish ----
        const bool just = hits && lane < k;
        float fin_lp = __fdiv_rn(top_lp, fin_div);
        if (all_fin_old && early == 1) fin_lp = __fadd_rn(fin_lp, BEAM_NEG);
        if (!unsat_old) fin_lp = __fadd_rn(fin_lp, BEAM_NEG);
        if (!just) fin_lp = __fadd_rn(fin_lp, BEAM_NEG);
        int rank_old = 0, rank_new = 0;              // position in the merged order [old 0..k) | new 0..K), ties to the lower index
        for (int i = 0; i < k; ++i) {
            const float o = __shfl(old_sc, i);
            rank_old += (o > old_sc || (o == old_sc && i < lane)) ? 1 : 0;
            rank_new += (o >= fin_lp) ? 1 : 0;
        }
        for (int i = 0; i < K; ++i) {
            const float o = __shfl(fin_lp, i);
            rank_old += (o > old_sc) ? 1 : 0;
            rank_new += (o > fin_lp || (o == fin_lp && i < lane)) ? 1 : 0;
        }
        const bool keep_old = old && rank_old < k, keep_new = cand && rank_new < k;
        // ---- writes ----
        if (cand && rank_open < k) {
            const int r = u * k + rank_open;
            run_scores[r] = open_lp;
            src_rows[r] = u * k + src_beam;
            next_tok[r] = tok;
            plan[r] = u * k + src_beam;
            plan[R + r] = tok;
        }
        if (keep_old) {
            const int r = u * k + rank_old;
            beam_scores[r] = old_sc; finished[r] = old_fin ? 1 : 0; lengths[r] = old_len;
            plan[2 * R + r] = u * k + lane; plan[3 * R + r] = -1;
        }
        if (keep_new) {
            const int r = u * k + rank_new;
            beam_scores[r] = fin_lp; finished[r] = just ? 1 : 0; lengths[r] = cur + 1 - P;
            plan[2 * R + r] = R + u * k + src_beam; plan[3 * R + r] = tok;
        }
        // ---- early-stopping heuristic on the new state ----
        const unsigned long long first_open = __ballot(cand && rank_open == 0);
        const float best_running = __fdiv_rn(__shfl(open_lp, (int)__ffsll((long long)first_open) - 1), hyp_div);
        float mn = INFINITY;                         // minimum of the k kept scores
        if (keep_old) mn = fminf(mn, old_sc);
        if (keep_new) mn = fminf(mn, fin_lp);
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) mn = fminf(mn, __shfl_xor(mn, o));
        const bool better_old = keep_old && best_running > (old_fin ? mn : BEAM_NEG);
        const bool better_new = keep_new && best_running > (just ? mn : BEAM_NEG);
        const bool unsat_new = unsat_old && __any(better_old || better_new);
        if (lane == 0) unsat[u] = unsat_new ? 1 : 0;
        any_unsat |= unsat_new ? 1 : 0;
        all_fin &= __all((!keep_old || old_fin) && (!keep_new || just)) ? 1 : 0;
        all_hits &= __all(!cand || hits) ? 1 : 0;
    }
    // ---- loop condition over the batch (TF `_beam_search_has_unfinished_sequences`) ----
    if (lane == 0) { flags[wave][0] = any_unsat; flags[wave][1] = all_fin; flags[wave][2] = all_hits; }
    __syncthreads();
    if (tid == 0) {
        int a = 0, f = 1, h = 1;
        for (int w = 0; w < BEAM_UP_NT / 64; ++w) { a |= flags[w][0]; f &= flags[w][1]; h &= flags[w][2]; }
        const bool go_on = a && !(f && early == 1) && !h;
        *stop = go_on ? 0 : 1;
    }
}

// The row moves the plan names, one workgroup per row: columns [0, cur] of running and of sequences (every buffer holds the pad
// token beyond the hypotheses' lengths, so nothing else differs).  in / out are different buffers: no row is read after another
// row has overwritten it.
__global__ __launch_bounds__(256) void beam_move_rows_kernel(const int64_t* run_in, int64_t* run_out, const int64_t* seq_in,
                                                             int64_t* seq_out, long tok_ld, int R, int cur, const int32_t* plan) {
    const int r = blockIdx.x;
    const int rs = plan[r], rt = plan[R + r], ss = plan[2 * R + r], st = plan[3 * R + r];
    if (rs < 0 || rs >= R || ss < 0 || ss >= 2 * R) return;                  // (never: the plan comes from beam_update_kernel)
    const int64_t* a = run_in + (long)rs * tok_ld;
    const int64_t* s = ss < R ? seq_in + (long)ss * tok_ld : run_in + (long)(ss - R) * tok_ld;
    int64_t* ao = run_out + (long)r * tok_ld;
    int64_t* so = seq_out + (long)r * tok_ld;
    for (int c = threadIdx.x; c <= cur; c += 256) {
        ao[c] = (c == cur && rt >= 0) ? (int64_t)rt : a[c];
        so[c] = (c == cur && st >= 0) ? (int64_t)st : s[c];
    }
}

extern "C" int dw_beam_update(const float* cand_val, const int32_t* cand_tok, int B, int k, int V, int cur, int prompt_len,
                              int max_length, int eos, int early_stopping, float fin_div, float hyp_div,
                              const int64_t* running_in, int64_t* running_out, const int64_t* sequences_in, int64_t* sequences_out,
                              int64_t tok_ld, float* run_scores, float* beam_scores, uint8_t* finished, int32_t* lengths,
                              uint8_t* unsat, int32_t* stop, int64_t* src_rows, int64_t* next_tok, int32_t* plan, void* stream) {
    DW_CLEAR_ERR();
    if (!cand_val || !cand_tok || !running_in || !running_out || !sequences_in || !sequences_out || !run_scores || !beam_scores ||
        !finished || !lengths || !unsat || !stop || !src_rows || !next_tok || !plan) return DW_EINVAL;
    if (running_in == running_out || sequences_in == sequences_out) return DW_EINVAL;
    if (B <= 0 || k < 1 || V <= 0 || eos < 0 || eos >= V || prompt_len < 1 || cur < prompt_len || cur >= max_length ||
        max_length > tok_ld) return DW_EINVAL;
    if (early_stopping < 0 || early_stopping > 2 || !(fin_div > 0.f) || !(hyp_div > 0.f)) return DW_EINVAL;
    if (k > BEAM_MAX_K || V > 16 * SEL_NT * 4 || (long)B * k > 65535) return DW_EUNSUP;
    hipLaunchKernelGGL(beam_update_kernel, dim3(1), dim3(BEAM_UP_NT), 0, (hipStream_t)stream, cand_val, cand_tok, B, k, V, cur,
                       prompt_len, max_length, eos, early_stopping, fin_div, hyp_div, run_scores, beam_scores, finished, lengths,
                       unsat, stop, src_rows, next_tok, plan);
    DW_CHECK_LAUNCH();
    hipLaunchKernelGGL(beam_move_rows_kernel, dim3(B * k), dim3(256), 0, (hipStream_t)stream, running_in, running_out,
                       sequences_in, sequences_out, (long)tok_ld, B * k, cur, plan);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
