// The slot step of continuous batching (decoding.SlotDecoder): the token selection of a batch whose rows -- slots -- stand at
// different positions of different windows.  Where greedy_select_kernel (decode.hip) takes the position n, the prompt length and
// the forced / first / no-EOS flags of a step as host arguments that hold for the whole batch, a slot carries them as device
// state: len (tokens held = the position this step fills), plen (prompt length, the begin_index of the rules), budget (plen +
// max_new_tokens), done.  One 1024-thread workgroup per slot reads its logits row -- the output of the pass that fed `cur` at
// position `row_t` (dw_decode_token_rows) -- and
//   * a slot that is done (finished, or never filled) is left alone and parked: row_t = 0, cur = tokens[b][0], so the next pass
//     rewrites position 0 of the slot's own cache and nothing else;
//   * inside the prompt (len < plen) the token is forced: nxt = tokens[b][len];
//   * otherwise nxt is the row's best allowed column under the rules of select_rules.h (row_rules + greedy_pick<false>, the walk of
//     greedy_select_kernel<false>) with the history [0, len), first = (len == plen), no_eos = (len - plen < min_new);
//   * tokens[b][len] = nxt, len += 1; a generated EOS or a spent budget sets done and parks the slot, else row_t = len - 1 and
//     cur = nxt feed the next pass.
// No argument depends on a position, nothing is allocated and no workgroup waits for another: the pass plus this launch replay
// from one HIP graph whatever the slots hold, and the host reads done / len only when it wants to refill.
#include "common.h"
#include "select_rules.h"
#include "../../include/dwamd.h"

// The scores of a window (SCORES; dw_slot_step_scores) -- what the seek loop's thresholds ask for, taken while the step holds the row:
//   * lp_sum[b] += s[nxt] - logsumexp(s) on every generated step, s = the processed row the pick has just judged: an excluded
//     column is -inf, and so is every text column once the mass rule has taken a timestamp.  The pick is the row's largest
//     allowed value, so the term is -log(sum exp(s - s[nxt])): one more walk over the row (row_sum_exp), which the L2 still
//     holds.  The mass rule has taken the text columns exactly when the pick is a timestamp: a timestamp that beats the best
//     text logit on its own carries the rule with it (logsumexp >= max).  A row with no allowed column adds nothing.
//   * nsp[b] = softmax(row)[nsp_col] on the step whose row is the output of input position nsp_pos[b] (len - 1 == nsp_pos[b]):
//     over the raw row when the step is forced (a prompt of several start tokens; the only forced step that reads logits), over
//     the processed row when it is generated (the first step behind a one-token prompt).
// The instance without SCORES is the kernel as it stood: every addition sits behind `if constexpr`.
template <bool RAW>
__device__ __forceinline__ float row_sum_exp(const bf16* row, int V, const uint8_t* suppress, const uint8_t* begin_suppress, int first,
                                             const RowRules& rr, bool mask_text, float M, float* redf) {
    const int tid = threadIdx.x;
    const bool word_masks = (((uintptr_t)suppress | (uintptr_t)begin_suppress) & 3) == 0;
    float sum = 0.f;
    auto add = [&](int c0, const bf16x4& x, unsigned mask, bool live) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const bool a = RAW ? (live && c0 + e < V) : (column_allowed(rr, c0, e, V, mask, 0, live) && !(mask_text && c0 + e < rr.tsb));
            if (a) sum += __expf(bf2f(x[e]) - M);
        }
    };
    constexpr int NPRE = 13;                           // as greedy_pick: the row is requested before anything is summed
    if (V <= NPRE * SEL_NT * 4) {
        const int clast = (V - 1) & ~3;
        bf16x4 xr[NPRE];
        unsigned mr[NPRE];
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int c0 = min(tid * 4 + i * SEL_NT * 4, clast);
            xr[i] = *(const bf16x4*)(row + c0);
            mr[i] = RAW ? 0u : rule_masks_of(suppress, begin_suppress, first, word_masks, c0, V);
        }
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int c0 = tid * 4 + i * SEL_NT * 4;
            add(min(c0, clast), xr[i], mr[i], c0 < V);
        }
    } else {
        for (int c0 = tid * 4; c0 < V; c0 += SEL_NT * 4)
            add(c0, *(const bf16x4*)(row + c0), RAW ? 0u : rule_masks_of(suppress, begin_suppress, first, word_masks, c0, V), true);
    }
    return block_sum<SEL_NT>(sum, redf);
}
// the largest value of the raw row (the softmax of a forced step)
__device__ __forceinline__ float row_max_raw(const bf16* row, int V, float* redf) {
    float m = -INFINITY;
    for (int c0 = threadIdx.x * 4; c0 < V; c0 += SEL_NT * 4) {
        const bf16x4 x = *(const bf16x4*)(row + c0);
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c0 + e < V) m = fmaxf(m, bf2f(x[e]));
    }
    return block_max<SEL_NT>(m, redf);
}

template <bool SCORES>
__global__ __launch_bounds__(SEL_NT) void slot_step_kernel(const bf16* logits, int V, long ld, const uint8_t* suppress,
                                                           const uint8_t* begin_suppress, int tb, int max_initial, int eos, int min_new,
                                                           int64_t* tokens, long tok_ld, int32_t* len, const int32_t* plen,
                                                           const int32_t* budget, uint8_t* done, int32_t* row_t, int64_t* cur,
                                                           float* lp_sum, float* nsp, const int32_t* nsp_pos, int nsp_col) {
    __shared__ Best red[SEL_NT / 64];
    __shared__ float redf[SEL_NT / 64];
    __shared__ int redi[SEL_NT / 64];
    const int b = blockIdx.x, tid = threadIdx.x;
    int64_t* row_tok = tokens + (long)b * tok_ld;
    const int n = len[b], P = plen[b];
    const bool parked = done[b] != 0;
    __syncthreads();                               // every thread holds the slot's state before thread 0 moves it
    if (parked || n < 1 || n >= tok_ld || P < 1) { // (a state no refill leaves behind parks the slot as well: nothing is written past the row)
        if (tid == 0) { done[b] = 1; row_t[b] = 0; cur[b] = row_tok[0]; }
        return;
    }
    const bool forced = n < P;                     // position n still belongs to the prompt (teacher forcing)
    long nxt = 0;
    if (!forced) {
        const RowRules rr = row_rules(row_tok, n, P, tb, max_initial, V, eos, n - P < min_new, redi);
        const Best pick = greedy_pick<false>(logits + (long)b * ld, V, suppress, begin_suppress, n == P, rr, nullptr, nullptr, 1.0f, red,
                                             redf);
        nxt = pick.i == 0x7fffffff ? 0 : pick.i;
        if constexpr (SCORES) {
            if (pick.i != 0x7fffffff) {            // (uniform: every thread holds the same pick)
                const bf16* row = logits + (long)b * ld;
                const bool mask_text = rr.ts_mode && pick.i >= rr.tsb;
                const float sum = row_sum_exp<false>(row, V, suppress, begin_suppress, n == P, rr, mask_text, pick.v, redf);
                if (tid == 0) {
                    const float lse = pick.v + logf(sum);          // (the pick itself is in the sum: sum >= 1)
                    lp_sum[b] += pick.v - lse;
                    if (nsp_col >= 0 && n - 1 == nsp_pos[b]) {
                        const bool a = column_allowed(rr, nsp_col, 0, V, (suppress && suppress[nsp_col]) ||
                                                      (n == P && begin_suppress && begin_suppress[nsp_col])) &&
                                       !(mask_text && nsp_col < rr.tsb);
                        nsp[b] = a ? __expf(bf2f(row[nsp_col]) - lse) : 0.f;
                    }
                }
            }
        }
    } else if constexpr (SCORES) {
        if (nsp_col >= 0 && n - 1 == nsp_pos[b]) { // (uniform) the one forced step that reads its row
            const bf16* row = logits + (long)b * ld;
            RowRules none;                         // (not read by the raw sum)
            none.tsb = V + 1;
            const float M = row_max_raw(row, V, redf);
            const float sum = row_sum_exp<true>(row, V, nullptr, nullptr, 0, none, false, M, redf);
            if (tid == 0) nsp[b] = __expf(bf2f(row[nsp_col]) - (M + logf(sum)));
        }
    }
    if (tid == 0) {
        if (forced) nxt = row_tok[n];
        row_tok[n] = nxt;
        len[b] = n + 1;
        if (!forced && (nxt == eos || n + 1 >= budget[b])) {
            done[b] = 1; row_t[b] = 0; cur[b] = row_tok[0];
        } else {
            row_t[b] = n; cur[b] = nxt;
        }
    }
}

static int slot_step_args(const void* logits, int S, int V, int64_t ld, int ts_begin, int eos, int64_t* tokens, int64_t tok_ld,
                          int32_t* len, const int32_t* plen, const int32_t* budget, uint8_t* done, int32_t* row_t, int64_t* cur) {
    if (!tokens || !len || !plen || !budget || !done || !row_t || !cur || S <= 0 || S > 65535 || tok_ld < 2) return DW_EINVAL;
    if ((((uintptr_t)len | (uintptr_t)plen | (uintptr_t)budget | (uintptr_t)row_t) & 3) || (((uintptr_t)tokens | (uintptr_t)cur) & 7))
        return DW_EINVAL;
    if (!logits || V <= 0 || ld < V || (ld & 3) || ((uintptr_t)logits & 7) || (ts_begin >= 0 && eos < 0)) return DW_EINVAL;
    return DW_OK;
}

extern "C" int dw_slot_step(const void* logits, int S, int V, int64_t ld, const uint8_t* suppress, const uint8_t* begin_suppress,
                            int ts_begin, int max_initial, int eos, int min_new, int64_t* tokens, int64_t tok_ld, int32_t* len,
                            const int32_t* plen, const int32_t* budget, uint8_t* done, int32_t* row_t, int64_t* cur, void* stream) {
    DW_CLEAR_ERR();
    if (slot_step_args(logits, S, V, ld, ts_begin, eos, tokens, tok_ld, len, plen, budget, done, row_t, cur) != DW_OK) return DW_EINVAL;
    hipLaunchKernelGGL(slot_step_kernel<false>, dim3(S), dim3(SEL_NT), 0, (hipStream_t)stream, (const bf16*)logits, V, (long)ld, suppress,
                       begin_suppress, ts_begin, max_initial, eos, min_new, tokens, (long)tok_ld, len, plen, budget, done, row_t, cur,
                       (float*)nullptr, (float*)nullptr, (const int32_t*)nullptr, -1);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

extern "C" int dw_slot_step_scores(const void* logits, int S, int V, int64_t ld, const uint8_t* suppress, const uint8_t* begin_suppress,
                                   int ts_begin, int max_initial, int eos, int min_new, int64_t* tokens, int64_t tok_ld, int32_t* len,
                                   const int32_t* plen, const int32_t* budget, uint8_t* done, int32_t* row_t, int64_t* cur,
                                   float* lp_sum, float* nsp, const int32_t* nsp_pos, int nsp_col, void* stream) {
    DW_CLEAR_ERR();
    if (slot_step_args(logits, S, V, ld, ts_begin, eos, tokens, tok_ld, len, plen, budget, done, row_t, cur) != DW_OK) return DW_EINVAL;
    if (!lp_sum || ((uintptr_t)lp_sum & 3) || nsp_col >= V) return DW_EINVAL;
    if (nsp_col >= 0 && (!nsp || !nsp_pos || (((uintptr_t)nsp | (uintptr_t)nsp_pos) & 3))) return DW_EINVAL;
    hipLaunchKernelGGL(slot_step_kernel<true>, dim3(S), dim3(SEL_NT), 0, (hipStream_t)stream, (const bf16*)logits, V, (long)ld, suppress,
                       begin_suppress, ts_begin, max_initial, eos, min_new, tokens, (long)tok_ld, len, plen, budget, done, row_t, cur,
                       lp_sum, nsp, nsp_pos, nsp_col < 0 ? -1 : nsp_col);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
