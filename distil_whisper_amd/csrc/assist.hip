// Speculative (assisted) greedy decoding, the two launches of a round that are not decoder passes.
//
// Reference behaviour (third-party `transformers`, TF: = transformers/generation/): `_assisted_decoding` (TF:utils.py) with the
// greedy branch of `_speculative_sampling`'s caller -- the assistant drafts k tokens one at a time through the target's logits
// processors (TF:candidate_generator.py `AssistedCandidateGenerator.get_candidates`), the target scores the k + 1 positions in one
// pass, `n_matches = ((~(candidate_new_tokens == selected_tokens[:, :-1])).cumsum(-1) < 1).sum()` and the sequence grows by the
// matching drafts plus the target's own next token; reached from run_eval.py:578-599, 706-707 (`assistant_model=`).  What the
// host loop of decoding.assisted_greedy_decode did with a dozen torch ops and two synchronisations per round:
//
//   dw_assist_pick    the token the logits rules select at n consecutive positions of every row: the greedy walk of
//                     select_rules.h (greedy_pick, shared with decode.hip) over a (position, row) grid like score_tokens_kernel
//                     (score.hip), with no EOS bookkeeping.  Position j of row b is judged against the history
//                     tokens[b][0, L + j): for j > 0 that history holds the drafts, which the draft steps stored before this
//                     launch, so the n positions of a row are independent workgroups.  This file holds no rule and no walk of
//                     its own: which row and position, and where the token is written.
//   dw_assist_accept  the round's bookkeeping for the whole batch in one workgroup, one thread per row: the length of the
//                     agreeing draft prefix, its minimum over the rows, the accepted tokens with the finished rows filled.
//
// Both are plain kernels on the caller's stream: nothing is allocated, nothing synchronises, no workgroup waits for another.
// Cost model of the pick: that of greedy_pick (a row lives on one CU); n x B rows run side by side on the 256 CUs.
#include "common.h"
#include "select_rules.h"                           // SEL_NT, Best, every logits rule and the greedy walk
#include "../../include/dwamd.h"

struct AssistPickP {
    const bf16* logits; long ld, batch_rows;
    const uint8_t* suppress; const uint8_t* begin_suppress;
    int64_t* tokens; long tok_ld;
    int64_t* own; long own_ld;
    int64_t* cur;
    int V, L, P0, min_new, tb, max_initial, eos, store;
};

__global__ __launch_bounds__(SEL_NT) void assist_pick_kernel(const AssistPickP p) {
    __shared__ Best red[SEL_NT / 64];
    __shared__ float redf[SEL_NT / 64];
    __shared__ int redi[SEL_NT / 64];
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int V = p.V;
    int64_t* row_tok = p.tokens + (long)b * p.tok_ld;
    const int n = p.L + j;                          // the sequence index this workgroup fills
    const bf16* row = p.logits + ((long)b * p.batch_rows + j) * p.ld;
    const int first = n == p.P0;
    const RowRules rr = row_rules(row_tok, n, p.P0, p.tb, p.max_initial, V, p.eos, (n - p.P0) < p.min_new, redi);
    const Best pick = greedy_pick<false>(row, V, p.suppress, p.begin_suppress, first, rr, nullptr, nullptr, 1.0f, red, redf);
    if (tid == 0) {
        const long nxt = pick.i == 0x7fffffff ? 0 : pick.i;
        p.own[(long)b * p.own_ld + j] = nxt;
        if (p.store) {                              // the assistant's draft step (n == 1): the next pass reads it
            row_tok[n] = nxt;
            p.cur[b] = nxt;
        }
    }
}

extern "C" int dw_assist_pick(const void* logits, int B, int n, int V, int64_t ld, int64_t batch_rows, const uint8_t* suppress,
                              const uint8_t* begin_suppress, int min_new, int ts_begin, int max_initial, int64_t* tokens,
                              int64_t tok_ld, int L, int begin_index, int eos, int64_t* own, int64_t own_ld, int store,
                              int64_t* cur, void* stream) {
    DW_CLEAR_ERR();
    if (!tokens || !own || B <= 0 || B > 65535 || n <= 0 || L < 1 || begin_index < 1 || begin_index > L) return DW_EINVAL;
    if (batch_rows < n || own_ld < n || tok_ld < (int64_t)L + n - (store ? 0 : 1) || min_new < 0 || eos >= V) return DW_EINVAL;
    if (store && (n != 1 || !cur)) return DW_EINVAL;
    if (!select_args_ok(logits, V, ld, L, ts_begin, begin_index, eos)) return DW_EINVAL;
    AssistPickP p;
    p.logits = (const bf16*)logits; p.ld = (long)ld; p.batch_rows = (long)batch_rows;
    p.suppress = suppress; p.begin_suppress = begin_suppress;
    p.tokens = tokens; p.tok_ld = (long)tok_ld; p.own = own; p.own_ld = (long)own_ld; p.cur = cur;
    p.V = V; p.L = L; p.P0 = begin_index; p.min_new = min_new; p.tb = ts_begin; p.max_initial = max_initial; p.eos = eos;
    p.store = store;
    hipLaunchKernelGGL(assist_pick_kernel, dim3(n, B), dim3(SEL_NT), 0, (hipStream_t)stream, p);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// dw_assist_accept: thread b owns row b.  m_b = the leading drafts tokens[b][L + j], j < k, that equal own[b][j] (k for a
// finished row); n_ok = the minimum over the rows; then, in order, tokens[b][L + j] = done[b] ? fill : own[b][j] and
// done[b] |= that token == eos for j <= n_ok.  Rows and k are a few; the launch is latency, not work.
// ---------------------------------------------------------------------------------------------------------------------
#define ASSIST_MAX_B 1024
#define ASSIST_MAX_K 1024

__global__ __launch_bounds__(ASSIST_MAX_B) void assist_accept_kernel(const int64_t* own, long own_ld, int64_t* tokens, long tok_ld,
                                                                     int B, int L, int k, int eos, int fill, uint8_t* done,
                                                                     int32_t* result) {
    __shared__ int s_min, s_live;
    const int b = threadIdx.x;
    if (b == 0) { s_min = k; s_live = 0; }
    __syncthreads();
    const bool row = b < B;
    const int64_t* o = own + (long)b * own_ld;
    int64_t* t = tokens + (long)b * tok_ld + L;
    bool fin = false;
    if (row) {
        fin = eos >= 0 && done[b];
        int m = k;
        if (!fin) {
            m = 0;
            while (m < k && o[m] == t[m]) ++m;
        }
        if (m < k) atomicMin(&s_min, m);
    }
    __syncthreads();
    const int n_ok = s_min;
    if (row) {
        for (int j = 0; j <= n_ok; ++j) {
            const int64_t c = fin ? (int64_t)fill : o[j];
            t[j] = c;
            if (eos >= 0 && c == eos) fin = true;
        }
        if (eos >= 0) done[b] = fin ? 1 : 0;
        if (!fin) atomicOr(&s_live, 1);
    }
    __syncthreads();
    if (b == 0) {
        result[0] = n_ok;
        result[1] = (eos >= 0 && !s_live) ? 1 : 0;
    }
}

extern "C" int dw_assist_accept(const int64_t* own, int64_t own_ld, int64_t* tokens, int64_t tok_ld, int B, int L, int k, int eos,
                                int fill, uint8_t* done, int32_t* result, void* stream) {
    DW_CLEAR_ERR();
    if (!own || !tokens || !result || B <= 0 || L < 1 || k < 0 || (eos >= 0 && !done)) return DW_EINVAL;
    if (B > ASSIST_MAX_B || k > ASSIST_MAX_K) return DW_EUNSUP;
    if (own_ld < (int64_t)k + 1 || tok_ld < (int64_t)L + k + 1) return DW_EINVAL;
    hipLaunchKernelGGL(assist_accept_kernel, dim3(1), dim3((B + 63) / 64 * 64), 0, (hipStream_t)stream, own, (long)own_ld, tokens,
                       (long)tok_ld, B, L, k, eos, fill, done, result);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Per-row acceptance (decoding._assisted_rounds_device_rows): every row of the batch keeps its own length len[b] (int32 device
// array), its own agreeing prefix and its own end; one row's rejected draft costs the other rows nothing.  The decoder passes of
// such a round run at per-row positions (dw_decode_step_rows, decode.hip).
//   dw_assist_pick_rows    dw_assist_pick with the first judged position of row b = len[b] + j0 instead of the host's L: the same
//                          calls into select_rules.h, the position read from the device.
//   dw_assist_accept_rows  the round's bookkeeping, thread b owns row b: agreeing prefix, accepted tokens up to the row's own EOS
//                          or `total`, the new length, the start positions of the next round's passes for both models, the
//                          round's four result words.
// ---------------------------------------------------------------------------------------------------------------------
struct AssistPickRowsP {
    AssistPickP u;                                  // (u.L is not read: the position comes from len)
    const int32_t* len; int j0;
};

__global__ __launch_bounds__(SEL_NT) void assist_pick_rows_kernel(const AssistPickRowsP q) {
    __shared__ Best red[SEL_NT / 64];
    __shared__ float redf[SEL_NT / 64];
    __shared__ int redi[SEL_NT / 64];
    const AssistPickP& p = q.u;
    const int j = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int V = p.V;
    int64_t* row_tok = p.tokens + (long)b * p.tok_ld;
    const int n = max(q.len[b], p.P0) + q.j0 + j;     // the sequence index this workgroup fills
    if (n >= p.tok_ld) {                            // behind the buffer: a row that has ended (its pick is never read)
        if (tid == 0) p.own[(long)b * p.own_ld + j] = 0;
        return;
    }
    const bf16* row = p.logits + ((long)b * p.batch_rows + j) * p.ld;
    const int first = n == p.P0;
    const RowRules rr = row_rules(row_tok, n, p.P0, p.tb, p.max_initial, V, p.eos, (n - p.P0) < p.min_new, redi);
    const Best pick = greedy_pick<false>(row, V, p.suppress, p.begin_suppress, first, rr, nullptr, nullptr, 1.0f, red, redf);
    if (tid == 0) {
        const long nxt = pick.i == 0x7fffffff ? 0 : pick.i;
        p.own[(long)b * p.own_ld + j] = nxt;
        if (p.store) {                              // the assistant's draft step (n == 1): the next pass reads it
            row_tok[n] = nxt;
            p.cur[b] = nxt;
        }
    }
}

extern "C" int dw_assist_pick_rows(const void* logits, int B, int n, int V, int64_t ld, int64_t batch_rows, const uint8_t* suppress,
                                   const uint8_t* begin_suppress, int min_new, int ts_begin, int max_initial, int64_t* tokens,
                                   int64_t tok_ld, const int32_t* len, int j0, int begin_index, int eos, int64_t* own,
                                   int64_t own_ld, int store, int64_t* cur, void* stream) {
    DW_CLEAR_ERR();
    if (!tokens || !own || !len || B <= 0 || B > 65535 || n <= 0 || j0 < 0 || begin_index < 1) return DW_EINVAL;
    if (batch_rows < n || own_ld < n || tok_ld < (int64_t)begin_index + 1 || tok_ld > 0x7fffffff || min_new < 0 || eos >= V)
        return DW_EINVAL;
    if (store && (n != 1 || !cur)) return DW_EINVAL;
    if (!select_args_ok(logits, V, ld, begin_index, ts_begin, begin_index, eos)) return DW_EINVAL;
    AssistPickRowsP q;
    AssistPickP& p = q.u;
    p.logits = (const bf16*)logits; p.ld = (long)ld; p.batch_rows = (long)batch_rows;
    p.suppress = suppress; p.begin_suppress = begin_suppress;
    p.tokens = tokens; p.tok_ld = (long)tok_ld; p.own = own; p.own_ld = (long)own_ld; p.cur = cur;
    p.V = V; p.L = 0; p.P0 = begin_index; p.min_new = min_new; p.tb = ts_begin; p.max_initial = max_initial; p.eos = eos;
    p.store = store;
    q.len = len; q.j0 = j0;
    hipLaunchKernelGGL(assist_pick_rows_kernel, dim3(n, B), dim3(SEL_NT), 0, (hipStream_t)stream, q);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// dw_assist_accept_rows: thread b owns row b, whose drafts stand at tokens[b][len[b], len[b] + k).  A live row: m_b = the leading
// drafts that equal own[b][j]; for j = 0 .. m_b in order tokens[b][len[b] + j] = own[b][j], the row ending behind an EOS or at
// `total`; len[b] = its new length.  A row that has ended (now or before) takes `fill` behind its end as far as this round's drafts
// went, and is parked at position 0 for the passes to come.  Rows and k are a few; the launch is latency, not work.
__global__ __launch_bounds__(ASSIST_MAX_B) void assist_accept_rows_kernel(const int64_t* own, long own_ld, int64_t* tokens, long tok_ld,
                                                                          int B, int k, int total, int eos, int fill, int32_t* len,
                                                                          uint8_t* done, int32_t* pos_t, int32_t* pos_a,
                                                                          int32_t* result) {
    __shared__ int s_acc, s_off, s_live, s_max;
    const int b = threadIdx.x;
    if (b == 0) { s_acc = 0; s_off = 0; s_live = 0; s_max = 0; }
    __syncthreads();
    if (b < B) {
        const int64_t* o = own + (long)b * own_ld;
        int64_t* t = tokens + (long)b * tok_ld;
        int L = min(max(len[b], 1), total);
        bool fin = done[b] != 0 || L >= total;
        const int end = min(L + k, total - 1);      // the last position this round's drafts or the target's token can have reached
        if (!fin) {
            const int kb = end - L;                 // drafts offered to this row (k for a live row: the caller sized k so)
            int m = 0;
            while (m < kb && o[m] == t[L + m]) ++m;
            int w = 0;                              // tokens written
            while (w <= m) {
                const int64_t c = o[w];
                t[L + w] = c;
                ++w;
                if (eos >= 0 && c == eos) { fin = true; break; }
            }
            atomicAdd(&s_acc, min(w, m));
            atomicAdd(&s_off, kb);
            L += w;
            if (L >= total) fin = true;
            len[b] = L;
        }
        if (fin) {
            for (int i = L; i <= end; ++i) t[i] = fill;
        } else {
            atomicOr(&s_live, 1);
            atomicMax(&s_max, L);
        }
        done[b] = fin ? 1 : 0;
        pos_t[b] = fin ? 0 : L - 1;                 // the target's cache is valid below len - 1, the assistant's below len - 2
        pos_a[b] = fin ? 0 : L - 2;
    }
    __syncthreads();
    if (b == 0) {
        result[0] = s_acc;
        result[1] = s_off;
        result[2] = s_live ? 0 : 1;
        result[3] = s_max;
    }
}

extern "C" int dw_assist_accept_rows(const int64_t* own, int64_t own_ld, int64_t* tokens, int64_t tok_ld, int B, int k, int total,
                                     int eos, int fill, int32_t* len, uint8_t* done, int32_t* pos_target, int32_t* pos_assistant,
                                     int32_t* result, void* stream) {
    DW_CLEAR_ERR();
    if (!own || !tokens || !len || !done || !pos_target || !pos_assistant || !result || B <= 0 || k < 0 || total < 2)
        return DW_EINVAL;
    if (B > ASSIST_MAX_B || k > ASSIST_MAX_K) return DW_EUNSUP;
    if (own_ld < (int64_t)k + 1 || tok_ld < (int64_t)total) return DW_EINVAL;
    hipLaunchKernelGGL(assist_accept_rows_kernel, dim3(1), dim3((B + 63) / 64 * 64), 0, (hipStream_t)stream, own, (long)own_ld,
                       tokens, (long)tok_ld, B, k, total, eos, fill, len, done, pos_target, pos_assistant, result);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
