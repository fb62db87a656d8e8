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

__global__ __launch_bounds__(SEL_NT) void slot_step_kernel(const bf16* logits, int V, long ld, const uint8_t* suppress,
                                                           const uint8_t* begin_suppress, int tb, int max_initial, int eos, int min_new,
                                                           int64_t* tokens, long tok_ld, int32_t* len, const int32_t* plen,
                                                           const int32_t* budget, uint8_t* done, int32_t* row_t, int64_t* cur) {
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

extern "C" int dw_slot_step(const void* logits, int S, int V, int64_t ld, const uint8_t* suppress, const uint8_t* begin_suppress,
                            int ts_begin, int max_initial, int eos, int min_new, int64_t* tokens, int64_t tok_ld, int32_t* len,
                            const int32_t* plen, const int32_t* budget, uint8_t* done, int32_t* row_t, int64_t* cur, void* stream) {
    DW_CLEAR_ERR();
    if (!tokens || !len || !plen || !budget || !done || !row_t || !cur || S <= 0 || S > 65535 || tok_ld < 2) return DW_EINVAL;
    if ((((uintptr_t)len | (uintptr_t)plen | (uintptr_t)budget | (uintptr_t)row_t) & 3) || (((uintptr_t)tokens | (uintptr_t)cur) & 7))
        return DW_EINVAL;
    if (!logits || V <= 0 || ld < V || (ld & 3) || ((uintptr_t)logits & 7) || (ts_begin >= 0 && eos < 0)) return DW_EINVAL;
    hipLaunchKernelGGL(slot_step_kernel, dim3(S), dim3(SEL_NT), 0, (hipStream_t)stream, (const bf16*)logits, V, (long)ld, suppress,
                       begin_suppress, ts_begin, max_initial, eos, min_new, tokens, (long)tok_ld, len, plen, budget, done, row_t, cur);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
