// Device code shared by the token-selection kernels (decode.hip: greedy / history / sampled selection; beam.hip: beam-search
// candidates): the workgroup shape, the (value, index) reduction, and the row state of the reference's logits rules
// (MinNewTokensLength, SuppressTokens, SuppressTokensAtBegin and WhisperTimeStampLogitsProcessor, TF:generation/logits_process.py)
// as two allowed id intervals plus two single banned ids.
#pragma once
#include "common.h"

#define SEL_NT 1024

struct Best { float v; int i; };
__device__ __forceinline__ Best better(Best a, Best b) {      // larger value wins, ties go to the smaller index
    return (b.v > a.v || (b.v == a.v && b.i < a.i)) ? b : a;
}
__device__ __forceinline__ Best block_best(Best x, Best* red) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        Best y; y.v = __shfl_xor(x.v, o); y.i = __shfl_xor(x.i, o);
        x = better(x, y);
    }
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    __syncthreads();
    if (lane == 0) red[wave] = x;
    __syncthreads();
    Best t = red[0];
    for (int i = 1; i < SEL_NT / 64; ++i) t = better(t, red[i]);
    return t;
}

// Every rule is a predicate on the column alone once the row state is known: column c may be selected iff it lies in
// [tlo, thi) (text / special ids below the first timestamp) or [slo, shi) (timestamp ids), is neither ban_eos nor ban_nots,
// and no byte mask names it.  tsb: first timestamp id (beyond the vocabulary when the timestamp rules are off).
struct RowRules {
    bool ts_mode;
    int tsb, tlo, thi, slo, shi, ban_eos, ban_nots;
    __device__ __forceinline__ bool in_range(int c) const {
        return ((c >= tlo && c < thi) || (c >= slo && c < shi)) && c != ban_eos && c != ban_nots;
    }
};

// Called by all SEL_NT threads of the workgroup (it synchronises when the timestamp rules are on).  row_tok: the row's sequence,
// of which [0, n) is the history (decoder prompt of begin_index tokens included); tb = no_timestamps_token_id + 1 (< 0: rules
// off); max_initial < 0: none; redi: SEL_NT / 64 ints of LDS.
__device__ __forceinline__ RowRules row_rules(const int64_t* row_tok, int n, int begin_index, int tb, int max_initial, int V,
                                              int eos, int no_eos, int* redi) {
    const int tid = threadIdx.x;
    RowRules r;
    r.ts_mode = tb >= 0;
    const int tsb = r.ts_mode ? tb : V + 1;
    r.tsb = tsb;
    // ---- row state of the timestamp rules (WhisperTimeStampLogitsProcessor) ----
    bool last_ts = false, pen_ts = true, any_ts = false;
    int ts_last = 0;
    const int L = n - begin_index;
    if (r.ts_mode && L >= 1) {
        last_ts = row_tok[n - 1] >= tsb;
        pen_ts = L >= 2 ? row_tok[n - 2] >= tsb : true;
        int pos = 0;                               // 1-based position (within the generated part) of the last timestamp
        for (int i = tid; i < L; i += SEL_NT) pos = row_tok[begin_index + i] >= tsb ? max(pos, i + 1) : pos;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) pos = max(pos, __shfl_xor(pos, o));
        if ((tid & 63) == 0) redi[tid >> 6] = pos;
        __syncthreads();
        pos = 0;
        for (int i = 0; i < SEL_NT / 64; ++i) pos = max(pos, redi[i]);
        any_ts = pos > 0;
        if (any_ts) {
            const int last_val = (int)row_tok[begin_index + pos - 1];
            ts_last = (last_ts && !pen_ts) ? last_val : last_val + 1;
        }
    }
    r.tlo = 0; r.thi = r.ts_mode ? tsb : V; r.slo = V; r.shi = V;       // allowed: [tlo, thi) and [slo, shi)
    r.ban_eos = no_eos ? eos : -1;
    r.ban_nots = r.ts_mode ? tsb - 1 : -1;
    if (r.ts_mode) {
        if (L >= 1) {
            if (last_ts && pen_ts) { r.slo = r.shi = V; }                       // after a closed pair: text only
            else {
                r.slo = any_ts ? max(tsb, ts_last) : tsb;                        // timestamps never decrease
                if (last_ts) r.tlo = eos;                                       // after text + timestamp: timestamp / EOS
            }
        } else {
            r.tlo = r.thi = 0;                                                  // the first sampled token is a timestamp
            r.slo = tsb;
            r.shi = max_initial >= 0 ? min(V, tsb + max_initial + 1) : V;
        }
    }
    return r;
}

// The suppress / begin-suppress byte masks of the four columns c0 .. c0 + 3 (c0 a multiple of 4): byte e != 0 means column
// c0 + e is suppressed.  word_masks: both masks are 4-byte aligned (one 32-bit load each).
__device__ __forceinline__ unsigned rule_masks_of(const uint8_t* suppress, const uint8_t* begin_suppress, int first, bool word_masks,
                                                  int c0, int V) {
    unsigned mask = 0;
    if (word_masks && c0 + 3 < V) {                 // (uniform except in the last chunk of a row)
        if (suppress) mask |= *(const unsigned*)(suppress + c0);
        if (first && begin_suppress) mask |= *(const unsigned*)(begin_suppress + c0);
    } else {
#pragma unroll
        for (int e = 0; e < 4; ++e)
            if (c0 + e < V && ((suppress && suppress[c0 + e]) || (first && begin_suppress && begin_suppress[c0 + e])))
                mask |= 0xffu << (8 * e);
    }
    return mask;
}
