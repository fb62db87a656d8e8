// The one statement of the reference's logits rules (MinNewTokensLength, SuppressTokens, SuppressTokensAtBegin and
// WhisperTimeStampLogitsProcessor, TF:generation/logits_process.py; RepetitionPenalty / NoRepeatNGram as history bitmaps) for the
// kernels that apply them -- decode.hip: greedy / history / sampled selection; beam.hip: beam-search candidates; score.hip: scores
// of finished sequences; assist.hip: the picks of a speculative round -- with the workgroup shape and the (value, index) reduction
// they share.  A rule changes here and nowhere else: the row state as two allowed id intervals plus two single banned ids
// (row_rules), the byte masks (rule_masks_of), the history bitmaps (build_history_bitmaps), the sequence-bias table
// (build_bias_bitmaps / bias_of), the clean-chunk test (classify_chunk) and the per-column predicate (column_allowed).  What the
// kernels keep to themselves is arithmetic: how they hold a row and in which order they sum -- except the kernels that keep
// only a row's argmax (greedy_select_kernel<false / true>, greedy_select_bias_kernel, assist.hip's assist_pick_kernel): their
// walk over the row is greedy_pick below, once.
#pragma once
#include "common.h"

#define SEL_NT 1024
#define SEL_HIST_V 65536                            // capacity of a history bitmap in columns (8 KB of LDS each)
#define SEL_BIAS_S 1024                             // most sequences of a bias table: one thread each (8 KB of LDS)

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
// and no byte mask names it (column_allowed below).  tsb: first timestamp id (beyond the vocabulary when the timestamp rules are off).
struct RowRules {
    bool ts_mode;
    int tsb, tlo, thi, slo, shi, ban_eos, ban_nots;
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

// The history bitmaps of RepetitionPenaltyLogitsProcessor and NoRepeatNGramLogitsProcessor, one bit per column, from the history
// row_tok[0, n) (decoder prompt included): `seen` -- the id occurs (built only when rep_pen != 1); `banned` -- the id would
// complete an n-gram of length `ngram` that the row already holds (ngram = 0: off).  Called by all SEL_NT threads; both bitmaps
// are SEL_HIST_V / 32 words of LDS, complete on return.
__device__ __forceinline__ void build_history_bitmaps(const int64_t* row_tok, int n, int V, float rep_pen, int ngram, unsigned* seen,
                                                      unsigned* banned) {
    const int tid = threadIdx.x;
    for (int w = tid; w < SEL_HIST_V / 32; w += SEL_NT) { seen[w] = 0u; banned[w] = 0u; }
    __syncthreads();
    const int g = ngram;
    for (int i = tid; i < n; i += SEL_NT) {
        const long t = row_tok[i];
        if (t < 0 || t >= V) continue;                                  // (no column: nothing to mark)
        const unsigned bit = 1u << ((int)t & 31);
        if (rep_pen != 1.0f) atomicOr(&seen[(int)t >> 5], bit);
        if (g > 0 && i >= g - 1) {                                      // tokens[i] followed the window [i - g + 1, i)
            bool hit = true;                                            // (n >= g here; g = 1: an empty window)
            for (int k = 1; k < g && hit; ++k) hit = row_tok[i - k] == row_tok[n - k];
            if (hit) atomicOr(&banned[(int)t >> 5], bit);
        }
    }
    __syncthreads();
}
// bit e: column c0 + e is set in the bitmap (c0 a multiple of 4, below SEL_HIST_V)
__device__ __forceinline__ unsigned history_bits_of(const unsigned* bitmap, int c0) { return (bitmap[c0 >> 5] >> (c0 & 31)) & 0xfu; }

// The table of SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor (`generate(sequence_bias=, bad_words_ids=)`), flattened by
// the host (decoding.sequence_bias_table): sequence s is tok[off[s], off[s + 1]) with the bias val[s] for the column of its last
// token.  The host hands the S <= SEL_BIAS_S sequences (of at most 32 tokens: its cap, no
// code here depends on a length) over ordered by that column (within a column in the caller's order, the
// one-token entry first, duplicates of one-token entries already resolved by assignment, `[eos]` bad words already dropped).
struct BiasTable { const int* tok; const int* off; const float* val; int S; };

// The reference's rule: a sequence of one token always counts; a longer one is ignored when it is longer than the history
// (len > n), else it counts iff the last len - 1 tokens of the history row_tok[0, n) (decoder prompt included; nothing at or
// beyond n is read) equal its prefix.  All biases of a column are summed first -- here by the thread of the column's first table
// entry, over the column's entries in table order (a sequence that does not count adds 0.0, as the reference's `where` does), so
// the sum does not depend on the arrival order of anything: no floating-point atomics -- and the sum is added to the logit once.
// On return col[s] holds the column of sequence s (ascending), sum[s] the merged bias where s is the first entry of its column;
// a column whose sum is -inf is ORed into `banned` (complete before the call: build_history_bitmaps), one whose sum is another
// non-zero value is set in `biased` (SEL_HIST_V / 32 words, built here).  Called by all SEL_NT threads; col / sum: SEL_BIAS_S
// entries of LDS each.  (Worst case: all S entries name one column and one thread adds S values, ~1 us per 30 entries.)
__device__ __forceinline__ void build_bias_bitmaps(const int64_t* row_tok, int n, int V, const BiasTable& t, unsigned* banned,
                                                   unsigned* biased, int* col, float* sum) {
    const int tid = threadIdx.x;
    for (int w = tid; w < SEL_HIST_V / 32; w += SEL_NT) biased[w] = 0u;
    int c = -1;
    if (tid < t.S) {
        const int o0 = t.off[tid], len = t.off[tid + 1] - o0;
        c = t.tok[o0 + len - 1];
        bool hit = len <= n;                                            // (n >= 1: a one-token sequence always counts)
        for (int k = 0; k < len - 1 && hit; ++k) hit = row_tok[n - (len - 1) + k] == (int64_t)t.tok[o0 + k];
        col[tid] = c;
        sum[tid] = hit ? t.val[tid] : 0.f;
    }
    __syncthreads();
    if (tid < t.S && (tid == 0 || col[tid - 1] != c)) {                 // the first entry of its column adds the column up
        float v = sum[tid];
        for (int s = tid + 1; s < t.S && col[s] == c; ++s) v += sum[s];
        sum[tid] = v;                                                   // (no other thread reads this column's entries)
        if (c >= 0 && c < V) {
            if (v == -INFINITY) atomicOr(&banned[c >> 5], 1u << (c & 31));
            else if (v != 0.f) atomicOr(&biased[c >> 5], 1u << (c & 31));
        }
    }
    __syncthreads();
}
// the merged bias of column c, whose `biased` bit is set: the first table entry of that column (col ascending: lower bound)
__device__ __forceinline__ float bias_of(const int* col, const float* sum, int S, int c) {
    int lo = 0, hi = S;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (col[mid] < c) lo = mid + 1; else hi = mid;
    }
    return sum[lo];
}

// The four columns c0 .. c0 + 3 (c0 a multiple of 4) as a whole.  clean: all four exist (`live`: the chunk is no clamped repeat
// of the row's last one), lie inside ONE allowed interval, and no mask byte, banned id or history bit (sbits / bbits of
// history_bits_of: seen -- or biased, which reads the same here -- / banned; 0 without history rules) names any of them -- each
// column then keeps its logit and counts as text (in_text) or timestamp.  A chunk that is not clean is judged column by column
// with column_allowed.
struct ChunkKind { bool clean, in_text; };
__device__ __forceinline__ ChunkKind classify_chunk(const RowRules& r, unsigned mask, bool live, int c0, int V, unsigned sbits = 0,
                                                    unsigned bbits = 0) {
    const int c3 = c0 + 3;
    const bool in_text = c0 >= r.tlo && c3 < r.thi, in_ts = c0 >= r.slo && c3 < r.shi;
    const bool inside = live && mask == 0 && c3 < V && (in_text || in_ts) && !(r.ban_eos >= c0 && r.ban_eos <= c3) &&
                        !(r.ban_nots >= c0 && r.ban_nots <= c3);
    return {inside && (sbits | bbits) == 0, in_text};
}

// Column c = c0 + e may be selected: it exists (c < V, and `live`: its chunk is no clamped repeat of the row's last one), byte e
// of `mask` (rule_masks_of) is clear, the row state allows it, and bit e of `bbits` (history_bits_of(banned); 0 without history
// rules) is clear.  For one column on its own: e = 0 with its byte and bit.  (The whole condition in one chain on purpose: as the
// tail of a caller's `live && c < V && ...` greedy_select_kernel<true> ran 0.2-0.4 us slower, profiles/select_rules_refactor.md.)
__device__ __forceinline__ bool column_allowed(const RowRules& r, int c0, int e, int V, unsigned mask, unsigned bbits = 0,
                                               bool live = true) {
    const int c = c0 + e;
    return live && c < V && !((mask >> (8 * e)) & 0xffu) && ((c >= r.tlo && c < r.thi) || (c >= r.slo && c < r.shi)) &&
           c != r.ban_eos && c != r.ban_nots && !((bbits >> e) & 1u);
}

// The greedy walk: the row's best allowed column under every rule above -- Best{value, column}, column 0x7fffffff when no column
// is allowed -- for the kernels that keep nothing of a row but its argmax (decode.hip greedy_select_kernel<HIST>, assist.hip
// assist_pick_kernel).  Called by all SEL_NT threads.  row: V bf16 logits, 8-byte aligned; begin_suppress counts only when
// `first` (tested at each use: with the pointer nulled instead greedy_select_kernel<true> ran 0.15 us slower,
// profiles/greedy_walk_refactor.md); HIST: seen / banned are the complete bitmaps of build_history_bitmaps and a seen column
// takes RepetitionPenaltyLogitsProcessor's v < 0 ? v * rep_pen : v / rep_pen (all three unused without HIST); red / redf:
// SEL_NT / 64 entries of LDS each.  BIAS (with HIST): biased / bcol / bsum / S are what build_bias_bitmaps left -- a biased
// column is judged as penal?(x + bias): SequenceBiasLogitsProcessor stands in front of the repetition penalty in the reference's
// list, and the banned bitmap already holds the bad words -- in both passes; the instances without BIAS compile as before.
// Pass 1 keeps the best allowed text token and the best allowed timestamp token, pass 2 (timestamp rules only) sums the
// timestamp probability mass for the "timestamps together beat the best text token" rule.  A row lives on ONE CU (one
// workgroup), so the walk is bound by instructions per column, not by bytes: a chunk of four columns that classify_chunk calls
// clean (almost every chunk) takes the short path of `judge` -- a compare and two selects per column; ascending order within a
// thread makes the strict compare keep the smallest index among equal values, better() does the same everywhere else.
template <bool HIST, bool BIAS = false>
__device__ __forceinline__ Best greedy_pick(const bf16* row, int V, const uint8_t* suppress, const uint8_t* begin_suppress, int first,
                                            const RowRules& rr, const unsigned* seen, const unsigned* banned, float rep_pen,
                                            Best* red, float* redf, const unsigned* biased = nullptr, const int* bcol = nullptr,
                                            const float* bsum = nullptr, int S = 0) {
    static_assert(HIST || !BIAS, "the bias table comes with the history bitmaps");
    const int tid = threadIdx.x;
    const int tsb = rr.tsb;
    auto penal = [&](float v) -> float { return v < 0.f ? v * rep_pen : v / rep_pen; };
    auto allowed = [&](int c) -> bool {               // (one column on its own: the probability-mass pass below)
        const unsigned masked = (suppress && suppress[c]) || (first && begin_suppress && begin_suppress[c]);
        unsigned ban = 0;
        if constexpr (HIST) ban = banned[c >> 5] >> (c & 31);
        return column_allowed(rr, c, 0, V, masked, ban);
    };
    // ---- pass 1: best allowed text token and best allowed timestamp token (the byte masks four columns at a time) ----
    const bool word_masks = (((uintptr_t)suppress | (uintptr_t)begin_suppress) & 3) == 0;
    auto masks_of = [&](int c0) -> unsigned { return rule_masks_of(suppress, begin_suppress, first, word_masks, c0, V); };
    Best bt = {-INFINITY, 0x7fffffff}, bs = {-INFINITY, 0x7fffffff};
    auto judge = [&](int c0, const bf16x4& x, unsigned mask, bool live) {
        unsigned sbits = 0, bbits = 0;                 // bit e: column c0 + e is in the history / banned
        unsigned xbits = 0;                            // bit e: column c0 + e takes a bias
        if constexpr (HIST) { sbits = history_bits_of(seen, c0); bbits = history_bits_of(banned, c0); }
        if constexpr (BIAS) xbits = history_bits_of(biased, c0);
        const ChunkKind kind = classify_chunk(rr, mask, live, c0, V, sbits | xbits, bbits);
        if (kind.clean) {
            const bool in_text = kind.in_text;
            float bv = in_text ? bt.v : bs.v;
            int bi = in_text ? bt.i : bs.i;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float v = bf2f(x[e]);
                if (v > bv) { bv = v; bi = c0 + e; }
            }
            if (in_text) { bt.v = bv; bt.i = bi; } else { bs.v = bv; bs.i = bi; }
            return;
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c0 + e;
            if (column_allowed(rr, c0, e, V, mask, bbits, live)) {
                float v = bf2f(x[e]);
                if constexpr (BIAS) { if ((xbits >> e) & 1u) v += bias_of(bcol, bsum, S, c); }
                if constexpr (HIST) { if ((sbits >> e) & 1u) v = penal(v); }
                const Best cand = {v, c};
                if (c < tsb) bt = better(bt, cand); else bs = better(bs, cand);
            }
        }
    };
    constexpr int NPRE = 13;                           // 13 x 4096 columns cover every Whisper vocabulary (51 866)
    if (V <= NPRE * SEL_NT * 4) {
        // The whole row is requested before anything is judged, with clamped addresses instead of branches around the
        // loads: as a loop, a thread's 13 chunks were 13 dependent L2 round trips (10 of the kernel's 19 us).
        const int clast = (V - 1) & ~3;
        bf16x4 xr[NPRE];
        unsigned mr[NPRE];
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int c0 = min(tid * 4 + i * SEL_NT * 4, clast);
            xr[i] = *(const bf16x4*)(row + c0);
            mr[i] = masks_of(c0);
        }
#pragma unroll
        for (int i = 0; i < NPRE; ++i) {
            const int c0 = tid * 4 + i * SEL_NT * 4;
            judge(min(c0, clast), xr[i], mr[i], c0 < V);
        }
    } else {
        for (int c0 = tid * 4; c0 < V; c0 += SEL_NT * 4) judge(c0, *(const bf16x4*)(row + c0), masks_of(c0), true);
    }
    bt = block_best(bt, red);
    bs = block_best(bs, red);
    Best pick = better(bt, bs);
    if (rr.ts_mode && bs.v > -INFINITY) {
        // mass rule: if logsumexp over the allowed timestamps exceeds the best text logit, a timestamp is taken
        float sum = 0.f;
        for (int c = tsb + tid; c < V; c += SEL_NT)
            if (allowed(c)) {
                float v = bf2f(row[c]);
                if constexpr (BIAS) { if ((biased[c >> 5] >> (c & 31)) & 1u) v += bias_of(bcol, bsum, S, c); }
                if constexpr (HIST) { if ((seen[c >> 5] >> (c & 31)) & 1u) v = penal(v); }
                sum += __expf(v - bs.v);
            }
        sum = wave_sum(sum);
        __syncthreads();
        if ((tid & 63) == 0) redf[tid >> 6] = sum;
        __syncthreads();
        sum = 0.f;
        for (int i = 0; i < SEL_NT / 64; ++i) sum += redf[i];
        if (bs.v + __logf(sum) > bt.v) pick = bs;
    }
    return pick;
}

// Host side, for the C entries of these kernels (the one header they share): what every entry asks of the logits rows and of
// the arguments of the timestamp rules (true: accept).  n: the position the step fills.
static inline bool select_args_ok(const void* logits, int V, int64_t ld, int n, int ts_begin, int begin_index, int eos) {
    if (!logits || V <= 0 || ld < V || (ld & 3) || ((uintptr_t)logits & 7)) return false;
    return !(ts_begin >= 0 && (eos < 0 || begin_index < 1 || begin_index > n));
}
