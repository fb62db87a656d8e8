// Offline distillation from stored top-k teacher log-probabilities (the format: include/dwamd.h, "Stored top-k teacher targets").
//   dw_logits_topk          one 1024-thread workgroup per row of teacher logits, the row in registers as dw_beam_candidates holds it:
//                           the k largest columns (equal values to the lower column) by a radix select over the ordered bf16 bits,
//                           ordered in LDS by (value descending, column ascending), their log-probabilities at temperature T and the
//                           probability mass of all other columns, summed term by term.
//   dw_distill_loss_topk    csrc/loss.hip's fused CE + KL loss and gradient with the teacher row replaced by those k + 1 numbers: the KL
//   dw_distill_loss_topk_w  divergence of the two distributions with the columns outside K merged into one bucket.  One workgroup per
//                           row, the student row in registers: one read of the row, one write of the gradient, no teacher row.
// Math of the loss (per row, z = student logits, m = their maximum, q = softmax(z / T), p_j = exp(logp[j]), r = rest, K = idx[0..k)):
//   ce      = m + log sum exp(z - m) - z[label]                                                        (the dense kernel's term)
//   e_c     = exp((z_c - m) / T),  Z = sum_c e_c,  S = max(sum_{c not in K} e_c, FLT_MIN)               (S: non-negative terms only)
//   row_kl  = sum_j p_j (logp[j] - ((z_{K_j} - m) / T - log Z)) + [r > 0] r (log r - (log S - log Z))
//   grad(c) = gs * [ cw/n_ce * (softmax(z)(c) - [c == label]) + kw*T/n_kl * g_c ],   g_c = e_c / Z - p_c        for c in K
//                                                                                     g_c = e_c * (1 / Z - r / S)  otherwise
// The exponentials of a student row are the fast ones (52 per thread, twice); a row's few logarithms, the members' exp(logp) and
// everything in dw_logits_topk (it runs once per dataset) are the accurate ones.
// Sums: every thread adds its <= 52 terms in fp32 in slot order, the 1024 partial sums are added in double in a fixed order; the
// histograms of the selection are integer counts.  Nothing depends on the arrival order of an atomic: equal inputs give equal bits.
#include <float.h>
#include "common.h"
#include "../../include/dwamd.h"

#define TK_NT 1024
#define TK_NCH 13                                   // chunks of four columns per thread: 13 * 4096 = 53 248 columns
#define TK_MAX_V (TK_NCH * TK_NT * 4)
#define TK_MAX_K 64

struct TkScratch { int hist[256]; int wtot[4]; int base; int digit; double redd[TK_NT / 64]; float redf[TK_NT / 64]; };

// a value every lane holds alike, moved to a scalar register (the row kernels have no vector register to spare for it)
__device__ __forceinline__ float tk_uniform(float x) { return __uint_as_float(__builtin_amdgcn_readfirstlane(__float_as_uint(x))); }
__device__ __forceinline__ float tk_block_max(float v, TkScratch* sc) { return tk_uniform(block_max<TK_NT>(v, sc->redf)); }
__device__ __forceinline__ double tk_block_sum_d(double d, TkScratch* sc) {     // the 1024 partial sums added in double, fixed order
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) d += __shfl_xor(d, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) sc->redd[threadIdx.x >> 6] = d;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int i = 0; i < TK_NT / 64; ++i) t += sc->redd[i];
    const unsigned long long u = __double_as_longlong(t);
    const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(u >> 32)), lo = (unsigned)__builtin_amdgcn_readfirstlane((int)u);
    return __longlong_as_double((long long)(((unsigned long long)hi << 32) | (unsigned long long)lo));
}
__device__ __forceinline__ float tk_block_sum(float part, TkScratch* sc) { return (float)tk_block_sum_d((double)part, sc); }

// Unsigned order of the 16 bits == order of the bf16 values; -0 counts as +0.  Selection works on INVERTED keys (0xffff - key): the
// k-th largest value is the k-th smallest inverted key.
__device__ __forceinline__ unsigned tk_key16(unsigned bits) {         // the 16 bits of a bf16 value
    const unsigned u = bits == 0x8000u ? 0u : bits;
    return (u & 0x8000u) ? (~u & 0xffffu) : (u | 0x8000u);
}

// dw_sample_select's search (csrc/decode.hip select_key) for 16-bit keys and unit weights: the smallest key K among the workgroup's
// items with count(items <= K) > T, eight bits at a time over a 256-bin LDS histogram.  `each(f)` calls f(key) for every item of the
// calling thread; the caller guarantees 0 <= T < count(all items).  *below: the number of items with a key < K.
template <class Each>
__device__ __forceinline__ unsigned tk_select(Each&& each, int T, TkScratch* sc, int* below) {
    const int tid = threadIdx.x, lane = tid & 63;
    unsigned prefix = 0;
    int base = 0;
#pragma unroll 1
    for (int shift = 8; shift >= 0; shift -= 8) {
        const unsigned pmask = shift == 8 ? 0u : 0xff00u;
        __syncthreads();
        if (tid < 256) sc->hist[tid] = 0;
        __syncthreads();
        each([&](unsigned key) {
            if ((key & pmask) == prefix) atomicAdd(&sc->hist[(key >> shift) & 255u], 1);
        });
        __syncthreads();
        int own = 0, incl = 0;
        if (tid < 256) {                           // inclusive scan of the 256 bins: within a wave, then across the four waves
            own = incl = sc->hist[tid];
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(incl, o);
                if (lane >= o) incl += y;
            }
            if (lane == 63) sc->wtot[tid >> 6] = incl;
        }
        __syncthreads();
        if (tid < 256) {
            for (int w = 0; w < (tid >> 6); ++w) incl += sc->wtot[w];
            const int before = base + incl - own;
            if (before <= T && before + own > T) { sc->digit = tid; sc->base = before; }     // exactly one bin
        }
        __syncthreads();
        prefix |= (unsigned)__builtin_amdgcn_readfirstlane(sc->digit) << shift;
        base = __builtin_amdgcn_readfirstlane(sc->base);
    }
    *below = base;
    return prefix;
}

// the bf16 value of a key, widened
__device__ __forceinline__ float tk_value(unsigned key) {
    const unsigned u = (key & 0x8000u) ? (key ^ 0x8000u) : (~key & 0xffffu);
    return __uint_as_float(u << 16);
}
// a value the compiler cannot see through: a loop that takes its own copy of a bound or of a zero is not merged with, or hoisted out
// of, the passes around it (hoisted, the 52 keys or exponentials of a thread would stay live in registers and spill)
template <class X>
__device__ __forceinline__ X tk_fresh(X x) { asm volatile("" : "+v"(x)); return x; }
// bits 0..3: which of a chunk's four columns lie inside the row, from n = V - (the chunk's first column).  Plain arithmetic here and
// in tk_bit / tk_inside below: as 52 compares the results would all be live in scalar registers at once.
__device__ __forceinline__ unsigned tk_in4(int n) { return (1u << min(max(n, 0), 4)) - 1u; }
// bit j as 0.f / 1.f
__device__ __forceinline__ float tk_bit(unsigned long long bits, int j) { return (float)((unsigned)(bits >> j) & 1u); }
// x where bit j is set, +0 otherwise (by its bits: x may be anything, an infinity included)
__device__ __forceinline__ float tk_inside(float x, unsigned long long bits, int j) {
    return __uint_as_float(__float_as_uint(x) & (0u - ((unsigned)(bits >> j) & 1u)));
}

// TK_CHUNK(j, zero[, acc]) in front of slot j of a loop over a thread's 52 slots: at the first slot of every chunk the loop's opaque
// zero (and its running value) pass through an asm statement, so the chunks are unpacked and consumed one after the other
#define TK_CHUNK_1(zero) asm volatile("" : "+v"(zero) :: "memory")
#define TK_CHUNK_2(zero, acc) asm volatile("" : "+v"(zero), "+v"(acc) :: "memory")
#define TK_CHUNK_PICK(a, b, c, name, ...) name
#define TK_CHUNK(j, ...)                                                             \
    do {                                                                             \
        if (((j) & 3) == 0) {                                                        \
            __builtin_amdgcn_sched_barrier(0);                                       \
            TK_CHUNK_PICK(j, __VA_ARGS__, TK_CHUNK_2, TK_CHUNK_1)(__VA_ARGS__);      \
        }                                                                            \
    } while (0)

__global__ __launch_bounds__(TK_NT) void logits_topk_kernel(const bf16* logits, int V, long ld, float T, int k, int32_t* idx,
                                                            float* logp, float* rest) {
    const float invT = 1.0f / T;
    __shared__ TkScratch sc;
    __shared__ unsigned win[TK_MAX_K];             // (key << 16) | (0xffff - column): larger = earlier in the stored order
    __shared__ int nwin;
    const int tid = threadIdx.x, tid4 = tid * 4;
    const long r = blockIdx.x;
    const bf16* row = logits + r * ld;
    auto off = [](int j) -> int { return (j >> 2) * (TK_NT * 4) + (j & 3); };      // slot j holds column tid4 + off(j)
    // ---- the row into registers as it is stored, two bf16 per register (slot j: bits 16 (j & 1) of xw[j >> 1]); slots beyond V repeat
    // the row's last chunk and are masked by `inbits` ----
    unsigned xw[TK_NCH * 2];
    unsigned long long inbits = 0;                  // bit j: slot j is inside the row
    {
        typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
        const int clast = (V - 1) & ~3;
#pragma unroll
        for (int i = 0; i < TK_NCH; ++i) {
            const u32x2 w = *(const u32x2*)(row + (unsigned)min(tid4 + i * TK_NT * 4, clast));
            xw[2 * i] = w[0]; xw[2 * i + 1] = w[1];
            inbits |= (unsigned long long)tk_in4(V - (tid4 + i * TK_NT * 4)) << (4 * i);
        }
    }
    // slot j's key.  `zero` is an opaque 0 that every loop over the slots takes afresh per chunk (TK_CHUNK): the chunks are unpacked
    // one after the other, and no loop keeps another loop's 52 keys or exponentials
    auto key_of = [&](int j, unsigned zero) -> unsigned { return tk_key16(((xw[j >> 1] ^ zero) >> (16 * (j & 1))) & 0xffffu); };
    unsigned mk = 0;                                // the thread's largest key (0: no column)
    {
        unsigned zero = 0u;
#pragma unroll
        for (int j = 0; j < TK_NCH * 4; ++j) {
            TK_CHUNK(j, zero, mk);
            mk = max(mk, key_of(j, zero) & (0u - ((unsigned)(inbits >> j) & 1u)));
        }
    }
    if (tid == 0) nwin = 0;
    const float m = tk_block_max(mk ? tk_value(mk) : -INFINITY, &sc);              // (key order is value order)
    // ---- the k-th largest value.  First over the 1024 thread maxima: their k-th largest is a lower bound of the row's k-th largest
    // (from V = 256 on at least 64 >= k threads hold a column; below that every column is a candidate), so that the second search
    // counts a handful of columns instead of V ----
    int below;
    unsigned lo = 0;
    if (V >= 4 * TK_MAX_K) lo = 0xffffu - tk_select([&](auto&& f) { if (mk) f(0xffffu - mk); }, k - 1, &sc, &below);
    const unsigned kth = 0xffffu - tk_select([&](auto&& f) {
        unsigned zero = 0u;
        const unsigned l = tk_fresh(lo);
        const unsigned long long in = tk_fresh(inbits);
#pragma unroll
        for (int j = 0; j < TK_NCH * 4; ++j) {
            TK_CHUNK(j, zero);
            const unsigned key = key_of(j, zero);
            if (((in >> j) & 1ull) && key >= l) f(0xffffu - key);
        }
    }, k - 1, &sc, &below);
    // `below` columns lie above the k-th value; of the columns equal to it the k - below lowest stay: the bound is found by the same
    // search over their column numbers (V <= 53 248 < 2^16)
    const int need = k - below;
    int dummy;
    const int cmax = (int)tk_select([&](auto&& f) {
        unsigned zero = 0u;
        const unsigned kk = tk_fresh(kth);
        const unsigned long long in = tk_fresh(inbits);
#pragma unroll
        for (int j = 0; j < TK_NCH * 4; ++j) {
            TK_CHUNK(j, zero);
            if (((in >> j) & 1ull) && key_of(j, zero) == kk) f((unsigned)(tid4 + off(j)));
        }
    }, need - 1, &sc, &dummy);
    // ---- e_c = exp((z_c - m) / T) once per column: Z over all V columns, the tail over the columns that did not win, term by term
    // (rest = tail / Z and logp = (z - m) / T - log Z: nothing is subtracted from a rounded log-sum-exp inside an exponent); the
    // winners go to LDS in arrival order ----
    // The two sums are kept in double from the first add and the row's log and quotient are taken in double: the stored logp and rest
    // are single roundings of values whose own error is that of the fp32 exponentials, averaged over the columns.
    double part = 0.0, tpart = 0.0;
    {
        unsigned zero = 0u;
        const unsigned long long in = tk_fresh(inbits);
#pragma unroll
        for (int j = 0; j < TK_NCH * 4; ++j) {
            TK_CHUNK(j, zero, part);
            const int c = tid4 + off(j);
            const unsigned key = key_of(j, zero);
            const bool inside = (in >> j) & 1ull, wins = key > kth || (key == kth && c <= cmax);
            if (inside) {                            // (a slot outside the row holds whatever lies behind it, pad columns included)
                const float e = expf((tk_value(key) - m) * invT);
                part += (double)e;
                if (!wins) tpart += (double)e;
            }
            if (inside && wins) {
                const int slot = atomicAdd(&nwin, 1);                  // (the order below does not depend on the slot)
                if (slot < TK_MAX_K) win[slot] = (key << 16) | (0xffffu - (unsigned)c);
            }
        }
    }
    const double Z = tk_block_sum_d(part, &sc);
    const double tail = tk_block_sum_d(tpart, &sc);  // (the barriers also publish win[])
    if (tid == 0) rest[r] = (float)(tail / Z);
    // ---- order: a winner's place is the number of winners in front of it (distinct columns: distinct words) ----
    if (tid < k) {
        const unsigned w = win[tid];
        int place = 0;
        for (int i = 0; i < k; ++i) place += win[i] > w ? 1 : 0;
        idx[r * k + place] = (int)(0xffffu - (w & 0xffffu));
        logp[r * k + place] = (float)(((double)tk_value(w >> 16) - (double)m) / (double)T - log(Z));
    }
}

extern "C" int dw_logits_topk(const void* logits, int rows, int V, int64_t ld, float temperature, int k, int32_t* idx,
                              float* logp, float* rest, void* stream) {
    DW_CLEAR_ERR();
    if (!logits || !idx || !logp || !rest) return DW_EINVAL;
    if (((uintptr_t)logits & 7) || ((uintptr_t)idx & 3) || ((uintptr_t)logp & 3) || ((uintptr_t)rest & 3)) return DW_EINVAL;
    if (rows <= 0 || V <= 0 || ld < V || (ld & 3) || !(temperature > 0.f) || !(temperature <= FLT_MAX)) return DW_EINVAL;
    if (k < 1 || k >= V) return DW_EINVAL;
    if (V > TK_MAX_V || k > TK_MAX_K) return DW_EUNSUP;
    hipLaunchKernelGGL(logits_topk_kernel, dim3(rows), dim3(TK_NT), 0, (hipStream_t)stream, (const bf16*)logits, V, (long)ld,
                       temperature, k, idx, logp, rest);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// The loss.  The label counts and the final means are csrc/loss.hip's (loss_count_kernel / loss_final_kernel), restated here: the two
// files share no kernel header, and the final means are taken in double here.
// ---------------------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void topk_loss_count_kernel(const int64_t* labels, int rows, int32_t* counts) {
    __shared__ float red[256 / 64];
    float n_ce = 0.f, n_kl = 0.f;
    for (int i = threadIdx.x; i < rows; i += 256) {
        const int64_t l = labels[i];
        n_ce += (l != -100) ? 1.f : 0.f;
        n_kl += (l >= 0) ? 1.f : 0.f;
    }
    n_ce = block_sum<256>(n_ce, red);
    n_kl = block_sum<256>(n_kl, red);
    if (threadIdx.x == 0) { counts[0] = (int32_t)n_ce; counts[1] = (int32_t)n_kl; }
}

__global__ __launch_bounds__(TK_NT) void topk_loss_row_kernel(const bf16* s_logits, const int32_t* idx, const float* logp,
                                                              const float* rest, int k, const int64_t* labels, int V, long ld,
                                                              float T, float ce_w, float kl_w, float grad_scale, bf16* dlogits,
                                                              float* row_ce, float* row_kl, const int32_t* counts,
                                                              const float* weights) {
    __shared__ TkScratch sc;
    __shared__ unsigned member[TK_MAX_V / 32];     // bit c: column c is one of the row's k
    __shared__ float mem_p[TK_MAX_K];
    const int tid = threadIdx.x, tid4 = tid * 4;
    const long row = blockIdx.x;
    const bf16* zs = s_logits + row * ld;
    bf16* dz = dlogits ? dlogits + row * ld : nullptr;
    const int64_t label = labels[row];
    const bool ce_ok = label != -100 && label >= 0 && label < V;
    const bool kl_ok = label >= 0;
    if (!ce_ok && !kl_ok) {                         // (uniform) the row is in neither sum: its targets are not looked at
        if (tid == 0) { row_ce[row] = 0.f; row_kl[row] = 0.f; }
        if (dz) {
            bf16x4 o;
#pragma unroll
            for (int e = 0; e < 4; ++e) o[e] = f2bf(0.f);
            for (long c0 = tid4; c0 < ld; c0 += TK_NT * 4) *(bf16x4*)(dz + c0) = o;
        }
        return;
    }
    auto off = [](int j) -> int { return (j >> 2) * (TK_NT * 4) + (j & 3); };
    const float invT = 1.0f / T;
    // ---- everything that is read from the row's memory is read before the gradient may overwrite it ----
    const float z_label = tk_uniform(ce_ok ? bf2f(zs[label]) : 0.f);
    typedef __attribute__((ext_vector_type(2))) unsigned u32x2;
    u32x2 xr[TK_NCH];                               // the row as it is stored, two bf16 per register
    {
        const int clast = (V - 1) & ~3;
#pragma unroll
        for (int i = 0; i < TK_NCH; ++i) xr[i] = *(const u32x2*)(zs + (unsigned)min(tid4 + i * TK_NT * 4, clast));
    }
    // column e of a chunk widened.  Every loop over the chunks takes its chunk through an asm statement together with the loop's
    // running values: chunk i + 1 is unpacked after chunk i is done, and no loop keeps another loop's 52 floats or exponentials
    auto val = [](u32x2 w, int e) -> float {
        return __uint_as_float((e & 1) ? (w[e >> 1] & 0xffff0000u) : (w[e >> 1] << 16));
    };
    int my_c = -1;                                  // thread j < k: member j (a column outside [0, V) is skipped, never dereferenced)
    float my_lp = 0.f, my_z = 0.f;
    if (kl_ok) {
        for (int w = tid; w < (V + 31) / 32; w += TK_NT) member[w] = 0u;
        if (tid < k) {
            const int c = idx[row * k + tid];
            my_lp = logp[row * k + tid];
            if (c >= 0 && c < V) { my_c = c; my_z = bf2f(zs[c]); }
        }
    }
    float ms = -INFINITY;
    unsigned long long inbits = 0;                  // bit j: slot j is inside the row
#pragma unroll
    for (int i = 0; i < TK_NCH; ++i) {
        const unsigned in4 = tk_in4(V - (tid4 + i * TK_NT * 4));
        inbits |= (unsigned long long)in4 << (4 * i);
        u32x2 w = xr[i];
        asm volatile("" : "+v"(w), "+v"(ms));
#pragma unroll
        for (int e = 0; e < 4; ++e) ms = fmaxf(ms, ((in4 >> e) & 1u) ? val(w, e) : -INFINITY);
    }
    ms = tk_block_max(ms, &sc);                     // (its barriers order the clearing of `member` before the bits)
    if (kl_ok && tid < k) {
        mem_p[tid] = my_c >= 0 ? expf(my_lp) : 0.f;
        if (my_c >= 0) atomicOr(&member[my_c >> 5], 1u << (my_c & 31));
    }
    __syncthreads();
    // ---- partition functions; the tail of the student's distribution as a sum of its own non-negative terms ----
    unsigned long long mbits = 0;                   // bit j: slot j is a member
    float zs1 = 0.f, zsT = 0.f, tail = 0.f;
    const unsigned long long in_b = tk_fresh(inbits);
#pragma unroll
    for (int i = 0; i < TK_NCH; ++i) {
        const int c0 = tid4 + i * TK_NT * 4;
        const unsigned mb = (kl_ok && c0 < V) ? (member[c0 >> 5] >> (c0 & 31)) & 15u : 0u;
        mbits |= (unsigned long long)mb << (4 * i);
        u32x2 w = xr[i];
        asm volatile("" : "+v"(w), "+v"(zs1), "+v"(zsT), "+v"(tail));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            // 0 / 1 factors, not selects: 52 compare results would all be live in scalar registers.  A slot outside the row holds
            // whatever lies behind it, pad columns included: its DIFFERENCE from the row maximum is cleared to +0 (tk_inside), so its
            // exponentials are exp(0) = 1 times the factor 0 wherever the row's values lie (a row far below -88 included).
            const float inside = tk_bit(in_b, 4 * i + e), out = (float)(((mb >> e) & 1u) ^ 1u);
            const float d = tk_inside(val(w, e) - ms, in_b, 4 * i + e);
            const float e1 = __expf(d), eT = __expf(d * invT) * inside;
            zs1 += e1 * inside;
            zsT += eT;
            tail += eT * out;
        }
    }
    zs1 = tk_block_sum(zs1, &sc);
    zsT = tk_block_sum(zsT, &sc);
    tail = fmaxf(tk_block_sum(tail, &sc), FLT_MIN);
    // ---- the row's two terms, by wave 0 (it holds all k <= 64 members) in double: the row's few logarithms and differences are not
    // where an fp32 rounding of an 11 (log Z at V = 5e4) should enter; one rounding at the store ----
    const float r = kl_ok ? rest[row] : 0.f;
    if (tid < 64) {
        const double logZ = log((double)zsT);
        double term = 0.0;
        if (kl_ok && tid < k && my_c >= 0)
            term = (double)mem_p[tid] * ((double)my_lp - (((double)my_z - (double)ms) * (double)invT - logZ));
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) term += __shfl_xor(term, o);
        if (tid == 0) {
            const double kl_rest = r > 0.f ? (double)r * (log((double)r) - (log((double)tail) - logZ)) : 0.0;
            row_ce[row] = ce_ok ? (float)((double)ms + log((double)zs1) - (double)z_label) : 0.f;
            row_kl[row] = kl_ok ? (float)(term + kl_rest) : 0.f;
        }
    }
    if (!dz) return;

    // ---- gradient w.r.t. the student logits (written in place of / next to them) ----
    if (weights) { ce_w = weights[0]; kl_w = weights[1]; }      // device-resident mix (dw_distill_loss_topk_w)
    const float n_ce = (float)max(counts[0], 1), n_kl = (float)max(counts[1], 1);
    const float gce = ce_ok ? grad_scale * ce_w / n_ce : 0.f;
    const float gkl = kl_ok ? grad_scale * kl_w * T / n_kl : 0.f;  // T^2 * (1/T)
    const float i1 = 1.0f / zs1, iS = 1.0f / zsT;
    const float ftail = iS - (r > 0.f ? r / tail : 0.f);
    const unsigned long long in_c = tk_fresh(inbits), mem_b = tk_fresh(mbits);
    const int lab = ce_ok ? (int)label : -1;        // (gce is 0 otherwise)
    const float msg = ms;
    const int ldw = (int)min(ld, (long)TK_MAX_V);   // the pitch inside the register window
#pragma unroll
    for (int i = 0; i < TK_NCH; ++i) {
        const int c0 = tid4 + i * TK_NT * 4;
        if (c0 >= ldw) continue;                    // (ld is a multiple of 8: a chunk lies inside the pitch or beyond it)
        bf16x4 o;
        u32x2 w = xr[i];
        asm volatile("" : "+v"(w) :: "memory");     // (behind the store of the chunk before)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = c0 + e;
            const float d = tk_inside(val(w, e) - msg, in_c, 4 * i + e);      // (+0 outside the row, as in the sums)
            const float p1 = __expf(d) * i1;
            const float eT = __expf(d * invT);
            // (a member's element is written again below, with its p_c)
            const float mb = tk_bit(mem_b, 4 * i + e);
            const float gk = eT * (ftail + mb * (iS - ftail));
            const float g = gce * (p1 - (c == lab ? 1.f : 0.f)) + gkl * gk;
            o[e] = f2bf(g * tk_bit(in_c, 4 * i + e));
        }
        *(bf16x4*)(dz + (unsigned)c0) = o;
    }
    // ---- the k members once more, by the threads that hold them: q_c - p_c.  q_c and p_c are both rounded before the subtraction
    // (a compiler-chosen contraction of the product leaves its rounding error behind, csrc/loss.hip): a student that reproduces the
    // stored probability gets exactly zero.  The barrier orders these stores behind the chunk stores of the same workgroup. ----
    __syncthreads();
    if (kl_ok && tid < k && my_c >= 0) {
        const float p1 = __expf(my_z - msg) * i1;
        float pS = __expf((my_z - msg) * invT) * iS;
        asm("" : "+v"(pS));
        dz[my_c] = f2bf(gce * (p1 - (my_c == lab ? 1.f : 0.f)) + gkl * (pS - mem_p[tid]));
    }
    {                                               // pad columns beyond the register window (ld > 53 248)
        bf16x4 o;
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = f2bf(0.f);
        for (long c0 = (long)TK_MAX_V + tid4; c0 < ld; c0 += TK_NT * 4) *(bf16x4*)(dz + c0) = o;
    }
}

__global__ __launch_bounds__(256) void topk_loss_final_kernel(const float* row_ce, const float* row_kl, int rows,
                                                              const int32_t* counts, float T, float ce_w, float kl_w, float* losses,
                                                              const float* weights) {
    __shared__ double red[2][256 / 64];
    double a = 0.0, b = 0.0;                        // (the means and the mix in double, rounded once at the store)
    for (int i = threadIdx.x; i < rows; i += 256) { a += (double)row_ce[i]; b += (double)row_kl[i]; }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((threadIdx.x & 63) == 0) { red[0][threadIdx.x >> 6] = a; red[1][threadIdx.x >> 6] = b; }
    __syncthreads();
    if (weights) { ce_w = weights[0]; kl_w = weights[1]; }
    if (threadIdx.x == 0) {
        a = b = 0.0;
        for (int w = 0; w < 256 / 64; ++w) { a += red[0][w]; b += red[1][w]; }
        // no valid label in the batch: NaN means, as the dense kernel reports them (csrc/loss.hip loss_final_kernel)
        const double ce = a / (double)counts[0];
        const double kl = b / (double)counts[1] * (double)T * (double)T;
        losses[0] = (float)ce;
        losses[1] = (float)kl;
        losses[2] = (float)((double)ce_w * ce + (double)kl_w * kl);
        losses[3] = (float)counts[0];
    }
}

static int distill_loss_topk_launch(const void* s_logits, const int32_t* idx, const float* logp, const float* rest, int k,
                                    const int64_t* labels, int rows, int V, int64_t ld, float temperature, float ce_weight,
                                    float kl_weight, const float* weights, float grad_scale, float* losses, void* dlogits,
                                    float* row_ce, float* row_kl, int32_t* counts, void* stream) {
    DW_CLEAR_ERR();
    if (!s_logits || !idx || !logp || !rest || !labels || !losses || !row_ce || !row_kl || !counts) return DW_EINVAL;
    if (rows <= 0 || V <= 0 || ld < V || (ld & 7) || !(temperature > 0.f)) return DW_EINVAL;
    if (((uintptr_t)s_logits & 15) || ((uintptr_t)dlogits & 15)) return DW_EINVAL;
    if (((uintptr_t)idx & 3) || ((uintptr_t)logp & 3) || ((uintptr_t)rest & 3)) return DW_EINVAL;
    if (k < 1 || k >= V) return DW_EINVAL;
    if (V > TK_MAX_V || k > TK_MAX_K) return DW_EUNSUP;
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(topk_loss_count_kernel, dim3(1), dim3(256), 0, s, labels, rows, counts);
    hipLaunchKernelGGL(topk_loss_row_kernel, dim3(rows), dim3(TK_NT), 0, s, (const bf16*)s_logits, idx, logp, rest, k, labels, V,
                       (long)ld, temperature, ce_weight, kl_weight, grad_scale, (bf16*)dlogits, row_ce, row_kl, counts, weights);
    hipLaunchKernelGGL(topk_loss_final_kernel, dim3(1), dim3(256), 0, s, row_ce, row_kl, rows, counts, temperature, ce_weight,
                       kl_weight, losses, weights);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

extern "C" int dw_distill_loss_topk(const void* s_logits, const int32_t* idx, const float* logp, const float* rest, int k,
                                    const int64_t* labels, int rows, int V, int64_t ld, float temperature, float ce_weight,
                                    float kl_weight, float grad_scale, float* losses, void* dlogits, float* row_ce, float* row_kl,
                                    int32_t* counts, void* stream) {
    return distill_loss_topk_launch(s_logits, idx, logp, rest, k, labels, rows, V, ld, temperature, ce_weight, kl_weight, nullptr,
                                    grad_scale, losses, dlogits, row_ce, row_kl, counts, stream);
}

extern "C" int dw_distill_loss_topk_w(const void* s_logits, const int32_t* idx, const float* logp, const float* rest, int k,
                                      const int64_t* labels, int rows, int V, int64_t ld, float temperature, const float* weights,
                                      float grad_scale, float* losses, void* dlogits, float* row_ce, float* row_kl, int32_t* counts,
                                      void* stream) {
    if (!weights || ((uintptr_t)weights & 3)) return DW_EINVAL;
    return distill_loss_topk_launch(s_logits, idx, logp, rest, k, labels, rows, V, ld, temperature, 0.f, 0.f, weights, grad_scale,
                                    losses, dlogits, row_ce, row_kl, counts, stream);
}
