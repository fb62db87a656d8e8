// SpecAugment of the training forward (TF:modeling_whisper.py _compute_mask_indices / WhisperModel._mask_input_features) for
// gfx950: ONE launch draws the time and the feature masks of every row from the device-resident step counter of the dropout
// generator and applies them to the fp32 log-mel features [B][n_mels][T].  One workgroup per (row, block of SA_FB mel bins):
// each re-derives its row's draws (15 spans at the defaults) into LDS bitmaps -- the 256 lanes compute the Philox words of a
// round of 256 draws in parallel, lane 0 walks Floyd's subset algorithm over them, all lanes widen the chosen starts to spans --
// and then streams its contiguous slab of SA_FB * T floats.  In place (out == in) only the zeros are stored.
// The draws are stated in include/dwamd.h (dw_spec_augment); Philox4x32-10 is the function of dropout.hip, copied so that
// dropout.hip compiles to the code it had.
#include "common.h"
#include "../../include/dwamd.h"

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

#define SA_NT 256          // lanes of a workgroup
#define SA_FB 4            // mel bins of a workgroup: B = 32, n_mels = 128 -> 1024 workgroups over the 256 CUs
#define SA_MAX_AXIS 16384  // longest axis (LDS: two bitmaps per axis)
#define SA_PRE 12          // vectors a lane requests ahead of the draws (out of place): 12 x 256 x 4 >= SA_FB x 3000 elements

__device__ __forceinline__ void sa_philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                                 uint32_t o[4]) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(PHILOX_M0, c0), lo0 = PHILOX_M0 * c0;
        const uint32_t hi1 = __umulhi(PHILOX_M1, c2), lo1 = PHILOX_M1 * c2;
        c0 = hi1 ^ c1 ^ k0;
        c1 = lo1;
        c2 = hi0 ^ c3 ^ k1;
        c3 = lo0;
        k0 += PHILOX_W0;
        k1 += PHILOX_W1;
    }
    o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
}

// spans of a row with `len` valid positions (compute_num_masked_span of the reference: double precision, this order of operations)
__device__ __forceinline__ int sa_span_count(int len, int axis, double prob, int mlen, int min_masks, double eps) {
#pragma clang fp contract(off)
    const double q = prob * (double)len / (double)mlen;
    const double v = q + eps;
    int n = v >= 2147483647.0 ? 2147483647 : (int)v;          // (a count that large is clipped to axis / mlen below)
    n = max(n, min_masks);
    if ((long)n * mlen > axis) n = axis / mlen;
    if (len - (mlen - 1) < n) n = max(len - (mlen - 1), 0);
    return n;
}

// any bit of positions lo .. hi (inclusive) set
__device__ __forceinline__ bool sa_any(const uint32_t* bm, int lo, int hi) {
    const int wl = lo >> 5, wh = hi >> 5;
    for (int w = wl; w <= wh; ++w) {
        uint32_t v = bm[w];
        if (w == wl) v &= 0xFFFFFFFFu << (lo & 31);
        if (w == wh) v &= 0xFFFFFFFFu >> (31 - (hi & 31));
        if (v) return true;
    }
    return false;
}

// The mask of one axis of row b into the LDS bitmap `bm` (bit p = position p is zeroed); `ch` is scratch of the same size (the
// chosen starts), `draws` SA_NT words.  Called by every lane of the workgroup; every branch around a barrier is uniform.
__device__ void sa_axis_mask(uint32_t* ch, uint32_t* bm, uint32_t* draws, int axis, int len, double prob, int mlen, int min_masks,
                             uint32_t site, uint32_t b, uint64_t st, uint32_t k0, uint32_t k1) {
    const int tid = threadIdx.x, words = (axis + 31) >> 5;
    for (int w = tid; w < words; w += SA_NT) { ch[w] = 0; bm[w] = 0; }
    const uint32_t s0 = (uint32_t)st, s1 = (uint32_t)(st >> 32);
    uint32_t o[4];
    sa_philox4x32_10(0u, site, s0, s1, k0, k1, o);
    const double eps = (double)o[0] * (1.0 / 4294967296.0);
    const int max_n = sa_span_count(axis, axis, prob, mlen, min_masks, eps);
    const int n = sa_span_count(len, axis, prob, mlen, min_masks, eps);
    __syncthreads();
    if (max_n == 0) return;
    if (n == 0) {                                   // the reference pads such a row with the dummy index axis - 1
        if (tid == 0) bm[(axis - 1) >> 5] = 1u << ((axis - 1) & 31);
        __syncthreads();
        return;
    }
    const int M = len - (mlen - 1);                 // candidates: starts 0 .. M - 1;  1 <= n <= M
    for (int base = 0; base < n; base += SA_NT) {
        const int w = base + tid;
        if (w < n) {
            sa_philox4x32_10(((b + 1u) << 16) | (uint32_t)(w >> 2), site, s0, s1, k0, k1, o);
            const uint32_t j1 = (uint32_t)(M - n + w) + 1u;
            draws[tid] = (uint32_t)(((uint64_t)o[w & 3] * (uint64_t)j1) >> 32);        // uniform in [0, j]
        }
        __syncthreads();
        if (tid == 0) {                             // Floyd: j = M - n .. M - 1, take j when t is already chosen
            const int cnt = min(SA_NT, n - base);
            for (int i = 0; i < cnt; ++i) {
                uint32_t t = draws[i];
                if ((ch[t >> 5] >> (t & 31)) & 1u) t = (uint32_t)(M - n + base + i);
                ch[t >> 5] |= 1u << (t & 31);
            }
        }
        __syncthreads();
    }
    // position p is masked iff a start lies in [p - mlen + 1, p]  (start + mlen - 1 <= len - 1 <= axis - 1: nothing to clamp)
    for (int p = tid; p < axis; p += SA_NT)
        if (sa_any(ch, max(0, p - mlen + 1), p)) atomicOr(&bm[p >> 5], 1u << (p & 31));
    __syncthreads();
}

template <bool VEC>
__global__ __launch_bounds__(SA_NT) void spec_augment_kernel(const float* in, float* out, int n_mels, int T, const int32_t* lengths,
                                                             double t_prob, int t_len, int t_min, double f_prob, int f_len,
                                                             int f_min, uint32_t k0, uint32_t k1, const uint64_t* step,
                                                             uint8_t* time_mask, uint8_t* feat_mask) {
    extern __shared__ uint32_t sa_lds[];
    const int tid = threadIdx.x, b = blockIdx.y, f0 = blockIdx.x * SA_FB;
    const int wt = (T + 31) >> 5, wf = (n_mels + 31) >> 5;
    uint32_t* tbm = sa_lds;              // time mask bits
    uint32_t* fbm = tbm + wt;            // feature mask bits
    uint32_t* ch = fbm + wf;             // chosen starts of the axis being drawn: max(wt, wf) words
    uint32_t* draws = ch + max(wt, wf);  // SA_NT words
    // the slab of this workgroup: rows f0 .. f0 + nrows - 1 of plane b, contiguous
    const int nrows = min(SA_FB, n_mels - f0);
    const long base = ((long)b * n_mels + f0) * T;
    const bool inplace = (const float*)out == in;
    const int vpr = T >> 2, nvec = nrows * vpr;      // (16-byte path)
    // out of place the slab's loads do not depend on the draws: the first SA_PRE vectors of every lane (all of them at SA_FB x
    // T = 4 x 3000) are requested now and land while the masks are drawn
    f32x4 pre[SA_PRE];
    if (VEC && !inplace) {
#pragma unroll
        for (int k = 0; k < SA_PRE; ++k) {
            const int i = tid + k * SA_NT;
            if (i < nvec) pre[k] = *(const f32x4*)(in + base + ((long)i << 2));
        }
    }
    const uint64_t st = step[0];
    if (t_prob > 0.0) {
        int len = lengths ? lengths[b] : T;
        len = min(max(len, 0), T);
        sa_axis_mask(ch, tbm, draws, T, len, t_prob, t_len, t_min, DW_SPEC_SITE_TIME, (uint32_t)b, st, k0, k1);
    } else {
        for (int w = tid; w < wt; w += SA_NT) tbm[w] = 0;
    }
    if (f_prob > 0.0) {
        sa_axis_mask(ch, fbm, draws, n_mels, n_mels, f_prob, f_len, f_min, DW_SPEC_SITE_FEATURE, (uint32_t)b, st, k0, k1);
    } else {
        for (int w = tid; w < wf; w += SA_NT) fbm[w] = 0;
    }
    __syncthreads();

    if (blockIdx.x == 0) {
        if (time_mask)
            for (int p = tid; p < T; p += SA_NT) time_mask[(long)b * T + p] = (uint8_t)((tbm[p >> 5] >> (p & 31)) & 1u);
        if (feat_mask)
            for (int f = tid; f < n_mels; f += SA_NT) feat_mask[(long)b * n_mels + f] = (uint8_t)((fbm[f >> 5] >> (f & 31)) & 1u);
    }

    if (VEC) {                                       // T % 4 == 0 and 16-byte aligned planes (launcher)
        // four mask bits of vector i of the slab: (p & 31) <= 28, so they lie in one word
        auto bits4 = [&](int i) -> uint32_t {
            const int r = i / vpr, p = (i - r * vpr) << 2;
            const int f = f0 + r;
            return ((fbm[f >> 5] >> (f & 31)) & 1u) ? 0xFu : ((tbm[p >> 5] >> (p & 31)) & 0xFu);
        };
        int first = tid;
        if (!inplace) {
#pragma unroll
            for (int k = 0; k < SA_PRE; ++k) {
                const int i = tid + k * SA_NT;
                if (i < nvec) {
                    const uint32_t m = bits4(i);
                    f32x4 x = pre[k];
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((m >> j) & 1u) x[j] = 0.f;
                    *(f32x4*)(out + base + ((long)i << 2)) = x;
                }
            }
            first = tid + SA_PRE * SA_NT;
        }
        for (int i = first; i < nvec; i += SA_NT) {
            const uint32_t m = bits4(i);
            const long e = base + ((long)i << 2);
            if (inplace) {
                if (m == 0xFu) {
                    *(f32x4*)(out + e) = f32x4{0.f, 0.f, 0.f, 0.f};
                } else if (m) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if ((m >> j) & 1u) out[e + j] = 0.f;
                }
            } else {
                f32x4 x = *(const f32x4*)(in + e);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if ((m >> j) & 1u) x[j] = 0.f;
                *(f32x4*)(out + e) = x;
            }
        }
    } else {
        const int nel = nrows * T;
        for (int i = tid; i < nel; i += SA_NT) {
            const int r = i / T, p = i - r * T;
            const int f = f0 + r;
            const bool m = (((fbm[f >> 5] >> (f & 31)) | (tbm[p >> 5] >> (p & 31))) & 1u) != 0;
            if (inplace) {
                if (m) out[base + i] = 0.f;
            } else {
                out[base + i] = m ? 0.f : in[base + i];
            }
        }
    }
}

extern "C" int dw_spec_augment(const float* in, float* out, int B, int n_mels, int T, const int32_t* lengths, double mask_time_prob,
                               int mask_time_length, int mask_time_min_masks, double mask_feature_prob, int mask_feature_length,
                               int mask_feature_min_masks, uint64_t seed, const uint64_t* step, uint8_t* time_mask,
                               uint8_t* feat_mask, void* stream) {
    DW_CLEAR_ERR();
    if (!in || !out || !step || B <= 0 || n_mels <= 0 || T <= 0) return DW_EINVAL;
    const bool t_on = mask_time_prob > 0.0, f_on = mask_feature_prob > 0.0;
    if (t_on && (mask_time_length < 1 || mask_time_length > T)) return DW_EINVAL;
    if (f_on && (mask_feature_length < 1 || mask_feature_length > n_mels)) return DW_EINVAL;
    if (((uintptr_t)in & 3) || ((uintptr_t)out & 3)) return DW_EINVAL;
    if (B > 65534 || T > SA_MAX_AXIS || n_mels > SA_MAX_AXIS) return DW_EUNSUP;       // row b draws at counter words (b + 1) << 16 | ...
    const int wt = (T + 31) >> 5, wf = (n_mels + 31) >> 5;
    const size_t lds = (size_t)(wt + wf + (wt > wf ? wt : wf) + SA_NT) * sizeof(uint32_t);
    const dim3 grid((n_mels + SA_FB - 1) / SA_FB, B);
    const bool vec = (T & 3) == 0 && !((uintptr_t)in & 15) && !((uintptr_t)out & 15);
    const uint32_t k0 = (uint32_t)seed, k1 = (uint32_t)(seed >> 32);
    if (vec)
        hipLaunchKernelGGL(spec_augment_kernel<true>, grid, dim3(SA_NT), lds, (hipStream_t)stream, in, out, n_mels, T, lengths,
                           mask_time_prob, mask_time_length, mask_time_min_masks, mask_feature_prob, mask_feature_length,
                           mask_feature_min_masks, k0, k1, step, time_mask, feat_mask);
    else
        hipLaunchKernelGGL(spec_augment_kernel<false>, grid, dim3(SA_NT), lds, (hipStream_t)stream, in, out, n_mels, T, lengths,
                           mask_time_prob, mask_time_length, mask_time_min_masks, mask_feature_prob, mask_feature_length,
                           mask_feature_min_masks, k0, k1, step, time_mask, feat_mask);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
