// Token-level timestamps (TF:generation_whisper.py:241-381 `_extract_token_timestamps`, :43-61 `_median_filter`, :64-115
// `_dynamic_time_warping`) on the device: the alignment heads' cross-attention probabilities, their normalisation /
// median filter / head average, and the dynamic programme with its backtrace.
//
// The reference keeps every decoding step's eager attention matrix, copies [batch, heads, tokens, 1500] to the host and runs a
// double Python loop per batch row.  The attention kernels of this library are flash-style and never hold the probabilities, so
// the alignment heads' rows are recomputed here from the q / k projections of one teacher-forced decoder pass.
#include "common.h"
#include "../../include/dwamd.h"

#define ALIGN_MAX_HEADS 32      // alignment heads per model (Whisper checkpoints list 4 - 23)
#define ALIGN_MAX_TOK 512       // token rows of the dynamic programme (max_target_positions = 448)
#define ALIGN_MAX_WIDTH 9       // median filter width (every Whisper config: 7)

static __device__ __forceinline__ bf16x8 ldg8(const bf16* base, long row, long ld, int col) {
    return *(const bf16x8*)(base + row * ld + col);
}

// ---------------------------------------------------------------------------------------------------------------------------
// dw_cross_attn_probs: softmax(scale * q k^T) of selected heads, written out in fp32.
// One workgroup of four waves per (32 queries, head slot, batch row).  The key tiles (32 keys) go round-robin over the waves;
// the scores S^T = K . Q^T of a tile are four 32x32x16 MFMAs on fragments loaded straight from global memory (a head's K rows
// are 128-byte pieces the L2 keeps: 188 KiB per (batch row, head), read by every query block).  Three sweeps over the keys --
// exact row maximum, sum of exp, normalised store -- instead of one sweep with the scores parked in LDS: 32 x 1500 floats per
// workgroup would leave one workgroup per CU, and recomputing a tile costs four MFMAs.
// Lane layout of a score tile (v_mfma_f32_32x32x16_bf16, A = keys, B = queries): lane holds query (lane & 31), keys
// (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5) for r = 0..15.
struct ProbsP {
    const bf16 *q, *k;
    const int32_t* heads;
    float* probs;
    int H, L, Lk, n_total, slot0;
    long ldq, ldk, kv_rows, ldp;
    float scale;
};

__global__ __launch_bounds__(256) void cross_attn_probs_kernel(const ProbsP p) {
    __shared__ float red[4][32];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int hi = lane >> 5, ln = lane & 31;
    const int b = blockIdx.z, slot = blockIdx.y;
    const int h = p.heads[slot];
    if (h < 0 || h >= p.H) return;                      // (uniform over the workgroup: a head id the model does not have)
    const int qrow = blockIdx.x * 32 + ln;
    const bool q_ok = qrow < p.L;
    const int qc = q_ok ? qrow : p.L - 1;
    const bf16* Q = p.q + (long)b * p.L * p.ldq + h * 64;
    const bf16* K = p.k + (long)b * p.kv_rows * p.ldk + h * 64;
    float* out = p.probs + (((long)b * p.n_total + p.slot0 + slot) * p.L + qc) * p.ldp;
    bf16x8 qf[4];
#pragma unroll
    for (int kk = 0; kk < 4; ++kk) qf[kk] = ldg8(Q, qc, p.ldq, kk * 16 + hi * 8);
    const int nkt = (p.Lk + 31) >> 5;
    const float ninf = -__builtin_inff();

    auto scores = [&](int kt, f32x16& s) __attribute__((always_inline)) {
        int krow = kt * 32 + ln;
        krow = krow < p.Lk ? krow : p.Lk - 1;
#pragma unroll
        for (int r = 0; r < 16; ++r) s[r] = 0.f;
#pragma unroll
        for (int kk = 0; kk < 4; ++kk)
            s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ldg8(K, krow, p.ldk, kk * 16 + hi * 8), qf[kk], s, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int key = kt * 32 + (r & 3) + 8 * (r >> 2) + 4 * hi;
            s[r] = key < p.Lk ? s[r] * p.scale : ninf;
        }
    };
    // value per query combined over the two half-waves and the four waves
    auto combine = [&](float v, bool is_max) __attribute__((always_inline)) {
        v = is_max ? xhalf_max(v) : xhalf_sum(v);
        __syncthreads();
        if (hi == 0) red[wave][ln] = v;
        __syncthreads();
        float t = red[0][ln];
#pragma unroll
        for (int w = 1; w < 4; ++w) t = is_max ? fmaxf(t, red[w][ln]) : t + red[w][ln];
        return t;
    };
    f32x16 s;
    float mx = ninf;
    for (int kt = wave; kt < nkt; kt += 4) {
        scores(kt, s);
#pragma unroll
        for (int r = 0; r < 16; ++r) mx = fmaxf(mx, s[r]);
    }
    mx = combine(mx, true);
    float sum = 0.f;
    for (int kt = wave; kt < nkt; kt += 4) {
        scores(kt, s);
#pragma unroll
        for (int r = 0; r < 16; ++r) sum += __expf(s[r] - mx);        // (masked keys: exp(-inf) = 0)
    }
    sum = combine(sum, false);
    for (int kt = wave; kt < nkt; kt += 4) {
        scores(kt, s);
        if (!q_ok) continue;
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            const int key = kt * 32 + 8 * g + 4 * hi;
            f32x4 v;
#pragma unroll
            for (int e = 0; e < 4; ++e) v[e] = __expf(s[4 * g + e] - mx) / sum;
            if (key + 4 <= p.Lk) {
                *(f32x4*)(out + key) = v;
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (key + e < p.Lk) out[key + e] = v[e];
            }
        }
    }
}

extern "C" int dw_cross_attn_probs(const void* q, const void* k, const int32_t* heads, int n, float* probs, int B, int H,
                                   int L, int Lk, int64_t ldq, int64_t ldk, int64_t kv_batch_rows, int n_total, int slot0,
                                   int64_t ldp, float scale, void* stream) {
    if (!q || !k || !heads || !probs) return DW_EINVAL;
    if (B < 1 || B > 65535 || H < 1 || L < 1 || L > ALIGN_MAX_TOK || Lk < 1 || n < 1 || n_total > ALIGN_MAX_HEADS) return DW_EINVAL;
    if (slot0 < 0 || slot0 + n > n_total || kv_batch_rows < Lk || ldp < Lk || ldq < (int64_t)H * 64 || ldk < (int64_t)H * 64)
        return DW_EINVAL;
    if ((ldq & 7) || (ldk & 7) || (ldp & 3) || ((uintptr_t)q & 15) || ((uintptr_t)k & 15) || ((uintptr_t)probs & 15))
        return DW_EINVAL;
    ProbsP p{(const bf16*)q, (const bf16*)k, heads, probs, H, L, Lk, n_total, slot0, ldq, ldk, kv_batch_rows, ldp, scale};
    DW_CLEAR_ERR();
    hipLaunchKernelGGL(cross_attn_probs_kernel, dim3((L + 31) / 32, n, B), dim3(256), 0, (hipStream_t)stream, p);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// dw_align_prepare (TF:generation_whisper.py:341-365): per (batch row, head, frame) column the mean and the population standard
// deviation over the token axis, (w - mean) / std, median of `width` along the frames (reflect padding, TF:43-61), mean over
// the heads, negated (the DTW minimises).
// One workgroup per (56 frames, batch row): wave lane = frame column of a 64-column window (4 columns of halo on each side for
// the median), the four waves share heads (statistics) and token rows (filter).  The statistics are accumulated in double and
// rounded once -- the reference's fp32 mean / std carry a summation error this pass does not need to add to; the normalisation
// itself is the reference's fp32 subtraction and IEEE division (a zero spread gives the same inf / NaN).
struct PrepP {
    const float* probs;
    float* cost;
    const int32_t *n_tok, *n_frames;
    int n, L, first_tok, max_frames, width;
    long ldp, ldc;
};

// total order of the reference's sort(): NaN above everything
static __device__ __forceinline__ bool med_less(float a, float b) { return a < b || (a == a && b != b); }

__global__ __launch_bounds__(256) void align_prepare_kernel(const PrepP p) {
    __shared__ float s_mean[ALIGN_MAX_HEADS][64], s_std[ALIGN_MAX_HEADS][64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int b = blockIdx.y;
    int N = p.n_tok[b], S = p.n_frames[b];
    N = min(max(N, 0), p.L - p.first_tok);
    S = min(max(S, 0), p.max_frames);
    const int c0 = blockIdx.x * 56;
    if (N <= 0 || c0 >= S) return;
    const int pw = p.width >> 1;
    const int gc = c0 - 4 + lane;                       // frame column of this lane
    const bool c_ok = gc >= 0 && gc < S;
    const float* W = p.probs + ((long)b * p.n * p.L + p.first_tok) * p.ldp + (c_ok ? gc : 0);
    const long head_stride = (long)p.L * p.ldp;
    for (int h = wave; h < p.n; h += 4) {
        const float* w = W + h * head_stride;
        double sum = 0.0;
#pragma unroll 8
        for (int t = 0; t < N; ++t) sum += (double)w[t * p.ldp];
        const double mean = sum / N;
        double var = 0.0;
#pragma unroll 8
        for (int t = 0; t < N; ++t) {
            const double dv = (double)w[t * p.ldp] - mean;
            var += dv * dv;
        }
        s_mean[h][lane] = (float)mean;
        s_std[h][lane] = (float)sqrt(var / N);
    }
    __syncthreads();
    const bool filter = S > pw && pw > 0;               // TF:53-54: rows no longer than the padding stay unfiltered
    // Window element d of the 9-wide padded window sits at frame offset d - 4 (the real window is centred in it: (9 - width) / 2
    // sentinels on each side, -inf below and NaN above, so that the median of the 9 is the median of the `width`); its source lane,
    // reflected at the borders of [0, S) (only offsets within the real window are used: |offset| <= pw < S)
    int src[ALIGN_MAX_WIDTH];
#pragma unroll
    for (int d = 0; d < ALIGN_MAX_WIDTH; ++d) {
        int g = gc + d - 4;
        g = g < 0 ? -g : g;
        g = g >= S ? 2 * (S - 1) - g : g;
        src[d] = min(max(g - c0 + 4, 0), 63);
    }
    const int o = lane - 4;
    const bool o_ok = o >= 0 && o < 56 && c_ok;
    const float fn = (float)p.n;
    const int lo_pad = (ALIGN_MAX_WIDTH - p.width) >> 1;
    for (int t = wave; t < N; t += 4) {
        float acc = 0.f;
        for (int h = 0; h < p.n; ++h) {
            const float wv = c_ok ? W[h * head_stride + t * p.ldp] : 0.f;
            const float z = (wv - s_mean[h][lane]) / s_std[h][lane];
            float m = z;
            if (filter) {
                float x[ALIGN_MAX_WIDTH];
#pragma unroll
                for (int d = 0; d < ALIGN_MAX_WIDTH; ++d) {
                    const float v = __shfl(z, src[d]);
                    const int e = d - lo_pad;
                    x[d] = e < 0 ? -__builtin_inff() : (e >= p.width ? __builtin_nanf("") : v);
                }
#pragma unroll
                for (int i = 0; i < ALIGN_MAX_WIDTH; ++i) {
                    int rank = 0;
#pragma unroll
                    for (int j = 0; j < ALIGN_MAX_WIDTH; ++j)
                        rank += (med_less(x[j], x[i]) || (!med_less(x[i], x[j]) && j < i)) ? 1 : 0;
                    if (rank == (ALIGN_MAX_WIDTH >> 1)) m = x[i];
                }
            }
            acc += m;
        }
        if (o_ok) p.cost[((long)b * p.L + t) * p.ldc + gc] = -(acc / fn);
    }
}

extern "C" int dw_align_prepare(const float* probs, int B, int n_heads, int L, int64_t ldp, int first_tok,
                                const int32_t* n_tok, const int32_t* n_frames, int max_frames, int median_filter_width,
                                float* cost, int64_t ldc, void* stream) {
    if (!probs || !n_tok || !n_frames || !cost) return DW_EINVAL;
    if (B < 1 || B > 65535 || n_heads < 1 || n_heads > ALIGN_MAX_HEADS || L < 1 || L > ALIGN_MAX_TOK) return DW_EINVAL;
    if (first_tok < 0 || first_tok >= L || max_frames < 1 || ldp < max_frames || ldc < max_frames) return DW_EINVAL;
    if (median_filter_width < 1 || median_filter_width > ALIGN_MAX_WIDTH || !(median_filter_width & 1)) return DW_EINVAL;
    PrepP p{probs, cost, n_tok, n_frames, n_heads, L, first_tok, max_frames, median_filter_width, ldp, ldc};
    DW_CLEAR_ERR();
    hipLaunchKernelGGL(align_prepare_kernel, dim3((max_frames + 55) / 56, B), dim3(256), 0, (hipStream_t)stream, p);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------------
// dw_dtw (TF:generation_whisper.py:64-115 + the jump extraction of :367-369): one workgroup per batch row, thread i owns row i
// of the (n_tok + 1) x (n_frames + 1) table and the workgroup walks its anti-diagonals -- cell (i, j) needs (i-1, j-1), (i-1, j)
// and (i, j-1), all on the two previous diagonals, which live in three rolling LDS rows.  The direction of every cell goes to
// the caller's scratch at two bits per cell (a thread's cells are consecutive frames: one 32-bit store per 16 diagonals), and one
// thread walks the path back.  Every loop is bounded by the table's shape whatever the matrix holds.
// Same path as the reference: its accumulated cost is a float32 array, so each cell is ONE fp32 addition (the float64 matrix
// operand holds fp32 values; rounding the exact sum of two floats through float64 first changes nothing), and the three-way
// choice is made with the same strict comparisons in the same order -- ties, inf and NaN fall through to "left" (2).
struct DtwP {
    const float* cost;
    const int32_t *n_tok, *n_frames;
    uint32_t* trace;
    int32_t* first_frame;
    int L, max_frames;
    long ldc, trace_ld;
};

__global__ __launch_bounds__(ALIGN_MAX_TOK) void dtw_kernel(const DtwP p) {
    __shared__ float diag[3][ALIGN_MAX_TOK + 1];
    const int b = blockIdx.x;
    int N = p.n_tok[b], M = p.n_frames[b];
    N = min(max(N, 0), p.L);
    M = min(max(M, 0), p.max_frames);
    if (N == 0) return;                                 // TF:336-339: the caller's zeros stand
    const int i = threadIdx.x + 1;                      // table row of this thread (token i - 1)
    const float inf = __builtin_inff();
    const float* crow = p.cost + ((long)b * p.L + (i - 1)) * p.ldc;
    uint32_t* trow = p.trace + ((long)b * p.L + (i - 1)) * p.trace_ld;
    // diagonal 0: (0, 0) = 0; diagonal 1: (0, 1) = (1, 0) = inf
    for (int x = threadIdx.x; x <= ALIGN_MAX_TOK; x += ALIGN_MAX_TOK) {
        diag[0][x] = x == 0 ? 0.f : inf;
        diag[1][x] = inf;
        diag[2][x] = inf;
    }
    __syncthreads();
    uint32_t word = 0;
    float m_next = (i <= N && M >= 1 && i == 1) ? crow[0] : 0.f;      // cell (1, 1) sits on diagonal 2
    int ia = 0, ib = 1, ic = 2;                         // rows of `diag` holding diagonals d - 2, d - 1, d
    for (int d = 2; d <= N + M; ++d) {
        const int j = d - i;
        const float m = m_next;
        // the next diagonal's matrix element (cell (i, j + 1)), requested before this diagonal's barrier
        if (i <= N && j + 1 >= 1 && j + 1 <= M) m_next = crow[j];
        if (i <= N) {
            if (j >= 1 && j <= M) {
                const float c0 = diag[ia][i - 1], c1 = diag[ib][i - 1], c2 = diag[ib][i];
                float c;
                uint32_t t;
                if (c0 < c1 && c0 < c2) { c = c0; t = 0; }
                else if (c1 < c0 && c1 < c2) { c = c1; t = 1; }
                else { c = c2; t = 2; }
                diag[ic][i] = m + c;
                word |= t << (2 * ((j - 1) & 15));
                if (((j - 1) & 15) == 15 || j == M) {
                    trow[(j - 1) >> 4] = word;
                    word = 0;
                }
            } else if (j == 0) {
                diag[ic][i] = inf;                      // column 0
            }
        }
        if (threadIdx.x == 0) diag[ic][0] = inf;        // row 0
        __syncthreads();
        const int tmp = ia; ia = ib; ib = ic; ic = tmp;
    }
    __threadfence();
    __syncthreads();
    if (threadIdx.x != 0) return;
    // backtrace (TF:90-107; row 0 of the trace is 2, column 0 is 1) -- first_frame[token] ends as the frame of the path's
    // EARLIEST point on that token: time_indices[jumps] of TF:367-369 (-1 when the path reaches the token in column 0)
    int bi = N, bj = M;
    long cached = -1;
    uint32_t w = 0;
    int32_t* ff = p.first_frame + (long)b * p.L;
    const uint32_t* tbase = p.trace + (long)b * p.L * p.trace_ld;
    for (int step = 0; step < N + M && (bi > 0 || bj > 0); ++step) {
        if (bi > 0) ff[bi - 1] = bj - 1;
        uint32_t t;
        if (bi == 0) t = 2;
        else if (bj == 0) t = 1;
        else {
            const long at = (long)(bi - 1) * p.trace_ld + ((bj - 1) >> 4);
            if (at != cached) { w = __hip_atomic_load(tbase + at, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); cached = at; }
            t = (w >> (2 * ((bj - 1) & 15))) & 3u;
        }
        if (t == 0) { --bi; --bj; }
        else if (t == 1) --bi;
        else --bj;
    }
}

extern "C" int dw_dtw(const float* cost, int B, int L, int64_t ldc, const int32_t* n_tok, const int32_t* n_frames,
                      int max_frames, uint32_t* trace, int64_t trace_ld, int32_t* first_frame, void* stream) {
    if (!cost || !n_tok || !n_frames || !trace || !first_frame) return DW_EINVAL;
    if (B < 1 || L < 1 || L > ALIGN_MAX_TOK || max_frames < 1 || ldc < max_frames) return DW_EINVAL;
    if (trace_ld < (max_frames + 15) / 16) return DW_EINVAL;
    DtwP p{cost, n_tok, n_frames, trace, first_frame, L, max_frames, ldc, trace_ld};
    DW_CLEAR_ERR();
    hipLaunchKernelGGL(dtw_kernel, dim3(B), dim3(ALIGN_MAX_TOK), 0, (hipStream_t)stream, p);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
