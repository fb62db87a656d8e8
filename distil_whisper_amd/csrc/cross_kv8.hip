// FP8 cross-attention K/V for the token step (opt-in: DwDecodeStep.cross_kv_fmt = 1).  The format is stated once, in
// include/dwamd.h ("FP8 cross-attention K/V"): OCP e4m3fn codes with one fp32 scale per (sequence, layer, tensor, column), codes
// head-major uint8 [B][H][src_len][64], scales float [B][2][D].  Two kernels:
//   cross_kv_quant_kernel       once per window and layer: bf16 K | V rows -> codes and scales (not the hot path)
//   attn_decode_proj_kv8_kernel the token step's cross-attention with its projection inside (decode.hip, mode 0) over the codes
#include "common.h"
#include "../../include/dwamd.h"

#define NEG_BIG_D (-1.0e30f)

typedef __attribute__((ext_vector_type(4))) unsigned u32x4;
typedef __attribute__((ext_vector_type(2))) unsigned u32x2;

// ---------------------------------------------------------------------------------------------------------------------
// Quantiser.  One workgroup per (64 columns of K | V = one head of one tensor, sequence): 8 lanes share a row (16 bytes = 8 columns
// each), 32 rows per sweep.  Sweep 1 takes the column maxima, sweep 2 reads the same 128-byte pieces again (192 KB per workgroup
// at 1500 rows: they come from L2) and writes 8 codes per lane -- a row of a head is 64 contiguous bytes of the output.
// ---------------------------------------------------------------------------------------------------------------------
constexpr int QNT = 256;
__global__ __launch_bounds__(QNT) void cross_kv_quant_kernel(const bf16* kv, long ld, uint8_t* k8, uint8_t* v8, float* scales,
                                                             int seq0, int src_len, int H) {
    __shared__ float amax_s[QNT / 8][64];
    __shared__ float inv_s[64];
    const int tid = threadIdx.x, r0 = tid >> 3, c8 = (tid & 7) * 8;
    const int hb = blockIdx.x, sq = blockIdx.y;              // hb < H: K of head hb; hb >= H: V of head hb - H
    const int D = H * 64;
    const bf16* src = kv + (long)sq * src_len * ld + hb * 64 + c8;
    float am[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int j = r0; j < src_len; j += QNT / 8) {
        const bf16x8 x = *(const bf16x8*)(src + (long)j * ld);
#pragma unroll
        for (int e = 0; e < 8; ++e) am[e] = fmaxf(am[e], fabsf(bf2f(x[e])));
    }
#pragma unroll
    for (int e = 0; e < 8; ++e) amax_s[r0][c8 + e] = am[e];
    __syncthreads();
    if (tid < 64) {
        float a = 0.f;
        for (int i = 0; i < QNT / 8; ++i) a = fmaxf(a, amax_s[i][tid]);
        const bool zero = a < 0x1p-100f;                         // (dwamd.h: such a column counts as zero; 448 / a stays finite)
        inv_s[tid] = zero ? 1.f : 448.f / a;
        scales[((long)(seq0 + sq) * 2 + (hb >= H)) * D + (hb % H) * 64 + tid] = zero ? 1.f : a / 448.f;
    }
    __syncthreads();
    float inv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) inv[e] = inv_s[c8 + e];
    uint8_t* dst = (hb >= H ? v8 : k8) + ((long)(seq0 + sq) * H + (hb % H)) * src_len * 64 + c8;
    for (int j = r0; j < src_len; j += QNT / 8) {
        const bf16x8 x = *(const bf16x8*)(src + (long)j * ld);
        float y[8];
#pragma unroll
        for (int e = 0; e < 8; ++e) y[e] = fminf(fmaxf(bf2f(x[e]) * inv[e], -448.f), 448.f);   // (a product only: nothing to contract)
        u32x2 c = {0u, 0u};
        c[0] = __builtin_amdgcn_cvt_pk_fp8_f32(y[0], y[1], c[0], false);
        c[0] = __builtin_amdgcn_cvt_pk_fp8_f32(y[2], y[3], c[0], true);
        c[1] = __builtin_amdgcn_cvt_pk_fp8_f32(y[4], y[5], c[1], false);
        c[1] = __builtin_amdgcn_cvt_pk_fp8_f32(y[6], y[7], c[1], true);
        *(u32x2*)(dst + (long)j * 64) = c;
    }
}

extern "C" int dw_cross_kv_quant(const void* kv, int64_t ld, void* k8, void* v8, float* scales, int seq0, int n_seq, int src_len,
                                 int H, void* stream) {
    DW_CLEAR_ERR();
    if (!kv || !k8 || !v8 || !scales) return DW_EINVAL;
    if (seq0 < 0 || n_seq < 1 || src_len < 1 || H < 1) return DW_EINVAL;
    if (((uintptr_t)kv & 15) || (ld & 7) || (((uintptr_t)k8 | (uintptr_t)v8) & 7) || ((uintptr_t)scales & 3)) return DW_EINVAL;
    if (n_seq > 65535 || H > 16384) return DW_EUNSUP;
    if (ld < 128L * H) return DW_EINVAL;
    hipLaunchKernelGGL(cross_kv_quant_kernel, dim3(2 * H, n_seq), dim3(QNT), 0, (hipStream_t)stream, (const bf16*)kv, (long)ld,
                       (uint8_t*)k8, (uint8_t*)v8, scales, seq0, src_len, H);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Token-step cross-attention with its projection inside, over FP8 K/V.  Workgroup shape, LayerNorm and q projection are those of
// attn_decode_proj_kernel<0, ...> (decode.hip) statement for statement, so that q is bit for bit what that kernel computes
// (tests/test_cross_kv_fp8_gpu.py holds the two together bit for bit through two-key probes); existing instantiations stay as they are.
// Then K's column scales fold into the query and V's into the output, once per workgroup, and the two passes read codes: 4 lanes
// share a key (16 bytes = 16 head dimensions each), 16 keys per wave instruction, eight key groups requested per lane before the
// first is used (64 KiB in flight per workgroup, as in the bf16 kernel).
// ---------------------------------------------------------------------------------------------------------------------
struct DecAttn8P {
    const void* x; long ldx;                   // residual stream [B][D] (f32 or bf16)
    const float* ln_g; const float* ln_b; float eps;
    const bf16* w; const float* bias;          // Wq [D][D], bq [D]
    const uint8_t* k8; const uint8_t* v8;      // codes [B][H][kv_rows][64]
    const float* kv_scale;                     // [B][2][D]
    long kv_rows;
    bf16* o; long ldo;
    int Lk;
    float scale;
};
template <bool XBF>
__device__ __forceinline__ void dec8_ld_x8(const void* x, long off, float (&v)[8]) {
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
// 16 codes of a lane as fp32 (v_cvt_pk_f32_fp8: two codes per instruction, exact)
__device__ __forceinline__ void dec8_codes(const u32x4 c, float (&f)[16]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const f32x2 lo = __builtin_amdgcn_cvt_pk_f32_fp8(c[i], false);
        const f32x2 hi = __builtin_amdgcn_cvt_pk_f32_fp8(c[i], true);
        f[i * 4 + 0] = lo[0]; f[i * 4 + 1] = lo[1]; f[i * 4 + 2] = hi[0]; f[i * 4 + 3] = hi[1];
    }
}
constexpr int DEC8_NW = 8;                     // waves per workgroup, as DEC_NW of decode.hip
template <bool XBF, int NI>                    // NI = D / 64
__global__ __launch_bounds__(64 * DEC8_NW, 4) void attn_decode_proj_kv8_kernel(const DecAttn8P p) {
    extern __shared__ __attribute__((aligned(16))) float dsm[];
    // [Lk scores (x4) | NW x 64 partial outputs | NW | NW | NW (sums) | 64 q | 64 V scales | 64 unused | D bf16 normalised row | D f32 row]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int h = blockIdx.y, b = blockIdx.z;
    constexpr int D = NI * 64;
    const int Lk = p.Lk;
    float* sc = dsm;
    float* part = dsm + ((p.Lk + 3) & ~3);
    float* redm = part + DEC8_NW * 64;
    float* redl = redm + DEC8_NW;
    float* reds = redl + DEC8_NW;
    float* qs = reds + DEC8_NW;
    float* svs = qs + 64;
    bf16* lnb = (bf16*)(svs + 128);
    float* xrow = (float*)(lnb + D);
    const float c = p.scale * 1.4426950408889634f;
    // ---- projection (decode.hip, attn_decode_proj_kernel: same statements, same order) ----
    const int j = tid >> 3, l = tid & 7;
    bf16x8 wf[NI];
    const bf16* const wrow0 = p.w + (long)(h * 64 + j) * D + l * 8;
#pragma unroll
    for (int i = 0; i < NI; ++i) wf[i] = *(const bf16x8*)(wrow0 + i * 64);
    {
        if (tid < (D >> 3)) {
            float xv[8];
            dec8_ld_x8<XBF>(p.x, (long)b * p.ldx + tid * 8, xv);
            *(f32x4*)(xrow + tid * 8) = f32x4{xv[0], xv[1], xv[2], xv[3]};
            *(f32x4*)(xrow + tid * 8 + 4) = f32x4{xv[4], xv[5], xv[6], xv[7]};
        }
        __syncthreads();
        const bool has = tid < (D >> 2);
        float s1 = 0.f;
        if (has) { const f32x4 a = *(const f32x4*)(xrow + tid * 4); s1 = (a[0] + a[1]) + (a[2] + a[3]); }
        const float mu = block_sum<64 * DEC8_NW>(s1, reds) / (float)D;
        float s2 = 0.f;
        if (has) {
            const f32x4 a = *(const f32x4*)(xrow + tid * 4);
#pragma unroll
            for (int e = 0; e < 4; ++e) { const float dd = a[e] - mu; s2 += dd * dd; }
        }
        const float rs = rsqrtf(block_sum<64 * DEC8_NW>(s2, reds) / (float)D + p.eps);
        f32x4 g4 = {0.f, 0.f, 0.f, 0.f}, b4 = {0.f, 0.f, 0.f, 0.f};
        if (has) {
            g4 = *(const f32x4*)(p.ln_g + tid * 4);
            b4 = *(const f32x4*)(p.ln_b + tid * 4);
        }
        asm volatile("" : "+v"(g4), "+v"(b4));
        if (has) {
            const f32x4 a = *(const f32x4*)(xrow + tid * 4);
            bf16x4 y;
#pragma unroll
            for (int e = 0; e < 4; ++e) y[e] = f2bf((a[e] - mu) * rs * g4[e] + b4[e]);
            *(bf16x4*)(lnb + tid * 4) = y;
        }
        __syncthreads();
    }
    {
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
        const float* const sK = p.kv_scale + (long)b * 2 * D + h * 64;
        // q . c as the bf16 kernel holds it, then K's column scale: score = sum_d (q_d c sK_d) float(code)
        if (l == 0) qs[j] = (bf2f(f2bf(acc + p.bias[h * 64 + j])) * c) * sK[j];
        if (l == 1) svs[j] = sK[D + j];
    }
    __syncthreads();
    // ---- attention over Lk keys: 4 lanes share a key (16 bytes = 16 head dimensions each) ----
    const int sub = lane >> 2, ds = (lane & 3) * 16;
    const uint8_t* K = p.k8 + ((long)b * gridDim.y + h) * p.kv_rows * 64 + ds;
    const uint8_t* V = p.v8 + ((long)b * gridDim.y + h) * p.kv_rows * 64 + ds;
    float qv[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) qv[e] = qs[ds + e];
    constexpr int UN = 8;                                // key groups requested ahead per lane
    constexpr int KG = 16;                               // keys per wave instruction
    float mx = NEG_BIG_D;
    for (int k0 = wave * KG; k0 < Lk; k0 += UN * DEC8_NW * KG) {
        u32x4 kr[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            int k = k0 + u * DEC8_NW * KG + sub;
            k = k < Lk ? k : Lk - 1;
            kr[u] = ld_stream<2>((const u32x4*)(K + (long)k * 64));
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int k = k0 + u * DEC8_NW * KG + sub;
            float kf[16];
            dec8_codes(kr[u], kf);
            float s = 0.f;
#pragma unroll
            for (int e = 0; e < 16; ++e) s = fmaf(qv[e], kf[e], s);
            s += __shfl_xor(s, 1);
            s += __shfl_xor(s, 2);
            if (k < Lk) {
                if ((lane & 3) == 0) sc[k] = s;
                mx = fmaxf(mx, s);
            }
        }
    }
    mx = wave_max(mx);
    if (lane == 0) redm[wave] = mx;
    __syncthreads();
    mx = redm[0];
#pragma unroll
    for (int i = 1; i < DEC8_NW; ++i) mx = fmaxf(mx, redm[i]);
    float o[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) o[e] = 0.f;
    float lsum = 0.f;
    for (int k0 = wave * KG; k0 < Lk; k0 += UN * DEC8_NW * KG) {
        u32x4 vr[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            int k = k0 + u * DEC8_NW * KG + sub;
            k = k < Lk ? k : Lk - 1;
            vr[u] = ld_stream<2>((const u32x4*)(V + (long)k * 64));
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int k = k0 + u * DEC8_NW * KG + sub;
            if (k < Lk) {
                const float pv = __builtin_amdgcn_exp2f(sc[k] - mx);
                lsum += pv;
                const float pb = round_bf16(pv);
                float vf[16];
                dec8_codes(vr[u], vf);
#pragma unroll
                for (int e = 0; e < 16; ++e) o[e] = fmaf(pb, vf[e], o[e]);
            }
        }
    }
    lsum = (lane & 3) == 0 ? lsum : 0.f;
    lsum = wave_sum(lsum);
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        o[e] += __shfl_xor(o[e], 4);
        o[e] += __shfl_xor(o[e], 8);
        o[e] += __shfl_xor(o[e], 16);
        o[e] += __shfl_xor(o[e], 32);
    }
    if (sub == 0) {
#pragma unroll
        for (int e = 0; e < 16; ++e) part[wave * 64 + ds + e] = o[e];
    }
    if (lane == 0) redl[wave] = lsum;
    __syncthreads();
    if (wave == 0) {
        float acc = 0.f, lt = 0.f;
#pragma unroll
        for (int i = 0; i < DEC8_NW; ++i) { acc += part[i * 64 + lane]; lt += redl[i]; }
        p.o[(long)b * p.ldo + h * 64 + lane] = f2bf(svs[lane] * (acc / lt));
    }
}

template <bool XBF>
static int launch_kv8_ni(const DecAttn8P& p, int D, const dim3& grid, const dim3& block, size_t smem, hipStream_t s) {
    switch (D >> 6) {
#define DW_NI(n) case n: hipLaunchKernelGGL((attn_decode_proj_kv8_kernel<XBF, n>), grid, block, smem, s, p); break;
        DW_NI(6) DW_NI(8) DW_NI(12) DW_NI(16) DW_NI(20)        // d_model 384 / 512 / 768 / 1024 / 1280
#undef DW_NI
        default: return DW_EUNSUP;
    }
    DW_CHECK_LAUNCH();
    return DW_OK;
}

extern "C" int dw_decode_attn_proj_kv8(const void* x, int x_dtype, int64_t ldx, const float* ln_g, const float* ln_b, float eps,
                                       const void* w, const float* bias, const void* k8, const void* v8, const float* kv_scale,
                                       int64_t kv_rows, void* o, int64_t ldo, int B, int H, int Lk, float scale, void* stream) {
    DW_CLEAR_ERR();
    if (x_dtype != DW_F32 && x_dtype != DW_BF16) return DW_EINVAL;
    if (!x || !ln_g || !ln_b || !w || !bias || !k8 || !v8 || !kv_scale || !o) return DW_EINVAL;
    if (B <= 0 || H <= 0 || Lk < 1 || Lk > kv_rows) return DW_EINVAL;
    // 16-byte loads: the row of x, the weight fragments, the code groups, four floats of gamma / beta per lane
    if ((((uintptr_t)x | (uintptr_t)w | (uintptr_t)k8 | (uintptr_t)v8 | (uintptr_t)ln_g | (uintptr_t)ln_b) & 15) || (ldx & 7))
        return DW_EINVAL;
    if ((((uintptr_t)bias | (uintptr_t)kv_scale) & 3) || ((uintptr_t)o & 1)) return DW_EINVAL;
    const int D = H * 64;
    if (B > 65535 || H > 65535 || !(D == 384 || D == 512 || D == 768 || D == 1024 || D == 1280) || Lk > 8192) return DW_EUNSUP;
    if (ldx < D || ldo < D) return DW_EINVAL;
    DecAttn8P p = {};
    p.x = x; p.ldx = ldx; p.ln_g = ln_g; p.ln_b = ln_b; p.eps = eps;
    p.w = (const bf16*)w; p.bias = bias;
    p.k8 = (const uint8_t*)k8; p.v8 = (const uint8_t*)v8; p.kv_scale = kv_scale; p.kv_rows = kv_rows;
    p.o = (bf16*)o; p.ldo = ldo; p.Lk = Lk; p.scale = scale;
    const size_t smem = ((((size_t)Lk + 3) & ~(size_t)3) + DEC8_NW * 64 + 3 * DEC8_NW + 3 * 64) * 4 + (size_t)D * 6;
    const dim3 grid(1, H, B), block(64 * DEC8_NW);
    return x_dtype == DW_BF16 ? launch_kv8_ni<true>(p, D, grid, block, smem, (hipStream_t)stream)
                              : launch_kv8_ni<false>(p, D, grid, block, smem, (hipStream_t)stream);
}
