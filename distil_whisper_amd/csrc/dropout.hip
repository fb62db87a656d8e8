// Training-mode dropout of the student (TF:modeling_whisper.py WhisperEncoder.forward / WhisperDecoder.forward: the embeddings;
// WhisperEncoderLayer / WhisperDecoderLayer: the three residual branches with `dropout`, the GELU output of fc1 with
// `activation_dropout`) for gfx950.  Streaming kernels in the style of elementwise.hip: one lane owns 8 consecutive elements
// of a row (one 16-byte bf16 access, two for fp32) and the ONE mask byte that covers them, rows are independent, no LDS.
// The mask comes from a counter-based generator (Philox4x32-10, Salmon et al., SC'11), so an element's bit depends only
// on (seed, step, site, element index): no generator state is carried between launches, and the step counter is read from
// device memory so that a replayed HIP graph draws fresh masks.
#include "common.h"
#include "../../include/dwamd.h"

#define PHILOX_M0 0xD2511F53u
#define PHILOX_M1 0xCD9E8D57u
#define PHILOX_W0 0x9E3779B9u
#define PHILOX_W1 0xBB67AE85u

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
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

// 8 consecutive elements at element offset i of a bf16 / f32 buffer (16-byte aligned by the launchers' checks)
__device__ __forceinline__ void load8(const void* p, int dt, long i, float v[8]) {
    if (dt == DW_BF16) {
        const bf16x8 t = *(const bf16x8*)((const bf16*)p + i);
#pragma unroll
        for (int e = 0; e < 8; ++e) v[e] = bf2f(t[e]);
    } else {
        const f32x4 a = *(const f32x4*)((const float*)p + i);
        const f32x4 b = *(const f32x4*)((const float*)p + i + 4);
#pragma unroll
        for (int e = 0; e < 4; ++e) { v[e] = a[e]; v[4 + e] = b[e]; }
    }
}
__device__ __forceinline__ void store8(void* p, int dt, long i, const float v[8]) {
    if (dt == DW_BF16) {
        bf16x8 t;
#pragma unroll
        for (int e = 0; e < 8; ++e) t[e] = f2bf(v[e]);
        *(bf16x8*)((bf16*)p + i) = t;
    } else {
        f32x4 a, b;
#pragma unroll
        for (int e = 0; e < 4; ++e) { a[e] = v[e]; b[e] = v[4 + e]; }
        *(f32x4*)((float*)p + i) = a;
        *(f32x4*)((float*)p + i + 4) = b;
    }
}

// out = residual + m * t,  t = u * scale, rounded to bf16 when u is bf16 (the reference multiplies in the tensor's dtype)
__global__ __launch_bounds__(256) void dropout_fwd_kernel(const void* u, int udt, long ldu, const void* res, int rdt, long ldr,
                                                          void* out, int odt, long ldo, uint8_t* mask, long nvec, int cols,
                                                          uint32_t thr, float scale, uint32_t k0, uint32_t k1, uint32_t site,
                                                          const uint64_t* step) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvec) return;
    const int vpr = cols >> 3;
    const long row = v / vpr;
    const int col = (int)(v - row * vpr) << 3;
    float x[8], r[8];
    load8(u, udt, row * ldu + col, x);
    if (res) load8(res, rdt, row * ldr + col, r);
    const uint64_t st = step[0];
    const uint64_t e = (uint64_t)row * (uint64_t)cols + (uint64_t)col;       // < 2^34 (launcher), a multiple of 8
    uint32_t w[8];
    philox4x32_10((uint32_t)(e >> 2), site, (uint32_t)st, (uint32_t)(st >> 32), k0, k1, w);
    philox4x32_10((uint32_t)(e >> 2) + 1u, site, (uint32_t)st, (uint32_t)(st >> 32), k0, k1, w + 4);
    uint32_t bits = 0;
    float y[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const bool keep = w[j] >= thr;
        bits |= (keep ? 1u : 0u) << j;
        float t = __fmul_rn(x[j], scale);          // (never contracted into the residual add)
        if (udt == DW_BF16) t = round_bf16(t);
        t = keep ? t : 0.f;
        y[j] = res ? r[j] + t : t;
    }
    store8(out, odt, row * ldo + col, y);
    mask[v] = (uint8_t)bits;
}

// out = m * t,  t = dy * scale, rounded to bf16 when dy is bf16
__global__ __launch_bounds__(256) void dropout_bwd_kernel(const void* dy, int ydt, long ldy, const uint8_t* mask, void* out,
                                                          int odt, long ldo, long nvec, int cols, float scale) {
    const long v = (long)blockIdx.x * 256 + threadIdx.x;
    if (v >= nvec) return;
    const int vpr = cols >> 3;
    const long row = v / vpr;
    const int col = (int)(v - row * vpr) << 3;
    float x[8], y[8];
    load8(dy, ydt, row * ldy + col, x);
    const uint32_t bits = mask[v];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float t = __fmul_rn(x[j], scale);          // (never contracted into the residual add)
        if (ydt == DW_BF16) t = round_bf16(t);
        y[j] = ((bits >> j) & 1u) ? t : 0.f;
    }
    store8(out, odt, row * ldo + col, y);
}

__global__ void dropout_tick_kernel(uint64_t* step) {
    if (threadIdx.x == 0 && blockIdx.x == 0) step[0] += 1;
}

static bool bad_operand(const void* p, int dt, int64_t ld, int cols) {
    if (dt != DW_F32 && dt != DW_BF16) return true;
    const int64_t q = dt == DW_BF16 ? 8 : 4;                  // elements per 16 bytes
    return ((uintptr_t)p & 15) || ld < cols || (ld % q);
}

extern "C" int dw_dropout_fwd(const void* u, int u_dtype, int64_t ldu, const void* residual, int r_dtype, int64_t ldr,
                              void* out, int out_dtype, int64_t ldo, uint8_t* mask, int rows, int cols, uint32_t thr,
                              float scale, uint64_t seed, int site, const uint64_t* step, void* stream) {
    DW_CLEAR_ERR();
    if (!u || !out || !mask || !step || rows <= 0 || cols <= 0 || (cols & 7) || site < 0) return DW_EINVAL;
    if (bad_operand(u, u_dtype, ldu, cols) || bad_operand(out, out_dtype, ldo, cols)) return DW_EINVAL;
    if (residual && bad_operand(residual, r_dtype, ldr, cols)) return DW_EINVAL;
    if ((int64_t)rows * cols >= ((int64_t)1 << 34)) return DW_EUNSUP;      // the element index fills counter word 0 only
    const long nvec = (long)rows * (cols >> 3);
    hipLaunchKernelGGL(dropout_fwd_kernel, dim3((nvec + 255) / 256), dim3(256), 0, (hipStream_t)stream, u, u_dtype, (long)ldu,
                       residual, r_dtype, (long)ldr, out, out_dtype, (long)ldo, mask, nvec, cols, thr, scale, (uint32_t)seed,
                       (uint32_t)(seed >> 32), (uint32_t)site, step);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

extern "C" int dw_dropout_bwd(const void* dy, int dy_dtype, int64_t lddy, const uint8_t* mask, void* out, int out_dtype,
                              int64_t ldo, int rows, int cols, float scale, void* stream) {
    DW_CLEAR_ERR();
    if (!dy || !out || !mask || rows <= 0 || cols <= 0 || (cols & 7)) return DW_EINVAL;
    if (bad_operand(dy, dy_dtype, lddy, cols) || bad_operand(out, out_dtype, ldo, cols)) return DW_EINVAL;
    const long nvec = (long)rows * (cols >> 3);
    hipLaunchKernelGGL(dropout_bwd_kernel, dim3((nvec + 255) / 256), dim3(256), 0, (hipStream_t)stream, dy, dy_dtype, (long)lddy,
                       mask, out, out_dtype, (long)ldo, nvec, cols, scale);
    DW_CHECK_LAUNCH();
    return DW_OK;
}

extern "C" int dw_dropout_tick(uint64_t* step, void* stream) {
    DW_CLEAR_ERR();
    if (!step) return DW_EINVAL;
    hipLaunchKernelGGL(dropout_tick_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, step);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
