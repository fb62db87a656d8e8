// Grouped weight-gradient GEMM (dw_wgrad_group): C_i (+)= A_i^T . B_i for up to four problems that share the contraction length k,
// both operands k-major bf16, ONE launch, one 320 x 256 output tile per workgroup and no K slices.
//
// Why: a weight matrix alone is 25-100 tiles of 256 x 256 and k = all tokens is very long, so dw_gemm_bf16 cuts k into 5 or 10
// slices to give every CU a job -- each slice stores an fp32 slab and dw_reduce_slices_ld adds the slabs (13 bytes of HBM traffic per
// byte of gradient, a prologue and an epilogue per 75-150 K tiles).  The four matrices of an encoder layer TOGETHER are 20 + 60 + 80
// + 80 = 240 tiles of 320 x 256: one round of the 256 CUs, one prologue and one epilogue per workgroup, one fp32 chain over k per
// output element straight from the accumulators into the gradient buffer, nothing to combine.
//
// The K loop is the eight-wave 16x16x32 loop of gemm_wp16.h (same sub-steps, same DMA halves, same pinned interleave) at HM = 5 row
// blocks per sub-step; what is this kernel's own:
//   * the k-major A image of 320 columns.  A k row is 40 slots of 16 bytes, and the 5-bit XOR of swk16 would leave it; 1 KiB DMA
//     pieces are 1.6 rows of it.  The image is therefore TWO images per stage: columns [0, 256) as [64][256] with swk16 (pieces of
//     two k rows, 32 per K tile: four per wave, a uniform stride of 16 k rows apart -- one lane offset, the stride in the scalar
//     offset), and columns [256, 320) as [64][64] behind it (32 KiB into the stage) with swk64 below (pieces of eight k rows: one per
//     wave, a second lane offset);
//   * the wave's rows.  Wave row wr (wave / 4) owns columns [128 wr, 128 wr + 128) of the first image (row blocks 0-7) and columns
//     [32 wr, 32 wr + 32) of the second (row blocks 8, 9): every fragment address is the same expression in both wave rows.  Its
//     output rows are m0 + 128 wr + [0, 128) and m0 + 256 + 32 wr + [0, 32): the fifth 32-row slab of the epilogue is displaced
//     (gemm_epilogue TAILED);
//   * the job: blockIdx.x -> (problem, tile_m, tile_n) from the problem list in the kernel arguments (a captured step replays it
//     unchanged).  Workgroup L runs on XCD L % 8; each XCD owns a contiguous range of the job list, and within a problem the list
//     runs fastest along the dimension with FEWER tiles, so the ~30 tiles of an XCD are a compact block of (tile_m, tile_n) that
//     shares a dozen operand panels in its L2 (fc1: 6 x 5 tiles on 11 panels; the other way round 30 tiles would stream 22).  No
//     dynamic hand-out: every job is k / 64 K tiles long.
// Epilogue: gemm_epilogue's fp32 run-time walk through the waves' LDS patches (full 128-byte rows) -- plain stores, or the fp32
// residual read-add-store with R = C, unrounded (accumulate).  No bias, no activation, no float atomics.
#include "gemm_wp16.h"

struct WgradGroupP {
    DwWgradProblem pr[DW_WGRAD_GROUP_MAX];
    int first[DW_WGRAD_GROUP_MAX];     // first job of problem i; the total for i >= count
    int total, k, accumulate;
};

// k-major image [64][64] (128-byte k rows): 16-byte slot s of k row r is stored at slot s ^ swk64(r).  A fragment read's 32 lanes of
// a pass take 32 bytes each of k rows {0..3, 8..11} + 16 j; row r starts 128 (r & 1) bytes into the 256 bytes of the 64 banks, and
// the XOR moves bit 1 of r by 32 and bit 3 by 64 bytes: eight rows, eight different 32-byte bank groups.  (swk16 is the same idea
// for 512-byte rows, which all start at bank 0: bits 0, 1 and 3 of r.)  swk64(r) == swk64(r + 4): one swizzle for both reads.
__device__ __forceinline__ int swk64(int krow) { return (((krow >> 1) & 1) << 1) | (((krow >> 3) & 1) << 2); }
// frag_kmajor16 on that image
__device__ __forceinline__ bf16x8 frag_kmajor16_w64(const char* tile, int x, int ks, int lane) {
    const int g = lane >> 4, p = lane & 15;
    const int col = x + ((p & 3) << 2);
    const int k0 = ks * 32 + g * 8 + (p >> 2);
    const int sw = (((p >> 3) & 1) << 1) | ((g & 1) << 2);      // swk64(k0) = swk64(k0 + 4)
    const char* a0 = tile + k0 * 128 + (((col >> 3) ^ sw) << 4) + ((p & 1) << 3);
    const char* a1 = a0 + 4 * 128;
    const bf16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)a0);
    const bf16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4bf16((lds_bf16x4_t*)a1);
    bf16x8 r;
    r[0] = lo[0]; r[1] = lo[1]; r[2] = lo[2]; r[3] = lo[3];
    r[4] = hi[0]; r[5] = hi[1]; r[6] = hi[2]; r[7] = hi[3];
    return r;
}

__global__ __launch_bounds__(512, 2) void wgrad_group_kernel(const WgradGroupP g) {
    constexpr int BM = 320, BN = 256, WN = 4, NW = 8, TN = BN / WN;
    constexpr int FM = BM / 2 / 16, FN = TN / 16, HM = FM / 2;      // 10 x 4 blocks of 16 x 16 per wave, 5 row blocks per sub-step
    constexpr int CPA = BM / 8 / NW, CPB = BN / 8 / NW;             // DMA pieces (1 KiB) per wave per operand per K tile: 5, 4
    constexpr int NA0 = (CPA + 1) / 2, NB0 = CPB / 2;
    constexpr int NH0 = NA0 + NB0, NH1 = CPA + CPB - NH0;
    constexpr int STAGE = (BM + BN) * 128, IMG1 = 256 * 128;        // one K tile: A [64][256] | A [64][64] | B [64][256]
    static_assert(NH0 == 5 && CPA == 5 && CPB == 4, "piece split");
    __shared__ __attribute__((aligned(1024))) char smem[2 * STAGE];

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int wr = wave / WN, wn0 = (wave % WN) * TN;
    const unsigned smem_w = wp_lds_addr(smem) + (unsigned)(wave * 1024);

    // ---- the job (see the head of the file) ----
    const int bid = blockIdx.x, xcd = bid & 7, local = bid >> 3;
    const int q = g.total >> 3, r = g.total & 7;
    if (local >= q + (xcd < r ? 1 : 0)) return;
    const int id = (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + local;
    int pi = 0;
#pragma unroll
    for (int i = 1; i < DW_WGRAD_GROUP_MAX; ++i)
        if (id >= g.first[i]) pi = i;
    GemmP p{};
    p.a = (const bf16*)g.pr[pi].a; p.b = (const bf16*)g.pr[pi].b; p.c = g.pr[pi].c;
    p.lda = g.pr[pi].lda; p.ldb = g.pr[pi].ldb; p.ldc = g.pr[pi].ldc;
    p.m = g.pr[pi].m; p.n = g.pr[pi].n; p.k = g.k;
    p.c_dtype = DW_F32; p.vec = 1; p.split_k = 1;
    if (g.accumulate) { p.r = p.c; p.ldr = p.ldc; p.r_dtype = DW_F32; }      // C += : the unrounded fp32 residual walk with R = C
    const int within = id - g.first[pi];
    const int tiles_m = p.m / BM, tiles_n = p.n / BN;
    int tm, tn;
    if (tiles_m <= tiles_n) { tn = within / tiles_m; tm = within - tn * tiles_m; }
    else { tm = within / tiles_n; tn = within - tm * tiles_n; }
    const int m0 = tm * BM, n0 = tn * BN;

    // ---- DMA sources: descriptor = the tile's first k row, voffset = the per-lane part, soffset = K advance + piece stride ----
    unsigned offA0, offA1, offB0;
    {
        const int krow = wave * 2 + (lane >> 5);                    // images of 256 columns: piece wave + 8 i = k rows 2 (wave + 8 i), + 1
        offA0 = (unsigned)((krow * (int)p.lda + (((lane & 31) ^ swk16(krow)) << 3)) * 2);
        offB0 = (unsigned)((krow * (int)p.ldb + (((lane & 31) ^ swk16(krow)) << 3)) * 2);
        const int krow1 = wave * 8 + (lane >> 3);                   // image of 64 columns: piece `wave` = k rows 8 wave .. 8 wave + 7
        offA1 = (unsigned)((krow1 * (int)p.lda + 256 + (((lane & 7) ^ swk64(krow1)) << 3)) * 2);
    }
    const int stepA = 128 * (int)p.lda, stepB = 128 * (int)p.ldb;
    const int pieceA = NW * 2 * (int)p.lda * 2, pieceB = NW * 2 * (int)p.ldb * 2;
    const int nt = p.k >> 6;
    const i32x4_t rsA = wp_rsrc(p.a + m0), rsB = wp_rsrc(p.b + n0);
    int kA = 0, kB = 0;

    f32x4 acc[FM][FN];
#pragma unroll
    for (int i = 0; i < FM; ++i)
#pragma unroll
        for (int j = 0; j < FN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    // load j of half h of the K tile at (kA, kB) into LDS buffer `buf` (A and B pieces alternate, A first; as gemm_wp16.h)
    auto dma1 = [&](auto hc, auto jc, int buf) __attribute__((always_inline)) {
        constexpr int h = decltype(hc)::value, j = decltype(jc)::value;
        constexpr int na = h ? CPA - NA0 : NA0, nb = h ? CPB - NB0 : NB0, nmin = na < nb ? na : nb;
        constexpr bool isA = j < 2 * nmin ? (j & 1) == 0 : na > nb;
        constexpr int idx = j < 2 * nmin ? j / 2 : j - nmin;
        constexpr int i = (isA ? (h ? NA0 : 0) : (h ? NB0 : 0)) + idx;
        static_assert(j < na + nb, "load index");
        const unsigned lb = smem_w + (unsigned)(buf * STAGE);
        if constexpr (isA && i == CPA - 1) wp_dma16i<IMG1>(rsA, lb, offA1, kA);
        else if constexpr (isA) wp_dma16p<i * (NW * 1024)>(rsA, lb, offA0, kA, i * pieceA);
        else wp_dma16p<i * (NW * 1024) + BM * 128>(rsB, lb, offB0, kB, i * pieceB);
    };
    auto dma = [&](auto hc, int buf) __attribute__((always_inline)) {
        static_for<0, (decltype(hc)::value ? NH1 : NH0)>([&](auto jc) __attribute__((always_inline)) { dma1(hc, jc, buf); });
    };

    bf16x8 aX[HM], aY[HM], bq[FN];        // A fragments of row half 0 / half 1; the k step's B fragments
    auto ldA1 = [&](bf16x8 (&dst)[HM], auto ic, int kstep, auto hc, int buf) __attribute__((always_inline)) {
        constexpr int blk = decltype(hc)::value * HM + decltype(ic)::value;
        const char* tA = smem + buf * STAGE;
        if constexpr (blk < 8) dst[decltype(ic)::value] = frag_kmajor16<256>(tA, wr * 128 + blk * 16, kstep, lane);
        else dst[decltype(ic)::value] = frag_kmajor16_w64(tA + IMG1, wr * 32 + (blk - 8) * 16, kstep, lane);
    };
    auto ldB1 = [&](auto jc, int kstep, int buf) __attribute__((always_inline)) {
        constexpr int j = decltype(jc)::value;
        bq[j] = frag_kmajor16<BN>(smem + buf * STAGE + BM * 128, wn0 + j * 16, kstep, lane);
    };
    // One sub-step (gemm_wp16.h): the HM x FN MFMAs of row half H, column-major, the operand loads of DMA half VH - 1 in the gaps of
    // column 0, the A fragments of the NEXT sub-step (half HN of k step kn of buffer bn) in the gaps of the first column without
    // DMA, the B fragments of the next k step each right behind the last MFMA of its column.
    auto substep = [&](auto hc, bf16x8 (&a)[HM], auto lac, bf16x8 (&an)[HM], int kn, auto hnc, int bn, auto rbc, int kb, int bb,
                       auto vhc, int dbuf) __attribute__((always_inline)) {
        constexpr int H = decltype(hc)::value;
        constexpr bool LA = decltype(lac)::value != 0, RB = decltype(rbc)::value != 0;
        constexpr int VH = decltype(vhc)::value;
        constexpr int NLD = VH == 1 ? NH0 : (VH == 2 ? NH1 : 0);
        constexpr int A0 = NLD > 0 ? HM : 0;
        static_assert(NLD <= HM, "operand loads of a half ride on the MFMAs of column 0");
        __builtin_amdgcn_sched_barrier(0);
        static_for<0, HM * FN>([&](auto qc) __attribute__((always_inline)) {
            constexpr int q = decltype(qc)::value, i = q % HM, j = q / HM;
            if constexpr (RB && i == 0 && j > 0) ldB1(std::integral_constant<int, j - 1>{}, kb, bb);
            acc[H * HM + i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(bq[j], a[i], acc[H * HM + i][j], 0, 0, 0);
            if constexpr (q < NLD) dma1(std::integral_constant<int, (VH > 0 ? VH - 1 : 0)>{}, qc, dbuf);
            if constexpr (LA && q >= A0 && q < A0 + HM) ldA1(an, std::integral_constant<int, q - A0>{}, kn, hnc, bn);
            __builtin_amdgcn_sched_barrier(0);
        });
        if constexpr (RB) { ldB1(std::integral_constant<int, FN - 1>{}, kb, bb); __builtin_amdgcn_sched_barrier(0); }
    };
    using I0 = std::integral_constant<int, 0>;
    using I1 = std::integral_constant<int, 1>;
    using I2 = std::integral_constant<int, 2>;
    auto pinA = [&](bf16x8 (&a)[HM]) __attribute__((always_inline)) {      // (ONE statement: one lgkmcnt wait for the set)
        asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]));
    };

    // ---- prologue: tile 0 whole, first half of tile 1, fragments of (tile 0, k step 0): A half 0 and B ----
    dma(I0{}, 0); dma(I1{}, 0);
    kA += stepA; kB += stepB;
    if (nt > 1) {
        dma(I0{}, 1);
        asm volatile("s_waitcnt vmcnt(5)" ::: "memory");      // (NH0: tile 0 has landed when only tile 1's first half is outstanding)
    } else wait_vm0();
    __syncthreads();
    static_for<0, HM>([&](auto ic) __attribute__((always_inline)) { ldA1(aX, ic, 0, I0{}, 0); });
    static_for<0, FN>([&](auto jc) __attribute__((always_inline)) { ldB1(jc, 0, 0); });
    __builtin_amdgcn_sched_barrier(0);

    // one K tile; MORE1: tile t+1 exists, MORE2: tile t+2 exists.  (kA, kB) point at tile t+1 on entry.
    // Entering: aX = A(t, k step 0, half 0), bq = B(t, k step 0).
    auto body = [&](auto m1c, auto m2c, int t) {
        constexpr bool MORE1 = decltype(m1c)::value, MORE2 = decltype(m2c)::value;
        const int buf = t & 1;
        // sub-step 0: (k step 0, half 0); refill aY <- (k step 0, half 1); second half of tile t+1's DMA
        pinA(aX);
        if constexpr (MORE1) { substep(I0{}, aX, I1{}, aY, 0, I1{}, buf, I0{}, 0, 0, I2{}, buf ^ 1); kA += stepA; kB += stepB; }
        else substep(I0{}, aX, I1{}, aY, 0, I1{}, buf, I0{}, 0, 0, I0{}, 0);
        // sub-step 1: (k step 0, half 1); refill aX <- (k step 1, half 0), bq <- B(k step 1) column by column
        pinA(aY);
        substep(I1{}, aY, I1{}, aX, 1, I0{}, buf, I1{}, 1, buf, I0{}, 0);
        // sub-step 2: (k step 1, half 0); refill aY <- (k step 1, half 1)
        pinA(aX);
        substep(I0{}, aX, I1{}, aY, 1, I1{}, buf, I0{}, 0, 0, I0{}, 0);
        // every wave: its DMA pieces of tile t+1 have landed, its last fragments of tile t are in registers
        pinA(aY);
        if constexpr (MORE1) {
            wait_vm0();
            __builtin_amdgcn_s_barrier();
            __builtin_amdgcn_sched_barrier(0);
        }
        // sub-step 3: (k step 1, half 1); refill aX, bq <- tile t+1, k step 0; first half of tile t+2's DMA
        if constexpr (MORE2) substep(I1{}, aY, I1{}, aX, 0, I0{}, buf ^ 1, I1{}, 0, buf ^ 1, I1{}, buf);
        else if constexpr (MORE1) substep(I1{}, aY, I1{}, aX, 0, I0{}, buf ^ 1, I1{}, 0, buf ^ 1, I0{}, 0);
        else substep(I1{}, aY, I0{}, aX, 0, I0{}, 0, I0{}, 0, 0, I0{}, 0);
    };
    int t = 0;
    for (; t + 2 < nt; ++t) body(std::true_type{}, std::true_type{}, t);
    if (nt >= 2) { body(std::true_type{}, std::false_type{}, t); ++t; }
    body(std::false_type{}, std::false_type{}, t);

    // wave rows: m0 + 128 wr + [0, 128), then the displaced fifth slab at m0 + 256 + 32 wr (128 - 96 wr rows behind the fourth)
    gemm_epilogue<FM / 2, FN / 2, TN, 4, GemmNoHook, true, 16, 0, f32x4[FM][FN], true>(p, acc, smem + STAGE, wave, lane, m0, wr * 128, n0, wn0, 0,
                                                                                     GemmNoHook(), nullptr, 128 - 96 * wr);
}

extern int g_gemm_cus;     // gemm.hip

extern "C" int dw_wgrad_group(const DwWgradProblem* problems, int count, int k, int accumulate, void* stream) {
    DW_CLEAR_ERR();
    if (!problems || count < 1 || count > DW_WGRAD_GROUP_MAX || k <= 0 || (k & 63)) return DW_EINVAL;
    WgradGroupP g{};
    long total = 0;
    for (int i = 0; i < count; ++i) {
        const DwWgradProblem& q = problems[i];
        if (!q.a || !q.b || !q.c || q.m <= 0 || q.n <= 0 || q.m % 320 || q.n % 256) return DW_EINVAL;
        if (((uintptr_t)q.a & 15) || ((uintptr_t)q.b & 15) || ((uintptr_t)q.c & 15)) return DW_EINVAL;
        if ((q.lda & 7) || (q.ldb & 7) || (q.ldc & 3) || q.lda < q.m || q.ldb < q.n || q.ldc < q.n) return DW_EINVAL;
        // the operand DMA addresses a problem's k rows with 31-bit buffer offsets (the rule of gemm_choose)
        if ((long)k * q.lda * 2 >= 0x7fffffffL || (long)k * q.ldb * 2 >= 0x7fffffffL) return DW_EINVAL;
        g.pr[i] = q;
        g.first[i] = (int)total;
        total += (long)(q.m / 320) * (q.n / 256);
        if (total > g_gemm_cus) return DW_EINVAL;      // one round: a workgroup per tile, all resident together
    }
    for (int i = count; i < DW_WGRAD_GROUP_MAX; ++i) g.first[i] = (int)total;
    g.total = (int)total; g.k = k; g.accumulate = accumulate ? 1 : 0;
    hipLaunchKernelGGL(wgrad_group_kernel, dim3(8 * (((int)total + 7) / 8)), dim3(512), 0, (hipStream_t)stream, g);
    DW_CHECK_LAUNCH();
    return DW_OK;
}
