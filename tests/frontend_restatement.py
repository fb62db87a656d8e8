"""Float64 restatements of the front end (csrc/logmel.hip), the conv stem helpers, embeddings, casts, add, column sums and row moves
(csrc/elementwise.hip), the split-K combination (dw_reduce_slices*, csrc/gemm.hip) and the GELU of the GEMM epilogues (csrc/common.h),
with the case tables, the seeded inputs and the dispatch facts of tests/test_frontend_edges_gpu.py.  Plain formulas on the inputs as
the kernels see them (bf16 / fp32 values widened exactly); no rounding point is shared with the kernels or with oracle/ref_ops.py,
except the two the operations themselves define (the bf16 gradient that gelu' multiplies: bf16(dy), bf16(col2im sum)).
tests/test_frontend_edges.py pins every statement to an independent authority on the CPU and the tables to the sources."""
import math

import torch

from training_restatement import bf16_ulp, row_err, to_bf16      # noqa: F401  (the metric of the training edge suite)

BF16, F32, F64 = torch.bfloat16, torch.float32, torch.float64


def _d(t):
    return None if t is None else t.detach().double()


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ---- dispatch facts (checked against the sources by the CPU test) ---------------------------------------------------------------------
LM_FRAMES_PER_TILE = 32         # LM_FR
LM_TILES_PER_WG = 12            # LQ_TPB: one workgroup of logmel_mfma_kernel owns 384 frames
LM_INIT_BLOCK = 64              # logmel_init_kernel: clips per block
LM_MAX_MELS = 256
IM2COL_MEL_FRAMES, IM2COL_MEL_CHANNELS = 64, 128    # im2col_mel_kernel: frames per block, channels per pass of the c0 loop
ADD_GRID_BLOCKS = 4096          # dw_add: grid cap, 256 elements per block and pass
COLSUM_ROW_LANES, COLSUM_MAX_GROUPS = 16, 64


def colsum_grid(rows):
    """-> (row groups = gridDim.y, whether the four-loads-in-flight loop runs at all): step = 16 * groups rows, the unrolled loop of
    the first lane runs iff 3 * step < rows."""
    groups = min(COLSUM_MAX_GROUPS, -(-rows // COLSUM_ROW_LANES))
    return groups, rows > 3 * COLSUM_ROW_LANES * groups


# ---- log-mel ------------------------------------------------------------------------------------------------------------------------
def logmel(audio, filters, dtype=F64, dead_frames=False):
    """Whisper's log-mel of audio [B, n] (n a multiple of 160, >= 400) -> [B, n_mels, n / 160]: reflect-padded centre frames of 400
    samples every 160, periodic Hann, direct 400-point DFT (bins 0 ... 200), power, filters [201, n_mels], log10(max(., 1e-10)),
    max(., clip maximum - 8), (. + 4) / 4.  dtype float64: the statement; float32: the same formula in fp32 arithmetic (what fp32 can
    give).  dead_frames: the WRONG maximum -- it includes the frames up to the next multiple of 32, read the way the kernel stages
    them (one reflection, then clamped to the clip), which the kernel computes and must leave out."""
    B, n = audio.shape
    n_frames = n // 160
    total = -(-n_frames // LM_FRAMES_PER_TILE) * LM_FRAMES_PER_TILE if dead_frames else n_frames
    idx = torch.arange(total)[:, None] * 160 - 200 + torch.arange(400)[None, :]
    idx = idx.abs()
    idx = torch.where(idx >= n, 2 * (n - 1) - idx, idx).clamp(0, n - 1)
    i = torch.arange(400, dtype=F64)
    win = (0.5 - 0.5 * torch.cos(2.0 * math.pi * i / 400.0)).to(dtype)
    kn = (torch.arange(400)[:, None] * torch.arange(201)[None, :]) % 400
    ang = 2.0 * math.pi * kn.double() / 400.0
    cos, sin = torch.cos(ang).to(dtype), torch.sin(ang).to(dtype)
    fw = audio.to(dtype)[:, idx] * win                      # [B, frames, 400]
    re, im = fw @ cos, fw @ sin
    mel = (re * re + im * im) @ filters.to(dtype)           # [B, frames, n_mels]
    log_spec = torch.log10(mel.clamp_min(1e-10)).transpose(1, 2)
    mx = log_spec.amax(dim=(1, 2), keepdim=True)
    log_spec = torch.maximum(log_spec[:, :, :n_frames], mx - 8.0)
    return ((log_spec + 4.0) / 4.0).contiguous()


def synthetic_bank(n_mels):
    """A non-negative [201, n_mels] bank with the supports the slaney bank never has: filter 0 all zero, filter 1 with a hole inside
    its support (bins 10 ... 30 without 15 ... 24), filter 2 a single weight at bin 0, filter 3 a single weight at bin 200, the others
    triangles of 5 to 24 bins placed along the spectrum."""
    f = torch.zeros(201, n_mels, dtype=F64)
    f[10:31, 1] = 0.02
    f[15:25, 1] = 0.0
    f[0, 2] = 0.05
    f[200, 3] = 0.05
    for m in range(4, n_mels):
        width = 5 + (m * 7) % 20
        lo = (m * 37) % (201 - width)
        k = torch.arange(width, dtype=F64)
        f[lo:lo + width, m] = 0.03 * (1.0 - (2.0 * (k + 0.5) / width - 1.0).abs())
    return f.float()


LOGMEL_FRAMES = [3, 31, 32, 33, 384, 385, 417]
LOGMEL_CLIPS = ["noise", "half_zero", "zero", "tones", "loud_silent", "dead"]
# (frames, batch, n_mels, clip): every frame count and every n_mels with noise, every other clip at the smallest shape that shows it
LOGMEL_CASES = [(3, 1, 80, "noise"), (31, 3, 128, "noise"), (32, 1, 4, "noise"), (33, 3, 80, "noise"), (384, 1, 128, "noise"),
                (385, 3, 256, "noise"), (417, 1, 80, "noise"), (32, 65, 4, "noise"), (3, 65, 128, "loud_silent"),
                (33, 1, 80, "half_zero"), (385, 1, 128, "half_zero"), (33, 3, 4, "zero"), (3, 1, 256, "zero"), (417, 1, 128, "tones"),
                (33, 1, 80, "tones"), (33, 3, 80, "loud_silent"), (33, 1, 80, "dead"), (33, 3, 256, "dead"), (33, 1, 128, "dead")]


def logmel_audio(frames, batch, clip, seed=0):
    n = frames * 160
    g = _gen(seed + 13 * frames + batch)
    # noise on a small offset and a small tone at the Nyquist frequency: bins 0 and 200, which the synthetic banks weigh on their own,
    # then hold energy in every frame (of white noise alone either is as close to zero in some frame as the batch is large, and its
    # logarithm asks more than fp32 holds: tests/test_frontend_edges.py checks what fp32 can give on every case)
    a = 0.1 * torch.randn(batch, n, generator=g) + 0.02 + 0.02 * (1.0 - 2.0 * (torch.arange(n) % 2))
    if clip == "half_zero":
        a[:, n // 2:] = 0.0
    elif clip == "zero":
        a.zero_()
    elif clip == "tones":           # the three-tone clip of test_logmel: 60 dB inside every frame
        t = torch.arange(n, dtype=F64) / 16000.0
        a[:] = (0.3 * torch.sin(2 * math.pi * 440.0 * t) + 0.05 * torch.sin(2 * math.pi * 3100.0 * t + 1.0) +
                3e-4 * torch.sin(2 * math.pi * 6050.0 * t)).float()
    elif clip == "loud_silent":     # the maxima are per clip: loud, silent, quiet, ...
        a[1::3] = 0.0
        a[2::3] *= 1e-3
    elif clip == "dead":            # quiet clip whose last 60 samples are loud: the frames past the end see them reflected
        a *= 1e-3
        a[:, n - 60:] = 0.5 * torch.randn(batch, 60, generator=g)
    else:
        assert clip == "noise"
    return a.contiguous()


# ---- conv stem --------------------------------------------------------------------------------------------------------------------
def im2col_mel(mel, kpad):
    """mel [B, C, T] -> [B*T, kpad] float64: column k*C + c of row (b, t) = mel[b, c, t + k - 1], zero outside the clip and in the
    pad columns.  (Rounded once to bf16 it is the kernel's output bit for bit.)"""
    B, C, T = mel.shape
    out = torch.zeros(B, T, kpad, dtype=F64)
    m = _d(mel).transpose(1, 2)                              # [B, T, C]
    for k in range(3):
        lo, hi = max(0, 1 - k), min(T, T + 1 - k)           # t with 0 <= t + k - 1 < T
        if hi > lo:
            out[:, lo:hi, k * C:(k + 1) * C] = m[:, lo + k - 1:hi + k - 1]
    return out.reshape(B * T, kpad)


def im2col_s2(a, B, T):
    """a [B*T, C] -> [B*T/2, 3C]: column k*C + c of row (b, t) = a[b, 2t + k - 1, c], zero outside."""
    C = a.shape[1]
    x = _d(a).reshape(B, T, C)
    out = torch.zeros(B, T // 2, 3, C, dtype=F64)
    for t in range(T // 2):
        for k in range(3):
            r = 2 * t + k - 1
            if 0 <= r < T:
                out[:, t, k] = x[:, r]
    return out.reshape(B * T // 2, 3 * C)


def col2im_s2(dxcol, B, T):
    """The transpose of im2col_s2: [B*T/2, 3C] -> [B*T, C], row (b, r) = the sum of dxcol[(b, t), k*C + c] over 2t + k - 1 = r."""
    C = dxcol.shape[1] // 3
    d = _d(dxcol).reshape(B, T // 2, 3, C)
    out = torch.zeros(B, T, C, dtype=F64)
    for t in range(T // 2):
        for k in range(3):
            r = 2 * t + k - 1
            if 0 <= r < T:
                out[:, r] += d[:, t, k]
    return out.reshape(B * T, C)


def _cdf(z):
    """The normal cdf through erfc: 1 + erf(z / sqrt2) has no digit left below z = -8.3 even in float64."""
    return 0.5 * torch.erfc(-z / math.sqrt(2.0))


def gelu(z):
    z = _d(z)
    return z * _cdf(z)


def gelu_grad(z):
    z = _d(z)
    return _cdf(z) + z * torch.exp(-0.5 * z * z) / math.sqrt(2.0 * math.pi)


def gelu_bwd(dy, z):
    """bf16(dy) * gelu'(z) in float64 (the gradient is a bf16 tensor by definition: autocast hands GELU's backward a bf16 dy)."""
    return to_bf16(_d(dy)).double() * gelu_grad(z)


def col2im_s2_gelu_bwd(dxcol, z, B, T):
    """bf16(col2im_s2(dxcol)) * gelu'(z): the col2im sum is conv2's input gradient, a bf16 tensor under autocast."""
    return to_bf16(col2im_s2(dxcol, B, T)).double() * gelu_grad(z)


def pack_conv_weight(w, kpad):
    """w [D, C, 3] -> [D, kpad]: column k*C + c = w[d, c, k], zero pad columns."""
    D, C, _ = w.shape
    out = torch.zeros(D, kpad, dtype=F64)
    for k in range(3):
        out[:, k * C:(k + 1) * C] = _d(w)[:, :, k]
    return out


def unpack_conv_grad(gwp, gw, accumulate):
    """gwp [D, kpad] -> gw [D, C, 3] (+)= : gw[d, c, k] = gwp[d, k*C + c].  One fp32 add at most: float64 rounded once is exact."""
    D, C, _ = gw.shape
    g = torch.stack([_d(gwp)[:, k * C:(k + 1) * C] for k in range(3)], 2)
    return _d(gw) + g if accumulate else g


# ---- the fast GELU of the GEMM epilogues (csrc/common.h gelu_y_s_pdf2): Abramowitz & Stegun 7.1.26 in float64 ------------------------
AS_P = 0.3275911
AS_A = (0.254829592, -0.284496736, 1.421413741, -1.453152027, 1.061405429)
EPS32 = 2.0 ** -24      # one fp32 rounding, relative


def _as_parts(z):
    z = _d(z)
    t = 1.0 / (1.0 + AS_P * z.abs() / math.sqrt(2.0))
    poly = ((((AS_A[4] * t + AS_A[3]) * t + AS_A[2]) * t + AS_A[1]) * t + AS_A[0])
    dpoly = ((4 * AS_A[4] * t + 3 * AS_A[3]) * t + 2 * AS_A[2]) * t + AS_A[1]
    e = torch.exp(-0.5 * z * z)
    return z, t, poly, dpoly, e


def gelu_fast(z):
    """The epilogues' formula in float64 -> gelu, gelu' (its own error: the approximation without any fp32 rounding)."""
    z, t, poly, _, e = _as_parts(z)
    s = 1.0 - poly * t * e
    cdf = 0.5 + 0.5 * torch.copysign(s, z)
    return (z.abs() * s + z) * 0.5, cdf + z * e / math.sqrt(2.0 * math.pi)


def gelu_fast_rounding_bound(z):
    """First-order a priori bound of what the fp32 roundings of gelu_y_s_pdf2 add to gelu and to gelu' at z, eps = 2^-24 per
    rounding, 2 eps per raw v_rcp_f32 / v_exp_f32 (1 ulp):
      t = rcp(fma(|z| / sqrt2, p, 1)):   the product, the fma, the reciprocal           dt   <= 4 eps t
      P(t), four fmas on values <= 1.46, each error carried on through factors t <= 1   dP   <= |P'(t)| dt + 4 * 1.46 eps
      e = exp2(z * z * c): two products and the rounded constant shift the exponent by 3 eps |z^2 c|, exp2 itself 2 eps
                                                                                        de/e <= (3 ln2 |z^2 c| + 2) eps
      tail = P * t * e, two products                                                    dtail <= tail (dP/P + dt/t + de/e + 2 eps)
      s = 1 - tail <= 1                                                                 ds   <= dtail + eps
      y = (|z| s + z) / 2, product and sum (or one fma)                                 dy   <= |z| (ds + eps) / 2 + eps |y|
                           ... and from z = 2^127 the sum is past the largest fp32 number: +inf, the function's stated domain ends there
      cdf = fma(copysign(s), 1/2, 1/2) <= 1                                             dcdf <= ds / 2 + eps
      pdf = e / sqrt(2 pi), one product with a rounded constant                          dpdf <= pdf (de/e + 2 eps)
      g = fma(z, pdf, cdf)                                                              dg   <= dcdf + |z| dpdf + eps (|cdf| + |z| pdf)
    -> (dy, dg)."""
    z, t, poly, dpoly, e = _as_parts(z)
    eps = EPS32
    dt = 4 * eps * t
    dP = dpoly.abs() * dt + 4 * 1.46 * eps
    de_rel = (3 * math.log(2.0) * (0.5 * z * z / math.log(2.0)) + 2) * eps
    tail = poly * t * e
    dtail = tail * (dP / poly + dt / t + de_rel + 2 * eps)
    ds = dtail + eps
    y, g = gelu_fast(z)
    dy = z.abs() * (ds + eps) / 2 + eps * y.abs()
    dy = torch.where(z >= GELU_FAST_DOMAIN, torch.full_like(dy, math.inf), dy)
    pdf = e / math.sqrt(2.0 * math.pi)
    cdf = g - z * pdf
    dg = ds / 2 + eps + z.abs() * pdf * (de_rel + 2 * eps) + eps * (cdf.abs() + z.abs() * pdf)
    return dy, dg


GELU_FAST_DOMAIN = 2.0 ** 127    # gelu_y_s_pdf2: |z| s + z overflows from here (csrc/common.h states it)
GELU_APPROX_ERF = 1.5e-7        # A & S 7.1.26: |erf error|; it halves through 0.5 * tail


def ulp_of(x, dtype):
    """One unit in the last place of `dtype` at |x| (float64 tensor), subnormal spacing below the smallest normal."""
    mant, emin = {BF16: (7, -126), torch.float16: (10, -14), F32: (23, -126)}[dtype]
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** emin))).clamp_min(emin)
    return torch.exp2(e - mant)


def gelu_sweep_bounds(z, out_dtype, grad_dtype):
    """Per element: approximation + fp32 roundings + half an ulp of the output type (taken at |reference| + the rest, which is
    where the fp32 value that gets rounded can lie) -> (bound of gelu, bound of gelu')."""
    z = _d(z)
    dy, dg = gelu_fast_rounding_bound(z)
    pre_y = 0.5 * GELU_APPROX_ERF * z.abs() + dy
    pre_g = 0.5 * GELU_APPROX_ERF + dg
    return (pre_y + 0.5 * ulp_of(gelu(z).abs() + pre_y, out_dtype), pre_g + 0.5 * ulp_of(gelu_grad(z).abs() + pre_g, grad_dtype))


def all_finite_bf16():
    """Every bf16 bit pattern as a tensor of 65536 values, NaN and infinity patterns replaced by zero."""
    bits = torch.arange(65536, dtype=torch.int32).to(torch.int16)
    v = bits.view(BF16).clone()
    v[~torch.isfinite(v.float())] = 0.0
    return v


def gelu_sweep_fp32_values(n=4096, seed=5):
    """n fp32 values of both signs, magnitudes log-uniform in [1e-6, 16]."""
    g = _gen(seed)
    mag = torch.exp(torch.rand(n, generator=g, dtype=F64) * (math.log(16.0) - math.log(1e-6)) + math.log(1e-6))
    sign = torch.where(torch.rand(n, generator=g) < 0.5, -1.0, 1.0).double()
    return (mag * sign).float()


GELU_SWEEP_SHAPE = dict(tile=128, M=128, K=64, N=65536)


# ---- embeddings -------------------------------------------------------------------------------------------------------------------
def embed_fwd(ids, tok, pos):
    B, T = ids.shape
    return _d(tok)[ids.reshape(-1)] + _d(pos)[:T].repeat(B, 1)


def embed_bwd(dx, ids, dtok, dpos):
    """-> dtok + the rows of dx summed by id, dpos with rows [0, T) += the sum over the batch (None stays None)."""
    B, T = ids.shape
    V = dtok.shape[0]
    onehot = torch.zeros(B * T, V, dtype=F64)
    onehot[torch.arange(B * T), ids.reshape(-1)] = 1.0
    out_tok = _d(dtok) + onehot.t() @ _d(dx)
    out_pos = None
    if dpos is not None:
        out_pos = _d(dpos).clone()
        out_pos[:T] += _d(dx).reshape(B, T, -1).sum(0)
    return out_tok, out_pos


EMBED_D, EMBED_T = [4, 260, 384, 1280], [1, 7, 448]
# (B, T, D): every D and T, B*T*(D/4) never a multiple of 256 except where noted by the CPU test
EMBED_FWD_CASES = [(1, 1, 4), (3, 7, 260), (2, 448, 384), (3, 7, 1280), (1, 448, 4), (5, 1, 260)]
EMBED_DTYPES = [(BF16, BF16), (BF16, F32), (F32, BF16), (F32, F32)]     # (table, out)
EMBED_V = 37
# (B, T, D, ids kind, dpos: None / "zero" / "filled", dtok filled)
EMBED_BWD_CASES = [(3, 7, 4, "distinct", "filled", True), (3, 7, 260, "distinct", None, False), (2, 9, 384, "distinct", "zero", True),
                   (16, 448, 4, "equal", "filled", False), (16, 448, 260, "equal", None, True), (4, 448, 384, "padded", "filled", True),
                   (16, 448, 384, "equal", "zero", False)]


def embed_ids(B, T, V, kind, seed=0):
    g = _gen(seed + B * 1000 + T)
    if kind == "random":
        ids = torch.randint(0, V, (B, T), generator=g)
        ids.view(-1)[0], ids.view(-1)[-1] = 0, V - 1
    elif kind == "distinct":
        assert B * T <= V
        ids = torch.randperm(V, generator=g)[:B * T].reshape(B, T)
    elif kind == "equal":
        ids = torch.full((B, T), V - 2)
    else:
        assert kind == "padded"      # labels: a few live tokens, then the pad id to the end of the row
        ids = torch.randint(0, V - 1, (B, T), generator=g)
        for b in range(B):
            ids[b, 5 + 11 * b:] = V - 1
    return ids.long().contiguous()


# ---- casts, add, column sums, row moves, slice sums -------------------------------------------------------------------------------------
CAST_N = [1, 2, 3, 4, 5, 1023, 1024, 1025, 1027]


def cast_specials_f32():
    """NaN, both infinities, signed zeros, fp32 and bf16 subnormals, round-to-even ties of both parities, the tie that carries into
    the exponent, the largest finite value (rounds to infinity) and the largest that does not."""
    bits = [0x7FC00000, 0x7F800000, 0xFF800000, 0x00000000, 0x80000000, 0x00000001, 0x80000001, 0x00010000, 0x00008000, 0x00018000,
            0x3F808000, 0x3F818000, 0x3F808001, 0x3F807FFF, 0x3FFF8000, 0x7F7FFFFF, 0x7F7F7FFF, 0x7F7F8000, 0xBF808000, 0xBF818000,
            0x7F800001, 0x007FFFFF]
    return torch.tensor([b - (1 << 32) if b >= 1 << 31 else b for b in bits], dtype=torch.int32).view(F32)


ADD_N = [1, 257, ADD_GRID_BLOCKS * 256 + 1027]
ADD_DTYPES = [(a, b, y) for a in (F32, BF16) for b in (F32, BF16) for y in (F32, BF16)]

COLSUM_ROWS = [1, 15, 16, 17, 1003, 1024, 1025, 3072, 3073, 4101, 5123, 8197]
COLSUM_COLS = [8, 120, 128, 136, 1280]


def colsum_cases():
    """(rows, cols, pad, off, accumulate, kind): every row count x two widths rotating through all five, pitch / slice offset /
    accumulate / data kind rotating at other periods; off > 0 = a column slice at a multiple-of-8 offset of a wider matrix."""
    out, k = [], 0
    for i, rows in enumerate(COLSUM_ROWS):
        for j in range(2):
            cols = COLSUM_COLS[(2 * i + j) % 5]
            out.append((rows, cols, (0, 8)[k % 2], (0, 0, 16)[k % 3], (k // 2) % 2, ("gauss", "cancel")[(k // 3) % 2]))
            k += 1
    out += [(8197, 1280, 8, 0, 0, "gauss"), (8197, 1280, 0, 0, 1, "cancel"), (3073, 1280, 0, 16, 0, "gauss"), (4101, 8, 0, 0, 1, "gauss")]
    return out


def colsum_input(rows, cols, kind, seed=0):
    g = _gen(seed + 17 * rows + cols)
    x = torch.randn(rows, cols, generator=g)
    if kind == "cancel":            # +-100 in pairs down each column, on top of the noise: the column sums are of the noise's size
        big = 100.0 * (1.0 + torch.rand(rows // 2, cols, generator=g))
        x[0:2 * (rows // 2):2] += big
        x[1:2 * (rows // 2):2] -= big
    return x.to(BF16)


def colsum(x, out0, accumulate):
    s = _d(x).sum(0)
    return _d(out0) + s if accumulate else s


def reduce_slices_fp32(part, out0, accumulate):
    """part [slices, ...] fp32, added in slice order in fp32 onto out0 (or zero): the kernels' chain, hence the exact expectation."""
    acc = out0.clone() if accumulate else torch.zeros_like(out0)
    for s in range(part.shape[0]):
        acc = acc + part[s]
    return acc


REDUCE_SLICES, REDUCE_N = [1, 2, 7], [4, 1028]
PACK_D, PACK_C = [1, 5, 384], [1, 80, 128]
IM2COL_MEL_C, IM2COL_MEL_T, IM2COL_MEL_B = [1, 80, 128, 129, 200], [1, 63, 64, 65, 130], [1, 3]
S2_T, S2_C, S2_B = [2, 4, 6, 130], [8, 24, 384], [1, 3]
GELU_BWD_N = [4, 1020, 1024, 1028, 1 << 16]


def kpad_of(C):
    """The next multiple of 64 above 3 * C (the engine's choice), 3 * C itself where that is one."""
    return -(-3 * C // 64) * 64


def gelu_z(n, seed=0):
    """bf16 pre-activations: N(0, 2^2), with signed zeros, values where gelu' is negative (z in [-3, -0.76]) and tails up to |z| = 12
    spliced in at fixed places."""
    g = _gen(seed + n)
    z = 2.0 * torch.randn(n, generator=g)
    special = torch.tensor([0.0, -0.0, -0.75, -1.0, -2.0, -3.0, 12.0, -12.0, 5.5, -5.5, 8.0, -8.0, 1e-3, -1e-3, 0.5, -0.5])
    k = min(n, special.numel())
    z[:k] = special[:k]
    if n >= 64:
        z[-k:] = special[:k]
    return z.to(BF16)
