"""Float64 restatements of the training kernels -- LayerNorm forward / backward (csrc/norm.hip), the fused CE + KL loss and its
gradient (csrc/loss.hip), the gradient norm and clipped AdamW (csrc/optim.hip) -- with the case tables, seeded inputs and the metric of
tests/test_training_kernels_edges_gpu.py.  Plain formulas on the inputs as the kernels see them (bf16 / fp32 values widened exactly);
no rounding point is shared with the kernels or with oracle/ref_ops.py.  tests/test_training_kernels_edges.py pins them against
torch's float64 autograd, AdamW and clip_grad_norm_, and checks that the tables hold every class the GPU module promises."""
import math

import torch

BF16, F32 = torch.bfloat16, torch.float32
LN_EPS = 1e-5


def _d(t):
    return None if t is None else t.detach().double()


def f32_as_double(x):
    """The double that equals float(x): what a kernel receives of a host scalar passed as `float`."""
    return float(torch.tensor(x, dtype=torch.float32).double())


# ---- the metric --------------------------------------------------------------------------------------------------------------
def row_err(x, ref, width):
    """max over the `width`-element rows of ||x - ref|| / max(||ref row||, rms), rms = root mean square of all row norms of ref
    (tests/attention_restatement.py row_err; width 1 = per element, for per-row statistics, per-column sums and flat vectors)."""
    x, ref = x.double().reshape(-1, width), ref.double().reshape(-1, width)
    n = ref.norm(dim=-1)
    rms = n.pow(2).mean().sqrt()
    return ((x - ref).norm(dim=-1) / torch.maximum(n, rms)).max().item()


def bf16_ulp(x):
    """One bf16 unit in the last place at |x| (float64 tensor): 2^(exponent - 7), 0 at 0."""
    e = torch.floor(torch.log2(x.abs().clamp_min(2.0 ** -126)))
    return torch.where(x == 0, torch.zeros_like(x), torch.exp2(e - 7))


def to_bf16(x64):
    return x64.float().to(BF16)


# ---- LayerNorm ---------------------------------------------------------------------------------------------------------------
def layernorm_fwd(x, gamma, beta, eps=LN_EPS):
    """-> y, mean, rstd (float64); eps as the kernel receives it (a float)."""
    x, gamma, beta = _d(x), _d(gamma), _d(beta)
    n = x.shape[1]
    mean = x.sum(-1) / n
    d = x - mean[:, None]
    var = (d * d).sum(-1) / n
    rstd = 1.0 / torch.sqrt(var + f32_as_double(eps))
    return d * rstd[:, None] * gamma + beta, mean, rstd


def layernorm_bwd(dy, x, mean, rstd, gamma, dres, lowp=False):
    """-> dres_out (= dres + dx, or dx when dres is None), dgamma, dbeta [, bf16(dres_out), column sums of the rounded values]."""
    dy, x, mean, rstd, gamma, dres = _d(dy), _d(x), _d(mean), _d(rstd), _d(gamma), _d(dres)
    n = x.shape[1]
    xh = (x - mean[:, None]) * rstd[:, None]
    g = dy * gamma
    c1 = g.sum(-1, keepdim=True) / n
    c2 = (g * xh).sum(-1, keepdim=True) / n
    out = rstd[:, None] * (g - c1 - xh * c2)
    if dres is not None:
        out = out + dres
    res = (out, (dy * xh).sum(0), dy.sum(0))
    if lowp:
        lo = to_bf16(out)
        res += (lo, lo.double().sum(0))
    return res


# ---- fused CE + KL loss ------------------------------------------------------------------------------------------------------
def _lse(z):
    m = z.max(-1, keepdim=True).values
    return m + torch.log(torch.exp(z - m).sum(-1, keepdim=True))


def distill_loss(s, t, labels, V, T, ce_w, kl_w, grad_scale):
    """-> row_ce [rows], row_kl [rows] (0 in the rows the label excludes, as the kernel stores them), losses [4] = (ce, kl,
    ce_w * ce + kl_w * kl, n_valid) with 0 / 0 = NaN for a batch without labels, gradient [rows, V] w.r.t. the student logits."""
    zs, zt = _d(s)[:, :V], _d(t)[:, :V]
    rows = zs.shape[0]
    ce_ok, kl_ok = labels != -100, labels >= 0
    n_ce, n_kl = int(ce_ok.sum()), int(kl_ok.sum())
    logp1 = zs - _lse(zs)
    logpS = zs / T - _lse(zs / T)
    logpT = zt / T - _lse(zt / T)
    pT = torch.exp(logpT)
    onehot = torch.zeros_like(zs)
    idx = torch.nonzero(ce_ok).flatten()
    onehot[idx, labels[idx]] = 1.0
    row_ce = -(logp1 * onehot).sum(-1)
    row_kl = (pT * (logpT - logpS)).sum(-1) * kl_ok
    nan = float("nan")
    ce = row_ce.sum().item() / n_ce if n_ce else nan
    kl = row_kl.sum().item() / n_kl * T * T if n_kl else nan
    losses = torch.tensor([ce, kl, ce_w * ce + kl_w * kl, float(n_ce)], dtype=torch.float64)
    grad = torch.zeros(rows, V, dtype=torch.float64, device=zs.device)
    if n_ce:
        grad += (grad_scale * ce_w / n_ce) * (torch.exp(logp1) - onehot) * ce_ok[:, None]
    if n_kl:
        grad += (grad_scale * kl_w * T / n_kl) * (torch.exp(logpS) - pT) * kl_ok[:, None]
    return row_ce, row_kl, losses, grad


# ---- gradient norm, clipped AdamW ----------------------------------------------------------------------------------------------
def sumsq(g):
    g = _d(g)
    return (g * g).sum()


def adamw_steps(p, g, m, v, sumsq, max_norm, grad_mul, lr, betas, eps, wd, steps):
    """`steps` updates (step counts 1 .. steps) from the same gradient -> p, m, v.  sumsq: the squared norm of g the update is given
    (None: no clipping); the gradient used is g * grad_mul * min(1, max_norm / (sqrt(sumsq) * |grad_mul| + 1e-6))."""
    p, g, m, v = _d(p).clone(), _d(g), _d(m).clone(), _d(v).clone()
    clip = float(grad_mul)
    if max_norm > 0 and sumsq is not None:
        norm = math.sqrt(float(sumsq)) * abs(grad_mul)
        clip *= min(1.0, max_norm / (norm + 1e-6))
    gg = g * clip
    b1, b2 = betas
    for step in range(1, steps + 1):
        p = p * (1.0 - lr * wd)
        m = b1 * m + (1.0 - b1) * gg
        v = b2 * v + (1.0 - b2) * gg * gg
        p = p - (lr / (1.0 - b1 ** step)) * m / (torch.sqrt(v) / math.sqrt(1.0 - b2 ** step) + eps)
    return p, m, v


# ---- inputs (seeded, generated on the CPU) -------------------------------------------------------------------------------------
def _gen(seed):
    return torch.Generator().manual_seed(seed)


LN_KINDS = ("gauss", "outliers", "constant", "small")    # row r of every LayerNorm input is of kind r % 4


def ln_inputs(rows, cols, dtype, seed=0):
    """-> x [rows, cols] of `dtype`, gamma, beta (fp32), dy (bf16), dres (fp32).  Rows by r % 4: Gaussian of scale 2 around 0.5; N(0, 1)
    with two outlier channels at +-300 (Whisper's residual stream); a constant row (variance 0: rstd = rsqrt(eps)); N(0, 1) * 1e-3
    (variance below eps)."""
    g = _gen(1000 * seed + 7 * rows + cols)
    x = torch.randn(rows, cols, generator=g)
    r = torch.arange(rows)
    k = r % 4
    x[k == 0] = x[k == 0] * 2.0 + 0.5
    hot = r[k == 1]
    x[hot, (7 * hot) % cols] = 300.0
    x[hot, (7 * hot + cols // 2) % cols] = -300.0
    x[k == 2] = 1.5
    x[k == 3] *= 1e-3
    gamma = 1.0 + 0.5 * torch.randn(cols, generator=g)
    beta = torch.randn(cols, generator=g)
    dy = torch.randn(rows, cols, generator=g).to(BF16)
    dres = torch.randn(rows, cols, generator=g)
    return x.to(dtype), gamma, beta, dy, dres


LOSS_PAD = 3.0e4        # the pad columns [V, ld) of both logit matrices: a kernel that reads one of them into a maximum or a sum is loud


def loss_inputs(V, ld, rows, regime, labels_kind, seed=0):
    """-> s, t (bf16 [rows, ld]), labels (int64 [rows]).
    regime: gauss (independent N(0, 2^2)), equal (student = teacher), near (student = bf16(teacher + 0.05 N(0, 1))), spiked (student
    N(0, 1) with one logit 40 above the row's maximum, the label on it).
    labels_kind: random (every fifth -100, from row 4), edges (0, V - 1, random, ... by row % 3, every fifth -100), ignored (all -100)."""
    g = _gen(seed + 31 * V + rows)
    t = (2.0 * torch.randn(rows, V, generator=g)).to(BF16)
    labels = torch.randint(0, V, (rows,), generator=g)
    r = torch.arange(rows)
    if labels_kind == "edges":
        labels[r % 3 == 0] = 0
        labels[r % 3 == 1] = V - 1
    labels[4::5] = -100
    if regime == "gauss":
        s = (2.0 * torch.randn(rows, V, generator=g)).to(BF16)
    elif regime == "equal":
        s = t.clone()
    elif regime == "near":
        s = (t.float() + 0.05 * torch.randn(rows, V, generator=g)).to(BF16)
    else:
        assert regime == "spiked"
        s = torch.randn(rows, V, generator=g).to(BF16)
        col = torch.where(labels >= 0, labels, r % V)
        s[r, col] = (s.float().max(-1).values + 40.0).to(BF16)
    if labels_kind == "ignored":
        labels[:] = -100
    else:
        assert labels_kind in ("random", "edges")
    full = lambda z: torch.cat([z, torch.full((rows, ld - V), LOSS_PAD, dtype=BF16)], 1).contiguous()
    return full(s), full(t), labels


def adamw_inputs(n, seed=0):
    """-> p ~ N(0, 1), g ~ N(0, 0.01^2), m ~ 0.01 N(0, 1), v ~ 1e-4 N(0, 1)^2: moments as after earlier steps."""
    g_ = _gen(seed + n)
    p = torch.randn(n, generator=g_)
    g = 0.01 * torch.randn(n, generator=g_)
    m = 0.01 * torch.randn(n, generator=g_)
    v = 1e-4 * torch.randn(n, generator=g_) ** 2
    return p, g, m, v


# ---- case tables ---------------------------------------------------------------------------------------------------------------
# LayerNorm.  Lanes hold float4 vectors: nv = ceil(cols / 256) of them (bf16 16-byte path: 8 elements, nv8 = ceil(cols / 512)).
LN_COLS = [4, 8, 252, 256, 260, 512, 516, 768, 772, 1024, 1028, 1276, 1280, 1284, 1540, 1544, 2044, 2048]
LN_ROWS = [1, 3, 5, 517]
LN_DTYPES = [F32, BF16]
LN_FALLBACK = [(cols, how) for cols in (512, 1280) for how in ("pitch+4", "base+8B")]      # bf16 input off the 16-byte accesses
LN_PERSIST = [(8192, 384), (8192, 1024), (8195, 260), (8191, 1280)]                          # fp32; the last: just below the threshold
LN_WRAP = [(4101, 384), (4101, 768), (3077, 1024), (1029, 2048), (2053, 1280)]              # backward: rows > the resident grid
LN_PREFETCH_OFF = [(2053, 1280), (517, 1028)]                                               # also with key 21 = 1: <5,12> in place of the prefetching kernel
LN_VARIANT_KEY, LN_VARIANT_DEFAULT = 21, 3
LN_PERSIST_ROWS = 8192


def ln_fwd_kernel(rows, cols, dtype, sixteen_byte=True, variant=LN_VARIANT_DEFAULT):
    """The instantiation dw_layernorm_fwd_ld launches (csrc/norm.hip).  sixteen_byte: pitches multiples of 8 and bases 16-byte aligned
    (otherwise, for bf16 rows of a multiple of 8 columns, the same kernel through 8-byte accesses)."""
    if dtype == BF16 and cols % 8 == 0:
        return f"ln_fwd_bf16x8_kernel<{max(1, min(4, -(-cols // 512)))},{'true' if sixteen_byte else 'false'}>"
    nv = -(-cols // 256)
    if (variant & 1) and dtype == F32 and nv <= 5 and rows >= LN_PERSIST_ROWS:
        return "ln_fwd_persist_kernel<5>"
    return f"ln_fwd_kernel<{'true' if dtype == BF16 else 'false'},{2 if nv <= 2 else 3 if nv <= 3 else 5 if nv <= 5 else 8}>"


def ln_bwd_kernel(rows, cols, variant=LN_VARIANT_DEFAULT):
    """-> (instantiation without the input type, rows per pass of the resident grid: more rows than that wrap the row loop)."""
    nv = -(-cols // 256)
    if (variant & 2) and nv == 5:
        return "ln_bwd_pf_kernel<.,5,8>", 256 * 8
    if nv <= 3:
        return f"ln_bwd_kernel<.,{2 if nv <= 2 else 3},4>", 256 * 4 * 4
    return ("ln_bwd_kernel<.,5,12>", 256 * 12) if nv <= 5 else ("ln_bwd_kernel<.,8,4>", 256 * 4)


# Loss.  One vector = 8 bf16; one pass of the 256-thread block = 2048 columns.
LOSS_VLD = [(5, 8), (8, 8), (9, 16), (1000, 1000), (2047, 2048), (2049, 2056), (4097, 4104), (51866, 51872), (51866, 51968)]
LOSS_ROWS = [1, 3, 97]
LOSS_T = [2.0, 1.0, 4.0]
LOSS_W = [(0.8, 1.0), (1.0, 0.0), (0.0, 1.0)]
LOSS_GS = [1.0, 0.125, 1024.0]
LOSS_REGIMES = ["gauss", "equal", "near", "spiked"]
LOSS_WAYS = ["in_place", "grad_out", "weights_dev"]


def loss_cases():
    """(V, ld, rows, labels_kind, T, (ce_w, kl_w), grad_scale, regime): every (V, ld) x rows once with the other parameters rotating
    at different periods, every (V, ld) with an all-ignored batch, and the flagship width at 97 rows in all four regimes."""
    out, k = [], 0
    for i, (V, ld) in enumerate(LOSS_VLD):
        for j, rows in enumerate(LOSS_ROWS):
            out.append((V, ld, rows, ("edges", "random")[(i + j) % 2], LOSS_T[k % 3], LOSS_W[(k // 2) % 3], LOSS_GS[(k // 4) % 3],
                        LOSS_REGIMES[(k + i) % 4]))
            k += 1
        out.append((V, ld, 3, "ignored", LOSS_T[i % 3], LOSS_W[i % 3], LOSS_GS[i % 3], "gauss"))
    for regime in LOSS_REGIMES:
        out.append((51866, 51968, 97, "edges", 2.0, (0.8, 1.0), 1.0, regime))
    seen = set()
    return [c for c in out if not (c in seen or seen.add(c))]


# AdamW and the gradient norm.  One pass of the AdamW grid = 4096 * 1024 elements, of the sumsq grid 2048 * 1024.
ADAMW_N = [1, 3, 4, 5, 1027, 2048 * 1024 + 1027, 4096 * 1024 + 1027]
ADAMW_HYPER = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
ADAMW_STEPS = 3
# clip: max_norm as a multiple of the gradient's norm (after grad_mul), 0 = max_norm 0, None = sumsq None
ADAMW_BRANCHES = [
    dict(name="clipping", clip=0.5, grad_mul=1.0, wd=0.01, shadow=True),
    dict(name="below_max_norm", clip=2.0, grad_mul=1.0, wd=0.01, shadow=True),
    dict(name="max_norm_0", clip=0, grad_mul=1.0, wd=0.01, shadow=True),
    dict(name="sumsq_none", clip=None, grad_mul=1.0, wd=0.0, shadow=True),
    dict(name="grad_mul_half", clip=0.5, grad_mul=0.5, wd=0.0, shadow=True),
    dict(name="grad_mul_1024th", clip=2.0, grad_mul=1.0 / 1024, wd=0.01, shadow=False),
]
ADAMW_BIG_BRANCHES = ["clipping", "grad_mul_1024th"]      # the branches the two wrapping sizes run (the small sizes run all)
ADAMW_GRID_PASS, SUMSQ_GRID_PASS = 4096 * 1024, 2048 * 1024
