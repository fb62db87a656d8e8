"""The training kernels -- LayerNorm forward / backward (csrc/norm.hip), the fused CE + KL loss and its gradient (csrc/loss.hip), the gradient
norm and clipped AdamW (csrc/optim.hip) -- at the edges of their dispatch, judged against the float64 restatements of
tests/training_restatement.py (pinned to torch's float64 autograd / AdamW on the CPU by tests/test_training_kernels_edges.py).

The bound, per judged tensor and PER CASE: row_err(kernel, float64) <= F * e_ref, e_ref = row_err(RefOps, float64) on the same inputs (the
bound form of tests/test_attention_edges_gpu.py; row_err per row for matrices, per element for per-row statistics, per-column sums and
flat vectors).  Everything exact is per case too: NaN-patterned guards around every output, zeros against a float64 reference of zero,
bit-identity between variants.

Measured on the MI355X, the largest row_err(kernel) / e_ref of any single case, that case, and F = the smallest of 2, 3, 4 that is at
least 1.5 x the ratio:
  y       1.00  (1 x 4 f32: bf16 rounding of the output on both sides)                        F 2
  lowp    1.00  (1 x 4 f32; against the unrounded float64 gradient, see ln_judge)             F 2
  mean    1.58  (517 x 252 bf16)                                                              F 3   few-value cases below
  rstd    1.91  (5 x 512 bf16)                                                                F 3
  dres    1.28  (1 x 4 bf16, pitch + 8)                                                       F 2   few-value cases below
  dgamma  1.37  (5 x 4 f32)                                                                   F 3
  dbeta   1.00  (517 x 8 f32)                                                                 F 2
  colsum  1.004 (5 x 1544 f32, pitch + 8)                                                     F 2
  losses  2.39  (V 5, one row, gauss; 2.20 at V 51866, 97 rows, spiked; losses[0:3] as one 3-vector)  F 4
  grad    1.00  per row (bf16 rounding); element-wise residual beyond one bf16 ulp 2.00
          (V 51866, one row, gauss: 7.3e-12 against 3.6e-12)                                  F 2 per row, 3 per element
  row_ce  1.14  (V 2049, 97 rows, near; absolute, against the fp32 statement of the formula -- the issue asks this form for row_kl
          only; row_ce cancels the same way on spiked rows and is judged alike)               F 2
  row_kl  1.44  (V 2047, 97 rows, near; absolute, likewise)                                   F 3   few-value case below
  p 2.13 (n 4, below max_norm)   m 1.55 (n 5, grad_mul 0.5)   v 1.73 (n 5, grad_mul 1/1024)   F 4, 3, 3
  sumsq   at most 5.2e-8 relative (n = 5); bound 2.5e-6 = the 37 roundings of the longest chain (12 in a thread's loop, 6 + 2 in the
          wave and block reductions, 8 + 6 + 2 in the second stage, one per square) x 2^-24, the a priori worst case

Few-value cases.  Where a case has at most 5 LayerNorm rows, or one loss row, e_ref is the luck of a handful of roundings: six such
cases have ratios past 4 / 1.5 although the kernel's own error is a rounding or two.  Each of these cases states an a priori rounding
bound (`floor`) and passes up to max(F * e_ref, floor); with more rows no floor exists.  The cases, in fp32 ulps (2^-23 relative):
  mean  1 x 768 f32: kernel 0.66 ulp, RefOps 0.21 (ratio 3.17); 1 x 1540 bf16: 0.67 / 0.15 (4.53); 5 x 1544 f32: 0.55 / 0.17 (3.21);
        3 x 2048 f32: 0.25 / 0.06 (4.07).  RefOps's mean is there the correctly rounded one (under half an ulp), which another order
        of summation cannot be asked to reproduce.  floor for mean and rstd: one ulp.
  dres  1 x 4 bf16, dense: 2.6 / 0.7 ulp of the row's norm (3.64).  Four columns leave dx = rstd * (g - c1 - xh * c2) two degrees of
        freedom: the terms cancel and each side's roundings of them are magnified alike.  floor: ln_dres_floor(), the roundings of
        that expression at the magnitude of its terms (here 27 ulp of the row: a worst case, not an estimate).
  row_kl  V 9, one row, T 2: kernel 2.8e-7, the fp32 statement 4.4e-8 absolute (6.37), on terms of magnitude 21: 0.11 / 0.02 ulp of
        them.  floor for row_ce and row_kl: loss_row_floors(), one ulp of the magnitudes the row's terms are differences of.

Fixed with this module (each showed as a failure of the named case):
* bf16 forward off the 16-byte path (x pitch cols + 4, or x 8 bytes into a 16-byte-aligned buffer) went to ln_fwd_kernel<true,.>, which
  sums a row in another lane order: y / mean / rstd differed in the last bit from the 16-byte path (fallback, 5 x 512 and 5 x 1280).  Rows
  of a multiple of 8 columns now run ln_fwd_bf16x8_kernel<., false>: same arithmetic, 8-byte accesses.
* ln_bwd_pf_kernel and ln_bwd_kernel<.,5,12> (key 21 = 1) gave residual gradients that differed in the last bit (2053 x 1280, 517 x 1028):
  the compiler contracted different products into the adds around them.  Both now spell out every rounding (LN_BWD_TERMS, ln_bwd_dx).
* dgamma, dbeta and the column sums of the bf16 copy were fp32 atomics, one per column per workgroup, into the output word: up to
  1024 additions in arrival order where torch.sum adds pairwise.  Judged by the rule like every other tensor they measured 5.3 x
  (dgamma) and 15.8 x (colsum) RefOps's error at 4101 x 768 bf16, 8.1 to 10.4 x at 517 rows, 2.7 x at 517 x 2048 f32 -- past 4 / 1.5 for
  every F -- and differed from run to run.  The workgroups now store float64 shares into a caller's workspace and ln_bwd_sums_kernel
  adds them in a fixed order and rounds once (ratios above; a dense and a padded run of the same values now give the same bits).
* student == teacher with ce_weight 0 left a gradient of 1e-10 * grad_scale instead of zero (V 8 / 1000 / 2049 / 51866, 3 rows, T 1):
  one of softmax(z_s / T), softmax(z_t / T) was contracted into their difference.  Both products are rounded first now.

Which instantiation each class reaches (tr.ln_fwd_kernel / tr.ln_bwd_kernel restate the dispatch; the CPU test checks the tables):
  forward, fp32:  cols <= 512 ln_fwd_kernel<false,2>, 516 ... 768 <false,3>, 772 ... 1280 <false,5>, 1284 ... 2048 <false,8> (rows 1 ... 517);
                  rows >= 8192 and cols <= 1280: ln_fwd_persist_kernel<5> at 384, 1024 and 260 columns (8195 rows), not at 8191 x 1280
  forward, bf16:  cols % 8 == 0: ln_fwd_bf16x8_kernel<1 ... 4, true> (<4>: 1544, 2048), <1 / 3, false> in the fallback test;
                  cols % 8 == 4 (4, 252, 260, 516, 772, 1028, 1276, 1284, 1540, 2044): ln_fwd_kernel<true,2 / 3 / 5 / 8>
  backward:       cols <= 512 ln_bwd_kernel<.,2,4>, ... 768 <.,3,4>, 772 ... 1024 <.,5,12>, 1028 ... 1280 ln_bwd_pf_kernel<.,5,8> (<.,5,12> with
                  key 21 = 1), 1284 ... 2048 <.,8,4>; the row loops wrap at 4101 x 384, 4101 x 768, 3077 x 1024, 1029 x 2048, 2053 x 1280
  sumsq / AdamW:  n = 2048 * 1024 + 1027 wraps the grid of dw_sumsq_f32, 4096 * 1024 + 1027 those of dw_adamw / dw_adamw_dev too"""
import contextlib

import pytest
import torch

import training_restatement as tr
from guarded import DEV, NAN32, Guarded, Guarded32

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
# F per judged tensor (module docstring)
F_BOUND = {"y": 2.0, "mean": 3.0, "rstd": 3.0, "dres": 2.0, "lowp": 2.0, "dgamma": 3.0, "dbeta": 2.0, "colsum": 2.0,
           "losses": 4.0, "grad": 2.0, "grad_elem": 3.0, "row_ce": 2.0, "row_kl": 3.0, "p": 4.0, "m": 3.0, "v": 3.0}
SUMSQ_REL = 2.5e-6      # module docstring
ATOMIC_ORDER = 1e-5     # dgamma / dbeta / column sums of two kernels that group the rows differently (the issue's figure)


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps(DEV)


@pytest.fixture(scope="module")
def ref():
    from oracle.ref_ops import RefOps
    return RefOps(DEV)


@contextlib.contextmanager
def ln_variant(ops, value):
    try:
        assert ops.lib.dw_debug_set(tr.LN_VARIANT_KEY, value) == 0
        yield
    finally:
        ops.lib.dw_debug_set(tr.LN_VARIANT_KEY, tr.LN_VARIANT_DEFAULT)


def relerr(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


def dev(*ts):
    return [t.to(DEV) for t in ts]


class Pool:
    """The figures of one test, each case judged on its own: rows() takes row_err(kernel, float64) and e_ref = row_err(RefOps, float64)
    of one case on the same inputs and prints them; check() asserts row_err <= F * e_ref for every case (an e_ref of exactly zero asks
    for an error of exactly zero).  A float64 reference that is identically zero asks for exact zeros on the spot.
    `floor`: an a priori rounding bound that a few-value case states for itself (module docstring, "Few-value cases"); the case then
    passes up to max(F * e_ref, floor)."""

    def __init__(self):
        self.notes, self.bad = [], []

    def _note(self, name, case, e, e_ref, floor=0.0):
        print(f"TRAIN_EDGE {case} {name} kernel {e:.4e} ref {e_ref:.4e} floor {floor:.4e} ratio {e / e_ref if e_ref else float('nan'):.3f}")
        self.notes.append((name, case, e, e_ref, floor))

    def expect(self, ok, what):
        if not ok:
            self.bad.append(what)

    def rows(self, name, case, x, x_ref, x64, width, floor=0.0):
        x64 = x64.to(x.device)
        self.expect(bool(torch.isfinite(x.float()).all()), f"{case} {name}: non-finite values")
        if not bool(x64.any()):
            print(f"TRAIN_EDGE {case} {name} zero reference, max|x| {x.double().abs().max().item():.3e}")
            return self.expect(not bool(x.any()), f"{case} {name}: not exactly zero against a zero reference")
        self._note(name, case, tr.row_err(x, x64, width), tr.row_err(x_ref, x64, width), floor)

    def absolute(self, name, case, x, x_ref, x64, floor=0.0):
        """|x - float64| against the largest |x_ref - float64| (per-row loss terms: a relative bound is impossible where they cancel)."""
        x64 = x64.to(x.device)
        self.expect(bool(torch.isfinite(x).all()), f"{case} {name}: non-finite values")
        self._note(name, case, (x.double() - x64).abs().max().item(), (x_ref.double() - x64).abs().max().item(), floor)

    def check(self):
        for name, case, e, e_ref, floor in self.notes:
            self.expect(e <= max(F_BOUND[name] * e_ref, floor), f"{case} {name}: {e:.3e} > {F_BOUND[name]:g} x {e_ref:.3e} (floor {floor:.3e})")
        assert not self.bad, "\n".join(self.bad)


# ---- LayerNorm -------------------------------------------------------------------------------------------------------------------
def padded_view(t, pad, off=0, fill=7.0):
    """t as a [rows, cols] view of a buffer with `pad` more columns per row, starting at column `off`."""
    if not pad:
        return t.contiguous()
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=t.device)
    buf[:, off:off + t.shape[1]] = t
    return buf[:, off:off + t.shape[1]]


def ln_forward(ops, x, gamma, beta, pad=0, save_stats=True):
    """ops.layernorm_fwd into a guarded y whose pitch is cols + pad -> y, mean, rstd."""
    y = Guarded(x.shape[0], x.shape[1], pad=pad)
    out, mean, rstd = ops.layernorm_fwd(x, gamma, beta, eps=tr.LN_EPS, save_stats=save_stats, out=y.live)
    torch.cuda.synchronize()
    assert y.intact(), "forward wrote outside y"
    assert out.data_ptr() == y.live.data_ptr() and (mean is None) == (not save_stats) and (rstd is None) == (not save_stats)
    return y.live, mean, rstd


def ln_backward(ops, dy, x, mean, rstd, gamma, dres0, pad=0):
    """ops.layernorm_bwd with every output guarded (dres0 None: the kernel writes a tensor of its own instead of accumulating)
    -> dres, dgamma, dbeta, lowp, colsum."""
    rows, cols = x.shape
    dg, db, cs = (Guarded32(cols, zero=True) for _ in range(3))
    lo = Guarded(rows, cols, pad=pad)
    dres = None
    if dres0 is not None:
        dres = Guarded(rows, cols, pad=pad, dtype=F32)
        dres.live.copy_(dres0)
    out = ops.layernorm_bwd(dy, x, mean, rstd, gamma, None if dres is None else dres.live, dg.live, db.live, out_lowp=lo.live, colsum=cs.live)
    torch.cuda.synchronize()
    for name, g in (("dgamma", dg), ("dbeta", db), ("colsum", cs), ("lowp", lo), ("dres", dres)):
        assert g is None or g.intact(), f"backward wrote outside {name}"
    assert dres is None or out.data_ptr() == dres.live.data_ptr()
    return out, dg.live, db.live, lo.live, cs.live


ULP32 = 2.0 ** -23      # one fp32 unit in the last place, relative


def ln_dres_floor(x, gamma, dy, mean, rstd, dres0, dres64):
    """Few-value cases: the a priori rounding error of dx = rstd * (g - c1 - xh * c2) (+ dres), g = dy * gamma, in row_err's measure.
    Eight fp32 roundings (g, xh twice, g - c1, the fma, the product with rstd, c1, c2), each at most 2^-24 of rstd * (|g| + |c1| +
    |xh * c2|), and one of the sum with dres: where the three terms cancel (a row of 4 columns has 2 degrees of freedom left) the error
    relative to dx is that much larger on both sides, by amounts that a handful of roundings do not average out."""
    x, dy, gamma, mean, rstd, dres64 = (t.double().to(x.device) for t in (x, dy, gamma, mean, rstd, dres64))
    xh, g = (x - mean[:, None]) * rstd[:, None], dy * gamma
    c1, c2 = g.mean(1, keepdim=True), (g * xh).mean(1, keepdim=True)
    mag = 8.0 * rstd[:, None] * (g.abs() + c1.abs() + (xh * c2).abs())
    if dres0 is not None:
        mag = mag + dres0.double().to(x.device).abs() + dres64.abs()
    n = dres64.norm(dim=1)
    return (2.0 ** -24 * mag.norm(dim=1) / torch.maximum(n, n.pow(2).mean().sqrt())).max().item()


def ln_judge(pool, case, ops, ref, x, gamma, beta, dy, dres0, pad=0, forward=True):
    """One forward + backward through the kernels (pitches cols + pad), judged against float64 next to RefOps on the same inputs; the
    backward of all three takes the KERNEL's mean and rstd.  -> the kernels' outputs."""
    rows, cols = x.shape
    few = rows <= 5     # (module docstring, "Few-value cases")
    xv, dyv = padded_view(x, pad), padded_view(dy, pad, fill=5.0)
    y, mean, rstd = ln_forward(ops, xv, gamma, beta, pad)
    if forward:
        y64, mean64, rstd64 = tr.layernorm_fwd(x, gamma, beta)
        ry, rmean, rrstd = ref.layernorm_fwd(x, gamma, beta, eps=tr.LN_EPS)
        pool.rows("y", case, y, ry, y64, cols)
        pool.rows("mean", case, mean, rmean, mean64, 1, floor=ULP32 if few else 0.0)
        pool.rows("rstd", case, rstd, rrstd, rstd64, 1, floor=ULP32 if few else 0.0)
    got = ln_backward(ops, dyv, xv, mean, rstd, gamma, dres0, pad)
    rdg, rdb, rcs = (torch.zeros(cols, device=DEV) for _ in range(3))
    rlo = torch.empty(rows, cols, dtype=BF16, device=DEV)
    rdres = ref.layernorm_bwd(dy, x, mean, rstd, gamma, None if dres0 is None else dres0.clone(), rdg, rdb, out_lowp=rlo, colsum=rcs)
    dres64, dg64, db64 = tr.layernorm_bwd(dy, x, mean, rstd, gamma, dres0)
    dres, dg, db, lo, cs = got
    pool.rows("dres", case, dres, rdres, dres64, cols, floor=ln_dres_floor(x, gamma, dy, mean, rstd, dres0, dres64) if few else 0.0)
    # the bf16 copy: bf16(dres) bit for bit, and as a rounding of the float64 gradient (against the restatement's own rounded copy
    # both sides would only count the elements that round the other way)
    pool.expect(torch.equal(lo, dres.to(BF16)), f"{case}: the bf16 copy is not bf16(dres)")
    pool.rows("lowp", case, lo, rlo, dres64, cols)
    pool.rows("dbeta", case, db, rdb, db64, 1)
    # the column sums are taken over the ROUNDED values, and one element of dres that rounds the other way moves a sum by a bf16 ulp:
    # each side's sums are judged against the float64 sums of its own stored copy
    e_dg, e_cs = tr.row_err(dg, dg64, 1), tr.row_err(cs, lo.double().sum(0), 1)
    pool._note("dgamma", case, e_dg, tr.row_err(rdg, dg64, 1))
    pool._note("colsum", case, e_cs, tr.row_err(rcs, rlo.double().sum(0), 1))
    return (y, mean, rstd) + got


@pytest.mark.parametrize("dtype", tr.LN_DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("cols", tr.LN_COLS)
def test_layernorm_width_sweep(ops, ref, cols, dtype):
    """Every width x rows 1, 3, 5, 517, dense (the backward writing a new dres) and with all pitches cols + 8 (the backward accumulating
    into a given dres): the padded run's forward must equal the dense one bit for bit."""
    pool = Pool()
    for rows in tr.LN_ROWS:
        x, gamma, beta, dy, dres0 = dev(*tr.ln_inputs(rows, cols, dtype))
        case = f"ln {rows}x{cols} {'bf16' if dtype == BF16 else 'f32'}"
        y, mean, rstd, dres, dg, db, lo, cs = ln_judge(pool, case + " dense", ops, ref, x, gamma, beta, dy, None)
        y2, mean2, rstd2, dres2, dg2, db2, lo2, cs2 = ln_judge(pool, case + " pitch+8", ops, ref, x, gamma, beta, dy, dres0, pad=8, forward=False)
        assert torch.equal(y2, y) and torch.equal(mean2, mean) and torch.equal(rstd2, rstd), case
        assert torch.equal(dg2, dg) and torch.equal(db2, db), case       # (the column sums are added in a fixed order)
    pool.check()


@pytest.mark.parametrize("cols,how", tr.LN_FALLBACK)
def test_layernorm_bf16_fallback_same_bits(ops, ref, cols, how):
    """bf16 input off the 16-byte path (ln_fwd_bf16x8_kernel<., false>; it was ln_fwd_kernel<true,.>): an x pitch of cols + 4, or an x
    that starts 8 bytes into a 16-byte-aligned buffer -- same y, mean and rstd as ln_fwd_bf16x8_kernel<., true> on the same values, and
    judged against float64 like it."""
    pool = Pool()
    for rows in (5, 517):
        x, gamma, beta, _, _ = dev(*tr.ln_inputs(rows, cols, BF16))
        y0, mean0, rstd0 = ln_forward(ops, x, gamma, beta)
        xv = padded_view(x, 4) if how == "pitch+4" else padded_view(x, 8, off=4)
        assert (xv.stride(0) % 8 != 0) == (how == "pitch+4") and (xv.data_ptr() % 16 == 8) == (how == "base+8B")
        y, mean, rstd = ln_forward(ops, xv, gamma, beta)
        assert torch.equal(y, y0) and torch.equal(mean, mean0) and torch.equal(rstd, rstd0), (rows, how)
        y64, mean64, rstd64 = tr.layernorm_fwd(x, gamma, beta)
        ry, rmean, rrstd = ref.layernorm_fwd(x, gamma, beta, eps=tr.LN_EPS)
        case = f"ln fallback {rows}x{cols} {how}"
        pool.rows("y", case, y, ry, y64, cols)
        pool.rows("mean", case, mean, rmean, mean64, 1)
        pool.rows("rstd", case, rstd, rrstd, rstd64, 1)
    pool.check()


@pytest.mark.parametrize("rows,cols", tr.LN_PERSIST)
def test_layernorm_persistent_forward(ops, ref, rows, cols):
    """fp32 input at the 8192-row threshold of ln_fwd_persist_kernel<5> (narrow rows: vectors of the prefetched row that no lane holds;
    8191 rows: the other side): against float64, bit-equal to key 21 = 2 (persistent off), and the same y without the statistics."""
    x, gamma, beta, _, _ = dev(*tr.ln_inputs(rows, cols, F32))
    y, mean, rstd = ln_forward(ops, x, gamma, beta, pad=8)
    with ln_variant(ops, 2):
        y2, mean2, rstd2 = ln_forward(ops, x, gamma, beta, pad=8)
    assert torch.equal(y, y2) and torch.equal(mean, mean2) and torch.equal(rstd, rstd2)
    y3, _, _ = ln_forward(ops, x, gamma, beta, save_stats=False)
    assert torch.equal(y3, y)
    pool, case = Pool(), f"ln persistent {rows}x{cols}"
    y64, mean64, rstd64 = tr.layernorm_fwd(x, gamma, beta)
    ry, rmean, rrstd = ref.layernorm_fwd(x, gamma, beta, eps=tr.LN_EPS)
    pool.rows("y", case, y, ry, y64, cols)
    pool.rows("mean", case, mean, rmean, mean64, 1)
    pool.rows("rstd", case, rstd, rrstd, rstd64, 1)
    pool.check()


@pytest.mark.parametrize("cols,dtype", [(260, F32), (1544, BF16), (516, BF16), (2048, F32)])
def test_layernorm_forward_without_statistics(ops, cols, dtype):
    x, gamma, beta, _, _ = dev(*tr.ln_inputs(5, cols, dtype))
    assert torch.equal(ln_forward(ops, x, gamma, beta, save_stats=False)[0], ln_forward(ops, x, gamma, beta)[0])


@pytest.mark.parametrize("dtype", tr.LN_DTYPES, ids=["f32", "bf16"])
@pytest.mark.parametrize("rows,cols", tr.LN_WRAP)
def test_layernorm_backward_row_loop_wraps(ops, ref, rows, cols, dtype):
    """More rows than the resident grid holds: some waves accumulate dgamma, dbeta and the column sums over two rows, some over one."""
    x, gamma, beta, dy, dres0 = dev(*tr.ln_inputs(rows, cols, dtype))
    pool = Pool()
    ln_judge(pool, f"ln wrap {rows}x{cols}", ops, ref, x, gamma, beta, dy, dres0, pad=8)
    pool.check()


@pytest.mark.parametrize("rows,cols", tr.LN_PREFETCH_OFF)
def test_layernorm_backward_without_prefetch_same_bits(ops, ref, rows, cols):
    """Key 21 = 1: ln_bwd_kernel<.,5,12> where the default runs the prefetching kernel (2053 rows wrap the latter only)."""
    x, gamma, beta, dy, dres0 = dev(*tr.ln_inputs(rows, cols, F32))
    _, mean, rstd = ln_forward(ops, x, gamma, beta)
    want = ln_backward(ops, dy, x, mean, rstd, gamma, dres0)
    pool = Pool()
    with ln_variant(ops, 1):
        got = ln_judge(pool, f"ln key21=1 {rows}x{cols}", ops, ref, x, gamma, beta, dy, dres0, forward=False)[3:]
    assert torch.equal(got[0], want[0]) and torch.equal(got[3], want[3])
    for i in (1, 2, 4):
        assert relerr(got[i], want[i]) <= ATOMIC_ORDER, i
    pool.check()


def test_layernorm_invalid_arguments_are_rejected_and_write_nothing(ops):
    """DW_EINVAL through the C ABI before any launch: cols not a multiple of 4 / above 2048, a pitch below cols or not a multiple of 4,
    mean without rstd, no / too small / misaligned workspace for the backward's column sums."""
    from distil_whisper_amd.ops_hip import DW_F32, _p
    rows, cols = 5, 2056
    x, dres_in = torch.zeros(rows, cols, device=DEV), torch.zeros(rows, cols, device=DEV)
    dy = torch.zeros(rows, cols, dtype=BF16, device=DEV)
    gamma, beta = torch.ones(cols, device=DEV), torch.zeros(cols, device=DEV)
    stats = torch.zeros(2, rows, device=DEV)
    y, mean, rstd = Guarded(rows, cols, pad=0), Guarded32(rows), Guarded32(rows)
    dres, lo = Guarded(rows, cols, pad=0, dtype=F32), Guarded(rows, cols, pad=0)
    dg, db, cs = Guarded32(cols), Guarded32(cols), Guarded32(cols)

    def f(c=256, ldx=None, ldy=None, mean_=mean.buf, rstd_=rstd.buf):
        ops._chk(ops.lib.dw_layernorm_fwd_ld(_p(x), DW_F32, _p(gamma), _p(beta), _p(y.buf), _p(mean_), _p(rstd_), rows, c, tr.LN_EPS,
                                             c if ldx is None else ldx, c if ldy is None else ldy, ops._stream()), "layernorm_fwd")

    need = ops.lib.dw_layernorm_bwd_ws_bytes(rows, 256)
    assert need == 3 * 2 * 256 * 8 and ops.lib.dw_layernorm_bwd_ws_bytes(rows, 6) == 0
    sums = Guarded32(need // 4)

    def b(c=256, lddy=None, ldx=None, lddres=None, ldlowp=None, sums_=sums.live, sums_bytes=need):
        ld = [c if v is None else v for v in (lddy, ldx, lddres, ldlowp)]
        ops._chk(ops.lib.dw_layernorm_bwd_ld(_p(dy), _p(x), DW_F32, _p(stats[0]), _p(stats[1]), _p(gamma), _p(dres.buf), 0, _p(dg.buf),
                                             _p(db.buf), _p(lo.buf), _p(cs.buf), rows, c, *ld, _p(sums_), sums_bytes, ops._stream()),
                 "layernorm_bwd")

    bad = [lambda: f(c=6), lambda: f(c=2052), lambda: f(ldx=252), lambda: f(ldy=252), lambda: f(ldx=258), lambda: f(ldy=258),
           lambda: f(rstd_=None), lambda: f(mean_=None),
           lambda: b(c=6), lambda: b(c=2052), lambda: b(lddy=252), lambda: b(ldx=252), lambda: b(lddres=252), lambda: b(ldlowp=252),
           lambda: b(lddy=258), lambda: b(ldx=258), lambda: b(lddres=258), lambda: b(ldlowp=258),
           lambda: b(sums_=None), lambda: b(sums_bytes=need - 8), lambda: b(sums_=sums.live[1:])]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError, match="code -1"):
            call()
        torch.cuda.synchronize()
        for g in (y, mean, rstd, dres, lo, dg, db, cs, sums):
            assert g.untouched(), i
    f()                                                            # (the valid calls of the same arguments run)
    b()
    torch.cuda.synchronize()
    assert not y.untouched() and not dres.untouched() and sums.intact()       # (the workspace: its stated bytes and no more)


# ---- loss ------------------------------------------------------------------------------------------------------------------------
def loss_rows_fp32(s, t, labels, V, T):
    """The formula of csrc/loss.hip's header comment in torch fp32 (torch.exp / log, not the hardware's): the per-row terms' own
    reference, since RefOps returns none -> row_ce, row_kl."""
    zs, zt = s[:, :V].float(), t[:, :V].float()
    ce_ok, kl_ok = labels != -100, labels >= 0
    ms, mt = zs.max(-1).values, zt.max(-1).values
    inv_t = torch.tensor(1.0 / T, dtype=F32, device=s.device)
    zs1 = torch.exp(zs - ms[:, None]).sum(-1)
    zs_t = torch.exp((zs - ms[:, None]) * inv_t).sum(-1)
    et = torch.exp((zt - mt[:, None]) * inv_t)
    zt_t = et.sum(-1)
    w = (et * (zt - zs)).sum(-1)
    z_label = zs.gather(1, labels.clamp_min(0)[:, None])[:, 0]
    ce = (ms + torch.log(zs1) - z_label) * ce_ok
    kl = (w / zt_t * inv_t - (mt * inv_t + torch.log(zt_t)) + (ms * inv_t + torch.log(zs_t))) * kl_ok
    return ce, kl


def loss_groups():
    """The cases of tr.loss_cases() by test: every (V, ld) its own, the 97-row cases of the flagship width one each (their float64
    restatement takes a second on the CPU)."""
    groups = {}
    for c in tr.loss_cases():
        V, ld, rows = c[:3]
        key = f"{V}-{ld}" if V < 51866 or rows < 97 else f"{V}-{ld}-97-{c[7]}-T{c[4]:g}"
        groups.setdefault(key, []).append(c)
    return groups


LOSS_GROUPS = loss_groups()
_loss64 = {}


def loss_row_floors(s, t, labels, V, T):
    """Few-value cases (one row: the issue's "max over rows" of the fp32 statement's error is then a single sample): one fp32 ulp of
    the magnitudes that a row's terms are differences of -- ce = lse(z_s) - z_s[label]; kl = T^2 * (sum p_t * (z_t - z_s) / T -
    lse(z_t / T) + lse(z_s / T)) -> floors of row_ce, row_kl."""
    zs, zt = s[:, :V].double(), t[:, :V].double()
    lab = labels.clamp_min(0).long()[:, None]
    ce = (torch.logsumexp(zs, 1).abs() + zs.gather(1, lab)[:, 0].abs()).max().item()
    pt = torch.softmax(zt / T, 1)
    kl = T * T * (torch.logsumexp(zs / T, 1).abs() + torch.logsumexp(zt / T, 1).abs() + (pt * (zt - zs).abs()).sum(1) / T).max().item()
    return ULP32 * ce, ULP32 * kl


def loss64(case):
    """float64 on the CPU, once per case whatever its ld."""
    V, ld, rows, kind, T, (ce_w, kl_w), gs, regime = case
    key = (V, rows, kind, T, ce_w, kl_w, gs, regime)
    if key not in _loss64:
        s, t, labels = tr.loss_inputs(V, V + (-V) % 8, rows, regime, kind)
        _loss64[key] = tr.distill_loss(s, t, labels, V, T, ce_w, kl_w, gs)
    return _loss64[key]


def loss_case(pool, ops, ref, case):
    V, ld, rows, kind, T, (ce_w, kl_w), gs, regime = case
    name = f"loss V{V} ld{ld} rows{rows} {kind} T{T:g} w{ce_w:g}/{kl_w:g} gs{gs:g} {regime}"
    s, t, labels = dev(*tr.loss_inputs(V, ld, rows, regime, kind))
    row_ce64, row_kl64, losses64, grad64 = (x.to(DEV) for x in loss64(case))
    # three ways
    g0 = Guarded(rows, ld, pad=0)
    g0.live.copy_(s)
    losses, row_ce, row_kl = ops.distill_loss(g0.live, t, labels, V, T, ce_w, kl_w, gs, True, return_rows=True)
    g1, s1 = Guarded(rows, ld, pad=0), s.clone()
    l1, ce1, kl1 = ops.distill_loss(s1, t, labels, V, T, ce_w, kl_w, gs, True, grad_out=g1.live, return_rows=True)
    g2 = Guarded(rows, ld, pad=0)
    g2.live.copy_(s)
    wdev = torch.tensor([ce_w, kl_w], dtype=F32, device=DEV)
    l2, ce2, kl2 = ops.distill_loss(g2.live, t, labels, V, T, 123.0, 456.0, gs, True, weights_dev=wdev, return_rows=True)
    l3 = ops.distill_loss(s.clone(), t, labels, V, T, ce_w, kl_w, gs, False)
    torch.cuda.synchronize()
    assert g0.intact() and g1.intact() and g2.intact(), f"{name}: wrote behind the gradient"
    assert torch.equal(s1, s), f"{name}: grad_out given, the student logits changed"
    same = lambda a, b: torch.equal(a.view(torch.int32 if a.dtype == F32 else torch.int16), b.view(torch.int32 if b.dtype == F32 else torch.int16))
    for way, got in (("grad_out", (l1, ce1, kl1, g1.live)), ("weights_dev", (l2, ce2, kl2, g2.live))):
        for a, b in zip(got, (losses, row_ce, row_kl, g0.live)):
            assert same(a, b), f"{name}: {way} differs from the in-place call"
    assert same(l3, losses), f"{name}: the losses differ without the gradient"
    grad = g0.live
    # RefOps and the fp32 statement of the kernel's formula on the same inputs
    rs = s.clone()
    rlosses = ref.distill_loss(rs, t, labels, V, T, ce_w, kl_w, gs, True)
    rce, rkl = loss_rows_fp32(s, t, labels, V, T)
    n_valid = int((labels != -100).sum())
    assert losses[3].item() == n_valid == losses64[3].item()
    pool.expect(not bool(grad[:, V:].any()), f"{name}: gradient pad columns not zero")
    if n_valid == 0:
        # the kernel comment's promise: NaN means, a gradient of exactly zero, losses[3] = 0 (the gate of dw_adam_tick)
        pool.expect(bool(torch.isnan(losses[:3]).all()), f"{name}: losses of an all-ignored batch {losses.tolist()}")
        pool.expect(not bool(grad.any()), f"{name}: gradient of an all-ignored batch not zero")
        pool.expect(not bool(row_ce.any()) and not bool(row_kl.any()), f"{name}: per-row terms of an all-ignored batch not zero")
        return
    pool.rows("losses", name, losses[:3], rlosses[:3], losses64[:3], 3)
    ce_floor, kl_floor = loss_row_floors(s, t, labels, V, T) if rows == 1 else (0.0, 0.0)
    pool.absolute("row_ce", name, row_ce, rce, row_ce64, floor=ce_floor)
    pool.absolute("row_kl", name, row_kl, rkl, row_kl64, floor=kl_floor)
    g, rg = grad[:, :V], rs[:, :V]
    pool.rows("grad", name, g, rg, grad64, V)
    # element-wise: one bf16 ulp around bf16(float64), plus F x what RefOps leaves beyond that; exactly zero where float64 is
    want, ulp = tr.to_bf16(grad64).double(), tr.bf16_ulp(grad64)
    res = ((g.double() - want).abs() - ulp).clamp_min(0.0)
    rres = ((rg.double() - want).abs() - ulp).clamp_min(0.0)
    zero = grad64 == 0
    pool.expect(not bool(g[zero].any()), f"{name}: gradient not zero where the float64 gradient is")
    if rres.max().item() == 0.0:
        pool.expect(res.max().item() == 0.0, f"{name}: gradient element off by 1 bf16 ulp + {res.max().item():.3e}, RefOps by none")
    else:
        pool._note("grad_elem", name, res.max().item(), rres.max().item())


@pytest.mark.parametrize("group", list(LOSS_GROUPS))
def test_distill_loss_edges(ops, ref, group):
    """Each case in place, with grad_out and with weights_dev (same bits), losses / per-row terms / gradient against float64."""
    pool = Pool()
    for case in LOSS_GROUPS[group]:
        loss_case(pool, ops, ref, case)
    pool.check()


def test_distill_loss_invalid_arguments_are_rejected_and_write_nothing(ops):
    from distil_whisper_amd.ops_hip import _p
    rows, V, ld = 3, 20, 32
    s, t, labels = dev(*tr.loss_inputs(V, ld, rows, "gauss", "random"))
    losses, row_ce, row_kl = Guarded32(4), Guarded32(rows), Guarded32(rows)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    grad = Guarded(rows, ld, pad=0)

    def f(s_=s.data_ptr(), t_=t.data_ptr(), g_=grad.buf.data_ptr(), V_=V, ld_=ld, T=2.0):
        ops._chk(ops.lib.dw_distill_loss(s_, t_, _p(labels), rows, V_, ld_, T, 0.8, 1.0, 1.0, _p(losses.buf), g_, _p(row_ce.buf),
                                         _p(row_kl.buf), _p(counts), ops._stream()), "distill_loss")

    bad = [lambda: f(V_=ld + 1), lambda: f(ld_=28), lambda: f(T=0.0), lambda: f(T=-1.0),
           lambda: f(s_=s.data_ptr() + 8), lambda: f(t_=t.data_ptr() + 8), lambda: f(g_=grad.buf.data_ptr() + 8)]
    for i, call in enumerate(bad):
        with pytest.raises(RuntimeError, match="code -1"):
            call()
        torch.cuda.synchronize()
        for g in (losses, row_ce, row_kl, grad):
            assert g.untouched(), i
    f()
    torch.cuda.synchronize()
    assert not losses.untouched() and not grad.untouched()


# ---- gradient norm and AdamW -------------------------------------------------------------------------------------------------------
def guarded_sumsq(ops, g, out):
    """ops.sumsq with its partials in a patterned workspace: only the first min(2048, blocks) slots may change."""
    ws = Guarded32(2048)
    ops._sumsq_ws = ws.live
    try:
        ops.sumsq(g, out)
        torch.cuda.synchronize()
    finally:
        ops._sumsq_ws = None
    nb = max(1, min(2048, (g.numel() // 4 + 255) // 256))
    assert ws.intact() and bool((ws.live[nb:].view(torch.int32) == NAN32).all()), "sumsq wrote outside its partials"
    assert bool(torch.isfinite(ws.live[:nb]).all())
    return out


def adamw_case(pool, ops, ref, n, branch, inputs):
    h, case = tr.ADAMW_HYPER, f"adamw n{n} {branch['name']}"
    p0, g, m0, v0 = inputs
    gmul, wd = branch["grad_mul"], branch["wd"]
    ss = None
    if branch["clip"] is not None:
        ss = Guarded32(1, zero=True)
        guarded_sumsq(ops, g, ss.live)
        assert ss.intact()
    norm64 = tr.sumsq(g).sqrt().item() * abs(gmul)
    max_norm = tr.f32_as_double(branch["clip"] * norm64) if branch["clip"] else 0.0
    ss_live = None if ss is None else ss.live
    runs = {}
    for path in ("host", "device"):
        p, m, v = Guarded32(n), Guarded32(n), Guarded32(n)
        for dst, src in ((p, p0), (m, m0), (v, v0)):
            dst.live.copy_(src)
        sh = Guarded(1, n, pad=16, guard_rows=0) if branch["shadow"] else None
        shadow = None if sh is None else sh.live[0]
        state = ops.adam_state(h["lr"], *h["betas"], 0)
        for step in range(1, tr.ADAMW_STEPS + 1):
            if path == "host":
                ops.adamw(p.live, g, m.live, v.live, shadow, ss_live, max_norm, gmul, h["lr"], *h["betas"], h["eps"], wd, step)
            else:
                ops.adam_tick(state)
                ops.adamw_dev(p.live, g, m.live, v.live, shadow, ss_live, max_norm, gmul, state, h["eps"], wd)
        torch.cuda.synchronize()
        for name, buf in (("p", p), ("m", m), ("v", v), ("shadow", sh)):
            assert buf is None or buf.intact(), f"{case} {path}: wrote behind {name}"
        assert path == "host" or float(state[1]) == tr.ADAMW_STEPS
        runs[path] = (p.live, m.live, v.live, shadow)
    for a, b in zip(runs["host"], runs["device"]):
        assert (a is None and b is None) or torch.equal(a, b), f"{case}: dw_adamw and dw_adam_tick + dw_adamw_dev differ"
    rp, rm, rv = p0.clone(), m0.clone(), v0.clone()
    for step in range(1, tr.ADAMW_STEPS + 1):
        ref.adamw(rp, g, rm, rv, None, ss_live, max_norm, gmul, h["lr"], *h["betas"], h["eps"], wd, step)
    want = tr.adamw_steps(p0, g, m0, v0, None if ss is None else ss.live.double().item(), max_norm, gmul, h["lr"], h["betas"], h["eps"], wd,
                          tr.ADAMW_STEPS)
    p, m, v, shadow = runs["host"]
    for name, x, rx, x64 in zip("pmv", (p, m, v), (rp, rm, rv), want):
        pool.rows(name, case, x, rx, x64, 1)
    if shadow is not None:
        off = (shadow.double() - tr.to_bf16(want[0]).double()).abs()
        pool.expect(bool((off <= tr.bf16_ulp(want[0])).all()), f"{case}: shadow more than a bf16 ulp from bf16(p)")


def test_adamw_small_sizes_all_branches(ops, ref):
    """n = 1, 3, 4, 5, 1027 (no full vector / one / one + a scalar tail / a tail on the block's second pass) x every branch."""
    pool = Pool()
    for n in [n for n in tr.ADAMW_N if n <= 1027]:
        inputs = dev(*tr.adamw_inputs(n))
        for branch in tr.ADAMW_BRANCHES:
            adamw_case(pool, ops, ref, n, branch, inputs)
    pool.check()


@pytest.mark.parametrize("n", [n for n in tr.ADAMW_N if n > 1027])
def test_adamw_grid_stride_wrap(ops, ref, n):
    """2048 * 1024 + 1027 wraps the grid of dw_sumsq_f32, 4096 * 1024 + 1027 that of the AdamW kernels as well; the scalar tail falls on the
    wrapped pass."""
    pool = Pool()
    inputs = dev(*tr.adamw_inputs(n))
    for branch in tr.ADAMW_BRANCHES:
        if branch["name"] in tr.ADAMW_BIG_BRANCHES:
            adamw_case(pool, ops, ref, n, branch, inputs)
    pool.check()


@pytest.mark.parametrize("n", tr.ADAMW_N)
def test_sumsq(ops, n):
    """Against float64 relative to the sum; added to what `out` holds; the same bits from a second call (the replicas' determinism)."""
    g = tr.adamw_inputs(n)[1].to(DEV)
    want = tr.sumsq(g).item()
    a, b = Guarded32(1, zero=True), Guarded32(1, zero=True)
    guarded_sumsq(ops, g, a.live)
    guarded_sumsq(ops, g, b.live)
    assert a.intact() and b.intact()
    assert a.live.view(torch.int32).item() == b.live.view(torch.int32).item()
    rel = abs(a.live.double().item() - want) / want
    print(f"TRAIN_EDGE sumsq n{n} rel {rel:.4e}")
    assert rel <= SUMSQ_REL
    base = 3.0 * want
    c = Guarded32(1)
    c.live.fill_(base)
    base32 = c.live.item()
    guarded_sumsq(ops, g, c.live)
    # out += s in fp32: the fp32 sum of the two fp32 terms, exactly
    assert c.live.item() == (torch.tensor(base32, dtype=F32) + a.live.cpu()[0]).item()
