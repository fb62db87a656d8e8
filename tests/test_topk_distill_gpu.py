"""The kernels of csrc/topk_distill.hip -- `dw_logits_topk`, `dw_distill_loss_topk`, `dw_distill_loss_topk_w` -- against the float64
restatement tests/topk_distill_restatement.py, and the trainer's steps with stored targets on the device.

The bound is the form of tests/test_training_kernels_edges_gpu.py, per judged tensor and PER CASE:
row_err(kernel, float64) <= F * e_ref, e_ref = row_err(torch fp32 statement of distil_whisper_amd/topk_distill.py, float64) on the same
inputs; `idx` is exact; losses[0:3] are one 3-vector; row_ce / row_kl are judged absolutely; the gradient per row and element-wise
beyond one bf16 ulp.  One-row cases of row_ce / row_kl state an a priori floor (one fp32 ulp of the magnitudes the terms are differences
of), as that module's few-value cases do; logp and rest have none.  The dense-limit test holds the kernel to F against float64 like
every case and, next to it, to 2 F e_ref against `dw_distill_loss` on the same rows: two kernels that each sit within F e_ref of
the same float64 values (measured: losses 1.25 and 0.51 e_ref, gradient 0.02 and 0.00 e_ref at V 1030 / 51866).

Measured on the MI355X, the largest row_err(kernel) / e_ref of any single case, that case, and F = the smallest of 2, 3, 4 that is at
least 1.5 x the ratio:
  logp    1.00  (V 1030, 5 rows, k 32, T 1; every case <= 1.00: the stored value is one rounding of a double)    F 2
  rest    1.00  (V 1030, pitch 1040, 3 rows, k 8, T 1)                                                           F 2
  losses  1.27  (V 51866, the 3 planted rows, T 2, k 8; losses[0:3] as one 3-vector)                             F 2
  row_ce  1.03  (V 51865, one row, under its floor; 1.00 at V 51865, 3 rows, near, k 64)                         F 2
  row_kl  1.44  (V 1030, 3 gauss rows shifted by -120, T 1, k 8: 1.4e-7 against 9.8e-8 absolute)                 F 3
  grad    1.00  per row (bf16 rounding); element-wise no case leaves a residual beyond one bf16 ulp on either side   F 2, 2
Two findings of the first measurements, fixed in the kernels rather than in F: with fast exponentials and fp32 logarithms `rest`
measured 12.1 x (V 1030, the all-equal row: every term carries the same error) and row_kl 5.3 x (the planted rows at V 51866: an
fp32 rounding of log Z = 11 enters the row's term), logp 4.4 x.  dw_logits_topk now sums accurate exponentials in double and takes
the row's log and quotient in double; the loss takes the row's few logarithms, differences and the means in double."""
import numpy as np
import pytest
import torch

import topk_distill_restatement as tk
import training_restatement as tr
from guarded import DEV, Guarded, Guarded32

pytestmark = pytest.mark.gpu

BF16, F32 = torch.bfloat16, torch.float32
ULP32 = 2.0 ** -23
# F per judged tensor (module docstring)
F_BOUND = {"logp": 2.0, "rest": 2.0, "losses": 2.0, "row_ce": 2.0, "row_kl": 3.0, "grad": 2.0, "grad_elem": 2.0}


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps(DEV)


class Pool:
    """tests/test_training_kernels_edges_gpu.py's Pool over this module's F_BOUND: every case is noted (and printed) with its own
    e_ref; check() asserts row_err <= max(F * e_ref, floor) for every case."""

    def __init__(self):
        self.notes, self.bad = [], []

    def note(self, name, case, e, e_ref, floor=0.0):
        print(f"TOPK_EDGE {case} {name} kernel {e:.4e} ref {e_ref:.4e} floor {floor:.4e} ratio {e / e_ref if e_ref else float('nan'):.3f}")
        self.notes.append((name, case, e, e_ref, floor))

    def expect(self, ok, what):
        if not ok:
            self.bad.append(what)

    def rows(self, name, case, x, x_ref, x64, width, floor=0.0):
        x64 = x64.to(x.device)
        self.expect(bool(torch.isfinite(x.float()).all()), f"{case} {name}: non-finite values")
        if not bool(x64.any()):
            return self.expect(not bool(x.any()), f"{case} {name}: not exactly zero against a zero reference")
        self.note(name, case, tr.row_err(x, x64, width), tr.row_err(x_ref, x64, width), floor)

    def absolute(self, name, case, x, x_ref, x64, floor=0.0):
        x64 = x64.to(x.device)
        self.expect(bool(torch.isfinite(x).all()), f"{case} {name}: non-finite values")
        self.note(name, case, (x.double() - x64).abs().max().item(), (x_ref.double() - x64).abs().max().item(), floor)

    def check(self):
        for name, case, e, e_ref, floor in self.notes:
            self.expect(e <= max(F_BOUND[name] * e_ref, floor), f"{case} {name}: {e:.3e} > {F_BOUND[name]:g} x {e_ref:.3e} (floor {floor:.3e})")
        assert not self.bad, "\n".join(self.bad)


def bits(x):
    return x.view(torch.int16) if x.dtype == BF16 else x.view(torch.int32)


# ---- dw_logits_topk ------------------------------------------------------------------------------------------------------------------
def run_topk(ops, z, V, T, k):
    """The C entry into guarded outputs -> idx int32 [rows, k], logp, rest."""
    from distil_whisper_amd.ops_hip import _p
    rows, ld = z.shape
    gi, gl, gr = Guarded32(rows * k), Guarded32(rows * k), Guarded32(rows)
    ops._chk(ops.lib.dw_logits_topk(_p(z), rows, V, ld, T, k, _p(gi.buf), _p(gl.buf), _p(gr.buf), ops._stream()), "logits_topk")
    torch.cuda.synchronize()
    assert gi.intact() and gl.intact() and gr.intact(), "dw_logits_topk wrote outside its outputs"
    return gi.live.view(torch.int32).view(rows, k).clone(), gl.live.view(rows, k).clone(), gr.live.clone()


TOPK_CASES = [(V, pad, rows, k, T) for i, (V, pad) in enumerate([(1030, 2), (1030, 10), (51865, 3), (51865, 7), (51866, 6), (51866, 102)])
              for j, (rows, k) in enumerate([(1, 1), (3, 8), (5, 32), (5, 64), (3, 64), (1, 32)]) for T in ((1.0, 2.0)[(i + j) % 2],)]


@pytest.mark.parametrize("V,pad", sorted({c[:2] for c in TOPK_CASES}))
def test_logits_topk(ops, V, pad):
    from distil_whisper_amd import topk_distill
    pool = Pool()
    for _, _, rows, k, T in [c for c in TOPK_CASES if c[:2] == (V, pad)]:
        case = f"topk V{V} ld{V + pad} rows{rows} k{k} T{T:g}"
        z = tk.tie_rows(V, k)[:rows]
        zp = torch.cat([z, torch.full((rows, pad), tr.LOSS_PAD, dtype=BF16)], 1).contiguous().to(DEV)
        idx, logp, rest = run_topk(ops, zp, V, T, k)
        idx2, logp2, rest2 = run_topk(ops, zp, V, T, k)
        assert torch.equal(idx, idx2) and torch.equal(bits(logp), bits(logp2)) and torch.equal(bits(rest), bits(rest2)), case
        widx, wlogp, wrest = tk.targets(z, V, T, k)
        assert np.array_equal(idx.cpu().numpy().astype(np.int64), widx), case
        ridx, rlogp, rrest = topk_distill.logits_topk_torch(zp, V, T, k)
        assert np.array_equal(ridx.cpu().numpy().astype(np.int64), widx), case
        pool.rows("logp", case, logp, rlogp, torch.from_numpy(wlogp), k)
        pool.rows("rest", case, rest, rrest, torch.from_numpy(wrest), 1)
    pool.check()


def test_logits_topk_invalid_arguments_are_rejected_and_write_nothing(ops):
    from distil_whisper_amd.ops_hip import _p
    rows, V, ld, k = 3, 40, 44, 4
    z = torch.randn(rows, ld, device=DEV).to(BF16)
    gi, gl, gr = Guarded32(rows * 64), Guarded32(rows * 64), Guarded32(rows)

    def f(z_=z.data_ptr(), i_=gi.buf.data_ptr(), l_=gl.buf.data_ptr(), r_=gr.buf.data_ptr(), V_=V, ld_=ld, T=2.0, k_=k, code=-1):
        with pytest.raises(RuntimeError, match=f"code {code}$"):
            ops._chk(ops.lib.dw_logits_topk(z_, rows, V_, ld_, T, k_, i_, l_, r_, ops._stream()), "logits_topk")

    f(z_=None), f(i_=None), f(l_=None), f(r_=None), f(z_=z.data_ptr() + 2), f(i_=gi.buf.data_ptr() + 2), f(T=0.0), f(T=-1.0)
    f(V_=ld + 1), f(ld_=V - 4), f(ld_=42), f(k_=0), f(k_=V), f(k_=V + 1)
    f(k_=65, V_=128, ld_=128, code=-2), f(V_=53252, ld_=53252, code=-2)          # (refused before anything is read)
    torch.cuda.synchronize()
    assert gi.untouched() and gl.untouched() and gr.untouched()
    ops._chk(ops.lib.dw_logits_topk(_p(z), rows, V, ld, 2.0, k, _p(gi.buf), _p(gl.buf), _p(gr.buf), ops._stream()), "logits_topk")
    torch.cuda.synchronize()
    assert not gi.untouched() and not gr.untouched()


# ---- dw_distill_loss_topk --------------------------------------------------------------------------------------------------------------
def planted(V, ld, T, k=8):
    """Two planted rows next to a Gaussian one.  Row 0: the student's mass outside the teacher's k columns is around 1e-12 while the
    teacher's `rest` is around 1e-3.  Row 1: rest == 0 (the teacher's tail 200 T below).  -> s, t, labels."""
    g = torch.Generator().manual_seed(V + 5)
    s, t = 2.0 * torch.randn(3, V, generator=g), 2.0 * torch.randn(3, V, generator=g)
    cols = torch.randperm(V, generator=g)[:k]
    top = torch.randn(k, generator=g)
    t[0], s[0] = -T * float(np.log(V * 1e3)), -T * float(np.log(V * 1e12))
    t[0, cols], s[0, cols] = top, torch.randn(k, generator=g)
    t[1] = -260.0 * T
    t[1, cols] = top
    full = lambda z: torch.cat([z.to(BF16), torch.full((3, ld - V), tr.LOSS_PAD, dtype=BF16)], 1).contiguous()
    return full(s), full(t), torch.tensor([int(cols[0]), V - 1, 0])


LOSS_CASES = [(V, ld, rows, kind, T, w, regime, k)
              for i, (V, ld) in enumerate([(1030, 1032), (51865, 51872), (51866, 51968)])
              for j, (rows, kind, w) in enumerate([(1, "random", (0.8, 1.0)), (3, "edges", (0.0, 1.0)), (97, "random", (0.8, 1.0)), (3, "ignored", (1.0, 0.0))])
              for T, regime, k in (((1.0, 2.0)[(i + j) % 2], ("gauss", "spiked", "near")[(i + j) % 3], (8, 32, 64, 1)[(i + j) % 4]),)]
LOSS_CASES += [(V, ld, 3, "planted", T, (0.8, 1.0), "planted", 8) for V, ld, T in ((1030, 1032, 2.0), (51866, 51968, 1.0), (51866, 51968, 2.0))]
# rows whose largest student logit lies below -88 (exp(0 - max) overflows fp32): a gauss row shifted by -120, and by -200 at T = 2
LOSS_CASES += [(1030, 1032, 3, "shift120", 1.0, (0.8, 1.0), "gauss", 8), (51866, 51968, 3, "shift200", 2.0, (0.8, 1.0), "gauss", 32),
               (51865, 51872, 1, "shift120", 2.0, (0.8, 1.0), "gauss", 8)]
_cache = {}


def loss_inputs(case):
    """Inputs and the float64 reference of a case, computed once (CPU)."""
    if case not in _cache:
        from distil_whisper_amd import topk_distill
        V, ld, rows, kind, T, w, regime, k = case
        if kind.startswith("shift"):
            s, t, labels = tr.loss_inputs(V, ld, rows, regime, "random")
            s[:, :V] = (s[:, :V].float() - float(kind[5:])).to(BF16)
        else:
            s, t, labels = planted(V, ld, T, k) if kind == "planted" else tr.loss_inputs(V, ld, rows, regime, kind)
        idx, logp, rest = topk_distill.logits_topk_torch(t, V, T, k)
        _cache[case] = (s, t, labels, idx, logp, rest, tk.loss(s, idx, logp, rest, labels, V, T, w[0], w[1], 1.0))
    return _cache[case]


def poisoned(idx, logp, rest, labels, V):
    idx, logp, rest = idx.clone(), logp.clone(), rest.clone()
    dead = labels < 0
    idx[dead] = 2 ** 31 - 1
    idx[dead, ::2] = -2 ** 31
    logp[dead] = float("nan")
    rest[dead] = float("inf")
    return idx, logp, rest


def loss_case(pool, ops, case):
    from distil_whisper_amd import topk_distill
    V, ld, rows, kind, T, (ce_w, kl_w), regime, k = case
    name = f"loss V{V} ld{ld} rows{rows} {kind} T{T:g} w{ce_w:g}/{kl_w:g} {regime} k{k}"
    s, t, labels, idx, logp, rest, want = loss_inputs(case)
    s, labels, idx, logp, rest = (x.to(DEV) for x in (s, labels, idx, logp, rest))
    row_ce64, row_kl64, losses64, grad64 = (x.to(DEV) for x in want)
    g0 = Guarded(rows, ld, pad=0)
    g0.live.copy_(s)
    losses, row_ce, row_kl = ops.distill_loss_topk(g0.live, idx, logp, rest, labels, V, T, ce_w, kl_w, 1.0, True, return_rows=True)
    pi, pl, pr = poisoned(idx, logp, rest, labels, V)
    g1, s1 = Guarded(rows, ld, pad=0), s.clone()
    l1, ce1, kl1 = ops.distill_loss_topk(s1, pi, pl, pr, labels, V, T, ce_w, kl_w, 1.0, True, grad_out=g1.live, return_rows=True)
    g2 = Guarded(rows, ld, pad=0)
    g2.live.copy_(s)
    wdev = torch.tensor([ce_w, kl_w], dtype=F32, device=DEV)
    l2, ce2, kl2 = ops.distill_loss_topk(g2.live, idx, logp, rest, labels, V, T, 123.0, 456.0, 1.0, True, weights_dev=wdev, return_rows=True)
    l3 = ops.distill_loss_topk(s.clone(), pi, pl, pr, labels, V, T, ce_w, kl_w, 1.0, False)
    torch.cuda.synchronize()
    assert g0.intact() and g1.intact() and g2.intact(), f"{name}: wrote behind the gradient"
    assert torch.equal(s1, s), f"{name}: grad_out given, the student logits changed"
    for way, got in (("grad_out + poisoned ignored rows", (l1, ce1, kl1, g1.live)), ("weights_dev", (l2, ce2, kl2, g2.live))):
        for a, b in zip(got, (losses, row_ce, row_kl, g0.live)):
            assert torch.equal(bits(a), bits(b)), f"{name}: {way} differs from the in-place call"
    assert torch.equal(bits(l3), bits(losses)), f"{name}: the losses differ without the gradient"
    grad = g0.live
    rs = s.clone()
    rlosses, rce, rkl = topk_distill.distill_loss_topk_torch(rs, idx, logp, rest, labels, V, T, ce_w, kl_w, 1.0, True, return_rows=True)
    n_valid = int((labels != -100).sum())
    assert losses[3].item() == n_valid == losses64[3].item()
    pool.expect(not bool(grad[:, V:].any()), f"{name}: gradient pad columns not zero")
    if n_valid == 0:
        pool.expect(bool(torch.isnan(losses[:3]).all()), f"{name}: losses of an all-ignored batch {losses.tolist()}")
        pool.expect(not bool(grad.any()), f"{name}: gradient of an all-ignored batch not zero")
        pool.expect(not bool(row_ce.any()) and not bool(row_kl.any()), f"{name}: per-row terms of an all-ignored batch not zero")
        return None
    pool.rows("losses", name, losses[:3], rlosses[:3], losses64[:3], 3)
    ce_floor = kl_floor = 0.0
    if rows == 1:
        zs = s[:, :V].double()
        ce_floor = ULP32 * (torch.logsumexp(zs, 1).abs() + zs.abs().max(1).values).max().item()
        kl_floor = ULP32 * (torch.logsumexp(zs / T, 1).abs() + zs.abs().max(1).values / T + logp.double().abs().max()).max().item()
    pool.absolute("row_ce", name, row_ce, rce, row_ce64, floor=ce_floor)
    pool.absolute("row_kl", name, row_kl, rkl, row_kl64, floor=kl_floor)
    g, rg = grad[:, :V], rs[:, :V]
    pool.rows("grad", name, g, rg, grad64, V)
    want_b, ulp = tr.to_bf16(grad64).double(), tr.bf16_ulp(grad64)
    res = ((g.double() - want_b).abs() - ulp).clamp_min(0.0)
    rres = ((rg.double() - want_b).abs() - ulp).clamp_min(0.0)
    pool.expect(not bool(g[grad64 == 0].any()), f"{name}: gradient not zero where the float64 gradient is")
    if rres.max().item() == 0.0:
        pool.expect(res.max().item() == 0.0, f"{name}: gradient element off by 1 bf16 ulp + {res.max().item():.3e}, the statement by none")
    else:
        pool.note("grad_elem", name, res.max().item(), rres.max().item())
    return losses, grad


@pytest.mark.parametrize("V,ld", sorted({c[:2] for c in LOSS_CASES}))
def test_distill_loss_topk(ops, V, ld):
    """Each case in place, with grad_out (and poisoned targets in the ignored rows), with weights_dev and without the gradient (same
    bits); losses / per-row terms / gradient against float64."""
    pool = Pool()
    for case in [c for c in LOSS_CASES if c[:2] == (V, ld)]:
        loss_case(pool, ops, case)
    pool.check()


@pytest.mark.parametrize("V,ld,T", [(1030, 1032, 2.0), (51866, 51968, 1.0)])
def test_distill_loss_topk_dense_limit(ops, V, ld, T):
    """Teacher rows whose tail lies 260 T below their k columns (rest == 0): the kernel against float64 under the bound, and against
    `dw_distill_loss` on the same rows -- both sit within their bounds of the same float64 values."""
    from distil_whisper_amd import topk_distill
    rows, k = 5, 8
    g = torch.Generator().manual_seed(V)
    t = torch.full((rows, V), -260.0 * T)
    cols = torch.stack([torch.randperm(V, generator=g)[:k] for _ in range(rows)])
    t.scatter_(1, cols, torch.randn(rows, k, generator=g) * 2.0)
    full = lambda z: torch.cat([z.to(BF16), torch.full((rows, ld - V), tr.LOSS_PAD, dtype=BF16)], 1).contiguous()
    s, t = full(2.0 * torch.randn(rows, V, generator=g)), full(t)
    labels = torch.tensor([1, -100, 5, V - 1, 0])
    idx, logp, rest = topk_distill.logits_topk_torch(t, V, T, k)
    assert not bool(rest.any())
    row_ce64, row_kl64, losses64, grad64 = (x.to(DEV) for x in tk.dense_loss(s, t, labels, V, T, 0.8, 1.0, 1.0))
    s, t, labels, idx, logp, rest = (x.to(DEV) for x in (s, t, labels, idx, logp, rest))
    a, b, r = s.clone(), s.clone(), s.clone()
    la = ops.distill_loss_topk(a, idx, logp, rest, labels, V, T, 0.8, 1.0, 1.0, True)
    lb = ops.distill_loss(b, t, labels, V, T, 0.8, 1.0, 1.0, True)
    lr = topk_distill.distill_loss_topk_torch(r, idx, logp, rest, labels, V, T, 0.8, 1.0, 1.0, True)
    pool, case = Pool(), f"dense limit V{V} T{T:g}"
    pool.rows("losses", case, la[:3], lr[:3], losses64[:3], 3)
    pool.rows("grad", case, a[:, :V], r[:, :V], grad64, V)
    e_l, e_g = tr.row_err(lr[:3], losses64[:3], 3), tr.row_err(r[:, :V], grad64, V)
    d_l, d_g = tr.row_err(la[:3], lb[:3].double(), 3), tr.row_err(a[:, :V], b[:, :V].double(), V)
    print(f"TOPK_EDGE {case} against dw_distill_loss: losses {d_l:.3e} (e_ref {e_l:.3e}) grad {d_g:.3e} (e_ref {e_g:.3e})")
    pool.expect(d_l <= 2 * F_BOUND["losses"] * e_l, f"{case}: losses differ from dw_distill_loss by {d_l:.3e}")
    pool.expect(d_g <= 2 * F_BOUND["grad"] * e_g, f"{case}: gradient differs from dw_distill_loss by {d_g:.3e}")
    pool.check()


def test_distill_loss_topk_invalid_arguments_are_rejected_and_write_nothing(ops):
    from distil_whisper_amd import topk_distill
    from distil_whisper_amd.ops_hip import _p
    rows, V, ld, k = 3, 20, 32, 4
    s, t, labels = (x.to(DEV) for x in tr.loss_inputs(V, ld, rows, "gauss", "random"))
    idx, logp, rest = topk_distill.logits_topk_torch(t, V, 2.0, k)
    losses, row_ce, row_kl = Guarded32(4), Guarded32(rows), Guarded32(rows)
    counts = torch.zeros(2, dtype=torch.int32, device=DEV)
    grad = Guarded(rows, ld, pad=0)
    wdev = torch.tensor([0.8, 1.0, 0.0], device=DEV)

    def f(s_=s.data_ptr(), i_=idx.data_ptr(), l_=logp.data_ptr(), r_=rest.data_ptr(), g_=grad.buf.data_ptr(), V_=V, ld_=ld, T=2.0, k_=k,
          code=-1, w_=None):
        with pytest.raises(RuntimeError, match=f"code {code}$"):
            if w_ is None:
                ops._chk(ops.lib.dw_distill_loss_topk(s_, i_, l_, r_, k_, _p(labels), rows, V_, ld_, T, 0.8, 1.0, 1.0, _p(losses.buf), g_,
                                                      _p(row_ce.buf), _p(row_kl.buf), _p(counts), ops._stream()), "distill_loss_topk")
            else:
                ops._chk(ops.lib.dw_distill_loss_topk_w(s_, i_, l_, r_, k_, _p(labels), rows, V_, ld_, T, w_, 1.0, _p(losses.buf), g_,
                                                        _p(row_ce.buf), _p(row_kl.buf), _p(counts), ops._stream()), "distill_loss_topk_w")
        torch.cuda.synchronize()
        for g in (losses, row_ce, row_kl, grad):
            assert g.untouched()

    f(V_=ld + 1), f(ld_=28), f(T=0.0), f(T=-1.0), f(s_=s.data_ptr() + 8), f(g_=grad.buf.data_ptr() + 8)
    f(i_=None), f(l_=None), f(r_=None), f(i_=idx.data_ptr() + 2), f(l_=logp.data_ptr() + 2), f(r_=rest.data_ptr() + 2)
    f(k_=0), f(k_=V), f(k_=65, V_=128, ld_=128, code=-2), f(V_=53256, ld_=53256, code=-2), f(w_=wdev.data_ptr() + 2), f(w_=wdev.data_ptr(), k_=0)
    ops._chk(ops.lib.dw_distill_loss_topk(_p(s), _p(idx), _p(logp), _p(rest), k, _p(labels), rows, V, ld, 2.0, 0.8, 1.0, 1.0, _p(losses.buf),
                                          _p(grad.buf), _p(row_ce.buf), _p(row_kl.buf), _p(counts), ops._stream()), "distill_loss_topk")
    torch.cuda.synchronize()
    assert not losses.untouched() and not grad.untouched()


# ---- the trainer on the device -------------------------------------------------------------------------------------------------------
def test_trainer_with_stored_targets_on_the_device(ops):
    """The CPU scenarios of tests/test_topk_distill.py at the micro width: the kernel path against the torch statements (a trainer
    whose ops lacks the two methods), no teacher launch with targets, trimmed / packed equal to untrimmed, the teacher-less trainer."""
    from distil_whisper_amd import TeacherTopK
    from distil_whisper_amd.distill import DistillationTrainer
    from oracle import whisper_oracle as wo
    from test_topk_distill import Spy, setup

    class Statements:
        """HipOps without the two methods: topk_distill falls back to its torch statements."""

        def __init__(self, inner):
            self._inner = inner

        def __getattr__(self, name):
            if name in ("logits_topk", "distill_loss_topk"):
                raise AttributeError(name)
            return getattr(self._inner, name)

    cfg_t, cfg_s, t_sd, s_sd, batch = setup(seed=3)
    dev = lambda sd: {k_: v.to(DEV) for k_, v in sd.items()}
    f, d, l = (batch[n].to(DEV) for n in ("input_features", "decoder_input_ids", "labels"))
    l = l.clone()
    l[0, 20:] = -100
    l[1, 9:] = -100
    rel = lambda a, b: ((a.float() - b.float()).norm() / (b.float().norm() + 1e-30)).item()
    a = DistillationTrainer(ops, dev(s_sd), cfg_s, dev(t_sd), cfg_t)
    b = DistillationTrainer(Statements(ops), dev(s_sd), cfg_s, dev(t_sd), cfg_t)
    dense = a.forward_backward(f, d, l).clone()
    ta, tb = a.teacher_targets(f, d, l, k=8), b.teacher_targets(f, d, l, k=8)
    live = l >= 0
    assert torch.equal(ta.idx[live], tb.idx[live]) and rel(ta.logp[live], tb.logp[live]) < 1e-5
    spy = Spy(a.teacher)
    la = a.forward_backward(f, d, l, teacher_topk=ta).clone()
    assert spy.n == {"encode": 0, "decode": 0}
    lb = b.forward_backward(f, d, l, teacher_topk=ta).clone()
    assert rel(la[:3], lb[:3]) < 1e-5 and la[3].item() == lb[3].item() == dense[3].item()
    assert abs(la[0].item() - dense[0].item()) <= 1e-5 * abs(dense[0].item()) and la[1].item() <= dense[1].item() * (1 + 1e-5)
    G = a.student_store.G.clone()
    assert rel(G, b.student_store.G) < 2e-2                      # (bf16 gradients of two roundings of the same loss)
    for vl in (20, [20, 9]):
        got = a.forward_backward(f, d, l, teacher_topk=ta, valid_len=vl)
        assert rel(got[:3], la[:3]) < 1e-5 and rel(a.student_store.G, G) < 2e-2, vl
    less = DistillationTrainer(ops, dev(s_sd), cfg_s, None, None)
    assert less.teacher is None
    ll = less.train_step(f, d, l, teacher_topk=ta)
    assert torch.equal(ll, la) and less.step_count == 1
    e = less.eval_step(f, d, l, teacher_topk=TeacherTopK(ta.idx, ta.logp, ta.rest, 1.0, ta.vocab))
    assert bool(torch.isfinite(e).all())
    with pytest.raises(ValueError):
        less.train_step(f, d, l)
    with pytest.raises(NotImplementedError):
        a.train_step_graphed(f, d, l, teacher_topk=ta)
    torch.cuda.synchronize()
