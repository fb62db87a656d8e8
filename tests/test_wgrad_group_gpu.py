"""dw_wgrad_group (csrc/gemm_wgrad_group.hip): the grouped weight-gradient GEMM -- C_i (+)= A_i^T . B_i for up to four problems in one
launch of 320 x 256 tiles, no K slices -- called directly and through the engine's layer backward.

Judged against the float64 product of the same bf16 inputs.  The bound is the one of the float64-judged weight-gradient test of the
training kernels, tests/test_training_kernels_edges_gpu.py::test_layernorm_width_sweep (dgamma, the LayerNorm weight gradient):
row_err(kernel, float64) <= F_BOUND["dgamma"] x e_ref, e_ref = row_err(RefOps, float64) on the same inputs, row_err per output row.
No number of this module's own.

Cases: one-problem groups (320, 256) and (640, 512); a four-problem group with four different (m, n) -- the matrices of an encoder
layer at D = 1280 -- whose 240 tiles exercise the job decoding on every XCD, both tile orders (tiles_m <= tiles_n and the reverse) and
a last XCD range; k = 64, 128, 192, 448 = 1, 2, 3 and 7 K tiles (every peeled branch of the K loop); leading dimensions larger than the
widths; overwrite onto NaN, accumulate onto a non-zero buffer, two launches bit for bit; the refusals."""
import ctypes as C

import pytest
import torch

import training_restatement as tr
from guarded import DEV, Guarded
from test_training_kernels_edges_gpu import F_BOUND

pytestmark = pytest.mark.gpu

F = F_BOUND["dgamma"]
LAYER = [(1280, 1280), (3840, 1280), (5120, 1280), (1280, 5120)]
GROUPS = {"one_tile": [(320, 256)], "four_tiles": [(640, 512)], "layer": LAYER}
DW_EINVAL = -1


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps(DEV)


@pytest.fixture(scope="module")
def ref():
    from oracle.ref_ops import RefOps
    return RefOps(DEV)


def rnd(shape, scale, seed, dtype=torch.bfloat16):
    g = torch.Generator(device=DEV).manual_seed(seed)
    return (torch.randn(shape, generator=g, device=DEV, dtype=torch.float32) * scale).to(dtype)


def operands(group, k, seed):
    """[(dy [k, m] with pitch m + 8, x [k, n] with pitch n + 16)] -- views into wider buffers"""
    out = []
    for i, (m, n) in enumerate(group):
        out.append((rnd((k, m + 8), 0.5, seed + 2 * i)[:, :m], rnd((k, n + 16), 0.5, seed + 2 * i + 1)[:, :n]))
    return out


def launch(ops, triples, k, accumulate):
    """dw_wgrad_group itself -> its return code"""
    from distil_whisper_amd.ops_hip import DwWgradProblem
    arr = (DwWgradProblem * len(triples))()
    for q, (dy, x, out) in zip(arr, triples):
        q.a, q.b, q.c = dy.data_ptr(), x.data_ptr(), out.data_ptr()
        q.lda, q.ldb, q.ldc = dy.stride(0), x.stride(0), out.stride(0)
        q.m, q.n = dy.shape[1], x.shape[1]
    rc = ops.lib.dw_wgrad_group(arr, len(triples), k, int(accumulate), ops._stream())
    torch.cuda.synchronize()
    return rc


def judge(what, got, want32, want64):
    e, e_ref = tr.row_err(got, want64, got.shape[1]), tr.row_err(want32, want64, got.shape[1])
    print(f"WGRAD_GROUP {what} kernel {e:.4e} ref {e_ref:.4e} ratio {e / e_ref if e_ref else float('nan'):.3f}")
    assert bool(torch.isfinite(got).all()), f"{what}: non-finite values"
    assert e <= F * e_ref, f"{what}: {e:.3e} > {F:g} x {e_ref:.3e}"


@pytest.mark.parametrize("k", [64, 128, 192, 448])
@pytest.mark.parametrize("name", list(GROUPS))
def test_group_against_float64(ops, ref, name, k):
    group = GROUPS[name]
    ab = operands(group, k, seed=100 + k)
    want64 = [dy.double().t() @ x.double() for dy, x in ab]
    want32 = [ref.gemm(dy, x, trans_a=True, trans_b=True, out_dtype=torch.float32) for dy, x in ab]
    # overwrite: every output NaN-patterned with its guards (pitch n + 4: leading dimension larger than the width); no stale value
    # survives and nothing outside the live view is written
    outs = [Guarded(m, n, pad=4, dtype=torch.float32) for m, n in group]
    assert launch(ops, [(dy, x, o.live) for (dy, x), o in zip(ab, outs)], k, False) == 0
    for i, o in enumerate(outs):
        assert o.intact(), f"{name} k={k} problem {i}: wrote outside the output"
        judge(f"{name} k={k} overwrite problem {i} {group[i]}", o.live, want32[i], want64[i])
    # the same launch again: the same bits
    again = [Guarded(m, n, pad=4, dtype=torch.float32) for m, n in group]
    assert launch(ops, [(dy, x, o.live) for (dy, x), o in zip(ab, again)], k, False) == 0
    for i, (o, o2) in enumerate(zip(outs, again)):
        assert torch.equal(o.live, o2.live), f"{name} k={k} problem {i}: two launches differ"
    # accumulate onto a non-zero buffer
    base = [rnd((m, n), 1.0, 900 + i, torch.float32) for i, (m, n) in enumerate(group)]
    accs = [Guarded(m, n, pad=4, dtype=torch.float32) for m, n in group]
    for a, b in zip(accs, base):
        a.live.copy_(b)
    assert launch(ops, [(dy, x, o.live) for (dy, x), o in zip(ab, accs)], k, True) == 0
    for i, o in enumerate(accs):
        assert o.intact(), f"{name} k={k} problem {i}: accumulate wrote outside the output"
        judge(f"{name} k={k} accumulate problem {i} {group[i]}", o.live, base[i] + want32[i], base[i].double() + want64[i])


@pytest.mark.parametrize("what,m,n,k", [("m = 256", 256, 256, 64), ("n = 320", 320, 320, 64), ("k = 96", 320, 256, 96),
                                        ("more tiles than CUs", 320 * 17, 256 * 16, 64)])
def test_refusals_launch_nothing(ops, what, m, n, k):
    dy, x = rnd((k, m), 0.5, 1), rnd((k, n), 0.5, 2)
    out = Guarded(m, n, pad=0, dtype=torch.float32)
    for accumulate in (False, True):
        assert launch(ops, [(dy, x, out.live)], k, accumulate) == DW_EINVAL, what
    assert out.untouched(), f"{what}: a refused call wrote to its output"
    # ... and as the second problem of a group whose first is fine
    dy0, x0 = rnd((k, 320), 0.5, 3), rnd((k, 256), 0.5, 4)
    out0 = Guarded(320, 256, pad=0, dtype=torch.float32)
    assert launch(ops, [(dy0, x0, out0.live), (dy, x, out.live)], k, False) == DW_EINVAL, what
    assert out0.untouched() and out.untouched(), f"{what}: a refused group wrote to an output"


def test_refusals_of_count_pointers_and_pitches(ops):
    k = 64
    dy, x = rnd((k, 320 + 8), 0.5, 5), rnd((k, 256 + 8), 0.5, 6)
    out = Guarded(320, 256, pad=4, dtype=torch.float32)
    good = (dy[:, :320], x[:, :256], out.live)
    from distil_whisper_amd.ops_hip import DwWgradProblem
    assert ops.lib.dw_wgrad_group(None, 1, k, 0, ops._stream()) == DW_EINVAL
    assert launch(ops, [good] * 5, k, False) == DW_EINVAL                                   # more than four problems
    assert ops.lib.dw_wgrad_group((DwWgradProblem * 1)(), 0, k, 0, ops._stream()) == DW_EINVAL
    assert launch(ops, [(dy[:, 4:324], x[:, :256], out.live)], k, False) == DW_EINVAL         # a 8 bytes off 16
    assert launch(ops, [(dy[:, :320], x[:, :256], out.buf[:320, 1:257])], k, False) == DW_EINVAL   # c 4 bytes off 16
    odd = rnd((k, 320 + 4), 0.5, 7)
    assert launch(ops, [(odd[:, :320], x[:, :256], out.live)], k, False) == DW_EINVAL         # lda not a multiple of 8
    assert out.untouched()
    assert launch(ops, [good], k, False) == 0 and out.intact()
