"""The helpers of tests/test_attention_edges_gpu.py, checked without a GPU: the float64 restatement of attention and its per-row
metric (tests/attention_restatement.py) against `RefOps("cpu")`, the restatement with the kernels' rounding points, and the closed
form of the mask census against the same.

Bounds: `RefOps` keeps lse in fp32 (within 5e-6 of float64 at these score sizes: one ulp of a value below 32 is 1.9e-6) and rounds
P, dS and the outputs to bf16, which costs row_err up to 3.9e-3 (o), 8.7e-3 (dq), 4.5e-3 (dk / dv) at unit-scale inputs and up to
3.2e-2 (dk) with q and k scaled by 4 -- all below 5e-2, where one wrong row (row_err of order 1) cannot hide."""
import pytest
import torch

import attention_restatement as ar
from oracle.ref_ops import RefOps

REF = RefOps("cpu")
SMALL = [c for c in ar.SWEEP if c[2] <= 447 and c[3] <= 447]
SMALL_BR = [c for c in ar.SWEEP_BR if c[2] <= 447 and c[3] <= 447]


@pytest.mark.parametrize("B,H,Lq,Lk,causal,f", SMALL)
def test_ref_ops_agrees_with_float64_per_row(B, H, Lq, Lk, causal, f):
    q, k, v, do = ar.sweep_inputs(B, H, Lq, Lk, f)
    o, lse = REF.attn_fwd(q, k, v, B, H, Lq, Lk, causal, ar.SCALE)
    o64, lse64 = ar.attn_fwd(q, k, v, B, H, Lq, Lk, causal)
    assert (lse.double() - lse64).abs().max().item() <= 5e-6
    ar.check("o", o, o64, H, 5e-2)
    dq, dk, dv = REF.attn_bwd(q, k, v, o, do, lse, B, H, Lq, Lk, causal, ar.SCALE)
    for name, x, want in zip(("dq", "dk", "dv"), (dq, dk, dv), ar.attn_bwd(q, k, v, do, B, H, Lq, Lk, causal)):
        ar.check(name, x, want, H, 5e-2)


@pytest.mark.parametrize("B,H,Lq,Lk,pitch", SMALL_BR)
def test_ref_ops_agrees_with_float64_bottom_right(B, H, Lq, Lk, pitch):
    q, k, v, _ = ar.sweep_inputs(B, H, Lq, Lk, kv_batch_rows=pitch)
    o, lse = REF.attn_fwd(q, k, v, B, H, Lq, Lk, 2, ar.SCALE, kv_batch_rows=pitch)
    o64, lse64 = ar.attn_fwd(q, k, v, B, H, Lq, Lk, 2, kv_batch_rows=pitch)
    assert (lse.double() - lse64).abs().max().item() <= 5e-6
    ar.check("o", o, o64, H, 5e-2)


def test_row_err_sees_one_wrong_row_that_the_frobenius_norm_hides():
    _, _, _, ref = ar.sweep_inputs(1, 2, 447, 1)
    x = ref.clone()
    x[200, 64:] = (x[200, 64:].float() * 1.3).bfloat16()       # one (row, head) vector 30 % off
    frob = ((x.float() - ref.float()).norm() / ref.float().norm()).item()
    assert frob < 1e-2 < 0.25 < ar.row_err(x, ref, 2) < 0.35
    assert ar.row_err(ref, ref, 2) == 0.0
    z = torch.zeros_like(ref)
    z[0, 0] = 1.0                                              # rows of a zero norm are judged on the tensor's scale
    assert ar.row_err(z * 0.5, z, 2) == pytest.approx(0.5)


def _census_cases():
    for causal in (0, 1):
        for Lq in ar.TILE_LQ:
            for Lk in ar.TILE_LK:
                yield 1, Lq, Lk, Lk, causal
    for B, Lq, Lk, pitch in ar.BR_CASES:
        yield B, Lq, Lk, pitch, 2
    for Lk in ar.ONE_LK:
        yield 1, 1, Lk, Lk, 0
        yield 1, 1, Lk, Lk, 2
    for Lk in ar.ONE_CAUSAL1_LK:
        yield 1, 1, Lk, Lk, 1


def test_census_closed_form_against_ref_ops():
    """Integer counts equal, lse within half the gap one key makes (the float64 restatement itself within 3e-7 of log n)."""
    for B, Lq, Lk, pitch, causal in _census_cases():
        k, v = ar.census_kv(B, Lk, pitch)
        q = ar.census_q(B * Lq)
        o, lse = REF.attn_fwd(q, k, v, B, ar.CENSUS_H, Lq, Lk, causal, ar.SCALE, kv_batch_rows=pitch)
        o64, lse64 = ar.attn_fwd(q, k, v, B, ar.CENSUS_H, Lq, Lk, causal, kv_batch_rows=pitch)
        n, want = ar.census_expect(Lq, Lk, causal)
        assert (lse64 - n.double().log()).abs().max().item() <= 3e-7
        for b in range(B):
            name = f"B{B} Lq{Lq} Lk{Lk} causal{causal} batch {b}"
            ar.census_check(name, o[b * Lq:(b + 1) * Lq], lse[b], Lq, Lk, causal)
            assert torch.equal(ar.census_counts(o64[b * Lq:(b + 1) * Lq], n), want), name
    for Lk in ar.ONE_LK_LSE_ONLY:           # head 0 counts pass 64: lse only
        k, v = ar.census_kv(1, Lk)
        o, lse = REF.attn_fwd(ar.census_q(1), k, v, 1, ar.CENSUS_H, 1, Lk, 0, ar.SCALE)
        ar.census_check(f"Lk{Lk}", o, lse[0], 1, Lk, 0, counts=False)


def test_census_expectation_by_hand():
    n, c = ar.census_expect(3, 130, 2)      # bottom-right aligned: query i sees keys <= i + 127
    assert n.tolist() == [128, 129, 130]
    assert c[0, :64].tolist() == [2] * 64 and c[1, :64].tolist() == [3] + [2] * 63 and c[2, :64].tolist() == [3, 3] + [2] * 62
    assert c[2, 64:67].tolist() == [64, 64, 2] and c[0, 64:67].tolist() == [64, 64, 0]
    n, c = ar.census_expect(1, 600, 1)      # causal 1: the single query is query 0
    assert n.tolist() == [1] and c.sum().item() == 2 and c[0, 0] == 1 and c[0, 64] == 1
    n, _ = ar.census_expect(130, 70, 1)     # more queries than keys: the late ones see every key
    assert n.tolist() == list(range(1, 71)) + [70] * 60
    assert ar.census_lse_bound(torch.tensor([1500])) == pytest.approx(0.5 * 6.7e-4, rel=1e-2)


@pytest.mark.parametrize("B,H,Lq,Lk,causal", [(1, 1, 1, 1, 0), (2, 2, 33, 1, 0), (1, 2, 70, 1, 1), (2, 1, 1, 9, 1), (1, 2, 1, 600, 1)])
def test_zero_reference_cases(B, H, Lq, Lk, causal):
    """Every query sees one key: P = 1, dS = 0, so dq = dk = 0, and dv is dO on the visible key.  The float64 restatement returns
    exact zeros (its delta is summed over the keys: one term).  `RefOps` forms delta = dO . o like the kernels, in fp32, next to
    dP = dO . v from a matrix product: the same 64 terms in two summation orders, so what it leaves depends on the BLAS at hand
    (measured: 0 at one query, 2e-7 at 33) and is held to the bound of a zero reference instead."""
    q, k, v, do = ar.sweep_inputs(B, H, Lq, Lk)
    dq64, dk64, dv64 = ar.attn_bwd(q, k, v, do, B, H, Lq, Lk, causal)
    assert ar.zero_ref(dq64) and ar.zero_ref(dk64) and not ar.zero_ref(dv64)
    o, lse = REF.attn_fwd(q, k, v, B, H, Lq, Lk, causal, ar.SCALE)
    dq, dk, dv = REF.attn_bwd(q, k, v, o, do, lse, B, H, Lq, Lk, causal, ar.SCALE)
    assert ar.check("dq", dq, dq64, H, 0.0) <= ar.ZERO_ABS and ar.check("dk", dk, dk64, H, 0.0) <= ar.ZERO_ABS
    assert ar.row_err(dv, dv64, H) <= 2.0 ** -8
