"""The helpers of tests/test_decode_edges_gpu.py, checked without a GPU: the float64 statement of the token step's attention with its
projection inside (tests/decode_restatement.py) against torch's own layer_norm / linear / scaled_dot_product_attention in float64,
its whole decoder pass against one `engine.decode_step` over `RefOps(lowp=float64)`, the census against its closed forms, and the
table of the kernel instantiations the cases reach.

Bounds: two float64 evaluations of the same expression in different orders -- 1e-12 relative to the row for the single operation.
The engine over `RefOps(lowp=float64)` keeps every tensor in float64 and rounds nothing to bf16, but RefOps forms its products and
LayerNorm statistics in fp32 (`.float()`): unit roundoff 6e-8 per operation, sums of up to 384 terms, some twenty operations deep
over two layers and the LM head -- 1e-5 of a row's norm asked (3e-7 seen), a hundred times below one bf16 rounding (2e-3).
`RefOps` in bf16 rounds the normalised row, q / k / v, P and o: row_err up to ~1e-2 at these sizes (5e-2 asked, as in test_attention_edges.py: one wrong row has row_err of order 1)."""
import pytest
import torch
import torch.nn.functional as F

import decode_restatement as dr
from oracle.ref_ops import RefOps

SMALL = [(384, 0, torch.float32, 9, 3, True), (384, 1, torch.bfloat16, 9, 3, True), (512, 1, torch.float32, 1, 1, False),
         (768, 0, torch.bfloat16, 65, 1, False), (1280, 1, torch.float32, 65, 3, True), (1024, 0, torch.float32, 2, 3, False)]


def _call(fn, mode, D, B, Lk, x, kv, kv_rows, params=None):
    ln_g, ln_b, w, bias = dr.sweep_params(D) if params is None else params
    if mode == 0 and params is None:
        w, bias = w[:D], bias[:D]
    return fn(mode, x, ln_g, ln_b, w, bias, kv[:, :D], kv[:, D:2 * D], B, D // 64, Lk, kv_rows=kv_rows)


@pytest.mark.parametrize("D,mode,dt,Lk,B,padded", SMALL)
def test_statement_against_torch_functional_in_float64(D, mode, dt, Lk, B, padded):
    H = D // 64
    x, kv, kv_rows = dr.sweep_case_inputs(D, mode, dt, Lk, B, padded)
    o, kn, vn = _call(dr.decode_attn_proj, mode, D, B, Lk, x, kv, kv_rows)
    ln_g, ln_b, w, bias = (t.double() for t in dr.sweep_params(D))
    ln = F.layer_norm(x.double(), (D,), ln_g, ln_b, dr.EPS)
    proj = F.linear(ln, w if mode == 1 else w[:D], bias if mode == 1 else bias[:D])
    nold = Lk - mode
    kv3 = kv.double().reshape(B, kv_rows, -1)[:, :nold, :2 * D]
    k3, v3 = kv3[..., :D], kv3[..., D:]
    if mode == 1:
        k3, v3 = torch.cat([k3, proj[:, None, D:2 * D]], 1), torch.cat([v3, proj[:, None, 2 * D:]], 1)
        assert dr.row_err(kn, proj[:, D:2 * D], H) <= 1e-12 and dr.row_err(vn, proj[:, 2 * D:], H) <= 1e-12
    heads = lambda t, L: t.reshape(B, L, H, 64).transpose(1, 2)
    want = F.scaled_dot_product_attention(heads(proj[:, :D], 1), heads(k3, Lk), heads(v3, Lk), scale=dr.SCALE)
    assert torch.isfinite(o).all()
    assert dr.row_err(o, want.transpose(1, 2).reshape(B, D), H) <= 1e-12


@pytest.mark.parametrize("D,mode,dt,Lk,B,padded", SMALL)
def test_ref_ops_composition_agrees_with_float64_per_row(D, mode, dt, Lk, B, padded):
    H = D // 64
    x, kv, kv_rows = dr.sweep_case_inputs(D, mode, dt, Lk, B, padded)
    got = _call(lambda *a, **k: dr.composed(RefOps("cpu"), *a, **k), mode, D, B, Lk, x, kv, kv_rows)
    want = _call(dr.decode_attn_proj, mode, D, B, Lk, x, kv, kv_rows)
    for name, a, b in zip(("o", "k_new", "v_new"), got, want):
        if b is None:
            assert a is None
            continue
        assert a.dtype == torch.bfloat16 and torch.isfinite(a.float()).all()
        assert dr.row_err(a, b, H) <= 5e-2, name


def test_a_dropped_key_and_a_dropped_column_show_in_row_err():
    """What a 0.06-sigma bound on the top logits lets through: one key of 65 left out moves a row by more than the bf16 yardstick."""
    D, Lk, B = 384, 65, 3
    x, kv, kv_rows = dr.sweep_case_inputs(D, 0, torch.float32, Lk, B, False)
    o, _, _ = _call(dr.decode_attn_proj, 0, D, B, Lk, x, kv, kv_rows)
    less, _, _ = _call(dr.decode_attn_proj, 0, D, B, Lk - 1, x, kv, kv_rows)
    ref, _, _ = _call(lambda *a, **k: dr.composed(RefOps("cpu"), *a, **k), 0, D, B, Lk, x, kv, kv_rows)
    assert dr.row_err(less, o, D // 64) > 4 * dr.row_err(ref, o, D // 64)


# ---- the whole pass ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,t", [(1, 0), (3, 5)])
def test_whole_pass_against_the_engine_over_float64_ref_ops(B, t):
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import ParamStore, WhisperDims, WhisperEngine
    dims = WhisperDims(384, 6, dr.PASS_FFN, 1, 2, dr.PASS_VOCAB, 8, max_src=dr.PASS_SRC)
    sd = {k: v.to(torch.bfloat16).float() for k, v in si.random_state_dict(dims, 11).items()}
    ref = RefOps("cpu", lowp=torch.float64)
    eng = WhisperEngine(ref, ParamStore(ref, dims, sd, trainable=False), torch.float64)
    g = torch.Generator().manual_seed(20 + t)
    D, ML = dims.d_model, dr.PASS_MAX_LEN
    enc = (0.5 * torch.randn(B * dims.max_src, D, generator=g)).bfloat16()
    ids = torch.randint(0, dims.vocab, (B, 1), generator=g)
    base = [(0.5 * torch.randn(B * ML, 2 * D, generator=g)).bfloat16().double() for _ in range(dims.dec_layers)]
    cache = eng.decode_init(enc.double(), B, ML)
    for kv, b0 in zip(cache["self"], base):
        kv.copy_(b0)
    cache["t"] = t
    logits = eng.decode_step(ids, cache)[:, :dims.vocab]
    want, rows = dr.decode_pass(sd, dims, ids, t, base, dr.cross_kv(sd, dims, enc, B))
    assert (logits - want).norm(dim=-1).max().item() <= 1e-5 * want.norm(dim=-1).min().item()
    for kv, b0, r in zip(cache["self"], base, rows):
        kv3, b3 = kv.view(B, ML, 2 * D), b0.view(B, ML, 2 * D)
        assert dr.row_err(kv3[:, t], r, 2 * dims.heads) <= 1e-5
        keep = torch.arange(ML) != t
        assert torch.equal(kv3[:, keep], b3[:, keep])


# ---- census --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("Lk", dr.CENSUS_LK)
def test_census_closed_form_against_the_enumerated_keys(Lk):
    for H in (1, 6, 20):
        assert torch.equal(dr.census_counts(Lk, H), dr.census_onehot(torch.arange(Lk), H).sum(0).long())
    assert int(dr.census_counts(Lk, 6)[:64].sum()) == Lk and int(dr.census_counts(Lk, 6)[64:128].sum()) == Lk


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("Lk", [1, 2, 9, 65, 129, 513])
def test_census_inputs_give_counts_over_lk_in_float64(mode, Lk):
    D, B = 384, 3
    c = dr.census_inputs(mode, D, B, Lk, padded=True)
    o, kn, vn = dr.decode_attn_proj(mode, c["x"], c["ln_g"], c["ln_b"], c["w"], c["bias"], c["kv"][:, :D], c["kv"][:, D:2 * D], B, 6, Lk,
                                    kv_rows=c["kv_rows"])
    want = dr.census_counts(Lk, 6).double() / Lk
    assert (o - want).abs().max().item() <= 1e-14
    assert torch.equal(dr.census_expect(Lk, 6), want.float().bfloat16())
    if mode == 1:
        assert not kn.any() and torch.equal(vn[1], dr.census_onehot([Lk - 1], 6)[0].double())
    # everything the operation must not read is loud
    kv3 = c["kv"].view(B, c["kv_rows"], -1)
    assert bool((kv3[:, Lk - mode:] == dr.CENSUS_PAD).all()) and bool((kv3[:, :, 2 * D:] == dr.CENSUS_PAD).all())
    assert kv3.shape[2] == 2 * D + dr.PITCH_PAD and c["kv_rows"] >= Lk + 1


def test_p_rounding_case_separates_rounded_from_unrounded_p():
    rounded, plain = dr.p_rounding_expect()
    c = dr.p_rounding_inputs(384)
    o, _, _ = dr.decode_attn_proj(0, c["x"], c["ln_g"], c["ln_b"], c["w"], c["bias"], c["kv"][:, :384], c["kv"][:, 384:], 1, 6, 2)
    assert abs(o[0, 0].item() - plain) <= 1e-15                     # the statement rounds nothing
    assert abs(rounded - plain) > 0.25 * abs(plain)                 # a bf16 ulp of o is 2^-8 relative: these are far apart
    assert not o[0, 1:].any()


# ---- which instantiation a case reaches ---------------------------------------------------------------------------------------------
def test_instantiation_table():
    assert len(dr.INSTANTIATIONS) == 20
    assert dr.instantiation(0, torch.float32, 1280) == (0, False, 20) and dr.instantiation(1, torch.bfloat16, 384) == (1, True, 6)
    for bad in ((2, torch.float32, 384), (0, torch.float16, 384), (0, torch.float32, 128), (1, torch.float32, 640), (0, torch.float32, 1344)):
        assert dr.instantiation(*bad) is None
    cases = dr.sweep_cases()
    assert {dr.instantiation(m, dt, D) for D, m, dt, *_ in cases} == dr.INSTANTIATIONS
    for inst in dr.INSTANTIATIONS:                                   # every instantiation meets every key count, batch and pitch
        mine = [(Lk, B, p) for D, m, dt, Lk, B, p, s in cases if dr.instantiation(m, dt, D) == inst and not s]
        assert sorted(mine) == sorted((Lk, B, p) for Lk in dr.SWEEP_LK for B in dr.SWEEP_B for p in (False, True))
    assert all(Lk <= dr.MAX_KEYS for Lk in dr.CENSUS_LK) and dr.MAX_KEYS in dr.CENSUS_LK and dr.MAX_KEYS - 1 in dr.CENSUS_LK


def test_whole_pass_table_reaches_every_instantiation():
    """Under key 7 = 0 a token step runs MODE 1 and MODE 0, under 4 (the default) MODE 0 alone, under 8 MODE 1 alone, under 12 neither;
    the rows pass never runs MODE 1."""
    seen = set()
    for D in dr.WIDTHS:
        for key in dr.PASS_KEYS:
            for B, t in dr.PASS_BT:
                fs, fc = dr.pass_launches(D, key, B, t)
                assert (fs, fc) == (key in (0, 8), key in (0, 4))
                for dt in (torch.float32, torch.bfloat16):
                    seen |= {dr.instantiation(1, dt, D)} if fs else set()
                    seen |= {dr.instantiation(0, dt, D)} if fc else set()
    assert seen == dr.INSTANTIATIONS
    assert dr.pass_launches(384, 4, 3, 5, rows_pass=True) == (False, True) and dr.pass_launches(384, 0, 3, 5, rows_pass=True) == (False, True)
    assert dr.pass_launches(128, 0, 1, 0) == (False, False)         # the width of the decoding fixtures: never the kernel
    assert all(B * 1 > lim for (B, _), lim in zip(dr.PASS_BT_384, (32, 64)))
