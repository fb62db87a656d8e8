"""The token step's attention with its projection inside (`attn_decode_proj_kernel`, csrc/decode.hip: LayerNorm, the q -- in MODE 1
the q / k / v -- projection of one head, the cache append and single-query attention in one workgroup), launched alone through
dw_decode_attn_proj, the function decode_pass dispatches it with, and judged per (row, head) vector against a float64 statement
that shares none of its rounding points (tests/decode_restatement.py; its helpers are checked on the CPU by tests/test_decode_edges.py).
All twenty instantiations: MODE 0 / 1, f32 / bf16 residual stream, d_model 384 / 512 / 768 / 1024 / 1280.

* Census (exact): zero gamma and zero weights leave q / k / v equal to their biases, cached K = 0 makes the scores equal, one-hot V
  rows indexed by key turn o into bf16(count / Lk) bit for bit -- WHICH keys entered the sum, over the 8-key group of a lane
  octet, the 64-key wave sweep, the 512-key outer sweep and the 8192-key limit, with the new key of MODE 1 served from LDS at every
  one of those positions (t = 0 included: no key in memory).  Everything the kernel must not read holds 1e4.
* P is rounded to bf16 in front of the PV product: a two-key case whose output is the rounding of P and nothing else.
* Boundary sweep: random inputs, every output and the cache behind NaN guards.  Bound per tensor:
  row_err(kernel, float64) <= F * e_ref with e_ref = row_err(RefOps, float64), the same operation composed from RefOps.layernorm_fwd,
  gemm and attn_fwd on the same inputs (they round where the kernel rounds: the normalised row, q / k / v, P and o); F covers the
  fp32-level differences (summation order, hardware exp2).  A case whose e_ref is exactly zero (one key in MODE 0: o is that key's
  value row) must be exact.
  Measured on the MI355X, largest row_err(kernel) / e_ref over all cases:
    o      1.57  (D 1280, MODE 1, bf16 stream, 65 keys, B 3: 8.53e-3 against 5.43e-3; next 1.52 at D 384, MODE 1, 2 keys, B 1 and
                 1.42 at D 512, MODE 1, 9 keys, B 1 -- a q, k or v element that rounds the other way after another order of the
                 fp32 sum, seen through a softmax over few keys)
    k_new  1.04  (D 1280, MODE 1, bf16 stream, 1 key, B 1, padded pitch)
    v_new  1.02  (D 768, MODE 1, f32 stream, 513 keys, B 3, padded pitch)
  F = the smallest of 2, 3, 4 that is at least 1.5 x the ratio: o 3, k_new 2, v_new 2.  No case needed a floor of its own: the 40
  cases whose e_ref is zero (MODE 0, one key) are exact in the kernel too.
* Invariances (bit-exact): one x row replicated over the batch; a padded K/V pitch against the dense one.
* Argument checks: every refusal of include/dwamd.h returns its code and leaves the outputs' sentinel fill alone.
* Whole pass: engine.decode_step (dw_decode_step) on two-layer decoders of the five widths under dw_debug_set key 7 = 0 / 4 / 8 / 12
  (MODE 1 and MODE 0, MODE 0 alone -- the default --, MODE 1 alone, neither), both stream dtypes, t = 0, mid-cache and the last
  cache row, batches past the rows <= 32 / <= 64 fusion switches, and one dw_decode_step_rows pass with n = 1 (the rows pass with
  the fused cross-attention).  Logits rows and the last layer's appended cache rows, as whole-row vectors:
  vec_err(kernels, float64 engine) <= F * vec_err(the same engine over RefOps in bf16, float64 engine).
  Measured on the MI355X:
    logits 1.08  (D 1280, f32 stream, B 3, t 5, the same under every value of the key)
    cache  1.07  (the rows pass, D 384, bf16 stream, row_t 5 / 0 / 23)
  F = 2 for both.  The four values of the key gave the same figures to four digits in every case: what the fused kernel's other
  order of the fp32 sums moves is below what the bf16 stores keep (that the key does switch the kernel in is shown by the
  mutations below: the whole pass fails under each of them that is not a rounding matter).
* Mutations of the kernel (each in bounds, each on a scratch copy, run against this module on the MI355X):
    the new key weighted from the clamped old row instead of knew / vnew  -> census (MODE 1), sweep (MODE 1), whole pass
    lsum summed over all eight lanes of a key                             -> census, sweep, P rounding, whole pass, rows pass
    the v bias read at the k offset                                       -> census (MODE 1: row t and o), sweep (MODE 1), whole pass
    `has` one thread short in the LayerNorm                               -> sweep (all twenty), both invariances, whole pass
    P left unrounded                                                      -> test_p_is_rounded_to_bf16_in_front_of_the_pv_product alone
  (the last one makes the kernel more accurate, so no bound against float64 can see it: the two-key case exists for it).
"""
import contextlib

import pytest
import torch

import decode_restatement as dr
from attention_restatement import NAN16
from guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F_BOUND = {"o": 3.0, "k_new": 2.0, "v_new": 2.0}            # see the module docstring
F_PASS = {"logits": 2.0, "cache": 2.0}                    # see the module docstring
EINVAL, EUNSUP = -1, -2
KEY7_DEFAULT = 4


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps(DEV)


@pytest.fixture(scope="module")
def ref():
    from oracle.ref_ops import RefOps
    return RefOps(DEV)


@contextlib.contextmanager
def key7(ops, value):
    try:
        assert ops.lib.dw_debug_set(7, value) == 0
        yield
    finally:
        ops.lib.dw_debug_set(7, KEY7_DEFAULT)


def bits(t):
    return t.view(torch.int16)


def run(ops, mode, D, B, Lk, x, ln_g, ln_b, w, bias, kv, kv_rows):
    """One launch through dw_decode_attn_proj with o behind NaN guards and the cache compared bit for bit around the one row it may
    write -> o [B, D], k_new, v_new [B, D] (the halves of cache row t; None in mode 0)."""
    H = D // 64
    o = Guarded(B, D, pad=8)
    before = kv.clone()
    ops.decode_attn_proj(mode, x, ln_g, ln_b, w, bias, kv[:, :D], kv[:, D:2 * D], B, H, Lk, kv_rows=kv_rows,
                         kv_app=kv if mode == 1 else None, out=o.live)
    torch.cuda.synchronize()
    assert o.intact(), "wrote outside o"
    assert torch.isfinite(o.live.float()).all(), "non-finite o"
    if mode == 0:
        assert torch.equal(bits(kv), bits(before)), "mode 0 wrote to the keys / values"
        return o.live, None, None
    t = Lk - 1
    a3, b3 = bits(kv).view(B, kv_rows, -1).clone(), bits(before).view(B, kv_rows, -1).clone()
    row = kv.view(B, kv_rows, -1)[:, t, :2 * D].clone()
    a3[:, t, :2 * D] = 0
    b3[:, t, :2 * D] = 0
    assert torch.equal(a3, b3), "a cache element outside row t changed"
    assert torch.isfinite(row.float()).all() and not bool((bits(row) == NAN16).any()), "row t is not fully written"
    return o.live, row[:, :D], row[:, D:]


# ---- census ----------------------------------------------------------------------------------------------------------------------
def census(ops, mode, D, B, Lk, dt):
    H = D // 64
    c = dr.census_inputs(mode, D, B, Lk, True, dt, DEV)
    o, kn, vn = run(ops, mode, D, B, Lk, c["x"], c["ln_g"], c["ln_b"], c["w"], c["bias"], c["kv"], c["kv_rows"])
    want = dr.census_expect(Lk, H).to(DEV)
    for b in range(B):
        if not torch.equal(o[b], want):
            col = int((o[b] != want).nonzero()[0])
            raise AssertionError(f"mode {mode} D {D} B {B} Lk {Lk} batch {b}: o * Lk = {o[b, col].item() * Lk:g} at head {col // 64} column "
                                 f"{col % 64}, {int(dr.census_counts(Lk, H)[col])} keys have their 1 there")
    if mode == 1:
        assert not bool(kn.any()), "row t, K half: the k bias is zero"
        assert torch.equal(vn, dr.census_onehot([Lk - 1], H).bfloat16().to(DEV).expand(B, -1)), "row t, V half: the v bias"


@pytest.mark.parametrize("B,dt", [(1, torch.float32), (3, torch.bfloat16)])
@pytest.mark.parametrize("mode", [0, 1])
def test_census_384(ops, mode, B, dt):
    for Lk in dr.CENSUS_LK:
        census(ops, mode, 384, B, Lk, dt)


@pytest.mark.parametrize("B,dt", [(1, torch.bfloat16), (3, torch.float32)])
@pytest.mark.parametrize("mode", [0, 1])
def test_census_1280_largest_lds_footprint(ops, mode, B, dt):
    D, lks = dr.CENSUS_WIDE
    for Lk in lks:
        census(ops, mode, D, B, Lk, dt)


@pytest.mark.parametrize("mode", [0, 1])
def test_census_8193_keys_are_unsupported_and_nothing_is_written(ops, mode):
    D, B, Lk = 384, 1, dr.MAX_KEYS + 1
    c = dr.census_inputs(mode, D, B, Lk, True, torch.float32, DEV)
    o, before = Guarded(B, D, pad=8), c["kv"].clone()
    with pytest.raises(RuntimeError, match="code -2"):
        ops.decode_attn_proj(mode, c["x"], c["ln_g"], c["ln_b"], c["w"], c["bias"], c["kv"][:, :D], c["kv"][:, D:2 * D], B, 6, Lk,
                             kv_rows=c["kv_rows"], kv_app=c["kv"] if mode == 1 else None, out=o.live)
    torch.cuda.synchronize()
    assert o.untouched() and torch.equal(bits(c["kv"]), bits(before))


def test_p_is_rounded_to_bf16_in_front_of_the_pv_product(ops):
    """o = (1 - bf16(P)) / (1 + P) where P left unrounded gives (1 - P) / (1 + P), 40 % away.  Asked: within two bf16 ulps (2^-7
    relative: one for the stored o, and the hardware exp2's last fp32 bits move 1 - bf16(P) by nothing and 1 + P by 1e-7)."""
    rounded, plain = dr.p_rounding_expect()
    for D in (384, 1280):
        c = dr.p_rounding_inputs(D, DEV)
        o, _, _ = run(ops, 0, D, 1, 2, c["x"], c["ln_g"], c["ln_b"], c["w"], c["bias"], c["kv"], c["kv_rows"])
        got = o[0, 0].item()
        print(f"DEC_EDGE p-rounding D {D}: o {got:.6e}, with bf16(P) {rounded:.6e}, with P {plain:.6e}")
        assert abs(got - rounded) <= 2.0 ** -7 * abs(rounded), (got, rounded, plain)
        assert not bool(o[0, 1:].any())


# ---- boundary sweep against float64 ----------------------------------------------------------------------------------------------
def case_name(D, mode, dt, Lk, B, padded, spiked):
    return f"D{D} mode{mode} {'bf16' if dt == torch.bfloat16 else 'f32'} Lk{Lk} B{B}{' padded' if padded else ''}{' spiked' if spiked else ''}"


def judge(name, case, x, x_ref, x64, H):
    assert torch.isfinite(x.float()).all(), f"{case} {name}: non-finite values"
    e, e_ref = dr.row_err(x, x64, H), dr.row_err(x_ref, x64, H)
    print(f"DEC_EDGE {case} {name} kernel {e:.4e} ref {e_ref:.4e} ratio {e / e_ref if e_ref else float('nan'):.3f}")
    if e_ref == 0.0:
        assert e == 0.0, f"{case} {name}: row_err {e:.3e} where RefOps is exact"
    else:
        assert e <= F_BOUND[name] * e_ref, f"{case} {name}: row_err {e:.3e} > {F_BOUND[name]:g} x {e_ref:.3e}"


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", dr.WIDTHS)
def test_sweep_per_row_against_float64(ops, ref, D, mode, dt):
    H = D // 64
    ln_g, ln_b, w, bias = dr.sweep_params(D, DEV)
    if mode == 0:
        w, bias = w[:D], bias[:D]
    mine = [c for c in dr.sweep_cases() if c[:3] == (D, mode, dt)]
    assert len(mine) >= len(dr.SWEEP_LK) * 4
    for _, _, _, Lk, B, padded, spiked in mine:
        case = case_name(D, mode, dt, Lk, B, padded, spiked)
        x, kv, kv_rows = dr.sweep_case_inputs(D, mode, dt, Lk, B, padded, spiked, DEV)
        k, v = kv[:, :D], kv[:, D:2 * D]
        want = dr.decode_attn_proj(mode, x, ln_g, ln_b, w, bias, k, v, B, H, Lk, kv_rows=kv_rows)
        comp = dr.composed(ref, mode, x, ln_g, ln_b, w, bias, k, v, B, H, Lk, kv_rows=kv_rows)
        got = run(ops, mode, D, B, Lk, x, ln_g, ln_b, w, bias, kv, kv_rows)
        for name, a, r, a64 in zip(("o", "k_new", "v_new"), got, comp, want):
            if a64 is not None:
                judge(name, case, a, r, a64, H)


# ---- invariances -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", dr.WIDTHS)
def test_replicated_row_gives_identical_outputs_for_every_batch_entry(ops, D, mode):
    B = 3
    ln_g, ln_b, w, bias = dr.sweep_params(D, DEV)
    if mode == 0:
        w, bias = w[:D], bias[:D]
    for Lk, dt in ((1, torch.float32), (65, torch.bfloat16), (513, torch.float32)):
        x, kv, kv_rows = dr.sweep_case_inputs(D, mode, dt, Lk, B, True, False, DEV)
        x = x[:1].expand(B, -1).contiguous()
        kv3 = kv.view(B, kv_rows, -1)
        kv3[1:] = kv3[:1]
        o, kn, vn = run(ops, mode, D, B, Lk, x, ln_g, ln_b, w, bias, kv, kv_rows)
        for t in (o, kn, vn):
            if t is not None:
                assert torch.equal(bits(t[1:].contiguous()), bits(t[:1].expand(B - 1, -1).contiguous())), (Lk, mode)


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("D", dr.WIDTHS)
def test_padded_pitch_gives_the_bits_of_the_dense_one(ops, D, mode):
    B = 3
    ln_g, ln_b, w, bias = dr.sweep_params(D, DEV)
    if mode == 0:
        w, bias = w[:D], bias[:D]
    for Lk, dt in ((2, torch.bfloat16), (65, torch.float32), (1500, torch.bfloat16)):
        x, dense, kv_rows = dr.sweep_case_inputs(D, mode, dt, Lk, B, False, False, DEV)
        padded = torch.full((B * kv_rows, 2 * D + dr.PITCH_PAD), float("nan"), dtype=torch.bfloat16, device=DEV)
        padded[:, :2 * D] = dense
        a = run(ops, mode, D, B, Lk, x, ln_g, ln_b, w, bias, dense, kv_rows)
        b = run(ops, mode, D, B, Lk, x, ln_g, ln_b, w, bias, padded, kv_rows)
        for u, v in zip(a, b):
            if u is not None:
                assert torch.equal(bits(u.contiguous()), bits(v.contiguous())), (Lk, mode)


# ---- argument checks -------------------------------------------------------------------------------------------------------------
def test_every_refusal_returns_its_code_and_writes_nothing(ops):
    from distil_whisper_amd.ops_hip import DW_BF16, DW_F32
    D, H, B, Lk, kv_rows = 384, 6, 2, 9, 12
    ln_g, ln_b, w, bias = dr.sweep_params(D, DEV)
    x = torch.randn(B, D + 8, device=DEV)
    pitch = 2 * D + 16
    kv = torch.randn(B * kv_rows, pitch, device=DEV).bfloat16()
    o, before = Guarded(B, D, pad=8), None
    good = dict(mode=1, x=x.data_ptr(), x_dtype=DW_F32, ldx=D + 8, ln_g=ln_g.data_ptr(), ln_b=ln_b.data_ptr(), eps=1e-5, w=w.data_ptr(),
                bias=bias.data_ptr(), k=kv.data_ptr(), v=kv.data_ptr() + 2 * D, ldkv=pitch, kv_rows=kv_rows, kv_app=kv.data_ptr(),
                o=o.live.data_ptr(), ldo=o.live.stride(0), B=B, H=H, Lk=Lk, scale=0.125)

    def call(**over):
        a = dict(good, **over)
        return ops.lib.dw_decode_attn_proj(a["mode"], a["x"], a["x_dtype"], a["ldx"], a["ln_g"], a["ln_b"], a["eps"], a["w"], a["bias"], a["k"],
                                           a["v"], a["ldkv"], a["kv_rows"], a["kv_app"], a["o"], a["ldo"], a["B"], a["H"], a["Lk"],
                                           a["scale"], ops._stream())

    bad = [(EINVAL, dict(mode=2)), (EINVAL, dict(mode=-1)), (EINVAL, dict(x_dtype=2)), (EINVAL, dict(x_dtype=-1))]
    bad += [(EINVAL, {n: None}) for n in ("x", "ln_g", "ln_b", "w", "bias", "k", "v", "o", "kv_app")]          # null pointers
    bad += [(EINVAL, dict(Lk=0)), (EINVAL, dict(Lk=-3)), (EINVAL, dict(Lk=kv_rows + 1)), (EINVAL, dict(B=0)), (EINVAL, dict(H=0))]
    bad += [(EINVAL, {n: good[n] + 8}) for n in ("x", "w", "k", "v", "ln_g", "ln_b")]                           # 8-byte aligned only
    bad += [(EINVAL, dict(x=good["x"] + 4)), (EINVAL, dict(ln_g=good["ln_g"] + 4)), (EINVAL, dict(k=good["k"] + 2))]
    bad += [(EINVAL, dict(ldx=D + 4)), (EINVAL, dict(ldkv=pitch + 4)), (EINVAL, dict(ldkv=pitch - 2))]         # pitches not multiples of 8
    bad += [(EINVAL, dict(mode=0, x_dtype=DW_BF16, ldx=D + 4))]
    bad += [(EINVAL, dict(ldx=D - 8)), (EINVAL, dict(ldo=D - 8)), (EINVAL, dict(ldkv=2 * D - 8)), (EINVAL, dict(mode=0, ldkv=D - 8))]
    bad += [(EUNSUP, dict(H=h)) for h in (1, 2, 5, 7, 10, 14, 18, 21, 65535)]                                # D outside the five classes
    bad += [(EUNSUP, dict(Lk=dr.MAX_KEYS + 1, kv_rows=dr.MAX_KEYS + 8)), (EUNSUP, dict(B=65536)), (EUNSUP, dict(H=65536))]
    before = kv.clone()
    for want, over in bad:
        assert call(**over) == want, over
    torch.cuda.synchronize()
    assert o.untouched() and torch.equal(bits(kv), bits(before))
    assert call() == 0                                           # the valid call of the same arguments runs
    torch.cuda.synchronize()
    assert o.intact() and torch.isfinite(o.live.float()).all() and not torch.equal(bits(kv), bits(before))
    want, kn, vn = dr.decode_attn_proj(1, x[:, :D], ln_g, ln_b, w, bias, before[:, :D], before[:, D:2 * D], B, H, Lk, kv_rows=kv_rows)
    assert dr.row_err(o.live, want, H) <= 2e-2


# ---- whole pass ------------------------------------------------------------------------------------------------------------------
def _engines(ops, D, seed):
    """Two-layer decoders of width D over the same bf16-rounded weights: the kernels and RefOps in bf16 per stream dtype, and the
    float64 engine (as _pair_of_engines of test_assist_rows_gpu.py builds them)."""
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import ParamStore, WhisperDims, WhisperEngine
    from oracle.ref_ops import RefOps
    dims = WhisperDims(D, D // 64, dr.PASS_FFN, 1, 2, dr.PASS_VOCAB, 8, max_src=dr.PASS_SRC)
    sd = {k: v.to(torch.bfloat16).float() for k, v in si.random_state_dict(dims, seed, ops.device).items() if k.startswith("model.decoder.")}
    rb, r64 = RefOps(DEV), RefOps(DEV, lowp=torch.float64)

    def eng(o, stream):
        return WhisperEngine(o, ParamStore(o, dims, sd, trainable=False, decoder_only=True), stream)

    return dims, {dt: (eng(ops, dt), eng(rb, dt)) for dt in (torch.float32, torch.bfloat16)}, eng(r64, torch.float64)


def _pass_inputs(dims, B, seed):
    g = torch.Generator().manual_seed(seed)
    D = dims.d_model
    enc = (0.5 * torch.randn(B * dims.max_src, D, generator=g)).to(DEV).bfloat16()
    ids = torch.randint(0, dims.vocab, (B, 1), generator=g).to(DEV)
    base = [(0.5 * torch.randn(B * dr.PASS_MAX_LEN, 2 * D, generator=g)).to(DEV).bfloat16() for _ in range(dims.dec_layers)]
    return enc, ids, base


def _step(eng, enc, ids, base, B, t, row_t=None):
    """-> logits [B, vocab], the last layer's cache rows written [B, 2D], float64 copies; every other cache row must keep its bits."""
    d, ML = eng.dims, dr.PASS_MAX_LEN
    dt = torch.float64 if eng.lowp == torch.float64 else torch.bfloat16
    cache = eng.decode_init(enc.to(dt), B, ML)
    for kv, b0 in zip(cache["self"], base):
        kv.copy_(b0.to(dt))
    if row_t is None:
        cache["t"] = t
        logits = eng.decode_step(ids, cache)
        rows = torch.full((B,), t, device=DEV)
    else:
        rt = torch.tensor(row_t, dtype=torch.int32, device=DEV)
        logits = eng.decode_multi_rows(ids, cache, rt, max(row_t))
        rows = rt.long()
    logits = logits[:, :d.vocab].double().clone()
    torch.cuda.synchronize()
    r = torch.arange(B, device=DEV)
    for kv, b0 in zip(cache["self"], base):
        kv3, b3 = kv.view(B, ML, -1).clone(), b0.to(dt).view(B, ML, -1).clone()
        kv3[r, rows], b3[r, rows] = 0, 0
        assert torch.equal(kv3, b3), "a cache row other than the appended one changed"
    return logits, cache["self"][-1].view(B, ML, -1)[r, rows].double().clone()


def _judge_pass(case, got, comp, want):
    for name, a, r, a64 in zip(("logits", "cache"), got, comp, want):
        assert torch.isfinite(a).all(), f"{case} {name}"
        e, e_ref = dr.vec_err(a, a64), dr.vec_err(r, a64)
        print(f"DEC_PASS {case} {name} kernels {e:.4e} ref {e_ref:.4e} ratio {e / e_ref:.3f}")
        assert e_ref > 0 and e <= F_PASS[name] * e_ref, f"{case} {name}: {e:.3e} > {F_PASS[name]:g} x {e_ref:.3e}"


@pytest.mark.parametrize("D", dr.WIDTHS)
def test_whole_pass_under_every_fusion_key(ops, D):
    dims, engs, eng64 = _engines(ops, D, 30 + D)
    cases = list(dr.PASS_BT) + (list(dr.PASS_BT_384) if D == 384 else [])
    for dt, (hip, rb) in engs.items():
        for B, t in cases:
            enc, ids, base = _pass_inputs(dims, B, 1000 * B + t + D)
            want = _step(eng64, enc, ids, base, B, t)
            comp = _step(rb, enc, ids, base, B, t)
            for key in dr.PASS_KEYS:
                with key7(ops, key):
                    got = _step(hip, enc, ids, base, B, t)
                _judge_pass(f"D{D} {'f32' if dt == torch.float32 else 'bf16'} B{B} t{t} key{key}", got, comp, want)


def test_rows_pass_with_one_new_token_runs_the_fused_cross_attention(ops):
    """dw_decode_step_rows, n = 1, width 384, the default key: its cross-attention is attn_decode_proj_kernel<0, ., 6>."""
    D, B, row_t = 384, 3, [5, 0, dr.PASS_MAX_LEN - 1]
    assert dr.pass_launches(D, KEY7_DEFAULT, B, max(row_t), rows_pass=True) == (False, True)
    dims, engs, eng64 = _engines(ops, D, 77)
    enc, ids, base = _pass_inputs(dims, B, 4242)
    want = _step(eng64, enc, ids, base, B, None, row_t)
    for dt, (hip, rb) in engs.items():
        comp = _step(rb, enc, ids, base, B, None, row_t)
        got = _step(hip, enc, ids, base, B, None, row_t)
        _judge_pass(f"rows pass D{D} {'f32' if dt == torch.float32 else 'bf16'} row_t {row_t}", got, comp, want)
