"""FP8 cross-attention K/V on the MI355X (csrc/cross_kv8.hip; the format: include/dwamd.h "FP8 cross-attention K/V").

* Quantiser (`dw_cross_kv_quant`) against the numpy statement (tests/kv_quant_restatement.py): codes and scales bit for bit at
  src_len 1, 7, 15, 16, 17, 63, 64, 65, 1500; width 384 with 1 to 3 sequences and width 1280 with 2; dense and padded row pitch;
  seq0 > 0; the special columns of the CPU test in the first columns of K and of V; every byte outside the addressed sequences
  (the other sequences' codes and scales, guard bytes behind the buffers) keeps its canary.
* `dw_decode_attn_proj_kv8` against the float64 statement (tests/decode_restatement.py `decode_attn_proj`, mode 0) over the
  values s * float(code) of the same codes: same src_len and width matrix, bf16 and fp32 x.  Per row b, with
  dev(o, ref) = ||o[b] - ref[b]|| / ||ref[b]||:  dev(FP8 kernel, float64 over the codes) <= 1.25 x dev(today's bf16 kernel,
  float64 over the bf16 values) on the same problem -- the project's margin for a kernel that reorders fp32 sums.  The measured
  ratio is printed (KV8_ATTN lines).  With ONE key the bf16 kernel is exact (o is the value row) and the bound would be zero, while
  o = bf16(sV * float(code)) carries the one rounding of its store whatever the kernel does: there the test asks for that value
  bit for bit, which is the most any implementation of the format can give.
* q is the bf16 kernel's, bit for bit: two-key problems whose K / V are +-448 or 0 (scale exactly 1, codes exact), one probed
  pair of head dimensions per batch row, all fp32 sums of both kernels exact -- the two kernels' outputs must agree bit for bit
  (a projection summed in another order shows; one differing ulp of one element may not: see the test).
* Every refusal of the two entries: its code, nothing launched, canaries intact.
* Whole passes: `dw_decode_step` and `dw_decode_token_rows` at cross_kv_fmt = 1, widths 384 and 1280, 3 and 18 rows, against the
  per-kernel Python form over oracle.ref_ops in bf16 on the SAME FP8 cache, both judged against the float64 engine on that cache:
  vec_err(kernels) <= 2 x vec_err(per-kernel form), the tolerance tests/test_decode_edges_gpu.py states for key 7 = 4.
  cross_kv_fmt = 0 ignores the new fields bit for bit; the descriptor's refusals launch nothing.
* Graph replay equals eager on an FP8 cache (GreedyDecoder, SlotDecoder), and the token comparison of tests/test_cross_kv_fp8.py
  with the kernels on one side: delta and the margins still come from the two torch statements on the CPU.
"""
import numpy as np
import pytest
import torch

import decode_restatement as dr
import kv_quant_restatement as kr
from guarded import Guarded

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
EINVAL, EUNSUP = -1, -2
SRC_LENS = (1, 7, 15, 16, 17, 63, 64, 65, 1500)
RATIO = 1.25
F_PASS = 2.0
CANARY8, CANARY_S = 0xA5, -7.25


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps(DEV)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- quantiser ------------------------------------------------------------------------------------------------------------------
def quant_buffers(B, H, S, guard=256):
    """Canaried buffers of a layer: k8, v8 [B, H, S, 64] and scales [B, 2, 64 H] as views of flat buffers with `guard` extra elements."""
    n = B * H * S * 64
    flat = [torch.full((n + guard,), CANARY8, dtype=torch.uint8, device=DEV) for _ in range(2)]
    sflat = torch.full((B * 2 * 64 * H + guard,), CANARY_S, dtype=torch.float32, device=DEV)
    return flat, sflat, [f[:n].view(B, H, S, 64) for f in flat], sflat[:B * 2 * 64 * H].view(B, 2, 64 * H)


def quant_input(D, n_seq, S, pitch, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(n_seq, S, 2 * D, generator=g)
    x[:, :, 40] *= 30.0                                         # an outlier channel of K
    x[:, :, D + 70] *= 30.0                                     # and one of V
    for i in range(n_seq):
        sp = torch.from_numpy(kr.special_columns(S, seed=seed + i))
        x[i, :, :8] = sp
        x[i, :, D + 64:D + 72] = sp
    buf = torch.full((n_seq * S, pitch), float("nan"), dtype=torch.bfloat16)
    buf[:, :2 * D] = x.reshape(n_seq * S, 2 * D).bfloat16()
    return buf.to(DEV)


@pytest.mark.parametrize("S", SRC_LENS)
def test_quantiser_against_the_restatement(ops, S):
    for D, n_seq, seq0, pad in ((384, 1, 0, 0), (384, 2, 1, 64), (384, 3, 2, 8), (1280, 2, 1, 64)):
        H, B = D // 64, seq0 + n_seq + 1
        kv = quant_input(D, n_seq, S, 2 * D + pad, 100 * S + D + n_seq)
        flat, sflat, (k8, v8), sc = quant_buffers(B, H, S)
        ops.cross_kv_quant(kv, k8, v8, sc, seq0, n_seq, S, H)
        torch.cuda.synchronize()
        got_k, got_v, got_s = k8.cpu().numpy(), v8.cpu().numpy(), sc.cpu().numpy()
        x = kv[:, :2 * D].float().cpu().numpy().reshape(n_seq, S, 2 * D)
        for i in range(n_seq):
            for name, cols, got, row in (("K", slice(0, D), got_k, 0), ("V", slice(D, 2 * D), got_v, 1)):
                want_c, want_s = kr.quantize(x[i][:, cols])
                case = f"S{S} D{D} n_seq{n_seq} seq0{seq0} pad{pad} sequence {i} {name}"
                assert np.array_equal(got_s[seq0 + i, row].view(np.uint32), want_s.view(np.uint32)), f"{case}: scales"
                hm = kr.head_major(want_c, H)
                if not np.array_equal(got[seq0 + i], hm):
                    h, j, c = np.argwhere(got[seq0 + i] != hm)[0]
                    raise AssertionError(f"{case}: code {got[seq0 + i][h, j, c]:#x} for {x[i][j, cols][64 * h + c]!r} * 448 / amax, "
                                         f"want {hm[h, j, c]:#x} (head {h} row {j} column {c})")
        # everything outside the addressed sequences keeps its canary
        for f, view in zip(flat, (k8, v8)):
            keep = f.clone()
            keep[:view.numel()].view(B, H, S, 64)[seq0:seq0 + n_seq] = CANARY8
            assert bool((keep == CANARY8).all()), f"S{S} D{D}: codes written outside sequences [{seq0}, {seq0 + n_seq})"
        keep = sflat.clone()
        keep[:sc.numel()].view(B, 2, D)[seq0:seq0 + n_seq] = CANARY_S
        assert bool((keep == CANARY_S).all()), f"S{S} D{D}: scales written outside sequences [{seq0}, {seq0 + n_seq})"


def test_quantiser_refusals_write_nothing(ops):
    D, H, S, B = 384, 6, 9, 2
    kv = quant_input(D, B, S, 2 * D + 8, 5)
    flat, sflat, (k8, v8), sc = quant_buffers(B, H, S)
    good = dict(kv=kv.data_ptr(), ld=kv.stride(0), k8=k8.data_ptr(), v8=v8.data_ptr(), sc=sc.data_ptr(), seq0=0, n_seq=B, S=S, H=H)

    def call(**over):
        a = dict(good, **over)
        return ops.lib.dw_cross_kv_quant(a["kv"], a["ld"], a["k8"], a["v8"], a["sc"], a["seq0"], a["n_seq"], a["S"], a["H"], ops._stream())
    bad = [(EINVAL, {n: None}) for n in ("kv", "k8", "v8", "sc")]
    bad += [(EINVAL, dict(seq0=-1)), (EINVAL, dict(n_seq=0)), (EINVAL, dict(S=0)), (EINVAL, dict(H=0))]
    bad += [(EINVAL, dict(kv=good["kv"] + 8)), (EINVAL, dict(ld=good["ld"] + 4)), (EINVAL, dict(k8=good["k8"] + 4)),
            (EINVAL, dict(v8=good["v8"] + 1)), (EINVAL, dict(sc=good["sc"] + 2))]
    bad += [(EUNSUP, dict(n_seq=65536)), (EUNSUP, dict(H=16385)), (EINVAL, dict(ld=2 * D - 8))]
    for want, over in bad:
        assert call(**over) == want, over
    torch.cuda.synchronize()
    assert all(bool((f == CANARY8).all()) for f in flat) and bool((sflat == CANARY_S).all())
    assert call() == 0
    torch.cuda.synchronize()
    assert not bool((k8 == CANARY8).all()) and bool((sc != CANARY_S).all())


# ---- the attention kernel ---------------------------------------------------------------------------------------------------------
def quantised(ops, kv, B, H, Lk, kv_rows):
    """The first Lk rows of every sequence of kv [B * kv_rows, >= 2D] through the quantiser -> k8, v8, scales, and the values
    s * float(code) as float64 [B * Lk, D] each."""
    D = 64 * H
    live = kv.view(B, kv_rows, -1)[:, :Lk, :2 * D].reshape(B * Lk, 2 * D).contiguous()
    k8 = torch.empty(B, H, Lk, 64, dtype=torch.uint8, device=DEV)
    v8, sc = torch.empty_like(k8), torch.empty(B, 2, D, device=DEV)
    ops.cross_kv_quant(live, k8, v8, sc, 0, B, Lk, H)
    table = torch.from_numpy(kr.E4M3FN).to(DEV)

    def values(c8, s):
        return (table[c8.long()].permute(0, 2, 1, 3).reshape(B, Lk, D) * s.double()[:, None, :]).reshape(B * Lk, D)
    return k8, v8, sc, values(k8, sc[:, 0]), values(v8, sc[:, 1])


def dev_rows(o, ref):
    o, ref = o.double(), ref.double()
    return ((o - ref).norm(dim=-1) / ref.norm(dim=-1)).tolist()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Lk", SRC_LENS)
def test_attention_over_codes_against_float64(ops, Lk, dt):
    for D, B in ((384, 1), (384, 3), (1280, 2)):
        H = D // 64
        ln_g, ln_b, w, bias = dr.sweep_params(D, DEV)
        w, bias = w[:D], bias[:D]
        x, kv, kv_rows = dr.sweep_case_inputs(D, 0, dt, Lk, B, False, False, DEV)
        k8, v8, sc, kval, vval = quantised(ops, kv, B, H, Lk, kv_rows)
        o = Guarded(B, D, pad=8)
        ops.decode_attn_proj_kv8(x, ln_g, ln_b, w, bias, k8, v8, sc, B, H, Lk, out=o.live)
        torch.cuda.synchronize()
        assert o.intact() and torch.isfinite(o.live.float()).all()
        want8, _, _ = dr.decode_attn_proj(0, x, ln_g, ln_b, w, bias, kval, vval, B, H, Lk)
        case = f"D{D} B{B} Lk{Lk} {'f32' if dt == torch.float32 else 'bf16'}"
        if Lk == 1:
            exact = (sc[:, 1] * kr_decode_dev(v8).permute(0, 2, 1, 3).reshape(B, D)).bfloat16()
            assert torch.equal(bits(o.live), bits(exact)), f"{case}: one key, o is not bf16(sV * float(code))"
            print(f"KV8_ATTN {case} one key: exact")
            continue
        ob = ops.decode_attn_proj(0, x, ln_g, ln_b, w, bias, kv[:, :D], kv[:, D:2 * D], B, H, Lk, kv_rows=kv_rows)
        torch.cuda.synchronize()
        wantb, _, _ = dr.decode_attn_proj(0, x, ln_g, ln_b, w, bias, kv[:, :D], kv[:, D:2 * D], B, H, Lk, kv_rows=kv_rows)
        for b, (e8, eb) in enumerate(zip(dev_rows(o.live, want8), dev_rows(ob, wantb))):
            print(f"KV8_ATTN {case} row {b}: fp8 {e8:.4e} bf16 {eb:.4e} ratio {e8 / eb:.3f}")
            assert eb > 0 and e8 <= RATIO * eb, f"{case} row {b}: {e8:.3e} > {RATIO} x {eb:.3e}"


def kr_decode_dev(c8):
    return torch.from_numpy(kr.E4M3FN).to(DEV)[c8.long()].float()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["f32", "bf16"])
@pytest.mark.parametrize("D", [384, 1280])
def test_q_is_the_bf16_kernels_bit_for_bit(ops, D, dt):
    """Row b of 32 (one x row replicated) probes head dimensions 2b and 2b + 1 of every head: key 0 is 448 e_2b, key 1 is 448 e_2b+1,
    the values are +448 and -448 in every column.  Every column's largest magnitude is 448 or 0: scale exactly 1, codes exact.  A
    score is one product, the PV sum two products in different lanes: no fp32 sum of either kernel rounds differently, so with
    equal q elements o = 448 (bf16(P0) - bf16(P1)) / (P0 + P1) must agree bit for bit.  The converse holds only in the large: at scale
    2^-9 the two scores are about 1.3 q apart, a one-ulp step of one q element moves P by about 0.3 % |q| -- under a bf16 step for
    |q| < 1 -- and o is rounded once more, so a single differing ulp can pass; another order of the projection's sums, which moves
    many of the 64 x H probed elements, cannot."""
    H, B, Lk = D // 64, 32, 2
    ln_g, ln_b, w, bias = dr.sweep_params(D, DEV)
    w, bias = w[:D], bias[:D]
    x = dr.sweep_case_inputs(D, 0, dt, Lk, 1, False, False, DEV)[0].expand(B, -1).contiguous()
    kv = torch.zeros(B, Lk, 2 * D, device=DEV)
    for b in range(B):
        kv[b, 0, 2 * b:D:64] = 448.0
        kv[b, 1, 2 * b + 1:D:64] = 448.0
    kv[:, 0, D:] = 448.0
    kv[:, 1, D:] = -448.0
    kv = kv.reshape(B * Lk, 2 * D).bfloat16()
    k8, v8, sc, kval, vval = quantised(ops, kv, B, H, Lk, Lk)
    assert bool((sc == 1.0).all()) and torch.equal(kval, kv[:, :D].double()) and torch.equal(vval, kv[:, D:].double())
    scale = 2.0 ** -9
    o8 = ops.decode_attn_proj_kv8(x, ln_g, ln_b, w, bias, k8, v8, sc, B, H, Lk, scale=scale)
    ob = ops.decode_attn_proj(0, x, ln_g, ln_b, w, bias, kv[:, :D], kv[:, D:], B, H, Lk, scale=scale)
    torch.cuda.synchronize()
    assert torch.equal(bits(o8), bits(ob))
    assert len(set(o8.float().flatten().tolist())) > 8 * H, "the probes do not see q"


def test_attention_refusals_write_nothing(ops):
    from distil_whisper_amd.ops_hip import DW_BF16, DW_F32
    D, H, B, Lk, kv_rows = 384, 6, 2, 9, 12
    ln_g, ln_b, w, bias = dr.sweep_params(D, DEV)
    x = torch.randn(B, D + 8, device=DEV)
    k8 = torch.randint(0, 120, (B, H, kv_rows, 64), dtype=torch.uint8, device=DEV)
    v8 = torch.randint(0, 120, (B, H, kv_rows, 64), dtype=torch.uint8, device=DEV)
    sc = torch.rand(B, 2, D, device=DEV) + 0.5
    o = Guarded(B, D, pad=8)
    good = dict(x=x.data_ptr(), x_dtype=DW_F32, ldx=D + 8, ln_g=ln_g.data_ptr(), ln_b=ln_b.data_ptr(), eps=1e-5, w=w.data_ptr(),
                bias=bias.data_ptr(), k8=k8.data_ptr(), v8=v8.data_ptr(), sc=sc.data_ptr(), kv_rows=kv_rows, o=o.live.data_ptr(),
                ldo=o.live.stride(0), B=B, H=H, Lk=Lk, scale=0.125)

    def call(**over):
        a = dict(good, **over)
        return ops.lib.dw_decode_attn_proj_kv8(a["x"], a["x_dtype"], a["ldx"], a["ln_g"], a["ln_b"], a["eps"], a["w"], a["bias"], a["k8"],
                                               a["v8"], a["sc"], a["kv_rows"], a["o"], a["ldo"], a["B"], a["H"], a["Lk"], a["scale"],
                                               ops._stream())
    bad = [(EINVAL, dict(x_dtype=2)), (EINVAL, dict(x_dtype=-1))]
    bad += [(EINVAL, {n: None}) for n in ("x", "ln_g", "ln_b", "w", "bias", "k8", "v8", "sc", "o")]
    bad += [(EINVAL, dict(Lk=0)), (EINVAL, dict(Lk=kv_rows + 1)), (EINVAL, dict(B=0)), (EINVAL, dict(H=0))]
    bad += [(EINVAL, {n: good[n] + 8}) for n in ("x", "w", "k8", "v8", "ln_g", "ln_b")]
    bad += [(EINVAL, dict(ldx=D + 4)), (EINVAL, dict(x_dtype=DW_BF16, ldx=D + 4)), (EINVAL, dict(bias=good["bias"] + 2)),
            (EINVAL, dict(sc=good["sc"] + 2)), (EINVAL, dict(o=good["o"] + 1))]
    bad += [(EUNSUP, dict(H=h)) for h in (1, 2, 5, 7, 10, 14, 18, 21, 65535)]
    bad += [(EUNSUP, dict(Lk=dr.MAX_KEYS + 1, kv_rows=dr.MAX_KEYS + 8)), (EUNSUP, dict(B=65536)), (EUNSUP, dict(H=65536))]
    bad += [(EINVAL, dict(ldx=D - 8)), (EINVAL, dict(ldo=D - 8))]
    for want, over in bad:
        assert call(**over) == want, over
    torch.cuda.synchronize()
    assert o.untouched()
    assert call() == 0
    torch.cuda.synchronize()
    assert o.intact() and torch.isfinite(o.live.float()).all()


# ---- whole passes -------------------------------------------------------------------------------------------------------------------
def _engines(ops, D, seed):
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import ParamStore, WhisperDims, WhisperEngine
    from oracle.ref_ops import RefOps
    dims = WhisperDims(D, D // 64, dr.PASS_FFN, 1, 2, dr.PASS_VOCAB, 8, max_src=dr.PASS_SRC)
    sd = {k: v.to(torch.bfloat16).float() for k, v in si.random_state_dict(dims, seed, ops.device).items() if k.startswith("model.decoder.")}

    def eng(o, stream):
        return WhisperEngine(o, ParamStore(o, dims, sd, trainable=False, decoder_only=True), stream)
    return dims, eng(ops, torch.bfloat16), eng(RefOps(DEV), torch.bfloat16), eng(RefOps(DEV, lowp=torch.float64), torch.float64)


def _inputs(dims, B, seed):
    g = torch.Generator().manual_seed(seed)
    D = dims.d_model
    enc = (0.5 * torch.randn(B * dims.max_src, D, generator=g)).to(DEV).bfloat16()
    ids = torch.randint(0, dims.vocab, (B, 1), generator=g).to(DEV)
    base = [(0.5 * torch.randn(B * dr.PASS_MAX_LEN, 2 * D, generator=g)).to(DEV).bfloat16() for _ in range(dims.dec_layers)]
    return enc, ids, base


def _step(eng, enc, ids, base, B, t, cross8=None, row_t=None):
    """One token step on an FP8 cache -> logits [B, vocab] and the last layer's appended cache rows [B, 2D] as float64, and the
    cache.  cross8: the codes and scales every engine decodes from (the first engine's own)."""
    d, ML = eng.dims, dr.PASS_MAX_LEN
    dt = torch.float64 if eng.lowp == torch.float64 else torch.bfloat16
    cache = eng.decode_init(enc.to(dt), B, ML, cross_kv_dtype="fp8")
    if cross8 is not None:
        for trio, src in zip(cache["cross8"], cross8):
            for a, b in zip(trio, src):
                a.copy_(b)
    for kv, b0 in zip(cache["self"], base):
        kv.copy_(b0.to(dt))
    if row_t is None:
        cache["t"] = t
        logits = eng.decode_step(ids, cache)
        rows = torch.full((B,), t, device=DEV)
    else:
        rt = torch.tensor(row_t, dtype=torch.int32, device=DEV)
        logits = eng.decode_token_rows(ids, cache, rt, max(row_t))
        rows = rt.long()
    logits = logits[:, :d.vocab].double().clone()
    torch.cuda.synchronize()
    r = torch.arange(B, device=DEV)
    return logits, cache["self"][-1].view(B, ML, -1)[r, rows].double().clone(), cache


@pytest.mark.parametrize("B", [3, 18])
@pytest.mark.parametrize("D", [384, 1280])
def test_whole_passes_on_an_fp8_cache(ops, D, B):
    dims, hip, rb, r64 = _engines(ops, D, 50 + D)
    enc, ids, base = _inputs(dims, B, 7000 + 10 * B + D)
    row_t = [(5, 0, dr.PASS_MAX_LEN - 1)[b % 3] for b in range(B)]
    for name, kw in (("step", dict(t=5)), ("token_rows", dict(t=None, row_t=row_t))):
        got_l, got_c, cache = _step(hip, enc, ids, base, B, **kw)
        assert cache["cross8"][0][0].dtype == torch.uint8 and hip._decode_desc(cache, 1)[0].cross_kv_fmt == 1
        comp = _step(rb, enc, ids, base, B, cross8=cache["cross8"], **kw)
        want = _step(r64, enc, ids, base, B, cross8=cache["cross8"], **kw)
        for what, a, r, a64 in (("logits", got_l, comp[0], want[0]), ("cache", got_c, comp[1], want[1])):
            e, e_ref = dr.vec_err(a, a64), dr.vec_err(r, a64)
            print(f"KV8_PASS D{D} B{B} {name} {what}: kernels {e:.4e} per-kernel form {e_ref:.4e} ratio {e / e_ref:.3f}")
            assert torch.isfinite(a).all() and e_ref > 0 and e <= F_PASS * e_ref, f"D{D} B{B} {name} {what}: {e:.3e} > {F_PASS} x {e_ref:.3e}"


def test_fmt_0_ignores_the_new_fields_and_the_descriptor_refusals_launch_nothing(ops):
    import ctypes as C
    D, B = 384, 3
    dims, hip, _, _ = _engines(ops, D, 61)
    enc, ids, base = _inputs(dims, B, 99)
    ML = dr.PASS_MAX_LEN

    def bf16_pass(poke):
        cache = hip.decode_init(enc, B, ML)
        for kv, b0 in zip(cache["self"], base):
            kv.copy_(b0)
        desc, ws, layers, _ = hip._decode_desc(cache, 1)
        assert desc.cross_kv_fmt == 0 and layers[0].cross_k8 is None and layers[0].cross_scale is None
        if poke:                                   # valid device pointers that must not be read
            for L in layers:
                L.cross_k8, L.cross_v8, L.cross_scale = ws["a"].data_ptr(), ws["a"].data_ptr(), ws["x"].data_ptr()
        cache["t"] = 5
        logits = hip.decode_step(ids, cache).clone()
        torch.cuda.synchronize()
        return logits, [kv.clone() for kv in cache["self"]]
    (l0, c0), (l1, c1) = bf16_pass(False), bf16_pass(True)
    assert torch.equal(bits(l0), bits(l1)) and all(torch.equal(bits(a), bits(b)) for a, b in zip(c0, c1))
    # refusals at cross_kv_fmt = 1 (and of any other value), with the logits behind a canary
    cache = hip.decode_init(enc, B, ML, cross_kv_dtype="fp8")
    desc, ws, layers, _ = hip._decode_desc(cache, 1)
    desc.ids, desc.t = ids.data_ptr(), 5
    ws["logits"].fill_(-3.0)
    rt = torch.zeros(B, dtype=torch.int32, device=DEV)
    lib, st = ops.lib, ops._stream()
    assert ops.lib.dw_debug_set(7, 12) == 0
    try:
        assert lib.dw_decode_step(C.byref(desc), st) == EUNSUP                                   # the unfused cross-attention
    finally:
        ops.lib.dw_debug_set(7, 4)
    assert lib.dw_decode_step_rows(C.byref(desc), rt.data_ptr(), 5, st) == EUNSUP
    desc.n_new = 2
    assert lib.dw_decode_step(C.byref(desc), st) == EUNSUP
    desc.n_new = 1
    desc.cross_kv_fmt = 2
    assert lib.dw_decode_step(C.byref(desc), st) == EINVAL
    desc.cross_kv_fmt = 1
    keep = layers[1].cross_scale
    layers[1].cross_scale = None
    assert lib.dw_decode_step(C.byref(desc), st) == EINVAL
    assert lib.dw_decode_token_rows(C.byref(desc), rt.data_ptr(), 5, st) == EINVAL
    layers[1].cross_scale = keep
    torch.cuda.synchronize()
    assert bool((ws["logits"] == -3.0).all()), "a refused pass launched something"
    assert lib.dw_decode_step(C.byref(desc), st) == 0
    torch.cuda.synchronize()
    assert not bool((ws["logits"] == -3.0).all())


# ---- graphs and tokens --------------------------------------------------------------------------------------------------------------
def test_graph_replay_equals_eager_and_the_tokens_are_those_of_the_bf16_cache(ops, monkeypatch):
    from distil_whisper_amd.decoding import GreedyDecoder, SlotDecoder
    from oracle import gen_golden_decode as gd
    from oracle.ref_ops import RefOps
    from tests import test_cross_kv_fp8 as cpu
    from tests import test_slots as ts
    model, enc = ts.planted_target(ops, dtype=torch.bfloat16, width=384)
    cpu_model, cpu_enc = ts.planted_target(RefOps("cpu"), dtype=torch.bfloat16, width=384)
    eng, S = model.engine, model.dims.max_src
    windows = ts.make_windows(cpu.noisy(cpu_enc).to(DEV), 7, S)
    rec = cpu.record_windows(monkeypatch)
    kw = dict(suppress_tokens=gd.SUPPRESS)
    runs = {}
    for dt, graphs in ((None, False), ("fp8", False), ("fp8", True)):
        del rec[:]
        for key, e, prompt, max_new in windows[:3]:
            dec = GreedyDecoder(eng, 3, len(prompt) + max_new, eos_token_id=gd.EOS, pad_token_id=gd.EOS, use_graphs=graphs,
                                check_every=1, cross_kv_dtype=dt, **kw)
            dec.run(e.repeat(3, 1), torch.tensor([prompt] * 3, device=DEV), max_new)
        sd = SlotDecoder(eng, 3, len(ts.PROMPT) + 2 + 9, gd.EOS, check_every=2, use_graphs=graphs, cross_kv_dtype=dt, **kw)
        assert len(list(sd.run(iter(windows)))) == 7
        assert ("cross8" in sd.cache) == (dt == "fp8") and bool(sd.graphs) == graphs
        runs[dt, graphs] = [(k, e.cpu(), p, r) for k, e, p, r in rec]
    eager, replay = runs["fp8", False], runs["fp8", True]
    assert len(eager) == len(replay) == 16
    assert sorted((str(k), r) for k, _, _, r in eager) == sorted((str(k), r) for k, _, _, r in replay)
    for what, sel in (("greedy", "batch"), ("slot", "slot")):
        plain = [w for w in runs[None, False] if w[0][0] == sel]
        fp8 = [w for w in eager if w[0][0] == sel]
        cpu.judge(cpu_model.engine, plain, fp8, f"{what} on the GPU", suppress=gd.SUPPRESS)
