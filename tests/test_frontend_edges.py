"""CPU companion of tests/test_frontend_edges_gpu.py: the float64 statements of tests/frontend_restatement.py against independent
authorities -- torch.stft and transformers' WhisperFeatureExtractor for the log-mel, F.conv1d and its float64 autograd for the
im2col / col2im / weight layouts, autograd of F.gelu, nn.Embedding's autograd -- the fp32 log-mel statement against the float64 one
on every case's input (no case asks more than fp32 can give), the dead-frame clip's power to discriminate, the error of the
epilogue GELU's formula itself, and the dispatch tables against the constants in the sources."""
import math
import os
import re

import pytest
import torch
import torch.nn.functional as F

import frontend_restatement as fr

TOL = 1e-12
CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "distil_whisper_amd", "csrc")
F64 = torch.float64


def rel(a, b):
    a, b = a.double(), b.double()
    return ((a - b).norm() / b.norm().clamp_min(1e-300)).item()


def slaney(n_mels):
    from transformers.audio_utils import mel_filter_bank
    return torch.tensor(mel_filter_bank(201, n_mels, 0.0, 8000.0, 16000, norm="slaney", mel_scale="slaney"), dtype=torch.float32)


def bank(n_mels):
    return slaney(n_mels) if n_mels in (80, 128) else fr.synthetic_bank(n_mels)


# ---- log-mel ------------------------------------------------------------------------------------------------------------------------
def stft_logmel(audio, filters):
    win = torch.hann_window(400, periodic=True, dtype=F64)
    st = torch.stft(audio.double(), 400, 160, window=win, center=True, pad_mode="reflect", return_complex=True)
    power = st[..., :-1].abs() ** 2                                   # [B, 201, frames]
    mel = filters.double().t() @ power
    log_spec = torch.clamp(mel, min=1e-10).log10()
    log_spec = torch.maximum(log_spec, log_spec.amax(dim=(1, 2), keepdim=True) - 8.0)
    return (log_spec + 4.0) / 4.0


@pytest.mark.parametrize("frames,batch,n_mels,clip", fr.LOGMEL_CASES)
def test_logmel_statement_equals_stft_and_fp32_is_enough(frames, batch, n_mels, clip):
    audio, filt = fr.logmel_audio(frames, batch, clip), bank(n_mels)
    want = stft_logmel(audio, filt)
    got = fr.logmel(audio, filt)
    assert got.shape == (batch, n_mels, frames) and (got - want).abs().max().item() <= 1e-9
    if clip == "zero":
        assert bool((got == (-10.0 + 4.0) / 4.0).all())
    e32 = (fr.logmel(audio, filt, dtype=torch.float32).double() - got).abs().max().item()
    print(f"FRONT_EDGE logmel fp32 statement {frames}x{batch}x{n_mels} {clip}: {e32:.3e}")
    assert e32 <= 0.5e-4
    if clip == "dead":          # a maximum that takes in the dead frames cannot pass the GPU test's 1e-4
        wrong = fr.logmel(audio, filt, dead_frames=True)
        diff = (wrong - got).abs()
        print(f"FRONT_EDGE dead frames included: max {diff.max().item():.3f}, {100 * (diff > 1e-4).double().mean().item():.0f} % of the outputs")
        assert diff.max().item() > 1e-2


def test_logmel_statement_equals_whisper_feature_extractor():
    """30 s, the only length the extractor does not pad.  The extractor's STFT is single precision (its own docstring promises 1e-5;
    measured here against float64: 1.5e-5 at the worst of 384 000 outputs, 3e-8 on average), so it is held to what the fp32 statement
    is held to, 0.5e-4: it pins the formula -- filters, log10, clip, affine, the dropped last frame -- and torch.stft pins the digits."""
    from transformers import WhisperFeatureExtractor
    audio = 0.1 * torch.randn(1, 480000, generator=torch.Generator().manual_seed(0))
    for n_mels in (80, 128):
        fe = WhisperFeatureExtractor(feature_size=n_mels)
        want = torch.tensor(fe(audio[0].numpy(), sampling_rate=16000, return_tensors="np").input_features)
        filt = torch.tensor(fe.mel_filters, dtype=torch.float32)
        assert torch.equal(filt, slaney(n_mels))
        got = fr.logmel(audio, filt)
        assert got.shape == want.shape and (got - want.double()).abs().max().item() <= 0.5e-4


def test_synthetic_bank_has_the_supports_it_promises():
    for n_mels in (4, 256):
        f = fr.synthetic_bank(n_mels)
        assert f.shape == (201, n_mels) and bool((f >= 0).all())
        assert not bool(f[:, 0].any())
        nz = torch.nonzero(f[:, 1]).flatten()
        assert nz.min() == 10 and nz.max() == 30 and nz.numel() < 21
        assert torch.nonzero(f[:, 2]).flatten().tolist() == [0] and torch.nonzero(f[:, 3]).flatten().tolist() == [200]
        assert all(bool(f[:, m].any()) for m in range(4, n_mels))


# ---- conv stem --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,C,T,D", [(1, 1, 1, 1), (3, 80, 65, 5), (2, 129, 130, 3), (1, 64, 63, 2)])
def test_im2col_mel_and_packed_weight_equal_conv1d(B, C, T, D):
    g = torch.Generator().manual_seed(B + C + T)
    mel, w = torch.randn(B, C, T, generator=g), torch.randn(D, C, 3, generator=g)
    for kpad in {fr.kpad_of(C), 3 * C}:
        x, wp = fr.im2col_mel(mel, kpad), fr.pack_conv_weight(w, kpad)
        assert x.shape == (B * T, kpad) and not bool(x[:, 3 * C:].any()) and not bool(wp[:, 3 * C:].any())
        want = F.conv1d(mel.double(), w.double(), padding=1)
        assert rel((x @ wp.t()).reshape(B, T, D).transpose(1, 2), want) <= TOL
    # the weight gradient through the same layouts: unpack(dY^T X) = conv1d's autograd
    wd = w.double().requires_grad_(True)
    dy = torch.randn(B, D, T, generator=g, dtype=F64)
    F.conv1d(mel.double(), wd, padding=1).backward(dy)
    kpad = fr.kpad_of(C)
    gwp = dy.transpose(1, 2).reshape(B * T, D).t() @ fr.im2col_mel(mel, kpad)
    gw0 = torch.randn(D, C, 3, generator=g)
    assert rel(fr.unpack_conv_grad(gwp, gw0, False), wd.grad) <= TOL
    assert rel(fr.unpack_conv_grad(gwp, gw0, True) - gw0.double(), wd.grad) <= TOL


@pytest.mark.parametrize("B,T,C,D", [(1, 2, 8, 3), (3, 4, 24, 2), (3, 6, 8, 5), (2, 130, 24, 4)])
def test_im2col_s2_and_col2im_s2_equal_strided_conv1d_and_its_autograd(B, T, C, D):
    g = torch.Generator().manual_seed(B + C + T)
    a = torch.randn(B * T, C, generator=g).to(torch.bfloat16)
    w = torch.randn(D, C, 3, generator=g)
    x = a.double().reshape(B, T, C).transpose(1, 2).requires_grad_(True)
    y = F.conv1d(x, w.double(), stride=2, padding=1)                 # [B, D, T/2]
    wp = fr.pack_conv_weight(w, 3 * C)
    assert rel((fr.im2col_s2(a, B, T) @ wp.t()).reshape(B, T // 2, D).transpose(1, 2), y.detach()) <= TOL
    dy = torch.randn(B, D, T // 2, generator=g, dtype=F64)
    y.backward(dy)
    dxcol = dy.transpose(1, 2).reshape(B * T // 2, D) @ wp          # [B*T/2, 3C]
    assert rel(fr.col2im_s2(dxcol, B, T), x.grad.transpose(1, 2).reshape(B * T, C)) <= TOL


def test_gelu_statements_equal_autograd():
    z = torch.cat([fr.gelu_z(1024).double(), torch.linspace(-12, 12, 4097, dtype=F64)]).requires_grad_(True)
    y = F.gelu(z)
    y.sum().backward()
    # (a few float64 ulps of the value, absolutely below 1: torch's own 1 + erf has no relative accuracy in the lower tail)
    assert bool(((fr.gelu(z) - y.detach()).abs() <= 1e-15 * y.detach().abs().clamp_min(1.0)).all())
    assert (fr.gelu_grad(z) - z.grad).abs().max().item() <= 1e-15
    # ... where the statement keeps it: against the asymptotic series of the Mills ratio, gelu'(z) ~ pdf(z) (1/|z| - 1/|z|^3 + 3/|z|^5 - 15/|z|^7 - |z|)
    zt = torch.tensor([-20.0, -30.0], dtype=F64)
    pdf = torch.exp(-0.5 * zt * zt) / math.sqrt(2.0 * math.pi)
    series = pdf * ((1 / zt.abs() - 1 / zt.abs() ** 3 + 3 / zt.abs() ** 5 - 15 / zt.abs() ** 7) - zt.abs())
    assert bool(((fr.gelu_grad(zt) - series).abs() <= 1e-6 * series.abs()).all())
    assert bool((fr.gelu_grad(z.detach()) < 0).any())
    dy = torch.randn(z.numel())
    assert torch.equal(fr.gelu_bwd(dy, z.detach()), dy.to(torch.bfloat16).double() * fr.gelu_grad(z))


def test_epilogue_gelu_formula_error_and_bound_terms():
    """Abramowitz & Stegun 7.1.26 in float64 against erf: what the approximation costs before any fp32 rounding -- at most 2.2e-7 for
    gelu (near z = -3.08) and 0.75e-7 + ... for gelu' -- inside the first term of the GPU sweep's bound at every z."""
    z = torch.cat([fr.all_finite_bf16().double(), fr.gelu_sweep_fp32_values().to(torch.bfloat16).double(),
                   torch.linspace(-16, 16, 200001, dtype=F64)])
    y, g = fr.gelu_fast(z)
    ey, eg = (y - fr.gelu(z)).abs(), (g - fr.gelu_grad(z)).abs()
    k = int(ey.argmax())
    print(f"FRONT_EDGE A&S formula in float64: gelu {ey.max().item():.3e} at z = {z[k].item():.3f}, gelu' {eg.max().item():.3e}")
    assert ey.max().item() <= 2.3e-7 and 2.5 <= abs(z[k].item()) <= 3.5
    assert bool((ey <= 0.5 * fr.GELU_APPROX_ERF * z.abs() + 1e-18).all()) and bool((eg <= 0.5 * fr.GELU_APPROX_ERF + 1e-18).all())
    dy, dg = fr.gelu_fast_rounding_bound(z)
    fin = z.abs() <= 16
    print(f"FRONT_EDGE fp32 rounding terms on |z| <= 16: gelu {dy[fin].max().item():.3e}, gelu' {dg[fin].max().item():.3e}")
    assert bool(torch.isfinite(dy[z < fr.GELU_FAST_DOMAIN]).all()) and bool(torch.isinf(dy[z >= fr.GELU_FAST_DOMAIN]).all())
    assert int((fr.all_finite_bf16().double() >= fr.GELU_FAST_DOMAIN).sum()) == 128
    assert bool(torch.isfinite(dg).all()) and dy[fin].max().item() < 3e-6 and dg[fin].max().item() < 3e-6
    assert fr.ulp_of(torch.tensor([1.0, 0.75, 2.0 ** -20, 0.0], dtype=F64), torch.float16).tolist() == [2.0 ** -10, 2.0 ** -11, 2.0 ** -24, 2.0 ** -24]
    assert fr.ulp_of(torch.tensor([1.0, 255.0], dtype=F64), torch.bfloat16).tolist() == [2.0 ** -7, 1.0]


# ---- embeddings -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", fr.EMBED_BWD_CASES, ids=str)
def test_embedding_statements_equal_nn_embedding_autograd(case):
    B, T, D, kind, dpos_kind, dtok_filled = case
    D = min(D, 8)
    V = max(fr.EMBED_V, B * T) if kind == "distinct" else fr.EMBED_V
    g = torch.Generator().manual_seed(B * T + D)
    ids = fr.embed_ids(B, T, V, kind)
    tok, pos = torch.nn.Embedding(V, D).double(), torch.nn.Embedding(448, D).double()
    dx = torch.randn(B * T, D, generator=g)
    out = tok(ids) + pos(torch.arange(T))[None]
    assert rel(fr.embed_fwd(ids, tok.weight, pos.weight), out.detach().reshape(B * T, D)) <= TOL
    out.backward(dx.double().reshape(B, T, D))
    dtok0, dpos0 = torch.randn(V, D, generator=g), torch.randn(448, D, generator=g)
    got_tok, got_pos = fr.embed_bwd(dx, ids, dtok0, dpos0)
    assert rel(got_tok - dtok0.double(), tok.weight.grad) <= TOL and rel(got_pos - dpos0.double(), pos.weight.grad) <= TOL
    assert fr.embed_bwd(dx, ids, dtok0, None)[1] is None
    never = torch.ones(V, dtype=torch.bool)
    never[ids.reshape(-1)] = False
    assert torch.equal(got_tok[never], dtok0.double()[never]) and torch.equal(got_pos[T:], dpos0.double()[T:])


# ---- small statements ---------------------------------------------------------------------------------------------------------------
def test_small_statements():
    x = fr.colsum_input(17, 8, "cancel")
    out0 = torch.randn(8)
    assert torch.equal(fr.colsum(x, out0, True), out0.double() + x.double().sum(0)) and torch.equal(fr.colsum(x, out0, False), x.double().sum(0))
    assert x.float().abs().max() > 100 and x.double().sum(0).abs().max() < 40
    part, o = torch.randn(7, 12), torch.randn(12)
    want = o.clone()
    for s in range(7):
        want += part[s]
    assert torch.equal(fr.reduce_slices_fp32(part, o, True), want) and torch.equal(fr.reduce_slices_fp32(part[:1], o, False), part[0] + 0.0)
    sp = fr.cast_specials_f32()
    assert bool(torch.isnan(sp[0])) and sp[1] == math.inf and sp[2] == -math.inf and bool(torch.isnan(sp[-2]))
    assert math.copysign(1.0, sp[4].item()) == -1.0 and sp[5].item() == 2.0 ** -149
    b = sp.to(torch.bfloat16).view(torch.int16).tolist()
    bits = lambda v: v & 0xFFFF
    # ties to even: 0x3F808000 -> 0x3F80, 0x3F818000 -> 0x3F82; above / below the tie; carry into the exponent; overflow to infinity
    assert [bits(v) for v in b[10:18]] == [0x3F80, 0x3F82, 0x3F81, 0x3F80, 0x4000, 0x7F80, 0x7F7F, 0x7F80]
    assert bits(b[8]) == 0x0000 and bits(b[9]) == 0x0002 and bits(b[6]) == 0x8000


# ---- the tables hold what the GPU module promises, and the dispatch facts are those of the sources --------------------------------------
def _src(name):
    return open(os.path.join(CSRC, name)).read()


def test_dispatch_facts_equal_the_sources():
    lm, el = _src("logmel.hip"), _src("elementwise.hip")
    assert int(re.search(r"#define LM_FR (\d+)", lm).group(1)) == fr.LM_FRAMES_PER_TILE
    assert int(re.search(r"#define LQ_TPB (\d+)", lm).group(1)) == fr.LM_TILES_PER_WG
    assert f"dim3((batch + {fr.LM_INIT_BLOCK - 1}) / {fr.LM_INIT_BLOCK}), dim3({fr.LM_INIT_BLOCK})" in lm
    assert f"n_mels > {fr.LM_MAX_MELS}" in lm and "n_samples < 400 || (n_samples % 160)" in lm
    assert f"blockIdx.x * {fr.IM2COL_MEL_FRAMES};" in el and f"c0 += {fr.IM2COL_MEL_CHANNELS})" in el
    assert f"if (nb > {fr.ADD_GRID_BLOCKS}) nb = {fr.ADD_GRID_BLOCKS};" in el
    assert f"int ry = (rows + {fr.COLSUM_ROW_LANES - 1}) / {fr.COLSUM_ROW_LANES};" in el and f"if (ry > {fr.COLSUM_MAX_GROUPS}) ry = {fr.COLSUM_MAX_GROUPS};" in el
    assert "const int step = gridDim.y * 16;" in el and "for (; r + 3 * step < rows; r += 4 * step)" in el
    cm = _src("common.h")
    for c in fr.AS_A + (fr.AS_P,):
        assert f"{abs(c):.9g}f" in cm or f"{abs(c)}f" in cm, c


def test_case_tables_hold_every_class():
    assert fr.LOGMEL_FRAMES == [3, 31, 32, 33, 384, 385, 417]
    cases = fr.LOGMEL_CASES
    assert {c[0] for c in cases} == set(fr.LOGMEL_FRAMES) and {c[1] for c in cases} == {1, 3, 65} and {c[2] for c in cases} == {4, 80, 128, 256}
    assert {c[3] for c in cases} == set(fr.LOGMEL_CLIPS) and all((c[0] * c[2]) % 4 == 0 for c in cases)
    tile, wg = fr.LM_FRAMES_PER_TILE, fr.LM_FRAMES_PER_TILE * fr.LM_TILES_PER_WG
    assert {3, tile - 1, tile, tile + 1, wg, wg + 1, wg + tile + 1} == set(fr.LOGMEL_FRAMES)
    assert max(c[1] for c in cases) > fr.LM_INIT_BLOCK
    # colsum: both sides of the unrolled loop's threshold, with and without a remainder, the group count capped
    assert fr.COLSUM_ROWS == [1, 15, 16, 17, 1003, 1024, 1025, 3072, 3073, 4101, 5123, 8197]
    assert [fr.colsum_grid(r)[1] for r in fr.COLSUM_ROWS] == [False] * 8 + [True] * 4
    assert fr.colsum_grid(1025) == (64, False) and fr.colsum_grid(1024) == (64, False) and fr.colsum_grid(1003)[0] == 63
    assert (4101 - 4096) > 0 and 8197 > 2 * 4096
    cs = fr.colsum_cases()
    assert {c[0] for c in cs} == set(fr.COLSUM_ROWS) and {c[1] for c in cs} == set(fr.COLSUM_COLS)
    for key, vals in ((2, {0, 8}), (3, {0, 16}), (4, {0, 1}), (5, {"gauss", "cancel"})):
        assert {c[key] for c in cs} == vals
        assert {c[key] for c in cs if fr.colsum_grid(c[0])[1]} == vals            # ... also among the cases of the unrolled loop
    assert any(c[0] == 8197 and c[1] == 1280 for c in cs)
    # add: all eight combinations, the grid wraps once with a ragged tail
    assert len(set(fr.ADD_DTYPES)) == 8 and fr.ADD_N[-1] > fr.ADD_GRID_BLOCKS * 256 and fr.ADD_N[-1] % 256
    assert fr.CAST_N == [1, 2, 3, 4, 5, 1023, 1024, 1025, 1027] and {n % 4 for n in fr.CAST_N} == {0, 1, 2, 3}
    # embeddings
    assert {c[2] for c in fr.EMBED_FWD_CASES} == set(fr.EMBED_D) and {c[1] for c in fr.EMBED_FWD_CASES} == set(fr.EMBED_T)
    assert any((B * T * (D // 4)) % 256 for B, T, D in fr.EMBED_FWD_CASES) and len(fr.EMBED_DTYPES) == 4
    assert {c[2] for c in fr.EMBED_BWD_CASES} == {4, 260, 384} and {c[3] for c in fr.EMBED_BWD_CASES} == {"distinct", "equal", "padded"}
    assert {c[4] for c in fr.EMBED_BWD_CASES} == {None, "zero", "filled"} and any(c[0] * c[1] == 16 * 448 and c[3] == "equal" for c in fr.EMBED_BWD_CASES)
    ids = fr.embed_ids(4, 448, fr.EMBED_V, "padded")
    assert int((ids == fr.EMBED_V - 1).sum()) > 4 * 400 and ids.max() == fr.EMBED_V - 1
    ids = fr.embed_ids(3, 7, fr.EMBED_V, "random")
    assert ids.min() == 0 and ids.max() == fr.EMBED_V - 1
    # conv stem
    assert fr.IM2COL_MEL_C == [1, 80, 128, 129, 200] and fr.IM2COL_MEL_T == [1, 63, 64, 65, 130]
    assert max(fr.IM2COL_MEL_C) > fr.IM2COL_MEL_CHANNELS and fr.kpad_of(64) == 192 and fr.kpad_of(80) == 256 and fr.kpad_of(1) == 64
    assert fr.S2_T == [2, 4, 6, 130] and fr.S2_C == [8, 24, 384] and fr.GELU_BWD_N == [4, 1020, 1024, 1028, 65536]
    z = fr.gelu_z(1024).double()
    assert bool((fr.gelu_grad(z) < 0).any()) and z.abs().max() == 12 and bool((z == 0).any())
    assert fr.all_finite_bf16().numel() == 65536 and int((fr.all_finite_bf16() == 0).sum()) == 258
    v = fr.gelu_sweep_fp32_values()
    assert v.numel() == 4096 and 1e-6 <= v.abs().min() and v.abs().max() <= 16 and bool((v < 0).any()) and bool((v > 0).any())
