"""FP8 cross-attention K/V (include/dwamd.h "FP8 cross-attention K/V"; distil_whisper_amd/kv_quant.py) on the CPU.

* The torch statement (kv_quant) against the numpy statement (tests/kv_quant_restatement.py), bit for bit: all 256 codes, the
  special columns (ties of the grid, +-448 after scaling, the subnormal range, a column of zeros and magnitudes below 2^-100, one
  non-zero, a +-30 outlier),
  and the bound every dequantised element obeys by the format alone.
* The public surface: every refusal fires before `engine.encode` runs; None and "bf16" are the call without the argument, tokens
  and logits bit for bit; a refilled cache keeps its addresses; `decode_refill` of one slot leaves the other slots alone.
* Tokens: GreedyDecoder, SlotDecoder (7 windows on 3 slots), PseudoLabeller and LongFormTranscriber (batch path and
  continuous=True) with cross_kv_dtype="fp8" against themselves without it, over oracle.ref_ops in bf16 (no kernels: the torch
  statements on both sides).  Every decoded window is recorded at `GreedyDecoder.run` / `SlotDecoder.run`; for a window,
  delta = the largest logit difference between the FP8 and the bf16 statement when both are fed the bf16 path's tokens, and a
  generated step is EXEMPT when the bf16 path's top-2 margin among the allowed tokens is below 4 delta.  Windows without an
  exempt step must be equal token for token, windows with one up to it, and at most a quarter of the windows may hold one.
  The model is the planted width-384 target of tests/test_slots.py (scale 4, head gain 4, seed 21) over its planted encoder rows
  plus noise (`noisy`: without it every K / V column is constant and quantises exactly).  Measured on the CPU (ref_ops bf16; the
  tests print it): delta <= 0.125 -- one bf16 step of a logit of 30 -- against a smallest top-2 margin of 6.1 in all 52 recorded
  windows, so no window holds an exempt step and every token is equal.  (A model of random weights does not serve: at width 384,
  std 0.1, its margins fall to 0.1 and all of its windows held an exempt step.)
"""
import numpy as np
import pytest
import torch

import kv_quant_restatement as kr
from distil_whisper_amd import kv_quant as kq
from distil_whisper_amd.decoding import GreedyDecoder, SlotDecoder
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps
from tests import test_slots as ts


# ---- the format ---------------------------------------------------------------------------------------------------------------
def test_all_256_codes_decode_to_the_table():
    got = kq.decode(torch.arange(256, dtype=torch.uint8)).double().numpy()
    nan = np.isnan(kr.E4M3FN)
    assert nan.sum() == 2 and np.array_equal(np.isnan(got), nan)
    assert np.array_equal(got[~nan], kr.E4M3FN[~nan]) and np.array_equal(np.signbit(got[~nan]), np.signbit(kr.E4M3FN[~nan]))
    # and every finite value encodes to its own code (the two zeros keep their sign)
    fin = np.flatnonzero(~nan)
    assert np.array_equal(kr.encode(kr.E4M3FN[fin].astype(np.float32)), fin.astype(np.uint8))


def test_exact_ties_go_to_the_even_code_and_saturation_never_gives_nan():
    grid = kr.E4M3FN[:127]
    mid = ((grid[:-1] + grid[1:]) / 2).astype(np.float32)
    y = np.concatenate([mid, -mid, np.float32([448.0, -448.0, 464.0, 1e9, -1e9, 2.0 ** -10, -(2.0 ** -10), 0.0, -0.0])])
    want = kr.encode(y)
    assert np.array_equal(want[:126] % 2, np.zeros(126, dtype=np.uint8))                   # every tie landed on an even code
    assert not np.isin(want, [0x7F, 0xFF]).any() and want[252] == 0x7E and want[253] == 0xFE and want[254] == 0x7E
    assert want[257] == 0x00 and want[258] == 0x80 and want[-1] == 0x80                     # half the smallest subnormal: to even, signed
    got = torch.from_numpy(y).clamp(-448.0, 448.0).to(torch.float8_e4m3fn).view(torch.uint8).numpy()
    assert np.array_equal(got, want)


@pytest.mark.parametrize("rows", [1, 7, 15, 16, 17, 63, 64, 65, 1500])
def test_torch_quantiser_equals_the_numpy_statement(rows):
    x = kr.special_columns(rows, seed=rows)
    codes, s = kq.quantize(torch.from_numpy(x)[None].bfloat16())
    want_c, want_s = kr.quantize(x)
    assert np.array_equal(codes[0].numpy(), want_c)
    assert np.array_equal(s[0].numpy().view(np.uint32), want_s.view(np.uint32))
    assert want_s[0] == 1.0 and not (want_c[:, 0] & 0x7F).any()                             # the zero column (|x| < 2^-100): signed zeros
    assert not np.isin(want_c, [0x7F, 0xFF]).any()
    if rows > 1:
        assert (np.abs(kr.decode(want_c)).max(0)[1:6] == 448.0).all()                       # a column's largest magnitude is +-448
    deq = kq.dequantize(codes, s)[0].numpy()
    assert np.array_equal(deq, kr.dequantize(want_c, want_s).astype(np.float32))            # (torch rounds the product to fp32)
    assert (np.abs(deq.astype(np.float64) - x) <= kr.dequant_bound(x, want_s)).all()
    assert (np.abs(kr.dequantize(want_c, want_s) - x) <= kr.dequant_bound(x, want_s)).all()
    # an outlier does not cost the other columns their precision: column 7 has its own scale
    if rows >= 63:
        assert want_s[2] > 4 * want_s[7]


def test_bound_on_random_bf16_values_with_an_outlier_channel():
    g = torch.Generator().manual_seed(3)
    x = torch.randn(2, 300, 128, generator=g)
    x[:, :, 5] *= 30.0
    x = x.bfloat16()
    codes, s = kq.quantize(x)
    for b in range(2):
        xb = x[b].float().numpy()
        want_c, want_s = kr.quantize(xb)
        assert np.array_equal(codes[b].numpy(), want_c) and np.array_equal(s[b].numpy(), want_s)
        assert (np.abs(kr.dequantize(want_c, want_s) - xb) <= kr.dequant_bound(xb, want_s)).all()


def test_torch_attention_over_codes_against_float64():
    g = torch.Generator().manual_seed(9)
    B, H, S = 2, 6, 37
    D = 64 * H
    kv = torch.randn(B * S, 2 * D, generator=g).bfloat16()
    q = torch.randn(B, D, generator=g).bfloat16()
    k8, v8 = torch.zeros(B, H, S, 64, dtype=torch.uint8), torch.zeros(B, H, S, 64, dtype=torch.uint8)
    sc = torch.ones(B, 2, D)
    kq.quantize_into(kv, k8, v8, sc, 0, B, S, H)
    o = kq.attention(q, k8, v8, sc, 0.125).float().numpy()
    for b in range(B):
        x = kv[b * S:(b + 1) * S].float().numpy()
        ck, sk = kr.quantize(x[:, :D])
        cv, sv = kr.quantize(x[:, D:])
        assert np.array_equal(k8[b].numpy(), kr.head_major(ck, H)) and np.array_equal(v8[b].numpy(), kr.head_major(cv, H))
        assert np.array_equal(sc[b, 0].numpy(), sk) and np.array_equal(sc[b, 1].numpy(), sv)
        want = kr.attend(q[b].float().numpy(), ck, cv, sk, sv)
        assert np.abs(o[b] - want).max() <= 2.0 ** -8 * np.abs(want).max() + 2.0 ** -7 * np.abs(want).mean()     # bf16 P, bf16 o


# ---- models -------------------------------------------------------------------------------------------------------------------
def _ops():
    return RefOps("cpu")            # lowp bf16: the torch bf16 statement on one side, the torch FP8 statement on the other


def _model384(seed=23):
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperFeatureExtractor, WhisperForConditionalGeneration
    from oracle import whisper_oracle as wo
    cfg = wo.OracleConfig(384, 6, 768, 1, 2, gd.V, 80, pad_token_id=gd.EOS, decoder_start_token_id=gd.SOT)
    ops = _ops()
    model = WhisperForConditionalGeneration(cfg, ops=ops, state_dict=wo.init_state_dict(cfg, seed, std=0.1))
    model.generation_config = GenerationConfig.from_any(gd.generation_fields(multilingual=True, suppress=True, timestamps=False))
    model.generation_config.alignment_heads = [[0, 1], [1, 0]]
    return cfg, model, WhisperFeatureExtractor(feature_size=80, ops=ops)


@pytest.fixture(scope="module")
def m384():
    return _model384()


# ---- the surface ----------------------------------------------------------------------------------------------------------------
def test_every_refusal_comes_before_the_encoder_runs(m384, monkeypatch):
    from distil_whisper_amd.longform import LongFormTranscriber
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    cfg, model, fe = m384
    f = gd.features(5, 2)

    def no_encode(*a, **k):
        raise AssertionError("the encoder ran before the refusal")
    monkeypatch.setattr(type(model.engine), "encode", no_encode)
    base = dict(language="en", max_new_tokens=4, cross_kv_dtype="fp8")
    for extra in (dict(return_timestamps=True),                                                      # the seek loop
                  dict(input_features=gd.features(5, 1).repeat(1, 1, 2), return_timestamps=True),     # more than 30 s
                  dict(num_beams=2), dict(assistant_model=model),
                  dict(return_dict_in_generate=True, output_scores=True), dict(return_dict_in_generate=True, output_logits=True),
                  dict(return_token_timestamps=True), dict(condition_on_prev_tokens=True, return_timestamps=True),
                  dict(temperature=(0.0, 0.4), return_timestamps=True)):
        kw = dict(base, **extra)
        with pytest.raises(NotImplementedError, match="fp8"):
            model.generate(kw.pop("input_features", f), **kw)
    with pytest.raises(ValueError, match="use_cache"):
        model.generate(f, use_cache=False, **base)
    for bad in ("fp16", "FP8", 8, "e4m3"):
        with pytest.raises(ValueError, match="cross_kv_dtype"):
            model.generate(f, language="en", max_new_tokens=4, cross_kv_dtype=bad)
        with pytest.raises(ValueError, match="cross_kv_dtype"):
            GreedyDecoder(model.engine, 2, 8, cross_kv_dtype=bad)
        with pytest.raises(ValueError, match="cross_kv_dtype"):
            SlotDecoder(model.engine, 2, 8, gd.EOS, cross_kv_dtype=bad)
        with pytest.raises(ValueError, match="cross_kv_dtype"):
            PseudoLabeller(model, fe, batch_size=2, max_new_tokens=4, eos_token_id=gd.EOS, cross_kv_dtype=bad)
        with pytest.raises(ValueError, match="cross_kv_dtype"):
            LongFormTranscriber(model, fe, batch_size=2, max_new_tokens=4, eos_token_id=gd.EOS, cross_kv_dtype=bad)
    kw = dict(batch_size=2, max_new_tokens=4, eos_token_id=gd.EOS, cross_kv_dtype="fp8")
    for extra in (dict(num_beams=2), dict(assistant_model=model),
                  dict(timestamp_rules=dict(no_timestamps_token_id=gd.NOTIMESTAMPS, max_initial_timestamp_index=50))):
        with pytest.raises(NotImplementedError, match="fp8"):
            PseudoLabeller(model, fe, **kw, **extra)
    # a width without the kernel
    narrow, _ = ts.planted_target(_ops())
    assert narrow.dims.d_model == 128
    with pytest.raises(ValueError, match="width"):
        GreedyDecoder(narrow.engine, 2, 8, cross_kv_dtype="fp8")
    with pytest.raises(ValueError, match="width"):
        SlotDecoder(narrow.engine, 2, 8, gd.EOS, cross_kv_dtype="fp8")
    with pytest.raises(ValueError, match="width"):
        narrow.generate(f, max_new_tokens=2, cross_kv_dtype="fp8")
    with pytest.raises(ValueError, match="width"):
        narrow.engine.decode_init(torch.zeros(narrow.dims.max_src, 128), 1, 8, cross_kv_dtype="fp8")
    # the multi-token passes do not read an FP8 cache
    eng = model.engine
    cache = eng.decode_slots_init(2, 8, cross_kv_dtype="fp8")
    with pytest.raises(NotImplementedError, match="token step"):
        eng.decode_multi(torch.zeros(2, 2, dtype=torch.long), cache)
    with pytest.raises(NotImplementedError, match="token step"):
        eng.decode_multi_rows(torch.zeros(2, 2, dtype=torch.long), cache, torch.zeros(2, dtype=torch.int32), 0)


def _spy_logits(monkeypatch, engine):
    seen = []
    step = type(engine).decode_step

    def spy(self, ids, cache):
        out = step(self, ids, cache)
        seen.append(out.clone())
        return out
    monkeypatch.setattr(type(engine), "decode_step", spy)
    return seen


def test_none_and_bf16_are_the_call_without_the_argument(m384, monkeypatch):
    cfg, model, fe = m384
    f = gd.features(7, 2)
    seen = _spy_logits(monkeypatch, model.engine)
    kw = dict(language="en", max_new_tokens=5)
    runs = []
    for extra in ({}, dict(cross_kv_dtype=None), dict(cross_kv_dtype="bf16")):
        del seen[:]
        model._decoders = {}
        runs.append((model.generate(f, **kw, **extra), [t.clone() for t in seen]))
    for tok, logits in runs[1:]:
        assert torch.equal(tok, runs[0][0]) and len(logits) == len(runs[0][1]) > 0
        assert all(torch.equal(a.view(torch.int16), b.view(torch.int16)) for a, b in zip(logits, runs[0][1]))
    assert "cross8" not in next(iter(model._decoders.values())).cache
    # and "fp8" is another cache: it runs, and its logits are not the bf16 cache's
    del seen[:]
    out = model.generate(f, **kw, cross_kv_dtype="fp8")
    assert out.shape[0] == 2 and "cross8" in next(iter(model._decoders.values())).cache
    assert not all(torch.equal(a, b) for a, b in zip(seen, runs[0][1]))
    sampled = model.generate(f, language="en", max_new_tokens=3, temperature=0.7, repetition_penalty=1.2, cross_kv_dtype="fp8")
    stamped = model.generate(f, language="en", max_new_tokens=3, return_timestamps=True, force_unique_generate_call=True,
                             cross_kv_dtype="fp8")
    assert sampled.shape[0] == 2 and stamped.shape[0] == 2


def _addresses(cache):
    out = [t.data_ptr() for t in cache["self"]] + [cache["cross_stage"].data_ptr()]
    for trio in cache["cross8"]:
        out += [t.data_ptr() for t in trio]
    return out


def test_a_refilled_cache_keeps_its_addresses_and_a_refill_leaves_the_other_slots_alone(m384):
    cfg, model, fe = m384
    eng, S, D = model.engine, cfg.max_src, cfg.d_model
    g = torch.Generator().manual_seed(11)
    enc = torch.randn(3 * S, D, generator=g).bfloat16()
    cache = eng.decode_init(enc, 3, 8, cross_kv_dtype="fp8")
    assert cache["cross"] == [None] * cfg.dec_layers and cache["cross_stage"].shape == (3 * S, 2 * D)
    assert all(k.dtype == torch.uint8 and k.shape == (3, cfg.heads, S, 64) and s.shape == (3, 2, D) for k, _, s in cache["cross8"])
    at = _addresses(cache)
    first = [[t.clone() for t in trio] for trio in cache["cross8"]]
    again = eng.decode_init(torch.randn(3 * S, D, generator=g).bfloat16(), 3, 8, cache=cache)
    assert again is cache and _addresses(cache) == at
    assert not torch.equal(cache["cross8"][0][0], first[0][0])
    # slots: one window's rows of staging; a refill of slot 1 writes slot 1 alone and gives what decode_init gave that window
    slots = eng.decode_slots_init(3, 8, cross_kv_dtype="fp8")
    assert slots["cross_stage"].shape == (S, 2 * D)
    for b in range(3):
        eng.decode_refill(slots, b, enc[b * S:(b + 1) * S])
    for trio, want in zip(slots["cross8"], first):
        assert all(torch.equal(a, b) for a, b in zip(trio, want))
    at = _addresses(slots)
    eng.decode_refill(slots, 1, torch.randn(S, D, generator=g).bfloat16())
    assert _addresses(slots) == at
    for trio, want in zip(slots["cross8"], first):
        for a, b in zip(trio, want):
            assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and not torch.equal(a[1], b[1])


# ---- tokens ---------------------------------------------------------------------------------------------------------------------
def noisy(enc, seed=1):
    """The planted encoder rows are constant over a window's positions: every K / V column would quantise exactly (x * inv = +-448)
    and the two statements would agree bit for bit.  Noise of half the rows' mean magnitude gives every column a spread to round;
    the planted decisions stand far above it."""
    g = torch.Generator().manual_seed(seed)
    return (enc.float() + 0.5 * enc.float().abs().mean() * torch.randn(enc.shape, generator=g)).bfloat16()


def record_windows(monkeypatch):
    """Every window decoded from here on, at GreedyDecoder.run / SlotDecoder.run: [(key, enc rows, prompt, row cut behind its EOS)]."""
    out = []
    g_run, s_run = GreedyDecoder.run, SlotDecoder.run

    def cut(row, P, eos):
        return row[:row.index(eos, P) + 1] if eos is not None and eos in row[P:] else row

    def greedy(self, enc_out, prompt_ids, max_new_tokens, min_new_tokens=0):
        tok = g_run(self, enc_out, prompt_ids, max_new_tokens, min_new_tokens)
        S = self.eng.dims.max_src
        for b in range(prompt_ids.shape[0]):
            out.append((("batch", len(out)), enc_out[b * S:(b + 1) * S].clone(), prompt_ids[b].tolist(),
                        cut(tok[b].tolist(), prompt_ids.shape[1], self.eos)))
        return tok

    def slots(self, windows):
        held = {}

        def feed():
            for w in windows:
                held[w[0]] = (w[1].clone(), [int(t) for t in torch.as_tensor(w[2]).reshape(-1).tolist()])
                yield w
        for key, row in s_run(self, feed()):
            out.append((("slot", key), *held[key], row.tolist()))
            yield key, row
    monkeypatch.setattr(GreedyDecoder, "run", greedy)
    monkeypatch.setattr(SlotDecoder, "run", slots)
    return out


def exempt_step(engine, enc_rows, prompt, row, suppress=(), begin_suppress=()):
    """-> (delta, index of the first exempt generated token of `row` or None, smallest margin): both statements fed the bf16 path's
    tokens of one window."""
    V, P = engine.dims.vocab, len(prompt)
    caches = [engine.decode_init(enc_rows, 1, len(row) + 1, cross_kv_dtype=dt) for dt in (None, "fp8")]
    delta, margins = 0.0, []
    for t in range(len(row) - 1):
        ids = torch.tensor([[row[t]]])
        lb, lf = (engine.decode_step(ids, c)[0, :V].float().clone() for c in caches)
        delta = max(delta, float((lb - lf).abs().max()))
        if t + 1 >= P:
            lb[list(suppress)] = -float("inf")
            if t + 1 == P:
                lb[list(begin_suppress)] = -float("inf")
            top = lb.topk(2).values
            margins.append((t + 1, float(top[0] - top[1])))
    hit = [n for n, m in margins if m < 4 * delta]
    return delta, (hit[0] if hit else None), min([m for _, m in margins], default=float("inf"))


def judge(engine, plain, fp8, what, suppress=(), begin_suppress=()):
    """The rule of the module docstring over two recordings of the same windows; -> number of windows with an exempt step."""
    assert len(plain) == len(fp8) > 0, what
    # (slots finish in an order that depends on the tokens: by key; batches come in plan order: by index)
    fp8 = {k: r for k, _, _, r in fp8} if plain[0][0][0] == "slot" else [r for _, _, _, r in fp8]
    exempt, deltas, margins = 0, [], []
    for i, (key, enc, prompt, row) in enumerate(plain):
        got = fp8[i] if isinstance(fp8, list) else fp8[key]
        delta, at, margin = exempt_step(engine, enc, prompt, row, suppress, begin_suppress)
        deltas.append(delta)
        margins.append(margin)
        if at is None:
            assert got == row, f"{what} window {key}: tokens differ without an exempt step (delta {delta:.3g}, margin {margin:.3g})"
        else:
            exempt += 1
            assert got[:at] == row[:at], f"{what} window {key}: tokens differ in front of the exempt step {at}"
    print(f"KV8_TOKENS {what}: {len(plain)} windows, {exempt} with an exempt step, delta <= {max(deltas):.4g}, smallest margin {min(margins):.4g}")
    assert 4 * exempt <= len(plain), f"{what}: {exempt} of {len(plain)} windows hold an exempt step"
    return exempt


def test_greedy_and_slot_decoder_on_the_planted_model(monkeypatch):
    ops = _ops()
    model, enc = ts.planted_target(ops, dtype=torch.bfloat16, width=384)
    eng, S = model.engine, model.dims.max_src
    windows = ts.make_windows(noisy(enc), 7, S)
    rec = record_windows(monkeypatch)
    kw = dict(suppress_tokens=gd.SUPPRESS)
    runs = {}
    for dt in (None, "fp8"):
        del rec[:]
        for key, e, prompt, max_new in windows:                      # GreedyDecoder: every window in a batch of three rows
            dec = GreedyDecoder(eng, 3, len(prompt) + max_new, eos_token_id=gd.EOS, pad_token_id=gd.EOS, use_graphs=False, check_every=1,
                                cross_kv_dtype=dt, **kw)
            dec.run(e.repeat(3, 1), torch.tensor([prompt] * 3), max_new)
            assert ("cross8" in dec.cache) == (dt == "fp8")
        runs["greedy", dt] = list(rec)
        del rec[:]
        sd = SlotDecoder(eng, 3, len(ts.PROMPT) + 2 + 9, gd.EOS, check_every=2, cross_kv_dtype=dt, **kw)
        assert len(list(sd.run(iter(windows)))) == 7 and ("cross8" in sd.cache) == (dt == "fp8")
        runs["slot", dt] = list(rec)
    assert len(runs["greedy", None]) == 21 and len(runs["slot", None]) == 7
    assert len({len(r) for _, _, _, r in runs["slot", None]}) > 1                 # rows end at different lengths
    for what in ("greedy", "slot"):
        judge(eng, runs[what, None], runs[what, "fp8"], what, suppress=gd.SUPPRESS)


def test_labeller_and_transcriber(monkeypatch):
    """The planted width-384 target behind the real packing, windowing and decoders: the encoder is replaced by one that hands
    out the planted encoder rows (kinds 0, 1, 2 in turn), since the planted decoder answers those rows and no audio produces them."""
    from distil_whisper_amd.longform import LongFormTranscriber
    from distil_whisper_amd.modeling import WhisperFeatureExtractor
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    ops = _ops()
    model, enc = ts.planted_target(ops, dtype=torch.bfloat16, width=384)
    fe = WhisperFeatureExtractor(feature_size=80, ops=ops)
    S, served = model.dims.max_src, [0]
    enc = noisy(enc)

    def planted_encode(self, feats, save=False):
        rows = [enc[((served[0] + b) % 3) * S:((served[0] + b) % 3 + 1) * S] for b in range(feats.shape[0])]
        served[0] += feats.shape[0]
        return torch.cat(rows), None
    monkeypatch.setattr(type(model.engine), "encode", planted_encode)
    rng = np.random.default_rng(10)
    rec = record_windows(monkeypatch)
    audios = [0.1 * rng.standard_normal(n).astype(np.float32) for n in (200_000, 150_000, 300_000, 100_000, 260_000, 90_000, 120_000)]
    spk = [0, 0, 0, 1, 2, 3, 4]
    for continuous in (False, True):
        kw = dict(batch_size=2, max_new_tokens=9, prompt_ids=ts.PROMPT, eos_token_id=gd.EOS, use_graphs=False, suppress_tokens=gd.SUPPRESS,
                  continuous=continuous, check_every=2)
        outs, recs = [], []
        for dt in (None, "fp8"):
            del rec[:]
            served[0] = 0
            outs.append(PseudoLabeller(model, fe, cross_kv_dtype=dt, **kw)(audios, spk))
            recs.append(list(rec))
        assert len(outs[0][1]) == 6 and len({len(r) for r in outs[0][0]}) > 1
        n = judge(model.engine, recs[0], recs[1], f"labeller continuous={continuous}", suppress=gd.SUPPRESS)
        assert n or outs[0] == outs[1]
    long_audios = [0.1 * rng.standard_normal(n).astype(np.float32) for n in (1_100_000, 480_000, 700_000)]
    for continuous in (False, True):
        kw = dict(batch_size=2, chunk_length_s=30.0, max_new_tokens=9, prompt_ids=ts.PROMPT, eos_token_id=gd.EOS,
                  suppress_tokens=gd.SUPPRESS, use_graphs=False, continuous=continuous, check_every=3)
        outs, recs = [], []
        for dt in (None, "fp8"):
            del rec[:]
            served[0] = 0
            outs.append(LongFormTranscriber(model, fe, cross_kv_dtype=dt, **kw)(long_audios))
            recs.append(list(rec))
        assert len(outs[0]) == 3 and any(outs[0])
        n = judge(model.engine, recs[0], recs[1], f"transcriber continuous={continuous}", suppress=gd.SUPPRESS)
        assert n or outs[0] == outs[1]


def test_the_entries_are_declared_and_bound():
    import os
    from distil_whisper_amd import build, ops_hip
    header = open(os.path.join(os.path.dirname(os.path.abspath(ops_hip.__file__)), "..", "include", "dwamd.h")).read()
    for name in ("dw_cross_kv_quant", "dw_decode_attn_proj_kv8"):
        assert f"int {name}(" in header and name in ops_hip.EXPORTED_SYMBOLS
    assert "cross_kv8.hip" in build.SOURCES
    for method in ("cross_kv_quant", "decode_attn_proj_kv8"):
        assert hasattr(ops_hip.HipOps, method)
    fields = [f for f, _ in ops_hip.DwDecoderLayer._fields_]
    assert fields[-3:] == ["cross_k8", "cross_v8", "cross_scale"] and ops_hip.DwDecodeStep._fields_[-1][0] == "cross_kv_fmt"
