"""Continuous batching on the MI355X.

* `dw_decode_attn_proj_rows` alone: for every row b the output o[b] and the whole cache of the row -- the K/V row appended at
  row_t[b] and the canary pattern everywhere else -- equal, bit for bit, what `dw_decode_attn_proj(mode=1)` writes when called on
  that single row with Lk = row_t[b] + 1.  Key counts mixed in one launch from 1, 2, 8, 9 (the 8-key group), 63, 64, 65 (the 64-key
  sweep of the 8 waves), 511, 512, 513 (the 512-key outer step), a row at 1 key beside a row at 513, the last row of the cache, a
  padded K/V pitch, a host bound above every row.  Every refusal returns its code and writes nothing.
* `dw_decode_token_rows` under `dw_debug_set(7, 0)` -- the self-attention fusion on, which the default key (4) has off: there the
  entry is the pass of `dw_decode_step_rows`, checked as such -- against `dw_decode_step`: equal positions give the uniform step's
  logits and caches bit for bit, mixed positions give row b the uniform step's logits and cache row at t = row_t[b].
* `dw_slot_step` against the numpy restatement on the planted launches of tests/slots_cases.py; integers are exact.
* `SlotDecoder` on the tiny planted model of tests/test_slots.py in bf16: every window against `GreedyDecoder` at the same batch
  size under the near-tie rule of tests/test_assist_rows_gpu.py, graph replay against eager, fewer steps than the batch path,
  `PseudoLabeller` / `LongFormTranscriber` with `continuous=True` against themselves without it."""

import pytest
import torch

from oracle import gen_golden_decode as gd
from tests import slots_cases as sc
from tests.test_assist_rows import EXACT_ULPS
from tests.test_slots import PROMPT, batch_path_steps, greedy_rows, make_windows, planted_target

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EINVAL, EUNSUP = -1, -2
KEY7_DEFAULT = 4


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps(DEV)


@pytest.fixture()
def key7(ops):
    def set_key(value):
        assert ops.lib.dw_debug_set(7, value) == 0
    yield set_key
    ops.lib.dw_debug_set(7, KEY7_DEFAULT)


def bits(t):
    return t.contiguous().view(torch.int16)


# ---- dw_decode_attn_proj_rows ---------------------------------------------------------------------------------------------------
KV_ROWS = 520
ROW_KEYS = [((1, 2, 8), None, 0), ((9, 63, 64), None, 0), ((65, 511, 512), None, 64), ((513, 1, KV_ROWS), None, 0),
            ((1, 513, 64), KV_ROWS - 1, 0), ((2, 65, 9), 300, 64)]                  # (key counts per row, host bound or None, pitch pad)


def proj_inputs(D, dt, B, pad, seed):
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(B, D).to(DEV).to(dt)
    ln_g, ln_b = (1.0 + 0.1 * rnd(D)).to(DEV), (0.1 * rnd(D)).to(DEV)
    w = (rnd(3 * D, D) / D ** 0.5).to(DEV).bfloat16()
    bias = (0.1 * rnd(3 * D)).to(DEV)
    cache = (0.5 * rnd(B * KV_ROWS, 2 * D + pad)).to(DEV).bfloat16()               # history below row_t, the canary everywhere else
    return x, ln_g, ln_b, w, bias, cache


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("D", [384, 1280])
def test_rows_kernel_equals_the_uniform_kernel_on_every_row_alone(ops, D, dt):
    B, H = 3, D // 64
    for i, (keys, bound, pad) in enumerate(ROW_KEYS):
        x, ln_g, ln_b, w, bias, base = proj_inputs(D, dt, B, pad, 10 * i + D)
        row_t = torch.tensor([k - 1 for k in keys], dtype=torch.int32, device=DEV)
        cache = base.clone()
        max_t = max(keys) - 1 if bound is None else bound
        o = ops.decode_attn_proj_rows(x, ln_g, ln_b, w, bias, cache[:, :D], cache[:, D:2 * D], B, H, row_t, max_t, kv_rows=KV_ROWS,
                                      kv_app=cache)
        torch.cuda.synchronize()
        for b, Lk in enumerate(keys):
            one = base[b * KV_ROWS:(b + 1) * KV_ROWS].clone()
            ob = ops.decode_attn_proj(1, x[b:b + 1], ln_g, ln_b, w, bias, one[:, :D], one[:, D:2 * D], 1, H, Lk, kv_rows=KV_ROWS, kv_app=one)
            torch.cuda.synchronize()
            assert torch.equal(bits(o[b]), bits(ob[0])), (keys, b, "o")
            got = cache[b * KV_ROWS:(b + 1) * KV_ROWS]
            assert torch.equal(bits(got), bits(one)), (keys, b, "cache")
            keep = torch.ones(KV_ROWS, dtype=torch.bool, device=DEV)
            keep[Lk - 1] = False
            assert torch.equal(bits(got[keep]), bits(base[b * KV_ROWS:(b + 1) * KV_ROWS][keep])), (keys, b, "canary")
            assert not torch.equal(bits(got[Lk - 1, :2 * D]), bits(base[b * KV_ROWS + Lk - 1, :2 * D])), (keys, b, "nothing appended")


def test_rows_kernel_refusals_return_their_codes_and_write_nothing(ops):
    from distil_whisper_amd.ops_hip import DW_BF16, DW_F32
    D, H, B, kv_rows = 384, 6, 2, 12
    x, ln_g, ln_b, w, bias, _ = proj_inputs(D, torch.float32, B, 0, 1)
    pitch = 2 * D + 16
    kv = torch.full((B * kv_rows, pitch), 3.0, dtype=torch.bfloat16, device=DEV)
    big = torch.full((9000, 2 * D), 3.0, dtype=torch.bfloat16, device=DEV)
    o = torch.full((B, D), 3.0, dtype=torch.bfloat16, device=DEV)
    rt = torch.zeros(B + 1, dtype=torch.int32, device=DEV)
    good = dict(x=x.data_ptr(), x_dtype=DW_F32, ldx=D, ln_g=ln_g.data_ptr(), ln_b=ln_b.data_ptr(), eps=1e-5, w=w.data_ptr(),
                bias=bias.data_ptr(), k=kv.data_ptr(), v=kv.data_ptr() + 2 * D, ldkv=pitch, kv_rows=kv_rows, kv_app=kv.data_ptr(),
                o=o.data_ptr(), ldo=D, B=B, H=H, scale=0.125, row_t=rt.data_ptr(), max_t=8)

    def call(**over):
        a = dict(good, **over)
        return ops.lib.dw_decode_attn_proj_rows(a["x"], a["x_dtype"], a["ldx"], a["ln_g"], a["ln_b"], a["eps"], a["w"], a["bias"], a["k"],
                                                a["v"], a["ldkv"], a["kv_rows"], a["kv_app"], a["o"], a["ldo"], a["B"], a["H"], a["scale"],
                                                a["row_t"], a["max_t"], ops._stream())
    bad = [(EINVAL, dict(row_t=None)), (EINVAL, dict(row_t=rt.data_ptr() + 2)), (EINVAL, dict(max_t=kv_rows)), (EINVAL, dict(max_t=-1)),
           (EUNSUP, dict(max_t=8192, kv_rows=9000, k=big.data_ptr(), v=big.data_ptr() + 2 * D, kv_app=big.data_ptr(), ldkv=2 * D, B=1)),
           # the refusals of the uniform entry
           (EINVAL, dict(x_dtype=2)), (EINVAL, dict(x=None)), (EINVAL, dict(kv_app=None)), (EINVAL, dict(B=0)), (EINVAL, dict(x=x.data_ptr() + 4)),
           (EINVAL, dict(ldkv=pitch + 4)), (EINVAL, dict(bias=bias.data_ptr() + 2)), (EUNSUP, dict(H=5)), (EUNSUP, dict(B=65536)),
           (EINVAL, dict(ldx=D - 8)), (EINVAL, dict(ldo=D - 1)), (EINVAL, dict(ldkv=2 * D - 8))]
    for code, over in bad:
        assert call(**over) == code, over
    torch.cuda.synchronize()
    assert bool((kv == 3.0).all()) and bool((big == 3.0).all()) and bool((o == 3.0).all())
    assert call(max_t=kv_rows - 1) == 0                                     # the largest bound that fits
    torch.cuda.synchronize()
    assert bool(torch.isfinite(o.float()).all()) and not bool((o == 3.0).all())


# ---- dw_decode_token_rows -------------------------------------------------------------------------------------------------------
def _engine(ops, dims, seed):
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    sd = {k: v.to(torch.bfloat16).float() for k, v in si.random_state_dict(dims, seed, ops.device).items()}
    return WhisperForConditionalGeneration(dims, ops=ops, state_dict=sd, dtype=torch.bfloat16).engine


@pytest.fixture(scope="module")
def tiny(ops):
    from distil_whisper_amd.engine import WhisperDims
    return _engine(ops, WhisperDims(384, 6, 1536, 1, 2, 51865, 80, max_src=128), 3)    # Whisper tiny's width: the narrowest with the kernel


@pytest.fixture(scope="module")
def wide(ops):
    from distil_whisper_amd.engine import WhisperDims
    return _engine(ops, WhisperDims(1280, 20, 5120, 1, 2, 51866, 128, max_src=128), 5)


def _fresh(cache, selfs, t):
    return {"B": cache["B"], "max_len": cache["max_len"], "t": t, "cross": cache["cross"], "self": [s.clone() for s in selfs]}


def check_token_rows(ops, eng, B, row_t, max_len, seed, key):
    """Under key 7 = `key`: 0 -- dw_decode_token_rows against dw_decode_step, bit for bit; 4 -- against dw_decode_step_rows."""
    d = eng.dims
    D = d.d_model
    g = torch.Generator().manual_seed(seed)
    enc = (torch.randn(B * d.max_src, D, generator=g) * 0.5).to(DEV).bfloat16()
    ids = torch.randint(0, d.vocab, (B, 1), generator=g).to(DEV)
    cache = eng.decode_init(enc, B, max_len)
    base = [(torch.randn(B * max_len, 2 * D, generator=g) * 0.5).to(DEV).bfloat16() for _ in cache["self"]]
    rt = torch.tensor(row_t, dtype=torch.int32, device=DEV)
    c1 = _fresh(cache, base, 0)
    got = eng.decode_token_rows(ids, c1, rt, max(row_t))[:B, :d.vocab].clone()
    torch.cuda.synchronize()
    assert bool(torch.isfinite(got.float()).all())
    if key == 4:
        c2 = _fresh(cache, base, 0)
        want = eng.decode_multi_rows(ids, c2, rt, max(row_t))[:B, :d.vocab].clone()
        assert torch.equal(bits(got), bits(want))
        for a, b in zip(c1["self"], c2["self"]):
            assert torch.equal(bits(a), bits(b))
        return
    for t in sorted(set(row_t)):
        c2 = _fresh(cache, base, t)
        uni = eng.decode_step(ids, c2)[:B, :d.vocab].clone()
        torch.cuda.synchronize()
        for b in [b for b, tb in enumerate(row_t) if tb == t]:
            assert torch.equal(bits(got[b]), bits(uni[b])), (row_t, b, "logits")
            for l, (a, u) in enumerate(zip(c1["self"], c2["self"])):
                a3, u3 = a.view(B, max_len, 2 * D)[b], u.view(B, max_len, 2 * D)[b]
                assert torch.equal(bits(a3), bits(u3)), (row_t, b, l, "cache")     # the new row and the untouched rows of row b


@pytest.mark.parametrize("key", [0, 4])
@pytest.mark.parametrize("B", [3, 18])
def test_token_rows_equal_the_uniform_step_tiny(ops, tiny, key7, B, key):
    key7(key)
    max_len = 160
    mixed = [0, 63, max_len - 1, 64, 5, 65, 8, 1, 127, 128, 129, 7, 9, 31, 32, 33, 2, 100][:B]
    for i, row_t in enumerate(([70] * B, [0] * B, mixed)):
        check_token_rows(ops, tiny, B, row_t, max_len, 100 * B + i, key)


@pytest.mark.parametrize("key", [0, 4])
@pytest.mark.parametrize("B", [3, 18])
def test_token_rows_equal_the_uniform_step_at_distil_large_v3_width(ops, wide, key7, B, key):
    key7(key)
    max_len = 128
    mixed = [0, 63, max_len - 1, 64, 5, 65, 8, 1, 126, 100, 37, 7, 9, 31, 32, 33, 2, 58][:B]
    for i, row_t in enumerate(([41] * B, mixed)):
        check_token_rows(ops, wide, B, row_t, max_len, 200 * B + i, key)


def test_token_rows_refuses_more_than_one_new_token(ops, tiny):
    import ctypes as C
    eng = tiny
    d = eng.dims
    B, max_len = 2, 32
    cache = eng.decode_init(torch.zeros((B * d.max_src, d.d_model), dtype=torch.bfloat16, device=DEV), B, max_len)
    rt = torch.zeros(B, dtype=torch.int32, device=DEV)
    s = C.c_void_p(torch.cuda.current_stream(DEV).cuda_stream)
    for n, want in ((2, EINVAL), (1, 0)):
        desc, ws, _, _ = eng._decode_desc(cache, n)
        ids = torch.zeros((B, n), dtype=torch.long, device=DEV)
        desc.ids = ids.data_ptr()
        ws["logits"].fill_(3.0)
        assert ops.lib.dw_decode_token_rows(C.byref(desc), rt.data_ptr(), 10, s) == want
        assert ops.lib.dw_decode_token_rows(C.byref(desc), None, 10, s) == EINVAL
        assert ops.lib.dw_decode_token_rows(C.byref(desc), rt.data_ptr(), max_len, s) == EINVAL
        torch.cuda.synchronize()
        assert bool((ws["logits"] == 3.0).all()) == (want != 0)


# ---- dw_slot_step ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ts", [False, True])
@pytest.mark.parametrize("V,ld", [(1030, 1032), (51865, 51872), (51866, 51868)])
def test_slot_step_kernel_matches_the_restatement(ops, V, ld, ts):
    from distil_whisper_amd.decoding import token_mask
    c = sc.make_launch(V, ts)
    S = c["tokens"].shape[0]
    lg = torch.full((S, ld), 50.0, dtype=torch.bfloat16, device=DEV)                # (a pad column would win if read)
    lg[:, :V] = torch.from_numpy(c["logits"]).to(DEV).bfloat16()
    tokens = torch.from_numpy(c["tokens"]).to(DEV)
    length, plen, budget = (torch.from_numpy(c[k]).to(torch.int32).to(DEV) for k in ("length", "plen", "budget"))
    done = torch.from_numpy(c["done"]).to(DEV)
    row_t, cur = torch.full((S,), -5, dtype=torch.int32, device=DEV), torch.full((S, 1), -5, dtype=torch.long, device=DEV)
    r = c["ts"]
    ops.slot_step(lg, V, tokens, length, plen, budget, done, row_t, cur, suppress=token_mask(c["suppress"], V, DEV, torch.uint8),
                  begin_suppress=token_mask(c["begin_suppress"], V, DEV, torch.uint8),
                  ts_begin=-1 if r is None else r["no_timestamps_token_id"] + 1, max_initial=-1 if r is None else r["max_initial_timestamp_index"],
                  eos=c["eos"], min_new=c["min_new"])
    torch.cuda.synchronize()
    sc.check_launch(c, tokens.cpu().numpy(), length.tolist(), done.tolist(), row_t.tolist(), cur.cpu().numpy())
    assert plen.tolist() == c["plen"].tolist() and budget.tolist() == c["budget"].tolist()


def test_slot_step_refusals_write_nothing(ops):
    V, S = 1030, 2
    lg = torch.zeros((S, 1032), dtype=torch.bfloat16, device=DEV)
    tokens = torch.full((S, 8), 3, dtype=torch.long, device=DEV)
    st = torch.full((5, 4), 2, dtype=torch.int32, device=DEV)
    done = torch.zeros(S, dtype=torch.bool, device=DEV)
    cur = torch.full((S, 1), 3, dtype=torch.long, device=DEV)
    good = dict(logits=lg.data_ptr(), S=S, V=V, ld=1032, ts_begin=-1, eos=900, tokens=tokens.data_ptr(), tok_ld=8, len=st[0].data_ptr(),
                plen=st[1].data_ptr(), budget=st[2].data_ptr(), done=done.data_ptr(), row_t=st[3].data_ptr(), cur=cur.data_ptr())

    def call(**over):
        a = dict(good, **over)
        return ops.lib.dw_slot_step(a["logits"], a["S"], a["V"], a["ld"], None, None, a["ts_begin"], -1, a["eos"], 0, a["tokens"],
                                    a["tok_ld"], a["len"], a["plen"], a["budget"], a["done"], a["row_t"], a["cur"], ops._stream())
    for over in (dict(logits=None), dict(S=0), dict(V=0), dict(ld=1028), dict(ld=1033), dict(logits=lg.data_ptr() + 2), dict(tokens=None),
                 dict(len=None), dict(plen=None), dict(budget=None), dict(done=None), dict(row_t=None), dict(cur=None), dict(tok_ld=1),
                 dict(len=st[0].data_ptr() + 2), dict(ts_begin=1000, eos=-1)):
        assert call(**over) == EINVAL, over
    torch.cuda.synchronize()
    assert bool((tokens == 3).all()) and bool((st == 2).all()) and bool((cur == 3).all()) and not bool(done.any())


# ---- the scheduler --------------------------------------------------------------------------------------------------------------
def margins_of_greedy(monkeypatch, ops):
    """Spy on `greedy_select` of the reference decode: the smallest gap between the selection and the runner-up over live rows, in
    bf16 ulps of the best score."""
    from distil_whisper_amd.decoding import processed_scores
    seen = []
    orig = type(ops).greedy_select

    def spy(self, logits, V, tokens, n, cur, **k):
        if not k.get("forced"):
            r = None if k.get("ts_begin", -1) < 0 else dict(no_timestamps_token_id=k["ts_begin"] - 1,
                                                            max_initial_timestamp_index=None if k["max_initial"] < 0 else k["max_initial"])
            s = processed_scores(logits[:tokens.shape[0], :V], tokens, n, begin_index=k.get("begin_index", 1), eos=k.get("eos"),
                                 no_eos=k.get("no_eos", False), first=k.get("first", False), suppress=k.get("suppress"),
                                 begin_suppress=k.get("begin_suppress"), timestamp_rules=r)
            top = s.topk(2, -1).values[0]                                  # (row 0: the window under test)
            if not bool(k["done"][0]):
                seen.append(((top[0] - top[1]) / torch.exp2(torch.floor(torch.log2(top[0].abs().clamp(min=1e-30))) - 7)).item())
        return orig(self, logits, V, tokens, n, cur, **k)
    monkeypatch.setattr(type(ops), "greedy_select", spy)
    return seen


def compare_windows(monkeypatch, ops, model, windows, S, got, **kw):
    tried = exact = 0
    want = {}
    for w in windows:
        seen = margins_of_greedy(monkeypatch, ops)
        want.update(greedy_rows(model.engine, [w], S, gd.EOS, **kw))
        monkeypatch.undo()
        tried += 1
        margin = min(seen)
        if margin <= EXACT_ULPS:                                            # (<= 0: an exactly tied selection)
            print(f"window {w[0]}: margin {margin:.1f} ulps, not held to equality")
            continue
        assert got[w[0]] == want[w[0]], (w[0], margin)
        exact += 1
    print(f"windows tried {tried}, compared {exact}")
    assert exact >= 1 and 2 * (tried - exact) <= tried
    return want


@pytest.mark.parametrize("width,key,n_windows,S,check_every", [(128, 4, 7, 3, 2), (128, 4, 5, 2, 8), (128, 4, 1, 3, 4), (128, 4, 0, 3, 4),
                                                               (384, 0, 7, 3, 2), (384, 4, 7, 3, 2), (384, 0, 5, 2, 8)])
def test_slot_decoder_rows_equal_the_batch_decoder_and_graphs_equal_eager(ops, monkeypatch, key7, width, key, n_windows, S, check_every):
    """width 128 has no token-step attention with the projection inside: the pass is dw_decode_step_rows' under either key.  At 384
    key 0 runs the per-row kernel, the default key (4) the separate launches."""
    from distil_whisper_amd.decoding import SlotDecoder
    model, enc = planted_target(ops, dtype=torch.bfloat16, width=width)
    enc = enc.to(DEV).bfloat16()
    windows = make_windows(enc, n_windows, model.dims.max_src)
    runs = {}
    key7(key)
    for name, graphs in (("eager", False), ("graphs", True)):
        dec = SlotDecoder(model.engine, S, len(PROMPT) + 2 + 9, gd.EOS, suppress_tokens=gd.SUPPRESS, check_every=check_every,
                          use_graphs=graphs)
        runs[name] = {k: r.tolist() for k, r in dec.run(iter(windows))}
        assert len(runs[name]) == n_windows
        steps = dec.steps
        if graphs and n_windows:
            assert len(dec.graphs) >= 1
            assert {k: r.tolist() for k, r in dec.run(iter(windows))} == runs[name]           # replay over the same buffers
            assert dec.steps == 2 * steps
    assert runs["eager"] == runs["graphs"]
    if not n_windows:
        return
    want = compare_windows(monkeypatch, ops, model, windows, S, runs["graphs"], suppress_tokens=gd.SUPPRESS)
    if n_windows > S and check_every <= 2:
        assert steps < batch_path_steps(windows, S, gd.EOS, want)


def test_labeller_and_transcriber_continuous_on_the_device(ops, monkeypatch):
    from distil_whisper_amd.longform import LongFormTranscriber
    from distil_whisper_amd.modeling import WhisperFeatureExtractor, WhisperForConditionalGeneration
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    from tests.test_assist_gpu import peaked
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=False)
    P, eos = len(PROMPT), gd.EOS
    seq = [50, 61, 72, 83, 94, 105, eos, 116]
    model = WhisperForConditionalGeneration(gd.CFG_T, ops=ops, state_dict=peaked(gd.weights(77), P, seq, 100.0), dtype=torch.bfloat16)
    fe = WhisperFeatureExtractor(feature_size=80, ops=ops)
    kw = dict(batch_size=2, max_new_tokens=8, prompt_ids=PROMPT, eos_token_id=eos, suppress_tokens=fields["suppress_tokens"],
              begin_suppress_tokens=fields["begin_suppress_tokens"])
    audios = [gd.audio(30 + i, n) for i, n in enumerate((150_000, 200_000, 100_000, 300_000, 250_000))]
    speakers = (0, 0, 0, 1, 2)
    want = PseudoLabeller(model, fe, **kw)(audios, speakers)
    for graphs in (False, True):
        lab = PseudoLabeller(model, fe, continuous=True, check_every=2, use_graphs=graphs, **kw)
        assert lab(audios, speakers) == want and lab.slot_decoder.steps > 0
    assert all(row == seq[:seq.index(eos)] for row in want[0])
    long_audio = [gd.audio(40, 1_100_000), gd.audio(41, 480_000)]
    for extra in ({}, dict(return_timestamps=True, no_timestamps_token_id=gd.NOTIMESTAMPS)):
        tkw = dict(kw, prompt_ids=PROMPT[:3] if extra else PROMPT, chunk_length_s=30.0, **extra)
        ref = LongFormTranscriber(model, fe, **tkw)(long_audio)
        assert LongFormTranscriber(model, fe, continuous=True, check_every=3, **tkw)(long_audio) == ref
