"""Speculative (assisted) decoding on the MI355X: the kernels of csrc/assist.hip against the float64 restatement on planted
rounds, `assist_pick(store=True)` against `greedy_select`, and the device-state rounds of `assisted_greedy_decode` against its
torch rounds (DW_ASSIST_TORCH=1) and against plain greedy decoding.

Equal scores: both paths of `assisted_greedy_decode` see the same bf16 logits, so their tokens can differ only where the best two
processed scores of a drafted or verified position are exactly equal (torch.argmax's order among equals is unspecified on the
device; the kernels take the lower column).  The torch leg reports, per selection, best minus runner-up of the raw logits; inputs
with a zero margin are not compared, and at most half of the inputs tried may go that way.  Against plain greedy decoding the
logits themselves come from another launch sequence (the multi-token verify pass against the token step): each rounds its fp32
LM-head sum to bf16 once (half an ulp each) over activations that may differ by one bf16 ulp (engine._decoder_layers_cached), so a
selection can turn only below a few ulps of the scores' magnitude; inputs are compared when every margin exceeds EXACT_ULPS = 4
LARGE_PEAK = 1000.0                                       # `peaked` at d_model 1280 (the layers' outputs are larger there)
bf16 ulps of the best score.

The models of these two tests have peaked logits (`peaked` below): with seeded random weights alone the logits are nearly flat,
most inputs hold an exactly tied selection somewhere among their ~100 selections and none keeps 8 emitted tokens 4 ulps apart
(measured on the MI355X: 2-5 of 6 inputs tied, 0 of 6 above the margin), so neither cap could be met by any implementation."""
import numpy as np
import pytest
import torch

from oracle import gen_golden_decode as gd
from tests import assist_cases as ac
from tests.assist_restatement import accept_ref

pytestmark = pytest.mark.gpu
EXACT_ULPS = 4
LARGE_PEAK = 1000.0                                       # `peaked` at d_model 1280 (the layers' outputs are larger there)


@pytest.fixture(scope="module")
def ops():
    from distil_whisper_amd.ops_hip import HipOps
    return HipOps("cuda:0")


def planted(V, B, k, name, sc):
    for seed in range(40):
        try:
            return ac.make_case(1000 * seed + 17 * B + k + len(name), V, B, k, sc)
        except AssertionError:
            continue
    raise AssertionError(f"no clear-margin case for {name}")


def device_round(ops, c, ld):
    """One verify round through the two entries -> (own, tokens, done, result) as numpy."""
    dev = ops.device
    B, n, V = c["logits"].shape
    L, k = c["L"], c["k"]
    rows = n + 2                                           # the pass scored more rows than the k + 1 that are read
    lg = torch.full((B * rows, ld), 50.0, dtype=torch.bfloat16, device=dev)        # (pad columns / rows would win if read)
    lg.view(B, rows, ld)[:, 2:, :V] = torch.from_numpy(c["logits"]).to(dev).to(torch.bfloat16)
    tokens = torch.from_numpy(c["tokens"]).to(dev)
    own = torch.full((B, n + 1), -5, dtype=torch.long, device=dev)
    done = torch.from_numpy(c["done"]).to(dev)
    result = torch.full((2,), -9, dtype=torch.int32, device=dev)
    sup = None
    if c["suppress"]:
        sup = torch.zeros(V, dtype=torch.uint8, device=dev)
        sup[torch.tensor(c["suppress"], device=dev)] = 1
    ts = c["ts"]
    ops.assist_pick(lg[2:], V, tokens, L, own, n=n, batch_rows=rows, suppress=sup, min_new=c["min_new"],
                    ts_begin=-1 if ts is None else ts["no_timestamps_token_id"] + 1,
                    max_initial=-1 if ts is None else ts["max_initial_timestamp_index"], begin_index=c["P0"], eos=c["eos"])
    ops.assist_accept(own, tokens, L, k, result, eos=c["eos"], fill=c["fill"], done=done)
    torch.cuda.synchronize()
    return own.cpu().numpy(), tokens.cpu().numpy(), done.cpu().numpy(), result.cpu().numpy()


def check_case(ops, c, ld, name):
    L, k = c["L"], c["k"]
    tok_ref, done_ref, n_ref, all_ref = accept_ref(c["own"], c["tokens"], L, k, c["done"], c["eos"], c["fill"])
    own, tokens, done, result = device_round(ops, c, ld)
    assert own[:, :k + 1].tolist() == c["own"].tolist(), name
    assert (own[:, k + 1:] == -5).all()
    assert result.tolist() == [n_ref, int(all_ref)], name
    assert tokens[:, L:L + n_ref + 1].tolist() == tok_ref[:, L:L + n_ref + 1].tolist(), name
    assert done.tolist() == done_ref.tolist(), name
    assert np.array_equal(tokens[:, :L], c["tokens"][:, :L]), name                         # in front of L: untouched
    assert np.array_equal(tokens[:, L + n_ref + 1:], c["tokens"][:, L + n_ref + 1:]), name   # behind L + n_ok: untouched


@pytest.mark.parametrize("V,ld", [(1030, 1032), (51865, 51872), (51866, 51868), (53252, 53312)])
def test_kernels_match_the_restatement_on_planted_rounds(ops, V, ld):
    small = V < 2000
    for B in (1, 3):
        for k in ((0, 1, 5) if small else (5,)):
            for name, sc in ac.scenarios(B, k).items():
                if not small and (B, name) not in ((3, "rows_differ"), (3, "done_row"), (1, "eos_accepted"), (3, "min_new_inside"),
                                                   (1, "suppress"), (3, "ts_first"), (1, "ts_text_ts"), (3, "ts_pair"),
                                                   (3, "ts_open"), (1, "ts_mass_taken"), (3, "ts_mass_not_taken")):
                    continue
                check_case(ops, planted(V, B, k, name, sc), ld, (V, B, k, name))


def test_two_equal_best_values_go_to_the_lower_column(ops):
    sc = ac.scenarios(2, 1)["all_accepted"]
    for V, ld in ((1030, 1032), (53252, 53312)):
        c = planted(V, 2, 1, "all_accepted", sc)
        for b in range(2):
            for j in range(2):
                w = int(c["own"][b, j])
                hi, lo = w + 4099, w - 5                  # the same value in another thread's chunk, above and below
                c["logits"][b, j, hi if hi < c["eos"] else lo] = c["logits"][b, j, w]
                if hi >= c["eos"]:
                    c["own"][b, j] = lo
        # (the drafts were derived before the twins were planted: row agreement may change, the restated accept follows `own`)
        check_case(ops, c, ld, V)


def test_draft_step_equals_greedy_select(ops):
    """`assist_pick(n=1, store=True)` against `greedy_select` on the same rows (no row done): one statement of the rules."""
    dev = ops.device
    for V, ld in ((1030, 1032), (51866, 51868)):
        for name in ("all_accepted", "suppress", "min_new_inside", "ts_first", "ts_text_ts", "ts_pair", "ts_open", "ts_mass_taken"):
            c = planted(V, 3, 0, name, ac.scenarios(3, 0)[name])
            B, L, ts = 3, c["L"], c["ts"]
            lg = torch.zeros((B, ld), dtype=torch.bfloat16, device=dev)
            lg[:, :V] = torch.from_numpy(c["logits"][:, 0]).to(dev).to(torch.bfloat16)
            sup = None
            if c["suppress"]:
                sup = torch.zeros(V, dtype=torch.uint8, device=dev)
                sup[torch.tensor(c["suppress"], device=dev)] = 1
            kw = dict(ts_begin=-1 if ts is None else ts["no_timestamps_token_id"] + 1,
                      max_initial=-1 if ts is None else ts["max_initial_timestamp_index"], begin_index=c["P0"], eos=c["eos"])
            t1, t2 = torch.from_numpy(c["tokens"]).to(dev), torch.from_numpy(c["tokens"]).to(dev)
            cur1, cur2 = torch.zeros((B, 1), dtype=torch.long, device=dev), torch.zeros((B, 1), dtype=torch.long, device=dev)
            own = torch.zeros((B, 1), dtype=torch.long, device=dev)
            ops.assist_pick(lg, V, t1, L, own, n=1, suppress=sup, min_new=c["min_new"], store=True, cur=cur1, **kw)
            ops.greedy_select(lg, V, t2, L, cur2, suppress=sup, first=(L == c["P0"]), no_eos=(L - c["P0"]) < c["min_new"],
                              fill=c["fill"], done=torch.zeros(B, dtype=torch.bool, device=dev), **kw)
            assert torch.equal(t1, t2) and torch.equal(cur1, cur2) and torch.equal(own, cur1), (V, name)
            assert own[:, 0].tolist() == c["own"][:, 0].tolist()


# ---- the rounds through assisted_greedy_decode -------------------------------------------------------------------------------------
def _run(monkeypatch, torch_path, target, assistant, enc, prompt, max_new, k, margins=None, calls=None, **kw):
    from distil_whisper_amd import decoding
    monkeypatch.setenv(decoding.ASSIST_TORCH_ENV, "1" if torch_path else "0")
    if margins is not None:                               # best minus runner-up of the raw logits at every selection of the torch leg
        orig = decoding.assist_pick_torch

        def spy(logits, *a, **k2):
            own = orig(logits, *a, **k2)
            lg = logits.float()
            best = lg.gather(-1, own[..., None])
            second = orig(lg.scatter(-1, own[..., None], float("-inf")), *a, **k2)
            gap = (best - lg.gather(-1, second[..., None]))[..., 0]
            margins.append((gap / torch.exp2(torch.floor(torch.log2(best[..., 0].abs().clamp(min=1e-30))) - 7)).min().item())
            return own
        monkeypatch.setattr(decoding, "assist_pick_torch", spy)
    if calls is not None:
        for name in ("assist_pick", "assist_accept"):
            fn = getattr(type(target.ops), name)

            def counted(self, *a, _fn=fn, _name=name, **k2):
                calls[_name] = calls.get(_name, 0) + 1
                return _fn(self, *a, **k2)
            monkeypatch.setattr(type(target.ops), name, counted)
    out = decoding.assisted_greedy_decode(target, assistant, enc, enc, prompt, max_new, k, **kw)
    monkeypatch.undo()
    return out[0].tolist(), out[1], out[2]


def _selected(tried, checked):
    print(f"inputs tried {tried}, compared {checked}, rejected {tried - checked}")
    assert checked >= 1 and 2 * (tried - checked) <= tried


def _compare_paths(monkeypatch, target, assistant, encs, prompt, max_new, k, plain=None, **kw):
    """Kernel rounds against torch rounds on the inputs without an exactly tied selection; with `plain` (a function enc ->
    sequences of plain greedy decoding) also against it where every margin exceeds EXACT_ULPS."""
    tried = same = exact = 0
    results = []
    for enc in encs:
        margins, calls = [], {}
        tried += 1
        want = _run(monkeypatch, True, target, assistant, enc, prompt, max_new, k, margins=margins, **kw)
        if min(margins) <= 0.0:
            continue
        got = _run(monkeypatch, False, target, assistant, enc, prompt, max_new, k, calls=calls, **kw)
        assert got == want
        assert calls.get("assist_pick", 0) > 0 and calls.get("assist_accept", 0) > 0
        same += 1
        results.append(got)
        if plain is not None and min(margins) > EXACT_ULPS:
            ref = plain(enc)                               # (the rounds stop once every row is done: the rest is pad)
            for g, r in zip(got[0], ref):
                assert r[:len(g)] == g and all(t == kw.get("pad_token_id") for t in r[len(g):])
            exact += 1
    _selected(tried, same)
    if plain is not None:
        _selected(tried, exact)
    return results


def peaked(sd, P, seq, c):
    """The state dict with the decoder position rows P - 1 .. set to c x the embedding of seq[0], seq[1], ...: the position
    dominates the residual stream, so the tied LM head's best column at the step that predicts generated token i is seq[i], far
    above the rest (|E|^2 against |E| x a few sigma), wherever the rules allow it.  Seeded random weights alone have nearly flat
    logits: among the ~100 selections of a decode two best bf16 scores are exactly equal in most inputs (measured: 2-5 of 6), and no
    input keeps 8 emitted tokens EXACT_ULPS apart -- such models cannot meet the selection cap, a trained-like peaked one does."""
    sd = dict(sd)
    pos, E = sd["model.decoder.embed_positions.weight"].clone(), sd["model.decoder.embed_tokens.weight"]
    for i, t in enumerate(seq):
        pos[P - 1 + i] = c * E[t].to(pos.dtype)
    sd["model.decoder.embed_positions.weight"] = pos
    return sd


@pytest.mark.parametrize("timestamps", [False, True])
@pytest.mark.parametrize("B", [1, 2])
@pytest.mark.parametrize("k", [1, 5])
def test_kernel_rounds_equal_torch_rounds_and_plain_greedy_tiny(ops, monkeypatch, timestamps, B, k):
    """The tiny model of the decode fixtures with peaked positions (`peaked`): the target emits a sequence that walks through the
    timestamp states and ends in EOS before the budget does; the decoder-only student agrees with it except at generated
    positions 2 and 5, so rounds accept all, some and none of their drafts."""
    from distil_whisper_amd.decoding import GreedyDecoder
    from distil_whisper_amd.modeling import WhisperForCausalLM, WhisperForConditionalGeneration
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=timestamps)
    ids = [gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE] + ([] if timestamps else [gd.NOTIMESTAMPS])
    P, eos, max_new, T0 = len(ids), gd.EOS, 8, gd.TS0
    seq_t = [T0 + 1, 50, 61, T0 + 5, T0 + 5, 72, T0 + 9, eos] if timestamps else [50, 61, 72, 83, 94, 105, eos, 116]
    seq_s = list(seq_t)
    seq_s[2], seq_s[5] = 400, 401
    sd_t = gd.weights(77)
    sd_s, cfg_s = gd.student(peaked(sd_t, P, seq_s, 100.0))
    teacher = WhisperForConditionalGeneration(gd.CFG_T, ops=ops, state_dict=peaked(sd_t, P, seq_t, 100.0), dtype=torch.bfloat16)
    causal = WhisperForCausalLM(cfg_s, ops=ops, state_dict=sd_s, dtype=torch.bfloat16)
    prompt = torch.tensor([ids] * B, device=ops.device)
    rules = dict(begin_index=P, no_timestamps_token_id=gd.NOTIMESTAMPS, max_initial_timestamp_index=50) if timestamps else None
    kw = dict(eos_token_id=eos, suppress_tokens=fields["suppress_tokens"], min_new_tokens=2, pad_token_id=eos,
              timestamp_rules=rules)
    encs = [teacher.engine.encode(gd.features(500 + s, B).to(ops.device), save=False)[0] for s in range(3)]
    dec = GreedyDecoder(teacher.engine, B, P + max_new, eos_token_id=eos, suppress_tokens=fields["suppress_tokens"],
                        timestamp_rules=rules, pad_token_id=eos, use_graphs=False)
    plain = lambda enc: dec.run(enc, prompt, max_new, min_new_tokens=2).tolist()
    stats = _compare_paths(monkeypatch, teacher.engine, causal.engine, encs, prompt, max_new, k, plain=plain, **kw)
    for seqs, drafted, accepted in stats:
        exp = seq_t[:seq_t.index(eos) + 1]                 # the planted sequence up to its EOS, then pad; partly drafted
        assert all(r[P:P + len(exp)] == exp and all(t == eos for t in r[P + len(exp):]) for r in seqs)
        assert 0 < accepted < drafted


def test_kernel_rounds_equal_torch_rounds_at_distil_large_v3_width(ops, monkeypatch):
    """d_model 1280, V = 51 866, a 4-layer target, 8 new tokens, peaked positions (`peaked`): (a) a second engine over the target's
    own weights drafts under the timestamp rules -- every draft is accepted --, (b) a 2-layer decoder-only assistant of another seed
    with a sequence of its own, no timestamp rules -- every draft is rejected."""
    import dataclasses
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForCausalLM, WhisperForConditionalGeneration
    d = WhisperDims(1280, 20, 5120, 1, 4, 51866, 128)
    d2 = dataclasses.replace(d, dec_layers=2)
    B, eos, P, T0 = 2, 50257, 3, 50365
    seq_t = [T0 + 3, 1000, 2000, T0 + 40, T0 + 40, 3000, 4000, 5000]
    seq_a = [1500, 2500, 3500, 4500, 5500, 6500, 7500, 8500]
    sd_t = peaked(si.random_state_dict(d, 5, ops.device), P, seq_t, LARGE_PEAK)
    teacher = WhisperForConditionalGeneration(d, ops=ops, state_dict=sd_t, dtype=torch.bfloat16)
    twin = WhisperForCausalLM(d, ops=ops, state_dict=sd_t, dtype=torch.bfloat16)
    other = WhisperForCausalLM(d2, ops=ops, state_dict=peaked(si.random_state_dict(d2, 6, ops.device), P, seq_a, LARGE_PEAK),
                               dtype=torch.bfloat16)
    prompt = torch.tensor([[50258, 50259, 50360]] * B, device=ops.device)
    g = torch.Generator().manual_seed(11)
    encs = [(torch.randn(B * d.max_src, d.d_model, generator=g) * 0.5).to(ops.device).to(torch.bfloat16) for _ in range(2)]
    rules = dict(begin_index=P, no_timestamps_token_id=50364, max_initial_timestamp_index=50)
    kw = dict(eos_token_id=eos, min_new_tokens=1, pad_token_id=eos, timestamp_rules=rules)
    acc = _compare_paths(monkeypatch, teacher.engine, twin.engine, encs, prompt, 8, 5, **kw)
    # (b) without the timestamp rules: behind a rejected draft of another token class they would ban the target's planted token,
    # and the verified position would fall back to the flat scores underneath, where equal best values are common
    kw = dict(eos_token_id=eos, min_new_tokens=1, pad_token_id=eos)
    rej = _compare_paths(monkeypatch, teacher.engine, other.engine, encs, prompt, 8, 5, **kw)
    print("accepted / drafted: twin", [(a, dr) for _, dr, a in acc], " other", [(a, dr) for _, dr, a in rej])
    assert all(a == dr > 0 and all(r[P:] == seq_t for r in s) for s, dr, a in acc)
    assert all(a == 0 < dr and all(r[P:] == seq_t for r in s) for s, dr, a in rej)


def test_fixture_assistant_scenarios_with_a_decoder_only_assistant(ops):
    import json
    import os
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForCausalLM, WhisperForConditionalGeneration
    gold = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode.json")))
    todo = [s for s in gold["scenarios"] if s.get("assistant") and s.get("kind") == "short" and not s.get("use_encoder_outputs")]
    assert todo
    for s in todo:
        sd_t = gd.weights(s["seed"])
        sd_s, cfg_s = gd.student(sd_t)
        teacher = WhisperForConditionalGeneration(gd.CFG_T, ops=ops, state_dict=sd_t)
        teacher.generation_config = GenerationConfig.from_any(s["generation_config"])
        causal = WhisperForCausalLM(cfg_s, ops=ops, state_dict=sd_s)
        assert s["model"] == "teacher"
        f = gd.features(s["seed"] + 1, s["B"]).to(ops.device)
        got = teacher.generate(f, assistant_model=causal, return_dict_in_generate=True, **s["gen_kwargs"]).sequences
        assert got.tolist() == s["sequences"], s["name"]
