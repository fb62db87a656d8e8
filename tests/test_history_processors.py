"""`generate(repetition_penalty=..., no_repeat_ngram_size=...)` through the selection kernel's history path, the part that needs
no GPU: the restatement of the two rules (tests/history_restatement.py) against the reference's processors, the drop-in over that
restatement (`HistoryRefOps`: the decoder calls `greedy_select_history` as it does on the GPU) and over plain `RefOps` (the
eager torch path) against tests/golden/history_processors.json (tools/gen_golden_history_processors.py) and against a live
`transformers` call, the refusals, the C entry's argument checks and the schedulers' new arguments.

Greedy search under these rules is deterministic: every comparison is token for token."""
import ctypes
import functools

import pytest
import torch

import history_restatement as hr
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps

GOLD = hr.gold()
SC = {s["name"]: s for s in GOLD["scenarios"]}
SHORT = ["repetition_penalty", "no_repeat_2gram", "no_repeat_1gram", "both", "timestamps_one_window"]
NAMES = SHORT + ["seek_loop"]


@functools.lru_cache(maxsize=None)
def _model(name, kind):
    ops = hr.HistoryRefOps("cpu", lowp=torch.float32) if kind == "history" else RefOps("cpu", lowp=torch.float32)
    return hr.dropin(ops, SC[name])


def test_fixture_holds_every_scenario_and_the_options_matter():
    assert sorted(SC) == sorted(NAMES)
    for name, sc in SC.items():
        assert sc["sequences"] != sc["baseline"], f"{name}: the reference decodes the same tokens without the options"
        assert sc["B"] <= 2 and sc["kwargs"]["max_new_tokens"] <= 12
        assert any(k in sc["kwargs"] for k in ("repetition_penalty", "no_repeat_ngram_size"))
    assert SC["no_repeat_1gram"]["kwargs"]["no_repeat_ngram_size"] == 1 and SC["no_repeat_2gram"]["kwargs"]["no_repeat_ngram_size"] == 2
    assert {"repetition_penalty", "no_repeat_ngram_size"} <= set(SC["both"]["kwargs"])
    one = SC["timestamps_one_window"]["kwargs"]
    assert one["return_timestamps"] and one["force_unique_generate_call"]
    seek = SC["seek_loop"]
    assert seek["frames"] == 450 and seek["B"] == 2 and min(seek["passes"]) >= 2
    assert [[t for sg in row for t in sg["tokens"]] for row in seek["segments"]] == \
           [[t for t in row if t != gd.EOS] for row in seek["sequences"]]
    # single window: the rules hold in the reference's own output
    for name in SHORT:
        sc = SC[name]
        g = sc["kwargs"].get("no_repeat_ngram_size", 0)
        for row in sc["sequences"]:
            row = row[:row.index(gd.EOS) + 1] if gd.EOS in row else row
            grams = [tuple(row[i:i + g]) for i in range(len(row) - g + 1)] if g else []
            assert len(grams) == len(set(grams)), f"{name}: a repeated {g}-gram"


def test_restatement_of_the_two_rules_against_the_reference_processors():
    """step by step on random scores and histories: the imported classes, the restatement of tests/history_restatement.py and
    the product's torch versions (decoding.apply_*: the eager path) give the same scores, bit for bit"""
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import NoRepeatNGramLogitsProcessor, RepetitionPenaltyLogitsProcessor
    from distil_whisper_amd.decoding import apply_no_repeat_ngram, apply_repetition_penalty
    g = torch.Generator().manual_seed(11)
    V, B = 40, 3
    hits = 0
    for penalty, ngram in ((1.7, 2), (0.6, 3), (1.2, 1), (1.0, 2), (1.3, 0), (2.5, 5)):
        ids = torch.randint(0, 6, (B, 1), generator=g)
        for step in range(12):
            scores = (torch.randn(B, V, generator=g) * 2).bfloat16().float()          # widened bf16 logits, as in the kernel
            want = scores.clone()
            if penalty != 1.0:
                want = RepetitionPenaltyLogitsProcessor(penalty)(ids, want)
            if ngram:
                want = NoRepeatNGramLogitsProcessor(ngram)(ids, want)
            mine = torch.stack([hr.process_history_row(scores[b], ids[b].tolist(), penalty, ngram) for b in range(B)])
            prod = scores.clone()
            if penalty != 1.0:
                prod = apply_repetition_penalty(prod, ids, penalty)
            if ngram:
                prod = apply_no_repeat_ngram(prod, ids, ngram)
            assert torch.equal(mine.view(torch.int32), want.view(torch.int32)), (penalty, ngram, step)
            assert torch.equal(prod.view(torch.int32), want.view(torch.int32)), (penalty, ngram, step)
            hits += int(torch.isneginf(want).sum())
            # few distinct ids: repeated tokens and repeated n-grams from the second step on
            ids = torch.cat([ids, torch.randint(0, 6, (B, 1), generator=g)], 1)
    assert hits > 50
    assert hr.banned_ids([1, 2], 4) == set() and hr.banned_ids([1, 2, 3], 4) == set() and hr.banned_ids([5, 7, 5], 2) == {7}
    assert hr.banned_ids([5, 7, 5], 1) == {5, 7}


@pytest.mark.parametrize("name", NAMES)
def test_generate_equals_the_fixture_on_the_history_path_and_on_the_eager_path(name):
    sc = SC[name]
    model = _model(name, "history")
    model.ops.history_calls = 0
    assert hr.run(model, sc) == sc["sequences"]
    assert model.ops.history_calls > 0                       # the decoder really took the new entry
    eager = _model(name, "eager")
    assert not hasattr(eager.ops, "greedy_select_history")
    assert hr.run(eager, sc) == sc["sequences"]
    if sc["kind"] == "seek":
        got = model.generate(hr.inputs_of(sc), return_segments=True, **sc["kwargs"])
        assert got["sequences"].tolist() == sc["sequences"]
        assert len(got["segments"]) == len(sc["segments"])
        for got_row, want_row in zip(got["segments"], sc["segments"]):
            assert [list(s["tokens"]) for s in got_row] == [s["tokens"] for s in want_row]
            for s, w in zip(got_row, want_row):
                assert float(s["start"]) == pytest.approx(w["start"], abs=1e-6) and float(s["end"]) == pytest.approx(w["end"], abs=1e-6)


@pytest.mark.parametrize("name", NAMES)
def test_generate_equals_transformers_live(name):
    pytest.importorskip("transformers")
    sc = SC[name]
    f = hr.inputs_of(sc)
    with torch.no_grad():
        if sc["kind"] == "seek":
            ref = hr.reference_model(sc).generate(f, **sc["kwargs"]).tolist()
        else:
            ref = hr.reference_model(sc).generate(f, return_dict_in_generate=True, **sc["kwargs"]).sequences.tolist()
    assert ref == sc["sequences"]                            # the fixture is what this transformers decodes
    assert hr.run(_model(name, "history"), sc) == ref


def test_history_decoder_keeps_use_graphs_and_sampling_stays_eager():
    from distil_whisper_amd.decoding import GreedyDecoder
    sc = SC["both"]
    hist, eager = _model("both", "history").engine, _model("both", "eager").engine
    soft = dict(do_sample=False, repetition_penalty=1.3, no_repeat_ngram_size=3)
    dec = GreedyDecoder(hist, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft))
    assert dec.use_graphs and dec.history == dict(repetition_penalty=1.3, no_repeat_ngram=3)
    dec = GreedyDecoder(hist, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft, repetition_penalty=None))
    assert dec.use_graphs and dec.history == dict(repetition_penalty=1.0, no_repeat_ngram=3)
    # sampling, and ops without the entry: the eager torch selection as before
    dec = GreedyDecoder(hist, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft, do_sample=True, temperature=0.7))
    assert not dec.use_graphs and dec.history is None
    dec = GreedyDecoder(eager, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft))
    assert not dec.use_graphs and dec.history is None
    assert GreedyDecoder(hist, 2, 16, eos_token_id=gd.EOS, use_graphs=True).history is None
    del sc


def test_condition_on_prev_tokens_one_utterance_live_and_two_utterances_raise():
    """one utterance: the history of the rules includes the previous-text prompt, as in the reference (live); several: the
    reference's left-padding would enter the history -- a loud refusal before anything is decoded"""
    pytest.importorskip("transformers")
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=True)
    changed = 0
    for seed in (400, 401, 402):
        sc = dict(seed=seed, ts_fields=True, B=1)
        model = hr.dropin(hr.HistoryRefOps("cpu", lowp=torch.float32), sc)
        long1 = torch.cat([gd.features(seed + 2, 1), gd.features(seed + 3, 1)[..., :1000]], -1)
        kw = dict(max_new_tokens=6, return_timestamps=True, language="en", condition_on_prev_tokens=True)
        opts = dict(repetition_penalty=1.5, no_repeat_ngram_size=2)
        with torch.no_grad():
            ref = gd.hf_model(gd.CFG_T, gd.weights(seed), **fields).generate(long1, **kw, **opts).tolist()
        assert model.generate(long1, **kw, **opts).tolist() == ref, seed
        changed += model.generate(long1, **kw).tolist() != ref
    assert changed >= 1
    calls = []
    model.engine.encode = lambda *a, **k: calls.append(1)            # (nothing may be decoded before the refusal)
    two = gd.features(5, 2)[..., :700].contiguous()
    for opts in (dict(repetition_penalty=1.5), dict(no_repeat_ngram_size=2)):
        with pytest.raises(NotImplementedError, match="condition_on_prev_tokens") as e:
            model.generate(two, **kw, **opts)
        assert "repetition_penalty" in str(e.value) and "no_repeat_ngram_size" in str(e.value) and "pad" in str(e.value)
    assert not calls


def test_combinations_that_still_raise_name_the_option():
    sc = SC["seek_loop"]
    model = _model("seek_loop", "history")
    f = hr.inputs_of(sc)
    full = gd.features(sc["seed"] + 1, 2)
    base = dict(language="en", max_new_tokens=4)
    for opts in (dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2)):
        word = next(iter(opts))
        for extra in (dict(num_beams=2), dict(assistant_model=model), dict(use_cache=False),
                      dict(num_beams=2, return_timestamps=True), dict(assistant_model=model, return_timestamps=True)):
            with pytest.raises(NotImplementedError, match=word):
                model.generate(f if extra.get("return_timestamps") else full, **base, **opts, **extra)
        for flag in ("output_scores", "output_logits"):
            with pytest.raises(NotImplementedError, match=word) as e:
                model.generate(full, **base, **opts, return_dict_in_generate=True, **{flag: True})
            assert flag in str(e.value)
    # a positive temperature as a plain sampling switch inside the seek loop
    with pytest.raises(NotImplementedError, match="sampling"):
        model.generate(f, **base, return_timestamps=True, temperature=0.5)
    # seek_decode itself refuses beams / an assistant with the options
    with pytest.raises(NotImplementedError, match="repetition_penalty"):
        model.seek_decode(f, [450, 450], [[gd.SOT]] * 2, lambda P: (4, 0), gd.EOS, gd.EOS, gd.NOTIMESTAMPS, num_beams=2,
                          repetition_penalty=1.2)


def test_dw_greedy_select_history_rejects_bad_arguments_without_touching_the_gpu():
    from distil_whisper_amd import ops_hip
    lib = ops_hip.load_library()
    good = ctypes.c_void_p(0x10000)                 # never dereferenced: every call below fails validation before any launch

    def call(logits=good, B=2, V=1000, ld=1000, first=0, no_eos=0, forced=0, ts_begin=-1, max_initial=-1, tokens=good, tok_ld=16,
             n=4, begin=4, eos=900, fill=900, done=good, cur=good, penalty=1.2, ngram=2):
        return lib.dw_greedy_select_history(logits, B, V, ld, None, None, first, no_eos, forced, ts_begin, max_initial, tokens,
                                            tok_ld, n, begin, eos, fill, done, cur, penalty, ngram, None)
    assert call(logits=None) == -1 and call(tokens=None) == -1 and call(cur=None) == -1 and call(done=None) == -1
    assert call(penalty=0.0) == -1 and call(penalty=-1.5) == -1
    assert call(penalty=float("inf")) == -1 and call(penalty=float("nan")) == -1
    assert call(ngram=-1) == -1
    assert call(V=65537, ld=65540) == -1                                            # beyond the history bitmaps
    # what dw_greedy_select rejects
    assert call(B=0) == -1 and call(n=0) == -1 and call(n=16) == -1 and call(V=0) == -1
    assert call(ld=996) == -1 and call(ld=1002) == -1 and call(logits=ctypes.c_void_p(0x10004)) == -1
    assert call(ts_begin=912, eos=-1) == -1 and call(ts_begin=912, begin=0) == -1 and call(ts_begin=912, begin=5) == -1
    # a forced position takes no logits, but the options are checked all the same
    assert call(forced=1, logits=None, penalty=0.0) == -1 and call(forced=1, logits=None, ngram=-2) == -1
    assert "dw_greedy_select_history" in ops_hip.EXPORTED_SYMBOLS


def test_schedulers_hand_the_options_to_their_decoder():
    from distil_whisper_amd.longform import LongFormTranscriber
    from distil_whisper_amd.modeling import WhisperFeatureExtractor
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    model = _model("both", "history")
    fe = WhisperFeatureExtractor(feature_size=80, ops=model.ops)
    want = dict(do_sample=False, repetition_penalty=1.2, no_repeat_ngram_size=3)
    kw = dict(batch_size=2, max_new_tokens=4, eos_token_id=gd.EOS, use_graphs=True)
    for cls in (LongFormTranscriber, PseudoLabeller):
        sched = cls(model, fe, repetition_penalty=1.2, no_repeat_ngram_size=3, **kw)
        assert sched.decoder.soft == want and sched.decoder.use_graphs
        assert sched.decoder.history == dict(repetition_penalty=1.2, no_repeat_ngram=3)
        plain = cls(model, fe, **kw)
        assert plain.decoder.soft is None and plain.decoder.history is None
        assert cls(model, fe, repetition_penalty=1.0, no_repeat_ngram_size=0, **kw).decoder.soft is None
        with pytest.raises(ValueError, match="repetition_penalty"):
            cls(model, fe, repetition_penalty=0.0, **kw)
        with pytest.raises(ValueError, match="no_repeat_ngram_size"):
            cls(model, fe, no_repeat_ngram_size=-1, **kw)
    with pytest.raises(NotImplementedError, match="no_repeat_ngram_size"):
        PseudoLabeller(model, fe, num_beams=2, no_repeat_ngram_size=2, **kw)
    # the labeller's timestamp mode runs the seek loop: the options travel with it
    lab = PseudoLabeller(model, fe, repetition_penalty=1.2, timestamp_rules=dict(no_timestamps_token_id=gd.NOTIMESTAMPS), **kw)
    assert lab._history_kw == dict(repetition_penalty=1.2, no_repeat_ngram_size=0)


def test_transcriber_decodes_with_the_options():
    """the scheduler's output under the options is what per-window `generate` decodes under them, and differs from plain"""
    from distil_whisper_amd.longform import LongFormTranscriber
    from distil_whisper_amd.modeling import WhisperFeatureExtractor
    sc = SC["no_repeat_1gram"]
    model = _model("no_repeat_1gram", "history")
    fe = WhisperFeatureExtractor(feature_size=80, ops=model.ops)
    audio = [torch.from_numpy(gd.audio(3, 16000 * 4))]
    prompt = [gd.SOT, 902, gd.TRANSCRIBE, gd.NOTIMESTAMPS]
    fields = hr.fields_of(sc)
    kw = dict(batch_size=1, max_new_tokens=8, eos_token_id=gd.EOS, prompt_ids=prompt, use_graphs=False,
              suppress_tokens=fields["suppress_tokens"], begin_suppress_tokens=fields["begin_suppress_tokens"])
    got = LongFormTranscriber(model, fe, no_repeat_ngram_size=1, **kw)(audio)
    feats = fe([a.numpy() for a in audio], return_tensors="pt").input_features
    want = model.generate(feats, language="en", max_new_tokens=8, no_repeat_ngram_size=1).tolist()[0]
    want = [t for t in want if t != gd.EOS]
    assert list(got[0]) == want and len(set(want)) == len(want)
