"""`generate(sequence_bias=..., bad_words_ids=...)` through the selection kernel's bias table, the part that needs no GPU: the
torch statement of the rule (decoding.apply_sequence_bias over decoding.sequence_bias_table) and its restatement
(tests/sequence_bias_restatement.py) against the reference's two processors, the drop-in over that restatement (`BiasRefOps`: the
decoder calls `greedy_select_bias` as it does on the GPU) and over plain `RefOps` (the eager torch path) against
tests/golden/sequence_bias.json (tools/gen_golden_sequence_bias.py) and against a live `transformers` call, the reference's
validation errors, the refusals, the C entry's argument checks and the schedulers' new arguments.

Greedy search under these rules is deterministic: every comparison is token for token (scores: value for value)."""
import ctypes
import functools

import pytest
import torch

import sequence_bias_restatement as br
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps

GOLD = br.gold()
SC = {s["name"]: s for s in GOLD["scenarios"]}
SHORT = ["one_token_boost", "multi_token_boost", "two_on_one_column", "bad_words", "with_repetition_rules", "timestamps_one_window"]
NAMES = SHORT + ["seek_loop"]
INF = float("inf")


@functools.lru_cache(maxsize=None)
def _model(name, kind):
    ops = br.BiasRefOps("cpu", lowp=torch.float32) if kind == "bias" else RefOps("cpu", lowp=torch.float32)
    return br.dropin(ops, SC[name])


def test_fixture_holds_every_scenario_and_the_arguments_matter():
    assert sorted(SC) == sorted(NAMES)
    for name, sc in SC.items():
        assert sc["sequences"] != sc["baseline"], f"{name}: the reference decodes the same tokens without the arguments"
        assert sc["B"] <= 2 and sc["kwargs"]["max_new_tokens"] <= 12
        assert any(k in sc["kwargs"] for k in br.OPTIONS)
        assert sc["tried"] >= 1 and sum(sc["rejected"].values()) < sc["tried"]
    lens = lambda name: sorted(len(q) for q, _ in SC[name]["kwargs"]["sequence_bias"])          # noqa: E731
    assert lens("one_token_boost") == [1] and SC["one_token_boost"]["kwargs"]["sequence_bias"][0][1] > 0
    assert max(lens("multi_token_boost")) >= 2
    # the multi-token sequence meets its prefix in the reference's own unbiased output
    (q, v), = SC["multi_token_boost"]["kwargs"]["sequence_bias"]
    P = SC["multi_token_boost"]["P"]
    assert v > 0 and any(row[P:][i:i + len(q) - 1] == q[:-1] for row in SC["multi_token_boost"]["baseline"] for i in range(8))
    cols = [q[-1] for q, _ in SC["two_on_one_column"]["kwargs"]["sequence_bias"]]
    assert len(cols) >= 2 and len(set(cols)) == 1
    bad = SC["bad_words"]["kwargs"]["bad_words_ids"]
    assert {1, 2} <= {len(q) for q in bad} and [gd.EOS] in bad
    for row in SC["bad_words"]["sequences"]:                  # the rule holds in the reference's own output
        gen = row[SC["bad_words"]["P"]:]
        for q in bad:
            if q != [gd.EOS]:
                assert all(gen[i:i + len(q)] != q for i in range(len(gen)))
    both = SC["with_repetition_rules"]["kwargs"]
    assert {"sequence_bias", "bad_words_ids", "repetition_penalty", "no_repeat_ngram_size"} <= set(both)
    one = SC["timestamps_one_window"]["kwargs"]
    assert one["return_timestamps"] and one["force_unique_generate_call"]
    biased = [q[0] for q, _ in one["sequence_bias"]]
    assert any(t >= gd.TS0 for t in biased) and any(t < gd.EOS for t in biased)
    seek = SC["seek_loop"]
    assert seek["frames"] == 450 and seek["B"] == 2 and min(seek["passes"]) >= 2


def _random_case(g, V, n):
    """a table that reaches every branch of the rule for a history of n tokens over ids 1..5, and the two histories"""
    ids = torch.randint(1, 6, (3, n), generator=g)
    h = ids[0].tolist()
    val = lambda: float(torch.randint(-12, 13, (1,), generator=g).item()) / 4 or 0.75          # noqa: E731
    sb = [[[7], val()], [[8], val()], [[7], val()],                    # a duplicate one-token entry: the last bias is ASSIGNED
          [h[-1:] + [9], val()], [[3, 9], val()], [[9], val()],        # several sequences on one column
          [[2, 4], val()], [h[-2:] + [4], val()] if n >= 2 else [[1, 4], val()],
          [h + [11], val()],                                           # length n + 1: longer than the history, ignored
          [[6] + h + [11], val()]]                                     # length n + 2: ignored
    if n >= 2:
        sb.append([h[1:] + [12], val()])                               # length n: applies (its prefix is the last n - 1 tokens)
    bw = [[13], [h[-1], 14], [5, 15], h + [16], [30]]                  # [30] stands for the EOS id: dropped
    return ids, sb, bw


def test_apply_sequence_bias_against_the_reference_processors():
    """seeded random cases: the imported classes, the restatement and the product's torch statement give the same scores"""
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, SequenceBiasLogitsProcessor
    from distil_whisper_amd.decoding import apply_sequence_bias, sequence_bias_table
    g = torch.Generator().manual_seed(23)
    V, EOS = 40, 30
    applied = ignored = banned = 0
    for case in range(200):
        n = 1 + case % 7
        ids, sb, bw = _random_case(g, V, n)
        use_sb, use_bw = case % 5 != 3, case % 5 != 4
        scores = (torch.randn(3, V, generator=g) * 2).bfloat16().float()
        want = scores.clone()
        if use_sb:
            want = SequenceBiasLogitsProcessor(sb)(ids, want)
        if use_bw:
            want = NoBadWordsLogitsProcessor(bw, eos_token_id=EOS)(ids, want)
        table = sequence_bias_table(sb if use_sb else None, bw if use_bw else None, V, EOS)
        got = apply_sequence_bias(scores, ids, table)
        assert torch.equal(got, want), case
        mine = torch.stack([br.process_bias_row(scores[b].double(), ids[b].tolist(), sb if use_sb else None, bw if use_bw else None,
                                                EOS) for b in range(3)])
        assert torch.equal(mine.float(), want), case
        assert float(want[0, 30]) == float(scores[0, 30])             # the [eos] entry is gone
        banned += int(torch.isneginf(want).sum())
        if use_sb:
            assert float(want[1, 11]) == float(scores[1, 11])         # n + 1 and n + 2 tokens: ignored
            ignored += 1
            if n >= 2:
                applied += float(want[0, 12]) != float(scores[0, 12])
                assert float(want[0, 7]) == float(scores[0, 7] + sb[2][1])      # the later duplicate, not the sum
    assert applied > 50 and ignored > 100 and banned > 300
    # table order: ascending by column, the one-token entry first, bad words last; duplicates resolved
    t = sequence_bias_table([[[5, 9], 1.0], [[9], 0.5], [[7], 2.0], [[7], 3.0], [[4, 9], -1.0]], [[9], [30], [2, 7]], V, EOS)
    assert t.seqs == ((7,), (2, 7), (9,), (5, 9), (4, 9), (9,)) and t.vals == (3.0, -INF, 0.5, 1.0, -1.0, -INF)
    dev = t.tensors("cpu")
    assert dev["bias_off"].tolist() == [0, 1, 3, 4, 6, 8, 9] and dev["bias_tok"].tolist() == [7, 2, 7, 9, 5, 9, 4, 9, 9]
    assert dev["bias_tok"].dtype == dev["bias_off"].dtype == torch.int32 and dev["bias_val"].dtype == torch.float32
    assert sequence_bias_table(None, [[30]], V, EOS) is None and sequence_bias_table(None, None, V, EOS) is None
    assert t == sequence_bias_table({(5, 9): 1.0, (9,): 0.5, (7,): 3.0, (4, 9): -1.0}, [[9], [2, 7]], V, EOS) and hash(t) == hash(t)


def test_processed_scores_puts_the_bias_in_front_of_the_repetition_penalty():
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import (NoBadWordsLogitsProcessor, NoRepeatNGramLogitsProcessor,
                                                        RepetitionPenaltyLogitsProcessor, SequenceBiasLogitsProcessor)
    from distil_whisper_amd.decoding import processed_scores, sequence_bias_table
    V = 40
    ids = torch.tensor([[3, 5, 3, 7], [2, 5, 3, 5]])
    scores = torch.linspace(-3, 3, 2 * V).view(2, V).bfloat16().float()
    sb, bw = [[[7], 2.5], [[3, 5], -1.25], [[5, 3], 0.75]], [[3], [5, 9]]
    want = SequenceBiasLogitsProcessor(sb)(ids, scores.clone())
    want = NoRepeatNGramLogitsProcessor(2)(ids, RepetitionPenaltyLogitsProcessor(1.5)(ids, want))
    want = NoBadWordsLogitsProcessor(bw, eos_token_id=30)(ids, want)
    got = processed_scores(scores, ids, 4, begin_index=1, repetition_penalty=1.5, no_repeat_ngram=2,
                           sequence_bias=sequence_bias_table(sb, bw, V, 30))
    assert torch.equal(got, want)
    assert float(got[0, 7]) == float((scores[0, 7] + 2.5) / 1.5)            # biased, then penalised (fp32, as there)


@pytest.mark.parametrize("name", NAMES)
def test_generate_equals_the_fixture_on_the_kernel_entry_and_on_the_eager_path(name):
    sc = SC[name]
    model = _model(name, "bias")
    model.ops.bias_calls = 0
    assert br.run(model, sc) == sc["sequences"]
    assert model.ops.bias_calls > 0                          # the decoder really took the new entry
    eager = _model(name, "eager")
    assert not hasattr(eager.ops, "greedy_select_bias")
    assert br.run(eager, sc) == sc["sequences"]
    # without the arguments: the baseline, through the entries the decoder took before
    model.ops.bias_calls = 0
    base = dict(sc, kwargs=br.without_options(sc["kwargs"]))
    assert br.run(model, base) == sc["baseline"] and model.ops.bias_calls == 0
    if sc["kind"] == "seek":
        got = model.generate(br.inputs_of(sc), return_segments=True, **sc["kwargs"])
        assert got["sequences"].tolist() == sc["sequences"]
        for got_row, want_row in zip(got["segments"], sc["segments"]):
            assert [list(s["tokens"]) for s in got_row] == [s["tokens"] for s in want_row]


@pytest.mark.parametrize("name", ["multi_token_boost", "with_repetition_rules", "seek_loop"])
def test_generate_equals_transformers_live(name):
    pytest.importorskip("transformers")
    sc = SC[name]
    f = br.inputs_of(sc)
    with torch.no_grad():
        if sc["kind"] == "seek":
            ref = br.reference_model(sc).generate(f, **sc["kwargs"]).tolist()
        else:
            ref = br.reference_model(sc).generate(f, return_dict_in_generate=True, **sc["kwargs"]).sequences.tolist()
    assert ref == sc["sequences"]                            # the fixture is what this transformers decodes
    assert br.run(_model(name, "bias"), sc) == ref


def test_other_call_forms_take_the_table_too():
    """prompt_ids, decoder_input_ids, encoder_outputs and the dict form of the argument, against the reference (live)"""
    pytest.importorskip("transformers")
    sc = SC["multi_token_boost"]
    model, f = _model("multi_token_boost", "bias"), br.inputs_of(sc)
    kw = dict(sc["kwargs"])
    as_dict = {tuple(q): v for q, v in kw["sequence_bias"]}
    assert model.generate(f, return_dict_in_generate=True, **dict(kw, sequence_bias=as_dict)).sequences.tolist() == sc["sequences"]
    prompt = torch.tensor([gd.STARTOFPREV, 50, 51])
    dec_ids = torch.tensor([[gd.SOT, 902, gd.TRANSCRIBE, gd.NOTIMESTAMPS]] * 2)
    for extra in (dict(prompt_ids=prompt), dict(decoder_input_ids=dec_ids)):
        with torch.no_grad():
            ref = br.reference_model(sc).generate(f, return_dict_in_generate=True, **kw, **extra).sequences.tolist()
        assert model.generate(f, return_dict_in_generate=True, **kw, **extra).sequences.tolist() == ref, list(extra)
    enc, _ = model.engine.encode(f.float().contiguous(), save=False)
    d = model.dims
    got = model.generate(encoder_outputs=enc[:2 * d.max_src].view(2, d.max_src, d.d_model), return_dict_in_generate=True,
                         **kw).sequences.tolist()
    assert got == sc["sequences"]


def test_validation_errors_are_the_references():
    pytest.importorskip("transformers")
    from transformers.generation.logits_process import NoBadWordsLogitsProcessor, SequenceBiasLogitsProcessor
    from distil_whisper_amd.decoding import sequence_bias_table
    model = _model("one_token_boost", "bias")
    f = br.inputs_of(SC["one_token_boost"])
    calls = []
    keep = model.engine.encode
    model.engine.encode = lambda *a, **k: calls.append(1)
    try:
        for bad in ([], {}, "x", [[[1, 2], 1]], [[[1, -2], 1.0]], [[1, 2.0]], {(1, 2): 1}, {"a": 1.0}, {(): 1.0},
                    {(1, -1): 2.0}, [[[0], 1.0]]):
            with pytest.raises(ValueError) as ref:
                SequenceBiasLogitsProcessor(bad)
            with pytest.raises(ValueError) as got:
                sequence_bias_table(bad, None, gd.V, gd.EOS)
            assert str(got.value) == str(ref.value), bad
            with pytest.raises(ValueError):
                model.generate(f, language="en", max_new_tokens=3, sequence_bias=bad)
        for bad in ([], "x", [1, 2], [[1, -2]], [[1, 2.5]]):
            with pytest.raises(ValueError) as ref:
                NoBadWordsLogitsProcessor(bad, eos_token_id=gd.EOS)
            with pytest.raises(ValueError) as got:
                sequence_bias_table(None, bad, gd.V, gd.EOS)
            assert str(got.value) == str(ref.value), bad
        # an EMPTY sequence passes the reference's checks and fails inside its first step; here it is refused at once
        with pytest.raises(ValueError, match="sequence_bias"):
            sequence_bias_table([[[], 1.0]], None, gd.V, gd.EOS)
        with pytest.raises(ValueError, match="bad_words_ids"):
            sequence_bias_table(None, [[]], gd.V, gd.EOS)
        # an id beyond the vocabulary: the reference raises at its first step, with this message
        with pytest.raises(ValueError) as ref:
            SequenceBiasLogitsProcessor([[[5, gd.V], 1.0], [[gd.V + 3], 2.0]])(torch.zeros(1, 2, dtype=torch.long), torch.zeros(1, gd.V))
        for kw in (dict(sequence_bias=[[[5, gd.V], 1.0], [[gd.V + 3], 2.0]]), dict(bad_words_ids=[[5, gd.V], [gd.V + 3]])):
            with pytest.raises(ValueError) as got:
                model.generate(f, language="en", max_new_tokens=3, **kw)
            assert str(got.value) == str(ref.value)
        # the caps of the kernel's table
        with pytest.raises(NotImplementedError, match="1024"):
            model.generate(f, language="en", max_new_tokens=3, bad_words_ids=[[1 + i // 800, 1 + i % 800] for i in range(1025)])
        with pytest.raises(NotImplementedError, match="32"):
            model.generate(f, language="en", max_new_tokens=3, sequence_bias=[[list(range(1, 34)), 1.0]])
        with pytest.raises(NotImplementedError, match="NaN"):
            model.generate(f, language="en", max_new_tokens=3, sequence_bias=[[[5], float("nan")]])
        assert sequence_bias_table([[list(range(1, 33)), 1.0]], [[1 + i // 800, 1 + i % 800] for i in range(1023)], gd.V, gd.EOS).S == 1024
    finally:
        model.engine.encode = keep
    assert not calls                                         # nothing was encoded before a refusal


def test_combinations_that_raise_name_the_arguments_and_decode_nothing():
    sc = SC["seek_loop"]
    model = _model("seek_loop", "bias")
    f = br.inputs_of(sc)
    full = gd.features(sc["seed"] + 1, 2)
    base = dict(language="en", max_new_tokens=4)
    calls = []
    keep = model.engine.encode
    model.engine.encode = lambda *a, **k: calls.append(1)
    try:
        for opts in (dict(sequence_bias=[[[50], 1.0]]), dict(bad_words_ids=[[50, 51]])):
            for extra, word in ((dict(num_beams=2), "beam"), (dict(assistant_model=model), "assistant"),
                                (dict(use_cache=False), "use_cache"), (dict(temperature=0.7), "sampling"),
                                (dict(do_sample=True, temperature=0.7, top_k=0), "sampling"),
                                (dict(return_dict_in_generate=True, output_scores=True), "output_scores"),
                                (dict(return_dict_in_generate=True, output_logits=True), "output_logits"),
                                (dict(return_token_timestamps=True), "return_token_timestamps"),
                                (dict(num_beams=2, return_timestamps=True), "beam"),
                                (dict(assistant_model=model, return_timestamps=True), "assistant"),
                                (dict(return_timestamps=True, return_token_timestamps=True), "return_token_timestamps"),
                                (dict(return_timestamps=True, condition_on_prev_tokens=True), "condition_on_prev_tokens")):
                with pytest.raises(NotImplementedError, match="sequence_bias / bad_words_ids") as e:
                    model.generate(f if extra.get("return_timestamps") else full, **base, **opts, **extra)
                assert word in str(e.value), (extra, str(e.value))
        # seek_decode itself refuses what it cannot combine
        from distil_whisper_amd.decoding import sequence_bias_table
        table = sequence_bias_table([[[50], 1.0]], None, gd.V, gd.EOS)
        args = (f, [450, 450], [[gd.SOT]] * 2, lambda P: (4, 0), gd.EOS, gd.EOS, gd.NOTIMESTAMPS)
        for extra in (dict(num_beams=2), dict(assistant=(model.engine, None)), dict(condition_on_prev_tokens=True),
                      dict(token_timestamps=dict(alignment_heads=[[0, 0]], num_frames=None, time_precision=0.02))):
            with pytest.raises(NotImplementedError, match="sequence_bias"):
                model.seek_decode(*args, sequence_bias=table, **extra)
    finally:
        model.engine.encode = keep
    assert not calls


def test_arguments_off_take_the_existing_entries():
    """a spy on the ops: without the arguments `greedy_select_bias` is never called and the decoder is built without `soft`"""
    sc = SC["one_token_boost"]
    model = _model("one_token_boost", "bias")
    model.ops.bias_calls = 0
    seen = []
    keep = model.ops.greedy_select

    def spy(*a, **k):
        seen.append(1)
        return keep(*a, **k)
    model.ops.greedy_select = spy
    try:
        model._decoders = {}
        kw = br.without_options(sc["kwargs"])
        assert model.generate(br.inputs_of(sc), return_dict_in_generate=True, **kw).sequences.tolist() == sc["baseline"]
        (dec,) = model._decoders.values()
        assert dec.soft is None and dec.bias is None and dec.history is None
        assert model.ops.bias_calls == 0 and len(seen) > 0
        # None is "not given", as for every generation-config field
        model.generate(br.inputs_of(sc), sequence_bias=None, bad_words_ids=None, **kw)
        (dec,) = model._decoders.values()
        assert dec.soft is None and model.ops.bias_calls == 0
        # bad words that are all [eos]: nothing is left to apply
        model.generate(br.inputs_of(sc), bad_words_ids=[[gd.EOS]], **kw)
        (dec,) = model._decoders.values()
        assert dec.soft is None and model.ops.bias_calls == 0
    finally:
        del model.ops.greedy_select
        model._decoders = {}


def test_decoder_takes_the_table_with_graphs_and_sampling_stays_eager():
    from distil_whisper_amd.decoding import GreedyDecoder, sequence_bias_table
    bias, eager = _model("bad_words", "bias").engine, _model("bad_words", "eager").engine
    table = sequence_bias_table([[[50], 1.0], [[50, 60], 2.0]], [[70]], gd.V, gd.EOS)
    soft = dict(do_sample=False, repetition_penalty=1.3, no_repeat_ngram_size=3, sequence_bias=table)
    dec = GreedyDecoder(bias, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft))
    assert dec.use_graphs and dec.history is None
    assert dec.bias["repetition_penalty"] == 1.3 and dec.bias["no_repeat_ngram"] == 3
    assert dec.bias["bias_off"].tolist() == [0, 1, 3, 4] and dec.bias["bias_val"].tolist() == [1.0, 2.0, -INF]
    dec = GreedyDecoder(bias, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft, repetition_penalty=None, no_repeat_ngram_size=0))
    assert dec.use_graphs and dec.bias["repetition_penalty"] == 1.0 and dec.bias["no_repeat_ngram"] == 0
    dec = GreedyDecoder(bias, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft, do_sample=True, temperature=0.7))
    assert not dec.use_graphs and dec.bias is None and dec.sample is None
    dec = GreedyDecoder(eager, 2, 16, eos_token_id=gd.EOS, use_graphs=True, soft=dict(soft))
    assert not dec.use_graphs and dec.bias is None


def test_dw_greedy_select_bias_rejects_bad_arguments_without_touching_the_gpu():
    from distil_whisper_amd import ops_hip
    lib = ops_hip.load_library()
    good = ctypes.c_void_p(0x10000)                 # never dereferenced: every call below fails validation before any launch

    def call(logits=good, B=2, V=1000, ld=1000, first=0, no_eos=0, forced=0, ts_begin=-1, max_initial=-1, tokens=good, tok_ld=16,
             n=4, begin=4, eos=900, fill=900, done=good, cur=good, penalty=1.2, ngram=2, tok=good, off=good, val=good, S=3):
        return lib.dw_greedy_select_bias(logits, B, V, ld, None, None, first, no_eos, forced, ts_begin, max_initial, tokens,
                                         tok_ld, n, begin, eos, fill, done, cur, penalty, ngram, tok, off, val, S, None)
    assert call(S=-1) == -1 and call(S=1025) == -1
    assert call(tok=None) == -1 and call(off=None) == -1 and call(val=None) == -1
    # everything dw_greedy_select_history checks
    assert call(logits=None) == -1 and call(tokens=None) == -1 and call(cur=None) == -1 and call(done=None) == -1
    assert call(penalty=0.0) == -1 and call(penalty=float("nan")) == -1 and call(ngram=-1) == -1
    assert call(V=65537, ld=65540) == -1
    assert call(B=0) == -1 and call(n=0) == -1 and call(n=16) == -1 and call(V=0) == -1
    assert call(ld=996) == -1 and call(ld=1002) == -1 and call(logits=ctypes.c_void_p(0x10004)) == -1
    assert call(ts_begin=912, eos=-1) == -1 and call(ts_begin=912, begin=0) == -1 and call(ts_begin=912, begin=5) == -1
    assert call(forced=1, logits=None, S=2000) == -1
    assert "dw_greedy_select_bias" in ops_hip.EXPORTED_SYMBOLS and hasattr(ops_hip.HipOps, "greedy_select_bias")
    assert (ops_hip.HipOps.BIAS_MAX_SEQUENCES, ops_hip.HipOps.BIAS_MAX_TOKENS) == (1024, 32)


def test_schedulers_hand_the_arguments_to_their_decoder():
    from distil_whisper_amd.longform import LongFormTranscriber
    from distil_whisper_amd.modeling import WhisperFeatureExtractor
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    model = _model("bad_words", "bias")
    fe = WhisperFeatureExtractor(feature_size=80, ops=model.ops)
    kw = dict(batch_size=2, max_new_tokens=4, eos_token_id=gd.EOS, use_graphs=True)
    sb, bw = [[[50, 60], 2.0]], [[70], [gd.EOS]]
    for cls in (LongFormTranscriber, PseudoLabeller):
        sched = cls(model, fe, sequence_bias=sb, bad_words_ids=bw, **kw)
        table = sched.decoder.soft["sequence_bias"]
        assert table.seqs == ((50, 60), (70,)) and table.vals == (2.0, -INF)
        assert sched.decoder.use_graphs and sched.decoder.bias is not None and sched.decoder.history is None
        plain = cls(model, fe, **kw)
        assert plain.decoder.soft is None and plain.decoder.bias is None
        assert cls(model, fe, bad_words_ids=[[gd.EOS]], **kw).decoder.soft is None
        with pytest.raises(ValueError, match="sequence_bias"):
            cls(model, fe, sequence_bias=[], **kw)
        with pytest.raises(ValueError, match="vocabulary size"):
            cls(model, fe, bad_words_ids=[[gd.V]], **kw)
    for opts in (dict(sequence_bias=sb), dict(bad_words_ids=bw)):
        with pytest.raises(NotImplementedError, match=next(iter(opts))):
            PseudoLabeller(model, fe, num_beams=2, **opts, **kw)
    lab = PseudoLabeller(model, fe, bad_words_ids=bw, timestamp_rules=dict(no_timestamps_token_id=gd.NOTIMESTAMPS), **kw)
    assert lab._history_kw["sequence_bias"].seqs == ((70,),)
