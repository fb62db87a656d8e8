"""`generate(output_scores=True / output_logits=True, return_dict_in_generate=True)` and `compute_transition_scores`, the part that
needs no GPU: the drop-in over a torch restatement of the scoring kernel (tests/score_restatement.py, fp32 model) against what
the reference returned for the scenarios of tests/golden/generate_scores.npz (tools/gen_golden_generate_scores.py).

Bounds: the `-inf` pattern must be IDENTICAL (it depends on the logits only through the timestamp mass rule, and the generator
keeps a seed only when every such decision is 0.05 away from its threshold).  Finite values: 20 x `ref_reorder_dev`, the
reference's own |step-wise - teacher-forced| difference in fp32 (about 1.7e-6; the factor covers a second fp32 implementation whose
operation order differs in every layer) -- four orders below the logits' standard deviation (0.57), where any rule or indexing
error shows.  A log_softmax of values that are each off by d moves by at most 2 d: the normalised transition scores get 40 x."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import score_restatement as sr

META, ARR = sr.gold()
SC = {s["name"]: s for s in META["scenarios"]}
NAMES = ["plain", "min_new_tokens", "prompt_ids", "timestamps", "ragged_finish"]


def _ops():
    return sr.ScoreRefOps("cpu", lowp=torch.float32)


@functools.lru_cache(maxsize=None)
def _run(name):
    return sr.run_dropin(_ops(), SC[name])


def test_fixture_holds_every_scenario():
    assert sorted(SC) == sorted(NAMES)
    for name, sc in SC.items():
        seq, scores = ARR[f"{name}.sequences"], ARR[f"{name}.scores"]
        assert scores.shape == (sc["steps"], sc["B"], META["meta"]["vocab"]) and seq.shape == (sc["B"], sc["P"] + sc["steps"])
        assert sc["steps"] <= 8 and sc["B"] <= 3
        assert 0 < sc["ref_reorder_dev"] < 1e-4 and 0 < sc["ref_bf16_dev"] < 0.2 * sc["logit_sigma"]
        assert np.isfinite(ARR[f"{name}.logits"]).all() and np.isinf(scores).any()
    assert SC["timestamps"]["rule_margin"] >= META["meta"]["min_rule_margin"]
    ragged = SC["ragged_finish"]
    gen = ARR["ragged_finish.sequences"][:, ragged["P"]:]
    assert len({int((row == ragged["kwargs"]["eos_token_id"]).argmax()) if (row == ragged["kwargs"]["eos_token_id"]).any()
                else gen.shape[1] for row in gen}) >= 2


@pytest.mark.parametrize("name", NAMES)
def test_scores_and_logits_against_the_reference(name):
    sc = SC[name]
    _, out = _run(name)
    assert out.sequences.tolist() == ARR[f"{name}.sequences"].tolist()
    bound = 20 * sc["ref_reorder_dev"]
    for field in ("scores", "logits"):
        got, want = sr.stacked(out[field]), ARR[f"{name}.{field}"]
        assert got.shape == want.shape
        assert np.array_equal(np.isneginf(got), np.isneginf(want)), f"{name}.{field}: other columns are masked"
        fin = np.isfinite(want)
        assert np.isfinite(got[fin]).all()
        dev = float(np.abs(got[fin] - want[fin]).max())
        print(f"{name}.{field}: max |ours - reference| {dev:.3e} (bound {bound:.3e})")
        assert dev <= bound


@pytest.mark.parametrize("name", NAMES)
def test_compute_transition_scores(name):
    sc = SC[name]
    model, out = _run(name)
    P = sc["P"]
    for normalize, key, factor in ((False, "trans", 20), (True, "trans_norm", 40)):
        ours = model.compute_transition_scores(out.sequences, out.scores, normalize_logits=normalize)
        # the gather GenerationMixin does, on the same tensors handed over as a plain tuple
        plain = model.compute_transition_scores(out.sequences, tuple(out.scores), normalize_logits=normalize)
        st = torch.stack(tuple(out.scores), 1)
        st = torch.log_softmax(st, -1) if normalize else st
        gathered = st.gather(2, out.sequences[:, P:, None])[:, :, 0]
        assert ours.shape == (sc["B"], sc["steps"]) and ours.dtype == torch.float32
        assert torch.equal(plain, gathered)
        assert torch.equal(torch.isneginf(ours), torch.isneginf(gathered))
        fin = torch.isfinite(gathered)
        if normalize:
            assert (ours[fin] - gathered[fin]).abs().max().item() <= 1e-5       # float64 log_softmax against fp32
        else:
            assert torch.equal(ours, gathered)
        want = torch.from_numpy(ARR[f"{name}.{key}"])
        assert torch.equal(torch.isneginf(ours), torch.isneginf(want))
        fin = torch.isfinite(want)
        assert (ours[fin] - want[fin]).abs().max().item() <= factor * sc["ref_reorder_dev"]
    # the logits tuple carries the raw values; other sequences than the scored ones go through the gather
    raw = model.compute_transition_scores(out.sequences, out.logits)
    assert torch.equal(raw, torch.stack(tuple(out.logits), 1).gather(2, out.sequences[:, P:, None])[:, :, 0])
    other = out.sequences.clone()
    other[:, -1] = 41
    got = model.compute_transition_scores(other, out.scores)
    assert torch.equal(got[:, -1], out.scores[-1][:, 41]) and torch.equal(got[:, :-1], out.scores.chosen[:, :-1])


def test_shapes_and_keys_follow_the_reference():
    sc = SC["plain"]
    model, out = _run("plain")
    V = META["meta"]["vocab"]
    assert out.keys() == ["sequences", "scores", "logits"]
    for field in ("scores", "logits"):
        steps = out[field]
        assert isinstance(steps, tuple) and len(steps) == out.sequences.shape[1] - sc["P"]
        assert all(t.shape == (sc["B"], V) and t.dtype == torch.float32 for t in steps)
        assert steps.chosen.shape == steps.logprob.shape == (sc["B"], len(steps))
    f, kw = sr.inputs_of(sc), sr.call_kwargs(sc)
    only = model.generate(f, return_dict_in_generate=True, output_scores=True, **kw)
    assert only.keys() == ["sequences", "scores"] and only.logits is None
    assert all(torch.equal(a, b) for a, b in zip(only.scores, out.scores))
    only = model.generate(f, return_dict_in_generate=True, output_logits=True, **kw)
    assert only.keys() == ["sequences", "logits"] and only.scores is None
    assert all(torch.equal(a, b) for a, b in zip(only.logits, out.logits))
    # together with token timestamps, and without the KV cache
    import align_restatement as ar

    class Both(sr.ScoreRefOps, ar.AlignRefOps):
        pass
    m2 = sr.dropin(Both("cpu", lowp=torch.float32), sc)
    m2.generation_config.alignment_heads = [[0, 1], [1, 0]]
    both = m2.generate(f, return_dict_in_generate=True, output_scores=True, return_token_timestamps=True, **kw)
    assert both.keys() == ["sequences", "scores", "token_timestamps"]
    assert all(torch.equal(a, b) for a, b in zip(both.scores, out.scores))
    nocache = model.generate(f, return_dict_in_generate=True, output_scores=True, output_logits=True, use_cache=False, **kw)
    assert nocache.sequences.tolist() == out.sequences.tolist()
    assert all(torch.equal(a, b) for a, b in zip(nocache.scores, out.scores))
    # encoder_outputs / decoder_input_ids instead of features / the assembled prompt
    enc, _ = model.engine.encode(f.float().contiguous(), save=False)
    enc = enc[:sc["B"] * model.dims.max_src].view(sc["B"], -1, model.dims.d_model)
    alt = model.generate(encoder_outputs=enc, return_dict_in_generate=True,
                         output_scores=True, decoder_input_ids=out.sequences[:, :sc["P"]], max_new_tokens=sc["steps"])
    assert all(torch.equal(a, b) for a, b in zip(alt.scores, out.scores))


def test_a_call_that_yields_no_new_token_returns_empty_tuples():
    # GenerationMixin returns `scores=()` / `logits=()` when the length limit is the prompt's length
    sc = SC["plain"]
    model, _ = _run("plain")
    kw = dict(sr.call_kwargs(sc), max_new_tokens=0)
    out = model.generate(sr.inputs_of(sc), return_dict_in_generate=True, output_scores=True, output_logits=True, **kw)
    assert out.sequences.shape == (sc["B"], sc["P"])
    assert out.keys() == ["sequences", "scores", "logits"]
    assert isinstance(out.scores, tuple) and isinstance(out.logits, tuple) and len(out.scores) == len(out.logits) == 0


def test_plain_generate_is_unchanged_without_the_flags():
    from distil_whisper_amd import generation as G
    sc = SC["plain"]
    model, out = _run("plain")
    f, kw = sr.inputs_of(sc), sr.call_kwargs(sc)
    plain = model.generate(f, **kw)
    want = G.strip_and_pad(torch.from_numpy(ARR["plain.sequences"]), sc["P"], 900, 900)
    assert torch.is_tensor(plain) and plain.tolist() == want.tolist()
    # without return_dict_in_generate the flags are dropped, as the reference drops them
    flagged = model.generate(f, output_scores=True, output_logits=True, **kw)
    assert torch.is_tensor(flagged) and torch.equal(flagged, plain)
    bare = model.generate(f, return_dict_in_generate=True, **kw)
    assert bare.keys() == ["sequences"] and bare.scores is None and bare.logits is None
    assert bare.sequences.tolist() == out.sequences.tolist()


def test_combinations_that_are_not_implemented_raise():
    sc = SC["timestamps"]
    model = sr.dropin(_ops(), sc)
    f = sr.inputs_of(sc)
    base = dict(language="en", max_new_tokens=4, return_dict_in_generate=True)
    for flag in ("output_scores", "output_logits"):
        for extra, word in ((dict(num_beams=2), "beam"), (dict(assistant_model=model), "assistant"),
                            (dict(temperature=0.7), "sampling"), (dict(repetition_penalty=1.3), "repetition_penalty"),
                            (dict(no_repeat_ngram_size=2), "no_repeat_ngram_size"),
                            (dict(return_timestamps=True), "seek loop")):
            with pytest.raises(NotImplementedError, match=word) as e:
                model.generate(f, **base, **{flag: True}, **extra)
            assert "output_" in str(e.value)
    # the same calls without return_dict_in_generate run: the flags are dropped there
    assert torch.is_tensor(model.generate(f, language="en", max_new_tokens=3, num_beams=2, output_scores=True))
    out = model.generate(f, **base, output_scores=True)
    with pytest.raises(NotImplementedError, match="beam_indices"):
        model.compute_transition_scores(out.sequences, out.scores, beam_indices=torch.zeros(2, 4, dtype=torch.long))
    with pytest.raises(ValueError, match="not used by the model"):
        model.generate(f, **base, output_score=True)


def test_dw_score_tokens_rejects_bad_arguments_without_touching_the_gpu():
    from distil_whisper_amd import ops_hip
    lib = ops_hip.load_library()
    good = ctypes.c_void_p(0x10000)                 # never dereferenced: every call below fails validation before any launch

    def call(logits=good, dtype=1, B=2, L=3, V=1000, ld=1000, batch_rows=3, tokens=good, tok_ld=8, begin=4, min_new=0,
             ts_begin=-1, max_initial=-1, eos=900, scores=good, ld_scores=1000, chosen=good, logprob=good):
        return lib.dw_score_tokens(logits, dtype, B, L, V, ld, batch_rows, tokens, tok_ld, begin, None, None, min_new, ts_begin,
                                   max_initial, eos, scores, ld_scores, chosen, logprob, None)
    assert call(logits=None) == -1 and call(tokens=None) == -1
    assert call(scores=None, chosen=None, logprob=None) == -1                       # nothing to write
    assert call(dtype=2) == -1 and call(B=0) == -1 and call(L=0) == -1 and call(V=0) == -1 and call(B=70000) == -1
    assert call(ld=998) == -1 and call(ld=1002, V=1000) == -1                        # ld < V; ld not a multiple of 4
    assert call(logits=ctypes.c_void_p(0x10004)) == -1                              # bf16 rows need 8-byte alignment
    assert call(logits=ctypes.c_void_p(0x10008), dtype=0) == -1                     # fp32 rows need 16
    assert call(batch_rows=2) == -1 and call(tok_ld=6) == -1 and call(begin=-1) == -1 and call(min_new=-1) == -1
    assert call(eos=1000) == -1
    assert call(ts_begin=912, eos=-1) == -1 and call(ts_begin=912, begin=0, tok_ld=8) == -1 and call(ts_begin=1001) == -1
    assert call(ld_scores=996) == -1 and call(ld_scores=1002) == -1 and call(scores=ctypes.c_void_p(0x10008)) == -1
