"""Speculative decoding with per-row acceptance on the CPU: the torch round (`assist_pick_rows_torch`, `assist_accept_rows_torch`)
against the numpy restatement (tests/assist_rows_restatement.py) on planted rounds with rows at different lengths; the loop
`assisted_greedy_decode(per_row=True)` over the torch restatement of the kernels (oracle.ref_ops: no `assist_*_rows`, no
`decode_pass_rows`, so the torch round and the per-kernel form of `engine.decode_multi_rows`) against every row decoded alone by
plain greedy decoding; the public surface.

Near ties follow tests/test_assist_gpu.py: an input with an exactly tied selection is left out, one whose smallest margin is within
EXACT_ULPS bf16 ulps of the best score is not held to plain greedy, at most half of the inputs tried may go either way.  The models
are tests/assist_rows_cases.planted_pair, whose decisions are a quarter of the best score apart by construction."""
import json
import os

import numpy as np
import pytest
import torch

from distil_whisper_amd import decoding
from distil_whisper_amd.decoding import (GreedyDecoder, assist_accept_rows_torch, assist_pick_rows_torch,
                                         assisted_greedy_decode)
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps
from tests import assist_cases as ac
from tests import assist_rows_cases as arc
from tests.assist_rows_restatement import accept_rows_ref, pick_rows_ref

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "decode.json")))
EXACT_ULPS = 4
LENS = [7, 9, 12]


def torch_round(c):
    tok = torch.from_numpy(c["tokens"]).clone()
    V = c["logits"].shape[-1]
    sup = None
    if c["suppress"]:
        sup = torch.zeros(V)
        sup[torch.tensor(c["suppress"])] = float("-inf")
    own = assist_pick_rows_torch(torch.from_numpy(c["logits"]).float(), tok, c["lens"], 0, c["P0"], c["eos"], c["min_new"], sup, c["ts"])
    length = torch.tensor(c["lens"], dtype=torch.int32)
    done = torch.from_numpy(c["done"]).clone()
    pos_t, pos_a, result = assist_accept_rows_torch(own.clone(), tok, length, c["k"], c["total"], done, c["eos"], c["fill"])
    return own, tok, length, done, pos_t, pos_a, result


def check_round(got, c, name):
    """`got` = (own, tokens, lens, done, pos_t, pos_a, result) of the code under test as lists / arrays; every integer is exact."""
    own_ref, _ = pick_rows_ref(c["logits"], c["tokens"], c["lens"], 0, c["P0"], c["eos"], c["min_new"], c["suppress"], (), c["ts"])
    assert own_ref.tolist() == c["own"].tolist(), name       # (the single-row cases derived the same integers)
    tok_ref, len_ref, done_ref, pt_ref, pa_ref, res_ref = accept_rows_ref(own_ref, c["tokens"], c["lens"], c["k"], c["total"],
                                                                            c["done"], c["eos"], c["fill"])
    own, tok, length, done, pos_t, pos_a, result = got
    assert np.asarray(own)[:, :c["k"] + 1].tolist() == own_ref.tolist(), name
    assert np.asarray(tok).tolist() == tok_ref.tolist(), name
    assert list(length) == len_ref.tolist() and list(done) == done_ref.tolist(), name
    assert list(pos_t) == pt_ref.tolist() and list(pos_a) == pa_ref.tolist(), name
    assert list(result) == res_ref, name
    return tok_ref, len_ref, done_ref, res_ref


@pytest.mark.parametrize("k", [0, 1, 5])
def test_torch_round_matches_the_restatement_on_planted_rounds(k):
    B = 3
    seen = {}
    for name, sc in ac.scenarios(B, k).items():
        c = arc.planted_rows(1030, LENS, k, name)
        own, tok, length, done, pos_t, pos_a, result = torch_round(c)
        tok_ref, len_ref, done_ref, res = check_round((own.numpy(), tok.numpy(), length.tolist(), done.tolist(), pos_t, pos_a, result),
                                                      c, name)
        gained = [int(n) - int(o) for n, o in zip(len_ref, c["lens"])]
        seen[name] = gained
        L = c["lens"]
        if name == "all_accepted":                            # the longest row reaches `total` and ends there, the others go on
            assert gained == [k + 1] * B and done_ref.tolist() == [False, False, True] and res == [3 * k, 3 * k, 0, L[1] + k + 1]
            assert pos_t[2] == 0 and pos_a[2] == 0 and pos_t[0] == L[0] + k and pos_a[1] == L[1] + k - 1
        if name == "rows_differ":                             # every row keeps its own prefix
            assert gained == [k + 1, min(1, k) + 1, min(3, k) + 1]
        if name == "done_row":                                # a row that is already done: untouched length, `fill` behind it
            assert gained[2] == 0 and done_ref[2] and (tok_ref[2, L[2]:min(L[2] + k, c["total"] - 1) + 1] == c["fill"]).all()
            assert res[1] == 2 * k
        if name == "eos_accepted" and k >= 1:                 # EOS in the middle of the accepted prefix: the row ends there
            assert gained == [2] * B and done_ref.all() and res[:3] == [3 * min(2, k), 3 * k, 1]
            for b in range(B):
                assert tok_ref[b, L[b] + 1] == c["eos"]
                assert (tok_ref[b, L[b] + 2:min(L[b] + k, c["total"] - 1) + 1] == c["fill"]).all()      # later drafts are not kept
        if name == "min_new_inside":                          # the threshold crosses inside the drafts of row 0 only
            own_ref = c["own"]
            assert (own_ref[0, :min(2, k)] != c["eos"]).all() and (own_ref[1:, 0] == c["eos"]).all()
            assert k < 2 or own_ref[0, 2] == c["eos"]
        if name == "ts_first":
            assert c["lens"] == [c["P0"]] * B
    if k == 5:
        assert set(seen) == set(ac.scenarios(B, k))
        assert seen["reject_first"] == [1, 1, 1] and seen["reject_middle"] == [3, 3, 3]


def test_a_row_at_total_and_a_stale_length_stay_in_bounds():
    """Rows that have ended at the end of the buffer are not judged and not written; k drafts never reach past total - 1."""
    c = arc.planted_rows(1030, LENS, 5, "all_accepted")
    c["lens"] = [7, c["total"], c["total"] - 1]               # row 1 has ended at `total`; row 2 has room for the target's token only
    tok = torch.from_numpy(c["tokens"]).clone()
    own = assist_pick_rows_torch(torch.from_numpy(c["logits"]).float(), tok, c["lens"], 0, c["P0"], c["eos"], 0, None, None)
    own_ref, _ = pick_rows_ref(c["logits"], c["tokens"], c["lens"], 0, c["P0"], c["eos"], 0, (), (), None)
    assert own.tolist() == own_ref.tolist() and own[1].tolist() == [0] * 6 and own[2, 1:].tolist() == [0] * 5
    length, done = torch.tensor(c["lens"], dtype=torch.int32), torch.zeros(3, dtype=torch.bool)
    pos_t, pos_a, result = assist_accept_rows_torch(own.clone(), tok, length, 5, c["total"], done, c["eos"], c["fill"])
    ref = accept_rows_ref(own_ref, c["tokens"], c["lens"], 5, c["total"], np.zeros(3, dtype=bool), c["eos"], c["fill"])
    assert tok.tolist() == ref[0].tolist() and length.tolist() == ref[1].tolist() and done.tolist() == ref[2].tolist()
    assert (pos_t, pos_a, result) == (ref[3].tolist(), ref[4].tolist(), ref[5])
    assert done.tolist()[1:] == [True, True] and result[1] == 5          # only row 0 was offered drafts


# ---- the loop on the CPU ops --------------------------------------------------------------------------------------------------
SEQ = [50, 61, 72, 83, 94, 105, 116, 127, 138, 149]
WEAK = (2, 5, 8)
PROMPT = [gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE, gd.NOTIMESTAMPS]


def _engines(ops, seed, row_tokens, dtype=torch.float32):
    from distil_whisper_amd.modeling import WhisperForCausalLM, WhisperForConditionalGeneration
    sd_t, sd_a, enc = arc.planted_pair(gd.weights(seed), len(PROMPT), SEQ, WEAK, row_tokens, gd.CFG_T.d_model, gd.CFG_T.max_src, scale=4.0, head_gain=4.0)
    target = WhisperForConditionalGeneration(gd.CFG_T, ops=ops, state_dict=sd_t, dtype=dtype)
    assistant = WhisperForCausalLM(gd.CFG_T, ops=ops, state_dict={k: v for k, v in sd_a.items() if k.startswith("model.decoder.")},
                                   dtype=dtype)
    return target, assistant, enc


def run_rows(monkeypatch, target, assistant, enc, prompt, max_new, K, **kw):
    """-> (rows as lists, drafted, accepted, per-round gains of the rows live in that round, smallest margin in bf16 ulps of the
    best score over the selections of live rows)."""
    margins, gains, state = [], [], {"done": [False] * prompt.shape[0]}
    pick, accept = decoding.assist_pick_rows_torch, decoding.assist_accept_rows_torch

    def spy_pick(logits, tokens, lengths, j0, begin_index, *a, **k2):
        own = pick(logits, tokens, lengths, j0, begin_index, *a, **k2)
        for b, fin in enumerate(state["done"]):
            for j in range(logits.shape[1]):
                if fin or max(lengths[b], begin_index) + j0 + j >= tokens.shape[1]:
                    continue
                lg = logits[b, j].float().clone()
                best = lg[own[b, j]].item()
                lg[own[b, j]] = float("-inf")
                one = lg.view(1, 1, -1)
                second = decoding.assist_pick_torch(one, tokens[b:b + 1], max(lengths[b], begin_index) + j0 + j, begin_index, *a, **k2)
                gap = best - lg[second[0, 0]].item()
                margins.append(gap / 2.0 ** (np.floor(np.log2(max(abs(best), 1e-30))) - 7))
        return own

    def spy_accept(own, tokens, length, k, total, done, *a):
        before, was = length.tolist(), done.tolist()
        out = accept(own, tokens, length, k, total, done, *a)
        gains.append([n - o for n, o, w in zip(length.tolist(), before, was) if not w])
        state["done"] = done.tolist()
        return out

    monkeypatch.setattr(decoding, "assist_pick_rows_torch", spy_pick)
    monkeypatch.setattr(decoding, "assist_accept_rows_torch", spy_accept)
    ids, drafted, accepted = assisted_greedy_decode(target.engine, assistant.engine, enc, enc, prompt, max_new, K, per_row=True, **kw)
    monkeypatch.undo()
    return ids.tolist(), drafted, accepted, gains, min(margins)


def plain_rows(target, enc, prompt, max_new, eos, suppress):
    """Every row decoded alone at B = 1 by plain greedy decoding."""
    d = target.dims
    dec = GreedyDecoder(target.engine, 1, prompt.shape[1] + max_new, eos_token_id=eos, suppress_tokens=suppress, pad_token_id=eos,
                        use_graphs=False)
    return [dec.run(enc[b * d.max_src:(b + 1) * d.max_src], prompt[b:b + 1], max_new)[0].tolist() for b in range(prompt.shape[0])]


def selected(tried, checked):
    print(f"inputs tried {tried}, compared {checked}, left out {tried - checked}")
    assert checked >= 1 and 2 * (tried - checked) <= tried


def compare_with_plain(got, ref, pad):
    """The rounds stop once every row is done: a row is its plain greedy row, cut behind its end, then pad."""
    n = len(got[0])
    for g, r in zip(got, ref):
        r = r + [pad] * (n - len(r))
        assert g == r[:n] and all(t == pad for t in r[n:])


@pytest.mark.parametrize("with_eos", [True, False])
@pytest.mark.parametrize("K", [1, 5])
def test_every_row_equals_that_row_decoded_alone(monkeypatch, K, with_eos):
    """B = 3, seeds 21 / 22 / 23 (chosen on the CPU: every margin is far above EXACT_ULPS).  Rows accept different numbers of drafts
    in one round, row 2 ends at its own EOS long before the others."""
    ops = RefOps("cpu", lowp=torch.float32)
    assert not hasattr(ops, "assist_pick_rows") and not hasattr(ops, "decode_pass_rows")
    eos = gd.EOS if with_eos else None
    prompt = torch.tensor([PROMPT] * 3)
    max_new = 9
    tried = exact = 0
    for seed in (21, 22, 23):
        target, assistant, enc = _engines(ops, seed, [400, 410, gd.EOS])
        tried += 1
        got, drafted, accepted, gains, margin = run_rows(monkeypatch, target, assistant, enc, prompt, max_new, K, eos_token_id=eos,
                                                         suppress_tokens=gd.SUPPRESS, pad_token_id=eos)
        print(f"seed {seed}: margin {margin:.1f} ulps, drafted {drafted}, accepted {accepted}, gains {gains}")
        if margin <= EXACT_ULPS:                              # (<= 0: an exactly tied selection)
            continue
        compare_with_plain(got, plain_rows(target, enc, prompt, max_new, eos, gd.SUPPRESS), eos)
        want = arc.expected_rows(SEQ, WEAK, [400, 410, gd.EOS], eos, max_new)
        assert [g[len(PROMPT):len(PROMPT) + len(w)] for g, w in zip(got, want)] == want
        assert any(len(set(g)) > 1 for g in gains), "every row accepted alike in every round"
        assert 0 < accepted < drafted
        exact += 1
    selected(tried, exact)


def test_rounds_without_drafts_follow_one_another():
    """max_new_tokens such that rows reach total - 1 one after the other: k = 0 rounds in a row; the catch-up pass keeps the lagging
    rows' assistant cache within two tokens (the loop asserts its invariants on this path)."""
    ops = RefOps("cpu", lowp=torch.float32)
    target, assistant, enc = _engines(ops, 21, [400, 410, 420])
    prompt = torch.tensor([PROMPT] * 3)
    for max_new in (1, 2, 4, 7):
        ids, drafted, accepted = assisted_greedy_decode(target.engine, assistant.engine, enc, enc, prompt, max_new, 5, per_row=True,
                                                        suppress_tokens=gd.SUPPRESS)
        ref = plain_rows(target, enc, prompt, max_new, None, gd.SUPPRESS)
        assert ids.tolist() == ref, max_new


# ---- the public surface -------------------------------------------------------------------------------------------------------
def _model(ops, cfg, sd, fields):
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    m = WhisperForConditionalGeneration(cfg, ops=ops, state_dict=sd)
    m.generation_config = GenerationConfig.from_any(fields)
    return m


def _fixture_models(ops, seed, fields):
    sd_t = gd.weights(seed)
    sd_s, cfg_s = gd.student(sd_t)
    return _model(ops, gd.CFG_T, sd_t, fields), _model(ops, cfg_s, sd_s, fields)


def test_generate_flag_errors_are_raised_before_anything_is_decoded(monkeypatch):
    ops = RefOps("cpu", lowp=torch.float32)
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=True)
    teacher, student = _fixture_models(ops, 310, fields)
    f = gd.features(311, 2)

    def no_encode(*a, **k):
        raise AssertionError("the encoder ran before the refusal")
    monkeypatch.setattr(type(teacher.engine), "encode", no_encode)
    kw = dict(max_new_tokens=4, language="en")
    with pytest.raises(ValueError, match="assistant_model"):
        teacher.generate(f, assistant_per_row=True, **kw)
    with pytest.raises(NotImplementedError, match="use_cache"):
        teacher.generate(f, assistant_model=student, assistant_per_row=True, use_cache=False, **kw)
    with pytest.raises(NotImplementedError, match="seek loop"):
        teacher.generate(f, assistant_model=student, assistant_per_row=True, return_timestamps=True, **kw)
    long1 = torch.cat([f, f[..., :2200]], -1)
    with pytest.raises(NotImplementedError, match="seek loop"):
        teacher.generate(long1, assistant_model=student, assistant_per_row=True, return_timestamps=True, **kw)
    # whatever already raises with an assistant still does, before anything is decoded
    for extra in (dict(num_beams=2), dict(repetition_penalty=1.3), dict(no_repeat_ngram_size=2), dict(temperature=0.7),
                  dict(sequence_bias={(50,): 2.0}), dict(return_dict_in_generate=True, output_scores=True),
                  dict(return_token_timestamps=True)):
        with pytest.raises(NotImplementedError):
            teacher.generate(f, assistant_model=student, assistant_per_row=True, **kw, **extra)


def test_generate_with_the_flag_gives_every_row_its_own_greedy_output():
    ops = RefOps("cpu", lowp=torch.float32)
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=True)
    teacher, student = _fixture_models(ops, 310, fields)
    f = gd.features(315, 3)
    for kw in (dict(max_new_tokens=7, language="en"),
               dict(max_new_tokens=7, language="en", return_timestamps=True, force_unique_generate_call=True)):
        plain = teacher.generate(f, **kw)
        got = teacher.generate(f, assistant_model=student, assistant_per_row=True, **kw)
        assert got.tolist() == plain.tolist()
        assert teacher.last_drafted > 0


def test_generate_without_the_flag_is_unchanged_on_the_fixture_assistant_scenarios(monkeypatch):
    ops = RefOps("cpu", lowp=torch.float32)
    todo = [s for s in GOLD["scenarios"] if s.get("assistant") and s.get("kind") == "short" and not s.get("use_encoder_outputs")]
    assert todo

    def no_rows(*a, **k):
        raise AssertionError("the per-row rounds ran without the flag")
    monkeypatch.setattr(decoding, "_assisted_rounds_device_rows", no_rows)
    for s in todo:
        teacher, student = _fixture_models(ops, s["seed"], s["generation_config"])
        model = teacher if s["model"] == "teacher" else student
        f = gd.features(s["seed"] + 1, s["B"])
        for flag in ({}, dict(assistant_per_row=False)):
            got = model.generate(f, assistant_model=student, return_dict_in_generate=True, **flag, **s["gen_kwargs"]).sequences
            assert got.tolist() == s["sequences"], s["name"]


class _FE:
    """What PseudoLabeller asks of a feature extractor before the first call."""
    n_samples = 480000


def test_pseudo_labeller_constructor_errors():
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    ops = RefOps("cpu", lowp=torch.float32)
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=False)
    teacher, student = _fixture_models(ops, 310, fields)
    kw = dict(batch_size=2, max_new_tokens=4, prompt_ids=PROMPT, eos_token_id=gd.EOS, assistant_model=student)
    for extra in (dict(num_beams=2), dict(timestamp_rules=dict(no_timestamps_token_id=gd.NOTIMESTAMPS, max_initial_timestamp_index=50)),
                  dict(repetition_penalty=1.2), dict(no_repeat_ngram_size=3), dict(sequence_bias={(50,): 1.0}),
                  dict(bad_words_ids=[[50]])):
        with pytest.raises(NotImplementedError, match="assistant_model"):
            PseudoLabeller(teacher, _FE(), **kw, **extra)
    lab = PseudoLabeller(teacher, _FE(), **kw, num_assistant_tokens=3)
    assert lab.assistant is student and lab.num_assistant_tokens == 3
    assert PseudoLabeller(teacher, _FE(), **{**kw, "assistant_model": None}).assistant is None
