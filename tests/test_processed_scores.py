"""decoding.processed_scores -- the one torch statement of the logits rules, which every torch path of the package and
oracle.ref_ops select from -- against the installed transformers processors chained in the reference's order, and
decoding.token_mask against the reference's `torch.isin` over the vocabulary.  Both sides are the same fp32 torch ops on the CPU:
the -inf pattern and every finite value must be equal bit for bit."""
import itertools
import types

import pytest
import torch

from distil_whisper_amd.decoding import processed_scores, token_mask

V, TSB, EOS, P, ROWS = 96, 64, 50, 3, 4
NOTS = TSB - 1
MAX_INITIAL = 5
SUPPRESS = [1, 2, 9, 51, 52, 70, 95, 96, 200]            # (96 and 200 lie beyond the vocabulary: they name no column)
BEGIN_SUPPRESS = [7, EOS, 65]
PROMPT = [60, 61, 62]
# the generated part of each row in the six row states of the timestamp rules (rows of one state have one length); the text rows
# repeat tokens and 2-grams, so that the repetition penalty and the n-gram ban have something to name
STATES = {
    "first_generated_token": [[], [], [], []],
    "text": [[5, 7, 5, 7, 5], [8, 8, 8, 8, 8], [5, 6, 7, 5, 6], [30, 31, 32, 33, 31]],
    "closed_pair": [[64, 5, 6, 70, 70], [64, 5, 5, 64, 64], [66, 7, 8, 95, 95], [64, 64, 5, 66, 66]],
    "open_pair": [[64, 5, 6, 70], [64, 5, 5, 64], [65, 7, 8, 94], [70, 70, 5, 95]],
    "text_after_a_timestamp": [[66, 5, 6], [64, 5, 5], [90, 7, 8], [70, 70, 7]],
    "single_timestamp": [[66], [64], [95], [80]],
}


def reference_chain(lp, ids, penalty, ngram, no_eos, masks):
    n = ids.shape[1]
    cfg = types.SimpleNamespace(no_timestamps_token_id=NOTS, eos_token_id=EOS, bos_token_id=EOS,
                                max_initial_timestamp_index=MAX_INITIAL, _detect_timestamp_from_logprob=True)
    chain = []
    if penalty is not None:
        chain.append(lp.RepetitionPenaltyLogitsProcessor(penalty))
    if ngram:
        chain.append(lp.NoRepeatNGramLogitsProcessor(ngram))
    chain.append(lp.MinNewTokensLengthLogitsProcessor(P, n - P + (1 if no_eos else 0), EOS, device="cpu"))
    if masks:
        chain.append(lp.SuppressTokensAtBeginLogitsProcessor(BEGIN_SUPPRESS, P, device="cpu"))
        chain.append(lp.SuppressTokensLogitsProcessor(SUPPRESS, device="cpu"))
    chain.append(lp.WhisperTimeStampLogitsProcessor(cfg, begin_index=P))
    return chain


@pytest.mark.parametrize("state", list(STATES))
def test_processed_scores_equal_the_transformers_processor_chain(state):
    lp = pytest.importorskip("transformers.generation.logits_process")
    ids = torch.tensor([PROMPT + row for row in STATES[state]])
    assert ids.shape[0] == ROWS
    n = ids.shape[1]
    hist = torch.zeros(ROWS, n + 3, dtype=torch.long)
    hist[:, :n] = ids
    sup, bsup = token_mask(SUPPRESS, V, "cpu", torch.uint8), token_mask(BEGIN_SUPPRESS, V, "cpu")
    g = torch.Generator().manual_seed(len(state))
    fired = set()
    for penalty, ngram, no_eos, masks, shift in itertools.product((None, 1.3), (0, 2), (False, True), (False, True), (0.0, 9.0, -4.0)):
        scores = torch.randn(ROWS, V, generator=g) * 2.0
        scores[:, TSB:] += shift                       # (the mass rule quiet / firing)
        want = scores.clone()
        for proc in reference_chain(lp, ids, penalty, ngram, no_eos, masks):
            want = proc(ids, want)
        kept = scores.clone()
        got = processed_scores(scores, hist, n, begin_index=P, eos=EOS, no_eos=no_eos, first=(n == P),
                               suppress=sup if masks else None, begin_suppress=bsup if masks else None,
                               timestamp_rules=dict(no_timestamps_token_id=NOTS, max_initial_timestamp_index=MAX_INITIAL),
                               repetition_penalty=penalty, no_repeat_ngram=ngram)
        case = (penalty, ngram, no_eos, masks, shift)
        assert got.dtype == torch.float32 and got.shape == (ROWS, V)
        assert torch.equal(scores, kept), case          # the caller's scores are left alone
        assert torch.equal(torch.isinf(got), torch.isinf(want)), case
        assert torch.equal(got, want), case
        fired.add(bool(torch.isinf(got[:, :TSB]).all(1).any()))
    if state in ("text", "text_after_a_timestamp"):     # both outcomes of the mass rule were compared
        assert fired == {False, True}


def test_processed_scores_without_timestamp_rules_and_without_eos():
    lp = pytest.importorskip("transformers.generation.logits_process")
    ids = torch.tensor([PROMPT + row for row in STATES["text"]])
    n = ids.shape[1]
    scores = torch.randn(ROWS, V, generator=torch.Generator().manual_seed(1))
    want = lp.SuppressTokensLogitsProcessor(SUPPRESS, device="cpu")(ids, lp.NoRepeatNGramLogitsProcessor(2)(ids, scores.clone()))
    got = processed_scores(scores, ids, n, begin_index=P, no_eos=True, suppress=token_mask(SUPPRESS, V, "cpu"), no_repeat_ngram=2)
    assert torch.equal(got, want)
    assert processed_scores(scores.bfloat16(), ids, n, begin_index=P).dtype == torch.float32


def test_token_mask_is_isin_over_the_vocabulary():
    for ids in (SUPPRESS, BEGIN_SUPPRESS, [0], [V - 1, V - 1, 3], torch.tensor([4, 5])):
        want = torch.isin(torch.arange(V), torch.as_tensor(ids))
        for dtype in (torch.bool, torch.uint8):
            got = token_mask(ids, V, "cpu", dtype)
            assert got.dtype == dtype and got.shape == (V,)
            assert torch.equal(got.bool(), want)
    for ids in (None, [], [V, V + 7], [-1]):              # no id names a column: no mask
        assert token_mask(ids, V, "cpu") is None
