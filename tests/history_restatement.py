"""TEST INFRASTRUCTURE -- restatement of the history-dependent selection entry of libdwamd.so (`dw_greedy_select_history`,
csrc/decode.hip) with the interface of HipOps, for tests/test_history_processors*.py: `HistoryRefOps`, a subclass of
oracle.ref_ops.RefOps that adds `greedy_select_history`.  The two rules are written from the reference's processors
(TF:generation/logits_process.py `RepetitionPenaltyLogitsProcessor`, `NoRepeatNGramLogitsProcessor` with `_get_ngrams` /
`_calc_banned_ngram_tokens`) row by row on Python lists -- not from decoding.apply_repetition_penalty / apply_no_repeat_ngram,
which the tests compare with it --, plus the fixture's scenario plumbing.  The product never imports this module."""
import json
import os

import torch

import score_restatement as sr
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps

GOLD = os.path.join(sr.GOLD_DIR, "history_processors.json")
NEG = float("-inf")


def gold():
    with open(GOLD) as f:
        return json.load(f)


# ---- the two rules on one row ---------------------------------------------------------------------------------------------
def penalise_row(x, history, penalty):
    """RepetitionPenaltyLogitsProcessor on one row: x f32 [V] (copy returned), history = every token of the row so far (decoder
    prompt included).  A token that occurs several times is penalised once (the reference gathers, rescales and scatters)."""
    out = x.clone()
    p = torch.tensor(float(penalty), dtype=x.dtype)
    for t in set(history):
        out[t] = x[t] * p if bool(x[t] < 0) else x[t] / p              # IEEE multiply / divide in x's dtype
    return out


def banned_ids(history, g):
    """NoRepeatNGramLogitsProcessor on one row: the ids that would complete an n-gram of size g the row already holds."""
    n = len(history)
    if g <= 0 or n + 1 < g:
        return set()
    grams = {}                                                         # (g - 1 tokens) -> every token that followed them
    for i in range(n - g + 1):
        gram = tuple(history[i:i + g])
        grams.setdefault(gram[:-1], []).append(gram[-1])
    return set(grams.get(tuple(history[n - g + 1:n]), []))


def process_history_row(x, history, penalty=1.0, ngram=0):
    """both rules in the reference's order -> f32 [V] (a banned column holds -inf)"""
    out = penalise_row(x, history, penalty) if float(penalty) != 1.0 else x.clone()
    for t in banned_ids(history, int(ngram)):
        out[t] = NEG
    return out


def select_history_ref(logits, V, tokens, n, *, suppress=None, begin_suppress=None, first=False, no_eos=False, ts_begin=-1,
                       max_initial=-1, begin_index=1, eos=-1, fill=-1, done=None, repetition_penalty=1.0, no_repeat_ngram=0):
    """Token n of every row, the reference's way: the two history rules on the logits widened to fp32, then the remaining
    processors of score_restatement.process_row with the mass rule decided in float64, argmax (the first of equal maxima),
    EOS / pad bookkeeping.  -> (next int64 [B], done bool [B], margins [B]: min(top-two distance of the processed row,
    distance of the mass rule from its threshold))."""
    B = tokens.shape[0]
    toks = tokens.tolist()
    nxt, margins = [], []
    new_done = torch.zeros(B, dtype=torch.bool) if done is None else done.clone().cpu()
    for b in range(B):
        x = process_history_row(logits[b, :V].float().cpu(), toks[b][:n], repetition_penalty, no_repeat_ngram)
        j = n - begin_index
        assert bool(first) == (j == 0)                                 # (how the decoder calls it)
        keep, rule = sr.process_row(x.double(), toks[b][begin_index:n], j, V, suppress=suppress,
                                    begin_suppress=begin_suppress, min_new=10 ** 9 if no_eos else 0, ts_begin=ts_begin,
                                    max_initial=max_initial, eos=eos)
        y = torch.where(keep, x, torch.full_like(x, NEG))
        top = y.topk(2).values
        pick = int(y.argmax()) if bool(keep.any()) else 0
        margin = float(top[0] - top[1]) if bool(torch.isfinite(top[1])) else float("inf")
        margins.append(margin if rule is None else min(margin, rule))
        if eos >= 0:
            if bool(new_done[b]):
                pick = fill
            if pick == eos:
                new_done[b] = True
        nxt.append(pick)
    return torch.tensor(nxt, dtype=torch.int64), new_done, margins


class HistoryRefOps(RefOps):
    """RefOps + greedy_select_history: the two rules from the restatement above, the rest as RefOps.greedy_select."""

    def greedy_select_history(self, logits, V, tokens, n, cur, *, suppress=None, begin_suppress=None, first=False, no_eos=False,
                              forced=False, ts_begin=-1, max_initial=-1, begin_index=1, eos=-1, fill=-1, done=None,
                              repetition_penalty=1.0, no_repeat_ngram=0):
        self.history_calls = getattr(self, "history_calls", 0) + 1
        if not forced:
            B = tokens.shape[0]
            toks = tokens.tolist()
            logits = torch.stack([process_history_row(logits[b, :V].float(), toks[b][:n], repetition_penalty, no_repeat_ngram)
                                  for b in range(B)])
        self.greedy_select(logits, V, tokens, n, cur, suppress=suppress, begin_suppress=begin_suppress, first=first, no_eos=no_eos,
                           forced=forced, ts_begin=ts_begin, max_initial=max_initial, begin_index=begin_index, eos=eos, fill=fill,
                           done=done)


# ---- fixture scenarios ----------------------------------------------------------------------------------------------------
def fields_of(sc):
    return gd.generation_fields(multilingual=True, suppress=True, timestamps=sc["ts_fields"])


def inputs_of(sc):
    f = gd.features(sc["seed"] + 1, sc["B"])
    return f[..., :sc["frames"]].contiguous() if sc.get("frames") else f


def dropin(ops, sc, dtype=torch.float32):
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    m = WhisperForConditionalGeneration(gd.CFG_T, ops=ops, state_dict=gd.weights(sc["seed"]), dtype=dtype)
    m.generation_config = GenerationConfig.from_any(fields_of(sc))
    return m


def reference_model(sc):
    return gd.hf_model(gd.CFG_T, gd.weights(sc["seed"]), **fields_of(sc))


def run(model, sc, device="cpu", **extra):
    """the scenario's call on a drop-in model: full sequences (single window) or the plain seek-loop tokens, as lists"""
    f = inputs_of(sc).to(device)
    if sc["kind"] == "seek":
        return model.generate(f, **sc["kwargs"], **extra).tolist()
    return model.generate(f, return_dict_in_generate=True, **sc["kwargs"], **extra).sequences.tolist()
