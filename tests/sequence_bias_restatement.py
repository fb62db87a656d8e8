"""TEST INFRASTRUCTURE -- float64 restatement of the selection entry with the sequence-bias table (`dw_greedy_select_bias`,
csrc/decode.hip) for tests/test_sequence_bias*.py.  The rule is written from the reference's two processors
(TF:generation/logits_process.py `SequenceBiasLogitsProcessor.__call__` / `_prepare_bias_variables`, `NoBadWordsLogitsProcessor`)
on Python lists and numpy, from the caller's ARGUMENTS -- not from decoding.sequence_bias_table / apply_sequence_bias, which the tests
compare with it; the history rules and the remaining processors are those of tests/history_restatement.py and
tests/score_restatement.py.  Plus `BiasRefOps` (RefOps + `greedy_select_bias`, so that the decoder takes the entry it takes on the
GPU) and the plumbing of tests/golden/sequence_bias.json.  The product never imports this module."""
import json
import os

import numpy as np
import torch

import history_restatement as hr
import score_restatement as sr
from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps

GOLD = os.path.join(sr.GOLD_DIR, "sequence_bias.json")
NEG = float("-inf")


def gold():
    with open(GOLD) as f:
        return json.load(f)


# ---- the rule on one row ---------------------------------------------------------------------------------------------------
def _as_dict(sequence_bias):
    if sequence_bias is None:
        return {}
    if isinstance(sequence_bias, dict):
        return dict(sequence_bias)
    return {tuple(q): v for q, v in sequence_bias}                     # (a repeated sequence: first place, last bias)


def _one_processor(entries, history, V):
    """float64 [V]: the bias one SequenceBiasLogitsProcessor adds for this history -- one-token entries ASSIGNED, then every longer
    entry that is not longer than the history and whose prefix is the history's tail ADDED, in the dict's order"""
    bias = np.zeros(V, dtype=np.float64)
    for q, v in entries.items():
        if len(q) == 1:
            bias[q[0]] = v
    for q, v in entries.items():
        if len(q) == 1 or len(q) > len(history):
            continue
        if list(history[len(history) - (len(q) - 1):]) == list(q[:-1]):
            bias[q[-1]] += v
    return bias


def bias_rows(sequence_bias, bad_words_ids, eos, history, V):
    """(float64 [V] bias of SequenceBias, float64 [V] bias of NoBadWords: 0 or -inf) for one row's history"""
    bad = {tuple(q): NEG for q in (bad_words_ids or []) if eos is None or list(q) != [eos]}
    return _one_processor(_as_dict(sequence_bias), history, V), _one_processor(bad, history, V)


def process_bias_row(x, history, sequence_bias=None, bad_words_ids=None, eos=None, penalty=1.0, ngram=0):
    """x float64 [V] -> float64 [V] after the reference's first four processors, in its order: SequenceBias, RepetitionPenalty,
    NoRepeatNGram, NoBadWords (a banned column holds -inf)"""
    V = x.shape[0]
    b1, b2 = bias_rows(sequence_bias, bad_words_ids, eos, history, V)
    out = x + torch.from_numpy(b1)
    out = hr.process_history_row(out, history, penalty, ngram)
    return out + torch.from_numpy(b2)


def select_bias_ref(logits, V, tokens, n, *, sequence_bias=None, bad_words_ids=None, suppress=None, begin_suppress=None, first=False,
                    no_eos=False, ts_begin=-1, max_initial=-1, begin_index=1, eos=-1, fill=-1, done=None, repetition_penalty=1.0,
                    no_repeat_ngram=0):
    """Token n of every row in float64: the four processors above on the widened logits, then the remaining processors of
    score_restatement.process_row with the mass rule decided in float64, argmax (the first of equal maxima), EOS / pad
    bookkeeping.  -> (next int64 [B], done bool [B], margins [B]: min(top-two distance of the processed row, distance of the
    mass rule from its threshold), rule sides [B]: True = the mass rule removed the text columns, None = it had nothing to
    compare)."""
    B = tokens.shape[0]
    toks = tokens.tolist()
    nxt, margins, sides = [], [], []
    new_done = torch.zeros(B, dtype=torch.bool) if done is None else done.clone().cpu()
    for b in range(B):
        x = process_bias_row(logits[b, :V].double().cpu(), toks[b][:n], sequence_bias, bad_words_ids, eos if eos >= 0 else None,
                             repetition_penalty, no_repeat_ngram)
        j = n - begin_index
        assert bool(first) == (j == 0)
        keep, rule = sr.process_row(x, toks[b][begin_index:n], j, V, suppress=suppress, begin_suppress=begin_suppress,
                                    min_new=10 ** 9 if no_eos else 0, ts_begin=ts_begin, max_initial=max_initial, eos=eos)
        y = torch.where(keep, x, torch.full_like(x, NEG))
        top = y.topk(2).values
        pick = int(y.argmax()) if bool(keep.any()) else 0
        margin = float(top[0] - top[1]) if bool(torch.isfinite(top[1])) else float("inf")
        margins.append(margin if rule is None else min(margin, rule))
        sides.append(None if rule is None else (ts_begin >= 0 and not bool(keep[:ts_begin].any())))
        if eos >= 0:
            if bool(new_done[b]):
                pick = fill
            if pick == eos:
                new_done[b] = True
        nxt.append(pick)
    return torch.tensor(nxt, dtype=torch.int64), new_done, margins, sides


class BiasRefOps(hr.HistoryRefOps):
    """HistoryRefOps + greedy_select_bias: the table is read back from the three flat tensors the decoder hands over (so the
    flattening is under test as well), applied per row by the rule above in fp32, the rest as HistoryRefOps."""

    def greedy_select_bias(self, logits, V, tokens, n, cur, *, suppress=None, begin_suppress=None, first=False, no_eos=False,
                           forced=False, ts_begin=-1, max_initial=-1, begin_index=1, eos=-1, fill=-1, done=None,
                           repetition_penalty=1.0, no_repeat_ngram=0, bias_tok=None, bias_off=None, bias_val=None):
        self.bias_calls = getattr(self, "bias_calls", 0) + 1
        if not forced:
            off, tok, val = bias_off.tolist(), bias_tok.tolist(), bias_val.tolist()
            cols = [tok[off[s + 1] - 1] for s in range(len(val))]
            assert cols == sorted(cols) and bias_tok.dtype == bias_off.dtype == torch.int32 and bias_val.dtype == torch.float32
            toks = tokens.tolist()
            rows = []
            for b in range(tokens.shape[0]):
                x = logits[b, :V].float().clone()
                h = toks[b][:n]
                col_sum = {}
                for s, v in enumerate(val):                              # table order: the order of the sums
                    q = tok[off[s]:off[s + 1]]
                    hit = len(q) == 1 or (len(q) <= len(h) and h[len(h) - (len(q) - 1):] == q[:-1])
                    col_sum[q[-1]] = np.float32(col_sum.get(q[-1], np.float32(0.0))) + np.float32(v if hit else 0.0)
                for c, v in col_sum.items():
                    x[c] = x[c] + float(v)
                rows.append(x)
            logits = torch.stack(rows)
        self.greedy_select_history(logits, V, tokens, n, cur, suppress=suppress, begin_suppress=begin_suppress, first=first,
                                   no_eos=no_eos, forced=forced, ts_begin=ts_begin, max_initial=max_initial, begin_index=begin_index,
                                   eos=eos, fill=fill, done=done, repetition_penalty=repetition_penalty,
                                   no_repeat_ngram=no_repeat_ngram)


# ---- fixture scenarios (the plumbing of history_restatement: same micro model, same inputs) ------------------------------------
fields_of, inputs_of, dropin, reference_model, run = hr.fields_of, hr.inputs_of, hr.dropin, hr.reference_model, hr.run
OPTIONS = ("sequence_bias", "bad_words_ids")


def without_options(kw):
    return {k: v for k, v in kw.items() if k not in OPTIONS}


assert gd.V == 1000
