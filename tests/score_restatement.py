"""TEST INFRASTRUCTURE -- torch restatement of the token-scoring entry point of libdwamd.so (csrc/score.hip) with the interface of
HipOps, for tests/test_generate_scores*.py: a subclass of oracle.ref_ops.RefOps that adds `score_tokens`, written from the
reference's logits processors (TF:generation/logits_process.py) row by row, in float64 unless told otherwise, plus the fixture's
scenario plumbing.  The product never imports this module."""
import json
import os

import numpy as np
import torch

from oracle import gen_golden_decode as gd
from oracle.ref_ops import RefOps

GOLD_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
NEG = float("-inf")


def gold():
    with open(os.path.join(GOLD_DIR, "generate_scores.json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(GOLD_DIR, "generate_scores.npz"))


def process_row(x, history, j, V, *, suppress=None, begin_suppress=None, min_new=0, ts_begin=-1, max_initial=-1, eos=-1):
    """One row through MinNewTokensLength, SuppressTokensAtBegin, SuppressTokens and WhisperTimeStamp, statement for statement.
    x: [V] (any float dtype; the mass rule is decided in that dtype), history: the j tokens generated so far (list).
    -> (bool [V]: column kept, margin of the mass rule or None when the rule has nothing to compare)."""
    sc = x.clone()
    if j < min_new and eos >= 0:
        sc[eos] = NEG
    if j == 0 and begin_suppress is not None:
        sc[begin_suppress[:V].bool()] = NEG
    if suppress is not None:
        sc[suppress[:V].bool()] = NEG
    margin = None
    if ts_begin >= 0:
        tb = ts_begin
        sc[tb - 1] = NEG
        last_ts = len(history) >= 1 and history[-1] >= tb
        pen_ts = len(history) < 2 or history[-2] >= tb
        if last_ts:
            if pen_ts:
                sc[tb:] = NEG
            else:
                sc[:eos] = NEG
        stamps = [t for t in history if t >= tb]
        if stamps:
            ts_last = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
            sc[tb:ts_last] = NEG
        if j == 0:
            sc[:tb] = NEG
            if max_initial >= 0:
                sc[tb + max_initial + 1:] = NEG
        lp = torch.log_softmax(sc, -1)
        ts_lp = lp[tb:].logsumexp(-1)
        text = lp[:tb].max()
        if bool(torch.isfinite(ts_lp)) and bool(torch.isfinite(text)):
            margin = abs(float(ts_lp - text))
        if bool(ts_lp > text):
            sc[:tb] = NEG
    return sc > NEG, margin


def score_tokens_ref(logits, V, tokens, begin_index, L, *, batch_rows=None, suppress=None, begin_suppress=None, min_new=0,
                     ts_begin=-1, max_initial=-1, eos=-1, dtype=torch.float64):
    """-> (scores f32 [L, B, V], chosen f32 [B, L], logprob f32 [B, L], smallest mass-rule margin per row [B][L] (None = no
    decision)).  A kept column holds the logit widened to fp32 -- exact for bf16 --, whatever `dtype` the decisions are made in."""
    B = tokens.shape[0]
    rows = int(L) if batch_rows is None else int(batch_rows)
    P = int(begin_index)
    scores = torch.full((L, B, V), NEG, dtype=torch.float32, device=logits.device)
    chosen = torch.full((B, L), NEG, dtype=torch.float32, device=logits.device)
    logprob = torch.full((B, L), NEG, dtype=torch.float32, device=logits.device)
    margins = [[None] * L for _ in range(B)]
    toks = tokens.tolist()
    for b in range(B):
        for j in range(L):
            raw = logits[b * rows + j, :V]
            keep, margins[b][j] = process_row(raw.to(dtype), toks[b][P:P + j], j, V, suppress=suppress,
                                              begin_suppress=begin_suppress, min_new=min_new, ts_begin=ts_begin,
                                              max_initial=max_initial, eos=eos)
            wide = raw.float()
            scores[j, b] = torch.where(keep, wide, torch.full_like(wide, NEG))
            t = toks[b][P + j]
            if 0 <= t < V and bool(keep[t]):
                chosen[b, j] = wide[t]
                lp = torch.log_softmax(torch.where(keep, raw.to(dtype), torch.full((V,), NEG, dtype=dtype, device=raw.device)), -1)
                logprob[b, j] = lp[t].float()
    return scores, chosen, logprob, margins


class ScoreRefOps(RefOps):
    """RefOps + score_tokens in torch (decisions and log-probabilities in float64)."""

    def score_tokens(self, logits, V, tokens, begin_index, L, *, batch_rows=None, suppress=None, begin_suppress=None, min_new=0,
                     ts_begin=-1, max_initial=-1, eos=-1, want_scores=True, want_chosen=True):
        sc, chosen, logprob, _ = score_tokens_ref(logits, V, tokens, begin_index, L, batch_rows=batch_rows, suppress=suppress,
                                                  begin_suppress=begin_suppress, min_new=min_new, ts_begin=ts_begin,
                                                  max_initial=max_initial, eos=eos)
        return (sc if want_scores else None), (chosen if want_chosen else None), (logprob if want_chosen else None)


# ---- fixture scenarios ------------------------------------------------------------------------------------------------------
def fields_of(sc):
    return gd.generation_fields(multilingual=True, suppress=True, timestamps=sc["ts_fields"])


def inputs_of(sc):
    return gd.features(sc["seed"] + 1, sc["B"])


def call_kwargs(sc, device="cpu"):
    kw = dict(sc["kwargs"])
    if "prompt_ids" in kw:
        kw["prompt_ids"] = torch.tensor(kw["prompt_ids"], device=device)
    return kw


def dropin(ops, sc, dtype=torch.float32):
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    m = WhisperForConditionalGeneration(gd.CFG_T, ops=ops, state_dict=gd.weights(sc["seed"]), dtype=dtype)
    m.generation_config = GenerationConfig.from_any(fields_of(sc))
    return m


def run_dropin(ops, sc, model=None, **extra):
    m = model if model is not None else dropin(ops, sc)
    out = m.generate(inputs_of(sc).to(ops.device), return_dict_in_generate=True, output_scores=True, output_logits=True,
                     **call_kwargs(sc, ops.device), **extra)
    return m, out


def stacked(steps):
    """tuple of [B, V] -> numpy f32 [L, B, V]"""
    return torch.stack(tuple(steps), 0).float().cpu().numpy()
