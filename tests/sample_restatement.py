"""TEST INFRASTRUCTURE -- numpy restatement of the sampled selection entry of libdwamd.so (`dw_sample_select`, csrc/decode.hip)
for tests/test_sample_select*.py and tools/gen_golden_sample_select.py.  It states the six steps of the entry row by row, from the
reference's processors and warpers (TF:generation/logits_process.py) and `_sample` (TF:generation/utils.py):

  1. processed score: repetition penalty, banned n-gram columns, the min-new-tokens EOS ban, begin-suppress, suppress, the
     timestamp intervals, the timestamp mass rule (decided in float64); excluded = -inf;
  2. s / temperature, an IEEE fp32 division;
  3. top-k: columns below the k-th largest of all V scores go, ties at the threshold stay;
  4. top-p: a column goes iff the probability of all columns with a score <= its own is <= 1 - top_p; the largest stays.  (The
     reference removes a prefix of an ascending sort and so splits the group of equal scores at the boundary; `split_groups=True`
     states that instead, in the order numpy's stable sort gives -- the fixture generator uses it to find rows where it matters);
  5. the draw: argmax of softmax(s) / noise over the surviving columns, the first of equal quotients; no column at all: 0;
  6. EOS bookkeeping: a finished row takes `fill`, a row that draws EOS is finished.

With each token come three margins; a row is "near" when a few-ulp difference in `exp` or a division could move its token:
  quotient: relative gap between the best and the second-best quotient of the draw           (near below 1e-4)
  boundary: distance of a score group's cumulative mass from 1 - top_p, the closest group    (near below 1e-5)
  mass:     distance of the timestamp mass rule from its threshold                           (near below 1e-3)
The product never imports this module."""
import base64
import json
import os

import numpy as np

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sample_select.json")
NEAR = dict(quotient=1e-4, boundary=1e-5, mass=1e-3)
NEG = np.float32(-np.inf)


def gold():
    with open(GOLD) as f:
        return json.load(f)


# ---- bit patterns of the fixture (base64 of the little-endian words) --------------------------------------------------------
def bf16_pack(x):
    """float32 array holding bf16 values -> base64 of their 16-bit patterns"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    assert not np.any(u & 0xffff), "values are not bf16"
    return base64.b64encode((u >> 16).astype("<u2").tobytes()).decode()


def bf16_unpack(s, shape):
    u = np.frombuffer(base64.b64decode(s), dtype="<u2").astype(np.uint32) << 16
    return u.view(np.float32).reshape(shape)


def f32_pack(x):
    return base64.b64encode(np.ascontiguousarray(x, dtype="<f4").tobytes()).decode()


def f32_unpack(s, shape):
    return np.frombuffer(base64.b64decode(s), dtype="<f4").astype(np.float32).reshape(shape)


# ---- step 1 ---------------------------------------------------------------------------------------------------------------
def banned_ids(history, g):
    """NoRepeatNGramLogitsProcessor: the ids that would complete an n-gram of size g the row already holds"""
    n = len(history)
    if g <= 0 or n + 1 < g:
        return set()
    tail = tuple(history[n - g + 1:n])
    return {history[i + g - 1] for i in range(n - g + 1) if tuple(history[i:i + g - 1]) == tail}


def processed_row(x, history, gen, V, *, suppress=None, begin_suppress=None, first=False, no_eos=False, ts_begin=-1,
                  max_initial=-1, eos=-1, repetition_penalty=1.0, no_repeat_ngram=0):
    """x f32 [V] raw logits, history: every token of the row so far (prompt included), gen: the generated part of it.
    -> (processed scores f32 [V], margin of the mass rule or inf)"""
    s = np.array(x[:V], dtype=np.float32)
    p = np.float32(repetition_penalty)
    if float(p) != 1.0:
        for t in set(history):
            if 0 <= t < V:
                s[t] = x[t] * p if x[t] < 0 else x[t] / p
    for t in banned_ids(list(history), int(no_repeat_ngram)):
        if 0 <= t < V:
            s[t] = NEG
    if no_eos and eos >= 0:
        s[eos] = NEG
    if first and begin_suppress is not None:
        s[np.asarray(begin_suppress[:V]).astype(bool)] = NEG
    if suppress is not None:
        s[np.asarray(suppress[:V]).astype(bool)] = NEG
    margin = np.inf
    if ts_begin >= 0:
        tb = ts_begin
        s[tb - 1] = NEG
        last_ts = len(gen) >= 1 and gen[-1] >= tb
        pen_ts = len(gen) < 2 or gen[-2] >= tb
        if last_ts:
            if pen_ts:
                s[tb:] = NEG
            else:
                s[:eos] = NEG
        stamps = [t for t in gen if t >= tb]
        if stamps:
            ts_last = stamps[-1] if (last_ts and not pen_ts) else stamps[-1] + 1
            s[tb:ts_last] = NEG
        if len(gen) == 0:
            s[:tb] = NEG
            if max_initial >= 0:
                s[tb + max_initial + 1:] = NEG
        ts, text = s[tb:].astype(np.float64), s[:tb].astype(np.float64)
        if np.isfinite(ts).any():
            m = ts.max()
            ts_lse = m + np.log(np.exp(ts - m).sum())
            text_max = text.max() if text.size else -np.inf
            if np.isfinite(text_max):
                margin = abs(ts_lse - text_max)
            if ts_lse > text_max:
                s[:tb] = NEG
    return s, margin


# ---- steps 2 - 5 ----------------------------------------------------------------------------------------------------------
def warp_row(s, temperature=1.0, top_k=0, top_p=1.0, split_groups=False):
    """-> (warped scores f32 [V], distance of the closest group's cumulative mass from 1 - top_p, or inf)"""
    s = (s / np.float32(temperature)).astype(np.float32)
    V = s.shape[0]
    if top_k > 0:
        k = min(int(top_k), V)
        kth = np.sort(s)[V - k]
        s = np.where(s < kth, NEG, s)
    boundary = np.inf
    if top_p < 1.0 and np.isfinite(s).any():
        order = np.argsort(s, kind="stable")                       # ascending
        srt = s[order].astype(np.float64)
        e = np.exp(srt - srt[-1])
        cum = np.cumsum(e / e.sum())
        if not split_groups:
            # the mass of every column with a score <= this one: the cumulative sum at the last column of its group
            last = np.r_[srt[1:] != srt[:-1], True]
            idx = np.where(last, np.arange(V), V)
            idx = np.minimum.accumulate(idx[::-1])[::-1]
            cum = cum[idx]
        remove = cum <= 1.0 - float(top_p)
        remove[-1] = False
        live = np.isfinite(srt)
        live[-1] = False                                           # (the largest stays wherever its mass lies)
        if live.any():
            boundary = float(np.abs(cum[live] - (1.0 - float(top_p))).min())
        s = s.copy()
        s[order[remove]] = NEG
    return s, boundary


def draw_row(s, noise):
    """-> (column, relative gap to the second-best quotient); no surviving column: (0, inf)"""
    keep = np.isfinite(s)
    if not keep.any():
        return 0, np.inf
    z = s.astype(np.float64)
    e = np.where(keep, np.exp(z - z[keep].max()), 0.0)
    quot = np.where(keep, (e / e.sum()) / noise.astype(np.float64), -np.inf)
    best = int(np.argmax(quot))                                    # (the first of equal maxima)
    rest = np.delete(quot, best)
    second = rest.max() if rest.size else -np.inf
    gap = np.inf if not np.isfinite(second) else float((quot[best] - second) / quot[best]) if quot[best] > 0 else 0.0
    return best, gap


def sample_select_ref(logits, noise, V, tokens, n, *, suppress=None, begin_suppress=None, first=False, no_eos=False, ts_begin=-1,
                      max_initial=-1, begin_index=1, eos=-1, fill=-1, done=None, repetition_penalty=1.0, no_repeat_ngram=0,
                      temperature=1.0, top_k=0, top_p=1.0, split_groups=False):
    """logits f32 [B, >= V] (bf16 values), noise f32 [B, >= V], tokens int [B, >= n].
    -> (next int64 [B], done bool [B], margins: dict of three float arrays [B])"""
    logits, noise, tokens = np.asarray(logits, dtype=np.float32), np.asarray(noise, dtype=np.float32), np.asarray(tokens)
    B = tokens.shape[0]
    new_done = np.zeros(B, dtype=bool) if done is None else np.array(done, dtype=bool)
    nxt = np.zeros(B, dtype=np.int64)
    margins = {k: np.full(B, np.inf) for k in NEAR}
    for b in range(B):
        if eos >= 0 and new_done[b]:
            nxt[b] = fill
            continue
        hist = [int(t) for t in tokens[b, :n]]
        s, margins["mass"][b] = processed_row(
            logits[b], hist, hist[begin_index:], V, suppress=suppress, begin_suppress=begin_suppress, first=first, no_eos=no_eos,
            ts_begin=ts_begin, max_initial=max_initial, eos=eos, repetition_penalty=repetition_penalty,
            no_repeat_ngram=no_repeat_ngram)
        s, margins["boundary"][b] = warp_row(s, temperature, top_k, top_p, split_groups)
        nxt[b], margins["quotient"][b] = draw_row(s, noise[b, :V])
        if eos >= 0 and nxt[b] == eos:
            new_done[b] = True
    return nxt, new_done, margins


def near(margins):
    """bool [B]: the row's token could move under a few-ulp difference in exp / division"""
    return np.logical_or.reduce([margins[k] < NEAR[k] for k in NEAR])


def exponential_noise(shape, seed):
    """what the decoder draws: `empty(shape).exponential_(1, generator)` on the CPU generator of `seed`"""
    import torch
    g = torch.Generator().manual_seed(int(seed))
    return torch.empty(shape, dtype=torch.float32).exponential_(1.0, generator=g).numpy()
