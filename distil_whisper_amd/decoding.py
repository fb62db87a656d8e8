"""Batched greedy KV-cache decoding on the engine, with the per-token launch sequence captured in HIP graphs.

Reference behaviour: `model.generate(...)` as called by run_distillation.py:1524-1528 (`generate_step`) and
run_eval.py:739 / 806-844 (`benchmark_gen`: fixed number of new tokens on random encoder input) with greedy search
(`num_beams=1`, `top_k=0`): TF:generation_whisper.py:383 + the cache branches of TF:modeling_whisper.py:312-335, with
the `SuppressTokensLogitsProcessor` / `SuppressTokensAtBeginLogitsProcessor` steps (TF:generation_whisper.py:1774-1812).

One decoding step of the 2-layer student is ~30 kernel launches of a few microseconds each with M = batch rows, i.e.
launch-latency bound when driven from Python.  Every token position t has fixed shapes (cache length t+1, position
embedding row t), so the step for position t is captured once into a HIP graph and replayed for every later batch of
chunks; all tensors the graphs touch (current ids, token matrix, done flags, K/V caches) are allocated once.
"""
import os

import torch

from . import kv_quant

# DW_SAMPLE_TORCH=1 (read when a decoder is built): sampling stays on the torch ops of `_select_soft` on every engine, as on ops
# without `sample_select` -- the A/B leg of tools/bench_sample_select.py and the reference leg of tests/test_sample_select_gpu.py
SAMPLE_TORCH_ENV = "DW_SAMPLE_TORCH"


def apply_timestamp_rules(scores, tokens, n, begin_index, no_timestamps_token_id, eos_token_id,
                          max_initial_timestamp_index=None, return_rule_margin=False):
    """The decoding rules of `WhisperTimeStampLogitsProcessor` (TF:generation/logits_process.py; installed by
    TF:generation_whisper.py:1774-1812 when `return_timestamps=True`, run_eval.py:690-739) on a whole batch without
    host round trips: scores f32 [B, V] (modified copy returned), tokens int64 [B, >= n] of which the first n are
    the sequence so far (prompt included), begin_index = length of the forced prefix.
      * <|notimestamps|> is never sampled;
      * timestamps come in pairs: after text+timestamp only a timestamp or EOS may follow, after two timestamps only
        text; a timestamp may not be smaller than the last one emitted (nor repeat it when it closed a pair);
      * the first sampled token must be a timestamp, at most `max_initial_timestamp_index` steps in;
      * if the timestamps together are more probable than the most probable text token, a timestamp is sampled."""
    sc = scores.clone()
    B, V = sc.shape
    tb = no_timestamps_token_id + 1
    neg = float("-inf")
    col = torch.arange(V, device=sc.device)[None, :]
    sc[:, no_timestamps_token_id] = neg
    L = n - begin_index
    if L >= 1:
        last_ts = tokens[:, n - 1] >= tb
        pen_ts = tokens[:, n - 2] >= tb if L >= 2 else torch.ones_like(last_ts)
        sc = sc.masked_fill((last_ts & pen_ts)[:, None] & (col >= tb), neg)
        sc = sc.masked_fill((last_ts & ~pen_ts)[:, None] & (col < eos_token_id), neg)
        seq = tokens[:, begin_index:n]
        is_ts = seq >= tb
        any_ts = is_ts.any(1)
        pos = (is_ts.long() * torch.arange(1, L + 1, device=sc.device)[None, :]).max(1).values   # 1-based, 0 = none
        last_val = seq.gather(1, (pos - 1).clamp(min=0)[:, None])[:, 0]
        ts_last = torch.where(last_ts & ~pen_ts, last_val, last_val + 1)
        sc = sc.masked_fill(any_ts[:, None] & (col >= tb) & (col < ts_last[:, None]), neg)
    if L == 0:
        sc = sc.masked_fill(col < tb, neg)
        if max_initial_timestamp_index is not None:
            sc = sc.masked_fill(col > tb + max_initial_timestamp_index, neg)
    lp = torch.log_softmax(sc.float(), dim=-1)
    ts_lp = lp[:, tb:].logsumexp(-1)
    text_max = lp[:, :tb].max(-1).values
    out = sc.masked_fill((ts_lp > text_max)[:, None] & (col < tb), neg)
    if return_rule_margin:          # distance of the probability-mass decision from its threshold (fixture generator)
        return out, (ts_lp - text_max).abs()
    return out


def apply_repetition_penalty(scores, input_ids, penalty):
    """`RepetitionPenaltyLogitsProcessor` (TF:generation/logits_process.py): the scores of every token already in the row's
    sequence (prompt included) are divided by `penalty` when positive and multiplied when negative."""
    sc = torch.gather(scores, 1, input_ids)
    sc = torch.where(sc < 0, sc * penalty, sc / penalty)
    return scores.scatter(1, input_ids, sc)


def apply_no_repeat_ngram(scores, input_ids, n):
    """`NoRepeatNGramLogitsProcessor`: a token that would complete an n-gram the row's sequence already contains is banned.
    Vectorised: every window of n-1 tokens equal to the sequence's last n-1 tokens bans the token that followed it."""
    B, L = input_ids.shape
    if n <= 0 or L + 1 < n:
        return scores
    if n == 1:
        return scores.scatter(1, input_ids, float("-inf"))
    tail = input_ids[:, L - (n - 1):]                                     # [B, n-1]
    win = input_ids.unfold(1, n - 1, 1)[:, : L - (n - 1)]                  # [B, L-n+1, n-1]: windows that HAVE a follower
    hit = (win == tail[:, None, :]).all(-1)                               # [B, L-n+1]
    follow = input_ids[:, n - 1:]                                          # [B, L-n+1]
    # (several windows may name the same token: any hit bans it)
    ban_any = torch.zeros_like(scores, dtype=torch.int32).scatter_add_(1, follow, hit.to(torch.int32)) > 0
    return scores.masked_fill(ban_any, float("-inf"))


# caps of the selection kernel's bias table, stated here once: sequences (csrc/select_rules.h SEL_BIAS_S: one thread each, the C
# entry refuses more) and tokens per sequence (a host cap only: the kernel compares any length up to the history's)
SEQUENCE_BIAS_MAX_SEQUENCES, SEQUENCE_BIAS_MAX_TOKENS = 1024, 32


class SequenceBiasTable:
    """`sequence_bias` / `bad_words_ids` of one `generate` call, validated and flattened (`sequence_bias_table`): seqs -- tuples
    of token ids -- and vals -- their biases, -inf for a bad word -- in TABLE ORDER: ascending by the column (last token), within
    a column the one-token entry first, then the caller's order, bad words last.  That is the order in which the reference adds
    a column's biases up (`length_1_bias` first, then the dict's order; NoBadWords is a later processor), so the sum is the
    reference's bit for bit.  `tensors(device)`: tok int32 [T], off int32 [S + 1], val f32 [S] for `greedy_select_bias`.
    Hashable by content (a decoder is cached under its options)."""

    def __init__(self, seqs, vals):
        self.seqs, self.vals = tuple(tuple(int(t) for t in q) for q in seqs), tuple(float(v) for v in vals)
        self.S = len(self.seqs)
        self._dev = {}

    def __eq__(self, other):
        return isinstance(other, SequenceBiasTable) and (self.seqs, self.vals) == (other.seqs, other.vals)

    def __hash__(self):
        return hash((self.seqs, self.vals))

    def __repr__(self):
        return f"SequenceBiasTable({self.S} sequences)"

    def tensors(self, device):
        key = str(device)
        if key not in self._dev:
            off = [0]
            for q in self.seqs:
                off.append(off[-1] + len(q))
            self._dev[key] = dict(
                bias_tok=torch.tensor([t for q in self.seqs for t in q], dtype=torch.int32, device=device),
                bias_off=torch.tensor(off, dtype=torch.int32, device=device),
                bias_val=torch.tensor(self.vals, dtype=torch.float32, device=device))
        return self._dev[key]


def sequence_bias_table(sequence_bias, bad_words_ids, vocab, eos_token_id=None):
    """`generate(sequence_bias=, bad_words_ids=)` -> SequenceBiasTable, or None when neither names a sequence.  Host only.  It
    refuses everything the reference refuses, with the reference's messages, and MORE, EARLIER: an empty token list, a list-form
    element that is no (tokens, bias) pair -- the reference lets those through and fails inside its first step -- and an id >= vocab,
    which the reference reports at its first step, are refused here before anything is decoded.  The checks it shares are the reference's (`SequenceBiasLogitsProcessor._validate_arguments` / `_prepare_bias_variables`,
    `NoBadWordsLogitsProcessor`, TF:generation/logits_process.py): the list form becomes a dict -- a repeated sequence keeps its
    first place and its last bias, which is also how one-token duplicates end up ASSIGNED, not summed --, bad words that are
    exactly `[eos]` are dropped, an id >= vocab raises.  Beyond the kernel's caps (1024 sequences of at most 32 tokens) and for a
    bias that is NaN or +inf: NotImplementedError."""
    import numpy as np
    is_id = lambda t: isinstance(t, (int, np.integer))                                  # noqa: E731
    entries = []                                                                        # (sequence, bias, rank within a column)
    if sequence_bias is not None:
        sb = sequence_bias
        if not isinstance(sb, dict) and not isinstance(sb, list) or len(sb) == 0:
            raise ValueError(f"`sequence_bias` has to be a non-empty dictionary, or non-empty list of lists but is {sb}.")
        if isinstance(sb, dict):
            if any(not isinstance(q, tuple) for q in sb):
                raise ValueError(f"`sequence_bias` has to be a dict with tuples as keys, but is {sb}.")
            if any(any(not is_id(t) or t < 0 for t in q) or len(q) == 0 for q in sb):
                raise ValueError(f"Each key in `sequence_bias` has to be a non-empty tuple of positive integers, but is {sb}.")
            if any(not isinstance(v, float) for v in sb.values()):
                raise ValueError(f"`sequence_bias` has to be a dict with floats as values, but is {sb}.")
            as_dict = dict(sb)
        else:
            def pair_ok(e):
                return (isinstance(e, (list, tuple)) and len(e) == 2 and isinstance(e[0], list) and len(e[0]) > 0
                        and all(is_id(t) and t > 0 for t in e[0]) and isinstance(e[1], float))
            if any(not pair_ok(e) for e in sb):
                raise ValueError("Each element in `sequence_bias` has to be a non-empty list of lists of positive integers and "
                                 f"float, but is {sb}.")
            as_dict = {tuple(e[0]): e[1] for e in sb}
        entries += [(q, v, 0 if len(q) == 1 else 1) for q, v in as_dict.items()]
    if bad_words_ids is not None:
        bw = bad_words_ids
        if not isinstance(bw, list) or len(bw) == 0:
            raise ValueError(f"`bad_words_ids` has to be a non-empty list, but is {bw}.")
        if any(not isinstance(q, list) for q in bw):
            raise ValueError(f"`bad_words_ids` has to be a list of lists, but is {bw}.")
        if any(any(not is_id(t) or t < 0 for t in q) for q in bw):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
        if any(len(q) == 0 for q in bw):
            raise ValueError(f"Each list in `bad_words_ids` has to be a list of positive integers, but is {bw}.")
        eos = [] if eos_token_id is None else ([int(eos_token_id)] if is_id(eos_token_id) else [int(t) for t in eos_token_id])
        entries += [(q, float("-inf"), 2) for q in {tuple(q): None for q in bw if not any(list(q) == [e] for e in eos)}]
    for _, group in ((0, [e for e in entries if e[2] < 2]), (1, [e for e in entries if e[2] == 2])):   # (per processor, as there)
        invalid = [t for q, _, _ in group for t in q if t >= vocab]
        if invalid:
            raise ValueError(f"The model vocabulary size is {vocab}, but the following tokens were being biased: {invalid}")
    if not entries:
        return None
    if len(entries) > SEQUENCE_BIAS_MAX_SEQUENCES or any(len(q) > SEQUENCE_BIAS_MAX_TOKENS for q, _, _ in entries):
        raise NotImplementedError(
            f"sequence_bias / bad_words_ids: at most {SEQUENCE_BIAS_MAX_SEQUENCES} sequences of at most {SEQUENCE_BIAS_MAX_TOKENS} "
            f"tokens each are implemented on the MI355X path (got {len(entries)} sequences, the longest of "
            f"{max(len(q) for q, _, _ in entries)} tokens)")
    if any(v != v or v == float("inf") for _, v, _ in entries):
        raise NotImplementedError("sequence_bias: a bias of NaN or +inf is not implemented on the MI355X path")
    order = sorted(range(len(entries)), key=lambda i: (entries[i][0][-1], entries[i][2], i))
    return SequenceBiasTable([entries[i][0] for i in order], [entries[i][1] for i in order])


def apply_sequence_bias(scores, input_ids, table):
    """`SequenceBiasLogitsProcessor` and `NoBadWordsLogitsProcessor` (TF:generation/logits_process.py) on scores f32 [rows, V] with
    the history input_ids int64 [rows, n] (decoder prompt included), table: SequenceBiasTable.  The reference's rule to the letter:
    a one-token sequence always counts; a longer one is ignored when len(sequence) > n, else it counts iff the last len - 1 tokens
    of the history equal its prefix; the biases that count are summed per column first (a sequence that does not count adds 0.0)
    and the sum is added to the scores once.  A bad word is a bias of -inf: its processor stands behind the repetition rules in
    the reference's list, but nothing brings a -inf back, so one pass in front gives the same scores."""
    n = input_ids.shape[1]
    bias = torch.zeros_like(scores)
    zero = torch.zeros((), dtype=scores.dtype, device=scores.device)
    for seq, v in zip(table.seqs, table.vals):
        if len(seq) == 1:
            bias[:, seq[0]] += v
            continue
        if len(seq) > n:
            continue
        pre = torch.tensor(seq[:-1], dtype=input_ids.dtype, device=input_ids.device)
        match = (input_ids[:, n - len(pre):] == pre[None, :]).all(1)
        bias[:, seq[-1]] += torch.where(match, torch.full_like(zero, v), zero)
    return scores + bias


def warp_and_sample(scores, temperature=None, top_k=None, top_p=None, generator=None):
    """The sampling tail of `GenerationMixin._sample`: TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper (in
    that order, TF `_get_logits_processor`), softmax, one `torch.multinomial` draw per row."""
    sc = scores
    if temperature is not None and float(temperature) != 1.0:
        sc = sc / float(temperature)
    if top_k is not None and int(top_k) > 0:
        k = min(int(top_k), sc.shape[-1])
        kth = torch.topk(sc, k)[0][..., -1, None]
        sc = sc.masked_fill(sc < kth, float("-inf"))
    if top_p is not None and float(top_p) < 1.0:
        srt, idx = torch.sort(sc, descending=False)
        cum = srt.softmax(-1).cumsum(-1)
        remove = cum <= (1.0 - float(top_p))
        remove[..., -1:] = False                                          # min_tokens_to_keep = 1
        sc = sc.masked_fill(remove.scatter(1, idx, remove), float("-inf"))
    probs = torch.softmax(sc, dim=-1)
    return torch.multinomial(probs, num_samples=1, generator=generator)[:, 0]


def rule_kwargs(timestamp_rules, eos):
    """The keyword arguments by which the token-selection entries of `ops` take the timestamp rules (the dict given to
    GreedyDecoder, or None) and the EOS id (None: no EOS bookkeeping)."""
    r = timestamp_rules
    mi = None if r is None else r.get("max_initial_timestamp_index")
    return dict(ts_begin=-1 if r is None else int(r["no_timestamps_token_id"]) + 1, max_initial=-1 if mi is None else int(mi),
                begin_index=1 if r is None else int(r.get("begin_index", 1)), eos=-1 if eos is None else int(eos))


def token_mask(ids, V, device, dtype=torch.bool):
    """Token ids as a mask over the vocabulary: `dtype` [V], 1 at every id that lies in [0, V); None when none does.  An id beyond
    the vocabulary names no column and is dropped, as by the reference's `torch.isin(arange(V), ids)` (SuppressTokensLogitsProcessor)."""
    ids = sorted({int(t) for t in ([] if ids is None else ids) if 0 <= int(t) < V})
    if not ids:
        return None
    m = torch.zeros((V,), dtype=dtype, device=device)
    m[torch.as_tensor(ids, dtype=torch.long, device=device)] = 1
    return m


def processed_scores(scores, hist, n, *, begin_index, eos=None, no_eos=False, first=False, suppress=None, begin_suppress=None,
                     timestamp_rules=None, repetition_penalty=None, no_repeat_ngram=0, sequence_bias=None):
    """The scores of one step after the reference's logits processors, in its order (TF `_get_logits_processor`, then
    TF:generation_whisper.py:1774-1812): SequenceBias (with NoBadWords: `sequence_bias`, a SequenceBiasTable or None,
    `apply_sequence_bias`), RepetitionPenalty, NoRepeatNGram, MinNewTokensLength, SuppressTokensAtBegin, SuppressTokens,
    WhisperTimeStamp -> f32 [rows, V].  This is the one torch statement of what the selection kernels judge (csrc/select_rules.h):
    every torch path of the package and oracle.ref_ops select from it.  scores [rows, V] (logits, or their log-softmax under beam
    search; left unchanged); hist int64 [rows, >= n] of which the first n are the sequence so far, decoder prompt of `begin_index`
    tokens included; no_eos: fewer than min_new_tokens generated, EOS (`eos`, None: there is none) is excluded; first: position n
    is the first generated one, where `begin_suppress` counts; suppress / begin_suppress: bool or uint8 [>= V], non-zero = excluded
    (`token_mask`), or None; timestamp_rules: None or dict(no_timestamps_token_id, max_initial_timestamp_index)."""
    neg = float("-inf")
    V = scores.shape[-1]
    sc = scores.float()
    if sequence_bias is not None:
        sc = apply_sequence_bias(sc, hist[:, :n], sequence_bias)
    if repetition_penalty is not None and float(repetition_penalty) != 1.0:
        sc = apply_repetition_penalty(sc, hist[:, :n], float(repetition_penalty))
    if no_repeat_ngram:
        sc = apply_no_repeat_ngram(sc, hist[:, :n], int(no_repeat_ngram))
    if no_eos and eos is not None and 0 <= eos < V:
        sc = sc.clone()
        sc[:, eos] = neg
    if first and begin_suppress is not None:
        sc = sc.masked_fill(begin_suppress[:V].bool()[None, :], neg)
    if suppress is not None:
        sc = sc.masked_fill(suppress[:V].bool()[None, :], neg)
    if timestamp_rules is not None:
        sc = apply_timestamp_rules(sc, hist, n, int(begin_index), int(timestamp_rules["no_timestamps_token_id"]), eos,
                                   timestamp_rules.get("max_initial_timestamp_index"))
    return sc


def greedy_no_cache(engine, V, enc, ids, max_new, min_new, eos, pad, suppress, begin_suppress):
    """Greedy search that re-decodes the whole prefix at every step (no KV cache): the cross-check of the cached
    decoder."""
    B, dev = ids.shape[0], ids.device
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    sup, bsup = (token_mask(t, V, dev) for t in (suppress, begin_suppress))
    for step in range(max_new):
        T = ids.shape[1]
        logits, _ = engine.decode(ids.contiguous(), enc, save=False)
        sc = logits[: B * T, :V].view(B, T, -1)[:, -1].float()
        nxt = processed_scores(sc, ids, T, begin_index=T - step, eos=eos, no_eos=step < min_new, first=step == 0, suppress=sup,
                               begin_suppress=bsup).argmax(-1)
        if eos is not None:
            nxt = torch.where(done, torch.full_like(nxt, pad), nxt)
            done |= nxt == eos
        ids = torch.cat([ids, nxt[:, None]], 1)
        if eos is not None and bool(done.all()):
            break
    return ids


class GreedyDecoder:
    def __init__(self, engine, batch, max_len, eos_token_id=None, suppress_tokens=None, begin_suppress_tokens=None,
                 use_graphs=None, check_every=16, timestamp_rules=None, pad_token_id=None, soft=None, cross_kv_dtype=None):
        self.eng, self.B, self.max_len = engine, int(batch), int(max_len)
        d = engine.dims
        # "fp8": the cross-attention K/V of the cache as e4m3fn codes with column scales (engine.decode_init; include/dwamd.h) --
        # opt-in, it changes the numerics of the token step; None / "bf16": the cache as it always was
        self.cross_kv_dtype = kv_quant.normalize_dtype(cross_kv_dtype)
        if self.cross_kv_dtype is not None:
            kv_quant.check_width(d.d_model)
        if self.max_len > d.max_tgt:
            raise ValueError(f"max_len = {max_len} exceeds max_target_positions = {d.max_tgt}")
        dev = engine.ops.device
        self.dev = dev
        self.eos = eos_token_id
        self.use_graphs = (torch.device(dev).type == "cuda") if use_graphs is None else bool(use_graphs)
        self.check_every = int(check_every)
        self.tokens = torch.zeros((self.B, self.max_len), dtype=torch.long, device=dev)
        self.cur = torch.zeros((self.B, 1), dtype=torch.long, device=dev)
        self.done = torch.zeros((self.B,), dtype=torch.bool, device=dev)

        self.suppress = token_mask(suppress_tokens, d.vocab, dev, torch.uint8)
        self.begin_suppress = token_mask(begin_suppress_tokens, d.vocab, dev, torch.uint8)
        # dict(begin_index=, no_timestamps_token_id=, max_initial_timestamp_index=): WhisperTimeStampLogitsProcessor
        self.timestamp_rules = timestamp_rules
        if timestamp_rules is not None and eos_token_id is None:
            raise ValueError("timestamp rules need eos_token_id")
        self.fill = -1 if eos_token_id is None else (eos_token_id if pad_token_id is None else pad_token_id)
        # soft = dict(do_sample=, temperature=, top_k=, top_p=, repetition_penalty=, no_repeat_ngram_size=, generator=):
        # history-dependent processors and sampling of `GenerationMixin` (TF `_get_logits_processor` order: repetition
        # penalty, no-repeat n-gram, min-new-tokens, Whisper's suppress / begin-suppress / timestamp rules, then the
        # temperature / top-k / top-p warpers and the multinomial draw).
        # Without sampling the two history rules run inside the selection kernel (dw_greedy_select_history: the history is the
        # `tokens` buffer the kernel reads anyway, so the step stays one launch and is captured into the per-position graphs
        # like the plain one).  Sampling runs inside the selection kernel as well (dw_sample_select: processors, warpers and the
        # draw in one launch, captured like the others).  For one draw per row `torch.multinomial(probs, 1, generator=g)` is
        # `argmax(probs / q)` with `q = empty_like(probs).exponential_(1, generator=g)` on every device, so the only torch op
        # left is that `exponential_` into the static `noise` buffer [B, V] -- the shape of `probs`, so the generator advances as
        # on the torch path --, launched in front of every replay: outside the graph, hence no graph-safe generator registration.
        # soft["sequence_bias"] (a SequenceBiasTable: `generate(sequence_bias=, bad_words_ids=)`): greedy decoding applies it, with
        # the two history rules, inside the selection kernel (dw_greedy_select_bias; the table is three static device tensors, so
        # the step is captured like the others); sampling with a table takes the torch ops.
        # On ops without these entries (the torch restatement oracle.ref_ops), or with DW_SAMPLE_TORCH=1 for sampling, the
        # selection runs as torch ops on the step's logits, eagerly, without HIP-graph replay.
        # Generator state: both paths draw once per generated position and leave the loop at the same `check_every` boundary, so
        # they consume the generator identically; nothing has to be restored.
        self.soft = soft
        self.history = None
        self.bias = None
        self.sample = None
        self.noise = None
        if soft is not None:
            rp, ng = soft.get("repetition_penalty"), int(soft.get("no_repeat_ngram_size") or 0)
            rp = 1.0 if rp is None else float(rp)
            table = soft.get("sequence_bias")
            if table is not None:
                if not soft.get("do_sample") and hasattr(engine.ops, "greedy_select_bias"):
                    self.bias = dict(repetition_penalty=rp, no_repeat_ngram=ng, **table.tensors(dev))
                else:
                    self.use_graphs = False
            elif not soft.get("do_sample") and (rp != 1.0 or ng) and hasattr(engine.ops, "greedy_select_history"):
                self.history = dict(repetition_penalty=rp, no_repeat_ngram=ng)
            elif soft.get("do_sample") and hasattr(engine.ops, "sample_select") and os.environ.get(SAMPLE_TORCH_ENV, "0") in ("", "0"):
                t, k, p = soft.get("temperature"), soft.get("top_k"), soft.get("top_p")
                self.sample = dict(repetition_penalty=rp, no_repeat_ngram=ng, temperature=1.0 if t is None else float(t),
                                   top_k=0 if k is None else max(0, int(k)), top_p=1.0 if p is None else min(1.0, float(p)))
                self.noise = torch.empty((self.B, d.vocab), dtype=torch.float32, device=dev)
            else:
                self.use_graphs = False
        self.cache = None
        self.graphs = {}
        self.pool = None
        self._warm = False

    # mode 0: position t+1 is still inside the prompt (teacher forcing); 1: first generated token; 2: later tokens
    def _step(self, t, mode, no_eos=False):
        eng, d = self.eng, self.eng.dims
        self.cache["t"] = t
        logits = eng.decode_step(self.cur, self.cache)
        if self.soft is not None and self.history is None and self.sample is None and self.bias is None and mode != 0:
            self._select_soft(logits, t + 1, mode, no_eos)
            return
        # logits processors of the reference (min-new-tokens, begin-suppress, suppress, timestamp rules), the choice of the
        # token and the EOS bookkeeping in one launch (csrc/decode.hip); the next token lands in tokens[:, t+1] and in cur
        ops, args = eng.ops, (logits, d.vocab, self.tokens, t + 1, self.cur)
        common = dict(suppress=self.suppress, begin_suppress=self.begin_suppress, first=(mode == 1), no_eos=no_eos,
                      fill=self.fill, done=self.done, **rule_kwargs(self.timestamp_rules, self.eos))
        if self.sample is not None and mode != 0:
            # (`noise` holds this position's draw: `_run_step` filled it just before this launch / this graph's replay)
            ops.sample_select(*args, self.noise, **common, **self.sample)
        elif self.bias is not None:
            ops.greedy_select_bias(*args, forced=(mode == 0), **common, **self.bias)
        elif self.history is not None:
            ops.greedy_select_history(*args, forced=(mode == 0), **common, **self.history)
        else:
            ops.greedy_select(*args, forced=(mode == 0), **common)

    def _select_soft(self, logits, n, mode, no_eos):
        """Token n of every row from `logits` with the history-dependent processors / sampling of `self.soft`."""
        d, so, r = self.eng.dims, self.soft, self.timestamp_rules
        B = self.B
        sc = processed_scores(logits[:B, :d.vocab], self.tokens, n, begin_index=1 if r is None else r["begin_index"], eos=self.eos,
                              no_eos=no_eos, first=(mode == 1), suppress=self.suppress, begin_suppress=self.begin_suppress,
                              timestamp_rules=r, repetition_penalty=so.get("repetition_penalty"),
                              no_repeat_ngram=so.get("no_repeat_ngram_size") or 0, sequence_bias=so.get("sequence_bias"))
        if so.get("do_sample"):
            nxt = warp_and_sample(sc, so.get("temperature"), so.get("top_k"), so.get("top_p"), so.get("generator"))
        else:
            nxt = sc.argmax(-1)
        if self.eos is not None:
            nxt = torch.where(self.done, torch.full_like(nxt, self.fill), nxt)
            self.done.logical_or_(nxt == self.eos)
        self.tokens[:, n].copy_(nxt)
        self.cur.copy_(nxt.view(B, 1))

    def _run_step(self, t, mode, no_eos=False):
        if self.sample is not None and mode != 0:
            self.noise.exponential_(1.0, generator=self.soft.get("generator"))
        if not self.use_graphs:
            self._step(t, mode, no_eos)
            return
        g = self.graphs.get((t, mode, no_eos))
        if g is None:
            if not self._warm:
                # one eager step first: lazy initialisation inside torch must not happen under stream capture
                keep = (self.cur.clone(), self.tokens.clone(), self.done.clone())
                self._step(t, mode, no_eos)
                self.cur.copy_(keep[0]); self.tokens.copy_(keep[1]); self.done.copy_(keep[2])
                torch.cuda.synchronize(self.dev)
                self.pool = torch.cuda.graph_pool_handle()
                self._warm = True
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self.pool):
                self._step(t, mode, no_eos)
            self.graphs[(t, mode, no_eos)] = g
        g.replay()

    def run(self, enc_out, prompt_ids, max_new_tokens, min_new_tokens=0):
        """enc_out: encoder output of `batch` chunks (engine layout, rows = batch * max_source_positions);
        prompt_ids: int64 [batch, P] forced decoder prefix (P >= 1; position 0 = <|startoftranscript|>).
        Returns int64 [batch, P + n] with n <= max_new_tokens (stops early once every row has produced EOS)."""
        B, P = prompt_ids.shape
        if B != self.B:
            raise ValueError(f"decoder built for batch {self.B}, got {B}")
        total = P + int(max_new_tokens)
        if total > self.max_len:
            raise ValueError(f"prompt + max_new_tokens = {total} exceeds the decoder's max_len = {self.max_len}")
        self.cache = self.eng.decode_init(enc_out, B, self.max_len, cache=self.cache, cross_kv_dtype=self.cross_kv_dtype)
        self.tokens.zero_()
        self.tokens[:, :P].copy_(prompt_ids)
        self.done.zero_()
        self.cur.copy_(self.tokens[:, 0:1])
        n = P
        for t in range(total - 1):
            mode = 0 if t + 1 < P else (1 if t + 1 == P else 2)
            self._run_step(t, mode, bool(mode) and (t + 1 - P) < int(min_new_tokens))
            n = t + 2
            if self.eos is not None and mode and (t + 2 - P) % self.check_every == 0 and bool(self.done.all()):
                break
        return self.tokens[:, :n].clone()


def slot_step_torch(logits, V, tokens, length, plen, budget, done, row_t, cur, *, suppress=None, begin_suppress=None,
                    timestamp_rules=None, eos=None, min_new=0, lp_sum=None, nsp=None, nsp_pos=None, nsp_col=-1):
    """The slot step of continuous batching as torch ops and host arithmetic (`dw_slot_step`, csrc/slots.hip, is the kernel;
    include/dwamd.h states the rule): the path of oracle.ref_ops and the CPU.  logits [S, >= V]: row b is the output of the pass
    that fed cur[b] at position row_t[b]; tokens int64 [S, max_len]; length / plen / budget / row_t int32 [S]; done bool [S]; cur
    int64 [S, 1]; all updated in place.  A done slot is parked at position 0; inside its prompt a slot takes the forced token;
    otherwise the argmax of `processed_scores` with the slot's own history, begin_index = plen[b], first = (len == plen), no_eos =
    (len - plen < min_new); a generated EOS or a spent budget ends the slot.  With `lp_sum` (f32 [S]; `dw_slot_step_scores`): a
    generated step adds log_softmax(processed scores)[nxt] to lp_sum[b] (a row with no allowed column adds nothing), and with
    nsp_col >= 0 the step whose row is the output of input position nsp_pos[b] writes softmax(row)[nsp_col] into nsp[b] -- of the
    raw row when that step is forced, of the processed scores when it is generated; a parked slot keeps both."""
    lens, pls, buds, dns = length.tolist(), plen.tolist(), budget.tolist(), done.tolist()
    rules = None if timestamp_rules is None else dict(timestamp_rules)
    want_nsp = lp_sum is not None and int(nsp_col) >= 0
    at = nsp_pos.tolist() if want_nsp else None
    for b in range(tokens.shape[0]):
        n, P = lens[b], pls[b]
        if dns[b] or n < 1 or n >= tokens.shape[1] or P < 1:
            done[b] = True
            row_t[b] = 0
            cur[b, 0] = tokens[b, 0]
            continue
        forced = n < P
        if forced:
            nxt = int(tokens[b, n])
            if want_nsp and n - 1 == at[b]:
                nsp[b] = torch.softmax(logits[b, :V].float(), -1)[int(nsp_col)]
        else:
            sc = processed_scores(logits[b:b + 1, :V], tokens[b:b + 1], n, begin_index=P, eos=eos, no_eos=n - P < int(min_new),
                                  first=n == P, suppress=suppress, begin_suppress=begin_suppress, timestamp_rules=rules)
            nxt = int(sc.argmax(-1))
            if lp_sum is not None and bool(torch.isfinite(sc[0, nxt])):
                lsm = torch.log_softmax(sc[0].float(), -1)
                lp_sum[b] += lsm[nxt]
                if want_nsp and n - 1 == at[b]:
                    nsp[b] = lsm[int(nsp_col)].exp()
        tokens[b, n] = nxt
        length[b] = n + 1
        if not forced and ((eos is not None and nxt == eos) or n + 1 >= buds[b]):
            done[b] = True
            row_t[b] = 0
            cur[b, 0] = tokens[b, 0]
        else:
            row_t[b] = n
            cur[b, 0] = nxt


class SlotDecoder:
    """Continuous batching of greedy decoding: `slots` rows of one token loop, each at its own position of its own window; a row
    that has produced EOS (or spent its budget) hands its slot to the next waiting window instead of idling until the longest row
    of a batch is done.  Tokens are those of `GreedyDecoder` for the same window: the same rules, the same token step.

    A step is `engine.decode_token_rows` (dw_decode_token_rows: the token step with every row at its own position, fed from the
    device arrays `cur` / `row_t`) plus the slot step (`ops.slot_step`, dw_slot_step; `slot_step_torch` on ops without it), which
    selects every slot's token from the slot's own state (len, prompt length, budget, done) and writes the next feed.  Neither
    takes a host argument that depends on a position except the bound `max_t`, which only sizes LDS; with `use_graphs` the pair is
    captured once per bucket of 64 positions of that bound and replayed.  Every `check_every` steps the host reads `done` and `len`
    -- the only synchronisation --, yields the finished rows and refills their slots: the window's encoder rows are projected into
    the slot's cross-attention K/V (`engine.decode_refill`) and its prompt is teacher-forced one token per step like any other
    position.  The host's bound of `max_t` is the largest `len - 1` it last read (0 for a fresh slot) plus the steps since.

    run(windows): `windows` iterates (key, enc_rows, prompt_ids, max_new_tokens) -- enc_rows: the window's encoder output rows
    (engine layout), prompt_ids: P >= 1 ids (list or 1-D tensor), max_new_tokens >= 1 with P + max_new_tokens <= max_len.  Yields
    (key, row) as rows finish, row int64 = prompt + generated tokens up to and including EOS.  `steps` counts executed token steps.
    The source may yield `SlotDecoder.WAIT` -- "nothing now, but more may come once a live row has ended" (the seek loop: an
    utterance's next window is known only when the previous one is done): the empty slots stay empty until the next look, when
    the source is asked again; `run` ends when the source is exhausted and every slot is empty.

    scores=True: the slot step is dw_slot_step_scores and `run` yields (key, row, lp_sum, nsp) -- the sum of the generated tokens'
    log-probabilities under the processed scores and, with `nsp_col` (the <|nospeech|> id), softmax(row)[nsp_col] of the row behind
    input position `nsp_pos`, the optional fifth entry of a window (default: prompt length - 1, the first generated step)."""
    BUCKET = 64
    WAIT = object()

    def __init__(self, engine, slots, max_len, eos_token_id, suppress_tokens=None, begin_suppress_tokens=None, timestamp_rules=None,
                 min_new_tokens=0, pad_token_id=None, use_graphs=None, check_every=8, cross_kv_dtype=None, scores=False,
                 nsp_col=None):
        self.eng, self.S, self.max_len = engine, int(slots), int(max_len)
        d = engine.dims
        self.scores = bool(scores)
        self.nsp_col = -1 if nsp_col is None else int(nsp_col)
        if self.nsp_col >= d.vocab or (self.nsp_col >= 0 and not self.scores):
            raise ValueError("nsp_col names a column of the vocabulary and needs scores=True")
        self.cross_kv_dtype = kv_quant.normalize_dtype(cross_kv_dtype)      # "fp8": see GreedyDecoder
        if self.cross_kv_dtype is not None:
            kv_quant.check_width(d.d_model)
        if self.S < 1 or int(check_every) < 1:
            raise ValueError("SlotDecoder needs at least one slot and check_every >= 1")
        if self.max_len > d.max_tgt:
            raise ValueError(f"max_len = {max_len} exceeds max_target_positions = {d.max_tgt}")
        if eos_token_id is None:
            raise ValueError("SlotDecoder needs eos_token_id: a slot is handed on when its row ends")
        dev = engine.ops.device
        self.dev, self.eos = dev, int(eos_token_id)
        self.fill = self.eos if pad_token_id is None else int(pad_token_id)
        self.min_new = int(min_new_tokens)
        self.use_graphs = (torch.device(dev).type == "cuda" and hasattr(engine.ops, "slot_step")) if use_graphs is None else bool(use_graphs)
        self.check_every = int(check_every)
        self.timestamp_rules = timestamp_rules
        self.suppress = token_mask(suppress_tokens, d.vocab, dev, torch.uint8)
        self.begin_suppress = token_mask(begin_suppress_tokens, d.vocab, dev, torch.uint8)
        S = self.S
        self.tokens = torch.zeros((S, self.max_len), dtype=torch.long, device=dev)
        self.cur = torch.zeros((S, 1), dtype=torch.long, device=dev)
        self.done = torch.ones((S,), dtype=torch.bool, device=dev)
        self.state = torch.ones((5, S), dtype=torch.int32, device=dev)          # rows: len, plen, budget, row_t, nsp_pos
        self.len, self.plen, self.budget, self.row_t, self.nsp_pos = (self.state[i] for i in range(5))
        self.sc = torch.zeros((2, S), dtype=torch.float32, device=dev)          # rows: lp_sum, nsp (scores=True)
        self.cache = None
        self.graphs = {}
        self.pool = None
        self._warm = False
        self.steps = 0

    def _step(self, max_t):
        eng, V = self.eng, self.eng.dims.vocab
        logits = eng.decode_token_rows(self.cur, self.cache, self.row_t, max_t)
        r = self.timestamp_rules
        sc = dict(lp_sum=self.sc[0], nsp=self.sc[1], nsp_pos=self.nsp_pos, nsp_col=self.nsp_col) if self.scores else {}
        if hasattr(eng.ops, "slot_step"):
            mi = None if r is None else r.get("max_initial_timestamp_index")
            eng.ops.slot_step(logits, V, self.tokens, self.len, self.plen, self.budget, self.done, self.row_t, self.cur,
                              suppress=self.suppress, begin_suppress=self.begin_suppress,
                              ts_begin=-1 if r is None else int(r["no_timestamps_token_id"]) + 1, max_initial=-1 if mi is None else int(mi),
                              eos=self.eos, min_new=self.min_new, **sc)
        else:
            slot_step_torch(logits, V, self.tokens, self.len, self.plen, self.budget, self.done, self.row_t, self.cur,
                            suppress=self.suppress, begin_suppress=self.begin_suppress, timestamp_rules=r, eos=self.eos,
                            min_new=self.min_new, **sc)

    def _run_step(self, bound):
        # the pass is launched with the bucket's last position as max_t: it places the kernels' LDS regions only
        bucket = bound // self.BUCKET
        max_t = min((bucket + 1) * self.BUCKET, self.max_len) - 1
        self.steps += 1
        if not self.use_graphs:
            self._step(max_t)
            return
        g = self.graphs.get(bucket)
        if g is None:
            if not self._warm:
                # one eager step first: lazy initialisation inside torch must not happen under stream capture
                keep = (self.cur.clone(), self.tokens.clone(), self.done.clone(), self.state.clone(), self.sc.clone())
                self._step(max_t)
                self.cur.copy_(keep[0]); self.tokens.copy_(keep[1]); self.done.copy_(keep[2]); self.state.copy_(keep[3])
                self.sc.copy_(keep[4])
                torch.cuda.synchronize(self.dev)
                self.pool = torch.cuda.graph_pool_handle()
                self._warm = True
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g, pool=self.pool):
                self._step(max_t)
            self.graphs[bucket] = g
        g.replay()

    def _refill(self, b, enc_rows, prompt, max_new, nsp_pos=None):
        prompt = torch.as_tensor(prompt, dtype=torch.long).reshape(-1)
        P, max_new = int(prompt.numel()), int(max_new)
        if P < 1 or max_new < 1 or P + max_new > self.max_len:
            raise ValueError(f"a window needs 1 <= prompt length, 1 <= max_new_tokens and prompt + max_new_tokens <= max_len = "
                             f"{self.max_len} (got {P} + {max_new})")
        self.eng.decode_refill(self.cache, b, enc_rows)
        self.tokens[b, :P] = prompt.to(self.dev)
        self.state[:, b] = torch.tensor([1, P, P + max_new, 0, P - 1 if nsp_pos is None else int(nsp_pos)],
                                        dtype=torch.int32).to(self.dev)
        if self.scores:
            self.sc[:, b] = 0.0
        self.cur[b, 0] = self.tokens[b, 0]
        self.done[b] = False

    def run(self, windows):
        S = self.S
        if self.cache is None:
            self.cache = self.eng.decode_slots_init(S, self.max_len, cross_kv_dtype=self.cross_kv_dtype)
        self.done.fill_(True)                         # every slot empty: parked until a window takes it
        keys = [None] * S
        it = iter(windows)
        while True:
            dn, ln = self.done.tolist(), self.len.tolist()          # the loop's only synchronisation
            sc = self.sc.tolist() if self.scores else None
            for b in range(S):
                if keys[b] is not None and dn[b]:
                    row = self.tokens[b, :ln[b]].clone()
                    key, keys[b] = keys[b], None
                    yield (key, row, sc[0][b], sc[1][b]) if self.scores else (key, row)
            bound = 0
            waiting = False                           # the source has answered WAIT at this look: it is asked again at the next
            for b in range(S):
                if keys[b] is None and it is not None and not waiting:
                    w = next(it, None)
                    if w is None:
                        it = None
                    elif w is self.WAIT:
                        waiting = True
                    else:
                        keys[b] = w[0]
                        self._refill(b, *w[1:5])
                        ln[b] = 1
                if keys[b] is not None:
                    bound = max(bound, ln[b] - 1)
            if all(k is None for k in keys):
                if waiting:
                    raise RuntimeError("the window source answered WAIT with every slot empty: no live row can bring it a window")
                return
            for _ in range(self.check_every):
                self._run_step(min(bound, self.max_len - 1))
                bound += 1


class SeekWindowSource:
    """The window source of the timestamp seek loop on slots (modeling.seek_decode `slots=N`): an utterance's next window is
    known only when its previous one has ended, so the source keeps `fresh` (utterances not yet started), `cont` (utterances whose
    next window is known: encoded before any fresh one) and `ready` (encoded windows no slot has taken).  Asked for a window with
    `ready` empty it encodes up to N known windows in ONE call -- encode(utterances) -> [n, max_src, d_model] --, so at most 2 N
    encoded windows exist: N in slots, N ready.  With no window known and windows still inside slots it answers
    `SlotDecoder.WAIT`; with none inside slots either it is exhausted.  job(b, k) -> (prompt, max_new_tokens, nsp_pos) of
    utterance b's k-th window.  The consumer calls `ended(b, more)` for every window `SlotDecoder.run` hands back, before it asks
    for the next one.  `stats`: the encoder calls' batch sizes, the most encoded windows held, the windows ended."""

    def __init__(self, utterances, slots, encode, job):
        from collections import deque
        self.N, self.encode, self.job = int(slots), encode, job
        self.fresh, self.cont, self.ready = deque(utterances), deque(), deque()
        self.taken = {}                                # windows of utterance b handed to a slot
        self.live = 0
        self.stats = dict(steps=0, encoder_batches=[], max_held=0, windows=0)

    def ended(self, b, more):
        self.live -= 1
        self.stats["windows"] += 1
        if more:
            self.cont.append(b)

    def __iter__(self):
        while True:
            if not self.ready:
                take = []
                while len(take) < self.N and (self.cont or self.fresh):
                    take.append(self.cont.popleft() if self.cont else self.fresh.popleft())
                if not take:
                    if not self.live:
                        return
                    yield SlotDecoder.WAIT
                    continue
                enc = self.encode(take)
                self.stats["encoder_batches"].append(len(take))
                self.ready.extend((b, enc[i]) for i, b in enumerate(take))
                self.stats["max_held"] = max(self.stats["max_held"], len(self.ready) + self.live)
            b, rows = self.ready.popleft()
            k = self.taken.get(b, 0)
            self.taken[b] = k + 1
            self.live += 1
            yield (b, rows) + tuple(self.job(b, k))


# DW_ASSIST_TORCH=1 (read when an assisted decode starts): the round stays on the torch ops of `assist_pick_torch` / `assist_accept_torch`
# on every engine, as on ops without `assist_pick` / `assist_accept` -- the A/B leg of tools/bench_assist.py and the reference leg of
# tests/test_assist_gpu.py
ASSIST_TORCH_ENV = "DW_ASSIST_TORCH"


def assist_pick_torch(logits, hist, first_pos, begin_index, eos_token_id=None, min_new_tokens=0, suppress=None,
                      timestamp_rules=None, begin_suppress=None):
    """Greedy tokens int64 [B, n] from scores [B, n, V] whose row j predicts the token at sequence index first_pos + j (the torch
    path of oracle.ref_ops, of CPU runs, of unsupported sizes and of DW_ASSIST_TORCH=1; csrc/assist.hip `dw_assist_pick` is the
    kernel).  hist int64 [B, >= first_pos + n - 1]: the sequence those positions continue (history of the timestamp rules);
    begin_index: decoder prompt length; suppress: a mask of `processed_scores` (an f32 [V] vector with -inf at the suppressed ids reads
    the same), or None.  begin_suppress: the mask of the first generated position (None in `generate`, where an assistant switches
    it off as in the reference; pseudo_label.PseudoLabeller keeps its own)."""
    return torch.stack([processed_scores(logits[:, j], hist, first_pos + j, begin_index=begin_index, eos=eos_token_id,
                                         no_eos=first_pos + j - begin_index < min_new_tokens, suppress=suppress,
                                         first=first_pos + j == begin_index, begin_suppress=begin_suppress,
                                         timestamp_rules=timestamp_rules).argmax(-1)
                        for j in range(logits.shape[1])], 1)


def assist_accept_torch(own, draft, L, k, done, eos_token_id, fill):
    """The bookkeeping of one round as torch ops (`dw_assist_accept` is the kernel): own int64 [B, k + 1] the target's choices at
    positions L .. L + k, draft int64 [B, L + k] the sequence with the k drafts, done bool [B].  Returns (new int64 [B, n_ok + 1]:
    the accepted drafts -- equal to own -- plus the target's next token, finished rows filled; done; n_ok)."""
    if k > 0:
        agree = (own[:, :k] == draft[:, L:]) | done[:, None]
        n_ok = int(agree.long().cumprod(1).sum(1).min().item())
    else:
        n_ok = 0
    new = own[:, : n_ok + 1]                             # accepted draft tokens (== own) + the target's next token
    if eos_token_id is not None:
        for j in range(new.shape[1]):
            col = torch.where(done, torch.full_like(new[:, j], fill), new[:, j])
            new[:, j] = col
            done = done | (col == eos_token_id)
    return new, done, n_ok


def assist_pick_rows_torch(logits, tokens, lengths, j0, begin_index, eos_token_id=None, min_new_tokens=0, suppress=None,
                           timestamp_rules=None, begin_suppress=None):
    """`assist_pick_torch` with per-row positions (`dw_assist_pick_rows` is the kernel): scores [B, n, V] whose row (b, j) predicts
    tokens[b, lengths[b] + j0 + j] from the history tokens[b, :lengths[b] + j0 + j]; lengths: B ints.  -> int64 [B, n]; a position
    behind the buffer (a row that has ended at its end) is not judged and yields 0."""
    B, n = logits.shape[:2]
    own = torch.zeros((B, n), dtype=torch.long, device=logits.device)
    for b, L in enumerate(lengths):
        for j in range(n):
            at = max(int(L), begin_index) + j0 + j
            if at < tokens.shape[1]:
                own[b, j] = assist_pick_torch(logits[b:b + 1, j:j + 1], tokens[b:b + 1], at, begin_index, eos_token_id, min_new_tokens,
                                              suppress, timestamp_rules, begin_suppress)[0, 0]
    return own


def assist_accept_rows_torch(own, tokens, length, k, total, done, eos_token_id, fill):
    """The bookkeeping of one round with per-row lengths as host arithmetic over torch tensors (`dw_assist_accept_rows` is the
    kernel; include/dwamd.h states the rule): own int64 [B, >= k + 1] the target's choices at positions length[b] .. length[b] + k,
    tokens int64 [B, total] with row b's k drafts at [length[b], length[b] + k), length int32 [B], done bool [B]; tokens, length
    and done are updated in place.  Returns (pos_target, pos_assistant: lists of B ints, the start positions of the next round's
    passes -- length - 1 and length - 2, 0 for a row that has ended --, result = [drafts accepted, drafts offered, every row done,
    largest live length])."""
    B = tokens.shape[0]
    lens, fins, rows_own, rows_tok = length.tolist(), done.tolist(), own.tolist(), tokens.tolist()
    acc = off = top = 0
    pos_t, pos_a = [0] * B, [0] * B
    for b in range(B):
        L = min(max(lens[b], 1), total)
        fin = bool(fins[b]) or L >= total
        end = min(L + k, total - 1)
        if not fin:
            kb = end - L
            m = 0
            while m < kb and rows_own[b][m] == rows_tok[b][L + m]:
                m += 1
            w = 0
            while w <= m:
                c = rows_own[b][w]
                tokens[b, L + w] = c
                w += 1
                if eos_token_id is not None and c == eos_token_id:
                    fin = True
                    break
            acc += min(w, m)
            off += kb
            L += w
            fin = fin or L >= total
            length[b] = L
        if fin:
            if L <= end:
                tokens[b, L:end + 1] = fill
        else:
            top = max(top, L)
            pos_t[b], pos_a[b] = L - 1, L - 2
        done[b] = fin
    return pos_t, pos_a, [acc, off, int(bool(done.all())), top]


def assisted_greedy_decode(target, assistant, enc_target, enc_assistant, prompt_ids, max_new_tokens,
                           num_assistant_tokens=5, eos_token_id=None, suppress_tokens=None, min_new_tokens=0,
                           pad_token_id=None, use_cache=True, timestamp_rules=None, per_row=False, begin_suppress_tokens=None):
    """Speculative (assisted) greedy decoding: the small `assistant` engine drafts `num_assistant_tokens` tokens, the
    `target` engine scores all of them in ONE decoder pass and keeps the longest draft prefix that equals its own
    greedy choices plus its next token -- the output is token-for-token what target-only greedy decoding produces.

    Reference: run_eval.py:578-599, 706-707 (`assistant_model` of `generate`; the distilled student drafts for the
    teacher and shares its encoder output) and flax/run_speculative_decoding.py:76-107.  target / assistant:
    WhisperEngine; enc_*: their encoder outputs in engine layout (the same tensor when the encoders are shared);
    prompt_ids int64 [B, P].  With a batch the accepted length is the minimum over the rows that are still running
    (every emitted token is still each row's own greedy token).  suppress_tokens / min_new_tokens are the target's
    logits rules (SuppressTokensLogitsProcessor, MinNewTokensLengthLogitsProcessor); finished rows are filled with
    pad_token_id.  timestamp_rules (dict(begin_index, no_timestamps_token_id, max_initial_timestamp_index)): the
    WhisperTimeStampLogitsProcessor rules on every scored position, for the drafts and for the verification alike (the
    reference hands the same processors to the candidate generator): `return_timestamps=True` with an assistant.

    use_cache: both models keep KV caches.  The target verifies with `decode_multi` -- only the tokens it has not
    consumed yet (last accepted + drafts) go through the decoder, against the cached keys/values with the
    bottom-right aligned causal mask -- and rejected positions are dropped by rolling the cache position back; the
    assistant catches up on the accepted tokens the same way and drafts one token per step.  use_cache=False re-decodes
    the whole prefix every time (cross-check).

    Where the engines' ops have `assist_pick` / `assist_accept` (csrc/assist.hip) the cached round runs on device state: one `tokens`
    buffer [B, total], `done`, `own` and `result` for the whole call; every draft step is the assistant's pass plus one
    `assist_pick(n=1, store=True)`, the verification the target's pass, one `assist_pick(n=k + 1)` and one `assist_accept`, and the
    host reads `result` = (accepted drafts, every row done) once per round -- the only synchronisation.  On other ops
    (oracle.ref_ops, CPU), with DW_ASSIST_TORCH=1, with use_cache=False or beyond `assist_supported` the round is
    `assist_pick_torch` / `assist_accept_torch`: the same algorithm, the same minimum over the rows.  Equal scores: the lower column
    wins in the kernels (torch.argmax's order among equals is unspecified on the device).  Returns (ids [B, P + n], drafted, accepted).

    per_row=True (needs use_cache): every row accepts its OWN agreeing prefix and ends at its own EOS -- one row's rejected draft
    costs the other rows nothing, which is what makes an assistant pay at batch sizes above a few (the minimum over 16 rows'
    prefixes is close to zero for any model pair).  The rows then stand at different lengths, so from the second round on the
    decoder passes run at per-row positions (`engine.decode_multi_rows`, dw_decode_step_rows) and the round is
    `assist_pick_rows` / `assist_accept_rows` (`_assisted_rounds_device_rows`); on ops without them the same rounds run on
    `assist_pick_torch` per row and `assist_accept_rows_torch`.  Every row's output is still that row's own greedy output;
    drafted / accepted are summed over the rows that were live in a round.  begin_suppress_tokens (per_row only): excluded at
    the first generated position, for the drafts and the verification alike."""
    dt, da = target.dims, assistant.dims
    B, P0 = prompt_ids.shape
    ids = prompt_ids.clone()
    dev = ids.device
    total = P0 + int(max_new_tokens)
    if total > min(dt.max_tgt, da.max_tgt):
        raise ValueError(f"prompt + max_new_tokens = {total} exceeds max_target_positions")
    fill = eos_token_id if pad_token_id is None else pad_token_id
    ops_t, ops_a = target.ops, assistant.ops
    if begin_suppress_tokens and not per_row:
        raise NotImplementedError("begin_suppress_tokens with an assistant are implemented for per_row=True")
    if per_row:
        if not use_cache:
            raise NotImplementedError("per-row acceptance runs on the KV caches (use_cache=True)")
        kernels = (all(hasattr(o, "assist_pick_rows") and hasattr(o, "assist_accept_rows") for o in (ops_t, ops_a))
                   and ops_t.assist_supported(B, int(num_assistant_tokens)) and os.environ.get(ASSIST_TORCH_ENV, "0") in ("", "0"))
        return _assisted_rounds_device_rows(target, assistant, enc_target, enc_assistant, prompt_ids, total, int(num_assistant_tokens),
                                            eos_token_id, suppress_tokens, int(min_new_tokens), fill, timestamp_rules, kernels,
                                            begin_suppress_tokens)
    if (use_cache and all(hasattr(o, "assist_pick") and hasattr(o, "assist_accept") for o in (ops_t, ops_a))
            and ops_t.assist_supported(B, int(num_assistant_tokens)) and os.environ.get(ASSIST_TORCH_ENV, "0") in ("", "0")):
        return _assisted_rounds_device(target, assistant, enc_target, enc_assistant, prompt_ids, total, int(num_assistant_tokens),
                                       eos_token_id, suppress_tokens, int(min_new_tokens), fill, timestamp_rules)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    drafted = accepted = 0
    sup = {V: token_mask(suppress_tokens, V, dev) for V in {dt.vocab, da.vocab}}

    def pick(logits, d, first_pos, hist=None):
        return assist_pick_torch(logits, hist, first_pos, P0, eos_token_id, min_new_tokens, sup[d.vocab], timestamp_rules)

    def scores_nocache(eng, d, seq, enc, first):
        T = seq.shape[1]
        logits, _ = eng.decode(seq.contiguous(), enc, save=False)
        return logits[: B * T, : d.vocab].view(B, T, -1)[:, first:]

    ct = ca = None
    if use_cache:
        ct = target.decode_init(enc_target, B, total)
        ca = assistant.decode_init(enc_assistant, B, total)

    def scores_cached(eng, d, cache, seq):
        """feed the tokens of seq the cache has not consumed; scores [B, n, V] for those positions"""
        new = seq[:, cache["t"]:].contiguous()
        n = new.shape[1]
        logits = eng.decode_multi(new, cache)
        return logits[: B * n, : d.vocab].view(B, n, -1)

    while ids.shape[1] < total and not (eos_token_id is not None and bool(done.all())):
        L = ids.shape[1]
        k = min(int(num_assistant_tokens), total - L - 1)
        draft = ids
        for j in range(k):                                   # the assistant drafts k tokens greedily
            if use_cache:
                sc = scores_cached(assistant, da, ca, draft)[:, -1:]
            else:
                sc = scores_nocache(assistant, da, draft, enc_assistant, draft.shape[1] - 1)
            nxt = pick(sc, da, draft.shape[1], draft)[:, -1]
            draft = torch.cat([draft, nxt[:, None]], 1)
        if use_cache:
            sc = scores_cached(target, dt, ct, draft)[:, -(k + 1):]
        else:
            sc = scores_nocache(target, dt, draft, enc_target, L - 1)
        own = pick(sc, dt, L, draft)                         # [B, k + 1]: target's choice after each prefix
        new, done, n_ok = assist_accept_torch(own, draft, L, k, done, eos_token_id, fill)
        drafted += k
        accepted += n_ok
        ids = torch.cat([ids, new], 1)
        if use_cache:
            # positions L .. L+n_ok-1 hold accepted drafts (their K/V are valid); everything later is dropped
            ct["t"] = min(ct["t"], L + n_ok)
            ca["t"] = min(ca["t"], L + n_ok)
    return ids, drafted, accepted


def _assisted_rounds_device(target, assistant, enc_target, enc_assistant, prompt_ids, total, num_assistant_tokens, eos_token_id,
                            suppress_tokens, min_new_tokens, fill, timestamp_rules):
    """The cached rounds of `assisted_greedy_decode` on device state (csrc/assist.hip): the sequence lives in `tokens` [B, total],
    drafts included; per round k + 2 selection launches, one 8-byte read of `result`."""
    dt, da = target.dims, assistant.dims
    ops_t, ops_a = target.ops, assistant.ops
    B, P0 = prompt_ids.shape
    dev = prompt_ids.device
    K = num_assistant_tokens
    eos = -1 if eos_token_id is None else int(eos_token_id)
    tokens = torch.zeros((B, total), dtype=torch.long, device=dev)
    tokens[:, :P0].copy_(prompt_ids)
    cur = torch.zeros((B, 1), dtype=torch.long, device=dev)
    own = torch.zeros((B, K + 1), dtype=torch.long, device=dev)
    done = torch.zeros((B,), dtype=torch.bool, device=dev) if eos >= 0 else None
    result = torch.zeros((2,), dtype=torch.int32, device=dev)

    rk = rule_kwargs(timestamp_rules, eos_token_id)
    rules = dict(min_new=min_new_tokens if eos >= 0 else 0, ts_begin=rk["ts_begin"], max_initial=rk["max_initial"], begin_index=P0,
                 eos=eos)
    sup_t, sup_a = (token_mask(suppress_tokens, d.vocab, dev, torch.uint8) for d in (dt, da))     # decided once, on the host
    ct = target.decode_init(enc_target, B, total)
    ca = assistant.decode_init(enc_assistant, B, total)
    drafted = accepted = 0
    L, all_done = P0, False
    while L < total and not all_done:
        k = min(K, total - L - 1)
        for j in range(k):                                   # the assistant drafts k tokens greedily
            if j == 0:                                       # catch up on what the last round accepted (1 or 2 tokens; the prompt)
                n = L - ca["t"]
                logits = assistant.decode_multi(tokens[:, ca["t"]:L], ca)[n - 1:]
            else:
                n = 1
                logits = assistant.decode_step(cur, ca)
            ops_a.assist_pick(logits, da.vocab, tokens, L + j, own, n=1, batch_rows=n, suppress=sup_a, store=True, cur=cur, **rules)
        n = L + k - ct["t"]                                  # the target scores what it has not consumed: last accepted + drafts
        logits = target.decode_multi(tokens[:, ct["t"]:L + k], ct)[n - (k + 1):]
        ops_t.assist_pick(logits, dt.vocab, tokens, L, own, n=k + 1, batch_rows=n, suppress=sup_t, **rules)
        ops_t.assist_accept(own, tokens, L, k, result, eos=eos, fill=-1 if fill is None else int(fill), done=done)
        n_ok, fin = result.tolist()                          # the round's one synchronisation
        all_done = bool(fin)
        drafted += k
        accepted += n_ok
        # positions L .. L+n_ok-1 hold accepted drafts (their K/V are valid); everything later is dropped
        ct["t"] = min(ct["t"], L + n_ok)
        ca["t"] = min(ca["t"], L + n_ok)
        L += n_ok + 1
    return tokens[:, :L].clone(), drafted, accepted


def _assisted_rounds_device_rows(target, assistant, enc_target, enc_assistant, prompt_ids, total, num_assistant_tokens, eos_token_id,
                                 suppress_tokens, min_new_tokens, fill, timestamp_rules, kernels=True, begin_suppress_tokens=None):
    """The cached rounds of `assisted_greedy_decode(per_row=True)`: the state of `_assisted_rounds_device` plus, per row, `length`
    (int32: the row's tokens so far), `done`, and the positions `pos_t` / `pos_a` from which the two models' next passes re-feed
    the row.  The host reads `result` = (drafts accepted, drafts offered, every row done, largest live length) once per round and
    nothing else; from it k = min(K, total - 1 - largest live length), so no live row drafts past the buffer.

    Invariants, after every round, for every live row: the target's cache holds the K/V of the row's final tokens below
    length - 1, the assistant's below length - 2.  (The target has seen every accepted draft but not its own last token; the
    assistant has not seen the last draft it wrote, which is the only accepted draft it can miss.)  So the target's verify pass
    starts at length - 1 with k + 1 tokens and the assistant catches up with a 2-token pass at length - 2, whose second row
    drafts the first token.  The catch-up runs in EVERY round, also at k = 0: rounds without drafts follow one another while
    rows reach total - 1 one after the other, and a row that skipped a catch-up would lag by more than two tokens.  Re-feeding a
    position whose K/V are already valid rewrites them with values that may differ by a bf16 ulp from the first computation;
    only drafts and positions the target verifies again read them.  Round 1 is the uniform round: every row stands at the prompt
    length, so the prompt passes are `decode_multi`.  Rows that have ended are parked at position 0 (their passes stay inside
    their cache, their results are never read).  kernels=False: the same rounds with `assist_pick_torch` per row and
    `assist_accept_rows_torch` (which reads lengths on the host), and the invariants are checked as the passes are issued."""
    dt, da = target.dims, assistant.dims
    ops_t, ops_a = target.ops, assistant.ops
    B, P0 = prompt_ids.shape
    dev = prompt_ids.device
    K = num_assistant_tokens
    eos = -1 if eos_token_id is None else int(eos_token_id)
    tokens = torch.full((B, total), 0 if fill is None else int(fill), dtype=torch.long, device=dev)
    tokens[:, :P0].copy_(prompt_ids)
    cur = torch.zeros((B, 1), dtype=torch.long, device=dev)
    own = torch.zeros((B, K + 1), dtype=torch.long, device=dev)
    done = torch.zeros((B,), dtype=torch.bool, device=dev)
    length = torch.full((B,), P0, dtype=torch.int32, device=dev)
    pos_t, pos_a, pos_d = (torch.zeros((B,), dtype=torch.int32, device=dev) for _ in range(3))
    result = torch.zeros((4,), dtype=torch.int32, device=dev)
    ar = torch.arange(K + 1, device=dev)

    rk = rule_kwargs(timestamp_rules, eos_token_id)
    rules = dict(min_new=min_new_tokens if eos >= 0 else 0, ts_begin=rk["ts_begin"], max_initial=rk["max_initial"], begin_index=P0,
                 eos=eos)
    sup, bsup = ({V: token_mask(ids, V, dev, torch.uint8 if kernels else torch.bool) for V in {dt.vocab, da.vocab}}
                 for ids in (suppress_tokens, begin_suppress_tokens))
    valid_t, valid_a = [0] * B, [0] * B                      # kernels=False: leading cache positions that hold final tokens' K/V

    def fed(valid, start, n):                                # a pass may start at a valid position, not behind one
        for b, p in enumerate(start):
            assert p <= valid[b], "a cached pass would start behind the row's valid prefix"
            valid[b] = p + n

    def pick(ops, d, logits, n, j0, batch_rows, store):
        if kernels:
            ops.assist_pick_rows(logits, d.vocab, tokens, length, own, n=n, j0=j0, batch_rows=batch_rows, suppress=sup[d.vocab],
                                 begin_suppress=bsup[d.vocab], store=store, cur=cur if store else None, **rules)
            return
        lens = length.tolist()
        lg = torch.stack([logits[b * batch_rows:b * batch_rows + n, :d.vocab] for b in range(B)])
        own[:, :n] = assist_pick_rows_torch(lg, tokens, lens, j0, P0, eos_token_id, rules["min_new"], sup[d.vocab], timestamp_rules,
                                            bsup[d.vocab])
        if store:
            for b, L in enumerate(lens):
                if L + j0 < total:
                    tokens[b, L + j0] = own[b, 0]
                    cur[b, 0] = own[b, 0]

    ct = target.decode_init(enc_target, B, total)
    ca = assistant.decode_init(enc_assistant, B, total)
    drafted = accepted = 0
    top, first, all_done = P0, True, False
    while not all_done:
        k = min(K, total - 1 - top)
        if first:                                            # the uniform round: every row stands at P0
            for j in range(k):
                logits = assistant.decode_multi(tokens[:, :P0], ca)[P0 - 1:] if j == 0 else assistant.decode_step(cur, ca)
                pick(ops_a, da, logits, 1, j, P0 if j == 0 else 1, True)
            logits = target.decode_multi(tokens[:, :P0 + k], ct)[P0 - 1:]
            rows = P0 + k
            if not kernels:
                fed(valid_t, [0] * B, P0 + k)
                fed(valid_a, [0] * B, P0 + k - 1 if k else 0)
        else:
            if not kernels:
                fed(valid_a, pos_a.tolist(), 2)
            ids = tokens.gather(1, pos_a[:, None] + ar[None, :2])
            logits = assistant.decode_multi_rows(ids, ca, pos_a, top - 2)[1:]       # catch-up; its second row drafts token 0
            for j in range(k):
                if j:
                    torch.add(pos_a, 1 + j, out=pos_d)
                    if not kernels:
                        fed(valid_a, pos_d.tolist(), 1)
                    logits = assistant.decode_multi_rows(cur, ca, pos_d, top - 1 + j)
                pick(ops_a, da, logits, 1, j, 1 if j else 2, True)
            if not kernels:
                fed(valid_t, pos_t.tolist(), k + 1)
            ids = tokens.gather(1, pos_t[:, None] + ar[None, :k + 1])
            logits = target.decode_multi_rows(ids, ct, pos_t, top - 1)
            rows = k + 1
        pick(ops_t, dt, logits, k + 1, 0, rows, False)
        if kernels:
            ops_t.assist_accept_rows(own, tokens, length, k, total, result, done, pos_t, pos_a, eos=eos,
                                     fill=-1 if fill is None else int(fill))
            acc, off, fin, top = result.tolist()             # the round's one synchronisation
        else:
            pt, pa, (acc, off, fin, top) = assist_accept_rows_torch(own, tokens, length, k, total, done, eos_token_id,
                                                                    0 if fill is None else int(fill))
            pos_t.copy_(torch.tensor(pt, dtype=torch.int32))
            pos_a.copy_(torch.tensor(pa, dtype=torch.int32))
            for b, (L, f) in enumerate(zip(length.tolist(), done.tolist())):
                if f:                                        # parked: whatever the passes leave in the row is never read
                    valid_t[b] = valid_a[b] = total
                    continue
                assert valid_t[b] >= L - 1 and valid_a[b] >= L - 2, "the round left a live row's cache short of its invariant"
                valid_t[b], valid_a[b] = L - 1, min(valid_a[b], L - 1)
        all_done, first = bool(fin), False
        drafted += off
        accepted += acc
    return tokens[:, :int(length.max().item())].clone(), drafted, accepted


# DW_BEAM_TORCH=1 (read when a beam search starts): the step stays on the torch ops of `beam_step_torch` on every engine, as on ops
# without `beam_candidates` / `beam_update` -- the A/B leg of tools/bench_beam.py and the reference leg of tests/test_beam_step_gpu.py
BEAM_TORCH_ENV = "DW_BEAM_TORCH"
BEAM_NEG = -1.0e9


def _gather_beams(t, idx):                               # t [B, n, ...], idx [B, m] -> [B, m, ...]
    ix = idx
    while ix.dim() < t.dim():
        ix = ix.unsqueeze(-1)
    return torch.gather(t, 1, ix.expand(*idx.shape, *t.shape[2:]))


def _top_stable(x, k):
    """Indices of the k largest per row, equal values in ascending index order (torch.topk leaves that order unspecified; the
    kernels of csrc/beam.hip break ties the same way).  x [B, m] with m a few dozen."""
    return torch.sort(x, dim=1, descending=True, stable=True)[1][:, :k]


def beam_step_torch(st, logits, cur, cfg):
    """One step of `beam_search_decode` as torch ops (the path of oracle.ref_ops, of CPU runs and of DW_BEAM_TORCH=1): from the
    logits [B * k, V] of position `cur` to the new state.  st: dict(running, sequences int64 [B, k, max_length]; run_scores,
    beam_scores f32 [B, k]; finished bool [B, k]; lengths int64 [B, k]; unsat bool [B, 1]), replaced in place.  cfg:
    dict(P, max_length, nb, V, eos, min_new_tokens, length_penalty, early_stopping, sup, bsup -- bool [V] masks or None --,
    timestamp_rules).  Returns (src_rows int64 [B * k]: the row each new beam continues, go_on: 0-dim bool tensor).
    Among equal scores the lower index wins wherever the order can matter (the two small top-k)."""
    P, max_length, nb, V, eos = cfg["P"], cfg["max_length"], cfg["nb"], cfg["V"], cfg["eos"]
    length_penalty, early_stopping, tr = cfg["length_penalty"], cfg["early_stopping"], cfg["timestamp_rules"]
    running, sequences, run_scores = st["running"], st["sequences"], st["run_scores"]
    beam_scores, finished, lengths, unsat = st["beam_scores"], st["finished"], st["lengths"], st["unsat"]
    B = running.shape[0]
    dev = running.device
    keep = 2 * nb                                       # (number of EOS ids + 1) * num_beams continuations per utterance
    neg = BEAM_NEG
    lp = torch.log_softmax(logits.float(), dim=-1)
    flat = running[:, :, :cur].reshape(B * nb, cur)
    lp = processed_scores(lp, flat, cur, begin_index=P, eos=eos, no_eos=cur - P < int(cfg["min_new_tokens"]), first=cur == P,
                          suppress=cfg["sup"], begin_suppress=cfg["bsup"], timestamp_rules=tr)
    acc = (lp.view(B, nb, V) + run_scores[:, :, None]).reshape(B, nb * V)
    # equal scores go to the lower flat index beam * V + token, as in the kernels: torch.topk leaves their order unspecified, and
    # bf16 logits give one beam's best columns equal scores all the time.  (Twice as many as needed are taken and put in order, so
    # the rule holds unless more than `keep` columns tie with the last one kept.)
    top_lp, top_ix = torch.topk(acc, k=min(2 * keep, acc.shape[1]))
    by_ix = torch.sort(top_ix, dim=1, stable=True)[1]
    top_lp, top_ix = torch.gather(top_lp, 1, by_ix), torch.gather(top_ix, 1, by_ix)
    by_lp = _top_stable(top_lp, keep)
    top_lp, top_ix = torch.gather(top_lp, 1, by_lp), torch.gather(top_ix, 1, by_lp)
    src_beam, tok = top_ix // V, top_ix % V
    top_seq = _gather_beams(running, src_beam)
    top_seq[:, :, cur] = tok
    hits = (tok == eos) | (cur + 1 >= max_length)
    # open beams carried to the next step
    open_lp = top_lp + hits.float() * neg
    nxt = _top_stable(open_lp, nb)
    st["running"] = _gather_beams(top_seq, nxt)
    st["run_scores"] = run_scores = _gather_beams(open_lp, nxt)
    src_rows = (_gather_beams(src_beam, nxt) + torch.arange(B, device=dev)[:, None] * nb).reshape(-1)
    # finished hypotheses: only the best num_beams continuations may finish
    top_mask = torch.arange(keep, device=dev) < nb
    just = hits & top_mask[None, :]
    fin_lp = top_lp / float((cur + 1 - P) ** length_penalty)
    fin_lp = fin_lp + (finished.all(-1, keepdim=True) & (early_stopping is True)).float() * neg
    fin_lp = fin_lp + (~unsat).float() * neg
    fin_lp = fin_lp + (~just).float() * neg
    m_seq = torch.cat([sequences, top_seq], 1)
    m_sc = torch.cat([beam_scores, fin_lp], 1)
    m_fin = torch.cat([finished, just], 1)
    m_len = torch.cat([lengths, torch.full((B, keep), cur + 1 - P, dtype=lengths.dtype, device=dev)], 1)
    best = _top_stable(m_sc, nb)
    st["sequences"], st["beam_scores"] = _gather_beams(m_seq, best), _gather_beams(m_sc, best)
    st["finished"], st["lengths"] = _gather_beams(m_fin, best), _gather_beams(m_len, best)
    beam_scores, finished = st["beam_scores"], st["finished"]
    # early-stopping heuristic and loop condition (TF `_check_early_stop_heuristic`, `_beam_search_has_unfinished_sequences`)
    hyp_len = (max_length - P) if (early_stopping == "never" and length_penalty > 0.0) else (cur + 1 - P)
    best_running = run_scores[:, :1] / float(hyp_len ** length_penalty)
    worst_fin = torch.where(finished, beam_scores.min(1, keepdim=True)[0], torch.full_like(beam_scores, neg))
    st["unsat"] = unsat = unsat & (best_running > worst_fin).any(-1, keepdim=True)
    go_on = unsat.any() & ~hits.all()
    if early_stopping is True:
        go_on = go_on & ~finished.all()
    return src_rows, go_on


def beam_search_decode(engine, enc_out, prompt_ids, max_new_tokens, num_beams, eos_token_id, pad_token_id=None,
                       suppress_tokens=None, begin_suppress_tokens=None, min_new_tokens=0, length_penalty=1.0,
                       early_stopping=False, timestamp_rules=None, return_scores=False, check_every=4):
    """Beam search over the KV-cache decoder: `generate(num_beams=k)` of the reference (run_eval.py:143, 693;
    run_distillation.py:1428-1436; TF:generation/utils.py `_beam_search`, the vectorised v5 algorithm) -- per step the
    log-softmax of every live beam plus its running score, the top 2k continuations per utterance, the k best open ones
    carried on (their K/V cache rows gathered in place), finished ones merged into the k best finished hypotheses
    under the length penalty, and the early-stopping heuristic of `early_stopping` in {False, True, "never"}.
    The decoder passes are the engine's cached passes over B * k rows (prompt prefill in one multi-token pass, then
    token steps).  Where the engine's ops have `beam_candidates` / `beam_update` (csrc/beam.hip) the step is two entry calls on
    device-resident state: the loop condition lands in a device word that the host reads every `check_every` steps (once it is
    set the kernels leave the state alone), so nothing synchronises in between.  On other ops (oracle.ref_ops, CPU), with
    DW_BEAM_TORCH=1, or for num_beams > 16 / a vocabulary > 65 536 the step is `beam_step_torch`, which reads the loop condition
    every step.  Equal scores: the lower flat index beam * V + token wins in the kernels (torch.topk's order is unspecified).
    prompt_ids int64 [B, P] -> sequences int64 [B, P + n] (best finished hypothesis per row, padded with pad_token_id).
    return_scores=True -> (sequences, sequences_scores f32 [B], prefill_logits [B, P, V]): the best hypothesis' length-penalised
    score (`beam_scores[:, 0]`, what TF `_beam_search` returns as `sequences_scores`) and the logits of the prompt prefill of
    each utterance's beam 0 at every prompt position (the seek loop reads its no-speech probability there)."""
    dev = prompt_ids.device
    d = engine.dims
    ops = engine.ops
    B, P = prompt_ids.shape
    nb, V = int(num_beams), d.vocab
    max_length = P + int(max_new_tokens)
    if eos_token_id is None:
        raise ValueError("beam search needs eos_token_id")
    eos = int(eos_token_id)
    fill = int(pad_token_id) if pad_token_id is not None else eos
    keep = 2 * nb
    neg = BEAM_NEG
    use_kernels = (hasattr(ops, "beam_candidates") and hasattr(ops, "beam_update") and ops.beam_supported(nb, V)
                   and os.environ.get(BEAM_TORCH_ENV, "0") in ("", "0"))

    Lk, D = d.max_src, d.d_model
    enc_rep = enc_out[:B * Lk].view(B, Lk, D).repeat_interleave(nb, 0).reshape(B * nb * Lk, D).contiguous()
    cache = engine.decode_init(enc_rep, B * nb, max_length)
    running = torch.full((B, nb, max_length), fill, dtype=torch.long, device=dev)
    running[:, :, :P] = prompt_ids[:, None, :]
    run_scores = torch.zeros((B, nb), dtype=torch.float32, device=dev)
    run_scores[:, 1:] = neg
    st = dict(running=running, sequences=running.clone(), run_scores=run_scores,
              beam_scores=torch.full((B, nb), neg, dtype=torch.float32, device=dev),
              finished=torch.zeros((B, nb), dtype=torch.bool, device=dev),
              lengths=torch.zeros((B, nb), dtype=torch.int32 if use_kernels else torch.long, device=dev),   # generated tokens
              unsat=torch.ones((B, 1), dtype=torch.bool, device=dev))
    cur = P
    full = engine.decode_multi(running[:, :, :P].reshape(B * nb, P), cache)
    logits = full.view(B * nb, P, -1)[:, -1]             # [B * k, ld], V valid columns
    prefill = full.view(B, nb, P, -1)[:, 0, :, :V].clone() if return_scores else None

    def reorder(src_rows, n):                            # the carried beams' K/V rows (positions < n are live)
        for kvc in cache["self"]:
            v = kvc.view(B * nb, max_length, -1)
            v[:, :n].copy_(v[src_rows, :n])

    def divisors(c):                                     # in double on the host, as the torch step computes them
        hyp_len = (max_length - P) if (early_stopping == "never" and length_penalty > 0.0) else (c + 1 - P)
        return float((c + 1 - P) ** length_penalty), float(hyp_len ** length_penalty)

    if use_kernels:
        sup, bsup = (token_mask(ids, V, dev, torch.uint8) for ids in (suppress_tokens, begin_suppress_tokens))
        R = B * nb
        other = dict(running=torch.full_like(running, fill), sequences=torch.full_like(running, fill))
        other["running"][:, :, :P] = prompt_ids[:, None, :]
        other["sequences"][:, :, :P] = prompt_ids[:, None, :]
        cand_val = torch.empty((R, keep), dtype=torch.float32, device=dev)
        cand_tok = torch.empty((R, keep), dtype=torch.int32, device=dev)
        stop = torch.zeros((1,), dtype=torch.int32, device=dev)
        src_rows = torch.arange(R, dtype=torch.long, device=dev)
        next_tok = torch.zeros((R, 1), dtype=torch.long, device=dev)
        plan = torch.empty((4 * R,), dtype=torch.int32, device=dev)
        while True:
            ops.beam_candidates(
                logits, V, st["running"].view(R, max_length), cur, st["run_scores"], cand_val, cand_tok, stop, suppress=sup,
                begin_suppress=bsup, first=(cur == P), no_eos=(cur - P) < int(min_new_tokens),
                **rule_kwargs(timestamp_rules, eos))
            fin_div, hyp_div = divisors(cur)
            ops.beam_update(cand_val, cand_tok, B, nb, V, cur, P, max_length, eos, early_stopping, fin_div, hyp_div,
                            st["running"], other["running"], st["sequences"], other["sequences"], st["run_scores"],
                            st["beam_scores"], st["finished"], st["lengths"], st["unsat"], stop, src_rows, next_tok, plan)
            for name in ("running", "sequences"):        # ping-pong: no row is read after another row has overwritten it
                st[name], other[name] = other[name], st[name]
            cur += 1
            # (at cur == max_length every continuation was a hit: the kernel has set `stop`)
            if cur >= max_length or ((cur - P) % int(check_every) == 0 and bool(stop.item())):
                break
            reorder(src_rows, cur - 1)
            logits = engine.decode_step(next_tok, cache)
    else:
        cfg = dict(P=P, max_length=max_length, nb=nb, V=V, eos=eos, min_new_tokens=int(min_new_tokens),
                   length_penalty=length_penalty, early_stopping=early_stopping, sup=token_mask(suppress_tokens, V, dev),
                   bsup=token_mask(begin_suppress_tokens, V, dev), timestamp_rules=timestamp_rules)
        while True:
            src_rows, go_on = beam_step_torch(st, logits[:, :V], cur, cfg)
            reorder(src_rows, cur)
            cur += 1
            if not bool(go_on):
                break
            logits = engine.decode_step(st["running"][:, :, cur - 1].reshape(B * nb, 1).contiguous(), cache)
    out_len = P + int(st["lengths"][:, 0].max().item())
    seqs = st["sequences"][:, 0, :out_len].contiguous()
    if return_scores:
        return seqs, st["beam_scores"][:, 0].clone(), prefill
    return seqs
