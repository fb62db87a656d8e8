"""The timestamp seek loop (TF:generation_whisper.py:784-903) behind `WhisperForConditionalGeneration.seek_decode`, whose
docstring is the specification, and `generate`'s way into it (`generate_seek_loop`).

One call's state is a SeekContext; the pieces are functions of it.  The lockstep loop (`lockstep_loop`) goes pass by pass: the
decoder prompts of a pass (`build_prompts`), every group of equal prompt length down the temperature ladder (`decode_group`, the
four kinds of pass being `sampled_pass`, `assisted_pass`, `beam_pass` and `greedy_pass`), then every utterance moves on by what
its accepted window says.  The slot schedule (`slot_schedule`) runs the same windows as jobs of a decoding.SlotDecoder.  Both
loops end a window in `apply_window`.  Which arguments may be combined is generation.REFUSALS.

`decoding.processed_scores`, `decoding.beam_search_decode`, `generation.retrieve_segment`, `SlotDecoder.run` and the engine's
methods are looked up where they are called, so a test's patch of any of them is seen here.
"""
import math
import os
import zlib
from functools import partial
from types import SimpleNamespace

import torch

from . import decoding
from . import generation as G


class SeekContext:
    """What the pieces of one `seek_decode` call share: the call's arguments under their names (`a`: the dict the method builds,
    name by name, from its signature), and what is derived from them once (engine, dims, device, the rules as masks, `seek` and
    `segments` per utterance, `window_scores`).  No derived attribute takes an argument's name."""

    def __init__(self, model, a):
        self.__dict__.update(a)
        self.model, self.eng, self.d = model, model.engine, model.dims
        self.B, self.dev = self.input_features.shape[0], self.input_features.device
        self.nb = int(self.num_beams)
        self.rep_pen = None if self.repetition_penalty in (None, 1.0) else float(self.repetition_penalty)
        self.ngram = int(self.no_repeat_ngram_size or 0)
        self.hist_soft = None                  # decoding.GreedyDecoder `soft` of the greedy passes
        if self.rep_pen is not None or self.ngram or self.sequence_bias is not None:
            self.hist_soft = dict(do_sample=False, repetition_penalty=self.rep_pen, no_repeat_ngram_size=self.ngram)
            if self.sequence_bias is not None:
                self.hist_soft["sequence_bias"] = self.sequence_bias
        self.W, self.V, self.cut_off = 2 * model.dims.max_src, model.dims.vocab, model.dims.max_tgt // 2 - 1
        self.feats = self.input_features.to(torch.float32)
        self.seek = [0] * self.B
        t = self.temperatures
        self.temps = [0.0 if x is None else float(x) for x in (t if isinstance(t, (list, tuple)) else [t])]
        if callable(self.init_tokens):
            self.init = self.init_tokens(
                lambda: self.detect_language(self.eng.encode(window(self, list(range(self.B))), save=False)[0]))
        else:
            self.init = self.init_tokens
        self.P0 = len(self.init[0])
        self.nts = int(self.no_timestamps_token_id)
        self.tb = self.nts + 1
        self.prev_sot = self.prev_sot_token_id
        if self.prev_sot is None and self.suppress_tokens is not None and len(self.suppress_tokens) >= 2:
            self.prev_sot = self.suppress_tokens[-2]
        self.need_scores = self.logprob_threshold is not None or self.no_speech_threshold is not None

    def start(self):
        """The rules as the passes take them and the per-utterance results (after the refusals that follow language detection)."""
        self.sup, self.bsup = (self._vmask(ids) for ids in (self.suppress_tokens, self.begin_suppress_tokens))
        self.ts_rules = G.timestamp_rules(self.nts, self.max_initial_timestamp_index)
        # the sampled passes select inside the kernel (dw_sample_select) where the ops have it: per step one `exponential_` draw
        # of the shape [r, V] that `torch.multinomial` would draw itself, plus one launch; DW_SAMPLE_TORCH=1 keeps the torch ops
        # (the sampling kernel takes no bias table: with one the sampled passes are the torch ops of `processed`)
        self.sample_kernel = hasattr(self.eng.ops, "sample_select") and \
            os.environ.get(decoding.SAMPLE_TORCH_ENV, "0") in ("", "0") and self.sequence_bias is None
        self.segments = [[] for _ in range(self.B)]
        self.prompt = [int(x) for x in self.prompt_ids] if self.prompt_ids is not None else None
        self.first_segment_prompt = bool(self.prompt) and not self.prompt_all_segments
        if self.first_segment_prompt:
            body = self.prompt[1:] if (self.prev_sot is not None and self.prompt[0] == self.prev_sot) else self.prompt
            self.segments = [[{"tokens": list(body)}] for _ in range(self.B)]
        self.do_cond = [bool(self.condition_on_prev_tokens)] * self.B
        if not hasattr(self.model, "_seek_decoders"):
            self.model._seek_decoders = {}     # reused by later calls (pseudo-labelling decodes batch after batch)
        # (utterance, first frame, average log-probability, no-speech probability) of every scored pass over a window, in order
        self.window_scores = self.model.last_window_scores = []

    def _vmask(self, ids):                     # (all-false where no id names a column: the sampling kernel is given both)
        mk = decoding.token_mask(ids, self.V, self.dev)
        return torch.zeros(self.V, dtype=torch.bool, device=self.dev) if mk is None else mk

    def rules_at(self, P):
        return G.timestamp_rules(self.nts, self.max_initial_timestamp_index, begin_index=P)

    def result(self):
        return [sg[1:] for sg in self.segments] if self.first_segment_prompt else self.segments


def window(c, rows):
    seg = torch.zeros((len(rows), c.feats.shape[1], c.W), dtype=torch.float32, device=c.dev)
    for i, b in enumerate(rows):
        n = min(c.max_frames[b] - c.seek[b], c.W)
        seg[i, :, :n] = c.feats[b, :, c.seek[b]:c.seek[b] + n]
    return seg


def processed(c, raw, hist, n, P, min_new):
    """The reference's processed scores of one step: raw f32 [r, V], hist int64 [r, >= n] (n tokens so far)."""
    return decoding.processed_scores(raw, hist, n, begin_index=P, eos=c.eos, no_eos=n - P < min_new, first=n == P, suppress=c.sup,
                                     begin_suppress=c.bsup, timestamp_rules=c.ts_rules, repetition_penalty=c.rep_pen,
                                     no_repeat_ngram=c.ngram, sequence_bias=c.sequence_bias)


def sample(c, enc, ids, max_new, min_new, temp):
    """Multinomial sampling at temperature `temp` over the processed scores (fallback passes)."""
    eng, V, dev, pad = c.eng, c.V, c.dev, c.pad
    r, P = ids.shape
    cache = eng.decode_init(enc, r, P + max_new)
    toks = torch.full((r, P + max_new), pad, dtype=torch.long, device=dev)
    toks[:, :P] = ids
    done = torch.zeros(r, dtype=torch.bool, device=dev)
    logits = eng.decode_multi(ids, cache).view(r, P, -1)[:, -1]
    if c.sample_kernel:
        noise = torch.empty((r, V), dtype=torch.float32, device=dev)
        cur = torch.empty((r, 1), dtype=torch.long, device=dev)
    n = P
    while True:
        if c.sample_kernel:
            # processors, temperature, the draw and the EOS / pad bookkeeping in one launch (stepping stays eager: r
            # changes from pass to pass); the generator is consumed as by the multinomial below
            noise.exponential_(1.0)
            eng.ops.sample_select(
                logits, V, toks, n, cur, noise, suppress=c.sup.view(torch.uint8), begin_suppress=c.bsup.view(torch.uint8),
                first=(n == P), no_eos=(n - P < min_new), ts_begin=c.tb,
                max_initial=-1 if c.max_initial_timestamp_index is None else int(c.max_initial_timestamp_index),
                begin_index=P, eos=c.eos, fill=pad, done=done, repetition_penalty=1.0 if c.rep_pen is None else c.rep_pen,
                no_repeat_ngram=c.ngram, temperature=temp)
            nxt = cur[:, 0]
        else:
            pr = torch.softmax(processed(c, logits[:, :V].float(), toks, n, P, min_new) / temp, -1)
            nxt = torch.multinomial(pr, 1)[:, 0]
            nxt = torch.where(done, torch.full_like(nxt, pad), nxt)
            toks[:, n] = nxt
            done = done | (nxt == c.eos)
        n += 1
        if n >= P + max_new or bool(done.all()):
            break
        logits = eng.decode_step(nxt[:, None].contiguous(), cache)
    return toks[:, :n]


def scores_of(c, enc, ids, gens, min_new):
    """(average log-probability of the chosen tokens, P(<|nospeech|>) after <|startoftranscript|>) per row from
    ONE teacher-forced decoder pass over prompt + generated tokens (TF `_retrieve_avg_logprobs`, 1958-1975;
    `WhisperNoSpeechDetection`, TF:generation/logits_process.py)."""
    dev = c.dev
    r, P = ids.shape
    L = max(1, max(len(g) for g in gens))
    full = torch.full((r, P + L), c.eos, dtype=torch.long, device=dev)
    full[:, :P] = ids
    for i, g in enumerate(gens):
        if g:
            full[i, P:P + len(g)] = torch.as_tensor(g, dtype=torch.long, device=dev)
    T = full.shape[1]
    logits, _ = c.eng.decode(full[:, :T - 1].contiguous() if T > 1 else full, enc, save=False)
    logits = logits[:r * (T - 1)].view(r, T - 1, -1)[:, :, :c.V].float()
    tot = torch.zeros(r, dtype=torch.float64, device=dev)
    first = None
    for j in range(L):
        sc = processed(c, logits[:, P - 1 + j], full, P + j, P, min_new)
        if j == 0:
            first = sc
        lp = torch.log_softmax(sc, -1).gather(1, full[:, P + j:P + j + 1])[:, 0]
        live = torch.as_tensor([j < len(g) for g in gens], device=dev)
        tot += torch.where(live, lp.double(), torch.zeros_like(tot))
    avg = [float(tot[i]) / len(g) if g else 0.0 for i, g in enumerate(gens)]
    if c.P0 > 1:
        nsp = torch.softmax(logits[:, P - c.P0], -1)[:, c.nts - 1]
    else:
        nsp = torch.softmax(first, -1)[:, c.nts - 1]
    return avg, nsp.tolist()


def beam_no_speech(c, prefill, ids, P, min_new, nb):
    """P(<|nospeech|>) of a beam-search pass as the reference's `_need_fallback` reads it.  prefill f32 / bf16 [r, P, V]: the
    prompt-prefill logits of each utterance's beam 0.  With a decoder prompt of several start tokens
    `WhisperNoSpeechDetection` runs the model on its own, unexpanded inputs: one row per utterance, the softmax at the
    <|startoftranscript|> position.  With a single start token it keeps the processor scores of the first step, which in
    beam search are the r * nb expanded rows (log-probabilities, so `exp`, not renormalised after the other processors), and
    `_need_fallback` indexes that tensor with the UTTERANCE index (`no_speech_prob[index]`): utterance i is judged by
    expanded row i, i.e. by utterance i // nb.  Reproduced here as it is."""
    r = ids.shape[0]
    if c.P0 > 1:
        return torch.softmax(prefill[:, P - c.P0].float(), -1)[:, c.nts - 1].tolist()
    lp = processed(c, torch.log_softmax(prefill[:, P - 1].float(), -1), ids, P, P, min_new)
    per_row = lp[:, c.nts - 1].exp().tolist()
    return [per_row[i // nb] for i in range(r)]


def compression_ratio(c, tokens):
    nbytes = int(math.log2(c.V) / 8) + 1
    raw = b"".join(int(x).to_bytes(nbytes, "little") for x in tokens)
    return len(raw) / len(zlib.compress(raw))


def strip_pad(c, seq):
    if seq and seq[-1] == c.pad:           # TF:1064-1071: drop the padding (all but one EOS when pad == EOS)
        npad = sum(1 for x in seq if x == c.pad) - (1 if c.pad == c.eos else 0)
        if npad:
            seq = seq[:-npad]
    return seq


def judge(c, gen, avg, nsp):
    """(decode again at the next temperature, skip the window) of one decoded window (TF:1243-1287)."""
    fallback = skip = False
    if c.compression_ratio_threshold is not None and gen and compression_ratio(c, gen) > c.compression_ratio_threshold:
        fallback = True
    if c.logprob_threshold is not None and avg < c.logprob_threshold:
        fallback = True
    if c.no_speech_threshold is not None and avg < c.logprob_threshold and nsp > c.no_speech_threshold:
        fallback, skip = False, True
    return fallback, skip


def apply_window(c, b, gen, skip, snf, stamps=None):
    """A finished window of utterance b, of `snf` frames: skipped (no speech), the utterance moves past it; else `retrieve_segment`
    splits its tokens `gen` (a final EOS aside) into segments and says how far the utterance moves.  stamps = (P, the window's
    row of token timestamps) with token timestamps: the segments carry their slices of it."""
    if skip:
        c.seek[b] += snf
        return
    seq = gen[:-1] if (gen and gen[-1] == c.eos) else gen
    segs, offset = G.retrieve_segment(seq, c.tb, snf, time_offset=c.seek[b] * 0.01, with_idxs=stamps is not None)
    if stamps is not None:
        P, row = stamps
        # TF:800-802: the window's offset in seconds, a double; added to the float32 row as the reference adds it
        t_off = torch.tensor(c.seek[b], dtype=torch.float64) * c.token_timestamps["time_precision"] / 2
        for sg in segs:
            i0, i1 = sg["idxs"]
            sg["idxs"] = (P + i0, P + i1)
            sg["result"] = {"token_timestamps": row}
            sg["token_timestamps"] = row[P + i0:P + i1] + t_off
    c.seek[b] += offset
    c.segments[b] += segs


# ---- the slot schedule ----------------------------------------------------------------------------------------------------------
ONE_LENGTH = "the timestamp seek loop on slots needs decoder prompts of one length (init_tokens rows of different lengths)"


def slot_decoder(c, min_new):
    """The model's SlotDecoder for this configuration.  Slot decoders are kept apart from the lockstep loop's (whose many batch
    sizes must not push them out).  Each owns its K/V caches -- N slots x (max_target_positions self rows + max_source_positions
    cross rows) x 2 d_model per decoder layer: 0.6 GB per layer at 64 slots of d_model 1280 in bf16, 20 GB for large-v3's 32
    layers -- and its graphs, so only `seek_slot_decoders_max` (2: one configuration and a variant) stay alive; set the attribute
    to keep more."""
    N = int(c.slots)
    key = ("slots", N, c.eos, c.pad, c.nts, c.max_initial_timestamp_index, tuple(c.suppress_tokens or ()),
           tuple(c.begin_suppress_tokens or ()), min_new, int(c.check_every), c.cross_kv_dtype, c.use_graphs, c.need_scores)
    slot_decoders = c.model.__dict__.setdefault("_seek_slot_decoders", {})
    dec = slot_decoders.get(key)
    if dec is None:
        while len(slot_decoders) >= max(1, int(getattr(c.model, "seek_slot_decoders_max", 2))):
            slot_decoders.pop(next(iter(slot_decoders)))
        dec = slot_decoders[key] = decoding.SlotDecoder(
            c.eng, N, c.d.max_tgt, c.eos, suppress_tokens=c.suppress_tokens, begin_suppress_tokens=c.begin_suppress_tokens,
            timestamp_rules=c.ts_rules, min_new_tokens=min_new, pad_token_id=c.pad, use_graphs=c.use_graphs,
            check_every=c.check_every, cross_kv_dtype=c.cross_kv_dtype, scores=c.need_scores,
            nsp_col=c.nts - 1 if c.need_scores else None)
    return dec


def slot_job(c, P, per_pass, b, k):
    """The k-th window of utterance b as a SlotDecoder job: (decoder prompt of P tokens, max_new_tokens, forced prompt tokens).
    per_pass: lengths(P) of the k-th windows so far (the lockstep loop asks once per pass)."""
    while len(per_pass) <= k:
        per_pass.append(c.lengths(P))
    if per_pass[k][1] != per_pass[0][1]:
        raise NotImplementedError("the timestamp seek loop on slots needs one min_new_tokens for every window")
    return (c.prompt or []) + list(c.init[b]), per_pass[k][0], P - c.P0


def slot_encode(c, take):
    enc, _ = c.eng.encode(window(c, take), save=False)
    return enc[:len(take) * c.d.max_src].view(len(take), c.d.max_src, -1)


def slot_schedule(c):
    """The seek loop as a slot schedule: every (utterance, window) is a SlotDecoder job."""
    if callable(c.init_tokens) and len({len(r) for r in c.init}) > 1:          # (given rows were judged before the encoder ran)
        raise NotImplementedError(ONE_LENGTH)
    P, per_pass = len(c.prompt or []) + c.P0, []
    job = partial(slot_job, c, P, per_pass)
    job(0, 0)
    dec = slot_decoder(c, per_pass[0][1])
    source = decoding.SeekWindowSource([b for b in range(c.B) if c.seek[b] < c.max_frames[b]], int(c.slots),
                                       partial(slot_encode, c), job)
    steps0 = dec.steps
    for res in dec.run(source):
        b, seq = res[0], strip_pad(c, res[1][P:].tolist())
        avg = nsp = None
        if c.need_scores:
            avg, nsp = (float(res[2]) / len(seq) if seq else 0.0), float(res[3])
            c.window_scores.append((b, c.seek[b], avg, nsp))
        _, skip = judge(c, seq, avg, nsp)              # (one temperature: nothing to fall back to)
        apply_window(c, b, seq, skip, min(c.max_frames[b] - c.seek[b], c.W))
        source.ended(b, c.seek[b] < c.max_frames[b])
    c.model.last_seek_stats = dict(source.stats, steps=dec.steps - steps0)
    return c.result()


# ---- the lockstep loop ----------------------------------------------------------------------------------------------------------
def build_prompts(c, rows):
    """The decoder prompts of a pass (TF:1853-1918) -> {utterance: tokens}."""
    prompts = {}
    cond_now = any(c.do_cond[b] for b in rows) and len(c.segments[0]) > 0
    for b in rows:
        pre = []
        if cond_now:
            if c.prev_sot is None:
                raise ValueError("condition_on_prev_tokens needs prev_sot_token_id in the generation config")
            if c.do_cond[b] and c.segments[b]:
                for sg in c.segments[b]:
                    tk = sg["tokens"]
                    pre += tk[:-1] if (len(tk) > 2 and tk[-2] >= c.tb) else tk
                pre = pre[-c.cut_off:]
            pre = (list(c.prompt) if (c.prompt and c.prompt_all_segments) else [c.prev_sot]) + pre
        elif c.prompt:
            pre = list(c.prompt)
        prompts[b] = pre + list(c.init[b])
    return prompts


def sampled_pass(c, g, temp):
    """A fallback pass: one beam, sampled at `temp` (TF:1004-1005) -> (generated tokens per row, None)."""
    return sample(c, g.enc, g.ids, g.max_new, g.min_new, temp)[:, g.P:].tolist(), None


def assisted_pass(c, g):
    """The temperature-0 pass with a draft model (decoding.assisted_greedy_decode with the timestamp rules)."""
    a_eng, a_encode = c.assistant
    enc_a = g.enc.to(a_eng.lowp) if a_encode is None else a_encode(window(c, g.pending))
    out, nd, na = decoding.assisted_greedy_decode(
        c.eng, a_eng, g.enc, enc_a, g.ids, g.max_new, int(c.num_assistant_tokens), c.eos, suppress_tokens=c.suppress_tokens,
        min_new_tokens=g.min_new, pad_token_id=c.pad, timestamp_rules=c.rules_at(g.P))
    c.model.last_drafted = getattr(c.model, "last_drafted", 0) + nd
    c.model.last_accepted = getattr(c.model, "last_accepted", 0) + na
    out = torch.cat([out, torch.full((out.shape[0], g.P + g.max_new - out.shape[1]), c.pad, dtype=out.dtype, device=c.dev)], 1)
    return out[:, g.P:].tolist(), None


def beam_pass(c, g):
    """The temperature-0 pass as a beam search; with the thresholds also (the hypotheses' `sequences_scores`, their no-speech
    probabilities): the numbers the pass is judged by, without a teacher-forced pass (TF:1261-1264)."""
    out = decoding.beam_search_decode(
        c.eng, g.enc, g.ids, g.max_new, c.nb, c.eos, pad_token_id=c.pad, suppress_tokens=c.suppress_tokens,
        begin_suppress_tokens=c.begin_suppress_tokens, min_new_tokens=g.min_new, length_penalty=float(c.length_penalty),
        early_stopping=c.early_stopping, timestamp_rules=c.rules_at(g.P), return_scores=c.need_scores)
    scored = None
    if c.need_scores:
        out, beam_sc, prefill = out
        scored = (beam_sc.tolist(), beam_no_speech(c, prefill, g.ids, g.P, g.min_new, c.nb))
    return out[:, g.P:].tolist(), scored


def greedy_pass(c, g):
    """The temperature-0 pass on a kept decoding.GreedyDecoder; with token timestamps one alignment pass over the finished
    batch, whose rows go to `g.window_ts`."""
    decoders, P = c.model._seek_decoders, g.P
    key = (len(g.pending), P, g.max_new, c.eos, c.pad, c.nts, c.max_initial_timestamp_index, tuple(c.suppress_tokens or ()),
           tuple(c.begin_suppress_tokens or ()), c.rep_pen, c.ngram, c.sequence_bias)
    dec = decoders.get(key)
    if dec is None:
        if len(decoders) >= 4:             # (a decoder owns its K/V caches: keep a handful alive)
            decoders.pop(next(iter(decoders)))
        dec = decoders[key] = decoding.GreedyDecoder(
            c.eng, len(g.pending), P + g.max_new, eos_token_id=c.eos, suppress_tokens=c.suppress_tokens,
            begin_suppress_tokens=c.begin_suppress_tokens, use_graphs=False, pad_token_id=c.pad,
            check_every=4,                 # eager passes: stop within 3 steps of the last row's EOS
            timestamp_rules=c.rules_at(P), soft=c.hist_soft)
    full = dec.run(g.enc, g.ids, g.max_new, g.min_new)
    if c.token_timestamps is not None:
        from .alignment import extract_token_timestamps
        nf = c.token_timestamps["num_frames"]
        ts = extract_token_timestamps(
            c.model, G.trim_finished(full, P, c.eos, c.pad), g.enc, c.token_timestamps["alignment_heads"],
            None if nf is None else [nf[b] - c.seek[b] for b in g.pending], P, c.token_timestamps["time_precision"]).cpu()
        for i, b in enumerate(g.pending):
            g.window_ts[b] = ts[i]
    return full[:, P:].tolist(), None


def decode_group(c, rows, enc_all, prompts, P, lengths, accepted, window_ts):
    """The utterances of a pass whose decoder prompts have P tokens, down the temperature ladder (TF:970-1116): every pass decodes
    the rows still pending and `judge` says which of them go on to the next temperature.  accepted[b] = (tokens, skip)."""
    pending = [b for b in rows if len(prompts[b]) == P]
    for ti, temp in enumerate(c.temps):
        pos = [rows.index(b) for b in pending]
        g = SimpleNamespace(P=P, pending=pending, max_new=lengths[0], min_new=lengths[1], window_ts=window_ts,
                            enc=enc_all[pos].reshape(len(pending) * c.d.max_src, -1).contiguous(),
                            ids=torch.as_tensor([prompts[b] for b in pending], dtype=torch.long, device=c.dev))
        if temp > 0.0:
            out, scored = sampled_pass(c, g, temp)
        elif c.assistant is not None:
            out, scored = assisted_pass(c, g)
        elif c.nb > 1:
            out, scored = beam_pass(c, g)
        else:
            out, scored = greedy_pass(c, g)
        gens = [strip_pad(c, seq) for seq in out]
        avg = nsp = None
        if c.need_scores:
            avg, nsp = scored if scored is not None else scores_of(c, g.enc, g.ids, gens, g.min_new)
            c.window_scores.extend((b, c.seek[b], float(avg[i]), float(nsp[i])) for i, b in enumerate(pending))
        again = []
        for i, b in enumerate(pending):
            fallback, skip = judge(c, gens[i], avg[i] if c.need_scores else None, nsp[i] if c.need_scores else None)
            accepted[b] = (gens[i], skip)
            c.do_cond[b] = bool(c.condition_on_prev_tokens) and temp < 0.5
            if fallback:
                again.append(b)
        if not again or ti == len(c.temps) - 1:
            break
        pending = again


def lockstep_loop(c):
    """Pass by pass: the next window of every unfinished utterance is encoded, decoded and applied."""
    while any(c.seek[b] < c.max_frames[b] for b in range(c.B)):
        rows = [b for b in range(c.B) if c.seek[b] < c.max_frames[b]]
        snf = {b: min(c.max_frames[b] - c.seek[b], c.W) for b in rows}
        enc_all, _ = c.eng.encode(window(c, rows), save=False)
        enc_all = enc_all[:len(rows) * c.d.max_src].view(len(rows), c.d.max_src, -1)
        prompts = build_prompts(c, rows)
        accepted, window_ts = {}, {}
        # (the reference left-pads the batch to its longest prompt and derives the lengths from that, TF:835-840)
        lengths = c.lengths(max(len(prompts[b]) for b in rows))
        for P in sorted({len(prompts[b]) for b in rows}):
            decode_group(c, rows, enc_all, prompts, P, lengths, accepted, window_ts)
        for b in rows:
            gen, skip = accepted[b]
            apply_window(c, b, gen, skip, snf[b], None if c.token_timestamps is None else (len(prompts[b]), window_ts[b]))
    return c.result()


def seek_decode(model, a):
    """`WhisperForConditionalGeneration.seek_decode` with its arguments `a` by name: the refusals, then one of the two loops."""
    slots, init_tokens = a["slots"], a["init_tokens"]
    facts = G.seek_facts(a)
    if slots is None:
        if a["cross_kv_dtype"] is not None or a["use_graphs"] is not None:
            raise ValueError("seek_decode: cross_kv_dtype / use_graphs belong to the slot schedule (slots=N)")
    else:
        if int(slots) < 1 or int(a["check_every"]) < 1:
            raise ValueError("seek_decode(slots=N) needs N >= 1 slots and check_every >= 1")
        G.refuse(facts, "slots")
        if not callable(init_tokens) and len({len(r) for r in init_tokens}) > 1:
            raise NotImplementedError(ONE_LENGTH)
    G.refuse(facts, "bias", "history")
    c = SeekContext(model, a)                  # (language detection, where asked for, encodes the first windows)
    G.refuse(facts, "no_speech_threshold", "token_timestamps")
    c.start()
    return slot_schedule(c) if slots is not None else lockstep_loop(c)


def assistant_encode(am, feats):
    return am.engine.encode(feats.to(torch.float32).contiguous(), save=False)[0]


def window_lengths(gc, max_tgt, explicit_max_length, P):
    """(max_new_tokens, min_new_tokens) of a pass whose longest decoder prompt has P tokens."""
    max_new, min_new = G.resolve_lengths(gc, P, max_tgt, explicit_max_length)
    if gc.max_new_tokens is None:          # TF:1932-1940 mutates max_length on every pass
        gc.max_length = min(gc.max_length + min(max_tgt // 2 - 1, P), max_tgt)
    return max_new, min_new


def generate_seek_loop(model, plan, input_features, attention_mask, language, task, is_multilingual, prompt_ids, kwargs,
                       return_segments=False):
    """Timestamp-driven multi-pass transcription: `WhisperGenerationMixin.generate` steps 5-7 (TF:745-968) with
    temperature 0 and no fallback thresholds -- every utterance keeps a `seek` position in mel frames; each pass
    decodes the next <= 30 s window of every unfinished utterance with the timestamp rules, `retrieve_segment`
    splits the tokens at consecutive timestamp pairs and advances `seek` to the last predicted end of segment (or
    past the window).  Inputs of any length ([B, n_mels, frames]; batches of long inputs need `attention_mask`).
    Returns the concatenated segment tokens per utterance, right-padded with pad_token_id (the reference's plain
    return value), a GenerateOutput with `.sequences` and `.segments` (return_dict_in_generate), or -- with
    `return_segments=True`, like the reference (TF:generate, "8. If we return all segments") -- a plain dict
    {"sequences", "segments"}: per utterance the list of {"start", "end", "tokens"} in seconds / token ids (the
    reference's entries also carry the raw GenerationMixin output of their window under "result" and "idxs")."""
    from .modeling import _assistant_shares_encoder
    d, gc, token_ts = model.dims, plan.gc, plan.token_ts
    (B, _, frames), dev, W = input_features.shape, input_features.device, 2 * d.max_src
    assistant, begin_suppress_loop = None, (list(gc.begin_suppress_tokens) if gc.begin_suppress_tokens else None)
    am = plan.assistant_model
    if am is not None:
        am._sync_shadow()
        shared = _assistant_shares_encoder(am, d)     # (a distilled student keeps the teacher's encoder)
        a_encode = None if shared else partial(assistant_encode, am)
        assistant = (am.engine, a_encode)
        begin_suppress_loop = None     # TF:719-721: with an assistant the model must be able to return EOS right away
        model.last_drafted = model.last_accepted = 0
    if not hasattr(gc, "no_timestamps_token_id"):
        raise ValueError(G.NO_TIMESTAMPS_TOKEN)
    gc.return_timestamps = True
    G.set_language_and_task(gc, language, task, is_multilingual)
    if B > 1 and frames > W and attention_mask is None:
        raise ValueError("When doing batched long-form audio transcription, make sure to pass an `attention_mask`. "
                         "You can retrieve the `attention_mask` by doing `processor(audio, ..., "
                         "return_attention_mask=True)` ")
    if B > 1 and frames > W:
        max_frames = [int(x) for x in attention_mask.sum(-1).tolist()]
    else:
        max_frames = [frames] * B
    eos, pad = gc.eos_token_id, gc.pad_token_id
    if isinstance(eos, (list, tuple)):
        eos = eos[0]
    if eos is None:
        raise ValueError("return_timestamps=True needs eos_token_id in the generation config")
    if pad is None:
        pad = eos
    all_segments = getattr(gc, "prompt_condition_type", "first-segment") == "all-segments"
    slots = {} if plan.seek_slots is None else dict(slots=int(plan.seek_slots), cross_kv_dtype=plan.cross_kv_dtype,
                                                    use_graphs=plan.use_graphs)
    segments = model.seek_decode(
        input_features, max_frames, partial(G.retrieve_init_tokens, gc, B),
        partial(window_lengths, gc, d.max_tgt, "max_length" in kwargs), eos, pad, int(gc.no_timestamps_token_id),
        getattr(gc, "max_initial_timestamp_index", None), list(gc.suppress_tokens) if gc.suppress_tokens else None,
        begin_suppress_loop,
        detect_language=partial(model._detect_language, B=B, gc=gc), prev_sot_token_id=getattr(gc, "prev_sot_token_id", None),
        prompt_ids=(prompt_ids.tolist() if torch.is_tensor(prompt_ids) else prompt_ids),
        prompt_all_segments=all_segments and prompt_ids is not None, num_beams=plan.num_beams, assistant=assistant,
        num_assistant_tokens=(getattr(gc, "num_assistant_tokens", None) or getattr(
            getattr(am, "generation_config", None), "num_assistant_tokens", None) or 5),
        length_penalty=1.0 if getattr(gc, "length_penalty", None) is None else gc.length_penalty,
        early_stopping=getattr(gc, "early_stopping", False) or False,
        token_timestamps=token_ts, **plan.seek_history, **plan.fallback_args, **slots)
    rows_out = [[tok for sg in segments[b] for tok in sg["tokens"]] for b in range(B)]
    width = max((len(r) for r in rows_out), default=0)
    seqs = torch.full((B, width), pad, dtype=torch.long, device=dev)
    for b, r in enumerate(rows_out):
        if r:
            seqs[b, :len(r)] = torch.as_tensor(r, dtype=torch.long, device=dev)
    if token_ts is not None:
        # `_pad_to_max_length` (TF:150-235): per utterance the windows' own values of its segments' tokens (without the time
        # offsets, as the reference concatenates them), right-padded with the row's last value
        rows_ts = [[sg["result"]["token_timestamps"][sg["idxs"][0]:sg["idxs"][1]] for sg in segments[b]] for b in range(B)]
        ts = torch.zeros((B, width), dtype=torch.float32)
        for b, parts in enumerate(rows_ts):
            if parts:
                row = torch.cat(parts, -1)
                ts[b, :len(row)] = row
                if len(row):
                    ts[b, len(row):] = row[-1]
        if plan.as_dict:                       # TF:945-949: return_dict_in_generate switches return_segments on
            return G.GenerateOutput(seqs, token_timestamps=ts.to(dev), segments=segments)
        return dict({"sequences": seqs, "token_timestamps": ts.to(dev)}, **({"segments": segments} if return_segments else {}))
    if return_segments:
        return {"sequences": seqs, "segments": segments}
    return G.GenerateOutput(seqs, segments=segments) if plan.as_dict else seqs
