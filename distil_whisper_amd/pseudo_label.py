"""Pseudo-labelling throughput path: teacher-only batched generate over 30 s packs.

Reference: run_pseudo_labelling.py:632-673 (`concatenate_dataset`: consecutive samples of one speaker are appended
until the next one would exceed `max_input_length` = 30 s; `condition_on_prev` marks a pack that continues the
previous pack's speaker) and 861-996 (the teacher's `generate` over the packed batches under data parallelism, one
process per GPU, each on its own shard).  Here the packs are gathered on the GPU straight into the log-mel kernel's
[B, 480000] buffer and decoded by decoding.GreedyDecoder; sharding across ranks is by pack index (no collective).
"""
import numpy as np
import torch

from .decoding import GreedyDecoder


def pack_plan(lengths, speaker_ids=None, max_input_length=480000):
    """Greedy packing rule of `concatenate_dataset`: returns (packs, condition_on_prev) where packs[i] is the list of
    sample indices concatenated into pack i.  A sample joins the current pack iff it has the pack's speaker and the
    summed length stays <= max_input_length; otherwise it opens a new pack, flagged 1 when the speaker continues."""
    n = len(lengths)
    if n == 0:
        return [], []
    spk = [None] * n if speaker_ids is None else list(speaker_ids)
    packs, cond = [[0]], [0]
    cur_len, cur_spk = int(lengths[0]), spk[0]
    for i in range(1, n):
        same = spk[i] == cur_spk
        if same and int(lengths[i]) + cur_len <= max_input_length:
            packs[-1].append(i)
            cur_len += int(lengths[i])
        else:
            packs.append([i])
            cond.append(1 if same else 0)
            cur_len, cur_spk = int(lengths[i]), spk[i]
    return packs, cond


def shard(items, rank, world):
    """Contiguous per-rank shard of the pack list (what `accelerator.prepare(dataloader)` does for the reference)."""
    per = (len(items) + world - 1) // world
    return items[rank * per:(rank + 1) * per]


class PseudoLabeller:
    """audios (list of 1-D 16 kHz waveforms, each <= 30 s) -> (token id lists per pack, packs, condition_on_prev)."""

    def __init__(self, model, feature_extractor, batch_size=16, max_new_tokens=255, prompt_ids=None, eos_token_id=None,
                 timestamp_rules=None, use_graphs=None, rank=0, world=1, suppress_tokens=None,
                 begin_suppress_tokens=None, num_beams=1, overlap=False, decode_cus=64, repetition_penalty=None,
                 no_repeat_ngram_size=0, sequence_bias=None, bad_words_ids=None, assistant_model=None, num_assistant_tokens=5,
                 continuous=False, check_every=8, cross_kv_dtype=None, seek_slots=False, seek_group=8):
        from .longform import history_soft, refuse_continuous
        from .kv_quant import normalize_dtype
        self.model, self.fe = model, feature_extractor
        # cross_kv_dtype="fp8": the token loops (GreedyDecoder, SlotDecoder) keep the cross-attention K/V as FP8 codes -- half the
        # bytes the token step streams; opt-in, the labels may differ where two logits are close.  Only the token step reads
        # such a cache: the seek loop, beams and an assistant are refused here.
        cross_kv_dtype = normalize_dtype(cross_kv_dtype)
        # seek_slots=True (with timestamp_rules): the seek loop's windows as jobs of `batch_size` slots (model.seek_decode `slots`),
        # called over groups of seek_group * batch_size packs -- a pack's second window takes a slot as soon as the first has
        # ended, the token steps replay from a graph, and the FP8 cross-attention K/V are allowed.  Same labels.
        self.seek_slots, self.seek_group = bool(seek_slots), int(seek_group)
        if self.seek_slots:
            if timestamp_rules is None:
                raise ValueError("PseudoLabeller(seek_slots=True) schedules the timestamp seek loop: it needs timestamp_rules")
            if self.seek_group < 1 or int(check_every) < 1 or int(batch_size) < 1:
                raise ValueError("PseudoLabeller(seek_slots=True) needs seek_group >= 1, check_every >= 1 and batch_size >= 1")
            if overlap:
                raise ValueError("PseudoLabeller(seek_slots=True) cannot be combined with overlap=True (the slot schedule "
                                 "encodes and decodes in its own order)")
            for on, what in ((int(num_beams) > 1, "num_beams > 1"), (assistant_model is not None, "an assistant_model"),
                             (repetition_penalty not in (None, 1.0) or bool(no_repeat_ngram_size) or sequence_bias is not None
                              or bad_words_ids is not None,
                              "repetition_penalty / no_repeat_ngram_size / sequence_bias / bad_words_ids")):
                if on:
                    raise NotImplementedError(f"PseudoLabeller(seek_slots=True) with {what} is not implemented on the MI355X "
                                              "path (the slot step decodes greedily)")
        self._seek_kw = dict(slots=int(batch_size), check_every=int(check_every), cross_kv_dtype=cross_kv_dtype,
                             use_graphs=use_graphs) if self.seek_slots else {}
        if cross_kv_dtype is not None:
            for on, what in ((int(num_beams) > 1, "num_beams > 1"),
                             (timestamp_rules is not None and not self.seek_slots, "timestamp_rules (the seek loop)"),
                             (assistant_model is not None, "an assistant_model")):
                if on:
                    raise NotImplementedError(f'PseudoLabeller(cross_kv_dtype="fp8") with {what} is not implemented on the MI355X '
                                              "path (only the token step reads FP8 cross-attention K/V)")
        self.B, self.max_new = int(batch_size), int(max_new_tokens)
        self.rank, self.world = rank, world
        self.num_beams = int(num_beams)      # generation_num_beams of run_pseudo_labelling.py:835-843
        self._beam_kw = dict(suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens)
        # GenerationMixin's two rules against repetition loops: inside the selection kernel of the graph-captured token step
        # (decoding.GreedyDecoder `soft`) and of the seek loop's greedy passes; beam search does not take them
        # sequence_bias / bad_words_ids (hot-word boosts, forbidden words): the same launch, the same limits
        soft = history_soft(repetition_penalty, no_repeat_ngram_size, sequence_bias, bad_words_ids, model.dims.vocab, eos_token_id)
        if soft is not None and self.num_beams > 1:
            raise NotImplementedError("repetition_penalty / no_repeat_ngram_size / sequence_bias / bad_words_ids with num_beams > 1 "
                                      "are not implemented on the MI355X path (greedy decoding only)")
        self._history_kw = {} if soft is None else dict(repetition_penalty=soft["repetition_penalty"],
                                                        no_repeat_ngram_size=soft["no_repeat_ngram_size"])
        if soft is not None and soft.get("sequence_bias") is not None:
            self._history_kw["sequence_bias"] = soft["sequence_bias"]
        # assistant_model: speculative decoding of the plain greedy path with per-row acceptance (decoding.assisted_greedy_decode
        # per_row=True; run_eval.py:578-599 gives the teacher its distilled student) -- every pack keeps its own accepted drafts,
        # the labels are the teacher's own greedy labels.  A decoder-only WhisperForCausalLM drafts on the teacher's encoder output.
        self.assistant, self.num_assistant_tokens = assistant_model, int(num_assistant_tokens)
        if assistant_model is not None:
            for on, what in ((self.num_beams > 1, "num_beams > 1"), (timestamp_rules is not None, "timestamp_rules (the seek loop)"),
                             (soft is not None, "repetition_penalty / no_repeat_ngram_size / sequence_bias / bad_words_ids")):
                if on:
                    raise NotImplementedError(f"PseudoLabeller(assistant_model=) with {what} is not implemented on the MI355X path "
                                              "(the assistant drafts for plain greedy decoding)")
            if self.num_assistant_tokens < 1:
                raise ValueError("num_assistant_tokens must be at least 1")
            from .modeling import _assistant_shares_encoder
            self._assistant_own_encoder = not (_assistant_shares_encoder(assistant_model, model.dims))
            self._assist_kw = dict(eos_token_id=eos_token_id, suppress_tokens=suppress_tokens,
                                   begin_suppress_tokens=begin_suppress_tokens, per_row=True)
        d = model.dims
        dev = model.ops.device
        self.dev = dev
        self.prompt = torch.as_tensor([d.decoder_start_token_id] if prompt_ids is None else list(prompt_ids),
                                      dtype=torch.long, device=dev)
        if timestamp_rules is not None:
            timestamp_rules = dict(timestamp_rules, begin_index=len(self.prompt))
        self._ts_rules = timestamp_rules
        self.eos = eos_token_id
        # continuous=True: the plain greedy path on decoding.SlotDecoder -- a pack whose labels have ended hands its row of the token
        # loop to the next waiting pack; the encoder runs a batch ahead of the slots (longform.encoded_windows).  Same labels.
        self.continuous = bool(continuous)
        if self.continuous:
            refuse_continuous("PseudoLabeller", self.num_beams, assistant_model is not None, timestamp_rules is not None,
                              soft is not None, bool(overlap))
            from .decoding import SlotDecoder
            self.slot_decoder = SlotDecoder(model.engine, self.B, len(self.prompt) + self.max_new, eos_token_id,
                                            suppress_tokens=suppress_tokens, begin_suppress_tokens=begin_suppress_tokens,
                                            use_graphs=use_graphs, check_every=check_every, cross_kv_dtype=cross_kv_dtype)
        # (seek_slots=True decodes every window on model.seek_decode's slot decoder: no batch decoder is built)
        self.decoder = None if self.seek_slots else GreedyDecoder(
            model.engine, self.B, len(self.prompt) + self.max_new, eos_token_id=eos_token_id, suppress_tokens=suppress_tokens,
            begin_suppress_tokens=begin_suppress_tokens, use_graphs=use_graphs, timestamp_rules=timestamp_rules, soft=soft,
            cross_kv_dtype=cross_kv_dtype)
        self._wave = torch.zeros((self.B, feature_extractor.n_samples), dtype=torch.float32, device=dev)
        # overlap=True: the encoder of the next batch of packs beside the token loop of the current one (longform.two_stage_pipeline;
        # plain greedy decoding only -- the seek loop and beam search encode / decode in their own order)
        self.overlap = bool(overlap) and torch.device(dev).type == "cuda"
        self.decode_cus = int(decode_cus)

    def __call__(self, audios, speaker_ids=None, gather=False, group=None):
        """`gather=True`: every rank returns the labels of ALL packs (rank-ordered exchange of the id lists, the
        reference's pad_across_processes + gather_for_metrics, run_pseudo_labelling.py:893-895); otherwise packs of
        other ranks' shards come back as None."""
        model = self.model
        model._sync_shadow()
        audios = [torch.as_tensor(np.asarray(a, dtype=np.float32) if not torch.is_tensor(a) else a,
                                  dtype=torch.float32).reshape(-1).to(self.dev) for a in audios]
        packs, cond = pack_plan([a.numel() for a in audios], speaker_ids, self.fe.n_samples)
        mine = shard(list(range(len(packs))), self.rank, self.world)
        prompt = self.prompt[None, :].expand(self.B, -1).contiguous()
        out = {}
        def wave_to_features(batch):
            self._wave.zero_()
            for r, pi in enumerate(batch):
                pos = 0
                for si in packs[pi]:
                    n = audios[si].numel()
                    self._wave[r, pos:pos + n].copy_(audios[si])
                    pos += n
            return model.ops.logmel(self._wave, self.fe._filt)

        batches = [mine[b0:b0 + self.B] for b0 in range(0, len(mine), self.B)]
        plain = not (self._ts_rules is not None and self.num_beams == 1) and self.num_beams == 1
        encode = lambda b: model.engine.encode(wave_to_features(b), save=False)[0]
        decode = lambda enc: self.decoder.run(enc, prompt, self.max_new)
        if self.assistant is not None:
            from .decoding import assisted_greedy_decode
            am = self.assistant
            am._sync_shadow()
            if self._assistant_own_encoder:                # (its encoder differs from the teacher's: both encode the batch)
                def encode(b):
                    feats = wave_to_features(b)
                    return model.engine.encode(feats, save=False)[0], am.engine.encode(feats, save=False)[0]
            else:
                def encode(b, _enc=encode):
                    e = _enc(b)
                    return e, e.to(am.engine.lowp)
            decode = lambda encs: assisted_greedy_decode(model.engine, am.engine, encs[0], encs[1], prompt, self.max_new,
                                                         self.num_assistant_tokens, **self._assist_kw)[0]
        if plain:
            from .longform import continuous_batches, two_stage_pipeline
            if self.continuous:
                decoded = continuous_batches(self.slot_decoder, batches, encode, model.dims.max_src, self.prompt, self.max_new)
            else:
                decoded = two_stage_pipeline(self, model.ops, self.dev, batches, encode, decode, self.overlap, self.decode_cus)
            for batch, ids in decoded:
                for r, pi in enumerate(batch):
                    row = ids[r, self.prompt.numel():].tolist()
                    if self.eos is not None and self.eos in row:
                        row = row[:row.index(self.eos)]
                    out[pi] = [int(x) for x in row]
            batches = []
        if self.seek_slots:
            # groups of seek_group * batch_size packs: the features of a group are held, its windows are scheduled on the slots
            step = self.seek_group * self.B
            for g0 in range(0, len(mine), step):
                group_ = mine[g0:g0 + step]
                feats = torch.cat([wave_to_features(group_[b0:b0 + self.B])[:len(group_[b0:b0 + self.B])].clone()
                                   for b0 in range(0, len(group_), self.B)], 0)
                segs = model.seek_decode(feats, [feats.shape[-1]] * len(group_), [self.prompt.tolist()] * len(group_),
                                         lambda P: (self.max_new, 0), self.eos, self.eos, self._ts_rules["no_timestamps_token_id"],
                                         self._ts_rules.get("max_initial_timestamp_index"), **self._beam_kw, **self._seek_kw)
                for r, pi in enumerate(group_):
                    out[pi] = [int(t) for sg in segs[r] for t in sg["tokens"]]
            batches = []
        for batch in batches:
            feats = wave_to_features(batch)
            if self._ts_rules is not None and self.num_beams == 1:
                # generate(..., return_timestamps=True) of the reference is a seek loop (TF:784-903): a pack is decoded
                # in as many passes as its predicted end-of-segment timestamps require
                nb = len(batch)
                segs = model.seek_decode(feats[:nb], [feats.shape[-1]] * nb, [self.prompt.tolist()] * nb,
                                         lambda P: (self.max_new, 0), self.eos,
                                         self.eos, self._ts_rules["no_timestamps_token_id"],
                                         self._ts_rules.get("max_initial_timestamp_index"), **self._beam_kw,
                                         **self._history_kw)
                for r, pi in enumerate(batch):
                    out[pi] = [int(t) for sg in segs[r] for t in sg["tokens"]]
                continue
            enc, _ = model.engine.encode(feats, save=False)
            from .decoding import beam_search_decode
            ids = beam_search_decode(model.engine, enc, prompt, self.max_new, self.num_beams, self.eos,
                                     timestamp_rules=self._ts_rules, **self._beam_kw).cpu().numpy()
            for r, pi in enumerate(batch):
                row = ids[r, self.prompt.numel():].tolist()
                if self.eos is not None and self.eos in row:
                    row = row[:row.index(self.eos)]
                out[pi] = [int(x) for x in row]
        if gather and self.world > 1:
            from .gather import gather_token_lists
            fill = self.eos if self.eos is not None else 0
            rows = gather_token_lists([out[i] for i in mine], fill, self.dev, group=group)
            if len(rows) != len(packs):
                raise RuntimeError(f"gathered {len(rows)} label rows for {len(packs)} packs: ranks disagree on the plan")
            return rows, packs, cond
        return [out.get(i) for i in range(len(packs))], packs, cond
