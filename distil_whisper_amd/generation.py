"""Host side of `WhisperForConditionalGeneration.generate` for the MI355X engine: generation config, decoder prompt
assembly (language / task / timestamps / prompt_ids), length rules and the output conventions of the reference.

Reference behaviour (the arithmetic lives in the third-party `transformers` package, installed 5.15.0;
`TF:` = transformers/models/whisper/generation_whisper.py):
  * call sites: run_distillation.py:1524-1528 (`generate_step`), run_eval.py:690-739 (`gen_kwargs`: max_length,
    return_timestamps, num_beams, top_k=0, language/task for multilingual checkpoints, assistant_model, prompt_ids and
    the long-form thresholds), run_eval.py:806-844 (`benchmark_gen`: encoder_outputs + min/max_new_tokens),
    run_pseudo_labelling.py:861-996;
  * decoder prompt: TF:1455-1608 `_retrieve_init_tokens` (<|startoftranscript|>, language id, task id,
    <|notimestamps|> unless timestamps are requested), TF:1853-1918 `_prepare_decoder_input_ids` (prompt_ids in front);
  * lengths: TF:1920-1947 `_set_max_new_tokens_and_length`;
  * logits processors and their order: TF:1774-1812 (begin-suppress, suppress, timestamp rules);
  * token-level timestamps (`return_token_timestamps=True`, TF:241-381, 1146-1157, 1685-1700): alignment.py + csrc/align.hip;
    the generation config carries `alignment_heads` ([[layer, head], ...]), the model config `median_filter_width`;
  * per-step scores (`output_scores` / `output_logits` with `return_dict_in_generate`, TF:generation/utils.py `_sample`;
    `compute_transition_scores`): scoring.py + csrc/score.hip;
  * return value: without `return_dict_in_generate` the generated tokens only (decoder prompt and EOS stripped,
    right-padded with pad_token_id, TF:913-957 + `_pad_to_max_length`); with it an object whose `.sequences` holds
    prompt + generated tokens as GenerationMixin returns them.
Everything here is integer host logic; the token loop itself runs on the GPU in decoding.GreedyDecoder.
"""
import copy

import torch

# language code -> name (the public Whisper language list; `language=` accepts a code, a name or "<|code|>")
_LANGS = ("en:english,zh:chinese,de:german,es:spanish,ru:russian,ko:korean,fr:french,ja:japanese,pt:portuguese,"
          "tr:turkish,pl:polish,ca:catalan,nl:dutch,ar:arabic,sv:swedish,it:italian,id:indonesian,hi:hindi,fi:finnish,"
          "vi:vietnamese,he:hebrew,uk:ukrainian,el:greek,ms:malay,cs:czech,ro:romanian,da:danish,hu:hungarian,ta:tamil,"
          "no:norwegian,th:thai,ur:urdu,hr:croatian,bg:bulgarian,lt:lithuanian,la:latin,mi:maori,ml:malayalam,cy:welsh,"
          "sk:slovak,te:telugu,fa:persian,lv:latvian,bn:bengali,sr:serbian,az:azerbaijani,sl:slovenian,kn:kannada,"
          "et:estonian,mk:macedonian,br:breton,eu:basque,is:icelandic,hy:armenian,ne:nepali,mn:mongolian,bs:bosnian,"
          "kk:kazakh,sq:albanian,sw:swahili,gl:galician,mr:marathi,pa:punjabi,si:sinhala,km:khmer,sn:shona,yo:yoruba,"
          "so:somali,af:afrikaans,oc:occitan,ka:georgian,be:belarusian,tg:tajik,sd:sindhi,gu:gujarati,am:amharic,"
          "yi:yiddish,lo:lao,uz:uzbek,fo:faroese,ht:haitian creole,ps:pashto,tk:turkmen,nn:nynorsk,mt:maltese,"
          "sa:sanskrit,lb:luxembourgish,my:myanmar,bo:tibetan,tl:tagalog,mg:malagasy,as:assamese,tt:tatar,haw:hawaiian,"
          "ln:lingala,ha:hausa,ba:bashkir,jw:javanese,su:sundanese,yue:cantonese")
LANGUAGES = dict(item.split(":") for item in _LANGS.split(","))
TO_LANGUAGE_CODE = {name: code for code, name in LANGUAGES.items()}
TO_LANGUAGE_CODE.update({"burmese": "my", "valencian": "ca", "flemish": "nl", "haitian": "ht", "letzeburgesch": "lb",
                         "pushto": "ps", "panjabi": "pa", "moldavian": "ro", "moldovan": "ro", "sinhalese": "si",
                         "castilian": "es", "mandarin": "zh"})
TASK_IDS = ("translate", "transcribe")

# what `generate` understands; anything else raises (the reference's GenerationMixin validates its kwargs as well)
_CONFIG_KEYS = ("max_length", "max_new_tokens", "min_new_tokens", "num_beams", "do_sample", "top_k", "top_p",
                "eos_token_id", "pad_token_id", "bos_token_id", "decoder_start_token_id", "suppress_tokens",
                "begin_suppress_tokens", "no_timestamps_token_id", "max_initial_timestamp_index", "prev_sot_token_id",
                "lang_to_id", "task_to_id", "is_multilingual", "return_timestamps", "language", "task",
                "forced_decoder_ids", "num_return_sequences", "use_cache", "output_scores", "output_logits",
                "return_dict_in_generate",
                "num_assistant_tokens", "prompt_condition_type", "length_penalty", "repetition_penalty",
                "no_repeat_ngram_size", "temperature", "early_stopping", "num_beam_groups", "alignment_heads",
                "sequence_bias", "bad_words_ids")


class GenerationConfig:
    """Attribute bag with the fields of `model.generation_config` the reference reads and writes (run_distillation.py:
    1006-1049, run_eval.py:697; TF:640-700).  Unknown optional fields are simply absent (`hasattr` is False), which is
    what the reference's own checks rely on (e.g. `hasattr(generation_config, "is_multilingual")`)."""

    def __init__(self, **kw):
        self.max_length = 448
        self.max_new_tokens = None
        self.min_new_tokens = None
        self.num_beams = 1
        self.do_sample = False
        self.eos_token_id = None
        self.pad_token_id = None
        self.bos_token_id = None
        self.decoder_start_token_id = None
        self.suppress_tokens = None
        self.begin_suppress_tokens = None
        self.return_timestamps = False
        self.num_return_sequences = 1
        self.use_cache = True
        self.prompt_condition_type = "first-segment"
        for k, v in kw.items():
            setattr(self, k, v)

    @classmethod
    def from_model_config(cls, config):
        g = cls()
        for k in ("eos_token_id", "pad_token_id", "bos_token_id", "decoder_start_token_id", "suppress_tokens",
                  "begin_suppress_tokens", "forced_decoder_ids"):
            v = getattr(config, k, None)
            if v is not None:
                setattr(g, k, copy.copy(v))
        ml = getattr(config, "max_length", None)
        if ml:
            g.max_length = ml
        return g

    @classmethod
    def from_any(cls, obj):
        """Copy of a GenerationConfig of this module, of `transformers`, or of a plain dict."""
        if obj is None:
            return cls()
        if isinstance(obj, cls):
            return copy.deepcopy(obj)
        d = obj if isinstance(obj, dict) else (obj.to_dict() if hasattr(obj, "to_dict") else vars(obj))
        g = cls()
        for k, v in d.items():
            if k.startswith("_") or k in ("transformers_version",):
                continue
            if v is None and not hasattr(g, k):
                continue
            setattr(g, k, copy.deepcopy(v))
        return g

    def to_dict(self):
        return {k: copy.deepcopy(v) for k, v in vars(self).items() if not k.startswith("_")}

    def __repr__(self):
        return f"GenerationConfig({self.to_dict()})"


class GenerateOutput:
    """`return_dict_in_generate=True` result: .sequences int64 [B, prompt + generated] (GenerateEncoderDecoderOutput);
    .scores / .logits (output_scores / output_logits, else None): scoring.StepScores, one f32 [B, vocab] tensor per generated step."""

    def __init__(self, sequences, scores=None, token_timestamps=None, segments=None, logits=None):
        self.sequences = sequences
        self.scores = scores
        self.logits = logits
        if token_timestamps is not None:       # return_token_timestamps=True: float32 seconds per token of `sequences`
            self.token_timestamps = token_timestamps
        if segments is not None:
            self.segments = segments

    def __getitem__(self, k):
        return getattr(self, k)

    def keys(self):
        return [k for k in ("sequences", "scores", "logits", "token_timestamps", "segments") if getattr(self, k, None) is not None]


def language_to_id(language, gc):
    """TF:1465-1488."""
    language = language.lower()
    if language in gc.lang_to_id:
        token = language
    elif language in TO_LANGUAGE_CODE:
        token = f"<|{TO_LANGUAGE_CODE[language]}|>"
    elif language in TO_LANGUAGE_CODE.values():
        token = f"<|{language}|>"
    else:
        is_code = len(language) == 2
        raise ValueError(f"Unsupported language: {language}. Language should be one of:"
                         f" {list(TO_LANGUAGE_CODE.values()) if is_code else list(TO_LANGUAGE_CODE.keys())}.")
    if token not in gc.lang_to_id:
        raise ValueError(f"{token} is not supported by this specific model as it is not in the "
                         "`generation_config.lang_to_id`. (You should just add it to the generation config)")
    return gc.lang_to_id[token]


def set_language_and_task(gc, language, task, is_multilingual):
    """TF:1420-1453 (same checks, same messages)."""
    if is_multilingual is not None:
        if not hasattr(gc, "is_multilingual"):
            raise ValueError("The generation config is outdated and is thus not compatible with the `is_multilingual` "
                             "argument to `generate`. Please update the generation config.")
        gc.is_multilingual = is_multilingual
    if hasattr(gc, "is_multilingual") and not gc.is_multilingual:
        if task is not None or language is not None:
            raise ValueError("Cannot specify `task` or `language` for an English-only model. If the model is intended "
                             "to be multilingual, pass `is_multilingual=True` to generate, or update the generation "
                             "config.")
    if language is not None:
        if not hasattr(gc, "lang_to_id"):
            raise ValueError("The generation config is outdated and is thus not compatible with the `language` "
                             "argument to `generate`. Please update the generation config.")
        gc.language = language
    if task is not None:
        if not hasattr(gc, "task_to_id"):
            raise ValueError("The generation config is outdated and is thus not compatible with the `task` argument "
                             "to `generate`. Please update the generation config.")
        gc.task = task


def retrieve_init_tokens(gc, batch_size, detect_language=None):
    """TF:1455-1608: the forced decoder prefix per batch row as a python list of lists.  `detect_language()` is called
    (and must return one language token id per row) when the config knows languages but none was given."""
    task = getattr(gc, "task", None)
    language = getattr(gc, "language", None)
    init = [gc.decoder_start_token_id]
    if task is None and language is None:
        forced = getattr(gc, "forced_decoder_ids", None)
        if forced is not None and len(forced) > 0 and forced[0][0] == 1:
            forced = [list(f) for f in forced]
            i = 1
            while len(forced) > 0 and forced[0][0] == i:
                init.append(forced[0][1])
                forced = forced[1:]
                i += 1
            if len(forced) > 0:
                raise ValueError("You are using token ids in `forced_decoder_ids` that do not seem to correctly follow "
                                 f"the prompt pattern of Whisper. Make sure that {forced} has an entry for all "
                                 f"indices >= 1 and < {forced[0][0]}.")
    undefined_lang = len(init) <= 1 or init[1] is None
    if isinstance(language, (list, tuple)):
        if any(l is None for l in language):
            raise TypeError("Expected `language` to be `None`, a single string (e.g. `'en'`), or a list of strings "
                            "with length equal to the batch size. Got a list containing `None`.")
        if len(language) != batch_size:
            raise ValueError("When passing a list of languages, the length of the list must match the batch size. "
                             f"Expected length of {batch_size}, but got {len(language)} languages.")
        languages = list(language)
    elif language is None:
        languages = [None] * batch_size
    else:
        languages = [language]
    rows = [list(init) for _ in languages]
    lang_ids = None
    if language is not None:
        lang_ids = [language_to_id(l, gc) for l in languages]
    elif hasattr(gc, "lang_to_id") and undefined_lang:
        if detect_language is None:
            raise ValueError("language detection needs the model")
        lang_ids = [int(x) for x in detect_language()]
    if lang_ids is not None:
        for i in range(len(rows)):
            if len(rows[i]) > 1:
                rows[i][1] = lang_ids[i]
            else:
                rows[i].append(lang_ids[i])
    for i in range(len(rows)):
        if task is not None:
            if task not in TASK_IDS:
                raise ValueError(f"The `{task}` task is not supported. The task should be one of `{list(TASK_IDS)}`")
            rows[i].append(gc.task_to_id[task])
            # (the reference calls replace_or_add here and drops its result: the append above is the whole effect)
        elif language is not None and hasattr(gc, "task_to_id"):
            if not any(t in rows[i] for t in gc.task_to_id.values()):
                rows[i].append(gc.task_to_id["transcribe"])
        if not gc.return_timestamps and hasattr(gc, "no_timestamps_token_id") and \
                rows[i][-1] != gc.no_timestamps_token_id:
            rows[i].append(gc.no_timestamps_token_id)
        elif gc.return_timestamps and rows[i][-1] == getattr(gc, "no_timestamps_token_id", None):
            rows[i] = rows[i][:-1]
        rows[i] = [t for t in rows[i] if t is not None]
    if len(rows) == 1 and batch_size > 1:
        rows = [list(rows[0]) for _ in range(batch_size)]
    return rows


def resolve_lengths(gc, prompt_len, max_target_positions, explicit_max_length):
    """-> (max_new_tokens, min_new_tokens) for a decoder prompt of prompt_len tokens.  TF:1920-1947 plus
    GenerationMixin._prepare_generated_length: `max_new_tokens` wins over `max_length`; a `max_length` is extended by
    the (capped) prompt length because the reference counts it for the text after the forced prefix; the total never
    exceeds max_target_positions."""
    mnt = gc.max_new_tokens
    if (mnt or 0) + prompt_len > max_target_positions and mnt is not None:
        raise ValueError(
            f"The length of `decoder_input_ids`, including special start tokens, prompt tokens, and previous tokens, "
            f"is {prompt_len},  and `max_new_tokens` is {mnt}. Thus, the combined length of `decoder_input_ids` and "
            f"`max_new_tokens` is: {mnt + prompt_len}. This exceeds the `max_target_positions` of the Whisper model: "
            f"{max_target_positions}. You should either reduce the length of your prompt, or reduce the value of "
            f"`max_new_tokens`, so that their combined length is less than {max_target_positions}.")
    if mnt is None:
        # TF:1932-1940: `max_length` counts the text after the forced prefix -- it is extended by the (capped) prompt
        # length and bounded by max_target_positions; GenerationMixin then stops at that total length
        num_initial = min(max_target_positions // 2 - 1, prompt_len)
        max_length = min(gc.max_length + num_initial, max_target_positions)
        mnt = max_length - prompt_len
        if mnt <= 0:
            raise ValueError(f"Input length of decoder_input_ids is {prompt_len}, but `max_length` is set to "
                             f"{max_length}. This can lead to unexpected behavior. You should consider increasing "
                             "`max_length` or, better yet, setting `max_new_tokens`.")
    mn = gc.min_new_tokens or 0
    return int(mnt), int(min(mn, mnt))


def strip_and_pad(sequences, prompt_len, eos_token_id, pad_token_id, token_timestamps=None):
    """The plain return value of the reference's `generate` (TF:1060-1093 + `_pad_to_max_length`): per row the tokens
    after the decoder prompt, with trailing pads and the final EOS removed, right-padded to the longest row.
    token_timestamps (float32 [B, seq_len], return_token_timestamps=True): -> (tokens, the kept tokens' times, each row
    right-padded with its last value, TF:188-229)."""
    rows = []
    for row in sequences.tolist():
        seq = row[prompt_len:]
        if len(seq) and pad_token_id is not None and seq[-1] == pad_token_id:
            n_pad = sum(1 for t in seq if t == pad_token_id)
            if pad_token_id == eos_token_id:
                n_pad -= 1
            if n_pad:
                seq = seq[:-n_pad]
        if len(seq) and eos_token_id is not None and seq[-1] == eos_token_id:
            seq = seq[:-1]
        rows.append(seq)
    width = max((len(r) for r in rows), default=0)
    out = torch.full((len(rows), width), pad_token_id if pad_token_id is not None else 0, dtype=torch.long,
                     device=sequences.device)
    for i, r in enumerate(rows):
        if r:
            out[i, : len(r)] = torch.as_tensor(r, dtype=torch.long, device=sequences.device)
    if token_timestamps is not None:
        ts = torch.zeros((len(rows), width), dtype=token_timestamps.dtype, device=token_timestamps.device)
        for i, r in enumerate(rows):
            if r:
                ts[i, : len(r)] = token_timestamps[i, prompt_len:prompt_len + len(r)]
                ts[i, len(r):] = ts[i, len(r) - 1]
        return out, ts
    return out


def retrieve_segment(seq, timestamp_begin, seek_num_frames, time_offset=0.0, time_precision=0.02,
                     time_precision_features=0.01, input_stride=2, with_idxs=False):
    """`WhisperGenerationMixin._retrieve_segment` (TF:generation_whisper.py:1977-2075) on a list of token ids: split the
    tokens generated for one window at consecutive timestamp pairs ("end of segment" predictions) and say how many mel
    frames the window consumed.  -> (segments [{"start", "end", "tokens"}], segment_offset in frames).  with_idxs: every
    segment also says which slice of `seq` it is ("idxs", without the reference's decoder-prompt offset)."""
    n = len(seq)
    ts = [t >= timestamp_begin for t in seq]
    single_ending = ts[-2:] == [False, True]
    pairs = [i + 1 for i in range(n - 1) if ts[i] and ts[i + 1]]
    if pairs:
        slices = list(pairs)
        if single_ending:
            slices.append(n)
        else:
            slices[-1] += 1            # keep the last timestamp in the last segment: it marks "no single ending"
        segments, last = [], 0
        for i, cur in enumerate(slices):
            sl = seq[last:cur]
            is_last = i == len(slices) - 1
            end_tok = sl[-1] if (not is_last or single_ending) else sl[-2]
            segments.append({"start": time_offset + (sl[0] - timestamp_begin) * time_precision,
                             "end": time_offset + (end_tok - timestamp_begin) * time_precision, "tokens": sl})
            if with_idxs:
                segments[-1]["idxs"] = (last, cur)
            last = cur
        if single_ending:
            offset = int(seek_num_frames)          # a single timestamp at the end: no speech after it
        else:
            offset = (seq[last - 2] - timestamp_begin) * input_stride   # resume at the last predicted end of segment
        return segments, int(offset)
    stamps = [t for t in seq if t >= timestamp_begin]
    last_pos = int(seek_num_frames * time_precision_features / time_precision)
    if stamps and stamps[-1] != timestamp_begin:
        last_pos = stamps[-1] - timestamp_begin
    seg = {"start": time_offset, "end": time_offset + last_pos * time_precision, "tokens": list(seq)}
    if with_idxs:
        seg["idxs"] = (0, n)
    return [seg], int(seek_num_frames)


NO_TIMESTAMPS_TOKEN = ("You are trying to return timestamps, but the generation config is not properly set. Make "
                       "sure to initialize the generation config with the correct attributes that are needed "
                       "such as `no_timestamps_token_id`.")


def trim_finished(seqs, P, eos, pad):
    """GenerationMixin stops as soon as every row has emitted EOS: drop the all-padding columns a decoder that
    checks the stop condition every few steps (HIP-graph replay) may have appended."""
    if eos is None or seqs.shape[1] <= P:
        return seqs
    gen = seqs[:, P:]
    is_eos = gen == eos
    n = gen.shape[1]
    first = torch.where(is_eos.any(1), is_eos.float().argmax(1) + 1, torch.full((gen.shape[0],), n, device=gen.device))
    keep = int(first.max().item())
    return seqs[:, : P + keep]


def timestamp_rules(no_timestamps_token_id, max_initial_timestamp_index, begin_index=None):
    """The timestamp rules as the decoders and `processed_scores` take them; `begin_index` (the decoder prompt's length) where
    the consumer does not know it by itself (scoring.score_sequences and the slot step do)."""
    rules = dict(no_timestamps_token_id=int(no_timestamps_token_id), max_initial_timestamp_index=max_initial_timestamp_index)
    return rules if begin_index is None else dict(rules, begin_index=begin_index)


# ---- which arguments may not be combined --------------------------------------------------------------------------------
# The predicates of the table below and how a message names them.  `generate` (resolve_generate) and `seek_decode` (seek_facts)
# each state them once, on their own arguments; a predicate an entry point does not have is off.
LABELS = {
    "slots": "seek_slots / slots=N (the timestamp seek loop as a slot schedule)", "slots_below_one": "a number of slots below 1",
    "seek_loop": "the timestamp seek loop (return_timestamps=True without force_unique_generate_call, or more than 30 s of input)",
    "single_window": "single-window decoding (without the timestamp seek loop)", "no_timestamps": "return_timestamps off",
    "unique_call": "force_unique_generate_call", "encoder_outputs": "encoder_outputs", "decoder_input_ids": "decoder_input_ids",
    "positive_temperature": "a positive temperature (sampled fallback passes)",
    "plain_sampling": "plain sampling (positive temperature)",
    "fallback": "the temperature fallback / condition_on_prev_tokens (the seek loop)",
    "fallback_without_slots": "the temperature fallback / condition_on_prev_tokens without seek_slots (the lockstep seek loop)",
    "cond_prev": "condition_on_prev_tokens", "no_cond_prev": "condition_on_prev_tokens=True missing",
    "cond_prev_several": "condition_on_prev_tokens=True over several utterances", "length_penalty": "length_penalty",
    "beams": "beam search (num_beams > 1)", "no_beams": "num_beams=1", "beam_groups": "num_beam_groups > 1",
    "assistant": "an assistant_model", "no_assistant": "no assistant_model", "per_row": "assistant_per_row=True",
    "token_timestamps": "return_token_timestamps", "history": "repetition_penalty / no_repeat_ngram_size",
    "bias": "sequence_bias / bad_words_ids", "soft": "sampling / repetition_penalty / no_repeat_ngram_size",
    "history_or_bias": "repetition_penalty / no_repeat_ngram_size / sequence_bias / bad_words_ids", "no_cache": "use_cache=False",
    # the two differ on purpose: the slot schedule refuses the flags as such, single-window decoding only what it would have to
    # return (without return_dict_in_generate the reference drops both flags, and so does this path)
    "output_flags": "output_scores / output_logits (with or without return_dict_in_generate)",
    "step_scores": "output_scores / output_logits with return_dict_in_generate", "return_segments": "return_segments",
    "all_segments": "prompt_condition_type='all-segments'", "no_speech_threshold": "no_speech_threshold",
    "fp8": 'cross_kv_dtype="fp8"', "fp8_without_slots": 'cross_kv_dtype="fp8" without seek_slots',
    "no_logprob_threshold": "no logprob_threshold",
}
LEFT_PADS = ("the reference left-pads that batch with pad_token_id and its processors then count the pads as history, while this "
             "package decodes rows in groups of equal prompt length (no pads); pass one utterance per call")
SOFT_ONLY = ("implemented for greedy single-window decoding and the seek loop's greedy passes with the KV cache: not with "
             "beams, an assistant or use_cache=False")
SCHEDULES_SEEK_LOOP = "the slot schedule is the timestamp seek loop and needs return_timestamps=True and input_features"
STEP_SCORES = "per-step scores come from single-window greedy search"
NIE = NotImplementedError
# (feature, options, exception class, why): with the feature's predicate and one of the options' on, `refuse` raises, naming
# both.  Rows and options in the order the checks are made.
REFUSALS = (
    ("beams", ("beam_groups",), NIE, "group beam search"),
    ("slots", ("no_timestamps", "unique_call", "encoder_outputs"), ValueError, SCHEDULES_SEEK_LOOP),
    ("slots", ("slots_below_one",), ValueError, "seek_slots is the number of slots, at least 1"),
    ("slots", ("positive_temperature", "cond_prev", "beams", "assistant", "token_timestamps", "history_or_bias", "no_cache",
               "output_flags", "decoder_input_ids"), NIE, "the slot step decodes the windows greedily at temperature 0"),
    ("length_penalty", ("no_beams",), NIE, "length_penalty belongs to beam search"),
    ("per_row", ("no_assistant",), ValueError, "assistant_per_row=True needs an assistant_model"),
    ("per_row", ("no_cache", "beams"), NIE, "every row accepts its own draft prefix of a greedy search on the KV caches"),
    ("bias", ("beams", "assistant", "plain_sampling", "no_cache", "step_scores", "token_timestamps"), NIE,
     "the bias table is applied by the selection kernel of greedy decoding"),
    ("bias", ("cond_prev_several",), NIE, LEFT_PADS),
    ("soft", ("beams", "assistant", "no_cache"), NIE, SOFT_ONLY),
    ("history", ("beams", "assistant"), NIE, SOFT_ONLY),
    ("history", ("cond_prev_several",), NIE, LEFT_PADS),
    ("step_scores", ("beams", "assistant", "soft"), NIE, STEP_SCORES),
    ("no_speech_threshold", ("no_logprob_threshold",), ValueError,
     "no_speech_threshold needs logprob_threshold (the reference compares both)"),
    ("token_timestamps", ("beams", "assistant", "plain_sampling", "fallback", "positive_temperature"), NIE,
     "token timestamps are implemented for greedy decoding, single window and the timestamp seek loop"),
    ("fp8", ("no_cache",), ValueError, 'cross_kv_dtype="fp8" is a format of the KV cache'),
    ("fp8", ("beams", "assistant", "step_scores", "token_timestamps", "fallback_without_slots"), NIE,
     "only the token step reads FP8 cross-attention K/V"),
    ("encoder_outputs", ("fallback",), NIE, "the seek loop encodes every window itself and needs input_features"),
    ("seek_loop", ("fp8_without_slots",), NIE, "the FP8 cache is implemented for single-window decoding and the slot schedule"),
    ("seek_loop", ("plain_sampling",), NIE, "a temperature tuple runs the seek loop's sampled fallback passes"),
    ("seek_loop", ("per_row", "step_scores"), NIE, "both are implemented for single-window greedy search"),
    ("seek_loop", ("decoder_input_ids",), NIE, "pass prompt_ids, or force_unique_generate_call=True for a single window"),
    ("all_segments", ("no_cond_prev",), ValueError,
     "Make sure to set `condition_on_prev_tokens=True` when setting `prompt_condition_type='all-segments'`."),
    ("seek_loop", ("no_cache",), NIE, "the seek loop runs on the KV-cache decoder only"),
    ("assistant", ("beams",), ValueError, "assistant_model cannot be combined with beam search (TF raises the same)"),
    ("single_window", ("return_segments",), NIE, "return_segments comes with the timestamp seek loop (return_timestamps=True)"),
    ("single_window", ("fallback",), NIE, "the heuristics belong to the timestamp seek loop (return_timestamps=True)"),
)
MESSAGES = {NIE: "{feature} combined with {option} is not implemented on the MI355X path ({why})",
            ValueError: "{feature} with {option}: {why}"}


class Facts:
    """Attribute bag; every predicate of LABELS is off until its owner sets it.  A predicate that has to convert a value the
    caller gave (a temperature, the number of slots) is a callable, so that it runs where the table asks for it and not before
    an earlier refusal."""

    def __init__(self, **kw):
        self.__dict__.update(dict.fromkeys(LABELS, False), **kw)

    def on(self, name):
        v = getattr(self, name)
        return v() if callable(v) else v


def refuse(facts, *features):
    """Walks REFUSALS in its order over the rows of `features` and raises on the first whose two predicates are on."""
    for feature, options, exc, why in REFUSALS:
        if feature not in features or not facts.on(feature):
            continue
        for option in options:
            if facts.on(option):
                raise exc(MESSAGES[exc].format(feature=LABELS[feature], option=LABELS[option], why=why))


def seek_facts(a):
    """`seek_decode`'s arguments `a` (by name) as predicates of REFUSALS; what it cannot be asked -- use_cache, output flags,
    decoder_input_ids -- stays off."""
    t, cond = a["temperatures"], bool(a["condition_on_prev_tokens"])
    positive = lambda: any(x is not None and float(x) > 0.0 for x in (t if isinstance(t, (list, tuple)) else [t]))
    history = a["repetition_penalty"] not in (None, 1.0) or bool(a["no_repeat_ngram_size"])
    bias = a["sequence_bias"] is not None
    return Facts(slots=a["slots"] is not None, positive_temperature=positive, cond_prev=cond,
                 cond_prev_several=cond and a["input_features"].shape[0] > 1, beams=int(a["num_beams"]) > 1,
                 assistant=a["assistant"] is not None, token_timestamps=a["token_timestamps"] is not None, history=history,
                 bias=bias, history_or_bias=history or bias, no_speech_threshold=a["no_speech_threshold"] is not None,
                 no_logprob_threshold=a["logprob_threshold"] is None)


class GeneratePlan(Facts):
    """What `generate` knows before the encoder runs (resolve_generate): the merged generation config `gc`, `temps`,
    `fallback_args`, `uses_fallback`, `sample_temp`, `num_beams`, `soft` (the decoder's dict; as a predicate: any of it is on),
    `bias_table`, `seek_history` (the seek loop's keywords), `as_dict`, `want_scores`, `want_logits`, `token_ts`,
    the normalised `cross_kv_dtype`, `seek_slots`, `use_cache`, `use_graphs`,
    `assistant_model`, `return_timestamps`, and the predicates of REFUSALS."""


def resolve_generate(dims, generation_config, kwargs, *, input_features, unimplemented, return_timestamps, task,
                     condition_on_prev_tokens, temperature, compression_ratio_threshold, logprob_threshold, no_speech_threshold,
                     attention_mask, time_precision, return_token_timestamps, return_segments, return_dict_in_generate,
                     force_unique_generate_call, use_graphs, cross_kv_dtype, seek_slots):
    """Everything `generate` does before the encoder, on its arguments of the same names (`unimplemented`: name -> value of
    those the engine path refuses when set; `kwargs`: the rest).  Pure host work on `dims` and the generation config; each fact
    is computed once, and every combination the engine path does not run is raised here, in the order of REFUSALS, between the
    validations of single arguments -> GeneratePlan."""
    # ---- arguments the engine path does not implement: loud, never ignored
    for name, val in unimplemented.items():
        if val is not None and (not hasattr(val, "__len__") or len(val) > 0):
            raise NotImplementedError(f"generate({name}=...) is not implemented on the MI355X engine path")
    cond = bool(condition_on_prev_tokens)
    temps = list(temperature) if isinstance(temperature, (list, tuple)) else [temperature]
    fallback_args = dict(temperatures=temps, compression_ratio_threshold=compression_ratio_threshold,
                         logprob_threshold=logprob_threshold, no_speech_threshold=no_speech_threshold,
                         condition_on_prev_tokens=cond)
    uses_fallback = cond or compression_ratio_threshold is not None or logprob_threshold is not None or \
        no_speech_threshold is not None or len(temps) > 1
    # plain sampling: as in the reference's generate_with_fallback (TF:generation_whisper.py `do_sample = temperature is not
    # None and temperature > 0.0`), a positive `temperature` IS the switch -- `do_sample=True` alone decodes greedily
    sample_temp = float(temps[0]) if (not uses_fallback and temps[0] is not None and temps[0] > 0.0) else None
    engine_keys = ("encoder_outputs", "assistant_model", "decoder_input_ids", "use_cache", "assistant_per_row")
    unknown = [k for k in kwargs if k not in _CONFIG_KEYS and k not in engine_keys]
    if unknown:
        raise ValueError(f"The following `model_kwargs` are not used by the model: {unknown} (note: typos in the "
                         "generate arguments will also show up in this list)")
    gc = GenerationConfig.from_any(generation_config)
    for k in _CONFIG_KEYS:
        if k in kwargs and kwargs[k] is not None:
            setattr(gc, k, kwargs[k])
    num_beams = int(getattr(gc, "num_beams", 1) or 1)
    rp, nrn = getattr(gc, "repetition_penalty", None), int(getattr(gc, "no_repeat_ngram_size", 0) or 0)
    history = rp not in (None, 1.0) or bool(nrn)
    bias_given = getattr(gc, "sequence_bias", None) is not None or getattr(gc, "bad_words_ids", None) is not None
    output_flags = bool(getattr(gc, "output_scores", False)) or bool(getattr(gc, "output_logits", False))
    # per-step scores (TF:generation/utils.py `_sample`: `scores` / `raw_logits`); without return_dict_in_generate the
    # reference drops both flags, and so does this path
    as_dict = bool(return_dict_in_generate or getattr(gc, "return_dict_in_generate", False))
    want_scores = as_dict and bool(getattr(gc, "output_scores", False))
    want_logits = as_dict and bool(getattr(gc, "output_logits", False))
    if return_timestamps is None:
        return_timestamps = bool(getattr(gc, "return_timestamps", False))
    use_cache = kwargs.get("use_cache", True)
    n_utt = input_features if input_features is not None else kwargs.get("encoder_outputs")
    n_utt = n_utt.shape[0] if torch.is_tensor(n_utt) and n_utt.dim() == 3 else None
    p = GeneratePlan(
        gc=gc, temps=temps, fallback_args=fallback_args, uses_fallback=uses_fallback, sample_temp=sample_temp,
        num_beams=num_beams,
        as_dict=as_dict, want_scores=want_scores, want_logits=want_logits, return_timestamps=return_timestamps,
        seek_slots=seek_slots, use_cache=True if use_cache is None else use_cache, use_graphs=use_graphs,
        assistant_model=kwargs.get("assistant_model"), bias_table=None, soft=None, token_ts=None,
        # the predicates
        slots=seek_slots is not None, no_timestamps=not return_timestamps, unique_call=bool(force_unique_generate_call),
        encoder_outputs=kwargs.get("encoder_outputs") is not None,
        slots_below_one=lambda: isinstance(seek_slots, bool) or int(seek_slots) < 1,
        positive_temperature=lambda: any(t is not None and float(t) > 0.0 for t in temps), plain_sampling=sample_temp is not None,
        fallback=uses_fallback, fallback_without_slots=uses_fallback and seek_slots is None, cond_prev=cond, no_cond_prev=not cond,
        cond_prev_several=cond and n_utt is not None and n_utt > 1, beams=num_beams > 1, no_beams=num_beams == 1,
        beam_groups=(getattr(gc, "num_beam_groups", 1) or 1) != 1, assistant=kwargs.get("assistant_model") is not None,
        no_assistant=kwargs.get("assistant_model") is None, per_row=bool(kwargs.get("assistant_per_row", False)),
        token_timestamps=bool(return_token_timestamps), history_or_bias=history or bias_given,
        no_cache=use_cache is False, output_flags=output_flags, step_scores=want_scores or want_logits,
        decoder_input_ids=kwargs.get("decoder_input_ids") is not None,
        length_penalty=getattr(gc, "length_penalty", None) not in (None, 1.0), return_segments=bool(return_segments))
    # seek_slots=N: everything the slot schedule (seek_decode `slots`) does not run is refused here, before the encoder runs
    refuse(p, "beams", "slots")
    if (getattr(gc, "num_return_sequences", 1) or 1) != 1:
        raise NotImplementedError("num_return_sequences > 1 is not implemented on the MI355X path")
    # assistant_per_row=True: speculative decoding in which every row accepts its own draft prefix (decoding.
    # assisted_greedy_decode per_row).  Single-window greedy decoding on the KV caches only
    refuse(p, "length_penalty", "per_row")
    # sequence_bias / bad_words_ids (SequenceBiasLogitsProcessor / NoBadWordsLogitsProcessor): validated and flattened on the
    # host, applied by the selection kernel of greedy decoding (decoding.GreedyDecoder `soft`); elsewhere they raise
    if bias_given:
        from .decoding import sequence_bias_table
        p.bias_table = sequence_bias_table(getattr(gc, "sequence_bias", None), getattr(gc, "bad_words_ids", None), dims.vocab,
                                           gc.eos_token_id)
        p.bias = p.bias_table is not None          # (bad words that are all [eos] leave nothing to apply)
    refuse(p, "bias")
    # history-dependent processors / sampling (GenerationMixin's repetition penalty, no-repeat n-gram, temperature / top-k /
    # top-p sampling): on the single-call KV-cache decoder (decoding.GreedyDecoder `soft`); elsewhere they raise
    if sample_temp is not None or history or p.bias:
        # (an unset top_k is GenerationMixin's global default of 50 when sampling; run_eval.py:739 passes top_k=0 = off)
        tk = getattr(gc, "top_k", None)
        p.soft = dict(do_sample=sample_temp is not None, temperature=sample_temp, top_k=50 if tk is None else tk,
                      top_p=getattr(gc, "top_p", None), repetition_penalty=rp, no_repeat_ngram_size=nrn)
        if p.bias:
            p.soft["sequence_bias"] = p.bias_table
    p.seek_history = dict(repetition_penalty=rp, no_repeat_ngram_size=nrn, sequence_bias=p.bias_table)
    if gc.decoder_start_token_id is None:
        gc.decoder_start_token_id = dims.decoder_start_token_id
    refuse(p, "soft", "step_scores")
    # ---- token-level timestamps (TF:1685-1700 `_set_num_frames`): what the alignment pass needs, or a loud refusal
    if return_token_timestamps:
        from . import alignment as A
        if task == "translate" or (task is None and getattr(gc, "task", None) == "translate"):
            A.logger.warning(A.TRANSLATE_WARNING)
        if not hasattr(gc, "alignment_heads"):
            raise A.TokenTimestampsUnavailable(A.NO_ALIGNMENT_HEADS)
        A.check_filter_width(int(dims.median_filter_width))
        refuse(p, "token_timestamps")
        if attention_mask is not None:
            nf = [int(x) for x in attention_mask.sum(-1).tolist()]
        else:
            A.warn_once(A.NO_ATTENTION_MASK)
            nf = None
        p.token_ts = dict(alignment_heads=[list(x) for x in gc.alignment_heads], num_frames=nf,
                          time_precision=time_precision)
    # ---- FP8 cross-attention K/V: only the token step of decoding.GreedyDecoder reads them; refused before the encoder runs
    from . import kv_quant
    p.cross_kv_dtype = kv_quant.normalize_dtype(cross_kv_dtype)
    if p.cross_kv_dtype is not None:
        kv_quant.check_width(dims.d_model)
        p.fp8, p.fp8_without_slots = True, seek_slots is None
        refuse(p, "fp8")
    return p
