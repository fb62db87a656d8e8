"""TEST INFRASTRUCTURE -- which combinations of `generate` / `seek_decode` arguments are refused, with which exception class and on
which side of the encoder, and what the seek loop's two schedules log on the planted model of tests/seek_slots_cases.py.

tools/record_generate_refusals.py writes what this module observes into tests/golden/generate_refusals.json (made once, from the
commit named in the file, and never regenerated from later code); tests/test_generate_refusals.py replays it on the working tree.
Everything runs on the CPU (oracle.ref_ops in fp32); `engine.encode` is replaced by a stub that raises `EncoderReached`, so nothing
is decoded."""
import itertools

import torch

from oracle import gen_golden_decode as gd

FP8 = "cross_kv_dtype=fp8"


class EncoderReached(Exception):
    pass


def models():
    """-> {width: model}: gd.CFG_T (d_model 128, no FP8 token-step kernel) for every row but the FP8 atom's, which uses the width of
    tests/test_cross_kv_fp8.py (384); multilingual fields with timestamps and alignment heads; the encoder raises EncoderReached."""
    from oracle import whisper_oracle as wo
    from oracle.ref_ops import RefOps
    from tests.test_decode_parity import _model
    ops = RefOps("cpu", lowp=torch.float32)
    fields = gd.generation_fields(multilingual=True, suppress=True, timestamps=True)
    cfg384 = wo.OracleConfig(384, 6, 768, 1, 2, gd.V, 80, pad_token_id=gd.EOS, decoder_start_token_id=gd.SOT)
    out = {128: _model(ops, gd.CFG_T, gd.weights(300), fields), 384: _model(ops, cfg384, wo.init_state_dict(cfg384, 23, std=0.1), fields)}
    for m in out.values():
        m.generation_config.alignment_heads = [[0, 1], [1, 0]]
        m.reached = []

        def stub(*a, _m=m, **k):
            _m.reached.append(True)
            raise EncoderReached()
        m.engine.encode = stub
    return out


def outcome(model, call):
    """"encoder" when the stub's exception came out, else {"exception": class name, "encoder_reached": bool}."""
    del model.reached[:]
    try:
        call()
    except EncoderReached:
        return "encoder"
    except Exception as e:                             # noqa: BLE001 -- the class is what is recorded
        return {"exception": type(e).__name__, "encoder_reached": bool(model.reached)}
    return {"exception": None, "encoder_reached": bool(model.reached)}


def combinations(atoms):
    """No atom, every atom, every unordered pair of atoms that do not set the same keyword."""
    names = list(atoms)
    yield ()
    for a in names:
        yield (a,)
    for a, b in itertools.combinations(names, 2):
        if not set(atoms[a]) & set(atoms[b]):
            yield (a, b)


# ---- generate -------------------------------------------------------------------------------------------------------------------
def generate_atoms(model):
    return {"temperature=0.4": dict(temperature=0.4),
            "temperature=(0.0,0.4)+logprob_threshold": dict(temperature=(0.0, 0.4), logprob_threshold=-1.0),
            "condition_on_prev_tokens": dict(condition_on_prev_tokens=True),
            "num_beams=2": dict(num_beams=2),
            "assistant_model": dict(assistant_model=model),
            "assistant_per_row": dict(assistant_per_row=True),
            "return_token_timestamps": dict(return_token_timestamps=True),
            "repetition_penalty=1.2": dict(repetition_penalty=1.2),
            "no_repeat_ngram_size=3": dict(no_repeat_ngram_size=3),
            "sequence_bias": dict(sequence_bias={(50,): 1.0}),
            "bad_words_ids": dict(bad_words_ids=[[50]]),
            "use_cache=False": dict(use_cache=False),
            "output_scores": dict(output_scores=True),
            "output_scores+return_dict": dict(output_scores=True, return_dict_in_generate=True),
            "output_logits+return_dict": dict(output_logits=True, return_dict_in_generate=True),
            "decoder_input_ids": dict(decoder_input_ids=torch.tensor([[gd.SOT]] * 2)),
            FP8: dict(cross_kv_dtype="fp8"),
            "return_segments": dict(return_segments=True),
            "num_return_sequences=2": dict(num_return_sequences=2),
            "length_penalty=2.0": dict(length_penalty=2.0),
            "prompt_condition_type=all-segments": dict(prompt_condition_type="all-segments")}


def generate_contexts():
    """name -> (features of two utterances, keywords)."""
    short, long_ = gd.features(1, 2), torch.cat([gd.features(1, 2), gd.features(2, 2)[..., :1500]], -1)
    base = dict(language="en", max_new_tokens=4)
    return {"single": (short, dict(base)),
            "single_timestamps_unique_call": (short, dict(base, return_timestamps=True, force_unique_generate_call=True)),
            "seek": (short, dict(base, return_timestamps=True)),
            "seek_4500": (long_, dict(base, return_timestamps=True, attention_mask=torch.ones(2, 4500, dtype=torch.long))),
            "seek_slots=2": (short, dict(base, return_timestamps=True, seek_slots=2))}


def generate_outcomes(ms=None):
    ms = ms or models()
    out = {}
    for ctx, (feats, base) in generate_contexts().items():
        for combo in combinations(generate_atoms(None)):
            model = ms[384 if FP8 in combo else 128]
            atoms = generate_atoms(model)
            kw = dict(base)
            for a in combo:
                kw.update(atoms[a])
            out[" | ".join((ctx,) + combo)] = outcome(model, lambda: model.generate(feats, **kw))
    return out


# ---- seek_decode called directly ------------------------------------------------------------------------------------------------
def seek_atoms(model):
    from distil_whisper_amd.decoding import sequence_bias_table
    table = lambda sb, bw: sequence_bias_table(sb, bw, model.dims.vocab, gd.EOS)
    return {"temperatures=(0.4,)": dict(temperatures=(0.4,)),
            "temperatures=(0.0,0.4)+logprob_threshold": dict(temperatures=(0.0, 0.4), logprob_threshold=-1.0),
            "no_speech_threshold": dict(no_speech_threshold=0.6),
            "condition_on_prev_tokens": dict(condition_on_prev_tokens=True),
            "num_beams=2": dict(num_beams=2),
            "assistant": dict(assistant=(model.engine, None)),
            "token_timestamps": dict(token_timestamps=dict(alignment_heads=[[0, 0]], num_frames=None, time_precision=0.02)),
            "repetition_penalty=1.2": dict(repetition_penalty=1.2),
            "no_repeat_ngram_size=3": dict(no_repeat_ngram_size=3),
            "sequence_bias": dict(sequence_bias=table({(50,): 1.0}, None)),
            "bad_words_ids": dict(sequence_bias=table(None, [[50]])),
            FP8: dict(cross_kv_dtype="fp8"),
            "use_graphs": dict(use_graphs=False),
            "length_penalty=2.0": dict(length_penalty=2.0),
            "prompt_all_segments": dict(prompt_ids=[gd.STARTOFPREV, 41, 42], prompt_all_segments=True)}


def seek_outcomes(ms=None):
    ms = ms or models()
    init = [gd.SOT, gd.LANG["<|en|>"], gd.TRANSCRIBE]
    out = {}
    for B in (1, 2):
        feats = gd.features(1, B)
        args = (feats, [3000] * B, [init] * B, lambda P: (4, 0), gd.EOS, gd.EOS, gd.NOTIMESTAMPS, 50)
        for ctx, base in (("lockstep", {}), ("slots=2", dict(slots=2))):
            for combo in combinations(seek_atoms(ms[128])):
                model = ms[384 if FP8 in combo else 128]
                atoms = seek_atoms(model)
                kw = dict(base, suppress_tokens=gd.SUPPRESS)
                for a in combo:
                    kw.update(atoms[a])
                out[" | ".join((f"B={B}", ctx) + combo)] = outcome(model, lambda: model.seek_decode(*args, **kw))
    return out


# ---- the two schedules on the planted model ---------------------------------------------------------------------------------------
def schedule_logs(thresholds=None):
    """Per leg ("lockstep", "slots=2", "slots=3"), without and with the thresholds: the log of seek_slots_cases.Spy (encoder batches,
    `retrieve_segment` calls, window ends, teacher-forced passes), `last_seek_stats`, `last_window_scores` and the segments.
    thresholds: None derives them as tests/test_seek_slots.py does (the middle of the widest gaps of the lockstep numbers)."""
    import pytest
    from oracle.ref_ops import RefOps
    from tests import seek_slots_cases as ss
    from tests.test_seek_slots import seek_args, thresholds_from_lockstep
    ops = RefOps("cpu", lowp=torch.float32)
    out = {}
    with pytest.MonkeyPatch.context() as mp:
        model, enc = ss.planted_seek_model(ops, 3)
        feats, max_frames, _ = ss.utterances(2 * model.dims.max_src)
        B = feats.shape[0]
        args, kw = seek_args(feats, max_frames, [ss.INIT] * B), dict(suppress_tokens=gd.SUPPRESS)
        spy = ss.Spy(mp, model, enc)
        if thresholds is None:
            _, (lp_thr, _), (ns_thr, _) = thresholds_from_lockstep(model, args, kw)
            thresholds = dict(logprob_threshold=lp_thr, no_speech_threshold=ns_thr)
        out["thresholds"] = thresholds
        for name, th in (("plain", {}), ("thresholds", thresholds)):
            for leg, extra in (("lockstep", {}), ("slots=2", dict(slots=2, check_every=2)), ("slots=3", dict(slots=3, check_every=2))):
                spy.clear()
                model.__dict__.pop("last_seek_stats", None)
                segs = model.seek_decode(*args, **extra, **th, **kw)
                out[f"{name} | {leg}"] = dict(
                    log=[list(e) for e in spy.log], stats=getattr(model, "last_seek_stats", None),
                    window_scores=[list(s) for s in model.last_window_scores],
                    segments=[[[s["start"], s["end"], list(s["tokens"])] for s in row] for row in segs])
    return out
