"""TEST INFRASTRUCTURE -- generates tests/golden/history_processors.json: what the REFERENCE decodes with
`generate(repetition_penalty=..., no_repeat_ngram_size=...)` (`transformers.WhisperForConditionalGeneration`;
RepetitionPenaltyLogitsProcessor / NoRepeatNGramLogitsProcessor in front of Whisper's processors) on the seeded micro model of
oracle/gen_golden_decode.py (V = 1000), in fp32: single-window calls and one run of the timestamp seek loop.

A seed is only kept when
  * the reference's output DIFFERS from the same call without the two options (otherwise the scenario tests nothing),
  * single window: the output is `diverse` and the smallest top-two / mass-rule margin of the processed scores is at least
    MIN_MARGIN standard deviations of the logits (oracle.gen_golden_decode.hf_generate; the best such seed is taken),
  * the drop-in over the torch restatement of the kernels (oracle/ref_ops.py, the eager selection path) decodes the reference's
    tokens in fp32, in bf16, and in fp32 under four draws of uniform logit noise of +-NOISE / 2 standard deviations (the rule of
    oracle.gen_golden_decode.scenario_seek: the bf16 kernels move a logit by at most 0.025-0.04 sigma on these weights),
  * seek loop: every row takes at least two passes and the rows differ.

Run in the build container (needs `transformers`):  python tools/gen_golden_history_processors.py
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden_decode as gd  # noqa: E402
from oracle.gen_golden_decode import best_seed, diverse, features, generation_fields, hf_generate, weights  # noqa: E402

NOISE = 0.06
OUT = os.path.join(ROOT, "tests", "golden", "history_processors.json")
SEEDS = tuple(range(10, 310))

SCENARIOS = [
    dict(name="repetition_penalty", kind="short", B=2, ts_fields=False,
         kwargs=dict(language="en", max_new_tokens=7, repetition_penalty=1.6)),
    dict(name="no_repeat_2gram", kind="short", B=2, ts_fields=False,
         kwargs=dict(language="en", max_new_tokens=8, no_repeat_ngram_size=2)),
    dict(name="no_repeat_1gram", kind="short", B=2, ts_fields=False,
         kwargs=dict(language="en", max_new_tokens=7, no_repeat_ngram_size=1)),
    dict(name="both", kind="short", B=2, ts_fields=False,
         kwargs=dict(language="de", max_new_tokens=7, repetition_penalty=1.3, no_repeat_ngram_size=3)),
    # the timestamp rules in one window: timestamp tokens of the history are penalised in front of the mass rule
    dict(name="timestamps_one_window", kind="short", B=2, ts_fields=True,
         kwargs=dict(language="en", max_new_tokens=8, return_timestamps=True, force_unique_generate_call=True,
                     repetition_penalty=1.4, no_repeat_ngram_size=2)),
    # the reference's seek loop hands its generation config to GenerationMixin.generate for every window
    dict(name="seek_loop", kind="seek", B=2, ts_fields=True, frames=450,
         kwargs=dict(language="en", max_new_tokens=6, return_timestamps=True, repetition_penalty=1.5, no_repeat_ngram_size=2)),
]
OPTIONS = ("repetition_penalty", "no_repeat_ngram_size")


def without_options(kw):
    return {k: v for k, v in kw.items() if k not in OPTIONS}


def ours(sc, seed, lowp, sigma_noise=0.0, draw=0):
    """the scenario on this package over the torch restatement of the kernels (the eager selection path)"""
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration as Ours
    from oracle.ref_ops import RefOps
    m = Ours(gd.CFG_T, ops=RefOps("cpu", lowp=lowp), state_dict=weights(seed))
    m.generation_config = GenerationConfig.from_any(generation_fields(True, True, sc["ts_fields"]))
    if sigma_noise:
        g = torch.Generator().manual_seed(3000 + draw)
        eng = m.engine

        def noisy(fn):
            def f(ids, cache):
                lg = fn(ids, cache).float()
                return lg + (torch.rand(lg.shape, generator=g) - 0.5) * sigma_noise
            return f
        eng.decode_step, eng.decode_multi = noisy(eng.decode_step), noisy(eng.decode_multi)
    f = inputs(sc, seed)
    if sc["kind"] == "seek":
        return m.generate(f, **sc["kwargs"]).tolist()
    return m.generate(f, return_dict_in_generate=True, **sc["kwargs"]).sequences.tolist()


def inputs(sc, seed):
    f = features(seed + 1, sc["B"])
    return f[..., :sc["frames"]].contiguous() if sc.get("frames") else f


def robust(sc, seed, want, sigma):
    if ours(sc, seed, torch.float32) != want or ours(sc, seed, torch.bfloat16) != want:
        return False
    return all(ours(sc, seed, torch.float32, NOISE * sigma, k) == want for k in range(4))


def short(sc):
    fields = generation_fields(True, True, sc["ts_fields"])
    kept = {}

    def run(seed, final):
        sd = weights(seed)
        seq, _, margin = hf_generate(gd.CFG_T, sd, fields, inputs(sc, seed), **sc["kwargs"])
        rows = seq.tolist()
        base, _, _ = hf_generate(gd.CFG_T, sd, fields, inputs(sc, seed), **without_options(sc["kwargs"]))
        P = hf_generate.prompt_len
        why = "ok"
        if not diverse(rows, P):
            why = "degenerate"
        elif rows == base.tolist():
            why = "the options change nothing"
        elif margin < gd.MIN_MARGIN:
            why = "margin"
        ok = why == "ok"
        if ok:
            with torch.no_grad():
                lg = gd.hf_model(gd.CFG_T, sd, **fields)(input_features=inputs(sc, seed),
                                                         decoder_input_ids=seq[:, :-1]).logits
            ok = robust(sc, seed, rows, lg.float().std().item())
            why = "ok" if ok else "tokens change under bf16 / logit noise"
        kept[seed] = dict(sequences=rows, baseline=base.tolist(), P=P)
        print(f"{sc['name']:22s} seed {seed:3d}: margin {margin:.3f} {why}", flush=True)
        return {"diverse": ok}, margin
    seed, _, margin = best_seed(run, SEEDS)
    return dict(sc, seed=seed, margin=margin, **kept[seed])


def seek(sc):
    fields = generation_fields(True, True, True)
    for seed in SEEDS:
        sd, f = weights(seed), inputs(sc, seed)
        with torch.no_grad():
            out = gd.hf_model(gd.CFG_T, sd, **fields).generate(f, return_dict_in_generate=True, output_logits=True,
                                                               **sc["kwargs"])
            base = gd.hf_model(gd.CFG_T, sd, **fields).generate(f, **without_options(sc["kwargs"])).tolist()
        plain = out["sequences"].tolist()
        passes = [len(sg) for sg in out["segments"]]
        why = "ok"
        if min(passes) < 2 or plain[0] == plain[1]:
            why = f"passes {passes}"
        elif plain == base:
            why = "the options change nothing"
        else:
            sigma = torch.stack(out["segments"][0][0]["result"]["logits"], 1).float().std().item()
            if not robust(sc, seed, plain, sigma):
                why = "tokens change under bf16 / logit noise"
        print(f"{sc['name']:22s} seed {seed:3d}: {why}", flush=True)
        if why == "ok":
            segments = [[dict(start=float(sg["start"]), end=float(sg["end"]), tokens=sg["tokens"].tolist()) for sg in row]
                        for row in out["segments"]]
            return dict(sc, seed=seed, margin=NOISE, sequences=plain, baseline=base, segments=segments, passes=passes)
    raise SystemExit("seek loop: no seed survived: widen the seed search")


def one(sc):
    torch.set_num_threads(2)
    return seek(sc) if sc["kind"] == "seek" else short(sc)


def main():
    import multiprocessing as mp
    with mp.get_context("fork").Pool(len(SCENARIOS)) as pool:          # (the scenarios are independent seed searches)
        scenarios = pool.map(one, SCENARIOS)
    meta = dict(vocab=gd.V, min_margin=gd.MIN_MARGIN, noise=NOISE,
                note="made by tools/gen_golden_history_processors.py from transformers " + __import__("transformers").__version__)
    with open(OUT, "w") as f:
        json.dump(dict(meta=meta, scenarios=scenarios), f, indent=1)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
