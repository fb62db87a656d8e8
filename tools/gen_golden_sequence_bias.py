"""TEST INFRASTRUCTURE -- generates tests/golden/sequence_bias.json: what the REFERENCE decodes with
`generate(sequence_bias=..., bad_words_ids=...)` (`transformers.WhisperForConditionalGeneration`; SequenceBiasLogitsProcessor in
front of the repetition rules, NoBadWordsLogitsProcessor behind them, then Whisper's processors) on the seeded micro model of
oracle/gen_golden_decode.py (V = 1000), in fp32: single-window calls and one run of the timestamp seek loop.

The table of a scenario is made from the reference's own UNBIASED output of the seed (`TABLES` below: which of its tokens are
boosted, forbidden or used as a prefix; a seed tries a few candidates in a fixed order), so that a multi-token sequence really meets its prefix; the biases are multiples of the
standard deviation of the seed's logits, rounded to 0.25.  The fixture records the table that was used.

A seed is only kept when (the rules of tools/gen_golden_history_processors.py)
  * the reference's output DIFFERS from the same call without the two arguments,
  * single window: the output is `diverse` and the smallest top-two / mass-rule margin of the processed scores is at least
    MIN_MARGIN standard deviations of the logits (oracle.gen_golden_decode.hf_generate; the best such seed is taken),
  * the drop-in over the torch restatement of the kernels (oracle/ref_ops.py, the eager selection path) decodes the reference's
    tokens in fp32, in bf16, and in fp32 under four draws of uniform logit noise of +-NOISE / 2 standard deviations,
  * seek loop: every row takes at least two passes and the rows differ.
`tried` / `rejected` say how many seeds a scenario looked at and why the others were dropped.

Run in the build container (needs `transformers`):  python tools/gen_golden_sequence_bias.py [scenario ...]
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
OUT = os.path.join(ROOT, "tests", "golden", "sequence_bias.json")
SEEDS = tuple(range(10, 70))
OPTIONS = ("sequence_bias", "bad_words_ids")


def q(x):
    """a bias as a multiple of 0.25 (a float, as the reference's validation asks)"""
    return float(round(x * 4) / 4) or 0.25


# ---- candidate tables of a scenario from the unbiased output: gen = the generated tokens per row, s = the std of the logits.
# A seed tries them in this order and keeps the first that passes every rule above (at most MAX_TABLES of them). ----
MAX_TABLES = 9


def text(t):
    return 0 < t < gd.EOS


def texts(row):
    return list(dict.fromkeys(t for t in row if text(t)))


def t_one_token(gen, s):
    """a text token that only ONE row of the unbiased output holds, the rarest first: boosting the token both rows repeat anyway
    only repeats it more, in both rows alike"""
    both = gen[0] + gen[1]
    own = [t for t in texts(both) if (t in gen[0]) != (t in gen[1])]
    for a in sorted(own, key=both.count)[:3]:
        for scale in (1.0, 0.5, 1.5):
            yield dict(sequence_bias=[[[a], q(scale * s)]])


def t_multi_token(gen, s):
    """the reference's own output holds the prefix gen[0][i:i + 2]; the boosted continuation is another token of the batch"""
    for i in range(len(gen[0]) - 3):
        pre = gen[0][i:i + 2]
        for x in texts(gen[1] + gen[0]):
            if all(text(t) for t in pre) and x != gen[0][i + 2]:
                yield dict(sequence_bias=[[pre + [x], q(6 * s)]])
                break


def t_two_on_one_column(gen, s):
    """a one-token entry and two two-token entries on the column x (one prefix from each row's own output): the reference sums
    what counts for a row"""
    for i in range(len(gen[0]) - 2):
        a, b = gen[0][i], gen[1][i]
        for x in texts(gen[1] + gen[0]):
            if text(a) and text(b) and x != gen[0][i + 1]:
                yield dict(sequence_bias=[[[a, x], q(4 * s)], [[x], q(1 * s)], [[b, x], q(-0.5 * s)]])
                break


def t_bad_words(gen, s):
    for i in range(1, 4):
        a, b, c = gen[0][i], gen[1][i], gen[1][i + 1]
        if all(text(t) for t in (a, b, c)):
            yield dict(bad_words_ids=[[a], [b, c], [gd.EOS]])         # ([eos] alone is dropped by the reference)


def t_everything(gen, s):
    for i in range(1, 4):
        a, b, c, x = gen[0][i], gen[1][i], gen[1][i + 1], gen[0][i + 2]
        if all(text(t) for t in (a, b, c, x)):
            yield dict(sequence_bias=[[[x], q(1.5 * s)], [[b, x], q(2 * s)]], bad_words_ids=[[a], [b, c]])


def t_timestamps(gen, s):
    """one biased timestamp token (a later one than the row's first) and one biased text token"""
    ts = [t for t in gen[0] if t >= gd.TS0]
    for tx in texts(gen[0] + gen[1])[::-1][:3]:
        if ts and ts[0] + 7 < gd.V:
            yield dict(sequence_bias=[[[ts[0] + 7], q(4 * s)], [[tx], q(3 * s)]])


def t_seek(gen, s):
    """the windows of the micro model hold one or two text tokens: the first one of row 0 is forbidden, a timestamp is boosted"""
    ts = [t for t in gen[0] if t >= gd.TS0]
    for a in texts(gen[0])[:2]:
        for scale in (2.0, 1.0):
            if ts and ts[0] + 3 < gd.V:
                yield dict(sequence_bias=[[[ts[0] + 3], q(scale * s)]], bad_words_ids=[[a]])


def candidates(name, gen, s):
    """the first MAX_TABLES tables of scenario `name` (a row that ended early simply has fewer)"""
    out = []
    try:
        for table in TABLES[name](gen, s):
            out.append(table)
    except IndexError:
        pass
    return out[:MAX_TABLES]


TABLES = dict(one_token_boost=t_one_token, multi_token_boost=t_multi_token, two_on_one_column=t_two_on_one_column,
              bad_words=t_bad_words, with_repetition_rules=t_everything, timestamps_one_window=t_timestamps, seek_loop=t_seek)

SCENARIOS = [
    dict(name="one_token_boost", kind="short", B=2, ts_fields=False, kwargs=dict(language="en", max_new_tokens=8),
         seeds=[10, 250]),                             # (few seeds give two rows that differ and stay different under one boost)
    dict(name="multi_token_boost", kind="short", B=2, ts_fields=False, kwargs=dict(language="en", max_new_tokens=8)),
    dict(name="two_on_one_column", kind="short", B=2, ts_fields=False, kwargs=dict(language="de", max_new_tokens=8)),
    dict(name="bad_words", kind="short", B=2, ts_fields=False, kwargs=dict(language="en", max_new_tokens=8)),
    dict(name="with_repetition_rules", kind="short", B=2, ts_fields=False,
         kwargs=dict(language="en", max_new_tokens=8, repetition_penalty=1.3, no_repeat_ngram_size=2)),
    dict(name="timestamps_one_window", kind="short", B=2, ts_fields=True,
         kwargs=dict(language="en", max_new_tokens=8, return_timestamps=True, force_unique_generate_call=True)),
    dict(name="seek_loop", kind="seek", B=2, ts_fields=True, frames=450,
         kwargs=dict(language="en", max_new_tokens=6, return_timestamps=True)),
]


def ours(sc, seed, lowp, kwargs, sigma_noise=0.0, draw=0):
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
        return m.generate(f, **kwargs).tolist()
    return m.generate(f, return_dict_in_generate=True, **kwargs).sequences.tolist()


def inputs(sc, seed):
    f = features(seed + 1, sc["B"])
    return f[..., :sc["frames"]].contiguous() if sc.get("frames") else f


def robust(sc, seed, kwargs, want, sigma):
    if ours(sc, seed, torch.float32, kwargs) != want or ours(sc, seed, torch.bfloat16, kwargs) != want:
        return False
    return all(ours(sc, seed, torch.float32, kwargs, NOISE * sigma, k) == want for k in range(4))


def sigma_of(sd, fields, f, seq):
    with torch.no_grad():
        lg = gd.hf_model(gd.CFG_T, sd, **fields)(input_features=f, decoder_input_ids=seq[:, :-1]).logits
    return lg.float().std().item()


def short(sc):
    fields = generation_fields(True, True, sc["ts_fields"])
    kept, rejected = {}, {}

    def run(seed, final):
        sd, f = weights(seed), inputs(sc, seed)
        base, _, _ = hf_generate(gd.CFG_T, sd, fields, f, **sc["kwargs"])
        P = hf_generate.prompt_len
        tables = candidates(sc["name"], [row[P:] for row in base.tolist()], sigma_of(sd, fields, f, base))
        why, margin, ok = "no table from the unbiased output", 0.0, False
        for table in tables:
            kwargs = dict(sc["kwargs"], **table)
            seq, _, margin = hf_generate(gd.CFG_T, sd, fields, f, **kwargs)
            rows = seq.tolist()
            why = "ok"
            if not diverse(rows, P):
                why = "degenerate"
            elif rows == base.tolist():
                why = "the arguments change nothing"
            elif margin < gd.MIN_MARGIN:
                why = "margin"
            elif not robust(sc, seed, kwargs, rows, sigma_of(sd, fields, f, seq)):
                why = "tokens change under bf16 / logit noise"
            ok = why == "ok"
            if ok:
                kept[seed] = dict(kwargs=kwargs, sequences=rows, baseline=base.tolist(), P=P)
                break
        if not final and not ok:
            rejected[why] = rejected.get(why, 0) + 1
        print(f"{sc['name']:22s} seed {seed:3d}: margin {margin:.3f} {why}", flush=True)
        return {"diverse": ok}, margin
    seeds = range(*sc["seeds"]) if sc.get("seeds") else SEEDS
    seed, _, margin = best_seed(run, seeds)
    return dict(sc, seed=seed, margin=margin, tried=len(seeds), rejected=rejected, **kept[seed])


def seek(sc):
    fields = generation_fields(True, True, True)
    rejected = {}
    for tried, seed in enumerate(SEEDS, 1):
        sd, f = weights(seed), inputs(sc, seed)
        with torch.no_grad():
            base_out = gd.hf_model(gd.CFG_T, sd, **fields).generate(f, return_dict_in_generate=True, output_logits=True,
                                                                    **sc["kwargs"])
        base = base_out["sequences"].tolist()
        sigma = torch.stack(base_out["segments"][0][0]["result"]["logits"], 1).float().std().item()
        why = "no table from the unbiased output"
        for table in candidates(sc["name"], base, sigma):
            kwargs = dict(sc["kwargs"], **table)
            with torch.no_grad():
                out = gd.hf_model(gd.CFG_T, sd, **fields).generate(f, return_dict_in_generate=True, output_logits=True, **kwargs)
            plain = out["sequences"].tolist()
            passes = [len(sg) for sg in out["segments"]]
            why = "ok"
            if min(passes) < 2 or plain[0] == plain[1]:
                why = f"passes {passes}"
            elif plain == base:
                why = "the arguments change nothing"
            elif not robust(sc, seed, kwargs, plain, sigma):
                why = "tokens change under bf16 / logit noise"
            if why == "ok":
                break
        print(f"{sc['name']:22s} seed {seed:3d}: {why}", flush=True)
        if why == "ok":
            segments = [[dict(start=float(sg["start"]), end=float(sg["end"]), tokens=sg["tokens"].tolist()) for sg in row]
                        for row in out["segments"]]
            return dict(sc, kwargs=kwargs, seed=seed, margin=NOISE, tried=tried, rejected=rejected, sequences=plain,
                        baseline=base, segments=segments, passes=passes)
        key = "passes" if why.startswith("passes") else why
        rejected[key] = rejected.get(key, 0) + 1
    raise SystemExit("seek loop: no seed survived: widen the seed search")


def one(sc):
    torch.set_num_threads(1)
    try:
        return seek(sc) if sc["kind"] == "seek" else short(sc)
    except SystemExit as e:                                            # (the other scenarios' searches are kept)
        print(f"{sc['name']}: {e}", flush=True)
        return None


def main(only=()):
    """only: scenario names to search again; the others are kept from the fixture that exists"""
    import multiprocessing as mp
    todo = [sc for sc in SCENARIOS if not only or sc["name"] in only]
    with mp.get_context("fork").Pool(len(todo)) as pool:               # (the scenarios are independent seed searches)
        found = {sc["name"]: r for sc, r in zip(todo, pool.map(one, todo))}
    old = {}
    if only and os.path.exists(OUT):
        with open(OUT) as f:
            old = {sc["name"]: sc for sc in json.load(f)["scenarios"]}
    scenarios = [found.get(sc["name"]) or old.get(sc["name"]) for sc in SCENARIOS]
    missing = [sc["name"] for sc, r in zip(SCENARIOS, scenarios) if r is None]
    meta = dict(vocab=gd.V, min_margin=gd.MIN_MARGIN, noise=NOISE, seeds=[SEEDS[0], SEEDS[-1]],
                note="made by tools/gen_golden_sequence_bias.py from transformers " + __import__("transformers").__version__)
    with open(OUT, "w") as f:
        json.dump(dict(meta=meta, scenarios=[r for r in scenarios if r is not None]), f, indent=1)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")
    if missing:
        raise SystemExit(f"no seed survived for {missing}: widen the seed search")


if __name__ == "__main__":
    main(tuple(sys.argv[1:]))
