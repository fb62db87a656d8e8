"""TEST INFRASTRUCTURE -- generates tests/golden/token_timestamps.json: what the REFERENCE returns for
`generate(..., return_token_timestamps=True)` (`transformers.WhisperForConditionalGeneration`, TF:generation_whisper.py:241-381)
on the seeded micro model of oracle/gen_golden_decode.py, per scenario in fp32 and in bf16.

Token timestamps follow the alignment heads' cross-attention, and on random weights that is nearly flat: the per-column
normalisation divides by a tiny spread and the DTW path follows rounding noise.  A scenario is therefore only kept when
  * the reference decodes the same tokens in bf16 as in fp32,
  * at most MAX_BF16_SHARE of the generated tokens' bf16 timestamps lie more than one frame (0.02 s) from the fp32 ones
    (`ref_bf16_share`: the allowance tests/test_token_timestamps_gpu.py derives its bound from),
  * the fp32 timestamps do not change under three draws of relative 1e-4 noise on the attention probabilities
    (`stable_under_1e-4`: about a hundred times what a different fp32 summation order moves them by -- the CPU test compares
    two fp32 implementations bit for bit),
  * the matrix is not degenerate (no NaN, timestamps not all equal),
  * the tokens themselves survive bf16 on the MI355X path: as in oracle/gen_golden_decode.py (`scenario_seek`), the drop-in over
    the torch restatement of the kernels must decode the reference's tokens in bf16 and, in fp32, under four draws of uniform
    logit noise of +-TOKEN_NOISE / 2 standard deviations of the logits (`token_margin`; the bf16 kernels move a logit by at most
    0.025-0.04 sigma on these weights).
Each scenario walks its seed list until one passes; a scenario without a passing seed stops the script.

Run in the build container (needs `transformers`):  python tools/gen_golden_token_timestamps.py
"""
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden_decode as gd  # noqa: E402

ALIGNMENT_HEADS = [[0, 1], [1, 0], [1, 1]]
MAX_BF16_SHARE = 0.05
TOKEN_NOISE = 0.06
FRAME = 0.02
OUT = os.path.join(ROOT, "tests", "golden", "token_timestamps.json")

SCENARIOS = [
    # name, kind, seeds, batch, timestamps fields, kwargs, extras
    dict(name="plain", kind="single", seeds=(12, 13, 14, 16, 18, 19, 20, 21) + tuple(range(22, 120)), B=2, ts_fields=False,
         kwargs=dict(language="en", max_new_tokens=24)),
    dict(name="attention_mask", kind="single", seeds=(13, 12, 14, 16, 18, 19, 20, 21) + tuple(range(22, 120)), B=2, ts_fields=False,
         kwargs=dict(language="en", max_new_tokens=24), mask_frames=(3000, 2200)),
    dict(name="prompt_ids", kind="single", seeds=(14, 12, 13, 16, 18, 19, 20, 21) + tuple(range(22, 120)), B=2, ts_fields=False,
         kwargs=dict(language="en", max_new_tokens=24, prompt_ids=[gd.STARTOFPREV, 50, 60, 70])),
    dict(name="return_timestamps", kind="single", seeds=(16, 12, 13, 14, 18, 19, 20, 21) + tuple(range(22, 120)), B=2, ts_fields=True,
         kwargs=dict(language="en", max_new_tokens=24, return_timestamps=True, force_unique_generate_call=True)),
    dict(name="ragged_finish", kind="single", seeds=(12, 13, 14, 16, 18, 19, 20, 21) + tuple(range(22, 120)), B=3, ts_fields=False,
         kwargs=dict(language="en", max_new_tokens=24), pick_eos=True),
    # 45 s of input, some 38 windows of 20 tokens, ~190 of them kept: the case the feature was specified with.  The token-noise rule
    # is NOT applied to it (token_rule=False): every candidate costs six drop-in runs of ~38 windows, and the chance that hundreds
    # of greedy decisions all clear the noise band falls geometrically with their number (oracle/gen_golden_decode.py keeps its
    # own seek-loop scenarios short for that reason), so no seed search was made.  What is known instead of a margin: the reference
    # in bf16 and the drop-in's bf16 restatement decode the fixture's tokens, and so does the MI355X path -- asserted by
    # tests/test_token_timestamps_gpu.py, recorded in profiles/token_timestamps_bench.json.  `seek_short` below is the seek-loop
    # scenario with the rule on.
    dict(name="longform_segments", kind="seek", seeds=(14, 12, 13, 16), B=1, ts_fields=True, frames=4500, token_rule=False,
         kwargs=dict(language="en", max_new_tokens=20, return_timestamps=True, return_segments=True), mask_frames=(4500,)),
    # the seek loop with every rule on: an input longer than 30 s whose windows end after a few tokens
    dict(name="seek_short", kind="seek", seeds=tuple(range(10, 200)), B=1, ts_fields=True, frames=3600,
         kwargs=dict(language="en", max_new_tokens=6, return_timestamps=True, return_segments=True), mask_frames=(3600,),
         min_segments=2),
]


def fields_of(sc):
    f = gd.generation_fields(multilingual=True, suppress=True, timestamps=sc["ts_fields"])
    f["alignment_heads"] = [list(x) for x in ALIGNMENT_HEADS]
    return f


def inputs_of(sc, seed):
    B = sc["B"]
    if sc.get("frames"):
        n = -(-sc["frames"] // 3000)
        f = torch.cat([gd.features(seed + 1 + i, B) for i in range(n)], -1)[..., :sc["frames"]].contiguous()
    else:
        f = gd.features(seed + 1, B)
    mask = None
    if sc.get("mask_frames"):
        mask = torch.zeros(B, f.shape[-1], dtype=torch.long)
        for b, n in enumerate(sc["mask_frames"]):
            mask[b, :n] = 1
    return f, mask


def call_kwargs(sc, extra=None):
    kw = dict(sc["kwargs"])
    kw.update(extra or {})
    if "prompt_ids" in kw:
        kw["prompt_ids"] = torch.tensor(kw["prompt_ids"])
    return kw


def reference(sc, seed, dtype, extra=None, noise=None):
    """One reference call on a fresh model.  noise = (relative sigma, draw): the probabilities the reference's
    `_extract_token_timestamps` sees are multiplied by 1 + sigma * N(0, 1)."""
    m = gd.hf_model(gd.CFG_T, gd.weights(seed), **fields_of(sc)).to(dtype)
    f, mask = inputs_of(sc, seed)
    nan_seen = []
    orig = m._extract_token_timestamps

    def wrapped(generate_outputs, alignment_heads, **kw):
        ca = generate_outputs.cross_attentions
        nan_seen.append(any(bool(torch.isnan(w).any()) for step in ca for w in step))
        if noise is not None:
            g = torch.Generator().manual_seed(1000 * noise[1] + len(nan_seen))
            generate_outputs["cross_attentions"] = tuple(
                tuple(w * (1.0 + noise[0] * torch.randn(w.shape, generator=g).to(w.dtype)) for w in step) for step in ca)
        ts = orig(generate_outputs, alignment_heads, **kw)
        nan_seen[-1] = nan_seen[-1] or bool(torch.isnan(ts).any())
        return ts
    m._extract_token_timestamps = wrapped
    with torch.no_grad():
        out = m.generate(f.to(dtype), attention_mask=mask, return_token_timestamps=True, **call_kwargs(sc, extra))
    res = dict(sequences=out["sequences"].tolist(), token_timestamps=out["token_timestamps"].float().tolist(),
               nan=any(nan_seen))
    if "segments" in out:
        res["segments"] = [[dict(start=float(s["start"]), end=float(s["end"]), tokens=s["tokens"].tolist(),
                                 token_timestamps=s["token_timestamps"].double().tolist()) for s in row]
                           for row in out["segments"]]
    return res


def pick_eos(sc, seed):
    """A text token that ends the rows of the batch at different lengths when it is the EOS."""
    base = reference(sc, seed, torch.float32)["sequences"]
    first = {}
    for b, row in enumerate(base):
        for i, t in enumerate(row):
            first.setdefault(t, {}).setdefault(b, i)
    best = None
    for t, rows in first.items():
        if t >= gd.EOS:
            continue
        ends = sorted(rows.get(b, 10 ** 6) for b in range(len(base)))
        if 4 <= ends[0] and ends[0] + 3 <= ends[1]:
            if best is None or ends[0] > best[1]:
                best = (t, ends[0])
    return None if best is None else best[0]


def dropin_tokens(sc, seed, extra, lowp, noise_draw=None):
    """The tokens `generate` of this package decodes over the torch restatement of the kernels (no token timestamps: the token
    loop alone); noise_draw: uniform noise of +-TOKEN_NOISE / 2 sigma on every logit."""
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration as Ours
    from oracle.ref_ops import RefOps
    m = Ours(gd.CFG_T, ops=RefOps("cpu", lowp=lowp), state_dict=gd.weights(seed))
    m.generation_config = GenerationConfig.from_any(fields_of(sc))
    if noise_draw is not None:
        g = torch.Generator().manual_seed(3000 + noise_draw)
        eng = m.engine

        def noisy(fn):
            def f(ids, cache):
                lg = fn(ids, cache).float()
                sigma = lg[..., :gd.V].std().item()
                return lg + (torch.rand(lg.shape, generator=g) - 0.5) * TOKEN_NOISE * sigma
            return f
        eng.decode_step, eng.decode_multi = noisy(eng.decode_step), noisy(eng.decode_multi)
    f, mask = inputs_of(sc, seed)
    out = m.generate(f, attention_mask=mask, **call_kwargs(sc, extra))
    return (out["sequences"] if isinstance(out, dict) else out).tolist()


def share(a, b):
    x, y = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float((np.abs(x - y) > FRAME * 1.0001).mean()) if x.size else 0.0


def try_seed(sc, seed):
    extra = {}
    if sc.get("pick_eos"):
        t = pick_eos(sc, seed)
        if t is None:
            return None, "no token ends the rows at different lengths"
        extra["eos_token_id"] = t
    r32 = reference(sc, seed, torch.float32, extra)
    if r32["nan"]:
        return None, "degenerate (NaN)"
    flat = [t for row in r32["token_timestamps"] for t in row]
    if len(set(flat)) < 3:
        return None, "degenerate (timestamps all equal)"
    if sc.get("pick_eos") and len({len([t for t in row if t != gd.EOS]) for row in r32["sequences"]}) < 2:
        return None, "rows did not finish at different lengths"
    if sc.get("min_segments") and len(r32["segments"][0]) < sc["min_segments"]:
        return None, "too few segments"
    if dropin_tokens(sc, seed, extra, torch.float32) != r32["sequences"] or \
            dropin_tokens(sc, seed, extra, torch.bfloat16) != r32["sequences"]:
        return None, "the drop-in's restatement decodes other tokens in bf16"
    for draw in range(4 if sc.get("token_rule", True) else 0):
        if dropin_tokens(sc, seed, extra, torch.float32, draw) != r32["sequences"]:
            return None, f"tokens change under +-{TOKEN_NOISE / 2} sigma logit noise"
    r16 = reference(sc, seed, torch.bfloat16, extra)
    if r16["sequences"] != r32["sequences"]:
        return None, "bf16 reference decodes other tokens"
    sh = share(r32["token_timestamps"], r16["token_timestamps"])
    if sh > MAX_BF16_SHARE:
        return None, f"ref_bf16_share {sh:.3f}"
    for draw in range(3):
        rn = reference(sc, seed, torch.float32, extra, noise=(1e-4, draw))
        if rn["sequences"] != r32["sequences"] or rn["token_timestamps"] != r32["token_timestamps"]:
            return None, "not stable under 1e-4 noise"
    out = dict(name=sc["name"], kind=sc["kind"], seed=seed, B=sc["B"], ts_fields=sc["ts_fields"],
               kwargs=dict(sc["kwargs"], **extra), mask_frames=list(sc.get("mask_frames") or ()) or None,
               frames=sc.get("frames"), sequences=r32["sequences"], token_timestamps=r32["token_timestamps"],
               sequences_bf16=r16["sequences"], token_timestamps_bf16=r16["token_timestamps"], ref_bf16_share=sh,
               token_margin=TOKEN_NOISE if sc.get("token_rule", True) else None, **{"stable_under_1e-4": True})
    if "segments" in r32:
        out["segments"] = r32["segments"]
        out["segments_bf16_token_timestamps"] = [[s["token_timestamps"] for s in row] for row in r16["segments"]]
    return out, "ok"


def main(only=None):
    kept = []
    if only and os.path.exists(OUT):
        kept = [s for s in json.load(open(OUT))["scenarios"] if s["name"] not in only]
    for sc in SCENARIOS:
        if only and sc["name"] not in only:
            continue
        for seed in sc["seeds"]:
            got, why = try_seed(sc, seed)
            print(f"{sc['name']:20s} seed {seed:3d}: {why}", flush=True)
            if got is not None:
                kept.append(got)
                break
        else:
            raise SystemExit(f"{sc['name']}: no seed passes; widen its seed list")
    order = [s["name"] for s in SCENARIOS]
    kept.sort(key=lambda s: order.index(s["name"]))
    assert sum(s["kind"] == "single" for s in kept) >= 3
    meta = dict(alignment_heads=ALIGNMENT_HEADS, max_bf16_share=MAX_BF16_SHARE, frame=FRAME, median_filter_width=7,
                note="made by tools/gen_golden_token_timestamps.py from transformers " + __import__("transformers").__version__)
    with open(OUT, "w") as f:
        json.dump(dict(meta=meta, scenarios=kept), f)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main(only=set(sys.argv[1:]) or None)
