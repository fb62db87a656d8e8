"""Writes tests/golden/beam_thresholds.json: `generate(num_beams=k, logprob_threshold=, no_speech_threshold=,
compression_ratio_threshold=, temperature=(0.0,), return_segments=True)` through `transformers`' seek loop on the tiny model of
oracle.gen_golden_decode (weights and features from seeds), for tests/test_beam_step*.py.

WHICH reference.  `_need_fallback` (TF:generation_whisper.py:1261-1273) means to judge a beam-search window by its hypothesis'
`sequences_scores`, but tests `hasattr(seek_outputs[0], "sequences_scores")` on plain dicts: in the installed version the test is
false and the window is judged by `_retrieve_avg_logprobs` over the processed scores of expanded row `index` (another beam,
often another utterance).  This package implements the branch the reference's code states, so the scenarios run the reference
with that branch made reachable: the per-window outputs are wrapped in a dict whose keys are attributes, nothing else is touched.
One scenario per multilingual seed, kind "installed_differs", records in addition what the UNTOUCHED reference returns at a
threshold between the two quantities, where the two rules decide differently; tests pin that deviation.

Scenarios: 2 beams on a 45 s + 20 s batch and 3 beams on a 30 s batch, a multilingual and an English-only generation config.
With `temperature=(0.0,)` a failed log-probability threshold shows in the output only through the no-speech skip, so the
no-speech threshold sits below every observed probability where the log-probability decision is the subject:
  pass_all     logprob_threshold below every window's score;
  fail_some    logprob_threshold between two windows' scores (the windows below it are skipped);
  no_speech    logprob_threshold above every score, no_speech_threshold between two windows' probabilities;
  compression  compression_ratio_threshold between two windows' ratios (or 1.2), decisions recorded, nothing follows.
Every scenario records the reference's decisions per window (score, no-speech probability, compression ratio, needs_fallback,
should_skip) next to tokens and segments.
A seed is kept only if
  * this package's fp32 restatement (oracle.ref_ops) decodes the base scenario's tokens and, at every beam step, the top 2k + 1
    accumulated scores per utterance are at least MIN_MARGIN apart;
  * the reference with bf16 weights decodes the same tokens in the same windows; `bf16_dev_score` / `bf16_dev_no_speech` are its
    largest deviations from the fp32 run;
  * every threshold is at least four times that deviation away from every value it is compared with.
Also recorded: the first window's hypothesis score per utterance in float64 (a teacher-forced pass of the reference in double over
the window's sequence; the reference keeps its own beam scores in fp32 whatever the model's dtype) with `fp64_dev` = max |fp32 -
fp64|, and how many seeds were tried and rejected, with reasons.

    python tools/gen_golden_beam_thresholds.py          (needs transformers; CPU only, about a minute and a half)
"""
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from oracle import gen_golden_decode as gd          # noqa: E402
from oracle.ref_ops import RefOps                   # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "beam_thresholds.json")
MIN_MARGIN = 5e-4          # log-probability units: ~250 x the fp32 rounding of an accumulated score (ulp 1.9e-6 below 32)
MAX_NEW = 6


class _Out(dict):
    """A per-window output whose keys are attributes too, as `hasattr(seek_outputs[0], "sequences_scores")` expects."""
    def __getattr__(self, k):
        try:
            return self[k]
        except KeyError:
            raise AttributeError(k)


def inputs(seed, long):
    if not long:
        return gd.features(seed + 1, 2), {}
    a = torch.cat([gd.features(seed + 4, 1), gd.features(seed + 5, 1)[..., :1500]], -1)          # 45 s
    b = torch.cat([gd.features(seed + 6, 1)[..., :2000], torch.zeros(1, 80, 2500)], -1)          # 20 s, padded
    mask = torch.ones(2, 4500, dtype=torch.long)
    mask[1, 2000:] = 0
    return torch.cat([a, b], 0), dict(attention_mask=mask)


def reference(sd, fields, feats, kw, dtype=torch.float32, stated_branch=True):
    """-> (tokens, segments, decisions): one reference call; decisions = what `_need_fallback` saw and returned, in call order."""
    import transformers.models.whisper.generation_whisper as gw
    from transformers.generation.logits_process import WhisperNoSpeechDetection
    mixin = gw.WhisperGenerationMixin
    orig, orig_avg = mixin._need_fallback, mixin._retrieve_avg_logprobs
    decisions, avgs = [], []

    def need(self, seek_sequence, seek_outputs, index, logits_processor, generation_config, vocab_size, temperature):
        outs = [_Out(o) for o in seek_outputs] if stated_branch else seek_outputs
        fb, skip = orig(self, seek_sequence, outs, index, logits_processor, generation_config, vocab_size, temperature)
        nsp = None
        if generation_config.no_speech_threshold is not None:
            p = gw._get_attr_from_logit_processors(logits_processor, WhisperNoSpeechDetection, "no_speech_prob")
            nsp = float(p[index])
        decisions.append(dict(index=index, score=float(seek_outputs[index]["sequences_scores"]), no_speech_prob=nsp,
                              compression_ratio=float(self._retrieve_compression_ratio(seek_sequence, vocab_size)),
                              installed_avg_logprob=avgs.pop() if avgs else None, needs_fallback=bool(fb), should_skip=bool(skip)))
        return fb, skip

    def avg(*a, **k):
        v = orig_avg(*a, **k)
        avgs.append(float(v))
        return v
    mixin._need_fallback, mixin._retrieve_avg_logprobs = need, staticmethod(avg)
    try:
        m = gd.hf_model(gd.CFG_T, sd, **fields).to(dtype)
        with torch.no_grad():
            r = m.generate(feats.to(dtype), return_segments=True, **kw)
    finally:
        mixin._need_fallback, mixin._retrieve_avg_logprobs = orig, staticmethod(orig_avg)
    segs = [[dict(start=float(s["start"]), end=float(s["end"]), tokens=s["tokens"].tolist()) for s in row] for row in r["segments"]]
    first = [row[0]["result"]["sequences"].tolist() if row else None for row in r["segments"]]
    return dict(sequences=r["sequences"].tolist(), segments=segs, decisions=decisions, first_window=first)


def score_fp64(sd, fields, feats, seqs, P):
    m = gd.hf_model(gd.CFG_T, sd, **fields).double()
    out = []
    for u, seq in enumerate(seqs):
        ids = torch.tensor([seq])
        with torch.no_grad():
            lp = torch.log_softmax(m(input_features=feats[u:u + 1, :, :3000].double(), decoder_input_ids=ids[:, :-1]).logits[0], -1)
        n = len(seq) - P
        out.append(float(sum(lp[P - 1 + j, seq[P + j]] for j in range(n)) / n))
    return out


def ours_margin(sd, fields, feats, kw):
    """This package's fp32 restatement on the same call: (tokens, smallest gap among the top 2k + 1 accumulated scores of any step)."""
    from distil_whisper_amd import decoding
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    m = WhisperForConditionalGeneration(gd.CFG_T, ops=RefOps("cpu", lowp=torch.float32), state_dict=sd, dtype=torch.float32)
    m.generation_config = GenerationConfig.from_any(fields)
    real, gaps = decoding.beam_step_torch, []

    def spy(st, logits, cur, cfg):
        B, nb = st["run_scores"].shape
        lp = torch.log_softmax(logits.float(), -1)
        # the accumulated scores as the step masks them: recomputed through the step's own rules
        sc = lp.clone()
        if cur - cfg["P"] < cfg["min_new_tokens"]:
            sc[:, cfg["eos"]] = float("-inf")
        if cur == cfg["P"] and cfg["bsup"] is not None:
            sc = sc.masked_fill(cfg["bsup"][None, :], float("-inf"))
        if cfg["sup"] is not None:
            sc = sc.masked_fill(cfg["sup"][None, :], float("-inf"))
        tr = cfg["timestamp_rules"]
        if tr is not None:
            flat = st["running"][:, :, :cur].reshape(B * nb, cur)
            sc = decoding.apply_timestamp_rules(sc, flat, cur, tr["begin_index"], tr["no_timestamps_token_id"], cfg["eos"],
                                                tr.get("max_initial_timestamp_index"))
        acc = (sc.view(B, nb, -1) + st["run_scores"][:, :, None]).reshape(B, -1)
        top = torch.topk(acc, 2 * nb + 1)[0]
        gap = (top[:, :-1] - top[:, 1:])[top[:, :-1] > -1.0e8]
        gap = gap[torch.isfinite(gap)]
        if gap.numel():
            gaps.append(float(gap.min()))
        return real(st, logits, cur, cfg)
    decoding.beam_step_torch = spy
    try:
        out = m.generate(feats, return_segments=True, **kw)
    finally:
        decoding.beam_step_torch = real
    return out["sequences"].tolist(), min(gaps)


def mid_gap(values, need):
    """The midpoint of the widest gap between two sorted distinct values, if each side keeps `need`; else None."""
    v = sorted(set(values))
    gaps = [(b - a, (a + b) / 2) for a, b in zip(v, v[1:])]
    if not gaps:
        return None
    g, mid = max(gaps)
    return mid if g / 2 >= need else None


def try_seed(seed, multilingual, nb, long):
    fields = gd.generation_fields(multilingual=multilingual, suppress=True, timestamps=True)
    sd = gd.weights(seed)
    feats, extra = inputs(seed, long)
    base = dict(max_new_tokens=MAX_NEW, return_timestamps=True, num_beams=nb, temperature=(0.0,), **extra)
    if multilingual:
        base["language"] = "en"
    probe = dict(base, logprob_threshold=-100.0, no_speech_threshold=2.0)       # nothing fails, nothing is skipped
    r32 = reference(sd, fields, feats, probe)
    mine, margin = ours_margin(sd, fields, feats, probe)
    if mine != r32["sequences"]:
        return None, "the fp32 restatement decodes other tokens"
    if margin < MIN_MARGIN:
        return None, f"beam-step margin {margin:.2e}"
    r16 = reference(sd, fields, feats, probe, dtype=torch.bfloat16)
    if r16["sequences"] != r32["sequences"] or len(r16["decisions"]) != len(r32["decisions"]):
        return None, "the bf16 reference decodes other tokens"
    S = [d["score"] for d in r32["decisions"]]
    N = [d["no_speech_prob"] for d in r32["decisions"]]
    C = [d["compression_ratio"] for d in r32["decisions"]]
    dev_s = max(abs(a["score"] - b["score"]) for a, b in zip(r16["decisions"], r32["decisions"]))
    dev_n = max(abs(a["no_speech_prob"] - b["no_speech_prob"]) for a, b in zip(r16["decisions"], r32["decisions"]))
    P = len(r32["first_window"][0]) - MAX_NEW
    s64 = score_fp64(sd, fields, feats, r32["first_window"], P)
    first_scores = [next(d["score"] for d in r32["decisions"] if d["index"] == u) for u in range(2)]   # (the first pass holds both)
    thr_mid = mid_gap(S, 4 * dev_s)
    if thr_mid is None:
        return None, "no gap between window scores wide enough for a threshold"
    lo_nsp = min(N) / 2 if min(N) > 0 else None
    if multilingual and (lo_nsp is None or min(N) - lo_nsp < 4 * dev_n):
        return None, "no room below the no-speech probabilities"
    nsp_kw = dict(no_speech_threshold=lo_nsp) if lo_nsp is not None else {}
    cases = [("pass_all", dict(logprob_threshold=min(S) - max(0.5, 8 * dev_s), **nsp_kw)),
             ("fail_some", dict(logprob_threshold=thr_mid, **nsp_kw)),
             ("compression", dict(logprob_threshold=min(S) - max(0.5, 8 * dev_s), compression_ratio_threshold=mid_gap(C, 1e-6) or 1.2))]
    if multilingual:
        nst_mid = mid_gap(N, 4 * dev_n)
        if nst_mid is None:
            return None, "no gap between no-speech probabilities wide enough for a threshold"
        cases.append(("no_speech", dict(logprob_threshold=max(S) + max(0.5, 8 * dev_s), no_speech_threshold=nst_mid)))
    scen = []
    for kind, thr in cases:
        r = reference(sd, fields, feats, dict(base, **thr))
        scen.append(dict(kind=kind, thresholds=thr, sequences=r["sequences"], segments=r["segments"], decisions=r["decisions"]))
    kinds_seen = {s["kind"]: s for s in scen}
    fs = kinds_seen["fail_some"]["decisions"]
    if not (any(d["needs_fallback"] or d["should_skip"] for d in fs) and any(not (d["needs_fallback"] or d["should_skip"]) for d in fs)):
        return None, "fail_some does not show both outcomes"
    if multilingual:
        ns = kinds_seen["no_speech"]["decisions"]
        if not (any(d["should_skip"] for d in ns) and any(not d["should_skip"] for d in ns)):
            return None, "no_speech does not show both outcomes"
        # where the installed reference decides differently: a threshold between its own quantity and the hypothesis scores
        probe_i = reference(sd, fields, feats, dict(base, logprob_threshold=-100.0, no_speech_threshold=2.0), stated_branch=False)
        A = [d["installed_avg_logprob"] for d in probe_i["decisions"]]
        if all(a is not None for a in A) and min(A) - max(S) > 8 * dev_s:
            thr = dict(logprob_threshold=(min(A) + max(S)) / 2, no_speech_threshold=lo_nsp)
            stated = reference(sd, fields, feats, dict(base, **thr))
            installed = reference(sd, fields, feats, dict(base, **thr), stated_branch=False)
            scen.append(dict(kind="installed_differs", thresholds=thr, sequences=stated["sequences"], segments=stated["segments"],
                             decisions=stated["decisions"], installed_sequences=installed["sequences"],
                             installed_segments=installed["segments"], installed_decisions=installed["decisions"]))
    return dict(seed=seed, multilingual=multilingual, num_beams=nb, long=long, max_new_tokens=MAX_NEW, prompt_len=P,
                beam_step_margin=margin, bf16_dev_score=dev_s, bf16_dev_no_speech=dev_n, window_scores=S, no_speech_probs=N,
                first_window_sequences=r32["first_window"], first_window_scores_fp32=first_scores, first_window_scores_fp64=s64,
                fp64_dev=max(abs(a - b) for a, b in zip(first_scores, s64)),
                scenarios=scen), None


def main():
    groups, tried, rejected = [], 0, []
    for multilingual in (True, False):
        for nb, long in ((2, True), (3, False)):
            for seed in range(300, 360):
                tried += 1
                g, why = try_seed(seed, multilingual, nb, long)
                if g is None:
                    rejected.append(dict(seed=seed, multilingual=multilingual, num_beams=nb, reason=why))
                    continue
                groups.append(g)
                break
            else:
                raise SystemExit(f"no seed for multilingual={multilingual} num_beams={nb}")
    meta = dict(min_margin=MIN_MARGIN, seeds_tried=tried, seeds_rejected=len(rejected), rejected=rejected,
                note="made by tools/gen_golden_beam_thresholds.py from transformers' seek loop (fp32, CPU) with the "
                     "`sequences_scores` branch of `_need_fallback` made reachable; `installed_*`: the untouched reference")
    with open(OUT, "w") as f:
        json.dump(dict(meta=meta, groups=groups), f)
    print("wrote", OUT, "tried", tried, "rejected", len(rejected))
    for r in rejected:
        print("  rejected", r)
    for g in groups:
        print(g["seed"], g["multilingual"], g["num_beams"], "margin %.2e bf16 dev %.2e / %.2e fp64 dev %s" % (
            g["beam_step_margin"], g["bf16_dev_score"], g["bf16_dev_no_speech"], g["fp64_dev"]), [s["kind"] for s in g["scenarios"]])


if __name__ == "__main__":
    main()
