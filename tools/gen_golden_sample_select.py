"""Writes tests/golden/sample_select.json: single selection steps with sampling whose expected tokens come from `transformers`' own
processor and warper classes and `torch.multinomial` on the CPU -- RepetitionPenaltyLogitsProcessor, NoRepeatNGramLogitsProcessor,
MinNewTokensLengthLogitsProcessor, SuppressTokensLogitsProcessor, SuppressTokensAtBeginLogitsProcessor,
WhisperTimeStampLogitsProcessor, TemperatureLogitsWarper, TopKLogitsWarper, TopPLogitsWarper, in the order `_get_logits_processor`
installs them, then `softmax` and `torch.multinomial(probs, 1, generator=g)` as in `_sample`.  The noise the selection kernel needs
is recorded beside the tokens: `empty_like(probs).exponential_(1, generator=clone of g)`, which is what multinomial draws itself.

Every scenario is a batch of rows at one decoding position.  Seeds are consecutive; a scenario is redrawn with the next seed when
one of its rows is "near" (tests/sample_restatement.py: a few-ulp difference could move the token) or when the reference's way of
splitting the group of equal scores at the top-p boundary gives another token than keeping the group whole (the kernel's
documented deviation).  Any other disagreement between the reference and the restatement is an error.  The file records how many
rows were drawn and how many rejected; at most 2 % may be.

    python tools/gen_golden_sample_select.py          (needs transformers; CPU only)
"""
import json
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sample_restatement as sr  # noqa: E402

P = 4


def ids(V):
    return V - 100, V - 88                              # eos, first timestamp id (<|notimestamps|> = tb - 1)


def masks(V):
    eos, tb = ids(V)
    sup = np.zeros(V, dtype=np.uint8)
    sup[:6] = 1
    sup[30:34] = 1
    sup[eos + 1:tb - 1] = 1
    sup[tb + 50] = 1
    bsup = np.zeros(V, dtype=np.uint8)
    bsup[[20, eos, tb + 1]] = 1
    return sup, bsup


def scenarios():
    """name, V, generated history per row (lambda of eos, tb), options (`plant`: (row, column, logit), column -1 = EOS;
    `rows`: batch, 1 unless given).  The micro vocabulary keeps the file small: 60 text ids, EOS, specials, 88 timestamps."""
    A, B_, C = 11, 22, 35
    text = lambda e, t: [[A, B_, C, 51, 52], [A, B_, A, C, A], [51, 52, 53, 54, 55]]          # noqa: E731
    return [
        ("temperature", 160, text, dict(temperature=0.8)),
        ("top_k", 160, text, dict(temperature=1.3, top_k=5)),
        ("top_k_1", 160, text, dict(temperature=0.9, top_k=1)),
        ("top_p", 160, text, dict(temperature=0.7, top_p=0.6)),
        ("top_k_top_p", 160, text, dict(temperature=0.8, top_k=50, top_p=0.9, rows=2)),
        ("repetition_penalty", 160, text, dict(temperature=0.8, repetition_penalty=1.3, plant=[(0, A, 9.0), (1, A, 9.0)], rows=2)),
        ("no_repeat_ngram", 160, text, dict(temperature=0.8, no_repeat_ngram=2, plant=[(1, B_, 9.0), (1, C, 8.5)], rows=2)),
        ("suppress", 160, text, dict(temperature=1.0, suppress=True, plant=[(0, 3, 12.0), (1, 32, 12.0)], rows=2)),
        ("first_begin_suppress", 160, lambda e, t: [[], [], []],
         dict(temperature=1.0, suppress=True, begin_suppress=True, plant=[(0, 20, 12.0), (1, -1, 12.0)], rows=2)),
        ("no_eos", 160, text, dict(temperature=1.0, no_eos=True, plant=[(0, -1, 12.0), (1, -1, 12.0), (2, -1, 12.0)])),
        ("ts_first", 160, lambda e, t: [[], [], []], dict(temperature=0.8, timestamps=True, max_initial=50)),
        ("ts_closed_pair", 160, lambda e, t: [[t, 41, t + 5, t + 5], [t + 2, 42, t + 9, t + 9], [t + 1, 43, t + 3, t + 3]],
         dict(temperature=0.8, timestamps=True, ts_shift=3.0)),
        ("ts_text_timestamp", 160, lambda e, t: [[t + 1, 41, t + 9], [t + 1, 41, t + 30], [t + 2, 42, t + 11]],
         dict(temperature=0.8, timestamps=True, rows=2)),
        ("ts_mass_fires", 160, lambda e, t: [[t + 2, 41, 42], [t + 1, 43, 44], [t + 3, 45, 46]],
         dict(temperature=0.8, timestamps=True, ts_shift=4.0)),
        ("ts_mass_quiet", 160, lambda e, t: [[t + 2, 41, 42], [t + 1, 43, 44], [t + 3, 45, 46]],
         dict(temperature=0.8, timestamps=True, ts_shift=-4.0)),
        ("finished_row", 160, text, dict(temperature=0.8, done=[0, 1, 0], rows=3)),
        ("top_k_beyond_allowed", 160, lambda e, t: [[t + 1, 41, t + 70], [t + 1, 41, t + 75], [t + 2, 42, t + 80]],
         dict(temperature=0.9, top_k=40, timestamps=True)),
        ("all_together", 256, lambda e, t: [[t + 2, A, B_, A], [t + 1, A, B_, C], [t + 3, 51, 52, 51]],
         dict(temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.2, no_repeat_ngram=2, suppress=True, timestamps=True,
              ts_shift=-2.0, plant=[(0, B_, 9.0), (1, A, 8.0)], rows=3)),
        ("all_together_b1", 160, lambda e, t: [[t + 2, A, B_, A]],
         dict(temperature=0.7, top_k=20, top_p=0.8, repetition_penalty=1.2, no_repeat_ngram=2, suppress=True, timestamps=True,
              ts_shift=-2.0, no_eos=True)),
    ]


def build(V, gen_of, opt, seed):
    eos, tb = ids(V)
    gen = gen_of(eos, tb)[:opt.get("rows", 1)]
    B = len(gen)
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(B, V, generator=g) * 2.0
    if opt.get("timestamps"):
        logits[:, tb:] += opt.get("ts_shift", 0.0)
    for b, c, v in opt.get("plant", []):
        if b < B:
            logits[b, eos if c < 0 else c] = v
    logits = logits.bfloat16().float()
    tokens = np.zeros((B, P + 8), dtype=np.int64)
    for b in range(B):
        row = [eos + 1, eos + 2, eos + 7, 50] + list(gen[b])
        tokens[b, :len(row)] = row
    n = P + len(gen[0])
    return logits, tokens, n, g


def kernel_kwargs(V, opt, n):
    eos, tb = ids(V)
    sup, bsup = masks(V)
    return dict(suppress=sup if opt.get("suppress") else None, begin_suppress=bsup if opt.get("begin_suppress") else None,
                first=n == P, no_eos=bool(opt.get("no_eos")), ts_begin=tb if opt.get("timestamps") else -1,
                max_initial=opt.get("max_initial", -1), begin_index=P, eos=eos, fill=eos,
                repetition_penalty=opt.get("repetition_penalty", 1.0), no_repeat_ngram=opt.get("no_repeat_ngram", 0),
                temperature=opt.get("temperature", 1.0), top_k=opt.get("top_k", 0), top_p=opt.get("top_p", 1.0))


def reference(logits, tokens, n, kw, g, done):
    """the token of every row the way GenerationMixin._sample picks it -> (tokens, done, noise multinomial drew)"""
    from transformers.generation import logits_process as lp
    V = logits.shape[1]
    hist = torch.from_numpy(tokens[:, :n])
    procs = []
    if kw["repetition_penalty"] != 1.0:
        procs.append(lp.RepetitionPenaltyLogitsProcessor(penalty=kw["repetition_penalty"]))
    if kw["no_repeat_ngram"]:
        procs.append(lp.NoRepeatNGramLogitsProcessor(kw["no_repeat_ngram"]))
    if kw["no_eos"]:
        procs.append(lp.MinNewTokensLengthLogitsProcessor(P, 10 ** 6, kw["eos"]))
    if kw["suppress"] is not None:
        procs.append(lp.SuppressTokensLogitsProcessor(np.nonzero(kw["suppress"])[0].tolist()))
    if kw["begin_suppress"] is not None:
        procs.append(lp.SuppressTokensAtBeginLogitsProcessor(np.nonzero(kw["begin_suppress"])[0].tolist(), P))
    if kw["ts_begin"] >= 0:
        cfg = types.SimpleNamespace(no_timestamps_token_id=kw["ts_begin"] - 1, eos_token_id=kw["eos"], bos_token_id=kw["eos"],
                                    max_initial_timestamp_index=kw["max_initial"] if kw["max_initial"] >= 0 else None,
                                    _detect_timestamp_from_logprob=True)
        procs.append(lp.WhisperTimeStampLogitsProcessor(cfg, begin_index=P))
    if kw["temperature"] != 1.0:
        procs.append(lp.TemperatureLogitsWarper(kw["temperature"]))
    if kw["top_k"] > 0:
        procs.append(lp.TopKLogitsWarper(top_k=kw["top_k"], min_tokens_to_keep=1))
    if kw["top_p"] < 1.0:
        procs.append(lp.TopPLogitsWarper(top_p=kw["top_p"], min_tokens_to_keep=1))
    sc = logits.clone()
    for p in procs:
        sc = p(hist, sc)
    probs = torch.softmax(sc, dim=-1)
    noise = torch.empty_like(probs).exponential_(1.0, generator=g.clone_state())
    nxt = torch.multinomial(probs, num_samples=1, generator=g)[:, 0].numpy().copy()
    new_done = np.array(done, dtype=bool)
    nxt[new_done] = kw["fill"]
    new_done |= nxt == kw["eos"]
    return nxt, new_done, noise.numpy()


def main():
    out = dict(P=P, scenarios=[], drawn=0, rejected=0)
    seed = 20240
    for name, V, gen_of, opt in scenarios():
        for _ in range(50):
            seed += 1
            logits, tokens, n, g = build(V, gen_of, opt, seed)
            kw = kernel_kwargs(V, opt, n)
            B = tokens.shape[0]
            done = np.array(opt.get("done", [0] * B), dtype=bool)
            want, want_done, noise = reference(logits, tokens, n, kw, g, done)
            got, got_done, margins = sr.sample_select_ref(logits.numpy(), noise, V, tokens, n, done=done, **kw)
            split, _, _ = sr.sample_select_ref(logits.numpy(), noise, V, tokens, n, done=done, split_groups=True, **kw)
            out["drawn"] += B
            bad = sr.near(margins) & ~done
            differs = got != want
            # a token that differs off the margins must be the boundary group's doing: the split restatement is the reference
            unexplained = differs & ~bad & (split != want)
            if unexplained.any():
                raise SystemExit(f"{name}, seed {seed}: restatement {got} / {split} against transformers {want}, margins {margins}")
            if (bad | differs).any():
                out["rejected"] += int((bad | differs).sum())
                continue
            assert (got_done == want_done).all()
            out["scenarios"].append(dict(
                name=name, seed=seed, B=B, V=V, n=n, tokens=tokens.tolist(), done=done.astype(int).tolist(),
                kwargs={k: (None if v is None else np.nonzero(v)[0].tolist()) if k in ("suppress", "begin_suppress") else v
                        for k, v in kw.items()},                       # (the two masks as lists of ids)
                logits_bf16=sr.bf16_pack(logits.numpy()), noise_f32=sr.f32_pack(noise),
                expected=want.tolist(), expected_done=want_done.astype(int).tolist()))
            break
        else:
            raise SystemExit(f"{name}: no acceptable draw in 50 seeds")
    frac = out["rejected"] / out["drawn"]
    if frac > 0.02:
        raise SystemExit(f"{out['rejected']} of {out['drawn']} rows rejected ({100 * frac:.1f} %): above the cap of 2 %")
    path = sr.GOLD
    with open(path, "w") as f:
        head = {k: v for k, v in out.items() if k != "scenarios"}
        f.write(json.dumps(head, separators=(",", ":"))[:-1] + ',"scenarios":[\n')
        f.write(",\n".join(json.dumps(sc, separators=(",", ":")) for sc in out["scenarios"]))
        f.write("\n]}\n")
    print(f"{path}: {len(out['scenarios'])} scenarios, {out['drawn']} rows drawn, {out['rejected']} rejected, "
          f"{os.path.getsize(path) / 1024:.0f} KiB")


if __name__ == "__main__":
    main()
