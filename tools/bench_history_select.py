"""What `generate(repetition_penalty=1.2, no_repeat_ngram_size=3)` costs on the MI355X -> profiles/history_select_bench.json.

distil-large-v3 decoder dimensions (2 decoder layers, d_model 1280, 20 heads, vocabulary 51 866), seeded weights, 220 generated
tokens, batch 16 and 64 (the set-up of tools/bench_generate_scores.py), everything in ONE process.  Per batch, HIP events around
each call, median / min / max of 10 after 3 warm-ups:
  (a) `plain`: greedy `generate` on given encoder outputs, token steps replayed from HIP graphs;
  (b) `history_kernel`: the same call with the two options -- the selection kernel applies them (dw_greedy_select_history), token
      steps replayed from HIP graphs;
  (c) `history_eager`: the same options with the decoder forced onto the eager torch selection (`GreedyDecoder._select_soft`, no
      graph replay): what the package ran before the kernel had the rules;
and the two selection kernels alone at the middle of the sequence (history of 114 tokens) and at its end (223), 200 launches
between two events.  `spread_ms` of a leg is max - min over its 10 repeats; `b_minus_a_ms` and `c_minus_b_ms` stand next to it.
Nothing is promised here: the file records what was measured.
Usage:  python tools/bench_history_select.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "history_select_bench.json")
NEW, P = 220, 4
OPTIONS = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)


def timed(fn, warm=3, reps=10):
    import torch
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "reps": reps}


def kernel_us(fn, launches=200):
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(10):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / launches)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "launches": launches}


def batch(model, ops, B):
    import torch
    from distil_whisper_amd.modeling import BaseModelOutput
    dev, d = ops.device, model.dims
    g = torch.Generator().manual_seed(B)
    enc = (torch.randn(B, d.max_src, d.d_model, generator=g) * 0.5).to(dev)
    ids = torch.tensor([[50258, 50259, 50360, 50364]] * B, device=dev)
    kw = dict(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=ids, max_new_tokens=NEW,
              min_new_tokens=NEW, return_dict_in_generate=True)
    res = {"batch": B, "new_tokens": NEW, "prompt_tokens": P, "vocab": d.vocab, "options": OPTIONS}

    def decoder():
        (dec,) = model._decoders.values()
        return dec

    plain = model.generate(use_graphs=True, **kw).sequences
    res["plain"] = timed(lambda: model.generate(use_graphs=True, **kw))
    hist = model.generate(use_graphs=True, **OPTIONS, **kw).sequences
    dec = decoder()
    assert dec.history is not None and dec.use_graphs and len(dec.graphs) > 0
    res["history_kernel"] = timed(lambda: model.generate(use_graphs=True, **OPTIONS, **kw))
    # (c): the decoder of the same call without graphs, switched to the eager torch selection
    model.generate(use_graphs=False, **OPTIONS, **kw)
    dec = decoder()
    dec.history, dec.use_graphs = None, False
    eager = model.generate(use_graphs=False, **OPTIONS, **kw).sequences
    assert decoder() is dec
    res["history_eager"] = timed(lambda: model.generate(use_graphs=False, **OPTIONS, **kw))
    model._decoders = {}
    gen = hist[:, P:].tolist()
    res["sanity"] = {
        "tokens_differ_from_plain_share": float((hist != plain).float().mean()),
        # (the eager path divides by multiplying with the reciprocal on the GPU: a near tie may fall the other way)
        "rows_equal_to_eager_path": int((hist == eager).all(1).sum()),
        "rows_with_a_repeated_3gram": sum(len({tuple(r[i:i + 3]) for i in range(len(r) - 2)}) < len(r) - 2 for r in gen)}
    res["b_minus_a_ms"] = res["history_kernel"]["median_ms"] - res["plain"]["median_ms"]
    res["c_minus_b_ms"] = res["history_eager"]["median_ms"] - res["history_kernel"]["median_ms"]
    res["b_minus_a_us_per_step"] = res["b_minus_a_ms"] * 1e3 / NEW
    # the selection kernels alone, on the history the call above decoded
    logits = (torch.randn(B, (d.vocab + 63) // 64 * 64, generator=g) * 1.5).to(dev).bfloat16()
    sup = torch.zeros(d.vocab, dtype=torch.uint8)
    sup[list(model.generation_config.suppress_tokens)] = 1
    sup = sup.to(dev)
    cur = torch.zeros(B, 1, dtype=torch.int64, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    for n in (P + NEW // 2, P + NEW - 1):
        toks = hist.clone().contiguous()
        common = dict(suppress=sup, eos=50257, fill=50257, done=done)
        res[f"kernel_select_plain_n{n}"] = kernel_us(lambda: ops.greedy_select(logits, d.vocab, toks, n, cur, **common))
        res[f"kernel_select_history_n{n}"] = kernel_us(lambda: ops.greedy_select_history(
            logits, d.vocab, toks, n, cur, repetition_penalty=OPTIONS["repetition_penalty"],
            no_repeat_ngram=OPTIONS["no_repeat_ngram_size"], **common))
    return res


def main():
    import torch
    sys.path.insert(0, ROOT)
    from distil_whisper_amd import build
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    from distil_whisper_amd.ops_hip import HipOps
    dev = "cuda:0"
    ops = HipOps(dev)
    tdims = si.PRESETS["large-v3"]
    t_sd = si.random_state_dict(tdims, 0, dev)
    s_sd, sdims = si.student_from_teacher(t_sd, tdims, 32, 2)
    del t_sd
    model = WhisperForConditionalGeneration(sdims, ops=ops, state_dict=s_sd)
    model.generation_config = GenerationConfig.from_any(dict(
        eos_token_id=50257, pad_token_id=50257, decoder_start_token_id=50258, max_length=448,
        suppress_tokens=list(range(1, 90)) + list(range(50257, 50364)), begin_suppress_tokens=[220, 50257]))
    results = {"kernels_sha16": build.kernels_sha16(),
               "protocol": "one process; HIP events around each call, median of 10 after 3 warm-ups; spread_ms = max - min of the 10",
               "batches": [batch(model, ops, B) for B in (16, 64)]}
    torch.cuda.synchronize()
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
