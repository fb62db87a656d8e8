"""What `generate(temperature=0.8, top_k=50, top_p=0.9)` costs on the MI355X -> profiles/sample_select_bench.json.

distil-large-v3 decoder dimensions (2 decoder layers, d_model 1280, 20 heads, vocabulary 51 866), seeded weights, 220 generated
tokens, batch 16 and 64 (the set-up of tools/bench_history_select.py), everything in ONE process.  Per batch three decoders
(decoding.GreedyDecoder, what `generate` drives) on the same engine and encoder output, their runs INTERLEAVED (a, b, c, a, b, c,
...), HIP events around each run, median / min / max of 10 rounds after 3 warm-up rounds:
  (a) `greedy`: greedy selection, token steps replayed from HIP graphs;
  (b) `sample_kernel`: sampling through the selection kernel (dw_sample_select) -- per step one `exponential_` launch and the replay
      of a graph that ends in the kernel;
  (c) `sample_torch`: the same options on the torch path (DW_SAMPLE_TORCH=1: `GreedyDecoder._select_soft`, eager, no graph
      replay): what the package ran before the kernel sampled.
and, between two events over 200 launches, the sampled kernel alone next to the two greedy kernels and the `exponential_` draw, on
random logits (flat: top-p finds no narrow candidate set) and on the same logits with forty columns raised (peaked, as a trained
model's).  `spread_ms` of a leg is max - min over its 10 runs.  Nothing is promised here: the file records what was measured.
Usage:  python tools/bench_sample_select.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "sample_select_bench.json")
NEW, P = 220, 4
OPTIONS = dict(temperature=0.8, top_k=50, top_p=0.9)
EOS = 50257


def interleaved(legs, warm=3, reps=10):
    import torch
    for _ in range(warm):
        for fn in legs.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in legs}
    for _ in range(reps):
        for k, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    return {k: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v), "reps": reps}
            for k, v in ms.items()}


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


def batch(model, ops, B, suppress, begin_suppress):
    import torch
    from distil_whisper_amd import decoding
    eng, d, dev = model.engine, model.dims, ops.device
    g = torch.Generator().manual_seed(B)
    enc = (torch.randn(B, d.max_src, d.d_model, generator=g) * 0.5).to(dev).reshape(-1, d.d_model).to(eng.lowp).contiguous()
    ids = torch.tensor([[50258, 50259, 50360, 50364]] * B, device=dev)
    res = {"batch": B, "new_tokens": NEW, "prompt_tokens": P, "vocab": d.vocab, "options": OPTIONS}

    def decoder(soft, torch_path=False):
        os.environ[decoding.SAMPLE_TORCH_ENV] = "1" if torch_path else "0"
        try:
            return decoding.GreedyDecoder(eng, B, P + NEW, eos_token_id=EOS, suppress_tokens=suppress,
                                          begin_suppress_tokens=begin_suppress, use_graphs=True, pad_token_id=EOS, soft=soft)
        finally:
            del os.environ[decoding.SAMPLE_TORCH_ENV]
    soft = dict(do_sample=True, repetition_penalty=None, no_repeat_ngram_size=0, **OPTIONS)
    dec = {"greedy": decoder(None), "sample_kernel": decoder(dict(soft)), "sample_torch": decoder(dict(soft), torch_path=True)}
    assert dec["sample_kernel"].sample is not None and dec["sample_kernel"].use_graphs
    assert dec["sample_torch"].sample is None and not dec["sample_torch"].use_graphs
    legs = {k: (lambda v=v: v.run(enc, ids, NEW, NEW)) for k, v in dec.items()}
    torch.manual_seed(0)
    a = legs["sample_kernel"]()
    torch.manual_seed(0)
    b = legs["sample_torch"]()
    greedy = legs["greedy"]()
    assert len(dec["sample_kernel"].graphs) > 0
    res.update(interleaved(legs))
    # Under one seed the two paths draw the same noise; a row leaves the torch path's sequence at the first step where the top-p
    # boundary cuts through a group of equal scores (kept whole here, split by the torch sort) and the token falls into it -- the
    # flat bf16 logits of seeded random weights hold many equal scores among their top 50 -- and stays apart from there on.
    # Without top-p nothing but a near tie of two quotients separates them.
    no_p = dict(soft, top_p=None)
    pair = [decoder(dict(no_p)), decoder(dict(no_p), torch_path=True)]
    outs = []
    for dd in pair:
        torch.manual_seed(0)
        outs.append(dd.run(enc, ids, NEW, NEW))
    del pair
    res["sanity"] = {"rows_equal_to_torch_path_under_one_seed": int((a == b).all(1).sum()),
                     "tokens_equal_to_torch_path_share": float((a == b).float().mean()),
                     "first_step_a_row_leaves_the_torch_path": sorted(int(x) for x in (a != b).float().argmax(1)[(a != b).any(1)] - P),
                     "rows_equal_to_torch_path_without_top_p": int((outs[0] == outs[1]).all(1).sum()),
                     "tokens_differ_from_greedy_share": float((a != greedy).float().mean())}
    res["kernel_minus_greedy_ms"] = res["sample_kernel"]["median_ms"] - res["greedy"]["median_ms"]
    res["torch_minus_kernel_ms"] = res["sample_torch"]["median_ms"] - res["sample_kernel"]["median_ms"]
    res["kernel_minus_greedy_us_per_step"] = res["kernel_minus_greedy_ms"] * 1e3 / NEW
    res["kernel_leg_beats_torch_leg"] = bool(res["sample_kernel"]["median_ms"] < res["sample_torch"]["median_ms"])
    del dec, legs
    # the kernels alone, on the history the sampled run decoded
    flat = torch.randn(B, (d.vocab + 63) // 64 * 64, generator=g) * 1.5
    peaked = flat.clone()
    peaked[:, torch.randperm(d.vocab, generator=g)[:40]] += torch.linspace(14.0, 6.0, 40)
    sup = torch.zeros(d.vocab, dtype=torch.uint8)
    sup[list(suppress)] = 1
    sup = sup.to(dev)
    cur = torch.zeros(B, 1, dtype=torch.int64, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    noise = torch.empty(B, d.vocab, dtype=torch.float32, device=dev).exponential_(1.0)
    toks = a.clone().contiguous()
    n = P + NEW // 2
    common = dict(suppress=sup, eos=EOS, fill=EOS, done=done, no_eos=True)
    res["kernel_exponential_draw"] = kernel_us(lambda: noise.exponential_(1.0))
    for name, x in (("flat", flat), ("peaked", peaked)):
        logits = x.to(dev).bfloat16()
        k = res[f"kernels_{name}_logits_n{n}"] = {}
        k["greedy_select"] = kernel_us(lambda: ops.greedy_select(logits, d.vocab, toks, n, cur, **common))
        k["greedy_select_history"] = kernel_us(lambda: ops.greedy_select_history(
            logits, d.vocab, toks, n, cur, repetition_penalty=1.2, no_repeat_ngram=3, **common))
        for label, opt in (("temperature", dict(temperature=0.8)), ("top_k_50", dict(temperature=0.8, top_k=50)),
                           ("top_p_0.9", dict(temperature=0.8, top_p=0.9)), ("top_k_50_top_p_0.9", dict(OPTIONS)),
                           ("top_k_50_top_p_0.9_history", dict(OPTIONS, repetition_penalty=1.2, no_repeat_ngram=3))):
            k[f"sample_select_{label}"] = kernel_us(lambda: ops.sample_select(logits, d.vocab, toks, n, cur, noise, **common, **opt))
    return res


def main():
    import torch
    sys.path.insert(0, ROOT)
    from distil_whisper_amd import build
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    from distil_whisper_amd.ops_hip import HipOps
    dev = "cuda:0"
    ops = HipOps(dev)
    tdims = si.PRESETS["large-v3"]
    t_sd = si.random_state_dict(tdims, 0, dev)
    s_sd, sdims = si.student_from_teacher(t_sd, tdims, 32, 2)
    del t_sd
    model = WhisperForConditionalGeneration(sdims, ops=ops, state_dict=s_sd)
    suppress, begin_suppress = list(range(1, 90)) + list(range(50257, 50364)), [220, 50257]
    results = {"kernels_sha16": build.kernels_sha16(),
               "protocol": "one process; per batch three decoders run interleaved, HIP events around each run, median of 10 rounds "
                           "after 3 warm-up rounds; spread_ms = max - min of the 10",
               "batches": [batch(model, ops, B, suppress, begin_suppress) for B in (16, 64)]}
    torch.cuda.synchronize()
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
