"""What `generate(sequence_bias=...)` costs on the MI355X -> profiles/sequence_bias_bench.json.

The set-up of tools/bench_history_select.py: distil-large-v3 decoder dimensions (2 decoder layers, d_model 1280, 20 heads,
vocabulary 51 866), seeded weights, 220 generated tokens, batch 16 and 64, everything in ONE process.  HIP events around each
call, median / min / max of 10 after 3 warm-ups.  Per batch, first the graph legs, INTERLEAVED -- repeat r of every leg runs before
repeat r + 1 of any; each leg keeps its own decoder and captured graphs alive (`plain_back_to_back`, measured just before, is the
plain leg alone in ten consecutive repeats, the way tools/bench_history_select.py times it):
  `plain`           greedy `generate` on given encoder outputs, token steps replayed from HIP graphs (dw_greedy_select);
  `history_kernel`  the same with repetition_penalty=1.2, no_repeat_ngram_size=3 (dw_greedy_select_history);
  `bias_S`          the same as `plain` with a `sequence_bias` of S = 8, 128, 1024 seeded random sequences of 1-4 text tokens
                    with biases of +-1 .. 8 (dw_greedy_select_bias, graphs);
then, in a block of their own (they are host-bound and take up to seconds per call: next to them a graph leg starts on an idle GPU),
  `eager_S`         the same tables with the decoder forced onto the eager torch selection (`GreedyDecoder._select_soft`:
                    decoding.apply_sequence_bias, no graph replay), S = 8 and 128 interleaved with each other; S = 1024 is run
                    ONCE (`reps` says so: its Python loop over the table takes seconds per call) and its tokens are compared too.
Then the selection kernels alone at the end of the sequence (history of 223 tokens), 200 launches between two events: the three
table sizes, and three tables of 1024 entries that take the kernel apart -- `no_entry_counts` (two-token sequences whose prefix the
history never holds: the cost of testing the table), `one_token` (every entry counts: 1024 biased columns) and `one_column` (the
worst case of the merge).  `--kernels-only` runs just that part, each variant as one block of KERNELS_ONLY_LAUNCHES launches: the
run to put under a kernel trace (`kernel_trace_us` in the file is the median duration of each block's dispatches in such a trace).
`spread_ms` of a leg is max - min over its repeats.  Nothing is promised here: the file records what was measured.
Usage:  python tools/bench_sequence_bias.py [--kernels-only | --merge-trace KERNEL_TRACE_CSV]
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "sequence_bias_bench.json")
NEW, P = 220, 4
HISTORY = dict(repetition_penalty=1.2, no_repeat_ngram_size=3)
SIZES = (8, 128, 1024)
KERNELS_ONLY_LAUNCHES = 120


def table_of(S, seed=0):
    """S distinct sequences of 1-4 text ids with biases of +-1 .. 8 (a dict: the reference's own form)"""
    import numpy as np
    rng = np.random.default_rng(1000 + S + seed)
    sb = {}
    while len(sb) < S:
        q = tuple(int(t) for t in rng.integers(1000, 50000, size=int(rng.integers(1, 5))))
        sb[q] = float(rng.choice([-1, 1]) * rng.integers(4, 33)) / 4
    return sb


def interleaved(legs, warm=3, reps=10):
    """legs: name -> callable.  -> name -> timing (a single leg: back-to-back repeats)"""
    import torch
    for fn in legs.values():
        for _ in range(warm):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name in legs}
    for _ in range(reps):
        for name, fn in legs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1))
    return {name: {"median_ms": statistics.median(v), "min_ms": min(v), "max_ms": max(v), "spread_ms": max(v) - min(v),
                   "reps": len(v)} for name, v in ms.items()}


def kernel_us(fn, launches=200, reps=10):
    import torch
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(launches):
            fn()
        e1.record()
        e1.synchronize()
        us.append(e0.elapsed_time(e1) * 1e3 / launches)
    return {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "launches": launches}


def kernels(model, ops, B, hist, launches=200, reps=10):
    """the selection kernels alone on the history `hist` [B, P + NEW] at its last position"""
    import torch
    from distil_whisper_amd.decoding import sequence_bias_table
    dev, d = ops.device, model.dims
    g = torch.Generator().manual_seed(B)
    logits = (torch.randn(B, (d.vocab + 63) // 64 * 64, generator=g) * 1.5).to(dev).bfloat16()
    sup = torch.zeros(d.vocab, dtype=torch.uint8)
    sup[list(model.generation_config.suppress_tokens)] = 1
    sup = sup.to(dev)
    cur = torch.zeros(B, 1, dtype=torch.int64, device=dev)
    done = torch.zeros(B, dtype=torch.bool, device=dev)
    n = P + NEW - 1
    toks = hist.clone().contiguous()
    common = dict(suppress=sup, eos=50257, fill=50257, done=done)
    hk = dict(repetition_penalty=HISTORY["repetition_penalty"], no_repeat_ngram=HISTORY["no_repeat_ngram_size"])
    res = {f"kernel_select_plain_n{n}": kernel_us(lambda: ops.greedy_select(logits, d.vocab, toks, n, cur, **common), launches, reps),
           f"kernel_select_history_n{n}": kernel_us(lambda: ops.greedy_select_history(logits, d.vocab, toks, n, cur, **hk, **common),
                                                    launches, reps)}
    # three tables of 1024 entries that take the kernel apart (the history holds ids >= 1000 only)
    apart = {"1024_no_entry_counts": {(1 + i % 7, 1000 + 40 * i): 0.25 for i in range(1024)},
             "1024_one_token": {(1000 + 40 * i,): 0.25 for i in range(1024)},
             "1024_one_column": {(1000 + i, 2000): 0.25 for i in range(1024)}}
    for name, sb in list((str(S), table_of(S)) for S in SIZES) + list(apart.items()):
        t = sequence_bias_table(sb, None, d.vocab, 50257).tensors(dev)
        res[f"kernel_select_bias_{name}_n{n}"] = kernel_us(lambda: ops.greedy_select_bias(logits, d.vocab, toks, n, cur, **t, **common),
                                                           launches, reps)
    return res


VARIANTS = ("plain", "history", "bias_8", "bias_128", "bias_1024", "bias_1024_no_entry_counts", "bias_1024_one_token",
            "bias_1024_one_column")                        # the order in which `kernels` launches them


def merge_trace(csv_path):
    """`kernel_trace_us` of OUT from the kernel-trace CSV of a `--kernels-only` run: the dispatches of the selection kernels in
    start order are blocks of KERNELS_ONLY_LAUNCHES per variant, batch 16 first; per block the median / min / max duration"""
    import csv
    with open(csv_path) as f:
        rows = [r for r in csv.DictReader(f) if "greedy_select" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    assert len(rows) == 2 * len(VARIANTS) * KERNELS_ONLY_LAUNCHES, len(rows)
    with open(OUT) as f:
        results = json.load(f)
    for bi, entry in enumerate(results["batches"]):
        trace = {}
        for vi, name in enumerate(VARIANTS):
            blk = rows[(bi * len(VARIANTS) + vi) * KERNELS_ONLY_LAUNCHES:][:KERNELS_ONLY_LAUNCHES]
            assert len({r["Kernel_Name"] for r in blk}) == 1 and ("bias" in blk[0]["Kernel_Name"]) == name.startswith("bias"), name
            us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in blk]
            trace[name] = {"median_us": statistics.median(us), "min_us": min(us), "max_us": max(us), "dispatches": len(us)}
        entry["kernel_trace_us"] = trace
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps([e["kernel_trace_us"] for e in results["batches"]]))


def batch(model, ops, B):
    import torch
    from distil_whisper_amd.modeling import BaseModelOutput
    dev, d = ops.device, model.dims
    g = torch.Generator().manual_seed(B)
    enc = (torch.randn(B, d.max_src, d.d_model, generator=g) * 0.5).to(dev)
    ids = torch.tensor([[50258, 50259, 50360, 50364]] * B, device=dev)
    kw = dict(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=ids, max_new_tokens=NEW,
              min_new_tokens=NEW, return_dict_in_generate=True)
    res = {"batch": B, "new_tokens": NEW, "prompt_tokens": P, "vocab": d.vocab, "history_options": HISTORY}
    decoders, legs, outs = {}, {}, {}

    def leg(name, graphs, eager=False, **opts):
        """one leg with a decoder of its own: `generate` keeps a single live decoder, so the leg swaps its own in"""
        model._decoders = {}
        outs[name] = model.generate(use_graphs=graphs, **opts, **kw).sequences
        (dec,) = model._decoders.values()
        if eager:
            dec.bias, dec.use_graphs = None, False
        else:
            assert dec.use_graphs and len(dec.graphs) > 0
        decoders[name] = dict(model._decoders)

        def call():
            model._decoders = decoders[name]
            out = model.generate(use_graphs=graphs, **opts, **kw)
            assert next(iter(model._decoders.values())) is dec
            return out
        legs[name] = call

    leg("plain", True)
    leg("history_kernel", True, **HISTORY)
    for S in SIZES:
        leg(f"bias_{S}", True, sequence_bias=table_of(S))
        assert next(iter(decoders[f"bias_{S}"].values())).bias is not None
    # the plain leg the way tools/bench_history_select.py times it (ten back-to-back repeats): what THIS GPU and process give for
    # the figure of profiles/history_select_bench.json that the interleaved plain leg is read against
    res.update(interleaved({"plain_back_to_back": legs["plain"]}))
    res.update(interleaved(legs))
    # the eager legs in a block of their own, after the graph legs
    graph_legs = dict(legs)
    legs.clear()
    for S in SIZES:
        leg(f"eager_{S}", False, eager=True, sequence_bias=table_of(S))
    big = legs.pop("eager_1024")
    res.update(interleaved(legs))
    legs.update(graph_legs)
    for S in SIZES[:2]:
        outs[f"eager_{S}"] = legs[f"eager_{S}"]().sequences
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    outs["eager_1024"] = big().sequences
    e1.record()
    e1.synchronize()
    ms = e0.elapsed_time(e1)
    res["eager_1024"] = {"median_ms": ms, "min_ms": ms, "max_ms": ms, "spread_ms": 0.0, "reps": 1}
    model._decoders = {}
    plain = res["plain"]["median_ms"]
    res["sanity"] = {f"bias_{S}": {"tokens_differ_from_plain_share": float((outs[f"bias_{S}"] != outs["plain"]).float().mean()),
                                   "rows_equal_to_eager_path": int((outs[f"bias_{S}"] == outs[f"eager_{S}"]).all(1).sum())}
                     for S in SIZES}
    for name in ("history_kernel",) + tuple(f"bias_{S}" for S in SIZES) + tuple(f"eager_{S}" for S in SIZES):
        res[f"{name}_minus_plain_ms"] = res[name]["median_ms"] - plain
        res[f"{name}_minus_plain_us_per_step"] = (res[name]["median_ms"] - plain) * 1e3 / NEW
    res.update(kernels(model, ops, B, outs["history_kernel"]))
    return res


def main():
    if "--merge-trace" in sys.argv:
        return merge_trace(sys.argv[sys.argv.index("--merge-trace") + 1])
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
    if "--kernels-only" in sys.argv:
        g = torch.Generator().manual_seed(5)
        for B in (16, 64):
            hist = torch.randint(1000, 50000, (B, P + NEW), generator=g).to(dev)
            # (kernel_us launches 20 warm-ups first: 20 + 2 * 50 = KERNELS_ONLY_LAUNCHES per variant)
            print(json.dumps({"batch": B, **kernels(model, ops, B, hist, launches=50, reps=2)}))
        return
    results = {"kernels_sha16": build.kernels_sha16(),
               "protocol": "one process; legs interleaved; HIP events around each call, median of 10 after 3 warm-ups; "
                           "spread_ms = max - min of the repeats",
               "batches": [batch(model, ops, B) for B in (16, 64)]}
    torch.cuda.synchronize()
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
