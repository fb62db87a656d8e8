"""FP8 cross-attention K/V against the bf16 cache on the MI355X -> profiles/cross_kv_fp8_bench.json.

ONE process, the legs of a comparison INTERLEAVED (bf16, fp8, bf16, fp8, ...), median / min / max of RUNS timed repetitions after one
untimed repetition of each leg (which captures the HIP graphs).  Models: decoder dimensions of distil-large-v3 (2 decoder layers)
and large-v3 (32), d_model 1280, 20 heads, vocabulary 51 866, bf16, seeded random weights with planted label lengths, behind the
2-layer encoder of tools/bench_continuous.py (whose `planted_model` this tool imports: `windows_per_s` is NOT the throughput of a
full model).  Batch 16 and 64.  Recorded per model and batch:
  attn_launch   the cross-attention launch alone (dw_decode_attn_proj mode 0 against dw_decode_attn_proj_kv8): one graph holding the
                launch of every layer over that layer's own cache, replayed and timed by device events; us per launch and GB/s over
                the operand bytes (K, V, scales, Wq of the heads, x, o), computed from the shapes below
  greedy_step   GreedyDecoder's token step (decode pass + selection kernel), replayed graphs at positions P .. P + STEPS, ms per step
  slot_step     SlotDecoder's token step (dw_decode_token_rows + dw_slot_step), every slot live, ms per step
  labeller      PseudoLabeller wall clock (device synchronised on either side), 2 batches of windows, with and without continuous=True
  quant         dw_cross_kv_quant, us per window and layer (the projection GEMM in front of it is the same for both dtypes)
  cache_bytes   device memory of the cache's tensors (FP8: codes, scales and the one layer of bf16 staging)
  parent        with DW_PARENT_LIB=<libdwamd.so built from the parent commit, tools/build_base_lib.sh>: the bf16 attention launch and
                the bf16 token step through that library in the same process, interleaved with this tree's (their code is unchanged)
`format_cost`: what the format does to the logits -- relative RMS and largest difference of the FP8 path's logits from the bf16 path's
over 8 teacher-forced steps, next to the bf16 path's own difference from the fp32 torch statement (oracle.ref_ops, lowp fp32), on
random-normal encoder rows and on trained-like ones (4 x the spread: peaked attention; one channel 30 x: an outlier channel).
No trained checkpoint is on these machines: the effect on label quality (WER) is NOT measured.
Usage:  python tools/bench_cross_kv_fp8.py      (BENCH_RUNS=n overrides the 10 runs, BENCH_LAYERS=2|32 keeps one model)
"""
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "cross_kv_fp8_bench.json")
RUNS = int(os.environ.get("BENCH_RUNS", "10"))
STEPS = 64
PARENT_STEPS = 16        # decode passes per graph of the this-library / parent-library comparison


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]), "min": xs[0], "max": xs[-1]}


def interleaved(legs, runs=None):
    """legs: {name: fn -> ms}; one untimed call of each, then `runs` rounds over all legs in turn -> {name: stats}."""
    for fn in legs.values():
        fn()
    ms = {n: [] for n in legs}
    for _ in range(RUNS if runs is None else runs):
        for n, fn in legs.items():
            ms[n].append(fn())
    return {n: stats(v) for n, v in ms.items()}


def event_ms(fn):
    import torch
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b)


def wall_ms(fn):
    import torch
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def graph_of(fn):
    import torch
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        fn()
    return g


def cache_bytes(cache):
    import torch
    seen, total = set(), 0

    def walk(x):
        nonlocal total
        if torch.is_tensor(x):
            s = x.untyped_storage()
            if s.data_ptr() not in seen:
                seen.add(s.data_ptr())
                total += s.nbytes()
        elif isinstance(x, (list, tuple)):
            for y in x:
                walk(y)
    for k in ("self", "cross", "cross8", "cross_stage"):
        walk(cache.get(k))
    return total


class ParentLib:
    """The parent commit's library: its dw_decode_attn_proj has today's signature, its descriptors end in front of the new fields."""

    def __init__(self, path):
        from distil_whisper_amd import ops_hip as oh
        self.lib = C.CDLL(path)
        self.Layer = type("ParentLayer", (C.Structure,), {"_fields_": oh.DwDecoderLayer._fields_[:-3]})
        self.Step = type("ParentStep", (C.Structure,), {"_fields_": oh.DwDecodeStep._fields_[:-1]})
        self.lib.dw_decode_attn_proj.argtypes, self.lib.dw_decode_attn_proj.restype = oh._SIGS["dw_decode_attn_proj"]
        self.lib.dw_decode_step.argtypes, self.lib.dw_decode_step.restype = [C.POINTER(self.Step), C.c_void_p], C.c_int

    def descriptor(self, desc, layers, n_layers):
        old = (self.Layer * n_layers)()
        for i in range(n_layers):
            for f, _ in self.Layer._fields_:
                setattr(old[i], f, getattr(layers[i], f))
        step = self.Step()
        for f, _ in self.Step._fields_:
            setattr(step, f, getattr(desc, f))
        step.layers = C.cast(old, C.c_void_p)
        return step, old


def attn_launch(ops, eng, caches, B, parent):
    import torch
    d, st = eng.dims, eng.st
    D, H, S, nl = d.d_model, d.heads, d.max_src, d.dec_layers
    x = torch.randn(B, D, device=ops.device, dtype=eng.stream)
    o = torch.empty(B, D, device=ops.device, dtype=torch.bfloat16)
    par = []
    for i in range(nl):
        p = f"model.decoder.layers.{i}"
        cv = st.attn_views(f"{p}.encoder_attn")
        par.append((st.p[f"{p}.encoder_attn_layer_norm.weight"], st.p[f"{p}.encoder_attn_layer_norm.bias"], cv["wqkv"][:D], cv["bqkv"][:D]))

    def bf16():
        for i, (g, b, w, bq) in enumerate(par):
            kv = caches["bf16"]["cross"][i]
            ops.decode_attn_proj(0, x, g, b, w, bq, kv[:, :D], kv[:, D:], B, H, S, out=o)

    def fp8():
        for i, (g, b, w, bq) in enumerate(par):
            ops.decode_attn_proj_kv8(x, g, b, w, bq, *caches["fp8"]["cross8"][i], B, H, S, out=o)
    reps = max(4, 256 // nl)
    legs = {}
    for name, fn in (("bf16", bf16), ("fp8", fp8)):
        g = graph_of(fn)
        legs[name] = (lambda g=g: event_ms(lambda: [g.replay() for _ in range(reps)]) * 1e3 / (reps * nl))
    if parent is not None:
        from distil_whisper_amd.ops_hip import _dt, _p

        def old():
            for i, (g, b, w, bq) in enumerate(par):
                kv = caches["bf16"]["cross"][i]
                rc = parent.lib.dw_decode_attn_proj(0, _p(x), _dt(x), x.stride(0), _p(g), _p(b), 1e-5, _p(w), _p(bq), _p(kv[:, :D]),
                                                    _p(kv[:, D:]), kv.stride(0), S, None, _p(o), o.stride(0), B, H, S, 0.125, ops._stream())
                assert rc == 0
        g = graph_of(old)
        legs["bf16_parent_lib"] = (lambda g=g: event_ms(lambda: [g.replay() for _ in range(reps)]) * 1e3 / (reps * nl))
    us = interleaved(legs)
    small = D * D * 2 + B * D * (x.element_size() + 2) + 8 * D                 # Wq, x, o, gamma / beta
    nbytes = {"bf16": 2 * B * S * D * 2 + small, "fp8": 2 * B * S * D + B * 2 * D * 4 + small}
    out = {"replays_per_sample": reps, "operand_bytes": nbytes}
    for n, s in us.items():
        out[n] = {"us_per_launch": s, "GBps": nbytes["fp8" if n == "fp8" else "bf16"] / (s["median"] * 1e-6) / 1e9}
    out["fp8_over_bf16"] = us["fp8"]["median"] / us["bf16"]["median"]
    if parent is not None:
        out["bf16_over_parent_lib"] = us["bf16"]["median"] / us["bf16_parent_lib"]["median"]
    return out


def greedy_step(ops, model, enc, B, P, parent):
    import torch
    from distil_whisper_amd.decoding import GreedyDecoder
    prompt = torch.tensor([PROMPT] * B, device=ops.device)
    decs, legs, caches = {}, {}, {}
    for name, dt in (("bf16", None), ("fp8", "fp8")):
        dec = decs[name] = GreedyDecoder(model.engine, B, P + STEPS + 1, use_graphs=True, cross_kv_dtype=dt)
        dec.run(enc, prompt, STEPS)                                         # captures the graphs of positions P - 1 .. P + STEPS - 2
        caches[name] = dec.cache
        legs[name] = (lambda dec=dec: event_ms(lambda: [dec._run_step(t, 2) for t in range(P, P + STEPS - 1)]) / (STEPS - 1))
    if parent is not None:
        # the bf16 decode pass alone through either library (no selection kernel): one graph of STEPS - 1 passes each
        eng, cache = model.engine, decs["bf16"].cache
        desc, ws, layers, _ = eng._decode_desc(cache, 1)
        old, keep = parent.descriptor(desc, layers, eng.dims.dec_layers)
        ids = torch.full((B, 1), 1000, dtype=torch.long, device=ops.device)
        desc.ids = old.ids = ids.data_ptr()

        def passes(lib, dsc):
            for t in range(P, P + PARENT_STEPS):
                dsc.t = t
                assert lib.dw_decode_step(C.byref(dsc), ops._stream()) == 0
        g_new, g_old = graph_of(lambda: passes(ops.lib, desc)), graph_of(lambda: passes(parent.lib, old))
        legs["bf16_pass_this_lib"] = lambda: event_ms(g_new.replay) / PARENT_STEPS
        legs["bf16_pass_parent_lib"] = lambda: event_ms(g_old.replay) / PARENT_STEPS
    ms = interleaved(legs)
    out = {n: {"ms_per_step": s} for n, s in ms.items()}
    out["fp8_over_bf16"] = ms["fp8"]["median"] / ms["bf16"]["median"]
    if parent is not None:
        out["bf16_pass_over_parent_lib"] = ms["bf16_pass_this_lib"]["median"] / ms["bf16_pass_parent_lib"]["median"]
    return out, caches


def slot_step(ops, model, enc, B, P):
    from distil_whisper_amd.decoding import SlotDecoder
    S, legs = model.dims.max_src, {}
    for name, dt in (("bf16", None), ("fp8", "fp8")):
        sd = SlotDecoder(model.engine, B, P + STEPS + 2, EOS, suppress_tokens=[EOS], cross_kv_dtype=dt)     # (no slot ends early)
        sd.cache = model.engine.decode_slots_init(B, sd.max_len, cross_kv_dtype=dt)

        def steps(sd=sd):
            for b in range(B):                                              # every slot live, at the start of its window
                sd._refill(b, enc[b * S:(b + 1) * S], PROMPT, STEPS + 1)
            return event_ms(lambda: [sd._run_step(i) for i in range(STEPS)]) / STEPS
        legs[name] = steps
    ms = interleaved(legs)
    out = {n: {"ms_per_step": s} for n, s in ms.items()}
    out["fp8_over_bf16"] = ms["fp8"]["median"] / ms["bf16"]["median"]
    return out


def quant_cost(ops, eng, cache, B):
    d = eng.dims
    k8, v8, sc = cache["cross8"][0]
    g = graph_of(lambda: ops.cross_kv_quant(cache["cross_stage"], k8, v8, sc, 0, B, d.max_src, d.heads))
    us = interleaved({"q": lambda: event_ms(lambda: [g.replay() for _ in range(8)]) * 1e3 / (8 * B)})["q"]
    moved = B * d.max_src * 2 * d.d_model * (2 + 2 + 1)                     # two sweeps over the bf16 rows, one store of the codes
    return {"us_per_window_and_layer": us, "GBps_over_bytes_moved": moved / B / (us["median"] * 1e-6) / 1e9}


def labeller(ops, model, eos_vec, B):
    import numpy as np
    import torch
    import bench_continuous as bc
    from distil_whisper_amd.modeling import WhisperFeatureExtractor
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    dev, d, N = ops.device, model.dims, 2 * B
    rng = np.random.default_rng(B)
    kinds = rng.choice(len(bc.LENGTHS), size=N, p=bc.PROBS)
    levels = torch.tensor([bc.EOS_LEVELS[k] for k in kinds], dtype=torch.float32, device=dev)
    audios = [0.1 * rng.standard_normal(16000).astype(np.float32) for _ in range(N)]
    fe = WhisperFeatureExtractor(feature_size=d.n_mels, ops=ops)
    real_encode, calls = model.engine.encode, [0]

    def encode(feats, save=False):                       # tools/bench_continuous.py: the encoder runs, its output is replaced by planted rows
        out = real_encode(feats, save=save)
        lv = torch.zeros(B, device=dev)
        w0 = calls[0] * B
        lv[:max(0, min(B, N - w0))] = levels[w0:w0 + B]
        out[0].view(B, d.max_src, d.d_model).copy_((lv[:, None, None] * eos_vec[None, None, :]).to(out[0].dtype))
        calls[0] += 1
        return out
    model.engine.encode = encode
    try:
        kw = dict(batch_size=B, max_new_tokens=bc.MAX_NEW, prompt_ids=PROMPT, eos_token_id=EOS)
        labs = {f"{n}{'_continuous' if c else ''}": PseudoLabeller(model, fe, continuous=c, cross_kv_dtype=dt, **kw)
                for c in (False, True) for n, dt in (("bf16", None), ("fp8", "fp8"))}
        got = {}

        def leg(name):
            def run():
                calls[0] = 0
                return wall_ms(lambda: got.__setitem__(name, labs[name](audios, list(range(N)))[0]))
            return run
        ms = interleaved({n: leg(n) for n in labs}, runs=max(3, RUNS // 2))
        out = {n: {"ms": s, "windows_per_s": N / (s["median"] * 1e-3), "labels_equal_bf16": got[n] == got["bf16"]} for n, s in ms.items()}
        out["windows"] = N
        out["mean_label_length"] = float(np.mean([len(r) for r in got["bf16"]]))
        out["fp8_over_bf16"] = ms["fp8"]["median"] / ms["bf16"]["median"]
        out["fp8_over_bf16_continuous"] = ms["fp8_continuous"]["median"] / ms["bf16_continuous"]["median"]
        return out
    finally:
        model.engine.encode = real_encode


def format_cost(ops):
    """Logits of 8 teacher-forced steps, batch 4, a 2-layer decoder of large-v3's width: FP8 path vs bf16 path (kernels), and the
    bf16 path vs the fp32 torch statement."""
    import torch
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import ParamStore, WhisperDims, WhisperEngine
    from oracle.ref_ops import RefOps
    dims = WhisperDims(1280, 20, 5120, 1, 2, 51866, 128, max_src=1500)
    sd = {k: v.to(torch.bfloat16).float() for k, v in si.random_state_dict(dims, 9, ops.device).items() if k.startswith("model.decoder.")}
    hip = WhisperEngine(ops, ParamStore(ops, dims, sd, trainable=False, decoder_only=True), torch.bfloat16)
    r32 = RefOps(ops.device, lowp=torch.float32)
    ref = WhisperEngine(r32, ParamStore(r32, dims, sd, trainable=False, decoder_only=True), torch.float32)
    B, T, out = 4, 8, {}
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, dims.vocab, (B, T), generator=g).to(ops.device)
    base = torch.randn(B * dims.max_src, dims.d_model, generator=g).to(ops.device)
    like = 4.0 * base
    like[:, 77] *= 30.0
    for name, enc in (("random_normal", base), ("trained_like", like)):
        enc = enc.bfloat16()
        runs = {}
        for leg, eng, kw in (("bf16", hip, {}), ("fp8", hip, dict(cross_kv_dtype="fp8")), ("fp32", ref, {})):
            cache = eng.decode_init(enc.float() if leg == "fp32" else enc, B, T + 1, **kw)
            runs[leg] = torch.stack([eng.decode_step(ids[:, t:t + 1], cache)[:, :dims.vocab].double().clone() for t in range(T)])
        rms = runs["fp32"].pow(2).mean().sqrt()

        def diff(a, b):
            dlt = runs[a] - runs[b]
            return {"rel_rms": float(dlt.pow(2).mean().sqrt() / rms), "max_abs": float(dlt.abs().max()),
                    "argmax_changed": int((runs[a].argmax(-1) != runs[b].argmax(-1)).sum()), "of": B * T}
        out[name] = {"logit_rms": float(rms), "fp8_vs_bf16": diff("fp8", "bf16"), "bf16_vs_fp32_statement": diff("bf16", "fp32"),
                     "fp8_vs_fp32_statement": diff("fp8", "fp32")}
        print("format_cost", name, json.dumps(out[name]), flush=True)
    return out


PROMPT = [50258, 50259, 50360, 50364]
EOS = 50257


def main():
    import torch
    import bench_continuous as bc
    from distil_whisper_amd.build import kernels_sha16
    from distil_whisper_amd.ops_hip import HipOps
    ops = HipOps("cuda:0")
    parent = ParentLib(os.environ["DW_PARENT_LIB"]) if os.environ.get("DW_PARENT_LIB") else None
    res = {"tool": "tools/bench_cross_kv_fp8.py", "device": torch.cuda.get_device_name(0), "kernels_sha16": kernels_sha16(), "runs": RUNS,
           "steps_per_sample": STEPS, "encoder_layers": bc.ENC_LAYERS, "parent_lib": parent is not None,
           "note": "the effect on label quality (WER) is NOT measured: no trained checkpoint is on these machines", "models": {}}
    res["format_cost"] = format_cost(ops)
    only = os.environ.get("BENCH_LAYERS")
    for name, layers in (("distil_large_v3_decoder", 2), ("large_v3_decoder", 32)):
        if only and int(only) != layers:
            continue
        model, eos_vec = bc.planted_model(ops, layers)
        res["models"][name] = {"decoder_layers": layers}
        for B in (16, 64):
            g = torch.Generator().manual_seed(B)
            enc = torch.randn(B * model.dims.max_src, model.dims.d_model, generator=g).to(ops.device).bfloat16()
            row = {}
            row["greedy_step"], caches = greedy_step(ops, model, enc, B, len(PROMPT), parent)
            row["cache_bytes"] = {n: cache_bytes(c) for n, c in caches.items()}
            row["attn_launch"] = attn_launch(ops, model.engine, caches, B, parent)
            row["quant"] = quant_cost(ops, model.engine, caches["fp8"], B)
            del caches
            row["slot_step"] = slot_step(ops, model, enc, B, len(PROMPT))
            torch.cuda.empty_cache()
            row["labeller"] = labeller(ops, model, eos_vec, B)
            res["models"][name][f"batch_{B}"] = row
            print(name, B, json.dumps(row), flush=True)
            torch.cuda.empty_cache()
        del model
        torch.cuda.empty_cache()
        if os.path.isdir(os.path.dirname(OUT)):
            with open(OUT, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    print(OUT)


if __name__ == "__main__":
    main()
