"""The timestamp seek loop on slots next to the lockstep loop on the MI355X -> profiles/seek_slots_bench.json.

`seek_decode(slots=B)` (decoding.SlotDecoder: every window of every utterance is a job of B slots; graphs; optionally FP8
cross-attention K/V) against `seek_decode()` over batches of B utterances -- the call `PseudoLabeller(timestamp_rules=...)` makes
per batch, the parent commit's path, re-measured here -- in ONE process, the legs INTERLEAVED run by run, wall clock around each
call with a device synchronisation on either side, median / min / max of RUNS runs after one warm-up run of each (which captures the
HIP graphs).  The slot legs get all 4 B utterances in one call, as `PseudoLabeller(seek_slots=True, seek_group >= 4)` hands them
over.  The labeller's own log-mel front end is the same on either path and is not part of the measurement.

Set-up of tools/bench_continuous.py: decoder dimensions of distil-large-v3 (2 decoder layers) and of large-v3 (32), d_model 1280,
vocabulary 51 866, bf16, seeded random weights, an ENCODER OF ENC_LAYERS LAYERS (the subject is the token loop), so windows/s is
not the throughput of a full model.

Planted timestamped labels: utterances of 3000 frames.  The decoder's position rows plant (dual vectors of the planted embedding
rows) the sequence

    <0.00>  37 text tokens  <12.00> <12.00>  57 text tokens  <28.00>  EOS            (100 generated tokens)

at level 100 up to the closed pair and 55 behind it; the encoder output of a window is replaced (after the real encoder has run, so
its cost stays) by e W[EOS]: e = 77.5 ends the window behind the closed pair (40 tokens + EOS; the utterance moves 1200 frames), e = 0
lets it run to the single timestamp (the utterance moves past the window).  An utterance's plan says which of its windows are of
which kind: PLANS with proportions PROBS need 1 / 2 / 3 windows.  What was realised is in the file (`windows_per_utterance`).

Per leg: token steps executed, encoder calls with their batch sizes, wall clock, windows/s, and whether the segments equal the
lockstep leg's.  Separately (`slot_step_launches`) the launch time of dw_slot_step_scores against dw_slot_step and of dw_slot_step
through the parent commit's library (DW_PARENT_LIB) against this tree's -- 64 slots, V = 51 866, every slot at a generated step
under the timestamp rules, 20 launches between two events, interleaved -- and the two kernels' device durations from a
kernel-trace run of its own.
Usage:  python tools/bench_seek_slots.py            (BENCH_RUNS=n overrides the 10 runs; BENCH_LAYERS=2 runs one model)
        python tools/bench_seek_slots.py --launches [--keep]      the launch timings alone (--keep: into the file)
        rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_seek_slots.py --launches
        python tools/bench_seek_slots.py --trace DIR/.../..._kernel_stats.csv      merges the statistics into the file
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "seek_slots_bench.json")
RUNS = int(os.environ.get("BENCH_RUNS", "10"))
ENC_LAYERS = 2
INIT = [50258, 50259, 50360]                            # <|startoftranscript|> <|en|> <|transcribe|>
EOS, NOTS, MAX_NEW = 50257, 50364, 128
TB = NOTS + 1
N_TEXT_A, N_TEXT_B = 37, 57
PAIR, LAST = TB + 600, TB + 1400
PAIR_FRAMES = 1200
SEQ = [TB] + [1000 + 7 * i for i in range(N_TEXT_A)] + [PAIR, PAIR] + [2000 + 7 * i for i in range(N_TEXT_B)] + [LAST, EOS]
N_HIGH = 1 + N_TEXT_A + 2                                # positions planted at the high level: up to the closed pair
LEVEL_HIGH, LEVEL_LOW, E_PAIR, E_FULL = 100.0, 55.0, 77.5, 0.0
S_OUT, SCALE = 100.0, 10.0
PLANS = ((0,), (1, 0), (1, 1, 1))                        # kinds of an utterance's windows (1: ends behind the closed pair)
PROBS = (0.5, 0.3, 0.2)
KEY7_DEFAULT = 4


def planted_model(ops, dec_layers):
    import torch
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    d = WhisperDims(1280, 20, 5120, ENC_LAYERS, dec_layers, 51866, 128, max_src=1500, pad_token_id=EOS, decoder_start_token_id=INIT[0])
    sd = {k: v.cpu() for k, v in si.random_state_dict(d, 5, "cpu").items()}
    planted = sorted(set(SEQ))
    Es = sd["model.decoder.embed_tokens.weight"].double()[planted]
    W = torch.linalg.solve(Es @ Es.T, Es)               # dual vectors: W @ Es.T = I
    dual = {t: W[i] for i, t in enumerate(planted)}
    pos = sd["model.decoder.embed_positions.weight"].clone()
    for i, t in enumerate(SEQ):
        pos[len(INIT) - 1 + i] = ((LEVEL_HIGH if i < N_HIGH else LEVEL_LOW) * SCALE * dual[t]).to(pos.dtype)
    sd["model.decoder.embed_positions.weight"] = pos
    p = f"model.decoder.layers.{dec_layers - 1}.encoder_attn"
    eye = torch.eye(d.d_model)
    sd[f"{p}.v_proj.weight"], sd[f"{p}.v_proj.bias"] = eye.clone(), torch.zeros(d.d_model)
    sd[f"{p}.out_proj.weight"], sd[f"{p}.out_proj.bias"] = S_OUT * eye, torch.zeros(d.d_model)
    model = WhisperForConditionalGeneration(d, ops=ops, state_dict=sd, dtype=torch.bfloat16)
    return model, (SCALE / S_OUT * dual[EOS]).float().to(ops.device)


def stats(xs):
    xs = sorted(xs)
    med = xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2])
    return {"median": med, "min": xs[0], "max": xs[-1], "max_minus_min": xs[-1] - xs[0]}


def leg(ops, model, eos_vec, B, results):
    import numpy as np
    import torch
    from distil_whisper_amd.decoding import GreedyDecoder
    dev, d = ops.device, model.dims
    U = 4 * B
    rng = np.random.default_rng(B)
    plan = [PLANS[k] for k in rng.choice(len(PLANS), size=U, p=PROBS)]
    feats = 0.1 * torch.randn((U, d.n_mels, 3000), generator=torch.Generator().manual_seed(B))
    feats[:, 1] = torch.arange(U, dtype=torch.float32)[:, None]                  # channel 1: the utterance, channel 2: the frame
    feats[:, 2] = torch.arange(3000, dtype=torch.float32)[None, :]
    feats = feats.to(dev)
    real_encode, enc_calls = model.engine.encode, []

    def encode(f, save=False):
        out = real_encode(f, save=save)                           # the encoder runs; its output is replaced by the planted rows
        head = f[:, 1:3, 0].round().long().tolist()
        lv = torch.tensor([E_PAIR if plan[u][min(t // PAIR_FRAMES, len(plan[u]) - 1)] else E_FULL for u, t in head], device=dev)
        n = len(head)
        out[0][:n * d.max_src].view(n, d.max_src, d.d_model).copy_((lv[:, None, None] * eos_vec[None, None, :]).to(out[0].dtype))
        enc_calls.append(n)
        return out
    model.engine.encode = encode
    n_steps = [0]
    run_step = GreedyDecoder._run_step

    def counted(self, *a, **k):
        n_steps[0] += 1
        return run_step(self, *a, **k)
    GreedyDecoder._run_step = counted
    sup = [NOTS - 1, NOTS - 2]
    args = lambda f: (f, [3000] * f.shape[0], [INIT] * f.shape[0], lambda P: (MAX_NEW, 0), EOS, EOS, NOTS, 50)

    def lockstep(**kw):
        out = []
        for b0 in range(0, U, B):
            out += model.seek_decode(*args(feats[b0:b0 + B]), suppress_tokens=sup, **kw)
        return out

    def slots(ce, fp8=False, **kw):
        return model.seek_decode(*args(feats), suppress_tokens=sup, slots=B, check_every=ce, cross_kv_dtype="fp8" if fp8 else None, **kw)
    th = dict(logprob_threshold=-1.0, no_speech_threshold=0.6)
    legs = {"lockstep": lockstep, "slots_ce4": lambda: slots(4), "slots_ce8": lambda: slots(8), "slots_ce4_fp8": lambda: slots(4, True),
            "slots_ce8_fp8": lambda: slots(8, True), "lockstep_thresholds": lambda: lockstep(**th),
            "slots_ce8_thresholds": lambda: slots(8, **th)}
    try:
        ms, info, segs = {n: [] for n in legs}, {}, {}
        # two interleaved groups: four slot decoders (caches and graphs) are kept alive here, the thresholds need a fifth
        model.seek_slot_decoders_max = 4
        groups = ([n for n in legs if not n.endswith("thresholds")], [n for n in legs if n.endswith("thresholds")])
        for names, r in [(g, r) for g in groups for r in range(RUNS + 1)]:      # run 0: warm-up (graph capture), not kept
            print(f"batch {B}: run {r} of {', '.join(names)}", flush=True)
            for name in names:
                fn = legs[name]
                del enc_calls[:]
                n_steps[0] = 0
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = fn()
                torch.cuda.synchronize()
                t = (time.perf_counter() - t0) * 1e3
                if r:
                    ms[name].append(t)
                steps = model.last_seek_stats["steps"] if name.startswith("slots") else n_steps[0]
                info[name] = {"token_steps": steps, "encoder_calls": len(enc_calls), "encoder_batch_sizes": list(enc_calls),
                              "windows": sum(enc_calls)}
                segs[name] = [[(s["start"], s["end"], list(s["tokens"])) for s in row] for row in got]
        row = {"utterances": U, "plan_seed": B,        # (numpy default_rng(B).choice over PLANS with PROBS)
               "windows_per_utterance": {str(k): sum(1 for p in plan if len(p) == k) for k in (1, 2, 3)}, "legs": {}}
        for name in legs:
            st = stats(ms[name])
            ref = "lockstep_thresholds" if name.endswith("thresholds") else "lockstep"
            sizes = info[name].pop("encoder_batch_sizes")
            row["legs"][name] = dict(info[name], ms=st, windows_per_s=info[name]["windows"] / (st["median"] * 1e-3),
                                     encoder_batch_sizes={str(k): sizes.count(k) for k in sorted(set(sizes))},
                                     segments_equal_lockstep=segs[name] == segs[ref],
                                     time_over_lockstep=st["median"] / stats(ms[ref])["median"])
            print(B, name, json.dumps(row["legs"][name]), flush=True)
        results[f"batch_{B}"] = row
    finally:
        model.engine.encode = real_encode
        GreedyDecoder._run_step = run_step


def slot_step_launches(ops):
    """dw_slot_step_scores against dw_slot_step, and dw_slot_step through the parent commit's library (DW_PARENT_LIB=<libdwamd.so
    built from the parent, tools/build_base_lib.sh>) against this tree's: 64 slots, V = 51 866, every slot at a generated step under
    the timestamp rules.  A sample is BATCH launches between two events (the slots walk from position 8 to 8 + BATCH, none ends;
    the state is put back before every sample), divided by BATCH; 60 samples per leg after 5 warm-up samples, legs interleaved
    sample by sample."""
    import ctypes as C
    import torch
    from distil_whisper_amd import ops_hip as oh
    dev, S, V, ld, BATCH = ops.device, 64, 51866, 51868, 20
    g = torch.Generator().manual_seed(1)
    lg = (2.0 * torch.randn((S, ld), generator=g)).bfloat16().to(dev)
    tokens0 = torch.full((S, 32), 1000, dtype=torch.long)
    tokens0[:, :3] = torch.tensor(INIT)
    tokens0[:, 3] = TB
    tokens0 = tokens0.to(dev)
    state0 = torch.tensor([[8] * S, [3] * S, [31] * S, [0] * S, [0] * S], dtype=torch.int32, device=dev)
    tokens, state = tokens0.clone(), state0.clone()
    done, cur = torch.zeros(S, dtype=torch.bool, device=dev), torch.zeros((S, 1), dtype=torch.long, device=dev)
    sc = torch.zeros((2, S), dtype=torch.float32, device=dev)
    kw = dict(ts_begin=TB, max_initial=50, eos=EOS)
    legs = {"dw_slot_step": lambda: ops.slot_step(lg, V, tokens, state[0], state[1], state[2], done, state[3], cur, **kw),
            "dw_slot_step_scores": lambda: ops.slot_step(lg, V, tokens, state[0], state[1], state[2], done, state[3], cur, lp_sum=sc[0],
                                                         nsp=sc[1], nsp_pos=state[4], nsp_col=NOTS - 1, **kw)}
    if os.environ.get("DW_PARENT_LIB"):
        parent = C.CDLL(os.environ["DW_PARENT_LIB"])
        parent.dw_slot_step.argtypes, parent.dw_slot_step.restype = oh._SIGS["dw_slot_step"]
        p = lambda t: t.data_ptr()

        def through_parent():
            rc = parent.dw_slot_step(p(lg), S, V, ld, None, None, TB, 50, EOS, 0, p(tokens), tokens.stride(0), p(state[0]), p(state[1]),
                                     p(state[2]), p(done), p(state[3]), p(cur), ops._stream())
            assert rc == 0
        legs["dw_slot_step_parent_library"] = through_parent
    times = {n: [] for n in legs}
    for i in range(65):
        for name, launch in legs.items():
            tokens.copy_(tokens0); state.copy_(state0); done.zero_()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(BATCH):
                launch()
            e1.record()
            e1.synchronize()
            assert int(state[0][0]) == 8 + BATCH and not bool(done.any())
            if i >= 5:
                times[name].append(e0.elapsed_time(e1) * 1e3 / BATCH)
    out = {n: stats(t) for n, t in times.items()}
    out["unit"] = f"us per launch ({BATCH} launches between two events)"
    out["scores_over_plain"] = out["dw_slot_step_scores"]["median"] / out["dw_slot_step"]["median"]
    if "dw_slot_step_parent_library" in out:
        out["this_tree_over_parent_library"] = out["dw_slot_step"]["median"] / out["dw_slot_step_parent_library"]["median"]
    return out


def kernel_trace(csv_path):
    """The two instantiations' device durations from the kernel statistics of a kernel-trace run of `--launches` (a run of its
    own: `rocprofv3 --kernel-trace --stats -- python tools/bench_seek_slots.py --launches`)."""
    import csv
    out = {}
    with open(csv_path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name", "")
            if "slot_step_kernel" in name:
                key = "slot_step_kernel<true>" if "ILb1E" in name or "<true>" in name else "slot_step_kernel<false>"
                e = out.setdefault(key, {"calls": 0, "total_ns": 0.0})
                e["calls"] += int(row["Calls"])
                e["total_ns"] += float(row["TotalDurationNs"])
    for e in out.values():
        e["average_us"] = e["total_ns"] / e["calls"] / 1e3
    if len(out) == 2:
        out["true_over_false"] = out["slot_step_kernel<true>"]["average_us"] / out["slot_step_kernel<false>"]["average_us"]
    out["note"] = "device durations over all launches of the run (warm-up samples included), without DW_PARENT_LIB"
    return out


def update(key, value):
    out = os.environ.get("BENCH_OUT", OUT)
    with open(out) as f:
        res = json.load(f)
    res[key] = value
    write(res, out)


def write(res, out):
    with open(out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


def main():
    import torch
    from distil_whisper_amd.build import kernels_sha16
    from distil_whisper_amd.ops_hip import HipOps
    if "--trace" in sys.argv:                             # merge a kernel-trace run's statistics into the file
        tr = kernel_trace(sys.argv[sys.argv.index("--trace") + 1])
        print(json.dumps(tr))
        return update("slot_step_kernel_trace", tr)
    ops = HipOps("cuda:0")
    if "--launches" in sys.argv:                          # the launch timings alone (also the program of the kernel-trace run)
        la = slot_step_launches(ops)
        print(json.dumps(la), flush=True)
        if "--keep" in sys.argv:
            update("slot_step_launch", la)
        return
    res = {"tool": "tools/bench_seek_slots.py", "device": torch.cuda.get_device_name(0), "kernels_sha16": kernels_sha16(), "runs": RUNS,
           "encoder_layers": ENC_LAYERS, "max_new_tokens": MAX_NEW,
           "planted": {"generated_tokens_full_window": len(SEQ), "generated_tokens_pair_window": N_HIGH + 1, "pair_frames": PAIR_FRAMES,
                       "plans": PLANS, "probabilities": PROBS},
           "note": "windows_per_s is with a 2-layer encoder; lockstep = seek_decode over batches of B utterances (the labeller's call), "
                   "slots = one seek_decode(slots=B) over all 4 B utterances",
           "slot_step_launch": slot_step_launches(ops), "models": {}}
    print(json.dumps(res["slot_step_launch"]), flush=True)
    only = os.environ.get("BENCH_LAYERS")
    for name, layers in (("distil_large_v3_decoder", 2), ("large_v3_decoder", 32)):
        if only and int(only) != layers:
            continue
        model, eos_vec = planted_model(ops, layers)
        res["models"][name] = {"decoder_layers": layers}
        for B in (16, 64):
            leg(ops, model, eos_vec, B, res["models"][name])
        del model
        torch.cuda.empty_cache()
        out = os.environ.get("BENCH_OUT", OUT)
        if os.path.isdir(os.path.dirname(out)):
            write(res, out)
    print(OUT)


if __name__ == "__main__":
    main()
