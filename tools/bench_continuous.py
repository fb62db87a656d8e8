"""Pseudo-labelling with continuous batching next to the batch path on the MI355X -> profiles/continuous_bench.json.

`PseudoLabeller(continuous=True)` (decoding.SlotDecoder: a pack whose labels have ended hands its row of the token loop to the next
waiting pack) against `PseudoLabeller()` (decoding.GreedyDecoder: a batch runs until its longest row has produced EOS -- the parent
commit's path, re-measured here), in ONE process, their runs INTERLEAVED (batch, continuous, batch, continuous, ...), wall clock
around each call with a device synchronisation on either side, median / min / max of RUNS runs after one warm-up run of each (which
captures the HIP graphs).

Models: decoder dimensions of distil-large-v3 (2 decoder layers) and of large-v3 (32 decoder layers), d_model 1280, 20 heads,
vocabulary 51 866, bf16, seeded random weights.  The ENCODER HAS ENC_LAYERS LAYERS, not 32: the subject is the token loop; the
encoder's cost per window is the same on both paths and is measured alone (`encode_ms`) and subtracted for `ms_per_step`.  So
`windows_per_s` here is NOT the pseudo-labelling throughput of a full model.

Planted label lengths: the windows' lengths are planted, not learnt.  Position row P - 1 + i of the decoder holds c_i W[t_i] (W: dual
vectors of the planted embedding rows, tests/assist_rows_cases.planted_pair's construction), c_i a staircase LEVELS over the
generated positions; the encoder output of window w is replaced (after the real encoder has run, so its cost stays) by e_w W[EOS] at
every source position, which the last decoder layer's cross-attention (v_proj = I, out_proj = s I) adds to the stream: the window
emits t_i while c_i > e_w and EOS at the first position of the stair below e_w.  PLANNED lengths (generated tokens, EOS included)
LENGTHS with probabilities PROBS: mean 80.6 = 63 % of the longest (128).  The REALISED lengths are whatever the random layers leave
of that and are written to the file per leg, with `labels_equal` (continuous against batch path).

Legs: batch 16 and 64, 4 batches of windows each, `check_every` 4 / 8 / 16 of the continuous path (the batch path keeps its own 16);
at check_every 8 a third path runs the continuous loop under dw_debug_set(7, 0) -- the per-row self-attention with its projection
inside (dw_decode_attn_proj_rows); under the default key (4) the rows pass runs the QKV GEMM, the append and attn_rows_kernel.
Outputs per path: windows/s, token steps executed, ms per token step (wall clock minus `encode_ms`, over the steps).
No speed-up is claimed in advance: the file holds what came out.
Usage:  python tools/bench_continuous.py            (BENCH_RUNS=n overrides the 10 runs)
"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "profiles", "continuous_bench.json")
RUNS = int(os.environ.get("BENCH_RUNS", "10"))
ENC_LAYERS = 2
PROMPT = [50258, 50259, 50360, 50364]
EOS, MAX_NEW = 50257, 128
LENGTHS = (32, 52, 76, 100, 128)                       # generated tokens, EOS included (128: the budget, no EOS)
PROBS = (0.10, 0.20, 0.30, 0.25, 0.15)
LEVELS = (100.0, 85.0, 70.0, 55.0, 40.0)               # c_i over the stairs [0, 31), [31, 51), [51, 75), [75, 99), [99, 128)
EOS_LEVELS = (92.5, 77.5, 62.5, 47.5, 0.0)             # e_w of a window planned to end at LENGTHS[k]
S_OUT, SCALE = 100.0, 10.0


def planted_model(ops, dec_layers):
    import torch
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    d = WhisperDims(1280, 20, 5120, ENC_LAYERS, dec_layers, 51866, 128, max_src=1500, pad_token_id=EOS, decoder_start_token_id=PROMPT[0])
    sd = {k: v.cpu() for k, v in si.random_state_dict(d, 5, "cpu").items()}
    seq = [1000 + 7 * i for i in range(MAX_NEW)]
    planted = seq + [EOS]
    Es = sd["model.decoder.embed_tokens.weight"].double()[planted]
    W = torch.linalg.solve(Es @ Es.T, Es)              # dual vectors: W @ Es.T = I
    pos = sd["model.decoder.embed_positions.weight"].clone()
    stairs = [0] + [n - 1 for n in LENGTHS[:-1]] + [MAX_NEW]
    for i in range(MAX_NEW):
        k = max(j for j in range(len(LEVELS)) if stairs[j] <= i)
        pos[len(PROMPT) - 1 + i] = (LEVELS[k] * SCALE * W[i]).to(pos.dtype)
    sd["model.decoder.embed_positions.weight"] = pos
    p = f"model.decoder.layers.{dec_layers - 1}.encoder_attn"
    eye = torch.eye(d.d_model)
    sd[f"{p}.v_proj.weight"], sd[f"{p}.v_proj.bias"] = eye.clone(), torch.zeros(d.d_model)
    sd[f"{p}.out_proj.weight"], sd[f"{p}.out_proj.bias"] = S_OUT * eye, torch.zeros(d.d_model)
    model = WhisperForConditionalGeneration(d, ops=ops, state_dict=sd, dtype=torch.bfloat16)
    return model, (SCALE / S_OUT * W[-1]).float().to(ops.device)


def stats(xs):
    xs = sorted(xs)
    return {"median": xs[len(xs) // 2] if len(xs) % 2 else 0.5 * (xs[len(xs) // 2 - 1] + xs[len(xs) // 2]), "min": xs[0], "max": xs[-1]}


def leg(ops, model, eos_vec, B, results):
    import numpy as np
    import torch
    from distil_whisper_amd.decoding import GreedyDecoder
    from distil_whisper_amd.modeling import WhisperFeatureExtractor
    from distil_whisper_amd.pseudo_label import PseudoLabeller
    dev, d = ops.device, model.dims
    N = 4 * B
    rng = np.random.default_rng(B)
    kinds = rng.choice(len(LENGTHS), size=N, p=PROBS)
    levels = torch.tensor([EOS_LEVELS[k] for k in kinds], dtype=torch.float32, device=dev)
    audios = [0.1 * rng.standard_normal(16000).astype(np.float32) for _ in range(N)]      # one second each, a pack per sample
    speakers = list(range(N))
    fe = WhisperFeatureExtractor(feature_size=d.n_mels, ops=ops)
    real_encode, calls = model.engine.encode, [0]

    def encode(feats, save=False):
        out = real_encode(feats, save=save)                        # the encoder runs; its output is replaced by the planted rows
        lv = torch.zeros(B, device=dev)
        w0 = calls[0] * B
        lv[:max(0, min(B, N - w0))] = levels[w0:w0 + B]
        out[0].view(B, d.max_src, d.d_model).copy_((lv[:, None, None] * eos_vec[None, None, :]).to(out[0].dtype))
        calls[0] += 1
        return out
    model.engine.encode = encode
    n_steps = [0]
    run_step = GreedyDecoder._run_step

    def counted(self, *a, **k):
        n_steps[0] += 1
        return run_step(self, *a, **k)
    GreedyDecoder._run_step = counted
    kw = dict(batch_size=B, max_new_tokens=MAX_NEW, prompt_ids=PROMPT, eos_token_id=EOS)
    try:
        def timed(fn):
            calls[0] = 0
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            out = fn()
            torch.cuda.synchronize()
            return (time.perf_counter() - t0) * 1e3, out
        plain = PseudoLabeller(model, fe, **kw)
        ref = plain(audios, speakers)[0]                            # warm-up: captures the per-position graphs
        n_steps[0] = 0
        plain(audios, speakers)
        batch_steps = n_steps[0]
        lens = [min(len(r) + 1, MAX_NEW) for r in ref]             # generated tokens, EOS included
        # the encoder stage alone, the way both paths run it
        enc_ms = []
        for _ in range(max(3, RUNS // 2)):
            def enc_only():
                for b0 in range(0, N, B):
                    plain._wave.zero_()
                    model.engine.encode(ops.logmel(plain._wave, fe._filt), save=False)
            enc_ms.append(timed(enc_only)[0])
        enc_med = stats(enc_ms)["median"]
        out = {"windows": N, "planned_lengths": [int(LENGTHS[k]) for k in kinds], "realised_lengths": lens,
               "realised_mean_over_longest": float(np.mean(lens) / max(lens)), "encode_ms": stats(enc_ms), "check_every": {}}
        for ce in (4, 8, 16):
            paths = {"batch_path": (plain, None), "continuous": (PseudoLabeller(model, fe, continuous=True, check_every=ce, **kw), KEY7_DEFAULT)}
            if ce == 8:
                paths["continuous_key7_0"] = (PseudoLabeller(model, fe, continuous=True, check_every=ce, **kw), 0)
            ms, steps, equal = {n: [] for n in paths}, {}, {}
            for r in range(RUNS + 1):                               # run 0: warm-up (graph capture), not kept
                for name, (lab, key) in paths.items():
                    if key is not None:
                        ops.lib.dw_debug_set(7, key)
                    s0 = lab.slot_decoder.steps if key is not None else 0
                    n_steps[0] = 0
                    t, got = timed(lambda: lab(audios, speakers)[0])
                    ops.lib.dw_debug_set(7, KEY7_DEFAULT)
                    steps[name] = lab.slot_decoder.steps - s0 if key is not None else n_steps[0]
                    equal[name] = got == ref
                    if r:
                        ms[name].append(t)
            row = {}
            for name in paths:
                st = stats(ms[name])
                row[name] = {"ms": st, "token_steps": steps[name], "windows_per_s": N / (st["median"] * 1e-3),
                             "ms_per_step": (st["median"] - enc_med) / steps[name], "labels_equal": bool(equal[name])}
            row["steps_ratio"] = steps["continuous"] / steps["batch_path"]
            row["time_ratio"] = row["continuous"]["ms"]["median"] / row["batch_path"]["ms"]["median"]
            out["check_every"][str(ce)] = row
            print(B, ce, json.dumps(row), flush=True)
        assert batch_steps == out["check_every"]["4"]["batch_path"]["token_steps"]
        results[f"batch_{B}"] = out
    finally:
        model.engine.encode = real_encode
        GreedyDecoder._run_step = run_step
        ops.lib.dw_debug_set(7, KEY7_DEFAULT)


KEY7_DEFAULT = 4


def main():
    import torch
    from distil_whisper_amd.build import kernels_sha16
    from distil_whisper_amd.ops_hip import HipOps
    ops = HipOps("cuda:0")
    res = {"tool": "tools/bench_continuous.py", "device": torch.cuda.get_device_name(0), "kernels_sha16": kernels_sha16(), "runs": RUNS,
           "encoder_layers": ENC_LAYERS, "max_new_tokens": MAX_NEW, "prompt_length": len(PROMPT),
           "planted": {"lengths": LENGTHS, "probabilities": PROBS, "planned_mean_over_longest": sum(l * p for l, p in zip(LENGTHS, PROBS)) / max(LENGTHS),
                       "stair_levels": LEVELS, "eos_levels": EOS_LEVELS},
           "note": "windows_per_s is with a 2-layer encoder; ms_per_step = (median ms - encode_ms median) / token steps", "models": {}}
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
        if os.path.isdir(os.path.dirname(OUT)):
            with open(OUT, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")
    print(OUT)


if __name__ == "__main__":
    main()
