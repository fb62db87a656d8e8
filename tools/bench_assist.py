"""What one round of speculative (assisted) greedy decoding costs on the MI355X with the round as kernels and as torch ops, next to
the target's plain token step -> profiles/assist_bench.json.

Target: large-v3 decoder dimensions (32 decoder layers, d_model 1280, 20 heads, vocabulary 51 866; one encoder layer, the encoder is
not run), bf16.  Assistant: a decoder-only `WhisperForCausalLM` with 2 layers.  Seeded random weights, num_assistant_tokens = 5,
batch 1 and 4, ROUNDS new tokens per run (no EOS id, so no run ends early; random drafts are rejected, so as many rounds),
everything in ONE process.  Per batch the two paths of decoding.assisted_greedy_decode on the same engines and encoder output, their runs INTERLEAVED
(a, b, a, b, ...), HIP events around each run, median / min / max of 10 runs after 2 warm-up runs:
  (a) `assist_kernels`: per round k x dw_assist_pick(store) + dw_assist_pick(k + 1) + dw_assist_accept, `result` read once;
  (b) `assist_torch`:   DW_ASSIST_TORCH=1, `assist_pick_torch` / `assist_accept_torch` -- the parent commit's round.
Launches and host synchronisations per round come from torch's profiler over one run of each path.  In the same process the
target's plain graph-replayed token step (`GreedyDecoder`, 64 new tokens) is timed the same way.  Per leg: the time of one round,
and the break-even acceptance a* with round_time / (a* + 1) = plain token-step time: a round pays when it accepts more than a*
of its 5 drafts.  Random weights accept almost nothing (the observed count is recorded), and no trained checkpoint is at hand: the
acceptance rate of real models, and with it any end-to-end speed-up, is NOT measured here.  The memory figure is the device memory
of a full 2-layer student of the same dimensions with the large-v3 encoder (32 layers) minus that of the decoder-only assistant,
from the sizes of the flat stores (fp32 master + bf16 shadow + packed convolution weights).
Usage:  python tools/bench_assist.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "assist_bench.json")
K, P, PLAIN_NEW = 5, 4, 64
ROUNDS = 40                                              # new tokens of a run; random drafts are rejected, so about as many rounds
#                                                          (the last 5 draft fewer than 5 tokens: the sequence ends)


def interleaved(legs, warm=2, reps=10):
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


def counted(fn):
    """(kernel launches, host synchronisations) of one call, from torch's profiler."""
    import torch
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    launches = syncs = 0
    for ev in prof.events():
        name = ev.name
        if "LaunchKernel" in name or "hipModuleLaunchKernel" in name or "hipExtLaunchKernel" in name:
            launches += 1
        elif name in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize") or \
                (name.startswith("hipMemcpy") and "Async" not in name):
            syncs += 1
    return launches, syncs


def store_bytes(store):
    n = store.P.numel() * 4 + store.S.numel() * 2
    for t in (store.conv1_packed, store.conv2_packed):
        n += 0 if t is None else t.numel() * 2
    return n


def batch(target, assistant, ops, B):
    import torch
    from distil_whisper_amd import decoding
    eng, d, dev = target.engine, target.dims, ops.device
    g = torch.Generator().manual_seed(B)
    enc = (torch.randn(B, d.max_src, d.d_model, generator=g) * 0.5).to(dev).reshape(-1, d.d_model).to(eng.lowp).contiguous()
    ids = torch.tensor([[50258, 50259, 50360, 50364]] * B, device=dev)
    stats = {}

    def run(torch_path):
        before = os.environ.get(decoding.ASSIST_TORCH_ENV)
        os.environ[decoding.ASSIST_TORCH_ENV] = "1" if torch_path else "0"
        try:
            # (max_new_tokens bounds the rounds from above: a round emits accepted + 1 tokens; the rounds are counted below)
            out = decoding.assisted_greedy_decode(eng, assistant.engine, enc, enc, ids, ROUNDS, K)
            stats["torch" if torch_path else "kernels"] = out
            return out
        finally:
            if before is None:
                del os.environ[decoding.ASSIST_TORCH_ENV]
            else:
                os.environ[decoding.ASSIST_TORCH_ENV] = before
    legs = {"assist_kernels": lambda: run(False), "assist_torch": lambda: run(True)}
    a, b = legs["assist_kernels"](), legs["assist_torch"]()
    res = {"batch": B, "num_assistant_tokens": K, "new_tokens": ROUNDS, "prompt_tokens": P, "vocab": d.vocab,
           "sanity": {"same_tokens_as_torch_path": bool(a[0].shape == b[0].shape and (a[0] == b[0]).all()),
                      "drafted": a[1], "accepted": a[2], "drafted_torch": b[1], "accepted_torch": b[2]}}
    # rounds of a run: every round but the last drafts K tokens (the last rounds draft fewer: total - L - 1)
    rounds = {"assist_kernels": None, "assist_torch": None}
    for leg, out in (("assist_kernels", a), ("assist_torch", b)):
        rounds[leg] = ROUNDS - out[2]                    # one round per emitted token that was not an accepted draft
    res.update(interleaved(legs))
    dec = decoding.GreedyDecoder(eng, B, P + PLAIN_NEW)
    plain = interleaved({"plain_greedy": lambda: dec.run(enc, ids, PLAIN_NEW)})["plain_greedy"]
    plain["new_tokens"] = PLAIN_NEW
    plain["token_step_ms"] = plain["median_ms"] / (P - 1 + PLAIN_NEW)     # (the prompt is fed token by token as well)
    res["plain_greedy"] = plain
    for name, fn in legs.items():
        n_launch, n_sync = counted(fn)
        r = rounds[name]
        res[name].update(rounds=r, round_ms=res[name]["median_ms"] / r, round_spread_ms=res[name]["spread_ms"] / r,
                         launches_per_round=n_launch / r, host_syncs_per_round=n_sync / r)
        res[name]["break_even_accepted_per_round"] = res[name]["round_ms"] / plain["token_step_ms"] - 1.0
    res["torch_minus_kernels_ms_per_round"] = res["assist_torch"]["round_ms"] - res["assist_kernels"]["round_ms"]
    res["kernel_round_slower_beyond_spread"] = bool(
        res["assist_kernels"]["round_ms"] - res["assist_torch"]["round_ms"] >
        max(res["assist_kernels"]["round_spread_ms"], res["assist_torch"]["round_spread_ms"]))
    return res


def main():
    import dataclasses
    import torch
    sys.path.insert(0, ROOT)
    from distil_whisper_amd import build
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForCausalLM, WhisperForConditionalGeneration
    from distil_whisper_amd.ops_hip import HipOps
    dev = "cuda:0"
    ops = HipOps(dev)
    dims = WhisperDims(1280, 20, 5120, 1, 32, 51866, 128, decoder_start_token_id=50258)
    target = WhisperForConditionalGeneration(dims, ops=ops, seed=0, dtype=torch.bfloat16)
    assistant = WhisperForCausalLM(dataclasses.replace(dims, dec_layers=2), ops=ops, seed=1, dtype=torch.bfloat16)
    # memory: what a full student of the same dimensions (the large-v3 encoder, 32 layers) keeps on the device on top of the decoder:
    # fp32 master + bf16 shadow of every encoder tensor and the two packed convolution weights (entries are padded to 64 elements:
    # not counted)
    D, Fd, nm = dims.d_model, dims.ffn, dims.n_mels
    enc_elems = D * nm * 3 + D + D * D * 3 + D + dims.max_src * D + 32 * (4 * D * D + 4 * D + 2 * D + 2 * Fd * D + Fd + D + 2 * D) + 2 * D
    enc_bytes = enc_elems * 6 + (D * ((3 * nm + 63) // 64 * 64) + D * 3 * D) * 2
    full_bytes = store_bytes(assistant.store) + enc_bytes
    results = {"kernels_sha16": build.kernels_sha16(),
               "protocol": "one process; per batch the two paths run interleaved, HIP events around each run, median of 10 runs "
                           "after 2 warm-up runs; spread_ms = max - min of the 10; round_ms = median_ms / rounds",
               "not_measured": "random weights accept almost no draft and no trained checkpoint is available: the acceptance "
                               "rate of real models and any end-to-end speed-up are NOT measured; break_even_accepted_per_round is "
                               "what a model pair must exceed for a round to pay",
               "assistant_memory": {"decoder_only_bytes": store_bytes(assistant.store), "full_student_bytes": full_bytes,
                                    "saved_bytes": full_bytes - store_bytes(assistant.store)},
               "batches": [batch(target, assistant, ops, B) for B in (1, 4)]}
    torch.cuda.synchronize()
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
