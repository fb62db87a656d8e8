"""What `generate(num_beams=5)` costs on the MI355X with the beam step as kernels and as torch ops -> profiles/beam_bench.json.

distil-large-v3 decoder dimensions (2 decoder layers, d_model 1280, 20 heads, vocabulary 51 866), seeded weights, 5 beams, 16 and
64 utterances (80 / 320 decoder rows), 220 steps forced by min_new_tokens = max_new_tokens, everything in ONE process.  Per batch
the two paths of decoding.beam_search_decode on the same engine and encoder output, their runs INTERLEAVED (a, b, a, b, ...), HIP
events around each run, median / min / max of 10 rounds after 2 warm-up rounds:
  (a) `beam_kernels`: dw_beam_candidates + dw_beam_update per step, the loop condition read every 4 steps;
  (b) `beam_torch`:   DW_BEAM_TORCH=1, `decoding.beam_step_torch`, the loop condition read every step.  (This is the torch step as
      it is now: against the parent's it has lost two host synchronisations per step and gained the tie-ordering sorts and gathers
      on [B, 4k] tensors, about ten small launches.  The parent's own step was not timed.)
Launches and host synchronisations per step are counted with torch's profiler over one run of each path (kernel launches and
`hipStreamSynchronize` / `hipMemcpy` calls with a device-to-host copy); the two entries alone are timed between two events over
200 launches on the state and logits of step 110, next to the bytes each must move (candidates: the R x V bf16 logits once;
update: the candidates and the R token rows of `running` and `sequences`, read and written).  The `beam_update` figure is the whole
entry call -- the deciding launch and the row move -- plus this tool's one small reset copy; per-kernel times come from a
kernel-trace run of their own (profiles/beam_kernel_trace.json).  Nothing is promised here: the file records what was measured.
Usage:  python tools/bench_beam.py
"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "beam_bench.json")
NEW, P, K_BEAMS = 220, 4, 5
EOS = 50257


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


def batch(model, ops, B, suppress, begin_suppress):
    import torch
    from distil_whisper_amd import decoding
    eng, d, dev = model.engine, model.dims, ops.device
    g = torch.Generator().manual_seed(B)
    enc = (torch.randn(B, d.max_src, d.d_model, generator=g) * 0.5).to(dev).reshape(-1, d.d_model).to(eng.lowp).contiguous()
    ids = torch.tensor([[50258, 50259, 50360, 50364]] * B, device=dev)
    k, R, V = K_BEAMS, B * K_BEAMS, d.vocab
    res = {"utterances": B, "beams": k, "rows": R, "new_tokens": NEW, "prompt_tokens": P, "vocab": V}

    def run(torch_path):
        before = os.environ.get(decoding.BEAM_TORCH_ENV)
        os.environ[decoding.BEAM_TORCH_ENV] = "1" if torch_path else "0"
        try:
            return decoding.beam_search_decode(eng, enc, ids, NEW, k, EOS, pad_token_id=EOS, suppress_tokens=suppress,
                                               begin_suppress_tokens=begin_suppress, min_new_tokens=NEW, return_scores=True)
        finally:
            if before is None:
                del os.environ[decoding.BEAM_TORCH_ENV]
            else:
                os.environ[decoding.BEAM_TORCH_ENV] = before
    legs = {"beam_kernels": lambda: run(False), "beam_torch": lambda: run(True)}
    a, b = legs["beam_kernels"](), legs["beam_torch"]()
    res["sanity"] = {"rows_equal_to_torch_path": int((a[0] == b[0]).all(1).sum()),
                     "max_score_difference": float((a[1] - b[1]).abs().max())}
    res.update(interleaved(legs))
    for name, fn in legs.items():
        n_launch, n_sync = counted(fn)
        res[name].update(launches_per_step=n_launch / NEW, host_syncs_per_step=n_sync / NEW)
    res["torch_minus_kernels_ms"] = res["beam_torch"]["median_ms"] - res["beam_kernels"]["median_ms"]
    res["torch_minus_kernels_us_per_step"] = res["torch_minus_kernels_ms"] * 1e3 / NEW
    res["kernel_path_is_faster"] = bool(res["beam_kernels"]["median_ms"] < res["beam_torch"]["median_ms"])
    # the two entries alone, on the state of step 110 of the kernel run
    cur, L = P + NEW // 2, P + NEW
    running = torch.full((B, k, L), EOS, dtype=torch.long, device=dev)
    running[:, :, :cur] = a[0][:, None, :cur]
    other, seqs, seqs2 = running.clone(), running.clone(), running.clone()
    logits = (torch.randn(R, (V + 63) // 64 * 64, generator=g) * 1.5).to(dev).bfloat16()
    run_scores = -torch.rand(B, k, device=dev).cumsum(1) - 100.0
    st = dict(beam_scores=torch.full((B, k), -1.0e9, device=dev), finished=torch.zeros((B, k), dtype=torch.bool, device=dev),
              lengths=torch.zeros((B, k), dtype=torch.int32, device=dev), unsat=torch.ones(B, dtype=torch.bool, device=dev))
    cand_val = torch.empty((R, 2 * k), dtype=torch.float32, device=dev)
    cand_tok = torch.empty((R, 2 * k), dtype=torch.int32, device=dev)
    stop = torch.zeros(1, dtype=torch.int32, device=dev)
    src_rows, next_tok = torch.zeros(R, dtype=torch.long, device=dev), torch.zeros(R, dtype=torch.long, device=dev)
    plan = torch.empty(4 * R, dtype=torch.int32, device=dev)
    sup = torch.zeros(V, dtype=torch.uint8)
    sup[list(suppress)] = 1
    sup = sup.to(dev)
    scores0 = run_scores.clone()

    def candidates():
        ops.beam_candidates(logits, V, running.view(R, L), cur, run_scores, cand_val, cand_tok, stop, suppress=sup, no_eos=True, eos=EOS)

    def update():
        run_scores.copy_(scores0)                        # (the entry updates the scores in place: keep every launch alike)
        ops.beam_update(cand_val, cand_tok, B, k, V, cur, P, L, EOS, False, float(cur + 1 - P), float(cur + 1 - P), running, other,
                        seqs, seqs2, run_scores, st["beam_scores"], st["finished"], st["lengths"], st["unsat"], stop, src_rows,
                        next_tok, plan)
    kc = kernel_us(candidates)
    kc["bytes"] = R * V * 2
    kc["GB_per_s"] = kc["bytes"] / kc["median_us"] * 1e-3
    candidates()
    ku = kernel_us(update)
    ku["copy_launch_included"] = "run_scores.copy_ (one small launch) + update + row move"
    ku["bytes"] = R * 2 * k * 8 + 2 * 2 * R * (cur + 1) * 8
    ku["GB_per_s"] = ku["bytes"] / ku["median_us"] * 1e-3
    res[f"kernels_at_step_{NEW // 2}"] = {"beam_candidates": kc, "beam_update": ku}
    return res


def main():
    import torch
    sys.path.insert(0, ROOT)
    from distil_whisper_amd import build
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForConditionalGeneration
    from distil_whisper_amd.ops_hip import HipOps
    dev = "cuda:0"
    ops = HipOps(dev)
    # (the encoder is not run: one layer keeps the set-up short; the decoder is distil-large-v3's)
    dims = WhisperDims(1280, 20, 5120, 1, 2, 51866, 128, decoder_start_token_id=50258)
    model = WhisperForConditionalGeneration(dims, ops=ops, state_dict=si.random_state_dict(dims, 0, dev))
    suppress, begin_suppress = list(range(1, 90)) + list(range(50258, 50364)), [220, 50257]
    results = {"kernels_sha16": build.kernels_sha16(),
               "protocol": "one process; per batch the two paths run interleaved, HIP events around each run, median of 10 rounds "
                           "after 2 warm-up rounds; spread_ms = max - min of the 10",
               "batches": [batch(model, ops, B, suppress, begin_suppress) for B in (16, 64)]}
    torch.cuda.synchronize()
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
