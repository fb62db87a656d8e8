"""What `generate(return_token_timestamps=True)` costs on the MI355X, against the reference's host post-processing of the same
matrices -> profiles/token_timestamps_bench.json.

distil-large-v3 decoder dimensions (2 decoder layers, d_model 1280, 20 heads), seeded weights, six (layer, head) alignment pairs,
220 generated tokens, batch 16 and 64.  Per batch, in one child process under its own time limit (a child that fails ends the
run: nothing else is started on the GPU):
  (a) `generate` on given encoder outputs with and without `return_token_timestamps` (HIP events around the call, median of 10
      after 3 warm-ups; token steps replayed from HIP graphs in both legs);
  (b) the extra decoder pass (engine.alignment_probs) and the three kernels one by one (same protocol);
  (c) the reference's post-processing -- normalisation, `_median_filter`, head mean, `_dynamic_time_warping`, the expressions of
      TF:generation_whisper.py:341-369, imported from `transformers` when it is installed (the restatement of
      tests/align_restatement.py otherwise; `host_reference.source` says which) -- on the same probabilities copied to the host,
      row after row as the reference runs it, torch on 16 threads;
  plus the error pair of tests/test_token_timestamps_gpu.py::test_align_prepare on these matrices (kernel / fp32 restatement
  against float64).
A third child runs the scenarios of tests/golden/token_timestamps.json end to end (graphs off and on) and records, per scenario,
whether the tokens equal the fixture's and how many timestamps lie more than one frame from the fp32 reference's, beside the
bound the GPU test asserts (`end_to_end`).
What the measurement requires is checked, not just stored: the time added per batch must be below the host reference's for the
same batch in the same run, else the tool stops without writing the file.
Usage:  python tools/bench_token_timestamps.py            (parent: runs the children, writes the JSON)
"""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "token_timestamps_bench.json")
HEADS = [[0, 5], [0, 12], [1, 0], [1, 3], [1, 7], [1, 19]]
NEW, P = 220, 4
CHILD_LIMIT_S = 420


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
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "reps": reps}


def child(B):
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import BaseModelOutput, WhisperForConditionalGeneration
    from distil_whisper_amd.ops_hip import HipOps
    import align_restatement as ar
    torch.set_num_threads(16)
    dev = "cuda:0"
    ops = HipOps(dev)
    tdims = si.PRESETS["large-v3"]
    t_sd = si.random_state_dict(tdims, 0, dev)
    s_sd, sdims = si.student_from_teacher(t_sd, tdims, 32, 2)
    del t_sd
    model = WhisperForConditionalGeneration(sdims, ops=ops, state_dict=s_sd)
    d = model.dims
    model.generation_config = GenerationConfig.from_any(dict(
        eos_token_id=50257, pad_token_id=50257, decoder_start_token_id=50258, max_length=448, alignment_heads=HEADS))
    g = torch.Generator().manual_seed(B)
    enc = (torch.randn(B, d.max_src, d.d_model, generator=g) * 0.5).to(dev)
    ids = torch.tensor([[50258, 50259, 50360, 50364]] * B, device=dev)
    mask = torch.ones(B, 3000, dtype=torch.long, device=dev)
    kw = dict(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=ids, max_new_tokens=NEW,
              min_new_tokens=NEW, use_graphs=True, force_unique_generate_call=True)
    res = {"batch": B, "new_tokens": NEW, "prompt_tokens": P, "alignment_heads": HEADS}
    seqs = model.generate(**kw)
    assert seqs.shape == (B, P + NEW), seqs.shape
    res["generate_plain"] = timed(lambda: model.generate(**kw))
    out = model.generate(return_token_timestamps=True, attention_mask=mask, **kw)
    ts = out["token_timestamps"].cpu()
    assert out["sequences"].tolist() == seqs.tolist()
    res["generate_token_timestamps"] = timed(lambda: model.generate(return_token_timestamps=True, attention_mask=mask, **kw))
    res["added_ms"] = res["generate_token_timestamps"]["median_ms"] - res["generate_plain"]["median_ms"]
    res["sanity"] = {"min_s": float(ts.min()), "max_s": float(ts.max()),
                     "rows_non_decreasing": int(((ts[:, 1:] - ts[:, :-1]) >= 0).all(1).sum()), "rows": B}
    # (b) the pieces
    eng = model.engine
    enc2 = enc.reshape(-1, d.d_model).to(eng.lowp).contiguous()
    L = P + NEW - 1
    body = seqs[:, :L].contiguous()
    res["decoder_pass_with_probs"] = timed(lambda: eng.alignment_probs(body, enc2, HEADS))
    probs = eng.alignment_probs(body, enc2, HEADS)
    q = (torch.randn(B * L, d.d_model + 64, generator=g) * 0.5).to(torch.bfloat16).to(dev)[:, :d.d_model]
    k = (torch.randn(B * d.max_src, 2 * d.d_model + 64, generator=g) * 0.5).to(torch.bfloat16).to(dev)[:, :d.d_model]
    hd = torch.tensor([5, 12, 0], dtype=torch.int32, device=dev)
    scratch = torch.empty_like(probs)
    res["kernel_cross_attn_probs_3_heads"] = timed(lambda: ops.cross_attn_probs(q, k, hd, scratch, 0, B, L, d.max_src))
    del scratch, q, k
    nt = torch.full((B,), L - P, dtype=torch.int32, device=dev)
    nf = torch.full((B,), d.max_src, dtype=torch.int32, device=dev)
    cost = ops.align_prepare(probs, nt, nf, P, d.max_src, 7)
    res["kernel_align_prepare"] = timed(lambda: ops.align_prepare(probs, nt, nf, P, d.max_src, 7, cost=cost))
    first = ops.dtw(cost, nt, nf, d.max_src)
    res["kernel_dtw"] = timed(lambda: ops.dtw(cost, nt, nf, d.max_src, first_frame=first))
    torch.cuda.synchronize()
    # (c) the reference's post-processing of the same matrices on the host
    try:
        from transformers.models.whisper.generation_whisper import _dynamic_time_warping, _median_filter
        source = "transformers " + __import__("transformers").__version__
    except ImportError:
        _median_filter, source = ar.median_filter_ref, "restatement (tests/align_restatement.py): transformers not installed"

        def _dynamic_time_warping(m):
            return ar.dtw_first_frame_ref(m), None
    host = probs[..., :d.max_src].cpu()
    N = L - P
    t0 = time.perf_counter()
    same = 0
    for b in range(B):
        w = host[b, :, P:]
        std = torch.std(w, dim=-2, keepdim=True, unbiased=False)
        mean = torch.mean(w, dim=-2, keepdim=True)
        m = _median_filter((w - mean) / std, 7).mean(dim=0)
        r = _dynamic_time_warping(-m.double().numpy())
        if r[1] is not None:
            jumps = np.pad(np.diff(r[0]), (1, 0), constant_values=1).astype(bool)
            ff = r[1][jumps]
        else:
            ff = r[0]
        same += int(ff.tolist() == first[b, :N].cpu().tolist())
    res["host_reference"] = {"ms": (time.perf_counter() - t0) * 1e3, "source": source, "threads": 16,
                             "rows_with_the_gpu_path": same, "rows": B,
                             "note": "its own fp32 cost matrix, not the GPU's: rows can differ where the path follows rounding noise"}
    # error pair of the prepare stage on two rows of these matrices
    err_k = err_r = 0.0
    for b in range(min(B, 2)):
        w = host[b, :, P:]
        r64 = ar.prepare_ref(w.double(), 7)
        err_k = max(err_k, (cost[b, :N, :d.max_src].cpu().double() - r64).abs().max().item())
        err_r = max(err_r, (ar.prepare_ref(w, 7).double() - r64).abs().max().item())
    res["align_prepare_max_abs_error_vs_float64"] = {"kernel": err_k, "fp32_restatement": err_r}
    res["added_below_host_reference"] = res["added_ms"] < res["host_reference"]["ms"]
    print("RESULT " + json.dumps(res))


def child_e2e():
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from distil_whisper_amd.ops_hip import HipOps
    import align_restatement as ar
    ops = HipOps("cuda:0")
    gold = ar.gold()
    rows = []
    for sc in gold["scenarios"]:
        for graphs in ((False, True) if sc["kind"] == "single" else (False,)):
            extra = dict(use_graphs=graphs) if sc["kind"] == "single" else {}
            _, out = ar.run_dropin(ops, sc, gold["meta"], **extra)
            same = out["sequences"].tolist() == sc["sequences"]
            row = {"scenario": sc["name"], "seed": sc["seed"], "graphs": graphs, "tokens_equal_fixture": same,
                   "ref_bf16_share": sc["ref_bf16_share"]}
            if same:
                far, total = ar.far_tokens(out["token_timestamps"].cpu().tolist(), sc["token_timestamps"])
                row.update(tokens_far=far, tokens=total, tokens_allowed=max(2 * sc["ref_bf16_share"] * total, 1.0))
                if sc["kind"] == "seek":
                    row.update(ar.segment_shares(sc, out))
                    row["segments"] = len(out["segments"][0])
            rows.append(row)
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(rows))


def run_child(args, what):
    r = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, capture_output=True, text=True, timeout=CHILD_LIMIT_S)
    line = [x for x in r.stdout.splitlines() if x.startswith("RESULT ")]
    if r.returncode != 0 or not line:
        sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
        raise SystemExit(f"{what}: child ended with status {r.returncode}; nothing more is started")
    return json.loads(line[-1][7:])


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--child":
        return child(int(sys.argv[2]))
    if len(sys.argv) > 1 and sys.argv[1] == "--child-e2e":
        return child_e2e()
    sys.path.insert(0, ROOT)
    from distil_whisper_amd import build
    results = {"kernels_sha16": build.kernels_sha16(), "protocol": "HIP events around each call, median of 10 after 3 warm-ups",
               "batches": []}
    for B in (16, 64):
        res = run_child(["--child", str(B)], f"batch {B}")
        results["batches"].append(res)
        if not res["added_ms"] < res["host_reference"]["ms"]:
            raise SystemExit(f"batch {B}: token timestamps add {res['added_ms']:.1f} ms to generate, the reference's host "
                             f"post-processing of the same matrices takes {res['host_reference']['ms']:.1f} ms: requirement missed")
    results["end_to_end"] = run_child(["--child-e2e"], "end to end")
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
