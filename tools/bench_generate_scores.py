"""What `generate(output_scores=True, return_dict_in_generate=True)` costs on the MI355X -> profiles/generate_scores_bench.json.

distil-large-v3 decoder dimensions (2 decoder layers, d_model 1280, 20 heads, vocabulary 51 866), seeded weights, 220 generated
tokens, batch 16 and 64 (the set-up of tools/bench_token_timestamps.py).  Per batch, in one child process under its own time
limit (a child that fails ends the run: nothing else is started on the GPU):
  (a) `generate` on given encoder outputs without the flags -- the call as it was before the feature, the base --, with
      `output_scores`, and with `output_scores` + `output_logits` (HIP events around the call, median / min / max of 10 after 3
      warm-ups; token steps replayed from HIP graphs in every leg);
  (b) the pieces: the teacher-forced decoder pass (engine.decode over sequences[:, :-1]) and the scoring kernel alone, with the
      bytes the kernel has to move (the logits of the scored rows once, the fp32 scores once) over its time, beside the HBM rate
      a streaming kernel reaches on this part (6.3 TB/s, copy kernel); `chosen` / `logprob` alone (no score tensor written) is
      the same launch without the store.
Nothing is promised here: the file records what was measured, with the spread over the repeats.
Usage:  python tools/bench_generate_scores.py            (parent: runs the children, writes the JSON)
"""
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "profiles", "generate_scores_bench.json")
NEW, P = 220, 4
HBM_BYTES_PER_S = 6.3e12
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
    import torch
    sys.path.insert(0, ROOT)
    from distil_whisper_amd import student_init as si
    from distil_whisper_amd.generation import GenerationConfig
    from distil_whisper_amd.modeling import BaseModelOutput, WhisperForConditionalGeneration
    from distil_whisper_amd.ops_hip import HipOps
    dev = "cuda:0"
    ops = HipOps(dev)
    tdims = si.PRESETS["large-v3"]
    t_sd = si.random_state_dict(tdims, 0, dev)
    s_sd, sdims = si.student_from_teacher(t_sd, tdims, 32, 2)
    del t_sd
    model = WhisperForConditionalGeneration(sdims, ops=ops, state_dict=s_sd)
    d = model.dims
    suppress = list(range(1, 90)) + list(range(50257, 50364))
    model.generation_config = GenerationConfig.from_any(dict(
        eos_token_id=50257, pad_token_id=50257, decoder_start_token_id=50258, max_length=448, suppress_tokens=suppress,
        begin_suppress_tokens=[220, 50257]))
    g = torch.Generator().manual_seed(B)
    enc = (torch.randn(B, d.max_src, d.d_model, generator=g) * 0.5).to(dev)
    ids = torch.tensor([[50258, 50259, 50360, 50364]] * B, device=dev)
    kw = dict(encoder_outputs=BaseModelOutput(last_hidden_state=enc), decoder_input_ids=ids, max_new_tokens=NEW,
              min_new_tokens=NEW, use_graphs=True, return_dict_in_generate=True)
    res = {"batch": B, "new_tokens": NEW, "prompt_tokens": P, "vocab": d.vocab}
    seqs = model.generate(**kw).sequences
    assert seqs.shape == (B, P + NEW), seqs.shape
    out = model.generate(output_scores=True, output_logits=True, **kw)
    assert out.sequences.tolist() == seqs.tolist() and len(out.scores) == NEW and len(out.logits) == NEW
    st = torch.stack(tuple(out.scores[:8]), 1)
    res["sanity"] = {
        "masked_columns_step0": int(torch.isneginf(out.scores[0][0]).sum()), "masked_columns_step1": int(torch.isneginf(out.scores[1][0]).sum()),
        "logits_all_finite": bool(all(torch.isfinite(t).all() for t in out.logits[:8])),
        "argmax_equals_tokens_share": float((torch.stack(tuple(out.scores), 1).argmax(-1) == seqs[:, P:]).float().mean()),
        "chosen_is_gather": bool(torch.equal(out.scores.chosen[:, :8], st.gather(2, seqs[:, P:P + 8, None])[:, :, 0]))}
    del out, st
    res["generate_plain"] = timed(lambda: model.generate(**kw))
    res["generate_output_scores"] = timed(lambda: model.generate(output_scores=True, **kw))
    res["generate_output_scores_and_logits"] = timed(lambda: model.generate(output_scores=True, output_logits=True, **kw))
    res["added_ms_output_scores"] = res["generate_output_scores"]["median_ms"] - res["generate_plain"]["median_ms"]
    # (b) the pieces
    eng = model.engine
    enc2 = enc.reshape(-1, d.d_model).to(eng.lowp).contiguous()
    T = P + NEW
    body = seqs[:, :T - 1].contiguous()
    res["decoder_pass"] = timed(lambda: eng.decode(body, enc2, save=False))
    logits, _ = eng.decode(body, enc2, save=False)
    rows = logits[P - 1:]
    sup = torch.zeros(d.vocab, dtype=torch.uint8)
    sup[suppress] = 1
    sup = sup.to(dev)
    # the kernel alone: the entry point itself on preallocated results (no allocation inside the timed region)
    from distil_whisper_amd.ops_hip import _dt, _p, _rup4
    ldo = _rup4(d.vocab)
    o_scores = torch.empty((NEW, B, ldo), dtype=torch.float32, device=dev)
    o_chosen = torch.empty((B, NEW), dtype=torch.float32, device=dev)
    o_logprob = torch.empty((B, NEW), dtype=torch.float32, device=dev)

    def kernel(scores):
        rc = ops.lib.dw_score_tokens(_p(rows), _dt(rows), B, NEW, d.vocab, rows.stride(0), T - 1, _p(seqs), seqs.stride(0), P,
                                     _p(sup), None, NEW, -1, -1, 50257, _p(scores), ldo, _p(o_chosen), _p(o_logprob),
                                     ops._stream())
        assert rc == 0, rc
    res["kernel_score_tokens"] = timed(lambda: kernel(o_scores))
    nbytes = NEW * B * (d.vocab * logits.element_size() + ldo * 4)
    sec = res["kernel_score_tokens"]["median_ms"] * 1e-3
    res["kernel_score_tokens"].update(
        bytes=nbytes, bytes_per_s=nbytes / sec, share_of_hbm_rate=nbytes / sec / HBM_BYTES_PER_S, hbm_bytes_per_s=HBM_BYTES_PER_S,
        note="dw_score_tokens on preallocated results; bytes = the scored logits rows once + the fp32 scores once")
    res["kernel_score_tokens_chosen_only"] = timed(lambda: kernel(None))
    rules = dict(batch_rows=T - 1, suppress=sup, min_new=NEW, eos=50257)
    sc, ch, lp = ops.score_tokens(rows, d.vocab, seqs, P, NEW, **rules)
    assert torch.equal(sc, o_scores[:, :, :d.vocab]) and torch.equal(lp, o_logprob)        # the binding runs the same launch
    res["binding_score_tokens"] = timed(lambda: ops.score_tokens(rows, d.vocab, seqs, P, NEW, **rules))
    torch.cuda.synchronize()
    print("RESULT " + json.dumps(res))


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
    sys.path.insert(0, ROOT)
    from distil_whisper_amd import build
    results = {"kernels_sha16": build.kernels_sha16(), "protocol": "HIP events around each call, median of 10 after 3 warm-ups",
               "batches": []}
    for B in (16, 64):
        results["batches"].append(run_child(["--child", str(B)], f"batch {B}"))
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
