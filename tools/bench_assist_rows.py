"""What one round of speculative decoding costs on the MI355X with per-row acceptance, next to the minimum-rule round and the target's
plain token step -> profiles/assist_rows_bench.json.

The set-up of tools/bench_assist.py (its helpers are imported): target with large-v3 decoder dimensions (32 decoder layers, d_model
1280, 20 heads, vocabulary 51 866; one encoder layer, the encoder is not run), bf16; assistant a decoder-only `WhisperForCausalLM`
with 2 layers; seeded random weights, num_assistant_tokens = 5, ROUNDS new tokens per run (no EOS id; random drafts are rejected, so
as many rounds), batch 4 and 16, everything in ONE process.  Per batch the two paths of decoding.assisted_greedy_decode on the same
engines and encoder output, their runs INTERLEAVED (a, b, a, b, ...), HIP events around each run, median / min / max of 10 runs
after 2 warm-up runs:
  (a) `min_rule`: the uniform round (dw_assist_pick / dw_assist_accept, `decode_multi` / `decode_step` with their fused paths) -- the
      parent commit's round, re-measured here;
  (b) `per_row`:  `per_row=True`: from round 2 on every decoder pass is dw_decode_step_rows (no projection inside the self-attention,
      no fused K/V append), the assistant's 2-token catch-up pass runs every round, dw_assist_pick_rows / dw_assist_accept_rows.
Rounds are counted (calls of the accept entry), launches and host synchronisations per round come from torch's profiler over one
run of each path.  In the same process the target's plain graph-replayed token step (`GreedyDecoder`, 64 new tokens) is timed the
same way.

NOT measured: random weights accept no draft and no trained checkpoint is at hand, so the acceptance rate of real models, and with
it any end-to-end speed-up of either path, is not measured on these machines.  Two pieces of ARITHMETIC are added and marked as
such: the break-even accepted drafts per row per round, a* = round_ms / token_step_ms - 1 (a round emits a + 1 tokens per row), and
the expected accepted drafts per round if every draft of every row agreed independently with probability p -- per row sum_{j=1..K}
p^j, under the minimum rule sum_{j=1..K} p^(j B).
Usage:  python tools/bench_assist_rows.py
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
OUT = os.path.join(ROOT, "profiles", "assist_rows_bench.json")
K, P, PLAIN_NEW, ROUNDS = 5, 4, 64, 40
PROBS = (0.5, 0.7, 0.8, 0.9, 0.95)


def expected_accepted(p, B):
    return {"per_row": sum(p ** j for j in range(1, K + 1)), "min_rule": sum(p ** (j * B) for j in range(1, K + 1))}


def batch(target, assistant, ops, B):
    import torch
    from bench_assist import counted, interleaved
    from distil_whisper_amd import decoding
    eng, d, dev = target.engine, target.dims, ops.device
    g = torch.Generator().manual_seed(B)
    enc = (torch.randn(B, d.max_src, d.d_model, generator=g) * 0.5).to(dev).reshape(-1, d.d_model).to(eng.lowp).contiguous()
    ids = torch.tensor([[50258, 50259, 50360, 50364]] * B, device=dev)

    def run(per_row):
        return decoding.assisted_greedy_decode(eng, assistant.engine, enc, enc, ids, ROUNDS, K, per_row=per_row)
    legs = {"min_rule": lambda: run(False), "per_row": lambda: run(True)}
    # sanity run with the accept entries counted: the rounds of a run
    rounds, outs = {}, {}
    for leg, entry in (("min_rule", "assist_accept"), ("per_row", "assist_accept_rows")):
        fn, n = getattr(type(ops), entry), [0]

        def wrapped(self, *a, _fn=fn, _n=n, **k):
            _n[0] += 1
            return _fn(self, *a, **k)
        setattr(type(ops), entry, wrapped)
        try:
            outs[leg] = legs[leg]()
        finally:
            setattr(type(ops), entry, fn)
        rounds[leg] = n[0]
    a, b = outs["min_rule"], outs["per_row"]
    res = {"batch": B, "num_assistant_tokens": K, "new_tokens": ROUNDS, "prompt_tokens": P, "vocab": d.vocab,
           # (seeded random weights have nearly flat logits: the rows pass and the uniform pass round their sums in another order,
           # and a selection whose two best bf16 scores are an ulp apart turns -- rows of the two paths part at the first such
           # selection.  What the per-row path must equal is each row decoded alone: tests/test_assist_rows_gpu.py, peaked models)
           "sanity": {"rows_with_equal_tokens_on_both_paths": int((a[0] == b[0]).all(1).sum()) if a[0].shape == b[0].shape else 0,
                      "min_rule": {"drafted": a[1], "accepted": a[2]}, "per_row": {"drafted_over_rows": b[1], "accepted_over_rows": b[2]}}}
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
    res["per_row_minus_min_rule_ms_per_round"] = res["per_row"]["round_ms"] - res["min_rule"]["round_ms"]
    res["per_row_over_min_rule"] = res["per_row"]["round_ms"] / res["min_rule"]["round_ms"]
    res["arithmetic_not_measurement"] = {
        "break_even_accepted_per_row_per_round": {n: res[n]["round_ms"] / plain["token_step_ms"] - 1.0 for n in legs},
        "expected_accepted_per_round_at_independent_agreement_p": {str(p): expected_accepted(p, B) for p in PROBS}}
    return res


def main():
    import dataclasses
    import torch
    from distil_whisper_amd import build
    from distil_whisper_amd.engine import WhisperDims
    from distil_whisper_amd.modeling import WhisperForCausalLM, WhisperForConditionalGeneration
    from distil_whisper_amd.ops_hip import HipOps
    ops = HipOps("cuda:0")
    dims = WhisperDims(1280, 20, 5120, 1, 32, 51866, 128, decoder_start_token_id=50258)
    target = WhisperForConditionalGeneration(dims, ops=ops, seed=0, dtype=torch.bfloat16)
    assistant = WhisperForCausalLM(dataclasses.replace(dims, dec_layers=2), ops=ops, seed=1, dtype=torch.bfloat16)
    results = {"kernels_sha16": build.kernels_sha16(),
               "protocol": "one process; per batch the two paths run interleaved, HIP events around each run, median of 10 runs "
                           "after 2 warm-up runs; spread_ms = max - min of the 10; round_ms = median_ms / rounds (rounds counted)",
               "not_measured": "random weights accept no draft and no trained checkpoint is available: the acceptance rate of real "
                               "models and any end-to-end speed-up are NOT measured; the entries under arithmetic_not_measurement "
                               "are computed from the measured round and token-step times, not observed",
               "batches": [batch(target, assistant, ops, B) for B in (4, 16)]}
    torch.cuda.synchronize()
    with open(OUT, "w") as f:
        json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
