"""What the frozen teacher costs the distillation step, and what a step from stored top-k targets costs instead (README: large-v3
teacher, distil-large-v3 student, 32 clips, label lengths U{32..224}, packed live rows), in ONE process, eager steps, legs
interleaved, median of DW_NS (default 20) steps per leg with max - min, for MODE = full and recipe:
  dense                 the step as it is (teacher forward every step), this tree's library
  dense_parent_library  the same step through distil_whisper_amd/libdwamd_base.so -- the parent commit's kernels
                        (tools/build_base_lib.sh), when that file exists: the code is unchanged, so the two must agree within noise
  topk_k8 / 32 / 64     the step from stored targets, the teacher still resident
  teacherless_k32       the same step of a trainer built without a teacher (measured last: the teacher is freed first)
with torch.cuda.max_memory_allocated of each leg.  Then the kernels alone at the step's live row count and V = 51 866 (HIP events
around DW_NK launches): dw_distill_loss_topk (k = 32) against dw_distill_loss with their operand bytes, and dw_logits_topk.
Writes profiles/teacher_topk_bench.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distil_whisper_amd import ops_hip as _oh                          # noqa: E402
from distil_whisper_amd import student_init as si                      # noqa: E402
from distil_whisper_amd.build import kernels_sha16                     # noqa: E402
from distil_whisper_amd.distill import DistillationTrainer             # noqa: E402
from distil_whisper_amd.ops_hip import HipOps                          # noqa: E402

MODEL = os.environ.get("MODEL", "large-v3")
NS = int(os.environ.get("DW_NS", "20"))
NK = int(os.environ.get("DW_NK", "50"))
MODES = os.environ.get("MODES", "full,recipe").split(",")
KS = (8, 32, 64)
dev = "cuda:0"


def load_base(path):
    """the parent commit's library: it lacks this tree's new entry points, so only the symbols it exports get prototypes"""
    lib = C.CDLL(path)
    for name, (args, res) in _oh._SIGS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = args, res
    return lib


def timed(step, n):
    ms = []
    for _ in range(n):
        t0 = time.perf_counter()
        step()
        torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
    return ms


def summary(ms):
    return {"median_ms": round(statistics.median(ms), 2), "max_minus_min_ms": round(max(ms) - min(ms), 2), "steps": len(ms)}


def batch(tdims, B, T=447):
    g = torch.Generator(device=dev).manual_seed(1234)
    audio = 0.1 * torch.randn(B, 480000, generator=g, device=dev)
    ids = torch.randint(0, 50257, (B, T + 1), generator=g, device=dev)
    ids[:, 0] = tdims.decoder_start_token_id
    lens = torch.randint(32, 225, (B,), generator=g, device=dev)
    dec_in, labels = ids[:, :-1].contiguous(), ids[:, 1:].clone()
    labels[torch.arange(T, device=dev)[None, :] >= lens[:, None]] = -100
    return audio, dec_in, labels, [min(T, int(x)) for x in lens.tolist()]


def step_legs(ops, mode, base):
    recipe = mode == "recipe"
    tdims = si.PRESETS[MODEL]
    t_sd = si.random_state_dict(tdims, 0, dev)
    s_sd, sdims = si.student_from_teacher(t_sd, tdims, *si.STUDENT_LAYERS[MODEL])
    filt = torch.tensor(si.mel_filter_bank(tdims.n_mels), dtype=torch.float32, device=dev).contiguous()
    kw = dict(temperature=2.0, kl_weight=1.0, lr=1e-4, freeze_encoder=recipe, share_encoder=recipe, mel_filters=filt)
    tr = DistillationTrainer(ops, s_sd, sdims, t_sd, tdims, pad_teacher_rows=True, **kw)
    del t_sd
    B = int(os.environ.get("BATCH", "32"))
    audio, dec_in, labels, lens = batch(tdims, B)
    feats = tr.features(audio)
    targets = {k: tr.teacher_targets(feats, dec_in, labels, k=k, valid_len=lens) for k in KS}
    here = ops.lib
    legs = {"dense": (here, None)}
    if base is not None:
        legs["dense_parent_library"] = (base, None)
    for k in KS:
        legs[f"topk_k{k}"] = (here, targets[k])

    def run(trainer, lib, tt, n):
        ops.lib = lib
        try:
            return timed(lambda: trainer.train_step(trainer.features(audio), dec_in, labels, lr=0.0, valid_len=lens, teacher_topk=tt), n)
        finally:
            ops.lib = here

    times, mem = {name: [] for name in legs}, {}
    for name, (lib, tt) in legs.items():                       # first use of every leg, and its peak memory
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        run(tr, lib, tt, 2)
        mem[name] = torch.cuda.max_memory_allocated()
    half = max(1, NS // 2)
    for _ in range(2):                                         # two interleaved rounds
        for name, (lib, tt) in legs.items():
            times[name] += run(tr, lib, tt, half)
    live_rows = sum(lens)
    del tr
    torch.cuda.empty_cache()
    less = DistillationTrainer(ops, s_sd, sdims, None, None, **kw)
    del s_sd
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    run(less, here, targets[32], 2)
    mem["teacherless_k32"] = torch.cuda.max_memory_allocated()
    times["teacherless_k32"] = run(less, here, targets[32], 2 * half)
    del less
    torch.cuda.empty_cache()
    out = {name: dict(summary(ms), max_memory_allocated_GB=round(mem[name] / 2 ** 30, 2)) for name, ms in times.items()}
    if base is not None:
        out["dense_vs_parent_library_percent"] = round(100.0 * (out["dense"]["median_ms"] / out["dense_parent_library"]["median_ms"] - 1.0), 2)
    out["live_rows"] = live_rows
    return out


def kernels_alone(ops, rows, V=51866, T=2.0, k=32):
    ld = -(-V // 64) * 64
    g = torch.Generator(device=dev).manual_seed(7)
    s = (2.0 * torch.randn(rows, ld, generator=g, device=dev)).to(torch.bfloat16)
    t = (2.0 * torch.randn(rows, ld, generator=g, device=dev)).to(torch.bfloat16)
    labels = torch.randint(0, V, (rows,), generator=g, device=dev)
    idx, logp, rest = ops.logits_topk(t, V, T, k)
    grad = torch.empty_like(s)

    def per_launch(fn):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        for _ in range(NK):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) * 1e3 / NK

    row_bytes = 2 * V                                          # one bf16 row of V columns
    res = {}
    for name, fn, nbytes in (
            ("dw_distill_loss_topk", lambda: ops.distill_loss_topk(s, idx, logp, rest, labels, V, T, 0.8, 1.0, 1.0, True, grad_out=grad),
             rows * (2 * row_bytes + 8 * k + 4 + 8)),            # student row read once, gradient written once, k (idx, logp), rest, label
            ("dw_distill_loss", lambda: ops.distill_loss(s, t, labels, V, T, 0.8, 1.0, 1.0, True, grad_out=grad),
             rows * (3 * row_bytes + 8)),                        # both rows read (their re-reads come from cache), gradient written
            ("dw_logits_topk", lambda: ops.logits_topk(t, V, T, k), rows * (row_bytes + 8 * k + 4))):
        us = per_launch(fn)
        res[name] = {"us_per_call": round(us, 1), "operand_bytes": nbytes, "TBps": round(nbytes / us / 1e6, 2)}
    res["what"] = (f"{NK} back-to-back calls on one stream between HIP events (each call of a loss: its three launches); rows = {rows}, "
                   f"V = {V}, pitch {ld}, k = {k}, T = {T:g}; operand bytes = what the algorithm has to move once")
    return res


def main():
    ops = HipOps(dev)
    base_path = os.path.join(os.path.dirname(_oh.LIB_PATH), "libdwamd_base.so")
    base = load_base(base_path) if os.path.exists(base_path) else None
    out = {"what": "tools/bench_teacher_topk.py: eager distillation step, one process, interleaved legs, ms per step",
           "model": MODEL, "batch": int(os.environ.get("BATCH", "32")), "kernels_sha16": kernels_sha16(),
           "device": torch.cuda.get_device_name(0), "parent_library": base is not None, "modes": {}}
    rows = None
    for mode in MODES:
        out["modes"][mode] = step_legs(ops, mode, base)
        rows = out["modes"][mode]["live_rows"]
    out["kernels_alone"] = kernels_alone(ops, rows)
    path = os.environ.get("DW_OUT") or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                    "teacher_topk_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
