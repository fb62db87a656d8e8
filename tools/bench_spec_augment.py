"""What SpecAugment costs on the benchmark step (README: distil-large-v3 student, 32 clips, label lengths U{32..224}, packed
live rows), in ONE process, eager steps, median of 2 x DW_NS (default 10) steps per leg, legs interleaved:
  (a) augmentation off on this tree's library against the same step on distil_whisper_amd/libdwamd_base.so -- the parent
      commit's kernels (tools/build_base_lib.sh HEAD~1 or the commit to compare with), when that file exists;
  (b) augmentation on at the reference's defaults (mask_time_prob 0.05, length 10, min 2; no feature masking);
  (c) the same with mask_feature_prob = 0.1.
Then the kernel alone at B = 32, n_mels = 128, T = 3000 (HIP events around 25 replays of a graph of DW_NK = 200 launches): in place (only the
zeros are stored: bytes = 4 x masked elements) and out of place (every element read once and written once: 2 x 4 x B x n_mels x T),
against the README's streaming-copy figure.  Writes profiles/spec_augment_bench.json."""
import ctypes as C
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distil_whisper_amd import ops_hip as _oh                          # noqa: E402
from distil_whisper_amd import spec_augment as sa                      # noqa: E402
from distil_whisper_amd import student_init as si                      # noqa: E402
from distil_whisper_amd.build import kernels_sha16                     # noqa: E402
from distil_whisper_amd.distill import DistillationTrainer             # noqa: E402
from distil_whisper_amd.ops_hip import HipOps                          # noqa: E402

STREAM_COPY_TBS = 6.3          # README's streaming-copy figure of the MI355X
MODEL = os.environ.get("MODEL", "large-v3")
NS = int(os.environ.get("DW_NS", "10"))
NK = int(os.environ.get("DW_NK", "200"))
REPLAYS = 25
dev = "cuda:0"
DEFAULTS = sa.normalise({})
WITH_FEATURE = sa.normalise({"mask_feature_prob": 0.1})


def load_base(path):
    """the parent commit's library: it has no SpecAugment entry point, so only the symbols it exports get prototypes"""
    lib = C.CDLL(path)
    for name, (args, res) in _oh._SIGS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = args, res
    return lib


def kernel_alone(ops):
    B, n_mels, T = 32, 128, 3000
    x = torch.randn(B, n_mels, T, device=dev)
    out = torch.empty_like(x)
    st = ops.dropout_state(1)
    res = {}
    for name, p in (("defaults", DEFAULTS), ("mask_feature_prob_0.1", WITH_FEATURE)):
        _, tm, fm = ops.spec_augment(x, 1, st, p, out=out, want_masks=True)
        zeroed = int((tm.bool()[:, None, :] | fm.bool()[:, :, None]).sum().item())
        for form, dst, nbytes in (("in_place", None, 4 * zeroed), ("out_of_place", out, 2 * 4 * x.numel())):
            y = x.clone()
            for _ in range(10):
                ops.spec_augment(y, 1, st, p, out=dst)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()          # NK launches in one graph: the host's enqueue rate stays out of the figure
            with torch.cuda.graph(graph):
                for _ in range(NK):
                    ops.spec_augment(y, 1, st, p, out=dst)
            graph.replay()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(REPLAYS):
                graph.replay()
            e1.record()
            torch.cuda.synchronize()
            us = e0.elapsed_time(e1) * 1e3 / (NK * REPLAYS)
            res[f"{name}_{form}"] = {"us_per_launch": round(us, 2), "bytes": nbytes, "masked_share": round(zeroed / x.numel(), 4),
                                     "GBps": round(nbytes / us / 1e3, 1),
                                     "share_of_stream_copy": round(nbytes / us / 1e6 / STREAM_COPY_TBS, 3)}
    return {"shape": [B, n_mels, T], "launches_timed": NK * REPLAYS,
            "what": f"{REPLAYS} replays of a graph of {NK} back-to-back launches on one stream, HIP events", **res}


def main():
    ops = HipOps(dev)
    tdims = si.PRESETS[MODEL]
    t_sd = si.random_state_dict(tdims, 0, dev)
    s_sd, sdims = si.student_from_teacher(t_sd, tdims, *si.STUDENT_LAYERS[MODEL])
    filt = torch.tensor(si.mel_filter_bank(tdims.n_mels), dtype=torch.float32, device=dev).contiguous()
    tr = DistillationTrainer(ops, s_sd, sdims, t_sd, tdims, mel_filters=filt, pad_teacher_rows=True)
    del t_sd, s_sd
    B, T = int(os.environ.get("BATCH", "32")), 447
    g = torch.Generator(device=dev).manual_seed(1234)
    audio = 0.1 * torch.randn(B, 480000, generator=g, device=dev)
    ids = torch.randint(0, 50257, (B, T + 1), generator=g, device=dev)
    ids[:, 0] = tdims.decoder_start_token_id
    lens = torch.randint(32, 225, (B,), generator=g, device=dev)
    dec_in, labels = ids[:, :-1].contiguous(), ids[:, 1:].clone()
    labels[torch.arange(T, device=dev)[None, :] >= lens[:, None]] = -100
    lens = [min(T, int(x)) for x in lens.tolist()]
    here = ops.lib
    base_path = os.path.join(os.path.dirname(_oh.LIB_PATH), "libdwamd_base.so")
    base = load_base(base_path) if os.path.exists(base_path) else None

    def step():
        return tr.train_step(tr.features(audio), dec_in, labels, lr=0.0, valid_len=lens)

    def leg(lib, params):
        ops.lib = lib
        tr.spec_augment = params
        tr.student.set_spec_augment(params, seed=1)
        step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(NS):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    legs = {"off": (here, None), "on_defaults": (here, DEFAULTS), "on_mask_feature_prob_0.1": (here, WITH_FEATURE)}
    if base is not None:
        legs["off_parent_library"] = (base, None)
    leg(here, None)                                            # first-use initialisation, allocator warm-up
    times = {k: [] for k in legs}
    for _ in range(2):                                         # two interleaved rounds of NS steps per leg
        for k, (lib, params) in legs.items():
            times[k] += leg(lib, params)
    med = {k: statistics.median(v) for k, v in times.items()}
    ops.lib = here
    out = {"what": "tools/bench_spec_augment.py: eager distillation step, one process, interleaved legs, median ms per step",
           "model": MODEL, "batch": B, "steps_per_leg": 2 * NS, "kernels_sha16": kernels_sha16(),
           "device": torch.cuda.get_device_name(0), "median_ms": {k: round(v, 2) for k, v in med.items()},
           "all_ms": {k: [round(x, 2) for x in v] for k, v in times.items()},
           "added_ms_per_step_defaults": round(med["on_defaults"] - med["off"], 2),
           "added_ms_per_step_mask_feature_prob_0.1": round(med["on_mask_feature_prob_0.1"] - med["off"], 2),
           "off_vs_parent_library_percent": round(100.0 * (med["off"] / med["off_parent_library"] - 1.0), 2) if base is not None else None,
           "stream_copy_TBps_reference": STREAM_COPY_TBS, "kernel_alone": kernel_alone(ops)}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "spec_augment_bench.json")
    if os.environ.get("DW_OUT"):
        path = os.environ["DW_OUT"]
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
