"""What training-mode dropout costs on the benchmark step (README: distil-large-v3 student, 32 clips, label lengths U{32..224},
packed live rows), in ONE process, eager steps, median of DW_NS (default 10) steps per leg, legs interleaved:
  (a) probabilities 0 on this tree's library against the same step on distil_whisper_amd/libdwamd_base.so -- the parent
      commit's kernels (tools/build_base_lib.sh HEAD~1 or the commit to compare with), when that file exists;
  (b) dropout = activation_dropout = 0.1.
Then one step with per-launch events: time, bytes and GB/s of the dropout forward / backward launches.  Bytes are the
operands' sizes (inputs read once, outputs written once, one mask bit per element): at a residual site of the student
2 (bf16 branch) + 4 (fp32 stream) read and 4 + 1/8 written per element.  Writes profiles/dropout_bench.json."""
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

STREAM_COPY_TBS = 6.3          # README's streaming-copy figure of the MI355X
MODEL = os.environ.get("MODEL", "large-v3")
NS = int(os.environ.get("DW_NS", "10"))
dev = "cuda:0"


def load_base(path):
    """the parent commit's library: it has no dropout entry points, so only the symbols it exports get prototypes"""
    lib = C.CDLL(path)
    for name, (args, res) in _oh._SIGS.items():
        fn = getattr(lib, name, None)
        if fn is not None:
            fn.argtypes, fn.restype = args, res
    return lib


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

    def leg(lib, p):
        ops.lib = lib
        tr.student.set_dropout(p, p, seed=1)
        step()
        torch.cuda.synchronize()
        ms = []
        for _ in range(NS):
            t0 = time.perf_counter()
            step()
            torch.cuda.synchronize()
            ms.append((time.perf_counter() - t0) * 1e3)
        return ms

    legs = {"p0": (here, 0.0), "p0.1": (here, 0.1)}
    if base is not None:
        legs["p0_parent_library"] = (base, 0.0)
    leg(here, 0.0)                                             # first-use initialisation, allocator warm-up
    times = {k: [] for k in legs}
    for _ in range(2):                                         # two interleaved rounds of NS steps per leg
        for k, (lib, p) in legs.items():
            times[k] += leg(lib, p)
    med = {k: statistics.median(v) for k, v in times.items()}

    # per-launch events of one step with dropout on; the wrappers add up the operand bytes of every dropout launch
    ops.lib = here
    tr.student.set_dropout(0.1, 0.1, seed=1)
    nbytes = {"dropout_fwd": 0, "dropout_bwd": 0}
    elems = {"dropout_fwd": 0, "dropout_bwd": 0}
    fwd, bwd = ops.dropout_fwd, ops.dropout_bwd

    def size(t, rows, cols):
        return 0 if t is None else rows * cols * t.element_size()

    def fwd_counted(u, p, seed, state, site, residual=None, out=None, out_dtype=None, out_row_pad=0):
        o, m = fwd(u, p, seed, state, site, residual=residual, out=out, out_dtype=out_dtype, out_row_pad=out_row_pad)
        r, c = u.shape
        nbytes["dropout_fwd"] += size(u, r, c) + size(residual, r, c) + size(o, r, c) + r * c // 8
        elems["dropout_fwd"] += r * c
        return o, m

    def bwd_counted(dy, mask, p, out=None):
        o = bwd(dy, mask, p, out=out)
        r, c = dy.shape
        nbytes["dropout_bwd"] += size(dy, r, c) + size(o, r, c) + r * c // 8
        elems["dropout_bwd"] += r * c
        return o

    ops.dropout_fwd, ops.dropout_bwd = fwd_counted, bwd_counted
    ops.profile = {}
    step()
    prof = ops.collect_profile()
    ops.profile = None
    kernels = {}
    for k in ("dropout_fwd", "dropout_bwd"):
        ms = prof[k]["ms"]
        kernels[k] = {"launches": prof[k]["n"], "ms_per_step": round(ms, 3), "elements": elems[k], "bytes": nbytes[k],
                      "bytes_per_element": round(nbytes[k] / elems[k], 3), "GBps": round(nbytes[k] / ms / 1e6, 1),
                      "share_of_stream_copy": round(nbytes[k] / ms / 1e9 / STREAM_COPY_TBS, 3)}
    out = {"what": "tools/bench_dropout.py: eager distillation step, one process, interleaved legs, median ms per step",
           "model": MODEL, "batch": B, "steps_per_leg": 2 * NS, "kernels_sha16": kernels_sha16(),
           "device": torch.cuda.get_device_name(0), "median_ms": {k: round(v, 2) for k, v in med.items()},
           "all_ms": {k: [round(x, 2) for x in v] for k, v in times.items()},
           "added_ms_per_step_p0.1": round(med["p0.1"] - med["p0"], 2),
           "p0_vs_parent_library_percent": round(100.0 * (med["p0"] / med["p0_parent_library"] - 1.0), 2) if base is not None else None,
           "stream_copy_TBps_reference": STREAM_COPY_TBS, "kernels": kernels}
    path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "dropout_bench.json")
    if os.environ.get("DW_OUT"):
        path = os.environ["DW_OUT"]
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
