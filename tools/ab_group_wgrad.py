"""In-process A/B of WhisperEngine.group_wgrad (a layer's weight-gradient GEMMs in one grouped launch, dw_wgrad_group) on the full
distillation step -- bench.py's batch: large-v3 teacher, 32/2 student, B = 32, label lengths U{32..224}, packed live rows.

Alternating legs off / on of (a) the captured single-stream step (train_step_graphed; the plan is dropped and captured again for
every leg) and (b) the eager step with the teacher and weight-gradient side streams.  A leg is the median of DW_NS (default 12)
steps, each timed with HIP events on the main stream; DW_PAIRS (default 3) off/on pairs per mode.  The gain counts only if every
on-leg median is below every off-leg median of the mode; the spread of the off-legs is printed next to it.

    python tools/ab_group_wgrad.py [out.json]"""
import json, os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from distil_whisper_amd.ops_hip import HipOps
from distil_whisper_amd.distill import DistillationTrainer
from distil_whisper_amd import student_init as si
dev = "cuda:0"
ops = HipOps(dev)
MODEL = os.environ.get("MODEL", "large-v3")
tdims = si.PRESETS[MODEL]
t_sd = si.random_state_dict(tdims, 0, dev)
s_sd, sdims = si.student_from_teacher(t_sd, tdims, *si.STUDENT_LAYERS[MODEL])
filt = torch.tensor(si.mel_filter_bank(tdims.n_mels), dtype=torch.float32, device=dev).contiguous()
tr = DistillationTrainer(ops, s_sd, sdims, t_sd, tdims, mel_filters=filt)
del t_sd, s_sd
B, T = 32, 447
audio = 0.1 * torch.randn(B, 480000, device=dev)
ids = torch.randint(0, 50257, (B, T + 1), device=dev); ids[:, 0] = tdims.decoder_start_token_id
dec_in = ids[:, :-1].contiguous(); labels = ids[:, 1:].clone()
lens = torch.randint(32, 225, (B,), generator=torch.Generator().manual_seed(1234)).tolist()
labels[torch.arange(T, device=dev)[None, :] >= torch.tensor(lens, device=dev)[:, None]] = -100
NS, PAIRS = int(os.environ.get("DW_NS", "12")), int(os.environ.get("DW_PAIRS", "3"))


def graph_step():
    return tr.train_step_graphed(audio, dec_in, labels, valid_len=lens)


def eager_step():
    return tr.train_step(tr.features(audio), dec_in, labels, valid_len=lens)


def leg(step, pre):
    for _ in range(pre):
        step()
    torch.cuda.synchronize()
    ms = []
    for _ in range(NS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        step()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return sorted(ms)[len(ms) // 2]


out = {"model": MODEL, "steps_per_leg": NS, "statistic": "median ms/step of a leg, HIP events around each step"}
for mode, side, step, pre in (("hip_graph_single_stream", False, graph_step, 5), ("eager_side_streams", True, eager_step, 3)):
    tr.drop_graph()
    tr.overlap_teacher = side
    tr.set_overlap_wgrad(side)
    legs = {"off": [], "on": []}
    for _ in range(PAIRS):
        for name, on in (("off", False), ("on", True)):
            tr.drop_graph()
            torch.cuda.empty_cache()
            tr.student.group_wgrad = on
            n0 = tr.student.wgrad_groups_issued
            legs[name].append(round(leg(step, pre), 3))
            assert (tr.student.wgrad_groups_issued > n0) == (on and MODEL == "large-v3")
    out[mode] = dict(legs, off_spread=round(max(legs["off"]) - min(legs["off"]), 3),
                     gain_ms=round(sorted(legs["off"])[PAIRS // 2] - sorted(legs["on"])[PAIRS // 2], 3),
                     every_on_below_every_off=max(legs["on"]) < min(legs["off"]))
    print(mode, json.dumps(out[mode]), flush=True)
tr.drop_graph()
if len(sys.argv) > 1:
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)
