"""bench.py's plain run and its output dump: `--steps` timed steps and `ms_per_step` in the result line, nothing of
`--full` in a plain run, and `--dump-outputs DIR` writing float32 arrays of one step of the timed path from the seeded
initial state (a fixed, seeded sample of the big buffers, 64 MB at most in all)."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DUMPED = ["grad_norm.npy", "losses.npy", "student_grads_sample.npy", "student_params_sample.npy"]


def test_dump_outputs_writes_the_same_float32_sample_every_time(tmp_path):
    import bench
    g = torch.Generator().manual_seed(5)
    st = types.SimpleNamespace(P=torch.randn(5000, generator=g), G=torch.randn(5000, generator=g), train_start=1000,
                               train_end=4000)
    tr = types.SimpleNamespace(student_store=st, grad_norm=lambda: torch.tensor(2.5))
    losses = torch.tensor([1.0, 2.0, 3.0, 41.0])
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), tr, losses)
    assert sorted(os.listdir(tmp_path / "a")) == DUMPED
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in DUMPED) <= 64 << 20
    for f in DUMPED:
        a, b = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert a.dtype == np.float32 and np.array_equal(a, b), f
    assert np.array_equal(np.load(tmp_path / "a" / "losses.npy"), losses.numpy())
    assert np.load(tmp_path / "a" / "grad_norm.npy").tolist() == [2.5]
    p, gr = np.load(tmp_path / "a" / "student_params_sample.npy"), np.load(tmp_path / "a" / "student_grads_sample.npy")
    # the same positions of both buffers, all inside the trainable range
    pos = {float(v): i for i, v in enumerate(st.P.numpy())}
    idx = np.array([pos[float(v)] for v in p[:1000]])
    assert idx.min() >= 1000 and idx.max() < 4000 and np.array_equal(gr[:1000], st.G.numpy()[idx])


@pytest.mark.gpu
@pytest.mark.timeout(600)
def test_plain_run_times_its_steps_and_dumps_a_reproducible_step(tmp_path):
    dumps = []
    for steps, warmup in ((3, 1), (2, 2)):         # (different histories before the dumped step)
        out_dir = tmp_path / f"outputs_{steps}"
        r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps),
                            "--warmup", str(warmup), "--model", "tiny.en", "--batch", "2", "--dump-outputs", str(out_dir)],
                           capture_output=True, text=True, timeout=250)
        assert r.returncode == 0, r.stderr[-2000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1, r.stdout
        out = json.loads(lines[0])
        assert out["steps"] == steps and out["warmup"] == warmup and out["ms_per_step"] > 0 and out["value"] > 0
        assert out["unit"] == "audio-s/s" and out["higher_is_better"] is True and out["dtype"] == "bf16"
        assert out["ab"] is None and out["roofline"] is None and out["via_reference_loop"] is None and out["cpu_baseline"] is None
        assert sorted(os.listdir(out_dir)) == DUMPED
        dumps.append({f[:-len(".npy")]: np.load(out_dir / f) for f in DUMPED})
    a, b = dumps
    assert a["losses"].shape == (4,) and all(v.dtype == np.float32 and np.isfinite(v).all() for v in a.values())
    # one step from the same seeded state: equal up to the order of reordered sums
    assert np.allclose(a["losses"], b["losses"], rtol=1e-4) and np.allclose(a["grad_norm"], b["grad_norm"], rtol=1e-3)
    assert np.abs(a["student_params_sample"] - b["student_params_sample"]).max() <= 2.5e-4      # (AdamW lr 1e-4 per step)
