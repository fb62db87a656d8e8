"""Generates tests/golden/reference_calls.json: the answers of the reference's own functions to the calls the CPU tests
make, so that those tests run where the reference tree is absent (where it is present they re-derive every answer and
compare it with the recorded one).  Each function is exec'd from the reference at run time by the test helpers below:
  labels_trials          prepare_train_dataset (run_distillation.py:1167-1229), tests/test_labels.py's 40 trials
  decay_parameter_names  get_parameter_names + the bias rule (760-778, 1386-1391) on the micro drop-in student
  collator               DataCollatorSpeechSeq2SeqWithPadding on tests/test_oracle.py's two-sequence batch
  student_init           init_student_model_from_teacher (create_student_model.py:92-216): per-tensor digests
Run in the build container only: python oracle/gen_golden_reference_calls.py"""
import json
import os
import sys
import tempfile
from pathlib import Path

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import test_labels as tl  # noqa: E402
from tests import test_oracle as to  # noqa: E402
from tests import test_student_init as tsi  # noqa: E402

out = {"labels_trials": [tl.reference_labels(toks, prevs, 100 + trial, tp, cp)
                         for trial, toks, prevs, tp, cp in tl.reference_trials()],
       "decay_parameter_names": sorted(tl.reference_decay_names(tl.micro_student_module()))}
labels, dec_in = to.reference_collate()
out["collator"] = {"labels": labels.tolist(), "decoder_input_ids": dec_in.tolist()}
out["student_init"] = []
for kw in tsi.CASES:
    with tempfile.TemporaryDirectory() as d:
        out["student_init"].append({"kw": kw, "digests": tsi.reference_student_digests(Path(d), kw)})
path = os.path.join(ROOT, "tests", "golden", "reference_calls.json")
with open(path, "w") as f:
    json.dump(out, f, separators=(",", ":"))
print("wrote", path, os.path.getsize(path), "bytes")
