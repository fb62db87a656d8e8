"""`generate` and `seek_decode` refuse what they refused at the commit tests/golden/generate_refusals.json was recorded from
(tools/record_generate_refusals.py; the cases are tests/generate_refusals_cases.py): the same exception class, on the same side of
the encoder, for no atom, every atom and every pair of atoms in every context -- and the seek loop's two schedules log, on the
planted model of tests/seek_slots_cases.py, what they logged there, entry for entry.  CPU (oracle.ref_ops, fp32)."""
import json
import os

import pytest

from tests import generate_refusals_cases as rc

GOLD = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "generate_refusals.json")))


@pytest.fixture(scope="module")
def ms():
    return rc.models()


def compare(got, want):
    assert sorted(got) == sorted(want)
    wrong = {k: (got[k], want[k]) for k in want if got[k] != want[k]}
    assert not wrong, (len(wrong), dict(list(wrong.items())[:8]))
    refused = sum(1 for v in want.values() if v != "encoder" and v["exception"] is not None)
    reached = sum(1 for v in want.values() if v == "encoder")
    return refused, reached


def test_generate_refuses_what_the_recorded_commit_refused(ms):
    refused, reached = compare(rc.generate_outcomes(ms), GOLD["generate"])
    print(f"generate: {refused} refusals, {reached} combinations reach the encoder (recorded from {GOLD['recorded_from_commit']})")
    assert refused >= 150 and reached >= 100                       # the file is not hollow


def test_seek_decode_refuses_what_the_recorded_commit_refused(ms):
    refused, reached = compare(rc.seek_outcomes(ms), GOLD["seek_decode"])
    print(f"seek_decode: {refused} refusals, {reached} combinations reach the encoder")
    assert refused >= 150 and reached >= 100
    # the left-pad refusals depend on more than one utterance: both sides are in the file
    key = "lockstep | condition_on_prev_tokens | sequence_bias"
    assert GOLD["seek_decode"][f"B=1 | {key}"] == "encoder" and GOLD["seek_decode"][f"B=2 | {key}"]["exception"] == "NotImplementedError"


def test_both_schedules_log_what_they_logged_at_the_recorded_commit():
    """Encoder batches, `retrieve_segment` calls, window ends and teacher-forced passes in order, `last_seek_stats`, the segments
    and `last_window_scores`: all equal to what the file holds (floats as JSON writes them, which is exact for a double)."""
    want = GOLD["schedules"]
    got = json.loads(json.dumps(rc.schedule_logs(want["thresholds"])))      # (tuples as the file holds them)
    assert sorted(got) == sorted(want)
    legs = [k for k in want if k != "thresholds"]
    assert len(legs) == 6
    for leg in legs:
        for part in ("log", "stats", "segments", "window_scores"):
            assert got[leg][part] == want[leg][part], (leg, part)
    # what the scenario is for: several windows per utterance, skipped windows under the thresholds, no rescoring pass on slots
    assert ["decode"] in want["thresholds | lockstep"]["log"] and ["decode"] not in want["thresholds | slots=2"]["log"]
    assert want["thresholds | lockstep"]["window_scores"] and not want["plain | lockstep"]["window_scores"]
    assert max(len(row) for row in want["plain | lockstep"]["segments"]) > 1
