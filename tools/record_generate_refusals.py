"""Records which argument combinations `generate` and `seek_decode` refuse, and the seek loop's schedules on the planted model
-> tests/golden/generate_refusals.json (the cases: tests/generate_refusals_cases.py; replayed by tests/test_generate_refusals.py).

The file pins the behaviour of ONE commit across later restructuring of the host code: run this on that commit (with the cases
module and this tool copied in), commit the file, and do not regenerate it from the restructured code.  CPU only.
Usage:  python tools/record_generate_refusals.py [--commit SHA]     (SHA defaults to `git rev-parse HEAD`)
"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "generate_refusals.json")


def main():
    from tests import generate_refusals_cases as rc
    if "--commit" in sys.argv:
        sha = sys.argv[sys.argv.index("--commit") + 1]
    else:
        sha = subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=ROOT, text=True).strip()
    ms = rc.models()
    res = {"tool": "tools/record_generate_refusals.py", "recorded_from_commit": sha,
           "generate": rc.generate_outcomes(ms), "seek_decode": rc.seek_outcomes(ms), "schedules": rc.schedule_logs()}
    for part in ("generate", "seek_decode"):
        n_enc = sum(1 for v in res[part].values() if v == "encoder")
        print(f"{part}: {len(res[part])} combinations, {len(res[part]) - n_enc} refused, {n_enc} reach the encoder")
    with open(OUT, "w") as f:
        json.dump(res, f, indent=0, sort_keys=True)
        f.write("\n")
    print(OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
