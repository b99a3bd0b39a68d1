#!/usr/bin/env python3
"""Writes tests/golden/selection_cases.json: what HipMaskAndReplaceDiffusion selects, reports, logs, builds and releases in every
scenario of tests/_selection_cases.py, on the fake engines of tests/_fake_engine.py (CPU only, a few seconds).

The file is a characterization of the code it is run on: tests/test_selection_cases.py replays the scenarios and compares, so
regenerate it only where a change of the recorded behaviour is the point of the change.

    python tools/make_selection_golden.py [--check]
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (os.path.join(ROOT, "tests"), ROOT):
    if p not in sys.path:
        sys.path.insert(0, p)
OUT = os.path.join(ROOT, "tests", "golden", "selection_cases.json")


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--check", action="store_true", help="compare with the committed file instead of writing it")
    a = ap.parse_args()
    import _selection_cases as SC

    import layout_dm_amd.diffusion as D

    got = {c["name"]: dict(c, outcome=SC.run_case(D, c)) for c in SC.cases()}
    text = json.dumps(got, indent=1, sort_keys=True) + "\n"
    if a.check:
        same = open(OUT).read() == text
        print("identical" if same else "DIFFERENT")
        return 0 if same else 1
    with open(OUT, "w") as f:
        f.write(text)
    print(f"{OUT}: {len(got)} scenarios, {len(text)} bytes")
    return 0


if __name__ == "__main__":
    sys.exit(main())
