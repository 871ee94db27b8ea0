#!/usr/bin/env python3
"""Records tests/golden/shim_abi/<toy>.txt: what the adapters of an include/ directory hand to the C ABI in every scenario of
tests/shim_abi_cases.py (the stderr dumps of tests/stubs/record_abi.hpp; for the inertial toy also the write-back on stdout).

    git archive --prefix=parent/ <commit> include | tar -x -C <scratch>
    python tools/make_shim_abi_golden.py --include-dir <scratch>/parent/include --commit <commit>

The toys and stand-ins are this tree's, the headers under test are those of --include-dir: that is how a refactor of the adapters is
compared with the commit before it.  Two of the toys link the built library (for the argument checks)."""
import argparse
import os
import pathlib
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import shim_abi_cases as cases  # noqa: E402

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--include-dir", required=True)
    ap.add_argument("--commit", required=True, help="the commit the headers were taken from; named in each file's first line")
    a = ap.parse_args()
    os.makedirs(cases.GOLDEN, exist_ok=True)
    with tempfile.TemporaryDirectory() as tmp:
        for toy in cases.TOYS:
            body = cases.record(toy, os.path.abspath(a.include_dir), pathlib.Path(tmp))
            with open(os.path.join(cases.GOLDEN, toy + ".txt"), "w") as f:
                f.write("# tests/stubs/%s.cpp against include/ of commit %s\n%s" % (toy, a.commit, body))
            print(toy, len(body.splitlines()), "lines")
