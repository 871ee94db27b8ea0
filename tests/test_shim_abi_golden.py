"""Every struct the drop-in adapters (include/orbslam3_shim*.hpp) hand to the C ABI, against recordings taken with the headers of an
earlier commit (tests/golden/shim_abi/, made by tools/make_shim_abi_golden.py; the first line of each file names the commit): the toys
of tests/stubs/ are built against the tree's headers, every scenario of tests/shim_abi_cases.py is run, and the recording fakes' dumps
(tests/stubs/record_abi.hpp: every scalar as %a, every array as length, FNV-1a hash, first and last element) must equal the golden byte
for byte -- for the inertial toy, the only test that executes LocalInertialBAHIP and PoseInertialOptimizationHIP, also what it wrote
back.  No GPU: marshalling is host code."""
import os

import pytest

import shim_abi_cases as cases

INC = os.path.join(cases.ROOT, "include")


@pytest.mark.parametrize("toy", sorted(cases.TOYS))
def test_adapters_hand_the_recorded_bytes_to_the_c_abi(toy, tmp_path, pkg):
    with open(os.path.join(cases.GOLDEN, toy + ".txt")) as f:
        head, golden = f.read().split("\n", 1)
    assert head.startswith("# ") and "commit" in head
    got = cases.record(toy, INC, tmp_path)
    want = dict(s.split("\n", 1) for s in golden.split("== ")[1:])
    have = dict(s.split("\n", 1) for s in got.split("== ")[1:])
    assert list(have) == list(want) and len(have) == len(cases.TOYS[toy][0](tmp_path))
    for name in want:
        assert have[name] == want[name], "%s %s: the adapter hands over other bytes than the recorded ones" % (toy, name)
    assert got == golden
