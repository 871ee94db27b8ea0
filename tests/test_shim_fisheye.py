"""include/orbslam3_shim_fisheye.hpp (ComputeStereoFishEyeMatchesHIP) against the stand-in types of tests/stubs/ and a recording fake
of the C entry point (tests/stubs/shim_fisheye_toy.cpp): the header compiles with -Wall -Wextra -Werror, the frame's key points,
descriptors, counts, level table and rig arrive at the C ABI byte for byte (also from descriptor rows that are not contiguous), the
five members and mnCloseMPs are written from what the call returns, and a rig whose second camera is missing or not a fisheye goes to
the reference's own function.  No GPU: marshalling and write-back are host code (tests/test_fisheye_stereo_gpu.py runs the toy on the
device)."""
import os
import subprocess

import numpy as np
import pytest

import fisheye_stereo_cases as cases
import shim_fisheye_common as common

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")


def test_fisheye_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_fisheye.hpp"\n#include "orbslam3_shim_fisheye.hpp"\n'
                   'template void ORB_SLAM3::ComputeStereoFishEyeMatchesHIP<ORB_SLAM3::KannalaBrandt8Rig, ORB_SLAM3::RigFrame>(ORB_SLAM3::RigFrame&, orbm_matcher*);\n'
                   'int main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    src.write_text('#include "orbslam3_shim_fisheye.hpp"\nint main() { return 0; }\n')      # without the macro: the POD half only
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    return common.build_toy(tmp_path_factory.mktemp("shim_fisheye"), real=False)


@pytest.mark.parametrize("scenario", ["rig", "noncontiguous"])
def test_marshalling_round_trip_and_write_back(toy, scenario, tmp_path, pkg):
    import importlib
    capi = importlib.import_module("orb_slam3-1_amd.capi")
    c = cases.frame_case("frame_a")
    sent = common.case_bytes(capi, c)
    out = common.run_toy(toy, scenario, sent, tmp_path)
    n_l, n_r = len(c["kps_l"]), len(c["kps_r"])
    assert out["calls"] == [["orbm_stereo_fisheye", "handle", "7", "diagnostics", "0"]]
    assert (out["reference_calls"], out["close"]) == (0, 0) and out["sizes"] == [n_l, n_r, n_l, n_l, n_l]
    # what the C ABI received: the case file's bytes, the rig as an OrbxFisheyeRig
    got = open(tmp_path / "dump.bin", "rb").read()
    rig = bytes(capi.fisheye_rig(c["rig"]))
    assert got[:20] == sent[:20] and got[20:20 + 184] == rig and got[20 + 184:] == sent[20 + 120:]
    # the members: the fake's pattern, mvuRight all -1
    assert np.array_equal(out["left_to_right"], np.arange(n_l) + 100) and np.array_equal(out["right_to_left"], np.arange(n_r) + 200)
    assert np.array_equal(out["depth"], 0.5 * np.arange(n_l)) and (out["u_right"] == -1).all()
    assert np.array_equal(out["p3d"], np.arange(n_l)[:, None] + 0.25 * np.arange(3)[None, :])


@pytest.mark.parametrize("scenario", ["pinhole_right", "no_right"])
def test_other_rigs_go_to_the_reference(toy, scenario, tmp_path, pkg):
    import importlib
    capi = importlib.import_module("orb_slam3-1_amd.capi")
    out = common.run_toy(toy, scenario, common.case_bytes(capi, cases.frame_case("frame_b")), tmp_path)
    assert out["calls"] == [] and out["reference_calls"] == 1 and not os.path.exists(tmp_path / "dump.bin")
    assert out["close"] == 17 and out["sizes"] == [0, 0, 0, 3, 0]                   # nothing written by the adapter
