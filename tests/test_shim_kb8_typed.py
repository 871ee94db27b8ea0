"""The KannalaBrandt8 adapters (include/orbslam3_shim_kb8.hpp: PoseOptimizationAnyCamHIP, LocalBundleAdjustmentAnyCamHIP) against the
stand-in types of tests/stubs/ and a recording fake of the C entry points (tests/stubs/shim_kb8_toy.cpp): the header compiles with
-Wall -Wextra -Werror, one monocular fisheye camera goes to the device calls with the camera set before the solve and reset after
it and the eight parameters passed in order, and mixed cameras, a second camera or a pinhole go to the existing adapter.
No GPU: the routing, the marshalling and the write-back are host code."""
import os
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
PARAMS = [float(np.float32(v)) for v in (190.98, 190.97, 254.93, 256.90, 0.0034, 0.0007, -0.0020, 0.0002)]     # floats promoted to double


def test_kb8_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_kb8.hpp"\n#include "orbslam3_shim_kb8.hpp"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shim_kb8") / "shim_kb8_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_kb8_toy.cpp"), "-o", str(exe)])
    return lambda scenario: [ln.split() for ln in subprocess.run([str(exe), scenario], check=True, capture_output=True, text=True).stdout.splitlines()]


def _camera(line):
    return [float.fromhex(v) for v in line[3:]]


def test_pose_with_one_fisheye_camera_runs_on_the_device(toy):
    out = toy("pose_kb8")
    assert [ln[0] for ln in out] == ["pose_create", "pose_set_camera_kb8", "pose_optimize", "pose_set_camera_kb8", "returned",
                                     "pose_set_camera_kb8", "pose_optimize", "pose_set_camera_kb8", "returned"]
    assert _camera(out[1]) == PARAMS and out[3][3] == "NULL" and _camera(out[5]) == PARAMS and out[7][3] == "NULL"
    assert len({ln[2] for ln in out if ln[0] != "returned"}) == 1                   # one handle per thread, reused by the second frame
    call = out[2]
    assert call[call.index("n") + 1] == "5" and call[call.index("stereo") + 1] == "0"
    assert float.fromhex(call[call.index("huber") + 1]) == float(np.float32(np.sqrt(np.float32(5.991))))
    assert [float.fromhex(v) for v in call[-3:]] == [100.0, 50.0, -1.0]             # the first feature with a map point, monocular
    # write-back: pose moved by the fake; the fake's flags (every third edge, from the second) go to the features 0 2 3 5 6 that hold
    # a map point, features 1 and 4 keep what they had (true in the toy), as in the reference
    assert out[4][1] == "4" and float.fromhex(out[4][3]) == 0.5
    assert out[4][5:] == ["0", "1", "1", "0", "1", "0", "1"]


def test_pose_with_other_cameras_goes_to_the_existing_adapter(toy):
    out = toy("pose_pinhole")                   # PoseOptimizationHIP: the device, and no camera is ever set
    assert [ln[0] for ln in out] == ["pose_create", "pose_optimize", "returned"]
    out = toy("pose_stereo_obs")                # a feature with mvuRight >= 0: not a monocular frame, the existing adapter takes it
    assert [ln[0] for ln in out] == ["pose_create", "pose_optimize", "returned"] and out[1][out[1].index("stereo") + 1] == "1"
    out = toy("pose_rig")                       # a second camera: PoseOptimizationHIP hands the rig to the reference
    assert [ln[0] for ln in out] == ["reference", "returned"] and out[1][1] == "-7"


def test_window_with_one_fisheye_camera_runs_on_the_device(toy):
    out = toy("lba_kb8")
    assert [ln[0] for ln in out[:4]] == ["lba_create", "lba_set_camera_kb8", "lba_solve", "lba_set_camera_kb8"]
    assert _camera(out[1]) == PARAMS and out[3][3] == "NULL"
    call = out[2]
    val = lambda k: call[call.index(k) + 1]
    assert (val("poses"), val("fixed"), val("points"), val("edges"), val("stereo"), val("iters")) == ("4", "2", "3", "7", "0", "10")
    assert float.fromhex(val("lambda")) == 0.0
    assert out[4] == ["counters", "2", "3", "-1", "7", "change", "1"]              # num_MPs is never assigned, as in the reference
    kf = {int(ln[1]): ln for ln in out if ln[0] == "kf"}
    assert [kf[i][3] for i in range(4)] == ["1", "1", "1", "0"]                     # the fixed camera outside the window is not written
    mp = [ln for ln in out if ln[0] == "mp"]
    assert [float.fromhex(ln[3]) for ln in mp] == [1.0, 2.0, 3.0] and all(ln[7] == "1" for ln in mp)
    assert sum(int(ln[5]) for ln in mp) == 2                                        # chi2 6.5 > 5.991 and one edge behind the camera


@pytest.mark.parametrize("scenario", ["lba_mixed", "lba_rig", "lba_fixed_pinhole", "lba_stereo_obs"])
def test_window_with_other_cameras_goes_to_the_existing_adapter(toy, scenario):
    """a coefficient that differs, a key frame with mpCamera2, a pinhole camera among the fixed cameras (found by the walk only),
    an observation with mvuRight >= 0 (also found by the walk only):
    LocalBundleAdjustmentHIP, which hands all three to the reference; nothing is set, solved or written by the new adapter"""
    out = toy(scenario)
    assert out[0] == ["reference", "LocalBundleAdjustment"]
    assert not [ln for ln in out if ln[0].startswith("lba_")]
    assert out[1] == ["counters", "-1", "-1", "-1", "-1", "change", "0"]
    assert all(ln[3] == "0" for ln in out if ln[0] == "kf")
