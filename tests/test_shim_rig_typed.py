"""The two-camera fisheye adapters (include/orbslam3_shim_rig.hpp: PoseOptimizationRigHIP, LocalBundleAdjustmentRigHIP) against the
stand-in types of tests/stubs/ and a recording fake of the C entry points (tests/stubs/shim_rig_toy.cpp): the header compiles with
-Wall -Wextra -Werror; a rig frame and a rig window reach the device calls with the rig set before the solve and reset after it; the
edge kinds, observations and octaves are in the reference's order; the write-back reaches the right features; and a differing Trl
or parameter on a fixed key frame, a pinhole second camera and an observation with mvuRight >= 0 go to the existing adapter.
No GPU: the routing, the marshalling and the write-back are host code."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
f32 = lambda v: float(np.float32(v))
LEFT = [f32(v) for v in (190.98, 190.97, 254.93, 256.90, 0.0034, 0.0007, -0.0020, 0.0002)]       # floats promoted to double
RIGHT = [f32(v) for v in (189.40, 189.35, 252.10, 259.30, 0.0030, 0.0011, -0.0017, 0.00015)]
EDGE_RIGHT = 2


def test_rig_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_rig.hpp"\n#include "orbslam3_shim_rig.hpp"\n'
                   'using namespace ORB_SLAM3;\n'
                   'int main() { RigPoseFrame F; RigKeyFrame K; Map m; int a = 0, b = 0, c = 0, d = 0;\n'
                   '  LocalBundleAdjustmentRigHIP<KannalaBrandt8, RigKeyFrame>(&K, nullptr, &m, a, b, c, d);\n'
                   '  return PoseOptimizationRigHIP<KannalaBrandt8, RigPoseFrame>(&F); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shim_rig") / "shim_rig_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_rig_toy.cpp"), "-o", str(exe)])
    return lambda scenario: [ln.split() for ln in subprocess.run([str(exe), scenario], check=True, capture_output=True, text=True).stdout.splitlines()]


def _hex(tokens):
    return [float.fromhex(v) for v in tokens]


def _check_rig(line, trl):
    """the rig as set: left and right parameters in order, then Trl's quaternion (xyzw) and translation as the toy's own pose_in of it"""
    v = _hex(line[3:])
    assert v[:8] == LEFT and v[8:16] == RIGHT
    assert v[16:] == _hex(trl[1:]) and len(v) == 23
    assert abs(sum(q * q for q in v[16:20]) - 1) < 1e-6 and v[20] == f32(-0.1)


def test_rig_frame_runs_on_the_device(toy):
    out = toy("pose_rig")
    calls = [ln for ln in out if ln[0] not in ("pose_edge", "toy_trl")]
    assert [ln[0] for ln in calls] == ["pose_create", "pose_set_rig_kb8", "pose_optimize", "pose_set_rig_kb8", "returned"]
    _check_rig(calls[1], out[0])
    assert calls[3][3] == "NULL" and len({ln[2] for ln in calls[:4]}) == 1          # reset after the solve, on the same handle
    assert calls[2][calls[2].index("n") + 1] == "5"
    assert float.fromhex(calls[2][calls[2].index("huber") + 1]) == float(np.float32(np.sqrt(np.float32(5.991))))
    e = [ln for ln in out if ln[0] == "pose_edge"]
    # features 0 2 3 (left image: mvKeys, not mvKeysUn, which the toy sets to 900 / 800) then 4 6 (right image: mvKeysRight[0], [2])
    assert [int(ln[3]) for ln in e] == [0, 0, 0, EDGE_RIGHT, EDGE_RIGHT]
    assert [_hex(ln[5:8]) for ln in e] == [[100.0, 50.0, -1.0], [102.0, 52.0, -1.0], [103.0, 53.0, -1.0], [300.0, 250.0, -1.0], [302.0, 252.0, -1.0]]
    # the octave of the key point the edge was made from: left octaves 0 0 1, right octaves 2 0
    assert [float.fromhex(ln[9]) for ln in e] == [1.0, 1.0, f32(0.69), f32(0.48), 1.0]
    assert [float.fromhex(ln[11]) for ln in e] == [2.0, 3.0, 4.0, 5.0, 6.0]         # the map points in feature order
    # write-back over both lists: the fake flags edges 1 and 4 = features 2 (left) and 6 (right); features 1 and 5 hold no map point
    # and keep what they had (true in the toy)
    ret = calls[4]
    assert ret[1] == "4" and float.fromhex(ret[3]) == 0.5
    assert ret[5:] == ["0", "1", "1", "0", "0", "1", "1"]


@pytest.mark.parametrize("scenario", ["pose_pinhole2", "pose_stereo_obs"])
def test_other_frames_go_to_the_existing_adapter(toy, scenario):
    """a pinhole second camera; a left feature with a map point and mvuRight >= 0: PoseOptimizationAnyCamHIP, which hands a frame
    with mpCamera2 on to the reference; the new adapter sets, solves and writes nothing"""
    out = toy(scenario)
    assert [ln[0] for ln in out] == ["toy_trl", "reference", "returned"] and out[2][1] == "-7"
    assert out[2][5:] == ["1"] * 7


def test_rig_window_runs_on_the_device(toy):
    out = toy("lba_rig")
    calls = [ln for ln in out if ln[0] not in ("lba_edge", "toy_trl")]
    assert [ln[0] for ln in calls[:4]] == ["lba_create", "lba_set_rig_kb8", "lba_solve", "lba_set_rig_kb8"]
    _check_rig(calls[1], out[0])
    assert calls[3][3] == "NULL" and len({ln[2] for ln in calls[:4]}) == 1
    call = calls[2]
    val = lambda k: call[call.index(k) + 1]
    assert (val("poses"), val("fixed"), val("points"), val("edges"), val("iters")) == ("4", "2", "3", "9", "10")
    assert float.fromhex(val("lambda")) == 0.0
    # the reference's order: map points in list order (11, 12, 10), the observations of each by key frame; per observation the left
    # edge (mvKeysUn[left], octave 0) and then the right edge (mvKeysRight[right - NLeft], octave 1 -> mvInvLevelSigma2[1])
    un = lambda kf, k: [10.0 * kf + k, 20.0 * kf + k, -1.0]
    rt = lambda kf, k: [100.0 + 10.0 * kf + k, 200.0 + 20.0 * kf + k, -1.0]
    want = [(1, 1, 0, un(1, 1)), (1, 1, 2, rt(1, 1)), (2, 1, 0, un(2, 1)),
            (0, 2, 2, rt(0, 1)), (2, 2, 0, un(2, 2)), (2, 2, 2, rt(2, 0)), (3, 2, 0, un(3, 2)),
            (0, 0, 0, un(0, 0)), (1, 0, 2, rt(1, 0))]
    e = [ln for ln in out if ln[0] == "lba_edge"]
    assert [(int(ln[3]), int(ln[5]), int(ln[7]), _hex(ln[9:12])) for ln in e] == want
    assert [float.fromhex(ln[13]) for ln in e] == [1.0 if k == 0 else f32(0.69) for _, _, k, _ in want]
    assert calls[4] == ["counters", "2", "3", "-1", "9", "change", "1"]            # num_MPs is never assigned, as in the reference
    kf = {int(ln[1]): ln for ln in out if ln[0] == "kf"}
    assert [kf[i][3] for i in range(4)] == ["1", "1", "1", "0"]                     # the fixed camera outside the window is not written
    mp = [ln for ln in out if ln[0] == "mp"]
    assert [float.fromhex(ln[3]) for ln in mp] == [1.0, 2.0, 3.0] and all(ln[7] == "1" for ln in mp)
    # erased: edge 2 (left, chi2 6.5) -> point 1; edge 4 (left, behind the camera) and edge 5 (right, chi2 6.5: above 5.991, below the
    # 7.815 of a rectified-stereo edge) -> point 2 twice, the same (key frame, point) pair from the left list and from the right list
    assert [int(ln[5]) for ln in mp] == [0, 1, 2]


@pytest.mark.parametrize("scenario", ["lba_trl", "lba_param", "lba_pinhole2", "lba_stereo_obs"])
def test_other_windows_go_to_the_existing_adapter(toy, scenario):
    """another Trl and another right-camera coefficient on the fixed key frame (found by the walk only), a pinhole second camera, an
    edge-bearing observation with mvuRight >= 0: LocalBundleAdjustmentAnyCamHIP, which hands a window with mpCamera2 on to the
    reference; nothing is set, solved or written by the new adapter"""
    out = toy(scenario)
    assert out[1] == ["reference", "LocalBundleAdjustment"]
    assert not [ln for ln in out if ln[0].startswith("lba_")]
    assert out[2] == ["counters", "-1", "-1", "-1", "-1", "change", "0"]
    assert all(ln[3] == "0" for ln in out if ln[0] == "kf")
