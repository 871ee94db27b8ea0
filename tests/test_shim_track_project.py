"""The projection adapter (include/orbslam3_shim_track_project.hpp: TrackProjectHIP) against the stand-in types of tests/stubs/ and a
recording fake of the C entry points (tests/stubs/shim_track_project_toy.cpp): the header compiles with -Wall -Wextra -Werror; the loop of
Tracking::SearchLocalPoints reaches orbm_frustum_batch with byte-exact arrays (camera, pose record, positions, normals, RAW distances,
skip and bad flags) and writes the seven tracking members, IncreaseVisible and mmProjectPoints back; the last-frame overload projects
through orbm_project_last_batch and hands those arrays to orbm_search_by_projection_last; rig frames go to the reference.  No GPU: the
routing, the marshalling and the write-back are host code."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
f32 = np.float32
CAMERA = [458.5, 457.25, 367.125, 248.375, 47.75, -3.0, -2.0, 755.0, 483.0, float(f32(0.18232156))]


def test_track_project_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_track_project.hpp"\n#include "orbslam3_shim_track_project.hpp"\n'
                   'using namespace ORB_SLAM3;\n'
                   'int main() { TrackProjectFrame F, L; std::vector<MapPoint*> v; TrackProjectHIP<TrackProjectFrame, TrackProjectMapPoint> t(0.9f, true);\n'
                   '  return t.SearchLocalPointsProjectHIP(F, v, 0.5f) + t.SearchByProjection(F, L, 7.f, true); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shim_track_project") / "shim_track_project_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_track_project_toy.cpp"), "-o", str(exe)])

    def run(scenario):
        r = subprocess.run([str(exe), scenario], check=True, capture_output=True, text=True)
        return [ln.split() for ln in r.stdout.splitlines()], r.stderr
    return run


def _rows(out):
    return {ln[0]: (None if ln[1:] == ["NULL"] else [float.fromhex(v) for v in ln[1:]]) for ln in out
            if len(ln) > 1 and ln[0] not in ("orbm_create", "orbm_destroy", "returned", "n_levels", "point", "project_point", "reference") and not ln[0].startswith("orbm_")}


def _desc(rows, seed):
    return [float((i * 7 + seed) & 0xFF) for i in range(rows * 32)]


def _check_camera_and_pose(out, rows):
    """make_frame of the toy: a quarter turn about z, tcw = (0.25, -0.5, 1.5), mOw as GetCameraCenter() returns it"""
    assert rows["camera"] == CAMERA and ["n_levels", "3"] in out
    h = float(f32(np.sqrt(f32(2.0))) * f32(2) / f32(4))               # the stand-in's Quaternion(R): w = s / 4, z = 2 / s, s = 2 sqrt(2)
    z = float(f32(2.0) / (f32(np.sqrt(f32(2.0))) * f32(2)))
    assert rows["q"] == [0.0, 0.0, z, h]
    assert rows["Rcw"] == [0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0] and rows["tcw"] == [0.25, -0.5, 1.5] and rows["Ow"] == [0.5, 0.25, -1.5]


def test_search_local_points_projection(toy):
    out, err = toy("frustum")
    assert [ln[0] for ln in out[:3]] == ["orbm_create", "orbm_create", "orbm_frustum_batch"]
    call = out[2]
    assert call[2] == "2" and call[4] == "1" and call[6] == "5" and call[8] == "5" and float.fromhex(call[10]) == 0.5      # the adapter's own handle, one frame of five rows
    rows = _rows(out[3:])
    _check_camera_and_pose(out, rows)
    k = np.arange(5, dtype=f32)
    assert rows["xyz"] == [float(x) for i in k for x in (f32(0.5) * i, f32(1) - f32(0.25) * i, f32(3) + i)]
    assert rows["normal"] == [float(x) for i in k for x in (f32(0), f32(0.6), f32(0.8) - f32(0.125) * i)]
    assert rows["min_distance"] == [0.5, 1.5, 2.5, 3.5, 4.5] and rows["max_distance"] == [20.0, 21.0, 22.0, 23.0, 24.0]      # raw, not 0.8f * / 1.2f *
    assert rows["skip"] == [0.0, 0.0, 0.0, 1.0, 0.0] and rows["bad"] == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert "xyz len 15" in err and "max_distance len 5" in err        # record_abi's lines
    ret = [ln for ln in out if ln[0] == "returned"][0]
    assert ret[1] == "1" and ret[3] == "0"                           # nToMatch from the library, the reference's isInFrustum never called
    pts = {int(ln[1]): ln for ln in out if ln[0] == "point"}
    val = lambda ln, key: ln[ln.index(key) + 1]
    num = lambda ln, key: float.fromhex(val(ln, key))
    # point 100: in view -- all seven members, IncreaseVisible, mmProjectPoints
    p = pts[100]
    assert val(p, "in_view") == "1" and [num(p, c) for c in ("x", "y", "xr", "depth", "cos")] == [101.5, 11.25, 95.5, 4.5, 0.75] and val(p, "level") == "3" and val(p, "visible") == "1"
    # point 101: rejected after the bounds test -- the flag is cleared, the projection stored, the other members keep their stale values
    p = pts[101]
    assert val(p, "in_view") == "0" and [num(p, c) for c in ("x", "y", "xr", "depth", "cos")] == [202.5, 22.25, 902.0, 903.0, 0.125] and val(p, "level") == "9" and val(p, "visible") == "0"
    p = pts[102]
    assert val(p, "in_view") == "0" and [num(p, c) for c in ("x", "y")] == [-1.0, -1.0] and val(p, "visible") == "0"
    # points 103 (seen in this frame) and 104 (bad): isInFrustum is never reached, nothing is written
    for i in (103, 104):
        p = pts[i]
        assert val(p, "in_view") == "1" and [num(p, c) for c in ("x", "y", "xr", "depth", "cos")] == [900.0, 901.0, 902.0, 903.0, 0.125] and val(p, "visible") == "0"
    assert [(ln[1], float.fromhex(ln[2]), float.fromhex(ln[3])) for ln in out if ln[0] == "project_point"] == [("100", 101.5, 11.25)]


def test_search_local_points_of_a_rig_frame_and_of_no_points(toy):
    out, _ = toy("frustum_rig")
    assert not [ln for ln in out if ln[0] == "orbm_frustum_batch"]
    ret = [ln for ln in out if ln[0] == "returned"][0]
    assert ret[1] == "3" and ret[3] == "3"                           # the reference's loop: three points reach isInFrustum, two are skipped
    assert sorted(ln[1] for ln in out if ln[0] == "project_point") == ["100", "101", "102"]
    out, _ = toy("frustum_empty")
    assert not [ln for ln in out if ln[0] == "orbm_frustum_batch"] and [ln for ln in out if ln[0] == "returned"][0][1] == "0"


@pytest.mark.parametrize("scenario,level_window", [("last", 2), ("last_mono", 0)])
def test_last_frame_projection_feeds_the_search(toy, scenario, level_window):
    out, _ = toy(scenario)
    calls = [ln for ln in out if ln[0].startswith("orbm_") and ln[0] not in ("orbm_create", "orbm_destroy")]
    assert [c[0] for c in calls] == ["orbm_project_last_batch", "orbm_search_by_projection_last"]
    proj, search = calls
    assert proj[2] == "2" and proj[4] == "1" and proj[6] == "5" and proj[8] == "5"
    i0, i1 = out.index(proj), out.index(search)
    rows = _rows(out[i0 + 1:i1])
    _check_camera_and_pose(out, rows)
    # entries 0, 2 and 4 hold points 0, 1 and 3 of the toy; entry 1 has no point, entry 3 is an outlier
    assert rows["has_point"] == [1.0, 0.0, 1.0, 0.0, 1.0]
    xyz = [0.0] * 15
    for entry, k in ((0, 0), (2, 1), (4, 3)):
        xyz[3 * entry:3 * entry + 3] = [float(f32(0.1) * f32(k)), float(f32(-0.2) * f32(k)), 2.0 + k]
    assert rows["xyz"] == xyz
    # the search runs on the owned ORBmatcherHIP's handle with what the projection returned (the fake: entry 2 is behind the camera)
    # and the last frame's own arrays, filled where the projection is valid as ORBmatcherHIP always did
    assert search[2] == "1" and search[4] == "2" and search[6] == "5" and float.fromhex(search[8]) == 7.0 and search[10] == str(level_window) and search[12] == "0"
    rows = _rows(out[i1 + 1:])
    assert rows["valid"] == [1.0, 0.0, 0.0, 0.0, 1.0]
    assert rows["proj_u"] == [50.5, -1.0, -1.0, -1.0, 54.5] and rows["proj_v"] == [60.5, -1.0, -1.0, -1.0, 64.5] and rows["proj_ur"] == [40.5, 0.0, 0.0, 0.0, 44.5]
    assert rows["pts_octave"] == [0.0, 0.0, 0.0, 0.0, 1.0] and rows["pts_angle"] == [130.0, 0.0, 0.0, 0.0, 134.0]
    assert rows["has_obs"] == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert rows["pts_desc"] == _desc(1, 60) + [0.0] * 96 + _desc(1, 63)
    assert rows["cur_x"] == [11.5, 12.5] and rows["occupied"] == [0.0, 1.0]
    # the fake: feature 0 <- entry 3 (point 2 of the toy), feature 1 nulled
    assert [ln for ln in out if ln[0] == "returned"][0] == ["returned", "1", "slots", "2", "-1"]


def test_last_frame_search_of_a_rig_frame_goes_to_the_reference(toy):
    out, _ = toy("last_rig")
    assert not [ln for ln in out if ln[0] in ("orbm_project_last_batch", "orbm_search_by_projection_last")]
    assert ["reference", "SearchByProjection", "last", "frame"] in out and [ln for ln in out if ln[0] == "returned"][0][1] == "-8"
