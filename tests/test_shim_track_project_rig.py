"""The rig projection adapter (include/orbslam3_shim_track_project_rig.hpp: TrackProjectRigHIP) against the stand-in types of tests/stubs/
and a recording fake of the C entry points (tests/stubs/shim_track_project_rig_toy.cpp): the header compiles with -Wall -Wextra -Werror;
the loop of Tracking::SearchLocalPoints for a rig frame reaches orbm_frustum_rig_batch with byte-exact arrays (both cameras, mTrl, the rig
frame record, positions, normals, RAW distances, skip and bad flags) AND the stale tracking members of every map point, and writes back
what the library returned -- fresh values for a camera that sees the point, the stale ones for a camera that does not; the last-frame
overload projects through orbm_project_last_rig_batch and hands those arrays to orbm_search_by_projection_last_rig; a frame that is no
rig frame goes to the pinhole adapter.  No GPU: the routing, the marshalling and the write-back are host code."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
f32 = np.float32
H = float(f32(np.sqrt(f32(2.0))) * f32(2) / f32(4))                 # the stand-in's Quaternion(R) of a quarter turn: w = s / 4, s = 2 sqrt(2)
Z = float(f32(2.0) / (f32(np.sqrt(f32(2.0))) * f32(2)))


def test_track_project_rig_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_track_project_rig.hpp"\n#include "orbslam3_shim_track_project_rig.hpp"\n'
                   'using namespace ORB_SLAM3;\n'
                   'int main() { TrackProjectRigFrame F, L; std::vector<MapPoint*> v; TrackProjectRigHIP<TrackProjectRigFrame, TrackProjectRigMapPoint> t(0.9f, true);\n'
                   '  return t.SearchLocalPointsProjectHIP(F, v, 0.5f) + t.SearchByProjection(F, L, 7.f, true); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shim_track_project_rig") / "shim_track_project_rig_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_track_project_rig_toy.cpp"), "-o", str(exe)])

    def run(scenario):
        r = subprocess.run([str(exe), scenario], check=True, capture_output=True, text=True)
        return [ln.split() for ln in r.stdout.splitlines()], r.stderr
    return run


def _rows(out):
    return {ln[0]: (None if ln[1:] == ["NULL"] else [float.fromhex(v) for v in ln[1:]]) for ln in out
            if len(ln) > 1 and ln[0] not in ("orbm_create", "orbm_destroy", "returned", "n_levels", "point", "project_point") and not ln[0].startswith("orbm_")}


def _desc(rows, seed):
    return [float((i * 7 + seed) & 0xFF) for i in range(rows * 32)]


def _check_camera_and_pose(out, rows):
    """make_frame of the toy: Tcw a quarter turn about z with tcw = (0.25, -0.5, 1.5); Trl a quarter turn about y with trl = (-0.125, 0, 0.0625)"""
    assert rows["cam_left"] == [190.5, 191.5, 254.0, 256.0, 0.5, 0.25, -0.125, 0.0625] and rows["cam_right"] == [188.5, 189.5, 252.0, 255.0, 0.25, 0.125, -0.0625, 0.03125]
    assert rows["Rrl"] == [0.0, 0.0, -1.0, 0.0, 1.0, 0.0, 1.0, 0.0, 0.0] and rows["trl"] == [-0.125, 0.0, 0.0625] and rows["tlr"] == [0.0625, 0.0, 0.125]
    assert rows["q_rl"] == [0.0, -Z, 0.0, H]
    assert rows["bounds"] == [-3.0, -2.0, 515.0, 514.0, float(f32(0.18232156))] and ["n_levels", "3"] in out
    assert rows["q"] == [0.0, 0.0, Z, H]
    assert rows["Rcw"] == [0.0, -1.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0] and rows["tcw"] == [0.25, -0.5, 1.5] and rows["Ow"] == [0.5, 0.25, -1.5]
    assert rows["Rwc"] == [0.0, 1.0, 0.0, -1.0, 0.0, 0.0, 0.0, 0.0, 1.0]                   # GetRotationInverse(), not a transpose made by the adapter
    # the reference's expressions for the right camera: mR = Rrl * mRcw, mt = Rrl * mtcw + trl, twc = mRwc * tlr + mOw
    assert rows["R_r"] == [0.0, 0.0, -1.0, 1.0, 0.0, 0.0, 0.0, -1.0, 0.0]
    assert rows["t_r"] == [-1.5 - 0.125, -0.5, 0.25 + 0.0625] and rows["Ow_r"] == [0.5, 0.25 - 0.0625, -1.5 + 0.125]


def test_search_local_points_of_a_rig_frame(toy):
    out, err = toy("frustum")
    calls = [ln for ln in out if ln[0].startswith("orbm_") and ln[0] not in ("orbm_create", "orbm_destroy")]
    assert [c[0] for c in calls] == ["orbm_frustum_rig_batch"]
    call = calls[0]
    assert call[2] == "5" and call[4] == "1" and call[6] == "6" and call[8] == "6" and float.fromhex(call[10]) == 0.5      # the adapter's own handle, one frame of six rows
    rows = _rows(out[out.index(call) + 1:])
    _check_camera_and_pose(out, rows)
    k = np.arange(6, dtype=f32)
    assert rows["xyz"] == [float(x) for i in k for x in (f32(0.5) * i, f32(1) - f32(0.25) * i, f32(3) + i)]
    assert rows["normal"] == [float(x) for i in k for x in (f32(0), f32(0.6), f32(0.8) - f32(0.125) * i)]
    assert rows["min_distance"] == [0.5 + i for i in range(6)] and rows["max_distance"] == [20.0 + i for i in range(6)]      # raw, not 0.8f * / 1.2f *
    assert rows["skip"] == [0.0, 0.0, 0.0, 0.0, 1.0, 0.0] and rows["bad"] == [0.0, 0.0, 0.0, 0.0, 0.0, 1.0]
    # the stale members of every point travel in
    for name, base in (("in_proj_u", 900), ("in_proj_v", 910), ("in_track_depth", 920), ("in_proj_u_r", 930), ("in_proj_v_r", 940), ("in_track_depth_r", 950)):
        assert rows[name] == [float(base + i) for i in range(6)], name
    assert rows["in_view_cos"] == [0.125] * 6 and rows["in_view_cos_r"] == [0.25] * 6 and rows["in_pred_level"] == [9.0] * 6 and rows["in_pred_level_r"] == [8.0] * 6
    assert "xyz len 18" in err and "in_track_depth_r len 6" in err    # record_abi's lines
    ret = [ln for ln in out if ln[0] == "returned"][0]
    assert ret[1] == "3" and ret[3] == "0"                           # nToMatch from the library, the reference's isInFrustum never called
    pts = {int(ln[1]): ln for ln in out if ln[0] == "point"}
    val = lambda ln, key: ln[ln.index(key) + 1]
    num = lambda ln, key: float.fromhex(val(ln, key))
    L, Rk = ("x", "y", "depth", "cos"), ("xr", "yr", "depth_r", "cos_r")
    # point 100: both cameras -- ten members, one IncreaseVisible
    p = pts[100]
    assert val(p, "in_view") == "1" and [num(p, c) for c in L] == [101.5, 11.25, 4.5, 0.75] and val(p, "level") == "2"
    assert val(p, "in_view_r") == "1" and [num(p, c) for c in Rk] == [301.5, 31.25, 6.5, 0.875] and val(p, "level_r") == "1" and val(p, "visible") == "1"
    # point 101: the left camera only -- the right members keep what an earlier frame wrote, but for the flag and the level
    p = pts[101]
    assert val(p, "in_view") == "1" and [num(p, c) for c in L] == [102.5, 12.25, 5.5, 0.75] and val(p, "level") == "2"
    assert val(p, "in_view_r") == "0" and [num(p, c) for c in Rk] == [931.0, 941.0, 951.0, 0.25] and val(p, "level_r") == "-1" and val(p, "visible") == "1"
    # point 102: the right camera only -- the LEFT mTrackDepth stays stale, and the search will read it
    p = pts[102]
    assert val(p, "in_view") == "0" and [num(p, c) for c in L] == [902.0, 912.0, 922.0, 0.125] and val(p, "level") == "-1"
    assert val(p, "in_view_r") == "1" and [num(p, c) for c in Rk] == [303.5, 33.25, 8.5, 0.875] and val(p, "level_r") == "1" and val(p, "visible") == "1"
    # point 103: neither
    p = pts[103]
    assert val(p, "in_view") == "0" and val(p, "in_view_r") == "0" and [num(p, c) for c in L + Rk] == [903.0, 913.0, 923.0, 0.125, 933.0, 943.0, 953.0, 0.25]
    assert val(p, "level") == "-1" and val(p, "level_r") == "-1" and val(p, "visible") == "0"
    # points 104 (seen in this frame) and 105 (bad): isInFrustum is never reached, nothing is written
    for i in (104, 105):
        p = pts[i]
        assert val(p, "in_view") == "1" and val(p, "in_view_r") == "1" and val(p, "level") == "9" and val(p, "level_r") == "8" and val(p, "visible") == "0"
        assert [num(p, c) for c in L + Rk] == [900.0 + i - 100, 910.0 + i - 100, 920.0 + i - 100, 0.125, 930.0 + i - 100, 940.0 + i - 100, 950.0 + i - 100, 0.25]
    # mmProjectPoints: from the left camera alone
    assert [(ln[1], float.fromhex(ln[2]), float.fromhex(ln[3])) for ln in out if ln[0] == "project_point"] == [("100", 101.5, 11.25), ("101", 102.5, 12.25)]


def test_other_frames_and_no_points(toy):
    out, _ = toy("frustum_pinhole")
    calls = [ln for ln in out if ln[0].startswith("orbm_") and ln[0] not in ("orbm_create", "orbm_destroy")]
    assert [c[0] for c in calls] == ["orbm_frustum_batch"] and calls[0][2] == "2"          # the owned pinhole adapter's handle
    out, _ = toy("frustum_empty")
    assert not [ln for ln in out if ln[0].startswith("orbm_frustum")] and [ln for ln in out if ln[0] == "returned"][0][1] == "0"


@pytest.mark.parametrize("scenario,level_window", [("last", 2), ("last_mono", 0)])
def test_last_frame_projection_feeds_the_rig_search(toy, scenario, level_window):
    out, _ = toy(scenario)
    calls = [ln for ln in out if ln[0].startswith("orbm_") and ln[0] not in ("orbm_create", "orbm_destroy")]
    assert [c[0] for c in calls] == ["orbm_project_last_rig_batch", "orbm_search_by_projection_last_rig"]
    proj, search = calls
    assert proj[2] == "5" and proj[4] == "1" and proj[6] == "5" and proj[8] == "5"          # cap = Nleft + Nright of the last frame
    i0, i1 = out.index(proj), out.index(search)
    rows = _rows(out[i0 + 1:i1])
    _check_camera_and_pose(out, rows)
    assert rows["has_point"] == [1.0, 0.0, 1.0, 0.0, 1.0]                                  # entry 1 has no point, entry 3 is an outlier
    xyz = [0.0] * 15
    for entry, k in ((0, 0), (2, 1), (4, 3)):
        xyz[3 * entry:3 * entry + 3] = [float(f32(0.1) * f32(k)), float(f32(-0.2) * f32(k)), 2.0 + k]
    assert rows["xyz"] == xyz
    # the search runs on the owned ORBmatcherRigHIP's handle with what the projection returned (the fake: entry 2 is behind the camera)
    assert search[2] == "4" and search[4] == "2" and search[6] == "1" and search[8] == "5" and float.fromhex(search[10]) == 7.0
    assert search[12] == str(level_window) and search[14] == "0"
    rows = _rows(out[i1 + 1:])
    assert rows["valid"] == [1.0, 0.0, 0.0, 0.0, 1.0]
    assert rows["proj_u"] == [50.5, -1.0, -1.0, -1.0, 54.5] and rows["proj_v"] == [60.5, -1.0, -1.0, -1.0, 64.5]
    assert rows["proj_u_r"] == [70.5, -1.0, -1.0, -1.0, 74.5] and rows["proj_v_r"] == [80.5, -1.0, -1.0, -1.0, 84.5]
    # entry 0 is left key point 0, entry 4 is RIGHT key point 1 of the last frame: its octave and angle come from mvKeysRight
    assert rows["pts_octave"] == [0.0, 0.0, 0.0, 0.0, 1.0] and rows["pts_angle"] == [30.0, 0.0, 0.0, 0.0, 231.0]
    assert rows["has_obs"] == [0.0, 0.0, 0.0, 0.0, 1.0]
    assert rows["pts_desc"] == _desc(1, 60) + [0.0] * 96 + _desc(1, 63)
    assert rows["occupied"] == [0.0, 1.0, 0.0]
    # the fake: slot 0 <- entry 4 (point 3 of the toy), slot 2 nulled
    assert [ln for ln in out if ln[0] == "returned"][0] == ["returned", "1", "slots", "3", "100", "-1"]
