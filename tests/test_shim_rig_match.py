"""The rig-frame tracking-search adapter (include/orbslam3_shim_rig_match.hpp: ORBmatcherRigHIP) against the stand-in types of
tests/stubs/ and a recording fake of the C entry points (tests/stubs/shim_rig_match_toy.cpp): the header compiles with -Wall -Wextra
-Werror; a rig frame reaches orbm_search_by_projection_rig / _last_rig on the adapter's own handle with byte-exact arrays (raw key
points of both lists, the two halves of mDescriptors, the match tables, the slot occupancy, the ten tracking members, and projections
made with the LEFT camera's project on both sides); the write-back reaches the right slots; a conventional frame goes to the owned
ORBmatcherHIP.  No GPU: the routing, the marshalling and the write-back are host code."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
f32 = np.float32


def test_rig_match_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_rig_match.hpp"\n#include "orbslam3_shim_rig_match.hpp"\n'
                   'using namespace ORB_SLAM3;\n'
                   'int main() { RigMatchFrame F, L; std::vector<MapPoint*> v; ORBmatcherRigHIP<RigMatchFrame, RigMatchMapPoint> m(0.8f, true);\n'
                   '  return m.SearchByProjection(F, v, 3.f, false, 50.f) + m.SearchByProjection(F, L, 7.f, false); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shim_rig_match") / "shim_rig_match_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_rig_match_toy.cpp"), "-o", str(exe)])

    def run(scenario):
        r = subprocess.run([str(exe), scenario], check=True, capture_output=True, text=True)
        return [ln.split() for ln in r.stdout.splitlines()], r.stderr
    return run


def _rows(out):
    """the array lines after the call line: name -> list of floats (or None), a repeated name once per side"""
    rows = {}
    side = ""
    for ln in out:
        if ln[0] in ("left", "right") and ln[1] == "n":
            side = ln[0] + "."
            rows[side + "head"] = ln
            continue
        if ln[0] in ("left_to_right",):
            side = ""
        if ln[0] in ("x", "y", "octave", "angle", "desc", "scale_factors") and side:
            rows[side + ln[0]] = None if ln[1:] == ["NULL"] else [float.fromhex(v) for v in ln[1:]]
        elif len(ln) > 1 and ln[0] not in ("orbm_create", "orbm_destroy", "returned") and not ln[0].startswith("orbm_search"):
            rows[ln[0]] = None if ln[1:] == ["NULL"] else [float.fromhex(v) for v in ln[1:]]
    return rows


def _desc(rows, seed):
    return [float((i * 7 + seed) & 0xFF) for i in range(rows * 32)]


def _check_rig_frame(rows):
    """make_rig_frame of the toy: mvKeys (not mvKeysUn, which holds 900 / 800 / 77 / octave 5), mvKeysRight, the two halves of mDescriptors"""
    for side, n in (("left", 3), ("right", 2)):
        h = rows[side + ".head"]
        assert h[2] == str(n) and [float.fromhex(v) for v in h[4:8]] == [0.0, 0.0, 512.0, 512.0] and h[9:11] == ["64", "48"] and h[12] == "3" and h[14] == "NULL"
        assert rows[side + ".scale_factors"] == [1.0, float(f32(1.2)), float(f32(1.44))]
    assert rows["left.x"] == [100.5, 110.5, 120.5] and rows["left.y"] == [50.25, 51.25, 52.25]
    assert rows["left.octave"] == [0.0, 1.0, 0.0] and rows["left.angle"] == [10.0, 11.0, 12.0]
    assert rows["right.x"] == [300.0, 301.0] and rows["right.y"] == [250.0, 249.0]
    assert rows["right.octave"] == [2.0, 1.0] and rows["right.angle"] == [200.0, 201.0]
    whole = _desc(5, 3)
    assert rows["left.desc"] == whole[:96] and rows["right.desc"] == whole[96:]
    assert rows["left_to_right"] == [1.0, -1.0, 0.0] and rows["right_to_left"] == [2.0, 0.0]
    assert rows["assign"] == [-2.0] * 5
    assert rows["occupied"] == [0.0, 1.0, 0.0, 0.0, 0.0]              # slot 4 holds a point without observations


def test_map_point_search_of_a_rig_frame(toy):
    out, err = toy("mp_rig")
    assert [ln[0] for ln in out[:3]] == ["orbm_create", "orbm_create", "orbm_search_by_projection_rig"]
    call = out[2]
    assert call[2] == "2" and call[4] == "3"                          # the adapter's own handle (created after the owned ORBmatcherHIP's), three points
    assert [float.fromhex(call[i]) for i in (6, 10, 12)] == [3.0, 40.0, float(f32(0.8))] and call[8] == "1"
    rows = _rows(out[3:])
    _check_rig_frame(rows)
    k = np.arange(3)
    assert rows["in_view"] == [1.0, 0.0, 1.0] and rows["in_view_r"] == [0.0, 1.0, 1.0]
    assert rows["proj_u"] == [100.0, 101.0, 102.0] and rows["proj_v"] == [50.0, 51.0, 52.0] and rows["pred_level"] == [0.0, 1.0, 2.0]
    assert rows["proj_u_r"] == [300.0, 301.0, 302.0] and rows["proj_v_r"] == [250.0, 251.0, 252.0] and rows["pred_level_r"] == [-1.0, 0.0, 1.0]
    assert rows["view_cos"] == [float(f32(0.9) + f32(0.03) * f32(i)) for i in k]
    assert rows["view_cos_r"] == [float(f32(0.99) + f32(0.004) * f32(i)) for i in k]
    assert rows["track_depth"] == [5.0, 6.0, 7.0] and rows["bad"] == [0.0, 0.0, 1.0] and rows["has_obs"] == [0.0, 1.0, 1.0]
    assert rows["pts_desc"] == _desc(1, 40) + _desc(1, 41) + _desc(1, 42)
    # the fake assigns left slot 0 <- point 2, right slots 3 <- 0 and 4 <- 1; slot 1 keeps what it held (100), slot 2 stays NULL
    assert out[-3] == ["returned", "3", "slots", "2", "100", "-1", "0", "1"]
    assert "left_to_right len 3" in err and "pts_desc len 96" in err   # record_abi's lines


def _pinhole(fx, fy, cx, cy, p):
    return f32(f32(f32(fx) * p[0]) / p[2]) + f32(cx), f32(f32(f32(fy) * p[1]) / p[2]) + f32(cy)


@pytest.mark.parametrize("scenario,level_window", [("last_rig_rig", 1), ("last_rig_conv", 1), ("last_rig_mono", 0)])
def test_last_frame_search_of_a_rig_frame(toy, scenario, level_window):
    out, _ = toy(scenario)
    call = out[2]
    assert call[0] == "orbm_search_by_projection_last_rig" and call[2] == "2" and call[4] == "5"
    assert float.fromhex(call[6]) == 7.0 and call[8] == str(level_window) and call[10] == "0"     # tlc(2) = 0.5 > mb: forward, unless bMono
    rows = _rows(out[3:])
    _check_rig_frame(rows)
    # entry 1 has no point, 3 is an outlier, 4 is behind the camera; 0 and 2 hold points 0 and 1 of the toy
    assert rows["valid"] == [1.0, 0.0, 1.0, 0.0, 0.0]
    t, trl = np.array([0.25, -0.5, -0.5], f32), np.array([-0.1, 0.01, 0.02], f32)
    want = {k: [0.0] * 5 for k in ("proj_u", "proj_v", "proj_u_r", "proj_v_r")}
    for entry, k in ((0, 0), (2, 1)):
        x = np.array([f32(0.1) * f32(k), f32(-0.2) * f32(k), f32(2.0) + f32(k)], f32) + t          # no rotation: x + t
        u, v = _pinhole(458, 457, 367, 248, x)
        ur, vr = _pinhole(458, 457, 367, 248, x + trl)                 # mpCamera->project(Trl * x3Dc): the LEFT camera, not mpCamera2 (300, 301, 200, 201)
        want["proj_u"][entry], want["proj_v"][entry], want["proj_u_r"][entry], want["proj_v_r"][entry] = float(u), float(v), float(ur), float(vr)
    for k in want:
        assert rows[k] == want[k], k
    if scenario == "last_rig_conv":       # a conventional last frame: octave of mvKeys[i], angle of mvKeysUn[i]
        assert rows["pts_octave"] == [0.0, 0.0, 2.0, 0.0, 0.0] and rows["pts_angle"] == [130.0, 0.0, 132.0, 0.0, 0.0]
    else:                                  # a rig last frame, Nleft = 2: entry 0 from mvKeys[0], entry 2 from mvKeysRight[0]
        assert rows["pts_octave"] == [0.0, 0.0, 2.0, 0.0, 0.0] and rows["pts_angle"] == [30.0, 0.0, 230.0, 0.0, 0.0]
    assert rows["has_obs"] == [0.0, 0.0, 1.0, 0.0, 0.0]
    assert rows["pts_desc"] == _desc(1, 60) + [0.0] * 32 + _desc(1, 61) + [0.0] * 64
    # the fake: slot 1 <- entry 0 (over the point it held), slot 3 = -1 -> NULL; slot 4 keeps its point
    assert out[-3] == ["returned", "1", "slots", "-1", "0", "-1", "-1", "101"]


@pytest.mark.parametrize("scenario,entry", [("mp_conv", "orbm_search_by_projection"), ("last_conv", "orbm_search_by_projection_last")])
def test_conventional_frames_go_to_the_owned_matcher(toy, scenario, entry):
    out, _ = toy(scenario)
    calls = [ln for ln in out if ln[0].startswith("orbm_search") or ln[0] == "reference"]
    assert len(calls) == 1 and calls[0][0] == entry and calls[0][2] == "1"        # the handle of the owned ORBmatcherHIP
    assert out[-3] == ["returned", "0"]


def test_conventional_frame_after_a_rig_frame_keeps_the_existing_route(toy):
    """CurrentFrame.Nleft == -1, LastFrame.Nleft != -1: the owned ORBmatcherHIP decides, and hands it to the reference as before"""
    out, _ = toy("last_conv_from_rig")
    assert [ln[0] for ln in out] == ["orbm_create", "orbm_create", "reference", "returned", "orbm_destroy", "orbm_destroy"] and out[3][1] == "-8"
