"""The rig adapter of the vocabulary-guided searches and of Fuse (include/orbslam3_shim_rig_map.hpp: ORBmatcherRigMapHIP) against the
stand-in types of tests/stubs/ and a recording fake of the C entry points (tests/stubs/shim_rig_map_toy.cpp): the header compiles with
-Wall -Wextra -Werror; every combination of rig and conventional frames / key frames takes the route the header documents; the
arrays that reach the C ABI are byte-exact (concatenated angles, valid = 0 beyond NLeft, the side's raw key points and half of
mDescriptors, the -1 u_right array, the four relative poses and cameras); the write-back reaches the + NLeft slots.  No GPU: the
routing, the marshalling and the write-back are host code."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
f32 = np.float32


def test_rig_map_shim_compiles_against_standins_and_leaves_the_existing_adapters_alone(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_rig_map.hpp"\n#include "orbslam3_shim_rig_map.hpp"\n'
                   'using namespace ORB_SLAM3;\n'
                   'int main() { RigMatchFrame F; RigMapKeyFrame K; std::vector<MapPoint*> v; std::vector<std::pair<size_t, size_t> > p;\n'
                   '  ORBmatcherRigMapHIP<RigMatchFrame, RigMapKeyFrame, RigMatchMapPoint, KannalaBrandt8Rig, RigMapReference> m(0.8f, true);\n'
                   '  return m.SearchByBoW(&K, F, v) + m.SearchByBoW(&K, &K, v) + m.SearchForTriangulation(&K, &K, p, false) + m.Fuse(&K, v, 3.f, true)\n'
                   '         + m.rig().SearchByProjection(F, v, 3.f, false, 50.f) + m.matcher().Fuse(&K, v); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shim_rig_map") / "shim_rig_map_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_rig_map_toy.cpp"), "-o", str(exe)])

    def run(scenario):
        r = subprocess.run([str(exe), scenario], check=True, capture_output=True, text=True)
        out = [ln.split() for ln in r.stdout.splitlines()]
        assert [ln[:3] for ln in out[:3]] == [["orbm_create", "handle", str(k)] for k in (1, 2, 3)]       # the owned matchers' handles, then the adapter's own
        assert [ln[:3] for ln in out[-3:]] == [["orbm_destroy", "handle", str(k)] for k in (3, 2, 1)]
        body = out[3:-3]
        rows = {ln[0]: (None if ln[1:] == ["NULL"] else [float.fromhex(v) for v in ln[1:]]) for ln in body if len(ln) > 1 and not ln[0].startswith(("orbm_", "re"))}
        calls = [ln for ln in body if ln[0].startswith(("orbm_", "reference"))]
        tail = [ln for ln in body if ln[0] in ("returned", "replaced", "observations")]
        return calls, rows, tail
    return run


def _head(call):
    """the name / value pairs of a call line"""
    return dict(zip(call[1::2], call[2::2]))


def _desc(rows, seed):
    return [float((i * 7 + seed) & 0xFF) for i in range(rows * 32)]


RIG_KF_FV = dict(node=[3.0, 8.0], offset=[0.0, 2.0, 5.0], feat=[0.0, 3.0, 1.0, 2.0, 4.0])


def _check_fv(rows, name, want):
    for k, v in want.items():
        assert rows["%s.%s" % (name, k)] == v, (name, k)


@pytest.mark.parametrize("scenario", ["bow_rig", "bow_rig_convkf"])
def test_search_by_bow_of_a_rig_frame(toy, scenario):
    calls, rows, tail = toy(scenario)
    assert len(calls) == 1 and calls[0][0] == "orbm_search_by_bow_rig"
    h = _head(calls[0])
    assert h["handle"] == "3" and h["n_f"] == "6" and h["n_left_f"] == "4" and float.fromhex(h["nnratio"]) == 0.75 and h["check_orientation"] == "1"
    if scenario == "bow_rig":       # a rig key frame: the angles of mvKeys then mvKeysRight (mvKeysUn holds 77, 78, 79)
        assert h["n_kf"] == "5" and rows["angle_kf"] == [11.0, 12.0, 13.0, 201.0, 202.0] and rows["valid_kf"] == [1.0, 0.0, 0.0, 1.0, 1.0]
        assert rows["desc_kf"] == _desc(5, 1)
        _check_fv(rows, "fv_kf", RIG_KF_FV)
    else:                           # a conventional key frame: mvKeysUn
        assert h["n_kf"] == "4" and rows["angle_kf"] == [47.0, 48.0, 49.0, 50.0] and rows["valid_kf"] == [1.0, 1.0, 0.0, 1.0]
        _check_fv(rows, "fv_kf", dict(node=[3.0, 9.0], offset=[0.0, 2.0, 4.0], feat=[0.0, 1.0, 2.0, 3.0]))
    # the frame: mvKeys (20 ..) then mvKeysRight (220 ..), never mvKeysUn (120 ..); the whole of mDescriptors
    assert rows["angle_f"] == [20.0, 21.0, 22.0, 23.0, 220.0, 221.0] and rows["desc_f"] == _desc(6, 5)
    _check_fv(rows, "fv_f", dict(node=[3.0, 7.0], offset=[0.0, 2.0, 6.0], feat=[4.0, 0.0, 1.0, 5.0, 2.0, 3.0]))
    assert rows["match"] == [-1.0] * 6
    # the fake: slot 1 <- key-frame feature 0, the last right slot <- feature 3; the map points of those features come back
    want = ["-1", "0", "-1", "-1", "-1", "2"]
    assert tail == [["returned", "2", "matches"] + want]


@pytest.mark.parametrize("scenario,route", [("bow_conv_rigkf", ["reference", "SearchByBoW", "frame"]), ("bow_conv", ["orbm_search_by_bow", "handle", "1"])])
def test_search_by_bow_of_a_conventional_frame(toy, scenario, route):
    """a rig key frame under a conventional frame goes to the reference (the monocular entry would read mvKeysUn beyond NLeft)"""
    calls, _, tail = toy(scenario)
    assert len(calls) == 1 and calls[0][:3] == route
    assert tail == [["returned", "-11" if scenario == "bow_conv_rigkf" else "0"]]


def test_search_by_bow_between_rig_key_frames(toy):
    calls, rows, tail = toy("kfkf_rig")
    assert len(calls) == 1 and calls[0][0] == "orbm_search_by_bow_kfkf"
    h = _head(calls[0])
    assert h["handle"] == "3" and h["n1"] == "5" and h["n2"] == "5" and float.fromhex(h["nnratio"]) == 0.75 and h["check_orientation"] == "1"
    for q, seed in (("1", 1), ("2", 2)):
        # slot 1 holds no point, slot 2 a bad one, slots 3 and 4 lie beyond mvKeysUn.size() = NLeft; the angles are mvKeysUn's
        assert rows["valid" + q] == [1.0, 0.0, 0.0, 0.0, 0.0] and rows["angle" + q] == [77.0, 78.0, 79.0, 0.0, 0.0]
        assert rows["desc" + q] == _desc(5, seed)
        _check_fv(rows, "fv" + q, RIG_KF_FV)
    # the fake: feature 0 -> feature 3 of key frame 2, feature 4 -> feature 0: their map points (key frame 2's are 4 .. 7 of the toy)
    assert tail == [["returned", "2", "matches", "6", "-1", "-1", "-1", "4"]]


def test_search_by_bow_between_conventional_key_frames(toy):
    calls, rows, _ = toy("kfkf_conv")
    assert len(calls) == 1 and calls[0][0] == "orbm_search_by_bow_kfkf"
    assert rows["valid1"] == [1.0, 1.0, 0.0, 1.0] and rows["angle1"] == [47.0, 48.0, 49.0, 50.0] and rows["angle2"] == [48.0, 49.0, 50.0, 51.0]


def test_search_for_triangulation_between_rig_key_frames(toy):
    calls, rows, tail = toy("tri_rig")
    assert len(calls) == 1 and calls[0][0] == "orbm_search_for_triangulation_rig"
    h = _head(calls[0])
    assert h == dict(handle="3", n1="5", n_left_1="3", n2="5", n_left_2="3", n_levels="3", only_stereo="0", coarse="1", check_orientation="0")
    for q, seed in (("kf1", 1), ("kf2", 2)):
        assert rows[q + ".has_mp"] == [1.0, 0.0, 1.0, 1.0, 1.0] and rows[q + ".stereo"] is None
        # the raw key points of both lists, concatenated
        assert rows[q + ".x"] == [100.5 + seed, 110.5 + seed, 120.5 + seed, 300.0 + seed, 301.0 + seed] and rows[q + ".y"] == [50.25, 51.25, 52.25, 250.0, 249.0]
        assert rows[q + ".octave"] == [0.0, 1.0, 0.0, 2.0, 1.0] and rows[q + ".angle"] == [10.0 + seed, 11.0 + seed, 12.0 + seed, 200.0 + seed, 201.0 + seed]
        assert rows[q + ".desc"] == _desc(5, seed)
        _check_fv(rows, q + ".fv", RIG_KF_FV)
    cams = [[190.5, 190.25, 254.5, 256.75, 0.003, 0.0007, -0.002, 0.0002, 1e-6], [191.5, 191.25, 252.5, 254.75, 0.004, 0.0018, -0.0027, 0.0004, 2e-6],
            [290.5, 290.25, 354.5, 356.75, 0.013, 0.0107, -0.012, 0.0102, 3e-6], [291.5, 291.25, 352.5, 354.75, 0.014, 0.0118, -0.0127, 0.0104, 4e-6]]
    assert rows["cam"] == [float(f32(v)) for c in cams for v in c]        # key frame 1 left, right, key frame 2 left, right
    # the four relative poses, all values dyadic so that every float operation is exact: T1w = [I | t1], T2w = [Rz(90) | t2]
    t1, trl1 = np.array([0.25, -0.5, 0.75]), np.array([-0.125, 0.015625, 0.03125])
    R2, t2, trl2 = np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([1.5, 0.125, -0.375]), np.array([-0.25, 0.0625, 0.5])
    left1, right1 = (np.eye(3), t1), (np.eye(3), t1 + trl1)               # Tr1w = Trl * T1w
    inv = lambda R, t: (R.T, -(R.T @ t))
    w2, wr2 = inv(R2, t2), inv(R2, t2 + trl2)                             # Tw2, Twr2 = (Trl * T2w)^-1
    want_R, want_t = [], []
    for (Ra, ta), (Rb, tb) in ((left1, w2), (left1, wr2), (right1, w2), (right1, wr2)):      # ll, lr, rl, rr
        want_R += list((Ra @ Rb).reshape(-1)); want_t += list(Ra @ tb + ta)
    assert rows["R12"] == [float(v) for v in want_R] and rows["t12"] == [float(v) for v in want_t]
    sig = [1.0, float(f32(1.44)), float(f32(2.0736))]
    assert rows["level_sigma2_1"] == sig and rows["level_sigma2_2"] == sig
    assert tail == [["returned", "2", "pairs", "1", "4", "3", "0"]]        # vMatchedPairs in index order


@pytest.mark.parametrize("scenario,route", [("tri_conv", ["orbm_search_for_triangulation", "handle", "1"]), ("tri_mixed", ["reference", "SearchForTriangulation"]),
                                            ("tri_pinhole_rig", ["reference", "SearchForTriangulation"])])
def test_search_for_triangulation_of_other_pairs(toy, scenario, route):
    calls, _, _ = toy(scenario)
    assert len(calls) == 1 and calls[0][:len(route)] == route


def _pinhole(fx, fy, cx, cy, p):
    return f32(f32(f32(fx) * p[0]) / p[2]) + f32(cx), f32(f32(f32(fy) * p[1]) / p[2]) + f32(cy)


@pytest.mark.parametrize("scenario", ["fuse_left", "fuse_right"])
def test_fuse_on_a_rig_key_frame(toy, scenario):
    calls, rows, tail = toy(scenario)
    right = scenario == "fuse_right"
    assert len(calls) == 1 and calls[0][0] == "orbm_fuse_search"
    h = _head(calls[0])
    assert h["handle"] == "3" and h["n"] == ("2" if right else "3") and h["points"] == "4" and float.fromhex(h["th"]) == 2.5 and h["chi2_check"] == "1"
    assert calls[0][calls[0].index("grid") + 1:calls[0].index("grid") + 3] == ["64", "48"] and h["angle"] == "NULL" and h["frame_u_right"] == "NULL"
    i = calls[0].index("bounds")
    assert [float.fromhex(v) for v in calls[0][i + 1:i + 5]] == [0.0, 0.0, 752.0, 480.0]
    whole = _desc(5, 1)
    if right:       # mvKeysRight and rows [NLeft, N) of mDescriptors
        assert rows["x"] == [301.0, 302.0] and rows["y"] == [250.0, 249.0] and rows["octave"] == [2.0, 1.0] and rows["desc"] == whole[96:]
    else:           # the RAW mvKeys (mvKeysUn holds 900 / 800) and rows [0, NLeft)
        assert rows["x"] == [101.5, 111.5, 121.5] and rows["y"] == [50.25, 51.25, 52.25] and rows["octave"] == [0.0, 1.0, 0.0] and rows["desc"] == whole[:96]
    assert rows["u_right"] == [-1.0] * (2 if right else 3)                 # always the monocular gate
    assert rows["inv_level_sigma2"] == [1.0, float(f32(0.5) + f32(0.1)), 0.25] and rows["scale_factors"] == [1.0, float(f32(1.2)), float(f32(1.44))]
    # the projection: the side's pose (no rotation: x + t, and the right pose is Trl * Tcw) and the side's camera
    t = np.array([0.25, -0.5, -0.5], f32) + (np.array([-0.125, 0.015625, 0.03125], f32) if right else f32(0))
    cam = (300, 301, 200, 201) if right else (458, 457, 367, 248)
    want_u, want_v = [0.0] * 4, [0.0] * 4
    for k in range(3):                                                   # point 3 lies behind the camera
        x = np.array([f32(0.125) * f32(k), f32(-0.25) * f32(k), f32(2.0) + f32(k)], f32) + t
        u, v = _pinhole(*cam, x)
        want_u[k], want_v[k] = float(u), float(v)
    assert rows["valid"] == [1.0, 1.0, 1.0, 0.0] and rows["proj_u"] == want_u and rows["proj_v"] == want_v
    assert rows["pred_level"] == [0.0, 1.0, 2.0, 0.0] and rows["desc_mp"] == _desc(1, 60) + _desc(1, 61) + _desc(1, 62) + [0.0] * 32
    # the fake: point 0 -> side index 1 (10 bits), point 1 -> side index 0 (50), point 2 -> 51 bits: not fused
    if right:       # slots 4 and 3: both hold a point with fewer observations, which is replaced
        assert tail == [["returned", "2", "slots", "100", "-1", "101", "102", "103"], ["replaced", "-1", "-1", "1", "0"], ["observations", "-1", "-1", "-1", "-1"]]
    else:           # slot 1 is empty: point 0 is added there; slot 0's point is replaced by point 1
        assert tail == [["returned", "2", "slots", "100", "0", "101", "102", "103"], ["replaced", "1", "-1", "-1", "-1"], ["observations", "1", "-1", "-1", "-1"]]


@pytest.mark.parametrize("scenario,route", [("fuse_conv", ["orbm_fuse_search", "handle", "1"]), ("fuse_conv_right", ["reference", "Fuse", "bRight", "1"])])
def test_fuse_on_a_conventional_key_frame_keeps_the_existing_route(toy, scenario, route):
    calls, _, _ = toy(scenario)
    assert len(calls) == 1 and calls[0][:len(route)] == route
