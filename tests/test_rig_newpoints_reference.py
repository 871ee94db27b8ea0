"""The sequential reference of the rig CreateNewMapPoints (tests/rig_newpoints_reference.py) checked on its own: hand-built scenes
with the outcome written beside them by hand, the chain reading the kernel implements against the sequential loop, the scenes of
the GPU test against the caps of the guard bands, and the HOST build of the geometry the kernel runs
(csrc/orbm_new_points_rig_geometry.h, through tests/rig_newpoints_geometry_check.cpp) against the reference.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import rig_newpoints_cases as cases
import rig_newpoints_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HAND = ["accepted_once", "rejected_then_accepted", "four_records", "dist_from_left_centre", "stale_right", "stale_left", "stale_matchless",
        "stale_right_rejected", "far_rejected", "far_accepted", "scale_3_0", "scale_4_0", "scale_0_3", "scale_0_4"]
SCENES = list(cases.SHAPES) + list(cases.RANDOM)


def test_the_hand_list_is_complete():
    assert sorted(HAND) == sorted(cases.hand_cases())


@pytest.mark.parametrize("name", HAND)
@pytest.mark.parametrize("T", [np.float32, np.float64], ids=["f32", "f64"])
def test_hand_built_scene(name, T):
    """the outcome written by hand beside the scene, in both precisions, with no decision near a band"""
    c = cases.hand_cases()[name]
    ref = R.create_new_map_points_rig(c["scene"], T)
    for k in ("neighbour", "idx2", "n_matched", "n_created", "skipped"):
        assert np.array_equal(ref[k], c[k]), (name, k, ref[k], c[k])
    assert (ref["undecided_from"] < 0).all() and ref["state_open_at"] < 0 and not ref["baseline_open"]
    for (k, j), gates in c.get("rejected_by", {}).items():
        p = [p for p in ref["pairs"] if p[0] == c["idx1"][k] and p[1] == j]
        assert len(p) == 1 and not p[0][3] and p[0][7][-1][0] in gates, (name, p)


def test_accepted_feature_is_invisible_to_the_next_search():
    c = cases.hand_cases()["accepted_once"]
    ref = cases.expected("accepted_once")
    assert ref["match12"][0][0] >= 0 and ref["match12"][1][0] == -1
    # neighbour 1 alone would have matched it
    alone = R.create_new_map_points_rig(dict(kf1=c["scene"]["kf1"], neighbours=c["scene"]["neighbours"][1:], pairs=c["scene"]["pairs"][1:], params=c["scene"]["params"]))
    assert alone["neighbour"][0] == 0


def test_max_dist_is_taken_from_the_left_centre():
    c = cases.hand_cases()["dist_from_left_centre"]
    ref = cases.expected("dist_from_left_centre")
    assert c["scene"]["kf1"]["n_left"] == 0 and ref["neighbour"][0] == 0            # a right observation
    assert abs(ref["max_dist"][0] / c["max_dist_left"] - 1) < 1e-4
    assert abs(ref["max_dist"][0] / c["max_dist_right"] - 1) > 0.03
    # the normal is taken from the RIGHT centres: with the left centre of key frame 1 it would point elsewhere
    sc = c["scene"]
    n_left = R.normal_and_depth(ref["x3d"][0], sc["kf1"]["Ow"][0], sc["neighbours"][0]["Ow"][1], sc["kf1"]["Ow"][0], 1.0, 1.0)[0]
    assert np.abs(ref["normal"][0] - n_left).max() > 1e-3


def test_stale_hand_cases_keep_their_baselines_far_from_mb():
    """at least 10 % of mb on each side, so that no band touches the skip decisions"""
    for name in ("stale_right", "stale_left", "stale_matchless", "stale_right_rejected"):
        b, skipL, skipR = R.baseline_tests(cases.hand_cases()[name]["scene"])
        assert not skipL[0] and not skipR[0] and not skipL[1] and skipR[1]
        assert (np.abs(b[:, :2] / b[:, 2:3] - 1) >= 0.10).all(), (name, b)
    a, b = cases.expected("stale_right"), cases.expected("stale_left")
    assert a["state_after"] == [1, 1] and b["state_after"] == [0, 0]
    assert cases.expected("stale_matchless")["state_after"] == [0, 0]
    assert cases.expected("stale_right_rejected")["state_after"] == [1, 1]


@pytest.mark.parametrize("name", SCENES)
def test_scene_stays_within_the_caps_and_chain_equals_loop(name):
    """the conditions on every scene the GPU test uses: the bands leave at most 1 % of the reached (feature, neighbour) pairs and
    2 % of the features open, no skip decision hangs on a band, the float32 run flips nothing outside the bands and stays inside
    the recorded spread, Triangulate's matrix stays as well conditioned as TRI_DOUBLE_BOUND assumes -- and the chain reading the
    kernel implements (features independent given the skip decisions) equals the sequential loop"""
    sc, ref = cases.scene_of(name), cases.expected(name)
    pairs, feats = R.shares(ref)
    print("%s: %d reached pairs, %d created, open pairs %.4f features %.4f, skipped %s" % (name, len(ref["pairs"]), ref["n_created"].sum(), pairs, feats, ref["skipped"]))
    assert pairs <= R.CAP_PAIRS and feats <= R.CAP_FEATURES
    assert ref["state_open_at"] < 0 and not ref["baseline_open"]
    errs = R.compare(ref, cases.expected(name, True), sc, name)
    if errs:
        print("%s: float32 vs float64 point metric max %.3g over %d points, worst sigma1 / sigma3 %.1f" % (name, max(errs), len(errs), ref["cond_max"]))
        assert max(errs) <= R.SPREAD_F32
    assert ref["cond_max"] <= R.TRI_COND_MAX
    ch = R.chain(sc, ref["skipped"], np.float64)
    for k in ("neighbour", "idx2", "n_matched", "n_created"):
        assert np.array_equal(ch[k], ref[k]), k
    assert np.array_equal(ch["match12"], np.array(ref["match12"], np.int32).reshape(ch["match12"].shape))
    # the Ow1 state the host driver derives from the counters of a segment: the side of the highest matched idx1 of the most
    # recent neighbour with a match
    state = 0
    for j in range(len(sc["neighbours"])):
        if ch["n_matched"][j] > 0:
            state = int(ch["max_matched_idx1"][j] >= sc["kf1"]["n_left"])
        assert state == ref["state_after"][j], j


def test_scenes_cut_every_gate_and_take_both_states():
    rejected_at, states, skipped = set(), set(), 0
    for name in SCENES:
        ref = cases.expected(name)
        rejected_at |= {p[7][-1][0] for p in ref["pairs"] if not p[3] and p[7]}
        states |= set(ref["state_after"])
        skipped += int(ref["skipped"].sum())
    assert {"cosRays<bound", "z1>0", "reproj1", "far1", "scale_lo", "scale_hi"} <= rejected_at, rejected_at
    assert states == {0, 1} and skipped >= 6
    assert cases.expected("ambiguous_at_1")["skipped"].tolist() == [0, 1, 0] and cases.expected("ambiguous_at_1_left_only")["skipped"].tolist() == [0, 0, 0]
    assert cases.expected("random_10")["n_created"].sum() > 150 and cases.expected("random_3")["n_created"].sum() > 120


@pytest.fixture(scope="module")
def geometry_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("rnp") / "rig_newpoints_geometry_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "rig_newpoints_geometry_check.cpp")])
    return exe


@pytest.mark.parametrize("name", ["random_3", "random_10", "coarse_one_pair", "four_records", "dist_from_left_centre", "right_mixed"])
def test_host_build_of_the_kernel_geometry(name, geometry_exe, tmp_path):
    """the text the kernel compiles, built for the host: decisions outside the guard bands, points within 4 x the float32 spread
    of the float64 reference and within TRI_DOUBLE_BOUND of the float64 null vector of the same float matrix, normal and distances
    as MapPoint::UpdateNormalAndDepth gives them"""
    sc, ref = cases.scene_of(name), cases.expected(name)
    kf1 = sc["kf1"]
    R.pack_pairs(sc, [p[:3] for p in ref["pairs"]]).tofile(str(tmp_path / "in.bin"))
    subprocess.check_call([geometry_exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")])
    out = np.fromfile(str(tmp_path / "out.bin"), np.float32).reshape(-1, 9)
    assert len(out) == len(ref["pairs"]) > 0
    worst, worst_tri = 0.0, 0.0
    Ow = np.asarray(kf1["Ow"], np.float32).reshape(2, 3)
    for p, r in zip(ref["pairs"], out):
        i1, j, i2, accept, undecided, sinp, x3d, _ = p
        if undecided:
            continue
        assert bool(r[0]) == accept, (name, p[:5], p[7])
        if not accept:
            continue
        kf2 = sc["neighbours"][j]
        S1, S2 = R.side_of(kf1, i1 >= kf1["n_left"]), R.side_of(kf2, i2 >= kf2["n_left"])
        g = R.pair_geometry(S1, R.obs_of(kf1, i1), S2, R.obs_of(kf2, i2), sc["params"], np.float64, matrix_dtype=np.float32)
        worst = max(worst, R.point_error(r[1:4], x3d, S1["Ow"], sinp))
        d = np.abs(r[1:4].astype(np.float64) - g["x3d"])
        worst_tri = max(worst_tri, (d / (R.TRI_DOUBLE_BOUND_REL * np.abs(g["x3d"]) + R.TRI_DOUBLE_BOUND_ABS * np.linalg.norm(g["x3d"]))).max())
        nrm, mx, mn = R.normal_and_depth(r[1:4], S1["Ow"], S2["Ow"], Ow[0], kf1["scale_factors"][kf1["octave"][i1]], kf1["scale_factors"][-1])
        assert np.abs(r[4:7] - nrm).max() < 1e-6 and abs(r[7] / mx - 1) < 1e-6 and abs(r[8] / mn - 1) < 1e-6
    print("%s: host build point metric max %.3g (bar %.3g), worst share of the double bar %.3f" % (name, worst, 4 * R.SPREAD_F32, worst_tri))
    assert worst <= 4 * R.SPREAD_F32
    assert worst_tri <= 1.0


def test_baseline_tests_come_out_alike_in_both_precisions():
    """sqrt(d0 d0 + (d1 d1 + d2 d2)) < mb from either centre, every scene: no baseline inside the band, float32 decides as float64"""
    for name in SCENES:
        b32, skipL, skipR = R.baseline_tests(cases.scene_of(name), np.float32)
        b64, sL64, sR64 = R.baseline_tests(cases.scene_of(name), np.float64)
        assert np.array_equal(skipL, sL64) and np.array_equal(skipR, sR64), name
        assert (np.abs(b32[:, :2] / b32[:, 2:3] - 1) > R.GUARD_BASELINE).all(), name
