"""orbm_create_new_map_points_rig on the device against the sequential reference (tests/rig_newpoints_reference.py in float64).

Tolerances, all derived on the CPU from the reference alone (tests/test_rig_newpoints_reference.py asserts them for every scene
used here).  Integer results -- neighbour, idx2, n_matched, n_created, match12, skipped -- are identical for every feature outside
the guard bands: the borderline band of the search gate (fisheye_stereo_reference.borderline: 1e-6 on the cosine, 1e-4 on the
depths, 1e-3 relative on the two reprojection gates) and the bands of newpoints_reference on the per-match geometry (1e-6 on
cosines, 1e-3 relative on the reprojection / far / scale gates, 1e-3 of the distance on the depth signs).  The scenes leave at
most 1 % of the reached (feature, neighbour) pairs and 2 % of the features open (on these scenes: at most 0.42 % / 0.17 %), and no baseline test
within 1e-3 of mb.  Points: |x_dev - x_ref64| / |x_ref64 - Ow_side1| * sin(parallax); the float32 run of the reference differs from
the float64 run by at most 3.45e-7 on these scenes, the device gets 4 x 3.46e-7 = 1.38e-6.  Triangulated points additionally meet
TRI_DOUBLE_BOUND against the float64 null vector of the same float matrix (worst sigma1 / sigma3 on these scenes: 23).
The host build of the kernel's geometry meets all of these (worst point metric 2.0e-7, worst share of the double bar 0.88), and so
does the device (worst point metric 3.42e-7, worst share of the double bar 0.93); the tests print the live figures."""
import numpy as np
import pytest

import rig_newpoints_cases as cases
import rig_newpoints_reference as R

pytestmark = pytest.mark.gpu

HAND = ["accepted_once", "rejected_then_accepted", "four_records", "dist_from_left_centre", "stale_right", "stale_left", "stale_matchless",
        "stale_right_rejected", "far_rejected", "far_accepted", "scale_3_0", "scale_4_0", "scale_0_3", "scale_0_4"]
SEGMENTS = {"all_skipped": 1, "ambiguous_at_1": 2, "ambiguous_at_1_left_only": 2, "ambiguous_twice": 3, "ambiguous_twice_left_only": 3, "ambiguous_last": 2,
            "ambiguous_after_skipped": 2, "random_3": 1, "random_10": 2, "64_neighbours": 1}


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.Matcher(0.6, False)
    yield m
    m.close()


def run(matcher, sc):
    return matcher.create_new_map_points_rig(sc["kf1"], sc["neighbours"], sc["pairs"], sc["params"])


def check_outputs(sc, dev):
    created = dev["neighbour"] >= 0
    assert dev["created"] == int(created.sum()) == int(dev["n_created"].sum())
    assert np.array_equal(dev["n_created"], np.bincount(dev["neighbour"][created], minlength=len(sc["neighbours"])))
    assert (dev["idx2"][~created] == -1).all() and (dev["x3d"][~created] == 0).all() and (dev["normal"][~created] == 0).all()
    assert (dev["max_dist"][~created] == 0).all() and (dev["min_dist"][~created] == 0).all() and (dev["point_stereo"] == 0).all()
    assert (dev["match12"][:, np.asarray(sc["kf1"]["has_mp"], bool)] == -1).all()
    sk = dev["skipped"].astype(bool)
    assert (dev["match12"][sk] == -1).all() and (dev["n_matched"][sk] == 0).all() and not np.isin(dev["neighbour"][created], np.nonzero(sk)[0]).any()
    for j in range(len(sc["neighbours"])):
        assert dev["n_matched"][j] == int((dev["match12"][j] >= 0).sum())
        assert np.array_equal(dev["idx2"][dev["neighbour"] == j], dev["match12"][j][dev["neighbour"] == j])


def check_triangulated_in_double(sc, ref, dev, label):
    kf1 = sc["kf1"]
    worst, n = 0.0, 0
    for (i1, j, i2, accept, undecided, _, _, _) in ref["pairs"]:
        if not accept or undecided or dev["neighbour"][i1] != j or dev["idx2"][i1] != i2:
            continue
        kf2 = sc["neighbours"][j]
        g = R.pair_geometry(R.side_of(kf1, i1 >= kf1["n_left"]), R.obs_of(kf1, i1), R.side_of(kf2, i2 >= kf2["n_left"]), R.obs_of(kf2, i2), sc["params"],
                            np.float64, matrix_dtype=np.float32)
        d = np.abs(dev["x3d"][i1].astype(np.float64) - g["x3d"])
        worst = max(worst, (d / (R.TRI_DOUBLE_BOUND_REL * np.abs(g["x3d"]) + R.TRI_DOUBLE_BOUND_ABS * np.linalg.norm(g["x3d"]))).max())
        n += 1
    print("%s: worst share of the double bar %.3f over %d triangulated points" % (label, worst, n))
    assert worst <= 1.0


def check_against_reference(matcher, name):
    sc, ref = cases.scene_of(name), cases.expected(name)
    dev = run(matcher, sc)
    errs = R.compare(ref, dev, sc, name)
    check_outputs(sc, dev)
    if errs:
        print("%s: device point metric max %.3g over %d points (bar %.3g)" % (name, max(errs), len(errs), 4 * R.SPREAD_F32))
        assert max(errs) <= 4 * R.SPREAD_F32
    check_triangulated_in_double(sc, ref, dev, name)
    return ref, dev


@pytest.mark.parametrize("name", HAND)
def test_hand_built_scene(matcher, name):
    """the outcome written by hand beside the scene (tests/rig_newpoints_cases.py)"""
    c = cases.hand_cases()[name]
    dev = run(matcher, c["scene"])
    for k in ("neighbour", "idx2", "n_matched", "n_created", "skipped"):
        assert np.array_equal(dev[k], c[k]), (name, k, dev[k], c[k])
    check_outputs(c["scene"], dev)
    check_against_reference(matcher, name)
    if name == "dist_from_left_centre":
        assert abs(dev["max_dist"][0] / c["max_dist_left"] - 1) < 1e-4 and abs(dev["max_dist"][0] / c["max_dist_right"] - 1) > 0.03


@pytest.mark.parametrize("name", list(cases.SHAPES))
def test_shape_scene(matcher, name):
    """n_left in {0, n, between} on either side, neighbour nodes at the lane-group boundaries, 1 .. 64 neighbours, an empty neighbour,
    coarse on one pair, every neighbour skipped, and the segmented path: an ambiguous neighbour at 1, two in a row, one last"""
    ref, dev = check_against_reference(matcher, name)
    if name in SEGMENTS:
        assert matcher.create_new_map_points_rig_last()[1] == SEGMENTS[name]
    if name == "all_skipped":
        assert dev["created"] == 0 and dev["skipped"].all()


@pytest.mark.parametrize("name", list(cases.RANDOM))
def test_random_scene(matcher, name):
    """300 + 300 features against 3 and 10 neighbours"""
    ref, dev = check_against_reference(matcher, name)
    assert dev["created"] > 120 and len(cases.scene_of(name)["kf1"]["x"]) == 600
    ms, launches = matcher.create_new_map_points_rig_last()
    assert ms > 0 and launches == SEGMENTS[name]


def test_degenerate_scenes(matcher):
    sp = cases.special_scenes()
    dev = run(matcher, sp["kf1_empty"])
    assert dev["created"] == 0 and len(dev["neighbour"]) == 0 and (dev["n_matched"] == 0).all() and (dev["skipped"] == 0).all()
    assert matcher.create_new_map_points_rig_last() == (0.0, 0)
    dev = run(matcher, sp["no_common_node"])
    assert dev["created"] == 0 and (dev["neighbour"] == -1).all() and (dev["n_matched"] == 0).all() and (dev["match12"] == -1).all()
    sc = cases.shape_scene("two_neighbours")
    dev = run(matcher, dict(sc, neighbours=[], pairs=[]))
    assert dev["created"] == 0 and (dev["neighbour"] == -1).all() and len(dev["n_matched"]) == 0
    full = dict(sc, kf1=dict(sc["kf1"], has_mp=np.ones_like(sc["kf1"]["has_mp"])))
    dev = run(matcher, full)
    assert dev["created"] == 0 and (dev["n_matched"] == 0).all() and (dev["match12"] == -1).all()


def test_repeated_calls_are_bitwise_equal(matcher):
    sc = cases.scene_of("random_10")
    a = run(matcher, sc)
    run(matcher, cases.scene_of("ambiguous_twice"))                                 # another shape in between, on the same handle
    b = run(matcher, sc)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else a[k],
                              np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else b[k]), k


def test_ten_neighbours_equal_single_neighbour_calls_that_carry_has_mp(matcher):
    """one call against 10 neighbours == 10 calls against one neighbour each, with the points created so far as has_mp and the skip
    decisions of the one call (a single-neighbour call starts with the left centre and cannot know them)"""
    sc = cases.scene_of("random_10")
    whole = run(matcher, sc)
    has_mp = np.ascontiguousarray(sc["kf1"]["has_mp"]).copy()
    for j in range(len(sc["neighbours"])):
        if whole["skipped"][j]:
            assert whole["n_matched"][j] == 0
            continue
        one = run(matcher, dict(sc, kf1=dict(sc["kf1"], has_mp=has_mp.copy()), neighbours=[sc["neighbours"][j]], pairs=[sc["pairs"][j]]))
        assert one["skipped"][0] == 0
        acc = one["neighbour"] == 0
        assert np.array_equal(acc, whole["neighbour"] == j), j
        assert np.array_equal(one["idx2"][acc], whole["idx2"][acc]) and np.array_equal(one["match12"][0], whole["match12"][j])
        assert np.array_equal(one["x3d"][acc].view(np.uint32), whole["x3d"][acc].view(np.uint32))
        assert np.array_equal(one["normal"][acc].view(np.uint32), whole["normal"][acc].view(np.uint32))
        assert one["n_matched"][0] == whole["n_matched"][j] and one["n_created"][0] == whole["n_created"][j]
        has_mp[acc] = 1


def test_search_equals_the_rig_search_entry(matcher):
    """a single-neighbour call's match12 is what orbm_search_for_triangulation_rig returns for the pair"""
    sc = cases.scene_of("random_3")
    for j in (0, 2):
        one = run(matcher, dict(sc, neighbours=[sc["neighbours"][j]], pairs=[sc["pairs"][j]]))
        n, m12 = matcher.search_for_triangulation_rig(R.search_scene(sc, j, sc["kf1"]["has_mp"]))
        assert one["n_matched"][0] == n and np.array_equal(one["match12"][0], m12)


def test_bad_arguments_leave_the_handle_usable(pkg, matcher):
    sc = cases.scene_of("two_neighbours")
    good = run(matcher, sc)
    bad = dict(sc, neighbours=[dict(k) for k in sc["neighbours"]])
    bad["neighbours"][1]["octave"] = bad["neighbours"][1]["octave"].copy(); bad["neighbours"][1]["octave"][0] = 99
    with pytest.raises(pkg.OrbxError) as e:
        run(matcher, bad)
    assert e.value.code == -3
    again = run(matcher, sc)
    assert np.array_equal(good["neighbour"], again["neighbour"]) and np.array_equal(good["x3d"], again["x3d"])
