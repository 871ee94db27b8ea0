"""The numpy restatement of the two rig-frame tracking searches (tests/rig_match_reference.py) against the expectations stated
literally in tests/rig_match_cases.py, the event counts the seeded random rigs must contain, and -- with an empty right side and
every right-camera flag off -- against the restatements of the conventional searches.  No GPU."""
import numpy as np
import pytest

import rig_match_cases as cases
from matcher_reference import numpy_search_last, numpy_search_mp
from rig_match_reference import numpy_search_last_rig, numpy_search_mp_rig

HAND = cases.hand_built()


def run_reference(c, stats=None):
    a, o = c["assign"].copy(), c["occupied"].copy()
    if c["kind"] == "mp":
        n = numpy_search_mp_rig(c["rig"], c["pts"], c["th"], c["nnratio"], a, o, c["far_points"], c["th_far"], stats=stats)
    else:
        n = numpy_search_last_rig(c["rig"], c["pts"], c["th"], c["check_ori"], a, o, stats=stats)
    return n, a, o


@pytest.mark.parametrize("name", sorted(HAND))
def test_reference_equals_stated_expectation(name):
    c = HAND[name]
    n, a, o = run_reference(c)
    e = c["expect"]
    assert n == e["n"], name
    np.testing.assert_array_equal(a, e["assign"], name)
    np.testing.assert_array_equal(o, e["occupied"], name)


def test_hand_built_set_is_the_one_the_searches_need():
    want = ("left_match_with_partner", "right_match_with_r2l_partner", "left_ratio_exit_cancels_right", "empty_left_window_right_runs",
            "th_not_applied_on_the_right", "no_right_level", "partner_write_with_obs", "partner_write_without_obs", "partner_write_frees",
            "partner_write_overwrites", "right_view_only", "far_and_bad", "right_ratio_equal", "right_ratio_different", "right_best_100", "right_best_101",
            "ratio_boundary_10_of_20", "ratio_boundary_11_of_20", "one_ulp_outside", "left_window_empty", "filtered_levels", "all_occupied",
            "right_projection_outside", "level_window_forward", "level_window_backward", "shared_histogram", "tie_by_visiting_order", "no_orientation_check")
    for w in want:
        assert any(w in k for k in HAND), w


def test_random_set_contains_every_event():
    """a change of the generator cannot make the set vacuous"""
    mp, last = {}, {}
    for name, c in cases.random_calls().items():
        n, a, o = run_reference(c, mp if c["kind"] == "mp" else last)
        assert n > 0, name
    print("map points:", mp, " last frame:", last)
    assert mp.get("left", 0) >= 20 and mp.get("right", 0) >= 20
    assert last.get("left", 0) >= 20 and last.get("right", 0) >= 20
    assert mp.get("partner_l2r", 0) >= 5 and mp.get("partner_r2l", 0) >= 5
    assert mp.get("right_cancelled_by_left_ratio", 0) >= 1
    assert mp.get("right_research", 0) >= 1
    assert last.get("right_cancelled_by_empty_window", 0) >= 1
    assert last.get("drop_left", 0) >= 1 and last.get("drop_right", 0) >= 1 and last["drop_left"] + last["drop_right"] >= 3


def _mono(c):
    """the call with an empty right side and every right-camera flag off, and the same call for the conventional restatement"""
    rig = dict(c["rig"])
    nl = len(rig["left"]["x"])
    empty = cases.Side().grid()
    rig["right"] = empty
    rig["left_to_right"] = np.full(nl, -1, np.int32); rig["right_to_left"] = np.zeros(0, np.int32)
    pts = dict(c["pts"])
    if c["kind"] == "mp":
        pts["in_view_r"] = np.zeros_like(pts["in_view_r"])
    return dict(c, rig=rig, pts=pts, assign=c["assign"][:nl].copy(), occupied=c["occupied"][:nl].copy())


@pytest.mark.parametrize("seed", cases.RANDOM_SEEDS)
def test_without_a_right_side_the_restatements_equal_the_conventional_ones(seed):
    g_of = lambda rig: dict(rig["left"], u_right=None)
    c = _mono(cases.random_mp_call(seed, th=(1.0, 3.0, 1.0)[seed % 3]))
    n, a, o = run_reference(c)
    p = c["pts"]
    mp = dict(in_view=p["in_view"], u=p["proj_u"], v=p["proj_v"], level=p["pred_level"], view_cos=p["view_cos"], depth=p["track_depth"], bad=p["bad"],
              has_obs=p["has_obs"], desc=p["desc"])
    a1, o1 = c["assign"].copy(), c["occupied"].copy()
    n1 = numpy_search_mp(g_of(c["rig"]), c["rig"]["left"]["desc"], c["rig"]["scale"], mp, c["th"], c["nnratio"], a1, o1, c["far_points"], c["th_far"])
    assert n == n1 and n > 10
    np.testing.assert_array_equal(a, a1); np.testing.assert_array_equal(o, o1)

    c = _mono(cases.random_last_call(seed, level_window=seed % 3))
    n, a, o = run_reference(c)
    p = c["pts"]
    last = dict(valid=p["valid"], u=p["proj_u"], v=p["proj_v"], octave=p["octave"], angle=p["angle"], has_obs=p["has_obs"], desc=p["desc"],
                level_window=p["level_window"])
    a1, o1 = c["assign"].copy(), c["occupied"].copy()
    n1 = numpy_search_last(g_of(c["rig"]), c["rig"]["left"]["desc"], c["rig"]["left"]["angle"], c["rig"]["scale"], last, c["th"], c["check_ori"], a1, o1)
    assert n == n1 and n > 10
    np.testing.assert_array_equal(a, a1); np.testing.assert_array_equal(o, o1)
