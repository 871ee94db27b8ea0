"""The two rig-frame tracking searches on the device (orbm_search_by_projection_rig, orbm_search_by_projection_last_rig and their
batch forms) against the expectations stated in tests/rig_match_cases.py and against the numpy restatement
(tests/rig_match_reference.py): assign, occupied and n_matches integer for integer, no tolerance."""
import numpy as np
import pytest

import rig_match_cases as cases
from test_rig_match_reference import run_reference

pytestmark = pytest.mark.gpu

HAND = cases.hand_built()


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.Matcher(0.8, True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def shapes():
    return cases.shape_calls()


@pytest.fixture(scope="module")
def randoms():
    return cases.random_calls()


def run_kernel(m, c):
    a, o = c["assign"].copy(), c["occupied"].copy()
    m.nnratio, m.check_ori = c["nnratio"], c["check_ori"]
    if c["kind"] == "mp":
        n = m.search_by_projection_rig(c["rig"], c["pts"], c["th"], a, o, c["far_points"], c["th_far"])
    else:
        n = m.search_by_projection_last_rig(c["rig"], c["pts"], c["th"], a, o)
    return n, a, o


def run_kernel_batch(m, cs):
    qs = [dict(rig=c["rig"], pts=c["pts"], assign=c["assign"].copy(), occupied=c["occupied"].copy()) for c in cs]
    m.nnratio, m.check_ori = cs[0]["nnratio"], cs[0]["check_ori"]
    if cs[0]["kind"] == "mp":
        ns = m.search_by_projection_rig_batch(qs, cs[0]["th"], cs[0]["far_points"], cs[0]["th_far"])
    else:
        ns = m.search_by_projection_last_rig_batch(qs, cs[0]["th"])
    return [(n, q["assign"], q["occupied"]) for n, q in zip(ns, qs)]


def same(got, want, what):
    assert got[0] == want[0], "%s: n_matches %d, expected %d" % (what, got[0], want[0])
    np.testing.assert_array_equal(got[1], want[1], what + ": assign")
    np.testing.assert_array_equal(got[2], want[2], what + ": occupied")


@pytest.mark.parametrize("name", sorted(HAND))
def test_hand_built_call(matcher, name):
    c = HAND[name]
    e = c["expect"]
    same(run_kernel(matcher, c), (e["n"], e["assign"], e["occupied"]), name)


def test_hand_built_calls_in_one_launch(matcher):
    """every hand-built call of a kind and parameter set as one batch: the frames of a launch are independent"""
    groups = {}
    for name in sorted(HAND):
        c = HAND[name]
        groups.setdefault((c["kind"], c["th"], c["nnratio"], c["far_points"], c["th_far"], c["check_ori"]), []).append(name)      # (level_window is per query)
    for key, names in groups.items():
        for name, got in zip(names, run_kernel_batch(matcher, [HAND[n] for n in names])):
            e = HAND[name]["expect"]
            same(got, (e["n"], e["assign"], e["occupied"]), "batch " + name)


SHAPES = sorted(k + s for k in ("mp", "last") for s in ("_no_left_features", "_no_right_features", "_no_points", "_65_points", "_129_points",
                                                         "_unstaged_%d_a_side" % cases.UNSTAGED_N, "_host_grid_%d_and_%d" % cases.HOST_GRID_N, "_batch_of_3", "_70_features_in_one_cell",
                                                         "_window_wider_than_16_columns"))


@pytest.mark.parametrize("name", SHAPES)
def test_shape_call(matcher, shapes, name):
    c = shapes[name]
    if isinstance(c, list):
        for k, (got, one) in enumerate(zip(run_kernel_batch(matcher, c), c)):
            same(got, run_reference(one), "%s[%d]" % (name, k))
    else:
        want = run_reference(c)
        if "no_points" not in name and "no_left" not in name and "no_right" not in name:
            assert want[0] > 0, name
        same(run_kernel(matcher, c), want, name)


def test_shape_names_are_all_run(shapes):
    assert sorted(shapes) == SHAPES


@pytest.mark.parametrize("name", ["%s_random_%d" % (k, s) for k in ("mp", "last") for s in cases.RANDOM_SEEDS])
def test_random_rig(matcher, randoms, name):
    c = randoms[name]
    want = run_reference(c)
    assert want[0] > 20
    same(run_kernel(matcher, c), want, name)
    twice = run_kernel(matcher, c)
    same(twice, want, name + " (second call)")
    assert matcher.rig_search_last_kernel_ms() > 0.0


def test_random_rigs_as_batches(matcher, randoms):
    for kind in ("mp", "last"):
        cs = [randoms["%s_random_%d" % (kind, s)] for s in cases.RANDOM_SEEDS]
        cs = [c for c in cs if c["th"] == cs[-1]["th"]]          # th belongs to the launch, level_window to the query
        assert len(cs) >= 2
        for got, one in zip(run_kernel_batch(matcher, cs), cs):
            same(got, run_reference(one), kind + " batch")
