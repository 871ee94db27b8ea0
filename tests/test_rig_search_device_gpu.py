"""The two device-resident rig searches (include/orbslam3_hip_rig_track_device.h) against the expectations stated in
tests/rig_match_cases.py, the numpy restatement (tests/rig_match_reference.py) and the host-array batch entries: assign, occupied and
n_matches integer for integer, no tolerance.  The calls travel as [batch][cap] device arrays packed by tests/rig_track_device_pack.py,
whose fill rows, spare rows and spare slots hold sentinels."""
import copy

import numpy as np
import pytest

import rig_match_cases as cases
import rig_track_device_pack as DP
from test_rig_match_reference import run_reference

pytestmark = pytest.mark.gpu

HAND = cases.hand_built()
ERR_CAPACITY = -2
SHAPES = [k + s for k in ("mp", "last") for s in ("_no_left_features", "_no_right_features", "_no_points", "_65_points", "_129_points", "_70_features_in_one_cell",
                                                   "_window_wider_than_16_columns", "_batch_of_3", "_unstaged_%d_a_side" % cases.UNSTAGED_N)]


@pytest.fixture(scope="module")
def torch():
    return pytest.importorskip("torch")


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.Matcher(0.8, True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def shapes():
    return cases.shape_calls()


@pytest.fixture(scope="module")
def random_batches():
    """kind -> (the random rigs of the kind that share th, their reference results): computed once, never modified"""
    r = cases.random_calls()
    out = {}
    for kind in ("mp", "last"):
        cs = [r["%s_random_%d" % (kind, s)] for s in cases.RANDOM_SEEDS]
        cs = [c for c in cs if c["th"] == cs[-1]["th"]]
        out[kind] = (cs, [run_reference(c) for c in cs])
    return out


def run_device(torch, m, calls, spare=1, **kw):
    p = DP.pack(calls, spare)
    r = DP.Resident(torch, p)
    r.launch(m, **kw)
    per, raw = r.results()
    DP.check_untouched(p, raw, kw.get("n_slots", True))
    return per, r


def run_host_batch(m, cs):
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


def hand_groups():
    groups = {}
    for name in sorted(HAND):
        c = HAND[name]
        groups.setdefault((c["kind"], c["th"], c["nnratio"], c["far_points"], c["th_far"], c["check_ori"]), []).append(name)
    return groups


def test_hand_built_calls_as_batches(torch, matcher):
    """every hand-built call, grouped by launch parameters: one batch per group, every frame equals its stated expectation; the level
    windows of the last-frame calls travel through d_level_window"""
    groups = hand_groups()
    assert len(HAND) == 33
    assert max(len(c["rig"]["left"]["x"]) for c in HAND.values()) == 7 and max(len(c["rig"]["right"]["x"]) for c in HAND.values()) == 2
    assert sorted(len(v) for k, v in groups.items() if k[0] == "last") == [1, 11] and sorted(len(v) for k, v in groups.items() if k[0] == "mp") == [1, 1, 1, 4, 14]
    windows = set()
    for key, names in groups.items():
        cs = [HAND[n] for n in names]
        per, _ = run_device(torch, matcher, cs)
        for name, got in zip(names, per):
            e = HAND[name]["expect"]
            same(got, (e["n"], e["assign"], e["occupied"]), "batch " + name)
        if key[0] == "last":
            windows |= {c["pts"]["level_window"] for c in cs}
            # without d_level_window every frame searches ORBM_LEVELS_AROUND
            around = [dict(c, pts=dict(c["pts"], level_window=0)) for c in cs]
            per, _ = run_device(torch, matcher, cs, level_window=False)
            for name, got, c in zip(names, per, around):
                same(got, run_reference(c), "no level windows: " + name)
    assert windows == {0, 1, 2}


@pytest.mark.parametrize("name", SHAPES)
def test_shape_call(torch, matcher, shapes, name):
    c = shapes[name]
    cs = c if isinstance(c, list) else [c]
    per, _ = run_device(torch, matcher, cs)
    for k, (got, one) in enumerate(zip(per, cs)):
        want = run_reference(one)
        if not isinstance(c, list) and "no_points" not in name and "no_left" not in name and "no_right" not in name:
            assert want[0] > 0, name
        same(got, want, "%s[%d]" % (name, k))


def test_shape_names(shapes):
    """every shape of the host entries' tests but the two whose grid is built on the host, and the middle frame of the batch is empty"""
    assert sorted(SHAPES + ["%s_host_grid_%d_and_%d" % ((k,) + cases.HOST_GRID_N) for k in ("mp", "last")]) == sorted(shapes)
    for k in ("mp", "last"):
        mid = shapes[k + "_batch_of_3"][1]["rig"]
        assert len(mid["left"]["x"]) == 0 and len(mid["right"]["x"]) == 0


def test_side_of_8193_features_is_refused(torch, matcher, shapes):
    p = DP.pack([shapes["last_no_points"]])
    r = DP.Resident(torch, p)
    for side in ("cap_l", "cap_r"):
        p["frames"] = dict(p["frames"], **{side: 8193, "slot_cap": 8193 + 8192})
        with pytest.raises(RuntimeError) as e:
            r.launch(matcher)
        assert e.value.code == ERR_CAPACITY
        p["frames"] = dict(p["frames"], **{side: 8192})


@pytest.mark.parametrize("kind", ["mp", "last"])
def test_random_rigs_as_a_batch(torch, matcher, random_batches, kind):
    cs, want = random_batches[kind]
    assert len(cs) >= 2 and all(w[0] > 20 for w in want)
    per, r = run_device(torch, matcher, cs)
    host = run_host_batch(matcher, cs)
    for b, (got, w, h) in enumerate(zip(per, want, host)):
        same(got, w, "%s frame %d against the restatement" % (kind, b))
        same(got, h, "%s frame %d against the host batch entry" % (kind, b))
    r.reset_outputs()
    r.launch(matcher)
    twice, raw = r.results()
    DP.check_untouched(r.p, raw)
    for b, (got, first) in enumerate(zip(twice, per)):
        same(got, first, "%s frame %d, second call" % (kind, b))


def test_without_has_obs_every_point_has_observations(torch, matcher, random_batches):
    cs, _ = random_batches["last"]
    ones = [dict(c, pts=dict(c["pts"], has_obs=np.ones_like(c["pts"]["has_obs"]))) for c in cs]
    per, _ = run_device(torch, matcher, cs, has_obs=False, n_slots=False)
    for b, (got, c) in enumerate(zip(per, ones)):
        same(got, run_reference(c), "frame %d" % b)


@pytest.mark.parametrize("kind", ["mp", "last"])
def test_what_the_host_entries_refuse_is_clamped(torch, matcher, random_batches, kind):
    """Counts of cap + 5, a partner entry of n_r + 3 and a live level of n_levels in frame 1 of the random batch (whose frames all fill
    their capacities): the result is that of the clamped and sanitised values.  Every array has a spare row and every slot row spare
    slots, so an implementation without a clamp stays inside the allocations and fails here by comparison."""
    cs, want = random_batches[kind]
    p = DP.pack(cs, spare=1)
    h, b = p["host"], 1
    nl, nr, n = p["nl"][b], p["nr"][b], int(cs[b]["pts"]["n"])
    assert (nl, nr, n) == (p["frames"]["cap_l"], p["frames"]["cap_r"], p["cap"]) and min(nl, nr, n) >= 5
    fixed = copy.deepcopy(cs[b])
    for k in ("d_n_l", "d_n_r", "d_n"):
        h[k][b] = {"d_n_l": nl, "d_n_r": nr, "d_n": n}[k] + 5
    i = int(np.nonzero(cs[b]["rig"]["left_to_right"] >= 0)[0][0])
    h["d_left_to_right"][b, i] = nr + 3; fixed["rig"]["left_to_right"][i] = -1
    top = cases.NLEVELS - 1
    if kind == "last":
        j = int(np.nonzero(cs[b]["pts"]["valid"])[0][0])
        h["d_octave"][b, j] = cases.NLEVELS; fixed["pts"]["octave"][j] = top
    else:
        j = int(np.nonzero(cs[b]["pts"]["in_view"])[0][0]); jr = int(np.nonzero(cs[b]["pts"]["in_view_r"] & (cs[b]["pts"]["pred_level_r"] >= 0))[0][1])
        h["d_pred_level"][b, j] = cases.NLEVELS; fixed["pts"]["pred_level"][j] = top
        h["d_pred_level_r"][b, jr] = cases.NLEVELS + 3; fixed["pts"]["pred_level_r"][jr] = top
    r = DP.Resident(torch, p)
    r.launch(matcher)
    per, raw = r.results()
    DP.check_untouched(p, raw)
    for f, got in enumerate(per):
        same(got, run_reference(fixed) if f == b else want[f], "%s frame %d" % (kind, f))
    for k in p["host"]:
        if k not in DP.OUT_ARRAYS:
            np.testing.assert_array_equal(r.down(k), p["host"][k], err_msg="input array %s was written" % k)
