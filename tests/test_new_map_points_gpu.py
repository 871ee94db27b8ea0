"""orbm_create_new_map_points on the device against the composite reference: per neighbour in order, the C++ oracle's
SearchForTriangulation (check_ori = False) with the current has_mp of key frame 1, tests/newpoints_reference.py in float64 on
the matches, has_mp for the accepted ones.

Tolerances.  Decisions: identical outside the guard bands of newpoints_reference (1e-6 on cosines, 1e-3 relative on the
reprojection / far / scale gates, 1e-3 of the distance on the depth signs); the scenes leave <= 1 % of the reached pairs and
<= 2 % of the features undecided (measured on the CPU: at most 0.51 % / 0.58 %, test_newpoints_reference.py).  Points:
|x_dev - x_ref64| / |x_ref64 - Ow1| * sin(parallax); the float32 run of the reference differs from the float64 run by at most
1.02e-7 on these scenes (p99 9.5e-8; measured on the CPU, neither is the code under test), the device gets 4 x that.  Points
the kernel triangulates additionally meet TRI_DOUBLE_BOUND against the float64 null vector of the same float matrix.
The host build of the kernel's geometry meets all of these (test_newpoints_reference.py: worst point metric 9.5e-8, worst
share of the double bar 0.94); the device's own figures have not been recorded yet, the tests print them."""
import ctypes as C
import os

import numpy as np
import pytest

import newpoints_common as NC
import newpoints_reference as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.Matcher(0.6, False)
    yield m
    m.close()


def run(matcher, sc):
    return matcher.create_new_map_points(sc["kf1"], sc["neighbours"], sc["pairs"], sc["params"])


def check_against_reference(matcher, oracle, sc, label):
    ref = R.create_new_map_points(sc, NC.oracle_search(oracle, sc), np.float64)
    pairs, feats = NC.shares(ref)
    print("%s: %d reached pairs, undecided pairs %.4f features %.4f" % (label, len(ref["pairs"]), pairs, feats))
    assert pairs <= NC.CAP_PAIRS and feats <= NC.CAP_FEATURES
    dev = run(matcher, sc)
    errs = NC.compare(ref, dev, sc, label)
    created = dev["neighbour"] >= 0
    assert dev["created"] == int(created.sum()) == int(dev["n_created"].sum())
    assert np.array_equal(dev["n_created"], np.bincount(dev["neighbour"][created], minlength=len(sc["neighbours"])))
    assert (dev["idx2"][~created] == -1).all() and (dev["x3d"][~created] == 0).all() and (dev["normal"][~created] == 0).all()
    assert (dev["match12"][:, np.asarray(sc["kf1"]["has_mp"], bool)] == -1).all()
    if errs:
        print("%s: device point metric max %.3g p99 %.3g over %d points (bar %.3g)" % (label, max(errs), np.percentile(errs, 99), len(errs), 4 * NC.SPREAD_F32))
        assert max(errs) <= 4 * NC.SPREAD_F32
    return ref, dev


def check_triangulated_in_double(sc, ref, dev, label):
    kf1 = sc["kf1"]
    worst, n = 0.0, 0
    for (i1, j, i2, accept, undecided, _, _, _) in ref["pairs"]:
        if not accept or undecided or dev["neighbour"][i1] != j or dev["point_stereo"][i1]:
            continue
        kf2 = sc["neighbours"][j]
        g = R.pair_geometry(R.camera_of(kf1), R.obs_of(kf1, i1), R.camera_of(kf2), R.obs_of(kf2, i2), sc["params"], np.float64, matrix_dtype=np.float32)
        d = np.abs(dev["x3d"][i1].astype(np.float64) - g["x3d"])
        worst = max(worst, (d / (NC.TRI_DOUBLE_BOUND_REL * np.abs(g["x3d"]) + NC.TRI_DOUBLE_BOUND_ABS * np.linalg.norm(g["x3d"]))).max())
        n += 1
    print("%s: worst share of the double bar %.3f over %d triangulated points" % (label, worst, n))
    assert worst <= 1.0


def check_normal_and_depth(matcher, sc, dev):
    """bit-identical to orbm_update_normal_and_depth on the device's own x3d and the two camera centres"""
    kf1 = sc["kf1"]
    idx = np.nonzero(dev["neighbour"] >= 0)[0]
    if len(idx) == 0:
        return
    centers = np.empty((len(idx), 2, 3), np.float32)
    centers[:, 0] = kf1["Ow"]
    centers[:, 1] = np.array([sc["neighbours"][j]["Ow"] for j in dev["neighbour"][idx]], np.float32)
    nrm, mx, mn = matcher.UpdateNormalAndDepth(dev["x3d"][idx], centers.reshape(-1, 3), np.arange(len(idx) + 1, dtype=np.int32) * 2,
                                               np.tile(kf1["Ow"], (len(idx), 1)), kf1["scale_factors"][kf1["octave"][idx]], kf1["scale_factors"][-1])
    assert np.array_equal(nrm.view(np.uint32), dev["normal"][idx].view(np.uint32))
    assert np.array_equal(mx.view(np.uint32), dev["max_dist"][idx].view(np.uint32))
    assert np.array_equal(mn.view(np.uint32), dev["min_dist"][idx].view(np.uint32))


@pytest.mark.parametrize("name,kw", NC.SCENES, ids=[s[0] for s in NC.SCENES])
def test_create_new_map_points(matcher, oracle, name, kw):
    sc = NC.make_scene(kw)
    ref, dev = check_against_reference(matcher, oracle, sc, name)
    assert dev["created"] > 200
    check_triangulated_in_double(sc, ref, dev, name)
    check_normal_and_depth(matcher, sc, dev)


def test_golden_scene(matcher):
    d = dict(np.load(os.path.join(NC.ROOT, "tests", "golden", "new_map_points_100.npz")))
    sc, ref = NC.unflatten(d)
    pairs, feats = NC.shares(ref)
    assert pairs <= NC.CAP_PAIRS and feats <= NC.CAP_FEATURES
    dev = run(matcher, sc)
    errs = NC.compare(ref, dev, sc, "golden")
    assert dev["created"] >= 20 and max(errs) <= 4 * NC.SPREAD_F32
    check_normal_and_depth(matcher, sc, dev)


def test_neighbour_order(matcher, oracle):
    """permuting the neighbours changes the outcome only as the reference's order dependence says"""
    sc = NC.make_scene(NC.SCENES[3][1])
    base = run(matcher, sc)
    order = [7, 2, 9, 0, 4, 1, 8, 3, 6, 5]
    ps = NC.sub_scene(sc, order)
    ref, dev = check_against_reference(matcher, oracle, ps, "permuted")
    assert not np.array_equal(np.asarray(order)[np.maximum(dev["neighbour"], 0)][dev["neighbour"] >= 0], base["neighbour"][dev["neighbour"] >= 0]) \
        or not np.array_equal(dev["neighbour"] >= 0, base["neighbour"] >= 0)       # the order matters on this scene


def test_single_neighbour_equals_search_plus_geometry(matcher, oracle):
    sc = NC.make_scene(NC.SCENES[4][1])
    for j in (0, 5):
        one = NC.sub_scene(sc, [j])
        dev = run(matcher, one)
        kf2, pr = one["neighbours"][0], one["pairs"][0]
        k1 = dict(sc["kf1"])
        n, m12 = matcher.SearchForTriangulation(k1, kf2, pr["ep"], pr["F12"], kf2["level_sigma2"], kf2["scale_factors"], False, pr["coarse"])
        assert dev["n_matched"][0] == n and np.array_equal(dev["match12"][0], m12)
        ref = R.create_new_map_points(one, lambda _, has_mp: m12, np.float64)
        NC.compare(ref, dev, one, "single %d" % j)
        created = dev["neighbour"] >= 0
        assert created.sum() > 20 and np.array_equal(dev["idx2"][created], m12[created])


def test_degenerate_calls_return_nothing(matcher):
    sc = NC.make_scene(dict(seed=31, n=200, n_neighbours=3, stereo_frac=0.3))

    def clean(dev, nb):
        assert dev["created"] == 0 and (dev["neighbour"] == -1).all() and (dev["idx2"] == -1).all() and (dev["x3d"] == 0).all()
        assert (dev["point_stereo"] == 0).all() and (dev["normal"] == 0).all() and (dev["max_dist"] == 0).all() and (dev["min_dist"] == 0).all()
        assert len(dev["n_matched"]) == nb and (dev["n_created"] == 0).all()

    clean(run(matcher, NC.sub_scene(sc, [])), 0)                                    # n_neighbours = 0
    full = dict(sc); full["kf1"] = dict(sc["kf1"], has_mp=np.ones_like(sc["kf1"]["has_mp"]))
    dev = run(matcher, full); clean(dev, 3)                                         # every feature already holds a map point
    assert (dev["n_matched"] == 0).all()
    away = dict(sc); nb = [dict(k) for k in sc["neighbours"]]
    nodes, off, feat = nb[1]["fv"]
    nb[1]["fv"] = ((nodes + np.uint32(1000)).astype(np.uint32), off, feat)          # no vocabulary node in common with key frame 1
    away["neighbours"] = nb
    dev = run(matcher, away)
    assert dev["n_matched"][1] == 0 and dev["n_created"][1] == 0 and dev["created"] > 0 and (dev["neighbour"] != 1).all()
    empty = dict(sc)                                                                # n1 = 0
    k = sc["kf1"]
    empty["kf1"] = dict(k, desc=np.zeros((0, 32), np.uint8), fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)),
                        **{f: k[f][:0] for f in ("x", "y", "octave", "has_mp", "stereo", "u_right", "depth")})
    dev = run(matcher, empty)
    assert dev["created"] == 0 and len(dev["neighbour"]) == 0 and (dev["n_matched"] == 0).all()


def test_repeated_calls_are_bitwise_equal(matcher):
    sc = NC.make_scene(NC.SCENES[3][1])
    small = NC.make_scene(dict(seed=31, n=200, n_neighbours=3))
    a = run(matcher, sc)
    run(matcher, small)                                                             # another shape in between, on the same handle
    b = run(matcher, sc)
    for k in a:
        assert np.array_equal(np.asarray(a[k]).view(np.uint8) if isinstance(a[k], np.ndarray) else a[k],
                              np.asarray(b[k]).view(np.uint8) if isinstance(b[k], np.ndarray) else b[k]), k
    assert matcher.create_new_map_points_last_kernel_ms() > 0


def test_bad_arguments_leave_the_handle_usable(pkg, matcher):
    sc = NC.make_scene(dict(seed=31, n=200, n_neighbours=3))
    good = run(matcher, sc)
    bad = dict(sc); bad["neighbours"] = [dict(k) for k in sc["neighbours"]]
    bad["neighbours"][2]["octave"] = bad["neighbours"][2]["octave"].copy(); bad["neighbours"][2]["octave"][0] = 99
    with pytest.raises(pkg.OrbxError) as e:
        run(matcher, bad)
    assert e.value.code == -3
    many = NC.sub_scene(sc, [0] * (pkg.ORBM_MAX_NEIGHBOURS + 1))
    with pytest.raises(pkg.OrbxError) as e:
        run(matcher, many)
    assert e.value.code == -3
    again = run(matcher, sc)
    assert np.array_equal(good["neighbour"], again["neighbour"]) and np.array_equal(good["x3d"], again["x3d"])
    most = run(matcher, NC.sub_scene(sc, [0, 1, 2] * 21 + [0]))                     # ORBM_MAX_NEIGHBOURS itself is accepted
    assert most["created"] >= good["created"]
