"""The numpy reference of CreateNewMapPoints' geometry (tests/newpoints_reference.py) checked on its own, the scenes of the GPU
test against the caps of the guard bands, and the HOST build of the geometry the kernel runs (csrc/orbm_new_points_geometry.h,
through tests/newpoints_geometry_check.cpp) against the reference.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import newpoints_common as NC
import newpoints_reference as R

ROOT = NC.ROOT

SPREAD_F32, TRI_DOUBLE_BOUND_REL, TRI_DOUBLE_BOUND_ABS = NC.SPREAD_F32, NC.TRI_DOUBLE_BOUND_REL, NC.TRI_DOUBLE_BOUND_ABS


@pytest.fixture(scope="module")
def scenes(oracle):
    out = []
    for name, kw in NC.SCENES:
        sc = NC.make_scene(kw)
        out.append((name, sc, R.create_new_map_points(sc, NC.oracle_search(oracle, sc), np.float64)))
    return out


def test_scenes_stay_within_the_caps(scenes):
    """the guard bands leave at most 1 % of the reached pairs and 2 % of key frame 1's features undecided, every gate cuts both
    ways somewhere, and the plain-numpy search equals the C++ oracle's"""
    rejected_at, accepted, stereo = set(), 0, 0
    for name, sc, ref in scenes:
        pairs, feats = NC.shares(ref)
        print("%s: %d reached pairs, %d created, undecided pairs %.4f features %.4f" % (name, len(ref["pairs"]), ref["n_created"].sum(), pairs, feats))
        assert pairs <= NC.CAP_PAIRS and feats <= NC.CAP_FEATURES, name
        assert ref["n_created"].sum() > 200 and len(ref["pairs"]) > 2 * ref["n_created"].sum() * 0.6, name
        rejected_at |= {p[7][-1][0] for p in ref["pairs"] if not p[3] and p[7]}
        accepted += int(ref["n_created"].sum())
        stereo += int(ref["point_stereo"].sum())
        assert (ref["n_matched"] > 0).all()
    assert {"cosRays<bound", "z1>0", "reproj1", "reproj2", "far1", "scale_lo", "scale_hi"} <= rejected_at, rejected_at
    assert 0 < stereo < accepted
    name, sc, ref = scenes[0]
    search = R.numpy_search(sc)
    assert np.array_equal(search(0, sc["kf1"]["has_mp"]), ref["match12"][0])


def test_accepted_points_reproject_within_the_gates(scenes):
    for name, sc, ref in scenes:
        kf1 = sc["kf1"]
        for (i1, j, i2, accept, _, _, x3d, _) in ref["pairs"]:
            if not accept:
                continue
            for kf, i in ((kf1, i1), (sc["neighbours"][j], i2)):
                Xc = kf["Rcw"].astype(np.float64).reshape(3, 3) @ x3d + kf["tcw"]
                assert Xc[2] > 0
                u, v = kf["fx"] * Xc[0] / Xc[2] + kf["cx"], kf["fy"] * Xc[1] / Xc[2] + kf["cy"]
                s2 = float(kf["level_sigma2"][kf["octave"][i]])
                e2 = (u - kf["x"][i]) ** 2 + (v - kf["y"][i]) ** 2
                if kf["u_right"][i] >= 0:
                    e2 += (u - float(kf1["mbf"]) / Xc[2] - kf["u_right"][i]) ** 2
                    assert e2 <= 7.8 * s2 * (1 + 1e-9)
                else:
                    assert e2 <= 5.991 * s2 * (1 + 1e-9)


def test_noise_free_triangulation_equals_ground_truth():
    """without pixel noise, wrong matches or stereo, every triangulated point is the world point it came from, to the accuracy
    of the float pixel coordinates and poses"""
    sc = NC.make_scene(dict(seed=21, n=300, n_neighbours=4, noise_px=0.0, wrong_frac=0.0, off_octave_frac=0.0, clutter_frac=0.0))
    ref = R.create_new_map_points(sc, R.numpy_search(sc), np.float64)
    assert ref["n_created"].sum() > 50
    worst = 0.0
    for (i1, j, i2, accept, _, sinp, x3d, _) in ref["pairs"]:
        if accept:
            assert sc["truth"]["neighbours"][j]["point"][i2] == sc["truth"]["point1"][i1]
            worst = max(worst, NC.point_error(x3d, sc["truth"]["Xw"][sc["truth"]["point1"][i1]], sc["kf1"]["Ow"], sinp))
    print("noise-free: worst point error %.3g" % worst)
    assert worst < 16 * 2.0 ** -24         # a handful of float roundings: pixel coordinates (2^-24 of ~500 px over f), rotation, translation


def test_null_vector_svd_and_long_double_eigen_agree(scenes):
    name, sc, ref = scenes[0]
    C1 = R._cast(R.camera_of(sc["kf1"]), np.float64)
    n, worst = 0, 0.0
    for (i1, j, i2, accept, _, _, x3d, _) in ref["pairs"][:400]:
        if not accept or ref["point_stereo"][i1]:
            continue
        C2 = R._cast(R.camera_of(sc["neighbours"][j]), np.float64)
        o1, o2 = R.obs_of(sc["kf1"], i1), R.obs_of(sc["neighbours"][j], i2)
        xn1 = [(o1["x"] - C1["cx"]) / C1["fx"], (o1["y"] - C1["cy"]) / C1["fy"]]
        xn2 = [(o2["x"] - C2["cx"]) / C2["fx"], (o2["y"] - C2["cy"]) / C2["fy"]]
        A = R.triangulation_matrix(xn1, xn2, np.c_[C1["Rcw"], C1["tcw"]], np.c_[C2["Rcw"], C2["tcw"]], np.float64)
        a, b = R.null_vector_svd(A), np.asarray(R.null_vector_eig_longdouble(A), np.float64)
        worst = max(worst, min(np.abs(a - b).max(), np.abs(a + b).max()))
        n += 1
    assert n > 50 and worst < 1e-10, (n, worst)


def _toy_pair():
    """two cameras 0.3 apart looking down +z, a point at depth 4 seen by both without noise"""
    cam = dict(Rcw=np.eye(3, dtype=np.float32), tcw=np.zeros(3, np.float32), Ow=np.zeros(3, np.float32), fx=np.float32(458), fy=np.float32(457),
               cx=np.float32(367), cy=np.float32(248), invfx=np.float32(1) / np.float32(458), invfy=np.float32(1) / np.float32(457),
               mb=np.float32(0.11), mbf=np.float32(0.11 * 458))
    cam2 = dict(cam, tcw=np.array([-0.3, 0, 0], np.float32), Ow=np.array([0.3, 0, 0], np.float32))
    X = np.array([0.5, 0.2, 4.0])

    def obs(c, stereo):
        Xc = X + c["tcw"]
        u, v = c["fx"] * Xc[0] / Xc[2] + c["cx"], c["fy"] * Xc[1] / Xc[2] + c["cy"]
        return dict(x=np.float32(u), y=np.float32(v), ur=np.float32(u - c["mbf"] / Xc[2]) if stereo else np.float32(-1),
                    depth=np.float32(Xc[2]) if stereo else np.float32(-1), kx=np.float32(u), ky=np.float32(v), sigma2=np.float32(1), scale=np.float32(1))

    rule = dict(inertial=False, far_points=False, th_far=0.0, scale_factor_1=1.2)
    return cam, cam2, obs, rule, X


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_quirk_mbf_of_key_frame_1(T):
    """:669: a neighbour with another stereo rig whose u_right is consistent with its OWN mbf fails the 7.8 gate because the
    reference predicts its right-image column with key frame 1's mbf"""
    cam, cam2, obs, rule, _ = _toy_pair()
    cam2 = dict(cam2, mb=np.float32(0.2), mbf=np.float32(0.2 * 458))
    o1, o2 = obs(cam, False), obs(cam2, True)
    assert not R.pair_geometry(cam, o1, cam2, o2, rule, T)["accept"]
    g = R.pair_geometry(cam, o1, cam2, o2, rule, T, quirks=dict(mbf_of_kf1=False))
    assert g["accept"] and not g["undecided"]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_quirk_else_if_stereo2(T):
    """:575: both key points stereo, the neighbour much closer to the point: its stereo parallax would win and send the pair to
    UnprojectStereo, but it is never computed, so the pair is triangulated"""
    cam, cam2, obs, rule, X = _toy_pair()
    cam2 = dict(cam2, tcw=np.array([-0.38, -0.12, -2.4], np.float32), Ow=np.array([0.38, 0.12, 2.4], np.float32))
    o1, o2 = obs(cam, True), obs(cam2, True)        # stereo parallax 0.0275 (depth 4) and 0.069 (depth 1.6), ray parallax 0.05
    g = R.pair_geometry(cam, o1, cam2, o2, rule, T)
    h = R.pair_geometry(cam, o1, cam2, o2, rule, T, quirks=dict(else_if_stereo2=False))
    assert not g["point_stereo"] and h["point_stereo"]
    assert not g["undecided"] and not h["undecided"]


@pytest.mark.parametrize("T", [np.float32, np.float64])
def test_quirk_unproject_stereo_reads_distorted_key_points(T):
    """KeyFrame.cc:760-761: with a short baseline the stereo key point of key frame 1 is unprojected, from mvKeys"""
    cam, cam2, obs, rule, X = _toy_pair()
    cam2 = dict(cam2, tcw=np.array([-0.01, 0, 0], np.float32), Ow=np.array([0.01, 0, 0], np.float32))
    o1, o2 = obs(cam, True), obs(cam2, False)
    o1["kx"] = np.float32(o1["x"] + 1.5)
    g = R.pair_geometry(cam, o1, cam2, o2, rule, T)
    h = R.pair_geometry(cam, o1, cam2, o2, rule, T, quirks=dict(unproject_distorted=False))
    assert g["point_stereo"] and h["point_stereo"] and g["x3d"] is not None
    assert abs((g["x3d"][0] - h["x3d"][0]) - 1.5 * 4.0 / 458) < 1e-4 and abs(h["x3d"][0] - X[0]) < 1e-4


def test_quirk_double_thresholds():
    """:637: (float) > 5.991 * (float) is evaluated in double.  5.991f is above 5.991, so an error of exactly 5.991f * sigma2 is
    rejected by the reference and would pass a float comparison."""
    e2, s2 = np.float32(5.991), np.float32(1.0)
    assert float(e2) > R.chi2_threshold(5.991, s2, True)
    assert not float(e2) > R.chi2_threshold(5.991, s2, False)
    e2 = np.float32(7.8)                                # 7.8f is above 7.8 as well
    assert float(e2) > R.chi2_threshold(7.8, s2, True) and not float(e2) > R.chi2_threshold(7.8, s2, False)


def test_float32_reference_within_the_guard_and_spread(scenes):
    """float32 against float64 (neither is the code under test): no decision flips outside the guard bands; the point spread
    is what the device test's tolerance is derived from"""
    worst = 0.0
    for name, sc, ref in scenes:
        r32 = R.create_new_map_points(sc, lambda j, has_mp, ref=ref: ref["match12"][j], np.float32)
        errs = NC.compare(ref, r32, sc, name)
        worst = max(worst, max(errs))
        print("%s: float32 vs float64 point metric max %.3g p99 %.3g over %d points" % (name, max(errs), np.percentile(errs, 99), len(errs)))
    assert worst <= 1.5 * SPREAD_F32, worst


@pytest.fixture(scope="module")
def geometry_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nmp") / "newpoints_geometry_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-o", exe, os.path.join(ROOT, "tests", "newpoints_geometry_check.cpp")])
    return exe


def run_host_geometry(exe, sc, triples, tmp):
    NC.pack_pairs(sc, triples).tofile(os.path.join(tmp, "in.bin"))
    subprocess.check_call([exe, os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")])
    return np.fromfile(os.path.join(tmp, "out.bin"), np.float32).reshape(-1, 10)


def test_host_build_of_the_kernel_geometry(scenes, geometry_exe, tmp_path):
    """the text the kernel compiles, built for the host: decisions outside the guard bands, points within 4 x the float32
    spread of the float64 reference and within TRI_DOUBLE_BOUND of the float64 null vector of the same float matrix, normal and
    distances as MapPoint::UpdateNormalAndDepth gives them"""
    for name, sc, ref in scenes:
        out = run_host_geometry(geometry_exe, sc, [p[:3] for p in ref["pairs"]], str(tmp_path))
        assert len(out) == len(ref["pairs"])
        kf1 = sc["kf1"]
        worst, worst_tri = 0.0, 0.0
        for p, r in zip(ref["pairs"], out):
            i1, j, i2, accept, undecided, sinp, x3d, _ = p
            if undecided:
                continue
            assert bool(r[0]) == accept, (name, p[:5], p[7])
            if not accept:
                continue
            kf2 = sc["neighbours"][j]
            g = R.pair_geometry(R.camera_of(kf1), R.obs_of(kf1, i1), R.camera_of(kf2), R.obs_of(kf2, i2), sc["params"], np.float64, matrix_dtype=np.float32)
            assert bool(r[1]) == g["point_stereo"]
            worst = max(worst, NC.point_error(r[2:5], x3d, kf1["Ow"], sinp))
            if not g["point_stereo"]:
                d = np.abs(r[2:5].astype(np.float64) - g["x3d"])
                bound = TRI_DOUBLE_BOUND_REL * np.abs(g["x3d"]) + TRI_DOUBLE_BOUND_ABS * np.linalg.norm(g["x3d"])
                worst_tri = max(worst_tri, (d / bound).max())
            nrm, mx, mn = R.normal_and_depth(r[2:5], kf1["Ow"], kf2["Ow"], kf1["scale_factors"][kf1["octave"][i1]], kf1["scale_factors"][-1])
            assert np.abs(r[5:8] - nrm).max() < 1e-6 and abs(r[8] / mx - 1) < 1e-6 and abs(r[9] / mn - 1) < 1e-6
        print("%s: host build point metric max %.3g (bar %.3g), worst share of the double bar %.3f" % (name, worst, 4 * SPREAD_F32, worst_tri))
        assert worst <= 4 * SPREAD_F32
        assert worst_tri <= 1.0


def test_golden_file_satisfies_the_caps_and_is_reproducible(oracle):
    d = dict(np.load(os.path.join(ROOT, "tests", "golden", "new_map_points_100.npz")))
    sc, ref = NC.unflatten(d)
    pairs, feats = NC.shares(ref)
    assert pairs <= NC.CAP_PAIRS and feats <= NC.CAP_FEATURES
    assert ref["n_created"].sum() >= 20 and 0 < ref["point_stereo"].sum() < ref["n_created"].sum()
    again = R.create_new_map_points(sc, NC.oracle_search(oracle, sc), np.float64)
    for k in ("neighbour", "idx2", "x3d", "point_stereo", "undecided_from", "n_matched", "n_created"):
        assert np.array_equal(again[k], ref[k]), k
    assert [p[:5] for p in again["pairs"]] == [p[:5] for p in ref["pairs"]]
    size = os.path.getsize(os.path.join(ROOT, "tests", "golden", "new_map_points_100.npz"))
    others = [os.path.getsize(os.path.join(ROOT, "tests", "golden", f)) for f in os.listdir(os.path.join(ROOT, "tests", "golden"))
              if not f.startswith("new_map_points")]
    assert size <= max(others)
