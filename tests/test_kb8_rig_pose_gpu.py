"""PoseOptimization of a frame of a two-camera KannalaBrandt8 rig (pose_set_rig_kb8) against tests/kb8_rig_reference.py on
tests/golden/kb8_rig_pose_60.npz (60 edges, 30 of them on the right camera, 9 outliers: the two-edges-per-thread kernel) and
kb8_rig_pose_560.npz (560 edges, 281 right, 28 outliers: the four-edges-per-thread kernel).

Tolerance: 4 S, S = the spread of the reference under its one-ulp switch (tools/make_kb8_rig_golden.py), per output.  Outlier
flags, inliers and n_bad are demanded exactly, and so are iterations and trials per round against the reference's device model
(where the fixture says the model pins them: counts_pinned), for the reasons tests/test_kb8_pose_gpu.py gives; the chi2 per round
then agrees with the device model's to f64 accumulation, 1e-9 relative as there."""
import importlib

import numpy as np
import pytest

from kb8_rig_cases import ERR_ARG, SOLVER_FACTOR, all_left, pose_fixture, same_bits, with_kind

pytestmark = pytest.mark.gpu

BITS = ("q", "t", "outlier", "inliers", "n_bad", "iterations", "trials", "chi2")


def _check(r, g):
    np.testing.assert_array_equal(r["outlier"], g["ref_outlier"])
    assert (r["inliers"], r["n_bad"]) == (int(g["ref_inliers"]), int(g["ref_n_bad"]))
    for k, ref, S in (("q", g["ref_q"], float(g["S_q"])), ("t", g["ref_t"], float(g["S_t"])), ("chi2", g["ref_chi2"], float(g["S_chi2"]))):
        d = float(np.abs(np.asarray(r[k]) - ref).max())
        print("%s: |device - reference| %.3g, S %.3g" % (k, d, S))
        assert d <= SOLVER_FACTOR * S, k
    print("iterations %s trials %s (device model %s %s, host reference %s %s, counts pinned %d)" % (
        r["iterations"], r["trials"], g["dev_iterations"].tolist(), g["dev_trials"].tolist(), g["ref_iterations"].tolist(), g["ref_trials"].tolist(), int(g["counts_pinned"])))
    if int(g["counts_pinned"]):
        assert list(r["iterations"]) == g["dev_iterations"].tolist() and list(r["trials"]) == g["dev_trials"].tolist()
        np.testing.assert_allclose(r["chi2"], g["dev_chi2"], rtol=1e-9, atol=0)


@pytest.fixture(scope="module")
def solved(pkg):
    """the 60-edge fixture solved once on a fresh handle: the bits every later test compares with"""
    w, rig, g = pose_fixture(60)
    s = pkg.PoseSolver()
    try:
        s.set_rig_kb8(rig)
        return s.optimize_one(w)
    finally:
        s.close()


def test_pose_optimize_rig_60(solved):
    _check(solved, pose_fixture(60)[2])


def test_pose_optimize_rig_560(pkg):
    w, rig, g = pose_fixture(560)
    assert len(w["Xw"]) > 512
    s = pkg.PoseSolver()
    try:
        s.set_rig_kb8(rig)
        _check(s.optimize_one(w), g)
    finally:
        s.close()


def test_left_edges_under_a_rig_equal_the_monocular_camera(pkg):
    for n in (60, 560):
        w, rig, _ = pose_fixture(n)
        wl = all_left(w, "stereo")
        s = pkg.PoseSolver()
        try:
            s.set_rig_kb8(rig)
            a = s.optimize_one(wl)
            s.set_camera_kb8(rig["left"])           # the last setter wins
            b = s.optimize_one(wl)
        finally:
            s.close()
        same_bits(a, b, BITS)


def test_batch_equals_single_calls(pkg, solved):
    sk = importlib.import_module("orb_slam3-1_amd.synth_kb8")
    w, rig, g = pose_fixture(60)
    frames = [w, sk.perturbed_frame(w, 1), sk.perturbed_frame(w, 2)]
    s = pkg.PoseSolver()
    try:
        s.set_rig_kb8(rig)
        batch = s.optimize_batch(frames)
        for f, b in zip(frames, batch):
            same_bits(b, s.optimize_one(f), BITS)
    finally:
        s.close()
    same_bits(batch[0], solved, BITS)


def test_wrong_implementations_are_caught(pkg):
    """guards the tests, not the code: a rig with the cameras swapped, without R_rl, or with the right edges solved as left ones
    must change n_bad or move the pose by more than the tolerance"""
    w, rig, g = pose_fixture(60)
    swapped = dict(rig, left=rig["right"], right=rig["left"])
    no_rotation = dict(rig, q_rl=np.array([0.0, 0.0, 0.0, 1.0]))
    s = pkg.PoseSolver()
    try:
        for name, rg, prob in (("cameras swapped", swapped, w), ("R_rl = I", no_rotation, w), ("right edges as left edges", rig, all_left(w, "stereo"))):
            s.set_rig_kb8(rg)
            r = s.optimize_one(prob)
            dq, dt = float(np.abs(r["q"] - g["ref_q"]).max()), float(np.abs(r["t"] - g["ref_t"]).max())
            print("%s: n_bad %d (reference %d), |dq| %.3g (4 S %.3g), |dt| %.3g (4 S %.3g)" % (name, r["n_bad"], int(g["ref_n_bad"]), dq, 4 * float(g["S_q"]), dt, 4 * float(g["S_t"])))
            assert r["n_bad"] != int(g["ref_n_bad"]) or dq > SOLVER_FACTOR * float(g["S_q"]) or dt > SOLVER_FACTOR * float(g["S_t"]), name
    finally:
        s.close()


def test_argument_checks_leave_the_handle_usable(pkg, solved):
    w, rig, g = pose_fixture(60)
    s = pkg.PoseSolver()
    try:
        s.set_rig_kb8(rig)
        for kind in (1, 3):
            with pytest.raises(pkg.OrbxError) as e:
                s.optimize_one(with_kind(w, "stereo", 7, kind))
            assert e.value.code == ERR_ARG
            same_bits(s.optimize_one(w), solved, BITS)
        bad_fx = dict(rig, right=dict(rig["right"], fx=0.0))
        bad_fy = dict(rig, left=dict(rig["left"], fy=-1.0))
        zero_q = dict(rig, q_rl=np.zeros(4))
        nan_q = dict(rig, q_rl=np.array([np.nan, 0.0, 0.0, 1.0]))
        for bad in (bad_fx, bad_fy, zero_q, nan_q):
            with pytest.raises(pkg.OrbxError) as e:
                s.set_rig_kb8(bad)
            assert e.value.code == ERR_ARG
            same_bits(s.optimize_one(w), solved, BITS)          # the handle's rig is as it was
        with pytest.raises(pkg.OrbxError) as e:                  # rejected before any of the (null) device addresses is read
            s.optimize_batch_device(1, 64, 0, 0, 0, 0, 64, 0, np.ones(8, np.float32), dict(fx=1.0, fy=1.0, cx=0.0, cy=0.0), 0, 0, 0, 0)
        assert e.value.code == ERR_ARG
        same_bits(s.optimize_one(w), solved, BITS)
    finally:
        s.close()


def test_rig_reset_returns_the_pinhole_bits(pkg, synth):
    w = synth.make_pose_problem(3)
    wr, rig, _ = pose_fixture(60)
    fresh, used = pkg.PoseSolver(), pkg.PoseSolver()
    try:
        r0 = fresh.optimize_one(w)
        used.set_rig_kb8(rig)
        used.optimize_one(wr)
        used.set_rig_kb8(None)
        r1 = used.optimize_one(w)
        used.set_rig_kb8(rig)
        used.set_camera_kb8(None)                   # NULL to either setter returns the handle to the pinhole camera
        r2 = used.optimize_one(w)
    finally:
        fresh.close(); used.close()
    same_bits(r1, r0, BITS)
    same_bits(r2, r0, BITS)
