"""The numpy KannalaBrandt8 reference (tests/kb8_reference.py) against itself: projectJac against central differences of the smooth
projection, project against a long-double evaluation within the one-ulp bound, and the committed fixtures against the generator's
rules.  CPU only."""
import importlib
import os

import numpy as np

import kb8_reference as kr
from dense_ba_reference import LD
from kb8_cases import lba_fixture, pose_fixture


def _scene():
    sk = importlib.import_module("orb_slam3-1_amd.synth_kb8")
    return sk.tumvi_camera(), sk.make_camera_points(0, 4096)


def test_project_jac_matches_central_differences():
    cam, X = _scene()
    J = kr.project_jac(cam, X)
    num = np.zeros_like(J)
    for a in range(3):
        h = 1e-6 * np.abs(X).max(1)
        d = np.zeros_like(X); d[:, a] = h
        num[:, :, a] = ((kr.project_smooth(cam, X.astype(LD) + d, LD) - kr.project_smooth(cam, X.astype(LD) - d, LD)) / (2 * h[:, None])).astype(np.float64)
    # central differences with a relative step of 1e-6: truncation ~1e-12 of the derivative's scale, long-double rounding far below
    scale = np.abs(J).max((1, 2), keepdims=True)
    assert (np.abs(J - num) <= 1e-8 * scale).all(), float((np.abs(J - num) / scale).max())


def test_project_is_within_one_ulp_of_correctly_rounded_arctangents():
    """The tolerances of the GPU tests rest on: the host's theta and psi (libm's atan2f) and the device's (the correctly rounded
    float arctangent) differ by at most one float ulp.  Checked here against a long-double evaluation whose arctangents are rounded
    to float, with the bound of the device test.
    Not checked, because it does not hold: libm's atan2f within one ulp of the UNROUNDED value.  glibc 2.35 is up to 1.37 ulp
    (theta) and 1.14 ulp (psi) off on 11 of these 8192 arguments (printed below); its distance from the correctly rounded
    value is nevertheless exactly one ulp at most, which is the statement the tolerances need."""
    cam, X = _scene()
    exact = kr.project_exact_arctangents(cam, X).astype(np.float64)
    err = np.abs(kr.project(cam, X) - exact)
    bound = kr.project_bound(cam, X)
    raw = np.abs(kr.project(cam, X) - kr.project_exact_arctangents(cam, X, round_to_float=False).astype(np.float64))
    print("largest |project - exact| / bound: %.3f with the arctangents rounded to float, %.3f unrounded" % (float((err / bound).max()), float((raw / bound).max())))
    assert (err <= bound).all()
    # against the unrounded arctangents: 1.5 ulp, the correctly rounded value's half ulp plus libm's one from it (measured 1.37 with
    # glibc 2.35, 1.08 of the bound in pixels); a libm that drifts further fails here
    assert (raw <= 1.5 * bound).all()
    # and the perturbed switch moves theta and psi by exactly one float ulp
    th0, ps0 = kr.theta_psi(X)
    th1, ps1 = kr.theta_psi(X, np.random.RandomState(3))
    assert (np.abs(th1 - th0) <= kr.ulp32(th0) * 1.0000001).all() and (th1 != th0).all() and (ps1 != ps0).all()


def test_fixtures_are_what_the_generator_promises():
    w, cam, g = pose_fixture()
    assert len(w["Xw"]) == 60 and int(g["ref_n_bad"]) == 9 and not w["stereo"].any() and float(g["max_off_axis_deg"]) > 75
    r = kr.pose_optimize(w, cam)            # this host's libm need not be the generator's: within S, not bit for bit
    np.testing.assert_array_equal(r["outlier"], g["ref_outlier"])
    assert np.abs(r["q"] - g["ref_q"]).max() <= float(g["S_q"]) and np.abs(r["t"] - g["ref_t"]).max() <= float(g["S_t"])
    assert r["margins"].min() >= 1e-3
    d = kr.pose_optimize(w, cam, device_model=True)      # libm plays no part in the device model
    assert d["iterations"] == g["dev_iterations"].tolist() and d["trials"] == g["dev_trials"].tolist()
    assert (g["count_runs"] != g["count_runs"][0]).any()    # why the counts are not pinned against the host reference
    wl, caml, gl = lba_fixture()
    assert int(wl["pose_fixed"].sum()) == 2 and len(wl["pose_q"]) == 4 and len(wl["points"]) == 40 and 120 <= len(wl["edge_point"]) <= 140
    assert int(gl["is_outlier"].sum()) == 6 and (gl["count_runs"] == gl["count_runs"][0]).all()
    assert (np.abs(gl["ref_chi2"] - 5.991) / 5.991).min() >= 1e-3
