"""The CPU oracle's visual solvers against the dense long-double reference (tests/dense_ba_reference.py), which restates
the reference's edges, robust kernel and first Levenberg trial independently of oracle/.  Every analytic Jacobian is first
checked against central differences of its own residual, so the reference cannot share a wrong linearisation with the
oracle."""
import numpy as np
import pytest

import dense_ba_reference as D
from oracle_api import oracle_pose_optimize

LD = D.LD
JAC_TOL = 1e-7      # central differences in long double with h = 1e-7: truncation ~h^2, rounding ~eps_ld / h, both << 1e-9


def _cam():
    return dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, bf=47.906)


def _numeric(f, x0, h=LD(1e-7)):
    x0 = np.asarray(x0, LD)
    cols = []
    for k in range(len(x0)):
        d = np.zeros(len(x0), LD); d[k] = h
        cols.append((f(x0 + d) - f(x0 - d)) / (2 * h))
    return np.stack(cols, -1)


def _rel(a, b):
    return float(np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum()))


def test_reference_works_in_long_double():
    assert np.finfo(LD).eps < 1e-18
    x, _, _ = D.solve_refined(np.array([[4.0, 1.0], [1.0, 3.0]]), np.array([1.0, 2.0]))
    assert abs(float(x[0] - LD(1) / 11)) < 1e-18 and abs(float(x[1] - LD(7) / 11)) < 1e-18


@pytest.mark.parametrize("stereo", [0, 1])
def test_projection_jacobians_against_central_differences(stereo):
    """EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ (point and pose blocks) and the OnlyPose variants (pose block), each at
    several points.  The stereo residual rounds 1/z to float, which makes its difference quotient noise: the check uses the
    same residual with an exact 1/z, whose derivative the reference's formula is."""
    rs = np.random.RandomState(3 + stereo)
    cam = _cam()
    for _ in range(6):
        R = D.so3_exp(rs.normal(0, 0.3, 3)); t = np.asarray(rs.normal(0, 0.5, 3), LD)
        X = np.asarray([rs.uniform(-3, 3), rs.uniform(-2, 2), rs.uniform(2, 12)], LD)
        X = R.T @ (X - t)                                   # world point in front of the camera
        obs = np.array([[300.0, 200.0, 290.0]])
        st = np.array([stereo], np.uint8)

        def res(Rr, tt, XX, float_bf):
            return D.project_residual((Rr @ XX + tt)[None], obs, st, cam, float_invz=False, float_bf=float_bf)[0]
        Jp, Jx = D.project_jacobians((R @ X + t)[None], R[None], st, cam)
        Jp, Jx = Jp[0], Jx[0]
        Np = _numeric(lambda XX: res(R, t, XX, True), X)

        def pose_res(u):
            dR, dt = D.se3_exp(u)
            return res(dR @ R, dR @ t + dt, X, True)
        Nx = _numeric(pose_res, np.zeros(6))
        rows = 2 + stereo
        assert _rel(Jp[:rows], Np[:rows]) < JAC_TOL
        assert _rel(Jx[:rows], Nx[:rows]) < JAC_TOL
        assert not Jp[rows:].any() and not Jx[rows:].any()


def test_stereo_residual_rounds_like_the_reference():
    """types_six_dof_expmap.cpp:190-195: invz = 1.0f/z is a float; the binary edge's bf is a const float&, so bf*invz is a float
    product; the OnlyPose edge keeps a double bf (types_six_dof_expmap.h:235)"""
    Xc = np.array([[1.3, -0.7, 7.77]], LD)
    obs = np.zeros((1, 3)); st = np.ones(1, np.uint8)
    cam = _cam()
    invz32 = np.float32(1.0 / 7.77)
    r = D.project_residual(Xc, obs, st, cam)[0]
    assert r[0] == -(LD(1.3) * LD(invz32) * LD(cam["fx"]) + LD(cam["cx"]))
    assert r[2] == -(-r[0] - LD(np.float32(np.float32(cam["bf"]) * invz32)))
    r2 = D.project_residual(Xc, obs, st, cam, float_bf=False)[0]
    assert r2[2] == -(-r2[0] - LD(cam["bf"]) * LD(invz32))


@pytest.mark.parametrize("lam", [0.0, 30.0])
def test_oracle_lba_one_step_against_reference(oracle, synth, lam):
    """LocalBA, one Levenberg trial: mono + 30 % stereo, Huber active on >= 3 % of the edges, fixed key frames interleaved;
    lambda from the user and from 1e-5 * max diag H"""
    w = D.interleaved_window(synth, 41, 9)
    ref = D.lba_first_trial(w, lam)
    st = w["edge_stereo"].astype(bool)
    _, chi2 = D.lba_robust_chi2(w, *D._window_state(w))
    huber_on = np.where(st, chi2 > w["huber_stereo"] ** 2, chi2 > w["huber_mono"] ** 2)
    assert huber_on.mean() >= 0.03 and st.mean() > 0.2 and w["pose_fixed"][:-1].any()
    r = oracle.lba_solve(w, 1, lambda_init=lam)
    D.check_one_step(w, r, ref)
    if lam > 0:
        assert float(ref["lambda_init"]) == lam


def test_oracle_lba_lambda_update_and_tau_init(oracle, synth):
    (wa, la), (wb, lb) = D.lambda_windows(synth)
    ra = D.lba_first_trial(wa, la)
    assert 0.85 < ra["rho"] < 0.94 and 1 / 3 < ra["lambda_"] / ra["lambda_init"] < 2 / 3
    D.check_one_step(wa, oracle.lba_solve(wa, 1, lambda_init=la), ra)
    rb = D.lba_first_trial(wb, lb)
    assert rb["max_diag_point"] > 10 * rb["max_diag_pose"]
    assert abs(float(rb["lambda_init"]) / (1e-5 * rb["max_diag_point"]) - 1) < 1e-15
    D.check_one_step(wb, oracle.lba_solve(wb, 1, lambda_init=lb), rb)


def test_oracle_lba_ill_conditioned_against_reference(oracle):
    """far points on a short baseline, one free key frame with 5 observations: the oracle's plain f64 LDL^T stays within
    100 kappa eps of the refined solve"""
    for seed in range(2):
        w = D.make_far_window(seed, n_opt=10, n_fixed=2, n_points=150, obs_per_point=5)
        ref = D.lba_first_trial(w, 1e-3)
        assert ref["kappa"] > 1e6
        r = oracle.lba_solve(w, 1, lambda_init=1e-3)
        D.check_one_step(w, r, ref)


@pytest.mark.parametrize("seed,sf", [(0, 0.0), (1, 0.0), (2, 0.4), (3, 1.0)])
def test_oracle_pose_optimization_is_stationary(oracle, synth, seed, sf):
    """PoseOptimization: low noise, well separated gross outliers, so the final round's active set is known; at the returned
    pose the Newton step of the restated cost (no robust kernel) is at most 1e-9 of the total update"""
    w = synth.make_pose_problem(300 + seed, n=200, outlier_frac=0.1, stereo_frac=sf, noise_px=0.05)
    r = oracle_pose_optimize(oracle, w)
    np.testing.assert_array_equal(r["outlier"].astype(bool), w["is_outlier"])
    ratio, bound, _ = D.pose_stationarity(w, r)
    assert ratio <= bound, "Newton step / update %.3g > %.3g" % (ratio, bound)


def test_pose_problem_noise_keyword_keeps_default(synth):
    a = synth.make_pose_problem(7, n=50, outlier_frac=0.1, stereo_frac=0.5)
    b = synth.make_pose_problem(7, n=50, outlier_frac=0.1, stereo_frac=0.5, noise_px=1.0)
    for k in ("q", "t", "Xw", "obs", "inv_sigma2", "stereo"):
        np.testing.assert_array_equal(a[k], b[k])
    c = synth.make_pose_problem(7, n=50, outlier_frac=0.1, stereo_frac=0.5, noise_px=0.0)
    assert not np.array_equal(a["obs"], c["obs"]) and np.array_equal(a["Xw"], c["Xw"])
