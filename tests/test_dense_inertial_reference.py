"""The CPU oracle's inertial solvers against the dense long-double reference (tests/dense_inertial_reference.py), which restates
the reference's inertial edges, float getters, update rule and first Levenberg trial independently of oracle/.  Every analytic
Jacobian is first checked against long-double central differences of its own residual through the restated update rule, so the
reference cannot share a wrong linearisation with the oracle."""
import numpy as np
import pytest

import dense_ba_reference as D
import dense_inertial_reference as R
from oracle_api import oracle_inertial_solve, oracle_pose_inertial_optimize
from test_pose_inertial_gpu import _check_hessian_blocks

LD = D.LD
H_STEP = LD(1e-6)
JAC_TOL = 1e-10     # relative to the largest entry: 100 x the h^2 truncation term of a central difference at h = 1e-6; rounding eps_ld / h = 1e-13
BRANCH_TOL = 1e-5   # inside a 1e-5 branch the reference drops the first-order term W / 2 of its series: below d / 2 < 5e-6


def _two_frame_state(rs, er=0.1, dbg=0.03, dt=0.25):
    """two key frames and one link with a rotation error of `er` rad and a gyro bias delta of norm `dbg`"""
    unit = lambda: (lambda a: a / np.linalg.norm(a))(rs.normal(0, 1, 3))
    R1 = D.so3_exp(rs.normal(0, 0.4, 3)); dR = D.so3_exp(rs.normal(0, 0.2, 3))
    v1 = rs.normal(0, 0.5, 3); t1 = rs.normal(0, 1, 3)
    bias0 = np.concatenate([rs.normal(0, 0.05, 3), rs.normal(0, 0.01, 3)]).astype(np.float32)
    L = dict(kf1=0, kf2=1, dR=dR.astype(np.float64).astype(np.float32), dV=rs.normal(0, 0.3, 3).astype(np.float32), dP=rs.normal(0, 0.1, 3).astype(np.float32),
             JRg=(-dt * np.eye(3) + rs.normal(0, 0.02, (3, 3))).astype(np.float32), JVg=rs.normal(0, 0.01, (3, 3)).astype(np.float32),
             JVa=rs.normal(0, 0.2, (3, 3)).astype(np.float32), JPg=rs.normal(0, 0.003, (3, 3)).astype(np.float32),
             JPa=rs.normal(0, 0.03, (3, 3)).astype(np.float32), dT=np.float32(dt), bias0=bias0)
    bg = bias0[3:].astype(LD) + LD(dbg) * unit(); ba = bias0[:3].astype(LD) + rs.normal(0, 0.02, 3)
    dRc = R.get_deltas(L, bg, ba, smooth=True)[0]
    R2 = R1 @ dRc @ D.so3_exp(er * unit())                  # eR = dR^T R1^T R2 = Exp(er u)
    s = dict(Rwb=np.stack([R1, R2]), twb=np.stack([np.asarray(t1, LD), np.asarray(t1 + rs.normal(0, 0.2, 3), LD)]),
             vel=np.stack([np.asarray(v1, LD), np.asarray(v1 + rs.normal(0, 0.2, 3), LD)]), bg=np.stack([bg, bg]), ba=np.stack([ba, ba]),
             points=np.zeros((0, 3), LD))
    return L, s


def _perturbed(s, kf, block, d):
    s = R.copy_state(s)
    if block == "pose":
        R.update_pose(s, kf, d)
    else:
        s[block][kf] = s[block][kf] + d
    return s


def _numeric(f, s, kf, block, dim):
    cols = []
    for k in range(dim):
        d = np.zeros(dim, LD); d[k] = H_STEP
        cols.append((f(_perturbed(s, kf, block, d)) - f(_perturbed(s, kf, block, -d))) / (2 * H_STEP))
    return np.stack(cols, -1)


@pytest.mark.parametrize("er,dbg,loose", [(0.3, 0.07, ()), (0.05, 0.01, ()), (0.01, 5e-4, ()), (0.0, 0.0, ()),
                                          (4e-6, 0.03, ((0, 3), (9, 12), (15, 18))),       # |er| < 1e-5: LogSO3 / InverseRightJacobianSO3 branch
                                          (0.1, 2e-5, ((9, 12),))])                         # |JRg dbg| < 1e-5: RightJacobianSO3 branch
def test_edge_inertial_jacobian_against_central_differences(er, dbg, loose):
    """all 24 columns of EdgeInertial::linearizeOplus.  Exempt from 1e-10, and held to 1e-5 instead, are only the rotation rows of the
    column blocks named in `loose`, in the cases that sit inside a 1e-5 branch: there the reference's formula (identity) is not the
    derivative of its residual to first order in the angle, and the solvers must follow the reference."""
    rs = np.random.RandomState(int(1000 * er) + 7)
    L, s = _two_frame_state(rs, er, dbg)
    J = R.inertial_jacobian(L, s, smooth=True)
    f = lambda st: R.inertial_error(L, st, smooth=True)
    N = np.concatenate([_numeric(f, s, 0, "pose", 6), _numeric(f, s, 0, "vel", 3), _numeric(f, s, 0, "bg", 3), _numeric(f, s, 0, "ba", 3),
                        _numeric(f, s, 1, "pose", 6), _numeric(f, s, 1, "vel", 3)], 1)
    scale = float(np.abs(J).max())
    tol = np.full((9, 24), JAC_TOL)
    for a, b in loose:
        tol[0:3, a:b] = BRANCH_TOL
    err = np.abs(J - N).astype(np.float64) / scale
    print("EdgeInertial er %g dbg %g: worst %.3g (strict blocks %.3g)" % (er, dbg, err.max(), err[tol == JAC_TOL].max()))
    assert (err <= tol).all(), np.argwhere(err > tol)
    # the restated (float) getters give the same Jacobian up to the float rounding of dR and dbg
    assert np.abs(R.inertial_jacobian(L, s) - J).max() < 1e-5 * scale


def test_edge_prior_jacobian_against_central_differences():
    rs = np.random.RandomState(11)
    _, s = _two_frame_state(rs)
    pr = dict(prior_Rwb=s["Rwb"][0] @ D.so3_exp(rs.normal(0, 0.1, 3)), prior_twb=s["twb"][0] + rs.normal(0, 0.1, 3), prior_vel=s["vel"][0] + 0.1,
              prior_bg=s["bg"][0] - 0.01, prior_ba=s["ba"][0] + 0.02)
    J = R.prior_jacobian(pr, s)
    f = lambda st: R.prior_error(pr, st)
    N = np.concatenate([_numeric(f, s, 0, "pose", 6), _numeric(f, s, 0, "vel", 3), _numeric(f, s, 0, "bg", 3), _numeric(f, s, 0, "ba", 3)], 1)
    err = float(np.abs(J - N).max() / np.abs(J).max())
    print("EdgePriorPoseImu: %.3g" % err)
    assert err <= JAC_TOL


@pytest.mark.parametrize("stereo", [0, 1])
def test_visual_edges_on_a_body_pose_against_central_differences(stereo):
    """EdgeMono / EdgeStereo (pose and point block; the OnlyPose variants have the same pose block) on an ImuCamPose.  The calibration
    is consistent in long double (Rcb orthonormal, tbc = -Rbc tcb), as the reference's SetParam builds it (G2oTypes.cc:159-163); the
    stereo row uses the exact 1/z of ProjectStereo."""
    rs = np.random.RandomState(20 + stereo)
    Rcb = D.so3_exp(np.array([0.01, -0.02, 0.015])) @ np.array([[0, -1, 0], [0, 0, -1], [1, 0, 0]], LD)
    tcb = np.array([0.02, -0.01, 0.03], LD)
    pr = dict(Rcb=Rcb, tcb=tcb, tbc=-Rcb.T @ tcb, fx=458.654, fy=457.296, cx=367.215, cy=248.375, bf=47.9)
    for _ in range(4):
        _, s = _two_frame_state(rs)
        Rcw, tcw = R.camera_pose(pr, s["Rwb"][0], s["twb"][0])
        X = Rcw.T @ (np.array([rs.uniform(-3, 3), rs.uniform(-2, 2), rs.uniform(2, 12)], LD) - tcw)
        obs = np.array([[300.0, 200.0, 290.0]]); st = np.array([stereo], np.uint8)
        ne = 3 if stereo else 2
        _, _, Ji, Jj = R.visual_terms(pr, s["Rwb"][:1], s["twb"][:1], X[None], obs, st)
        f = lambda state, XX=X: R.visual_terms(pr, state["Rwb"][:1], state["twb"][:1], XX[None], obs, st, jac=False)[0][0]
        Nj = _numeric(f, s, 0, "pose", 6)
        Ni = np.stack([(f(s, X + d) - f(s, X - d)) / (2 * H_STEP) for d in np.eye(3, dtype=LD) * H_STEP], -1)
        scale = float(np.abs(Jj).max())
        ej, ei = float(np.abs(Jj[0] - Nj).max() / scale), float(np.abs(Ji[0] - Ni).max() / np.abs(Ji).max())
        print("visual edge stereo %d: pose %.3g point %.3g" % (stereo, ej, ei))
        assert ej <= JAC_TOL and ei <= JAC_TOL
        assert (Jj[0, ne:] == 0).all() and (Ji[0, ne:] == 0).all()


def _link_window(L, s):
    """the two frames and their link as a LocalInertialBA window without visual edges: key frame 0 fixed, key frame 1 free"""
    f64 = lambda a: np.asarray(a, LD).astype(np.float64)
    L = dict(L, info9=R._spd(np.random.RandomState(1), [2.5e5] * 3 + [1e4] * 3 + [4e4] * 3), info_gyro=np.eye(3) * 4e6, info_acc=np.eye(3) * 4e4, robust=np.uint8(0))
    return dict(n_kf=2, Rwb=f64(s["Rwb"]), twb=f64(s["twb"]), vel=f64(s["vel"]), bg=f64(s["bg"]), ba=f64(s["ba"]), pose_fixed=np.array([1, 0], np.uint8),
                has_imu=np.array([1, 1], np.uint8), imu_fixed=np.array([1, 0], np.uint8), Rcb=np.eye(3), tcb=np.zeros(3), tbc=np.zeros(3),
                fx=458.0, fy=457.0, cx=367.0, cy=248.0, bf=0.0, points=np.zeros((0, 3)), edge_kf=np.zeros(0, np.int32), edge_point=np.zeros(0, np.int32),
                edge_obs=np.zeros((0, 3)), edge_inv_sigma2=np.zeros(0), edge_stereo=np.zeros(0, np.uint8), links=[L], huber_mono=2.0, huber_stereo=2.0,
                huber_inertial=float(np.sqrt(16.92)), lambda_init=1.0, max_iters=1)


def test_float_getters_round_like_the_reference(oracle):
    """restated and smooth getters agree to float rounding; and a crafted link on which the float evaluation in the reference's order
    differs from an evaluation in higher precision rounded once pins the order: the oracle's chi2 of that link agrees with the
    restated getters to 1e-12, while the other rounding moves it by far more"""
    rs = np.random.RandomState(5)
    eps = 2.0 ** -23
    found = None
    for _ in range(40):
        L, s = _two_frame_state(rs, er=0.02, dbg=0.03)
        pr = _link_window(L, s)
        s = R.state_of(pr); L = pr["links"][0]
        dR, dV, dP, dbg = R.get_deltas(L, s["bg"][0], s["ba"][0])
        dRs, dVs, dPs, dbgs = R.get_deltas(L, s["bg"][0], s["ba"][0], smooth=True)
        assert np.abs(dR - dRs).max() < 4 * eps and np.abs(dbg - dbgs).max() < 0.05 * eps
        assert np.abs(dV - dVs).max() < 4 * eps * max(1, np.abs(dVs).max()) and np.abs(dP - dPs).max() < 4 * eps * max(1, np.abs(dPs).max())
        once = lambda a: a.astype(np.float64).astype(np.float32).astype(LD)
        shift = np.concatenate([np.zeros(3, LD), dV - once(dVs), dP - once(dPs)])   # error = ... - dV, ... - dP
        if found is None and (shift != 0).any():
            found = (pr, shift)
    assert found is not None, "no link on which the order of the float operations shows"
    pr, shift = found
    s = R.state_of(pr); L = pr["links"][0]
    Om = np.asarray(L["info9"], LD).reshape(9, 9)
    e = R.inertial_error(L, s)
    c, c_other = e @ Om @ e, (e + shift) @ Om @ (e + shift)
    got = oracle_inertial_solve(oracle, pr)["stats"]["chi2_initial"]
    print("crafted link: chi2 %.17g, oracle %.17g, with the other rounding %.17g" % (float(c), got, float(c_other)))
    assert abs(float(c_other / c) - 1) > 1e-9
    np.testing.assert_allclose(got, float(R.liba_chi2(pr, s)[0]), rtol=1e-12)


@pytest.mark.parametrize("permute", [False, True])
@pytest.mark.parametrize("lam", [1.0, 1e-2])
@pytest.mark.parametrize("n_opt", [1, 4, 5, 9])
def test_oracle_one_trial(oracle, synth, n_opt, lam, permute):
    """hard windows (general JRg, full information matrices, bias deltas of 0.02 with one link at exactly 0, two key frames 0.06 rad
    off), plain and renumbered newest first: trials, chi2_initial, chi2_final, lambda_, the step per block, per-edge chi2 and depth"""
    pr = R.liba_case(synth, n_opt, lam, permute)
    if permute:
        assert all(L["kf1"] > L["kf2"] for L in pr["links"])
    ref = R.liba_first_trial(pr)
    err, ratio = R.check_one_step(pr, oracle_inertial_solve(oracle, pr), ref)
    print("oracle n_opt %d lambda %g permute %d: step error %.3g (%.3g of its tolerance), kappa %.3g, rho %.3f"
          % (n_opt, lam, permute, err, ratio, ref["kappa"], float(ref["rho"])))


@pytest.mark.parametrize("n_opt,lam,permute", [c for c in R.LIBA_DEVICE_CASES if c[0] in (8, 32)])
def test_oracle_one_trial_at_the_device_sizes(oracle, synth, n_opt, lam, permute):
    """the sizes that only the device test needs (120 unknowns, and the 480-unknown limit): the first trial is accepted by reference and
    oracle on the CPU before any device run relies on it"""
    pr, ref = R.first_trial_of(synth, n_opt, lam, permute)
    err, ratio = R.check_one_step(pr, oracle_inertial_solve(oracle, pr), ref)
    print("oracle n_opt %d lambda %g permute %d: step error %.3g (%.3g of its tolerance), kappa %.3g" % (n_opt, lam, permute, err, ratio, ref["kappa"]))


def test_oracle_degenerate_windows(oracle, synth):
    for tag, pr in R.degenerate_windows(synth):
        ref = R.liba_first_trial(pr)
        err, ratio = R.check_one_step(pr, oracle_inertial_solve(oracle, pr), ref)
        print("oracle %s: step error %.3g (%.3g of its tolerance)" % (tag, err, ratio))


def test_hard_window_is_hard(synth):
    """the properties the window is built for: |JRg dbg| >> 1e-5 on most links and exactly 0 on one, |er| >= 0.05 rad on two links'
    key frames, full information matrices, a general JRg"""
    pr = R.liba_case(synth, 9, 1.0, True)
    s = R.state_of(pr)
    w, er = [], []
    for L in pr["links"]:
        dbg = R.get_deltas(L, s["bg"][L["kf1"]], s["ba"][L["kf1"]])[3]
        w.append(float(np.abs(np.asarray(L["JRg"], LD) @ dbg).max()))
        er.append(float(np.sqrt((R.inertial_error(L, s)[:3] ** 2).sum())))
        J = np.asarray(L["JRg"], np.float64)
        assert np.abs(J - J.T).max() > 1e-3 and np.abs(np.asarray(L["info9"])[0, 3:]).min() > 0 and np.abs(L["info_gyro"][0, 1]) > 0
        np.testing.assert_array_equal(L["info9"], L["info9"].T)
    assert sorted(w)[0] == 0 and sorted(w)[1] > 1e-3
    assert sum(e >= 0.05 for e in er) >= 2


def test_permutation_carries_everything_along(synth):
    """the renumbered window is the same problem: same chi2, and the same step for every key frame under its new number"""
    a, b = R.liba_case(synth, 5, 1.0, False), R.liba_case(synth, 5, 1.0, True)
    ra, rb = R.liba_first_trial(a), R.liba_first_trial(b)
    np.testing.assert_allclose(float(ra["chi2_initial"]), float(rb["chi2_initial"]), rtol=1e-15)
    n = 6
    for k in R.BLOCKS:
        for i in range(1, n):
            np.testing.assert_allclose(ra["steps"][k][i].astype(np.float64), rb["steps"][k][n - 1 - i].astype(np.float64), rtol=1e-9, atol=1e-18)


def test_oracle_lambda_update_outside_the_clamp(oracle, synth):
    """rho = 0.897 lies inside (0.85, 0.94), where lambda' = lambda (1 - (2 rho - 1)^3) is not clamped to lambda / 3 or 2 lambda / 3, so
    the + 1e-3 in the scale shows in lambda_.  Found by a search over seeds and perturbations: rotation perturbations of 0.55 rad and
    the Huber kernels switched off (their widths at 1e6).  Unclamped, lambda_ inherits the accuracy of the solved step through rho,
    so its tolerance is unclamped_lambda_rtol (1.5e-10 here; the oracle is off by 5.8e-12), 11 x below what the + 1e-3 moves."""
    pr = R.unclamped_lambda_window(synth)
    ref = R.liba_first_trial(pr)
    assert 0.85 < ref["rho"] < 0.94
    assert 1.0 / 3 + 1e-3 < float(ref["lambda_"]) / pr["lambda_init"] < 2.0 / 3 - 1e-3
    rtol, effect = R.unclamped_lambda_rtol(ref)
    r = oracle_inertial_solve(oracle, pr)
    print("unclamped lambda: rho %.4f, lambda_ off by %.3g, rtol %.3g, the 1e-3 in the scale moves it by %.3g"
          % (float(ref["rho"]), abs(r["stats"]["lambda_"] / float(ref["lambda_"]) - 1), rtol, effect))
    assert effect > 3 * rtol
    R.check_one_step(pr, r, ref, lambda_rtol=rtol)


def test_oracle_robust_link_on_both_sides(oracle, synth):
    for pr, above in R.robust_link_windows(synth):
        ref = R.liba_first_trial(pr)
        c = [float(c) for L, c in zip(pr["links"], ref["link_chi2"]) if L["robust"]]
        assert len(c) == 1 and (c[0] > pr["huber_inertial"] ** 2) == above, c
        R.check_one_step(pr, oracle_inertial_solve(oracle, pr), ref)


def test_pose_problem_hardening_keeps_synth_defaults(synth):
    """the hard frames are made from synth's output afterwards; synth's own defaults still give today's bytes"""
    a, _ = synth.make_pose_inertial_problem(3, n=20)
    R.hard_pose_inertial_problem(synth, 3, 20)
    b, _ = synth.make_pose_inertial_problem(3, n=20)
    for k in ("Rwb", "bg", "ba", "Xw", "obs"):
        np.testing.assert_array_equal(a[k], b[k])
    for k in ("JRg", "info9", "info_gyro"):
        np.testing.assert_array_equal(a["link"][k], b["link"][k])
    assert np.array_equal(a["link"]["JRg"], (-0.05 * np.eye(3)).astype(np.float32)) and np.count_nonzero(a["link"]["info9"]) == 9


@pytest.mark.parametrize("last_frame", [False, True])
@pytest.mark.parametrize("case", range(len(R.POSE_CASES)))
def test_oracle_pose_inertial_hessian_and_stationarity(oracle, synth, case, last_frame):
    """the per-frame solver of the oracle, both variants: flags equal to the planted outliers (valid because no restated chi2 lies
    within 1 % of its threshold), the prior Hessian at the returned state (15 x 15; for the last-frame variant the 30 x 30 before
    Marginalize with the prior edge and the non-diagonal prior_H, at the previous frame's final state, which only the oracle gives),
    the returned state a stationary point of the last round's cost.  The 25-edge case has fewer than 30 inliers, so the recovery pass
    with 18 / 24 runs; its inliers have chi2 << 1 and its outliers chi2 > 50, so the flags cannot tell whether it ran."""
    pr, gt = R.pose_case(synth, case, last_frame)
    r = oracle_pose_inertial_optimize(oracle, pr)
    ratio, bound = R.check_pose_result(pr, gt, r, _check_hessian_blocks, r["prev"] if last_frame else None)
    print("oracle pose case %d %s last_frame %d: Gauss-Newton step / update %.3g (bound %.3g)" % (case, R.POSE_CASES[case], last_frame, ratio, bound))
    assert ratio <= bound
