"""The HIP inertial solvers (liba_solve, liba_solve_batch, liba_pose_optimize_batch) against the dense long-double reference of
tests/dense_inertial_reference.py, not against oracle/: one Levenberg trial per window on hard windows (general JRg, full
information matrices, bias deltas, large rotation errors, key frames numbered newest first) at sizes around the factorisation's
60-row tiles and at its 480-unknown limit, and the per-frame solver's flags, prior Hessian and stationarity in both variants."""
import numpy as np
import pytest

import dense_inertial_reference as R
from oracle_api import oracle_pose_inertial_optimize
from test_pose_inertial_gpu import _check_hessian_blocks

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def solver(pkg):
    s = pkg.InertialSolver()
    yield s
    s.close()


@pytest.mark.parametrize("n_opt,lam,permute", R.LIBA_DEVICE_CASES)
def test_liba_solve_one_step(solver, synth, n_opt, lam, permute):
    pr, ref = R.first_trial_of(synth, n_opt, lam, permute)
    err, ratio = R.check_one_step(pr, solver.solve(pr), ref)
    print("n_opt %d lambda %g permute %d: kernel step error %.3g (%.3g of its tolerance), kappa %.3g, %d unknowns"
          % (n_opt, lam, permute, err, ratio, ref["kappa"], ref["n_unknowns"]))


def test_liba_solve_batch_one_step(pkg, synth):
    """windows of 1, 5 and 9 free key frames in one call, each against the reference (not against liba_solve)"""
    cases = [R.first_trial_of(synth, n, 1.0, bool(n % 2)) for n in (1, 5, 9)]
    b = pkg.LibaBatch()
    try:
        got = b.solve([pr for pr, _ in cases])
    finally:
        b.close()
    for (pr, ref), r in zip(cases, got):
        err, ratio = R.check_one_step(pr, r, ref)
        print("batch %d unknowns: kernel step error %.3g (%.3g of its tolerance)" % (ref["n_unknowns"], err, ratio))


def test_liba_solve_capacity(pkg, synth):
    """33 free key frames = 495 reduced unknowns = 9 tiles: refused on the host with ORBX_ERR_CAPACITY, and the handle stays good"""
    big = R.liba_case(synth, 33, 1.0, False)
    s = pkg.InertialSolver()
    try:
        with pytest.raises(pkg.OrbxError) as e:
            s.solve(big)
        assert e.value.code == pkg.capi.ORBX_ERR_CAPACITY
        pr, ref = R.first_trial_of(synth, 4, 1.0, False)
        R.check_one_step(pr, s.solve(pr), ref)
    finally:
        s.close()


def test_liba_solve_robust_link_on_both_sides(solver, synth):
    for pr, above in R.robust_link_windows(synth):
        ref = R.liba_first_trial(pr)
        c = [float(c) for L, c in zip(pr["links"], ref["link_chi2"]) if L["robust"]]
        assert len(c) == 1 and (c[0] > pr["huber_inertial"] ** 2) == above, c
        err, ratio = R.check_one_step(pr, solver.solve(pr), ref)
        print("robust link chi2 %.3g (huber^2 %.3g): kernel step error %.3g (%.3g of its tolerance)" % (c[0], pr["huber_inertial"] ** 2, err, ratio))


def test_liba_solve_unclamped_lambda(solver, synth):
    pr = R.unclamped_lambda_window(synth)
    ref = R.liba_first_trial(pr)
    rtol, effect = R.unclamped_lambda_rtol(ref)
    assert 0.85 < ref["rho"] < 0.94 and effect > 3 * rtol
    r = solver.solve(pr)
    print("unclamped lambda: rho %.4f, kernel lambda_ off by %.3g (rtol %.3g)" % (float(ref["rho"]), abs(r["stats"]["lambda_"] / float(ref["lambda_"]) - 1), rtol))
    R.check_one_step(pr, r, ref, lambda_rtol=rtol)


def test_liba_solve_degenerate_windows(solver, synth):
    for tag, pr in R.degenerate_windows(synth):
        ref = R.liba_first_trial(pr)
        err, ratio = R.check_one_step(pr, solver.solve(pr), ref)
        print("%s: kernel step error %.3g (%.3g of its tolerance), kappa %.3g" % (tag, err, ratio, ref["kappa"]))


def _worst_block(H, Hk):
    N = H.shape[0]
    return max(np.abs(H[a:a + 3, b:b + 3] - Hk[a:a + 3, b:b + 3]).max() / np.abs(H[a:a + 3, b:b + 3]).max()
               for a in range(0, N, 3) for b in range(0, N, 3) if np.abs(H[a:a + 3, b:b + 3]).max() > 0)


@pytest.mark.parametrize("last_frame", [False, True])
def test_liba_pose_optimize_batch_against_reference(solver, oracle, synth, last_frame):
    """both variants: 200 mono, 0.4 stereo, all stereo, 25 edges (fewer than 30 inliers, so the recovery pass with 18 / 24 runs; its
    inliers have chi2 << 1 and its outliers chi2 > 50, so the flags cannot tell whether it ran), none, rec_init = 1; 0.05 px noise,
    outliers of 15 px and more, a general JRg, full information matrices and a bias delta on the link, synth's non-diagonal prior_H.
    Flags equal to the planted outliers, H per 3 x 3 block against the long-double value at the returned state, the state stationary
    within the bound of pose_inertial_stationarity and never 10 x farther out than the oracle.  The last-frame variant's 30 x 30 is
    linearised at the previous frame's final state as well, which the ABI does not return: the oracle's is used (the oracle's own H
    and stationarity at that state are checked on the CPU)."""
    cases = [R.pose_case(synth, i, last_frame) for i in range(len(R.POSE_CASES))]
    got = solver.pose_optimize_batch([pr for pr, _ in cases])
    for i, ((pr, gt), r) in enumerate(zip(cases, got)):
        r0 = oracle_pose_inertial_optimize(oracle, pr)
        prev = r0["prev"] if last_frame else None
        ratio, bound = R.check_pose_result(pr, gt, r, _check_hessian_blocks, prev)
        ratio0 = R.pose_inertial_stationarity(pr, r0, prev)[0]
        herr = _worst_block(R.pose_inertial_hessian(pr, r, r["outlier"], prev).astype(np.float64), r["H"])
        print("pose case %d %s last_frame %d: Gauss-Newton step / update %.3g (oracle %.3g, bound %.3g), worst H block %.3g"
              % (i, R.POSE_CASES[i], last_frame, ratio, ratio0, bound, herr))
        assert ratio <= bound and ratio <= 10 * ratio0 + 1e-9
