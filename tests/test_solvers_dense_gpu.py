"""The HIP visual solvers (lba_solve, lba_solve_batch, lba_shard_optimize, pose_optimize_batch) against the dense
long-double reference of tests/dense_ba_reference.py, not against oracle/: one Levenberg trial per window, at sizes around
the factorisation's 60-unknown tiles (NB = 60, 10 free key frames a tile) and on both sides of the fused limit (80 free key
frames = 480 reduced unknowns run k_chol_flow, 81 = 486 take k_chol_diag / k_chol_panel / k_chol_update)."""
import numpy as np
import pytest

import dense_ba_reference as D
from oracle_api import oracle_pose_optimize

pytestmark = pytest.mark.gpu


def _window(synth, n_opt, seed):
    return D.interleaved_window(synth, 500 + seed, n_opt, n_points=12 * (n_opt + max(2, n_opt // 3)), obs=4)


@pytest.mark.parametrize("n_opt", [9, 10, 11, 20, 21, 80, 81])
@pytest.mark.parametrize("lam", [0.0, 30.0])
def test_lba_solve_one_step(pkg, synth, n_opt, lam):
    w = _window(synth, n_opt, n_opt)
    ref = D.lba_first_trial(w, lam)
    s = pkg.LbaSolver()
    try:
        r = s.solve(w, 1, lambda_init=lam)
    finally:
        s.close()
    err = D.check_one_step(w, r, ref)
    print("n_opt %d lambda %g: kernel step error %.3g, kappa %.3g" % (n_opt, lam, err, ref["kappa"]))


def test_lba_solve_lambda_update_and_tau_init(pkg, synth):
    """rho inside the unclamped range of the lambda update, and the largest diagonal of H in a point block"""
    s = pkg.LbaSolver()
    try:
        for w, lam in D.lambda_windows(synth):
            D.check_one_step(w, s.solve(w, 1, lambda_init=lam), D.lba_first_trial(w, lam))
    finally:
        s.close()


def test_lba_batch_and_shard_one_step(pkg, synth):
    ws = [_window(synth, n, 40 + n) for n in (9, 11, 21)]
    refs = [D.lba_first_trial(w, 0.0) for w in ws]
    b = pkg.LbaBatch()
    try:
        got = b.solve(ws, 1)
    finally:
        b.close()
    for w, r, ref in zip(ws, got, refs):
        D.check_one_step(w, r, ref)
    for w, ref in zip(ws[:2], refs[:2]):
        sh = pkg.LbaShard(w)
        try:
            st = sh.optimize(None, 1, max_iters=1)
            out = sh.download()
        finally:
            sh.close()
        out = dict(out, stats=st)
        D.check_one_step(w, out, ref)


def test_lba_ill_conditioned_windows(pkg, oracle, synth):
    """far points (50-200 m) on a 0.3 m baseline, one free key frame with 5 observations, a small user lambda: the kernel must
    be at least as accurate as the plain f64 solve of the oracle, both measured against the refined long-double solve"""
    s = pkg.LbaSolver()
    try:
        for seed, n_opt, lam in ((0, 10, 1e-3), (1, 10, 1e-3), (2, 21, 1e-4), (3, 81, 1e-3)):
            w = D.make_far_window(seed, n_opt=n_opt, n_fixed=2, n_points=15 * n_opt, obs_per_point=5, stereo_frac=0.2)
            ref = D.lba_first_trial(w, lam)
            r0 = oracle.lba_solve(w, 1, lambda_init=lam)
            r1 = s.solve(w, 1, lambda_init=lam)
            assert r1["stats"]["trials"] == 1 and r0["stats"]["trials"] == 1
            e0, e1 = D.lba_step_error(w, r0, ref), D.lba_step_error(w, r1, ref)
            print("ill-conditioned n_opt %d lambda %g: kappa %.3g, oracle error %.3g, kernel error %.3g" % (n_opt, lam, ref["kappa"], e0, e1))
            assert ref["kappa"] > 1e6
            assert e1 <= 10 * e0 + 1e-12, "kernel %.3g vs oracle %.3g" % (e1, e0)
    finally:
        s.close()


def test_pose_optimize_batch_is_stationary(pkg, oracle, synth):
    """mono frames, a stereo share, a frame of 1000 edges: the outlier flags equal the planted outliers, and the returned pose is a
    stationary point of the last round's cost (no robust kernel, active set = inliers).  A 1000-edge frame with a stereo share
    is left out: at 0.05 px noise its cost is flat at the float 1/z rounding and Levenberg stops on that plateau (oracle too)."""
    ws = [synth.make_pose_problem(300 + i, n=n, outlier_frac=0.1, stereo_frac=sf, noise_px=0.05)
          for i, (n, sf) in enumerate([(200, 0.0), (200, 0.0), (200, 0.4), (200, 1.0), (1000, 0.0)])]
    s = pkg.PoseSolver()
    try:
        got = s.optimize_batch(ws)
    finally:
        s.close()
    for w, r in zip(ws, got):
        np.testing.assert_array_equal(r["outlier"].astype(bool), w["is_outlier"])
        ratio, bound, kappa = D.pose_stationarity(w, r)
        ratio0, _, _ = D.pose_stationarity(w, oracle_pose_optimize(oracle, w))
        print("pose n %d stereo %.1f: Newton step / update %.3g (oracle %.3g, bound %.3g), kappa %.3g"
              % (len(w["Xw"]), w["stereo"].mean(), ratio, ratio0, bound, kappa))
        assert ratio <= bound
        # where the float 1/z plateau sets the bound, the kernel must also stop no farther out than the f64 oracle
        assert ratio <= 10 * ratio0 + 1e-9
        # per-edge chi2 classification of the returned pose, restated in float against the float thresholds
        chi2 = D.pose_chi2(w, r["q"], r["t"]).astype(np.float64).astype(np.float32)
        th = np.where(w["stereo"].astype(bool), np.float32(D.CHI2_STEREO), np.float32(D.CHI2_MONO))
        np.testing.assert_array_equal(chi2 > th, w["is_outlier"])
