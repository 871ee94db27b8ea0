"""The dense reference of FullInertialBA (tests/fullba_reference.py) checked on its own, and every number the device is held to in
tests/test_fullba_gpu.py, each next to the assertion that keeps it honest.  No GPU.

  - a link's Jacobian with respect to the shared bias is the derivative of its error (long-double difference quotients, smooth getters);
  - without a shared bias first_trial is liba_first_trial on the same window with every link robust, to the last bit;
  - SPREAD_FIXED / SPREAD_FREE: the largest pairwise deviation between the float64 run, the float64 run with the unknowns reversed
    and the long double run of optimize over the full-run cases; the device gets four times these;
  - case quality: on every one-trial case the tolerance check_one_step applies to a block is at most 1e-6 of the block's step:
    step_tolerance(kappa) is, and the float-getter floors (3e-4 of the smallest blocks' steps) are capped there, since the device
    reproduces the getters' floats (chi2_initial agrees to 1e-15) -- except the gauge-free cases at lambda 1e-5, whose condition number lambda sets.  Those are judged by
    the backward error of the step in the long-double system, against four times what the float64 reference's own step leaves
    (BACKWARD_F64);
  - the two readings of the prior edges' sign, one trial apart (printed; run with -s)."""
import numpy as np
import pytest

import dense_inertial_reference as R
import fullba_cases as C
import fullba_reference as F
from dense_ba_reference import step_tolerance

LD = np.longdouble
# recorded (CPU, numpy), rounded up to two digits: absolute per output block, relative for the final chi2.
# Gauge fixed (s12, k6; Levenberg stops on the relative-gain rule after 5 and 7 iterations, and the three runs end within a few ulps of each other):
SPREAD_FIXED = dict(Rwb=4.5e-16, twb=3.2e-15, vel=2.2e-15, bg=3.5e-15, ba=4.3e-17, points=2.5e-13, chi2=1.1e-14)
# Gauge free (s6, k12), on what the gauge leaves alone (fullba_reference.gauge_invariants).  The runs stop on the 1e-3 relative-gain
# rule after 7 iterations (9 and 10 trials), or, from the hard start of the max_iters = 7 cases, are cut by the limit (8 and 9 trials; the
# chi2 figure is theirs), while the estimate still drifts along the four free directions, whose curvature is lambda.
# ba is the least observable block without a prior (k12: 9.0e-7).
SPREAD_FREE = dict(bg=1.5e-8, ba=9.1e-7, rel_R=2.9e-8, rel_t=2.0e-7, body_v=2.0e-7, z=2.4e-7, chi2=5.1e-7)
# the backward error |(H + lambda I) x - b| / |b| that the float64 first_trial's own step, recovered from its output state, leaves in the
# long-double system of the gauge-free one-trial cases at lambda 1e-5 (kappa 8e10, 2.6e11, 1.9e12)
BACKWARD_F64 = dict(s2=1.3e-8, s7=3.8e-8, k5=1.4e-7)
QUALITY = F.QUALITY     # 1e-6


def _flow(r):
    s = r["stats"]
    return (s["iterations"], s["trials"], s["stop_reason"])


@pytest.fixture(scope="module")
def runs():
    """the three reference runs of every full-run case, computed once"""
    out = {}
    for name in C.FULL:
        pr = C.full_problem(name)
        out[name] = (pr, [F.optimize(pr, np.float64), F.optimize(pr, np.float64, reverse=True), F.optimize(pr, LD)])
    return out


def test_shared_bias_jacobian_is_the_derivative(synth):
    """every link of a shared-bias map: columns G1 / A1 of EdgeInertial's Jacobian against central differences of the error with
    the ONE bias moved in every key frame at once, as the solver moves it.  The stored dR is a float matrix, orthogonal to 6e-8 only,
    which is what the comparison is left with (1.4e-8); a wrong or missing block would show as O(1)."""
    pr = C.one_trial_problem(synth, "s7", 1.0)
    s = F.initial_state(pr)
    imu = np.asarray(pr["has_imu"]) != 0
    h = LD(1e-7)
    worst = 0.0
    for L in pr["links"]:
        J = R.inertial_jacobian(L, s, smooth=True)[:, 9:15]
        for c in range(6):
            key, a = ("bg", c) if c < 3 else ("ba", c - 3)
            plus, minus = R.copy_state(s), R.copy_state(s)
            plus[key][imu, a] += h; minus[key][imu, a] -= h
            q = (R.inertial_error(L, plus, smooth=True) - R.inertial_error(L, minus, smooth=True)) / (2 * h)
            worst = max(worst, float(np.abs(q - J[:, c]).max() / max(1.0, float(np.abs(J[:, c]).max()))))
    print("shared-bias Jacobian columns against difference quotients: worst %.3g" % worst)
    assert worst < 1e-6


def test_first_trial_is_liba_first_trial_without_a_shared_bias(synth):
    """a window all of whose points have a free observer, every link robust: the same bits as dense_inertial_reference.liba_first_trial"""
    w = R.hard_inertial_window(synth, 405, 5)
    pr = C.synth_fullba().full_map_from_window(w, 0, gauge_free=False, lambda_init=1.0, max_iters=1)
    assert F.active_sets(pr)["keep_pt"].all()
    a, b = F.first_trial(pr), R.liba_first_trial(pr)
    for k in ("chi2_initial", "chi2_final", "rho", "lambda_"):
        assert a[k] == b[k], k
    for k in b["state"]:
        assert np.array_equal(a["state"][k], b["state"][k]), k
    assert np.array_equal(a["point_step"], b["point_step"])


def test_dropped_unknowns_do_not_move(synth):
    """the IMU states of a key frame in no link, and a point seen only by fixed key frames, are no unknowns of the reference"""
    pr = C.one_trial_problem(synth, "k4", 1.0)
    lone = int(np.nonzero(np.asarray(pr["pose_fixed"]))[0][0])            # the fixed key frame: its link goes, its IMU states are set free
    pr["links"] = [L for L in pr["links"] if lone not in (int(L["kf1"]), int(L["kf2"]))]
    assert len(pr["links"]) == 3
    pr["imu_fixed"] = np.zeros_like(pr["imu_fixed"])
    pr["points"] = np.vstack([pr["points"], pr["points"][:1] + 0.1])
    e = int(np.nonzero(pr["edge_kf"] == lone)[0][0])
    for k in ("edge_kf", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo"):
        pr[k] = np.concatenate([pr[k], pr[k][e:e + 1]])
    pr["edge_point"][-1] = len(pr["points"]) - 1
    ref = F.first_trial(pr)
    assert not ref["act"]["imu_free"][lone] and not ref["act"]["keep_pt"][-1]
    for k in ("vel", "bg", "ba"):
        assert np.array_equal(ref["state"][k][lone], np.asarray(pr[k][lone], LD))
    assert np.array_equal(ref["state"]["points"][-1], np.asarray(pr["points"][-1], LD))


def test_spread_of_the_three_runs(runs):
    sp = dict(fixed={k: 0.0 for k in SPREAD_FIXED}, free={k: 0.0 for k in SPREAD_FREE})
    for name, (pr, rs) in runs.items():
        free = C.FULL[name]["gauge_free"]
        d = sp["free" if free else "fixed"]
        bl = [F.full_run_blocks(pr, r, free) for r in rs]
        for i in range(3):
            for j in range(i + 1, 3):
                for k in bl[0]:
                    d[k] = max(d[k], float(np.abs(bl[i][k] - bl[j][k]).max()))
                d["chi2"] = max(d["chi2"], float(abs(rs[i]["chi2_final"] - rs[j]["chi2_final"]) / abs(rs[j]["chi2_final"])))
        print("%-8s flows %s chi2 %.6g -> %.6g" % (name, [_flow(r) for r in rs], float(rs[0]["chi2_initial"]), float(rs[0]["chi2_final"])))
    print("gauge fixed: measured %s\n             recorded %s" % ({k: "%.3g" % v for k, v in sp["fixed"].items()}, SPREAD_FIXED))
    print("gauge free:  measured %s\n             recorded %s" % ({k: "%.3g" % v for k, v in sp["free"].items()}, SPREAD_FREE))
    for k, v in sp["fixed"].items():
        assert v <= SPREAD_FIXED[k], ("fixed", k, v)
    for k, v in sp["free"].items():
        assert v <= SPREAD_FREE[k], ("free", k, v)


def test_the_three_runs_agree_on_the_flow(runs):
    """iterations, trials and stop reason: the GPU test asserts them wherever these agree, which is every case"""
    for name, (_, rs) in runs.items():
        assert _flow(rs[0]) == _flow(rs[1]) == _flow(rs[2]), name
        assert rs[0]["chi2_final"] < rs[0]["chi2_initial"]


def test_full_runs_are_worth_running(runs):
    """every run takes more than three iterations, so that the re-orthonormalisation of Rwb on every third update of a pose takes part;
    the gauge-free ones reject trials; the two gauge-free runs at max_iters = 7 are cut by the iteration limit (stop reason 0), all others
    stop on the relative-gain rule"""
    flows = {name: _flow(rs[0]) for name, (_, rs) in runs.items()}
    for name, f in flows.items():
        c = C.FULL[name]
        cut = c["gauge_free"] and c["max_iters"] == 7
        assert f[0] >= 5 and f[2] == (0 if cut else 2) and (f[0] == 7 or not cut), (name, f)
        assert f[1] > f[0] or not c["gauge_free"], (name, f)


@pytest.mark.parametrize("name,lam", C.ONE_TRIAL_IDS)
def test_case_quality(synth, name, lam):
    pr, ref = C.one_trial_of(synth, name, lam)
    c = C.ONE_TRIAL[name]
    assert ref["n_unknowns"] == C.UNKNOWNS[name] and ref["rho"] > 0 and ref["resid"] < 1e-15
    tol = step_tolerance(ref["kappa"])
    worst, uncapped, _ = F.block_tolerances(pr, ref)
    print("%s lambda %g: %d unknowns, kappa %.3g, step tolerance %.3g; the largest tolerance a block is granted %.3g of its step (%.3g before the cap)"
          % (name, lam, ref["n_unknowns"], ref["kappa"], tol, worst, uncapped))
    if tol <= QUALITY:
        assert name not in BACKWARD_F64 or lam != 1e-5
        assert worst <= QUALITY        # what check_one_step applies: the float-getter floors never widen a block beyond 1e-6 of its step
        return
    assert c["gauge_free"] and lam == 1e-5 and name in BACKWARD_F64, "an ill-conditioned case that is not a gauge-free one at lambda 1e-5"
    r64 = F.first_trial(pr, np.float64)
    be = F.backward_error(pr, {k: np.asarray(v, np.float64) for k, v in r64["state"].items()}, ref)
    print("    backward error of the float64 reference's step %.3g (recorded %.3g)" % (be, BACKWARD_F64[name]))
    assert be <= BACKWARD_F64[name]


def test_one_trial_cases_have_links_on_both_sides_of_the_huber_threshold(synth):
    below = above = 0
    for name in C.ONE_TRIAL:
        pr, ref = C.one_trial_of(synth, name, 1.0)
        c = np.asarray(ref["link_chi2"], np.float64)
        below += int((c < pr["huber_inertial"] ** 2).sum()); above += int((c > pr["huber_inertial"] ** 2).sum())
        assert (c > pr["huber_inertial"] ** 2).any() or name == "s2", name
    assert below >= len(C.ONE_TRIAL) - 1 and above > 0, (below, above)


def test_prior_sign_report():
    """EdgePriorAcc / EdgePriorGyro as the solvers read them (estimate - prior) and as written (prior - estimate with +I): one trial on
    the golden shared-bias map, the bias steps and the trial's chi2 side by side.  A report: only the shape of the difference is asserted
    (the readings share H and chi2_initial and differ in the gradient of the 6 shared rows)."""
    pr = dict(C.full_problem("s12_100"), max_iters=1)
    a, b = F.first_trial(pr), F.first_trial(pr, as_written=True)
    kb = int(pr["links"][0]["kf1"])
    nrm = lambda v: float(np.sqrt((v * v).sum()))
    print("prior sign, one trial at lambda %g, priors %g / %g on a bias of |bg| %.3g |ba| %.3g:" % (pr["lambda_init"], pr["prior_g"], pr["prior_a"],
                                                                                                  nrm(np.asarray(pr["shared_bg"])), nrm(np.asarray(pr["shared_ba"]))))
    for key in ("bg", "ba"):
        sa, sb = a["steps"][key][kb], b["steps"][key][kb]
        print("    %s step: estimate - prior %s   as written %s   |difference| / |step| %.3g" % (key, np.asarray(sa, np.float64), np.asarray(sb, np.float64), nrm(sa - sb) / nrm(sa)))
    print("    chi2 after the trial: %.9g against %.9g (initial %.9g); whole step differs by %.3g of its norm" % (
        float(a["chi2_final"]), float(b["chi2_final"]), float(a["chi2_initial"]), nrm(a["x"] - b["x"]) / nrm(a["x"])))
    assert a["chi2_initial"] == b["chi2_initial"] and np.array_equal(a["_sys"]["S_ld"], b["_sys"]["S_ld"])
    d = a["_sys"]["bs"] - b["_sys"]["bs"]
    assert (d[:-6] == 0).all() and (d[-6:] != 0).any()
