"""fiba_solve (FullInertialBA on the device) against the dense reference of tests/fullba_reference.py.  Every number the device is held
to is written in tests/test_fullba_reference.py, next to the CPU assertion that keeps it honest; the cases are those of
tests/fullba_cases.py.

One trial (max_iters = 1) against first_trial in long double: chi2_initial to 1e-12 relative (the same errors summed in another
order); the states by dense_inertial_reference's check_one_step rule on this column map (every block within
step_tolerance(kappa) + 10 float-getter floors, and within 1e-6 of its step) wherever step_tolerance(kappa) <= 1e-6, and by the backward error of the recovered
step in the reference's long-double system on the gauge-free cases at lambda 1e-5, against four times what the float64 reference's
own step leaves there.  chi2 after the trial: 1e-11 + 2 step_tolerance(kappa) (chi2_initial - chi2_final) / chi2_final relative
(fullba_reference.chi2_final_rtol) -- a step that is off by delta of its norm moves the new cost by at most about 2 delta times the
decrease the step achieved; lambda after
the trial to 1e-12 where the update is clamped, else dense_inertial_reference.unclamped_lambda_rtol.

Full runs against optimize in float64: four times the recorded spread of the three reference runs per output block -- two
implementations may differ from each other by twice what each differs from the truth, and a factor two for operation order
(the reasoning of tests/test_imuinit_gpu.py).  Gauge-free maps are compared on what the gauge leaves alone.  Iterations, trials and
stop reason are asserted on every case: the three reference runs agree on all of them.  (Every run takes five iterations or more, so
ImuCamPose::Update's re-orthonormalisation of Rwb on every third update takes part: the inputs are float matrices, and it moves them by 3e-8.)

Exact: two calls agree bit for bit; a fixed key frame, the IMU states of a key frame in no link and a point seen only by fixed key
frames come back bit-identical; with a shared bias every key frame with IMU states returns one value; a raised stop flag returns the
inputs; liba_solve / liba_solve_batch return the bits recorded from the parent commit (tests/golden/liba_parent_bits.npz).

The device's own deviations (MI355X; every test prints them next to its bounds, run with -s).
One trial: chi2_initial off by at most 1.1e-15 relative.  Step error per block (share of its tolerance, which is capped at 1e-6 of the block's step): s2 6.4e-10 (6e-4), s6 1.5e-11 / 4.6e-12,
s7 4.9e-10 (5e-4), s53 1.1e-7 at lambda 1e-5 (0.11) / 4.8e-11, k4 5.5e-12 / 2.6e-12, k5 1.9e-10, k33 3.7e-10 / 2.4e-11; chi2 after the trial off
by at most 2.4e-10 relative (s53 at lambda 1e-5, kappa 3.3e6; its tolerance 8e-6), 1.07e-11 on s7 at lambda 1, below 1e-11 elsewhere.  Backward error of the
gauge-free cases at lambda 1e-5: s2 1.26e-8 (bound 5.2e-8), s7 3.74e-8 (1.52e-7), k5 1.36e-7 (5.6e-7): the float64 reference's own figures to three digits --
what is left is the rounding of the output states the step is recovered from.
Full runs, every flow equal to the reference's.  Gauge fixed (bounds Rwb 1.8e-15, twb 1.3e-14, vel 8.8e-15, bg 1.4e-14, ba 1.7e-16, points 1.0e-12,
chi2 4.4e-14): s12 Rwb 2.2e-16, twb 8.9e-16, vel 1.0e-15, bg 4.7e-15, ba 3.0e-18, points 6.9e-14, chi2 6.5e-15; k6 Rwb 8.9e-16, twb 6.2e-15, vel 3.8e-15,
bg 1.0e-17, ba 5.6e-17, points 5.5e-13, chi2 4.1e-16.  Gauge free (bounds bg 6.0e-8, ba 3.6e-6, rel_R 1.2e-7, rel_t 8.0e-7, body_v 8.0e-7, z 9.6e-7,
chi2 2.0e-6): s6_100 bg 1.5e-8, ba 5.9e-11, rel_R 3.1e-8, rel_t 2.1e-7, body_v 2.1e-7, z 2.6e-7, chi2 4.0e-8; k12_100 bg 3.1e-10, ba 3.0e-8, rel_R 3.3e-10,
rel_t 1.8e-9, body_v 1.1e-8, z 3.5e-9, chi2 6.5e-9; the two runs cut by the 7-iteration limit: s6_7 bg 1.2e-8, ba 3.1e-11, rel_R 2.2e-8, rel_t 1.5e-7, body_v 1.7e-7,
z 1.7e-7, chi2 9.5e-7; k12_7 bg 1.0e-9, ba 1.0e-7, rel_R 5.2e-10, rel_t 9.1e-9, body_v 4.7e-8, z 1.7e-8, chi2 6.3e-8.  A one-trial call takes 0.11 .. 0.16 ms on the device up to 81 unknowns and 0.52 .. 0.55 ms at 483 / 495."""
import importlib.util
import os

import numpy as np
import pytest

import dense_inertial_reference as R
import fullba_cases as C
import fullba_reference as F
from dense_ba_reference import step_tolerance
from test_fullba_reference import BACKWARD_F64, QUALITY, SPREAD_FIXED, SPREAD_FREE

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
BOUND_FIXED = {k: 4 * v for k, v in SPREAD_FIXED.items()}
BOUND_FREE = {k: 4 * v for k, v in SPREAD_FREE.items()}
OUTPUTS = ("Rwb", "twb", "vel", "bg", "ba", "points")


@pytest.fixture(scope="module")
def solver(pkg):
    s = pkg.FullInertialBA()
    yield s
    s.close()


def _flow(st):
    return (st["iterations"], st["trials"], st["stop_reason"])


def _check_trial(name, lam, pr, r, ref):
    st = r["stats"]
    assert st["iterations"] == 1 and st["trials"] == 1 and ref["rho"] > 0
    np.testing.assert_allclose(st["chi2_initial"], float(ref["chi2_initial"]), rtol=1e-12)
    tol = step_tolerance(ref["kappa"])
    if tol > QUALITY:
        be = F.backward_error(pr, r, ref)
        print("%s lambda %g: %d unknowns, kappa %.3g: backward error %.3g (bound %.3g)" % (name, lam, ref["n_unknowns"], ref["kappa"], be, 4 * BACKWARD_F64[name]))
        assert be <= 4 * BACKWARD_F64[name]
        return
    err, ratio = F.check_one_step(pr, r, ref)
    clamped = 1 - (2 * float(ref["rho"]) - 1) ** 3 <= 1.0 / 3
    np.testing.assert_allclose(st["lambda_"], float(ref["lambda_"]), rtol=1e-12 if clamped else R.unclamped_lambda_rtol(ref)[0])
    print("%s lambda %g: %d unknowns, kappa %.3g: step error %.3g (%.3g of its tolerance), chi2 after the trial off by %.3g relative"
          % (name, lam, ref["n_unknowns"], ref["kappa"], err, ratio, abs(st["chi2_final"] / float(ref["chi2_final"]) - 1)))


@pytest.mark.parametrize("name,lam", C.ONE_TRIAL_IDS)
def test_one_trial(solver, synth, name, lam):
    pr, ref = C.one_trial_of(synth, name, lam)
    _check_trial(name, lam, pr, solver.solve(pr), ref)


def _compare_full(name, pr, d, r, flow):
    free = C.FULL[name]["gauge_free"]
    bound = BOUND_FREE if free else BOUND_FIXED
    got, want = F.full_run_blocks(pr, d, free), F.full_run_blocks(pr, r, free)
    dev = {k: float(np.abs(got[k] - want[k]).max()) for k in got}
    dev["chi2"] = abs(d["stats"]["chi2_final"] - float(r["chi2_final"])) / float(r["chi2_final"])
    ini = abs(d["stats"]["chi2_initial"] - float(r["chi2_initial"])) / float(r["chi2_initial"])
    print("%-8s device flow %s reference flow %s chi2 %.6g -> %.6g (initial off by %.2e) | deviation %s | bounds %s" % (
        name, _flow(d["stats"]), flow, d["stats"]["chi2_initial"], d["stats"]["chi2_final"], ini, {k: "%.2e" % v for k, v in dev.items()},
        {k: "%.2e" % v for k, v in bound.items()}))
    assert ini <= 1e-12
    for k, v in dev.items():
        assert v <= bound[k], (k, v, bound[k])
    assert _flow(d["stats"]) == flow


@pytest.mark.parametrize("name", list(C.FULL))
def test_full_run(solver, name):
    pr, r = C.full_run_of(name)
    _compare_full(name, pr, solver.solve(pr), r, _flow(r["stats"]))


@pytest.mark.parametrize("name", ["s12_100", "k12_100"])
def test_golden(solver, name):
    """the recorded float64 reference results of tools/make_fullba_golden.py: pins the reference as well as the device"""
    g = np.load(os.path.join(GOLDEN, "fullba_12.npz"))
    st = g["%s_stats" % name]
    r = {k: g["%s_%s" % (name, k)] for k in OUTPUTS}
    r.update(chi2_initial=st[4], chi2_final=st[5])
    pr = C.full_problem(name)
    _compare_full(name, pr, solver.solve(pr), r, (int(st[0]), int(st[1]), int(st[2])))


def _exact_problem(shared):
    """8 key frames, key frame 0 fixed, key frame 4 in no link, one more point that only the fixed key frame sees"""
    pr = C.synth_fullba().make_full_map(77, n_kf=8, shared_bias=shared, gauge_free=False, n_no_imu=1, stereo_frac=0.3, bias_error=0.01, max_iters=3)
    pr["links"] = [L for L in pr["links"] if 4 not in (int(L["kf1"]), int(L["kf2"]))]
    pr["points"] = np.vstack([pr["points"], pr["points"][:1] + 0.1])
    e = int(np.nonzero(pr["edge_kf"] == 0)[0][0])
    for k in ("edge_kf", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo"):
        pr[k] = np.concatenate([pr[k], pr[k][e:e + 1]])
    pr["edge_point"][-1] = len(pr["points"]) - 1
    return pr


@pytest.mark.parametrize("shared", [1, 0])
def test_exactness(solver, shared):
    pr = _exact_problem(shared)
    a, b = solver.solve(pr), solver.solve(pr)
    for k in OUTPUTS:
        assert np.array_equal(a[k], b[k]), k
    assert a["stats"] == b["stats"] and a["stats"]["iterations"] == 3
    f64 = lambda k: np.asarray(pr[k], np.float64)
    for k in ("Rwb", "twb", "vel"):
        assert np.array_equal(a[k][0], f64(k).reshape(a[k].shape)[0]), "the fixed key frame's %s moved" % k
    assert np.array_equal(a["vel"][4], f64("vel")[4]), "the velocity of a key frame in no link moved"
    assert not np.array_equal(a["twb"][4], f64("twb")[4]), "its pose is free"
    assert np.array_equal(a["points"][-1], f64("points")[-1]), "a point seen only by the fixed key frame moved"
    assert (a["points"][:-1] != f64("points")[:-1]).any(1).all()
    imu = np.asarray(pr["has_imu"]) != 0
    if shared:
        for k in ("bg", "ba"):
            assert (a[k][imu] == a[k][imu][0]).all() and not np.array_equal(a[k][imu][0], f64("shared_" + k)), k
            assert np.array_equal(a[k][~imu], f64(k)[~imu])
    else:
        for k in ("bg", "ba"):
            assert np.array_equal(a[k][[0, 4]], f64(k)[[0, 4]]), "a fixed or unlinked %s moved" % k
            assert (a[k][[1, 2, 3, 5, 6, 7]] != f64(k)[[1, 2, 3, 5, 6, 7]]).any(1).all()


@pytest.mark.parametrize("shared", [1, 0])
def test_stop_flag(solver, shared):
    pr = _exact_problem(shared)
    flag = np.ones(1, np.uint8)
    r = solver.solve(pr, stop_flag=flag)
    assert _flow(r["stats"]) == (0, 0, 3)
    for k in OUTPUTS:
        assert np.array_equal(r[k], np.asarray(pr[k], np.float64).reshape(r[k].shape)), k
    flag[0] = 0
    a, b = solver.solve(pr, stop_flag=flag), solver.solve(pr)
    assert all(np.array_equal(a[k], b[k]) for k in OUTPUTS) and a["stats"] == b["stats"] and a["stats"]["stop_reason"] != 3


def test_capacity(pkg, synth):
    """1049 free key frames with their own biases in one chain, no points: 15735 unknowns, the first count above FIBA_MAX_UNKNOWNS =
    15732 that 15 a + 6 b reaches.  Refused on the host; the same handle then solves the two-key-frame case."""
    n = 1049
    assert 15 * n > pkg.capi.FIBA_MAX_UNKNOWNS >= 15 * (n - 1)
    small, ref = C.one_trial_of(synth, "s2", 1.0)
    L0 = small["links"][0]
    big = dict(small, n_kf=n, shared_bias=0, links=[dict(L0, kf1=i, kf2=i + 1) for i in range(n - 1)])
    for k, w in (("Rwb", 9), ("twb", 3), ("vel", 3), ("bg", 3), ("ba", 3)):
        big[k] = np.tile(np.asarray(small[k], np.float64).reshape(-1, w)[:1], (n, 1))
    for k in ("pose_fixed", "imu_fixed"):
        big[k] = np.zeros(n, np.uint8)
    big["has_imu"] = np.ones(n, np.uint8)
    for k in ("edge_kf", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo", "points"):
        big[k] = np.asarray(small[k])[:0]
    s = pkg.FullInertialBA()
    try:
        with pytest.raises(pkg.OrbxError) as e:
            s.solve(big)
        assert e.value.code == pkg.capi.ORBX_ERR_CAPACITY
        _check_trial("s2", 1.0, small, s.solve(small), ref)
    finally:
        s.close()


def test_argument_errors(pkg, solver, synth):
    small, _ = C.one_trial_of(synth, "s2", 1.0)
    bad = []
    bad.append(dict(small, links=[dict(small["links"][0], kf2=5)]))                             # an index out of range
    bad.append(dict(small, has_imu=np.array([1, 0], np.uint8)))                                # a link to a key frame without IMU states
    bad.append(dict(small, pose_fixed=np.ones(2, np.uint8), imu_fixed=np.ones(2, np.uint8), shared_bias=0))     # nothing to optimise
    bad.append(dict(small, links=[]))                                                          # a shared bias with no link
    bad.append(dict(small, lambda_init=0.0))
    for pr in bad:
        with pytest.raises(pkg.OrbxError) as e:
            solver.solve(pr)
        assert e.value.code == -3
    r = solver.solve(small)
    assert r["stats"]["iterations"] == 1


def test_existing_entry_points_return_the_parent_commits_bits(pkg, synth):
    """liba_solve on the golden window and two synthetic ones, and liba_solve_batch on the three together, against
    tests/golden/liba_parent_bits.npz (tools/make_fullba_golden.py parent-bits, run on the parent commit's build on an MI355X)"""
    spec = importlib.util.spec_from_file_location("make_fullba_golden", os.path.join(os.path.dirname(os.path.dirname(GOLDEN)), "tools", "make_fullba_golden.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    g = np.load(os.path.join(GOLDEN, "liba_parent_bits.npz"))
    wins = tool.parent_windows(synth)
    s = pkg.InertialSolver()
    b = pkg.LibaBatch()
    try:
        got = {}
        for i, w in enumerate(wins):
            tool.flatten("solve%d" % i, s.solve(w), got)
        for i, r in enumerate(b.solve(wins)):
            tool.flatten("batch%d" % i, r, got)
    finally:
        s.close(); b.close()
    assert sorted(got) == sorted(g.files)
    for k in g.files:
        assert np.array_equal(got[k], g[k]), k
