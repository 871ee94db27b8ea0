"""essg_optimize_4dof on the GPU against tests/posegraph4dof_reference.py (plain numpy, its own restatement of ExpSO3 / LogSO3 /
UpdateW, Edge4DoF, the numeric Jacobians, the information matrix and the Levenberg policy of Optimizer::OptimizeEssentialGraph4DoF).

Tolerances come from the reference alone: it is run in float64 and in long double on the cases of tests/posegraph4dof_cases.py
(both on the CPU, neither the code under test; tests/test_posegraph4dof_reference.py asserts that the recorded spread still
describes them), and the device gets four times the recorded spread -- two implementations may differ from each other by twice
what each differs from the truth, and a factor two for operation order.  Float outputs get one float unit in the last place of
the largest value on top (the device rounds a double that may sit on the other side of a rounding boundary).

Recorded spread (largest over the cases): rcw_out 5.17e-9, tcw_out 6.63e-8 absolute (translations reach 8), final chi2 2.47e-9
relative, pose_q 5.97e-8, pose_t 4.77e-7, corrected points 4.77e-7.  The numeric Jacobians divide the rounding of an error by
2e-9; results of an optimisation that stops before it has converged (the capped cases) inherit that.

Exact checks: fixed vertices come back bit-identical in rcw_out / tcw_out, and two runs agree bit for bit.  Iteration and trial
counts are asserted on the cases of STRICT_FLOW only (see tests/posegraph4dof_cases.py); those leave lambda_init at 0, so they
also cover the max diag H from which the device computes lambda_0.

The device's own deviations (MI355X; every test prints them next to its bounds, run with -s), largest over the cases: rcw_out
1.41e-8 (loop121_cap2; bound 2.07e-8), tcw_out 1.29e-7 (float40_tcb_cap2; bound 2.65e-7), final chi2 2.06e-9 relative (loop121_cap2;
bound 9.88e-9; 1e-13 .. 1e-15 on the uncapped cases), chi2_initial 2.5e-15 relative, pose_q 5.96e-8, pose_t 4.77e-7 and points
4.77e-7 (one float unit in the last place each); every flow equals the reference's, the uncapped ones included.  One
linearisation: 8.9e-16 .. 1.8e-15 (bound 1e-13).  One iteration at the computed lambda_0: rcw 2.65e-8, tcw 2.56e-7, lambda 2.4e-8
relative (bounds 1.2e-7, 1.6e-6, 3.5e-7)."""
import importlib
import os

import numpy as np
import pytest

import posegraph4dof_reference as ref
from posegraph4dof_cases import CASES, STRICT_FLOW
from test_posegraph4dof_reference import ONE_ITERATION_CASES, SPREAD, SPREAD_ONE_ITERATION

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = {k: 4 * v for k, v in SPREAD.items()}       # rcw 2.1e-8, tcw 2.7e-7, chi2 9.9e-9 relative, pose_q 2.4e-7, pose_t 1.9e-6, points 1.9e-6
OUTPUTS = ("rcw_out", "tcw_out", "pose_q", "pose_t", "points_out")
_REFERENCE = {}


def _ulp32(a):
    return float(np.spacing(np.float32(np.abs(a).max()))) if len(a) else 0.0


@pytest.fixture(scope="module")
def sp(pkg):
    return importlib.import_module("orb_slam3-1_amd.synth_posegraph")


@pytest.fixture(scope="module")
def solver(pkg):
    s = pkg.EssentialGraph()
    yield s
    s.close()


def _case(sp, name):
    """the graph of a case and its float64 reference result, computed once and shared (nobody writes to either)"""
    if name not in _REFERENCE:
        pr = sp.make_posegraph4dof(**CASES[name])
        _REFERENCE[name] = (pr, ref.optimize(pr, np.float64))
    return _REFERENCE[name]


def _flow(st):
    return (st["iterations"], st["trials"], st["stop_reason"])


def _compare(name, pr, d, r):
    s, q = d["stats"], r["stats"]
    dev = dict(rcw=np.abs(d["rcw_out"] - r["rcw_out"]).max(), tcw=np.abs(d["tcw_out"] - r["tcw_out"]).max(),
               pose_q=np.abs(d["pose_q"] - r["pose_q"]).max(), pose_t=np.abs(d["pose_t"] - r["pose_t"]).max(),
               points=np.abs(d["points_out"] - r["points_out"]).max() if len(r["points_out"]) else 0.0,
               chi2=abs(s["chi2_final"] - float(q["chi2_final"])) / float(q["chi2_final"]),
               chi2_initial=abs(s["chi2_initial"] - float(q["chi2_initial"])) / float(q["chi2_initial"]))
    print("%-18s device flow %s reference flow %s chi2 %.6g -> %.6g | deviation %s | bounds %s" % (
        name, _flow(s), _flow(q), s["chi2_initial"], s["chi2_final"], {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in BOUND.items()}))
    fixed = np.asarray(pr["fixed"]).astype(bool)
    assert np.array_equal(d["rcw_out"][fixed], np.asarray(pr["rcw"])[fixed]) and np.array_equal(d["tcw_out"][fixed], np.asarray(pr["tcw"])[fixed]), "a fixed vertex moved"
    assert dev["chi2_initial"] <= 1e-12                 # the same errors summed in another order: 6 E terms of ~1e-13 relative rounding
    assert dev["rcw"] <= BOUND["rcw"]
    assert dev["tcw"] <= BOUND["tcw"]
    assert dev["chi2"] <= BOUND["chi2"]
    assert dev["pose_q"] <= BOUND["pose_q"] + _ulp32(r["pose_q"])
    assert dev["pose_t"] <= BOUND["pose_t"] + _ulp32(r["pose_t"])
    assert dev["points"] <= BOUND["points"] + _ulp32(r["points_out"])
    if name in STRICT_FLOW:
        assert _flow(s) == _flow(q), name
    return dev


@pytest.mark.parametrize("name", list(CASES))
def test_full_solve_against_reference(sp, solver, name):
    """9 and 40 key frames and 121 with one fixed run the fused factorisation, 122 and 126 with five fixed the block launches;
    every variant; all value checks on every case"""
    pr, r = _case(sp, name)
    d = solver.optimize_4dof(pr)
    d2 = solver.optimize_4dof(pr)
    for k in OUTPUTS:
        assert np.array_equal(d[k], d2[k]), "two runs differ in %s" % k
    assert d["stats"] == d2["stats"]
    _compare(name, pr, d, r)
    free = ~np.asarray(pr["fixed"]).astype(bool)
    assert (d["tcw_out"][free] != np.asarray(pr["tcw"])[free]).any(1).all()             # every free vertex was updated


@pytest.mark.parametrize("name", ["loop9", "loop40", "multi40", "loop121", "multi122_cap2"])
def test_one_linearisation(sp, solver, name):
    """max_iters = 1 with a lambda so large that the step is b / lambda: the trial state exposes the assembled right-hand side,
    chi2_initial the errors.  H itself is covered by the full solves.  (Not on float-rounded inputs: there the first update
    replaces the stored camera pose by the one recomputed from the body pose, 1e-7 away, which a step of 1e-12 cannot pay for,
    so every trial is rejected and nothing is exposed.)"""
    pr = dict(_case(sp, name)[0], max_iters=1, lambda_init=1e12)
    d = solver.optimize_4dof(pr)
    L = ref.linearize(pr, ref.initial_state(pr, np.float64), np.float64)
    assert abs(d["stats"]["chi2_initial"] - float(L["chi2"])) <= 1e-12 * float(L["chi2"])
    r = ref.optimize(pr, np.float64)
    assert d["stats"]["iterations"] == 1 and d["stats"]["trials"] == r["stats"]["trials"] == 1
    step = np.abs(L["b"]).max() / 1e12
    dev = max(np.abs(d["rcw_out"] - r["rcw_out"]).max(), np.abs(d["tcw_out"] - r["tcw_out"]).max())
    print("%-18s largest |b| / lambda %.2e, deviation %.2e" % (name, step, dev))
    # the update is b / 1e12 (~1e-12), its error the Jacobians' ~1e-6 relative: far below the last place of a coordinate of up to
    # 8 (1.8e-15), which the ~20 operations that recompute the camera pose from the body pose may each round differently
    assert dev <= 1e-13
    free = ~np.asarray(pr["fixed"]).astype(bool)
    assert (d["tcw_out"][free] != np.asarray(pr["tcw"])[free]).any()


@pytest.mark.parametrize("name", ONE_ITERATION_CASES)
def test_first_trial_uses_the_computed_lambda(sp, solver, name):
    """lambda_init = 0 and one iteration: the only trial runs at lambda_0 = 1e-5 max diag H, which the device has to compute (before
    lambda is added to the diagonal).  The same lambda given explicitly reproduces the run; another one does not."""
    pr = dict(_case(sp, name)[0], max_iters=1, lambda_init=0.0)
    d = solver.optimize_4dof(pr)
    r = ref.optimize(pr, np.float64)
    lam0 = float(r["stats"]["lambda_0"])
    assert _flow(d["stats"]) == _flow(r["stats"]) == (1, 1, 0)
    # nothing has converged after one iteration, so the bounds are four times the reference's own float64 / long double spread on
    # exactly these one-iteration problems (SPREAD_ONE_ITERATION, asserted on the CPU), not the spread of the full cases.  lambda
    # after the accepted trial is lambda_0 times a factor in [1/3, 2/3] that depends on rho: it carries the deviation of max diag H
    bound = {k: 4 * v for k, v in SPREAD_ONE_ITERATION.items()}
    dev = dict(rcw=np.abs(d["rcw_out"] - r["rcw_out"]).max(), tcw=np.abs(d["tcw_out"] - r["tcw_out"]).max(),
               lambda_=abs(d["stats"]["lambda_"] - float(r["stats"]["lambda_"])) / float(r["stats"]["lambda_"]))
    print("%-18s lambda_0 %.6g, lambda after the trial: device %.6g reference %.6g | deviation %s | bounds %s" % (
        name, lam0, d["stats"]["lambda_"], float(r["stats"]["lambda_"]), {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in bound.items()}))
    for k in bound:
        assert dev[k] <= bound[k], k
    given = solver.optimize_4dof(dict(pr, lambda_init=lam0))
    # (the reference's lambda_0 may differ from the device's by the 3.5e-7 relative allowed above; the reference's own result
    # moves by 1.7e-8 at most over these cases when its lambda_0 is changed by that much -- measured on the CPU -- twice that)
    assert np.abs(given["tcw_out"] - d["tcw_out"]).max() <= 3.5e-8
    other = solver.optimize_4dof(dict(pr, lambda_init=1e3 * lam0))
    assert np.abs(other["tcw_out"] - d["tcw_out"]).max() > 1e-6


def test_golden(solver):
    g = np.load(os.path.join(ROOT, "tests", "golden", "posegraph4dof_40.npz"))
    pr = {k: g[k] for k in ("rcw", "tcw", "rwb", "twb", "rcb", "tcb", "fixed", "edge_vertices", "edge_rot", "edge_trans", "information", "points", "point_ref", "scw")}
    pr.update(max_iters=int(g["max_iters"]), lambda_init=float(g["lambda_init"]))
    d = solver.optimize_4dof(pr)
    r = dict(rcw_out=g["ref_rcw"], tcw_out=g["ref_tcw"], pose_q=g["ref_pose_q"], pose_t=g["ref_pose_t"], points_out=g["ref_points"],
             stats=dict(iterations=int(g["ref_flow"][0]), trials=int(g["ref_flow"][1]), stop_reason=int(g["ref_flow"][2]),
                        chi2_initial=float(g["ref_chi2_initial"]), chi2_final=float(g["ref_chi2_final"])))
    _compare("loop40_cap2", pr, d, r)


def test_stop_flag_and_handle_reuse(pkg, sp, solver):
    """a raised flag ends the call before the first iteration (stop reason 3, the input returned); one handle then serves a 4-DoF
    graph, a Sim3 graph and the 4-DoF graph again"""
    pr, _ = _case(sp, "loop40")
    flag = np.ones(1, np.uint8)
    d = solver.optimize_4dof(pr, stop_flag=flag)
    assert d["stats"]["stop_reason"] == 3 and d["stats"]["iterations"] == 0
    assert np.array_equal(d["rcw_out"], pr["rcw"]) and np.array_equal(d["tcw_out"], pr["tcw"])
    assert np.array_equal(d["pose_t"], pr["tcw"].astype(np.float32))
    sim3 = sp.make_posegraph(7, n=30, n_points=5)
    b0 = solver.optimize(sim3)
    a = solver.optimize_4dof(pr)
    b = solver.optimize(sim3)
    c = solver.optimize_4dof(pr)
    for k in OUTPUTS:
        assert np.array_equal(a[k], c[k]), k
    assert a["stats"] == c["stats"] and a["stats"]["iterations"] >= 1
    for k in ("sim3_out", "pose_q", "pose_t", "points_out"):
        assert np.array_equal(b[k], b0[k]), k
    assert b["stats"] == b0["stats"] and b["stats"]["iterations"] >= 1
    print("4-DoF, Sim3, 4-DoF on one handle: flows %s %s %s" % (_flow(a["stats"]), _flow(b["stats"]), _flow(c["stats"])))
    ms, stages = solver.last_device_ms()
    assert ms > 0 and stages["rounds"] > 0
