"""essg_optimize on the GPU against tests/posegraph_reference.py (plain numpy, its own restatement of g2o::Sim3, the numeric
Jacobians and the Levenberg policy of Optimizer::OptimizeEssentialGraph).

Tolerances come from the reference alone: it is run in float64 and in long double on the cases of tests/posegraph_cases.py (both
on the CPU, neither the code under test; tests/test_posegraph_reference.py asserts that the recorded spread still describes
them), and the device gets four times the recorded spread -- two implementations may differ from each other by twice what each
differs from the truth, and a factor two for operation order.  Float outputs get one float unit in the last place of the largest
value on top (the device rounds a double that may sit on the other side of a rounding boundary).

Recorded spread (largest over the cases): sim3_out 2.03e-6 absolute (translations reach 8), final chi2 2.12e-4 relative
(loop500; 1e-11 on the converged fixed-scale cases), pose_q 1.79e-7, pose_t 2.38e-6, corrected points 3.10e-6.  The numeric
Jacobians divide the rounding of an error by 2e-9, so they carry about 3e-6 absolute in float64; results of an optimisation that
stops before it has converged inherit that.

Exact checks: fixed vertices come back bit-identical, with fixed scale every scale does, and two runs agree bit for bit.
Iteration and trial counts are asserted on the cases of STRICT_FLOW only (see tests/posegraph_cases.py).

The device's own deviations are not recorded here yet: every test prints them (run with -s) next to its bounds."""
import importlib
import os

import numpy as np
import pytest

import posegraph_reference as ref
from posegraph_cases import CASES, STRICT_FLOW
from test_posegraph_reference import SPREAD

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = {k: 4 * v for k, v in SPREAD.items()}       # sim3 8.1e-6, chi2 8.5e-4 relative, pose_q 7.2e-7, pose_t 9.5e-6, points 1.2e-5


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


def _flow(st):
    return (st["iterations"], st["trials"], st["stop_reason"])


def _compare(name, pr, d, r):
    s, q = d["stats"], r["stats"]
    dev = dict(sim3=np.abs(d["sim3_out"] - r["sim3_out"]).max(), pose_q=np.abs(d["pose_q"] - r["pose_q"]).max(),
               pose_t=np.abs(d["pose_t"] - r["pose_t"]).max(),
               points=np.abs(d["points_out"] - r["points_out"]).max() if len(r["points_out"]) else 0.0,
               chi2=abs(s["chi2_final"] - float(q["chi2_final"])) / float(q["chi2_final"]),
               chi2_initial=abs(s["chi2_initial"] - float(q["chi2_initial"])) / float(q["chi2_initial"]))
    print("%-24s device flow %s reference flow %s chi2 %.6g -> %.6g | deviation %s | bounds %s" % (
        name, _flow(s), _flow(q), s["chi2_initial"], s["chi2_final"], {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in BOUND.items()}))
    fixed = pr["fixed"].astype(bool)
    assert np.array_equal(d["sim3_out"][fixed], pr["sim3"][fixed]), "a fixed vertex moved"
    if pr["fix_scale"]:
        assert np.array_equal(d["sim3_out"][:, 7], pr["sim3"][:, 7]), "a scale changed under fix_scale"
    assert dev["chi2_initial"] <= 1e-12                 # the same errors summed in another order: 7 E terms of ~1e-13 relative rounding
    assert dev["sim3"] <= BOUND["sim3"]
    assert dev["chi2"] <= BOUND["chi2"]
    assert dev["pose_q"] <= BOUND["pose_q"] + _ulp32(r["pose_q"])
    assert dev["pose_t"] <= BOUND["pose_t"] + _ulp32(r["pose_t"])
    assert dev["points"] <= BOUND["points"] + _ulp32(r["points_out"])
    if name in STRICT_FLOW:
        assert _flow(s) == _flow(q), name
    return dev


@pytest.mark.parametrize("name", list(CASES))
def test_full_solve_against_reference(sp, solver, name):
    """N = 60 runs the fused factorisation, 200 and 500 the block launches; every variant; all value checks on every case"""
    pr = sp.make_posegraph(**CASES[name])
    d = solver.optimize(pr)
    d2 = solver.optimize(pr)
    for k in ("sim3_out", "pose_q", "pose_t", "points_out"):
        assert np.array_equal(d[k], d2[k]), "two runs differ in %s" % k
    assert d["stats"] == d2["stats"]
    _compare(name, pr, d, ref.optimize(pr, np.float64))


@pytest.mark.parametrize("name", ["loop60", "merge60_fixscale", "loop200", "merge500_fixscale_cap2"])
def test_one_linearisation(sp, solver, name):
    """max_iters = 1 with a lambda so large that the step is b / lambda: the trial state exposes the assembled right-hand side,
    chi2_initial the errors.  H itself is covered by the full solves."""
    pr = dict(sp.make_posegraph(**CASES[name]), max_iters=1, lambda_init=1e12)
    d = solver.optimize(pr)
    L = ref.linearize(pr, np.asarray(pr["sim3"], np.float64), np.float64)
    assert abs(d["stats"]["chi2_initial"] - float(L["chi2"])) <= 1e-12 * float(L["chi2"])
    r = ref.optimize(pr, np.float64)
    assert d["stats"]["iterations"] == 1 and d["stats"]["trials"] == r["stats"]["trials"] == 1
    # the update is b / 1e12 (|b| up to ~1e2: 1e-10), its error the Jacobians' 3e-6 relative: far below the last place of a coordinate
    assert np.abs(d["sim3_out"] - r["sim3_out"]).max() <= 1e-13
    free = ~pr["fixed"].astype(bool)
    assert (d["sim3_out"][free] != pr["sim3"][free]).any()


def test_golden(solver):
    g = np.load(os.path.join(ROOT, "tests", "golden", "posegraph_60.npz"))
    pr = {k: g[k] for k in ("sim3", "fixed", "edge_vertices", "edge_measurement", "points", "point_ref")}
    pr.update(fix_scale=int(g["fix_scale"]), max_iters=int(g["max_iters"]), lambda_init=float(g["lambda_init"]))
    d = solver.optimize(pr)
    r = dict(sim3_out=g["ref_sim3"], pose_q=g["ref_pose_q"], pose_t=g["ref_pose_t"], points_out=g["ref_points"],
             stats=dict(iterations=int(g["ref_flow"][0]), trials=int(g["ref_flow"][1]), stop_reason=int(g["ref_flow"][2]),
                        chi2_initial=float(g["ref_chi2_initial"]), chi2_final=float(g["ref_chi2_final"])))
    _compare("loop60", pr, d, r)


def test_stop_flag_and_handle_reuse(sp, solver):
    """a raised flag ends the call before the first iteration (stop reason 3, the input returned); the handle then serves a
    smaller and a larger graph"""
    pr = sp.make_posegraph(**CASES["loop60"])
    flag = np.ones(1, np.uint8)
    d = solver.optimize(pr, stop_flag=flag)
    assert d["stats"]["stop_reason"] == 3 and d["stats"]["iterations"] == 0
    assert np.array_equal(d["sim3_out"], pr["sim3"])
    small = sp.make_posegraph(7, n=9, n_points=3)
    a = solver.optimize(small)
    b = solver.optimize(pr)
    c = solver.optimize(small)
    assert np.array_equal(a["sim3_out"], c["sim3_out"]) and a["stats"] == c["stats"]
    assert b["stats"]["iterations"] >= 1
    ms, stages = solver.last_device_ms()
    assert ms > 0 and stages["rounds"] > 0
