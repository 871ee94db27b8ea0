"""imu_init_optimize_batch on the GPU against tests/imuinit_reference.py (plain numpy, its own restatement of
EdgeInertialGS, the gravity-direction and scale vertices, the priors, and the Levenberg / Gauss-Newton policy, on a DENSE system).

Tolerances come from the reference alone: it is run in float64, in float64 with the unknowns reversed (the border eliminated first,
which is what the device's structured elimination amounts to) and in long double on the cases of tests/imuinit_cases.py (all on
the CPU, none the code under test; tests/test_imuinit_reference.py asserts that the recorded spread still describes them), and the
device gets four times the recorded spread -- two implementations may differ from each other by twice what each differs from the
truth, and a factor two for operation order.  chi2_initial gets 1e-12 relative: the same errors summed in another order.

Recorded spread (largest over the cases, all of it on kf3_mono, which runs to the cap of 200 iterations): vel 1.42e-12, bg 5.87e-14,
ba 1.32e-13, Rwg 1.82e-12, scale 8.68e-11 absolute, final chi2 6.30e-11 relative.

Exact checks on every case: two runs agree bit for bit; a key frame in no link keeps its velocity bit for bit; a fixed scale, Rwg or
bias (and fixed velocities) come back bit-identical.  Iteration and trial counts are asserted wherever the three reference runs
agree on them, two cases that end on an exact tie aside (STRICT_FLOW, see tests/imuinit_cases.py).

The device's own deviations (MI355X; every test prints them next to its bounds, run with -s), largest over the cases: vel 1.94e-13
(bound 5.68e-12), bg 8.41e-15 (2.35e-13), Rwg 2.48e-13 (7.28e-12), scale 1.20e-11 (3.47e-10), final chi2 8.44e-12 relative (2.52e-10),
all on kf3_mono, the case at the iteration cap; ba 3.05e-13 on kf3_mono_noprior (bound 5.28e-13); 1e-15 .. 1e-13 on the converged
cases; chi2_initial 2.2e-16 relative.  Every flow of STRICT_FLOW (27 cases) equals the reference's; of the two exact ties
kf2_bias does too, kf65_bias takes 13 trials against 14.  One iteration at the computed lambda_0: vel 7.7e-15, bg 8.5e-17,
ba 6.8e-14, Rwg 6.8e-15, scale 1.9e-13 (bounds 8.6e-15, 4.6e-16, 1.8e-13, 1.6e-14, 2.6e-13), lambda equal to the last bit.  The 64
problems of the batch test take 38 ms on the device in one call."""
import importlib
import os
import sys

import numpy as np
import pytest

import imuinit_reference as ref
from imuinit_cases import CASES, STRICT_FLOW, UNDERDETERMINED
from test_imuinit_reference import ONE_ITERATION_CASES, SPREAD, SPREAD_ONE_ITERATION

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BOUND = {k: 4 * v for k, v in SPREAD.items()}       # vel 5.7e-12, bg 2.3e-13, ba 5.3e-13, Rwg 7.3e-12, scale 3.5e-10, chi2 2.5e-10 relative
OUTPUTS = ("vel", "bg", "ba", "Rwg", "scale")
_REFERENCE = {}


@pytest.fixture(scope="module")
def sy(pkg):
    return importlib.import_module("orb_slam3-1_amd.synth_imuinit")


@pytest.fixture(scope="module")
def solver(pkg):
    s = pkg.ImuInit()
    yield s
    s.close()


def _case(sy, name):
    """the problem of a case and its float64 reference result, computed once and shared (nobody writes to either)"""
    if name not in _REFERENCE:
        pr = sy.make_imu_init(**CASES[name])[0]
        _REFERENCE[name] = (pr, ref.optimize(pr, np.float64))
    return _REFERENCE[name]


def _flow(st):
    return (st["iterations"], st["trials"], st["stop_reason"])


def _same(a, b):
    return all(np.array_equal(a[k], b[k]) for k in OUTPUTS) and a["chi2_initial"] == b["chi2_initial"] and a["chi2_final"] == b["chi2_final"] \
        and a["stats"] == b["stats"]


def _exact_checks(pr, d):
    """what must come back bit for bit"""
    n = len(pr["vel"])
    linked = np.zeros(n, bool)
    for L in pr["links"]:
        linked[[L["kf1"], L["kf2"]]] = True
    vel_in = np.asarray(pr["vel"], np.float64)
    assert np.array_equal(d["vel"][~linked], vel_in[~linked]), "the velocity of a key frame in no link moved"
    if not pr["free_vel"]:
        assert np.array_equal(d["vel"], vel_in), "a fixed velocity moved"
    elif len(pr["links"]) and pr["max_iters"]:
        assert (d["vel"][linked] != vel_in[linked]).any(1).all(), "a free velocity was not updated"
    if not pr["free_bias"]:
        assert np.array_equal(d["bg"], np.asarray(pr["bg"], np.float64)) and np.array_equal(d["ba"], np.asarray(pr["ba"], np.float64)), "a fixed bias moved"
    if not pr["free_gdir"]:
        assert np.array_equal(d["Rwg"], np.asarray(pr["Rwg"], np.float64)), "a fixed Rwg moved"
    if not pr["free_scale"]:
        assert d["scale"] == float(pr["scale"]), "a fixed scale moved"


def _compare(name, pr, d, r, strict=None):
    s, q = d["stats"], r["stats"]
    dev = {k: float(np.abs(d[k] - np.asarray(r[k], np.float64)).max()) for k in OUTPUTS}
    dev["chi2"] = abs(d["chi2_final"] - float(r["chi2_final"])) / float(r["chi2_final"])
    dev["chi2_initial"] = abs(d["chi2_initial"] - float(r["chi2_initial"])) / float(r["chi2_initial"])
    print("%-20s device flow %s reference flow %s chi2 %.6g -> %.6g | deviation %s | bounds %s" % (
        name, _flow(s), _flow(q), d["chi2_initial"], d["chi2_final"], {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in BOUND.items()}))
    _exact_checks(pr, d)
    assert s["chi2_initial"] == d["chi2_initial"] and s["chi2_final"] == d["chi2_final"]
    assert dev["chi2_initial"] <= 1e-12                 # the same errors summed in another order
    for k in OUTPUTS:
        assert dev[k] <= BOUND[k], k
    if name not in UNDERDETERMINED:
        assert dev["chi2"] <= BOUND["chi2"]
    if name in STRICT_FLOW if strict is None else strict:
        assert _flow(s) == _flow(q), name
    return dev


@pytest.mark.parametrize("name", list(CASES))
def test_full_solve_against_reference(sy, solver, name):
    """2, 3, 10, 65 (more links than a wave) and 130 key frames (three paths, two isolated key frames, shuffled) in each of the six
    settings; all value checks on every case"""
    pr, r = _case(sy, name)
    d = solver.optimize(pr)
    d2 = solver.optimize(pr)
    assert _same(d, d2), "two runs differ"
    _compare(name, pr, d, r)
    assert d["stats"]["iterations"] >= 1 and (d["stats"]["lambda_"] > 0) == (not pr["gauss_newton"])


@pytest.mark.parametrize("name", ONE_ITERATION_CASES)
def test_first_trial_uses_the_computed_lambda(sy, solver, name):
    """lambda_init = 0 and one iteration: the trials run from lambda_0 = 1e-5 max diag H, which the device has to compute (before lambda
    is added to the diagonal), over the velocity blocks and the border alike.  The same lambda given explicitly reproduces the run;
    another one does not."""
    pr = dict(_case(sy, name)[0], max_iters=1, lambda_init=0.0)
    d = solver.optimize(pr)
    r = ref.optimize(pr, np.float64)
    lam0 = float(r["stats"]["lambda_0"])
    assert _flow(d["stats"]) == _flow(r["stats"]) and d["stats"]["iterations"] == 1
    # nothing has converged after one iteration: the bounds are four times the reference's own spread on exactly these one-iteration
    # problems (SPREAD_ONE_ITERATION, asserted on the CPU).  lambda after the iteration is lambda_0 times one factor per trial: it
    # carries the deviation of max diag H, a sum of at most 18 products of Jacobian entries that are themselves ~10 operations deep;
    # the reference's runs share one assembly order, so their spread (one unit in the last place) says nothing about another
    # order: 64 units in the last place instead
    bound = {k: 4 * v for k, v in SPREAD_ONE_ITERATION.items()}
    bound["lambda_"] = max(bound["lambda_"], 64 * np.finfo(np.float64).eps)
    dev = {k: float(np.abs(d[k] - np.asarray(r[k], np.float64)).max()) for k in OUTPUTS}
    dev["lambda_"] = abs(d["stats"]["lambda_"] - float(r["stats"]["lambda_"])) / float(r["stats"]["lambda_"])
    print("%-20s lambda_0 %.6g, lambda after the iteration: device %.6g reference %.6g | deviation %s | bounds %s" % (
        name, lam0, d["stats"]["lambda_"], float(r["stats"]["lambda_"]), {k: "%.2e" % v for k, v in dev.items()}, {k: "%.2e" % v for k, v in bound.items()}))
    for k in bound:
        assert dev[k] <= bound[k], k
    given = solver.optimize(dict(pr, lambda_init=lam0))
    # (the reference's lambda_0 may differ from the device's in its last places: the result moves by that relative amount of the
    # step at most, and a step is below 10 in every unknown)
    for k in OUTPUTS:
        assert np.abs(given[k] - d[k]).max() <= 10 * bound["lambda_"] + bound[k], k
    assert _flow(given["stats"]) == _flow(d["stats"])
    other = solver.optimize(dict(pr, lambda_init=1e3 * lam0))
    moved = max(np.abs(other[k] - d[k]).max() for k in OUTPUTS)
    assert moved > 1e-6, moved


def test_batch_equals_single_calls(sy, solver):
    """64 problems of mixed sizes and settings in one call equal the 64 single calls bit for bit; the handle is reused across
    sizes throughout, growing and shrinking"""
    names = list(CASES)
    problems = [_case(sy, names[(7 * i) % len(names)])[0] for i in range(60)]
    problems += [dict(problems[3], links=[]), dict(problems[10], max_iters=0), dict(problems[22], max_iters=3), sy.make_imu_init(9, 256, variant="bias", max_iters=5)[0]]
    assert len(problems) == 64
    batch = solver.optimize_batch(problems)
    ms = solver.last_device_ms()
    singles = [solver.optimize(p) for p in problems]
    again = solver.optimize_batch(problems)
    for i, (b, s, a) in enumerate(zip(batch, singles, again)):
        assert _same(b, s), "problem %d of the batch differs from its single call" % i
        assert _same(b, a), "problem %d differs between two batches" % i
        _exact_checks(problems[i], b)
    print("64 problems in one call: %.3f ms on the device" % ms)
    assert ms > 0
    empty, capped = batch[60], batch[61]
    for d, p in ((empty, problems[60]), (capped, problems[61])):        # zero links / zero iterations: the inputs come back
        assert d["stats"]["iterations"] == 0 and d["stats"]["trials"] == 0
        assert np.array_equal(d["vel"], p["vel"]) and np.array_equal(d["Rwg"], p["Rwg"]) and d["scale"] == p["scale"]
        assert np.array_equal(d["bg"], p["bg"]) and np.array_equal(d["ba"], p["ba"])
    assert empty["chi2_initial"] == 0 and capped["chi2_initial"] > 0 and capped["chi2_final"] == capped["chi2_initial"]
    assert batch[62]["stats"]["iterations"] == 3
    r = ref.optimize(problems[63], np.float64)                          # the capacity: 256 key frames, every thread a position
    _compare("kf256_bias_5_iterations", problems[63], batch[63], r, strict=False)


def test_golden(solver):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        from make_imuinit_golden import unpack
    finally:
        sys.path.pop(0)
    g = np.load(os.path.join(ROOT, "tests", "golden", "imu_init_10.npz"))
    pr = unpack(g)
    d = solver.optimize(pr)
    r = dict(vel=g["ref_vel"], bg=g["ref_bg"], ba=g["ref_ba"], Rwg=g["ref_Rwg"], scale=float(g["ref_scale"]), chi2_initial=float(g["ref_chi2_initial"]),
             chi2_final=float(g["ref_chi2_final"]), stats=dict(iterations=int(g["ref_flow"][0]), trials=int(g["ref_flow"][1]), stop_reason=int(g["ref_flow"][2])))
    _compare("kf10_mono", pr, d, r)
