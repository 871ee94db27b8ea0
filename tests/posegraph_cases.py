"""The graphs of the pose-graph tests (tests/test_posegraph_reference.py on the CPU, tests/test_posegraph_gpu.py on the GPU):
name -> arguments of synth_posegraph.make_posegraph.  Sizes: 60 key frames (413 unknowns: the fused factorisation), 200 and 500
(block launches).  Variants: free and fixed scale, several fixed vertices with edges between two of them, duplicate edges.

STRICT_FLOW names the cases on which iteration and trial counts are asserted.  They were chosen on the CPU with the reference
alone: its float64 and long double runs take the same path, and every Levenberg decision and every branch of log clears
FLOW_MARGIN (asserted in test_posegraph_reference.py).  With fixed scale the optimisation converges, and once it has, the gain of
a trial is rounding noise of the numeric Jacobians (a difference quotient over 2e-9): the sign of rho there is not a property of
the algorithm.  The fixed-scale cases among the named ones therefore cap the iterations before that point (max_iters = 2, 3);
the uncapped fixed-scale cases are compared by value only."""
CASES = {
    "loop60": dict(seed=1, n=60, n_points=50),
    "loop60_b": dict(seed=3, n=60, n_points=50),
    "loop60_fixscale": dict(seed=1, n=60, fix_scale=True, n_points=50),
    "merge60": dict(seed=4, n=60, n_fixed=8, duplicates=6, n_points=50),
    "merge60_fixscale": dict(seed=1, n=60, n_fixed=8, duplicates=6, fix_scale=True, n_points=50),
    "loop60_fixscale_cap2": dict(seed=2, n=60, fix_scale=True, max_iters=2, n_points=50),
    "merge60_fixscale_cap3": dict(seed=5, n=60, fix_scale=True, n_fixed=8, duplicates=6, max_iters=3, rot_drift_deg=0.5, trans_drift=0.03, n_points=50),
    "loop200": dict(seed=1, n=200, n_points=100),
    "merge200_fixscale": dict(seed=2, n=200, fix_scale=True, n_fixed=10, duplicates=8, n_points=100),
    "loop500": dict(seed=1, n=500, n_points=200),
    "merge500_fixscale_cap2": dict(seed=2, n=500, fix_scale=True, n_fixed=12, duplicates=10, max_iters=2, n_points=200),
}
STRICT_FLOW = ["loop60", "loop60_b", "merge60", "loop60_fixscale_cap2", "merge60_fixscale_cap3", "loop200", "loop500", "merge500_fixscale_cap2"]
FLOW_MARGIN = 1e-12
