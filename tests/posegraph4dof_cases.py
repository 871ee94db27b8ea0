"""The graphs of the 4-DoF pose-graph tests (tests/test_posegraph4dof_reference.py on the CPU, tests/test_posegraph4dof_gpu.py on the
GPU): name -> arguments of synth_posegraph.make_posegraph4dof.  Sizes are the smallest at which the kernels can still go wrong:
9 key frames (28 edges: not a multiple of the 8 edges a linearisation workgroup takes, 32 unknowns: one partial Cholesky block),
40 (156 unknowns: three blocks, the last partial; more system blocks than one assembly workgroup holds), and the two sizes either
side of the point where dense_chol.h leaves the fused factorisation (kFusedMaxBlocks * NB = 480 unknowns): 121 key frames with one
fixed (480 unknowns, 8 blocks, fused) and 122 (484, 9 blocks, a diag / panel / update launch per block column).  Variants: one
fixed vertex; five fixed with edges between two of them and duplicate edges; float-rounded camera / body inputs with a camera-body
calibration that is not the identity; a CorrectedSim3 scale that is not 1 in scw.

STRICT_FLOW names the cases on which iteration and trial counts are asserted.  They were chosen on the CPU with the reference
alone: its float64 and long double runs take the same path, and every Levenberg decision clears FLOW_MARGIN (asserted in
test_posegraph4dof_reference.py).  With a fixed vertex this graph converges in three or four iterations, and once it has, the gain
of a trial is rounding noise of the numeric Jacobians (a difference quotient over 2e-9): the sign of rho there is not a property
of the algorithm.  The strict cases therefore cap the iterations before that point (max_iters = 2); the uncapped cases are
compared by value only.  All strict cases leave lambda_init at 0, so their first trial runs at the computed lambda_0 and the
second at what the first one's rho made of it: a wrong max diag H changes their chi2 trace."""
_BIG = dict(yaw_drift_deg=0.5, trans_drift=0.03)
CASES = {
    "loop9": dict(seed=1, n=9, n_points=5),
    "loop9_cap2": dict(seed=2, n=9, n_points=5, max_iters=2, **_BIG),
    "loop40": dict(seed=1, n=40, n_points=20, corrected_scale=1.02),
    "loop40_cap2": dict(seed=4, n=40, n_points=20, max_iters=2, **_BIG),
    "multi40": dict(seed=2, n=40, n_fixed=5, duplicates=4, n_points=20),
    "multi40_cap2": dict(seed=5, n=40, n_fixed=5, duplicates=4, n_points=20, max_iters=2, **_BIG),
    "float40_tcb": dict(seed=3, n=40, float_inputs=True, identity_tcb=False, n_points=20),
    "float40_tcb_cap2": dict(seed=6, n=40, float_inputs=True, identity_tcb=False, n_points=20, max_iters=2, **_BIG),
    "loop121": dict(seed=1, n=121, n_points=40),
    "loop121_cap2": dict(seed=2, n=121, n_points=40, max_iters=2, **_BIG),
    "loop122": dict(seed=1, n=122, n_points=40, corrected_scale=0.97),
    "multi122_cap2": dict(seed=2, n=126, n_fixed=5, duplicates=6, n_points=40, max_iters=2, **_BIG),
}
STRICT_FLOW = ["loop9_cap2", "loop40_cap2", "multi40_cap2", "float40_tcb_cap2", "loop121_cap2", "multi122_cap2"]
FLOW_MARGIN = 1e-6
