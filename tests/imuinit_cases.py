"""The cases of the IMU-initialisation tests (arguments of synth_imuinit.make_imu_init), shared by the reference's own tests, the GPU
tests and tools/make_imuinit_golden.py.  A test helper, not a test.

Key-frame counts: 2 and 3 (the smallest chains), 10, 65 (more links than a wave) and 130 (three paths plus two isolated key frames,
key frames and links shuffled).  On every count the six settings of synth_imuinit.VARIANTS: the full monocular one with the
first-stage priors (1e2, 1e10) and lambda_0 = 1e3; the same without priors, where lambda_0 has to be computed; scale fixed (stereo);
the biases-and-velocities overload; the Gauss-Newton overload with Huber 1 on every link; bFixedVel.
kf3_mono is the seed on which the reference runs to the cap of 200 iterations (317 trials)."""

COUNTS = (2, 3, 10, 65, 130)
SETTINGS = ("mono", "mono_noprior", "stereo", "bias", "scale_refine", "fixed_vel")


def _args(n, variant):
    a = dict(seed=100 + n, n=n, variant=variant)
    if n == 3 and variant == "mono":
        a["seed"] = 3
    if n == 130:
        a.update(n_paths=3, n_isolated=2, shuffle=True)
    return a


CASES = {"kf%d_%s" % (n, v): _args(n, v) for n in COUNTS for v in SETTINGS}

# Two key frames without priors: 3 + 3 + 6 + 2 + 1 unknowns against 9 residuals.  The system is under-determined, chi2 falls to
# ~1e-12 and below, and both its relative deviation and the flow are decided by rounding: out of the relative chi2 check and out of
# STRICT_FLOW.
UNDERDETERMINED = ("kf2_mono_noprior",)

# Flow (iterations, trials, stop reason) is asserted wherever the three reference runs (float64, float64 with the unknowns reversed,
# long double) agree on it; tests/test_imuinit_reference.py asserts that they do on exactly STRICT_FLOW.  They agree on every case.
# Two are left out all the same, each for its own reason, which that test also asserts:
#   kf2_bias   ends (stop reason 1) on trials that leave chi2 EXACTLY unchanged in float64: cur - trial chi2 == 0, so rho == 0 and the
#              sign the policy tests is that of a rounding error (decision margin 0 in both float64 runs, 4e-18 in long double);
#   kf65_bias  the same: its tenth trial of the last iteration is an exact tie in float64 (margin 0; 1.4e-18 in long double).
# An implementation that sums the same chi2 in another order may land on either side of an exact tie.
EXACT_TIE = ("kf2_bias", "kf65_bias")
STRICT_FLOW = tuple(k for k in CASES if k not in UNDERDETERMINED + EXACT_TIE)
