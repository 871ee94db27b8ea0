"""Writes tests/golden/sim3_ransac_120.npz and sim3_opt_120.npz: one seeded scene each (orb_slam3-1_amd/synth_sim3.py) plus
the outputs of the numpy reference (tests/sim3_reference.py) on it, so that the GPU tests do not depend on the generator's
RNG stream.  Needs the built library only for sim3_draw_triples (host code); no GPU.

The optimiser scene is the first seed on which every accept / reject decision of the reference's Levenberg loop is decisive
(relative chi2 difference >= 1e-10, and the long double run takes the same path): see FLOW_MARGIN in tests/test_sim3_gpu.py."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import sim3_reference as ref  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")


def _flow(r):
    return (list(r["iterations"]), list(r["trials"]), list(r["stop_reason"]))


def _flow_margin(r):
    return min([abs(cur - temp) / cur for tr in r["trace"] for cur, temp in tr] or [np.inf])


def main():
    ss = importlib.import_module("orb_slam3-1_amd.synth_sim3")
    p = ss.make_ransac_problem(1201, n=120, inlier=0.5, noise_px=1.0, fix_scale=False, n_hyp=300, min_inliers=15, two_cameras=True)
    r = ref.ransac(p, np.float64)
    np.savez_compressed(os.path.join(GOLDEN, "sim3_ransac_120.npz"), X1c=p["X1c"], X2c=p["X2c"], max_err1=p["max_err1"], max_err2=p["max_err2"],
                        K1=p["K1"], K2=p["K2"], fix_scale=p["fix_scale"], min_inliers=p["min_inliers"], triples=p["triples"],
                        R=r["R"], t=r["t"], s=r["s"], gap=r["gap"],
                        undecided=ref.pack_mask((np.abs(r["r1"] - 1) <= 1e-3) | (np.abs(r["r2"] - 1) <= 1e-3)),
                        count=r["count"], mask=r["mask"], converged=r["converged"], index=r["index"])
    print("ransac: converged %d index %d count %d" % (r["converged"], r["index"], r["count"][r["index"]]))
    for seed in range(100, 200):
        p = ss.make_opt_problem(seed, n=120, outlier_frac=0.1, fix_scale=False, n_unobserved=4, two_cameras=True)
        a, b = ref.optimize_sim3(p, np.float64), ref.optimize_sim3(p, np.longdouble)
        if _flow(a) == _flow(b) and _flow_margin(a) >= 1e-10:
            break
    else:
        raise SystemExit("no stable scene")
    np.savez_compressed(os.path.join(GOLDEN, "sim3_opt_120.npz"), **{k: p[k] for k in ("q", "t", "s", "X1c", "X2c", "obs1", "obs2", "inv_sigma2_1",
                        "inv_sigma2_2", "K1", "K2", "th2", "huber_delta", "fix_scale")},
                        ref_q=a["q"], ref_t=a["t"], ref_s=a["s"], ref_n_in=a["n_in"], ref_n_bad=a["n_bad"], ref_keep=a["keep"],
                        ref_chi2_final=a["chi2_final"], ref_chi2=np.array([float(v) for v in a["chi2"]]), ref_iterations=np.array(a["iterations"]),
                        ref_trials=np.array(a["trials"]), ref_stop_reason=np.array(a["stop_reason"]), ref_flow_margin=_flow_margin(a))
    print("optimise: seed %d flow %s margin %.1e n_in %d n_bad %d" % (seed, _flow(a), _flow_margin(a), a["n_in"], a["n_bad"]))


if __name__ == "__main__":
    main()
