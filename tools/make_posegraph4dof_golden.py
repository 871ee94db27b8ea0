"""Writes tests/golden/posegraph4dof_40.npz: one seeded 4-DoF essential graph (orb_slam3-1_amd/synth_posegraph.py, the case
loop40_cap2 of tests/posegraph4dof_cases.py) plus the outputs of the numpy reference (tests/posegraph4dof_reference.py, float64)
on it, so that the tests do not depend on the generator's RNG stream.  Needs the built library only because the package loads it;
no GPU."""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]
import posegraph4dof_reference as ref  # noqa: E402
from posegraph4dof_cases import CASES  # noqa: E402

KEYS = ("rcw", "tcw", "rwb", "twb", "rcb", "tcb", "fixed", "edge_vertices", "edge_rot", "edge_trans", "information", "max_iters", "lambda_init",
        "points", "point_ref", "scw")


def main():
    sp = importlib.import_module("orb_slam3-1_amd.synth_posegraph")
    p = sp.make_posegraph4dof(**CASES["loop40_cap2"])
    a, b = ref.optimize(p, np.float64), ref.optimize(p, np.longdouble)
    flow = lambda r: (r["stats"]["iterations"], r["stats"]["trials"], r["stats"]["stop_reason"])
    assert flow(a) == flow(b)
    st = a["stats"]
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "posegraph4dof_40.npz"), **{k: p[k] for k in KEYS},
                        ref_rcw=a["rcw_out"], ref_tcw=a["tcw_out"], ref_pose_q=a["pose_q"], ref_pose_t=a["pose_t"], ref_points=a["points_out"],
                        ref_flow=np.array(flow(a)), ref_chi2_initial=float(st["chi2_initial"]), ref_chi2_final=float(st["chi2_final"]),
                        ref_lambda_0=float(st["lambda_0"]), ref_flow_margin=a["flow_margin"])
    print("posegraph4dof_40: %d edges, flow %s, chi2 %.6g -> %.6g, lambda_0 %.6g, margin %.1e" % (
        len(p["edge_vertices"]), flow(a), st["chi2_initial"], st["chi2_final"], st["lambda_0"], a["flow_margin"]))


if __name__ == "__main__":
    main()
