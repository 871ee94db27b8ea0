#!/usr/bin/env python3
"""Writes tests/golden/imu_init_10.npz: the inputs of the case kf10_mono (tests/imuinit_cases.py) and the results of the float64
numpy reference (tests/imuinit_reference.py) on it.  No GPU: neither the library nor a device computes anything here.

    python tools/make_imuinit_golden.py
"""
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

LINK_ARRAYS = ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bias0", "info9")
SCALARS = ("scale", "free_vel", "free_bias", "free_gdir", "free_scale", "prior_g", "prior_a", "huber_delta", "gauss_newton", "lambda_init", "max_iters")


def pack(pr):
    """a problem dictionary as flat arrays"""
    L = pr["links"]
    out = {k: np.asarray(pr[k], np.float64) for k in ("Rwb", "twb", "vel", "bg", "ba", "Rwg")}
    out.update({k: np.float64(pr[k]) for k in SCALARS})
    out["link_kf"] = np.array([[l["kf1"], l["kf2"]] for l in L], np.int32)
    out["link_dT"] = np.array([l["dT"] for l in L], np.float32)
    out["link_robust"] = np.array([l["robust"] for l in L], np.uint8)
    for k in LINK_ARRAYS:
        out["link_" + k] = np.array([np.asarray(l[k]).ravel() for l in L], np.float64 if k == "info9" else np.float32)
    return out


def unpack(g):
    """the problem dictionary of a golden file"""
    pr = {k: g[k] for k in ("Rwb", "twb", "vel", "bg", "ba", "Rwg")}
    pr.update({k: float(g[k]) for k in SCALARS})
    for k in ("free_vel", "free_bias", "free_gdir", "free_scale", "gauss_newton", "max_iters"):
        pr[k] = int(pr[k])
    pr["links"] = [dict(kf1=int(g["link_kf"][l, 0]), kf2=int(g["link_kf"][l, 1]), dT=g["link_dT"][l], robust=g["link_robust"][l],
                        info_gyro=np.zeros((3, 3)), info_acc=np.zeros((3, 3)), **{k: g["link_" + k][l] for k in LINK_ARRAYS})
                   for l in range(len(g["link_kf"]))]
    return pr


def main():
    sy = importlib.import_module("orb_slam3-1_amd.synth_imuinit")
    import imuinit_reference as ref
    from imuinit_cases import CASES
    pr = sy.make_imu_init(**CASES["kf10_mono"])[0]
    r = ref.optimize(pr, np.float64)
    s = r["stats"]
    out = pack(pr)
    out.update(ref_vel=r["vel"], ref_bg=r["bg"], ref_ba=r["ba"], ref_Rwg=r["Rwg"], ref_scale=np.float64(r["scale"]),
               ref_chi2_initial=np.float64(r["chi2_initial"]), ref_chi2_final=np.float64(r["chi2_final"]),
               ref_flow=np.array([s["iterations"], s["trials"], s["stop_reason"]], np.int32))
    path = os.path.join(ROOT, "tests", "golden", "imu_init_10.npz")
    np.savez_compressed(path, **out)
    print("wrote %s (%d bytes): flow %s chi2 %.6g -> %.6g" % (path, os.path.getsize(path), tuple(out["ref_flow"]), r["chi2_initial"], r["chi2_final"]))


if __name__ == "__main__":
    main()
