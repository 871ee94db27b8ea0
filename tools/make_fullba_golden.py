#!/usr/bin/env python3
"""Writes the two golden files of tests/test_fullba_gpu.py.

  python tools/make_fullba_golden.py reference
      tests/golden/fullba_12.npz: the float64 reference results (tests/fullba_reference.optimize) of one shared-bias and one
      per-key-frame map of 12 key frames (fullba_cases s12_100, k12_100).  CPU only.

  python tools/make_fullba_golden.py parent-bits [--lib PATH] [--out DIR]
      tests/golden/liba_parent_bits.npz: what liba_solve returns on the window of tests/golden/inertial_5kf_120mp.npz and on two
      synthetic windows, and liba_solve_batch on the three together, bit for bit.  Run it on an MI355X with the library of the
      commit whose behaviour is to be pinned (--lib: a liborbslam3_hip.so other than the package's own); the FullInertialBA
      change shares kernels and the window setup with these entry points and must not move a bit of them."""
import argparse
import ctypes
import importlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden")
OUTPUTS = ("Rwb", "twb", "vel", "bg", "ba", "points", "chi2", "depth_positive")
STATS = ("iterations", "trials", "stop_reason", "lambda_", "chi2_initial", "chi2_final")


def parent_windows(synth):
    """the golden window (tools/make_golden.py) and two synthetic ones: 9 free key frames with covisible fixed ones, 3 with a bias error"""
    return [synth.make_inertial_window(45, n_opt=5, n_points=120, obs_per_point=4, stereo_frac=0.3, n_covisible_fixed=2)[0],
            synth.make_inertial_window(46, n_opt=9, n_points=200, obs_per_point=5, stereo_frac=0.5, n_covisible_fixed=3)[0],
            synth.make_inertial_window(47, n_opt=3, n_points=60, obs_per_point=3, bias_error=0.01)[0]]


def flatten(tag, r, out):
    for k in OUTPUTS:
        out["%s_%s" % (tag, k)] = np.asarray(r[k])
    out["%s_stats" % tag] = np.array([float(r["stats"][k]) for k in STATS])


def parent_bits(lib_path, out_dir):
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    except Exception:
        pass
    pkg = importlib.import_module("orb_slam3-1_amd")
    if lib_path:
        pkg.capi.lib = ctypes.CDLL(os.path.abspath(lib_path))
        pkg.capi.lib.orbx_last_error.restype = ctypes.c_char_p
    wins = parent_windows(importlib.import_module("orb_slam3-1_amd.synth"))
    out = {}
    s = pkg.capi.InertialSolver()
    for i, w in enumerate(wins):
        flatten("solve%d" % i, s.solve(w), out)
    s.close()
    b = pkg.capi.LibaBatch()
    for i, r in enumerate(b.solve(wins)):
        flatten("batch%d" % i, r, out)
    b.close()
    os.makedirs(out_dir, exist_ok=True)
    np.savez_compressed(os.path.join(out_dir, "liba_parent_bits.npz"), **out)
    print("liba_parent_bits.npz written from", lib_path or "the package's library")


def reference(out_dir):
    import fullba_cases as C
    out = {}
    for name in ("s12_100", "k12_100"):
        pr, r = C.full_run_of(name)
        for k in ("Rwb", "twb", "vel", "bg", "ba", "points"):
            out["%s_%s" % (name, k)] = np.asarray(r[k], np.float64)
        st = r["stats"]
        out["%s_stats" % name] = np.array([st["iterations"], st["trials"], st["stop_reason"], float(st["lambda_"]), float(r["chi2_initial"]), float(r["chi2_final"])])
    np.savez_compressed(os.path.join(out_dir, "fullba_12.npz"), **out)
    print("fullba_12.npz written")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=["reference", "parent-bits"])
    ap.add_argument("--lib", default=None)
    ap.add_argument("--out", default=OUT, help="directory to write to (default tests/golden)")
    a = ap.parse_args()
    reference(a.out) if a.what == "reference" else parent_bits(a.lib, a.out)
