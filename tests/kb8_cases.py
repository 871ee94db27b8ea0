"""What the KannalaBrandt8 GPU tests share: the golden fixtures as problem dictionaries.  A test helper, not a test."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SOLVER_FACTOR = 4.0     # the device may be 4 S from the unperturbed reference run (tools/make_kb8_golden.py)


def _camera(g):
    c = g["kb8"]
    return dict(fx=float(c[0]), fy=float(c[1]), cx=float(c[2]), cy=float(c[3]), k=[float(v) for v in c[4:8]])


def pose_fixture():
    g = np.load(os.path.join(GOLDEN, "kb8_pose_mono_60.npz"))
    cam = _camera(g)
    w = dict(q=g["q"], t=g["t"], Xw=g["Xw"], obs=g["obs"], inv_sigma2=g["inv_sigma2"], stereo=g["stereo"], huber_mono=float(g["huber_mono"]),
             huber_stereo=float(g["huber_stereo"]), fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], bf=0.0)
    return w, cam, g


def lba_fixture():
    g = np.load(os.path.join(GOLDEN, "kb8_lba_4kf_40mp.npz"))
    cam = _camera(g)
    w = {k: g[k] for k in ("pose_q", "pose_t", "pose_fixed", "points", "edge_point", "edge_pose", "edge_obs", "edge_inv_sigma2", "edge_stereo")}
    w.update(huber_mono=float(g["huber_mono"]), huber_stereo=float(g["huber_stereo"]), fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], bf=0.0)
    return w, cam, g


def same_bits(a, b, keys):
    for k in keys:
        np.testing.assert_array_equal(np.asarray(a[k]), np.asarray(b[k]), err_msg=k)
