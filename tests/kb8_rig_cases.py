"""What the two-camera KannalaBrandt8 GPU tests share: the golden fixtures of tools/make_kb8_rig_golden.py as problem dictionaries
and rigs.  A test helper, not a test."""
import os

import numpy as np

from kb8_cases import SOLVER_FACTOR, same_bits      # noqa: F401  (4 S, as for the monocular camera)

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ERR_ARG = -3            # ORBX_ERR_ARG
EDGE_RIGHT = 2          # ORBX_EDGE_RIGHT


def _camera(c):
    return dict(fx=float(c[0]), fy=float(c[1]), cx=float(c[2]), cy=float(c[3]), k=[float(v) for v in c[4:8]])


def rig_of(g):
    return dict(left=_camera(g["rig_left"]), right=_camera(g["rig_right"]), q_rl=g["rig_q_rl"].copy(), t_rl=g["rig_t_rl"].copy())


def pose_fixture(n_edges=60):
    """(problem, rig, fixture) of kb8_rig_pose_60.npz or kb8_rig_pose_560.npz"""
    g = np.load(os.path.join(GOLDEN, "kb8_rig_pose_%d.npz" % n_edges))
    rig = rig_of(g)
    cam = rig["left"]
    w = dict(q=g["q"], t=g["t"], Xw=g["Xw"], obs=g["obs"], inv_sigma2=g["inv_sigma2"], stereo=g["stereo"], huber_mono=float(g["huber_mono"]),
             huber_stereo=float(g["huber_stereo"]), fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], bf=0.0)
    return w, rig, g


def lba_fixture():
    g = np.load(os.path.join(GOLDEN, "kb8_rig_lba_4kf_40mp.npz"))
    rig = rig_of(g)
    cam = rig["left"]
    w = {k: g[k] for k in ("pose_q", "pose_t", "pose_fixed", "points", "edge_point", "edge_pose", "edge_obs", "edge_inv_sigma2", "edge_stereo")}
    w.update(huber_mono=float(g["huber_mono"]), huber_stereo=float(g["huber_stereo"]), fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], bf=0.0)
    return w, rig, g


def all_left(w, key):
    """the same problem with every edge on the left camera"""
    w = dict(w)
    w[key] = np.zeros_like(w[key])
    return w


def with_kind(w, key, edge, kind):
    w = dict(w)
    w[key] = w[key].copy()
    w[key][edge] = kind
    return w
