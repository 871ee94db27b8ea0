"""Seeded whole-map problems for FullInertialBA (reference src/Optimizer.cc:392-811; include/orbslam3_hip_fullba.h), built on
synth.make_inertial_window's trajectory, pre-integrated links and observations.  numpy only.

A problem dictionary has the keys of a LocalInertialBA window plus shared_bias, shared_bg, shared_ba, prior_g, prior_a."""
import copy

import numpy as np

from . import synth


def full_map_from_window(pr, shared_bias, gauge_free=False, permute=False, split=False, lambda_init=1e-5, max_iters=100, prior_g=1e2,
                         prior_a=1e6):
    """A whole-map problem from a LocalInertialBA window (synth.make_inertial_window, or one a test has made harder):
      - every key frame of the window is a vertex; gauge_free frees key frame 0 (pose and IMU states), otherwise it stays fixed;
      - the covisible key frames of the window (pose only, no IMU states) become FREE key frames without IMU;
      - shared_bias: one bias pair for the map, started at the bias of the last key frame with IMU states;
      - split: the middle link is removed, which leaves two trajectories with no link between them;
      - permute: the key frames with IMU states are renumbered newest first and the links reversed.
    Every link keeps its information as the window has it (the link to key frame 0 is the weak one)."""
    pr = copy.deepcopy(pr)
    n_kf = int(pr["n_kf"])
    imu = np.nonzero(np.asarray(pr["has_imu"]))[0]
    pr["pose_fixed"] = np.zeros(n_kf, np.uint8); pr["imu_fixed"] = np.zeros(n_kf, np.uint8)
    if not gauge_free:
        pr["pose_fixed"][0] = 1; pr["imu_fixed"][0] = 1
    if split and len(pr["links"]) > 2:
        del pr["links"][len(pr["links"]) // 2]
    if permute:
        n = len(imu)
        assert (imu == np.arange(n)).all()
        new = np.arange(n_kf); new[:n] = n - 1 - np.arange(n)
        inv = np.argsort(new)
        for k in ("Rwb", "twb", "vel", "bg", "ba", "pose_fixed", "has_imu", "imu_fixed"):
            pr[k] = np.ascontiguousarray(np.asarray(pr[k])[inv])
        pr["edge_kf"] = new[pr["edge_kf"]].astype(np.int32)
        for L in pr["links"]:
            L["kf1"], L["kf2"] = int(new[L["kf1"]]), int(new[L["kf2"]])
        pr["links"] = pr["links"][::-1]
    for L in pr["links"]:
        L["robust"] = np.uint8(1)
    last = int(np.nonzero(np.asarray(pr["has_imu"]))[0][-1])
    pr.update(shared_bias=int(bool(shared_bias)), shared_bg=np.array(pr["bg"][last], np.float64), shared_ba=np.array(pr["ba"][last], np.float64),
              prior_g=float(prior_g) if shared_bias else 0.0, prior_a=float(prior_a) if shared_bias else 0.0,
              lambda_init=float(lambda_init), max_iters=int(max_iters))
    return pr


def make_full_map(seed, n_kf=12, shared_bias=True, gauge_free=False, permute=False, n_no_imu=0, split=False, stereo_frac=0.0, bias_error=0.0,
                  points_per_kf=10, obs_per_point=4, lambda_init=1e-5, max_iters=100, prior_g=1e2, prior_a=1e6):
    """n_kf key frames with IMU states on one trajectory (two with split) and n_no_imu visual-only key frames; returns the problem"""
    w, _ = synth.make_inertial_window(seed, n_opt=n_kf - 1, n_points=points_per_kf * n_kf, obs_per_point=obs_per_point, bias_error=bias_error,
                                      stereo_frac=stereo_frac, n_covisible_fixed=n_no_imu)
    return full_map_from_window(w, shared_bias, gauge_free=gauge_free, permute=permute, split=split, lambda_init=lambda_init, max_iters=max_iters,
                                prior_g=prior_g, prior_a=prior_a)
