"""Seeded essential graphs for the pose-graph solver (EssgProblem of include/orbslam3_hip.h, the graph that
Optimizer::OptimizeEssentialGraph builds, reference src/Optimizer.cc:1517-1726): a trajectory that returns to its start, visual
odometry drift in rotation, translation and scale accumulated along it, spanning-tree, covisibility and old-loop edges measured
between the drifted poses (NonCorrectedSim3 / vScw), a set of key frames around the last one that the loop detection has
already moved onto the start of the trajectory (CorrectedSim3), loop-connection edges between that set and the key frames at the
start, and map points with the index of their reference key frame.  Pure numpy; a similarity is (R, t, s) here and
q xyzw, t, s (Scw) in what is returned."""
import numpy as np

from .synth import _quat_from_R, _rodrigues


def _mul(a, b):
    return a[0] @ b[0], a[2] * (a[0] @ b[1]) + a[1], a[2] * b[2]


def _inv(a):
    return a[0].T, -(a[0].T @ a[1]) / a[2], 1.0 / a[2]


def _pack(S):
    return np.concatenate([_quat_from_R(S[0]), S[1], [S[2]]])


def make_posegraph(seed, n=60, fix_scale=False, n_fixed=1, duplicates=0, n_points=0, n_corrected=5, n_old_loops=None,
                   rot_drift_deg=0.15, trans_drift=0.01, scale_drift=0.004, loop_noise=1.0, consistent=False, max_iters=20):
    """n key frames on a closed curve, about five edges per key frame.  Vertices 0 .. n_fixed-1 are fixed (n_fixed = 1 is the
    loop overload with the map's first key frame; more is the merge overload, whose edges between two fixed vertices stay in the
    graph).  duplicates repeats that many edges (the reference suppresses a repeated pair only between loop connections and
    covisibility edges).  consistent=True is the self-check variant: every measurement comes from the ground truth and the
    estimates are the ground truth moved a little, so the optimum is the ground truth itself and its chi2 is zero."""
    rs = np.random.RandomState(4243 + 7919 * seed)
    n_old_loops = n // 12 if n_old_loops is None else n_old_loops
    truth = []
    for i in range(n):
        a = 2 * np.pi * i / n
        Rwc = _rodrigues(np.array([0.0, a, 0.0])) @ _rodrigues(rs.normal(0, 0.02, 3))
        c = np.array([4.0 * np.sin(a), 0.3 * np.sin(3 * a), 4.0 - 4.0 * np.cos(a)]) + rs.normal(0, 0.02, 3)
        truth.append((Rwc.T, -Rwc.T @ c, 1.0))                                   # Tcw
    if consistent:
        drifted = truth
    else:
        drifted = [truth[0]]
        for i in range(1, n):
            rel = _mul(truth[i], _inv(truth[i - 1]))
            d = (_rodrigues(rs.normal(0, np.deg2rad(rot_drift_deg) / np.sqrt(3), 3)), rs.normal(0, trans_drift / np.sqrt(3), 3),
                 1.0 if fix_scale else float(np.exp(rs.normal(0, scale_drift))))
            drifted.append(_mul(_mul(d, rel), drifted[i - 1]))
    # the corrected set: the last n_corrected key frames, moved rigidly with the current key frame onto its loop match
    est = list(drifted)
    cur = n - 1
    if consistent:
        for i in range(n_fixed, n):
            d = (_rodrigues(rs.normal(0, 0.01, 3)), rs.normal(0, 0.02, 3), 1.0 if fix_scale else float(np.exp(rs.normal(0, 0.01))))
            est[i] = _mul(d, truth[i])
    else:
        noise = (_rodrigues(rs.normal(0, np.deg2rad(0.05), 3) * loop_noise), rs.normal(0, 0.003, 3) * loop_noise,
                 1.0 if fix_scale else float(np.exp(rs.normal(0, 0.002) * loop_noise)))
        cur_corrected = _mul(_mul(noise, _mul(truth[cur], _inv(truth[0]))), drifted[0])
        for i in range(n - n_corrected, n):
            est[i] = _mul(_mul(drifted[i], _inv(drifted[cur])), cur_corrected)
    edges, meas = [], []

    def add(i, j, from_estimate=False):
        src = est if (from_estimate and not consistent) else drifted
        edges.append((i, j))
        meas.append(_pack(_mul(src[j], _inv(src[i]))))                          # Sji = Sjw * Swi

    # loop connections first, as the reference adds them: corrected key frames to the key frames at the start, from vScw
    for i in range(n - n_corrected, n):
        for j in range(0, min(3, n - n_corrected)):
            if (i, j) == (cur, 0) or rs.uniform() < 0.5:
                add(i, j, from_estimate=True)
    loops = [(int(i), int(rs.randint(0, max(i - n // 4, 1)))) for i in rs.randint(n // 3, max(n - n_corrected, n // 3 + 1), n_old_loops)]
    for i in range(n):
        if i > 0:
            add(i, i - 1)                                                       # spanning tree: the parent
        for (a, b) in loops:
            if a == i and b < a:
                add(a, b)                                                       # loop edges of earlier closures
        for k in (2, 3, 4, 5):
            if i - k >= 0 and rs.uniform() < 0.9:
                add(i, i - k)                                                   # covisibility
    for _ in range(duplicates):
        k = int(rs.randint(0, len(edges)))
        edges.append(edges[k]); meas.append(meas[k].copy())
    fixed = np.zeros(n, np.uint8)
    fixed[:n_fixed] = 1
    pts = np.zeros((n_points, 3), np.float32)
    ref = rs.randint(0, n, n_points).astype(np.int32)
    for k in range(n_points):
        Xc = np.array([rs.uniform(-2, 2), rs.uniform(-1, 1), rs.uniform(2, 8)])
        S = est[ref[k]]
        pts[k] = S[0].T @ (Xc - S[1]) / S[2]
    return dict(sim3=np.ascontiguousarray(np.stack([_pack(S) for S in est])), fixed=fixed,
                edge_vertices=np.ascontiguousarray(np.array(edges, np.int32).reshape(-1, 2)),
                edge_measurement=np.ascontiguousarray(np.stack(meas)), fix_scale=int(fix_scale), max_iters=int(max_iters), lambda_init=1e-16,
                points=pts, point_ref=ref, truth=np.stack([_pack(S) for S in truth]))
