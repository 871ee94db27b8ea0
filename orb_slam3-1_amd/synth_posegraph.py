"""Seeded essential graphs for the pose-graph solver (EssgProblem of include/orbslam3_hip.h, the graph that
Optimizer::OptimizeEssentialGraph builds, reference src/Optimizer.cc:1517-1726): a trajectory that returns to its start, visual
odometry drift in rotation, translation and scale accumulated along it, spanning-tree, covisibility and old-loop edges measured
between the drifted poses (NonCorrectedSim3 / vScw), a set of key frames around the last one that the loop detection has
already moved onto the start of the trajectory (CorrectedSim3), loop-connection edges between that set and the key frames at the
start, and map points with the index of their reference key frame.  Pure numpy; a similarity is (R, t, s) here and
q xyzw, t, s (Scw) in what is returned.  make_posegraph4dof does the same for the graph of
Optimizer::OptimizeEssentialGraph4DoF (Essg4DofProblem): a gravity-aligned inertial trajectory that drifts in yaw and translation."""
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


def _rz(a):
    c, s = np.cos(a), np.sin(a)
    return np.array([[c, -s, 0.0], [s, c, 0.0], [0.0, 0.0, 1.0]])


def make_posegraph4dof(seed, n=40, n_fixed=1, duplicates=0, n_points=0, n_corrected=5, n_old_loops=None, yaw_drift_deg=0.15,
                       trans_drift=0.01, edge_noise=1.0, consistent=False, float_inputs=False, identity_tcb=True, corrected_scale=1.0,
                       max_iters=20, lambda_init=0.0):
    """The graph of Optimizer::OptimizeEssentialGraph4DoF (Essg4DofProblem of include/orbslam3_hip.h) for an inertial map: n key
    frames whose bodies go round a closed curve with their own small roll and pitch (gravity-aligned: the world's z is up), a drift
    in yaw and translation accumulated along it, and inertial (consecutive), loop and covisibility edges measured between the
    undrifted camera poses with a little noise (edge_noise scales it; consistent=True: none, and the optimum is the ground truth).
    Vertices 0 .. n_fixed-1 are fixed and undrifted, so n_fixed > 1 leaves edges between two fixed vertices in the graph;
    duplicates repeats that many edges.  float_inputs=True gives the vertices as the key-frame constructor of ImuCamPose reads them:
    camera pose and body pose each derived in float from the float Tcw, not consistent to the last bit; otherwise as the Sim3
    constructor computes them in double.  identity_tcb=False uses a camera-body calibration with a rotation and a lever arm.
    The last n_corrected key frames carry corrected_scale in scw (vScw of a CorrectedSim3 entry; the vertex drops it)."""
    rs = np.random.RandomState(9127 + 6007 * seed)
    n_old_loops = n // 12 if n_old_loops is None else n_old_loops
    if identity_tcb:
        Rcb, tcb = np.eye(3), np.zeros(3)
    else:
        Rcb = _rodrigues(np.array([0.02, -0.03, 0.01])) @ np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
        tcb = np.array([0.05, -0.02, 0.1])
    if float_inputs:
        Rcb, tcb = Rcb.astype(np.float32).astype(np.float64), tcb.astype(np.float32).astype(np.float64)

    def camera(Rwb, twb):
        return Rcb @ Rwb.T, Rcb @ (-Rwb.T @ twb) + tcb

    truth_b, drift_b = [], []
    yaw_d, t_d = 0.0, np.zeros(3)
    for i in range(n):
        a = 2 * np.pi * i / n
        Rwb = _rz(a + rs.normal(0, 0.02)) @ _rodrigues(np.append(rs.normal(0, 0.05, 2), 0.0))
        twb = np.array([4.0 * np.sin(a), 4.0 - 4.0 * np.cos(a), 0.3 * np.sin(3 * a)]) + rs.normal(0, 0.02, 3)
        truth_b.append((Rwb, twb))
        if i >= n_fixed and not consistent:
            yaw_d += rs.normal(0, np.deg2rad(yaw_drift_deg)); t_d = t_d + rs.normal(0, trans_drift / np.sqrt(3), 3)
        if consistent and i >= n_fixed:
            dz, dt = _rz(rs.normal(0, 0.01)), rs.normal(0, 0.02, 3)
        else:
            dz, dt = _rz(yaw_d), t_d
        drift_b.append((dz @ Rwb, dz @ twb + dt))
    truth = [camera(*b) for b in truth_b]
    edges, rot, trans = [], [], []

    def add(i, j):
        (Ri, ti), (Rj, tj) = truth[i], truth[j]
        dR, dt = Ri @ Rj.T, ti - Ri @ Rj.T @ tj                                 # Tij = Tiw * Tjw^-1
        if not consistent:
            dR = _rodrigues(rs.normal(0, np.deg2rad(0.02), 3) * edge_noise) @ dR
            dt = dt + rs.normal(0, 0.002, 3) * edge_noise
        edges.append((i, j)); rot.append(dR); trans.append(dt)

    cur = n - 1
    for i in range(max(n - n_corrected, 1), n):                                 # loop connections first
        for j in range(0, min(3, n - n_corrected)):
            if (i, j) == (cur, 0) or rs.uniform() < 0.5:
                add(i, j)
    loops = [(int(i), int(rs.randint(0, max(i - n // 4, 1)))) for i in rs.randint(n // 3, max(n - n_corrected, n // 3 + 1), n_old_loops)]
    for i in range(n):
        if i > 0:
            add(i, i - 1)                                                       # the inertial edge to mPrevKF
        for (a, b) in loops:
            if a == i and b < a:
                add(a, b)                                                       # loop edges of earlier closures
        for k in (2, 3, 4):
            if i - k >= 0 and rs.uniform() < 0.9:
                add(i, i - k)                                                   # covisibility
    for _ in range(duplicates):
        k = int(rs.randint(0, len(edges)))
        edges.append(edges[k]); rot.append(rot[k].copy()); trans.append(trans[k].copy())
    rcw, tcw, rwb, twb, scw = [], [], [], [], []
    for i, (Rwb_i, twb_i) in enumerate(drift_b):
        Rcw_i, tcw_i = camera(Rwb_i, twb_i)
        s = corrected_scale if i >= n - n_corrected else 1.0
        if float_inputs:        # KeyFrame::SetPose: everything in float from the float Tcw
            R32, t32 = Rcw_i.astype(np.float32), tcw_i.astype(np.float32)
            Rwc32 = np.ascontiguousarray(R32.T)
            twc32 = -(Rwc32 @ t32)
            rcw.append(R32.astype(np.float64)); tcw.append(t32.astype(np.float64))
            rwb.append((Rwc32 @ Rcb.astype(np.float32)).astype(np.float64)); twb.append((Rwc32 @ tcb.astype(np.float32) + twc32).astype(np.float64))
            s = 1.0
        else:                   # ImuCamPose(Rwc, twc, pKF) in double
            Rwc, twc = Rcw_i.T, -Rcw_i.T @ tcw_i
            rcw.append(Rwc.T); tcw.append(-Rwc.T @ twc)
            rwb.append(Rwc @ Rcb); twb.append(Rwc @ tcb + twc)
        scw.append(np.concatenate([_quat_from_R(rcw[-1]), s * tcw[-1], [s]]))
    scw = np.stack(scw)
    fixed = np.zeros(n, np.uint8)
    fixed[:n_fixed] = 1
    pts = np.zeros((n_points, 3), np.float32)
    ref = rs.randint(0, n, n_points).astype(np.int32)
    for k in range(n_points):
        Xc = np.array([rs.uniform(-2, 2), rs.uniform(-1, 1), rs.uniform(2, 8)])
        pts[k] = rcw[ref[k]].T @ (Xc - scw[ref[k], 4:7]) / scw[ref[k], 7]
    A = lambda v: np.ascontiguousarray(np.stack(v))
    return dict(rcw=A(rcw), tcw=A(tcw), rwb=A(rwb), twb=A(twb), rcb=A([Rcb] * n), tcb=A([tcb] * n), fixed=fixed,
                edge_vertices=np.ascontiguousarray(np.array(edges, np.int32).reshape(-1, 2)), edge_rot=A(rot), edge_trans=A(trans),
                information=np.diag([1e3, 1e3, 1.0, 1.0, 1.0, 1.0]), max_iters=int(max_iters), lambda_init=float(lambda_init),
                points=pts, point_ref=ref, scw=scw, truth_rcw=A([t[0] for t in truth]), truth_tcw=A([t[1] for t in truth]))
