"""Seeded scenes for the KannalaBrandt8 (fisheye) camera: camera-frame points for orbx_kb8_project, one monocular frame for
pose_optimize and a LocalBA window of monocular edges for lba_solve.  The dictionaries carry the fields of synth.make_pose_problem /
synth.make_ba_window (so the same geometry also runs with the pinhole camera, which the timing tool does) plus `kb8`, the camera
for the *_set_camera_kb8 calls.  Inputs are rounded through float32 where the reference holds floats.
The *_rig functions build the same for a rig of two fisheye cameras (`rig`, for the *_set_rig_kb8 calls): every map point is seen
by the left camera, the right camera or both, and the stereo byte of an edge names its camera (0 left, EDGE_RIGHT right)."""
import numpy as np

from .synth import _quat_from_R, _rodrigues


def _f32(a):
    return np.asarray(a, np.float64).astype(np.float32).astype(np.float64)


def tumvi_camera():
    """parameters like those of the TUM-VI sequences (512 x 512 fisheye), floats promoted to double like mvParameters"""
    fx, fy, cx, cy = (float(np.float32(v)) for v in (190.98, 190.97, 254.93, 256.90))
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, k=[float(np.float32(v)) for v in (0.0034, 0.0007, -0.0020, 0.0002)])


def project_exact(cam, Xc):
    """the KB8 projection in float64 throughout (the generator's ground truth; not the reference's float arctangents)"""
    Xc = np.asarray(Xc, np.float64)
    x, y, z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    theta = np.arctan2(np.sqrt(x * x + y * y), z)
    psi = np.arctan2(y, x)
    k = cam["k"]
    t2 = theta * theta
    r = theta * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    return np.stack([cam["fx"] * r * np.cos(psi) + cam["cx"], cam["fy"] * r * np.sin(psi) + cam["cy"]], -1)


def make_camera_points(seed, n, min_deg=0.5, max_deg=85.0, depth=(0.3, 30.0), floor=0.01):
    """n camera-frame points min_deg .. max_deg off the optical axis at depths (z) depth[0] .. depth[1], with
    sqrt(x^2 + y^2) >= floor * z: the reference's projectJac divides by that radius and is singular on the axis"""
    rs = np.random.RandomState(4100 + seed)
    lo = max(np.deg2rad(min_deg), np.arctan(floor) * (1 + 1e-9))
    th = rs.uniform(lo, np.deg2rad(max_deg), n)
    ph = rs.uniform(-np.pi, np.pi, n)
    z = np.exp(rs.uniform(np.log(depth[0]), np.log(depth[1]), n))
    rad = z * np.tan(th)
    X = np.stack([rad * np.cos(ph), rad * np.sin(ph), z], 1)
    assert (np.hypot(X[:, 0], X[:, 1]) >= floor * X[:, 2]).all()
    return X


def _directions(rs, n, max_deg, depth):
    th = rs.uniform(np.deg2rad(2.0), np.deg2rad(max_deg), n)
    ph = rs.uniform(-np.pi, np.pi, n)
    d = rs.uniform(depth[0], depth[1], n)              # distance along the ray: points near 80 degrees stay at a finite range
    return np.stack([d * np.sin(th) * np.cos(ph), d * np.sin(th) * np.sin(ph), d * np.cos(th)], 1)


def make_pose_problem_kb8(seed, n=60, n_outliers=9, noise_px=0.5, max_deg=80.0, cam=None):
    """one monocular fisheye frame: n map points up to max_deg off axis, n_outliers gross mismatches, noise on the rest"""
    rs = np.random.RandomState(4200 + seed)
    cam = cam or tumvi_camera()
    R = _rodrigues(rs.normal(0, 0.2, 3))
    t = rs.normal(0, 0.5, 3)
    Xc = _directions(rs, n, max_deg, (1.0, 8.0))
    Xw = _f32((Xc - t) @ R)                             # Xc = R Xw + t
    octave = rs.randint(0, 4, n)
    sig = 1.2 ** octave
    obs = project_exact(cam, Xw @ R.T + t) + rs.normal(0, noise_px, (n, 2)) * sig[:, None]
    is_outlier = np.zeros(n, bool)
    is_outlier[rs.choice(n, n_outliers, replace=False)] = True
    ang = rs.uniform(-np.pi, np.pi, n)
    obs[is_outlier] += (rs.uniform(25, 60, n)[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1))[is_outlier]
    dR = _rodrigues(rs.normal(0, np.deg2rad(1.0), 3))
    R0, t0 = dR @ R, dR @ t + rs.normal(0, 0.03, 3)
    obs3 = np.concatenate([_f32(obs), -np.ones((n, 1))], 1)
    return dict(q=_f32(_quat_from_R(R0)), t=_f32(t0), Xw=np.ascontiguousarray(Xw), obs=np.ascontiguousarray(obs3),
                inv_sigma2=_f32(1.0 / sig ** 2), stereo=np.zeros(n, np.uint8), is_outlier=is_outlier,
                fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], bf=0.0,
                huber_mono=float(np.float32(np.sqrt(5.991))), huber_stereo=float(np.float32(np.sqrt(7.815))), kb8=cam)


def perturbed_frame(w, seed):
    """the same frame from another initial pose (the other members of a batch)"""
    rs = np.random.RandomState(4300 + seed)
    w = dict(w)
    w["q"] = _f32(np.asarray(w["q"]) + rs.normal(0, 2e-3, 4))
    w["t"] = _f32(np.asarray(w["t"]) + rs.normal(0, 0.01, 3))
    return w


def make_ba_window_kb8(seed, n_kf=4, n_fixed=2, n_points=40, obs_per_point=None, n_outliers=6, noise_px=0.5, max_deg=75.0, drop_frac=0.0, cam=None):
    """a LocalBA window of monocular fisheye key frames: the last n_fixed poses are fixed, every point is seen by obs_per_point
    key frames (all of them by default) where it lies inside max_deg of the axis and in front of the camera; drop_frac of the
    points lose one of those observations (a point keeps two at least)"""
    rs = np.random.RandomState(4400 + seed)
    cam = cam or tumvi_camera()
    obs_per_point = obs_per_point or n_kf
    Rs, ts = [], []
    for i in range(n_kf):
        c = np.array([0.25 * i, 0.05 * np.sin(1.7 * i), 0.08 * np.cos(0.9 * i)])
        Rcw = _rodrigues(np.array([0.03 * np.sin(1.3 * i), 0.05 * np.cos(0.7 * i) + 0.02 * i, 0.02 * i])).T
        Rs.append(Rcw); ts.append(-Rcw @ c)
    Rs, ts = np.array(Rs), np.array(ts)
    mid = n_kf // 2
    Xc = _directions(rs, n_points, max_deg * 0.8, (2.0, 10.0))
    pts = (Xc - ts[mid]) @ Rs[mid]
    e = dict(pt=[], pose=[], obs=[], w=[])
    for l in range(n_points):
        Xl = Rs @ pts[l] + ts
        off = np.degrees(np.arctan2(np.hypot(Xl[:, 0], Xl[:, 1]), Xl[:, 2]))
        seen = [i for i in rs.permutation(n_kf) if off[i] < max_deg and off[i] > 1.0][:obs_per_point]
        if len(seen) > 2 and rs.uniform() < drop_frac:
            seen = seen[:-1]
        for ip in sorted(seen):
            sig = 1.2 ** int(rs.randint(0, 3))
            uv = project_exact(cam, Xl[ip]) + rs.normal(0, noise_px * sig, 2)
            e["pt"].append(l); e["pose"].append(int(ip)); e["obs"].append([uv[0], uv[1], -1.0]); e["w"].append(1.0 / sig ** 2)
    obs = np.array(e["obs"])
    bad = rs.choice(len(obs), n_outliers, replace=False)
    ang = rs.uniform(-np.pi, np.pi, len(bad))
    obs[bad, :2] += rs.uniform(25, 60, len(bad))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    is_outlier = np.zeros(len(obs), bool); is_outlier[bad] = True
    fixed = np.zeros(n_kf, np.uint8); fixed[n_kf - n_fixed:] = 1
    q0 = np.zeros((n_kf, 4)); t0 = np.zeros((n_kf, 3))
    for i in range(n_kf):
        R, t = Rs[i], ts[i]
        if not fixed[i]:
            dR = _rodrigues(rs.normal(0, np.deg2rad(0.5), 3))
            R, t = dR @ R, dR @ t + rs.normal(0, 0.01, 3)
        q0[i] = _quat_from_R(R); t0[i] = t
    return dict(pose_q=_f32(q0), pose_t=_f32(t0), pose_fixed=fixed, points=_f32(pts + rs.normal(0, 0.03, pts.shape)),
                edge_point=np.asarray(e["pt"], np.int32), edge_pose=np.asarray(e["pose"], np.int32), edge_obs=_f32(obs),
                edge_inv_sigma2=_f32(e["w"]), edge_stereo=np.zeros(len(obs), np.uint8), is_outlier=is_outlier,
                fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], bf=0.0,
                huber_mono=float(np.float32(np.sqrt(5.991))), huber_stereo=float(np.float32(np.sqrt(7.815))), kb8=cam)


# ------------------------------------------------------------------------------------------------ a rig of two fisheye cameras
EDGE_RIGHT = 2      # ORBX_EDGE_RIGHT of include/orbslam3_hip_kb8.h


def make_rig():
    """left = tumvi_camera(); a right camera whose every parameter differs visibly (swapping the two moves a projection by pixels);
    Trl = a 0.10 m baseline and 3 degrees about a skew axis (dropping R_rl from a Jacobian is a wrong Jacobian).  q_rl (xyzw) and
    t_rl pass through float32 like the Sophus::SE3f the reference keeps."""
    f = lambda v: float(np.float32(v))
    right = dict(fx=f(189.40), fy=f(189.35), cx=f(252.10), cy=f(259.30), k=[f(v) for v in (0.0030, 0.0011, -0.0017, 0.00015)])
    axis = np.array([0.4, 0.8, 0.45])
    R_rl = _rodrigues(np.deg2rad(3.0) * axis / np.linalg.norm(axis))
    c_right = np.array([0.10, -0.003, 0.002])          # the right camera's centre in the left camera's frame
    return dict(left=tumvi_camera(), right=right, q_rl=_f32(_quat_from_R(R_rl)), t_rl=_f32(-R_rl @ c_right))


def rig_R_t(rig):
    """(R_rl, t_rl) in float64 from the rig's (normalised) quaternion"""
    x, y, z, w = np.asarray(rig["q_rl"], np.float64) / np.linalg.norm(rig["q_rl"])
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return R, np.asarray(rig["t_rl"], np.float64)


def _off_axis_deg(X):
    return np.degrees(np.arctan2(np.hypot(X[..., 0], X[..., 1]), X[..., 2]))


def _plant_outliers(rs, obs, kind, n_outliers):
    """gross mismatches in both cameras: half of them (rounded up) on left edges, the rest on right edges"""
    left, right = np.nonzero(kind == 0)[0], np.nonzero(kind != 0)[0]
    n_l = min((n_outliers + 1) // 2, len(left)) if len(right) else n_outliers
    bad = np.concatenate([rs.choice(left, n_l, replace=False), rs.choice(right, n_outliers - n_l, replace=False)]).astype(int)
    ang = rs.uniform(-np.pi, np.pi, len(bad))
    obs[bad, :2] += rs.uniform(25, 60, len(bad))[:, None] * np.stack([np.cos(ang), np.sin(ang)], 1)
    is_outlier = np.zeros(len(obs), bool); is_outlier[bad] = True
    return is_outlier


def make_pose_problem_rig(seed, n=60, n_outliers=9, noise_px=0.5, max_deg=75.0, rig=None):
    """one frame of a two-camera fisheye rig with n edges: about a third of the map points are seen by the left camera only, a third
    by the right camera only and a third by both (two edges on one point, as a rig frame holds a matched point at i < Nleft and at
    i >= Nleft); the edges are shuffled, so that left and right ones meet in every wave.  obs[:, :2] of a right edge is the key
    point in the right image."""
    rs = np.random.RandomState(4600 + seed)
    rig = rig or make_rig()
    R_rl, t_rl = rig_R_t(rig)
    R = _rodrigues(rs.normal(0, 0.2, 3))
    t = rs.normal(0, 0.5, 3)
    pts, kinds = [], []             # per edge: the point in the left camera's frame, the camera
    while len(kinds) < n:
        X = _directions(rs, 1, max_deg, (1.0, 8.0))[0]
        off_r = _off_axis_deg(R_rl @ X + t_rl)
        cls = int(rs.randint(0, 3))                     # 0 left only, 1 right only, 2 both
        if cls != 0 and not (1.0 < off_r < max_deg + 5.0):
            continue
        if cls == 2 and len(kinds) + 2 > n:
            cls = 0
        for k in ([0], [EDGE_RIGHT], [0, EDGE_RIGHT])[cls]:
            pts.append(X); kinds.append(k)
    order = rs.permutation(n)
    Xc = np.array(pts)[order]; kind = np.array(kinds, np.uint8)[order]
    Xw = _f32((Xc - t) @ R)
    octave = rs.randint(0, 4, n)
    sig = 1.2 ** octave
    Xl = Xw @ R.T + t
    uv = np.where((kind != 0)[:, None], project_exact(rig["right"], Xl @ R_rl.T + t_rl), project_exact(rig["left"], Xl))
    obs = uv + rs.normal(0, noise_px, (n, 2)) * sig[:, None]
    is_outlier = _plant_outliers(rs, obs, kind, n_outliers)
    dR = _rodrigues(rs.normal(0, np.deg2rad(1.0), 3))
    R0, t0 = dR @ R, dR @ t + rs.normal(0, 0.03, 3)
    obs3 = np.concatenate([_f32(obs), -np.ones((n, 1))], 1)
    cam = rig["left"]
    return dict(q=_f32(_quat_from_R(R0)), t=_f32(t0), Xw=np.ascontiguousarray(Xw), obs=np.ascontiguousarray(obs3),
                inv_sigma2=_f32(1.0 / sig ** 2), stereo=kind, is_outlier=is_outlier,
                fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], bf=0.0,
                huber_mono=float(np.float32(np.sqrt(5.991))), huber_stereo=float(np.float32(np.sqrt(7.815))), rig=rig)


def make_ba_window_rig(seed, n_kf=4, n_fixed=2, n_points=40, obs_per_point=None, n_outliers=6, noise_px=0.5, max_deg=75.0, drop_frac=0.0, rig=None, one_edge=False):
    """a LocalBA window of rig key frames, the geometry of make_ba_window_kb8: every observation of a point by a key frame is a left
    edge, a right edge or a left edge followed by a right edge on the same (key frame, point) pair, a third each, in the order
    LocalBundleAdjustment adds them.  one_edge: every observation is a left edge or a right edge, half each (the edge count is then
    that of make_ba_window_kb8 with the same arguments, which the timing tool wants)"""
    rs = np.random.RandomState(4700 + seed)
    rig = rig or make_rig()
    R_rl, t_rl = rig_R_t(rig)
    obs_per_point = obs_per_point or n_kf
    Rs, ts = [], []
    for i in range(n_kf):
        c = np.array([0.25 * i, 0.05 * np.sin(1.7 * i), 0.08 * np.cos(0.9 * i)])
        Rcw = _rodrigues(np.array([0.03 * np.sin(1.3 * i), 0.05 * np.cos(0.7 * i) + 0.02 * i, 0.02 * i])).T
        Rs.append(Rcw); ts.append(-Rcw @ c)
    Rs, ts = np.array(Rs), np.array(ts)
    mid = n_kf // 2
    Xc = _directions(rs, n_points, max_deg * 0.8, (2.0, 10.0))
    pts = (Xc - ts[mid]) @ Rs[mid]
    e = dict(pt=[], pose=[], obs=[], w=[], kind=[])
    for l in range(n_points):
        Xl = Rs @ pts[l] + ts
        Xr = Xl @ R_rl.T + t_rl
        off, off_r = _off_axis_deg(Xl), _off_axis_deg(Xr)
        seen = [i for i in rs.permutation(n_kf) if 1.0 < off[i] < max_deg and 1.0 < off_r[i] < max_deg][:obs_per_point]
        if len(seen) > 2 and rs.uniform() < drop_frac:
            seen = seen[:-1]
        for ip in sorted(seen):
            for k in ([0], [EDGE_RIGHT], [0, EDGE_RIGHT])[int(rs.randint(0, 2 if one_edge else 3))]:
                sig = 1.2 ** int(rs.randint(0, 3))
                uv = (project_exact(rig["right"], Xr[ip]) if k else project_exact(rig["left"], Xl[ip])) + rs.normal(0, noise_px * sig, 2)
                e["pt"].append(l); e["pose"].append(int(ip)); e["obs"].append([uv[0], uv[1], -1.0]); e["w"].append(1.0 / sig ** 2); e["kind"].append(k)
    obs = np.array(e["obs"])
    kind = np.asarray(e["kind"], np.uint8)
    is_outlier = _plant_outliers(rs, obs, kind, n_outliers)
    fixed = np.zeros(n_kf, np.uint8); fixed[n_kf - n_fixed:] = 1
    q0 = np.zeros((n_kf, 4)); t0 = np.zeros((n_kf, 3))
    for i in range(n_kf):
        R, t = Rs[i], ts[i]
        if not fixed[i]:
            dR = _rodrigues(rs.normal(0, np.deg2rad(0.5), 3))
            R, t = dR @ R, dR @ t + rs.normal(0, 0.01, 3)
        q0[i] = _quat_from_R(R); t0[i] = t
    cam = rig["left"]
    return dict(pose_q=_f32(q0), pose_t=_f32(t0), pose_fixed=fixed, points=_f32(pts + rs.normal(0, 0.03, pts.shape)),
                edge_point=np.asarray(e["pt"], np.int32), edge_pose=np.asarray(e["pose"], np.int32), edge_obs=_f32(obs),
                edge_inv_sigma2=_f32(e["w"]), edge_stereo=kind, is_outlier=is_outlier,
                fx=cam["fx"], fy=cam["fy"], cx=cam["cx"], cy=cam["cy"], bf=0.0,
                huber_mono=float(np.float32(np.sqrt(5.991))), huber_stereo=float(np.float32(np.sqrt(7.815))), rig=rig)
