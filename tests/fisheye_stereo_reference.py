"""Numpy restatement of Frame::ComputeStereoFishEyeMatches for a two-camera KannalaBrandt8 rig.  A test helper, not a test.

Restated from the reference text (read as text; nothing copied):
  src/Frame.cc:1246-1286                          knnMatch(left lapping, right lapping, 2), Lowe's ratio, write-back
  src/CameraModels/KannalaBrandt8.cpp:116-143     unproject: Newton on theta, at most 10 steps, tan(theta) / theta_d
  src/CameraModels/KannalaBrandt8.cpp:67-93       project(Vector3f)
  src/CameraModels/KannalaBrandt8.cpp:394-406     Triangulate: the null vector of a 4x4
  src/CameraModels/KannalaBrandt8.cpp:306-375     TriangulateMatches: the codes -1 .. -5 or z1

Two evaluations of the geometry, chosen by `dtype`:
  faithful (numpy.float32)  float32 at every point the C++ stores a float, double where the C++ compares in double; the null vector
                            from numpy.linalg.svd of the float32 matrix.  tan / atan2 / sin / cos are the float rounding of the
                            float64 function (a correctly rounded model of libm's float functions, which are within one ulp).
  exact (numpy.float64)     everything in float64.

A rig is dict(left=cam, right=cam, precision_l, precision_r, Rlr (3, 3), tlr (3,)), cam = dict(fx, fy, cx, cy, k[4]) -- values
that are floats."""
import numpy as np

FAITHFUL, EXACT = np.float32, np.float64
COS_LIMIT, CHI2, MIN_DEPTH = 0.9998, 5.991, np.float32(0.0001)


def ratio_ok(d0, d1):
    """(*it)[0].distance < (*it)[1].distance * 0.7: cv::DMatch::distance is a float, 0.7 a double"""
    return np.asarray(d0, np.float32).astype(np.float64) < np.asarray(d1, np.float32).astype(np.float64) * 0.7


def hamming_matrix(a, b):
    """(n, 32) x (m, 32) uint8 -> (n, m) Hamming distances"""
    A = np.unpackbits(np.asarray(a, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    B = np.unpackbits(np.asarray(b, np.uint8).reshape(-1, 32), axis=1).astype(np.int32)
    return A.sum(1)[:, None] + B.sum(1)[None, :] - 2 * (A @ B.T)


def knn2(desc_l, desc_r):
    """per left descriptor: d0, d1 (-1 where there is no first / second neighbour), the index of the best, and whether it passes"""
    n, m = len(desc_l), len(desc_r)
    d0 = np.full(n, -1, np.int32); d1 = np.full(n, -1, np.int32); idx = np.full(n, -1, np.int32)
    if n == 0 or m == 0:
        return d0, d1, idx, np.zeros(n, bool)
    D = hamming_matrix(desc_l, desc_r)
    idx = D.argmin(1).astype(np.int32)
    d0 = D[np.arange(n), idx].astype(np.int32)
    if m < 2:
        return d0, d1, idx, np.zeros(n, bool)
    D2 = D.copy()
    D2[np.arange(n), idx] = 1 << 20
    d1 = D2.min(1).astype(np.int32)
    return d0, d1, idx, ratio_ok(d0, d1)


def _cam(cam, precision, T):
    return [T(cam[k]) for k in ("fx", "fy", "cx", "cy")] + [T(v) for v in cam["k"]] + [T(precision)]


def _fn(f, T, *args):
    """a transcendental: the `T` rounding of the float64 function of the arguments"""
    return f(*[np.asarray(a, T).astype(np.float64) for a in args]).astype(T)


def unproject(cam, precision, uv, T):
    fx, fy, cx, cy, k0, k1, k2, k3, prec = _cam(cam, precision, T)
    uv = np.asarray(uv, T)
    pwx, pwy = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
    theta_d = np.sqrt(pwx * pwx + pwy * pwy)
    half_pi = T(np.pi / 2)
    theta_d = np.minimum(np.maximum(-half_pi, theta_d), half_pi)
    theta = theta_d.copy()
    live = theta_d.astype(np.float64) > 1e-8
    run = live.copy()
    one = T(1)
    for _ in range(10):
        theta2 = theta * theta; theta4 = theta2 * theta2; theta6 = theta4 * theta2; theta8 = theta4 * theta4
        a, b, c, d = k0 * theta2, k1 * theta4, k2 * theta6, k3 * theta8
        fix = (theta * (one + a + b + c + d) - theta_d) / (one + T(3) * a + T(5) * b + T(7) * c + T(9) * d)
        theta = np.where(run, theta - fix, theta)
        run = run & ~(np.abs(fix) < prec)
    with np.errstate(divide="ignore", invalid="ignore"):
        scale = np.where(live, _fn(np.tan, T, theta) / theta_d, one).astype(T)
    return np.stack([pwx * scale, pwy * scale, np.ones_like(pwx)], 1)


def project(cam, X, T):
    fx, fy, cx, cy, k0, k1, k2, k3, _ = _cam(cam, 1.0, T)
    X = np.asarray(X, T)
    x2_plus_y2 = X[:, 0] * X[:, 0] + X[:, 1] * X[:, 1]
    theta = _fn(np.arctan2, T, np.sqrt(x2_plus_y2), X[:, 2])
    psi = _fn(np.arctan2, T, X[:, 1], X[:, 0])
    theta2 = theta * theta; theta3 = theta * theta2; theta5 = theta3 * theta2; theta7 = theta5 * theta2; theta9 = theta7 * theta2
    r = theta + k0 * theta3 + k1 * theta5 + k2 * theta7 + k3 * theta9
    return np.stack([fx * r * _fn(np.cos, T, psi) + cx, fy * r * _fn(np.sin, T, psi) + cy], 1)


def _dot3(a, b):
    """Eigen's fixed-size reduction of three products: a0 b0 + (a1 b1 + a2 b2)"""
    return a[..., 0] * b[..., 0] + (a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2])


def triangulate(p1, p2, R21, t21, T):
    n = len(p1)
    Tcw1 = np.hstack([np.eye(3, dtype=T), np.zeros((3, 1), T)])
    Tcw2 = np.hstack([R21, t21[:, None]]).astype(T)
    A = np.zeros((n, 4, 4), T)
    A[:, 0] = p1[:, 0:1] * Tcw1[2] - Tcw1[0]
    A[:, 1] = p1[:, 1:2] * Tcw1[2] - Tcw1[1]
    A[:, 2] = p2[:, 0:1] * Tcw2[2] - Tcw2[0]
    A[:, 3] = p2[:, 1:2] * Tcw2[2] - Tcw2[1]
    assert A.dtype == T
    h = np.linalg.svd(A)[2][:, 3, :]
    assert h.dtype == T
    with np.errstate(divide="ignore", invalid="ignore"):
        return h[:, :3] / h[:, 3:4]


def triangulate_matches(rig, pts_l, pts_r, sigma_l, sigma_r, dtype=FAITHFUL):
    """TriangulateMatches of n pixel pairs.  Returns dict(code [n] (-1 .. -5, or z1), p3d [n, 3] (zeros unless accepted), and the
    gate quantities cos, z1, z2, e1, e2 (float64 views; nan where the evaluation did not reach the gate))"""
    T = dtype
    n = len(pts_l)
    pts_l, pts_r = np.asarray(pts_l, T).reshape(n, 2), np.asarray(pts_r, T).reshape(n, 2)
    s1, s2 = np.asarray(sigma_l, np.float32).astype(np.float64), np.asarray(sigma_r, np.float32).astype(np.float64)
    R12, t12 = np.asarray(rig["Rlr"], T), np.asarray(rig["tlr"], T)
    r1 = unproject(rig["left"], rig["precision_l"], pts_l, T)
    r2 = unproject(rig["right"], rig["precision_r"], pts_r, T)
    r21 = np.stack([_dot3(R12[i], r2) for i in range(3)], 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        cos = _dot3(r1, r21) / (np.sqrt(_dot3(r1, r1)) * np.sqrt(_dot3(r21, r21)))
        R21 = R12.T.copy()
        t21 = np.array([_dot3(-R21[i], t12) for i in range(3)], T)
        x3D = triangulate(r1, r2, R21, t21, T)
        z1 = x3D[:, 2]
        z2 = _dot3(R21[2], x3D) + t21[2]
        uv1 = project(rig["left"], x3D, T)
        ex, ey = uv1[:, 0] - pts_l[:, 0], uv1[:, 1] - pts_l[:, 1]
        e1 = ex * ex + ey * ey
        x3D2 = np.stack([_dot3(R21[i], x3D) + t21[i] for i in range(3)], 1)
        uv2 = project(rig["right"], x3D2, T)
        ex, ey = uv2[:, 0] - pts_r[:, 0], uv2[:, 1] - pts_r[:, 1]
        e2 = ex * ex + ey * ey
        assert all(v.dtype == T for v in (cos, z1, z2, e1, e2))
        code = np.zeros(n, T)
        todo = np.ones(n, bool)
        reached = {}
        for name, c, hit in (("cos", -1, cos.astype(np.float64) > COS_LIMIT), ("z1", -2, z1 <= 0), ("z2", -3, z2 <= 0),
                             ("e1", -4, e1.astype(np.float64) > CHI2 * s1), ("e2", -5, e2.astype(np.float64) > CHI2 * s2)):
            reached[name] = todo.copy()
            code[todo & hit] = c
            todo &= ~hit
    code[todo] = z1[todo]
    p3d = np.where(todo[:, None], x3D, T(0)).astype(T)
    out = dict(code=code, p3d=p3d, accepted=todo, gate1=CHI2 * s1, gate2=CHI2 * s2)
    for name, v in (("cos", cos), ("z1", z1), ("z2", z2), ("e1", e1), ("e2", e2)):
        out[name] = np.where(reached[name], v.astype(np.float64), np.nan)
    return out


def outcome(code):
    """-1 .. -5, or 0 for an accepted pair (code = z1 > 0)"""
    code = np.asarray(code, np.float64)
    return np.where(code > 0, 0, np.round(code)).astype(np.int32)


def borderline(exact):
    """pairs whose outcome a rounding may change: judged on the `exact` evaluation, gate by gate as far as it went"""
    with np.errstate(invalid="ignore"):
        b = np.abs(exact["cos"] - COS_LIMIT) <= 1e-6
        b |= (np.abs(exact["z1"]) < 1e-4) | (np.abs(exact["z2"]) < 1e-4)
        b |= np.abs(exact["e1"] - exact["gate1"]) <= 1e-3 * exact["gate1"]
        b |= np.abs(exact["e2"] - exact["gate2"]) <= 1e-3 * exact["gate2"]
    return b


def stereo_fisheye(rig, kps_l, desc_l, mono_l, kps_r, desc_r, mono_r, level_sigma2, dtype=FAITHFUL):
    """The whole function.  kps = (n, 3) float array-likes of x, y, octave.  Returns left_to_right, right_to_left, depth, p3d
    (unset entries -1 / -1 / -1.0 / zeros), the k-NN diagnostics knn_right, knn_d0, knn_d1 over the whole left array, and `geo`:
    triangulate_matches of the survivors with `left` = their left indices."""
    kps_l, kps_r = np.asarray(kps_l, np.float64).reshape(-1, 3), np.asarray(kps_r, np.float64).reshape(-1, 3)
    desc_l, desc_r = np.asarray(desc_l, np.uint8).reshape(-1, 32), np.asarray(desc_r, np.uint8).reshape(-1, 32)
    n_l, n_r = len(kps_l), len(kps_r)
    sig = np.asarray(level_sigma2, np.float32)
    ltr = np.full(n_l, -1, np.int32); rtl = np.full(n_r, -1, np.int32)
    depth = np.full(n_l, -1.0, np.float32); p3d = np.zeros((n_l, 3), np.float32)
    knn_right = np.full(n_l, -1, np.int32); knn_d0 = np.full(n_l, -1, np.int32); knn_d1 = np.full(n_l, -1, np.int32)
    d0, d1, idx, ok = knn2(desc_l[mono_l:], desc_r[mono_r:])
    knn_d0[mono_l:], knn_d1[mono_l:] = d0, d1
    left = np.nonzero(ok)[0] + mono_l
    right = idx[ok] + mono_r
    knn_right[left] = right
    geo = triangulate_matches(rig, kps_l[left, :2], kps_r[right, :2], sig[kps_l[left, 2].astype(int)], sig[kps_r[right, 2].astype(int)], dtype)
    geo["left"], geo["right"] = left, right
    for j in range(len(left)):                       # the reference's loop: a later left key point overwrites mvRightToLeftMatch
        z = np.float32(geo["code"][j])
        if z > MIN_DEPTH:
            ltr[left[j]] = right[j]; rtl[right[j]] = left[j]
            depth[left[j]] = z; p3d[left[j]] = geo["p3d"][j]
    return dict(left_to_right=ltr, right_to_left=rtl, depth=depth, p3d=p3d, knn_right=knn_right, knn_d0=knn_d0, knn_d1=knn_d1, geo=geo)
