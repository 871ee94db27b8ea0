"""Plain-numpy reference of the loop-closing geometry, written from the reference sources and sharing no code with the product:

* Sim3Solver (src/Sim3Solver.cc): Horn's closed form (ComputeSim3, :311-412) through numpy.linalg.eigh, the two-sided inlier
  test (CheckInliers, :415-439) and the selection rule of iterate (:149-294).
* Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381) with g2o's numeric differentiation (base_binary_edge.hpp:147-196),
  Huber kernels and Levenberg (optimization_algorithm_levenberg.cpp:61-185).

Every function takes the number format as `dt`: the RANSAC part runs in float32 or float64 (eigh has no long double), the
optimiser in float64 or numpy.longdouble.  The spread between two formats on the same inputs is what the GPU tests derive
their tolerances from.  Sums whose order matters to a comparison are explicit loops or einsum."""
import numpy as np


# ---------------------------------------------------------------------------------------------------------------------
# Sim3Solver
# ---------------------------------------------------------------------------------------------------------------------
def quat_wxyz_to_R(q):
    """rotation matrix of unit quaternions q[..., (w, x, y, z)]"""
    qw, qx, qy, qz = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw),
                  2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw),
                  2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)], -1)
    return R.reshape(q.shape[:-1] + (3, 3))


def horn_N(P1, P2, dt=np.float64):
    """centroids, relative coordinates and the symmetric 4x4 N of ComputeSim3 (:316-349).  P1, P2: [H][3 points][3]."""
    P1 = np.asarray(P1).astype(dt)
    P2 = np.asarray(P2).astype(dt)
    O1 = (P1[:, 0] + P1[:, 1] + P1[:, 2]) / dt(3)
    O2 = (P2[:, 0] + P2[:, 1] + P2[:, 2]) / dt(3)
    A = P1 - O1[:, None]
    B = P2 - O2[:, None]
    M = np.einsum("hki,hkj->hij", B, A)                  # M = Pr2 * Pr1^T (:328)
    N = np.empty((len(M), 4, 4), dt)
    N[:, 0, 0] = M[:, 0, 0] + M[:, 1, 1] + M[:, 2, 2]
    N[:, 0, 1] = N[:, 1, 0] = M[:, 1, 2] - M[:, 2, 1]
    N[:, 0, 2] = N[:, 2, 0] = M[:, 2, 0] - M[:, 0, 2]
    N[:, 0, 3] = N[:, 3, 0] = M[:, 0, 1] - M[:, 1, 0]
    N[:, 1, 1] = M[:, 0, 0] - M[:, 1, 1] - M[:, 2, 2]
    N[:, 1, 2] = N[:, 2, 1] = M[:, 0, 1] + M[:, 1, 0]
    N[:, 1, 3] = N[:, 3, 1] = M[:, 2, 0] + M[:, 0, 2]
    N[:, 2, 2] = -M[:, 0, 0] + M[:, 1, 1] - M[:, 2, 2]
    N[:, 2, 3] = N[:, 3, 2] = M[:, 1, 2] + M[:, 2, 1]
    N[:, 3, 3] = -M[:, 0, 0] - M[:, 1, 1] + M[:, 2, 2]
    return O1, O2, A, B, N


def horn(P1, P2, fix_scale, dt=np.float64, negate=False):
    """ComputeSim3 for H point triples at once.  Returns R [H][3][3], t [H][3], s [H] and the relative eigen-gap
    (l1 - l2) / |l1| of N.  negate=True flips the sign of the eigenvector (an eigen-solver may return either)."""
    O1, O2, A, B, N = horn_N(P1, P2, dt)
    w, v = np.linalg.eigh(N)                             # ascending: column 3 belongs to the largest eigenvalue (:352-362)
    q = v[:, :, 3]
    if negate:
        q = -q
    gap = (w[:, 3] - w[:, 2]) / np.abs(w[:, 3])
    # the reference goes through atan2 and SO3::exp (:365-368): the rotation by 2 atan2(|v|, w) about v / |v|, which is the
    # rotation of the unit quaternion (w, v), the same for (w, v) and (-w, -v)
    q = q / np.sqrt(np.einsum("hi,hi->h", q, q))[:, None]
    R = quat_wxyz_to_R(q).astype(dt)
    P3 = np.einsum("hij,hkj->hki", R, B)                 # (:371)
    if fix_scale:
        s = np.ones(len(R), dt)
    else:
        s = (np.einsum("hki,hki->h", A, P3) / np.einsum("hki,hki->h", P3, P3)).astype(dt)       # (:375-385)
    t = O1 - s[:, None] * np.einsum("hij,hj->hi", R, O2)   # (:391)
    return R, t.astype(dt), s, gap


def project(X, K):
    """Pinhole::project (src/CameraModels/Pinhole.cpp:43-49); K = (fx, fy, cx, cy)"""
    return np.stack([K[0] * X[..., 0] / X[..., 2] + K[2], K[1] * X[..., 1] / X[..., 2] + K[3]], -1)


def map_points(R, t, s, X):
    """T12 applied to points: s R X + t for every hypothesis; [H][n][3]"""
    return s[:, None, None] * np.einsum("hij,nj->hni", R, X) + t[:, None]


def check_inliers(R, t, s, prob, dt=np.float64):
    """CheckInliers (:415-439) for every hypothesis: the ratios err1 / max_err1, err2 / max_err2 [H][n] and the inlier matrix"""
    X1 = prob["X1c"].astype(dt)
    X2 = prob["X2c"].astype(dt)
    K1 = prob["K1"].astype(dt)
    K2 = prob["K2"].astype(dt)
    p1 = project(X1, K1)                                 # mvP1im1 / mvP2im2 (:117-118)
    p2 = project(X2, K2)
    Y = map_points(R, t, s, X2)                          # T12 (:396-400)
    si = (dt(1) / s)
    Rt = np.swapaxes(R, 1, 2)
    ti = -(si[:, None] * np.einsum("hij,hj->hi", Rt, t))  # T21 (:403-411)
    Z = si[:, None, None] * np.einsum("hij,nj->hni", Rt, X1) + ti[:, None]
    d1 = p1[None] - project(Y, K1)
    d2 = project(Z, K2) - p2[None]
    err1 = d1[..., 0] * d1[..., 0] + d1[..., 1] * d1[..., 1]
    err2 = d2[..., 0] * d2[..., 0] + d2[..., 1] * d2[..., 1]
    e1 = prob["max_err1"].astype(dt)[None]
    e2 = prob["max_err2"].astype(dt)[None]
    return err1 / e1, err2 / e2, (err1 < e1) & (err2 < e2)


def select(counts, min_inliers):
    """iterate's bookkeeping (:192-209 / :265-287) run over all hypotheses with mnBestInliers starting at 0.
    Returns (converged, index)."""
    best, index = 0, -1
    for h, c in enumerate(counts):
        if c >= best:
            best, index = int(c), h
            if c > min_inliers:
                return 1, h
    return 0, index


def ransac(prob, dt=np.float64):
    """the whole solver on the given triples.  prob: X1c, X2c [n][3], max_err1/2 [n], K1, K2 (fx fy cx cy), fix_scale,
    min_inliers, triples [H][3]"""
    n, H = len(prob["X1c"]), len(prob["triples"])
    W = (n + 63) // 64
    if n < prob["min_inliers"] or n < 3:                 # bNoMore (:155-159)
        return dict(scored=0, converged=0, index=-1, count=np.zeros(H, np.int32), inl=np.zeros((H, n), bool),
                    mask=np.zeros((H, W), np.uint64))
    tri = np.asarray(prob["triples"])
    R, t, s, gap = horn(prob["X1c"][tri], prob["X2c"][tri], prob["fix_scale"], dt)
    r1, r2, inl = check_inliers(R, t, s, prob, dt)
    count = np.einsum("hn->h", inl.astype(np.int64)).astype(np.int32)
    converged, index = select(count, prob["min_inliers"])
    return dict(scored=1, converged=converged, index=index, count=count, inl=inl, mask=pack_mask(inl), R=R, t=t, s=s, gap=gap,
                r1=r1, r2=r2)


def pack_mask(inl):
    """[H][n] bool -> [H][ceil(n / 64)] uint64, bit k % 64 of word k / 64"""
    H, n = inl.shape
    W = (n + 63) // 64
    pad = np.zeros((H, W * 64), np.uint8)
    pad[:, :n] = inl
    return np.packbits(pad, axis=1, bitorder="little").view(np.uint64).reshape(H, W)


def unpack_mask(mask, n):
    H = mask.shape[0]
    bits = np.unpackbits(np.ascontiguousarray(mask).view(np.uint8).reshape(H, -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


# ---------------------------------------------------------------------------------------------------------------------
# g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h); a similarity is (q = (x, y, z, w), t, s)
# ---------------------------------------------------------------------------------------------------------------------
def _skew(v, dt):
    O = np.zeros((3, 3), dt)
    O[0, 1], O[0, 2], O[1, 0], O[1, 2], O[2, 0], O[2, 1] = -v[2], v[1], v[2], -v[0], -v[1], v[0]
    return O


def _matmul3(A, B, dt):
    C = np.zeros((3, 3), dt)
    for i in range(3):
        for j in range(3):
            C[i, j] = A[i, 0] * B[0, j] + A[i, 1] * B[1, j] + A[i, 2] * B[2, j]
    return C


def quat_from_R(R, dt):
    """Eigen's Quaternion(Matrix3): (x, y, z, w)"""
    q = np.zeros(4, dt)
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    if tr > 0:
        t = np.sqrt(tr + dt(1))
        q[3] = dt(0.5) * t
        t = dt(0.5) / t
        q[0], q[1], q[2] = (R[2, 1] - R[1, 2]) * t, (R[0, 2] - R[2, 0]) * t, (R[1, 0] - R[0, 1]) * t
    else:
        i = 0
        if R[1, 1] > R[0, 0]:
            i = 1
        if R[2, 2] > R[i, i]:
            i = 2
        j, k = (i + 1) % 3, (i + 2) % 3
        t = np.sqrt(R[i, i] - R[j, j] - R[k, k] + dt(1))
        q[i] = dt(0.5) * t
        t = dt(0.5) / t
        q[3] = (R[k, j] - R[j, k]) * t
        q[j] = (R[j, i] + R[i, j]) * t
        q[k] = (R[k, i] + R[i, k]) * t
    return q


def quat_rotate(q, v):
    """Eigen's Quaternion * Vector3 (also for a quaternion that is not exactly unit); v may be [..., 3] columns as v[0..2]"""
    ux, uy, uz = q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]
    ux, uy, uz = ux + ux, uy + uy, uz + uz
    return (v[0] + q[3] * ux + (q[1] * uz - q[2] * uy),
            v[1] + q[3] * uy + (q[2] * ux - q[0] * uz),
            v[2] + q[3] * uz + (q[0] * uy - q[1] * ux))


def quat_mul(a, b, dt):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                     a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                     a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]], dt)


def sim3_exp(u, dt):
    """Sim3(const Vector7d& update) (sim3.h:70-142): update = (omega, upsilon, sigma)"""
    u = np.asarray(u, dt)
    omega, upsilon, sigma = u[0:3], u[3:6], u[6]
    theta = np.sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2])
    Om = _skew(omega, dt)
    Om2 = _matmul3(Om, Om, dt)
    s = np.exp(sigma)
    I = np.eye(3, dtype=dt)
    eps = dt(0.00001)
    one = dt(1)
    if abs(sigma) < eps:
        C = one
        if theta < eps:
            A, B = one / 2, one / 6
            R = I + Om + Om2
        else:
            theta2 = theta * theta
            A = (one - np.cos(theta)) / theta2
            B = (theta - np.sin(theta)) / (theta2 * theta)
            R = I + np.sin(theta) / theta * Om + (one - np.cos(theta)) / (theta * theta) * Om2
    else:
        C = (s - one) / sigma
        if theta < eps:
            sigma2 = sigma * sigma
            A = ((sigma - one) * s + one) / sigma2
            B = ((dt(0.5) * sigma2 - sigma + one) * s) / (sigma2 * sigma)
            R = I + Om + Om2
        else:
            R = I + np.sin(theta) / theta * Om + (one - np.cos(theta)) / (theta * theta) * Om2
            a, b = s * np.sin(theta), s * np.cos(theta)
            theta2, sigma2 = theta * theta, sigma * sigma
            c = theta2 + sigma2
            A = (a * sigma + (one - b) * theta) / (theta * c)
            B = (C - ((b - one) * sigma + a * theta) / c) * one / theta2
    q = quat_from_R(R, dt)
    Wm = A * Om + B * Om2 + C * I
    t = np.array([Wm[i, 0] * upsilon[0] + Wm[i, 1] * upsilon[1] + Wm[i, 2] * upsilon[2] for i in range(3)], dt)
    return q, t, dt(s)


def sim3_mul(a, b, dt):
    """Sim3::operator* (:266-272)"""
    rt = quat_rotate(a[0], b[1])
    return quat_mul(a[0], b[0], dt), np.array([a[2] * rt[i] + a[1][i] for i in range(3)], dt), a[2] * b[2]


def sim3_inv(a, dt):
    """Sim3::inverse (:233-236)"""
    qc = np.array([-a[0][0], -a[0][1], -a[0][2], a[0][3]], dt)
    m = dt(-1) / a[2]
    return qc, np.array(quat_rotate(qc, m * a[1]), dt), dt(1) / a[2]


def sim3_map(S, X):
    """Sim3::map (:144-146) of points X [n][3] -> three coordinate arrays"""
    r = quat_rotate(S[0], (X[:, 0], X[:, 1], X[:, 2]))
    return S[2] * r[0] + S[1][0], S[2] * r[1] + S[1][1], S[2] * r[2] + S[1][2]


def sim3_from_Rts(R, t, s, dt=np.float64):
    """g2o::Sim3(const Matrix3d& R, const Vector3d& t, double s) (:64-67)"""
    return quat_from_R(np.asarray(R, dt), dt), np.asarray(t, dt).copy(), dt(s)


def quat_xyzw_to_R(q):
    q = np.asarray(q, np.float64)
    q = q / np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return quat_wxyz_to_R(np.array([q[3], q[0], q[1], q[2]]))


# ---------------------------------------------------------------------------------------------------------------------
# Optimizer::OptimizeSim3
# ---------------------------------------------------------------------------------------------------------------------
def edge_errors(S, Si, pr, dt):
    """computeError of every pair (OptimizableTypes.h:183-190, :204-211): e12 = obs1 - project1(S12 X2c),
    e21 = obs2 - project2(S12^-1 X1c); [n][4]"""
    K1, K2 = pr["_K1"], pr["_K2"]
    y = sim3_map(S, pr["_X2"])
    z = sim3_map(Si, pr["_X1"])
    e = np.empty((len(pr["_X1"]), 4), dt)
    e[:, 0] = pr["_o1"][:, 0] - (K1[0] * y[0] / y[2] + K1[2])
    e[:, 1] = pr["_o1"][:, 1] - (K1[1] * y[1] / y[2] + K1[3])
    e[:, 2] = pr["_o2"][:, 0] - (K2[0] * z[0] / z[2] + K2[2])
    e[:, 3] = pr["_o2"][:, 1] - (K2[1] * z[1] / z[2] + K2[3])
    return e


def edge_chi2(e, pr):
    """chi2() of both edges of every pair with information inv_sigma2 * I; [n][2]"""
    w1, w2 = pr["_w1"], pr["_w2"]
    return np.stack([e[:, 0] * (w1 * e[:, 0]) + e[:, 1] * (w1 * e[:, 1]), e[:, 2] * (w2 * e[:, 2]) + e[:, 3] * (w2 * e[:, 3])], 1)


def _oplus(S, u, fix_scale, dt):
    """VertexSim3Expmap::oplusImpl (OptimizableTypes.h:158-167)"""
    u = np.array(u, dt)
    if fix_scale:
        u[6] = 0
    return sim3_mul(sim3_exp(u, dt), S, dt)


def numeric_jacobians(S, pr, dt):
    """linearizeOplus of base_binary_edge.hpp:147-196 for the Sim3 vertex: central differences, delta = 1e-9; [n][4][7]"""
    delta = dt(1e-9)
    scalar = dt(1) / (2 * delta)
    J = np.zeros((len(pr["_X1"]), 4, 7), dt)
    for d in range(7):
        u = np.zeros(7, dt)
        u[d] = delta
        Sp = _oplus(S, u, pr["fix_scale"], dt)
        u[d] = -delta
        Sm = _oplus(S, u, pr["fix_scale"], dt)
        J[:, :, d] = scalar * (edge_errors(Sp, sim3_inv(Sp, dt), pr, dt) - edge_errors(Sm, sim3_inv(Sm, dt), pr, dt))
    return J


def analytic_jacobians(S, pr, dt=np.float64):
    """closed-form Jacobians of both edges for the left perturbation exp(u) * S (a check of the numeric scheme only)"""
    n = len(pr["_X1"])
    J = np.zeros((n, 4, 7), dt)
    Si = sim3_inv(S, dt)
    Y = np.stack(sim3_map(S, pr["_X2"]), 1)
    Z = np.stack(sim3_map(Si, pr["_X1"]), 1)
    Rinv = quat_xyzw_to_R(Si[0]).astype(dt)
    for k in range(n):
        for side, (P, K) in enumerate(((Y[k], pr["_K1"]), (Z[k], pr["_K2"]))):
            dp = np.array([[K[0] / P[2], 0, -K[0] * P[0] / (P[2] * P[2])], [0, K[1] / P[2], -K[1] * P[1] / (P[2] * P[2])]], dt)
            if side == 0:            # exp(u) S X = Y + omega x Y + upsilon + sigma Y
                D = np.concatenate([-_skew(P, dt), np.eye(3, dtype=dt), P[:, None]], 1)
            else:                    # (exp(u) S)^-1 X = S^-1 (X - omega x X - upsilon - sigma X)
                X = pr["_X1"][k]
                D = -(Si[2] * Rinv) @ np.concatenate([-_skew(X, dt), np.eye(3, dtype=dt), X[:, None]], 1)
            J[k, 2 * side:2 * side + 2] = -dp @ D
    if pr["fix_scale"]:
        J[:, :, 6] = 0
    return J


def _huber(chi, delta, dt):
    """RobustKernelHuber::robustify: rho, rho'"""
    dsq = delta * delta
    if chi <= dsq:
        return chi, dt(1)
    sq = np.sqrt(chi)
    return 2 * sq * delta - dsq, delta / sq


def _robust_chi2(e, active, robust, pr, dt):
    """activeRobustChi2: edges in graph order (e12 and e21 of pair 0, of pair 1, ...)"""
    c = edge_chi2(e, pr)
    total = dt(0)
    for k in np.nonzero(active)[0]:
        for side in range(2):
            total += _huber(c[k, side], pr["_delta"], dt)[0] if robust else c[k, side]
    return total


def _ldlt_solve(H, b, dt):
    """dense LDL^T without pivoting (g2o's LinearSolverDense uses Eigen's pivoted LDLT: the same solution up to rounding);
    ok = every pivot positive"""
    n = len(b)
    L = np.zeros((n, n), dt)
    D = np.zeros(n, dt)
    ok = True
    for j in range(n):
        d = H[j, j]
        for k in range(j):
            d -= L[j, k] * L[j, k] * D[k]
        ok = ok and bool(d > 0) and bool(np.isfinite(d))
        D[j] = d
        for i in range(j + 1, n):
            v = H[i, j]
            for k in range(j):
                v -= L[i, k] * L[j, k] * D[k]
            L[i, j] = v / d
    x = np.zeros(n, dt)
    for i in range(n):
        v = b[i]
        for k in range(i):
            v -= L[i, k] * x[k]
        x[i] = v
    x = x / D
    for i in range(n - 1, -1, -1):
        v = x[i]
        for k in range(i + 1, n):
            v -= L[k, i] * x[k]
        x[i] = v
    return x, ok


def _levenberg(S, active, robust, max_it, pr, dt):
    """SparseOptimizer::optimize(max_it) with OptimizationAlgorithmLevenberg (levenberg.cpp:61-185).  Returns the estimate,
    the errors as last computed, and iterations / trials / stop reason / chi2."""
    e = edge_errors(S, sim3_inv(S, dt), pr, dt)
    stats = dict(iterations=0, trials=0, stop_reason=0, chi2=dt(0), trace=[])     # trace: (chi2 before, chi2 of the trial) per trial
    idx = np.nonzero(active)[0]
    if len(idx) == 0:
        return S, e, stats
    lam, ni, n_bad = dt(0), dt(2), 0
    for it in range(max_it):
        e = edge_errors(S, sim3_inv(S, dt), pr, dt)      # computeActiveErrors
        cur = _robust_chi2(e, active, robust, pr, dt)
        ini = cur
        J = numeric_jacobians(S, pr, dt)                 # buildSystem: linearizeOplus + constructQuadraticForm (:55-120)
        c = edge_chi2(e, pr)
        H = np.zeros((7, 7), dt)
        b = np.zeros(7, dt)
        for k in idx:
            for side in range(2):
                w = pr["_w1"][k] if side == 0 else pr["_w2"][k]
                rho1 = _huber(c[k, side], pr["_delta"], dt)[1] if robust else dt(1)
                Jk = J[k, 2 * side:2 * side + 2]
                r = e[k, 2 * side:2 * side + 2]
                omega_r = rho1 * (-(w * r))
                for a in range(7):
                    b[a] += Jk[0, a] * omega_r[0] + Jk[1, a] * omega_r[1]
                    for cc in range(a, 7):
                        H[a, cc] += Jk[0, a] * (rho1 * w) * Jk[0, cc] + Jk[1, a] * (rho1 * w) * Jk[1, cc]
        for a in range(7):
            for cc in range(a):
                H[a, cc] = H[cc, a]
        if it == 0:                                      # computeLambdaInit (:171-185)
            lam = dt(1e-5) * max(abs(H[j, j]) for j in range(7))
            ni, n_bad = dt(2), 0
        qmax, rho = 0, dt(0)
        while True:
            x, ok = _ldlt_solve(H + lam * np.eye(7, dtype=dt), b, dt)
            if ok:
                St = _oplus(S, x, pr["fix_scale"], dt)
            else:
                St, x = S, np.zeros(7, dt)
            e = edge_errors(St, sim3_inv(St, dt), pr, dt)
            temp = _robust_chi2(e, active, robust, pr, dt)
            if not ok:
                temp = dt(np.finfo(np.float64).max)
            scale = dt(0)
            for j in range(7):
                scale += x[j] * (lam * x[j] + b[j])
            scale += dt(1e-3)
            stats["trace"].append((float(cur), float(temp)))
            rho = (cur - temp) / scale
            if rho > 0 and np.isfinite(temp):
                alpha = dt(1) - (2 * rho - 1) ** 3
                alpha = min(alpha, dt(2) / 3)
                lam *= max(dt(1) / 3, alpha)
                ni = dt(2)
                cur = temp
                S = St
            else:
                lam *= ni
                ni *= 2
            qmax += 1
            if not (rho < 0 and qmax < 10):
                break
        stats["iterations"] += 1
        stats["trials"] += qmax
        stats["chi2"] = cur
        if qmax == 10 or rho == 0:
            stats["stop_reason"] = 1
            break
        n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
        if n_bad >= 3:
            stats["stop_reason"] = 2
            break
    return S, e, stats


def _prepare(pr, dt):
    pr = dict(pr)
    for k, src in (("_X1", "X1c"), ("_X2", "X2c"), ("_o1", "obs1"), ("_o2", "obs2"), ("_w1", "inv_sigma2_1"), ("_w2", "inv_sigma2_2"),
                   ("_K1", "K1"), ("_K2", "K2")):
        pr[k] = np.asarray(pr[src], np.float64).astype(dt)
    pr["_X1"] = pr["_X1"].reshape(-1, 3)
    pr["_X2"] = pr["_X2"].reshape(-1, 3)
    pr["_o1"] = pr["_o1"].reshape(-1, 2)
    pr["_o2"] = pr["_o2"].reshape(-1, 2)
    pr["_delta"] = dt(pr["huber_delta"])
    return pr


def optimize_sim3(pr, dt=np.float64):
    """Optimizer::OptimizeSim3 on the flattened graph.  pr: q (x y z w), t, s, X1c, X2c [n][3], obs1, obs2 [n][2],
    inv_sigma2_1/2 [n], K1, K2, th2, huber_delta, fix_scale.  Returns q, t, s, n_in, n_bad, keep [n], the per-round statistics
    and chi2_final [n][2] of the last test."""
    pr = _prepare(pr, dt)
    n = len(pr["_X1"])
    th2 = dt(pr["th2"])
    S0 = (np.asarray(pr["q"], np.float64).astype(dt), np.asarray(pr["t"], np.float64).astype(dt), dt(pr["s"]))
    active = np.ones(n, bool)
    S, e, st0 = _levenberg(S0, active, True, 5, pr, dt)                  # optimize(5) with Huber (:2306-2308)
    c = edge_chi2(e, pr)                                                  # the errors as last computed (:2313-2340)
    bad = (c[:, 0] > th2) | (c[:, 1] > th2)
    n_bad = int(np.count_nonzero(bad))
    keep = ~bad
    out = dict(n_bad=n_bad, iterations=[st0["iterations"], 0], trials=[st0["trials"], 0], stop_reason=[st0["stop_reason"], 0],
               chi2=[st0["chi2"], dt(0)], chi2_final=c, trace=[st0["trace"], []])
    if n - n_bad < 10:                                                    # (:2348-2349): g2oS12 is not written
        out.update(q=S0[0], t=S0[1], s=S0[2], n_in=0, keep=keep)
        return out
    S, e, st1 = _levenberg(S, keep, False, 10 if n_bad > 0 else 5, pr, dt)  # (:2342-2353)
    e = edge_errors(S, sim3_inv(S, dt), pr, dt)                           # computeError on the final estimate (:2364-2365)
    c = edge_chi2(e, pr)
    good = keep & ~((c[:, 0] > th2) | (c[:, 1] > th2))
    out.update(q=S[0], t=S[1], s=S[2], n_in=int(np.count_nonzero(good)), keep=good, chi2_final=c)
    out["trace"][1] = st1["trace"]
    out["iterations"][1], out["trials"][1], out["stop_reason"][1], out["chi2"][1] = st1["iterations"], st1["trials"], st1["stop_reason"], st1["chi2"]
    return out
