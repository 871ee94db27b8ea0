"""Reference for the pose-graph solver (essg_optimize): what Optimizer::OptimizeEssentialGraph computes once its graph is built
(reference src/Optimizer.cc:1729-1779), in plain numpy, vectorised over the edges, in float64 or numpy.longdouble.  It restates
g2o::Sim3 (Thirdparty/g2o/g2o/types/sim3.h), VertexSim3Expmap::oplusImpl, EdgeSim3::computeError, the numeric Jacobian of
base_binary_edge.hpp:147-196 and the Levenberg policy of optimization_algorithm_levenberg.cpp:61-169 on its own: nothing here is
shared with csrc/sim3_group.h or csrc/lm_control.h.  The linear system is dense (numpy.linalg.solve; in long double the float64
solution is refined with long double residuals until it stops moving).

Besides the results it returns how close it came to taking another path: the smallest distance of |sigma| and of 1 - d from
the branch thresholds of log over every evaluation, and the smallest relative margin of every Levenberg decision (the sign of
rho, the 1e-3 gain rule).  The spread between the two formats on the same inputs is what the GPU tests derive their tolerances
from; the margins say on which cases a count of iterations may be asserted."""
import numpy as np

EPS = 0.00001
DELTA = 1e-9


def _c(dt, v):
    return np.asarray(v, dt)


def quat_mul(a, b):
    ax, ay, az, aw = a[..., 0], a[..., 1], a[..., 2], a[..., 3]
    bx, by, bz, bw = b[..., 0], b[..., 1], b[..., 2], b[..., 3]
    return np.stack([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz], -1)


def quat_rot(q, v):
    u = 2 * np.cross(q[..., :3], v)
    return v + q[..., 3:4] * u + np.cross(q[..., :3], u)


def quat_to_R(q):
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    R = np.empty(q.shape[:-1] + (3, 3), q.dtype)
    R[..., 0, 0] = 1 - (2 * y * y + 2 * z * z); R[..., 0, 1] = 2 * y * x - 2 * z * w; R[..., 0, 2] = 2 * z * x + 2 * y * w
    R[..., 1, 0] = 2 * y * x + 2 * z * w; R[..., 1, 1] = 1 - (2 * x * x + 2 * z * z); R[..., 1, 2] = 2 * z * y - 2 * x * w
    R[..., 2, 0] = 2 * z * x - 2 * y * w; R[..., 2, 1] = 2 * z * y + 2 * x * w; R[..., 2, 2] = 1 - (2 * x * x + 2 * y * y)
    return R


def quat_from_R(R):
    """Eigen's Quaternion(Matrix3d): the trace branch, else the largest diagonal element"""
    dt = R.dtype
    flat = R.reshape(-1, 3, 3)
    q = np.empty((len(flat), 4), dt)
    for n, M in enumerate(flat):
        t = M[0, 0] + M[1, 1] + M[2, 2]
        if t > 0:
            r = np.sqrt(t + 1)
            f = _c(dt, 0.5) / r
            q[n] = [(M[2, 1] - M[1, 2]) * f, (M[0, 2] - M[2, 0]) * f, (M[1, 0] - M[0, 1]) * f, _c(dt, 0.5) * r]
        else:
            i = 0
            if M[1, 1] > M[0, 0]: i = 1
            if M[2, 2] > M[i, i]: i = 2
            j, k = (i + 1) % 3, (i + 2) % 3
            r = np.sqrt(M[i, i] - M[j, j] - M[k, k] + 1)
            f = _c(dt, 0.5) / r
            q[n, i] = _c(dt, 0.5) * r; q[n, 3] = (M[k, j] - M[j, k]) * f
            q[n, j] = (M[j, i] + M[i, j]) * f; q[n, k] = (M[k, i] + M[i, k]) * f
    return q.reshape(R.shape[:-2] + (4,))


def _skew(v):
    O = np.zeros(v.shape[:-1] + (3, 3), v.dtype)
    O[..., 0, 1] = -v[..., 2]; O[..., 0, 2] = v[..., 1]; O[..., 1, 0] = v[..., 2]
    O[..., 1, 2] = -v[..., 0]; O[..., 2, 0] = -v[..., 1]; O[..., 2, 1] = v[..., 0]
    return O


def _abc(sigma, s, small, theta):
    """A, B, C of W = A Omega + B Omega^2 + C I in the four branches (|sigma| < eps) x (small angle)"""
    dt = sigma.dtype
    one = _c(dt, 1)
    flat = np.abs(sigma) < EPS
    th = np.where(small, one, theta)                      # (unused where small; keeps the divisions finite)
    sg = np.where(flat, one, sigma)
    sn, cs = np.sin(th), np.cos(th)
    th2, sg2 = th * th, sg * sg
    C = np.where(flat, one, (s - 1) / sg)
    a, b, c = s * sn, s * cs, th2 + sg2
    A = np.where(flat, np.where(small, one / 2, (1 - cs) / th2),
                 np.where(small, ((sg - 1) * s + 1) / sg2, (a * sg + (1 - b) * th) / (th * c)))
    B = np.where(flat, np.where(small, one / 6, (th - sn) / (th2 * th)),
                 np.where(small, ((_c(dt, 0.5) * sg2 - sg + 1) * s) / (sg2 * sg), (C - ((b - 1) * sg + a * th) / c) * 1 / th2))
    return A, B, C


def sim3_exp(u):
    """Sim3(const Vector7d&): u = (omega, upsilon, sigma) -> (..., 8) q xyzw, t, s"""
    dt = u.dtype
    om, ups, sigma = u[..., :3], u[..., 3:6], u[..., 6]
    theta = np.sqrt((om * om).sum(-1))
    O = _skew(om)
    O2 = O @ O
    s = np.exp(sigma)
    small = theta < EPS
    th = np.where(small, _c(dt, 1), theta)
    I = np.eye(3, dtype=dt)
    R = np.where(small[..., None, None], I + O + O2,
                 I + (np.sin(th) / th)[..., None, None] * O + ((1 - np.cos(th)) / (th * th))[..., None, None] * O2)
    A, B, C = _abc(sigma, s, small, theta)
    W = A[..., None, None] * O + B[..., None, None] * O2 + C[..., None, None] * I
    t = (W @ ups[..., None])[..., 0]
    return np.concatenate([quat_from_R(R), t, s[..., None]], -1)


def _solve3(W, t):
    """W^-1 t by cofactors (W is C I plus a small skew part: far from singular)"""
    a, b, c = W[..., 0, 0], W[..., 0, 1], W[..., 0, 2]
    d, e, f = W[..., 1, 0], W[..., 1, 1], W[..., 1, 2]
    g, h, i = W[..., 2, 0], W[..., 2, 1], W[..., 2, 2]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    x = t[..., 0] * (e * i - f * h) - b * (t[..., 1] * i - f * t[..., 2]) + c * (t[..., 1] * h - e * t[..., 2])
    y = a * (t[..., 1] * i - f * t[..., 2]) - t[..., 0] * (d * i - f * g) + c * (d * t[..., 2] - t[..., 1] * g)
    z = a * (e * t[..., 2] - t[..., 1] * h) - b * (d * t[..., 2] - t[..., 1] * g) + t[..., 0] * (d * h - e * g)
    return np.stack([x, y, z], -1) / det[..., None]


def sim3_log(S):
    """Sim3::log -> (u, margins): margins[..., 0] = ||sigma| - eps|, margins[..., 1] = |(1 - eps) - d|"""
    dt = S.dtype
    s = S[..., 7]
    sigma = np.log(s)
    R = quat_to_R(S[..., :4])
    d = _c(dt, 0.5) * (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1)
    dR = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1)
    small = d > 1 - EPS
    dd = np.where(small, _c(dt, 0), d)
    theta = np.arccos(dd)
    om = np.where(small[..., None], _c(dt, 0.5) * dR, (theta / (2 * np.sqrt(1 - dd * dd)))[..., None] * dR)
    A, B, C = _abc(sigma, s, small, theta)
    O = _skew(om)
    W = A[..., None, None] * O + B[..., None, None] * (O @ O) + C[..., None, None] * np.eye(3, dtype=dt)
    ups = _solve3(W, S[..., 4:7])
    margins = np.stack([np.abs(np.abs(sigma) - EPS), np.abs((1 - EPS) - d)], -1)
    return np.concatenate([om, ups, sigma[..., None]], -1), margins


def sim3_mul(a, b):
    return np.concatenate([quat_mul(a[..., :4], b[..., :4]), a[..., 7:8] * quat_rot(a[..., :4], b[..., 4:7]) + a[..., 4:7],
                           a[..., 7:8] * b[..., 7:8]], -1)


def sim3_inv(a):
    qc = a[..., :4] * np.asarray([-1, -1, -1, 1], a.dtype)
    return np.concatenate([qc, quat_rot(qc, (-1 / a[..., 7:8]) * a[..., 4:7]), 1 / a[..., 7:8]], -1)


def sim3_map(S, X):
    return S[..., 7:8] * quat_rot(S[..., :4], X) + S[..., 4:7]


def oplus(est, u, fix_scale):
    if fix_scale:
        u = u.copy()
        u[..., 6] = 0
    return sim3_mul(sim3_exp(u), est)


def edge_errors(C, Si, Sj):
    """EdgeSim3::computeError for all edges: log(C * v0 * v1^-1) -> (errors [E, 7], margins [E, 2])"""
    return sim3_log(sim3_mul(sim3_mul(C, Si), sim3_inv(Sj)))


def numeric_jacobians(C, Si, Sj, fixed_i, fixed_j, fix_scale):
    """central differences with delta 1e-9 through oplus, columns of a fixed vertex zero -> (Ji, Jj [E, 7, 7], margins)"""
    dt = C.dtype
    E = len(C)
    J = [np.zeros((E, 7, 7), dt), np.zeros((E, 7, 7), dt)]
    scalar = _c(dt, 1) / (2 * _c(dt, DELTA))
    margin = np.full(2, np.inf)
    for side in (0, 1):
        for d in range(7):
            pm = []
            for sign in (1, -1):
                add = np.zeros((E, 7), dt)
                add[:, d] = sign * _c(dt, DELTA)
                P = oplus(Sj if side else Si, add, fix_scale)
                e, m = edge_errors(C, Si if side else P, P if side else Sj)
                margin = np.minimum(margin, m.min(0).astype(np.float64)) if E else margin
                pm.append(e)
            J[side][:, :, d] = scalar * (pm[0] - pm[1])
    J[0][np.asarray(fixed_i, bool)] = 0
    J[1][np.asarray(fixed_j, bool)] = 0
    return J[0], J[1], margin


def edge_blocks(Ji, Jj, e):
    """per edge: Ji^T Ji, Ji^T Jj, Jj^T Jj, -Ji^T e, -Jj^T e, chi2 (information = identity, no robust kernel)"""
    T = lambda M: np.swapaxes(M, -1, -2)
    return (T(Ji) @ Ji, T(Ji) @ Jj, T(Jj) @ Jj, -(T(Ji) @ e[..., None])[..., 0], -(T(Jj) @ e[..., None])[..., 0], (e * e).sum(-1))


def _solve(H, b, dt):
    if dt == np.float64:
        return np.linalg.solve(H, b)
    H64 = H.astype(np.float64)
    x = np.linalg.solve(H64, b.astype(np.float64)).astype(dt)
    for _ in range(8):
        r = b - H @ x
        dx = np.linalg.solve(H64, r.astype(np.float64)).astype(dt)
        x = x + dx
        if np.abs(dx).max() <= 1e-19 * max(np.abs(x).max(), 1e-300):
            break
    return x


def linearize(pr, est, dt):
    """errors, chi2, dense H (7 Nf x 7 Nf) and b over the free vertices in index order"""
    ev = np.asarray(pr["edge_vertices"]).reshape(-1, 2)
    fixed = np.asarray(pr["fixed"]).astype(bool)
    C = np.asarray(pr["edge_measurement"], dt).reshape(-1, 8)
    col = np.cumsum(~fixed) - 1
    nf = int((~fixed).sum())
    Si, Sj = est[ev[:, 0]], est[ev[:, 1]]
    e, m0 = edge_errors(C, Si, Sj)
    Ji, Jj, m1 = numeric_jacobians(C, Si, Sj, fixed[ev[:, 0]], fixed[ev[:, 1]], bool(pr["fix_scale"]))
    Hii, Hij, Hjj, bi, bj, chi = edge_blocks(Ji, Jj, e)
    H = np.zeros((7 * nf, 7 * nf), dt)
    b = np.zeros(7 * nf, dt)
    for k in range(len(ev)):
        i, j = ev[k]
        ci, cj = col[i], col[j]
        if not fixed[i]:
            H[7 * ci:7 * ci + 7, 7 * ci:7 * ci + 7] += Hii[k]
            b[7 * ci:7 * ci + 7] += bi[k]
        if not fixed[j]:
            H[7 * cj:7 * cj + 7, 7 * cj:7 * cj + 7] += Hjj[k]
            b[7 * cj:7 * cj + 7] += bj[k]
        if not fixed[i] and not fixed[j]:
            H[7 * ci:7 * ci + 7, 7 * cj:7 * cj + 7] += Hij[k]
            H[7 * cj:7 * cj + 7, 7 * ci:7 * ci + 7] += Hij[k].T
    margin = np.minimum(m0.min(0).astype(np.float64), m1) if len(ev) else np.full(2, np.inf)
    return dict(e=e, chi2=chi.sum(), chi2_edge=chi, H=H, b=b, Ji=Ji, Jj=Jj, blocks=(Hii, Hij, Hjj, bi, bj), branch_margin=margin)


def _chi2(pr, est, dt):
    ev = np.asarray(pr["edge_vertices"]).reshape(-1, 2)
    C = np.asarray(pr["edge_measurement"], dt).reshape(-1, 8)
    e, m = edge_errors(C, est[ev[:, 0]], est[ev[:, 1]])
    return (e * e).sum(-1).sum(), (m.min(0).astype(np.float64) if len(ev) else np.full(2, np.inf))


def optimize(pr, dt=np.float64):
    """initializeOptimization(); optimize(max_iters) with setUserLambdaInit(lambda_init); then the SE3 recovery and the map-point
    correction of :1735-1777.  Returns sim3_out (dt), pose_q / pose_t / points_out (float32), the statistics, and the margins."""
    est = np.asarray(pr["sim3"], dt).reshape(-1, 8).copy()
    est0 = est.copy()
    fixed = np.asarray(pr["fixed"]).astype(bool)
    free = np.flatnonzero(~fixed)
    fix_scale = bool(pr["fix_scale"])
    lam = _c(dt, pr["lambda_init"])
    ni = _c(dt, 2)
    n_bad = 0
    iterations = trials = 0
    stop_reason = 0
    trace = []
    branch = np.full(2, np.inf)
    flow_margin = np.inf
    chi_initial = None
    cur = None
    for it in range(int(pr["max_iters"])):
        L = linearize(pr, est, dt)
        branch = np.minimum(branch, L["branch_margin"])
        cur = ini = L["chi2"]
        if it == 0:
            chi_initial = cur
        rho = _c(dt, 0)
        qmax = 0
        while True:
            x = _solve(L["H"] + lam * np.eye(len(L["b"]), dtype=dt), L["b"], dt)
            trial = est.copy()
            trial[free] = oplus(est[free], x.reshape(-1, 7), fix_scale)
            chi_new, m = _chi2(pr, trial, dt)
            branch = np.minimum(branch, m)
            scale = (x * (lam * x + L["b"])).sum() + _c(dt, 1e-3)
            rho = (cur - chi_new) / scale
            ok = bool(rho > 0) and bool(np.isfinite(chi_new))
            flow_margin = min(flow_margin, float(abs(cur - chi_new) / max(abs(cur), 1e-300)))
            if ok:
                alpha = min(1 - (2 * rho - 1) ** 3, _c(dt, 2) / 3)
                lam = lam * max(_c(dt, 1) / 3, alpha)
                ni = _c(dt, 2)
                cur = chi_new
                est = trial
            else:
                lam = lam * ni
                ni = ni * 2
            qmax += 1
            trials += 1
            if not (rho < 0 and qmax < 10):
                break
        iterations += 1
        trace.append(cur)
        if qmax == 10 or rho == 0:
            stop_reason = 1
            break
        gain = (ini - cur) * 1000
        flow_margin = min(flow_margin, float(abs(gain - ini) / max(abs(ini), 1e-300)))
        n_bad = n_bad + 1 if gain < ini else 0
        if n_bad >= 3:
            stop_reason = 2
            break
    out = dict(sim3_out=est, stats=dict(iterations=iterations, trials=trials, stop_reason=stop_reason, chi2_initial=chi_initial,
                                         chi2_final=cur, chi2_trace=trace, lambda_=lam),
               branch_margin=branch, flow_margin=flow_margin)
    out.update(epilogue(pr, est0, est))
    return out


def epilogue(pr, est0, est):
    """[R | t / s] in float as Sophus::SE3f(rotation().cast<float>(), translation().cast<float>() / s) evaluates it: the scale is
    converted to float and divides the float translation; the float quaternion is normalised by the SO3 constructor.  Points:
    correctedSwr.map(Srw.map(P)) in the reference's double (here: the format of est), cast to float."""
    q = est[:, :4].astype(np.float32)
    q = q / np.sqrt((q * q).sum(1, dtype=np.float32))[:, None]
    t = est[:, 4:7].astype(np.float32) / est[:, 7:8].astype(np.float32)
    res = dict(pose_q=q, pose_t=t)
    pts = np.asarray(pr.get("points", np.zeros((0, 3), np.float32)), np.float32).reshape(-1, 3)
    if len(pts):
        ref = np.asarray(pr["point_ref"])
        res["points_out"] = sim3_map(sim3_inv(est[ref]), sim3_map(est0[ref], pts.astype(est.dtype))).astype(np.float32)
    else:
        res["points_out"] = np.zeros((0, 3), np.float32)
    return res
