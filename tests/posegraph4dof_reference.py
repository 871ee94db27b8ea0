"""Reference for the 4-DoF pose-graph solver (essg_optimize_4dof): what Optimizer::OptimizeEssentialGraph4DoF computes once its
graph is built (reference src/Optimizer.cc:5541-5586), in plain numpy, vectorised over vertices and edges, in float64 or
numpy.longdouble.  It restates ExpSO3 / LogSO3 / NormalizeRotation (src/G2oTypes.cc:782-814), ImuCamPose::UpdateW with its update
counter (:222-256) as VertexPose4DoF::oplusImpl calls it, Edge4DoF::computeError (include/G2oTypes.h:831-836), the numeric
Jacobian of base_binary_edge.hpp:147-196, the information matrix, and the Levenberg policy with computeLambdaInit
(optimization_algorithm_levenberg.cpp:61-185) on its own: nothing here is shared with csrc/pose4dof_group.h or csrc/lm_control.h.
DR is kept as the full 3 x 3 matrix and rotations are normalised by a polar iteration (the factor U V^T of the reference's SVD),
where the device carries a (cos, sin) pair and divides by a norm.  The control flow of the Levenberg loop is the one
posegraph_reference.optimize restates; the quaternion and Sim3 helpers of the epilogue are taken from that module.

Besides the results it returns the smallest relative margin of every Levenberg decision (the sign of rho, the 1e-3 gain rule):
the margins say on which cases a count of iterations may be asserted, and the spread between the two formats on the same inputs
is what the GPU tests derive their tolerances from."""
import numpy as np

from posegraph_reference import _solve, quat_from_R, sim3_inv, sim3_map

DELTA = 1e-9


def _c(dt, v):
    return np.asarray(v, dt)


def _inv3(M):
    a, b, c = M[..., 0, 0], M[..., 0, 1], M[..., 0, 2]
    d, e, f = M[..., 1, 0], M[..., 1, 1], M[..., 1, 2]
    g, h, i = M[..., 2, 0], M[..., 2, 1], M[..., 2, 2]
    det = a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g)
    C = np.stack([np.stack([e * i - f * h, c * h - b * i, b * f - c * e], -1), np.stack([f * g - d * i, a * i - c * g, c * d - a * f], -1),
                  np.stack([d * h - e * g, b * g - a * h, a * e - b * d], -1)], -2)
    return C / det[..., None, None]


def normalize_rotation(R):
    """NormalizeRotation: U V^T of the SVD, i.e. the orthogonal polar factor, here by Newton's iteration X <- (X + X^-T) / 2
    (quadratic; the inputs are within 1e-9 of a rotation, so three steps reach the last bit of a long double)"""
    X = R
    for _ in range(4):
        X = (X + np.swapaxes(_inv3(X), -1, -2)) / 2
    return X


def exp_so3(w):
    """ExpSO3 with its d < 1e-5 branch; w [..., 3]"""
    dt = w.dtype
    x, y, z = w[..., 0], w[..., 1], w[..., 2]
    d2 = x * x + y * y + z * z
    d = np.sqrt(d2)
    W = np.zeros(w.shape[:-1] + (3, 3), dt)
    W[..., 0, 1] = -z; W[..., 0, 2] = y; W[..., 1, 0] = z; W[..., 1, 2] = -x; W[..., 2, 0] = -y; W[..., 2, 1] = x
    small = d < 1e-5
    ds = np.where(small, _c(dt, 1), d)
    I = np.eye(3, dtype=dt)
    W2 = W @ W
    res = np.where(small[..., None, None], I + W + _c(dt, 0.5) * W2,
                   I + W * (np.sin(ds) / ds)[..., None, None] + W2 * ((1 - np.cos(ds)) / (ds * ds))[..., None, None])
    return normalize_rotation(res)


def log_so3(R):
    """LogSO3 with both early returns: costheta outside [-1, 1] and |sin theta| < 1e-5"""
    dt = R.dtype
    tr = R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2]
    w = np.stack([(R[..., 2, 1] - R[..., 1, 2]) / 2, (R[..., 0, 2] - R[..., 2, 0]) / 2, (R[..., 1, 0] - R[..., 0, 1]) / 2], -1)
    ct = (tr - 1) * _c(dt, 0.5)
    outside = (ct > 1) | (ct < -1)
    theta = np.arccos(np.where(outside, _c(dt, 0), ct))
    s = np.sin(theta)
    bare = outside | (np.abs(s) < 1e-5)
    f = np.where(bare, _c(dt, 1), theta / np.where(bare, _c(dt, 1), s))
    return w * f[..., None]


def initial_state(pr, dt):
    A = lambda k, shape: np.asarray(pr[k], dt).reshape(shape).copy()
    n = len(np.asarray(pr["fixed"]))
    return dict(DR=np.tile(np.eye(3, dtype=dt), (n, 1, 1)), twb=A("twb", (-1, 3)), its=np.zeros(n, int), Rcw=A("rcw", (-1, 3, 3)), tcw=A("tcw", (-1, 3)),
                Rwb0=A("rwb", (-1, 3, 3)), Rcb=A("rcb", (-1, 3, 3)), tcb=A("tcb", (-1, 3)))


def update_w(st, u, move):
    """oplusImpl(u = yaw, tx, ty, tz) on the vertices of the mask `move`: UpdateW with ur = (0, 0, u0), ut = (u1, u2, u3).  The camera
    pose comes from the DR of before the clean-up; the counter is part of the state"""
    dt = st["twb"].dtype
    ur = np.zeros(u.shape[:-1] + (3,), dt)
    ur[..., 2] = u[..., 0]
    DR = exp_so3(ur) @ st["DR"]
    Rwb = DR @ st["Rwb0"]
    twb = st["twb"] + u[..., 1:4]
    its = st["its"] + 1
    clean = its >= 5
    DRc = DR.copy()
    DRc[..., 0, 2] = 0; DRc[..., 1, 2] = 0; DRc[..., 2, 0] = 0; DRc[..., 2, 1] = 0
    DR = np.where(clean[:, None, None], normalize_rotation(DRc), DR)
    its = np.where(clean, 0, its)
    Rbw = np.swapaxes(Rwb, -1, -2)
    tbw = -(Rbw @ twb[..., None])[..., 0]
    Rcw = st["Rcb"] @ Rbw
    tcw = (st["Rcb"] @ tbw[..., None])[..., 0] + st["tcb"]
    m = np.asarray(move, bool)
    out = dict(st)
    out.update(DR=np.where(m[:, None, None], DR, st["DR"]), twb=np.where(m[:, None], twb, st["twb"]), its=np.where(m, its, st["its"]),
               Rcw=np.where(m[:, None, None], Rcw, st["Rcw"]), tcw=np.where(m[:, None], tcw, st["tcw"]))
    return out


def edge_errors(dR, dt_, Ri, ti, Rj, tj):
    """Edge4DoF::computeError for all edges -> [E, 6]"""
    RjT = np.swapaxes(Rj, -1, -2)
    rot = log_so3(Ri @ RjT @ np.swapaxes(dR, -1, -2))
    tr = (Ri @ (-(RjT @ tj[..., None])))[..., 0] + ti - dt_
    return np.concatenate([rot, tr], -1)


def _edges(pr, dt):
    ev = np.asarray(pr["edge_vertices"]).reshape(-1, 2)
    return ev, np.asarray(pr["edge_rot"], dt).reshape(-1, 3, 3), np.asarray(pr["edge_trans"], dt).reshape(-1, 3), np.asarray(pr["information"], dt).reshape(6, 6)


def errors(pr, st, dt):
    ev, dR, dtr, _ = _edges(pr, dt)
    i, j = ev[:, 0], ev[:, 1]
    return edge_errors(dR, dtr, st["Rcw"][i], st["tcw"][i], st["Rcw"][j], st["tcw"][j])


def _chi2(pr, st, dt):
    e = errors(pr, st, dt)
    W = _edges(pr, dt)[3]
    return ((e @ W) * e).sum(-1)


def numeric_jacobians(pr, st, dt):
    """central differences with delta 1e-9 through oplusImpl, columns of a fixed vertex zero -> Ji, Jj [E, 6, 4]"""
    ev, dR, dtr, _ = _edges(pr, dt)
    fixed = np.asarray(pr["fixed"]).astype(bool)
    E, n = len(ev), len(fixed)
    J = [np.zeros((E, 6, 4), dt), np.zeros((E, 6, 4), dt)]
    scalar = _c(dt, 1) / (2 * _c(dt, DELTA))
    i, j = ev[:, 0], ev[:, 1]
    for d in range(4):
        moved = []
        for sign in (1, -1):
            add = np.zeros((n, 4), dt)
            add[:, d] = sign * _c(dt, DELTA)
            moved.append(update_w(st, add, np.ones(n, bool)))
        for side in (0, 1):
            pm = []
            for P in moved:
                A, B = (st, P) if side else (P, st)
                pm.append(edge_errors(dR, dtr, A["Rcw"][i], A["tcw"][i], B["Rcw"][j], B["tcw"][j]))
            J[side][:, :, d] = scalar * (pm[0] - pm[1])
    J[0][fixed[i]] = 0
    J[1][fixed[j]] = 0
    return J[0], J[1]


def linearize(pr, st, dt):
    """errors, chi2, dense H (4 Nf x 4 Nf) and b over the free vertices in index order"""
    ev, _, _, W = _edges(pr, dt)
    fixed = np.asarray(pr["fixed"]).astype(bool)
    col = np.cumsum(~fixed) - 1
    nf = int((~fixed).sum())
    e = errors(pr, st, dt)
    Ji, Jj = numeric_jacobians(pr, st, dt)
    T = lambda M: np.swapaxes(M, -1, -2)
    We = e @ W                                      # W is symmetric
    Hii, Hij, Hjj = T(Ji) @ W @ Ji, T(Ji) @ W @ Jj, T(Jj) @ W @ Jj
    bi, bj = -(T(Ji) @ We[..., None])[..., 0], -(T(Jj) @ We[..., None])[..., 0]
    chi = (We * e).sum(-1)
    H = np.zeros((4 * nf, 4 * nf), dt)
    b = np.zeros(4 * nf, dt)
    for k in range(len(ev)):
        i, j = ev[k]
        ci, cj = col[i], col[j]
        if not fixed[i]:
            H[4 * ci:4 * ci + 4, 4 * ci:4 * ci + 4] += Hii[k]
            b[4 * ci:4 * ci + 4] += bi[k]
        if not fixed[j]:
            H[4 * cj:4 * cj + 4, 4 * cj:4 * cj + 4] += Hjj[k]
            b[4 * cj:4 * cj + 4] += bj[k]
        if not fixed[i] and not fixed[j]:
            H[4 * ci:4 * ci + 4, 4 * cj:4 * cj + 4] += Hij[k]
            H[4 * cj:4 * cj + 4, 4 * ci:4 * ci + 4] += Hij[k].T
    return dict(e=e, chi2=chi.sum(), chi2_edge=chi, H=H, b=b, Ji=Ji, Jj=Jj)


def optimize(pr, dt=np.float64):
    """initializeOptimization(); optimize(max_iters) with lambda_0 = 1e-5 max diag H unless lambda_init > 0; then the pose
    recovery and the map-point correction of :5548-5586.  Returns rcw_out / tcw_out (dt), pose_q / pose_t / points_out (float32), the
    statistics (lambda_0 among them) and the smallest margin of a Levenberg decision."""
    st = initial_state(pr, dt)
    fixed = np.asarray(pr["fixed"]).astype(bool)
    free = ~fixed
    lam = lam0 = None
    ni = _c(dt, 2)
    n_bad = 0
    iterations = trials = 0
    stop_reason = 0
    trace = []
    flow_margin = np.inf
    chi_initial = cur = None
    for it in range(int(pr["max_iters"])):
        L = linearize(pr, st, dt)
        cur = ini = L["chi2"]
        if it == 0:
            chi_initial = cur
            lam = lam0 = _c(dt, pr["lambda_init"]) if pr["lambda_init"] > 0 else _c(dt, 1e-5) * np.abs(np.diag(L["H"])).max()
        rho = _c(dt, 0)
        qmax = 0
        while True:
            x = _solve(L["H"] + lam * np.eye(len(L["b"]), dtype=dt), L["b"], dt)
            u = np.zeros((len(fixed), 4), dt)
            u[free] = x.reshape(-1, 4)
            trial = update_w(st, u, free)
            chi_new = _chi2(pr, trial, dt).sum()
            scale = (x * (lam * x + L["b"])).sum() + _c(dt, 1e-3)
            rho = (cur - chi_new) / scale
            ok = bool(rho > 0) and bool(np.isfinite(chi_new))
            flow_margin = min(flow_margin, float(abs(cur - chi_new) / max(abs(cur), 1e-300)))
            if ok:
                alpha = min(1 - (2 * rho - 1) ** 3, _c(dt, 2) / 3)
                lam = lam * max(_c(dt, 1) / 3, alpha)
                ni = _c(dt, 2)
                cur = chi_new
                st = trial
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
    if chi_initial is None:
        chi_initial = cur = _chi2(pr, st, dt).sum()
    out = dict(rcw_out=st["Rcw"], tcw_out=st["tcw"], state=st,
               stats=dict(iterations=iterations, trials=trials, stop_reason=stop_reason, chi2_initial=chi_initial, chi2_final=cur,
                          chi2_trace=trace, lambda_=lam, lambda_0=lam0), flow_margin=flow_margin)
    out.update(epilogue(pr, st["Rcw"], st["tcw"]))
    return out


def epilogue(pr, Rcw, tcw):
    """SetPose(SE3d(Quaterniond(Ri), ti).cast<float>()): the quaternion normalised in double by Sophus::SO3d's constructor and in
    float by SO3f's; points: Sim3(Ri, ti, 1).inverse().map(vScw[ref].map(P)) in the format of the estimate, cast to float."""
    dt = Rcw.dtype
    q = quat_from_R(Rcw)
    qn = (q / np.sqrt((q * q).sum(1))[:, None]).astype(np.float32)
    qn = qn / np.sqrt((qn * qn).sum(1, dtype=np.float32))[:, None]
    res = dict(pose_q=qn, pose_t=tcw.astype(np.float32))
    pts = np.asarray(pr.get("points", np.zeros((0, 3), np.float32)), np.float32).reshape(-1, 3)
    if len(pts):
        ref = np.asarray(pr["point_ref"])
        scw = np.asarray(pr["scw"], dt).reshape(-1, 8)
        S = np.concatenate([q, tcw, np.ones((len(q), 1), dt)], -1)
        res["points_out"] = sim3_map(sim3_inv(S[ref]), sim3_map(scw[ref], pts.astype(dt))).astype(np.float32)
    else:
        res["points_out"] = np.zeros((0, 3), np.float32)
    return res
