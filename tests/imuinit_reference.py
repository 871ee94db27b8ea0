"""Dense reference for the IMU initialisation (imu_init_optimize_batch): the three Optimizer::InertialOptimization overloads as
one problem.  A test helper, not a test.

Plain numpy, parametrised by dtype (np.float64 or np.longdouble).  Every residual, Jacobian, robust weight and the Levenberg /
Gauss-Newton policy is restated from the reference text (cited file:line, read as text; nothing copied); the system over the free
unknowns is assembled DENSELY and solved by Cholesky -- no chain elimination, no Schur complement: that is the device's business.

Follows:
  src/G2oTypes.cc:617-640            EdgeInertialGS::computeError
  src/G2oTypes.cc:642-718            EdgeInertialGS::linearizeOplus, the analytic Jacobians AS WRITTEN: the scale column carries no
                                     factor s although the update is s <- s exp(u)
  include/G2oTypes.h:257-317         GDirection::Update (Rwg <- Rwg ExpSO3(u0, u1, 0)), VertexScale::oplusImpl
  src/G2oTypes.cc:777-854            ExpSO3, LogSO3, InverseRightJacobianSO3, RightJacobianSO3 with their 1e-5 branches
  src/ImuTypes.cc:276-307            GetDelta*: float expressions (the restatement of dense_inertial_reference.get_deltas, here
                                     vectorised over the links; test_imuinit_reference.py holds the two together bit for bit)
  src/Optimizer.cc:3101-3114         EdgePriorAcc / EdgePriorGyro: information prior x I, prior value 0
  Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-185, optimization_algorithm_gauss_newton.cpp:49-90
  Thirdparty/g2o/g2o/core/robust_kernel_impl.cpp   RobustKernelHuber

Unknowns: the velocities of the key frames that appear in a link (ascending key frame), then gyro bias, accelerometer bias, gravity
direction (2), log-scale -- whichever are free.  reverse=True numbers them the other way round, so the factorisation eliminates the
border first: the same mathematics in another operation order.  In long double the Cholesky factor is LAPACK's f64 one and the
solution is refined with long-double residuals until it is a long-double solution (numpy.linalg has no long double).
"""
import numpy as np
import scipy.linalg

F32 = np.float32
LD = np.longdouble
GRAVITY = float(np.float32(9.81))           # const float IMU::GRAVITY_VALUE (include/ImuTypes.h:43)


def skew(v):
    z = np.zeros(v.shape[:-1], v.dtype)
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def inv3(a):
    c00 = a[..., 1, 1] * a[..., 2, 2] - a[..., 1, 2] * a[..., 2, 1]
    c01 = a[..., 1, 2] * a[..., 2, 0] - a[..., 1, 0] * a[..., 2, 2]
    c02 = a[..., 1, 0] * a[..., 2, 1] - a[..., 1, 1] * a[..., 2, 0]
    det = a[..., 0, 0] * c00 + a[..., 0, 1] * c01 + a[..., 0, 2] * c02
    adj = np.stack([np.stack([c00, a[..., 0, 2] * a[..., 2, 1] - a[..., 0, 1] * a[..., 2, 2], a[..., 0, 1] * a[..., 1, 2] - a[..., 0, 2] * a[..., 1, 1]], -1),
                    np.stack([c01, a[..., 0, 0] * a[..., 2, 2] - a[..., 0, 2] * a[..., 2, 0], a[..., 0, 2] * a[..., 1, 0] - a[..., 0, 0] * a[..., 1, 2]], -1),
                    np.stack([c02, a[..., 0, 1] * a[..., 2, 0] - a[..., 0, 0] * a[..., 2, 1], a[..., 0, 0] * a[..., 1, 1] - a[..., 0, 1] * a[..., 1, 0]], -1)], -2)
    return adj / det[..., None, None]


def polar(R):
    """NormalizeRotation (G2oTypes.h:67-71): the orthogonal polar factor, by Newton iteration; batched"""
    for _ in range(10):
        Rn = (R + np.swapaxes(inv3(R), -1, -2)) / 2
        done = np.abs(Rn - R).max() < 1e-16
        R = Rn
        if done:
            break
    return R


def _eye(v):
    return np.broadcast_to(np.eye(3, dtype=v.dtype), v.shape[:-1] + (3, 3)).copy()


def exp_so3(w):
    """ExpSO3 (G2oTypes.cc:782-798); batched"""
    d2 = (w * w).sum(-1); d = np.sqrt(d2)
    W = skew(w)
    small = d < 1e-5
    ds = np.where(small, 1, d); d2s = np.where(small, 1, d2)
    a = np.where(small, 1, np.sin(ds) / ds); b = np.where(small, w.dtype.type(0.5), (1 - np.cos(ds)) / d2s)
    return polar(_eye(w) + W * a[..., None, None] + (W @ W) * b[..., None, None])


def log_so3(R):
    """LogSO3 (G2oTypes.cc:800-814) with its |sin theta| < 1e-5 branch; batched"""
    w = np.stack([R[..., 2, 1] - R[..., 1, 2], R[..., 0, 2] - R[..., 2, 0], R[..., 1, 0] - R[..., 0, 1]], -1) / 2
    c = (R[..., 0, 0] + R[..., 1, 1] + R[..., 2, 2] - 1) * R.dtype.type(0.5)
    inside = (c <= 1) & (c >= -1)
    th = np.arccos(np.where(inside, c, 0)); s = np.sin(th)
    plain = ~inside | (np.abs(s) < 1e-5)
    return np.where(plain[..., None], w, (th / np.where(plain, 1, s))[..., None] * w)


def inv_right_jacobian(v):
    """InverseRightJacobianSO3 (G2oTypes.cc:821-832); batched"""
    d2 = (v * v).sum(-1); d = np.sqrt(d2)
    small = d < 1e-5
    ds = np.where(small, 1, d)
    W = skew(v)
    c = np.where(small, 0, 1 / ds ** 2 - (1 + np.cos(ds)) / (2 * ds * np.sin(ds)))
    return _eye(v) + np.where(small[..., None, None], 0, W / 2) + (W @ W) * c[..., None, None]


def right_jacobian(v):
    """RightJacobianSO3 (G2oTypes.cc:839-854); batched"""
    d2 = (v * v).sum(-1); d = np.sqrt(d2)
    small = d < 1e-5
    ds = np.where(small, 1, d)
    W = skew(v)
    a = np.where(small, 0, (1 - np.cos(ds)) / ds ** 2); b = np.where(small, 0, (ds - np.sin(ds)) / (ds ** 2 * ds))
    return _eye(v) - W * a[..., None, None] + (W @ W) * b[..., None, None]


def huber(chi2, delta, on):
    """RobustKernelHuber::robustify: (rho, rho') of a squared error; on: the link carries the kernel"""
    dsq = delta * delta
    big = on & ~(chi2 <= dsq)
    s = np.sqrt(np.where(big, chi2, 1))
    return np.where(big, 2 * s * delta - dsq, chi2), np.where(big, delta / s, chi2.dtype.type(1))


# ------------------------------------------------------------------------------------------------ the problem in arrays
def arrays_of(pr, dt):
    """the links of a problem dictionary as arrays [m, ...] (float members stay float32) and the fixed poses in dt"""
    L = pr["links"]
    m = len(L)
    f = lambda key, shape: np.array([np.asarray(l[key], F32).reshape(shape) for l in L], F32).reshape((m,) + shape)
    a = dict(kf1=np.array([int(l["kf1"]) for l in L], int), kf2=np.array([int(l["kf2"]) for l in L], int),
             dR=f("dR", (3, 3)), dV=f("dV", (3,)), dP=f("dP", (3,)), JRg=f("JRg", (3, 3)), JVg=f("JVg", (3, 3)), JVa=f("JVa", (3, 3)),
             JPg=f("JPg", (3, 3)), JPa=f("JPa", (3, 3)), bias0=f("bias0", (6,)), dT=np.array([F32(l["dT"]) for l in L], F32).astype(dt),
             info9=np.array([np.asarray(l["info9"], np.float64).reshape(9, 9) for l in L], dt).reshape(m, 9, 9),
             robust=np.array([bool(l["robust"]) for l in L], bool),
             Rwb=np.asarray(pr["Rwb"], np.float64).reshape(-1, 3, 3).astype(dt), twb=np.asarray(pr["twb"], np.float64).reshape(-1, 3).astype(dt))
    return a


def _mv32(J, d):
    """Matrix3f * Vector3f in float, the three products summed in order, no contraction; batched over the links"""
    return (J[:, :, 0] * d[:, 0:1] + J[:, :, 1] * d[:, 1:2]) + J[:, :, 2] * d[:, 2:3]


def get_deltas(a, bg, ba, dt):
    """(dR, dV, dP, dbg) of Preintegrated::GetDeltaRotation / Velocity / Position / GetDeltaBias at the shared bias, for every link:
    float expressions on a float bias; the exponential of JRg dbg is the quaternion one, evaluated in dt and rounded to float, the float
    product dR * E is re-orthonormalised and rounded to float (dense_inertial_reference.get_deltas, vectorised)"""
    bgf = np.asarray(bg, dt).astype(np.float64).astype(F32); baf = np.asarray(ba, dt).astype(np.float64).astype(F32)
    dbg = bgf[None, :] - a["bias0"][:, 3:]; dba = baf[None, :] - a["bias0"][:, :3]
    w = _mv32(a["JRg"], dbg).astype(dt)
    th2 = (w * w).sum(-1); th = np.sqrt(th2)
    small = th < 1e-5
    ths = np.where(small, 1, th)
    imag = np.where(small, dt(0.5) - th2 / 48, np.sin(ths / 2) / ths); real = np.where(small, 1 - th2 / 8, np.cos(ths / 2))
    qx, qy, qz, qw = imag * w[:, 0], imag * w[:, 1], imag * w[:, 2], real
    E = np.stack([np.stack([1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)], -1),
                  np.stack([2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)], -1),
                  np.stack([2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)], -1)], -2)
    E = E.astype(np.float64).astype(F32)
    d0 = a["dR"]
    Rf = (d0[:, :, 0:1] * E[:, 0:1, :] + d0[:, :, 1:2] * E[:, 1:2, :]) + d0[:, :, 2:3] * E[:, 2:3, :]
    dR = polar(Rf.astype(dt)).astype(np.float64).astype(F32).astype(dt)
    dV = (a["dV"] + _mv32(a["JVg"], dbg)) + _mv32(a["JVa"], dba)
    dP = (a["dP"] + _mv32(a["JPg"], dbg)) + _mv32(a["JPa"], dba)
    return dR, dV.astype(dt), dP.astype(dt), dbg.astype(dt)


def initial_state(pr, dt):
    return dict(vel=np.asarray(pr["vel"], np.float64).reshape(-1, 3).astype(dt), bg=np.asarray(pr["bg"], np.float64).astype(dt),
                ba=np.asarray(pr["ba"], np.float64).astype(dt), Rwg=np.asarray(pr["Rwg"], np.float64).reshape(3, 3).astype(dt),
                scale=dt(pr["scale"]))


def errors(a, st, dt, with_parts=False):
    """EdgeInertialGS::computeError of every link: [m, 9] = (er, ev, ep)"""
    dR, dV, dP, dbg = get_deltas(a, st["bg"], st["ba"], dt)
    gI = np.array([0, 0, -GRAVITY], dt)
    g = st["Rwg"] @ gI
    s = st["scale"]
    T = lambda M: np.swapaxes(M, -1, -2)
    Rbw1 = T(a["Rwb"][a["kf1"]]); Rwb2 = a["Rwb"][a["kf2"]]
    v1, v2 = st["vel"][a["kf1"]], st["vel"][a["kf2"]]
    p1, p2 = a["twb"][a["kf1"]], a["twb"][a["kf2"]]
    tt = a["dT"][:, None]
    eR = T(dR) @ Rbw1 @ Rwb2
    er = log_so3(eR)
    ev = np.einsum("mij,mj->mi", Rbw1, s * (v2 - v1) - g * tt) - dV
    ep = np.einsum("mij,mj->mi", Rbw1, s * (p2 - p1 - v1 * tt) - g * tt * tt / 2) - dP
    e = np.concatenate([er, ev, ep], -1)
    return (e, eR, Rbw1, dbg) if with_parts else e


def jacobians(a, st, dt):
    """EdgeInertialGS::linearizeOplus of every link: [m, 9, 15], columns V1 (3) V2 (3) gyro bias (3) accelerometer bias (3) gravity
    direction (2) scale (1).  The pose columns are never needed: every pose is fixed."""
    e, eR, Rbw1, dbg = errors(a, st, dt, True)
    m = len(e)
    T = lambda M: np.swapaxes(M, -1, -2)
    s = st["scale"]
    tt = a["dT"][:, None, None]
    J = np.zeros((m, 9, 15), dt)
    J[:, 3:6, 0:3] = -s * Rbw1
    J[:, 6:9, 0:3] = -s * Rbw1 * tt
    J[:, 3:6, 3:6] = s * Rbw1
    invJr = inv_right_jacobian(e[:, 0:3])
    JRg = a["JRg"].astype(dt)
    J[:, 0:3, 6:9] = -invJr @ T(eR) @ right_jacobian(np.einsum("mij,mj->mi", JRg, dbg)) @ JRg
    J[:, 3:6, 6:9] = -a["JVg"].astype(dt)
    J[:, 6:9, 6:9] = -a["JPg"].astype(dt)
    J[:, 3:6, 9:12] = -a["JVa"].astype(dt)
    J[:, 6:9, 9:12] = -a["JPa"].astype(dt)
    Gm = np.zeros((3, 2), dt)
    Gm[0, 1] = -GRAVITY; Gm[1, 0] = GRAVITY
    dG = st["Rwg"] @ Gm
    J[:, 3:6, 12:14] = -(Rbw1 @ dG) * tt
    J[:, 6:9, 12:14] = -dt(0.5) * (Rbw1 @ dG) * tt * tt
    v1, v2 = st["vel"][a["kf1"]], st["vel"][a["kf2"]]
    p1, p2 = a["twb"][a["kf1"]], a["twb"][a["kf2"]]
    J[:, 3:6, 14] = np.einsum("mij,mj->mi", Rbw1, v2 - v1)                              # no factor s: as written (:716)
    J[:, 6:9, 14] = np.einsum("mij,mj->mi", Rbw1, p2 - p1 - v1 * a["dT"][:, None])      # (:717)
    return e, J


def oplus(pr, st, u_vel, u_border, dt):
    """the update of every vertex: velocities and biases by addition, Rwg <- Rwg ExpSO3(u0, u1, 0), s <- s exp(u)"""
    n = dict(st)
    n["vel"] = st["vel"] + u_vel
    if pr["free_bias"]:
        n["bg"] = st["bg"] + u_border[0:3]; n["ba"] = st["ba"] + u_border[3:6]
    if pr["free_gdir"]:
        n["Rwg"] = st["Rwg"] @ exp_so3(np.array([u_border[6], u_border[7], 0], dt))
    if pr["free_scale"]:
        n["scale"] = st["scale"] * np.exp(u_border[8])
    return n


class Layout:
    """where the free unknowns sit in the dense system"""

    def __init__(self, pr, a, n_kf, reverse):
        in_link = np.zeros(n_kf, bool)
        in_link[a["kf1"]] = True; in_link[a["kf2"]] = True
        self.vel_kf = np.flatnonzero(in_link) if pr["free_vel"] else np.zeros(0, int)
        nv = 3 * len(self.vel_kf)
        self.vcol = -np.ones(n_kf, int)
        self.vcol[self.vel_kf] = 3 * np.arange(len(self.vel_kf))
        free9 = np.array([bool(pr["free_bias"])] * 6 + [bool(pr["free_gdir"])] * 2 + [bool(pr["free_scale"])])
        self.border = np.flatnonzero(free9)
        self.bcol = -np.ones(9, int)
        self.bcol[self.border] = nv + np.arange(len(self.border))
        self.n = nv + len(self.border)
        self.perm = np.arange(self.n)[::-1] if reverse else np.arange(self.n)
        self.priors = bool(pr["free_bias"])

    def link_cols(self, k1, k2):
        """dense column of each of a link's 15 Jacobian columns, -1: fixed"""
        c = -np.ones(15, int)
        if self.vcol[k1] >= 0:
            c[0:3] = self.vcol[k1] + np.arange(3); c[3:6] = self.vcol[k2] + np.arange(3)
        c[6:15] = self.bcol
        return c

    def split(self, x, n_kf, dt):
        u_vel = np.zeros((n_kf, 3), dt)
        if len(self.vel_kf):
            u_vel[self.vel_kf] = x[:3 * len(self.vel_kf)].reshape(-1, 3)
        u_b = np.zeros(9, dt)
        u_b[self.border] = x[3 * len(self.vel_kf):]
        return u_vel, u_b


def chi2_of(pr, a, st, dt):
    """active robust chi2: the links (Huber on the robust ones) and, while the biases are free, the two priors"""
    e = errors(a, st, dt)
    chi = np.einsum("mi,mij,mj->m", e, a["info9"], e)
    rho0, _ = huber(chi, dt(pr.get("huber_delta", 0.0)), a["robust"])
    total = rho0.sum()
    if pr["free_bias"]:
        total = total + dt(pr["prior_a"]) * (st["ba"] * st["ba"]).sum() + dt(pr["prior_g"]) * (st["bg"] * st["bg"]).sum()
    return total


def linearize(pr, a, st, lay, dt):
    """robust chi2, dense H and b over the free unknowns (constructQuadraticForm: H += J^T rho' Omega J, b -= J^T rho' Omega e)"""
    e, J = jacobians(a, st, dt)
    chi = np.einsum("mi,mij,mj->m", e, a["info9"], e)
    rho0, rho1 = huber(chi, dt(pr.get("huber_delta", 0.0)), a["robust"])
    W = a["info9"] * rho1[:, None, None]
    Hl = np.swapaxes(J, -1, -2) @ W @ J
    bl = -np.einsum("mji,mj->mi", J, np.einsum("mij,mj->mi", W, e))
    H = np.zeros((lay.n, lay.n), dt); b = np.zeros(lay.n, dt)
    for l in range(len(e)):
        c = lay.link_cols(a["kf1"][l], a["kf2"][l])
        sel = np.flatnonzero(c >= 0)
        H[np.ix_(c[sel], c[sel])] += Hl[l][np.ix_(sel, sel)]
        b[c[sel]] += bl[l][sel]
    total = rho0.sum()
    if lay.priors:
        for k in range(3):
            H[lay.bcol[k], lay.bcol[k]] += dt(pr["prior_g"]); b[lay.bcol[k]] -= dt(pr["prior_g"]) * st["bg"][k]
            H[lay.bcol[3 + k], lay.bcol[3 + k]] += dt(pr["prior_a"]); b[lay.bcol[3 + k]] -= dt(pr["prior_a"]) * st["ba"][k]
        total = total + dt(pr["prior_a"]) * (st["ba"] * st["ba"]).sum() + dt(pr["prior_g"]) * (st["bg"] * st["bg"]).sum()
    return dict(chi2=total, H=H, b=b, e=e, J=J)


def solve_spd(A, b, dt):
    """A x = b by Cholesky; None unless A is positive definite.  Long double: the f64 factor, refined with long-double residuals."""
    try:
        c = scipy.linalg.cho_factor(A.astype(np.float64), lower=True)
    except (np.linalg.LinAlgError, ValueError):
        return None
    x = scipy.linalg.cho_solve(c, b.astype(np.float64)).astype(dt)
    if dt is not np.float64:
        for _ in range(4):
            x = x + scipy.linalg.cho_solve(c, (b - A @ x).astype(np.float64)).astype(dt)
    return x if np.isfinite(x).all() else None


def optimize(pr, dt=np.float64, reverse=False):
    """initializeOptimization(); optimize(max_iters) with Levenberg (lambda_0 = lambda_init, or 1e-5 max diag H when that is 0) or
    Gauss-Newton.  Returns the estimates, chi2 initial / final, the flow (iterations, trials, stop reason, lambda_0, lambda) and
    flow_margin: the smallest relative margin of a Levenberg decision (the sign of rho: |chi2 - trial chi2| / chi2; the 1e-3 gain
    rule: |1000 gain - chi2| / chi2).  A run whose margin exceeds the chi2 deviation a test allows cannot take another flow."""
    st = initial_state(pr, dt)
    n_kf = len(st["vel"])
    out_stats = dict(iterations=0, trials=0, stop_reason=0, lambda_0=None, lambda_=dt(0))
    if len(pr["links"]) == 0:
        return dict(vel=st["vel"], bg=st["bg"], ba=st["ba"], Rwg=st["Rwg"], scale=st["scale"], chi2_initial=dt(0), chi2_final=dt(0), flow_margin=np.inf, stats=out_stats)
    a = arrays_of(pr, dt)
    lay = Layout(pr, a, n_kf, reverse)
    gn = bool(pr.get("gauss_newton", 0))
    chi_initial = cur = chi2_of(pr, a, st, dt)
    lam = dt(0); lam0 = None
    ni = dt(2)
    n_bad = 0
    iterations = trials = stop_reason = 0
    trace = []
    flow_margin = np.inf
    P = lay.perm

    def solve(H, b, lam):
        A = (H + lam * np.eye(lay.n, dtype=dt))[np.ix_(P, P)]
        xp = solve_spd(A, b[P], dt)
        if xp is None:
            return None
        x = np.zeros(lay.n, dt)
        x[P] = xp
        return x

    for it in range(int(pr["max_iters"])):
        L = linearize(pr, a, st, lay, dt)
        cur = ini = L["chi2"]
        if gn:
            x = solve(L["H"], L["b"], dt(0))
            iterations += 1; trials += 1
            if x is None:
                stop_reason = 4
                break
            st = oplus(pr, st, *lay.split(x, n_kf, dt), dt)
            cur = chi2_of(pr, a, st, dt)
            trace.append(cur)
            continue
        if it == 0:
            lam = lam0 = dt(pr["lambda_init"]) if pr["lambda_init"] > 0 else dt(1e-5) * np.abs(np.diag(L["H"])).max()
        rho = dt(0)
        qmax = 0
        while True:
            x = solve(L["H"], L["b"], lam)
            if x is None:
                chi_new = dt(np.finfo(np.float64).max); trial = st
                scale = dt(1e-3)
            else:
                trial = oplus(pr, st, *lay.split(x, n_kf, dt), dt)
                chi_new = chi2_of(pr, a, trial, dt)
                scale = (x * (lam * x + L["b"])).sum() + dt(1e-3)
            rho = (cur - chi_new) / scale
            flow_margin = min(flow_margin, float(abs(cur - chi_new) / max(abs(cur), 1e-300)))
            if bool(rho > 0) and bool(np.isfinite(chi_new)):
                alpha = min(1 - (2 * rho - 1) ** 3, dt(2) / 3)
                lam = lam * max(dt(1) / 3, alpha)
                ni = dt(2)
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
        flow_margin = min(flow_margin, float(abs((ini - cur) * 1000 - ini) / max(abs(ini), 1e-300)))
        n_bad = n_bad + 1 if (ini - cur) * 1000 < ini else 0
        if n_bad >= 3:
            stop_reason = 2
            break
    # a key frame in no link has no active edge: its velocity is the input's
    return dict(vel=st["vel"], bg=st["bg"], ba=st["ba"], Rwg=st["Rwg"], scale=st["scale"], chi2_initial=chi_initial, chi2_final=cur,
                flow_margin=flow_margin, stats=dict(iterations=iterations, trials=trials, stop_reason=stop_reason, lambda_0=lam0, lambda_=lam, chi2_trace=trace))
