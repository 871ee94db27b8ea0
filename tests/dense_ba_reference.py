"""Dense long-double reference for the visual solvers: LocalBA (lba_solve, lba_solve_batch, lba_shard_optimize) and
PoseOptimization (pose_optimize_batch).  A test helper, not a test.

Independent of oracle/: numpy in np.longdouble, float64 inputs, every residual, Jacobian, robust weight and the Levenberg
first trial restated from the reference text (cited file:line, read as text; nothing copied), the system assembled densely
(points eliminated exactly per landmark), solved in f64 by LAPACK and refined with long-double residuals.

Follows:
  src/OptimizableTypes.cpp:139-160, src/CameraModels/Pinhole.cpp:43-49,71-81   EdgeSE3ProjectXYZ (mono), double projection
  Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:189-197,237-274              EdgeStereoSE3ProjectXYZ, float invz / float bf
  Thirdparty/g2o/g2o/types/types_six_dof_expmap.cpp:293-316,338-380              ...OnlyPose variants (double bf)
  Thirdparty/g2o/g2o/types/se3quat.h:223-257                                     SE3Quat::exp (small-angle branch I+O+O^2, V=R)
  Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:73-76, types_sba.h:52-56      oplus: left exp * T; points additive
  Thirdparty/g2o/g2o/core/base_binary_edge.hpp:75-100, base_unary_edge.hpp:56-62 rho'*Omega in H, rho'*Omega*e in b
  Thirdparty/g2o/g2o/core/robust_kernel_impl.cpp:65-91                           Huber robustify
  Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:94-160,171-194   lambda init, first trial, rho, scale + 1e-3
  src/Optimizer.cc:814-1115                                                      PoseOptimization rounds, float chi2 thresholds
"""
import numpy as np
import scipy.linalg

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is no wider than float64 here: the reference would lose its precision silently"

CHI2_MONO = float(np.float32(5.991))       # Optimizer.cc:836-837, const float chi2Mono[4] / chi2Stereo[4]
CHI2_STEREO = float(np.float32(7.815))


# ------------------------------------------------------------------------------------------------ SO(3) / SE(3) in long double
def skew(v):
    v = np.asarray(v, LD)
    z = np.zeros(v.shape[:-1], LD)
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def quat_to_R(q):
    """(x, y, z, w) -> R, normalised in long double"""
    q = np.asarray(q, LD)
    q = q / np.sqrt((q * q).sum(-1, keepdims=True))
    x, y, z, w = q[..., 0], q[..., 1], q[..., 2], q[..., 3]
    return np.stack([np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)], -1),
                     np.stack([2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)], -1),
                     np.stack([2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)], -1)], -2)


def inv3(A):
    """closed-form inverse of (..., 3, 3) long-double matrices (numpy.linalg has no long double)"""
    a = A
    c00 = a[..., 1, 1] * a[..., 2, 2] - a[..., 1, 2] * a[..., 2, 1]
    c01 = a[..., 1, 2] * a[..., 2, 0] - a[..., 1, 0] * a[..., 2, 2]
    c02 = a[..., 1, 0] * a[..., 2, 1] - a[..., 1, 1] * a[..., 2, 0]
    det = a[..., 0, 0] * c00 + a[..., 0, 1] * c01 + a[..., 0, 2] * c02
    adj = np.stack([np.stack([c00, a[..., 0, 2] * a[..., 2, 1] - a[..., 0, 1] * a[..., 2, 2], a[..., 0, 1] * a[..., 1, 2] - a[..., 0, 2] * a[..., 1, 1]], -1),
                    np.stack([c01, a[..., 0, 0] * a[..., 2, 2] - a[..., 0, 2] * a[..., 2, 0], a[..., 0, 2] * a[..., 1, 0] - a[..., 0, 0] * a[..., 1, 2]], -1),
                    np.stack([c02, a[..., 0, 1] * a[..., 2, 0] - a[..., 0, 0] * a[..., 2, 1], a[..., 0, 0] * a[..., 1, 1] - a[..., 0, 1] * a[..., 1, 0]], -1)], -2)
    return adj / det[..., None, None]


def so3_exp(w):
    """exact Rodrigues exponential"""
    w = np.asarray(w, LD)
    th = np.sqrt((w * w).sum())
    O = skew(w)
    if th == 0:
        return np.eye(3, dtype=LD)
    return np.eye(3, dtype=LD) + np.sin(th) / th * O + (1 - np.cos(th)) / (th * th) * (O @ O)


def so3_log(R):
    v = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], LD) / 2
    s = np.sqrt((v * v).sum())
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2
    th = np.arctan2(s, c)
    return v if s == 0 else v * (th / s)


def se3_exp_g2o(u):
    """SE3Quat::exp (se3quat.h:223-257): update = (omega, upsilon).  Below theta = 1e-5 g2o takes R = I + O + O^2 and V = R;
    the SE3Quat constructor turns R into a unit quaternion (Eigen's Shepperd branch for trace > 0, then normalises)."""
    u = np.asarray(u, LD)
    om, up = u[:3], u[3:]
    th = np.sqrt((om * om).sum())
    O = skew(om)
    O2 = O @ O
    I = np.eye(3, dtype=LD)
    if th < 1e-5:
        R = I + O + O2
        V = R
    else:
        R = I + np.sin(th) / th * O + (1 - np.cos(th)) / (th * th) * O2
        V = I + (1 - np.cos(th)) / (th * th) * O + (th - np.sin(th)) / th ** 3 * O2
    t = np.sqrt(R[0, 0] + R[1, 1] + R[2, 2] + 1)
    q = np.array([(R[2, 1] - R[1, 2]) / (2 * t), (R[0, 2] - R[2, 0]) / (2 * t), (R[1, 0] - R[0, 1]) / (2 * t), t / 2], LD)
    return quat_to_R(q), V @ up


def se3_exp(u):
    """exact SE(3) exponential, (omega, upsilon) order"""
    u = np.asarray(u, LD)
    om, up = u[:3], u[3:]
    th = np.sqrt((om * om).sum())
    O = skew(om)
    I = np.eye(3, dtype=LD)
    if th == 0:
        return I, up.copy()
    V = I + (1 - np.cos(th)) / (th * th) * O + (th - np.sin(th)) / th ** 3 * (O @ O)
    return so3_exp(om), V @ up


def se3_log(R, t):
    om = so3_log(R)
    th = np.sqrt((om * om).sum())
    O = skew(om)
    I = np.eye(3, dtype=LD)
    V = I if th == 0 else I + (1 - np.cos(th)) / (th * th) * O + (th - np.sin(th)) / th ** 3 * (O @ O)
    return np.concatenate([om, inv3(V) @ np.asarray(t, LD)])


def pose_tangent(R1, t1, R0, t0):
    """log(T1 * T0^-1): the left update that takes T0 to T1"""
    dR = R1 @ R0.T
    return se3_log(dR, t1 - dR @ t0)


# ------------------------------------------------------------------------------------------------ camera edges
def project_residual(Xc, obs, stereo, cam, float_invz=True, float_bf=True):
    """obs - cam_project(Xc) for mono and stereo edges, (E, 3) with 0 in the third row of a mono edge.
    mono: Pinhole::project in double (Pinhole.cpp:43-49).  stereo: invz = 1.0f / z rounded to float
    (types_six_dof_expmap.cpp:190,340); bf is a float in the binary edge's cam_project (:189) and a double member in the
    OnlyPose edge.  float_invz=False gives the smooth variant that central differences need."""
    Xc = np.asarray(Xc, LD)
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    fx, fy, cx, cy = (LD(cam[k]) for k in ("fx", "fy", "cx", "cy"))
    obs = np.asarray(obs, LD)
    st = np.asarray(stereo).astype(bool)
    r = np.zeros((len(Xc), 3), LD)
    r[:, 0] = obs[:, 0] - (fx * x / z + cx)
    r[:, 1] = obs[:, 1] - (fy * y / z + cy)
    if st.any():
        zs = z[st]
        if float_invz:
            invz32 = (1.0 / zs.astype(np.float64)).astype(np.float32)
            invz = invz32.astype(LD)
            # binary edge: const float &bf times float invz is a float product; OnlyPose: double bf times float invz
            bfz = (np.float32(cam["bf"]) * invz32).astype(LD) if float_bf else LD(cam["bf"]) * invz
        else:
            invz = 1 / zs
            bfz = LD(cam["bf"]) * invz
        u = x[st] * invz * fx + cx
        v = y[st] * invz * fy + cy
        r[st, 0] = obs[st, 0] - u
        r[st, 1] = obs[st, 1] - v
        r[st, 2] = obs[st, 2] - (u - bfz)
    return r


def project_jacobians(Xc, R, stereo, cam):
    """the reference's analytic linearizeOplus: (J_point (E,3,3), J_pose (E,3,6)) of the error, rows beyond a mono edge's 2
    are zero.  Mono: -projectJac * R and -projectJac * [-[Xc]x | I] (OptimizableTypes.cpp:149-159).  Stereo:
    types_six_dof_expmap.cpp:251-273 (binary) and 359-379 (OnlyPose, same values); the third row adds the bf/z terms."""
    Xc = np.asarray(Xc, LD)
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    fx, fy, bf = LD(cam["fx"]), LD(cam["fy"]), LD(cam["bf"])
    E = len(Xc)
    st = np.asarray(stereo).astype(bool)
    P = np.zeros((E, 3, 3), LD)                 # d(projection)/d(Xc)
    P[:, 0, 0] = fx / z
    P[:, 0, 2] = -fx * x / (z * z)
    P[:, 1, 1] = fy / z
    P[:, 1, 2] = -fy * y / (z * z)
    P[st, 2, 0] = P[st, 0, 0]
    P[st, 2, 2] = P[st, 0, 2] + bf / (z[st] * z[st])
    S = np.zeros((E, 3, 6), LD)                 # d(exp(xi) Xc)/d(xi) = [-[Xc]x | I]
    S[:, :, :3] = -skew(Xc)
    S[:, :, 3:] = np.eye(3, dtype=LD)
    Jp = -np.einsum("eij,ejk->eik", P, np.broadcast_to(np.asarray(R, LD), (E, 3, 3)) if np.ndim(R) == 2 else np.asarray(R, LD))
    Jx = -np.einsum("eij,ejk->eik", P, S)
    return Jp, Jx


def huber(chi2, delta):
    """RobustKernelHuber::robustify (robust_kernel_impl.cpp:65-91): (rho, rho'); delta <= 0 means no kernel"""
    chi2 = np.asarray(chi2, LD)
    delta = np.broadcast_to(np.asarray(delta, LD), chi2.shape)
    dsqr = delta * delta
    big = (delta > 0) & (chi2 > dsqr)
    s = np.sqrt(np.where(big, chi2, 1))
    return np.where(big, 2 * s * delta - dsqr, chi2), np.where(big, delta / s, LD(1))


# ------------------------------------------------------------------------------------------------ LocalBA window
def _window_state(w):
    R = quat_to_R(w["pose_q"])
    t = np.asarray(w["pose_t"], LD)
    return R, t, np.asarray(w["points"], LD)


def lba_edges(w, R, t, X, float_invz=True):
    """per-edge Xc, residual, chi2 (information invSigma2 * I) at the state (R, t, X)"""
    ep, el = w["edge_pose"], w["edge_point"]
    Xc = np.einsum("eij,ej->ei", R[ep], X[el]) + t[ep]
    r = project_residual(Xc, w["edge_obs"], w["edge_stereo"], w, float_invz=float_invz)
    chi2 = np.asarray(w["edge_inv_sigma2"], LD) * (r * r).sum(1)
    return Xc, r, chi2


def lba_robust_chi2(w, R, t, X):
    """activeRobustChi2 and the per-edge chi2 at (R, t, X)"""
    _, _, chi2 = lba_edges(w, R, t, X)
    delta = np.where(np.asarray(w["edge_stereo"]).astype(bool), w["huber_stereo"], w["huber_mono"])
    return huber(chi2, delta)[0].sum(), chi2


def lba_first_trial(w, lambda_user=0.0, refine=3):
    """The first Levenberg trial of LocalBA: H, b in long double with rho'*Omega (base_binary_edge.hpp:91-100),
    lambda = user value or 1e-5 * max diag H (levenberg.cpp:94,171-185), (H + lambda I) dx = b with the points eliminated
    per landmark, the update through SE3Quat::exp, rho with the +1e-3 in the scale (:130-131) and the lambda after it.
    Returns the step (per free pose the tangent log(T1 T0^-1), per point the delta) with the solve's own accuracy:
    kappa = 2-norm condition of the reduced (Schur) system, resid = its relative residual after refinement."""
    R0, t0, X0 = _window_state(w)
    free = np.asarray(w["pose_fixed"]) == 0
    col = np.cumsum(free) - 1
    nP, nL = int(free.sum()), len(X0)
    ep, el = np.asarray(w["edge_pose"]), np.asarray(w["edge_point"])
    Xc, r, chi2 = lba_edges(w, R0, t0, X0)
    st = np.asarray(w["edge_stereo"]).astype(bool)
    rho0, rho1 = huber(chi2, np.where(st, w["huber_stereo"], w["huber_mono"]))
    Jp, Jx = project_jacobians(Xc, R0[ep], st, w)
    wgt = rho1 * np.asarray(w["edge_inv_sigma2"], LD)          # rho' * Omega (Omega = invSigma2 * I)
    Hll = np.zeros((nL, 3, 3), LD); bl = np.zeros((nL, 3), LD)
    np.add.at(Hll, el, np.einsum("edi,e,edj->eij", Jp, wgt, Jp))
    np.add.at(bl, el, -np.einsum("edi,e,ed->ei", Jp, wgt, r))
    fe = np.nonzero(free[ep])[0]
    pc = col[ep[fe]]
    Hpp = np.zeros((nP, 6, 6), LD); bp = np.zeros((nP, 6), LD)
    np.add.at(Hpp, pc, np.einsum("edi,e,edj->eij", Jx[fe], wgt[fe], Jx[fe]))
    np.add.at(bp, pc, -np.einsum("edi,e,ed->ei", Jx[fe], wgt[fe], r[fe]))
    W = np.einsum("edi,e,edj->eij", Jx[fe], wgt[fe], Jp[fe])    # 6x3 pose-point blocks
    if lambda_user > 0:
        lam = LD(lambda_user)
    else:
        diag = np.concatenate([np.diagonal(Hpp, axis1=1, axis2=2).ravel(), np.diagonal(Hll, axis1=1, axis2=2).ravel()])
        lam = LD(1e-5) * np.abs(diag).max()
    I3, I6 = np.eye(3, dtype=LD), np.eye(6, dtype=LD)
    Dinv = inv3(Hll + lam * I3)
    # reduced system S xp = bs over the free poses, points eliminated exactly
    n = 6 * nP
    S = np.zeros((nP, 6, nP, 6), LD)
    for i in range(nP):
        S[i, :, i, :] = Hpp[i] + lam * I6
    WD = np.einsum("eij,ejk->eik", W, Dinv[el[fe]])
    bs = bp.copy()
    np.add.at(bs, pc, -np.einsum("eij,ej->ei", WD, bl[el[fe]]))
    order = np.argsort(el[fe], kind="stable")
    lf = el[fe][order]
    starts = np.searchsorted(lf, np.arange(nL + 1))
    ia, ib = [], []
    for l in range(nL):
        es = order[starts[l]:starts[l + 1]]
        if len(es):
            a, b = np.meshgrid(es, es, indexing="ij")
            ia.append(a.ravel()); ib.append(b.ravel())
    if ia:
        ia, ib = np.concatenate(ia), np.concatenate(ib)
        blocks = np.einsum("pij,pkj->pik", WD[ia], W[ib])
        Sv = S.transpose(0, 2, 1, 3)                            # view (nP, nP, 6, 6)
        np.add.at(Sv, (pc[ia], pc[ib]), -blocks)
    S = S.reshape(n, n)
    bs = bs.reshape(n)
    xp, resid, kappa = solve_refined(S, bs, refine)
    xl = np.einsum("lij,lj->li", Dinv, bl - _scatter_wtx(W, xp.reshape(nP, 6), pc, el[fe], nL))
    # update (oplus) and the trial's chi2, rho, lambda
    R1, t1 = R0.copy(), t0.copy()
    tang = np.zeros((nP, 6), LD)
    for i in np.nonzero(free)[0]:
        dR, dt = se3_exp_g2o(xp[6 * col[i]:6 * col[i] + 6])
        R1[i], t1[i] = dR @ R0[i], dR @ t0[i] + dt
        tang[col[i]] = pose_tangent(R1[i], t1[i], R0[i], t0[i])
    X1 = X0 + xl
    chi_ini = rho0.sum()
    chi_new, _ = lba_robust_chi2(w, R1, t1, X1)
    scale = (xp * (lam * xp + bp.reshape(n))).sum() + (xl * (lam * xl + bl)).sum() + LD(1e-3)
    rho = (chi_ini - chi_new) / scale
    lam_next = lam * max(LD(1) / 3, min(LD(2) / 3, 1 - (2 * rho - 1) ** 3)) if rho > 0 else lam * 2
    diag_pose = float(np.abs(np.diagonal(Hpp, axis1=1, axis2=2)).max()) if nP else 0.0
    diag_point = float(np.abs(np.diagonal(Hll, axis1=1, axis2=2)).max()) if nL else 0.0
    return dict(pose_step=tang, point_step=xl, R1=R1, t1=t1, X1=X1, chi2_initial=chi_ini, chi2_final=chi_new, rho=rho,
                max_diag_pose=diag_pose, max_diag_point=diag_point,
                lambda_init=lam, lambda_=lam_next, kappa=kappa, resid=resid, x_pose=xp.reshape(nP, 6))


def _scatter_wtx(W, xp, pc, el, nL):
    out = np.zeros((nL, 3), LD)
    np.add.at(out, el, np.einsum("eij,ei->ej", W, xp[pc]))
    return out


def solve_refined(A, b, rounds=3):
    """A x = b: LU in f64 (LAPACK), then `rounds` of iterative refinement with long-double residuals.
    Returns (x, |b - A x| / |b| in long double, 2-norm condition estimate of A)."""
    n = len(b)
    if n == 0:
        return np.zeros(0, LD), LD(0), 1.0
    A = np.asarray(A, LD); b = np.asarray(b, LD)
    lu = scipy.linalg.lu_factor(A.astype(np.float64))
    x = scipy.linalg.lu_solve(lu, b.astype(np.float64)).astype(LD)
    for _ in range(rounds):
        res = b - A @ x
        x = x + scipy.linalg.lu_solve(lu, res.astype(np.float64)).astype(LD)
    res = b - A @ x
    rel = np.sqrt((res * res).sum() / (b * b).sum()) if (b != 0).any() else LD(0)
    return x, rel, float(np.linalg.cond(A.astype(np.float64)))


def lba_state_from(out, w):
    """(R, t, X) of a solver output dict (pose_q, pose_t, points) in long double"""
    return quat_to_R(out["pose_q"]), np.asarray(out["pose_t"], LD), np.asarray(out["points"], LD)


def lba_step_error(w, out, ref):
    """worst per-block relative error of a solver's one-step output against lba_first_trial: per free pose
    |log(T1 T0^-1) - step_ref| / |step_ref|, per point |dX - dX_ref| / |dX_ref|"""
    R0, t0, X0 = _window_state(w)
    R1, t1, X1 = lba_state_from(out, w)
    free = np.nonzero(np.asarray(w["pose_fixed"]) == 0)[0]
    worst = 0.0
    for k, i in enumerate(free):
        d = pose_tangent(R1[i], t1[i], R0[i], t0[i]) - ref["pose_step"][k]
        worst = max(worst, float(np.sqrt((d * d).sum() / (ref["pose_step"][k] ** 2).sum())))
    d = (X1 - X0) - ref["point_step"]
    nrm = np.sqrt((ref["point_step"] ** 2).sum(1))
    if len(nrm):
        worst = max(worst, float((np.sqrt((d * d).sum(1)) / nrm).max()))
    return worst


def step_tolerance(kappa):
    """per-block relative tolerance on a well-conditioned step: an f64 factorisation loses about kappa * 2^-53; 100 covers the
    accumulation order, 1e-9 is the floor below which the float-rounded stereo residuals leave nothing to compare"""
    return max(1e-9, 100.0 * kappa * 2.0 ** -53)


# ------------------------------------------------------------------------------------------------ PoseOptimization
def pose_problem_edges(w, R, t, float_invz=True):
    Xc = np.asarray(w["Xw"], LD) @ R.T + t
    r = project_residual(Xc, w["obs"], w["stereo"], w, float_invz=float_invz, float_bf=False)
    return Xc, r


def pose_newton_step(w, q, t, active):
    """Newton step H^-1 g of the PoseOptimization cost over `active` edges without robust kernel (the last round,
    Optimizer.cc:1036-1038) at the pose (q, t), and the total update log(T T0^-1) from the frame's initial pose."""
    R = quat_to_R(q); t = np.asarray(t, LD)
    act = np.asarray(active).astype(bool)
    sub = {k: (np.asarray(w[k])[act] if k in ("Xw", "obs", "inv_sigma2", "stereo") else w[k]) for k in w}
    Xc, r = pose_problem_edges(sub, R, t)
    _, Jx = project_jacobians(Xc, R, sub["stereo"], sub)
    om = np.asarray(sub["inv_sigma2"], LD)
    H = np.einsum("edi,e,edj->ij", Jx, om, Jx)
    g = np.einsum("edi,e,ed->i", Jx, om, r)
    step, _, kappa = solve_refined(H, -g)
    R0 = quat_to_R(w["q"]); t0 = np.asarray(w["t"], LD)
    return step, pose_tangent(R, t, R0, t0), kappa


def pose_chi2(w, q, t):
    """per-edge chi2 at (q, t), compared in float as the reference does (Optimizer.cc:1018-1030)"""
    _, r = pose_problem_edges(w, quat_to_R(q), np.asarray(t, LD))
    return np.asarray(w["inv_sigma2"], LD) * (r * r).sum(1)


# ------------------------------------------------------------------------------------------------ checks shared by the CPU and GPU tests
def interleaved_window(synth, seed, n_opt, stereo_frac=0.3, n_points=None, obs=5):
    """make_ba_window with fixed key frames interleaved among the free ones (every third pose fixed)"""
    n_fixed = max(2, n_opt // 3)
    w = synth.make_ba_window(seed, n_opt=n_opt, n_fixed=n_fixed, n_points=n_points or 20 * (n_opt + n_fixed), obs_per_point=obs,
                             stereo_frac=stereo_frac, outlier_frac=0.05)
    n = n_opt + n_fixed
    fixed = np.zeros(n, np.uint8)
    fixed[np.linspace(1, n - 1, n_fixed).astype(int)] = 1
    w["pose_fixed"] = fixed
    return w


def check_one_step(w, r, ref, tol=None):
    """a solver's one-step output (lba_solve(w, 1, lambda)) against lba_first_trial: returns the step error"""
    st = r["stats"]
    assert st["iterations"] == 1 and st["trials"] == 1 and ref["rho"] > 0
    # chi2 sums and lambda: the reference sums in long double, the solvers in f64 over a few thousand edges
    np.testing.assert_allclose(st["chi2_initial"], float(ref["chi2_initial"]), rtol=1e-12)
    np.testing.assert_allclose(st["chi2_final"], float(ref["chi2_final"]), rtol=1e-11)
    np.testing.assert_allclose(st["lambda_"], float(ref["lambda_"]), rtol=1e-12)
    assert ref["resid"] < 1e-15, "reference solve residual %.3g" % ref["resid"]
    err = lba_step_error(w, r, ref)
    tol = step_tolerance(ref["kappa"]) if tol is None else tol
    assert err <= tol, "step error %.3g > %.3g (kappa %.3g)" % (err, tol, ref["kappa"])
    # per-edge chi2 at the returned state, restated
    _, pe = lba_robust_chi2(w, *lba_state_from(r, w))
    np.testing.assert_allclose(r["chi2"], pe.astype(np.float64), rtol=1e-9, atol=1e-10)
    return err


def pose_stationarity(w, res):
    """|Newton step| / |total update| of the last round's cost at the returned pose, and the bound it must meet: 1e-9, plus for
    stereo edges 10 x the Newton step that the float 1/z rounding contributes at that pose, H^-1 J^T Omega (r_float - r_exact):
    the float cost is flat to that level and Levenberg stops anywhere on the plateau (observed up to 2.4 x the estimate)"""
    act = ~np.asarray(w["is_outlier"], bool)
    step, total, kappa = pose_newton_step(w, res["q"], res["t"], act)
    tn = np.sqrt((total * total).sum())
    ratio = float(np.sqrt((step * step).sum()) / tn)
    floor = 0.0
    if w["stereo"][act].any():
        sub = {k: (np.asarray(w[k])[act] if k in ("Xw", "obs", "inv_sigma2", "stereo") else w[k]) for k in w}
        R, t = quat_to_R(res["q"]), np.asarray(res["t"], LD)
        Xc, r_float = pose_problem_edges(sub, R, t)
        r_exact = project_residual(Xc, sub["obs"], sub["stereo"], sub, float_invz=False, float_bf=False)
        _, Jx = project_jacobians(Xc, R, sub["stereo"], sub)
        om = np.asarray(sub["inv_sigma2"], LD)
        H = np.einsum("edi,e,edj->ij", Jx, om, Jx)
        d, _, _ = solve_refined(H, np.einsum("edi,e,ed->i", Jx, om, r_float - r_exact))
        floor = float(10 * np.sqrt((d * d).sum()) / tn)
    return ratio, 1e-9 + floor, kappa


# ------------------------------------------------------------------------------------------------ windows
def make_far_window(seed, n_opt=10, n_fixed=2, n_points=200, obs_per_point=5, weak_obs=5, stereo_frac=0.0, baseline=0.3):
    """An ill-conditioned LocalBA window: points at 50-200 m depth seen from key frames on a short baseline, and the last
    free key frame kept to `weak_obs` observations.  Same field layout as synth.make_ba_window (inputs rounded through f32)."""
    rs = np.random.RandomState(777 + seed)
    fx, fy, cx, cy = [float(np.float32(v)) for v in (458.654, 457.296, 367.215, 248.375)]
    bf = float(np.float32(47.90639384423901))
    n_poses = n_opt + n_fixed
    pts = np.stack([rs.uniform(-40, 40, n_points), rs.uniform(-25, 25, n_points), rs.uniform(50, 200, n_points)], 1)
    Rs, ts = [], []
    for i in range(n_poses):
        c = np.array([baseline * (i / max(n_poses - 1, 1) - 0.5), 0.02 * np.sin(i), 0.02 * np.cos(i)])
        Rcw = _rot(np.array([0.01 * np.sin(1.3 * i), 0.02 * np.cos(0.7 * i), 0.005 * i])).T
        Rs.append(Rcw); ts.append(-Rcw @ c)
    Rs, ts = np.array(Rs), np.array(ts)
    weak = n_opt - 1
    e = dict(pt=[], pose=[], obs=[], w=[], st=[])
    weak_left = weak_obs
    for l in range(n_points):
        Xc = Rs @ pts[l] + ts
        cand = [i for i in rs.permutation(n_poses) if i != weak][:obs_per_point]
        if weak_left > 0 and l % 7 == 3:
            cand = cand[:-1] + [weak]
            weak_left -= 1
        for ip in sorted(cand):
            sig = 1.2 ** int(rs.randint(0, 3))
            u = fx * Xc[ip, 0] / Xc[ip, 2] + cx + rs.normal(0, sig)
            v = fy * Xc[ip, 1] / Xc[ip, 2] + cy + rs.normal(0, sig)
            s = rs.uniform() < stereo_frac
            ur = u - bf / Xc[ip, 2] + rs.normal(0, sig) if s else -1.0
            e["pt"].append(l); e["pose"].append(int(ip)); e["obs"].append([u, v, ur]); e["w"].append(1.0 / sig ** 2); e["st"].append(int(s))
    q0 = np.zeros((n_poses, 4)); t0 = np.zeros((n_poses, 3))
    fixed = np.zeros(n_poses, np.uint8); fixed[n_opt:] = 1
    for i in range(n_poses):
        R, t = Rs[i], ts[i]
        if not fixed[i]:
            dR = _rot(rs.normal(0, np.deg2rad(0.3), 3))
            R, t = dR @ R, dR @ t + rs.normal(0, 0.01, 3)
        q0[i] = _quat(R); t0[i] = t
    f32 = lambda a: np.asarray(a, np.float64).astype(np.float32).astype(np.float64)
    return dict(pose_q=f32(q0), pose_t=f32(t0), pose_fixed=fixed, points=f32(pts + rs.normal(0, 0.5, pts.shape)),
                edge_point=np.asarray(e["pt"], np.int32), edge_pose=np.asarray(e["pose"], np.int32), edge_obs=f32(e["obs"]),
                edge_inv_sigma2=f32(e["w"]), edge_stereo=np.asarray(e["st"], np.uint8), fx=fx, fy=fy, cx=cx, cy=cy, bf=bf,
                huber_mono=float(np.float32(np.sqrt(5.991))), huber_stereo=float(np.float32(np.sqrt(7.815))))


def lambda_windows(synth):
    """windows that pin the rest of the first trial: (a) rho = 0.90, inside (0.85, 0.94) where lambda' = lambda * (1 - (2 rho - 1)^3)
    is not clamped, so the +1e-3 in the scale (levenberg.cpp:130-131) moves lambda_ by ~1e-6; (b) the largest diagonal of H in a
    point block (levenberg.cpp:171-185 takes it over poses and points)"""
    a = interleaved_window(synth, 61, 9)
    a["huber_mono"] = a["huber_stereo"] = 0.0
    b = add_heavy_point(interleaved_window(synth, 62, 9))
    return [(a, 1.0), (b, 0.0)]


def add_heavy_point(w, weight=1e4, depth=2.0):
    """append one point seen only by the window's first two fixed key frames, with information `weight`, and switch the robust
    kernels off: its 3 x 3 diagonal then outweighs every free pose's, so the tau initialisation of lambda reads a point block"""
    w = dict(w)
    fixed = np.nonzero(np.asarray(w["pose_fixed"]) != 0)[0][:2]
    R = quat_to_R(w["pose_q"][fixed]).astype(np.float64)
    t = np.asarray(w["pose_t"], np.float64)[fixed]
    X = R[0].T @ (np.array([0.1, -0.05, depth]) - t[0])
    obs = []
    for k in range(2):
        Xc = R[k] @ X + t[k]
        obs.append([w["fx"] * Xc[0] / Xc[2] + w["cx"] + 0.3, w["fy"] * Xc[1] / Xc[2] + w["cy"] - 0.2, -1.0])
    n = len(w["points"])
    w["points"] = np.vstack([w["points"], X + 0.01])
    w["edge_point"] = np.concatenate([w["edge_point"], [n, n]]).astype(np.int32)
    w["edge_pose"] = np.concatenate([w["edge_pose"], fixed]).astype(np.int32)
    w["edge_obs"] = np.vstack([w["edge_obs"], obs])
    w["edge_inv_sigma2"] = np.concatenate([w["edge_inv_sigma2"], [weight, weight]])
    w["edge_stereo"] = np.concatenate([w["edge_stereo"], [0, 0]]).astype(np.uint8)
    w["huber_mono"] = w["huber_stereo"] = 0.0
    return w


def _rot(wv):
    return so3_exp(np.asarray(wv, LD)).astype(np.float64)


def _quat(R):
    w = np.sqrt(max(1 + R[0, 0] + R[1, 1] + R[2, 2], 1e-300)) / 2
    return np.array([(R[2, 1] - R[1, 2]) / (4 * w), (R[0, 2] - R[2, 0]) / (4 * w), (R[1, 0] - R[0, 1]) / (4 * w), w])
