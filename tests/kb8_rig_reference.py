"""Numpy reference for a rig of two KannalaBrandt8 cameras in PoseOptimization and LocalBundleAdjustment: the left-camera edges of
kb8_reference.py plus the right-camera edges.  A test helper, not a test.

Restated from the reference text (read as text; nothing copied):
  include/OptimizableTypes.h:69-78      EdgeSE3ProjectXYZOnlyPoseToBody: obs - pCamera->project((mTrl * Tlw).map(Xw)); depth of that point
  src/OptimizableTypes.cpp:91-107       its Jacobian: -projectJac(X_r) * R_rl * SE3deriv(X_l)
  include/OptimizableTypes.h:127-138    EdgeSE3ProjectXYZToBody: the same error with the point a vertex
  src/OptimizableTypes.cpp:192-213      its Jacobians: -projectJac(X_r) * R_rw (point), -projectJac(X_r) * R_rl * SE3deriv(X_l) (pose)
  src/Optimizer.cc:929-991, 1296-1400   the two drivers add left and right edges interleaved; g2o sums them in that order
The camera functions, the Huber kernel, the dense LDL^T, the pose update, the Levenberg controller and the `perturb` /
`device_model` / `jitter` switches are those of kb8_reference.py, imported.

X_r is evaluated as R_rl X_l + t_rl (the map of the map, as the reference's linearizeOplus writes it) in the errors too, where the
reference composes mTrl * Tlw into one SE3Quat first.  The two differ by the rounding of a few f64 operations, which is what the
`jitter` switch models, and far less than the one float ulp of theta and psi that `perturb` moves at every evaluation.

A rig is a dict left, right (cameras as in kb8_reference), q_rl (xyzw, normalised here as the SE3Quat constructor does), t_rl.
The kind of an edge is 0 (left camera) or RIGHT.  With no right edge every function here performs the operations of its
kb8_reference counterpart with rig["left"], in the same order."""
import numpy as np

import kb8_reference as kr
from kb8_reference import CHI2_MONO_F32, Levenberg, _huber, _ldlt_solve, _quat_normalize, _R, _se3_rows, pose_oplus

RIGHT = 2


def rig_frames(rig):
    """(R_rl, t_rl) as float64"""
    return _R(_quat_normalize(rig["q_rl"])), np.asarray(rig["t_rl"], np.float64)


def to_right(rig, Xl):
    R_rl, t_rl = rig_frames(rig)
    return np.asarray(Xl, np.float64) @ R_rl.T + t_rl


def edge_project(rig, right, Xl, perturb=None, device_model=False):
    """project of each edge's own camera: (E, 2), and the point in that camera's frame (E, 3)"""
    Xp = np.array(Xl, np.float64)
    uv = np.zeros((len(Xp), 2))
    left = ~right
    if right.any():
        Xp[right] = to_right(rig, Xp[right])
    if left.any():
        uv[left] = kr.project(rig["left"], Xp[left], perturb, device_model)
    if right.any():
        uv[right] = kr.project(rig["right"], Xp[right], perturb, device_model)
    return uv, Xp


def edge_N(rig, right, Xl):
    """-projectJac of each edge's own camera at its own point, times R_rl on a right edge: (E, 2, 3)"""
    Xl = np.asarray(Xl, np.float64)
    N = np.zeros((len(Xl), 2, 3))
    left = ~right
    if left.any():
        N[left] = -kr.project_jac(rig["left"], Xl[left])
    if right.any():
        R_rl, _ = rig_frames(rig)
        N[right] = np.einsum("eij,jk->eik", -kr.project_jac(rig["right"], to_right(rig, Xl[right])), R_rl)
    return N


def pose_jacobian(rig, right, Xl):
    """d error / d pose of each edge (E, 2, 6)"""
    return _se3_rows(edge_N(rig, right, Xl), np.asarray(Xl, np.float64))


def point_jacobian(rig, right, Xl, R_lw):
    """d error / d point of each edge (E, 2, 3); R_lw (E, 3, 3)"""
    return np.einsum("eij,ejk->eik", edge_N(rig, right, Xl), R_lw)


# ------------------------------------------------------------------------------------------------ PoseOptimization
def pose_optimize(w, rig, perturb=None, device_model=False, jitter=None):
    """Optimizer::PoseOptimization of one rig frame: kb8_reference.pose_optimize with w["stereo"] the kind of every edge"""
    Xw = np.asarray(w["Xw"], np.float64); obs = np.asarray(w["obs"], np.float64)[:, :2]; om = np.asarray(w["inv_sigma2"], np.float64)
    right_all = np.asarray(w["stereo"]) != 0
    n = len(Xw)
    delta = float(w["huber_mono"])
    q0, t0 = _quat_normalize(w["q"]), np.asarray(w["t"], np.float64)
    q, t = q0, t0
    err = np.zeros((n, 2))
    active = np.ones(n, bool); outlier = np.zeros(n, bool)
    iters, trials, chis, margins = [0] * 4, [0] * 4, [0.0] * 4, []
    robust = True
    n_bad = 0

    def errors(q, t, idx):
        Xc = Xw[idx] @ _R(q).T + t
        if jitter is not None:
            Xc = Xc * (1 + 4e-16 * jitter.standard_normal(Xc.shape))
        return Xc, obs[idx] - edge_project(rig, right_all[idx], Xc, perturb, device_model)[0]

    for rnd in range(4 if n >= 3 else 0):
        q, t = q0, t0
        idx = np.nonzero(active)[0]
        if len(idx):
            lm = Levenberg()
            for it in range(10):
                Xc, r = errors(q, t, idx)
                err[idx] = r
                rho0, rho1 = _huber(om[idx] * (r * r).sum(1), delta, robust)
                J = pose_jacobian(rig, right_all[idx], Xc)
                H = np.einsum("edi,e,edj->ij", J, rho1 * om[idx], J)
                b = -np.einsum("edi,e,ed->i", J, rho1 * om[idx], r)
                lm.linearized(rho0.sum(), it == 0, 1e-5 * np.abs(np.diag(H)).max())
                while True:
                    x, ok = _ldlt_solve(H + lm.lam * np.eye(6), b)
                    if ok:
                        qt, tt = pose_oplus(q, t, x)
                    else:
                        qt, tt, x = q, t, np.zeros(6)
                    _, r = errors(qt, tt, idx)
                    err[idx] = r
                    tchi = _huber(om[idx] * (r * r).sum(1), delta, robust)[0].sum()
                    if lm.trial(ok, tchi, (x * (lm.lam * x + b)).sum()):
                        q, t = qt, tt
                    if not lm.more_trials():
                        break
                iters[rnd] += 1; trials[rnd] += lm.qmax; chis[rnd] = lm.cur
                if lm.stop():
                    break
        off = np.nonzero(outlier)[0]
        if len(off):
            err[off] = errors(q, t, off)[1]
        chi2 = (om * (err * err).sum(1)).astype(np.float32)
        margins.append(np.abs(chi2.astype(np.float64) - 5.991) / 5.991)
        outlier = chi2 > CHI2_MONO_F32
        active = ~outlier
        n_bad = int(outlier.sum())
        if rnd == 2:
            robust = False
        if n < 10:
            break
    return dict(q=q, t=t, outlier=outlier.astype(np.uint8), inliers=0 if n < 3 else n - n_bad, n_bad=n_bad, iterations=iters, trials=trials,
                chi2=chis, margins=np.array(margins))


# ------------------------------------------------------------------------------------------------ LocalBundleAdjustment
def lba_solve(w, rig, max_iters=10, lambda_init=0.0, perturb=None, device_model=False, jitter=None):
    """lba_solve of a rig window: kb8_reference.lba_solve with w["edge_stereo"] the kind of every edge; depth_positive of a right
    edge is that of X_r"""
    fixed = np.asarray(w["pose_fixed"]) != 0
    col = np.cumsum(~fixed) - 1
    nP, nL = int((~fixed).sum()), len(w["points"])
    ep, el = np.asarray(w["edge_pose"]), np.asarray(w["edge_point"])
    right = np.asarray(w["edge_stereo"]) != 0
    obs = np.asarray(w["edge_obs"], np.float64)[:, :2]; om = np.asarray(w["edge_inv_sigma2"], np.float64)
    delta = float(w["huber_mono"])
    q = np.array([_quat_normalize(v) for v in np.asarray(w["pose_q"], np.float64)])
    t = np.asarray(w["pose_t"], np.float64).copy()
    X = np.asarray(w["points"], np.float64).copy()
    fe = np.nonzero(~fixed[ep])[0]
    pc = col[ep[fe]]

    def errors(q, t, X):
        R = np.array([_R(v) for v in q])
        Xc = np.einsum("eij,ej->ei", R[ep], X[el]) + t[ep]
        if jitter is not None:
            Xc = Xc * (1 + 4e-16 * jitter.standard_normal(Xc.shape))
        return R, Xc, obs - edge_project(rig, right, Xc, perturb, device_model)[0]

    lm = Levenberg()
    stats = dict(iterations=0, trials=0, stop_reason=0, chi2_initial=0.0, chi2_final=0.0)
    r = np.zeros((len(ep), 2))
    for it in range(max_iters):
        R, Xc, r = errors(q, t, X)
        rho0, rho1 = _huber(om * (r * r).sum(1), delta)
        N = edge_N(rig, right, Xc)
        Ji = np.einsum("eij,ejk->eik", N, R[ep])
        Jj = _se3_rows(N, Xc)
        wgt = rho1 * om
        Hll = np.zeros((nL, 3, 3)); bl = np.zeros((nL, 3)); Hpp = np.zeros((nP, 6, 6)); bp = np.zeros((nP, 6))
        np.add.at(Hll, el, np.einsum("edi,e,edj->eij", Ji, wgt, Ji))
        np.add.at(bl, el, -np.einsum("edi,e,ed->ei", Ji, wgt, r))
        np.add.at(Hpp, pc, np.einsum("edi,e,edj->eij", Jj[fe], wgt[fe], Jj[fe]))
        np.add.at(bp, pc, -np.einsum("edi,e,ed->ei", Jj[fe], wgt[fe], r[fe]))
        W = np.einsum("edi,e,edj->eij", Jj[fe], wgt[fe], Ji[fe])
        mdp = np.abs(np.diagonal(Hpp, axis1=1, axis2=2)).max() if nP else 0.0
        mdl = np.abs(np.diagonal(Hll, axis1=1, axis2=2)).max() if nL else 0.0
        lm.linearized(rho0.sum(), it == 0, lambda_init if lambda_init > 0 else 1e-5 * max(mdp, mdl))
        if it == 0:
            stats["chi2_initial"] = lm.cur
        while True:
            lam = lm.lam
            Dinv = np.linalg.inv(Hll + lam * np.eye(3))
            S = np.zeros((nP, nP, 6, 6))
            for i in range(nP):
                S[i, i] = Hpp[i] + lam * np.eye(6)
            WD = np.einsum("eij,ejk->eik", W, Dinv[el[fe]])
            bs = bp.copy()
            np.add.at(bs, pc, -np.einsum("eij,ej->ei", WD, bl[el[fe]]))
            for l in range(nL):
                es = np.nonzero(el[fe] == l)[0]
                for a in es:
                    for b_ in es:
                        S[pc[a], pc[b_]] -= WD[a] @ W[b_].T
            Sd = S.transpose(0, 2, 1, 3).reshape(6 * nP, 6 * nP)
            try:
                np.linalg.cholesky(Sd)
                xp = np.linalg.solve(Sd, bs.reshape(-1)).reshape(nP, 6)
                solved = True
            except np.linalg.LinAlgError:
                xp = np.zeros((nP, 6)); solved = False
            Wx = np.zeros((nL, 3))
            np.add.at(Wx, el[fe], np.einsum("eij,ei->ej", W, xp[pc]))
            xl = np.einsum("lij,lj->li", Dinv, bl - Wx)
            qn, tn = q.copy(), t.copy()
            for i in np.nonzero(~fixed)[0]:
                qn[i], tn[i] = pose_oplus(q[i], t[i], xp[col[i]])
            Xn = X + xl
            _, _, r = errors(qn, tn, Xn)
            tchi = _huber(om * (r * r).sum(1), delta)[0].sum()
            scale = (xp * (lam * xp + bp)).sum() + (xl * (lam * xl + bl)).sum()
            if lm.trial(solved, tchi, scale):
                q, t, X = qn, tn, Xn
            stats["trials"] += 1
            if not lm.more_trials():
                break
        stats["iterations"] += 1
        stats["chi2_final"] = lm.cur
        stats["stop_reason"] = lm.stop()
        if stats["stop_reason"]:
            break
    stats["lambda_"] = lm.lam
    R = np.array([_R(v) for v in q])
    Xl = np.einsum("eij,ej->ei", R[ep], X[el]) + t[ep]
    if right.any():
        Xl[right] = to_right(rig, Xl[right])
    depth = Xl[:, 2] > 0
    return dict(pose_q=q, pose_t=t, points=X, chi2=om * (r * r).sum(1), depth_positive=depth.astype(np.uint8), stats=stats)
