"""Numpy reference for the KannalaBrandt8 edges of PoseOptimization and LocalBundleAdjustment.  A test helper, not a test.

Restated from the reference text (read as text; nothing copied):
  src/CameraModels/KannalaBrandt8.cpp:46-65     project(Vector3d): theta, psi through atan2f / sqrtf on float-rounded arguments
  src/CameraModels/KannalaBrandt8.cpp:145-175   projectJac: all double
  src/OptimizableTypes.cpp:24-38,139-160        EdgeSE3ProjectXYZOnlyPose / EdgeSE3ProjectXYZ: obs - project, -projectJac * (R | SE3deriv)
  Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-194, sparse_optimizer.cpp:354-419   Levenberg
  src/Optimizer.cc:814-1115                     PoseOptimization: four rounds, float chi2 against 5.991
theta and psi are the host libm's sqrtf / atan2f on numpy.float32 values; everything else is float64 (the update's exponential
is evaluated in long double by dense_ba_reference.se3_exp_g2o and rounded).  atan2f is called in libm itself, through ctypes:
numpy.arctan2 on float32 arrays runs numpy's own SIMD kernel where the CPU has one, which was measured up to 2.5 ulp from the exact
value -- not the function the reference calls, and not within the one ulp that glibc documents and the tolerances rest on.

`perturb`: a numpy RandomState, or None.  With one, theta and psi of EVERY evaluation move by one float ulp (nextafter) with a
random sign: the model of a second correct implementation of atan2f.  The tolerances of the GPU tests are the spread of the
outputs under that switch (tools/make_kb8_golden.py)."""
import ctypes
import ctypes.util

import numpy as np

from dense_ba_reference import LD, quat_to_R, se3_exp_g2o

CHI2_MONO_F32 = np.float32(5.991)


# ------------------------------------------------------------------------------------------------ the camera
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.atan2f.argtypes = [ctypes.c_float, ctypes.c_float]
_libm.atan2f.restype = ctypes.c_float
_atan2f_each = np.frompyfunc(lambda y, x: _libm.atan2f(float(y), float(x)), 2, 1)


def atan2f(y, x):
    """libm's atan2f, element by element, on float32 arrays"""
    y, x = np.asarray(y), np.asarray(x)
    assert y.dtype == np.float32 and x.dtype == np.float32
    return np.asarray(_atan2f_each(y, x), dtype=np.float64).astype(np.float32)


def cam_params(cam):
    """(fx, fy, cx, cy, k0..k3) as float64: mvParameters are floats promoted to double where they are used"""
    return tuple(float(cam[k]) for k in ("fx", "fy", "cx", "cy")) + tuple(float(v) for v in cam["k"])


def atan2_rounded(y, x):
    """the float rounding of the f64 atan2 of float arguments: what csrc/camera_kb8.h computes on the device"""
    return np.arctan2(np.asarray(y, np.float32).astype(np.float64), np.asarray(x, np.float32).astype(np.float64)).astype(np.float32)


def theta_psi(Xc, perturb=None, device_model=False):
    """device_model: the two arctangents as the device evaluates them (atan2_rounded) instead of libm's atan2f"""
    Xc = np.asarray(Xc, np.float64)
    x, y, z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    x2_plus_y2 = x * x + y * y
    at = atan2_rounded if device_model else atan2f
    theta = at(np.sqrt(x2_plus_y2.astype(np.float32)), z.astype(np.float32))
    psi = at(y.astype(np.float32), x.astype(np.float32))
    assert theta.dtype == np.float32 and psi.dtype == np.float32
    if perturb is not None:
        inf = np.float32(np.inf)
        theta = np.nextafter(theta, np.where(perturb.randint(0, 2, theta.shape) > 0, inf, -inf).astype(np.float32))
        psi = np.nextafter(psi, np.where(perturb.randint(0, 2, psi.shape) > 0, inf, -inf).astype(np.float32))
    return theta.astype(np.float64), psi.astype(np.float64)


def radius(cam, theta):
    """r(theta) in the operation order of project()"""
    _, _, _, _, k0, k1, k2, k3 = cam_params(cam)
    theta2 = theta * theta
    theta3 = theta * theta2
    theta5 = theta3 * theta2
    theta7 = theta5 * theta2
    theta9 = theta7 * theta2
    return theta + k0 * theta3 + k1 * theta5 + k2 * theta7 + k3 * theta9


def radius_derivative(cam, theta):
    """fd = dr / dtheta as projectJac writes it"""
    _, _, _, _, k0, k1, k2, k3 = cam_params(cam)
    theta2 = theta * theta
    theta4 = theta2 * theta2
    theta6 = theta2 * theta4
    theta8 = theta4 * theta4
    return 1 + 3 * k0 * theta2 + 5 * k1 * theta4 + 7 * k2 * theta6 + 9 * k3 * theta8


def project(cam, Xc, perturb=None, device_model=False):
    """KannalaBrandt8::project(Vector3d) of (..., 3) points -> (..., 2)"""
    fx, fy, cx, cy = cam_params(cam)[:4]
    theta, psi = theta_psi(Xc, perturb, device_model)
    r = radius(cam, theta)
    return np.stack([fx * r * np.cos(psi) + cx, fy * r * np.sin(psi) + cy], -1)


def project_smooth(cam, Xc, dtype=np.float64):
    """the same projection with theta and psi evaluated in `dtype` (float64 or long double): what project() rounds, and what
    central differences can be taken of"""
    Xc = np.asarray(Xc, dtype)
    p = [dtype(v) for v in cam_params(cam)]
    x, y, z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    theta = np.arctan2(np.sqrt(x * x + y * y), z)
    psi = np.arctan2(y, x)
    t2 = theta * theta
    r = theta * (1 + t2 * (p[4] + t2 * (p[5] + t2 * (p[6] + t2 * p[7]))))
    return np.stack([p[0] * r * np.cos(psi) + p[2], p[1] * r * np.sin(psi) + p[3]], -1)


def project_exact_arctangents(cam, Xc, round_to_float=True):
    """project() with the two arctangents of its float-rounded arguments evaluated in long double and then rounded to float (the
    correctly rounded atan2f, which is what the device computes) or left unrounded, and the rest in long double.  (The rounding
    of the arguments themselves belongs to the function.)"""
    Xc = np.asarray(Xc, np.float64)
    x, y, z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    rho = np.sqrt((x * x + y * y).astype(np.float32))
    theta = np.arctan2(rho.astype(LD), z.astype(np.float32).astype(LD))
    psi = np.arctan2(y.astype(np.float32).astype(LD), x.astype(np.float32).astype(LD))
    if round_to_float:
        theta, psi = theta.astype(np.float32).astype(LD), psi.astype(np.float32).astype(LD)
    p = [LD(v) for v in cam_params(cam)]
    t2 = theta * theta
    r = theta * (1 + t2 * (p[4] + t2 * (p[5] + t2 * (p[6] + t2 * p[7]))))
    return np.stack([p[0] * r * np.cos(psi) + p[2], p[1] * r * np.sin(psi) + p[3]], -1)


def project_jac(cam, Xc):
    """KannalaBrandt8::projectJac of (N, 3) points -> (N, 2, 3), float64, the expressions as written"""
    fx, fy, _, _, k0, k1, k2, k3 = cam_params(cam)
    Xc = np.asarray(Xc, np.float64)
    X, Y, Z = Xc[..., 0], Xc[..., 1], Xc[..., 2]
    x2, y2, z2 = X * X, Y * Y, Z * Z
    r2 = x2 + y2
    r = np.sqrt(r2)
    r3 = r2 * r
    theta = np.arctan2(r, Z)
    theta2 = theta * theta; theta3 = theta2 * theta
    theta4 = theta2 * theta2; theta5 = theta4 * theta
    theta6 = theta2 * theta4; theta7 = theta6 * theta
    theta8 = theta4 * theta4; theta9 = theta8 * theta
    f = theta + theta3 * k0 + theta5 * k1 + theta7 * k2 + theta9 * k3
    fd = 1 + 3 * k0 * theta2 + 5 * k1 * theta4 + 7 * k2 * theta6 + 9 * k3 * theta8
    J = np.zeros(Xc.shape[:-1] + (2, 3))
    J[..., 0, 0] = fx * (fd * Z * x2 / (r2 * (r2 + z2)) + f * y2 / r3)
    J[..., 1, 0] = fy * (fd * Z * Y * X / (r2 * (r2 + z2)) - f * Y * X / r3)
    J[..., 0, 1] = fx * (fd * Z * Y * X / (r2 * (r2 + z2)) - f * Y * X / r3)
    J[..., 1, 1] = fy * (fd * Z * y2 / (r2 * (r2 + z2)) + f * x2 / r3)
    J[..., 0, 2] = -fx * fd * X / (r2 + z2)
    J[..., 1, 2] = -fy * fd * Y / (r2 + z2)
    return J


def ulp32(v):
    """spacing of float32 at |v|"""
    v = np.abs(np.asarray(v, np.float64)).astype(np.float32)
    return (np.nextafter(v, np.float32(np.inf)) - v).astype(np.float64)


def project_bound(cam, Xc):
    """per point the bound (du, dv) on |project - exact| that one float ulp of theta and of psi allows:
    f * (fd * ulp32(theta) + r * ulp32(psi)) + 1e-9  (the rounding of theta moves r by fd per unit, that of psi turns r)"""
    fx, fy = cam_params(cam)[:2]
    theta, psi = theta_psi(Xc)
    b = np.abs(radius_derivative(cam, theta)) * ulp32(theta) + np.abs(radius(cam, theta)) * ulp32(psi)
    return np.stack([fx * b + 1e-9, fy * b + 1e-9], -1)


# ------------------------------------------------------------------------------------------------ SE(3) state: (q xyzw, t)
def _quat_mul(a, b):
    return np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1], a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                     a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0], a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])


def _quat_normalize(q):
    q = np.asarray(q, np.float64)
    if q[3] < 0:
        q = -q
    return q / np.sqrt((q * q).sum())


def _quat_from_R(R):
    t = R[0, 0] + R[1, 1] + R[2, 2]
    assert t > 0, "an update this large is outside what the tests build"
    s = np.sqrt(t + 1)
    return np.array([(R[2, 1] - R[1, 2]) / (2 * s), (R[0, 2] - R[2, 0]) / (2 * s), (R[1, 0] - R[0, 1]) / (2 * s), s / 2], np.float64)


def pose_oplus(q, t, u):
    """SE3Quat::exp(u) * (q, t), u = (omega, upsilon) (types_six_dof_expmap.h:73-76)"""
    dR, dt = se3_exp_g2o(u)
    dR, dt = dR.astype(np.float64), dt.astype(np.float64)
    return _quat_normalize(_quat_mul(_quat_normalize(_quat_from_R(dR)), q)), dR @ t + dt


def _R(q):
    return quat_to_R(q).astype(np.float64)


def _se3_rows(N, Xc):
    """N (E, 2, 3) = -projectJac  ->  N * [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1]  (E, 2, 6)"""
    x, y, z = Xc[:, 0], Xc[:, 1], Xc[:, 2]
    J = np.zeros((len(Xc), 2, 6))
    a0, a1, a2 = N[:, :, 0], N[:, :, 1], N[:, :, 2]
    J[:, :, 0] = a1 * (-z)[:, None] + a2 * y[:, None]
    J[:, :, 1] = a0 * z[:, None] + a2 * (-x)[:, None]
    J[:, :, 2] = a0 * (-y)[:, None] + a1 * x[:, None]
    J[:, :, 3], J[:, :, 4], J[:, :, 5] = a0, a1, a2
    return J


def _huber(chi, delta, on=True):
    chi = np.asarray(chi, np.float64)
    dsq = delta * delta
    big = (chi > dsq) if (on and delta > 0) else np.zeros(chi.shape, bool)
    s = np.sqrt(np.where(big, chi, 1.0))
    return np.where(big, 2 * s * delta - dsq, chi), np.where(big, delta / s, 1.0)


def _ldlt_solve(A, b):
    """LinearSolverDense: LDL^T without pivoting; ok = every pivot positive and finite"""
    n = len(b)
    L = np.zeros((n, n)); D = np.zeros(n)
    ok = True
    for j in range(n):
        d = A[j, j] - (L[j, :j] * L[j, :j] * D[:j]).sum()
        ok = ok and bool(d > 0) and bool(np.isfinite(d))
        D[j] = d
        for i in range(j + 1, n):
            L[i, j] = (A[i, j] - (L[i, :j] * L[j, :j] * D[:j]).sum()) / d
    x = np.zeros(n)
    for i in range(n):
        x[i] = b[i] - (L[i, :i] * x[:i]).sum()
    x = x / D
    for i in range(n - 1, -1, -1):
        x[i] = x[i] - (L[i + 1:, i] * x[i + 1:]).sum()
    return x, ok


class Levenberg:
    """g2o's policy (levenberg.cpp:61-169): lambda, nu, rho, the stop rules"""

    def __init__(self):
        self.lam, self.ni, self.n_bad, self.rho, self.qmax = 0.0, 2.0, 0, 0.0, 0
        self.cur = self.ini = 0.0

    def linearized(self, chi2, first, lambda0):
        self.cur = self.ini = chi2
        if first:
            self.lam, self.ni, self.n_bad = lambda0, 2.0, 0
        self.rho, self.qmax = 0.0, 0

    def trial(self, solved, chi_new, scale):
        temp = chi_new if solved else np.finfo(np.float64).max
        self.rho = (self.cur - temp) / (scale + 1e-3)
        ok = bool(self.rho > 0 and np.isfinite(temp))
        if ok:
            alpha = min(1.0 - (2 * self.rho - 1) ** 3, 2.0 / 3.0)
            self.lam *= max(1.0 / 3.0, alpha)
            self.ni = 2.0
            self.cur = temp
        else:
            self.lam *= self.ni
            self.ni *= 2
        self.qmax += 1
        return ok

    def more_trials(self):
        return self.rho < 0 and self.qmax < 10

    def stop(self):
        if self.qmax == 10 or self.rho == 0:
            return 1
        self.n_bad = self.n_bad + 1 if (self.ini - self.cur) * 1e3 < self.ini else 0
        return 2 if self.n_bad >= 3 else 0


# ------------------------------------------------------------------------------------------------ PoseOptimization
def pose_optimize(w, cam, perturb=None, device_model=False, jitter=None):
    """Optimizer::PoseOptimization of one monocular KB8 frame: w = dict(q, t, Xw, obs, inv_sigma2, huber_mono).
    Returns q, t, outlier, inliers, n_bad, iterations[4], trials[4], chi2[4] and `margins`: per round and edge
    |chi2 - 5.991| / 5.991 of the classification (how far a flag is from flipping).
    device_model: theta and psi as the device rounds them -- the staircase the device's Levenberg walks, so that its iterations
    and trials can be compared.  jitter (a RandomState): every camera-frame point is scaled by 1 + 4e-16 * N(0, 1) at every
    evaluation, the model of another order of the f64 operations; a run whose counts survive it does not hang on the last bit."""
    Xw = np.asarray(w["Xw"], np.float64); obs = np.asarray(w["obs"], np.float64)[:, :2]; om = np.asarray(w["inv_sigma2"], np.float64)
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
        return Xc, obs[idx] - project(cam, Xc, perturb, device_model)

    for rnd in range(4 if n >= 3 else 0):
        q, t = q0, t0
        idx = np.nonzero(active)[0]
        if len(idx):
            lm = Levenberg()
            for it in range(10):
                Xc, r = errors(q, t, idx)
                err[idx] = r
                rho0, rho1 = _huber(om[idx] * (r * r).sum(1), delta, robust)
                J = _se3_rows(-project_jac(cam, Xc), Xc)
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
        # classification with float chi2 (:1016-1100): an inactive edge did not follow the estimate and is evaluated first
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
def lba_solve(w, cam, max_iters=10, lambda_init=0.0, perturb=None):
    """lba_solve of a monocular KB8 window (the fields of synth.make_ba_window): g2o Levenberg with the points eliminated per
    landmark and the reduced system solved by Cholesky.  chi2 is, as in g2o, that of the errors as LAST computed (the last trial's,
    also when it was rejected); depth_positive belongs to the accepted state."""
    fixed = np.asarray(w["pose_fixed"]) != 0
    col = np.cumsum(~fixed) - 1
    nP, nL = int((~fixed).sum()), len(w["points"])
    ep, el = np.asarray(w["edge_pose"]), np.asarray(w["edge_point"])
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
        return R, Xc, obs - project(cam, Xc, perturb)

    lm = Levenberg()
    stats = dict(iterations=0, trials=0, stop_reason=0, chi2_initial=0.0, chi2_final=0.0)
    r = np.zeros((len(ep), 2))
    for it in range(max_iters):
        R, Xc, r = errors(q, t, X)
        rho0, rho1 = _huber(om * (r * r).sum(1), delta)
        N = -project_jac(cam, Xc)
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
    depth = (np.einsum("eij,ej->ei", R[ep], X[el]) + t[ep])[:, 2] > 0
    return dict(pose_q=q, pose_t=t, points=X, chi2=om * (r * r).sum(1), depth_positive=depth.astype(np.uint8), stats=stats)
