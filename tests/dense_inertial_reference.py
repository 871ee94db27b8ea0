"""Dense long-double reference for the inertial solvers: LocalInertialBA (liba_solve, liba_solve_batch) and the per-frame
PoseInertialOptimizationLastKeyFrame / ...LastFrame (liba_pose_optimize_batch).  A test helper, not a test.

Independent of oracle/: numpy in np.longdouble, every residual, Jacobian, robust weight and the Levenberg first trial restated from
the reference text (cited file:line, read as text; nothing copied), the system assembled densely with the landmarks eliminated
exactly, solved in f64 by LAPACK and refined with long-double residuals.  The SO(3) / projection / solve helpers are those of
dense_ba_reference.py.

Follows:
  src/G2oTypes.cc:192-220            ImuCamPose::Update: twb += Rwb ut, Rwb <- Rwb Exp(ur); Rcw = Rcb Rbw, tcw = Rcb tbw + tcb
  src/G2oTypes.cc:170-190            Project / ProjectStereo (double 1/z, double bf) / isDepthPositive
  include/G2oTypes.h:342-490, src/G2oTypes.cc:349-450    EdgeMono / EdgeStereo and their OnlyPose variants
  src/G2oTypes.cc:514-594            EdgeInertial::computeError / linearizeOplus (vertex order P1 V1 G1 A1 P2 V2)
  include/G2oTypes.h:635-700         EdgeGyroRW / EdgeAccRW: e = b2 - b1, J = (-I, +I)
  src/G2oTypes.cc:731-760            EdgePriorPoseImu
  src/G2oTypes.cc:777-854            ExpSO3, LogSO3, InverseRightJacobianSO3, RightJacobianSO3 with their 1e-5 branches
  src/ImuTypes.cc:276-307            GetDeltaBias / GetDeltaRotation / GetDeltaVelocity / GetDeltaPosition: float expressions
  Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:94-160    first trial, rho with the + 1e-3 in the scale, lambda update
  src/Optimizer.cc:4831-4870         the 15 x 15 Hessian that PoseInertialOptimizationLastKeyFrame leaves as the next prior
  src/Optimizer.cc:5084-5090,5236-5281   PoseInertialOptimizationLastFrame: the prior edge's kernel, the 30 x 30 Hessian before Marginalize

One documented deviation of the project is followed, because the chi2 comparisons at 1e-12 need the very same floats: the
reference evaluates Sophus::SO3f::exp(JRg dbg) in float; oracle and kernels evaluate the quaternion exponential in double and round
its rotation matrix to float (oracle/inertial_oracle.cpp header).  Everything around it (float bias difference, float JRg dbg, float
dR * E, the polar factor rounded to float, float dV / dP sums in the reference's order) is restated in np.float32.
"""
import numpy as np

import dense_ba_reference as D
from dense_ba_reference import LD, huber, inv3, project_residual, skew, so3_exp, so3_log, solve_refined, step_tolerance

F32 = np.float32
I3 = np.eye(3, dtype=LD)
GRAVITY = np.array([0, 0, -9.81], LD)           # IMU::GRAVITY_VALUE (ImuTypes.h), g = (0, 0, -G)
BLOCKS = ("rot", "trans", "vel", "bg", "ba")


# ------------------------------------------------------------------------------------------------ SO(3) as the reference writes it
def polar(R):
    """NormalizeRotation (G2oTypes.h:67-71): U V^T of the SVD = the orthogonal polar factor, by Newton iteration in long double"""
    R = np.asarray(R, LD)
    for _ in range(10):
        Rn = (R + inv3(R).T) / 2
        if np.abs(Rn - R).max() < 1e-19:
            return Rn
        R = Rn
    return R


def exp_so3(w):
    """ExpSO3 (G2oTypes.cc:782-798)"""
    w = np.asarray(w, LD)
    d2 = (w * w).sum(); d = np.sqrt(d2)
    W = skew(w)
    if d < 1e-5:
        return polar(I3 + W + LD(0.5) * (W @ W))
    return polar(I3 + W * (np.sin(d) / d) + (W @ W) * ((1 - np.cos(d)) / d2))


def log_so3(R):
    """LogSO3 (G2oTypes.cc:800-814), with its |sin theta| < 1e-5 branch"""
    w = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]], LD) / 2
    c = (R[0, 0] + R[1, 1] + R[2, 2] - 1) * LD(0.5)
    if c > 1 or c < -1:
        return w
    th = np.arccos(c); s = np.sin(th)
    if abs(s) < 1e-5:
        return w
    return th * w / s


def inv_right_jacobian(v):
    """InverseRightJacobianSO3 (G2oTypes.cc:821-832)"""
    v = np.asarray(v, LD)
    d2 = (v * v).sum(); d = np.sqrt(d2)
    if d < 1e-5:
        return I3.copy()
    W = skew(v)
    return I3 + W / 2 + (W @ W) * (1 / d2 - (1 + np.cos(d)) / (2 * d * np.sin(d)))


def right_jacobian(v):
    """RightJacobianSO3 (G2oTypes.cc:839-854)"""
    v = np.asarray(v, LD)
    d2 = (v * v).sum(); d = np.sqrt(d2)
    if d < 1e-5:
        return I3.copy()
    W = skew(v)
    return I3 - W * ((1 - np.cos(d)) / d2) + (W @ W) * ((d - np.sin(d)) / (d2 * d))


# ------------------------------------------------------------------------------------------------ the pre-integration getters
def _f32(a):
    """double (or long double) -> float as a C cast of a double does"""
    return np.asarray(a, LD).astype(np.float64).astype(F32)


def _matvec32(J, d):
    """Matrix3f * Vector3f in float, accumulated column by column, no contraction"""
    J = np.asarray(J, F32).reshape(3, 3); d = np.asarray(d, F32)
    return (J[:, 0] * d[0] + J[:, 1] * d[1]) + J[:, 2] * d[2]


def get_deltas(L, bg, ba, smooth=False):
    """(dR, dV, dP, dbg) of Preintegrated::GetDeltaRotation / Velocity / Position / GetDeltaBias for the bias (ba, bg) of the link's
    first key frame.  IMU::Bias holds floats, so the estimate is cast to float first; bias0 = (bax bay baz bwx bwy bwz).
    smooth=True keeps every step in long double (exact exponential, no rounding): what a difference quotient needs."""
    b0 = np.asarray(L["bias0"], F32)
    if smooth:
        dbg = np.asarray(bg, LD) - b0[3:].astype(LD); dba = np.asarray(ba, LD) - b0[:3].astype(LD)
        m = lambda k: np.asarray(L[k], F32).reshape(3, 3).astype(LD)
        dR = polar(m("dR") @ so3_exp(m("JRg") @ dbg))
        dV = np.asarray(L["dV"], F32).astype(LD) + m("JVg") @ dbg + m("JVa") @ dba
        dP = np.asarray(L["dP"], F32).astype(LD) + m("JPg") @ dbg + m("JPa") @ dba
        return dR, dV, dP, dbg
    dbg = _f32(bg) - b0[3:]; dba = _f32(ba) - b0[:3]                                   # float - float
    w = _matvec32(L["JRg"], dbg).astype(LD)
    th2 = (w * w).sum(); th = np.sqrt(th2)
    imag, real = (LD(0.5) - th2 / 48, 1 - th2 / 8) if th < 1e-5 else (np.sin(th / 2) / th, np.cos(th / 2))
    qx, qy, qz, qw = imag * w[0], imag * w[1], imag * w[2], real
    E = _f32([[1 - 2 * (qy * qy + qz * qz), 2 * (qx * qy - qz * qw), 2 * (qx * qz + qy * qw)],
              [2 * (qx * qy + qz * qw), 1 - 2 * (qx * qx + qz * qz), 2 * (qy * qz - qx * qw)],
              [2 * (qx * qz - qy * qw), 2 * (qy * qz + qx * qw), 1 - 2 * (qx * qx + qy * qy)]])
    dR0 = np.asarray(L["dR"], F32).reshape(3, 3)
    Rf = (dR0[:, 0:1] * E[0:1, :] + dR0[:, 1:2] * E[1:2, :]) + dR0[:, 2:3] * E[2:3, :]   # float product, k = 0, 1, 2 in order
    dR = _f32(polar(Rf.astype(LD))).astype(LD)                                         # the result is a Matrix3f
    dV = (np.asarray(L["dV"], F32) + _matvec32(L["JVg"], dbg)) + _matvec32(L["JVa"], dba)
    dP = (np.asarray(L["dP"], F32) + _matvec32(L["JPg"], dbg)) + _matvec32(L["JPa"], dba)
    return dR, dV.astype(LD), dP.astype(LD), dbg.astype(LD)


# ------------------------------------------------------------------------------------------------ states and the update rule
def state_of(pr):
    """long-double copy of the states of a window or of a solver output: Rwb, twb, vel, bg, ba (per key frame) and points"""
    s = {k: np.array(pr[k], LD) for k in ("Rwb", "twb", "vel", "bg", "ba")}
    s["points"] = np.array(pr["points"], LD).reshape(-1, 3) if "points" in pr else np.zeros((0, 3), LD)
    return s


def copy_state(s):
    return {k: v.copy() for k, v in s.items()}


def update_pose(s, i, pu):
    """ImuCamPose::Update (G2oTypes.cc:192-220): the translation moves along the OLD body axes, the rotation is a right update"""
    pu = np.asarray(pu, LD)
    s["twb"][i] = s["twb"][i] + s["Rwb"][i] @ pu[3:]
    s["Rwb"][i] = s["Rwb"][i] @ exp_so3(pu[:3])


def camera_pose(pr, Rwb, twb):
    """Rcw = Rcb Rbw, tcw = Rcb tbw + tcb with tbw = -Rbw twb (G2oTypes.cc:211-218); batched over leading axes"""
    Rcb = np.asarray(pr["Rcb"], LD); tcb = np.asarray(pr["tcb"], LD)
    Rbw = np.swapaxes(np.asarray(Rwb, LD), -1, -2)
    tbw = -np.einsum("...ij,...j->...i", Rbw, np.asarray(twb, LD))
    return np.einsum("ij,...jk->...ik", Rcb, Rbw), np.einsum("ij,...j->...i", Rcb, tbw) + tcb


# ------------------------------------------------------------------------------------------------ visual edges on a body pose
def visual_terms(pr, Rwb, twb, X, obs, stereo, jac=True):
    """EdgeMono / EdgeStereo (and OnlyPose) on body poses Rwb, twb (E, ...) and points X (E, 3): residual obs - Project (3rd row 0
    on a mono edge), Xc, and the reference's analytic Jacobians J_point = -proj_jac Rcw (E, 3, 3) and
    J_pose = proj_jac Rcb SE3deriv(Xb) (E, 3, 6), Xb = Rbc Xc + tbc (G2oTypes.cc:349-450)"""
    Rcw, tcw = camera_pose(pr, Rwb, twb)
    Xc = np.einsum("eij,ej->ei", Rcw, np.asarray(X, LD)) + tcw
    r = project_residual(Xc, obs, stereo, pr, float_invz=False)
    if not jac:
        return r, Xc, None, None
    E = len(Xc)
    P = -D.project_jacobians(Xc, I3, stereo, pr)[0]                 # proj_jac, the stereo row with + bf / z^2
    Rcb = np.asarray(pr["Rcb"], LD)
    Xb = Xc @ Rcb + np.asarray(pr["tbc"], LD)                       # Rbc Xc + tbc with Rbc = Rcb^T
    S = np.zeros((E, 3, 6), LD)
    S[:, :, :3] = -skew(Xb)
    S[:, :, 3:] = I3
    return r, Xc, -np.einsum("eij,ejk->eik", P, Rcw), np.einsum("eij,jk,ekl->eil", P, Rcb, S)


# ------------------------------------------------------------------------------------------------ inertial edges
def inertial_error(L, s, smooth=False):
    """EdgeInertial::computeError (G2oTypes.cc:514-534): (er, ev, ep)"""
    k1, k2 = int(L["kf1"]), int(L["kf2"])
    dR, dV, dP, _ = get_deltas(L, s["bg"][k1], s["ba"][k1], smooth)
    dt = LD(float(L["dT"]))
    R1t = s["Rwb"][k1].T
    er = log_so3(dR.T @ R1t @ s["Rwb"][k2])
    ev = R1t @ (s["vel"][k2] - s["vel"][k1] - GRAVITY * dt) - dV
    ep = R1t @ (s["twb"][k2] - s["twb"][k1] - s["vel"][k1] * dt - GRAVITY * dt * dt / 2) - dP
    return np.concatenate([er, ev, ep])


def inertial_jacobian(L, s, smooth=False):
    """EdgeInertial::linearizeOplus (G2oTypes.cc:536-594): 9 x 24, columns P1 (rot, trans) V1 G1 A1 P2 (rot, trans) V2"""
    k1, k2 = int(L["kf1"]), int(L["kf2"])
    dR, _, _, dbg = get_deltas(L, s["bg"][k1], s["ba"][k1], smooth)
    dt = LD(float(L["dT"]))
    m = lambda k: np.asarray(L[k], F32).reshape(3, 3).astype(LD)
    R1, R2 = s["Rwb"][k1], s["Rwb"][k2]
    R1t = R1.T
    eR = dR.T @ R1t @ R2
    invJr = inv_right_jacobian(log_so3(eR))
    J = np.zeros((9, 24), LD)
    J[0:3, 0:3] = -invJr @ R2.T @ R1
    J[3:6, 0:3] = skew(R1t @ (s["vel"][k2] - s["vel"][k1] - GRAVITY * dt))
    J[6:9, 0:3] = skew(R1t @ (s["twb"][k2] - s["twb"][k1] - s["vel"][k1] * dt - LD(0.5) * GRAVITY * dt * dt))
    J[6:9, 3:6] = -I3
    J[3:6, 6:9] = -R1t
    J[6:9, 6:9] = -R1t * dt
    JRg = m("JRg")
    J[0:3, 9:12] = -invJr @ eR.T @ right_jacobian(JRg @ dbg) @ JRg
    J[3:6, 9:12] = -m("JVg")
    J[6:9, 9:12] = -m("JPg")
    J[3:6, 12:15] = -m("JVa")
    J[6:9, 12:15] = -m("JPa")
    J[0:3, 15:18] = invJr
    J[6:9, 18:21] = R1t @ R2
    J[3:6, 21:24] = R1t
    return J


def prior_error(pr, s, i=0):
    """EdgePriorPoseImu::computeError (G2oTypes.cc:731-745): (er, et, ev, ebg, eba) of key frame i against the prior"""
    Rp = np.asarray(pr["prior_Rwb"], LD)
    return np.concatenate([log_so3(Rp.T @ s["Rwb"][i]), Rp.T @ (s["twb"][i] - np.asarray(pr["prior_twb"], LD)),
                           s["vel"][i] - np.asarray(pr["prior_vel"], LD), s["bg"][i] - np.asarray(pr["prior_bg"], LD),
                           s["ba"][i] - np.asarray(pr["prior_ba"], LD)])


def prior_jacobian(pr, s, i=0):
    """EdgePriorPoseImu::linearizeOplus (G2oTypes.cc:747-760): 15 x 15, columns rot trans vel bg ba"""
    Rp = np.asarray(pr["prior_Rwb"], LD)
    J = np.eye(15, dtype=LD)
    J[0:3, 0:3] = inv_right_jacobian(log_so3(Rp.T @ s["Rwb"][i]))
    J[3:6, 3:6] = Rp.T @ s["Rwb"][i]
    return J


# ------------------------------------------------------------------------------------------------ LocalInertialBA
def _offsets(pr):
    """reduced unknowns: per key frame 6 for a free pose, 9 (v, bg, ba) for free IMU states, -1 = fixed or absent"""
    n = int(pr["n_kf"])
    op = -np.ones(n, int); oi = -np.ones(n, int)
    k = 0
    for i in range(n):
        if not pr["pose_fixed"][i]:
            op[i] = k; k += 6
        if pr["has_imu"][i] and not pr["imu_fixed"][i]:
            oi[i] = k; k += 9
    return op, oi, k


def _link_columns(L, op, oi):
    """global offsets of a link's six vertices (P1 V1 G1 A1 P2 V2) and their positions in the 24 columns"""
    k1, k2 = int(L["kf1"]), int(L["kf2"])
    i1 = oi[k1]
    off = [op[k1], i1, i1 + 3 if i1 >= 0 else -1, i1 + 6 if i1 >= 0 else -1, op[k2], oi[k2]]
    return off, [0, 6, 9, 12, 15, 21], [6, 3, 3, 3, 6, 3]


def liba_chi2(pr, s):
    """activeRobustChi2 of a window at state s, the per-link chi2 of the inertial edges, the per-edge chi2 and depth signs"""
    tot = LD(0)
    link_chi2 = []
    for L in pr["links"]:
        e = inertial_error(L, s)
        c = e @ np.asarray(L["info9"], LD).reshape(9, 9) @ e
        link_chi2.append(c)
        tot += huber(c, pr["huber_inertial"])[0] if L["robust"] else c
        k1, k2 = int(L["kf1"]), int(L["kf2"])
        for key, info in (("bg", "info_gyro"), ("ba", "info_acc")):
            d = s[key][k2] - s[key][k1]
            tot += d @ np.asarray(L[info], LD).reshape(3, 3) @ d
    ek = np.asarray(pr["edge_kf"]); el = np.asarray(pr["edge_point"])
    st = np.asarray(pr["edge_stereo"]).astype(bool)
    if len(ek):
        r, Xc, _, _ = visual_terms(pr, s["Rwb"][ek], s["twb"][ek], s["points"][el], pr["edge_obs"], st, jac=False)
        chi2 = np.asarray(pr["edge_inv_sigma2"], LD) * (r * r).sum(1)
        tot += huber(chi2, np.where(st, pr["huber_stereo"], pr["huber_mono"]))[0].sum()
        depth = Xc[:, 2] > 0
    else:
        chi2 = np.zeros(0, LD); depth = np.zeros(0, bool)
    return tot, np.array(link_chi2, LD), chi2, depth


def liba_first_trial(pr, refine=3):
    """The first Levenberg trial of LocalInertialBA at lambda = pr["lambda_init"] (the reference sets 1e0 or 1e-2,
    Optimizer.cc:2540-2545): H, b over pose / velocity / gyro bias / accelerometer bias / landmark unknowns with rho' * Omega (Huber
    with huber_inertial on links with `robust`, none on the random walks, Huber mono / stereo on the visual edges), landmarks
    eliminated exactly, (H + lambda I) dx = b, the update rule, rho with the + 1e-3 in the scale and the lambda after the trial.
    Returns per free key frame the steps (rot, trans in the body frame, vel, bg, ba; NaN where a block is fixed), the point steps,
    kappa / resid of the reduced solve, chi2_initial, chi2_final, rho, lambda_, link_chi2 and the state after the trial."""
    s0 = state_of(pr)
    op, oi, n = _offsets(pr)
    lam = LD(pr["lambda_init"])
    assert lam > 0
    H = np.zeros((n, n), LD); b = np.zeros(n, LD)
    link_sys = []
    for L in pr["links"]:
        e = inertial_error(L, s0); J = inertial_jacobian(L, s0)
        Om = np.asarray(L["info9"], LD).reshape(9, 9)
        c = e @ Om @ e
        rho1 = huber(c, pr["huber_inertial"])[1] if L["robust"] else LD(1)
        Om = rho1 * Om
        off, loc, dim = _link_columns(L, op, oi)
        cols = np.concatenate([np.arange(o, o + d) if o >= 0 else -np.ones(d, int) for o, d in zip(off, dim)])
        ok = cols >= 0
        Jf = J[:, ok]
        H[np.ix_(cols[ok], cols[ok])] += Jf.T @ Om @ Jf
        b[cols[ok]] -= Jf.T @ Om @ e
        link_sys.append((cols[ok], Jf.T @ Om))
        k1, k2 = int(L["kf1"]), int(L["kf2"])
        for key, info, o in (("bg", "info_gyro", 3), ("ba", "info_acc", 6)):
            O3 = np.asarray(L[info], LD).reshape(3, 3)
            d = s0[key][k2] - s0[key][k1]
            for k, sg in ((k1, -1), (k2, 1)):
                if oi[k] >= 0:
                    a = oi[k] + o
                    H[a:a + 3, a:a + 3] += O3
                    b[a:a + 3] -= sg * (O3 @ d)
            if oi[k1] >= 0 and oi[k2] >= 0:
                a1, a2 = oi[k1] + o, oi[k2] + o
                H[a1:a1 + 3, a2:a2 + 3] -= O3
                H[a2:a2 + 3, a1:a1 + 3] -= O3
    ek = np.asarray(pr["edge_kf"]); el = np.asarray(pr["edge_point"])
    st = np.asarray(pr["edge_stereo"]).astype(bool)
    nL = len(s0["points"])
    Hll = np.zeros((nL, 3, 3), LD); bl = np.zeros((nL, 3), LD)
    W = np.zeros((len(ek), 6, 3), LD)
    if len(ek):
        r, _, Ji, Jj = visual_terms(pr, s0["Rwb"][ek], s0["twb"][ek], s0["points"][el], pr["edge_obs"], st)
        chi2 = np.asarray(pr["edge_inv_sigma2"], LD) * (r * r).sum(1)
        wgt = huber(chi2, np.where(st, pr["huber_stereo"], pr["huber_mono"]))[1] * np.asarray(pr["edge_inv_sigma2"], LD)
        np.add.at(Hll, el, np.einsum("edi,e,edj->eij", Ji, wgt, Ji))
        np.add.at(bl, el, -np.einsum("edi,e,ed->ei", Ji, wgt, r))
        Hjj = np.einsum("edi,e,edj->eij", Jj, wgt, Jj)
        bj = -np.einsum("edi,e,ed->ei", Jj, wgt, r)
        W = np.einsum("edi,e,edj->eij", Jj, wgt, Ji)
        for e in np.nonzero(op[ek] >= 0)[0]:
            o = op[ek[e]]
            H[o:o + 6, o:o + 6] += Hjj[e]
            b[o:o + 6] += bj[e]
    Dinv = inv3(Hll + lam * I3) if nL else np.zeros((0, 3, 3), LD)
    S = H + lam * np.eye(n, dtype=LD)
    bs = b.copy()
    by_pt = [[] for _ in range(nL)]
    for e in np.nonzero(op[ek] >= 0)[0] if len(ek) else []:
        by_pt[el[e]].append(e)
    for l, es in enumerate(by_pt):
        for ea in es:
            oa = op[ek[ea]]
            Z = W[ea] @ Dinv[l]
            bs[oa:oa + 6] -= Z @ bl[l]
            for eb in es:
                ob = op[ek[eb]]
                S[oa:oa + 6, ob:ob + 6] -= Z @ W[eb].T
    x, resid, kappa = solve_refined(S, bs, refine)
    xl = np.zeros((nL, 3), LD)
    for l, es in enumerate(by_pt):
        c = bl[l].copy()
        for e in es:
            o = op[ek[e]]
            c -= W[e].T @ x[o:o + 6]
        xl[l] = Dinv[l] @ c
    s1 = copy_state(s0)
    nk = int(pr["n_kf"])
    steps = {k: np.full((nk, 3), np.nan, LD) for k in BLOCKS}
    for i in range(nk):
        if op[i] >= 0:
            update_pose(s1, i, x[op[i]:op[i] + 6])
            steps["rot"][i] = x[op[i]:op[i] + 3]; steps["trans"][i] = x[op[i] + 3:op[i] + 6]
        if oi[i] >= 0:
            for k, key in enumerate(("vel", "bg", "ba")):
                d = x[oi[i] + 3 * k:oi[i] + 3 * k + 3]
                s1[key][i] = s1[key][i] + d
                steps[key][i] = d
    s1["points"] = s0["points"] + xl
    chi_ini, link_chi2, _, _ = liba_chi2(pr, s0)
    chi_new, _, _, _ = liba_chi2(pr, s1)
    scale = (x * (lam * x + b)).sum() + (xl * (lam * xl + bl)).sum() + LD(1e-3)
    rho = (chi_ini - chi_new) / scale
    lam_next = lam * max(LD(1) / 3, min(LD(2) / 3, 1 - (2 * rho - 1) ** 3)) if rho > 0 else lam * 2
    return dict(steps=steps, point_step=xl, state=s1, chi2_initial=chi_ini, chi2_final=chi_new, rho=rho, lambda_=lam_next, kappa=kappa,
                resid=resid, link_chi2=link_chi2, n_unknowns=n,
                _sys=dict(S=S.astype(np.float64), link_sys=link_sys, Dinv=Dinv, W=W, by_pt=by_pt, op=op, oi=oi))


def _block_steps(pr, s0, s1):
    """per key frame the five 3-vectors that take state s0 to s1 under the update rule: rotation tangent Log(R0^T R1), translation in
    the old body frame R0^T (t1 - t0), and the additive velocity / bias deltas"""
    out = {}
    out["rot"] = np.stack([so3_log(s0["Rwb"][i].T @ s1["Rwb"][i]) for i in range(len(s0["Rwb"]))])
    out["trans"] = np.einsum("kji,kj->ki", s0["Rwb"], s1["twb"] - s0["twb"])
    for k in ("vel", "bg", "ba"):
        out[k] = s1[k] - s0[k]
    return out


def float_getter_floor(pr, ref):
    """The step that a one-float-ulp change of every bias-corrected dR, dV, dP produces, to first order H^-1 J^T Omega delta_e with
    the landmarks eliminated: delta_e is 2^-23 on a rotation row (the entries of dR are below 1) and the float spacing at dV_i, dP_i on
    the others; the 9 components of every link are taken as independent (root sum of squares).  Computed from the inputs alone.
    Returns dict(rot, trans, vel, bg, ba: (n_kf,) absolute floors, points: (n_points,))."""
    sy = ref["_sys"]
    n = ref["n_unknowns"]
    nk = int(pr["n_kf"])
    s0 = state_of(pr)
    floors = {k: np.zeros(nk) for k in BLOCKS}
    fl_pts = np.zeros(len(s0["points"]))
    if n == 0 or not pr["links"]:
        return dict(floors, points=fl_pts)
    rhs = []
    for L, (cols, JtO) in zip(pr["links"], sy["link_sys"]):
        k1 = int(L["kf1"])
        _, dV, dP, _ = get_deltas(L, s0["bg"][k1], s0["ba"][k1])
        de = np.concatenate([np.full(3, 2.0 ** -23), np.spacing(np.abs(dV.astype(np.float64)).astype(F32)).astype(np.float64),
                             np.spacing(np.abs(dP.astype(np.float64)).astype(F32)).astype(np.float64)])
        for r in range(9):
            v = np.zeros(n)
            v[cols] = (JtO[:, r] * de[r]).astype(np.float64)
            rhs.append(v)
    X = np.linalg.solve(sy["S"], np.array(rhs).T)                     # (n, 9 * links)
    op, oi = sy["op"], sy["oi"]
    rss = lambda M: np.sqrt((M * M).sum())
    for i in range(nk):
        if op[i] >= 0:
            floors["rot"][i] = rss(X[op[i]:op[i] + 3]); floors["trans"][i] = rss(X[op[i] + 3:op[i] + 6])
        if oi[i] >= 0:
            for k, key in enumerate(("vel", "bg", "ba")):
                floors[key][i] = rss(X[oi[i] + 3 * k:oi[i] + 3 * k + 3])
    ek = np.asarray(pr["edge_kf"])
    W = sy["W"].astype(np.float64); Dinv = sy["Dinv"].astype(np.float64)
    for l, es in enumerate(sy["by_pt"]):
        if es:
            c = sum(W[e].T @ X[op[ek[e]]:op[ek[e]] + 6] for e in es)
            fl_pts[l] = rss(Dinv[l] @ c)
    return dict(floors, points=fl_pts)


def _ratio(err, step, tol0, floor):
    """err / |step|, or with a floor err / (tol0 |step| + 10 floor); a block whose reference step is exactly 0 must not move beyond the floor"""
    den = step if floor is None else tol0 * step + 10 * floor
    return err / den if den > 0 else (0.0 if err == 0 else np.inf)


def liba_step_error(pr, out, ref, floor=None):
    """Worst per-block error of a solver's one-trial output against liba_first_trial, each block (per free key frame: rotation tangent,
    body-frame translation, velocity, bg, ba; per point its delta) relative to the reference block's norm.  With `floor` (from
    float_getter_floor) the figure is the error divided by the block's tolerance step_tolerance(kappa) + 10 floor / |step|, so a
    return value <= 1 passes; without it the plain relative error.  Returns (worst, name of the worst block)."""
    s0 = state_of(pr); s1 = state_of(out)
    got = _block_steps(pr, s0, s1); want = _block_steps(pr, s0, ref["state"])
    tol0 = step_tolerance(ref["kappa"])
    worst, where = 0.0, None
    nrm = lambda a: float(np.sqrt((a * a).sum()))
    for k in BLOCKS:
        for i in range(int(pr["n_kf"])):
            if np.isnan(ref["steps"][k][i]).any():
                assert nrm(got[k][i]) == 0, "fixed block %s of key frame %d moved" % (k, i)
                continue
            rel = _ratio(nrm(got[k][i] - want[k][i]), nrm(want[k][i]), tol0, None if floor is None else floor[k][i])
            if rel > worst:
                worst, where = rel, (k, i)
    d = s1["points"] - ref["state"]["points"]
    for l in range(len(d)):
        rel = _ratio(nrm(d[l]), nrm(ref["point_step"][l]), tol0, None if floor is None else floor["points"][l])
        if rel > worst:
            worst, where = rel, ("point", l)
    return worst, where


def unclamped_lambda_rtol(ref):
    """Tolerance on lambda_ where the update is not clamped.  There lambda' = lambda (1 - (2 rho - 1)^3) moves with rho, and rho's
    scale x . (lambda x + b) is first order in the solved step x.  A backward-stable f64 factorisation gives x to kappa 2^-53; x enters
    the scale twice, and the reduced system itself is summed in f64 (once more each): rtol = 1e-12 + |d ln lambda' / d ln rho| 4 kappa 2^-53.
    Also returns the relative change of lambda_ that dropping the + 1e-3 from the scale would cause, which the tolerance must stay
    well below for the check to see that term."""
    rho = float(ref["rho"])
    sens = 6 * (2 * rho - 1) ** 2 * rho / (1 - (2 * rho - 1) ** 3)
    scale = float((ref["chi2_initial"] - ref["chi2_final"]) / ref["rho"])
    return 1e-12 + sens * 4 * ref["kappa"] * 2.0 ** -53, sens * 1e-3 / scale


def check_one_step(pr, r, ref, lambda_rtol=1e-12):
    """a solver's one-trial output (max_iters = 1) against liba_first_trial: iterations, trials, the three scalars, the step error per
    block, the per-edge chi2 and depth signs restated at the returned state.  Returns (plain step error, error / tolerance)."""
    st = r["stats"]
    assert st["iterations"] == 1 and st["trials"] == 1 and ref["rho"] > 0, (st, float(ref["rho"]))
    np.testing.assert_allclose(st["chi2_initial"], float(ref["chi2_initial"]), rtol=1e-12)
    np.testing.assert_allclose(st["chi2_final"], float(ref["chi2_final"]), rtol=1e-11)
    np.testing.assert_allclose(st["lambda_"], float(ref["lambda_"]), rtol=lambda_rtol)
    assert ref["resid"] < 1e-15, "reference solve residual %.3g" % ref["resid"]
    err, _ = liba_step_error(pr, r, ref)
    ratio, where = liba_step_error(pr, r, ref, float_getter_floor(pr, ref))
    assert ratio <= 1, "step error / tolerance %.3g at %s (plain error %.3g, kappa %.3g)" % (ratio, where, err, ref["kappa"])
    _, _, pe, depth = liba_chi2(pr, state_of(r))
    np.testing.assert_allclose(r["chi2"], pe.astype(np.float64), rtol=1e-9, atol=1e-10)
    np.testing.assert_array_equal(np.asarray(r["depth_positive"]).astype(bool), depth)
    return err, ratio


# ------------------------------------------------------------------------------------------------ the per-frame solver
def _frame_state(pr, res, prev=None):
    """state of the two frames: [1] the current frame as returned; [0] the other frame as given (the fixed last key frame), or `prev`,
    the previous frame's optimised state of the last-frame variant"""
    s = state_of(pr)
    for k in ("Rwb", "twb", "vel", "bg", "ba"):
        s[k][1] = np.asarray(res[k], LD)
        if prev is not None:
            s[k][0] = np.asarray(prev[k], LD)
    return s


def _frame_visual(pr, s, keep):
    Xw = np.asarray(pr["Xw"], LD)[keep]
    E = len(Xw)
    r, Xc, _, Jj = visual_terms(pr, np.broadcast_to(s["Rwb"][1], (E, 3, 3)), np.broadcast_to(s["twb"][1], (E, 3)), Xw,
                                np.asarray(pr["obs"])[keep], np.asarray(pr["stereo"])[keep])
    return r, Xc, Jj, np.asarray(pr["inv_sigma2"], LD)[keep]


def _frame_system(pr, s, keep, weights=True):
    """H and gradient J^T Omega e of the per-frame cost at state s.  Unknowns: previous frame (pose, v, bg, ba), current frame (pose, v,
    bg, ba), 30 in all; the last-key-frame variant keeps frame [0] fixed and gets the current frame's 15 x 15.  Terms: the inertial
    edge, the two random walks (e = b_cur - b_prev, J = -I, +I), the visual edges in `keep` without kernel and, for the last-frame
    variant, EdgePriorPoseImu on the previous frame with information prior_H and its Huber weight (delta 5, Optimizer.cc:5084-5090;
    weights=False: GetHessian, no weight)."""
    L = pr["link"]
    H = np.zeros((30, 30), LD); g = np.zeros(30, LD)
    e = inertial_error(L, s); J = inertial_jacobian(L, s)       # the link's 24 columns are the first 24 unknowns
    Om = np.asarray(L["info9"], LD).reshape(9, 9)
    H[0:24, 0:24] += J.T @ Om @ J; g[0:24] += J.T @ Om @ e
    for key, info, a in (("bg", "info_gyro", 9), ("ba", "info_acc", 12)):
        O3 = np.asarray(L[info], LD).reshape(3, 3)
        d = O3 @ (s[key][1] - s[key][0])
        b = 15 + a
        H[a:a + 3, a:a + 3] += O3; H[b:b + 3, b:b + 3] += O3; H[a:a + 3, b:b + 3] -= O3; H[b:b + 3, a:a + 3] -= O3
        g[a:a + 3] -= d; g[b:b + 3] += d
    if keep.any():
        r, _, Jj, om = _frame_visual(pr, s, keep)
        H[15:21, 15:21] += np.einsum("edi,e,edj->ij", Jj, om, Jj); g[15:21] += np.einsum("edi,e,ed->i", Jj, om, r)
    if not pr.get("last_frame", 0):
        return H[15:, 15:], g[15:]
    ep = prior_error(pr, s); Jp = prior_jacobian(pr, s)
    Hp = np.asarray(pr["prior_H"], LD).reshape(15, 15)
    w = huber(ep @ Hp @ ep, 5.0)[1] if weights else LD(1)
    H[0:15, 0:15] += w * (Jp.T @ Hp @ Jp); g[0:15] += w * (Jp.T @ Hp @ ep)
    return H, g


def pose_inertial_hessian(pr, res, outlier, prev=None):
    """The Hessian that the per-frame solver leaves for the next frame's prior, without robust weights.
    Last-key-frame variant (Optimizer.cc:4831-4870), 15 x 15 at the returned state: GetHessian2 of the inertial edge in the 9 x 9
    (pose, velocity) block, GetHessian2 of the two random walks in the bias blocks, GetHessian of every visual edge whose outlier
    flag is clear in the 6 x 6.
    Last-frame variant (Optimizer.cc:5236-5281), the 30 x 30 before Marginalize: GetHessian of the inertial edge (24 x 24), of the
    random walks (both frames and the cross blocks), of EdgePriorPoseImu on the previous frame, and the visual 6 x 6.  It is
    linearised at the previous frame's optimised state too; the product ABI does not return that state, so `prev` is the oracle's."""
    assert bool(pr.get("last_frame", 0)) == (prev is not None)
    return _frame_system(pr, _frame_state(pr, res, prev), ~np.asarray(outlier).astype(bool), weights=False)[0]


def pose_inertial_stationarity(pr, res, prev=None):
    """|Gauss-Newton step| / |total update| of the last round's cost at the returned state: no visual kernel, active set = the edges
    not flagged, the inertial edge and the random walks unweighted (Optimizer.cc:4606-4612 sets no kernel on them), the prior with its
    Huber weight.  In the last-key-frame variant the last key frame is fixed, so the float getters are constants of the problem and
    there is no float plateau: the bound is 1e-9.  In the last-frame variant (both frames' 30 unknowns, `prev` = the previous frame's
    optimised state) that frame's biases move, the cost is flat at the float rounding of the getters, and the bound adds 10 x the
    step of one float ulp in dR, dV, dP, H^-1 J^T Omega delta_e, as pose_stationarity does for the float 1/z.
    Returns (ratio, bound, kappa)."""
    assert bool(pr.get("last_frame", 0)) == (prev is not None)
    s = _frame_state(pr, res, prev)
    H, g = _frame_system(pr, s, ~np.asarray(res["outlier"]).astype(bool))
    step, _, kappa = solve_refined(H, -g)
    tot = _block_steps(pr, state_of(pr), s)
    total = np.concatenate([tot[k][i] for i in ((0, 1) if prev is not None else (1,)) for k in BLOCKS])
    tn = np.sqrt((total * total).sum())
    floor = 0.0
    if prev is not None:
        L = pr["link"]
        _, dV, dP, _ = get_deltas(L, s["bg"][0], s["ba"][0])
        sp = lambda v: np.spacing(np.abs(v.astype(np.float64)).astype(F32)).astype(np.float64)
        de = np.concatenate([np.full(3, 2.0 ** -23), sp(dV), sp(dP)])
        rhs = np.zeros((30, 9))
        rhs[:24] = (inertial_jacobian(L, s).T @ np.asarray(L["info9"], LD).reshape(9, 9)).astype(np.float64) * de
        X = np.linalg.solve(H.astype(np.float64), rhs)
        floor = float(10 * np.sqrt((X * X).sum()) / tn)
    return float(np.sqrt((step * step).sum()) / tn), 1e-9 + floor, kappa


def pose_inertial_flags(pr, res):
    """per-edge chi2 at the returned state with its threshold (5.991, 1.5 x 5.991 for close mono points, 7.815; float constants of
    Optimizer.cc:4560-4562,4716-4789; the last-frame variant ends on the same values, :4955-4957), the depth of every point, and the flags these give"""
    s = _frame_state(pr, res)
    n = len(pr["Xw"])
    r, Xc, _, om = _frame_visual(pr, s, np.ones(n, bool))
    chi2 = (om * (r * r).sum(1)).astype(np.float64)
    st = np.asarray(pr["stereo"]).astype(bool); close = np.asarray(pr["close_point"]).astype(bool)
    th = np.where(st, float(F32(7.815)), np.where(close, float(F32(1.5 * F32(5.991))), float(F32(5.991))))
    z = Xc[:, 2].astype(np.float64)
    return chi2, th, z, (chi2.astype(F32) > th.astype(F32)) | (~st & ~(z > 0))


# ------------------------------------------------------------------------------------------------ windows and frames
def _spd(rs, diag, corr=0.3):
    """SPD matrix with the given diagonal and correlations of +-corr between all components"""
    d = np.sqrt(np.asarray(diag, np.float64))
    u = rs.choice([-1.0, 1.0], len(d))
    C = (1 - corr) * np.eye(len(d)) + corr * np.outer(u, u)
    return C * np.outer(d, d)


def harden_link(rs, L):
    """general JRg (kept as float32), full SPD info9 / info_gyro / info_acc on the synthetic diagonals"""
    dt = float(L["dT"])
    L["JRg"] = (-dt * np.eye(3) + rs.normal(0, 0.02, (3, 3))).astype(F32)
    L["info9"] = _spd(rs, np.diag(L["info9"]))
    L["info_gyro"] = _spd(rs, np.diag(L["info_gyro"]))
    L["info_acc"] = _spd(rs, np.diag(L["info_acc"]))


def hard_inertial_window(synth, seed, n_opt, n_points=None, obs=4, stereo_frac=0.3, n_covisible_fixed=0, permute=False, bias_error=0.02,
                         big_rot=0.06, lambda_init=1.0):
    """synth.make_inertial_window made hard, with max_iters = 1:
      - a general JRg and full information matrices on every link (harden_link);
      - a bias delta of `bias_error` on every link; in a window with several links one of them has dbg exactly 0, so both branches of
        the exponential and of RightJacobianSO3 run;
      - biases that differ from key frame to key frame (2e-4 / 2e-3), so the random walks have a gradient;
      - a rotation perturbation of `big_rot` rad on the first and the last free key frame;
      - permute=True renumbers the temporal key frames newest first (kf1 > kf2 on every link, the order of the reference's
        vpOptimizableKFs) and carries every per-key-frame array and index along."""
    pr, _ = synth.make_inertial_window(seed, n_opt=n_opt, n_points=n_points or 12 * n_opt, obs_per_point=obs, bias_error=bias_error,
                                       stereo_frac=stereo_frac, n_covisible_fixed=n_covisible_fixed)
    rs = np.random.RandomState(7919 + seed)
    f32 = lambda a: np.asarray(a, F32).astype(np.float64)
    for L in pr["links"]:
        harden_link(rs, L)
    n = n_opt + 1                                           # the temporal key frames
    rb = np.random.RandomState(15485863 + seed)
    pr["bg"][:n] = f32(pr["bg"][:n] + rb.normal(0, 2e-4, (n, 3))); pr["ba"][:n] = f32(pr["ba"][:n] + rb.normal(0, 2e-3, (n, 3)))
    if len(pr["links"]) > 1:
        Lz = pr["links"][len(pr["links"]) // 2]
        Lz["bias0"] = np.concatenate([pr["ba"][Lz["kf1"]], pr["bg"][Lz["kf1"]]]).astype(F32)
    for i in sorted(set([1, n_opt])):
        a = rs.normal(0, 1, 3)
        pr["Rwb"][i] = f32(pr["Rwb"][i] @ so3_exp(big_rot * a / np.linalg.norm(a)).astype(np.float64))
    pr["lambda_init"] = float(lambda_init); pr["max_iters"] = 1
    if permute:
        new = np.arange(pr["n_kf"]); new[:n] = n - 1 - np.arange(n)
        inv = np.argsort(new)
        for k in ("Rwb", "twb", "vel", "bg", "ba", "pose_fixed", "has_imu", "imu_fixed"):
            pr[k] = np.ascontiguousarray(np.asarray(pr[k])[inv])
        pr["edge_kf"] = new[pr["edge_kf"]].astype(np.int32)
        for L in pr["links"]:
            L["kf1"], L["kf2"] = int(new[L["kf1"]]), int(new[L["kf2"]])
        pr["links"] = pr["links"][::-1]
    return pr


def hard_pose_inertial_problem(synth, seed, n, stereo_frac=0.0, outlier_frac=0.1, bias_delta=0.01, **kw):
    """synth.make_pose_inertial_problem at 0.05 px noise (gross outliers 15-40 px) with a general JRg, full information matrices and
    a bias delta on the link, so that the bias Jacobians of the pre-integration take part"""
    pr, gt = synth.make_pose_inertial_problem(seed, n=n, outlier_frac=outlier_frac, stereo_frac=stereo_frac, noise_px=0.05, **kw)
    rs = np.random.RandomState(104729 + seed)
    harden_link(rs, pr["link"])
    f32 = lambda a: np.asarray(a, F32).astype(np.float64)
    pr["bg"] = f32(pr["bg"] + bias_delta); pr["ba"] = f32(pr["ba"] + bias_delta)
    return pr, gt


# ------------------------------------------------------------------------------------------------ the cases shared by the CPU and GPU tests
def liba_case(synth, n_opt, lam, permute):
    """one-trial window of n_opt free key frames: about 12 points per key frame with 4 observations each.  The stereo share (0.3 / 1.0)
    alternates with the size, the covisible fixed key frames (0 at lambda 1, 3 at lambda 1e-2) with lambda, so every tiled size runs
    with and without them"""
    return hard_inertial_window(synth, 100 + n_opt, n_opt, stereo_frac=0.3 if n_opt % 2 else 1.0, n_covisible_fixed=3 if lam < 1 else 0,
                                permute=permute, lambda_init=lam)


# sizes of the device test: 1 free key frame; 4 = one 60-row tile exactly; 5 = the first two-tile system (75 unknowns, odd, so a padding
# row); 8 / 9 = 120 / 135 unknowns across the second tile boundary; 32 = the 480-unknown limit of 8 tiles.  permute alternates.
LIBA_DEVICE_CASES = [(n, lam, bool((n + (lam < 1)) % 2)) for n in (1, 4, 5, 8, 9, 32) for lam in (1.0, 1e-2)]
_trials = {}


def first_trial_of(synth, n_opt, lam, permute):
    """(window, liba_first_trial) of a case, computed once per session and left unchanged"""
    key = (n_opt, lam, permute)
    if key not in _trials:
        pr = liba_case(synth, n_opt, lam, permute)
        _trials[key] = (pr, liba_first_trial(pr))
    return _trials[key]


def degenerate_windows(synth):
    """no visual edges (a pure inertial chain); no links (a pure visual window); the single free key frame is LIBA_DEVICE_CASES' n = 1"""
    a = liba_case(synth, 4, 1.0, False)
    for k in ("edge_kf", "edge_point", "edge_inv_sigma2", "edge_stereo", "edge_obs", "points"):
        a[k] = a[k][:0]
    b = liba_case(synth, 4, 1.0, True)
    b["links"] = []
    return [("no visual edges", a), ("no links", b)]


def unclamped_lambda_window(synth):
    pr = hard_inertial_window(synth, 204, 5, big_rot=0.55)
    pr["huber_mono"] = pr["huber_stereo"] = pr["huber_inertial"] = 1e6
    return pr


def robust_link_windows(synth):
    """(window, robust link's chi2 above huber_inertial^2): the link to the fixed key frame carries the kernel; its information is scaled by
    1e-2 (Optimizer.cc:2651), so it takes a 0.3 rad perturbation on its free end to put its chi2 above 16.92; with 0.06 rad it is below"""
    return [(hard_inertial_window(synth, 300, 4, big_rot=0.3), True), (hard_inertial_window(synth, 300, 4), False)]


POSE_CASES = [dict(n=200), dict(n=200, stereo_frac=0.4), dict(n=200, stereo_frac=1.0), dict(n=25, outlier_frac=0.3), dict(n=0), dict(n=200, rec_init=1)]


def pose_case(synth, i, last_frame=False):
    """case i of POSE_CASES; last_frame=True: the same with the previous frame free and tied to synth's non-diagonal prior_H"""
    kw = dict(POSE_CASES[i])
    rec = kw.pop("rec_init", 0)
    pr, gt = hard_pose_inertial_problem(synth, (500 if last_frame else 400) + i, last_frame=last_frame, **kw)
    pr["rec_init"] = rec
    return pr, gt


def check_pose_result(pr, gt, r, check_hessian_blocks, prev=None):
    """a per-frame result against the reference: flags = planted outliers = flags restated at the returned state (no edge within 1 % of
    its threshold or with a depth near 0, no edge left out), counters consistent, H per 3 x 3 block at the returned state (and, for the
    last-frame variant, at the previous frame's state `prev`).  Returns pose_inertial_stationarity's (ratio, bound)."""
    n = len(pr["Xw"])
    flags = np.asarray(r["outlier"]).astype(bool)
    chi2, th, z, restated = pose_inertial_flags(pr, r)
    if n:
        assert np.abs(chi2 / th - 1).min() > 0.01 and np.abs(z).min() > 0.1, "case too close to a threshold: choose another seed"
    np.testing.assert_array_equal(flags, gt["is_outlier"])
    np.testing.assert_array_equal(flags, restated)
    assert r["n_bad"] == int(flags.sum()) and r["inliers"] == n - r["n_bad"]
    H = pose_inertial_hessian(pr, r, flags, prev).astype(np.float64)
    assert H.shape == np.asarray(r["H"]).shape
    check_hessian_blocks(H, np.asarray(r["H"]), "H against the long-double reference")
    return pose_inertial_stationarity(pr, r, prev)[:2]
