"""Dense reference for FullInertialBA (fiba_solve; reference src/Optimizer.cc:392-811).  A test helper, not a test.

Every edge term, Jacobian, float getter, Huber weight, the refined solve and the step tolerance are those of
dense_inertial_reference.py / dense_ba_reference.py, imported.  Added here: what the whole-map function does differently --
  - the column map with ONE gyro-bias and ONE accelerometer-bias vertex for the map (bInit, :456-466, :506-510): the 6 shared
    columns come last and every link's G1 / A1 columns address them;
  - EdgePriorGyro / EdgePriorAcc with prior value 0 (:570-590).  `as_written=False` reads the edge as estimate - prior, as the
    solvers do; True as the text has it: computeError prior - estimate (G2oTypes.h:778-781,802-805) with linearizeOplus +I
    (G2oTypes.cc:762-774), which flips the sign of the edge's gradient and leaves its Hessian and chi2;
  - a Huber kernel on every inertial edge (:540-542), none on the random walks, which exist only without a shared bias;
  - g2o activates only vertices that have an edge: the IMU states of a key frame in no link, the pose of a key frame with neither
    an observation nor a link, and a point none of whose observers is free (bAllFixed, :714-718) are no unknowns and do not move;
  - ImuCamPose::Update re-orthonormalises Rwb on every third update of a pose (its >= 3), which only a run of several iterations meets;
  - first_trial: one Levenberg trial at lambda_init (long double by default), like liba_first_trial;
  - optimize: the whole Levenberg loop on the dense system with the policy of csrc/lm_control.h
    (optimization_algorithm_levenberg.cpp:61-169 inside sparse_optimizer.cpp:395-414), in float64, float64 with the unknowns in
    reverse order, or long double.
A float64 run evaluates the imported terms in float64 too: the helper modules take their working type from their global LD, which
`precision` rebinds for the duration of a run."""
import contextlib

import numpy as np
import scipy.linalg

import dense_ba_reference as D
import dense_inertial_reference as R
from dense_ba_reference import solve_refined, step_tolerance
from dense_inertial_reference import BLOCKS, F32, _block_steps, _ratio, copy_state, get_deltas, inertial_error, inertial_jacobian, state_of, update_pose, visual_terms

LD = np.longdouble


@contextlib.contextmanager
def precision(T):
    """the working type of dense_ba_reference / dense_inertial_reference for the duration of a run"""
    saved = (D.LD, R.LD, R.I3, R.GRAVITY)
    D.LD = R.LD = T
    R.I3 = np.eye(3, dtype=T); R.GRAVITY = np.asarray(saved[3], T)
    try:
        yield
    finally:
        D.LD, R.LD, R.I3, R.GRAVITY = saved


# ------------------------------------------------------------------------------------------------ what is an unknown
def active_sets(pr):
    nk = int(pr["n_kf"])
    linked = np.zeros(nk, bool); seen = np.zeros(nk, bool)
    for L in pr["links"]:
        linked[int(L["kf1"])] = linked[int(L["kf2"])] = True
    ek = np.asarray(pr["edge_kf"], int); el = np.asarray(pr["edge_point"], int)
    seen[ek] = True
    pose_free = (np.asarray(pr["pose_fixed"]) == 0) & (linked | seen)
    imu_free = (np.asarray(pr["has_imu"]) != 0) & (np.asarray(pr["imu_fixed"]) == 0) & linked
    keep_pt = np.zeros(len(np.asarray(pr["points"]).reshape(-1, 3)), bool)
    keep_pt[el[pose_free[ek]]] = True
    return dict(pose_free=pose_free, imu_free=imu_free, keep_pt=keep_pt, keep_edge=keep_pt[el] if len(el) else np.zeros(0, bool))


def column_map(pr, act):
    """offsets of pose (6), velocity (3), gyro bias, accelerometer bias (3 each) per key frame, -1 where there is no unknown; with a
    shared bias og / oa of every key frame with IMU states are the shared columns n - 6, n - 3"""
    nk = int(pr["n_kf"])
    shared = bool(pr.get("shared_bias", 0))
    op, ov, og, oa = (-np.ones(nk, int) for _ in range(4))
    k = 0
    for i in range(nk):
        if act["pose_free"][i]:
            op[i] = k; k += 6
        if act["imu_free"][i]:
            ov[i] = k; k += 3
            if not shared:
                og[i] = k; oa[i] = k + 3; k += 6
    if shared:
        imu = np.asarray(pr["has_imu"]) != 0
        og[imu] = k; oa[imu] = k + 3; k += 6
    return dict(op=op, ov=ov, og=og, oa=oa, n=k, shared=shared)


def reduced_problem(pr, act):
    """the problem as liba_chi2 / the edge loops see it: every link robust, no random walks with a shared bias, only the kept edges"""
    shared = bool(pr.get("shared_bias", 0))
    q = dict(pr)
    q["links"] = [dict(L, robust=1, **(dict(info_gyro=np.zeros((3, 3)), info_acc=np.zeros((3, 3))) if shared else {})) for L in pr["links"]]
    ke = act["keep_edge"]
    for k in ("edge_kf", "edge_point", "edge_obs", "edge_inv_sigma2", "edge_stereo"):
        q[k] = np.asarray(pr[k])[ke]
    return q


def initial_state(pr):
    s = state_of(pr)
    s["its"] = np.zeros(int(pr["n_kf"]), int)              # ImuCamPose::its: updates since the last NormalizeRotation of Rwb
    if pr.get("shared_bias", 0):
        imu = np.asarray(pr["has_imu"]) != 0
        s["bg"][imu] = np.asarray(pr["shared_bg"], R.LD); s["ba"][imu] = np.asarray(pr["shared_ba"], R.LD)
    return s


def chi2(pr, q, s):
    """the active robust chi2 at state s: links (Huber on all), random walks or the two priors, the kept visual edges"""
    tot, link_chi2, _, _ = R.liba_chi2(q, s)
    if pr.get("shared_bias", 0):
        kb = int(pr["links"][0]["kf1"])
        tot = tot + R.LD(pr["prior_g"]) * (s["bg"][kb] * s["bg"][kb]).sum() + R.LD(pr["prior_a"]) * (s["ba"][kb] * s["ba"][kb]).sum()
    return tot, link_chi2


# ------------------------------------------------------------------------------------------------ linearisation and one trial
def linearize(pr, q, s0, act, cm, as_written=False):
    """H, b over the pose / velocity / bias columns of the column map, and the landmark parts Hll, bl, W of the kept edges"""
    T = R.LD
    n = cm["n"]
    op, ov, og, oa = cm["op"], cm["ov"], cm["og"], cm["oa"]
    H = np.zeros((n, n), T); b = np.zeros(n, T)
    link_sys = []
    dims = [6, 3, 3, 3, 6, 3]
    for L in q["links"]:
        e = inertial_error(L, s0); J = inertial_jacobian(L, s0)
        Om = np.asarray(L["info9"], T).reshape(9, 9)
        c = e @ Om @ e
        Om = D.huber(c, pr["huber_inertial"])[1] * Om
        k1, k2 = int(L["kf1"]), int(L["kf2"])
        off = [op[k1], ov[k1], og[k1], oa[k1], op[k2], ov[k2]]
        cols = np.concatenate([np.arange(o, o + d) if o >= 0 else -np.ones(d, int) for o, d in zip(off, dims)])
        ok = cols >= 0
        Jf = J[:, ok]
        H[np.ix_(cols[ok], cols[ok])] += Jf.T @ Om @ Jf
        b[cols[ok]] -= Jf.T @ Om @ e
        link_sys.append((cols[ok], Jf.T @ Om))
        if cm["shared"]:
            continue
        for key, info, o in (("bg", "info_gyro", og), ("ba", "info_acc", oa)):          # EdgeGyroRW / EdgeAccRW: e = b2 - b1, J = (-I, +I)
            O3 = np.asarray(L[info], T).reshape(3, 3)
            d = s0[key][k2] - s0[key][k1]
            for k, sg in ((k1, -1), (k2, 1)):
                if o[k] >= 0:
                    a = o[k]
                    H[a:a + 3, a:a + 3] += O3
                    b[a:a + 3] -= sg * (O3 @ d)
            if o[k1] >= 0 and o[k2] >= 0:
                a1, a2 = o[k1], o[k2]
                H[a1:a1 + 3, a2:a2 + 3] -= O3
                H[a2:a2 + 3, a1:a1 + 3] -= O3
    if cm["shared"]:
        kb = int(pr["links"][0]["kf1"])
        sign = 1 if as_written else -1          # b = -J^T Omega e with J = +I: e = estimate gives -prior * estimate, e = -estimate the opposite
        for key, prior, o in (("bg", "prior_g", og[kb]), ("ba", "prior_a", oa[kb])):
            H[o:o + 3, o:o + 3] += T(pr[prior]) * np.eye(3, dtype=T)
            b[o:o + 3] += sign * T(pr[prior]) * s0[key][kb]
    ek = np.asarray(q["edge_kf"], int); el = np.asarray(q["edge_point"], int)
    st = np.asarray(q["edge_stereo"]).astype(bool)
    nL = len(s0["points"])
    Hll = np.zeros((nL, 3, 3), T); bl = np.zeros((nL, 3), T)
    W = np.zeros((len(ek), 6, 3), T)
    if len(ek):
        r, _, Ji, Jj = visual_terms(q, s0["Rwb"][ek], s0["twb"][ek], s0["points"][el], q["edge_obs"], st)
        c2 = np.asarray(q["edge_inv_sigma2"], T) * (r * r).sum(1)
        wgt = D.huber(c2, np.where(st, q["huber_stereo"], q["huber_mono"]))[1] * np.asarray(q["edge_inv_sigma2"], T)
        np.add.at(Hll, el, np.einsum("edi,e,edj->eij", Ji, wgt, Ji))
        np.add.at(bl, el, -np.einsum("edi,e,ed->ei", Ji, wgt, r))
        Hjj = np.einsum("edi,e,edj->eij", Jj, wgt, Jj)
        bj = -np.einsum("edi,e,ed->ei", Jj, wgt, r)
        W = np.einsum("edi,e,edj->eij", Jj, wgt, Ji)
        for e in np.nonzero(op[ek] >= 0)[0]:
            o = op[ek[e]]
            H[o:o + 6, o:o + 6] += Hjj[e]
            b[o:o + 6] += bj[e]
    by_pt = [[] for _ in range(nL)]
    for e in np.nonzero(op[ek] >= 0)[0] if len(ek) else []:
        by_pt[el[e]].append(e)
    return dict(H=H, b=b, Hll=Hll, bl=bl, W=W, by_pt=by_pt, ek=ek, el=el, link_sys=link_sys)


def reduced_system(lin, cm, lam, act):
    T = R.LD
    n = cm["n"]
    op = cm["op"]
    nL = len(lin["Hll"])
    Dinv = np.zeros((nL, 3, 3), T)
    kp = np.nonzero(act["keep_pt"])[0]
    if len(kp):
        Dinv[kp] = D.inv3(lin["Hll"][kp] + lam * np.eye(3, dtype=T))
    S = lin["H"] + lam * np.eye(n, dtype=T)
    bs = lin["b"].copy()
    W, ek, bl = lin["W"], lin["ek"], lin["bl"]
    for l, es in enumerate(lin["by_pt"]):
        for ea in es:
            oa = op[ek[ea]]
            Z = W[ea] @ Dinv[l]
            bs[oa:oa + 6] -= Z @ bl[l]
            for eb in es:
                ob = op[ek[eb]]
                S[oa:oa + 6, ob:ob + 6] -= Z @ W[eb].T
    return S, bs, Dinv


def apply_step(pr, s0, lin, cm, x, Dinv):
    """the state after the step x of the reduced system (landmarks by back-substitution), the steps per block, the point steps"""
    T = R.LD
    op, ov, og, oa = cm["op"], cm["ov"], cm["og"], cm["oa"]
    W, ek, bl = lin["W"], lin["ek"], lin["bl"]
    nL = len(lin["Hll"])
    xl = np.zeros((nL, 3), T)
    for l, es in enumerate(lin["by_pt"]):
        if not es:
            continue
        c = bl[l].copy()
        for e in es:
            o = op[ek[e]]
            c -= W[e].T @ x[o:o + 6]
        xl[l] = Dinv[l] @ c
    s1 = copy_state(s0)
    nk = int(pr["n_kf"])
    steps = {k: np.full((nk, 3), np.nan, T) for k in BLOCKS}
    for i in range(nk):
        if op[i] >= 0:
            update_pose(s1, i, x[op[i]:op[i] + 6])
            s1["its"][i] += 1                               # G2oTypes.cc:222-227: every third update Rwb is re-orthonormalised (the inputs
            if s1["its"][i] >= 3:                           # are float matrices, orthogonal to 6e-8 only, so this moves them); push / pop
                s1["Rwb"][i] = R.polar(s1["Rwb"][i])        # restore the counter with the estimate
                s1["its"][i] = 0
            steps["rot"][i] = x[op[i]:op[i] + 3]; steps["trans"][i] = x[op[i] + 3:op[i] + 6]
        for key, o in (("vel", ov[i]), ("bg", og[i]), ("ba", oa[i])):
            if o >= 0:
                s1[key][i] = s1[key][i] + x[o:o + 3]
                steps[key][i] = x[o:o + 3]
    s1["points"] = s0["points"] + xl
    return s1, steps, xl


def _solve(S, bs, T, reverse, refine=3):
    """(x, solved, resid, kappa): long double through solve_refined, float64 by Cholesky; reverse eliminates the unknowns last first"""
    n = len(bs)
    perm = np.arange(n)[::-1] if reverse else np.arange(n)
    A = S[np.ix_(perm, perm)]; rhs = bs[perm]
    try:
        c = scipy.linalg.cho_factor(A.astype(np.float64), lower=True)
    except np.linalg.LinAlgError:
        return np.zeros(n, T), False, None, None
    if T is np.float64:
        y, resid, kappa = scipy.linalg.cho_solve(c, rhs), None, None
    else:
        y, resid, kappa = solve_refined(A, rhs, refine)
    x = np.zeros(n, T)
    x[perm] = y
    return x, True, resid, kappa


def first_trial(pr, dtype=LD, as_written=False, refine=3):
    """The first Levenberg trial of FullInertialBA at lambda_init; the dictionary of liba_first_trial plus the column map"""
    with precision(dtype):
        T = R.LD
        act = active_sets(pr); cm = column_map(pr, act); q = reduced_problem(pr, act)
        s0 = initial_state(pr)
        lam = T(pr["lambda_init"])
        lin = linearize(pr, q, s0, act, cm, as_written)
        S, bs, Dinv = reduced_system(lin, cm, lam, act)
        x, solved, resid, kappa = _solve(S, bs, T, False, refine)
        assert solved
        if kappa is None:
            kappa = float(np.linalg.cond(S.astype(np.float64)))
        s1, steps, xl = apply_step(pr, s0, lin, cm, x, Dinv)
        chi_ini, link_chi2 = chi2(pr, q, s0)
        chi_new, _ = chi2(pr, q, s1)
        scale = (x * (lam * x + lin["b"])).sum() + (xl * (lam * xl + lin["bl"])).sum() + T(1e-3)
        rho = (chi_ini - chi_new) / scale
        lam_next = lam * max(T(1) / 3, min(T(2) / 3, 1 - (2 * rho - 1) ** 3)) if rho > 0 else lam * 2
        return dict(steps=steps, point_step=xl, state=s1, chi2_initial=chi_ini, chi2_final=chi_new, rho=rho, lambda_=lam_next, kappa=kappa,
                    resid=resid, link_chi2=link_chi2, n_unknowns=cm["n"], x=x, cm=cm, act=act,
                    _sys=dict(S=S.astype(np.float64), S_ld=S, bs=bs, link_sys=lin["link_sys"], Dinv=Dinv, W=lin["W"], by_pt=lin["by_pt"], ek=lin["ek"]))


def optimize(pr, dtype=np.float64, reverse=False, as_written=False):
    """FullInertialBA's optimize(max_iters) with setUserLambdaInit(lambda_init): the loop of lm_control.h.  Returns the final state's
    arrays (Rwb, twb, vel, bg, ba, points), chi2_initial / chi2_final and stats (iterations, trials, stop_reason, lambda_)."""
    with precision(dtype):
        T = R.LD
        act = active_sets(pr); cm = column_map(pr, act); q = reduced_problem(pr, act)
        s = initial_state(pr)
        lam = T(pr["lambda_init"]); ni = T(2)
        n_bad = iterations = trials = stop_reason = 0
        chi, _ = chi2(pr, q, s)
        chi_initial = chi
        for _ in range(int(pr["max_iters"])):
            lin = linearize(pr, q, s, act, cm, as_written)
            ini_chi = chi
            rho = T(0); qmax = 0
            while True:
                S, bs, Dinv = reduced_system(lin, cm, lam, act)
                x, solved, _, _ = _solve(S, bs, T, reverse)
                s1, _, xl = apply_step(pr, s, lin, cm, x, Dinv)
                temp = chi2(pr, q, s1)[0] if solved else T(np.finfo(np.float64).max)
                scale = (x * (lam * x + lin["b"])).sum() + (xl * (lam * xl + lin["bl"])).sum()
                rho = (chi - temp) / (scale + T(1e-3))
                if rho > 0 and np.isfinite(temp):
                    alpha = min(1 - (2 * rho - 1) ** 3, T(2) / 3)
                    lam = lam * max(T(1) / 3, alpha); ni = T(2)
                    chi = temp; s = s1
                else:
                    lam = lam * ni; ni = ni * 2
                qmax += 1; trials += 1
                if not (rho < 0 and qmax < 10):
                    break
            iterations += 1
            if qmax == 10 or rho == 0:
                stop_reason = 1
                break
            n_bad = n_bad + 1 if (ini_chi - chi) * 1e3 < ini_chi else 0
            if n_bad >= 3:
                stop_reason = 2
                break
        out = {k: np.array(s[k]) for k in ("Rwb", "twb", "vel", "bg", "ba", "points")}
        out.update(chi2_initial=chi_initial, chi2_final=chi, stats=dict(iterations=iterations, trials=trials, stop_reason=stop_reason, lambda_=lam))
        return out


# ------------------------------------------------------------------------------------------------ comparing a one-trial output
def getter_floor(pr, ref):
    """dense_inertial_reference.float_getter_floor on this column map: the step that a one-float-ulp change of every bias-corrected
    dR, dV, dP produces, per block (absolute), from the inputs alone"""
    sy, cm = ref["_sys"], ref["cm"]
    n, nk = cm["n"], int(pr["n_kf"])
    s0 = initial_state(pr)
    floors = {k: np.zeros(nk) for k in BLOCKS}
    fl_pts = np.zeros(len(s0["points"]))
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
    if not rhs:
        return dict(floors, points=fl_pts)
    X = np.linalg.solve(sy["S"], np.array(rhs).T)
    rss = lambda M: np.sqrt((M * M).sum())
    for i in range(nk):
        if cm["op"][i] >= 0:
            floors["rot"][i] = rss(X[cm["op"][i]:cm["op"][i] + 3]); floors["trans"][i] = rss(X[cm["op"][i] + 3:cm["op"][i] + 6])
        for key, o in (("vel", cm["ov"][i]), ("bg", cm["og"][i]), ("ba", cm["oa"][i])):
            if o >= 0:
                floors[key][i] = rss(X[o:o + 3])
    W = sy["W"].astype(np.float64); Dinv = sy["Dinv"].astype(np.float64)
    for l, es in enumerate(sy["by_pt"]):
        if es:
            c = sum(W[e].T @ X[cm["op"][sy["ek"][e]]:cm["op"][sy["ek"][e]] + 6] for e in es)
            fl_pts[l] = rss(Dinv[l] @ c)
    return dict(floors, points=fl_pts)


QUALITY = 1e-6      # no block of a one-trial case is granted more than this share of its step, whatever its float-getter floor


def _tolerance(step, tol0, floor):
    """absolute tolerance of a block: dense_inertial_reference's tol0 |step| + 10 floor, but at most QUALITY |step| (a block whose
    reference step is exactly 0 keeps the floor alone)"""
    t = tol0 * step + 10 * floor
    return min(t, QUALITY * step) if step > 0 else t


def block_tolerances(pr, ref):
    """(the largest relative tolerance step_error applies to a block, the same without the QUALITY cap, the floors)"""
    floor = getter_floor(pr, ref)
    tol0 = step_tolerance(ref["kappa"])
    nrm = lambda a: float(np.sqrt((a * a).sum()))
    worst, uncapped = tol0, tol0
    blocks = [(ref["steps"][k][i], floor[k][i]) for k in BLOCKS for i in range(int(pr["n_kf"])) if not np.isnan(ref["steps"][k][i]).any()]
    blocks += [(ref["point_step"][l], floor["points"][l]) for l, es in enumerate(ref["_sys"]["by_pt"]) if es]
    for st, fl in blocks:
        if nrm(st) > 0:
            worst = max(worst, min(tol0 + 10 * fl / nrm(st), QUALITY))
            uncapped = max(uncapped, tol0 + 10 * fl / nrm(st))
    return worst, uncapped, floor


def _ratio_capped(err, step, tol0, floor):
    if floor is None:
        return _ratio(err, step, tol0, None)
    den = _tolerance(step, tol0, floor)
    return err / den if den > 0 else (0.0 if err == 0 else np.inf)


def step_error(pr, out, ref, floor=None):
    """liba_step_error on this column map: the worst per-block error of a one-trial output against first_trial, relative to the block's
    step, or (with floor) to its tolerance, which never exceeds QUALITY of the block's step.  A block that is no unknown must come back exactly: with a shared bias every key frame
    with IMU states carries the shared step."""
    s0 = initial_state(pr); s1 = state_of(out)
    got = _block_steps(pr, s0, s1); want = _block_steps(pr, s0, ref["state"])
    tol0 = step_tolerance(ref["kappa"])
    worst, where = 0.0, None
    nrm = lambda a: float(np.sqrt((a * a).sum()))
    for k in BLOCKS:
        for i in range(int(pr["n_kf"])):
            if np.isnan(ref["steps"][k][i]).any():
                assert nrm(got[k][i]) == 0, "block %s of key frame %d is no unknown and moved" % (k, i)
                continue
            rel = _ratio_capped(nrm(got[k][i] - want[k][i]), nrm(want[k][i]), tol0, None if floor is None else floor[k][i])
            if rel > worst:
                worst, where = rel, (k, i)
    d = s1["points"] - ref["state"]["points"]
    for l in range(len(d)):
        rel = _ratio_capped(nrm(d[l]), nrm(ref["point_step"][l]), tol0, None if floor is None else floor["points"][l])
        if rel > worst:
            worst, where = rel, ("point", l)
    return worst, where


def recovered_step(pr, out, ref):
    """the step x of the reduced system that takes the initial state to a solver's output, through the update rule"""
    cm = ref["cm"]
    s0 = initial_state(pr); s1 = state_of(out)
    st = _block_steps(pr, s0, s1)
    x = np.zeros(cm["n"], LD)
    for i in range(int(pr["n_kf"])):
        if cm["op"][i] >= 0:
            x[cm["op"][i]:cm["op"][i] + 3] = st["rot"][i]; x[cm["op"][i] + 3:cm["op"][i] + 6] = st["trans"][i]
        for key, o in (("vel", cm["ov"][i]), ("bg", cm["og"][i]), ("ba", cm["oa"][i])):
            if o >= 0:
                x[o:o + 3] = st[key][i]
    return x


def backward_error(pr, out, ref):
    """|(H + lambda I) x - b| / |b| of the recovered step in the reference's long-double reduced system"""
    x = recovered_step(pr, out, ref)
    S, bs = ref["_sys"]["S_ld"], ref["_sys"]["bs"]
    r = S @ x - bs
    return float(np.sqrt((r * r).sum() / (bs * bs).sum()))


def chi2_final_rtol(ref):
    """Relative tolerance on the chi2 after the trial.  A step that is off by delta of its norm (delta <= step_tolerance(kappa), what
    check_one_step grants the states) moves the new cost to first order by the gradient there times the error, at most about
    2 delta times the decrease the step achieved; 1e-11 is dense_inertial_reference.check_one_step's figure for summation order."""
    gain = float((ref["chi2_initial"] - ref["chi2_final"]) / ref["chi2_final"])
    return 1e-11 + 2 * step_tolerance(ref["kappa"]) * gain


def check_scalars(r, ref):
    st = r["stats"]
    assert st["iterations"] == 1 and st["trials"] == 1 and ref["rho"] > 0, (st, float(ref["rho"]))
    np.testing.assert_allclose(st["chi2_initial"], float(ref["chi2_initial"]), rtol=1e-12)
    np.testing.assert_allclose(st["chi2_final"], float(ref["chi2_final"]), rtol=chi2_final_rtol(ref))


def check_one_step(pr, r, ref):
    """a one-trial output (max_iters = 1) against first_trial by dense_inertial_reference.check_one_step's rule: the scalars, then every
    block within step_tolerance(kappa) + 10 float-getter floors and within QUALITY of its step.  Returns (plain step error, error / tolerance)."""
    check_scalars(r, ref)
    assert ref["resid"] < 1e-15, "reference solve residual %.3g" % ref["resid"]
    err, _ = step_error(pr, r, ref)
    ratio, where = step_error(pr, r, ref, getter_floor(pr, ref))
    assert ratio <= 1, "step error / tolerance %.3g at %s (plain error %.3g, kappa %.3g)" % (ratio, where, err, ref["kappa"])
    return err, ratio


# ------------------------------------------------------------------------------------------------ what a free gauge leaves alone
def gauge_invariants(pr, out):
    """biases; per link Rwb_i^T Rwb_j, Rwb_i^T (twb_j - twb_i), Rwb_i^T v_i, Rwb_j^T v_j; the z components of Rwb's third row, of the
    translation differences and of the velocities (gravity pins roll and pitch, and leaves yaw and the translation free)"""
    Rw, t, v = (np.asarray(out[k], LD) for k in ("Rwb", "twb", "vel"))
    rel_R, rel_t, body_v = [], [], []
    for L in pr["links"]:
        i, j = int(L["kf1"]), int(L["kf2"])
        rel_R.append(Rw[i].T @ Rw[j]); rel_t.append(Rw[i].T @ (t[j] - t[i])); body_v.append(Rw[i].T @ v[i]); body_v.append(Rw[j].T @ v[j])
    imu = np.asarray(pr["has_imu"]) != 0
    return dict(bg=np.asarray(out["bg"], LD)[imu], ba=np.asarray(out["ba"], LD)[imu], rel_R=np.array(rel_R), rel_t=np.array(rel_t), body_v=np.array(body_v),
                z=np.concatenate([Rw[:, 2, :].ravel(), (t[:, 2] - t[0, 2]), v[imu, 2]]))


FULL_BLOCKS_FIXED = ("Rwb", "twb", "vel", "bg", "ba", "points")
FULL_BLOCKS_FREE = ("bg", "ba", "rel_R", "rel_t", "body_v", "z")


def full_run_blocks(pr, out, gauge_free):
    if gauge_free:
        return gauge_invariants(pr, out)
    return {k: np.asarray(out[k], LD) for k in FULL_BLOCKS_FIXED}
