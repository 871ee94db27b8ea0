"""A numpy restatement of IMU pre-integration (a helper, not a test): the recurrences of IMU::Preintegrated::Initialize /
IntegrateNewMeasurement, the Get* of a changed bias with the prediction of Tracking::PredictStateIMU, the interpolation loop of
Tracking::PreintegrateIMU and the information matrix of EdgeInertial, with the working type as a parameter.

  truth                 T = np.longdouble, the polar factor by Newton's X <- (X + X^-T) / 2 to convergence
  float32 variants      VARIANTS: as written (polar factor by SVD); the matrix products associated the other way with the polar
                        factor by Newton; sin / cos taken in float64 and rounded
  the information       from a float C in mpmath at 60 digits (info9_truth), and the float64 restatement (info9_float64)

None of this is the code under test.  States are dictionaries of arrays of type T; measurements and biases are float32 values,
which every wider type holds exactly."""
import numpy as np

EPS = np.float32(1e-4)
GRAVITY = np.float32(9.81)
BLOCKS = ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "avgA", "avgW", "dT", "C9", "Cwalk")
PREDICTED = ("Rwb2", "twb2", "Vwb2")
VARIANTS = {"as_written": dict(polar="svd", assoc="left", trig="native"),
            "other_association": dict(polar="newton", assoc="right", trig="native"),
            "trig_float64": dict(polar="svd", assoc="left", trig="float64")}


def hat(v, T):
    z = T(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], dtype=T)


def _cofactor_inverse_transpose(X, T):
    c = np.empty((3, 3), dtype=T)
    for r in range(3):
        for q in range(3):
            r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (q + 1) % 3, (q + 2) % 3
            c[r, q] = X[r1, c1] * X[r2, c2] - X[r1, c2] * X[r2, c1]
    det = X[0, 0] * c[0, 0] + X[0, 1] * c[0, 1] + X[0, 2] * c[0, 2]
    return c / det


def polar_factor(X, T, how):
    """U V^T of X (NormalizeRotation)"""
    if how == "svd":
        U, _, Vt = np.linalg.svd(X.astype(np.float64 if T is np.longdouble else T))
        return (U @ Vt).astype(T)
    X = X.astype(T)
    for _ in range(100):
        N = (X + _cofactor_inverse_transpose(X, T)) / T(2)
        done = np.abs(N - X).max() <= 2 * np.finfo(T).eps
        X = N
        if done:
            break
    return X


def _sin_cos(d, T, trig):
    if trig == "float64" and T is np.float32:
        return T(np.sin(np.float64(d))), T(np.cos(np.float64(d)))
    return T(np.sin(d)), T(np.cos(d))


def rotation_increment(w, bias_w, dt, T, trig):
    """IntegratedRotation: (deltaR, rightJ)"""
    v = np.array([(T(w[k]) - T(bias_w[k])) * dt for k in range(3)], dtype=T)
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = T(np.sqrt(d2))
    W = hat(v, T)
    I = np.eye(3, dtype=T)
    if d < T(EPS):
        return I + W, I.copy(), True
    s, c = _sin_cos(d, T, trig)
    return I + W * s / d + W @ W * (T(1) - c) / d2, I - W * (T(1) - c) / d2 + W @ W * (d - s) / (d2 * d), False


def initialize(bias, nga, nga_walk, T):
    z3, z33 = np.zeros(3, dtype=T), np.zeros((3, 3), dtype=T)
    return dict(dT=T(0), b=np.asarray(bias, np.float32).astype(T), nga=np.asarray(nga, np.float32).astype(T), nga_walk=np.asarray(nga_walk, np.float32).astype(T),
                dR=np.eye(3, dtype=T), dV=z3.copy(), dP=z3.copy(), JRg=z33.copy(), JVg=z33.copy(), JVa=z33.copy(), JPg=z33.copy(), JPa=z33.copy(),
                avgA=z3.copy(), avgW=z3.copy(), C=np.zeros((15, 15), dtype=T), n_meas=0, first_order=0)


def integrate_one(s, a, w, dt, T, polar="newton", assoc="left", trig="native"):
    """IntegrateNewMeasurement on the state s (in place)"""
    dt = T(dt)
    half = T(0.5)
    b = s["b"]
    acc = np.array([T(a[k]) - b[k] for k in range(3)], dtype=T)
    accW = np.array([T(w[k]) - b[3 + k] for k in range(3)], dtype=T)
    dR, dT = s["dR"], s["dT"]
    s["avgA"] = (dT * s["avgA"] + dR @ acc * dt) / (dT + dt)
    s["avgW"] = (dT * s["avgW"] + accW * dt) / (dT + dt)
    s["dP"] = s["dP"] + s["dV"] * dt + half * dR @ acc * dt * dt
    s["dV"] = s["dV"] + dR @ acc * dt
    Wacc = hat(acc, T)
    A = np.eye(9, dtype=T)
    B = np.zeros((9, 6), dtype=T)
    A[3:6, 0:3] = -dR * dt @ Wacc
    A[6:9, 0:3] = -half * dR * dt * dt @ Wacc
    A[6:9, 3:6] = np.eye(3, dtype=T) * dt
    B[3:6, 3:6] = dR * dt
    B[6:9, 3:6] = half * dR * dt * dt
    s["JPa"] = s["JPa"] + s["JVa"] * dt - half * dR * dt * dt
    s["JPg"] = s["JPg"] + s["JVg"] * dt - half * dR * dt * dt @ Wacc @ s["JRg"]
    s["JVa"] = s["JVa"] - dR * dt
    s["JVg"] = s["JVg"] - dR * dt @ Wacc @ s["JRg"]
    deltaR, rightJ, first_order = rotation_increment(w, b[3:], dt, T, trig)
    s["first_order"] += int(first_order)
    s["dR"] = polar_factor(dR @ deltaR, T, polar)
    A[0:3, 0:3] = deltaR.T
    B[0:3, 0:3] = rightJ * dt
    N = np.diag(s["nga"])
    C9 = s["C"][0:9, 0:9]
    if assoc == "left":
        s["C"][0:9, 0:9] = (A @ C9) @ A.T + (B @ N) @ B.T
    else:
        s["C"][0:9, 0:9] = A @ (C9 @ A.T) + B @ (N @ B.T)
    s["C"][9:15, 9:15] += np.diag(s["nga_walk"])
    s["JRg"] = deltaR.T @ s["JRg"] - rightJ * dt
    s["dT"] = dT + dt
    s["n_meas"] += 1
    assert all(v.dtype == T for v in s.values() if isinstance(v, np.ndarray)) and type(s["dT"]) is T
    return s


def integrate(case, T, polar="newton", assoc="left", trig="native", state=None, first=0, count=None):
    """Initialize(bias) (unless a state is given) and the measurements case["a"], ["w"], ["dt"][first : first + count] in order"""
    s = initialize(case["bias"], case["nga"], case["nga_walk"], T) if state is None else state
    n = len(case["dt"]) if count is None else first + count
    for i in range(first, n):
        integrate_one(s, case["a"][i], case["w"][i], case["dt"][i], T, polar, assoc, trig)
    return s


def truth(case):
    return integrate(case, np.longdouble, "newton")


def exp_so3(v, T):
    d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2]
    d = T(np.sqrt(d2))
    W = hat(v, T)
    I = np.eye(3, dtype=T)
    if d2 < T(1e-16):
        return I + W + W @ W * T(0.5)
    return I + W * T(np.sin(d)) / d + W @ W * (T(1) - T(np.cos(d))) / d2



def predict(s, Rwb1, twb1, Vwb1, bias, T, polar="newton"):
    """PredictStateIMU's arithmetic with GetDeltaRotation / Velocity / Position(bias): (Rwb2, twb2, Vwb2)"""
    Rwb1, twb1, Vwb1 = (np.asarray(x, np.float32).astype(T) for x in (Rwb1, twb1, Vwb1))
    bias = np.asarray(bias, np.float32).astype(T)
    dba, dbg = bias[:3] - s["b"][:3], bias[3:] - s["b"][3:]
    dRb = polar_factor(s["dR"] @ exp_so3(s["JRg"] @ dbg, T), T, polar)
    dVb = s["dV"] + s["JVg"] @ dbg + s["JVa"] @ dba
    dPb = s["dP"] + s["JPg"] @ dbg + s["JPa"] @ dba
    t = s["dT"]
    Gz = np.array([0, 0, -T(GRAVITY)], dtype=T)
    return dict(Rwb2=polar_factor(Rwb1 @ dRb, T, polar), twb2=twb1 + Vwb1 * t + T(0.5) * t * t * Gz + Rwb1 @ dPb, Vwb2=Vwb1 + t * Gz + Rwb1 @ dVb)


def blocks(s):
    """the output blocks of a state that the tolerance rule names"""
    out = {k: np.asarray(s[k]) for k in BLOCKS[:11]}
    C = np.asarray(s["C"]).reshape(15, 15)
    out["C9"] = C[0:9, 0:9]
    out["Cwalk"] = np.diagonal(C[9:15, 9:15])
    return out


def block_error(X, truth_):
    """max |X - truth| / max |truth|; a block that is zero in truth has to be zero"""
    X, t = np.asarray(X, np.longdouble), np.asarray(truth_, np.longdouble)
    den = np.abs(t).max()
    if den == 0:
        return 0.0 if np.abs(X).max() == 0 else float("inf")
    return float(np.abs(X - t).max() / den)


def zero_blocks_are_zero(C):
    C = np.asarray(C).reshape(15, 15)
    off = C[9:15, 9:15] - np.diag(np.diagonal(C[9:15, 9:15]))
    return not C[0:9, 9:15].any() and not C[9:15, 0:9].any() and not off.any()


# ---- the information of a link ----
def info9_truth(C, info_scale=1.0):
    """EdgeInertial's information from the float C, in mpmath at 60 digits, rounded to float64"""
    import mpmath as mp
    with mp.workdps(60):
        M = mp.matrix(9, 9)
        Cf = np.asarray(C, np.float32).reshape(15, 15)
        for r in range(9):
            for c in range(9):
                M[r, c] = mp.mpf(float(Cf[r, c]))
        Inv = M ** -1
        Sym = (Inv + Inv.T) / 2
        E, Q = mp.eigsy(Sym)
        for k in range(9):
            if E[k] < mp.mpf("1e-12"):
                E[k] = mp.mpf(0)
        R = Q * mp.diag([E[k] for k in range(9)]) * Q.T * mp.mpf(info_scale)
        return np.array([[float(R[r, c]) for c in range(9)] for r in range(9)], np.float64)


def info9_float64(C, info_scale=1.0):
    Cf = np.asarray(C, np.float32).reshape(15, 15)[0:9, 0:9].astype(np.float64)
    Inv = np.linalg.inv(Cf)
    Sym = (Inv + Inv.T) / 2
    E, Q = np.linalg.eigh(Sym)
    E[E < 1e-12] = 0
    return (Q * E) @ Q.T * info_scale


def info9_bound(C):
    """100 kappa_2(C9) 2^-53 on the relative Frobenius error"""
    Cf = np.asarray(C, np.float32).reshape(15, 15)[0:9, 0:9].astype(np.float64)
    return 100 * float(np.linalg.cond(Cf, 2)) * 2.0 ** -53


def walk_info(C):
    Cf = np.asarray(C, np.float32).reshape(15, 15).astype(np.float64)
    return np.linalg.inv(Cf[9:12, 9:12]), np.linalg.inv(Cf[12:15, 12:15])


def rel_frobenius(X, t):
    return float(np.linalg.norm(np.asarray(X, np.float64) - t) / np.linalg.norm(t))


# ---- the interpolation loop of Tracking::PreintegrateIMU, float32 ----
def frame_measurements(ts_ns, gyro, acce, t_prev_ns, t_cur_ns):
    """samples (int64 ns, float32 [n][3] x 2) of one stream -> (a [n-1][3], w [n-1][3], dt [n-1]) float32; times are ts / 1e9 in double"""
    sec = lambda x: np.float64(np.int64(x)) / np.float64(1e9)
    return frame_measurements_seconds([sec(x) for x in ts_ns], gyro, acce, sec(t_prev_ns), sec(t_cur_ns))


def frame_measurements_seconds(t, gyro, acce, tp, tc):
    """the same with the times as doubles in seconds (IMU::Point::t, Frame::mTimeStamp)"""
    f = np.float32
    n = max(len(t) - 1, 0)
    t, tp, tc = [np.float64(x) for x in t], np.float64(tp), np.float64(tc)
    A, W, D = np.zeros((n, 3), f), np.zeros((n, 3), f), np.zeros(n, f)
    acce, gyro = np.asarray(acce, f), np.asarray(gyro, f)
    for i in range(n):
        if i == 0 and i < n - 1:
            tab, tini = f(t[i + 1] - t[i]), f(t[i] - tp)
            k = f(tini / tab)
            A[i] = (acce[i] + acce[i + 1] - (acce[i + 1] - acce[i]) * k) * f(0.5)
            W[i] = (gyro[i] + gyro[i + 1] - (gyro[i + 1] - gyro[i]) * k) * f(0.5)
            D[i] = f(t[i + 1] - tp)
        elif i < n - 1:
            A[i] = (acce[i] + acce[i + 1]) * f(0.5)
            W[i] = (gyro[i] + gyro[i + 1]) * f(0.5)
            D[i] = f(t[i + 1] - t[i])
        elif i > 0:
            tab, tend = f(t[i + 1] - t[i]), f(t[i + 1] - tc)
            k = f(tend / tab)
            A[i] = (acce[i] + acce[i + 1] - (acce[i + 1] - acce[i]) * k) * f(0.5)
            W[i] = (gyro[i] + gyro[i + 1] - (gyro[i + 1] - gyro[i]) * k) * f(0.5)
            D[i] = f(tc - t[i])
        else:
            A[i], W[i], D[i] = acce[i], gyro[i], f(tc - tp)
    return A, W, D
