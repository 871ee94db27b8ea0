"""The seeded cases of the IMU pre-integration tests (a helper, not a test): measurements of gravity plus N(0, 1.5) m/s^2 and
N(0, 0.4) rad/s at dt = 0.005, a non-zero bias and the noise diagonals of a 200 Hz EuRoC-class IMU.  The lengths are the smallest at
which each path can break: 1 (every Jacobian but JRg, JVa, JPa is zero), 2, 3, 7, 65 (past one wave, if lanes shared a job), 400;
two seeds per length.  "slow7" turns at a gyro-minus-bias rate below 1e-4 / dt, so every one of its measurements takes the
first-order branch of the rotation increment; it belongs to the cases of length 7.  "fast3" turns by about 0.7 rad per sample (no IMU
does; an implementation may take sin and cos another way at small angles, and this is the case beyond any such threshold); it
belongs to the cases of length 3."""
import numpy as np

DT = np.float32(0.005)
FREQ = 200.0
# NoiseGyro, NoiseAcc, GyroWalk, AccWalk of a EuRoC-class IMU, as IMU::Calib::Set squares them (continuous -> discrete at 200 Hz)
NG, NA, NGW, NAW = 1.7e-4, 2.0e-3, 1.9393e-5, 3.0e-3
_sf = np.sqrt(FREQ)
NGA = np.array([(NG * _sf) ** 2] * 3 + [(NA * _sf) ** 2] * 3, np.float32)
NGA_WALK = np.array([(NGW / _sf) ** 2] * 3 + [(NAW / _sf) ** 2] * 3, np.float32)

LENGTHS = (1, 2, 3, 7, 65, 400)
CASES = {}
for _n in LENGTHS:
    for _k in range(2):
        CASES["n%d_%s" % (_n, "ab"[_k])] = dict(seed=1000 + 10 * _n + _k, n=_n, slow=False)
CASES["slow7"] = dict(seed=77, n=7, slow=True)
CASES["fast3"] = dict(seed=33, n=3, slow=False, fast=True)


def make_case(name):
    c = CASES[name]
    rng = np.random.default_rng(c["seed"])
    n = c["n"]
    bias = np.r_[rng.normal(0, 0.05, 3), rng.normal(0, 0.01, 3)].astype(np.float32)        # bax bay baz bwx bwy bwz
    g = np.array([0.3, -0.2, 9.79])
    a = (g + rng.normal(0, 1.5, (n, 3))).astype(np.float32)
    if c["slow"]:
        w = (bias[3:].astype(np.float64) + rng.normal(0, 0.003, (n, 3))).astype(np.float32)   # |w - b| dt < 1e-4 by a wide margin
    else:
        w = rng.normal(0, 80.0 if c.get("fast") else 0.4, (n, 3)).astype(np.float32)
    dt = np.full(n, DT, np.float32)
    # what the prediction starts from: a body pose and velocity, and a bias that moved since the pre-integration
    q = rng.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    x, y, z, s = q
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * s), 2 * (x * z + y * s)], [2 * (x * y + z * s), 1 - 2 * (x * x + z * z), 2 * (y * z - x * s)],
                  [2 * (x * z - y * s), 2 * (y * z + x * s), 1 - 2 * (x * x + y * y)]]).astype(np.float32)
    pred = dict(Rwb1=R, twb1=rng.normal(0, 2, 3).astype(np.float32), Vwb1=rng.normal(0, 1, 3).astype(np.float32),
                bias=(bias + np.r_[rng.normal(0, 0.05, 3), rng.normal(0, 0.005, 3)]).astype(np.float32))
    return dict(name=name, n=n, a=a, w=w, dt=dt, bias=bias, nga=NGA, nga_walk=NGA_WALK, pred=pred)


def cases_of_length(n):
    return [k for k, c in CASES.items() if c["n"] == n]


# ---- the reference results, computed once and shared by the tests (nobody writes to them) ----
_DATA = {}


def reference_data():
    """truth[name] / truth_pred[name]: the long-double blocks; errors[variant][name][block]: what each float32 variant misses truth
    by; budget[n][block]: the largest of those over the variants and the cases of length n; C32[name]: the float32 C as written"""
    if _DATA:
        return _DATA
    import imu_preint_reference as ref
    truth, truth_pred, C32 = {}, {}, {}
    errors = {v: {} for v in ref.VARIANTS}
    for name in CASES:
        c = make_case(name)
        t = ref.truth(c)
        truth[name] = ref.blocks(t)
        truth_pred[name] = ref.predict(t, T=np.longdouble, **c["pred"])
        for v, opt in ref.VARIANTS.items():
            s = ref.integrate(c, np.float32, **opt)
            p = ref.predict(s, T=np.float32, polar=opt["polar"], **c["pred"])
            b = ref.blocks(s)
            errors[v][name] = {k: ref.block_error(b[k], truth[name][k]) for k in ref.BLOCKS}
            errors[v][name].update({k: ref.block_error(p[k], truth_pred[name][k]) for k in ref.PREDICTED})
            if v == "as_written":
                C32[name] = s["C"].copy()
    budget = {n: {k: max(errors[v][name][k] for v in errors for name in cases_of_length(n)) for k in ref.BLOCKS + ref.PREDICTED} for n in LENGTHS}
    _DATA.update(truth=truth, truth_pred=truth_pred, errors=errors, budget=budget, C32=C32)
    return _DATA


def bound(budget):
    """what an implementation in float is held to: two float evaluations differ from each other by up to twice what each differs from
    truth, a factor two for operation order, and four units in the last place of a float"""
    return 4 * budget + 4 * 2.0 ** -24


def check_against_truth(name, got, keys, label="device"):
    """got[k] for k in keys (blocks of a state, or a prediction) against truth within the bound of the case's length; prints every figure"""
    import imu_preint_reference as ref
    d = reference_data()
    n = CASES[name]["n"]
    t = dict(d["truth"][name], **d["truth_pred"][name])
    bad = []
    for k in keys:
        e, lim = ref.block_error(got[k], t[k]), bound(d["budget"][n][k])
        print("%-8s %-6s %s %.2e  budget %.2e  bound %.2e" % (name, k, label, e, d["budget"][n][k], lim))
        if not e <= lim:
            bad.append((k, e, lim))
    assert not bad, "%s: %s" % (name, bad)


# ---- the cases as the arrays of the C ABI ----
def pack(capi, names, extra_states=0):
    """one job per case (reset with the case's bias, then all its measurements): (states, jobs, meas)"""
    cases = [make_case(n) for n in names]
    states = capi.imu_state_new(len(cases) + extra_states, NGA, NGA_WALK)
    jobs = np.zeros(len(cases), capi.IMU_JOB_DTYPE)
    ms, off = [], 0
    for i, c in enumerate(cases):
        jobs[i] = (i, off, c["n"], 1, c["bias"])
        m = np.zeros(c["n"], capi.IMU_MEAS_DTYPE)
        m["a"], m["w"], m["dt"] = c["a"], c["w"], c["dt"]
        ms.append(m)
        off += c["n"]
    return states, jobs, np.concatenate(ms)


def predict_jobs(capi, names):
    pj = np.zeros(len(names), capi.IMU_PREDICT_JOB_DTYPE)
    for i, n in enumerate(names):
        p = make_case(n)["pred"]
        pj[i] = (i, p["Rwb1"], p["twb1"], p["Vwb1"], p["bias"])
    return pj


def clamp_state(capi, state7):
    """the crafted state of the eigenvalue clamp: the n = 7 C9 with row and column 8 zeroed and C[8][8] = 1e13, so that the information
    has the eigenvalue 1e-13 < 1e-12 on the axis e8"""
    s = np.array(state7, capi.IMU_STATE_DTYPE)
    s["C"][8, :] = 0
    s["C"][:, 8] = 0
    s["C"][8, 8] = 1e13
    return s


def frame_streams():
    """sample streams for the interpolation loop: n_imu = 0, 1, 2, 3, 8 with int64 time stamps near 1.4e18 ns at about 200 Hz with
    jitter, the previous frame's time just after the first sample and this frame's just before the last"""
    rng = np.random.default_rng(5)
    out = []
    for n in (0, 1, 2, 3, 8):
        t0 = 1403636579763555584 + int(rng.integers(0, 10 ** 9))
        ts = t0 + np.cumsum(5_000_000 + rng.integers(-40_000, 40_000, max(n, 1))).astype(np.int64)
        ts = ts[:n]
        t_prev = int(ts[0]) + 1_234_567 if n else t0
        t_cur = int(ts[-1]) - 2_345_678 if n > 1 else t_prev + 50_000_000
        out.append(dict(ts=ts, gyro=rng.normal(0, 0.4, (n, 3)).astype(np.float32), acce=(np.array([0.3, -0.2, 9.79]) + rng.normal(0, 1.5, (n, 3))).astype(np.float32),
                        t_prev=t_prev, t_cur=t_cur))
    return out
