"""include/orbslam3_shim_loop.hpp (Sim3SolverHIP, OptimizeSim3HIP) against the stand-ins of tests/stubs/: it compiles against
them unchanged (no GPU), and on a toy pair of key frames its glue -- which matches become correspondences (src/Sim3Solver.cc:73-91)
or edge pairs (src/Optimizer.cc:2167-2304), the iterate() bookkeeping, the write-back -- gives what the C ABI gives on the
flattened inputs (GPU).  Glue, not numerics: neither an oracle nor a build of the reference.  The toy driver turns the zero
fill of the stand-in's default-constructed matrices into NaN (Eigen leaves them uninitialised), so every matrix the adapters
return must have been written coefficient by coefficient.  """
import importlib
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "orb_slam3-1_amd")


def test_loop_shim_compiles_against_standins(tmp_path):
    """the header alone: the reference fallbacks (Sim3Solver, Optimizer::OptimizeSim3, absent from the stand-ins) sit in
    dependent contexts and are not instantiated"""
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "orbslam3_shim_loop.hpp"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    src.write_text('#include "orbslam3_shim_loop.hpp"\nint main() { return 0; }\n')       # without the macro: the POD half only
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory, pkg):
    exe = tmp_path_factory.mktemp("shim_loop") / "shim_loop_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_loop_toy.cpp"),
                           "-o", str(exe), "-L", LIBDIR, "-lorbslam3_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_loop_toy_builds_and_instantiates_the_adapters(toy):
    r = subprocess.run([toy], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr


# ---- the toy case ----
F32 = np.float32


def _rot_f32(q):
    """Eigen::Quaternionf::toRotationMatrix as the stand-in computes it, in float; q = (x, y, z, w)"""
    x, y, z, w = (F32(v) for v in q)
    two, one = F32(2), F32(1)
    return np.array([[one - two * (y * y + z * z), two * (x * y - z * w), two * (x * z + y * w)],
                     [two * (x * y + z * w), one - two * (x * x + z * z), two * (y * z - x * w)],
                     [two * (x * z - y * w), two * (y * z + x * w), one - two * (x * x + y * y)]], F32)


def _to_camera(R, t, X):
    """R * X + t in float, products summed in order"""
    X = X.astype(F32)
    out = np.zeros_like(X)
    for r in range(3):
        out[:, r] = ((F32(0) + R[r, 0] * X[:, 0]) + R[r, 1] * X[:, 1]) + R[r, 2] * X[:, 2] + F32(t[r])
    return out


def _make_case(seed, n1=90, fix_scale=0, min_inliers=12, max_its=300, all_points=0, inlier=0.7):
    synth = importlib.import_module("orb_slam3-1_amd.synth")
    rs = np.random.RandomState(seed)
    K1, K2 = [458.654, 457.296, 367.215, 248.375], [435.2047, 435.2047, 367.4517, 252.2008]
    q1 = synth._quat_from_R(synth._rodrigues(rs.normal(0, 0.2, 3))).astype(F32)
    q2 = synth._quat_from_R(synth._rodrigues(rs.normal(0, 0.2, 3))).astype(F32)
    t1, t2 = rs.normal(0, 0.5, 3).astype(F32), rs.normal(0, 0.5, 3).astype(F32)
    R1, R2 = _rot_f32(q1).astype(np.float64), _rot_f32(q2).astype(np.float64)
    # the two maps differ by a similarity: camera-frame points X1 = s R X2 + t
    X1c = np.stack([rs.uniform(-3, 3, n1), rs.uniform(-2, 2, n1), rs.uniform(2, 10, n1)], 1)
    Rs = synth._rodrigues(rs.normal(0, 0.1, 3))
    s = 1.0 if fix_scale else 1.15
    ts = rs.uniform(-0.3, 0.3, 3)
    X2c = ((X1c - ts) @ Rs) / s
    out = rs.uniform(size=n1) > inlier
    X2c[out] = np.stack([rs.uniform(-3, 3, out.sum()), rs.uniform(-2, 2, out.sum()), rs.uniform(2, 10, out.sum())], 1)
    X1w = ((X1c - t1) @ R1).astype(F32)
    X2w = ((X2c - t2) @ R2).astype(F32)
    sig2 = (1.2 ** (2 * np.arange(8))).astype(F32)
    oct1, oct2, lvl2 = rs.randint(0, 8, n1), rs.randint(0, 8, n1), rs.randint(0, 8, n1)
    flags = dict(has_match=rs.uniform(size=n1) < 0.9, has1=rs.uniform(size=n1) < 0.93, bad1=rs.uniform(size=n1) < 0.05,
                 obs1=rs.uniform(size=n1) < 0.95, bad2=rs.uniform(size=n1) < 0.05, in2=rs.uniform(size=n1) < 0.85)
    perm = rs.permutation(n1 + 7)[:n1]                  # feature index in key frame 2
    i2 = np.where(flags["in2"], perm, -1)
    kp1 = np.stack([K1[0] * X1c[:, 0] / X1c[:, 2] + K1[2], K1[1] * X1c[:, 1] / X1c[:, 2] + K1[3]], 1) + rs.normal(0, 0.7, (n1, 2))
    kp2 = np.stack([K2[0] * X2c[:, 0] / X2c[:, 2] + K2[2], K2[1] * X2c[:, 1] / X2c[:, 2] + K2[3]], 1) + rs.normal(0, 0.7, (n1, 2))
    dR = synth._rodrigues(rs.normal(0, 0.01, 3))
    S0 = dict(q=synth._quat_from_R(dR @ Rs), t=ts + rs.normal(0, 0.01, 3), s=s if fix_scale else s * 1.01)
    return dict(n1=n1, n2=n1 + 7, K1=K1, K2=K2, q1=q1, q2=q2, t1=t1, t2=t2, X1w=X1w, X2w=X2w, sig2=sig2, inv_sig2=(F32(1) / sig2).astype(F32),
                oct1=oct1, oct2=oct2, lvl2=lvl2, i2=i2, kp1=kp1.astype(F32), kp2=kp2.astype(F32), S0=S0, fix_scale=fix_scale,
                min_inliers=min_inliers, max_its=max_its, seed=424242 + seed, all_points=all_points, th2=10.0, **flags)


def _write_case(c, path):
    with open(path, "w") as f:
        f.write("%d %d %d %d %d %r\n" % (c["fix_scale"], c["min_inliers"], c["max_its"], c["seed"], c["all_points"], c["th2"]))
        f.write(" ".join(repr(float(v)) for v in list(c["S0"]["q"]) + list(c["S0"]["t"]) + [c["S0"]["s"]]) + "\n")
        for kid, K, q, t in ((7, c["K1"], c["q1"], c["t1"]), (19, c["K2"], c["q2"], c["t2"])):
            f.write("%d " % kid + " ".join(repr(float(F32(v))) for v in list(K) + list(q) + list(t)) + "\n")
            f.write(" ".join(repr(float(v)) for v in c["sig2"]) + "\n" + " ".join(repr(float(v)) for v in c["inv_sig2"]) + "\n")
        f.write("%d %d\n" % (c["n1"], c["n2"]))
        for i in range(c["n1"]):
            f.write("%d %d %d %d %d %d " % (c["has_match"][i], c["has1"][i], c["bad1"][i], c["obs1"][i], c["bad2"][i], c["i2"][i]))
            f.write(" ".join(repr(float(v)) for v in list(c["X1w"][i]) + list(c["X2w"][i])))
            f.write(" %r %r %d %r %r %d %d\n" % (float(c["kp1"][i, 0]), float(c["kp1"][i, 1]), c["oct1"][i], float(c["kp2"][i, 0]), float(c["kp2"][i, 1]),
                                                c["oct2"][i], c["lvl2"][i]))


def _parse(out):
    d = {}
    for line in out.strip().splitlines():
        tok = line.split()
        if tok[0] in ("indices1", "X1c", "X2c", "max_err1", "max_err2", "T", "R", "ts", "inliers", "Tfind", "S12", "null_after", "null_before"):
            d[tok[0]] = np.array([float.fromhex(v) for v in tok[2:]])
            assert len(d[tok[0]]) == int(tok[1])
        else:
            for k, v in zip(tok[0::2], tok[1::2]):
                d[k] = float(v)
    return d


def _run(toy, mode, case, tmp_path):
    path = str(tmp_path / ("%s.txt" % mode))
    _write_case(case, path)
    r = subprocess.run(["timeout", "-k", "10", "120", toy, mode, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return _parse(r.stdout)


@pytest.mark.gpu
@pytest.mark.parametrize("seed,fix_scale,min_inliers,inlier", [(1, 0, 12, 0.7), (2, 1, 12, 0.7), (3, 0, 45, 0.5), (4, 0, 200, 0.7)])
def test_sim3_solver_adapter_equals_c_abi(toy, pkg, tmp_path, seed, fix_scale, min_inliers, inlier):
    c = _make_case(seed, fix_scale=fix_scale, min_inliers=min_inliers, inlier=inlier)
    d = _run(toy, "ransac", c, tmp_path)
    # which matches become correspondences (:73-91): match present, point 1 present, neither bad, both observed in their key frames
    want = [i for i in range(c["n1"]) if c["has_match"][i] and c["has1"][i] and not c["bad1"][i] and not c["bad2"][i] and c["obs1"][i] and c["i2"][i] >= 0]
    idx = d["indices1"].astype(int)
    assert idx.tolist() == want and int(d["N"]) == len(want) and 0 < len(want) < c["n1"]
    X1 = _to_camera(_rot_f32(c["q1"]), c["t1"], c["X1w"][idx])
    X2 = _to_camera(_rot_f32(c["q2"]), c["t2"], c["X2w"][idx])
    assert np.allclose(d["X1c"].reshape(-1, 3), X1, rtol=1e-5, atol=1e-5) and np.allclose(d["X2c"].reshape(-1, 3), X2, rtol=1e-5, atol=1e-5)
    assert np.array_equal(d["max_err1"], np.floor(9.210 * c["sig2"][c["oct1"][idx]].astype(np.float64)))      # the vector<size_t> truncation
    assert np.array_equal(d["max_err2"], np.floor(9.210 * c["sig2"][c["oct2"][idx]].astype(np.float64)))
    assert d["reseed_same"] == 1                        # SetSeed() after a walk starts it over
    assert np.isfinite(d["T"]).all() and np.isfinite(d["Tfind"]).all() and np.isfinite(d["R"]).all() and np.isfinite(d["ts"]).all()
    # SetRansacParameters (:123-147)
    N, H = len(want), int(d["H"])
    if min_inliers == N:
        expect_H = 1
    else:
        eps = float(F32(min_inliers) / F32(N))
        with np.errstate(all="ignore"):
            it = np.ceil(np.log(1 - 0.99) / np.log(1 - eps ** 3))
        expect_H = max(1, min(int(it), c["max_its"])) if np.isfinite(it) else c["max_its"]
    assert H == expect_H
    if N < min_inliers:
        assert (d["converge"], d["nomore"], d["ninliers"], d["calls"]) == (0, 1, 0, 1) and not d["inliers"].any()
        assert np.array_equal(d["T"].reshape(4, 4), np.eye(4))
        return
    prob = dict(X1c=d["X1c"].astype(F32), X2c=d["X2c"].astype(F32), max_err1=d["max_err1"].astype(F32), max_err2=d["max_err2"].astype(F32),
                K1=np.array(c["K1"], F32), K2=np.array(c["K2"], F32), fix_scale=fix_scale, min_inliers=min_inliers,
                triples=pkg.sim3_draw_triples(c["seed"], N, H))
    s = pkg.Sim3Solver()
    r = s.ransac(prob)
    s.close()
    assert r["scored"] == 1 and (int(d["converge"]), int(d["nomore"])) == ((1, 0) if r["converged"] else (0, 1))
    h = r["index"]
    T = np.eye(4, dtype=F32)
    T[:3, :3] = r["T12"][h, 12] * r["T12"][h, :9].reshape(3, 3)
    T[:3, 3] = r["T12"][h, 9:12]
    assert np.array_equal(d["T"].reshape(4, 4).astype(F32), T)
    assert np.array_equal(d["R"].astype(F32), r["T12"][h, :9]) and np.array_equal(d["ts"].astype(F32), r["T12"][h, 9:13])
    sim3_ref = importlib.import_module("sim3_reference")
    bits = sim3_ref.unpack_mask(r["mask"], N)[h]
    if r["converged"]:
        expect = np.zeros(c["n1"], bool)
        expect[idx[bits]] = True                        # vbInliers is indexed by mvnIndices1 (:204-206)
        assert np.array_equal(d["inliers"].astype(bool), expect) and int(d["ninliers"]) == int(r["count"][h]) == int(bits.sum())
        assert int(d["calls"]) == h // 20 + 1           # iterate(20, ...) walks twenty hypotheses per call
        assert np.array_equal(d["Tfind"].reshape(4, 4).astype(F32), T) and int(d["find_ninliers"]) == int(r["count"][h])
    else:
        assert int(d["nomore"]) == 1 and not d["inliers"].any() and int(d["ninliers"]) == 0
        assert int(d["calls"]) == (H + 19) // 20
        assert np.array_equal(d["Tfind"].reshape(4, 4), np.eye(4))          # the 4-argument iterate returns Identity (:215)


def _flatten_opt(c):
    """Optimizer::OptimizeSim3's graph (:2167-2304) from the case, independently of the adapter"""
    R1, R2 = _rot_f32(c["q1"]), _rot_f32(c["q2"])
    X1 = _to_camera(R1, c["t1"], c["X1w"])
    X2 = _to_camera(R2, c["t2"], c["X2w"])
    rows = []
    for i in range(c["n1"]):
        if not c["has_match"][i] or not c["has1"][i] or c["bad1"][i] or c["bad2"][i]:
            continue
        if c["i2"][i] < 0 and not c["all_points"]:
            continue
        if X2[i, 2] < 0:
            continue
        rows.append(i)
    rows = np.array(rows)
    o2 = c["kp2"][rows].astype(np.float64)
    w2 = c["inv_sig2"][c["oct2"][rows]].astype(np.float64)
    un = c["i2"][rows] < 0
    invz = F32(1) / X2[rows, 2]
    o2[un] = np.stack([X2[rows, 0] * invz, X2[rows, 1] * invz], 1)[un].astype(np.float64)
    w2[un] = c["inv_sig2"][c["lvl2"][rows]].astype(np.float64)[un]
    return rows, dict(q=c["S0"]["q"], t=c["S0"]["t"], s=c["S0"]["s"], X1c=X1[rows].astype(np.float64), X2c=X2[rows].astype(np.float64),
                      obs1=c["kp1"][rows].astype(np.float64), obs2=o2, inv_sigma2_1=c["inv_sig2"][c["oct1"][rows]].astype(np.float64), inv_sigma2_2=w2,
                      K1=np.array(c["K1"], F32).astype(np.float64), K2=np.array(c["K2"], F32).astype(np.float64), th2=10.0,
                      huber_delta=float(np.sqrt(F32(10.0))), fix_scale=c["fix_scale"])


@pytest.mark.gpu
@pytest.mark.parametrize("seed,fix_scale,all_points,n1", [(5, 0, 0, 90), (6, 1, 1, 90), (7, 0, 1, 14)])
def test_optimize_sim3_adapter_equals_c_abi(toy, pkg, tmp_path, seed, fix_scale, all_points, n1):
    c = _make_case(seed, n1=n1, fix_scale=fix_scale, all_points=all_points, inlier=0.8)
    d = _run(toy, "opt", c, tmp_path)
    rows, prob = _flatten_opt(c)
    s = pkg.Sim3Solver()
    r = s.optimize(prob)
    s.close()
    before, after = d["null_before"].astype(bool), d["null_after"].astype(bool)
    assert np.array_equal(before, ~np.asarray(c["has_match"]))
    dropped = np.zeros(c["n1"], bool)
    dropped[rows[~r["keep"]]] = True
    assert np.array_equal(after, before | dropped)      # exactly the entries the C entry reports as dropped are nulled
    if len(rows) - r["n_bad"] < 10:
        assert int(d["ret"]) == 0 and d["hessian_sum"] == 3.0 * 49                  # returns before mAcumHessian is touched (:2348-2356)
        assert np.allclose(d["S12"], list(c["S0"]["q"]) + list(c["S0"]["t"]) + [c["S0"]["s"]], rtol=0, atol=1e-15)
        return
    assert int(d["ret"]) == r["n_in"] > 10 and d["hessian_sum"] == 0.0
    assert np.allclose(d["S12"], list(r["q"]) + list(r["t"]) + [r["s"]], rtol=1e-6, atol=1e-7)
    if all_points:
        assert (c["i2"][rows] < 0).any()                # the case does hold unobserved points


def test_non_pinhole_cameras_reach_the_reference(toy, tmp_path):
    """no device needed: the fallback is taken before any device call"""
    c = _make_case(8)
    d = _run(toy, "fallback", c, tmp_path)
    assert d["uses_reference"] == 1 and d["solver_calls"] >= 2 and d["opt_calls"] == 1 and d["ret"] == -7 and d["scale"] == -1
