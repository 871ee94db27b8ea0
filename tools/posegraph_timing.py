"""Times essg_optimize (Optimizer::OptimizeEssentialGraph on the device) on 100, 500 and 1 000 key frames with about five edges
per key frame, against a single-threaded CPU restatement, and writes profiles/posegraph_timing.json.  Needs a GPU.

Device: wall time of one call (host arrays in and out), the HIP-event time of all its launches, and the call's split into
graph structure + upload / Levenberg rounds / epilogue + download (essg_last_device_ms).
CPU: tools/posegraph_cpu.cpp compiled here with g++ -O3 -ffp-contract=off (errors, numeric Jacobians and edge blocks from the same
C++ text the kernels compile), the Levenberg policy in Python, the linear solve SPARSE: scipy.sparse.linalg.splu (SuperLU) on the
assembled 7N x 7N matrix.  That is not the reference's solver (Eigen's SimplicialLDLT through g2o's LinearSolverEigen); it is the
sparse direct solver available here.  Both sides run the same number of iterations and trials (printed).

Exit status 1 unless the device call beats the CPU restatement at 500 key frames.

With the argument 4dof the same for essg_optimize_4dof (Optimizer::OptimizeEssentialGraph4DoF, the pose graph of an inertial map:
4N unknowns, lambda_0 computed from max diag H): it writes profiles/posegraph4dof_timing.json, and its exit status is 0 whoever wins."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]
try:
    import torch  # noqa: F401  (one HIP runtime per process: see tests/conftest.py)
except Exception:
    pass
import numpy as np  # noqa: E402
import scipy.sparse as sps  # noqa: E402
from scipy.sparse.linalg import splu  # noqa: E402


def build_cpu(tmp):
    so = os.path.join(tmp, "posegraph_cpu.so")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-o", so, os.path.join(ROOT, "tools", "posegraph_cpu.cpp")])
    lib = C.CDLL(so)
    lib.pg_linearize.restype = C.c_double
    lib.pg_linearize.argtypes = [C.c_int] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p]
    lib.pg_update_errors.restype = C.c_double
    lib.pg_update_errors.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
    lib.pg4_linearize.restype = C.c_double
    lib.pg4_linearize.argtypes = [C.c_int] + [C.c_void_p] * 7
    lib.pg4_update_errors.restype = C.c_double
    lib.pg4_update_errors.argtypes = [C.c_int, C.c_int] + [C.c_void_p] * 8
    return lib


def cpu_optimize_4dof(lib, pr):
    """the same loop for the 4-DoF graph: 4 x 4 blocks, the edges' information inside the records, lambda_0 = 1e-5 max diag H unless
    the problem sets one.  The final state comes back too (rcw_out, tcw_out)."""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    f8 = lambda k, w: np.ascontiguousarray(pr[k], np.float64).reshape(-1, w)
    nV = len(pr["fixed"])
    est = np.zeros((nV, 18))
    est[:, 0] = 1.0; est[:, 2:5] = f8("twb", 3); est[:, 6:15] = f8("rcw", 9); est[:, 15:18] = f8("tcw", 3)
    konst = np.ascontiguousarray(np.concatenate([f8("rwb", 9), f8("rcb", 9), f8("tcb", 3)], 1))
    meas = np.ascontiguousarray(np.concatenate([f8("edge_rot", 9), f8("edge_trans", 3)], 1))
    W = np.ascontiguousarray(pr["information"], np.float64).reshape(36)
    ev, fixed = np.ascontiguousarray(pr["edge_vertices"], np.int32), np.ascontiguousarray(pr["fixed"], np.uint8)
    nE = len(ev)
    col = np.where(fixed == 0, np.cumsum(fixed == 0) - 1, -1).astype(np.int32)
    nf = int((fixed == 0).sum())
    ci, cj = col[ev[:, 0]], col[ev[:, 1]]
    r4, c4 = np.divmod(np.arange(16), 4)
    rows, cols, src = [], [], []
    for (a, b, off, mask, tr) in ((ci, ci, 0, ci >= 0, False), (cj, cj, 32, cj >= 0, False), (ci, cj, 16, (ci >= 0) & (cj >= 0), False), (cj, ci, 16, (ci >= 0) & (cj >= 0), True)):
        e = np.flatnonzero(mask)
        rows.append((4 * a[e][:, None] + (c4 if tr else r4)).ravel()); cols.append((4 * b[e][:, None] + (r4 if tr else c4)).ravel())
        src.append((57 * e[:, None] + off + np.arange(16)).ravel())
    rows, cols, src = np.concatenate(rows), np.concatenate(cols), np.concatenate(src)
    rec = np.zeros((nE, 57))
    trial = np.zeros_like(est)
    lam, ni, n_bad, iters, trials = float(pr["lambda_init"]), 2.0, 0, 0, 0
    t_lin = t_solve = t_upd = 0.0
    eye = sps.identity(4 * nf, format="csc")
    cur = None
    for it in range(int(pr["max_iters"])):
        t0 = time.perf_counter()
        cur = ini = lib.pg4_linearize(nE, p(meas), p(W), p(ev), p(est), p(konst), p(fixed), p(rec))
        t_lin += time.perf_counter() - t0
        flat = rec.ravel()
        b = np.zeros(4 * nf)
        for (a, off) in ((ci, 48), (cj, 52)):
            e = np.flatnonzero(a >= 0)
            np.add.at(b, (4 * a[e][:, None] + np.arange(4)).ravel(), rec[e, off:off + 4].ravel())
        rho, qmax = 0.0, 0
        while True:
            t0 = time.perf_counter()
            H = sps.csc_matrix((flat[src], (rows, cols)), shape=(4 * nf, 4 * nf))
            if it == 0 and qmax == 0 and not lam > 0:
                lam = 1e-5 * float(np.abs(H.diagonal()).max())
            x = splu((H + lam * eye).tocsc()).solve(b)
            t_solve += time.perf_counter() - t0
            t0 = time.perf_counter()
            chi_new = lib.pg4_update_errors(nV, nE, p(meas), p(W), p(ev), p(est), p(konst), p(col), p(x), p(trial))
            t_upd += time.perf_counter() - t0
            rho = (cur - chi_new) / (float(x @ (lam * x + b)) + 1e-3)
            if rho > 0 and np.isfinite(chi_new):
                lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3)); ni = 2.0; cur = chi_new; est, trial = trial, est
            else:
                lam *= ni; ni *= 2
            qmax += 1; trials += 1
            if not (rho < 0 and qmax < 10):
                break
        iters += 1
        if qmax == 10 or rho == 0:
            break
        n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    return dict(iterations=iters, trials=trials, chi2_final=cur, linearize_ms=1e3 * t_lin, solve_ms=1e3 * t_solve, update_ms=1e3 * t_upd), \
        est[:, 6:15].reshape(-1, 3, 3).copy(), est[:, 15:18].copy()


def cpu_optimize(lib, pr):
    """the reference's loop (optimization_algorithm_levenberg.cpp:61-169) around the C++ edge work and a sparse LU"""
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    est = np.ascontiguousarray(pr["sim3"], np.float64).copy()
    meas, ev, fixed = np.ascontiguousarray(pr["edge_measurement"]), np.ascontiguousarray(pr["edge_vertices"], np.int32), np.ascontiguousarray(pr["fixed"], np.uint8)
    nV, nE, fs = len(est), len(ev), int(pr["fix_scale"])
    col = np.where(fixed == 0, np.cumsum(fixed == 0) - 1, -1).astype(np.int32)
    nf = int((fixed == 0).sum())
    ci, cj = col[ev[:, 0]], col[ev[:, 1]]
    r7, c7 = np.divmod(np.arange(49), 7)
    rows, cols, src = [], [], []
    for (a, b, off, mask, tr) in ((ci, ci, 0, ci >= 0, False), (cj, cj, 98, cj >= 0, False), (ci, cj, 49, (ci >= 0) & (cj >= 0), False), (cj, ci, 49, (ci >= 0) & (cj >= 0), True)):
        e = np.flatnonzero(mask)
        rows.append((7 * a[e][:, None] + (c7 if tr else r7)).ravel()); cols.append((7 * b[e][:, None] + (r7 if tr else c7)).ravel())
        src.append((162 * e[:, None] + off + np.arange(49)).ravel())
    rows, cols, src = np.concatenate(rows), np.concatenate(cols), np.concatenate(src)
    rec = np.zeros((nE, 162))
    trial = np.zeros_like(est)
    lam, ni, n_bad, iters, trials = float(pr["lambda_init"]), 2.0, 0, 0, 0
    t_lin = t_solve = t_upd = 0.0
    eye = sps.identity(7 * nf, format="csc")
    for it in range(int(pr["max_iters"])):
        t0 = time.perf_counter()
        cur = ini = lib.pg_linearize(nE, p(meas), p(ev), p(est), p(fixed), fs, p(rec))
        t_lin += time.perf_counter() - t0
        flat = rec.ravel()
        b = np.zeros(7 * nf)
        for (a, off) in ((ci, 147), (cj, 154)):
            e = np.flatnonzero(a >= 0)
            np.add.at(b, (7 * a[e][:, None] + np.arange(7)).ravel(), rec[e, off:off + 7].ravel())
        rho, qmax = 0.0, 0
        while True:
            t0 = time.perf_counter()
            H = sps.csc_matrix((flat[src], (rows, cols)), shape=(7 * nf, 7 * nf))
            x = splu((H + lam * eye).tocsc()).solve(b)
            t_solve += time.perf_counter() - t0
            t0 = time.perf_counter()
            chi_new = lib.pg_update_errors(nV, nE, p(meas), p(ev), p(est), p(col), p(x), fs, p(trial))
            t_upd += time.perf_counter() - t0
            rho = (cur - chi_new) / (float(x @ (lam * x + b)) + 1e-3)
            if rho > 0 and np.isfinite(chi_new):
                lam *= max(1 / 3, min(1 - (2 * rho - 1) ** 3, 2 / 3)); ni = 2.0; cur = chi_new; est, trial = trial, est
            else:
                lam *= ni; ni *= 2
            qmax += 1; trials += 1
            if not (rho < 0 and qmax < 10):
                break
        iters += 1
        if qmax == 10 or rho == 0:
            break
        n_bad = n_bad + 1 if (ini - cur) * 1e3 < ini else 0
        if n_bad >= 3:
            break
    return dict(iterations=iters, trials=trials, chi2_final=cur, linearize_ms=1e3 * t_lin, solve_ms=1e3 * t_solve, update_ms=1e3 * t_upd)


def main_4dof():
    pkg = importlib.import_module("orb_slam3-1_amd")
    sp = importlib.import_module("orb_slam3-1_amd.synth_posegraph")
    out = dict(cpu="single-threaded C++ restatement (tools/posegraph_cpu.cpp, g++ -O3 -ffp-contract=off) with numeric Jacobians; linear solve "
                   "scipy.sparse.linalg.splu (SuperLU) on the assembled matrix -- NOT Eigen's SimplicialLDLT, which the reference uses",
               sizes={})
    g = pkg.EssentialGraph()
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_cpu(tmp)
        for n in (100, 500, 1000):
            pr = sp.make_posegraph4dof(1, n=n, n_points=4 * n)
            g.optimize_4dof(pr)                                      # allocation and first-launch costs stay out of the timing
            calls = []
            for _ in range(3):
                t0 = time.perf_counter(); d = g.optimize_4dof(pr); wall = 1e3 * (time.perf_counter() - t0)
                ms, stages = g.last_device_ms()
                calls.append(dict(call_ms=wall, device_event_ms=ms, **stages))
            best = min(calls, key=lambda c: c["call_ms"])
            t0 = time.perf_counter(); c, rcw, tcw = cpu_optimize_4dof(lib, pr); cpu_ms = 1e3 * (time.perf_counter() - t0)
            out["sizes"][str(n)] = dict(key_frames=n, edges=int(len(pr["edge_vertices"])), unknowns=4 * int((pr["fixed"] == 0).sum()),
                                        device=dict(best, iterations=d["stats"]["iterations"], trials=d["stats"]["trials"], chi2_final=d["stats"]["chi2_final"]),
                                        cpu=dict(c, call_ms=cpu_ms), speedup=cpu_ms / best["call_ms"],
                                        largest_difference=dict(rcw=float(np.abs(rcw - d["rcw_out"]).max()), tcw=float(np.abs(tcw - d["tcw_out"]).max())))
            print(n, json.dumps(out["sizes"][str(n)]), flush=True)
    g.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "posegraph4dof_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    return 0


def main():
    pkg = importlib.import_module("orb_slam3-1_amd")
    sp = importlib.import_module("orb_slam3-1_amd.synth_posegraph")
    out = dict(cpu="single-threaded C++ restatement (tools/posegraph_cpu.cpp, g++ -O3 -ffp-contract=off) with numeric Jacobians; linear solve "
                   "scipy.sparse.linalg.splu (SuperLU) on the assembled matrix -- NOT Eigen's SimplicialLDLT, which the reference uses",
               sizes={})
    g = pkg.EssentialGraph()
    with tempfile.TemporaryDirectory() as tmp:
        lib = build_cpu(tmp)
        for n in (100, 500, 1000):
            pr = sp.make_posegraph(1, n=n, fix_scale=True, n_points=4 * n)
            g.optimize(pr)                                           # allocation and first-launch costs stay out of the timing
            calls = []
            for _ in range(3):
                t0 = time.perf_counter(); d = g.optimize(pr); wall = 1e3 * (time.perf_counter() - t0)
                ms, stages = g.last_device_ms()
                calls.append(dict(call_ms=wall, device_event_ms=ms, **stages))
            best = min(calls, key=lambda c: c["call_ms"])
            t0 = time.perf_counter(); c = cpu_optimize(lib, pr); cpu_ms = 1e3 * (time.perf_counter() - t0)
            out["sizes"][str(n)] = dict(key_frames=n, edges=int(len(pr["edge_vertices"])), unknowns=7 * int((pr["fixed"] == 0).sum()),
                                        device=dict(best, iterations=d["stats"]["iterations"], trials=d["stats"]["trials"], chi2_final=d["stats"]["chi2_final"]),
                                        cpu=dict(c, call_ms=cpu_ms), speedup=cpu_ms / best["call_ms"])
            print(n, json.dumps(out["sizes"][str(n)]), flush=True)
    g.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "posegraph_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    return 0 if out["sizes"]["500"]["speedup"] > 1.0 else 1


if __name__ == "__main__":
    sys.exit(main_4dof() if sys.argv[1:] == ["4dof"] else main())
