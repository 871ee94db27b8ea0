#!/usr/bin/env python3
"""Times imu_init_optimize_batch (the three Optimizer::InertialOptimization overloads on the device) against a single-threaded CPU
restatement and writes profiles/imuinit_timing.json.  Needs a GPU.

    python tools/imuinit_timing.py

Three settings, each the full monocular first-stage problem (priors 1e2 / 1e10, lambda_0 = 1e3, up to 200 iterations) of
synth_imuinit.make_imu_init: one problem of 10 key frames, one of 100, and 64 problems of 20 key frames in one call.
Device: host arrays in, host arrays out, wall time of the call (staging, one launch, the copy back), best of three after a warm-up
call; the HIP-event time of the launch beside it.
CPU: tools/imuinit_cpu.cpp compiled here with g++ -O3 -ffp-contract=off -- the same per-link text the kernel compiles and the same
structured solve, one loop where the kernel has a workgroup; the 64 problems one after the other on one thread.  It is not g2o:
BlockSolverX with LinearSolverEigen allocates its sparse structure per call and factors it without knowing that it is a bordered
chain, so the reference itself is slower than this restatement.
No threshold is asserted and the exit status is 0 whoever wins: one problem alone is a serial chain of dependent f64 operations."""
import ctypes as C
import importlib
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def build_cpu(tmp):
    so = os.path.join(tmp, "imuinit_cpu.so")
    subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", "-shared", "-fPIC", "-o", so,
                           os.path.join(ROOT, "tools", "imuinit_cpu.cpp")])
    return so


def best_of(f, n=3):
    f()                                     # warm-up
    best = float("inf")
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return 1e3 * best


def main():
    pkg = importlib.import_module("orb_slam3-1_amd")
    capi = importlib.import_module("orb_slam3-1_amd.capi")
    sy = importlib.import_module("orb_slam3-1_amd.synth_imuinit")
    settings = dict(one_problem_10_key_frames=[sy.make_imu_init(110, 10)[0]],
                    one_problem_100_key_frames=[sy.make_imu_init(1100, 100)[0]],
                    batch_64_problems_of_20_key_frames=[sy.make_imu_init(2000 + i, 20)[0] for i in range(64)])
    out = dict(cpu="single-threaded C++ restatement (tools/imuinit_cpu.cpp, g++ -O3 -ffp-contract=off): the kernel's per-link text and "
                   "structured solve in one loop; a batch runs its problems one after the other", unit="ms, best of 3 after a warm-up", settings={})
    solver = pkg.ImuInit()
    with tempfile.TemporaryDirectory() as tmp:
        cpu = C.CDLL(build_cpu(tmp))
        cpu.imuinit_cpu_optimize.argtypes = [C.POINTER(capi.ImuInitProblem), C.POINTER(capi.ImuInitResult)]
        for name, problems in settings.items():
            n = len(problems)
            dev_prep, cpu_prep = capi.imu_init_prepare(problems), capi.imu_init_prepare(problems)

            def run_device():
                rc = capi.lib.imu_init_optimize_batch(solver._h, dev_prep["problems"], n, dev_prep["results"])
                assert rc == 0, capi.lib.orbx_last_error()

            def run_cpu():
                for i in range(n):
                    assert cpu.imuinit_cpu_optimize(C.byref(cpu_prep["problems"][i]), C.byref(cpu_prep["results"][i])) == 0

            t_dev = best_of(run_device)
            t_kernel = solver.last_device_ms()
            t_cpu = best_of(run_cpu)
            d, c = capi.imu_init_results(dev_prep), capi.imu_init_results(cpu_prep)
            flows = [(r["stats"]["iterations"], r["stats"]["trials"], r["stats"]["stop_reason"]) for r in d]
            agree = max(float(np.abs(a["vel"] - b["vel"]).max()) for a, b in zip(d, c))
            out["settings"][name] = dict(problems=n, key_frames=len(problems[0]["vel"]), device_call_ms=round(t_dev, 4), device_kernel_ms=round(t_kernel, 4),
                                         cpu_ms=round(t_cpu, 4), cpu_over_device=round(t_cpu / t_dev, 3), iterations=[f[0] for f in flows],
                                         trials=[f[1] for f in flows], largest_velocity_difference_device_cpu=agree)
            print(name, json.dumps(out["settings"][name]), flush=True)
    solver.close()
    with open(os.path.join(ROOT, "profiles", "imuinit_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
