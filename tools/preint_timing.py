#!/usr/bin/env python3
"""Times IMU pre-integration on the device (imu_preintegrate_batch, imu_links_batch) against one host core and writes
profiles/preint_timing.json.  Needs a GPU.

    python tools/preint_timing.py

Sizes: 256 streams x 2 accumulators x 7 measurements (Tracking::PreintegrateIMU of a server with 256 clients: per stream one job
that resets and one that continues, over the same measurements); 256 and 4096 states x 20 measurements (Reintegrate() for every key
frame of a map); 4096 links; one job of 20 measurements alone.  `scaling` is the launch alone (HIP events) over the number of jobs at
20 measurements each: with a lane per job it is the length of ONE job's serial chain until the device runs out of SIMDs.
Device: host arrays in, host arrays out, wall time of the call (staging, one launch, the copy back), best of three after a warm-up
call; the HIP-event time of the launch beside it.
CPU: tools/preint_cpu.cpp compiled here with g++ -O3 -ffp-contract=off -- csrc/imu_preint_math.h, the very functions the kernels run
one lane each, in a plain loop on one thread.  It is not the reference: Eigen's dense 9 x 9 products and a JacobiSVD per measurement
make IMU::Preintegrated slower than this restatement.
No threshold is asserted and the exit status is 0 whoever wins: one job alone is a serial chain of dependent operations."""
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
NGA = np.array([5.78e-6] * 3 + [8e-4] * 3, np.float32)
NGA_WALK = np.array([1.88e-12] * 3 + [4.5e-8] * 3, np.float32)


def best_of(f, n=3):
    f()                                     # warm-up
    best = float("inf")
    for _ in range(n):
        t0 = time.perf_counter()
        f()
        best = min(best, time.perf_counter() - t0)
    return 1e3 * best


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def make_meas(capi, rng, n):
    m = np.zeros(n, capi.IMU_MEAS_DTYPE)
    m["a"] = np.array([0.3, -0.2, 9.79]) + rng.normal(0, 1.5, (n, 3))
    m["w"] = rng.normal(0, 0.4, (n, 3))
    m["dt"] = 0.005
    return m


def reintegrate_jobs(capi, rng, n_states, per):
    jobs = np.zeros(n_states, capi.IMU_JOB_DTYPE)
    jobs["state"], jobs["first"], jobs["count"], jobs["reset"] = np.arange(n_states), np.arange(n_states) * per, per, 1
    jobs["bias"] = rng.normal(0, 0.02, (n_states, 6))
    return capi.imu_state_new(n_states, NGA, NGA_WALK), jobs, make_meas(capi, rng, n_states * per)


def frame_jobs(capi, rng, streams, per):
    states = capi.imu_state_new(2 * streams, NGA, NGA_WALK)
    jobs = np.zeros(2 * streams, capi.IMU_JOB_DTYPE)
    jobs["state"] = np.arange(2 * streams)
    jobs["first"] = np.repeat(np.arange(streams) * per, 2)
    jobs["count"] = per
    jobs["reset"] = np.tile([0, 1], streams)                # since the last key frame: continuing; since the last frame: starts here
    jobs["bias"] = rng.normal(0, 0.02, (2 * streams, 6))
    return states, jobs, make_meas(capi, rng, streams * per)


def main():
    pkg = importlib.import_module("orb_slam3-1_amd")
    capi = importlib.import_module("orb_slam3-1_amd.capi")
    rng = np.random.default_rng(1)
    pre = pkg.ImuPreintegrator()
    out = dict(cpu="one host core (tools/preint_cpu.cpp, g++ -O3 -ffp-contract=off): the functions of csrc/imu_preint_math.h that the kernels run one lane each, in a plain loop",
               unit="ms, best of 3 after a warm-up", settings={}, scaling=[])
    settings = dict(frame_256_streams_2_states_7_measurements=frame_jobs(capi, rng, 256, 7),
                    reintegrate_256_states_20_measurements=reintegrate_jobs(capi, rng, 256, 20),
                    reintegrate_4096_states_20_measurements=reintegrate_jobs(capi, rng, 4096, 20),
                    one_job_20_measurements=reintegrate_jobs(capi, rng, 1, 20))
    with tempfile.TemporaryDirectory() as tmp:
        so = os.path.join(tmp, "libpreint_cpu.so")
        subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", so,
                               os.path.join(ROOT, "tools", "preint_cpu.cpp")])
        cpu = C.CDLL(so)
        last = None
        for name, (states, jobs, meas) in settings.items():
            d_states, c_states = states.copy(), states.copy()
            st = np.zeros(len(jobs), np.int32)

            def run_device():
                d_states[:] = states
                assert not pre.preintegrate(d_states, jobs, meas).any()

            def run_cpu():
                c_states[:] = states
                cpu.preint_cpu_preintegrate(_p(c_states), len(c_states), _p(jobs), len(jobs), _p(meas), len(meas), _p(st))

            t_dev = best_of(run_device)
            t_kernel = pre.last_device_ms()
            t_cpu = best_of(run_cpu)
            differ = int(sum(a.tobytes() != b.tobytes() for a, b in zip(d_states, c_states)))
            out["settings"][name] = dict(jobs=len(jobs), measurements_per_job=int(jobs["count"][0]), device_call_ms=round(t_dev, 4), device_kernel_ms=round(t_kernel, 4),
                                         cpu_ms=round(t_cpu, 4), cpu_over_device=round(t_cpu / t_dev, 3), states_not_bit_identical_device_cpu=differ,
                                         largest_difference_device_cpu=float(max(np.abs(d_states[k] - c_states[k]).max() for k in ("dR", "dV", "dP", "JRg", "JPg", "C"))))
            print(name, json.dumps(out["settings"][name]), flush=True)
            if len(jobs) == 4096:
                last = d_states
        # the informations of 4096 links from the 4096 states
        spec = np.zeros(4096, capi.IMU_LINK_SPEC_DTYPE)
        spec["state"] = spec["walk_state"] = np.arange(4096)
        spec["info_scale"] = 1.0
        links_c, st_c = np.zeros(4096, capi.LIBA_LINK_DTYPE), np.zeros(4096, np.int32)
        res = {}

        def links_device():
            res["d"] = pre.links(last, spec)

        def links_cpu():
            cpu.preint_cpu_links(_p(last), len(last), _p(spec), 4096, _p(links_c), _p(st_c))

        t_dev = best_of(links_device)
        t_kernel = pre.last_device_ms()
        t_cpu = best_of(links_cpu)
        assert not res["d"][1].any() and not st_c.any()
        rel = float(np.abs(res["d"][0]["info9"] - links_c["info9"]).max() / np.abs(links_c["info9"]).max())
        out["settings"]["links_4096"] = dict(links=4096, device_call_ms=round(t_dev, 4), device_kernel_ms=round(t_kernel, 4), cpu_ms=round(t_cpu, 4),
                                             cpu_over_device=round(t_cpu / t_dev, 3), largest_relative_info9_difference_device_cpu=rel)
        print("links_4096", json.dumps(out["settings"]["links_4096"]), flush=True)
        for n in (1, 64, 512, 4096, 16384):
            states, jobs, meas = reintegrate_jobs(capi, rng, n, 20)
            best = float("inf")
            for _ in range(4):
                assert not pre.preintegrate(states, jobs, meas).any()
                best = min(best, pre.last_device_ms())
            out["scaling"].append(dict(jobs=n, measurements_per_job=20, device_kernel_ms=round(best, 4)))
        print("scaling", json.dumps(out["scaling"]), flush=True)
    pre.close()
    with open(os.path.join(ROOT, "profiles", "preint_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
