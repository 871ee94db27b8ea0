"""Times CreateNewMapPoints for two-camera fisheye rigs on the device and writes profiles/rig_newpoints_timing.json.

Workload: a rig key frame of 1000 + 1000 key points against 10 and 30 rig neighbours of 1000 + 1000 key points each
(orb_slam3-1_amd/synth_rig_mapping.py, about 260 vocabulary nodes a key frame), in one process:
 (a) orbm_create_new_map_points_rig: one call, host arrays in and out (the arguments are flattened once, outside the timed region);
 (b) the sequence it replaces, on the entries that existed before it: per neighbour the baseline test, one
     orbm_search_for_triangulation_rig call with has_mp of key frame 1 as the previous neighbours left it, and the per-match geometry
     of csrc/orbm_new_points_rig_geometry.h on one host core (tools/rig_newpoints_cpu.cpp, built here with g++ and called in process);
 (c) the device time of (a)'s launches alone (HIP events).
(a) and (b) alternate; each figure is the best of three after a warm-up.  Before anything is timed the call is checked against the
sequential reference of tests/rig_newpoints_reference.py on a 300 + 300 feature scene.  The tool exits 1 unless (a) < (b) at both
neighbour counts and (a) and (b) create the same points (neighbour and idx2 of every feature, and the skipped neighbours).

    python tools/rig_newpoints_timing.py [--out profiles/rig_newpoints_timing.json] [--neighbours 10 30]"""
import argparse
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
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N_SIDE, N_PTS = 1000, 800


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_newpoints_timing.json"))
    ap.add_argument("--neighbours", type=int, nargs="+", default=[10, 30])
    args = ap.parse_args()
    import torch  # noqa: F401  first: one HIP runtime per process, see tests/conftest.py
    pkg = importlib.import_module("orb_slam3-1_amd")
    capi = importlib.import_module("orb_slam3-1_amd.capi")
    synth = importlib.import_module("orb_slam3-1_amd.synth_rig_mapping")
    import rig_newpoints_cases as cases
    import rig_newpoints_reference as R
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    lib = pkg.lib
    capi._rig_bow_argtypes(); capi._rig_newpoints_argtypes()
    m = pkg.Matcher(0.6, False)

    sc = cases.scene_of("random_10")
    dev = m.create_new_map_points_rig(sc["kf1"], sc["neighbours"], sc["pairs"], sc["params"])
    errs = R.compare(cases.expected("random_10"), dev, sc, "random_10")
    if max(errs) > 4 * R.SPREAD_F32:
        raise SystemExit("the device result differs from the restatement")

    out = dict(unit="ms per key frame, best of 3 after a warm-up", key_points_per_frame="%d + %d" % (N_SIDE, N_SIDE), runs={})
    ok = True
    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "librig_newpoints_cpu.so")
        subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                               "-o", so, os.path.join(ROOT, "tools", "rig_newpoints_cpu.cpp")])
        cpu = C.CDLL(so)
        cpu.rnp_cpu_skip.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        cpu.rnp_cpu_neighbour.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 8
        for K in args.neighbours:
            sc = synth.make_rig_mapping_scene(seed=900 + K, n_pts=N_PTS, n_neighbours=K, total=2 * N_SIDE, far_points=True, th_far=7.0)
            kf1 = sc["kf1"]
            n1 = len(kf1["x"])
            prep_a = capi.rig_new_points_args(kf1, sc["neighbours"], sc["pairs"], sc["params"])

            def run_a():
                t0 = time.perf_counter()
                run_a.created = m.create_new_map_points_rig_launch(prep_a)
                return 1e3 * (time.perf_counter() - t0)

            # (b): the same flattened key frames, with a has_mp array of key frame 1 that the host half updates in place
            has_mp0 = np.ascontiguousarray(kf1["has_mp"], np.uint8).copy()
            has_mp = has_mp0.copy()
            prep_b = capi.rig_new_points_args(dict(kf1, has_mp=has_mp), sc["neighbours"], sc["pairs"], sc["params"])
            kfs, prs, o = prep_b["kfs"], prep_b["pairs"], prep_b["arrays"]
            assert kfs[0].side.has_mp == has_mp.ctypes.data
            sides = [C.pointer(kfs[q].side) for q in range(1 + K)]
            kf_ptr = [C.addressof(kfs[q]) for q in range(1 + K)]
            m12 = np.full(n1, -1, np.int32)
            state = C.c_int32(0)
            skipped_b = np.zeros(K, np.uint8)

            def run_b():
                t0 = time.perf_counter()
                has_mp[:] = has_mp0
                o["neighbour"][:] = -1; o["idx2"][:] = -1
                state.value = 0
                skipped_b[:] = 0
                created = 0
                for j in range(K):
                    if cpu.rnp_cpu_skip(kf_ptr[0], kf_ptr[1 + j], state.value):
                        skipped_b[j] = 1
                        continue
                    n = lib.orbm_search_for_triangulation_rig(m._h, sides[0], kfs[0].n_left, sides[1 + j], kfs[1 + j].n_left, prs[j].geom, kfs[0].level_sigma2,
                                                              kfs[1 + j].level_sigma2, min(kfs[0].n_levels, kfs[1 + j].n_levels), 0, prs[j].coarse, 0, m12.ctypes.data)
                    if n < 0:
                        raise SystemExit("orbm_search_for_triangulation_rig failed: %d" % n)
                    created += cpu.rnp_cpu_neighbour(kf_ptr[0], kf_ptr[1 + j], m12.ctypes.data, C.addressof(prep_b["params"]), j, has_mp.ctypes.data,
                                                     o["neighbour"].ctypes.data, o["idx2"].ctypes.data, o["x3d"].ctypes.data, o["normal"].ctypes.data,
                                                     o["max_dist"].ctypes.data, o["min_dist"].ctypes.data, C.addressof(state))
                run_b.created = created
                return 1e3 * (time.perf_counter() - t0)

            run_a(); run_b()                                            # warm-up
            ta, tb, kernel = [], [], []
            for _ in range(3):
                ta.append(run_a())
                ms, launches = m.create_new_map_points_rig_last()
                kernel.append(ms)
                tb.append(run_b())
            a = capi.rig_new_points_result(prep_a, run_a.created)
            same = bool(np.array_equal(a["neighbour"], o["neighbour"][:n1]) and np.array_equal(a["idx2"], o["idx2"][:n1]) and np.array_equal(a["skipped"], skipped_b)
                        and run_a.created == run_b.created)
            acc = a["neighbour"] >= 0
            bits = int((a["x3d"][acc].view(np.uint32) != o["x3d"][:n1][acc].view(np.uint32)).any(axis=1).sum())
            rec = dict(neighbours=K, features=n1, n_left=int(kf1["n_left"]), created=int(run_a.created), matched=int(a["n_matched"].sum()),
                       skipped=int(a["skipped"].sum()), launches=launches, call_ms=round(min(ta), 4), sequence_ms=round(min(tb), 4), kernel_ms=round(min(kernel), 4),
                       sequence_over_call=round(min(tb) / min(ta), 3), created_identical=same, points_with_other_float_bits=bits)
            out["runs"]["neighbours_%d" % K] = rec
            print(json.dumps(rec), flush=True)
            ok = ok and same and min(ta) < min(tb)
    m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
