#!/usr/bin/env python3
"""Timing of orbm_create_new_map_points (needs a HIP device).  A key frame of 1500 features against 10 and 30 neighbours
(orb_slam3-1_amd/synth_mapping.py, mixed mono / stereo).  In one process, alternating per repetition after a warm-up:
  (a) the new call, host arrays in and out: one upload, one launch, one download (host clock around the C call, which ends in a
      stream synchronise); kernel ms from orbm_create_new_map_points_last_kernel_ms (HIP events around the kernel);
  (b) what the library offered before for the same work: n_neighbours calls of orbm_search_for_triangulation alone (each uploads
      key frame 1 again, launches one workgroup and synchronises), WITHOUT any triangulation;
  (c) for context, the numpy float64 geometry (tests/newpoints_reference.py) on the matches the device found, timed once.
(a) does strictly more than (b); the requirement is (a) < (b) at both neighbour counts, and the tool exits 1 when it does not
hold.  Writes profiles/newpoints_timing.json."""
import argparse
import ctypes as C
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def _stats(ts):
    ts = np.asarray(ts) * 1e3
    return dict(median=float(np.median(ts)), p10=float(np.percentile(ts, 10)), p90=float(np.percentile(ts, 90)))


def upload_bytes(sc):
    """bytes of input arrays the new call moves to the device: every key frame once"""
    total = 0
    for kf in [sc["kf1"]] + sc["neighbours"]:
        n = len(kf["x"])
        total += n * (32 + 2 + 4 * 5 + (8 if kf.get("key_x") is not None else 0)) + 4 * (len(kf["fv"][1]) + len(kf["fv"][2])) + 8 * len(kf["scale_factors"])
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--features", type=int, default=1500)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "newpoints_timing.json"))
    a = ap.parse_args()
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch first)
        device_name = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "unknown"
    except Exception:
        device_name = "unknown (torch not importable)"
    pkg = importlib.import_module("orb_slam3-1_amd")
    sm = importlib.import_module("orb_slam3-1_amd.synth_mapping")
    import newpoints_reference as R
    if pkg.device_count() < 1:
        raise SystemExit("newpoints_timing needs a HIP device: there is nothing to fall back to")
    m = pkg.Matcher(0.6, False)
    lib = pkg.lib
    rows, ok = [], True
    for nn in (10, 30):
        sc = sm.make_mapping_scene(500 + nn, n=a.features, n_neighbours=nn, stereo_frac=0.4, max_baseline=0.8)
        full = m.create_new_map_points(sc["kf1"], sc["neighbours"], sc["pairs"], sc["params"])      # with match12, for (c)
        prep = m.create_new_map_points_prepare(sc["kf1"], sc["neighbours"], sc["pairs"], sc["params"])
        prep["out"].match12 = None                                                                  # the call as a user makes it
        # (b): the arguments of the n searches, marshalled once
        sides, keep = [], []
        for k in [sc["kf1"]] + sc["neighbours"]:
            fv = pkg.capi._fv(k["fv"])
            keep.append(fv)
            sides.append(pkg.Matcher._TriSide(len(k["x"]), k["desc"].ctypes.data, k["has_mp"].ctypes.data, k["stereo"].ctypes.data, k["x"].ctypes.data,
                                              k["y"].ctypes.data, k["octave"].ctypes.data, k["angle"].ctypes.data, fv))
        m12 = np.full(len(sc["kf1"]["x"]), -1, np.int32)
        args = [(C.byref(sides[0]), C.byref(sides[1 + j]), C.c_float(p["ep"][0]), C.c_float(p["ep"][1]), p["F12"].ctypes.data_as(C.c_void_p),
                 k["level_sigma2"].ctypes.data_as(C.c_void_p), k["scale_factors"].ctypes.data_as(C.c_void_p), len(k["scale_factors"]), 0,
                 int(p["coarse"]), 0, m12.ctypes.data_as(C.c_void_p)) for j, (k, p) in enumerate(zip(sc["neighbours"], sc["pairs"]))]

        def new_call():
            return m.create_new_map_points_launch(prep)

        def searches():
            t = 0
            for x in args:
                t += lib.orbm_search_for_triangulation(m._h, *x)
            return t

        for _ in range(a.warmup):
            new_call(); searches()
        ta, tb, kms = [], [], []
        for _ in range(a.reps):
            t0 = time.perf_counter(); created = new_call(); t1 = time.perf_counter()
            kms.append(m.create_new_map_points_last_kernel_ms())
            t2 = time.perf_counter(); searches(); t3 = time.perf_counter()
            ta.append(t1 - t0); tb.append(t3 - t2)
        assert created == full["created"]
        t0 = time.perf_counter()
        ref = R.create_new_map_points(sc, lambda j, has_mp: full["match12"][j], np.float64)
        host_ms = (time.perf_counter() - t0) * 1e3
        row = dict(features=a.features, n_neighbours=nn, created=int(created), reached_pairs=len(ref["pairs"]), upload_bytes=upload_bytes(sc),
                   new_call_ms=_stats(ta), kernel_ms=float(np.median(kms)), searches_only_ms=_stats(tb), numpy_geometry_ms=host_ms,
                   new_call_faster=bool(np.median(ta) < np.median(tb)))
        ok = ok and row["new_call_faster"]
        rows.append(row)
        print(row, flush=True)
    m.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(dict(device=device_name, reps=a.reps, warmup=a.warmup, requirement="new_call_ms < searches_only_ms at both neighbour counts",
                       requirement_met=ok, rows=rows), f, indent=1)
    print("wrote", a.out)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
