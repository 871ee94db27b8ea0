"""Times the rig projection entries of include/orbslam3_hip_track_project_rig.h on the device and writes
profiles/track_project_rig_timing.json.

Workload: 1 / 64 / 256 rig frames x 2 048 local map points (orbm_frustum_rig_batch_device, both cameras per point) and x 2 000
last-frame entries (orbm_project_last_rig_batch_device), inputs from orb_slam3-1_amd/synth_track.py, all rows live.  Per size, in
one process:
 (a) the device entry on resident arrays: whole-call time (enqueue + synchronise, host clock) and kernel time (HIP events around it);
 (b) the sequence it replaces: the same header (csrc/track_project_rig_geometry.h) on one host core (tools/track_project_rig_cpu.cpp,
     built here with g++), plus the upload of the arrays the rig searches read (the eleven projection arrays of OrbmRigMapPoints; the
     five of OrbmRigLastPoints) from pinned host memory.
(a) and (b) alternate; each figure is the best of three after a warm-up.  No ratio is fixed in advance: the tool records what it
measures, and how many values differ between device and host (atan2 / sin / cos may differ in the last bit).  It exits 1 only when a
device call at 256 frames is not faster than the sequence it replaces: a floor that a broken kernel misses, not a goal.

    python tools/track_project_rig_timing.py [--out profiles/track_project_rig_timing.json] [--frames 1 64 256]"""
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
sys.path[:0] = [ROOT]

LOCAL_POINTS, LAST_POINTS = 2048, 2000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "track_project_rig_timing.json"))
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 64, 256])
    args = ap.parse_args()
    import torch  # first: one HIP runtime per process, see tests/conftest.py
    pkg = importlib.import_module("orb_slam3-1_amd")
    capi = importlib.import_module("orb_slam3-1_amd.capi")
    synth = importlib.import_module("orb_slam3-1_amd.synth_track")
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    st = torch.cuda.current_stream().cuda_stream
    m = pkg.Matcher(0.8, True)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    out = dict(unit="ms per batch, best of 3 after a warm-up", local_points=LOCAL_POINTS, last_points=LAST_POINTS, settings={})
    F_OUT = tuple(capi.RIG_FRUSTUM_DTYPES.items())
    L_OUT = tuple(capi.RIG_LAST_DTYPES.items())
    ok = True

    def best(run_a, run_b):
        run_a(); run_b()
        ta, tb = [], []
        for _ in range(3):
            ta.append(run_a()); tb.append(run_b())
        return [min(x[i] for x in ta) for i in range(2)], [min(x[i] for x in tb) for i in range(2)]

    with tempfile.TemporaryDirectory() as d:
        so = os.path.join(d, "libtrack_project_rig_cpu.so")
        subprocess.check_call(["g++", "-O3", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-I", os.path.join(ROOT, "include"), "-o", so,
                               os.path.join(ROOT, "tools", "track_project_rig_cpu.cpp")])
        cpu = C.CDLL(so)
        cpu.tprc_frustum.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int]
        cpu.tprc_project_last.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        for B in args.frames:
            for kind, rows in (("frustum", LOCAL_POINTS), ("last", LAST_POINTS)):
                case = synth.make_rig_local_map_case(700 + B, B, rows, full=True) if kind == "frustum" else synth.make_rig_last_frame_case(800 + B, B, rows, full=True)
                names = F_OUT if kind == "frustum" else L_OUT
                cam = capi.track_rig_camera(case["cam"])
                d_pose, d_fp = up(np.asarray(case["pose7"], np.float64)), torch.zeros(B * 43, dtype=torch.float32, device=dev)
                m.rig_frame_pose_batch_device(case["cam"], d_pose.data_ptr(), B, 1, d_fp.data_ptr(), st)
                torch.cuda.synchronize()
                fp = d_fp.cpu().numpy().reshape(B, 43).copy()
                d_out = [torch.zeros(B * rows * np.dtype(dt).itemsize, dtype=torch.uint8, device=dev) for _, dt in names]     # the stale state: zeros on both sides
                d_cnt = torch.zeros(B, dtype=torch.int32, device=dev)
                h_out = {k: torch.zeros(B * rows * np.dtype(dt).itemsize, dtype=torch.uint8).pin_memory() for k, dt in names}
                h_cnt = np.zeros(B, np.int32)
                host = {k: h_out[k].numpy().view(dt) for k, dt in names}
                read = [k for k, _ in names if k != "track_depth_r"]   # what the searches read
                d_up = {k: torch.zeros_like(h_out[k], device=dev) for k in read}
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                if kind == "frustum":
                    keys = ("xyz", "normal", "min_distance", "max_distance", "skip", "bad", "n")
                    h_in = [np.ascontiguousarray(case[k]) for k in keys]
                    d_in = [up(a) for a in h_in]
                    pts_d = tuple(t.data_ptr() for t in d_in) + (rows,)
                    outs_d = tuple(t.data_ptr() for t in d_out) + (d_cnt.data_ptr(),)
                    pts_h = capi.LocalPoints(*[a.ctypes.data for a in h_in], rows)
                    out_h = capi.RigFrustumOut(*[host[k].ctypes.data for k, _ in names], h_cnt.ctypes.data)
                    launch = lambda: m.frustum_rig_batch_device(case["cam"], d_fp.data_ptr(), pts_d, float(case["cos_limit"]), outs_d, B, st)
                    on_host = lambda: cpu.tprc_frustum(C.byref(cam), fp.ctypes.data, C.byref(pts_h), C.c_float(case["cos_limit"]), C.byref(out_h), B)
                else:
                    h_in = [np.ascontiguousarray(case[k]) for k in ("xyz", "has_point", "n")]
                    d_in = [up(a) for a in h_in]
                    outs_d = tuple(t.data_ptr() for t in d_out)
                    out_h = capi.RigLastProjOut(*[host[k].ctypes.data for k, _ in names])
                    launch = lambda: m.project_last_rig_batch_device(case["cam"], d_fp.data_ptr(), d_in[0].data_ptr(), d_in[1].data_ptr(), d_in[2].data_ptr(), rows, outs_d, B, st)
                    on_host = lambda: cpu.tprc_project_last(C.byref(cam), fp.ctypes.data, h_in[0].ctypes.data, h_in[1].ctypes.data, h_in[2].ctypes.data, rows, C.byref(out_h), B)

                def run_a():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    e0.record(); launch(); e1.record()
                    torch.cuda.synchronize()
                    return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)

                def run_b():
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    on_host()
                    t1 = time.perf_counter()
                    for k in read:
                        d_up[k].copy_(h_out[k], non_blocking=True)
                    torch.cuda.synchronize()
                    return 1e3 * (time.perf_counter() - t0), 1e3 * (t1 - t0)

                (call_ms, kernel_ms), (seq_ms, host_ms) = best(run_a, run_b)
                differing = {}
                for (k, dt), t in zip(names, d_out):
                    got = t.cpu().numpy().view(dt)
                    nd = int((got.view(np.uint8).reshape(-1, np.dtype(dt).itemsize) != host[k].view(np.uint8).reshape(-1, np.dtype(dt).itemsize)).any(1).sum())
                    if nd:
                        differing[k] = nd
                seen = "in_view" if kind == "frustum" else "valid"
                rec = dict(entry=kind, frames=B, rows_per_frame=rows, in_view=int(host[seen].sum()), call_ms=round(call_ms, 4), kernel_ms=round(kernel_ms, 4),
                           sequence_ms=round(seq_ms, 4), sequence_host_ms=round(host_ms, 4), sequence_upload_ms=round(seq_ms - host_ms, 4),
                           sequence_over_call=round(seq_ms / call_ms, 3), values_differing_from_host=differing)
                if kind == "frustum":
                    rec["in_view_right"] = int(host["in_view_r"].sum())
                    rec["n_to_match_equal"] = bool(np.array_equal(d_cnt.cpu().numpy(), h_cnt))
                out["settings"]["%s_frames_%d" % (kind, B)] = rec
                print(json.dumps(rec), flush=True)
                if B == 256:
                    ok = ok and call_ms < seq_ms
    m.close()
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not ok:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
