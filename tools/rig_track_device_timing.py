"""Times the device-resident rig tracking entries (include/orbslam3_hip_rig_track_device.h) and writes
profiles/rig_track_device_timing.json.

Searches: 1, 64 and 256 rig frames of 1000 + 1000 key points and 900 projected points, the workload of tools/rig_match_timing.py (four
seeded rigs of tests/rig_match_cases.py), resident in device memory.  Per batch: the wall time of the call followed by a stream
synchronise, and the device time of setup + grid + search (HIP events around the call).  Beside them the host-array batch entries in
the same process on the same scenes: the wall time of the call and orbm_rig_search_last_kernel_ms (grid + search).  Every number is
the best of three after a warm-up.  The first batch of every search is compared with the host entry before anything is timed.

The two kinds of number answer to different things.  The call time is what a tracker waits for: the tool exits 1 when the
device-resident call is not faster than the host-array call at 64 and at 256 frames.  The kernel time is the same k_rig in both, so
the device-resident figure should equal the host entry's up to the setup kernel: both and their difference are recorded, no target.

Pose: pose_optimize_rig_batch_device at 256 frames x 750 matched slots (375 per side, slots of 1000 + 1000) beside pose_optimize_batch
with the same edges.

    python tools/rig_track_device_timing.py [--out profiles/rig_track_device_timing.json] [--frames 1 64 256]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

N_SIDE, N_PTS, N_SCENES = 1000, 900, 4
POSE_FRAMES, POSE_EDGES_PER_SIDE = 256, 375


def best_of(f, n=3):
    f()
    best = (float("inf"), 0.0)
    for _ in range(n):
        best = min(best, f())
    return best


def time_searches(pkg, torch, frames_list, out):
    import rig_match_cases as cases
    import rig_track_device_pack as DP
    m = pkg.Matcher(0.8, True)
    scenes = {"mp": [cases.random_mp_call(200 + s, nl=N_SIDE, nr=N_SIDE, n_pts=N_PTS) for s in range(N_SCENES)],
              "last": [cases.random_last_call(200 + s, nl=N_SIDE, nr=N_SIDE, n_pts=N_PTS) for s in range(N_SCENES)]}
    ok = True
    for kind in ("mp", "last"):
        for B in frames_list:
            cs = [scenes[kind][b % N_SCENES] for b in range(B)]
            r = DP.Resident(torch, DP.pack(cs, spare=0))
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def host():
                qs = [dict(rig=c["rig"], pts=c["pts"], assign=c["assign"].copy(), occupied=c["occupied"].copy()) for c in cs]
                m.nnratio, m.check_ori = cs[0]["nnratio"], cs[0]["check_ori"]
                t0 = time.perf_counter()
                if kind == "mp":
                    ns = m.search_by_projection_rig_batch(qs, cs[0]["th"], cs[0]["far_points"], cs[0]["th_far"])
                else:
                    ns = m.search_by_projection_last_rig_batch(qs, cs[0]["th"])
                host.qs, host.ns = qs, ns
                return 1e3 * (time.perf_counter() - t0), m.rig_search_last_kernel_ms()

            def device():
                r.reset_outputs()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                e0.record()
                r.launch(m)
                e1.record()
                torch.cuda.synchronize()
                return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)

            host_ms, host_kernel_ms = best_of(host)
            if B == frames_list[0]:
                device()
                per, _ = r.results()
                for b, (n, a, o) in enumerate(per):
                    if n != host.ns[b] or not np.array_equal(a, host.qs[b]["assign"]) or not np.array_equal(o, host.qs[b]["occupied"]):
                        raise SystemExit("%s: frame %d of the device-resident entry differs from the host entry" % (kind, b))
            dev_ms, dev_kernel_ms = best_of(device)
            rec = dict(search=kind, frames=B, matches=int(sum(host.ns)), device_call_ms=round(dev_ms, 4), device_kernels_ms=round(dev_kernel_ms, 4),
                       host_call_ms=round(host_ms, 4), host_kernels_ms=round(host_kernel_ms, 4), kernels_difference_ms=round(dev_kernel_ms - host_kernel_ms, 4),
                       call_speedup=round(host_ms / dev_ms, 2))
            out["settings"]["%s_frames_%d" % (kind, B)] = rec
            print(json.dumps(rec), flush=True)
            if B in (64, 256) and not dev_ms < host_ms:
                ok = False
    m.close()
    return ok


def time_pose(pkg, torch, out):
    from kb8_rig_cases import EDGE_RIGHT, pose_fixture
    w, rig, g = pose_fixture(560)
    table = np.sort(np.unique(g["inv_sigma2"]))[::-1].astype(np.float32)
    octave = np.searchsorted(-table.astype(np.float64), -g["inv_sigma2"]).astype(np.int32)
    rng = np.random.default_rng(1)
    side = {0: np.nonzero(w["stereo"] == 0)[0], 1: np.nonzero(w["stereo"] == EDGE_RIGHT)[0]}
    B, n_mp, slot_cap = POSE_FRAMES, len(w["Xw"]), 2 * N_SIDE
    kps = [np.zeros((B, N_SIDE, 7), np.float32) for _ in range(2)]
    assign = np.full((B, slot_cap), -1, np.int32)
    xyz = np.tile(w["Xw"].astype(np.float32)[None], (B, 1, 1))
    probs = []
    for b in range(B):
        edges = []
        for s in (0, 1):
            e = side[s][rng.integers(0, len(side[s]), POSE_EDGES_PER_SIDE)]          # (with repetition: the fixture has 280 edges a side)
            slots = np.sort(rng.choice(N_SIDE, POSE_EDGES_PER_SIDE, replace=False))
            kps[s][b, slots, 0:2] = w["obs"][e, 0:2]; kps[s].view(np.int32)[b, slots, 5] = octave[e]
            assign[b, s * N_SIDE + slots] = e
            edges.append(e)
        e = np.concatenate(edges)
        probs.append(dict(w, Xw=xyz[b][e].astype(np.float64), obs=w["obs"][e], inv_sigma2=w["inv_sigma2"][e],
                          stereo=np.array([0] * POSE_EDGES_PER_SIDE + [EDGE_RIGHT] * POSE_EDGES_PER_SIDE, np.uint8)))
    dev = torch.device("cuda", 0)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    n = up(np.full(B, N_SIDE, np.int32))
    t = dict(kl=up(kps[0]), kr=up(kps[1]), assign=up(assign), xyz=up(xyz), pose=up(np.tile(np.concatenate([w["q"], w["t"]])[None], (B, 1))),
             pose_out=up(np.zeros((B, 7))), inliers=up(np.zeros(B, np.int32)), outlier=up(np.zeros((B, slot_cap), np.uint8)))
    frames = dict(d_kps_l=t["kl"].data_ptr(), d_n_l=n.data_ptr(), cap_l=N_SIDE, d_kps_r=t["kr"].data_ptr(), d_n_r=n.data_ptr(), cap_r=N_SIDE, d_assign=t["assign"].data_ptr(),
                  slot_cap=slot_cap, d_mp_xyz=t["xyz"].data_ptr(), mp_cap=n_mp, d_pose=t["pose"].data_ptr(), inv_level_sigma2=table, huber_mono=float(w["huber_mono"]))
    s = pkg.PoseSolver()
    s.set_rig_kb8(rig)
    prep = s.prepare(probs)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    st = torch.cuda.current_stream().cuda_stream

    def device():
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        e0.record()
        s.optimize_rig_batch_device(frames, B, t["pose_out"].data_ptr(), t["inliers"].data_ptr(), t["outlier"].data_ptr(), None, st)
        e1.record()
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0), e0.elapsed_time(e1)

    def host():
        t0 = time.perf_counter()
        s.launch(prep)
        return 1e3 * (time.perf_counter() - t0), s.last_kernel_ms()

    dev_ms, dev_kernel_ms = best_of(device)
    host_ms, host_kernel_ms = best_of(host)
    res = s.results(prep)
    inl = t["inliers"].cpu().numpy().view(np.int32)
    if [r["inliers"] for r in res] != inl.tolist():
        raise SystemExit("pose: the device-resident entry's inliers differ from pose_optimize_batch's")
    s.close()
    rec = dict(frames=B, matched_slots=2 * POSE_EDGES_PER_SIDE, slots=slot_cap, device_call_ms=round(dev_ms, 4), device_kernels_ms=round(dev_kernel_ms, 4),
               host_call_ms=round(host_ms, 4), host_kernel_ms=round(host_kernel_ms, 4), call_speedup=round(host_ms / dev_ms, 2))
    out["pose"] = rec
    print(json.dumps(rec), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rig_track_device_timing.json"))
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 64, 256])
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("orb_slam3-1_amd")
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    out = dict(unit="ms per batch, best of 3 after a warm-up", key_points_per_side=N_SIDE, points=N_PTS, settings={})
    ok = time_searches(pkg, torch, args.frames, out)
    time_pose(pkg, torch, out)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    if not ok:
        raise SystemExit("the device-resident call is not faster than the host-array call at 64 or 256 frames")


if __name__ == "__main__":
    main()
