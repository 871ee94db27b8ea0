"""Times Frame::ComputeStereoFishEyeMatches on the device against one host core and writes profiles/fisheye_stereo_timing.json.

Shapes: 1, 64 and 256 rig frames of 1000 + 1000 key points with 60 % of each side in the lapping area (600 x 600 descriptor pairs per
frame), built from eight seeded scenes of the TUM-VI-like rig of tests/fisheye_stereo_cases.py.
Device, host entry: orbm_stereo_fisheye frame after frame -- wall time of the calls (staging, two launches, the copy back) and the
kernel time of its HIP events, summed over the frames.  Device-resident entry: orbm_stereo_fisheye_batch_device on torch tensors, one
call per batch, timed by HIP events on the stream around 50 back-to-back calls (the mean of them).  Each is the best of three after a warm-up.
CPU: tools/fisheye_stereo_cpu.cpp compiled here with g++ -O3 -mpopcnt -ffp-contract=off: the same search as a plain loop and the shared
header csrc/kb8_stereo_geometry.h on one core, best of three after a warm-up.  The results of the two are compared entry by entry.

    python tools/fisheye_stereo_timing.py [--out profiles/fisheye_stereo_timing.json] [--frames 1 64 256]"""
import argparse
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

N_SIDE, N_LAP, CAP, N_SCENES = 1000, 600, 1024, 8
REPS = 50         # calls of the device-resident entry between the two events: one call alone is a fraction of a millisecond


def make_scene(cases, common, capi, seed):
    """one frame: 400 non-lapping + 600 lapping key points per side; 450 lapping pairs see the same point (a few descriptor bits
    flipped), the rest are distractors"""
    rs = np.random.RandomState(seed)
    rig = cases.RIGS["tumvi"]
    n_pairs = 450
    pl, pr, ol, orr = cases._scene(rig, rs, n_pairs)
    mono = N_SIDE - N_LAP
    kl = np.column_stack([rs.uniform(20, 490, (N_SIDE, 2)), rs.randint(0, cases.N_LEVELS, N_SIDE)])
    kr = np.column_stack([rs.uniform(20, 490, (N_SIDE, 2)), rs.randint(0, cases.N_LEVELS, N_SIDE)])
    dl, dr = cases._random_desc(rs, N_SIDE), cases._random_desc(rs, N_SIDE)
    perm = rs.permutation(N_LAP)[:n_pairs]
    for j in range(n_pairs):
        kl[mono + j] = (pl[j, 0], pl[j, 1], ol[j]); kr[mono + perm[j]] = (pr[j, 0], pr[j, 1], orr[j])
        dr[mono + perm[j]] = cases.flip_bits(rs, dl[mono + j], rs.randint(0, 25))
    return common.keypoints(capi, kl), dl, common.keypoints(capi, kr), dr, mono


def best_of(f, n=3):
    f()
    best = float("inf")
    for _ in range(n):
        best = min(best, f())
    return best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fisheye_stereo_timing.json"))
    ap.add_argument("--frames", type=int, nargs="+", default=[1, 64, 256])
    args = ap.parse_args()
    import torch
    pkg = importlib.import_module("orb_slam3-1_amd")
    capi = importlib.import_module("orb_slam3-1_amd.capi")
    import fisheye_stereo_cases as cases
    import shim_fisheye_common as common
    if pkg.device_count() < 1:
        raise SystemExit("no HIP device: nothing is measured without one")
    dev = torch.device("cuda", 0)
    rig = cases.RIGS["tumvi"]
    scenes = [make_scene(cases, common, capi, 100 + s) for s in range(N_SCENES)]
    out = dict(cpu="one host core (tools/fisheye_stereo_cpu.cpp, g++ -O3 -mpopcnt -ffp-contract=off): the 2-NN Hamming search as a plain loop and "
                   "csrc/kb8_stereo_geometry.h, the functions the kernels run",
               unit="ms per batch, best of 3 after a warm-up", key_points_per_side=N_SIDE, lapping_per_side=N_LAP, settings={})
    m = pkg.Matcher()
    with tempfile.TemporaryDirectory() as d:
        exe = os.path.join(d, "fisheye_stereo_cpu")
        subprocess.check_call(["g++", "-O3", "-mpopcnt", "-ffp-contract=off", "-std=c++17", "-o", exe, os.path.join(ROOT, "tools", "fisheye_stereo_cpu.cpp")])
        for B in args.frames:
            kps = {s: np.zeros((B, CAP), capi.KP_DTYPE) for s in "lr"}
            desc = {s: np.zeros((B, CAP, 32), np.uint8) for s in "lr"}
            n = np.full(B, N_SIDE, np.int32)
            mono = np.zeros(B, np.int32)
            for b in range(B):
                kl, dl, kr, dr, mo = scenes[b % N_SCENES]
                kps["l"][b, :N_SIDE], desc["l"][b, :N_SIDE], kps["r"][b, :N_SIDE], desc["r"][b, :N_SIDE], mono[b] = kl, dl, kr, dr, mo

            # host entry, frame after frame
            def host():
                t0 = time.perf_counter()
                k_ms, res = 0.0, []
                for b in range(B):
                    kl, dl, kr, dr, mo = scenes[b % N_SCENES]
                    res.append(m.stereo_fisheye(rig, kl, dl, mo, kr, dr, mo, cases.LEVEL_SIGMA2))
                    k_ms += m.stereo_fisheye_last_kernel_ms()
                host.kernel_ms, host.res = k_ms, res
                return 1e3 * (time.perf_counter() - t0)
            host_ms = best_of(host)

            # device-resident entry
            up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1)).to(dev)
            t = dict(kl=up(kps["l"]), dl=up(desc["l"]), kr=up(kps["r"]), dr=up(desc["r"]), n=up(n), mono=up(mono))
            o = dict(ltr=torch.zeros(B * CAP, dtype=torch.int32, device=dev), rtl=torch.zeros(B * CAP, dtype=torch.int32, device=dev),
                     depth=torch.zeros(B * CAP, dtype=torch.float32, device=dev), p3d=torch.zeros(B * CAP * 3, dtype=torch.float32, device=dev))
            stream = torch.cuda.current_stream().cuda_stream
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

            def device():
                torch.cuda.synchronize()
                e0.record()
                for _ in range(REPS):
                    m.stereo_fisheye_device(rig, B, CAP, t["kl"].data_ptr(), t["dl"].data_ptr(), t["n"].data_ptr(), t["mono"].data_ptr(), t["kr"].data_ptr(),
                                            t["dr"].data_ptr(), t["n"].data_ptr(), t["mono"].data_ptr(), cases.LEVEL_SIGMA2, o["ltr"].data_ptr(), o["rtl"].data_ptr(),
                                            o["depth"].data_ptr(), o["p3d"].data_ptr(), stream=stream)
                e1.record()
                torch.cuda.synchronize()
                return e0.elapsed_time(e1) / REPS
            dev_ms = best_of(device)

            # one host core
            path_in, path_out = os.path.join(d, "in.bin"), os.path.join(d, "out.bin")
            with open(path_in, "wb") as f:
                f.write(np.array([B, CAP, cases.N_LEVELS], np.int32).tobytes()); f.write(cases.rig_floats(rig).tobytes()); f.write(cases.LEVEL_SIGMA2.tobytes())
                for s in "lr":
                    f.write(kps[s].tobytes()); f.write(desc[s].tobytes()); f.write(n.tobytes()); f.write(mono.tobytes())
            cpu = json.loads(subprocess.check_output([exe, path_in, path_out], text=True))
            raw = np.fromfile(path_out, np.uint8)
            N = B * CAP
            c_ltr, c_rtl = raw[:4 * N].view(np.int32).reshape(B, CAP), raw[4 * N:8 * N].view(np.int32).reshape(B, CAP)
            c_depth, c_p3d = raw[8 * N:12 * N].view(np.float32).reshape(B, CAP), raw[12 * N:].view(np.float32).reshape(B, CAP, 3)
            g_ltr, g_rtl = o["ltr"].cpu().numpy().reshape(B, CAP)[:, :N_SIDE], o["rtl"].cpu().numpy().reshape(B, CAP)[:, :N_SIDE]
            g_depth, g_p3d = o["depth"].cpu().numpy().reshape(B, CAP)[:, :N_SIDE], o["p3d"].cpu().numpy().reshape(B, CAP, 3)[:, :N_SIDE]
            host_same = all(np.array_equal(host.res[b]["left_to_right"], g_ltr[b]) and host.res[b]["p3d"].tobytes() == g_p3d[b].tobytes() for b in range(B))
            both = (g_ltr >= 0) & (c_ltr[:, :N_SIDE] >= 0)
            rel = np.abs(g_p3d[both].astype(np.float64) - c_p3d[:, :N_SIDE][both]).max(initial=0.0) / max(np.abs(c_p3d).max(), 1e-30)
            out["settings"]["frames_%d" % B] = dict(
                frames=B, descriptor_pairs=int(B * N_LAP * N_LAP), matches=int((g_ltr >= 0).sum()),
                host_entry_call_ms=round(host_ms, 4), host_entry_kernel_ms=round(host.kernel_ms, 4), device_entry_ms=round(dev_ms, 4),
                cpu_ms=round(cpu["cpu_ms"], 4), cpu_over_host_entry=round(cpu["cpu_ms"] / host_ms, 3), cpu_over_device_entry=round(cpu["cpu_ms"] / dev_ms, 3),
                pairs_per_second_device_entry=round(B * N_LAP * N_LAP / (dev_ms * 1e-3), 0),
                host_entry_equals_device_entry=bool(host_same),
                matches_differ_device_cpu=int((g_ltr != c_ltr[:, :N_SIDE]).sum() + (g_rtl != c_rtl[:, :N_SIDE]).sum()),
                depth_not_bit_identical_device_cpu=int((g_depth[both] != c_depth[:, :N_SIDE][both]).sum()),
                largest_point_difference_device_cpu_over_largest_coordinate=float(rel))
            print(json.dumps(out["settings"]["frames_%d" % B]), flush=True)
    m.close()
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
