#!/usr/bin/env python3
"""What do the right-camera edges of a two-camera KannalaBrandt8 rig cost?  Times pose_optimize_batch on 256 frames of 300 edges and
lba_solve on a window of 50 key frames / 2000 map points / 20 000 edges -- the sizes of tools/kb8_timing.py -- with a rig set on the
handle and half the edges on the right camera, against the monocular KB8 kernels on a monocular scene of the same sizes.  The two
solve different problems, so per-frame-trial and per-trial times are what compares, not the totals.  Best of three calls after a
warm-up call.  Every step is a process of its own under its own time limit; a step that fails, is killed or times out ends the run
there.  Writes profiles/kb8_rig_timing.json.  Needs an MI355X.

    python tools/kb8_rig_timing.py            # all four steps
    python tools/kb8_rig_timing.py --step pose_rig      (internal: one step, prints one JSON line)
"""
import argparse
import importlib
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
STEPS = {"pose_rig": 120, "pose_kb8": 120, "lba_rig": 180, "lba_kb8": 180}      # seconds


def run_step(step):
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    except Exception:
        pass
    pkg = importlib.import_module("orb_slam3-1_amd")
    sk = importlib.import_module("orb_slam3-1_amd.synth_kb8")
    kind, cam = step.split("_")
    if kind == "pose":
        if cam == "rig":
            frames = [sk.make_pose_problem_rig(100 + i, n=300, n_outliers=30) for i in range(256)]
        else:
            frames = [sk.make_pose_problem_kb8(100 + i, n=300, n_outliers=30) for i in range(256)]
        s = pkg.PoseSolver()
        if cam == "rig":
            s.set_rig_kb8(frames[0]["rig"])
        else:
            s.set_camera_kb8(frames[0]["kb8"])
        prep = s.prepare(frames)
        s.launch(prep)
        calls = []
        for _ in range(3):
            t0 = time.perf_counter(); s.launch(prep); wall = 1e3 * (time.perf_counter() - t0)
            calls.append(dict(call_ms=wall, kernel_ms=s.last_kernel_ms()))
        res = s.results(prep)
        s.close()
        best = min(calls, key=lambda c: c["call_ms"])
        trials = sum(sum(r["trials"]) for r in res)
        right = sum(int((f["stereo"] != 0).sum()) for f in frames) / (256.0 * 300.0)
        return dict(step=step, frames=256, edges_per_frame=300, right_share=right, trials_total=trials, kernel_us_per_frame=1e3 * best["kernel_ms"] / 256,
                    kernel_ns_per_frame_trial=1e6 * best["kernel_ms"] / max(trials, 1), mean_inliers=sum(r["inliers"] for r in res) / 256.0, **best)
    args = dict(n_kf=50, n_fixed=10, n_points=2000, obs_per_point=10, n_outliers=400)
    w = sk.make_ba_window_rig(200, one_edge=True, **args) if cam == "rig" else sk.make_ba_window_kb8(200, **args)
    s = pkg.LbaSolver()
    if cam == "rig":
        s.set_rig_kb8(w["rig"])
    else:
        s.set_camera_kb8(w["kb8"])
    s.solve(w, 10, 0.0)
    calls = []
    for _ in range(3):
        t0 = time.perf_counter(); r = s.solve(w, 10, 0.0); calls.append(1e3 * (time.perf_counter() - t0))
    s.close()
    st = r["stats"]
    return dict(step=step, key_frames=50, points=2000, edges=len(w["edge_point"]), right_share=float((w["edge_stereo"] != 0).mean()), iterations=st["iterations"],
                trials=st["trials"], stop_reason=st["stop_reason"], chi2_initial=st["chi2_initial"], chi2_final=st["chi2_final"], call_ms=min(calls),
                call_ms_per_trial=min(calls) / max(st["trials"], 1))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--step", choices=sorted(STEPS))
    args = ap.parse_args()
    if args.step:
        print("KB8_RIG_TIMING " + json.dumps(run_step(args.step)), flush=True)
        return 0
    out = dict(note="best of three calls after a warm-up call; the kb8 rows run a monocular scene of the same sizes through the monocular KB8 kernels", rows=[])
    for step in ("pose_rig", "pose_kb8", "lba_rig", "lba_kb8"):
        try:
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--step", step], capture_output=True, text=True, timeout=STEPS[step])
        except subprocess.TimeoutExpired:
            print("%s: no result within %d s; stopping here" % (step, STEPS[step]), file=sys.stderr)
            return 1
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("KB8_RIG_TIMING ")]
        if r.returncode != 0 or not line:
            print("%s: exit status %d; stopping here\n%s" % (step, r.returncode, r.stderr[-2000:]), file=sys.stderr)
            return 1
        out["rows"].append(json.loads(line[0][len("KB8_RIG_TIMING "):]))
        print(step, json.dumps(out["rows"][-1]), flush=True)
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "kb8_rig_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
