#!/usr/bin/env python3
"""Times fiba_solve (Optimizer::FullInertialBA on the device) on whole maps of 20 / 100 / 300 key frames with a shared bias
(bInit, 9 N + 6 unknowns with key frame 0 fixed) and with per-key-frame biases (15 N): the host call and the device time (HIP
events around the Levenberg rounds) per call and per trial, the best of three after a warm-up call.  Writes
profiles/fullba_timing.json.  Needs an MI355X.  No CPU restatement of g2o's sparse solve exists here, so no ratio is computed."""
import importlib
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    try:
        import torch  # noqa: F401  (one HIP runtime per process: torch's, loaded first)
    except Exception:
        pass
    pkg = importlib.import_module("orb_slam3-1_amd")
    sf = importlib.import_module("orb_slam3-1_amd.synth_fullba")
    out = dict(note="best of three calls after a warm-up call; 10 points per key frame, 4 observations each, stereo share 0.3, max_iters 7", sizes={})
    s = pkg.FullInertialBA()
    for n in (20, 100, 300):
        for shared in (1, 0):
            pr = sf.make_full_map(3, n_kf=n, shared_bias=shared, stereo_frac=0.3, bias_error=0.01, max_iters=7)
            s.solve(pr)                                             # allocation and first-launch costs stay out of the timing
            calls = []
            for _ in range(3):
                t0 = time.perf_counter(); d = s.solve(pr); wall = 1e3 * (time.perf_counter() - t0)
                calls.append(dict(call_ms=wall, device_ms=s.last_device_ms()))
            best = min(calls, key=lambda c: c["call_ms"])
            st = d["stats"]
            key = "%d_%s" % (n, "shared" if shared else "per_kf")
            out["sizes"][key] = dict(key_frames=n, points=len(pr["points"]), edges=len(pr["edge_kf"]), links=len(pr["links"]),
                                     unknowns=(9 * (n - 1) + 6) if shared else 15 * (n - 1), iterations=st["iterations"], trials=st["trials"],
                                     stop_reason=st["stop_reason"], chi2_initial=st["chi2_initial"], chi2_final=st["chi2_final"],
                                     device_ms_per_trial=best["device_ms"] / max(st["trials"], 1), **best)
            print(key, json.dumps(out["sizes"][key]), flush=True)
    s.close()
    os.makedirs(os.path.join(ROOT, "profiles"), exist_ok=True)
    with open(os.path.join(ROOT, "profiles", "fullba_timing.json"), "w") as f:
        json.dump(out, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
