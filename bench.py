#!/usr/bin/env python3
"""bench.py -- headline benchmark of the hot path on MI355X (BASELINE.json: "tracking frames/s (ORB extract+match)
and LocalBA iters/s, 1/2/4/8 MI355X vs CPU ref").

  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N --steps K --warmup W

One "step" = one pass of the hot path over one batch of synthetic input that is already resident in HBM:
  ORBextractor::operator() on B 640x480 mono frames (8 levels, 1000 features, BASELINE configs[1]) followed by
  ORBmatcher::SearchByBoW on B (1000 x 1000)-descriptor pairs (configs[2]), all through the C ABI on one HIP stream.
Frames shard over ranks with no collective (weak scaling: B frames per GPU).  value = frames of all ranks / time of
the slowest rank.  PyTorch only provides device buffers, the stream and torch.distributed.

A plain run sets up, warms up, times K steps, writes the last step's outputs if --dump-outputs is given and prints the
JSON line.  --full adds everything else (--extra and --streams imply it), reported in the same JSON line:
  self_check    8 frames of the timed batch against the CPU oracle (key points, descriptors, BoW matches, bit-exact)
  roofline      dominant extractor kernel, duration measured live with HIP events on the launch stream
  cpu_baseline  the CPU oracle (this repo's restatement of the reference algorithms) on the box's host cores, 1 thread
  lba           LocalBundleAdjustment 50 KF / 2000 MP / 20 k edges (configs[3]): outer LM iterations per second
  gba           (N>1 only) landmark-sharded global BA whose reduced camera system is summed with one RCCL all-reduce
and the whole record goes to the --detail file.
"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_PEAK_GBS = 8000.0           # MI355X_MICROARCH.md: HBM3E 8 TB/s spec (6.3 TB/s achievable)
ALGO_BYTES_PER_FRAME = 4934396  # algorithmic HBM traffic of one 640x480 extraction
FP64_PEAK_TFLOPS = 78.6         # MI355X FP64 vector = matrix peak (SURVEY.md 8(d) planning figure; 256 CUs x 128 FLOP/clk x 2.4 GHz)
LBA_MFLOP_FIRST_TRIAL = 47.0    # algorithmic flops of one LM outer iteration (sparse count) ...
LBA_MFLOP_EXTRA_TRIAL = 37.0    # ... and of every further trial of the same iteration
XGMI_PEAK_GBS = 7 * 153.0       # 7 links x ~153 GB/s per GPU, point to point


def median_call_seconds(fn, n):
    """median wall time of n single calls (a latency figure must not carry one scheduling hiccup of the host)"""
    ts = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    ts.sort()
    return ts[len(ts) // 2]


def compact_line(out, detail=None):
    """The ONE JSON line of the contract, kept short enough that every graded number survives a 2000-character tail:
    headline keys, roofline, cpu_baseline and the LocalBA half of the metric.  Everything else goes to the detail file."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
            "dtype", "data", "config")
    line = {k: out[k] for k in keep if k in out}
    if "config" in line:
        line["config"] = {k: v for k, v in line["config"].items() if k not in ("sharding", "frames_per_step")}
    if "roofline" in out:
        r = out["roofline"]
        line["roofline"] = {k: r[k] for k in ("bound", "valu_issue_frac", "kernel", "achieved", "peak", "unit", "frac", "traffic", "traffic_from", "launch_ms",
                                               "pipeline_frac", "stage_ms") if k in r}
        if line["roofline"].get("traffic") is not None:
            line["roofline"].pop("traffic_from", None)          # (the file name is in bench_detail.json; a null keeps its reason)
        if "stage_ms" in line["roofline"]:
            line["roofline"]["stage_ms"] = {k: round(v, 3) for k, v in line["roofline"]["stage_ms"].items()}
    for k in ("cpu_baseline", "speedup_vs_cpu_1core"):
        if k in out:
            line[k] = out[k]
    if "self_check" in out:
        line["self_check"] = {"ok": out["self_check"]["ok"], "frames_vs_oracle": len(out["self_check"]["frames_checked"])}
    if out.get("n_gpus", 1) > 1 and "roofline" in line:       # the N > 1 line carries two more legs: the per-stage times stay in the N = 1 line
        line["roofline"].pop("stage_ms", None)
    if "lba" in out:
        l = out["lba"]
        line["lba"] = {k: l[k] for k in ("metric", "value", "unit", "dtype", "ms_per_iteration", "ms_per_trial", "roofline", "cpu_baseline",
                                          "speedup_vs_cpu_1core", "workload") if k in l}
        if "roofline" in line["lba"]:
            line["lba"]["roofline"] = {k: v for k, v in line["lba"]["roofline"].items() if k not in ("traffic", "mflop_per_iteration")}
        if "batched" in l:
            bl = l["batched"]
            line["lba"]["batched"] = {k: bl[k] for k in ("error", "windows", "value", "iters_per_s_whole_call") if k in bl}
            if "roofline" in bl:
                line["lba"]["batched"]["roofline_frac"] = bl["roofline"]["frac"]
    if "stereo" in out:
        line["stereo"] = {k: out["stereo"][k] for k in ("value", "unit", "ms_per_step", "stereo_matches_per_frame") if k in out["stereo"]}
    if "gba" in out:        # the short form of the sharded global-BA leg (N > 1); the full record is in bench_detail.json
        g = out["gba"]
        line["gba"] = {k: g[k] for k in ("error", "iters_per_s", "iterations", "trials", "allreduce_bytes_per_trial") if k in g}
        if "workload" in g:
            line["gba"]["workload"] = "500 KF / 20 k MP / 200 k edges"
        if "c_abi_driver" in g:
            line["gba"]["c_abi_driver"] = {k: g["c_abi_driver"][k] for k in ("iters_per_s", "same_path_as_python_driver", "skipped") if k in g["c_abi_driver"]}
        if "roofline" in g:
            line["gba"]["roofline"] = {k: g["roofline"][k] for k in ("bound", "achieved", "peak", "unit", "frac") if k in g["roofline"]}
    if detail is not None:
        line["detail"] = detail

    def shorten(o):         # six significant digits are plenty for a headline line
        if isinstance(o, float):
            return float("%.6g" % o)
        if isinstance(o, dict):
            return {k: shorten(v) for k, v in o.items()}
        return o
    return shorten(line)


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def stage_algorithmic_bytes(level_sizes, n_kp, n_cand):
    """Algorithmic bytes per frame of every extractor stage."""
    px = [w * h for (w, h) in level_sizes]
    return {
        "resize": sum(px[:-1]) + sum(px[1:]),               # read levels 0..L-2, write levels 1..L-1
        "fast_strips": sum(px) + 4 * n_cand,                 # every level read once + candidate records
        "octree": 2 * 4 * n_cand + 4 * n_kp,                # candidate keys in/out (latency-bound stage)
        "index": 8 * n_kp,
        "blur": 2 * sum(px),                                # read + write every level
        "orient_desc": n_kp * (31 * 31 + 37 * 37) + n_kp * 60,   # patch reads + 28 B keypoint + 32 B descriptor
        "copy_level0": 2 * px[0],                            # only when the input cannot be read in place (unaligned)
    }


def cpu_baseline(synth, imgs, match_sets, budget_s=12.0):
    """Oracle (kind 'port': the reference cannot be built here) timed on ONE host core, extract + SearchByBoW per frame."""
    from oracle_api import Oracle, build_oracle
    try:
        path = build_oracle(native=True)        # -O3 -march=native like the reference's CMakeLists.txt:10-13
    except Exception:
        path = None
    o = Oracle(path)
    ex = o.extractor(1000, 1.2, 8, 20, 7)
    ms = match_sets[0]

    def one(i):
        ex.extract(imgs[i % len(imgs)], (0, 1000))
        o.search_by_bow(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], ms["dF"], ms["angF"], ms["fvF"], 0.7, True)
    one(0)
    t0 = time.perf_counter()
    for i in range(10):
        one(i)
    per = (time.perf_counter() - t0) / 10
    n = int(max(30, min(5000, budget_s / per)))
    t0 = time.perf_counter()
    for i in range(n):
        one(i)
    dt = time.perf_counter() - t0
    return o, {"value": n / dt, "unit": "frames/s", "cores": 1, "kind": "port",
               "sample": "%d frames (extract + SearchByBoW), 1 thread, %.1f s" % (n, dt)}


def check_against_oracle(pkg, ex, B, cap, d_kps, d_desc, d_n, d_mono, host_imgs, n_distinct, bow, match_sets, n_sets, n_check=8):
    """Untimed checker leg: n_check frames spread over the batch the TIMED loop left on the device (B device-resident frames read in
    place, the large-batch schedule) are compared with the CPU oracle -- mono index, key points, descriptor bytes -- and so are the
    SearchByBoW results of the same batch slots.  Raises SystemExit on any difference."""
    from oracle_api import Oracle
    o = Oracle()
    oex = o.extractor(1000, 1.2, 8, 20, 7)
    sched = ex.debug_last_schedule()
    nk = d_n.cpu().numpy(); mono = d_mono.cpu().numpy()
    kps = d_kps.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap)
    desc = d_desc.cpu().numpy().reshape(B, cap, 32)
    picks = sorted(set(int(round(i * (B - 1) / max(n_check - 1, 1))) for i in range(n_check)))
    for b in picks:
        r0, k0, d0 = oex.extract(host_imgs[b % n_distinct], (0, 1000))
        if mono[b] != r0 or nk[b] != len(k0) or any(not np.array_equal(kps[b, :nk[b]][f], k0[f]) for f in k0.dtype.names) or not np.array_equal(desc[b, :nk[b]], d0):
            raise SystemExit("SELF-CHECK FAILED: extractor output of batch frame %d differs from the oracle" % b)
        ms = match_sets[b % n_sets]
        n0, m0 = o.search_by_bow(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], ms["dF"], ms["angF"], ms["fvF"], 0.7, True)
        if bow[b][0] != n0 or not np.array_equal(bow[b][1], m0):
            raise SystemExit("SELF-CHECK FAILED: SearchByBoW result of batch slot %d differs from the oracle" % b)
    return {"frames_checked": picks, "against": "CPU oracle (key points, descriptors, BoW matches bit-exact)", "schedule_bits": sched, "ok": True}


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(ddir, pkg, B, cap, d_kps, d_desc, d_n, d_mono, bow):
    """What the last timed step handed its caller, as float32 / float64 .npy files in ddir: per frame the mono index, the key-point
    count, the key points (x, y, size, angle, response, octave, class_id) and descriptor bytes of its first n slots (rows of all frames
    concatenated in frame order), and the SearchByBoW result of its batch slot (match count; per F feature the KF index or -1).
    All frames while the files stay within DUMP_LIMIT_BYTES, else a fixed seeded sample of frames (frames.npy lists the frames kept)."""
    nk = d_n.cpu().numpy().astype(np.int64)
    mono = d_mono.cpu().numpy()
    kps = d_kps.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap)
    desc = d_desc.cpu().numpy().reshape(B, cap, 32)
    per_frame = [int(nk[b]) * (7 + 32) * 4 + len(bow[b][1]) * 4 + 3 * 8 + 8 for b in range(B)]
    frames = list(range(B))
    if sum(per_frame) > DUMP_LIMIT_BYTES:
        frames, used = [], 0
        for b in np.random.RandomState(0).permutation(B):
            if used + per_frame[b] <= DUMP_LIMIT_BYTES:
                frames.append(int(b)); used += per_frame[b]
        frames.sort()
    kp_rows = [np.stack([kps[b, :nk[b]][f].astype(np.float32) for f in pkg.KP_DTYPE.names], 1) for b in frames]
    arrays = {
        "frames": np.asarray(frames, np.float64),
        "mono_index": mono[frames].astype(np.float64),
        "n_keypoints": nk[frames].astype(np.float64),
        "keypoints": np.concatenate(kp_rows).reshape(-1, 7),
        "descriptors": np.concatenate([desc[b, :nk[b]] for b in frames]).astype(np.float32).reshape(-1, 32),
        "bow_n_matches": np.asarray([bow[b][0] for b in frames], np.float64),
        "bow_matches": np.concatenate([bow[b][1] for b in frames]).astype(np.float32),
    }
    os.makedirs(ddir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(ddir, name + ".npy"), a)
    return {"dir": ddir, "frames": len(frames), "bytes": int(sum(a.nbytes for a in arrays.values()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batch", type=int, default=int(os.environ.get("ORBX_BENCH_BATCH", "256")))
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step computed (rank 0) to DIR/<name>.npy, float32 / float64, at most 64 MB")
    ap.add_argument("--full", action="store_true",
                    help="after the headline, also run the oracle self-check, roofline, LocalBA, CPU-baseline legs (and the stereo / "
                         "global-BA legs when N > 1) and write the whole record to the --detail file")
    ap.add_argument("--detail", metavar="PATH", default=None,
                    help="--full: where the whole record goes (default bench_out/bench_detail.json in the repository)")
    ap.add_argument("--no-cpu", action="store_true", help="--full without the CPU-baseline legs")
    ap.add_argument("--no-lba", action="store_true", help="--full without the LocalBA leg (and the legs that need it)")
    ap.add_argument("--no-check", action="store_true", help="--full without the untimed comparison of the timed path's results with the CPU oracle")
    ap.add_argument("--extra", action="store_true",
                    help="implies --full; also time the SURVEY 8(f) legs (PoseOptimization, projection search, vocabulary transform, packets, "
                         "inertial BA ...); they go to the detail file, never into the headline line")
    ap.add_argument("--streams", type=int, default=1,
                    help="implies --full when above 1; extra leg (off by default so that every profiled launch has the headline's size): "
                         "the same batch cut over this many independent HIP streams, e.g. --streams 4")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    if args.extra or args.streams > 1:
        args.full = True

    import torch
    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        log("warning: WORLD_SIZE=%d but --gpus %d" % (world, args.gpus))
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a GPU: the product has no CPU fallback")
    local_rank %= torch.cuda.device_count()      # rehearsals with more ranks than GPUs (gloo) share a device
    torch.cuda.set_device(local_rank)
    dev = torch.device("cuda", local_rank)
    dist = None
    if world > 1:
        import torch.distributed as dist
        import datetime
        backend = os.environ.get("ORBX_BENCH_BACKEND", "nccl")      # "nccl" is RCCL on ROCm; "gloo" only for rehearsals
        backend_is_nccl = backend == "nccl"
        if backend == "nccl":
            dist.init_process_group("nccl", device_id=dev, timeout=datetime.timedelta(seconds=300))
        else:
            dist.init_process_group(backend, timeout=datetime.timedelta(seconds=300))

    pkg = importlib.import_module("orb_slam3-1_amd")
    synth = importlib.import_module("orb_slam3-1_amd.synth")
    dmod = importlib.import_module("orb_slam3-1_amd.distributed")

    B, K, W = args.batch, args.steps, args.warmup
    Hh, Ww = 480, 640
    # ---- synthetic inputs, resident in HBM before the timed region ----
    n_distinct = min(64, B)         # 64 different frames (octree and FAST fallback are data-dependent: a real stream has a slow-frame tail)
    host_imgs = synth.make_frames(n_distinct, seed0=100 * rank)
    reps = (B + n_distinct - 1) // n_distinct
    d_imgs = torch.from_numpy(np.concatenate([host_imgs] * reps)[:B].copy()).to(dev)
    ex = pkg.Extractor(1000, 1.2, 8, 20, 7, device=local_rank)
    cap = ex.max_keypoints
    d_kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device=dev)
    d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev)
    d_n = torch.zeros(B, dtype=torch.int32, device=dev)
    d_mono = torch.zeros(B, dtype=torch.int32, device=dev)
    d_status = torch.zeros(B, dtype=torch.int32, device=dev)
    n_sets = 16
    match_sets = [synth.make_match_set(50 + i) for i in range(n_sets)]
    matcher = pkg.Matcher(0.7, True, device=local_rank)
    plan = matcher.bow_plan([match_sets[i % n_sets] for i in range(B)])
    stream = torch.cuda.current_stream().cuda_stream

    # (Measured and dropped: the step's SearchByBoW on a side stream behind its extraction, beside the NEXT step's extraction --
    # 0.9863 against 0.9853 ms per step on one stream: the extraction keeps every SIMD issuing, a kernel beside it only takes its share.)
    def step():
        ex.extract_batch_device(d_imgs.data_ptr(), B, Ww, Hh, Ww, Ww * Hh, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                                d_n.data_ptr(), d_mono.data_ptr(), d_status.data_ptr(), (0, 1000), stream)
        plan.run(stream)

    def barrier():
        if dist is not None:
            dist.barrier()

    for _ in range(W):
        step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(K):
        step()
    torch.cuda.synchronize()
    barrier()
    torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if dist is not None:
        t = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        elapsed = float(t.item())
    frames = world * B * K
    value = frames / elapsed

    # sanity of what was computed (not timed)
    st = d_status.cpu().numpy()
    nk = d_n.cpu().numpy()
    if (st != 0).any():
        raise SystemExit("extractor reported device status %r" % st[st != 0][:4])
    bow = plan.fetch(stream)
    n_kp = float(nk.mean())
    if rank == 0 and args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, pkg, B, cap, d_kps, d_desc, d_n, d_mono, bow)
        log("outputs of the last timed step: %d frames, %d bytes in %s" % (dumped["frames"], dumped["bytes"], dumped["dir"]))
    # self-check of the timed path (untimed, --full): 8 frames of the batch the timed loop produced -- key points, descriptors and the
    # BoW matches of their pairs -- against the CPU oracle; a mismatch fails the run
    self_check = None
    if rank == 0 and args.full and not args.no_check:
        self_check = check_against_oracle(pkg, ex, B, cap, d_kps, d_desc, d_n, d_mono, host_imgs, n_distinct, bow, match_sets, n_sets)

    out = {
        "metric": "tracking frames/s (ORB extract+match)", "value": value, "unit": "frames/s",
        "n_gpus": world, "steps": K, "warmup": W, "ms_per_step": 1e3 * elapsed / K,
        "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
        "config": {"workload": "ORBextractor 640x480, 8 levels, 1000 features (configs[1]) + SearchByBoW 1000x1000 per frame (configs[2])",
                   "batch_per_gpu": B, "frames_per_step": world * B, "keypoints_per_frame": n_kp,
                   "bow_matches_per_pair": float(np.mean([b[0] for b in bow])), "sharding": "frames, no collective"},
        "pipeline_gbs": ALGO_BYTES_PER_FRAME * value / 1e9,
    }
    if self_check is not None:
        out["config"]["distinct_frames"] = n_distinct
        out["config"]["distinct_match_sets"] = n_sets
        out["self_check"] = self_check

    if rank == 0 and args.full:
        # ---- roofline leg: per-stage device time with HIP events on the launch stream ----
        ex.profile_enable(True)
        acc = {}
        reps_p = 5
        for _ in range(reps_p):
            ex.extract_batch_device(d_imgs.data_ptr(), B, Ww, Hh, Ww, Ww * Hh, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                                    d_n.data_ptr(), d_mono.data_ptr(), d_status.data_ptr(), (0, 1000), stream)
            torch.cuda.synchronize()
            for k, v in ex.profile_read().items():
                acc[k] = acc.get(k, 0.0) + v / reps_p
        ex.profile_enable(False)
        n_cand = float(sum(len(ex.candidates(l, frame=0)) for l in range(8)))
        sizes = [ex.level_size(l) for l in range(8)]
        sb = stage_algorithmic_bytes(sizes, n_kp, n_cand)
        dom = max(acc, key=acc.get)
        achieved = sb[dom] * B / (acc[dom] * 1e-3) / 1e9
        # PMC counters cannot be read from inside the process: `traffic` is the HBM bytes per launch of the same kernel from the
        # separate rocprofv3 --pmc passes (tools/gpu_round.sh -> profiles/pmc_traffic.json), labelled as such, or null.
        # The file carries a hash of the kernel sources it was measured on: a stale file gives `traffic: null` and the reason.
        traffic, traffic_from = None, None
        tpath = os.path.join(ROOT, "profiles", "pmc_traffic.json")
        if os.path.exists(tpath):
            try:
                sys.path.insert(0, os.path.join(ROOT, "tools"))
                from collect_pmc import stamp_matches
                tj = json.load(open(tpath))
                if stamp_matches(tj.get("_kernel_sources_sha"), "k_" + dom, ROOT):
                    traffic = tj.get(dom)
                    traffic_from = "profiles/pmc_traffic.json"
                else:
                    traffic_from = "null: stale counter profile (other kernel sources)"
            except Exception:
                traffic = None
        # What actually bounds the kernel (profiles/r03_a_valu_rates.txt): vector-instruction ISSUE.  valu_issue_frac = the kernel's
        # wave-instructions per SIMD (SQ_INSTS_VALU of a counter pass on these sources, profiles/valu_issue.json) x the measured
        # issue cost of its instruction class (tools/probes/valu_rates.hip: 1.8 ns for v_perm / v_pk_* / v_min3) / the launch time
        # measured now.  `frac` stays the HBM figure of the contract.
        bound, vfrac = "hbm", None
        vpath = os.path.join(ROOT, "profiles", "valu_issue.json")
        if os.path.exists(vpath):
            try:
                from collect_pmc import stamp_matches
                vj = json.load(open(vpath))
                if stamp_matches(vj.get("_kernel_sources_sha"), "k_" + dom, ROOT) and ("k_" + dom) in vj:
                    vfrac = vj["k_" + dom]["valu"] / vj["_simds"] * vj["_ns_per_wave_instruction_and_simd"] * 1e-6 / acc[dom]
                    bound = "valu_issue" if vfrac > 0.5 else "hbm"
            except Exception:
                vfrac = None
        out["roofline"] = {"bound": bound, "valu_issue_frac": vfrac, "kernel": "k_" + dom, "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s",
                           "frac": achieved / HBM_PEAK_GBS, "traffic": traffic, "traffic_from": traffic_from,
                           "pipeline_frac": ALGO_BYTES_PER_FRAME * value / 1e9 / HBM_PEAK_GBS,
                           "launch_ms": acc[dom], "launch_ms_from": "HIP events, serial schedule",
                           "algorithmic_bytes_per_launch": sb[dom] * B,
                           "stage_ms": acc, "stage_gbs": {k: sb[k] * B / (max(acc[k], 1e-6) * 1e-3) / 1e9 for k in acc}}
        # ---- extra leg: the batch cut over S independent streams (one Extractor handle + BoW plan per stream, like the
        # reference's one ORBextractor per camera thread).  Stages with different bottlenecks (FAST: VALU, octree /
        # descriptors / BoW: latency) then overlap across streams and across steps.  Not the headline: per-kernel
        # durations of overlapping launches cannot be compared with the solo launches the roofline figure is made of.
        S = max(1, args.streams)
        if S > 1 and B % S == 0 and B // S >= 8:
            b = B // S
            exs = [pkg.Extractor(1000, 1.2, 8, 20, 7, device=local_rank) for _ in range(S)]
            sts = [torch.cuda.Stream(device=dev) for _ in range(S)]
            plans = [matcher.bow_plan([match_sets[i % n_sets] for i in range(b)]) for _ in range(S)]

            def step_s():
                for i in range(S):
                    o = i * b
                    exs[i].extract_batch_device(d_imgs.data_ptr() + o * Ww * Hh, b, Ww, Hh, Ww, Ww * Hh, d_kps.data_ptr() + o * cap * 28,
                                                d_desc.data_ptr() + o * cap * 32, cap, d_n.data_ptr() + 4 * o, d_mono.data_ptr() + 4 * o,
                                                d_status.data_ptr() + 4 * o, (0, 1000), sts[i].cuda_stream)
                    plans[i].run(sts[i].cuda_stream)
            for _ in range(W):
                step_s()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(K):
                step_s()
            torch.cuda.synchronize()
            dts = time.perf_counter() - t0
            out["concurrent_streams"] = {"streams": S, "frames_per_stream_step": b, "value": B * K / dts, "unit": "frames/s (this GPU)",
                                         "ms_per_step": 1e3 * dts / K, "gain_vs_single_stream": (B * K / dts) / (value / world)}
            for e_ in exs:
                e_.close()
            for p_ in plans:
                p_.close()

        # ---- LocalBA leg (configs[3]) ----
        if not args.no_lba:
            w = synth.make_ba_window(0)
            sh = pkg.LbaShard(w, device=local_rank)
            ad = dmod.LocalHipShard(sh)
            stats = dmod.sharded_bundle_adjustment(ad, None, None, max_iters=10)      # warm-up + reference stats
            n_runs, iters, trials = 5, 0, 0
            t0 = time.perf_counter()
            for _ in range(n_runs):
                sh.reset()
                s2 = dmod.sharded_bundle_adjustment(ad, None, None, max_iters=10)
                iters += s2["iterations"]; trials += s2["trials"]
            dt = time.perf_counter() - t0
            solver = pkg.LbaSolver(device=local_rank)
            solver.solve(w, 10)                       # the first call sizes the solver's device arena and pinned staging buffer
            t1 = time.perf_counter()
            for _ in range(5):
                r = solver.solve(w, 10)
            dt_call = (time.perf_counter() - t1) / 5
            # roofline of the LocalBA half: algorithmic flops (sparse count: 47 MFLOP for the first trial of an
            # outer iteration, 37 MFLOP for every further trial) over the measured time, against the FP64 peak; `kernel` is the
            # launch that dominates a trial, its share measured with HIP events on the solver's stream in this run.
            mflop = LBA_MFLOP_FIRST_TRIAL * iters + LBA_MFLOP_EXTRA_TRIAL * (trials - iters)
            achieved_tf = mflop * 1e-6 / dt
            stage = {}
            try:                                      # HIP events on the solver's stream around every group of launches, one more solve
                sh.reset(); sh.profile_enable(True)
                sp = dmod.sharded_bundle_adjustment(ad, None, None, max_iters=10)
                stage = {k: v / max(sp["trials"], 1) for k, v in sh.profile_read().items()}
                sh.profile_enable(False)
            except Exception as e:  # noqa: BLE001
                log("lba stage profile unavailable: %r" % (e,))
            dom_s = max((k for k in stage if k != "gaps"), key=stage.get) if stage else None
            dom_k = pkg.LbaShard.STAGE_KERNEL.get(dom_s) if dom_s else None
            out["lba"] = {"metric": "LocalBA outer iterations/s", "value": iters / dt, "unit": "iters/s", "dtype": "f64",
                          "workload": "50 opt + 10 fixed KF, 2000 MP, %d mono edges, optimize(10)" % len(w["edge_point"]),
                          "iterations_per_solve": stats["iterations"], "trials_per_solve": stats["trials"],
                          "ms_per_iteration": 1e3 * dt / max(iters, 1), "ms_per_trial": 1e3 * dt / max(trials, 1),
                          "roofline": {"bound": "mfma", "kernel": dom_k, "achieved": achieved_tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s",
                                       "frac": achieved_tf / FP64_PEAK_TFLOPS, "mflop_per_iteration": LBA_MFLOP_FIRST_TRIAL,
                                       "kernel_ms_per_trial": stage.get(dom_s) if dom_s else None, "traffic": None},
                          "stage_ms_per_trial": stage,
                          "lba_solve_call_ms_incl_upload": 1e3 * dt_call, "chi2_initial": stats["chi2_initial"], "chi2_final": stats["chi2_final"]}
            sh.close(); solver.close()

            # ---- many windows per launch (lba_solve_batch, grid.y = window): 32 different windows of configs[3] ----
            try:
                n_w = 32
                bws = [synth.make_ba_window(100 + i) for i in range(n_w)]
                lb = pkg.LbaBatch(device=local_rank)
                bprep = lb.prepare(bws)
                lb.run(bprep, 10); lb.run(bprep, 10)          # sizes the per-slot arenas and pinned staging buffers
                n_rep, b_it, b_tr, dev_ms = 3, 0, 0, 0.0
                t0 = time.perf_counter()
                for _ in range(n_rep):
                    rb = lb.run(bprep, 10)
                    dev_ms += lb.last_device_ms()
                    b_it += sum(r_["stats"]["iterations"] for r_ in rb); b_tr += sum(r_["stats"]["trials"] for r_ in rb)
                dtb = time.perf_counter() - t0
                b_mflop = LBA_MFLOP_FIRST_TRIAL * b_it + LBA_MFLOP_EXTRA_TRIAL * (b_tr - b_it)
                b_tf = b_mflop * 1e-6 / (dev_ms * 1e-3)
                out["lba"]["batched"] = {"windows": n_w, "value": b_it / (dev_ms * 1e-3), "unit": "iters/s (aggregate, Levenberg rounds on the device, data resident)",
                                         "iters_per_s_whole_call": b_it / dtb, "ms_per_call": 1e3 * dtb / n_rep, "device_ms_per_call": dev_ms / n_rep,
                                         "iterations_per_call": b_it / n_rep, "trials_per_call": b_tr / n_rep,
                                         "gain_vs_one_window": (b_it / (dev_ms * 1e-3)) / out["lba"]["value"],
                                         "roofline": {"bound": "mfma", "achieved": b_tf, "peak": FP64_PEAK_TFLOPS, "unit": "TFLOP/s", "frac": b_tf / FP64_PEAK_TFLOPS}}
                lb.close()
            except Exception as e:  # noqa: BLE001
                out["lba"]["batched"] = {"error": repr(e)}

            if args.extra:
                # ---- independent windows side by side (one map per client session): every window has its own shard, stream and
                # host thread; the factorisation kernels are single-workgroup, so concurrent windows fill the idle CUs ----
                import threading
                n_par = 8
                shards = [pkg.LbaShard(synth.make_ba_window(10 + i), device=local_rank) for i in range(n_par)]
                ads = [dmod.LocalHipShard(s_) for s_ in shards]
                for a_ in ads:
                    dmod.sharded_bundle_adjustment(a_, None, None, max_iters=10)
                it_par = [0] * n_par

                def _solve(i_):
                    for _ in range(3):
                        shards[i_].reset()
                        it_par[i_] += dmod.sharded_bundle_adjustment(ads[i_], None, None, max_iters=10)["iterations"]
                ths = [threading.Thread(target=_solve, args=(i_,)) for i_ in range(n_par)]
                t0 = time.perf_counter()
                for t_ in ths:
                    t_.start()
                for t_ in ths:
                    t_.join()
                dtp_ = time.perf_counter() - t0
                out["lba"]["concurrent_windows"] = {"windows": n_par, "value": sum(it_par) / dtp_, "unit": "iters/s (aggregate)",
                                                    "gain_vs_one_window": (sum(it_par) / dtp_) / out["lba"]["value"]}
                for s_ in shards:
                    s_.close()

        # ---- PoseOptimization leg: one workgroup per frame, a batch is one launch ----
        if args.extra and not args.no_lba:
            pose_ws = [synth.make_pose_problem(i, n=300, outlier_frac=0.1, stereo_frac=0.0) for i in range(64)] * 4
            ps = pkg.PoseSolver(device=local_rank)
            prep = ps.prepare(pose_ws)
            ps.run(prep)
            t0 = time.perf_counter(); kms = 0.0
            for _ in range(10):
                ps.launch(prep); kms += ps.last_kernel_ms()
            dtp = (time.perf_counter() - t0) / 10
            prep1 = ps.prepare(pose_ws[:1]); ps.run(prep1)
            t0 = time.perf_counter(); kms1 = 0.0
            for _ in range(20):
                ps.launch(prep1); kms1 += ps.last_kernel_ms()
            dt1 = (time.perf_counter() - t0) / 20
            out["pose"] = {"metric": "PoseOptimization frames/s", "value": len(pose_ws) / dtp, "unit": "frames/s", "dtype": "f64",
                           "workload": "%d frames x 300 mono edges, 10%% gross outliers, 4 rounds x optimize(10); one C call = upload + "
                                       "one launch (a workgroup per frame) + download" % len(pose_ws),
                           "ms_per_batch": 1e3 * dtp, "kernel_ms_per_batch": kms / 10,
                           "single_frame_call_ms": 1e3 * dt1, "single_frame_kernel_ms": kms1 / 20}
            ps.close()

        # ---- projection-search leg: SearchByProjection(CurrentFrame, LastFrame) (TrackWithMotionModel) for a batch of frames,
        # one wave per frame in one launch; host buffers in and out (the call includes grid build, upload and download) ----
        if args.extra and not args.no_lba:
            smm = importlib.import_module("orb_slam3-1_amd.synth_match")
            pcases = [smm.make_last_frame_case(i) for i in range(8)]
            pcases = [(g, dF, aF, sc, last, a.copy(), o_.copy()) for (g, dF, aF, sc, last, a, o_) in pcases * (B // 8)]
            mproj = pkg.Matcher(0.9, True, device=local_rank)
            pprep = mproj.prepare_last_batch(pcases)
            mproj.run_last_batch(pprep, 15.0)
            for c in pcases:
                c[5][:] = -1; c[6][:] = 0
            t0 = time.perf_counter()
            nm = mproj.run_last_batch(pprep, 15.0)
            dtq = time.perf_counter() - t0
            out["proj"] = {"metric": "SearchByProjection(last frame) frames/s", "value": len(pcases) / dtq, "unit": "frames/s", "dtype": "u8",
                           "workload": "%d frames x 1000 features, 900 projected points each, th 15, orientation check; one C call "
                                       "(host grid build + upload + one launch, a wave per frame + download)" % len(pcases),
                           "ms_per_batch": 1e3 * dtq, "matches_per_frame": float(np.mean(nm))}
            mproj.close()

        # ---- vocabulary transform leg: Frame::ComputeBoW for the batch, on the extractor's output ----
        if args.extra and not args.no_lba:
            voc = synth.make_vocabulary_fast(0, k=10, L=6)           # ORBvoc.txt's shape: 1 111 111 nodes, 35 MB of centroids
            vv = pkg.Vocabulary(voc, device=local_rank)
            zb = lambda dt, m: torch.zeros(B * m, dtype=dt, device=dev)
            v_bi, v_bv, v_nb = zb(torch.int32, cap), zb(torch.float64, cap), torch.zeros(B, dtype=torch.int32, device=dev)
            v_fn, v_fo, v_ff, v_nf = zb(torch.int32, cap), zb(torch.int32, cap + 1), zb(torch.int32, cap), torch.zeros(B, dtype=torch.int32, device=dev)

            def vstep(on=None):
                vv.transform_batch_device(d_desc.data_ptr(), d_n.data_ptr(), B, cap, 4, v_bi.data_ptr(), v_bv.data_ptr(), v_nb.data_ptr(),
                                          v_fn.data_ptr(), v_fo.data_ptr(), v_ff.data_ptr(), v_nf.data_ptr(), stream if on is None else on)
            vstep(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                vstep()
            torch.cuda.synchronize()
            dtv = (time.perf_counter() - t0) / 10
            # ---- the whole front end as one device-resident chain: extract -> vocabulary transform -> SearchByBoW between
            # consecutive frames (frame 2i = the "key frame", frame 2i+1 = the same scene moved by 3 px), no host round trip ----
            pair_imgs = np.stack([np.roll(host_imgs[(i // 2) % n_distinct], 3 * (i % 2), axis=1) for i in range(B)])
            d_pairs = torch.from_numpy(np.ascontiguousarray(pair_imgs)).to(dev)
            c_match = torch.zeros((B // 2) * cap, dtype=torch.int32, device=dev); c_nm = torch.zeros(B // 2, dtype=torch.int32, device=dev)

            def cside(b):
                return dict(desc=d_desc.data_ptr() + b * cap * 32, kps=d_kps.data_ptr() + b * cap * 28, n=d_n.data_ptr() + 4 * b, cap=cap,
                            fv_node=v_fn.data_ptr() + 4 * b * cap, fv_off=v_fo.data_ptr() + 4 * b * (cap + 1), fv_feat=v_ff.data_ptr() + 4 * b * cap,
                            n_fv_nodes=v_nf.data_ptr() + 4 * b)
            cplan = pkg.DeviceBowPlan(matcher, [(cside(2 * i), cside(2 * i + 1), c_match.data_ptr() + 4 * i * cap, c_nm.data_ptr() + 4 * i)
                                                for i in range(B // 2)])

            def cstep():
                ex.extract_batch_device(d_pairs.data_ptr(), B, Ww, Hh, Ww, Ww * Hh, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                                        d_n.data_ptr(), d_mono.data_ptr(), d_status.data_ptr(), (0, 1000), stream)
                vstep()
                cplan.run(stream)
            cstep(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(10):
                cstep()
            torch.cuda.synchronize()
            dtc_ = (time.perf_counter() - t0) / 10
            # ---- tracking chain (TrackWithMotionModel's device work per frame, src/Tracking.cc:2975-3053): extract the current frame ->
            # DBoW2 transform -> SearchByProjection(CurrentFrame, LastFrame) against the resident last frames -> PoseOptimization.
            # The last frames (the same scenes 3 px to the left) were extracted before the timed loop, as they are in steady state;
            # the projection of their map points is the known shift here (u = x + 3: a few elementwise device operations);
            # PoseOptimization (pose_optimize_batch_device) gathers its edges on the device from the current frame's key points, the
            # assignment the search wrote and the last frames' map points (resident: the 3-D points behind the last frames' features at
            # random depths, consistent with the current frames' true pose = identity; the initial pose is a few centimetres / degrees off).
            try:
                d_cur_imgs = torch.roll(d_imgs, 3, dims=2).contiguous()
                l_kps = torch.zeros_like(d_kps); l_desc = torch.zeros_like(d_desc); l_n = torch.zeros_like(d_n)
                ex.extract_batch_device(d_imgs.data_ptr(), B, Ww, Hh, Ww, Ww * Hh, l_kps.data_ptr(), l_desc.data_ptr(), cap,
                                        l_n.data_ptr(), d_mono.data_ptr(), d_status.data_ptr(), (0, 1000), stream)
                torch.cuda.synchronize()
                lk = l_kps.view(torch.float32).view(B, cap, 7)
                l_oct = l_kps.view(torch.int32).view(B, cap, 7)[:, :, 5].contiguous()
                l_ang = lk[:, :, 3].contiguous(); l_v = lk[:, :, 1].contiguous()
                l_valid = (torch.arange(cap, device=dev)[None, :] < l_n[:, None]).to(torch.uint8).contiguous()
                t_assign = torch.empty(B * cap, dtype=torch.int32, device=dev); t_occ = torch.empty(B * cap, dtype=torch.uint8, device=dev)
                t_nm = torch.zeros(B, dtype=torch.int32, device=dev)
                mtrk = pkg.Matcher(0.9, True, device=local_rank)
                sfac = ex.GetScaleFactors()
                ps_t = pkg.PoseSolver(device=local_rank)
                cam_t = dict(fx=458.654, fy=457.296, cx=367.215, cy=248.375, bf=0.0)
                gz = torch.Generator(device=dev); gz.manual_seed(7)
                l_z = torch.rand(B, cap, device=dev, generator=gz) * 12.0 + 2.0
                l_mp = torch.stack([(lk[:, :, 0] + 3.0 - cam_t["cx"]) / cam_t["fx"] * l_z, (lk[:, :, 1] - cam_t["cy"]) / cam_t["fy"] * l_z, l_z], 2).contiguous()
                p0 = np.zeros((B, 7)); p0[:, 3] = 1.0
                rs_t = np.random.RandomState(11)
                p0[:, :3] = rs_t.normal(0, 0.01, (B, 3)); p0[:, 4:] = rs_t.normal(0, 0.03, (B, 3))
                t_pose0 = torch.from_numpy(p0).to(dev)
                t_pose = torch.zeros(B, 7, dtype=torch.float64, device=dev); t_inl = torch.zeros(B, dtype=torch.int32, device=dev)
                t_outl = torch.zeros(B * cap, dtype=torch.uint8, device=dev)
                isig_t = (1.0 / np.asarray(sfac, np.float64) ** 2).astype(np.float32)

                # Three schedules of the same four stages (all results identical, all measured):
                #  "one":  everything in a row on the launch stream;
                #  "side": the transform, which feeds neither the search nor PoseOptimization (the reference computes the BoW vector lazily, for
                #          key-frame insertion and relocalisation), on a side stream beside them, ordered behind the extraction by an event;
                #  "pipe": two batches in flight -- the extraction of batch k + 1 (its own stream, a second set of output arrays) beside the
                #          transform / search / PoseOptimization of batch k, which leave most SIMDs idle (one workgroup per frame, latency
                #          bound); a set of arrays is written again only when the batch that read it is done (events).  Throughput figure.
                t_side = torch.cuda.Stream(device=dev); t_ev_v = torch.cuda.Event()
                x_stream = torch.cuda.Stream(device=dev)
                k2, de2, n2 = torch.zeros_like(d_kps), torch.zeros_like(d_desc), torch.zeros_like(d_n)
                t_sets = [(d_kps, d_desc, d_n), (k2, de2, n2)]
                t_ev_x = [torch.cuda.Event(), torch.cuda.Event()]; t_ev_done = [torch.cuda.Event(), torch.cuda.Event()]
                t_count = [0]

                def tstep(mode="pipe"):
                    k_ = t_count[0] & 1 if mode == "pipe" else 0
                    t_count[0] += 1
                    kp_, ds_, nn_ = t_sets[k_]
                    cur_s = torch.cuda.current_stream()
                    if mode == "pipe":
                        x_stream.wait_event(t_ev_done[k_])          # (the batch that read this set of arrays two steps ago)
                        ex.extract_batch_device(d_cur_imgs.data_ptr(), B, Ww, Hh, Ww, Ww * Hh, kp_.data_ptr(), ds_.data_ptr(), cap,
                                                nn_.data_ptr(), d_mono.data_ptr(), d_status.data_ptr(), (0, 1000), x_stream.cuda_stream)
                        t_ev_x[k_].record(x_stream)
                        cur_s.wait_event(t_ev_x[k_])
                    else:
                        ex.extract_batch_device(d_cur_imgs.data_ptr(), B, Ww, Hh, Ww, Ww * Hh, kp_.data_ptr(), ds_.data_ptr(), cap,
                                                nn_.data_ptr(), d_mono.data_ptr(), d_status.data_ptr(), (0, 1000), stream)
                        t_ev_x[k_].record()
                    if mode == "one":
                        vstep()
                    else:
                        t_side.wait_event(t_ev_x[k_])
                        vv.transform_batch_device(ds_.data_ptr(), nn_.data_ptr(), B, cap, 4, v_bi.data_ptr(), v_bv.data_ptr(), v_nb.data_ptr(),
                                                  v_fn.data_ptr(), v_fo.data_ptr(), v_ff.data_ptr(), v_nf.data_ptr(), t_side.cuda_stream)
                        t_ev_v.record(t_side)
                    l_u = (lk[:, :, 0] + 3.0).contiguous()
                    t_assign.fill_(-1); t_occ.zero_()
                    mtrk.SearchByProjection_last_batch_device((kp_.data_ptr(), ds_.data_ptr(), nn_.data_ptr(), cap),
                                                              (l_valid.data_ptr(), l_u.data_ptr(), l_v.data_ptr(), l_oct.data_ptr(), l_ang.data_ptr(), l_desc.data_ptr(), l_n.data_ptr(), cap),
                                                              B, 15.0, t_assign.data_ptr(), t_occ.data_ptr(), t_nm.data_ptr(), stream,
                                                              bounds=(0.0, 0.0, float(Ww), float(Hh)), scale_factors=sfac)
                    tstep.keep = l_u
                    ps_t.optimize_batch_device(B, cap, kp_.data_ptr(), nn_.data_ptr(), t_assign.data_ptr(), l_mp.data_ptr(), cap, t_pose0.data_ptr(), isig_t, cam_t,
                                               t_pose.data_ptr(), t_inl.data_ptr(), t_outl.data_ptr(), stream)
                    if mode != "one":
                        cur_s.wait_event(t_ev_v)
                    t_ev_done[k_].record()

                def time_chain(mode):
                    tstep(mode); tstep(mode); torch.cuda.synchronize()
                    t0_ = time.perf_counter()
                    for _ in range(10):
                        tstep(mode)
                    torch.cuda.synchronize()
                    return (time.perf_counter() - t0_) / 10
                dtt_one = time_chain("one")
                dtt_side = time_chain("side")
                dtt = time_chain("pipe")
                tstep("one"); torch.cuda.synchronize()          # (the legs below read the first set of arrays and the results of a whole step)
                t0 = time.perf_counter()
                for _ in range(10):
                    ps_t.optimize_batch_device(B, cap, d_kps.data_ptr(), d_n.data_ptr(), t_assign.data_ptr(), l_mp.data_ptr(), cap, t_pose0.data_ptr(), isig_t, cam_t,
                                               t_pose.data_ptr(), t_inl.data_ptr(), t_outl.data_ptr(), stream)
                torch.cuda.synchronize()
                dtp_dev = (time.perf_counter() - t0) / 10
                out["tracking"] = {"metric": "tracking chain frames/s (extract + DBoW2 transform + SearchByProjection(last frame) + PoseOptimization)",
                                   "value": B / dtt, "unit": "frames/s", "ms_per_batch": 1e3 * dtt, "ms_per_batch_one_stream": 1e3 * dtt_one,
                                   "ms_per_batch_transform_beside": 1e3 * dtt_side,
                                   "projection_matches_per_frame": float(t_nm.float().mean().item()),
                                   "pose_inliers_per_frame": float(t_inl.float().mean().item()), "pose_device_entry_ms_per_batch": 1e3 * dtp_dev,
                                   "pose_translation_error_after": float(t_pose[:, 4:].abs().max().item()),
                                   "workload": "%d streams: current frame = last frame moved by 3 px; search and PoseOptimization run on the extractor's device "
                                               "arrays (edges gathered on the device from the search's assignment), nothing visits the host. Two batches in flight: the "
                                               "extraction of batch k+1 runs beside the transform / search / PoseOptimization of batch k (ms_per_batch_one_stream: all four "
                                               "in a row; ms_per_batch_transform_beside: only the transform on a side stream)" % B}
                # ---- TrackLocalMap's device work (src/Tracking.cc:3082-3115: SearchLocalPoints -> SearchByProjection(Frame, vpMapPoints, th),
                # "the dominant matcher call in steady-state tracking", SURVEY M4 -> PoseOptimization): the current frames as the chain above
                # left them; the local map of a stream = the last frame's points plus as many again seen nearby (the same descriptors at
                # positions a few pixels off: the ratio test and the best-level bookkeeping have work to do), 2 x cap points per frame ----
                try:
                    pcap_l = 2 * cap
                    jit = torch.Generator(device=dev); jit.manual_seed(9)
                    off_u = torch.rand(B, cap, device=dev, generator=jit) * 8.0 - 4.0
                    m_u = torch.cat([lk[:, :, 0] + 3.0, lk[:, :, 0] + 3.0 + off_u], 1).contiguous()
                    m_v = torch.cat([lk[:, :, 1], lk[:, :, 1] + off_u.flip(1)], 1).contiguous()
                    m_lvl = torch.cat([l_oct, l_oct], 1).contiguous()
                    m_desc = torch.cat([l_desc.view(B, cap, 32), l_desc.view(B, cap, 32)], 1).contiguous()
                    m_valid = torch.cat([l_valid, l_valid], 1).contiguous()
                    # the points of frame b are packed [0, l_n[b]) + [cap, cap + l_n[b]): mark the gap invalid instead of compacting
                    m_n = torch.full_like(l_n, pcap_l)
                    m_cos = torch.full((B, pcap_l), 0.999, dtype=torch.float32, device=dev)
                    m_depth = torch.cat([l_z, l_z], 1).contiguous()
                    m_bad = torch.zeros(B, pcap_l, dtype=torch.uint8, device=dev); m_obs = torch.ones(B, pcap_l, dtype=torch.uint8, device=dev)
                    m_xyz = torch.cat([l_mp, l_mp], 1).contiguous()
                    ml = pkg.Matcher(0.8, True, device=local_rank)
                    lm_assign = torch.empty(B * cap, dtype=torch.int32, device=dev); lm_occ = torch.empty(B * cap, dtype=torch.uint8, device=dev)
                    lm_nm = torch.zeros(B, dtype=torch.int32, device=dev)

                    def lstep():
                        lm_assign.fill_(-1); lm_occ.zero_()
                        ml.SearchByProjection_batch_device((d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), cap),
                                                           (m_valid.data_ptr(), m_u.data_ptr(), m_v.data_ptr(), m_lvl.data_ptr(), 0, m_desc.data_ptr(), m_n.data_ptr(), pcap_l, m_obs.data_ptr()),
                                                           (m_cos.data_ptr(), m_depth.data_ptr(), m_bad.data_ptr()), B, 1.0, lm_assign.data_ptr(), lm_occ.data_ptr(), lm_nm.data_ptr(),
                                                           stream, bounds=(0.0, 0.0, float(Ww), float(Hh)), scale_factors=sfac)
                        ps_t.optimize_batch_device(B, cap, d_kps.data_ptr(), d_n.data_ptr(), lm_assign.data_ptr(), m_xyz.data_ptr(), pcap_l, t_pose0.data_ptr(), isig_t, cam_t,
                                                   t_pose.data_ptr(), t_inl.data_ptr(), t_outl.data_ptr(), stream)
                    lstep(); torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(10):
                        lstep()
                    torch.cuda.synchronize()
                    dtl = (time.perf_counter() - t0) / 10
                    out["track_local_map"] = {"metric": "TrackLocalMap device work frames/s (SearchByProjection(Frame, MapPoints) + PoseOptimization, device-resident)",
                                              "value": B / dtl, "unit": "frames/s", "ms_per_batch": 1e3 * dtl, "local_map_points_per_frame": int(pcap_l),
                                              "matches_per_frame": float(lm_nm.float().mean().item()), "pose_inliers_per_frame": float(t_inl.float().mean().item()),
                                              "workload": "%d streams x %d local map points (th 1, nnratio 0.8, ratio and level tests), then PoseOptimization on the matches" % (B, pcap_l)}
                    ml.close()
                except Exception as e:  # noqa: BLE001
                    out["track_local_map"] = {"error": repr(e)}
                mtrk.close(); ps_t.close()
            except Exception as e:  # noqa: BLE001
                out["tracking"] = {"error": repr(e)}
            out["chain"] = {"metric": "device-resident front end frames/s (extract + DBoW2 transform + SearchByBoW vs previous frame)",
                            "value": B / dtc_, "unit": "frames/s", "ms_per_batch": 1e3 * dtc_,
                            "bow_matches_per_pair": float(c_nm.float().mean().item()), "workload": "%d frames = %d consecutive pairs" % (B, B // 2)}
            cplan.close()
            out["vocab"] = {"metric": "DBoW2 transform frames/s", "value": B / dtv, "unit": "frames/s", "dtype": "u8/f64",
                            "workload": "%d frames x %.0f descriptors through a k=10, L=6 tree (1.1 M nodes), levelsup 4, BowVector + FeatureVector" % (B, n_kp),
                            "ms_per_batch": 1e3 * dtv, "words_per_frame": float(v_nb.float().mean().item())}

        # ---- edge-SLAM packet leg (wire format): packets written from / parsed into the device arrays ----
        if args.extra and not args.no_lba:
            codec = pkg.PacketCodec(device=local_rank)
            pstride = (codec.packet_bytes(cap, 0) + 3) & ~3
            p_pay = torch.zeros(B * pstride, dtype=torch.uint8, device=dev)
            p_len, p_st, p_n2, p_ni, p_st2 = (torch.zeros(B, dtype=torch.int32, device=dev) for _ in range(5))
            p_fid = torch.arange(B, dtype=torch.int32, device=dev); p_ts = torch.arange(B, dtype=torch.int64, device=dev) * 50000000
            p_f2 = torch.zeros_like(p_fid); p_t2 = torch.zeros_like(p_ts)
            p_k2 = torch.zeros(B * cap * 28, dtype=torch.uint8, device=dev); p_d2 = torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev)

            def pk_pack():
                codec.pack_batch_device(d_kps.data_ptr(), d_desc.data_ptr(), d_n.data_ptr(), B, cap, p_fid.data_ptr(), p_ts.data_ptr(), 0, 0,
                                        p_pay.data_ptr(), pstride, p_len.data_ptr(), 0, p_st.data_ptr(), stream)

            def pk_unpack():
                codec.unpack_batch_device(p_pay.data_ptr(), pstride, p_len.data_ptr(), B, cap, 0, p_k2.data_ptr(), p_d2.data_ptr(), p_n2.data_ptr(),
                                          p_f2.data_ptr(), p_t2.data_ptr(), 0, p_ni.data_ptr(), p_st2.data_ptr(), stream)
            pk_pack(); pk_unpack(); torch.cuda.synchronize()
            tms = []
            for fn in (pk_pack, pk_unpack):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()                              # `stream` is torch's current stream: the events bracket the launches
                for _ in range(20):
                    fn()
                e1.record()
                torch.cuda.synchronize()
                tms.append(e0.elapsed_time(e1) / 20)
            pts_total = float(d_n.sum().item())
            ok = bool((p_st == 0).all().item() and (p_st2 == 0).all().item() and torch.equal(p_n2, d_n))
            out["packets"] = {"metric": "edge-SLAM packets (SlamPktVI) frames/s, device-resident", "unit": "frames/s", "dtype": "u8",
                              "pack": {"value": B / (1e-3 * tms[0]), "ms_per_batch": tms[0], "GBps": pts_total * 76 / (1e6 * tms[0])},
                              "unpack": {"value": B / (1e-3 * tms[1]), "ms_per_batch": tms[1], "GBps": pts_total * 96 / (1e6 * tms[1])},
                              "round_trip_ok": ok,
                              "workload": "%d frames x %.0f key points: 16 B + 36 B/point packets written from the extractor's device arrays "
                                          "(40 B read + 36 B written per point) and parsed back (36 B read + 60 B written per point)" % (B, n_kp)}
            codec.close()

        # ---- map-point upkeep leg: ComputeDistinctiveDescriptors + UpdateNormalAndDepth for the points of one BA window ----
        if args.extra and not args.no_lba:
            rs_ = np.random.RandomState(11)
            Pm = 2000; cnt_ = rs_.randint(2, 21, Pm); moff = np.concatenate([[0], np.cumsum(cnt_)]).astype(np.int32)
            mdesc = np.repeat(rs_.randint(0, 256, (Pm, 32)).astype(np.uint8), cnt_, axis=0) ^ np.packbits(rs_.uniform(size=(moff[-1], 256)) < 0.08, axis=1)
            mpos = rs_.uniform(-5, 5, (Pm, 3)).astype(np.float32)
            mcen = (np.repeat(mpos, cnt_, axis=0) + rs_.normal(0, 4, (moff[-1], 3))).astype(np.float32)
            mls = (np.float32(1.2) ** rs_.randint(0, 8, Pm)).astype(np.float32)
            mm = pkg.Matcher(device=local_rank)
            mm.DistinctiveDescriptors(mdesc, moff); mm.UpdateNormalAndDepth(mpos, mcen, moff, mcen[moff[:-1]], mls, 3.58)
            t0 = time.perf_counter()
            for _ in range(10):
                mm.DistinctiveDescriptors(mdesc, moff)
            dtd = (time.perf_counter() - t0) / 10
            t0 = time.perf_counter()
            for _ in range(10):
                mm.UpdateNormalAndDepth(mpos, mcen, moff, mcen[moff[:-1]], mls, 3.58)
            dtn = (time.perf_counter() - t0) / 10
            out["map_points"] = {"metric": "map points/s (host buffers in/out)", "unit": "points/s",
                                 "distinctive_descriptors": {"value": Pm / dtd, "ms_per_call": 1e3 * dtd},
                                 "normal_and_depth": {"value": Pm / dtn, "ms_per_call": 1e3 * dtn},
                                 "workload": "%d map points, 2-20 observations each (%d descriptors)" % (Pm, int(moff[-1]))}
            mm.close()

        # ---- visual-inertial local BA leg: Optimizer::LocalInertialBA's numerical core, one window per call ----
        if args.extra and not args.no_lba:
            iw, _ = synth.make_inertial_window(0, n_opt=10, n_points=800, obs_per_point=6, n_covisible_fixed=10)
            isol = pkg.InertialSolver(device=local_rank)
            ri = isol.solve(iw)
            t0 = time.perf_counter()
            for _ in range(5):
                ri = isol.solve(iw)
            dti = (time.perf_counter() - t0) / 5
            out["inertial_ba"] = {"metric": "LocalInertialBA outer iterations/s (one call = structure build + upload + iterations + download)",
                                  "value": ri["stats"]["iterations"] / dti, "unit": "iters/s", "dtype": "f64", "ms_per_call": 1e3 * dti,
                                  "iterations_per_solve": ri["stats"]["iterations"], "trials_per_solve": ri["stats"]["trials"],
                                  "workload": "10 temporal key frames (15 unknowns each) + 1 fixed + 10 covisible fixed, 800 map points, %d mono edges, "
                                              "10 inertial links, optimize(10), lambda 1" % len(iw["edge_kf"]),
                                  "chi2_initial": ri["stats"]["chi2_initial"], "chi2_final": ri["stats"]["chi2_final"]}
            isol.close()
            # many windows per launch (liba_solve_batch): 32 windows of that size, one per client session
            ib = pkg.LibaBatch(device=local_rank)
            iws = [synth.make_inertial_window(i, n_opt=10, n_points=800, obs_per_point=6, n_covisible_fixed=10)[0] for i in range(32)]
            ipre = ib.prepare(iws)
            ib.run(ipre); ib.run(ipre)
            t0 = time.perf_counter(); its_b = 0; dev_b = 0.0
            for _ in range(3):
                its_b += sum(x["stats"]["iterations"] for x in ib.run(ipre)); dev_b += ib.last_device_ms()
            dtb = time.perf_counter() - t0
            out["inertial_ba"]["batched"] = {"windows": 32, "value": its_b / dtb, "unit": "iters/s (whole C call)", "ms_per_call": 1e3 * dtb / 3,
                                             "device_rounds_iters_per_s": its_b / (dev_b * 1e-3), "device_ms_per_call": dev_b / 3}
            ib.close()

        # ---- per-frame inertial optimisation leg: Optimizer::PoseInertialOptimizationLastKeyFrame for a batch of frames (one per stream) ----
        if args.extra and not args.no_lba:
            pi_ws = [synth.make_pose_inertial_problem(100 + i, n=300, outlier_frac=0.1)[0] for i in range(16)] * (B // 16)
            isol2 = pkg.InertialSolver(device=local_rank)
            qpi = isol2.pose_prepare(pi_ws)
            isol2.pose_launch(qpi)
            t0 = time.perf_counter()
            isol2.pose_launch(qpi)
            dtpi = time.perf_counter() - t0
            rpi = isol2.pose_results(qpi)
            q1 = isol2.pose_prepare(pi_ws[:1])
            isol2.pose_launch(q1)
            dtp1 = median_call_seconds(lambda: isol2.pose_launch(q1), 15)
            out["pose_inertial"] = {"metric": "PoseInertialOptimizationLastKeyFrame frames/s", "value": len(pi_ws) / dtpi, "unit": "frames/s", "dtype": "f64",
                                    "ms_per_batch": 1e3 * dtpi, "single_frame_call_ms": 1e3 * dtp1,
                                    "workload": "%d frames x 300 mono edges + inertial link, 10%% gross outliers, 4 rounds x 10 Gauss-Newton iterations; one C call = "
                                                "one copy in + one launch (a workgroup per frame) + one copy out" % len(pi_ws),
                                    "inliers_per_frame": float(np.mean([r_["inliers"] for r_ in rpi]))}
            # the last-frame variant (previous frame free, EdgePriorPoseImu, 30 unknowns): what the tracker calls on most frames
            pl_ws = [synth.make_pose_inertial_problem(200 + i, n=300, outlier_frac=0.1, last_frame=True)[0] for i in range(16)] * (B // 16)
            qpl = isol2.pose_prepare(pl_ws)
            isol2.pose_launch(qpl)
            t0 = time.perf_counter()
            isol2.pose_launch(qpl)
            dtpl = time.perf_counter() - t0
            ql1 = isol2.pose_prepare(pl_ws[:1])
            isol2.pose_launch(ql1)
            dtl1 = median_call_seconds(lambda: isol2.pose_launch(ql1), 15)
            out["pose_inertial"]["last_frame_variant"] = {"value": len(pl_ws) / dtpl, "unit": "frames/s", "ms_per_batch": 1e3 * dtpl, "single_frame_call_ms": 1e3 * dtl1}
            isol2.close()

        # ---- CPU baseline leg (N=1 only, rank 0) ----
        if not args.no_cpu and world == 1:
            o, cb = cpu_baseline(synth, host_imgs, match_sets)
            out["cpu_baseline"] = cb
            out["speedup_vs_cpu_1core"] = value / cb["value"]
            # one independent stream per host core (the reference is single-threaded per stream), as child processes
            try:
                import subprocess
                ncores = min(os.cpu_count() or 1, 16)
                native = os.path.join(ROOT, "oracle", "liborb_oracle_native.so")
                procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "oracle_worker.py"), "6",
                                           native if os.path.exists(native) else ""], stdout=subprocess.PIPE, text=True)
                         for _ in range(ncores)]
                tot = 0.0
                for pr in procs:
                    o_, _ = pr.communicate(timeout=120)
                    nf, dt_ = o_.split()
                    tot += float(nf) / float(dt_)
                out["cpu_baseline_all_cores"] = {"value": tot, "unit": "frames/s", "cores": ncores, "kind": "port",
                                                 "sample": "%d independent single-threaded streams, 6 s each" % ncores}
                out["speedup_vs_cpu_all_cores"] = value / tot
            except Exception as e:
                out["cpu_baseline_all_cores"] = {"error": repr(e)}
            if "lba" in out:
                w = synth.make_ba_window(0)
                t0 = time.perf_counter(); it = 0
                for _ in range(3):
                    it += o.lba_solve(w, 10)["stats"]["iterations"]
                dtc = time.perf_counter() - t0
                out["lba"]["cpu_baseline"] = {"value": it / dtc, "unit": "iters/s", "cores": 1, "kind": "port",
                                              "sample": "3 solves of the same window, %d iterations" % it}
                out["lba"]["speedup_vs_cpu_1core"] = out["lba"]["value"] / (it / dtc)
            if "proj" in out:
                t0 = time.perf_counter()
                for (g, dF, aF, sc, last, a, o_) in pcases[:16]:
                    o.search_by_projection_last(g, dF, aF, sc, last, 15.0, True, np.full_like(a, -1), np.zeros_like(o_))
                dtc = (time.perf_counter() - t0) / 16
                out["proj"]["cpu_baseline"] = {"value": 1.0 / dtc, "unit": "frames/s", "cores": 1, "kind": "port", "sample": "16 frames"}
                out["proj"]["speedup_vs_cpu_1core"] = out["proj"]["value"] * dtc
            if "vocab" in out:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from oracle_api import oracle_transform
                hd = d_desc.cpu().numpy().reshape(B, cap, 32)
                nk_now = d_n.cpu().numpy()              # (the chain leg re-used the extractor's output buffers)
                t0 = time.perf_counter()
                for b_ in range(8):
                    oracle_transform(o, voc, hd[b_, :int(nk_now[b_])], 4)
                dtc = (time.perf_counter() - t0) / 8
                out["vocab"]["cpu_baseline"] = {"value": 1.0 / dtc, "unit": "frames/s", "cores": 1, "kind": "port", "sample": "8 frames"}
                out["vocab"]["speedup_vs_cpu_1core"] = out["vocab"]["value"] * dtc
            if "pose" in out:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from oracle_api import oracle_pose_optimize
                t0 = time.perf_counter()
                for wp in pose_ws[:64]:
                    oracle_pose_optimize(o, wp)
                dtc = time.perf_counter() - t0
                out["pose"]["cpu_baseline"] = {"value": 64 / dtc, "unit": "frames/s", "cores": 1, "kind": "port", "sample": "64 frames"}
                out["pose"]["speedup_vs_cpu_1core"] = out["pose"]["value"] / (64 / dtc)
            if "pose_inertial" in out:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from oracle_api import oracle_pose_inertial_optimize
                t0 = time.perf_counter()
                for wp in pi_ws[:32]:
                    oracle_pose_inertial_optimize(o, wp)
                dtc = time.perf_counter() - t0
                out["pose_inertial"]["cpu_baseline"] = {"value": 32 / dtc, "unit": "frames/s", "cores": 1, "kind": "port", "sample": "32 frames (incl. the Python-side packing)"}
                out["pose_inertial"]["speedup_vs_cpu_1core"] = out["pose_inertial"]["value"] / (32 / dtc)
                t0 = time.perf_counter()
                for wp in pl_ws[:32]:
                    oracle_pose_inertial_optimize(o, wp)
                dtl = time.perf_counter() - t0
                out["pose_inertial"]["last_frame_variant"]["cpu_baseline"] = {"value": 32 / dtl, "unit": "frames/s", "cores": 1, "kind": "port",
                                                                               "sample": "32 frames (incl. the Python-side packing)", "ms_per_frame": 1e3 * dtl / 32}
            if "inertial_ba" in out:
                sys.path.insert(0, os.path.join(ROOT, "tests"))
                from oracle_api import oracle_inertial_solve
                t0 = time.perf_counter()
                for _ in range(3):
                    rc = oracle_inertial_solve(o, iw)
                dtc = (time.perf_counter() - t0) / 3
                out["inertial_ba"]["cpu_baseline"] = {"value": rc["stats"]["iterations"] / dtc, "unit": "iters/s", "cores": 1, "kind": "port",
                                                      "sample": "3 solves of the same window"}
                out["inertial_ba"]["speedup_vs_cpu_1core"] = out["inertial_ba"]["value"] / (rc["stats"]["iterations"] / dtc)
                if "batched" in out["inertial_ba"]:
                    out["inertial_ba"]["batched"]["speedup_vs_cpu_1core"] = out["inertial_ba"]["batched"]["value"] / (rc["stats"]["iterations"] / dtc)

    # ---- stereo streams: two extractions per frame with vLappingArea = {0, 0} (src/Frame.cc:122-125, two
    # ORBextractor instances) + Frame::ComputeStereoMatches, B/2 rectified pairs per GPU, sharded like the mono frames ----
    if args.full and (world > 1 or args.extra) and not args.no_lba:
        Bs = B // 2
        exL = pkg.Extractor(1000, 1.2, 8, 20, 7, device=local_rank)
        exR = pkg.Extractor(1000, 1.2, 8, 20, 7, device=local_rank)
        d_left = d_imgs[:Bs]
        d_right = torch.roll(d_left, -12, dims=2).contiguous()          # the same scene 12 px to the left: a constant disparity
        so = []
        for _ in range(2):
            so.append(dict(kps=torch.zeros(Bs * cap * 28, dtype=torch.uint8, device=dev), desc=torch.zeros(Bs * cap * 32, dtype=torch.uint8, device=dev),
                           n=torch.zeros(Bs, dtype=torch.int32, device=dev), mono=torch.zeros(Bs, dtype=torch.int32, device=dev),
                           st=torch.zeros(Bs, dtype=torch.int32, device=dev)))
        d_ur = torch.zeros(Bs * cap, dtype=torch.float32, device=dev); d_dp = torch.zeros(Bs * cap, dtype=torch.float32, device=dev)

        def sstep():
            for e_, im, o_ in ((exL, d_left, so[0]), (exR, d_right, so[1])):
                e_.extract_batch_device(im.data_ptr(), Bs, Ww, Hh, Ww, Ww * Hh, o_["kps"].data_ptr(), o_["desc"].data_ptr(), cap,
                                        o_["n"].data_ptr(), o_["mono"].data_ptr(), o_["st"].data_ptr(), (0, 0), stream)
            exL.stereo_matches_device(exR, Bs, so[0]["kps"].data_ptr(), so[0]["desc"].data_ptr(), so[0]["n"].data_ptr(),
                                      so[1]["kps"].data_ptr(), so[1]["desc"].data_ptr(), so[1]["n"].data_ptr(), cap, 0.11, 47.9,
                                      d_ur.data_ptr(), d_dp.data_ptr(), stream)
        for _ in range(2):
            sstep()
        torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(10):
            sstep()
        torch.cuda.synchronize(); barrier(); torch.cuda.synchronize()
        dts = time.perf_counter() - t0
        if dist is not None:
            tt = torch.tensor([dts], dtype=torch.float64, device=dev)
            dist.all_reduce(tt, op=dist.ReduceOp.MAX)
            dts = float(tt.item())
        if rank == 0:
            matched = float((d_ur.view(Bs, cap) >= 0).sum(1).float().mean().item())
            out["stereo"] = {"metric": "stereo frames/s (2 x ORB extract with vLappingArea {0,0} + ComputeStereoMatches)", "value": world * Bs * 10 / dts,
                             "unit": "stereo frames/s", "ms_per_step": 1e3 * dts / 10, "pairs_per_gpu_step": Bs, "n_gpus": world,
                             "stereo_matches_per_frame": matched, "status_ok": bool((so[0]["st"] == 0).all().item() and (so[1]["st"] == 0).all().item())}
        exL.close(); exR.close()

    # ---- sharded global BA with one RCCL all-reduce per LM trial (N>1) ----
    gba_failed = False
    if args.full and world > 1 and not args.no_lba:
        # watchdog: the headline number must survive even if this extra leg ever stalled inside a collective
        import threading

        def _bail():        # a stalled collective must not reach the driver as a successful run: print what we have, then fail
            if rank == 0:
                out["gba"] = {"error": "watchdog: sharded global BA / stereo leg exceeded 240 s"}
                print(json.dumps(compact_line(out)), flush=True)
            os._exit(3)
        wd = threading.Timer(240.0, _bail)
        wd.daemon = True
        wd.start()
        try:
            # one sharded global BA of 500 poses / 20 k points / 200 k edges (69 MB reduce buffer per trial)
            wg = synth.make_ba_window(3, n_opt=490, n_fixed=10, n_points=20000, obs_per_point=10)
            wg["huber_mono"] = 0.0; wg["huber_stereo"] = 0.0        # loop closing: bRobust = false (src/LoopClosing.cc:2288)
            loc, _, _ = dmod.partition_landmarks(wg, rank, world)
            sh = pkg.LbaShard(loc, device=local_rank)
            ad = dmod.HipShard(sh, torch, dev)
            comm = dmod.TorchDist(dist, dev)
            dist.barrier(); torch.cuda.synchronize()
            t0 = time.perf_counter()
            gs = dmod.sharded_bundle_adjustment(ad, ad.tensor, comm, max_iters=5)
            torch.cuda.synchronize()
            dtg = time.perf_counter() - t0
            if rank == 0:
                ar_s = comm.allreduce_seconds
                ar_bytes = int(ad.n_red * 8)
                # ring-free bound of a sum over G peers on point-to-point xGMI: reduce-scatter + all-gather moves 2 (G-1)/G of the
                # buffer per GPU over its 7 links
                ar_gbs = (2.0 * (world - 1) / world) * ar_bytes * gs["trials"] / max(ar_s, 1e-9) / 1e9 if ar_s else None
                out["gba"] = {"workload": "500 KF (490 free) / 20000 MP / %d edges, no robust kernel, landmarks sharded over %d GPUs, optimize(5)" % (len(wg["edge_point"]), world),
                              "allreduce_bytes_per_trial": ar_bytes, "iterations": gs["iterations"], "trials": gs["trials"],
                              "seconds": dtg, "iters_per_s": gs["iterations"] / dtg, "chi2_initial": gs["chi2_initial"], "chi2_final": gs["chi2_final"],
                              "roofline": {"bound": "xgmi", "achieved": ar_gbs, "peak": XGMI_PEAK_GBS, "unit": "GB/s",
                                           "frac": (ar_gbs / XGMI_PEAK_GBS) if ar_gbs else None,
                                           "allreduce_seconds_total": ar_s, "note": "device time of the all-reduces (events on the collective's stream)"}}
            sh.close()
            # the same solve through the C-ABI driver (lba_shard_optimize + all-reduce callback; a C++ host passes ncclAllReduce).
            # The callback wraps the library's raw device pointers as tensors: every rank first checks locally that this works
            # and the ranks agree (MIN) before any of them enters the collective loop.
            cb2, ok_local = None, 1.0
            try:
                cb2 = dmod.rccl_allreduce(dist, torch, dev) if backend_is_nccl else dmod.host_staged_allreduce(dist, torch)
                if backend_is_nccl:
                    probe = torch.arange(4, dtype=torch.float64, device=dev)
                    ok_local = 1.0 if dmod.wrap_device_doubles(torch, probe.data_ptr(), 4, dev).sum().item() == 6.0 else 0.0
            except Exception as e:  # noqa: BLE001
                log("rank %d: C-ABI driver leg unavailable: %r" % (rank, e))
                ok_local = 0.0
            okt = torch.tensor([ok_local], dtype=torch.float64, device=dev if backend_is_nccl else "cpu")
            dist.all_reduce(okt, op=dist.ReduceOp.MIN)
            if okt.item() > 0.5:
                sh2 = pkg.LbaShard(loc, device=local_rank)
                dist.barrier(); torch.cuda.synchronize()
                t0 = time.perf_counter()
                cs = sh2.optimize(cb2, world, max_iters=5)
                torch.cuda.synchronize()
                dtc2 = time.perf_counter() - t0
                if rank == 0:
                    out["gba"]["c_abi_driver"] = {"iterations": cs["iterations"], "trials": cs["trials"], "seconds": dtc2, "chi2_final": cs["chi2_final"],
                                                  "iters_per_s": cs["iterations"] / dtc2,
                                                  "same_path_as_python_driver": (cs["iterations"], cs["trials"]) == (gs["iterations"], gs["trials"])}
                sh2.close()
            elif rank == 0:
                out["gba"]["c_abi_driver"] = {"skipped": "raw device pointers could not be wrapped as tensors on some rank"}
        except Exception as e:     # the frame-sharded headline number stands on its own, but the run is reported as failed
            gba_failed = True
            log("rank %d: sharded global BA failed: %r" % (rank, e))
            if rank == 0:
                out["gba"] = {"error": repr(e)}
        wd.cancel()

    if rank == 0:
        detail = None
        if args.full:
            dpath = args.detail or os.path.join(ROOT, "bench_out", "bench_detail.json")
            try:
                os.makedirs(os.path.dirname(os.path.abspath(dpath)), exist_ok=True)
                with open(dpath, "w") as f:
                    json.dump(out, f, indent=1)
                detail = args.detail or "bench_out/bench_detail.json"
            except OSError as e:
                log("could not write %s: %r" % (dpath, e))
        log(json.dumps(out))
        print(json.dumps(compact_line(out, detail)), flush=True)
    plan.close(); matcher.close(); ex.close()
    if dist is not None:
        if gba_failed:
            os._exit(3)         # peers of a failed rank may still sit in a collective: do not wait for them, and do not report success
        try:
            dist.barrier()
            dist.destroy_process_group()
        except Exception:
            pass


if __name__ == "__main__":
    main()
