"""TrackWithMotionModel + TrackLocalMap of two-camera fisheye rig frames as ONE device-resident chain
(include/orbslam3_hip_rig_track_device.h):

  rig frame pose -> last-frame projection -> last-frame search -> PoseOptimization (rig edges) -> hand-over -> rig frame pose
      -> frustum projection -> local-map search -> PoseOptimization (rig edges)

Route A enqueues the nine calls on device arrays and synchronises once at the end.  Route B runs the same chain, but the two
searches and the two pose optimisations go through their host-array entries (download, call, upload).  The two routes must agree
exactly: assign, occupied, counts, outlier flags, the hand-over's outputs, and both poses bit for bit.

The scene: three rig frames whose key points lie (within a pixel) on the true projections of a local map of 200 points, the first 120
of which are the last frame's points; the chain starts from a pose a little off the true one.  Measured on the host route: at least
20 last-frame matches and at least 10 inliers in both pose calls per frame (asserted below, so that the comparison is not vacuous)."""
import numpy as np
import pytest

import rig_match_cases as MC
import rig_track_device_pack as DP
import track_project_rig_cases as TC
import track_project_rig_reference as RR

pytestmark = pytest.mark.gpu

F32 = np.float32
B, PCAP, LAST_CAP, N_NOISE, SLOT_EXTRA = 3, 200, 120, 60, 6
TH_LAST, TH_MAP, N_LEVELS = 15.0, 1.0, 8
SCALE = (F32(1.2) ** np.arange(N_LEVELS)).astype(F32)
INV_SIGMA2 = (1.0 / SCALE.astype(np.float64) ** 2).astype(F32)
HUBER = float(F32(np.sqrt(5.991)))
FRUSTUM_OUT = TC.ST.RIG_STATE
LAST_OUT = (("valid", np.uint8), ("proj_u", F32), ("proj_v", F32), ("proj_u_r", F32), ("proj_v_r", F32))


def build_scene(seed=7):
    """everything both routes start from, as numpy arrays (no GPU)"""
    rng = np.random.default_rng(seed)
    cam = TC.ST.rig_camera(yaw=0.8)
    w, h = float(cam["max_x"]), float(cam["max_y"])
    true = TC.ST.make_poses(seed + 50, B, unnormalised_every=0)
    case = TC.ST.make_rig_local_map_case(seed + 1, B, PCAP, cam=cam, poses=true, full=True)
    case["skip"][:] = 0
    ref = RR.frustum(case, state=case["state"])
    last_case = dict(cam=cam, pose7=true, xyz=np.ascontiguousarray(case["xyz"][:, :LAST_CAP]), n=np.full(B, LAST_CAP, np.int32),
                     has_point=(rng.random((B, LAST_CAP)) < 0.9).astype(np.uint8))
    lref = RR.project_last(last_case)
    desc = rng.integers(0, 256, (B, PCAP, 32)).astype(np.uint8)
    has_obs = (rng.random((B, PCAP)) < 0.85).astype(np.uint8)
    octave = np.where(ref["in_view"] != 0, ref["pred_level"], np.where(ref["in_view_r"] != 0, ref["pred_level_r"], rng.integers(0, 4, (B, PCAP)))).astype(np.int32)
    octave = np.clip(octave, 0, N_LEVELS - 1)
    rigs = []
    for b in range(B):
        l, r = MC.Side(w, h), MC.Side(w, h)
        lv = (lref["valid"][b] != 0)
        for i in range(PCAP):
            d = lambda: MC._noisy(rng, desc[b, i], 20)
            jit = lambda: float(rng.uniform(-1, 1))
            if ref["in_view"][b, i]:
                l.add(float(ref["proj_u"][b, i]) + jit(), float(ref["proj_v"][b, i]) + jit(), d(), int(octave[b, i]), float(rng.uniform(0, 360)))
            elif i < LAST_CAP and lv[i]:
                l.add(float(lref["proj_u"][b, i]) + jit(), float(lref["proj_v"][b, i]) + jit(), d(), int(octave[b, i]), float(rng.uniform(0, 360)))
            if ref["in_view_r"][b, i]:
                r.add(float(ref["proj_u_r"][b, i]) + jit(), float(ref["proj_v_r"][b, i]) + jit(), d(), int(max(ref["pred_level_r"][b, i], 0)), float(rng.uniform(0, 360)))
        for side in (l, r):
            for _ in range(N_NOISE):
                side.add(float(rng.uniform(5, w - 5)), float(rng.uniform(5, h - 5)), rng.integers(0, 256, 32).astype(np.uint8), int(rng.integers(0, 4)), float(rng.uniform(0, 360)))
        rigs.append(MC.make_rig(l, r, scale=SCALE))
    init = true.copy()
    init[:, :4] /= np.linalg.norm(init[:, :4], axis=1)[:, None]
    init[:, :4] += rng.normal(0, 0.002, (B, 4)); init[:, 4:] += rng.normal(0, 0.008, (B, 3))
    init = init.astype(F32).astype(np.float64)
    return dict(cam=cam, case=case, last_case=last_case, desc=desc, has_obs=has_obs, octave=octave, rigs=rigs, init=init, true=true,
                angle=rng.uniform(0, 360, (B, LAST_CAP)).astype(F32), last_local=np.tile(np.arange(LAST_CAP, dtype=np.int32), (B, 1)))


def solver_rig(cam):
    c = lambda p: dict(fx=float(p[0]), fy=float(p[1]), cx=float(p[2]), cy=float(p[3]), k=[float(v) for v in p[4:8]])
    return dict(left=c(cam["left"]), right=c(cam["right"]), q_rl=np.asarray(cam["q_rl"], np.float64), t_rl=np.asarray(cam["trl"], np.float64))


def slot_problems(S, assign, xyz, pose):
    """the PoseProblems of the batch from assign [B][slot_cap] in slot order, and the slot of every edge"""
    probs, slots = [], []
    for b, rig in enumerate(S["rigs"]):
        L, R = rig["left"], rig["right"]
        nl, nr = len(L["x"]), len(R["x"])
        s = np.nonzero((assign[b, :nl + nr] >= 0) & (assign[b, :nl + nr] < xyz.shape[1]))[0]
        x, y, oc = (np.concatenate([L[k], R[k]])[s] for k in ("x", "y", "octave"))        # right slot j sits at nl + j
        probs.append(dict(q=pose[b, :4], t=pose[b, 4:], Xw=xyz[b][assign[b, s]].astype(np.float64).reshape(-1, 3),
                          obs=np.stack([x.astype(F32), y.astype(F32), np.full(len(s), -1.0, F32)], 1).astype(np.float64).reshape(-1, 3),
                          inv_sigma2=INV_SIGMA2[oc].astype(np.float64), stereo=np.where(s >= nl, 2, 0).astype(np.uint8),
                          fx=0.0, fy=0.0, cx=0.0, cy=0.0, bf=0.0, huber_mono=HUBER, huber_stereo=0.0))
        slots.append(s)
    return probs, slots


class Chain:
    def __init__(self, pkg, torch, S):
        self.pkg, self.torch, self.S = pkg, torch, S
        self.dev = torch.device("cuda", 0)
        self.st = torch.cuda.current_stream().cuda_stream
        rigs = S["rigs"]
        self.nl, self.nr = [len(r["left"]["x"]) for r in rigs], [len(r["right"]["x"]) for r in rigs]
        self.cap_l, self.cap_r = max(self.nl), max(self.nr)
        self.slot_cap = self.cap_l + self.cap_r + SLOT_EXTRA
        kl, kr = DP.key_points([r["left"] for r in rigs], self.cap_l, B), DP.key_points([r["right"] for r in rigs], self.cap_r, B)
        dl, dr = np.zeros((B, self.cap_l, 32), np.uint8), np.zeros((B, self.cap_r, 32), np.uint8)
        for b, r in enumerate(rigs):
            dl[b, :self.nl[b]] = r["left"]["desc"]; dr[b, :self.nr[b]] = r["right"]["desc"]
        case = S["case"]
        up = self.up
        self.t = dict(
            kl=up(kl), kr=up(kr), dl=up(dl), dr=up(dr), nl=up(np.array(self.nl, np.int32)), nr=up(np.array(self.nr, np.int32)),
            l2r=up(np.full((B, self.cap_l), -1, np.int32)), r2l=up(np.full((B, self.cap_r), -1, np.int32)),
            init=up(S["init"]), rp=up(np.zeros((B, 43), F32)), rp2=up(np.zeros((B, 43), F32)),
            last_xyz=up(S["last_case"]["xyz"]), has_point=up(S["last_case"]["has_point"]), n_last=up(S["last_case"]["n"]),
            l_octave=up(S["octave"][:, :LAST_CAP]), l_angle=up(S["angle"]), l_obs=up(S["has_obs"][:, :LAST_CAP]), l_desc=up(S["desc"][:, :LAST_CAP]),
            assign=up(np.full((B, self.slot_cap), -1, np.int32)), occ=up(np.zeros((B, self.slot_cap), np.uint8)), nm=up(np.zeros(B, np.int32)), n_slots=up(np.zeros(B, np.int32)),
            pose1=up(np.zeros((B, 7))), inl1=up(np.zeros(B, np.int32)), outl1=up(np.zeros((B, self.slot_cap), np.uint8)),
            last_local=up(S["last_local"]), bad=up(case["bad"]), obs=up(S["has_obs"]), desc=up(S["desc"]),
            assign2=up(np.full((B, self.slot_cap), -9, np.int32)), occ2=up(np.full((B, self.slot_cap), 9, np.uint8)), skip=up(np.full((B, PCAP), 9, np.uint8)),
            dropped=up(np.full(B, -9, np.int32)),
            xyz=up(case["xyz"]), normal=up(case["normal"]), mind=up(case["min_distance"]), maxd=up(case["max_distance"]), n_pts=up(case["n"]),
            n_to_match=up(np.zeros(B, np.int32)), nm2=up(np.zeros(B, np.int32)), n_slots2=up(np.zeros(B, np.int32)),
            pose2=up(np.zeros((B, 7))), inl2=up(np.zeros(B, np.int32)), outl2=up(np.zeros((B, self.slot_cap), np.uint8)))
        for k, dt in LAST_OUT:
            self.t["lp_" + k] = up(np.zeros((B, LAST_CAP), dt))
        for k, dt in FRUSTUM_OUT:
            self.t["fr_" + k] = up(np.asarray(case["state"][k], dt))
        self.shape = dict(assign=(np.int32, (B, self.slot_cap)), occ=(np.uint8, (B, self.slot_cap)), nm=(np.int32, (B,)), n_slots=(np.int32, (B,)),
                          pose1=(np.float64, (B, 7)), inl1=(np.int32, (B,)), outl1=(np.uint8, (B, self.slot_cap)),
                          assign2=(np.int32, (B, self.slot_cap)), occ2=(np.uint8, (B, self.slot_cap)), skip=(np.uint8, (B, PCAP)), dropped=(np.int32, (B,)),
                          nm2=(np.int32, (B,)), n_slots2=(np.int32, (B,)), pose2=(np.float64, (B, 7)), inl2=(np.int32, (B,)), outl2=(np.uint8, (B, self.slot_cap)))
        for k, dt in LAST_OUT:
            self.shape["lp_" + k] = (dt, (B, LAST_CAP))
        for k, dt in FRUSTUM_OUT:
            self.shape["fr_" + k] = (dt, (B, PCAP))

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def down(self, k):
        dt, shape = self.shape[k]
        return self.t[k].cpu().numpy().view(dt).reshape(shape).copy()

    def put(self, k, a):
        self.t[k].copy_(self.up(np.ascontiguousarray(a, self.shape[k][0])))

    def p(self, k):
        return self.t[k].data_ptr()

    def frames(self):
        S, p = self.S, self.p
        g = S["rigs"][0]["left"]
        return dict(d_kps_l=p("kl"), d_desc_l=p("dl"), d_n_l=p("nl"), cap_l=self.cap_l, d_kps_r=p("kr"), d_desc_r=p("dr"), d_n_r=p("nr"), cap_r=self.cap_r,
                    d_left_to_right=p("l2r"), d_right_to_left=p("r2l"), min_x=g["min_x"], min_y=g["min_y"], max_x=g["max_x"], max_y=g["max_y"],
                    grid_cols=g["cols"], grid_rows=g["rows"], scale_factors=SCALE, slot_cap=self.slot_cap)

    def pose_frames(self, assign, xyz, mp_cap, pose):
        p = self.p
        return dict(d_kps_l=p("kl"), d_n_l=p("nl"), cap_l=self.cap_l, d_kps_r=p("kr"), d_n_r=p("nr"), cap_r=self.cap_r, d_assign=p(assign), slot_cap=self.slot_cap,
                    d_mp_xyz=p(xyz), mp_cap=mp_cap, d_pose=p(pose), inv_level_sigma2=INV_SIGMA2, huber_mono=HUBER)

    def host_pose(self, ps, assign, xyz, pose_in, pose_out, inl, outl):
        """download, pose_optimize_batch, upload"""
        self.torch.cuda.synchronize()
        a = self.down(assign)
        probs, slots = slot_problems(self.S, a, xyz, self.t[pose_in].cpu().numpy().view(np.float64).reshape(B, 7))
        res = ps.optimize_batch(probs)
        flags = np.zeros((B, self.slot_cap), np.uint8)
        for b, (r, s) in enumerate(zip(res, slots)):
            flags[b, s] = r["outlier"]
        self.put(pose_out, np.stack([np.concatenate([r["q"], r["t"]]) for r in res])); self.put(inl, [r["inliers"] for r in res]); self.put(outl, flags)

    def host_search(self, m, kind, pts_of, th, assign, occ, nm, n_slots, **kw):
        """download, the host-array batch entry, upload"""
        self.torch.cuda.synchronize()
        a, o = self.down(assign), self.down(occ)
        qs = []
        for b, rig in enumerate(self.S["rigs"]):
            n = self.nl[b] + self.nr[b]
            qs.append(dict(rig=rig, pts=pts_of(b), assign=a[b, :n].copy(), occupied=o[b, :n].copy()))
        ns = m.search_by_projection_last_rig_batch(qs, th) if kind == "last" else m.search_by_projection_rig_batch(qs, th, **kw)
        for b, q in enumerate(qs):
            n = self.nl[b] + self.nr[b]
            a[b, :n] = q["assign"]; o[b, :n] = q["occupied"]
        self.put(assign, a); self.put(occ, o); self.put(nm, ns); self.put(n_slots, [x + y for x, y in zip(self.nl, self.nr)])

    def run(self, m, ps, device_route):
        S, p, st, cam, case = self.S, self.p, self.st, self.S["cam"], self.S["case"]
        m.rig_frame_pose_batch_device(cam, p("init"), B, 1, p("rp"), st)
        m.project_last_rig_batch_device(cam, p("rp"), p("last_xyz"), p("has_point"), p("n_last"), LAST_CAP, tuple(p("lp_" + k) for k, _ in LAST_OUT), B, st)
        if device_route:
            last = dict(d_valid=p("lp_valid"), d_u=p("lp_proj_u"), d_v=p("lp_proj_v"), d_u_r=p("lp_proj_u_r"), d_v_r=p("lp_proj_v_r"), d_octave=p("l_octave"),
                        d_angle=p("l_angle"), d_has_obs=p("l_obs"), d_desc=p("l_desc"), d_n=p("n_last"), cap=LAST_CAP)
            m.search_by_projection_last_rig_batch_device(self.frames(), last, B, TH_LAST, p("assign"), p("occ"), p("nm"), p("n_slots"), st)
            ps.optimize_rig_batch_device(self.pose_frames("assign", "last_xyz", LAST_CAP, "init"), B, p("pose1"), p("inl1"), p("outl1"), None, st)
        else:
            def last_pts(b):
                d = {k: self.down("lp_" + k)[b] for k, _ in LAST_OUT}
                d.update(octave=np.ascontiguousarray(S["octave"][b, :LAST_CAP]), angle=S["angle"][b].copy(), has_obs=np.ascontiguousarray(S["has_obs"][b, :LAST_CAP]),
                         desc=np.ascontiguousarray(S["desc"][b, :LAST_CAP]), n=LAST_CAP, level_window=0)
                return d
            self.host_search(m, "last", last_pts, TH_LAST, "assign", "occ", "nm", "n_slots")
            self.host_pose(ps, "assign", S["last_case"]["xyz"], "init", "pose1", "inl1", "outl1")
        m.track_handover_batch_device(p("assign"), p("outl1"), p("n_slots"), self.slot_cap, p("last_local"), LAST_CAP, p("bad"), p("obs"), PCAP,
                                      p("assign2"), p("occ2"), p("skip"), p("dropped"), B, st)
        m.rig_frame_pose_batch_device(cam, p("pose1"), B, 1, p("rp2"), st)
        m.frustum_rig_batch_device(cam, p("rp2"), (p("xyz"), p("normal"), p("mind"), p("maxd"), p("skip"), p("bad"), p("n_pts"), PCAP), float(case["cos_limit"]),
                                   tuple(p("fr_" + k) for k, _ in FRUSTUM_OUT) + (p("n_to_match"),), B, st)
        if device_route:
            mp = {"d_" + k.replace("proj_", ""): p("fr_" + k) for k, _ in FRUSTUM_OUT if k != "track_depth_r"}
            mp.update(d_bad=p("bad"), d_has_obs=p("obs"), d_desc=p("desc"), d_n=p("n_pts"), cap=PCAP)
            m.search_by_projection_rig_batch_device(self.frames(), mp, B, TH_MAP, p("assign2"), p("occ2"), p("nm2"), p("n_slots2"), st, far_points=True, th_far=20.0)
            ps.optimize_rig_batch_device(self.pose_frames("assign2", "xyz", PCAP, "pose1"), B, p("pose2"), p("inl2"), p("outl2"), None, st)
        else:
            def map_pts(b):
                d = {k: self.down("fr_" + k)[b] for k, _ in FRUSTUM_OUT if k != "track_depth_r"}
                d.update(bad=np.ascontiguousarray(case["bad"][b]), has_obs=np.ascontiguousarray(S["has_obs"][b]), desc=np.ascontiguousarray(S["desc"][b]), n=PCAP)
                return d
            self.host_search(m, "mp", map_pts, TH_MAP, "assign2", "occ2", "nm2", "n_slots2", far_points=True, th_far=20.0)
            self.host_pose(ps, "assign2", case["xyz"], "pose1", "pose2", "inl2", "outl2")
        self.torch.cuda.synchronize()
        return {k: self.down(k) for k in self.shape}


def test_device_route_equals_host_route(pkg):
    torch = pytest.importorskip("torch")
    S = build_scene()
    m, ps = pkg.Matcher(0.8, False), pkg.PoseSolver()         # (random key-point angles: no rotation check)
    try:
        ps.set_rig_kb8(solver_rig(S["cam"]))
        a = Chain(pkg, torch, S).run(m, ps, True)
        b = Chain(pkg, torch, S).run(m, ps, False)
    finally:
        m.close(); ps.close()
    print("host route: last-frame matches %s, inliers %s; local-map writes %s, inliers %s; dropped %s" % (b["nm"], b["inl1"], b["nm2"], b["inl2"], b["dropped"]))
    print("|pose2 - true| per frame: %s" % np.abs(b["pose2"] - np.concatenate([S["true"][:, :4] / np.linalg.norm(S["true"][:, :4], axis=1)[:, None], S["true"][:, 4:]], 1)).max(1))
    assert b["nm"].min() >= 20 and b["inl1"].min() >= 10 and b["inl2"].min() >= 10
    for k in a:
        assert a[k].tobytes() == b[k].tobytes(), "%s differs between the device route and the host route" % k
    assert (a["n_slots"] == a["n_slots2"]).all() and (a["dropped"] == 0).all() and b["nm2"].min() > 0
