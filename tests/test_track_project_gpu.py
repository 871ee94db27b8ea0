"""The projection entries of include/orbslam3_hip_track_project.h on the GPU against tests/track_project_reference.py: frustum and
last-frame projection on the boundary rows and on random cases, the pose conversion, the host-array entries, the hand-over, and the
whole tracking chain with its projections made on the device.  Equality is exact; levels follow the tie rule of
track_project_reference.level_mismatches (device logf and numpy's float32 log may differ in the last bit)."""
import numpy as np
import pytest

import track_project_cases as TC
import track_project_reference as R

pytestmark = pytest.mark.gpu

F32 = np.float32
FRUSTUM_OUT = (("valid", np.uint8), ("u", F32), ("v", F32), ("octave", np.int32), ("view_cos", F32), ("track_depth", F32), ("proj_ur", F32))
LAST_OUT = (("valid", np.uint8), ("u", F32), ("v", F32), ("proj_ur", F32))


class Dev:
    """numpy <-> device buffers (torch only allocates and copies)"""

    def __init__(self):
        self.torch = pytest.importorskip("torch")
        self.dev = self.torch.device("cuda", 0)
        self.stream = self.torch.cuda.current_stream().cuda_stream

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def zeros(self, count, dtype, fill=0):
        return self.up(np.full(count, fill, dtype))

    def down(self, t, dtype, shape):
        return t.cpu().numpy().view(dtype).reshape(shape).copy()

    def sync(self):
        self.torch.cuda.synchronize()


def device_frustum(D, m, case, normalise=1):
    """orbm_frame_pose_batch_device + orbm_frustum_batch_device -> (pose records [B][19], outputs).  The output buffers start as 0x5a
    bytes: every row must be written."""
    B, pcap = case["skip"].shape
    d_pose = D.up(np.asarray(case["pose7"], np.float64)); d_fp = D.zeros(B * 19, F32)
    ins = [D.up(np.asarray(case[k], F32)) for k in ("xyz", "normal", "min_distance", "max_distance")] + \
          [D.up(np.asarray(case[k], np.uint8)) for k in ("skip", "bad")] + [D.up(np.asarray(case["n"], np.int32))]
    outs = [D.zeros(B * pcap * np.dtype(dt).itemsize, np.uint8, 0x5a) for _, dt in FRUSTUM_OUT] + [D.zeros(B * 4, np.uint8, 0x5a)]
    m.frame_pose_batch_device(d_pose.data_ptr(), B, normalise, d_fp.data_ptr(), D.stream)
    m.frustum_batch_device(case["cam"], d_fp.data_ptr(), tuple(t.data_ptr() for t in ins) + (pcap,), float(case["cos_limit"]),
                           tuple(t.data_ptr() for t in outs), B, D.stream)
    D.sync()
    out = {k: D.down(t, dt, (B, pcap)) for (k, dt), t in zip(FRUSTUM_OUT, outs)}
    out["n_to_match"] = D.down(outs[-1], np.int32, (B,))
    return D.down(d_fp, F32, (B, 19)), out


def device_last(D, m, case, normalise=1):
    B, cap = case["has_point"].shape
    d_pose = D.up(np.asarray(case["pose7"], np.float64)); d_fp = D.zeros(B * 19, F32)
    d_xyz, d_has, d_n = D.up(np.asarray(case["xyz"], F32)), D.up(np.asarray(case["has_point"], np.uint8)), D.up(np.asarray(case["n"], np.int32))
    outs = [D.zeros(B * cap * np.dtype(dt).itemsize, np.uint8, 0x5a) for _, dt in LAST_OUT]
    m.frame_pose_batch_device(d_pose.data_ptr(), B, normalise, d_fp.data_ptr(), D.stream)
    m.project_last_batch_device(case["cam"], d_fp.data_ptr(), d_xyz.data_ptr(), d_has.data_ptr(), d_n.data_ptr(), cap, tuple(t.data_ptr() for t in outs), B, D.stream)
    D.sync()
    return D.down(d_fp, F32, (B, 19)), {k: D.down(t, dt, (B, cap)) for (k, dt), t in zip(LAST_OUT, outs)}


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.Matcher(0.8, True)
    yield m
    m.close()


def test_frustum_parity(matcher):
    D = Dev()
    case = TC.frustum_boundary_case()
    rec, out = device_frustum(D, matcher, case)
    ref = R.frustum(case)
    np.testing.assert_array_equal(rec, R.frame_pose_record(R.frame_pose(case["pose7"], 1)))
    TC.check_frustum_boundary_rows(out, case)           # the hand-built rows: exact, no tie rule
    TC.assert_frustum_equal(out, ref, case["cam"]["n_levels"], what="boundaries")
    assert list(out["n_to_match"][:2]) == [0, 1]
    for k, c in enumerate(TC.random_frustum_cases()):   # rotated poses, several blocks per frame
        _, out = device_frustum(D, matcher, c)
        TC.assert_frustum_equal(out, R.frustum(c), c["cam"]["n_levels"], max_tie_share=0.001, what="random %d" % k)


def test_last_frame_projection(matcher):
    D = Dev()
    case = TC.last_boundary_case()
    _, out = device_last(D, matcher, case)
    ref = R.project_last(case)
    TC.check_last_boundary_rows(out, case)
    TC.assert_last_equal(out, ref, "boundaries")
    # frame 1 is rotated: on some of its points Rcw*x and the quaternion's _transformVector differ in the last bit, so the equality
    # above shows that the kernel rotates through the quaternion, as the reference does
    alt = R.project_last(case, through_matrix=True)
    differs = (ref["valid"][1] != 0) & (alt["valid"][1] != 0) & ((ref["u"][1] != alt["u"][1]) | (ref["v"][1] != alt["v"][1]))
    print("points on which the two forms differ: %d of %d" % (differs.sum(), (ref["valid"][1] != 0).sum()))
    assert differs.sum() >= 1
    for k, c in enumerate(TC.random_last_cases()):
        _, out = device_last(D, matcher, c)
        TC.assert_last_equal(out, R.project_last(c), "random %d" % k)


def test_pose_conversion(matcher):
    D = Dev()
    poses = TC.pose_cases()
    d_pose = D.up(poses)
    for normalise in (0, 1):
        d_fp = D.zeros(len(poses) * 19 * 4, np.uint8, 0x5a)
        matcher.frame_pose_batch_device(d_pose.data_ptr(), len(poses), normalise, d_fp.data_ptr(), D.stream)
        D.sync()
        np.testing.assert_array_equal(D.down(d_fp, F32, (len(poses), 19)), R.frame_pose_record(R.frame_pose(poses, normalise)), err_msg="normalise %d" % normalise)


def test_host_entries_are_bit_identical(matcher):
    D = Dev()
    case = TC.frustum_boundary_case()
    rec, dev_out = device_frustum(D, matcher, case)
    host = matcher.frustum_batch(case, rec)
    for k in dev_out:
        np.testing.assert_array_equal(host[k].view(np.uint8), dev_out[k].view(np.uint8), err_msg=k)        # bytes: NaN payloads included
    assert matcher.track_project_last_kernel_ms() > 0
    case = TC.last_boundary_case()
    rec, dev_out = device_last(D, matcher, case)
    host = matcher.project_last_batch(case, rec)
    for k in dev_out:
        np.testing.assert_array_equal(host[k].view(np.uint8), dev_out[k].view(np.uint8), err_msg=k)


def device_handover(D, m, c, pcap):
    B, cap = c["assign"].shape
    ins = {k: D.up(c[k]) for k in ("assign", "outlier", "n_cur", "last_local", "bad", "has_obs")}
    a_local, occ, skip, dropped = D.zeros(B * cap * 4, np.uint8, 0x5a), D.zeros(B * cap, np.uint8, 0x5a), D.zeros(B * pcap, np.uint8, 0x5a), D.zeros(B * 4, np.uint8, 0x5a)
    m.track_handover_batch_device(ins["assign"].data_ptr(), ins["outlier"].data_ptr(), ins["n_cur"].data_ptr(), cap, ins["last_local"].data_ptr(), c["last_local"].shape[1],
                                  ins["bad"].data_ptr(), ins["has_obs"].data_ptr(), pcap, a_local.data_ptr(), occ.data_ptr(), skip.data_ptr(), dropped.data_ptr(), B, D.stream)
    D.sync()
    return dict(assign_local=D.down(a_local, np.int32, (B, cap)), occupied=D.down(occ, np.uint8, (B, cap)), skip=D.down(skip, np.uint8, (B, pcap)),
                n_dropped=D.down(dropped, np.int32, (B,)))


def test_handover(matcher):
    D = Dev()
    c = TC.handover_case()
    ref = R.handover(**c)
    # the case holds what it was built to hold
    assert ref["n_dropped"][0] == 1 and (ref["assign_local"][0] >= 0).sum() == 19 - 4 - 1 - 1 and ref["skip"][0].sum() == 17
    assert ((ref["assign_local"][0] >= 0) & (ref["occupied"][0] == 0)).sum() == 1 and (ref["assign_local"][0] == 32).sum() == 2
    out = device_handover(D, matcher, c, c["bad"].shape[1])
    for k in ref:
        np.testing.assert_array_equal(out[k], ref[k], err_msg=k)
    # several frames, a capacity above one block
    rs = np.random.RandomState(8)
    B, cap, pcap = 3, 700, 900
    c = dict(assign=rs.randint(-1, cap, (B, cap)).astype(np.int32), outlier=(rs.uniform(size=(B, cap)) < 0.2).astype(np.uint8), n_cur=np.array([0, 650, 700], np.int32),
             last_local=rs.randint(-1, pcap, (B, cap)).astype(np.int32), bad=(rs.uniform(size=(B, pcap)) < 0.1).astype(np.uint8), has_obs=(rs.uniform(size=(B, pcap)) < 0.8).astype(np.uint8))
    c["assign"][rs.uniform(size=(B, cap)) < 0.4] = -1
    ref = R.handover(**c)
    out = device_handover(D, matcher, c, pcap)
    for k in ref:
        np.testing.assert_array_equal(out[k], ref[k], err_msg="random " + k)


def test_tracking_chain_projected_on_device(pkg, oracle, synth):
    """extract -> pose record -> project last frame -> last-frame search -> pose -> hand-over -> pose record -> frustum over a local
    table -> map-point search -> pose: enqueued back to back on one stream, ONE synchronisation at the end.  Images, shift and depths
    are those of test_chain_gpu.run_tracking_chain; the local table is the last frames' points plus as many again (the same pixels at
    other random depths, as map points of their own)."""
    from oracle_api import oracle_pose_optimize
    D = Dev()
    torch, dev, st = D.torch, D.dev, D.stream
    B, seed0, shift, (W_, H_) = 2, 80, 3, (640, 480)
    last_imgs = np.stack([synth.make_frame(seed0 + i, W_, H_) for i in range(B)])
    cur_imgs = np.ascontiguousarray(np.roll(last_imgs, shift, axis=2))
    cam = dict(fx=float(F32(458.654)), fy=float(F32(457.296)), cx=float(F32(367.215)), cy=float(F32(248.375)), bf=0.0,
               huber_mono=float(F32(np.sqrt(5.991))), huber_stereo=float(F32(np.sqrt(7.815))))
    rs = np.random.RandomState(5)
    ex, m, m2, ps = pkg.Extractor(), pkg.Matcher(0.9, True), pkg.Matcher(0.8, True), pkg.PoseSolver()
    cap = ex.max_keypoints
    pcap = 2 * cap
    sfac = np.asarray(ex.GetScaleFactors(), F32)
    isig = (1.0 / sfac.astype(np.float64) ** 2).astype(F32)
    tcam = dict(fx=F32(cam["fx"]), fy=F32(cam["fy"]), cx=F32(cam["cx"]), cy=F32(cam["cy"]), bf=F32(0), min_x=F32(0), min_y=F32(0), max_x=F32(W_), max_y=F32(H_),
                log_scale_factor=np.log(F32(1.2)), n_levels=len(sfac))
    oex = oracle.extractor()
    TH1, TH2, COS = 15.0, 3.0, F32(0.5)
    try:
        z = lambda dt, k: torch.zeros(B * k, dtype=dt, device=dev)
        l_kps, l_desc, l_n = z(torch.uint8, cap * 28), z(torch.uint8, cap * 32), z(torch.int32, 1)
        c_kps, c_desc, c_n = z(torch.uint8, cap * 28), z(torch.uint8, cap * 32), z(torch.int32, 1)
        d_mono, d_st = z(torch.int32, 1), z(torch.int32, 1)
        d_last = torch.from_numpy(last_imgs.copy()).to(dev); d_cur = torch.from_numpy(cur_imgs.copy()).to(dev)
        ex.extract_batch_device(d_last.data_ptr(), B, W_, H_, W_, W_ * H_, l_kps.data_ptr(), l_desc.data_ptr(), cap, l_n.data_ptr(), d_mono.data_ptr(), d_st.data_ptr(), (0, 1000), st)
        D.sync()
        # ---- resident state of the last frames and the local map, built on the host from the device's key points ----
        nL = D.down(l_n, np.int32, (B,))
        lk = D.down(l_kps, F32, (B, cap, 7)); l_oct_h = D.down(l_kps, np.int32, (B, cap, 7))[:, :, 5].copy()
        l_desc_h = D.down(l_desc, np.uint8, (B, cap, 32))
        lu, lv = lk[:, :, 0] + F32(shift), lk[:, :, 1]
        back = lambda zs: np.stack([(lu - tcam["cx"]) / tcam["fx"] * zs, (lv - tcam["cy"]) / tcam["fy"] * zs, zs], 2).astype(F32)
        zs = rs.uniform(2.0, 14.0, (B, cap)).astype(F32)               # (the depths of run_tracking_chain: the first draw of RandomState(5))
        l_mp_h = back(zs)
        live_l = np.arange(cap)[None, :] < nL[:, None]
        loc = dict(cam=tcam, cos_limit=COS, xyz=np.concatenate([l_mp_h, back(rs.uniform(2.0, 14.0, (B, cap)).astype(F32))], 1))
        dist = np.linalg.norm(loc["xyz"].astype(np.float64), axis=2)
        loc["normal"] = (loc["xyz"] / np.maximum(dist, 1e-9)[:, :, None]).astype(F32)
        oct2 = np.concatenate([l_oct_h, l_oct_h], 1)
        loc["max_distance"] = (dist * sfac[oct2] * rs.uniform(0.9, 1.1, (B, pcap))).astype(F32)       # UpdateNormalAndDepth's, off the level boundaries
        loc["min_distance"] = (loc["max_distance"] / sfac[-1]).astype(F32)
        loc["bad"] = np.concatenate([~live_l, np.zeros((B, cap), bool)], 1).astype(np.uint8)            # the dead rows between the two halves
        loc["n"] = (cap + nL).astype(np.int32)
        loc_desc = np.concatenate([l_desc_h, l_desc_h], 1); loc_obs = np.ones((B, pcap), np.uint8)
        last_local = np.where(live_l, np.arange(cap)[None, :], -1).astype(np.int32)
        p0 = np.zeros((B, 7)); p0[:, 3] = 1.0
        p0[:, :3] = rs.normal(0, 0.002, (B, 3)); p0[:, 4:] = rs.normal(0, 0.01, (B, 3))                  # the motion model's prediction
        p0 = p0.astype(F32).astype(np.float64)
        d = {k: D.up(v) for k, v in dict(l_mp=l_mp_h, l_oct=l_oct_h, l_ang=lk[:, :, 3], has_point=np.ones((B, cap), np.uint8), p0=p0, last_local=last_local,
                                         xyz=loc["xyz"], normal=loc["normal"], mind=loc["min_distance"], maxd=loc["max_distance"], bad=loc["bad"], loc_n=loc["n"],
                                         loc_desc=loc_desc, loc_obs=loc_obs).items()}
        fp1, fp2 = D.zeros(B * 19, F32), D.zeros(B * 19, F32)
        pl = [D.zeros(B * cap * np.dtype(dt).itemsize, np.uint8) for _, dt in LAST_OUT]
        fr = [D.zeros(B * pcap * np.dtype(dt).itemsize, np.uint8) for _, dt in FRUSTUM_OUT] + [D.zeros(B, np.int32)]
        t_assign = D.zeros(B * cap, np.int32, -1); t_occ = D.zeros(B * cap, np.uint8); t_nm = D.zeros(B, np.int32)
        a_local = D.zeros(B * cap, np.int32); occ2 = D.zeros(B * cap, np.uint8); skip = D.zeros(B * pcap, np.uint8); dropped = D.zeros(B, np.int32); nm2 = D.zeros(B, np.int32)
        pose1, inl1, outl1 = D.zeros(B * 7, np.float64), D.zeros(B, np.int32), D.zeros(B * cap, np.uint8)
        pose2, inl2, outl2 = D.zeros(B * 7, np.float64), D.zeros(B, np.int32), D.zeros(B * cap, np.uint8)
        cur = (c_kps.data_ptr(), c_desc.data_ptr(), c_n.data_ptr(), cap)
        bounds = (0.0, 0.0, float(W_), float(H_))
        D.sync()
        # ---- the chain: ten calls enqueued back to back, one synchronisation at the end ----
        ex.extract_batch_device(d_cur.data_ptr(), B, W_, H_, W_, W_ * H_, c_kps.data_ptr(), c_desc.data_ptr(), cap, c_n.data_ptr(), d_mono.data_ptr(), d_st.data_ptr(), (0, 1000), st)
        m.frame_pose_batch_device(d["p0"].data_ptr(), B, 1, fp1.data_ptr(), st)
        m.project_last_batch_device(tcam, fp1.data_ptr(), d["l_mp"].data_ptr(), d["has_point"].data_ptr(), l_n.data_ptr(), cap, tuple(t.data_ptr() for t in pl), B, st)
        m.SearchByProjection_last_batch_device(cur, (pl[0].data_ptr(), pl[1].data_ptr(), pl[2].data_ptr(), d["l_oct"].data_ptr(), d["l_ang"].data_ptr(), l_desc.data_ptr(), l_n.data_ptr(), cap),
                                               B, TH1, t_assign.data_ptr(), t_occ.data_ptr(), t_nm.data_ptr(), st, bounds=bounds, scale_factors=sfac)
        ps.optimize_batch_device(B, cap, c_kps.data_ptr(), c_n.data_ptr(), t_assign.data_ptr(), d["l_mp"].data_ptr(), cap, d["p0"].data_ptr(), isig, cam,
                                 pose1.data_ptr(), inl1.data_ptr(), outl1.data_ptr(), st)
        m.track_handover_batch_device(t_assign.data_ptr(), outl1.data_ptr(), c_n.data_ptr(), cap, d["last_local"].data_ptr(), cap, d["bad"].data_ptr(), d["loc_obs"].data_ptr(), pcap,
                                      a_local.data_ptr(), occ2.data_ptr(), skip.data_ptr(), dropped.data_ptr(), B, st)
        m.frame_pose_batch_device(pose1.data_ptr(), B, 1, fp2.data_ptr(), st)
        m.frustum_batch_device(tcam, fp2.data_ptr(), (d["xyz"].data_ptr(), d["normal"].data_ptr(), d["mind"].data_ptr(), d["maxd"].data_ptr(), skip.data_ptr(), d["bad"].data_ptr(),
                                                      d["loc_n"].data_ptr(), pcap), float(COS), tuple(t.data_ptr() for t in fr), B, st)
        handed = (a_local.clone(), occ2.clone())        # (device-side copies in stream order: the search below overwrites its in/out arrays)
        m2.SearchByProjection_batch_device(cur, (fr[0].data_ptr(), fr[1].data_ptr(), fr[2].data_ptr(), fr[3].data_ptr(), 0, d["loc_desc"].data_ptr(), d["loc_n"].data_ptr(), pcap,
                                                 d["loc_obs"].data_ptr()), (fr[4].data_ptr(), fr[5].data_ptr(), d["bad"].data_ptr()), B, TH2,
                                           a_local.data_ptr(), occ2.data_ptr(), nm2.data_ptr(), st, bounds=bounds, scale_factors=sfac)
        ps.optimize_batch_device(B, cap, c_kps.data_ptr(), c_n.data_ptr(), a_local.data_ptr(), d["xyz"].data_ptr(), pcap, pose1.data_ptr(), isig, cam,
                                 pose2.data_ptr(), inl2.data_ptr(), outl2.data_ptr(), st)
        D.sync()
        g_ = lambda t, dt, shape: D.down(t, dt, shape)
        proj = {k: g_(t, dt, (B, cap)) for (k, dt), t in zip(LAST_OUT, pl)}
        fru = {k: g_(t, dt, (B, pcap)) for (k, dt), t in zip(FRUSTUM_OUT, fr)}; fru["n_to_match"] = g_(fr[-1], np.int32, (B,))
        assign1 = g_(t_assign, np.int32, (B, cap)); nm1 = g_(t_nm, np.int32, (B,)); P1 = g_(pose1, np.float64, (B, 7)); I1 = g_(inl1, np.int32, (B,)); O1 = g_(outl1, np.uint8, (B, cap))
        hand = dict(assign_local=g_(handed[0], np.int32, (B, cap)), occupied=g_(handed[1], np.uint8, (B, cap)), skip=g_(skip, np.uint8, (B, pcap)), n_dropped=g_(dropped, np.int32, (B,)))
        assign2 = g_(a_local, np.int32, (B, cap)); nm2_h = g_(nm2, np.int32, (B,)); P2 = g_(pose2, np.float64, (B, 7)); I2 = g_(inl2, np.int32, (B,)); O2 = g_(outl2, np.uint8, (B, cap))
        rec1, rec2 = g_(fp1, F32, (B, 19)), g_(fp2, F32, (B, 19)); nC_dev = g_(c_n, np.int32, (B,))
    finally:
        ex.close(); m.close(); m2.close(); ps.close()

    def close_to(pose, gref, q_start, t_start):
        q0 = q_start / np.linalg.norm(q_start)
        dq = np.abs(np.asarray(gref["q"]) - q0).max(); dt = np.abs(np.asarray(gref["t"]) - t_start).max()
        return np.abs(pose[:4] - gref["q"]).max() <= 1e-4 * dq + 1e-12 and np.abs(pose[4:] - gref["t"]).max() <= 1e-4 * dt + 1e-12

    # ---- first half: the projection is the reference's on the predicted pose, search and pose are the oracle's on it ----
    last_case = dict(cam=tcam, pose7=p0, xyz=l_mp_h, has_point=np.ones((B, cap), np.uint8), n=nL)
    np.testing.assert_array_equal(rec1, R.frame_pose_record(R.frame_pose(p0, 1)))
    TC.assert_last_equal(proj, R.project_last(last_case), "chain, last frame")
    # ---- second half: the reference on the device's OWN first pose (device poses match the oracle's only to 1e-4) ----
    np.testing.assert_array_equal(rec2, R.frame_pose_record(R.frame_pose(P1, 1)))
    ref_hand = R.handover(assign1, O1, nC_dev, last_local, loc["bad"], loc_obs)
    for k in ref_hand:
        np.testing.assert_array_equal(hand[k], ref_hand[k], err_msg="hand-over " + k)
    assert (hand["n_dropped"] == 0).all()
    TC.assert_frustum_equal(fru, R.frustum(dict(loc, pose7=P1, skip=hand["skip"])), len(sfac), max_tie_share=0.001, what="chain, frustum")
    for b in range(B):
        _, kL, dL = oex.extract(last_imgs[b], (0, 1000)); _, kC, dC = oex.extract(cur_imgs[b], (0, 1000))
        n_l, nC = len(kL), len(kC)
        assert n_l == nL[b] and nC == nC_dev[b]
        g = dict(x=np.ascontiguousarray(kC["x"]), y=np.ascontiguousarray(kC["y"]), octave=np.ascontiguousarray(kC["octave"]),
                 min_x=0.0, min_y=0.0, max_x=float(W_), max_y=float(H_), cols=64, rows=48)
        last = dict(u=proj["u"][b, :n_l].copy(), v=proj["v"][b, :n_l].copy(), octave=np.ascontiguousarray(kL["octave"]), angle=np.ascontiguousarray(kL["angle"]),
                    valid=proj["valid"][b, :n_l].copy(), desc=dL, has_obs=np.ones(n_l, np.uint8))
        a0 = np.full(nC, -1, np.int32); o0 = np.zeros(nC, np.uint8)
        n0 = oracle.search_by_projection_last(g, dC, np.ascontiguousarray(kC["angle"]), sfac, last, TH1, True, a0, o0)
        assert nm1[b] == n0 > 300
        np.testing.assert_array_equal(assign1[b, :nC], a0)
        feat = np.nonzero(a0 >= 0)[0]
        obs = lambda f: np.stack([kC["x"][f], kC["y"][f], np.full(len(f), -1.0, F32)], 1).astype(np.float64)
        w = dict(cam, q=p0[b, :4], t=p0[b, 4:], Xw=l_mp_h[b, a0[feat]].astype(np.float64), stereo=np.zeros(len(feat), np.uint8), obs=obs(feat),
                 inv_sigma2=isig[kC["octave"][feat]].astype(np.float64))
        gref = oracle_pose_optimize(oracle, w)
        full = np.zeros(cap, np.uint8); full[feat] = gref["outlier"]
        np.testing.assert_array_equal(O1[b], full)
        assert I1[b] == int(gref["inliers"]) > 200
        assert close_to(P1[b], gref, p0[b, :4], p0[b, 4:])
        # the second search and pose: the oracle on the device's projections
        n_p = int(loc["n"][b])
        mp = dict(in_view=fru["valid"][b, :n_p].copy(), u=fru["u"][b, :n_p].copy(), v=fru["v"][b, :n_p].copy(), level=fru["octave"][b, :n_p].copy(),
                  view_cos=fru["view_cos"][b, :n_p].copy(), depth=fru["track_depth"][b, :n_p].copy(), desc=np.ascontiguousarray(loc_desc[b, :n_p]),
                  has_obs=np.ascontiguousarray(loc_obs[b, :n_p]), bad=np.ascontiguousarray(loc["bad"][b, :n_p]))
        a2 = hand["assign_local"][b, :nC].copy(); o2 = hand["occupied"][b, :nC].copy()
        n2 = oracle.search_by_projection(g, dC, sfac, mp, TH2, 0.8, a2, o2)
        print("frame %d: %d + %d matches, %d in view of %d local points, inliers %d -> %d" % (b, n0, n2, fru["n_to_match"][b], n_p, I1[b], I2[b]))
        assert nm2_h[b] == n2 > 10         # (hundreds of features are left unmatched by the first search; their pixels have a second map point)
        np.testing.assert_array_equal(assign2[b, :nC], a2)
        feat = np.nonzero(a2 >= 0)[0]
        w = dict(cam, q=P1[b, :4], t=P1[b, 4:], Xw=loc["xyz"][b, a2[feat]].astype(np.float64), stereo=np.zeros(len(feat), np.uint8), obs=obs(feat),
                 inv_sigma2=isig[kC["octave"][feat]].astype(np.float64))
        gref = oracle_pose_optimize(oracle, w)
        full = np.zeros(cap, np.uint8); full[feat] = gref["outlier"]
        np.testing.assert_array_equal(O2[b], full)
        assert I2[b] == int(gref["inliers"]) > 200
        assert close_to(P2[b], gref, P1[b, :4], P1[b, 4:])
        assert np.abs(P2[b, 4:]).max() < 0.02          # and it found the true pose (identity)
