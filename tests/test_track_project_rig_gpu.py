"""The rig projection entries of include/orbslam3_hip_track_project_rig.h on the GPU against tests/track_project_rig_reference.py.
Decisions, levels (tie rule of track_project_reference.level_mismatches) and the preserved stale state are equal on every row that
is not open; proj_u / proj_v of passing rows lie within the KannalaBrandt8 bar of the reference (4 x SPREAD_F32 of
rig_newpoints_reference, relative to |u - cx| + |cx|); view_cos, track_depth, the frame records and UnprojectStereoFishEye hold no
transcendental and are bit-exact.  In/out and output buffers start as 0x5a bytes, so an unwritten output and an overwritten stale
value both show.

Measured on an MI355X (this file prints the live values): over the hand-built and the random scenes 0 of the 1 000 frustum
projections and 0 of the 1 508 last-frame projections differ from the reference at all (worst |device - reference| = 0.000 of the
bar), and 0 differ from the host build of the header."""
import os
import subprocess

import numpy as np
import pytest

import rig_match_cases as MC
import track_project_rig_cases as TC
import track_project_rig_reference as RR

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRUSTUM_OUT = TC.ST.RIG_STATE
LAST_OUT = (("valid", np.uint8), ("proj_u", F32), ("proj_v", F32), ("proj_u_r", F32), ("proj_v_r", F32))


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


def pattern_state(B, pcap):
    """every array of the state as 0x5a bytes"""
    return {k: np.full(B * pcap * np.dtype(dt).itemsize, 0x5a, np.uint8).view(dt).reshape(B, pcap).copy() for k, dt in FRUSTUM_OUT}


def device_frustum(D, m, case, state, normalise=1):
    """orbm_rig_frame_pose_batch_device + orbm_frustum_rig_batch_device -> (rig pose records [B][43], the arrays after the call)"""
    B, pcap = case["skip"].shape
    d_pose = D.up(np.asarray(case["pose7"], np.float64)); d_fp = D.zeros(B * 43 * 4, np.uint8, 0x5a)
    ins = [D.up(np.asarray(case[k], F32)) for k in ("xyz", "normal", "min_distance", "max_distance")] + \
          [D.up(np.asarray(case[k], np.uint8)) for k in ("skip", "bad")] + [D.up(np.asarray(case["n"], np.int32))]
    outs = [D.up(np.asarray(state[k], dt)) for k, dt in FRUSTUM_OUT] + [D.zeros(B * 4, np.uint8, 0x5a)]
    m.rig_frame_pose_batch_device(case["cam"], d_pose.data_ptr(), B, normalise, d_fp.data_ptr(), D.stream)
    m.frustum_rig_batch_device(case["cam"], d_fp.data_ptr(), tuple(t.data_ptr() for t in ins) + (pcap,), float(case["cos_limit"]),
                               tuple(t.data_ptr() for t in outs), B, D.stream)
    D.sync()
    out = {k: D.down(t, dt, (B, pcap)) for (k, dt), t in zip(FRUSTUM_OUT, outs)}
    out["n_to_match"] = D.down(outs[-1], np.int32, (B,))
    return D.down(d_fp, F32, (B, 43)), out


def device_last(D, m, case, normalise=1):
    B, cap = case["has_point"].shape
    d_pose = D.up(np.asarray(case["pose7"], np.float64)); d_fp = D.zeros(B * 43 * 4, np.uint8, 0x5a)
    d_xyz, d_has, d_n = D.up(np.asarray(case["xyz"], F32)), D.up(np.asarray(case["has_point"], np.uint8)), D.up(np.asarray(case["n"], np.int32))
    outs = [D.zeros(B * cap * np.dtype(dt).itemsize, np.uint8, 0x5a) for _, dt in LAST_OUT]
    m.rig_frame_pose_batch_device(case["cam"], d_pose.data_ptr(), B, normalise, d_fp.data_ptr(), D.stream)
    m.project_last_rig_batch_device(case["cam"], d_fp.data_ptr(), d_xyz.data_ptr(), d_has.data_ptr(), d_n.data_ptr(), cap, tuple(t.data_ptr() for t in outs), B, D.stream)
    D.sync()
    return D.down(d_fp, F32, (B, 43)), {k: D.down(t, dt, (B, cap)) for (k, dt), t in zip(LAST_OUT, outs)}


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.Matcher(0.8, True)
    yield m
    m.close()


@pytest.fixture(scope="module")
def host_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tpr_gpu") / "track_project_rig_geometry_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"), "-o", exe,
                           os.path.join(ROOT, "tests", "track_project_rig_geometry_check.cpp")])
    return exe


def host_build(exe, tmp, mode, case):
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(TC.pack(mode, case, 1))
    subprocess.check_call([exe, src, dst])
    with open(dst, "rb") as f:
        return TC.unpack(mode, case, f.read())[1]


def test_frustum_decisions_and_stale_state(matcher, host_exe, tmp_path):
    D = Dev()
    case = TC.frustum_hand_case()
    _, out = device_frustum(D, matcher, case, case["state"])           # the sentinel state: the literal expectations of the hand-built rows
    TC.check_frustum_hand_rows(out, case)
    for name, c, seen_l, seen_r in TC.bounds_cases():                   # batch 1: the eight strict bounds comparisons
        _, o = device_frustum(D, matcher, c, pattern_state(1, TC.PCAP))
        TC.check_bounds_case(o, seen_l, seen_r, name)
    worst, differ, host_differ, total = 0.0, 0, 0, 0
    for k, c in enumerate([case] + TC.random_frustum_cases()):
        B, pcap = c["skip"].shape
        state = pattern_state(B, pcap)
        _, out = device_frustum(D, matcher, c, state)
        ref = RR.frustum(c, state=state)
        w, d = TC.compare_frustum(out, ref, c["cam"]["n_levels"], "scene %d" % k)
        host = host_build(host_exe, tmp_path, 0, dict(c, state=state))
        for sfx in ("", "_r"):
            seen = (out["in_view" + sfx] != 0) & (host["in_view" + sfx] != 0)
            total += int(seen.sum()) * 2
            host_differ += int(((out["proj_u" + sfx] != host["proj_u" + sfx]) & seen).sum() + ((out["proj_v" + sfx] != host["proj_v" + sfx]) & seen).sum())
        worst, differ = max(worst, w), differ + d
    print("frustum: worst |device - reference| / bar %.3f; %d of %d projections differ from the reference at all, %d from the host build of the header" % (
        worst, differ, total, host_differ))


def test_last_frame_projection(matcher, host_exe, tmp_path):
    D = Dev()
    case = TC.last_hand_case()
    _, out = device_last(D, matcher, case)
    TC.check_last_hand_rows(out, case)
    # uv_r through the LEFT camera's parameters: equal to the reference, and pixels away from what mpCamera2 would give
    ref, alt = RR.project_last(case), RR.project_last(case, right_camera_for_uvr=True)
    i = [r[0] for r in TC.LAST_ROWS].index("in_view")
    assert abs(float(out["proj_u_r"][0, i]) - float(ref["proj_u_r"][0, i])) <= ref["guard"]["proj_u_r"][0, i] < 0.01
    assert abs(float(out["proj_u_r"][0, i]) - float(alt["proj_u_r"][0, i])) > 5
    worst, differ, host_differ, total = 0.0, 0, 0, 0
    for k, c in enumerate([case] + TC.random_last_cases()):
        _, out = device_last(D, matcher, c)
        w, d = TC.compare_last(out, RR.project_last(c), "scene %d" % k)
        host = host_build(host_exe, tmp_path, 1, c)
        ok = (out["valid"] != 0) & (host["valid"] != 0)
        total += int(ok.sum()) * 4
        host_differ += sum(int(((out[f] != host[f]) & ok).sum()) for f in ("proj_u", "proj_v", "proj_u_r", "proj_v_r"))
        worst, differ = max(worst, w), differ + d
    print("last frame: worst |device - reference| / bar %.3f; %d of %d projections differ from the reference at all, %d from the host build of the header" % (
        worst, differ, total, host_differ))


def test_rig_frame_record(matcher):
    D = Dev()
    poses = TC.pose_cases()
    cam = TC.ST.rig_camera()
    d_pose = D.up(poses)
    for normalise in (0, 1):
        d_fp = D.zeros(len(poses) * 43 * 4, np.uint8, 0x5a)
        matcher.rig_frame_pose_batch_device(cam, d_pose.data_ptr(), len(poses), normalise, d_fp.data_ptr(), D.stream)
        D.sync()
        want = RR.rig_frame_pose_record(RR.rig_frame_pose(cam, poses, normalise))
        np.testing.assert_array_equal(D.down(d_fp, F32, (len(poses), 43)).view(np.uint32), want.view(np.uint32), err_msg="normalise %d" % normalise)


def test_host_entries_are_bit_identical(matcher):
    D = Dev()
    case = TC.frustum_hand_case()
    state = pattern_state(*case["skip"].shape)
    rec, dev_out = device_frustum(D, matcher, case, state)
    host = matcher.frustum_rig_batch(case, rec, state)
    for k in dev_out:
        np.testing.assert_array_equal(host[k].view(np.uint8), dev_out[k].view(np.uint8), err_msg=k)
    assert matcher.track_project_rig_last_kernel_ms() > 0
    case = TC.last_hand_case()
    rec, dev_out = device_last(D, matcher, case)
    host = matcher.project_last_rig_batch(case, rec)
    for k in dev_out:
        np.testing.assert_array_equal(host[k].view(np.uint8), dev_out[k].view(np.uint8), err_msg=k)


def test_unproject_stereo_fisheye(matcher):
    D = Dev()
    c = TC.unproject_case()
    B, cap = c["valid"].shape
    d_pose = D.up(np.asarray(c["pose7"], np.float64)); d_fp = D.zeros(B * 43, F32)
    d_pts, d_val, d_n, d_w = D.up(c["points"]), D.up(c["valid"]), D.up(c["n"]), D.up(c["world"])
    matcher.rig_frame_pose_batch_device(c["cam"], d_pose.data_ptr(), B, 1, d_fp.data_ptr(), D.stream)
    matcher.unproject_stereo_fisheye_batch_device(d_fp.data_ptr(), d_pts.data_ptr(), d_val.data_ptr(), d_n.data_ptr(), cap, d_w.data_ptr(), B, D.stream)
    D.sync()
    want = RR.unproject(RR.rig_frame_pose(c["cam"], c["pose7"], 1), c["points"], c["valid"], c["n"], c["world"])
    got = D.down(d_w, F32, (B, cap, 3))
    np.testing.assert_array_equal(got.view(np.uint32), want.view(np.uint32))          # bit-exact: no transcendentals
    assert (got[1] == -555).all() and (got[0] != -555).any()
    host = matcher.unproject_stereo_fisheye_batch(D.down(d_fp, F32, (B, 43)), c["points"], c["valid"], c["n"], c["world"])
    np.testing.assert_array_equal(host.view(np.uint32), got.view(np.uint32))


def test_two_calls_return_the_same_bits(matcher):
    D = Dev()
    c = TC.random_frustum_cases()[1]
    state = pattern_state(*c["skip"].shape)
    a, b = device_frustum(D, matcher, c, state), device_frustum(D, matcher, c, state)
    np.testing.assert_array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
    for k in a[1]:
        np.testing.assert_array_equal(a[1][k].view(np.uint8), b[1][k].view(np.uint8), err_msg=k)
    c = TC.random_last_cases()[1]
    a, b = device_last(D, matcher, c), device_last(D, matcher, c)
    for k in a[1]:
        np.testing.assert_array_equal(a[1][k].view(np.uint8), b[1][k].view(np.uint8), err_msg=k)


def _rig_on_projections(rng, size, left_uv, right_uv, desc, level, level_r, n_noise=40):
    """a rig frame with a left key point near every left projection and a right key point near every right one (descriptor: the
    point's, a few bits flipped), plus random key points"""
    l, r = MC.Side(*size), MC.Side(*size)
    for side, uv, lv in ((l, left_uv, level), (r, right_uv, level_r)):
        for i in np.nonzero(np.isfinite(uv[:, 0]))[0]:
            side.add(float(uv[i, 0] + rng.uniform(-1, 1)), float(uv[i, 1] + rng.uniform(-1, 1)), MC._noisy(rng, desc[i], 20), int(max(lv[i], 0)), float(rng.uniform(0, 360)))
        for _ in range(n_noise):
            side.add(float(rng.uniform(5, size[0] - 5)), float(rng.uniform(5, size[1] - 5)), rng.integers(0, 256, 32).astype(np.uint8), int(rng.integers(0, 4)), float(rng.uniform(0, 360)))
    return MC.make_rig(l, r)


def test_chain_into_the_rig_searches(pkg, matcher):
    """device frustum / last-frame projection -> OrbmRigMapPoints / OrbmRigLastPoints pointed at the downloaded rows ->
    orbm_search_by_projection_rig_batch / _last_rig_batch: assign, occupied and n_matches equal those of the same searches fed by
    the reference's projection.  The stale left mTrackDepth is 1000 on half of the points and 1 on the others: with bFarPoints and
    thFarPoints = 30 the search drops a point that only the right camera sees when its STALE depth is far, whatever its depth now."""
    D = Dev()
    rng = np.random.default_rng(5)
    cam = TC.ST.rig_camera(yaw=0.8)
    size = (float(cam["max_x"]), float(cam["max_y"]))
    c = TC.ST.make_rig_local_map_case(71, 2, 200, cam=cam, full=True)
    B, pcap = c["skip"].shape
    state = pattern_state(B, pcap)
    state["track_depth"] = np.where(rng.random((B, pcap)) < 0.5, F32(1000), F32(1)).astype(F32)
    ref = RR.frustum(c, state=state)
    assert not ref["open"].any(), "a row of this scene hangs on a guard band: change the scene"
    _, out = device_frustum(D, matcher, c, state)
    desc = rng.integers(0, 256, (B, pcap, 32)).astype(np.uint8)
    has_obs = (rng.random((B, pcap)) < 0.8).astype(np.uint8)
    m = pkg.Matcher(0.8, False)           # (random key-point angles: no rotation check in the last-frame search)
    try:
        for name, src in (("device", out), ("reference", ref)):
            queries = []
            for b in range(B):
                uv = np.where((ref["in_view"][b] != 0)[:, None], np.stack([ref["proj_u"][b], ref["proj_v"][b]], 1), np.nan)
                uvr = np.where((ref["in_view_r"][b] != 0)[:, None], np.stack([ref["proj_u_r"][b], ref["proj_v_r"][b]], 1), np.nan)
                rig = _rig_on_projections(np.random.default_rng(100 + b), size, uv, uvr, desc[b], ref["pred_level"][b], ref["pred_level_r"][b])
                pts = {k: np.ascontiguousarray(src[k][b]) for k, _ in FRUSTUM_OUT if k != "track_depth_r"}
                pts.update(bad=np.ascontiguousarray(c["bad"][b]), has_obs=has_obs[b].copy(), desc=np.ascontiguousarray(desc[b]), n=pcap)
                slots = len(rig["left"]["x"]) + len(rig["right"]["x"])
                queries.append(dict(rig=rig, pts=pts, assign=np.full(slots, -1, np.int32), occupied=np.zeros(slots, np.uint8)))
            n = m.search_by_projection_rig_batch(queries, 1.0, far_points=True, th_far=30.0)
            if name == "device":
                first = (n, [q["assign"].copy() for q in queries], [q["occupied"].copy() for q in queries])
        assert first[0] == n and min(n) > 30
        for b in range(B):
            np.testing.assert_array_equal(first[1][b], queries[b]["assign"]); np.testing.assert_array_equal(first[2][b], queries[b]["occupied"])
            right_only = (ref["in_view"][b] == 0) & (ref["in_view_r"][b] != 0) & (c["bad"][b] == 0)
            matched = np.zeros(pcap, bool); matched[first[1][b][first[1][b] >= 0]] = True
            stale_far = out["track_depth"][b] == 1000
            assert (right_only & stale_far).sum() >= 2 and not matched[right_only & stale_far].any()       # dropped by the stale left depth
            assert matched[right_only & ~stale_far].sum() >= 2 and (ref["track_depth_r"][b][right_only & stale_far] < 30).any()
            print("frame %d: %d matches; right-only points: %d dropped by a stale far depth, %d of %d others matched" % (
                b, n[b], (right_only & stale_far).sum(), matched[right_only & ~stale_far].sum(), (right_only & ~stale_far).sum()))
        # ---- the last-frame search ----
        lc = TC.ST.make_rig_last_frame_case(72, 2, 200, cam=cam, full=True)
        lref = RR.project_last(lc)
        assert not lref["open"].any(), "a row of this scene hangs on a guard band: change the scene"
        _, lout = device_last(D, matcher, lc)
        cap = lc["has_point"].shape[1]
        octave = rng.integers(0, 4, (B, cap)).astype(np.int32); angle = rng.uniform(0, 360, (B, cap)).astype(F32)
        for name, src in (("device", lout), ("reference", lref)):
            queries = []
            for b in range(B):
                ok = (lref["valid"][b] != 0)[:, None]
                inside = (lref["proj_u_r"][b] > 0) & (lref["proj_u_r"][b] < size[0]) & (lref["proj_v_r"][b] > 0) & (lref["proj_v_r"][b] < size[1])
                uv = np.where(ok, np.stack([lref["proj_u"][b], lref["proj_v"][b]], 1), np.nan)
                uvr = np.where(ok & inside[:, None], np.stack([lref["proj_u_r"][b], lref["proj_v_r"][b]], 1), np.nan)
                rig = _rig_on_projections(np.random.default_rng(200 + b), size, uv, uvr, desc[b], octave[b], octave[b])
                pts = {k: np.ascontiguousarray(src[k][b]) for k, _ in LAST_OUT}
                pts.update(octave=octave[b].copy(), angle=angle[b].copy(), has_obs=has_obs[b].copy(), desc=np.ascontiguousarray(desc[b]), n=cap, level_window=0)
                slots = len(rig["left"]["x"]) + len(rig["right"]["x"])
                queries.append(dict(rig=rig, pts=pts, assign=np.full(slots, -1, np.int32), occupied=np.zeros(slots, np.uint8)))
            n = m.search_by_projection_last_rig_batch(queries, 7.0)
            if name == "device":
                first = (n, [q["assign"].copy() for q in queries], [q["occupied"].copy() for q in queries])
        assert first[0] == n and min(n) > 10
        for b in range(B):
            np.testing.assert_array_equal(first[1][b], queries[b]["assign"]); np.testing.assert_array_equal(first[2][b], queries[b]["occupied"])
        print("last-frame search: %s matches" % n)
    finally:
        m.close()
