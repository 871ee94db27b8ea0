"""Parity of the HIP matcher (through the C ABI) against the CPU oracle: match sets must be identical."""
import importlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("seed,n,ratio,ori", [(0, 1000, 0.7, True), (1, 1000, 0.75, True), (2, 1000, 0.9, False),
                                              (3, 64, 0.7, True), (4, 2500, 0.6, True)])
def test_search_by_bow(pkg, oracle, synth, seed, n, ratio, ori):
    ms = synth.make_match_set(seed, n=n)
    n0, m0 = oracle.search_by_bow(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], ms["dF"], ms["angF"], ms["fvF"], ratio, ori)
    m = pkg.Matcher(ratio, ori)
    try:
        n1, m1 = m.SearchByBoW(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], ms["dF"], ms["angF"], ms["fvF"])
    finally:
        m.close()
    assert n1 == n0
    np.testing.assert_array_equal(m1, m0)
    assert n0 > 0.2 * n * 0.5       # the case is not degenerate


def test_search_by_bow_batch(pkg, oracle, synth):
    sets = [synth.make_match_set(10 + i, n=500 + 100 * i) for i in range(5)]
    m = pkg.Matcher(0.7, True)
    try:
        res = m.SearchByBoW_batch(sets)
    finally:
        m.close()
    for ms, (n1, m1) in zip(sets, res):
        n0, m0 = oracle.search_by_bow(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], ms["dF"], ms["angF"], ms["fvF"], 0.7, True)
        assert n1 == n0
        np.testing.assert_array_equal(m1, m0)


def test_search_by_bow_edge_cases(pkg, oracle, synth):
    ms = synth.make_match_set(7, n=300)
    m = pkg.Matcher(0.7, True)
    try:
        # no valid KF map points -> no matches
        z = np.zeros_like(ms["validKF"])
        n1, m1 = m.SearchByBoW(ms["dKF"], z, ms["angKF"], ms["fvKF"], ms["dF"], ms["angF"], ms["fvF"])
        assert n1 == 0 and (m1 == -1).all()
        # disjoint vocabularies -> no common node
        fv2 = (ms["fvF"][0] + 100000, ms["fvF"][1], ms["fvF"][2])
        n1, m1 = m.SearchByBoW(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], ms["dF"], ms["angF"], fv2)
        assert n1 == 0
        # ragged: a frame feature listed under two nodes breaks the DBoW2 invariant -> serial path, still equal to the oracle
        nodes, offs, feat = [a.copy() for a in ms["fvF"]]
        feat2 = np.concatenate([feat, feat[:3]]).astype(np.uint32)
        nodes2 = np.concatenate([nodes, [nodes[-1] + 5]]).astype(np.uint32)
        offs2 = np.concatenate([offs, [offs[-1] + 3]]).astype(np.int32)
        nodesK = np.concatenate([ms["fvKF"][0], [nodes[-1] + 5]]).astype(np.uint32)
        offsK = np.concatenate([ms["fvKF"][1], [ms["fvKF"][1][-1] + 3]]).astype(np.int32)
        featK = np.concatenate([ms["fvKF"][2], ms["fvKF"][2][:3]]).astype(np.uint32)
        n0, m0 = oracle.search_by_bow(ms["dKF"], ms["validKF"], ms["angKF"], (nodesK, offsK, featK), ms["dF"], ms["angF"], (nodes2, offs2, feat2), 0.7, True)
        n1, m1 = m.SearchByBoW(ms["dKF"], ms["validKF"], ms["angKF"], (nodesK, offsK, featK), ms["dF"], ms["angF"], (nodes2, offs2, feat2))
        assert n1 == n0
        np.testing.assert_array_equal(m1, m0)
        # empty frame
        e = (np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32))
        n1, m1 = m.SearchByBoW(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], np.zeros((0, 32), np.uint8), np.zeros(0, np.float32), e)
        assert n1 == 0 and len(m1) == 0
    finally:
        m.close()


@pytest.mark.parametrize("seed", [0, 1])
def test_search_by_bow_kfkf(pkg, oracle, synth, seed):
    ms = synth.make_match_set(20 + seed, n=800)
    rs = np.random.RandomState(seed)
    valid2 = (rs.uniform(size=len(ms["dF"])) < 0.9).astype(np.uint8)
    n0, m0 = oracle.search_by_bow_kfkf(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], ms["dF"], valid2, ms["angF"], ms["fvF"], 0.8, True)
    m = pkg.Matcher(0.8, True)
    try:
        n1, m1 = m.SearchByBoW_KFKF(ms["dKF"], ms["validKF"], ms["angKF"], ms["fvKF"], ms["dF"], valid2, ms["angF"], ms["fvF"])
    finally:
        m.close()
    assert n1 == n0 and n0 > 50
    np.testing.assert_array_equal(m1, m0)


@pytest.mark.parametrize("seed,th,far", [(0, 1.0, False), (1, 3.0, False), (2, 15.0, True), (3, 1.0, False)])
def test_search_by_projection(pkg, oracle, sm, seed, th, far):
    g, dF, angF, scale, mp, assign, occ = sm.make_projection_case(seed)
    a0, o0 = assign.copy(), occ.copy()
    n0 = oracle.search_by_projection(g, dF, scale, mp, th, 0.8, a0, o0, b_far=far, th_far=20.0)
    m = pkg.Matcher(0.8, True)
    try:
        a1, o1 = assign.copy(), occ.copy()
        n1 = m.SearchByProjection(g, dF, scale, mp, th, a1, o1, far_points=far, th_far=20.0)
    finally:
        m.close()
    assert n1 == n0 and n0 > 100
    np.testing.assert_array_equal(a1, a0)
    np.testing.assert_array_equal(o1, o0)


@pytest.mark.parametrize("seed,th,far,frac", [(4, 1.0, False, 0.0), (5, 3.0, False, 0.5), (6, 3.0, True, 1.0), (7, 15.0, False, 0.5),
                                              (8, 1.0, False, 1.0)])
def test_search_by_projection_rectified_stereo(pkg, oracle, sm, seed, th, far, frac):
    """the mvuRight gate of src/ORBmatcher.cc:92-98 (F.Nleft == -1 && F.mvuRight[idx] > 0) at stereo shares 0 / 0.5 / 1"""
    g, dF, angF, scale, mp, assign, occ = sm.make_projection_case(seed, stereo_frac=frac)
    a0, o0 = assign.copy(), occ.copy()
    n0 = oracle.search_by_projection(g, dF, scale, mp, th, 0.8, a0, o0, b_far=far, th_far=20.0)
    gm = {k: v for k, v in g.items() if k != "u_right"}
    am, om = assign.copy(), occ.copy()
    nm = oracle.search_by_projection(gm, dF, scale, mp, th, 0.8, am, om, b_far=far, th_far=20.0)
    m = pkg.Matcher(0.8, True)
    try:
        a1, o1 = assign.copy(), occ.copy()
        n1 = m.SearchByProjection(g, dF, scale, mp, th, a1, o1, far_points=far, th_far=20.0)
        a2, o2 = assign.copy(), occ.copy()
        n2 = m.SearchByProjection(gm, dF, scale, mp, th, a2, o2, far_points=far, th_far=20.0)     # mono results unchanged
    finally:
        m.close()
    assert n1 == n0 and n0 > 100
    np.testing.assert_array_equal(a1, a0); np.testing.assert_array_equal(o1, o0)
    assert n2 == nm
    np.testing.assert_array_equal(a2, am)
    if frac == 0.0:
        np.testing.assert_array_equal(a0, am)            # no feature has a right coordinate: the monocular search
    elif th <= 3.0:
        assert not np.array_equal(a0, am)                # the gate bites (at th = 15 the window is wider than the synthetic ur errors)


@pytest.mark.parametrize("seed,th,ori,frac,lw", [(3, 15.0, True, 0.0, 0), (4, 15.0, True, 0.5, 0), (5, 7.0, True, 1.0, 0),
                                                 (6, 15.0, True, 0.5, 1), (7, 15.0, True, 0.5, 2), (8, 7.0, False, 1.0, 1),
                                                 (9, 15.0, True, 1.0, 2), (10, 15.0, True, None, 1), (11, 15.0, True, None, 2)])
def test_search_by_projection_last_frame_stereo(pkg, oracle, sm, seed, th, ori, frac, lw):
    """!bMono: the ur gate (:1751-1757) and the forward / backward level windows (:1692-1693, :1728-1733)"""
    g, dF, angF, scale, last, assign, occ = sm.make_last_frame_case(seed, stereo_frac=frac, level_window=lw)
    a0, o0 = assign.copy(), occ.copy()
    n0 = oracle.search_by_projection_last(g, dF, angF, scale, last, th, ori, a0, o0)
    m = pkg.Matcher(0.9, ori)
    try:
        a1, o1 = assign.copy(), occ.copy()
        n1 = m.SearchByProjection_last(g, dF, angF, scale, last, th, a1, o1)
    finally:
        m.close()
    assert n1 == n0 and n0 > 60
    np.testing.assert_array_equal(a1, a0)
    np.testing.assert_array_equal(o1, o0)


def test_projection_stereo_argument_errors(pkg, oracle, sm):
    """a stereo frame without the points' right columns is refused, never searched as if it were monocular; and a refused call leaves
    the handle usable: the next good call of every entry that shares the frame staging equals its oracle"""
    import rig_match_cases
    from test_rig_match_reference import run_reference
    g, dF, angF, scale, last, assign, occ = sm.make_last_frame_case(2, n=200, n_last=100, stereo_frac=0.5)
    bad = {k: v for k, v in last.items() if k != "ur"}
    m = pkg.Matcher(0.9, True)
    try:
        with pytest.raises(pkg.OrbxError):
            m.SearchByProjection_last(g, dF, angF, scale, bad, 15.0, assign.copy(), occ.copy())
        bad = dict(last); bad["level_window"] = 3
        with pytest.raises(pkg.OrbxError):
            m.SearchByProjection_last(g, dF, angF, scale, bad, 15.0, assign.copy(), occ.copy())
        bad = dict(last); bad["octave"] = last["octave"].copy(); bad["octave"][np.flatnonzero(last["valid"])[0]] = len(scale)
        with pytest.raises(pkg.OrbxError, match="out of range"):
            m.SearchByProjection_last(g, dF, angF, scale, bad, 15.0, assign.copy(), occ.copy())
        a0, o0 = assign.copy(), occ.copy()
        n0 = oracle.search_by_projection_last(g, dF, angF, scale, last, 15.0, True, a0, o0)
        a1, o1 = assign.copy(), occ.copy()
        assert m.SearchByProjection_last(g, dF, angF, scale, last, 15.0, a1, o1) == n0 and n0 > 20
        np.testing.assert_array_equal(a1, a0); np.testing.assert_array_equal(o1, o0)
        for c in (rig_match_cases.random_mp_call(1), rig_match_cases.random_last_call(1)):
            want = run_reference(c)
            ra, ro = c["assign"].copy(), c["occupied"].copy()
            m.nnratio, m.check_ori = c["nnratio"], c["check_ori"]
            if c["kind"] == "mp":
                rn = m.search_by_projection_rig(c["rig"], c["pts"], c["th"], ra, ro, c["far_points"], c["th_far"])
            else:
                rn = m.search_by_projection_last_rig(c["rig"], c["pts"], c["th"], ra, ro)
            assert rn == want[0] and rn > 20
            np.testing.assert_array_equal(ra, want[1]); np.testing.assert_array_equal(ro, want[2])
        fg, fd, fscale, fur, fs2, fpts = sm.make_fuse_case(5, n_pts=300)
        bi0, bd0 = oracle.fuse_search(fg, fd, fscale, fur, fs2, fpts, 3.0, True)
        bi1, bd1 = m.FuseSearch(fg, fd, fscale, fur, fs2, fpts, 3.0, True)
        np.testing.assert_array_equal(bi1, bi0); np.testing.assert_array_equal(bd1, bd0)
        assert (bi0 >= 0).sum() > 20
    finally:
        m.close()


@pytest.mark.parametrize("seed,th,ori", [(0, 7.0, True), (1, 15.0, True), (2, 15.0, False)])
def test_search_by_projection_last_frame(pkg, oracle, sm, seed, th, ori):
    g, dF, angF, scale, last, assign, occ = sm.make_last_frame_case(seed)
    a0, o0 = assign.copy(), occ.copy()
    n0 = oracle.search_by_projection_last(g, dF, angF, scale, last, th, ori, a0, o0)
    m = pkg.Matcher(0.9, ori)
    try:
        a1, o1 = assign.copy(), occ.copy()
        n1 = m.SearchByProjection_last(g, dF, angF, scale, last, th, a1, o1)
    finally:
        m.close()
    assert n1 == n0 and n0 > 100
    np.testing.assert_array_equal(a1, a0)
    np.testing.assert_array_equal(o1, o0)


@pytest.mark.parametrize("seed,th,dist,ori", [(0, 10.0, 100, True), (1, 3.0, 64, True), (2, 10.0, 100, False)])
def test_search_by_projection_keyframe(pkg, oracle, sm, seed, th, dist, ori):
    """SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (:1889-2010): relocalisation calls it with
    (10, 100) and (3, 64) (src/Tracking.cc:3791,3804)."""
    g, dF, angF, scale, pts, assign, occ = sm.make_kf_projection_case(seed)
    a0, o0 = assign.copy(), occ.copy()
    n0 = oracle.search_by_projection_kf(g, dF, angF, scale, pts, th, dist, ori, a0, o0)
    m = pkg.Matcher(0.9, ori)
    try:
        a1, o1 = assign.copy(), occ.copy()
        n1 = m.SearchByProjection_kf(g, dF, angF, scale, pts, th, dist, a1, o1)
    finally:
        m.close()
    assert n1 == n0 and n0 > 50
    np.testing.assert_array_equal(a1, a0)
    np.testing.assert_array_equal(o1, o0)


@pytest.mark.parametrize("seed,th,ratio", [(0, 8, 1.5), (1, 3, 1.0), (2, 30, 1.0)])
def test_search_by_projection_sim3(pkg, oracle, sm, seed, th, ratio):
    """SearchByProjection(KeyFrame*, Sim3f&, vpPoints, vpMatched, th, ratioHamming) (:427-532): loop closing calls it with
    (8, 1.5), (3..5, 1.0) and (30, 1.0) (src/LoopClosing.cc)."""
    g, dKF, angKF, scale, pts, assign, occ = sm.make_kf_projection_case(seed + 10)
    a0, o0 = assign.copy(), occ.copy()
    n0 = oracle.search_by_projection_sim3(g, dKF, scale, pts, th, ratio, a0, o0)
    m = pkg.Matcher(0.75, True)
    try:
        a1, o1 = assign.copy(), occ.copy()
        n1 = m.SearchByProjection_sim3(g, dKF, scale, pts, th, ratio, a1, o1)
    finally:
        m.close()
    assert n1 == n0 and n0 > 50
    np.testing.assert_array_equal(a1, a0)
    np.testing.assert_array_equal(o1, o0)


@pytest.mark.parametrize("seed,th,chi2,npts", [(0, 3.0, True, 3000), (1, 3.0, False, 3000), (2, 4.0, True, 1), (3, 2.5, True, 0),
                                               (4, 3.0, True, 20000)])
def test_fuse_search(pkg, oracle, sm, seed, th, chi2, npts):
    """search core of both ORBmatcher::Fuse overloads: best key point per candidate map point, one wave per point"""
    g, dKF, scale, u_right, inv_s2, pts = sm.make_fuse_case(seed, n_pts=npts)
    bi0, bd0 = oracle.fuse_search(g, dKF, scale, u_right, inv_s2, pts, th, chi2)
    m = pkg.Matcher(0.6, True)
    try:
        bi1, bd1 = m.FuseSearch(g, dKF, scale, u_right, inv_s2, pts, th, chi2)
    finally:
        m.close()
    np.testing.assert_array_equal(bi1, bi0)
    np.testing.assert_array_equal(bd1, bd0)
    if npts >= 3000:
        assert (bd0 <= 50).sum() > 0.2 * npts          # plenty of fusable points (TH_LOW) ...
        assert (bi0 < 0).sum() > 0                     # ... and some with an empty window / all candidates gated out


@pytest.mark.parametrize("seed,only_stereo,coarse,ori", [(0, False, False, True), (1, True, False, True), (2, False, True, False), (3, False, False, False)])
def test_search_for_triangulation(pkg, oracle, sm, seed, only_stereo, coarse, ori):
    """SearchForTriangulation (:907-1146): per-feature search inside shared vocabulary nodes, epipole / epipolar gates,
    `dist > bestDist -> continue` (the last equally good candidate wins), rotation histogram"""
    k1, k2, ep, F12, sigma2, scale = sm.make_triangulation_case(seed)
    n0, m0 = oracle.search_for_triangulation(k1, k2, ep, F12, sigma2, scale, only_stereo, coarse, ori)
    m = pkg.Matcher(0.6, ori)
    try:
        n1, m1 = m.SearchForTriangulation(k1, k2, ep, F12, sigma2, scale, only_stereo, coarse)
    finally:
        m.close()
    assert n1 == n0 and n0 > (5 if only_stereo else 60)
    np.testing.assert_array_equal(m1, m0)


@pytest.mark.parametrize("seed,win,ratio,ori", [(0, 100, 0.9, True), (1, 30, 0.9, True), (2, 100, 0.7, False)])
def test_search_for_initialization(pkg, oracle, sm, seed, win, ratio, ori):
    """SearchForInitialization (:648-763): level-0 features only, matched-distance feedback, stolen matches, ratio test"""
    f1, g2, d2, a2, scale = sm.make_initialization_case(seed)
    n0, m0 = oracle.search_for_initialization(f1, g2, d2, a2, win, ratio, ori)
    m = pkg.Matcher(ratio, ori)
    try:
        n1, m1 = m.SearchForInitialization(f1, g2, d2, a2, scale, win)
    finally:
        m.close()
    assert n1 == n0 and n0 > 100
    np.testing.assert_array_equal(m1, m0)
    assert n0 == int((m0 >= 0).sum())
    assert len(set(m0[m0 >= 0])) == n0                   # one-to-one after the stealing


def test_search_by_projection_last_batch(pkg, oracle, sm):
    """a wave per frame: the batched launch equals the per-frame oracle runs (ragged sizes, an empty query)"""
    cases, refs = [], []
    # ragged sizes, an empty query, and per-query stereo shares / level windows (every stream has its own motion)
    for i, (n, nl, frac, lw) in enumerate(((1000, 900, None, 0), (400, 700, 0.5, 1), (1000, 0, None, 0), (1500, 1200, 1.0, 2), (64, 50, 0.5, 0))):
        g, dF, angF, scale, last, assign, occ = sm.make_last_frame_case(30 + i, n=n, n_last=max(nl, 1), stereo_frac=frac, level_window=lw)
        if nl == 0:
            last = {k: v[:0].copy() for k, v in last.items()}
        a0, o0 = assign.copy(), occ.copy()
        n0 = oracle.search_by_projection_last(g, dF, angF, scale, last, 15.0, True, a0, o0)
        refs.append((n0, a0, o0))
        cases.append((g, dF, angF, scale, last, assign.copy(), occ.copy()))
    m = pkg.Matcher(0.9, True)
    try:
        ns = m.run_last_batch(m.prepare_last_batch(cases), 15.0)
    finally:
        m.close()
    for (n0, a0, o0), n1, c in zip(refs, ns, cases):
        assert n1 == n0
        np.testing.assert_array_equal(c[5], a0); np.testing.assert_array_equal(c[6], o0)


def test_search_by_projection_last_batch_device(pkg, oracle, sm):
    """the device-resident batch entry of SearchByProjection(CurrentFrame, LastFrame): frames as [batch][cap] key-point records +
    descriptors + counts in HBM (what orbx_extract_batch_device leaves), last-frame points as device arrays, ragged counts, the
    grid built on the device -- against the oracle frame by frame (assignments, occupancy, match counts)"""
    import torch
    dev = torch.device("cuda", 0)
    B, cap, pcap = 12, 1100, 1000
    cases = [sm.make_last_frame_case(40 + i, n=1000 - 37 * (i % 5), n_last=900 - 41 * (i % 4)) for i in range(B)]
    scale = cases[0][3]
    kps = np.zeros((B, cap), pkg.KP_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); nn = np.zeros(B, np.int32)
    pv = np.zeros((B, pcap), np.uint8); pu = np.zeros((B, pcap), np.float32); pw = np.zeros((B, pcap), np.float32)
    po = np.zeros((B, pcap), np.int32); pa = np.zeros((B, pcap), np.float32); pd = np.zeros((B, pcap, 32), np.uint8); pn = np.zeros(B, np.int32)
    ph = np.zeros((B, pcap), np.uint8)
    assign = np.full((B, cap), -1, np.int32); occ = np.zeros((B, cap), np.uint8)
    for b, (g, dF, aF, sc, last, a, o) in enumerate(cases):
        n = len(g["x"]); nn[b] = n
        kps[b, :n]["x"] = g["x"]; kps[b, :n]["y"] = g["y"]; kps[b, :n]["octave"] = g["octave"]; kps[b, :n]["angle"] = aF
        desc[b, :n] = dF
        m_ = len(last["u"]); pn[b] = m_
        pv[b, :m_] = last["valid"]; pu[b, :m_] = last["u"]; pw[b, :m_] = last["v"]; po[b, :m_] = last["octave"]; pa[b, :m_] = last["angle"]; pd[b, :m_] = last["desc"]; ph[b, :m_] = last["has_obs"]
        assign[b, :n] = a; occ[b, :n] = o
        assert (g["min_x"], g["min_y"], g["max_x"], g["max_y"]) == (cases[0][0]["min_x"], cases[0][0]["min_y"], cases[0][0]["max_x"], cases[0][0]["max_y"])
    t = lambda a_: torch.from_numpy(np.ascontiguousarray(a_).view(np.uint8).reshape(-1)).to(dev)
    d = {k: t(v) for k, v in dict(kps=kps, desc=desc, n=nn, pv=pv, pu=pu, pw=pw, po=po, pa=pa, pd=pd, pn=pn, ph=ph, assign=assign, occ=occ).items()}
    d_nm = torch.zeros(B, dtype=torch.int32, device=dev)
    g0 = cases[0][0]
    m = pkg.Matcher(0.9, True)
    try:
        m.SearchByProjection_last_batch_device((d["kps"].data_ptr(), d["desc"].data_ptr(), d["n"].data_ptr(), cap),
                                               (d["pv"].data_ptr(), d["pu"].data_ptr(), d["pw"].data_ptr(), d["po"].data_ptr(), d["pa"].data_ptr(), d["pd"].data_ptr(), d["pn"].data_ptr(), pcap, d["ph"].data_ptr()),
                                               B, 15.0, d["assign"].data_ptr(), d["occ"].data_ptr(), d_nm.data_ptr(), torch.cuda.current_stream().cuda_stream,
                                               bounds=(g0["min_x"], g0["min_y"], g0["max_x"], g0["max_y"]), scale_factors=scale)
        torch.cuda.synchronize()
    finally:
        m.close()
    a1 = d["assign"].cpu().numpy().view(np.int32).reshape(B, cap); o1 = d["occ"].cpu().numpy().reshape(B, cap); nm = d_nm.cpu().numpy()
    for b, (g, dF, aF, sc, last, a, o) in enumerate(cases):
        a0, o0 = a.copy(), o.copy()
        n0 = oracle.search_by_projection_last(g, dF, aF, sc, last, 15.0, True, a0, o0)
        n = len(g["x"])
        assert nm[b] == n0 > 100, "frame %d" % b
        np.testing.assert_array_equal(a1[b, :n], a0); np.testing.assert_array_equal(o1[b, :n], o0)


def test_search_by_projection_last_batch_device_empty_frames(pkg, sm):
    """frames without features, frames without points, a batch of one: no matches, nothing written"""
    import torch
    dev = torch.device("cuda", 0)
    B, cap, pcap = 3, 64, 32
    z = lambda n, dt: torch.zeros(n, dtype=dt, device=dev)
    kps = z(B * cap * 28, torch.uint8); desc = z(B * cap * 32, torch.uint8); nn = torch.tensor([0, 5, 0], dtype=torch.int32, device=dev)
    pv = z(B * pcap, torch.uint8); pu = z(B * pcap, torch.float32); pw = z(B * pcap, torch.float32); po = z(B * pcap, torch.int32)
    pa = z(B * pcap, torch.float32); pd = z(B * pcap * 32, torch.uint8); pn = torch.tensor([7, 0, 0], dtype=torch.int32, device=dev)
    assign = torch.full((B * cap,), -1, dtype=torch.int32, device=dev); occ = z(B * cap, torch.uint8); nm = torch.full((B,), 99, dtype=torch.int32, device=dev)
    m = pkg.Matcher(0.9, True)
    try:
        m.SearchByProjection_last_batch_device((kps.data_ptr(), desc.data_ptr(), nn.data_ptr(), cap),
                                               (pv.data_ptr(), pu.data_ptr(), pw.data_ptr(), po.data_ptr(), pa.data_ptr(), pd.data_ptr(), pn.data_ptr(), pcap),
                                               B, 15.0, assign.data_ptr(), occ.data_ptr(), nm.data_ptr(), torch.cuda.current_stream().cuda_stream,
                                               bounds=(0.0, 0.0, 640.0, 480.0), scale_factors=np.float32(1.2) ** np.arange(8, dtype=np.float32))
        torch.cuda.synchronize()
    finally:
        m.close()
    assert nm.cpu().tolist() == [0, 0, 0] and int((assign != -1).sum().item()) == 0


def test_search_by_projection_batch_device(pkg, oracle, sm):
    """the device-resident batch entry of SearchByProjection(Frame, MapPoints): ragged frames and point sets, far-point gate, ratio
    test -- against the oracle frame by frame"""
    import torch
    dev = torch.device("cuda", 0)
    B, cap, pcap = 10, 1100, 1000
    cases = [sm.make_projection_case(60 + i, n=1000 - 41 * (i % 4), n_mp=900 - 53 * (i % 5)) for i in range(B)]
    scale = cases[0][3]
    kps = np.zeros((B, cap), pkg.KP_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); nn = np.zeros(B, np.int32)
    pv = np.zeros((B, pcap), np.uint8); pu = np.zeros((B, pcap), np.float32); pw = np.zeros((B, pcap), np.float32); po = np.zeros((B, pcap), np.int32)
    pd = np.zeros((B, pcap, 32), np.uint8); pn = np.zeros(B, np.int32); ph = np.zeros((B, pcap), np.uint8)
    vc = np.zeros((B, pcap), np.float32); dp = np.zeros((B, pcap), np.float32); bd = np.zeros((B, pcap), np.uint8)
    assign = np.full((B, cap), -1, np.int32); occ = np.zeros((B, cap), np.uint8)
    for b, (g, dF, aF, sc, mp, a, o) in enumerate(cases):
        n = len(g["x"]); nn[b] = n
        kps[b, :n]["x"] = g["x"]; kps[b, :n]["y"] = g["y"]; kps[b, :n]["octave"] = g["octave"]; kps[b, :n]["angle"] = aF
        desc[b, :n] = dF
        m_ = len(mp["u"]); pn[b] = m_
        pv[b, :m_] = mp["in_view"]; pu[b, :m_] = mp["u"]; pw[b, :m_] = mp["v"]; po[b, :m_] = mp["level"]; pd[b, :m_] = mp["desc"]; ph[b, :m_] = mp["has_obs"]
        vc[b, :m_] = mp["view_cos"]; dp[b, :m_] = mp["depth"]; bd[b, :m_] = mp["bad"]
        assign[b, :n] = a; occ[b, :n] = o
    t = lambda a_: torch.from_numpy(np.ascontiguousarray(a_).view(np.uint8).reshape(-1)).to(dev)
    d = {k: t(v) for k, v in dict(kps=kps, desc=desc, n=nn, pv=pv, pu=pu, pw=pw, po=po, pd=pd, pn=pn, ph=ph, vc=vc, dp=dp, bd=bd, assign=assign, occ=occ).items()}
    d_nm = torch.zeros(B, dtype=torch.int32, device=dev)
    g0 = cases[0][0]
    m = pkg.Matcher(0.8, True)
    try:
        m.SearchByProjection_batch_device((d["kps"].data_ptr(), d["desc"].data_ptr(), d["n"].data_ptr(), cap),
                                          (d["pv"].data_ptr(), d["pu"].data_ptr(), d["pw"].data_ptr(), d["po"].data_ptr(), 0, d["pd"].data_ptr(), d["pn"].data_ptr(), pcap, d["ph"].data_ptr()),
                                          (d["vc"].data_ptr(), d["dp"].data_ptr(), d["bd"].data_ptr()), B, 3.0, d["assign"].data_ptr(), d["occ"].data_ptr(), d_nm.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream, bounds=(g0["min_x"], g0["min_y"], g0["max_x"], g0["max_y"]), scale_factors=scale,
                                          far_points=True, th_far=20.0)
        torch.cuda.synchronize()
    finally:
        m.close()
    a1 = d["assign"].cpu().numpy().view(np.int32).reshape(B, cap); o1 = d["occ"].cpu().numpy().reshape(B, cap); nm = d_nm.cpu().numpy()
    for b, (g, dF, aF, sc, mp, a, o) in enumerate(cases):
        a0, o0 = a.copy(), o.copy()
        n0 = oracle.search_by_projection(g, dF, sc, mp, 3.0, 0.8, a0, o0, b_far=True, th_far=20.0)
        n = len(g["x"])
        assert nm[b] == n0 > 100, "frame %d" % b
        np.testing.assert_array_equal(a1[b, :n], a0); np.testing.assert_array_equal(o1[b, :n], o0)


@pytest.mark.parametrize("n", [1600, 1700, 1750, 1850, 1950, 2100])
def test_projection_searches_around_the_lds_staging_limit(pkg, oracle, sm, n):
    """found by probing: the decision whether a frame is staged in LDS compared its size with a fixed 150 KB and ignored the search kernel's
    own static LDS, so frames of about 1 700 .. 1 900 features (staged size between the true budget and 150 KB) failed with ORBX_ERR_HIP --
    and left an error behind that failed the next call too.  The budget now comes from the kernels' attributes: both tracking searches,
    host entry and device-resident entry, equal the oracle across the limit."""
    import torch
    dev = torch.device("cuda", 0)
    g, dF, aF, sc, last, a, oc = sm.make_last_frame_case(11, n=n, n_last=900)
    a0, o0 = a.copy(), oc.copy()
    n0 = oracle.search_by_projection_last(g, dF, aF, sc, last, 15.0, True, a0, o0)
    g2, dF2, aF2, sc2, mp, a2, oc2 = sm.make_projection_case(11, n=n, n_mp=1500)
    b0, p0 = a2.copy(), oc2.copy()
    k0 = oracle.search_by_projection(g2, dF2, sc2, mp, 3.0, 0.8, b0, p0)
    m = pkg.Matcher(0.8, True)
    try:
        a1, o1 = a.copy(), oc.copy()
        n1 = m.SearchByProjection_last(g, dF, aF, sc, last, 15.0, a1, o1)
        b1, p1 = a2.copy(), oc2.copy()
        k1 = m.SearchByProjection(g2, dF2, sc2, mp, 3.0, b1, p1)
        # the device-resident entry on the same frame (cap = n)
        kps = np.zeros((1, n), pkg.KP_DTYPE)
        kps[0]["x"] = g["x"]; kps[0]["y"] = g["y"]; kps[0]["octave"] = g["octave"]; kps[0]["angle"] = aF
        tt = lambda x_: torch.from_numpy(np.ascontiguousarray(x_).view(np.uint8).reshape(-1)).to(dev)
        d = {k_: tt(v_) for k_, v_ in dict(kps=kps, desc=dF, n=np.array([n], np.int32), pv=last["valid"], pu=last["u"], pw=last["v"], po=last["octave"], pa=last["angle"],
                                           pd=last["desc"], pn=np.array([len(last["u"])], np.int32), ph=last["has_obs"], assign=a.copy(), occ=oc.copy()).items()}
        d_nm = torch.zeros(1, dtype=torch.int32, device=dev)
        m2 = pkg.Matcher(0.9, True)
        m2.SearchByProjection_last_batch_device((d["kps"].data_ptr(), d["desc"].data_ptr(), d["n"].data_ptr(), n),
                                                (d["pv"].data_ptr(), d["pu"].data_ptr(), d["pw"].data_ptr(), d["po"].data_ptr(), d["pa"].data_ptr(), d["pd"].data_ptr(), d["pn"].data_ptr(), len(last["u"]), d["ph"].data_ptr()),
                                                1, 15.0, d["assign"].data_ptr(), d["occ"].data_ptr(), d_nm.data_ptr(), torch.cuda.current_stream().cuda_stream,
                                                bounds=(g["min_x"], g["min_y"], g["max_x"], g["max_y"]), scale_factors=sc)
        torch.cuda.synchronize()
        m2.close()
        a3 = d["assign"].cpu().numpy().view(np.int32); o3 = d["occ"].cpu().numpy()
    finally:
        m.close()
    assert (n1, k1) == (n0, k0)
    np.testing.assert_array_equal(a1, a0); np.testing.assert_array_equal(o1, o0)
    np.testing.assert_array_equal(b1, b0); np.testing.assert_array_equal(p1, p0)
    assert int(d_nm.item()) == n0
    np.testing.assert_array_equal(a3, a0); np.testing.assert_array_equal(o3, o0)


@pytest.mark.parametrize("n", [8193, 20000])
def test_projection_searches_on_large_frames(pkg, oracle, sm, n):
    """the two branches of the host driver that frames of ordinary size never take.  8193 features: one more than the device's grid sort
    takes, so Frame::AssignFeaturesToGrid runs on the host -- for the whole batch when one of its frames is that large (the second half:
    the same frame in one launch with a 500-feature frame).  20000 features: the block-parallel search's two tables alone would need more
    than 9 bytes a feature, over 160 KB of LDS whatever the static part is, so the sequential kernel runs, unstaged.  (Its staged
    instance is reachable only through the ORBM_PROJ_SEQUENTIAL knob, read once per process: tools/proj_timing.py covers it.)"""
    big = sm.make_last_frame_case(21, n=n, n_last=130)
    g, dF, aF, sc, last, a, oc = big
    a0, o0 = a.copy(), oc.copy()
    n0 = oracle.search_by_projection_last(g, dF, aF, sc, last, 15.0, True, a0, o0)
    g2, dF2, aF2, sc2, mp, a2, oc2 = sm.make_projection_case(21, n=n, n_mp=130)
    b0, p0 = a2.copy(), oc2.copy()
    k0 = oracle.search_by_projection(g2, dF2, sc2, mp, 3.0, 0.8, b0, p0)
    assert n0 > 40 and k0 > 40
    m = pkg.Matcher(0.8, True)
    try:
        a1, o1 = a.copy(), oc.copy()
        n1 = m.SearchByProjection_last(g, dF, aF, sc, last, 15.0, a1, o1)
        b1, p1 = a2.copy(), oc2.copy()
        k1 = m.SearchByProjection(g2, dF2, sc2, mp, 3.0, b1, p1)
        assert (n1, k1) == (n0, k0)
        np.testing.assert_array_equal(a1, a0); np.testing.assert_array_equal(o1, o0)
        np.testing.assert_array_equal(b1, b0); np.testing.assert_array_equal(p1, p0)
        if n == 8193:
            small = sm.make_last_frame_case(22, n=500, n_last=130)
            sa, so = small[5].copy(), small[6].copy()
            sn = oracle.search_by_projection_last(small[0], small[1], small[2], small[3], small[4], 15.0, True, sa, so)
            cases = [big[:5] + (a.copy(), oc.copy()), small[:5] + (small[5].copy(), small[6].copy())]
            assert m.run_last_batch(m.prepare_last_batch(cases), 15.0) == [n0, sn] and sn > 40
            np.testing.assert_array_equal(cases[0][5], a0); np.testing.assert_array_equal(cases[0][6], o0)
            np.testing.assert_array_equal(cases[1][5], sa); np.testing.assert_array_equal(cases[1][6], so)
    finally:
        m.close()


def _crowd(rs, g, desc, targets, followers=7):
    """`targets` features of the frame, each with `followers` other features moved next to it (same level, a few bits of its descriptor
    flipped): points aimed at a target find a queue of acceptable candidates, so the later ones get what the earlier ones left."""
    idx = rs.choice(len(desc), min(targets * (followers + 1), len(desc)), replace=False)
    hot = idx[:targets]
    for k, j in enumerate(idx[targets:]):
        h = hot[k % targets]
        g["x"][j] = g["x"][h] + rs.uniform(-2, 2); g["y"][j] = g["y"][h] + rs.uniform(-2, 2); g["octave"][j] = g["octave"][h]
        desc[j] = desc[h] ^ np.packbits(rs.uniform(size=256) < 0.02 * (1 + k // targets))
    g["x"][:] = np.clip(g["x"], 0, g["max_x"] - 1); g["y"][:] = np.clip(g["y"], 0, g["max_y"] - 1)
    return hot


@pytest.mark.parametrize("seed,targets,noise", [(0, 4, 0.02), (1, 40, 0.05), (2, 1, 0.0), (3, 120, 0.1)])
def test_projection_searches_under_contention(pkg, oracle, sm, seed, targets, noise):
    """Many points after the same few features: every point's best candidate has usually been taken by an earlier point, often its second
    best as well -- the resolution's stand-in rule (a free speculative second best IS the best of the rest where only the best counts),
    the window walk behind it, the map-point search's ratio test on a shrinking pool and same-feature writers inside one block of 64.
    Point order decides everything here; the result must be the sequential loop's."""
    rs = np.random.RandomState(40 + seed)
    for n_pts in (64, 500, 1500):
        # SearchByProjection(CurrentFrame, LastFrame) with and without the orientation check
        g, dF, aF, sc, last, a, oc = sm.make_last_frame_case(20 + seed, n=1000, n_last=n_pts)
        hot = _crowd(rs, g, dF, targets)
        tgt = hot[rs.randint(0, targets, n_pts)]
        last["u"] = (g["x"][tgt] + rs.normal(0, 1.0, n_pts)).astype(np.float32); last["v"] = (g["y"][tgt] + rs.normal(0, 1.0, n_pts)).astype(np.float32)
        last["octave"] = g["octave"][tgt].astype(np.int32)
        last["desc"] = np.ascontiguousarray(dF[tgt] ^ (np.packbits(rs.uniform(size=(n_pts, 256)) < noise, axis=1)))
        last["valid"][:] = 1
        for ori in (True, False):
            a0, o0 = a.copy(), oc.copy()
            n0 = oracle.search_by_projection_last(g, dF, aF, sc, last, 15.0, ori, a0, o0)
            m = pkg.Matcher(0.9, ori)
            try:
                a1, o1 = a.copy(), oc.copy()
                n1 = m.SearchByProjection_last(g, dF, aF, sc, last, 15.0, a1, o1)
            finally:
                m.close()
            assert n1 == n0, (n_pts, ori)
            np.testing.assert_array_equal(a1, a0); np.testing.assert_array_equal(o1, o0)
        # SearchByProjection(Frame, MapPoints): best AND second best among the free features
        g2, dF2, aF2, sc2, mp, a2, oc2 = sm.make_projection_case(20 + seed, n=1000, n_mp=n_pts)
        hot = _crowd(rs, g2, dF2, targets)
        tgt = hot[rs.randint(0, targets, n_pts)]
        mp["u"] = (g2["x"][tgt] + rs.normal(0, 1.0, n_pts)).astype(np.float32); mp["v"] = (g2["y"][tgt] + rs.normal(0, 1.0, n_pts)).astype(np.float32)
        mp["level"] = g2["octave"][tgt].astype(np.int32)
        mp["desc"] = np.ascontiguousarray(dF2[tgt] ^ (np.packbits(rs.uniform(size=(n_pts, 256)) < noise, axis=1)))
        mp["in_view"][:] = 1; mp["bad"][:] = 0
        b0, p0 = a2.copy(), oc2.copy()
        k0 = oracle.search_by_projection(g2, dF2, sc2, mp, 5.0, 0.9, b0, p0)
        m = pkg.Matcher(0.9, True)
        try:
            b1, p1 = a2.copy(), oc2.copy()
            k1 = m.SearchByProjection(g2, dF2, sc2, mp, 5.0, b1, p1)
        finally:
            m.close()
        assert k1 == k0, n_pts
        np.testing.assert_array_equal(b1, b0); np.testing.assert_array_equal(p1, p0)


@pytest.mark.parametrize("n_pts", [1, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 320])
def test_projection_searches_at_block_boundaries(pkg, oracle, sm, n_pts):
    """point counts around the multiples of 64: the search kernel takes the points in blocks of 64 through a three-stage pipeline (resolve
    block b, walk block b + 1, build block b + 2, loads of block b + 3 in flight) -- the first / last / only block and the blocks whose
    successors do not exist are the cases its conditions have to get right."""
    g, dF, aF, sc, last, a, oc = sm.make_last_frame_case(60, n=1000, n_last=n_pts)
    a0, o0 = a.copy(), oc.copy()
    n0 = oracle.search_by_projection_last(g, dF, aF, sc, last, 15.0, True, a0, o0)
    g2, dF2, aF2, sc2, mp, a2, oc2 = sm.make_projection_case(60, n=1000, n_mp=n_pts)
    b0, p0 = a2.copy(), oc2.copy()
    k0 = oracle.search_by_projection(g2, dF2, sc2, mp, 4.0, 0.8, b0, p0)
    m = pkg.Matcher(0.8, True)
    try:
        a1, o1 = a.copy(), oc.copy()
        n1 = m.SearchByProjection_last(g, dF, aF, sc, last, 15.0, a1, o1)
        b1, p1 = a2.copy(), oc2.copy()
        k1 = m.SearchByProjection(g2, dF2, sc2, mp, 4.0, b1, p1)
    finally:
        m.close()
    assert (n1, k1) == (n0, k0)
    np.testing.assert_array_equal(a1, a0); np.testing.assert_array_equal(o1, o0)
    np.testing.assert_array_equal(b1, b0); np.testing.assert_array_equal(p1, p0)


@pytest.mark.parametrize("seed,ori", [(0, True), (1, False)])
def test_search_by_bow_node_sizes(pkg, oracle, synth, seed, ori):
    """vocabulary nodes of 1 .. 600 Frame features: the kernel keeps the candidates of a node in registers up to 32 / 64 / 96 of them, walks
    larger nodes from memory with a bitmask per lane up to 512 and leaves the rest to one lane -- every path, and the boundaries between
    them, against the oracle (real frames through a vocabulary hold a few nodes beyond 32 features; the synthetic match sets none)."""
    ms = synth.make_match_set(30 + seed, n=2600)
    n = len(ms["dF"])
    sizes = [1, 15, 16, 17, 31, 32, 33, 47, 48, 49, 63, 64, 65, 80, 95, 96, 97, 130, 200, 513, 600]
    node_f = np.zeros(n, np.int64)
    pos = 0
    for k_, sz in enumerate(sizes):
        node_f[pos:pos + sz] = 10 + 3 * k_
        pos += sz
    rs = np.random.RandomState(5 + seed)
    node_f[pos:] = 500 + rs.randint(0, 8, n - pos)          # the rest: a few nodes of ordinary size
    # a key-frame feature mostly falls into the node of the frame feature it is a copy of; some go astray
    node_k = node_f[ms["perm"]].copy()
    astray = rs.uniform(size=n) < 0.1
    node_k[astray] = rs.choice(np.unique(node_f), int(astray.sum()))
    fvF, fvK = synth.feature_vector(node_f), synth.feature_vector(node_k)
    n0, m0 = oracle.search_by_bow(ms["dKF"], ms["validKF"], ms["angKF"], fvK, ms["dF"], ms["angF"], fvF, 0.75, ori)
    m = pkg.Matcher(0.75, ori)
    try:
        n1, m1 = m.SearchByBoW(ms["dKF"], ms["validKF"], ms["angKF"], fvK, ms["dF"], ms["angF"], fvF)
        k0, q0 = oracle.search_by_bow_kfkf(ms["dKF"], ms["validKF"], ms["angKF"], fvK, ms["dF"], np.ones(n, np.uint8), ms["angF"], fvF, 0.75, ori)
        k1, q1 = m.SearchByBoW_KFKF(ms["dKF"], ms["validKF"], ms["angKF"], fvK, ms["dF"], np.ones(n, np.uint8), ms["angF"], fvF)
    finally:
        m.close()
    assert n1 == n0 and n0 > 500
    np.testing.assert_array_equal(m1, m0)
    assert k1 == k0
    np.testing.assert_array_equal(q1, q0)
