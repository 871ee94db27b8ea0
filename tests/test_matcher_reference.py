"""CPU checks that pin the matcher oracle a second time: (1) every restatement of tests/matcher_reference.py equals the oracle on
random synthetic cases that are not degenerate, (2) on every hand-built boundary scenario of tests/matcher_boundary_cases.py
the stated expectation, the restatement and the oracle agree (reference src/ORBmatcher.cc; PARITY UNPINNED otherwise)."""
import re

import numpy as np
import pytest

import matcher_boundary_cases as mbc
import matcher_reference as ref


def _big_nodes(synth, ms, seed):
    """vocabulary nodes of 1 .. 130 frame features (as test_search_by_bow_node_sizes lays them out, smaller)"""
    n = len(ms["dF"])
    sizes = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 130]
    node_f = np.zeros(n, np.int64)
    pos = 0
    for k_, sz in enumerate(sizes):
        node_f[pos:pos + sz] = 10 + 3 * k_
        pos += sz
    rs = np.random.RandomState(5 + seed)
    node_f[pos:] = 500 + rs.randint(0, 8, n - pos)
    node_k = node_f[ms["perm"]].copy()
    astray = rs.uniform(size=n) < 0.1
    node_k[astray] = rs.choice(np.unique(node_f), int(astray.sum()))
    return synth.feature_vector(node_k), synth.feature_vector(node_f)


@pytest.mark.parametrize("seed,n,ratio,ori,big", [(0, 400, 0.7, True, False), (1, 500, 0.9, False, False), (2, 500, 0.75, True, True)])
def test_bow_vs_numpy(oracle, synth, seed, n, ratio, ori, big):
    ms = synth.make_match_set(seed, n=n)
    fvK, fvF = _big_nodes(synth, ms, seed) if big else (ms["fvKF"], ms["fvF"])
    a = (ms["dKF"], ms["validKF"], ms["angKF"], fvK, ms["dF"], ms["angF"], fvF, ratio, ori)
    n0, m0 = oracle.search_by_bow(*a)
    n1, m1 = ref.search_by_bow(*a)
    assert n1 == n0 and n1 >= 30
    np.testing.assert_array_equal(m1, m0)
    valid2 = (np.random.RandomState(seed).uniform(size=n) < 0.9).astype(np.uint8)
    b = (ms["dKF"], ms["validKF"], ms["angKF"], fvK, ms["dF"], valid2, ms["angF"], fvF, ratio, ori)
    k0, q0 = oracle.search_by_bow_kfkf(*b)
    k1, q1 = ref.search_by_bow_kfkf(*b)
    assert k1 == k0 and k1 >= 30
    np.testing.assert_array_equal(q1, q0)


@pytest.mark.parametrize("seed,th,dist,ori", [(0, 10.0, 100, True), (1, 3.0, 64, True), (2, 10.0, 100, False)])
def test_keyframe_projection_vs_numpy(oracle, sm, seed, th, dist, ori):
    g, dF, angF, scale, pts, assign, occ = sm.make_kf_projection_case(seed, n=500, n_pts=400)
    a0, o0 = assign.copy(), occ.copy()
    n0 = oracle.search_by_projection_kf(g, dF, angF, scale, pts, th, dist, ori, a0, o0)
    a1, o1 = assign.copy(), occ.copy()
    n1 = ref.search_by_projection_kf(g, dF, angF, scale, pts, th, dist, ori, a1, o1)
    assert n1 == n0 and n1 >= 30
    np.testing.assert_array_equal(a1, a0); np.testing.assert_array_equal(o1, o0)


@pytest.mark.parametrize("seed,th,ratio", [(0, 8, 1.5), (1, 3, 1.0), (2, 30, 1.0)])
def test_sim3_projection_vs_numpy(oracle, sm, seed, th, ratio):
    g, dKF, angKF, scale, pts, assign, occ = sm.make_kf_projection_case(seed + 10, n=500, n_pts=400)
    a0, o0 = assign.copy(), occ.copy()
    n0 = oracle.search_by_projection_sim3(g, dKF, scale, pts, th, ratio, a0, o0)
    a1, o1 = assign.copy(), occ.copy()
    n1 = ref.search_by_projection_sim3(g, dKF, scale, pts, th, ratio, a1, o1)
    assert n1 == n0 and n1 >= 30
    np.testing.assert_array_equal(a1, a0); np.testing.assert_array_equal(o1, o0)


@pytest.mark.parametrize("seed,th,chi2", [(0, 3.0, True), (1, 3.0, False), (2, 4.0, True)])
def test_fuse_search_vs_numpy(oracle, sm, seed, th, chi2):
    g, dKF, scale, u_right, inv_s2, pts = sm.make_fuse_case(seed, n=500, n_pts=400)
    bi0, bd0 = oracle.fuse_search(g, dKF, scale, u_right, inv_s2, pts, th, chi2)
    bi1, bd1 = ref.fuse_search(g, dKF, scale, u_right, inv_s2, pts, th, chi2)
    assert int((bd1 <= ref.TH_LOW).sum()) >= 30 and int((bi1 < 0).sum()) > 0
    np.testing.assert_array_equal(bi1, bi0); np.testing.assert_array_equal(bd1, bd0)


@pytest.mark.parametrize("seed,only_stereo,coarse,ori", [(0, False, False, True), (1, True, False, True), (2, False, True, False)])
def test_triangulation_vs_numpy(oracle, sm, seed, only_stereo, coarse, ori):
    k1, k2, ep, F12, sigma2, scale = sm.make_triangulation_case(seed, n=500)
    if only_stereo:         # the synthetic case has 40 % stereo features on either side, too few pairs at this size: make it 90 %
        rs = np.random.RandomState(seed)
        k1 = dict(k1, stereo=(rs.uniform(size=500) < 0.9).astype(np.uint8)); k2 = dict(k2, stereo=(rs.uniform(size=500) < 0.9).astype(np.uint8))
    n0, m0 = oracle.search_for_triangulation(k1, k2, ep, F12, sigma2, scale, only_stereo, coarse, ori)
    n1, m1 = ref.search_for_triangulation(k1, k2, ep, F12, sigma2, scale, only_stereo, coarse, ori)
    assert n1 == n0 and n1 >= 30
    np.testing.assert_array_equal(m1, m0)


@pytest.mark.parametrize("seed,win,ratio,ori", [(0, 100, 0.9, True), (1, 30, 0.9, True), (2, 100, 0.7, False)])
def test_initialization_vs_numpy(oracle, sm, seed, win, ratio, ori):
    f1, g2, d2, a2, scale = sm.make_initialization_case(seed, n=500)
    n0, m0 = oracle.search_for_initialization(f1, g2, d2, a2, win, ratio, ori)
    n1, m1 = ref.search_for_initialization(f1, g2, d2, a2, win, ratio, ori)
    assert n1 == n0 and n1 >= 30
    np.testing.assert_array_equal(m1, m0)


def test_three_maxima_and_rotation_bin_vs_oracle(oracle):
    import ctypes as C
    rs = np.random.RandomState(3)
    hists = [rs.randint(0, 4, 30) for _ in range(200)] + [rs.randint(0, 40, 30) * (rs.uniform(size=30) < 0.2) for _ in range(200)]
    hists += [np.zeros(30, int), np.eye(30, dtype=int)[4] * 7, np.array([10, 1] + [0] * 28), np.array([0] * 27 + [3, 30, 3])]
    for h in hists:
        c = np.ascontiguousarray(h, np.int32)
        i1, i2, i3 = C.c_int(), C.c_int(), C.c_int()
        oracle.lib.orbm_oracle_three_maxima(c.ctypes.data_as(C.c_void_p), 30, C.byref(i1), C.byref(i2), C.byref(i3))
        assert ref.three_maxima(c) == (i1.value, i2.value, i3.value), h
    # the bin of round(rot * (1.0f/30)): halves go away from zero, 29.5 and above wrap to bin 0
    assert [ref.rot_bin(a, 0.0) for a in (0.0, 14.9, 15.0, 45.0, 75.0, 359.0)] == [0, 0, 1, 2, 3, 12]
    assert ref.rot_bin(10.0, 25.0) == ref.rot_bin(345.0, 0.0) == 12 and ref.rot_bin(0.0, 1.0) == 12


def test_grid_walk_equals_the_window_of_the_tracking_restatement(sm):
    """the literal cell walk of Frame::GetFeaturesInArea here and the order-and-box restatement of test_projection_oracle.py
    give the same candidates in the same order"""
    g, dF, angF, scale, last, assign, occ = sm.make_last_frame_case(1, n=500, n_last=300)
    grid, order = ref.Grid(g), ref._visit_order(g)
    total = 0
    for i in range(300):
        oc = int(last["octave"][i]); r = np.float32(15.0) * scale[oc]
        for lo, hi in ((oc - 1, oc + 1), (oc, -1), (0, oc), (-1, -1)):
            a = grid.features_in_area(last["u"][i], last["v"][i], r, lo, hi)
            b = ref._window(g, order, last["u"][i], last["v"][i], r, lo, hi)
            assert a == list(b)
            total += len(a)
    assert total > 1000


# ---- the boundary scenarios --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(mbc.CALLS))
def test_boundary_call_expectation_equals_restatement_equals_oracle(oracle, name):
    call = mbc.CALLS[name]()
    want = mbc.expected(call)
    got_ref = mbc.run(call, mbc.reference_backend())
    got_orc = mbc.run(call, mbc.oracle_backend(oracle))
    mbc.assert_same(got_ref, want, "restatement vs stated expectation")
    mbc.assert_same(got_orc, want, "oracle vs stated expectation")


def test_every_scenario_names_its_reference_line_and_every_family_shows_both_outcomes():
    seen = {}
    for name in sorted(mbc.CALLS):
        call = mbc.CALLS[name]()
        assert call["scenarios"], name
        for s in call["scenarios"]:
            assert re.match(r":\d+", s["line"]), (name, s)
            seen.setdefault(s["family"], set()).add(bool(s["accepted"]))
    assert set(seen) == set(mbc.FAMILIES), sorted(set(mbc.FAMILIES) ^ set(seen))
    for fam, outcomes in seen.items():
        assert outcomes == {True, False}, fam
