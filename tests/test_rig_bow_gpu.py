"""k_bow_rig and k_tri_rig (orb_slam3-1_amd/csrc/orbm_rig_bow.inc) against the plain loops of tests/rig_bow_reference.py: integer-equal on
the hand-built calls, the shape calls and the seeded random calls of tests/rig_bow_cases.py, alone and batched.  Key-frame-1
features with a borderline Hamming survivor (tests/fisheye_stereo_reference.borderline on the float64 evaluation; capped at 2 % of a
case by tests/test_rig_bow_reference.py) are left out of the match12 comparison of the random triangulation calls."""
import numpy as np
import pytest

import rig_bow_cases as cases
import rig_bow_reference as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def matchers(pkg):
    made = {}

    def get(nnratio, check_ori):
        key = (float(nnratio), bool(check_ori))
        if key not in made:
            made[key] = pkg.Matcher(nnratio, check_ori)
        return made[key]
    yield get
    for m in made.values():
        m.close()


def _same(got, want, what):
    n, m = got
    wn, wm = want
    m, wm = np.asarray(m), np.asarray(wm)
    bad = np.nonzero(m != wm)[0]
    assert not len(bad) and n == wn, "%s: count %d (want %d), %d slots differ, first %s: got %s want %s" % (what, n, wn, len(bad), bad[:8], m[bad[:8]], wm[bad[:8]])


@pytest.mark.parametrize("name", sorted(cases.bow_hand_cases()))
def test_bow_hand_built(matchers, name):
    c = cases.bow_hand_cases()[name]
    _same(matchers(c["nnratio"], c["check_ori"]).search_by_bow_rig(c["call"]), (c["want_n"], c["want_match"]), name)


@pytest.mark.parametrize("name", sorted(cases.bow_shape_cases()))
def test_bow_shapes(matchers, name):
    call, ori = cases.bow_shape_cases()[name]
    _same(matchers(cases.NNRATIO, ori).search_by_bow_rig(call), cases.bow_expected("shape", name), name)


@pytest.mark.parametrize("name", sorted(cases.bow_random_cases()))
def test_bow_random(matchers, name):
    call, ori = cases.bow_random_cases()[name]
    m = matchers(cases.NNRATIO, ori)
    _same(m.search_by_bow_rig(call), cases.bow_expected("random", name), name)
    assert m.rig_bow_last_kernel_ms() > 0.0


@pytest.mark.parametrize("ori", (False, True))
def test_bow_batch_equals_the_single_calls(matchers, ori):
    """every call with this orientation setting in ONE launch (hand-built ones at the common ratio included: empty pairs, a serial pair
    and 2000-feature pairs side by side)"""
    names = [("shape", k) for k, (_, o) in cases.bow_shape_cases().items() if o == ori] + [("random", k) for k, (_, o) in cases.bow_random_cases().items() if o == ori]
    calls = [{"shape": cases.bow_shape_cases, "random": cases.bow_random_cases}[g]()[k][0] for g, k in names]
    hand = [(k, c) for k, c in cases.bow_hand_cases().items() if c["check_ori"] == ori and c["nnratio"] == cases.NNRATIO]
    got = matchers(cases.NNRATIO, ori).search_by_bow_rig_batch(calls + [c["call"] for _, c in hand])
    for (g, k), r in zip(names, got):
        _same(r, cases.bow_expected(g, k), "batch " + k)
    for (k, c), r in zip(hand, got[len(names):]):
        _same(r, (c["want_n"], c["want_match"]), "batch " + k)


@pytest.mark.parametrize("name", sorted(cases.tri_hand_cases()))
def test_triangulation_hand_built(matchers, name):
    c = cases.tri_hand_cases()[name]
    got = matchers(cases.NNRATIO, c["check_ori"]).search_for_triangulation_rig(c["call"], c["only_stereo"], c["coarse"])
    _same(got, (c["want_n"], c["want_match"]), name)


def _same_decided(got, name, coarse=False, ori=False):
    n, m = got
    wn, wm, und = cases.tri_random_expected(name, coarse, ori)
    bad = np.nonzero((m != wm) & ~und)[0]
    print("%s: %d features, %d undecided, %d matches (reference %d)" % (name, len(m), und.sum(), n, wn))
    assert not len(bad), "%s: %d decided features differ, first %s: got %s want %s" % (name, len(bad), bad[:8], m[bad[:8]], wm[bad[:8]])
    assert n == int((m >= 0).sum())
    assert abs(n - wn) <= und.sum()


@pytest.mark.parametrize("name", sorted(cases.RANDOM_TRI))
def test_triangulation_random(matchers, name):
    m = matchers(cases.NNRATIO, False)
    _same_decided(m.search_for_triangulation_rig(cases.tri_random_case(name)), name)
    assert m.rig_bow_last_kernel_ms() > 0.0


@pytest.mark.parametrize("name", sorted(cases.RANDOM_TRI))
def test_triangulation_random_coarse_with_orientation(matchers, name):
    """one histogram couples all features, so the orientation check runs on the gate-free (coarse) search: integer-equal everywhere"""
    got = matchers(cases.NNRATIO, True).search_for_triangulation_rig(cases.tri_random_case(name), coarse=True)
    wn, wm, _ = cases.tri_random_expected(name, True, True)
    _same(got, (wn, wm), name)


def test_triangulation_batch_equals_the_single_calls(matchers):
    """one key frame against several neighbours (has_mp per pair) and unrelated pairs in ONE search launch"""
    m = matchers(cases.NNRATIO, False)
    names = sorted(cases.RANDOM_TRI)
    base = cases.tri_random_case("tri_tumvi_b")
    again = [cases.with_has_mp(base, s) for s in (1, 2)]
    hand = [c for c in cases.tri_hand_cases().values() if not c["coarse"] and not c["only_stereo"] and not c["check_ori"]]
    got = m.search_for_triangulation_rig_batch([cases.tri_random_case(k) for k in names] + again + [c["call"] for c in hand])
    for k, r in zip(names, got):
        _same_decided(r, k)
    und = cases.tri_random_expected("tri_tumvi_b")[2]
    for s, r in zip(again, got[len(names):]):
        single = m.search_for_triangulation_rig(s)
        assert single[0] == r[0] and np.array_equal(single[1], r[1])
        assert (r[1][s["kf1"]["has_mp"] != 0] == -1).all()
        wn, wm = ref.search_for_triangulation_rig(s)
        assert np.array_equal(r[1][~und], wm[~und])
    for c, r in zip(hand, got[len(names) + 2:]):
        _same(r, (c["want_n"], c["want_match"]), "batch hand-built")


def test_triangulation_with_a_key_frame_2_feature_in_two_nodes(matchers):
    """only key frame 1's features must be unique; a repeated feature of key frame 2 is a candidate in both nodes, as in the reference"""
    G, B = cases.scene_geometry("diverging"), cases.base_desc(2)
    k1, _ = cases.tri_side([cases.feat(G, 0, False, cases.P0, cases.at(B, 0), node=5), cases.feat(G, 0, False, cases.P0, cases.at(B, 1), node=6)])
    k2, _ = cases.tri_side([cases.feat(G, 1, False, cases.P0, cases.at(B, 4), node=5), cases.feat(G, 1, False, cases.P0, cases.at(B, 9), node=6)])
    ids, off, feat = k2["fv"]
    k2 = dict(k2, fv=(ids, off, np.array([0, 0], np.uint32)))           # feature 0 sits in node 5 and in node 6; feature 1 in none
    t = dict(kf1=k1, kf2=k2, geom=G["geom"], sigma2_1=cases.LEVEL_SIGMA2, sigma2_2=cases.LEVEL_SIGMA2)
    want = ref.search_for_triangulation_rig(t)
    assert want[1].tolist() == [0, 0] and not ref.undecided(t).any()    # both key-frame-1 features take it
    _same(matchers(cases.NNRATIO, False).search_for_triangulation_rig(t), want, "repeated key-frame-2 feature")


def test_only_stereo_batch_returns_no_match_without_a_launch(matchers):
    m = matchers(cases.NNRATIO, False)
    got = m.search_for_triangulation_rig_batch([cases.tri_random_case("tri_tumvi_b")] * 2, only_stereo=True)
    for n, m12 in got:
        assert n == 0 and (m12 == -1).all()
    assert m.rig_bow_last_kernel_ms() == 0.0
