"""k_octree's bucket table: every key is placed once by the quadtree cell it falls into, nodes above the table's depth divide by
differences of the cells' prefix sums, nodes below it partition their keys as before, and the final selection breaks ties of the
response by candidate order.  Every image of octree_bucket_cases.py -- each shown, on the CPU oracle's candidates, to reach the
situation it was built for -- with ORBX_OCT_WAVES = 1, 2 and 4 in every home of the keys; key points and descriptors against the
CPU oracle, field by field, bit for bit."""
import numpy as np
import pytest

import octree_bucket_cases as bc
import octree_buckets as ob
import octree_cases as oc

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
HOMES = {
    "lds": ({}, (1, 3)),
    "dyn_fallback": ({"ORBX_OCT_DYN_KEYS": "64"}, (1, 3)),
    "scratch": ({"ORBX_OCT_LDS_KEYS": "0"}, (2,)),
}

_ref = {}


def _oracle(oracle, case, args=None):
    """(extract result, per-level analysis) of the case, computed once"""
    args = args or case.args
    key = (case.name, args)
    if key not in _ref:
        oex = oracle.extractor(*args)
        res = oex.extract(case.image, (0, 1000))
        _ref[key] = (res, bc.analyse(oex, args[2], case.depth_max))
    return _ref[key]


def _same(kps, desc, ref, what):
    r0, okps, odesc = ref
    assert len(kps) == len(okps), "%s: %d vs %d key points" % (what, len(kps), len(okps))
    for f in FIELDS:
        np.testing.assert_array_equal(kps[f], okps[f], err_msg="%s field %s" % (what, f))
    np.testing.assert_array_equal(desc, odesc, err_msg=what)


def _env(monkeypatch, waves, home_env, case_env):
    monkeypatch.setenv("ORBX_OCT_WAVES", str(waves))
    for k, v in list(home_env.items()) + list(case_env.items()):
        monkeypatch.setenv(k, v)


@pytest.mark.parametrize("home", sorted(HOMES))
@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("case", bc.CASES, ids=lambda c: c.name)
def test_case_in_every_key_home(pkg, oracle, monkeypatch, case, waves, home):
    env, variants = HOMES[home]
    _env(monkeypatch, waves, env, case.env)
    ref, levels = _oracle(oracle, case)
    assert len(ref[1]) > 0, "the oracle found no key point"
    if case.check is not None:
        assert case.check(levels[case.level]), "%s: the image does not reach what it was built for" % case.name
    ex = pkg.Extractor(*case.args)
    try:
        mono, kps, desc = ex(case.image, (0, 1000))
        assert mono == ref[0]
        assert ex.debug_last_schedule() & 3 in variants
        assert ex.debug_octree_waves(1) == waves
        _same(kps, desc, ref, "%s, %d waves, %s" % (case.name, waves, home))
    finally:
        ex.close()


def test_sparse_levels_hold_none_one_and_few(oracle):
    """(what `sparse_levels` is built for, on all its levels at once)"""
    _, levels = _oracle(oracle, bc.BY_NAME["sparse_levels"])
    totals = [lv["total"] for lv in levels]
    assert 0 in totals and 1 in totals and any(1 < t < lv["N"] for t, lv in zip(totals, levels)), totals


@pytest.mark.parametrize("home", sorted(HOMES))
@pytest.mark.parametrize("waves", [1, 2, 4])
def test_batch_of_three_frames_with_different_counts(pkg, oracle, monkeypatch, waves, home):
    env, variants = HOMES[home]
    _env(monkeypatch, waves, env, {})
    names = ["split_lines_n217", "ties_across_fast_cells", "sorted_break"]
    args = (217,) + oc.ARGS_TAIL
    refs = [_oracle(oracle, bc.BY_NAME[n], args) for n in names]
    totals = [lv[0]["total"] for _, lv in refs]
    assert len(set(totals)) == 3 and min(totals) > 0, totals
    ex = pkg.Extractor(*args)
    try:
        mono, n, kps, desc = ex.extract_batch(np.stack([bc.BY_NAME[k].image for k in names]))
        assert ex.debug_last_schedule() & 3 in variants and ex.debug_octree_waves(1) == waves
        for b, (ref, _) in enumerate(refs):
            assert mono[b] == ref[0] and n[b] == len(ref[1]) > 0
            _same(kps[b, :n[b]], desc[b, :n[b]], ref, "frame %d (%s)" % (b, names[b]))
    finally:
        ex.close()


@pytest.mark.parametrize("depth", ["6", "2"])
@pytest.mark.parametrize("waves", [1, 2, 4])
def test_node_pool_in_the_hbm_scratch(pkg, oracle, monkeypatch, waves, depth):
    """a budget of 2700 features: node pool, counters and maps live in global memory (k_octree<false, false>)"""
    _env(monkeypatch, waves, {}, {"ORBX_OCT_TAB_DEPTH": depth})
    case = bc.BY_NAME["split_lines_n1000"]
    args = (2700,) + oc.ARGS_TAIL
    ref, _ = _oracle(oracle, case, args)
    ex = pkg.Extractor(*args)
    try:
        mono, kps, desc = ex(case.image, (0, 1000))
        assert mono == ref[0] and len(ref[1]) > 0 and ex.debug_last_schedule() & 3 == 0 and ex.debug_octree_waves(1) == waves
        assert ex.debug_octree_table(0)[0] == int(depth)
        _same(kps, desc, ref, "node pool in HBM, %d waves, depth %s" % (waves, depth))
    finally:
        ex.close()


@pytest.mark.parametrize("w,h,args,depth_max", [(320, 240, (1000, 1.2, 8, 20, 7), 6), (640, 480, (1000, 1.2, 8, 20, 7), 6), (320, 100, (60, 1.2, 2, 20, 7), 6),
                                                (67, 67, (60, 1.2, 2, 20, 7), 6), (640, 480, (6, 1.2, 1, 20, 7), 6), (320, 240, (1000, 1.2, 4, 20, 7), 2),
                                                (500, 120, (300, 1.2, 3, 20, 7), 6)])
def test_device_table_is_the_python_table(pkg, oracle, monkeypatch, w, h, args, depth_max):
    """(h) depth, roots and boundaries of every level as the device holds them"""
    monkeypatch.setenv("ORBX_OCT_TAB_DEPTH", str(depth_max))
    oex = oracle.extractor(*args)
    img = bc.noise(w, h, 3)
    oex.extract(img, (0, 1000))
    nfeat = oex.tables()["nfeat"]
    ex = pkg.Extractor(*args)
    try:
        ex(img, (0, 1000))
        for l in range(args[2]):
            lw, lh = oex.level_size(l)
            D, n_ini, xb, yb = ob.level_table(lw, lh, int(nfeat[l]), depth_max)
            gD, gn, gxb, gyb = ex.debug_octree_table(l)
            assert (gD, gn) == (D, n_ini), "level %d" % l
            np.testing.assert_array_equal(gxb, xb.reshape(gxb.shape))
            np.testing.assert_array_equal(gyb, yb)
    finally:
        ex.close()
