"""k_octree with 1, 2 and 4 waves per (frame, level) workgroup: the control wave hands the key partition of its one-by-one nodes, the
initial gather and the final selection to the helper waves.  Every dot image of octree_cases.py (test_octree_reference.py shows
what their traces cover), with ORBX_OCT_WAVES = 1, 2 and 4, in every home of the keys and of the node pool; key points and
descriptors against the CPU oracle, field by field, bit for bit."""
import numpy as np
import pytest

import octree_cases as oc

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
# home of the keys: how it is forced, and the instantiations (bits 0-1 of debug_last_schedule) that serve it
HOMES = {
    "lds": ({}, (1, 3)),                                    # a single frame: both key buffers in LDS (k_octree<true, true> or k_octree_dyn)
    "dyn_fallback": ({"ORBX_OCT_DYN_KEYS": "64"}, (1, 3)),   # k_octree_dyn with room for 64 keys: more candidates take its scratch body
    "scratch": ({"ORBX_OCT_LDS_KEYS": "0"}, (2,)),          # k_octree<false, true>
}

_ref = {}


def _oracle(oracle, case, N=None):
    key = (case.name, N)
    if key not in _ref:
        args = case.args if N is None else (N,) + oc.ARGS_TAIL
        _ref[key] = oracle.extractor(*args).extract(case.image(), (0, 1000))
    return _ref[key]


def _same(kps, desc, ref, what):
    r0, okps, odesc = ref
    assert len(kps) == len(okps), "%s: %d vs %d key points" % (what, len(kps), len(okps))
    for f in FIELDS:
        np.testing.assert_array_equal(kps[f], okps[f], err_msg="%s field %s" % (what, f))
    np.testing.assert_array_equal(desc, odesc, err_msg=what)


@pytest.mark.parametrize("home", sorted(HOMES))
@pytest.mark.parametrize("waves", [1, 2, 4])
@pytest.mark.parametrize("case", oc.CASES, ids=lambda c: c.name)
def test_case_in_every_key_home(pkg, oracle, monkeypatch, case, waves, home):
    env, variants = HOMES[home]
    monkeypatch.setenv("ORBX_OCT_WAVES", str(waves))
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    ref = _oracle(oracle, case)
    ex = pkg.Extractor(*case.args)
    try:
        mono, kps, desc = ex(case.image(), (0, 1000))
        assert mono == ref[0]
        assert ex.debug_last_schedule() & 3 in variants
        assert ex.debug_octree_waves(1) == waves
        _same(kps, desc, ref, "%s, %d waves, %s" % (case.name, waves, home))
    finally:
        ex.close()


@pytest.mark.parametrize("waves", [1, 2, 4])
def test_node_pool_in_the_hbm_scratch(pkg, oracle, monkeypatch, waves):
    """a budget of 2700 features: the node pool does not fit LDS (k_octree<false, false>)"""
    monkeypatch.setenv("ORBX_OCT_WAVES", str(waves))
    case = oc.BY_NAME["grid_n1000"]
    ref = _oracle(oracle, case, 2700)
    ex = pkg.Extractor(2700, *oc.ARGS_TAIL)
    try:
        mono, kps, desc = ex(case.image(), (0, 1000))
        assert mono == ref[0] and ex.debug_last_schedule() & 3 == 0 and ex.debug_octree_waves(1) == waves
        _same(kps, desc, ref, "node pool in HBM, %d waves" % waves)
    finally:
        ex.close()


def test_workgroups_leave_at_different_times(pkg, oracle, monkeypatch):
    """three different frames and a blank one in one call, four waves each: the blank frame's workgroup takes the first early return
    while the others still post jobs"""
    monkeypatch.setenv("ORBX_OCT_WAVES", "4")
    names = ["grid_n1000", "blank", "sub_7", "quad_257_256_65_64"]
    imgs = np.stack([oc.BY_NAME[n].image() for n in names])
    N = 1000
    ex = pkg.Extractor(N, *oc.ARGS_TAIL)
    try:
        mono, n, kps, desc = ex.extract_batch(imgs)
        assert ex.debug_octree_waves(1) == 4
        for b, name in enumerate(names):
            ref = _oracle(oracle, oc.BY_NAME[name], N)
            assert mono[b] == ref[0] and n[b] == len(ref[1])
            _same(kps[b, :n[b]], desc[b, :n[b]], ref, "frame %d (%s)" % (b, name))
    finally:
        ex.close()
