"""The numpy reference of FAST over the cells of a level (fast_cells_reference.py) and the designed frames (fast_cells_cases.py), without
a GPU:

  * every frame does what it was drawn for, in the reference's own output (fast_cells_cases.assert_design);
  * on every frame the reference equals the CPU oracle's vToDistributeKeys in x, y and response -- two independent statements of the
    same definition, which pins the oracle as well;
  * every deliberately wrong variant of the reference is told apart from the truth by the frames named here, so a device kernel with
    that mistake fails test_fast_cells_gpu.py on them; the variants' computation without a deviation equals the truth everywhere."""
import numpy as np
import pytest

import fast_cells_cases as cc
import fast_cells_reference as fr
import fast_strip_setup_cases as sc

NAMES = list(cc.cases())

# wrong variant -> the designed frames that expose it (every one of them must)
EXPOSED_BY = {
    "threshold_ge": ["threshold and fallback, one strip", "threshold and fallback, across strips", "pairs inside a cell", "sheet m=7 dark",
                     "sheet m=7 bright", "graded sheet m=20 bright", "graded sheet m=20 dark", "graded sheet m=7 bright", "graded sheet m=7 dark"],
    "response_m": ["sheet m=21 bright", "sheet m=8 dark", "ranking"],
    "nms_ge": ["pairs inside a cell", "borders at iniThFAST", "borders in the fallback"],
    "nms_sub_threshold": ["pairs inside a cell"],
    "nms_across_border": ["borders at iniThFAST", "borders in the fallback", "edges at iniThFAST", "edges in the fallback"],
    "fallback_before_nms": ["threshold and fallback, one strip", "threshold and fallback, across strips"],
    "fallback_per_row": ["threshold and fallback, one strip", "threshold and fallback, across strips", "pairs inside a cell"],
    "fallback_adds": ["threshold and fallback, one strip", "threshold and fallback, across strips"],
    "emit_column_major": ["ranking", "pairs inside a cell", "sheet m=21 dark"],
    "cells_column_major": ["sheet m=21 bright", "sheet m=20 dark", "borders at iniThFAST", "ranking"],
}


def test_every_variant_has_a_frame():
    assert set(EXPOSED_BY) == set(fr.VARIANTS) - {"same"}
    assert all(n in cc.cases() for names in EXPOSED_BY.values() for n in names)


@pytest.mark.parametrize("name", NAMES)
def test_designed_frame_against_the_oracle(oracle, name):
    case = cc.cases()[name]
    want = cc.numpy_candidates(name)          # (holds the case's own statement against the reference)
    ref = sc.reference(oracle, ("fast cells", name), case.img, cc.ARGS)
    assert ref["sizes"] == [(cc.W, cc.H)]
    cc.assert_candidates(cc.as_tuples(ref["cands"][0]), want, name)
    assert fr.level_candidates(case.img, cc.INI, cc.MIN, "same") == want


@pytest.mark.parametrize("variant", sorted(EXPOSED_BY))
def test_wrong_variant_is_told_apart(variant):
    for name in EXPOSED_BY[variant]:
        case = cc.cases()[name]
        assert fr.level_candidates(case.img, cc.INI, cc.MIN, variant) != cc.numpy_candidates(name), \
            "%s (%s) gives the true list on '%s'" % (variant, fr.VARIANTS[variant], name)


@pytest.mark.parametrize("noise", cc.NOISE, ids=[n[0] for n in cc.NOISE])
def test_noise_frame_against_the_oracle(oracle, noise):
    """level 0 of the noise frames (the upper levels depend on the resize: the GPU test runs the reference on the device's own levels)"""
    name, w, h, nlevels, seed = noise
    img = sc.noise_frame(w, h, seed)
    ref = sc.reference(oracle, ("fast cells", name), img, (500, 1.2, nlevels, cc.INI, cc.MIN))
    want = fr.level_candidates(img, cc.INI, cc.MIN)
    assert len(want) > 500
    cc.assert_candidates(cc.as_tuples(ref["cands"][0]), want, name)
    assert fr.level_candidates(img, cc.INI, cc.MIN, "same") == want


def test_building_blocks():
    """a dot is one corner with M = m; the thresholds are strict; pairs and chains of dots suppress as the definition says"""
    def keys(dots, t, size=21):
        img = np.full((size, size), 100, np.uint8)
        for x, y, m in dots:
            img[y, x] -= m
        return [(int(x), int(y), int(s)) for x, y, s in fr.fast_definitional(img, t)]
    assert keys([(10, 10, 21)], 20) == [(10, 10, 20)] and keys([(10, 10, 20)], 20) == [] and keys([(10, 10, 20)], 7) == [(10, 10, 19)]
    assert keys([(10, 10, 8)], 7) == [(10, 10, 7)] and keys([(10, 10, 7)], 7) == []
    assert keys([(10, 10, 30), (11, 10, 30)], 20) == [] and keys([(10, 10, 30), (11, 10, 31)], 20) == [(11, 10, 30)]
    assert keys([(9, 10, 30), (10, 10, 31), (11, 10, 40)], 20) == [(11, 10, 39)]
    assert keys([(3, 3, 30), (2, 3, 40), (17, 17, 30), (18, 17, 40)], 20) == [(3, 3, 29), (17, 17, 29)]      # the 3-pixel border counts as 0
