"""The minThFAST fallback of the FAST strip kernel: for a cell that finds nothing at iniThFAST the four waves of the strip's workgroup
share the quick test, and ONE of them scores, suppresses, ranks and emits the cell without a further workgroup barrier.  Candidates of
every level, key points and descriptors against the CPU oracle, bit for bit, on frames drawn so that strips hold 1, 2, 3, 4 and more
than 4 such cells, cells of more than 32 rows, and corner lists that overflow inside the one-wave part (fast_fallback_cases.py draws
the frames)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_fallback_cases as fc

pytestmark = pytest.mark.gpu


def _check_single(pkg, oracle, img, args, what, cap=None, cells=None):
    oex = oracle.extractor(*args)
    r0, okps, odesc = oex.extract(img, (0, 1000))
    if cells is not None:
        fc.assert_design(oex, cells, img.shape[1], img.shape[0])
    ex = pkg.Extractor(*args)
    try:
        if cap is not None:
            ex.debug_set_fast_corner_cap(cap)
        mono, kps, desc = ex(img, (0, 1000))
        assert mono == r0
        fc.assert_same(ex, oex, kps, desc, okps, odesc, 0, what, nlevels=args[2])
    finally:
        ex.close()
    return len(okps)


@pytest.mark.parametrize("cap", [1, 7, 40])
def test_faint_frame_small_corner_caps(pkg, oracle, cap):
    """faint everywhere: every cell falls back, and with a corner list of 1, 7 or 40 entries the owner of a cell overflows and scans
    the rows and columns of its cell"""
    rs = np.random.RandomState(12)
    rs.uniform(size=(240, 160))                       # (the frame of test_fast_threshold_fallback_cells: same draws)
    faint = (100 + 10 * (rs.uniform(size=(240, 320)) < 0.5)).astype(np.uint8)
    assert _check_single(pkg, oracle, faint, fc.ARGS, "faint frame, cap %d" % cap, cap=cap) > 100


@pytest.mark.parametrize("name", ["checker", "runs"])
def test_strips_with_one_to_four_fallback_cells(pkg, oracle, name):
    cells = fc.checker_cells() if name == "checker" else fc.run_cells()
    img = fc.cell_image(320, 240, cells, 3)
    assert _check_single(pkg, oracle, img, fc.ARGS, name, cells=cells) > 100


def test_more_fallback_cells_than_waves():
    """a strip of six cells, five and six of them faint (the strip width is read once per process: a process of its own)"""
    env = dict(os.environ, ORBX_STRIP_WIDTH="250")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fast_fallback_cases.py")],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "wide strips ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


def _tall(seed):
    rs = np.random.RandomState(seed)
    return (100 + 10 * (rs.uniform(size=(101, 160)) < 0.5)).astype(np.uint8)


def test_tall_cell(pkg, oracle):
    """160 x 101, 2 levels: level 0 is one cell row of 63 interior rows (a wave's share of them must fit the 5-bit row field of an
    entry; the owner of a cell walks all 63)"""
    args = (500, 1.2, 2, 20, 7)
    img = _tall(7)
    oex = oracle.extractor(*args)
    oex.extract(img, (0, 1000))
    c = oex.level_candidates(0)
    assert c["y"].min() + 16 < 19 + 31 and c["y"].max() + 16 >= 19 + 32 and c["response"].max() < 20
    assert _check_single(pkg, oracle, img, args, "tall cell") > 50


def test_tall_cell_batch(pkg, oracle):
    args = (500, 1.2, 2, 20, 7)
    imgs = np.stack([_tall(s) for s in (7, 8, 9)])
    ex = pkg.Extractor(*args)
    try:
        mono, n, kps, desc = ex.extract_batch(imgs)
        for b in range(len(imgs)):
            oex = oracle.extractor(*args)
            r0, okps, odesc = oex.extract(imgs[b], (0, 1000))
            assert mono[b] == r0 and n[b] == len(okps) > 50
            fc.assert_same(ex, oex, kps[b, :n[b]], desc[b, :n[b]], okps, odesc, b, "batch frame %d" % b, nlevels=2)
    finally:
        ex.close()
