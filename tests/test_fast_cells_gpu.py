"""k_fast_strips at its exact decision boundaries: the candidates of every level (Extractor.candidates = vToDistributeKeys) against the
plain numpy reference of fast_cells_reference.py -- count, then x, y and response in order --, then key points and descriptors against
the CPU oracle, on the designed frames of fast_cells_cases.py.  Everything is integer: every comparison is equality.

What the frames decide (each asserts it on the reference's own output, and test_fast_cells_reference.py shows for every listed mistake
a frame that a kernel making it fails):

  quick test   stamp sheets: an arc of exactly nine at 16 rotations x 2 polarities x every place of the centre in its quad, margins
               21 / 20 / 8 / 7 (iniThFAST, fallback, response 7, nothing), backgrounds 0, 19, 20, 21, 234, 235, 236, 255 where v - t and
               v + t saturate, and sheets with the rest of the ring on the opposite side
  threshold    M > t strictly at 20 and at 7, response M - 1; graded stamps, whose compass pixels pass the quick test at t while the score
               tree gives M = t exactly (a uniform stamp with M = t never gets past the quick test), at 20, 21, 7 and 8
  fallback     per cell, decided after the suppression (an equal pair empties a cell), cells of one strip / of two strips / of two rows
  suppression  strict, among corners at the current threshold only, stopping at the cell interior: pairs and chains inside a cell;
               pairs astride a cell border inside a strip, a strip border, the cell-row border and the meeting point of four cells, and
               one pixel to either side; the first and last detection row and column
  ranking      a lattice of 220 winners over the words of a cell's mask, a single winner on a mask's last bit
  order        cells in table order, row-major inside

in these configurations: host entry in batches of 1, 5 (in order) and 3 (shuffled); the in-place device entry with padded rows; the
corner lists at their default size and at 1 entry, which sends every wave through the overflow scan in the iniThFAST and the minThFAST
pass; one strip per cell row (a child process with ORBX_STRIP_WIDTH = 250); and two noise frames of 3 and 2 levels, the reference run on
the device's own level images."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_cells_cases as cc
import fast_cells_reference as fr
import fast_strip_setup_cases as sc
from test_fast_strip_setup_gpu import _device_batch

pytestmark = pytest.mark.gpu

NAMES = list(cc.cases())
CAPS = [None, 1]
_level_refs = {}


def _cap_id(cap):
    return "default corner cap" if cap is None else "corner cap %d" % cap


@pytest.mark.parametrize("name", NAMES)
def test_single_frame(pkg, oracle, name):
    cc.run_batch(pkg, oracle, [name], "single frame")


@pytest.mark.parametrize("name", NAMES)
def test_single_frame_overflow_scan(pkg, oracle, name):
    cc.run_batch(pkg, oracle, [name], "single frame, corner cap 1", corner_cap=1)


@pytest.mark.parametrize("cap", CAPS, ids=_cap_id)
def test_host_batches(pkg, oracle, cap):
    """batches of 5 in the frames' own order and of 3 in a shuffled one: a frame's result does not depend on its neighbours in the grid"""
    for k, names in enumerate(cc.batches(NAMES, 5)):
        cc.run_batch(pkg, oracle, names, "batch of 5 no. %d, %s" % (k, _cap_id(cap)), corner_cap=cap)
    for k, names in enumerate(cc.batches(NAMES, 3, seed=3)):
        cc.run_batch(pkg, oracle, names, "shuffled batch of 3 no. %d, %s" % (k, _cap_id(cap)), corner_cap=cap)


@pytest.mark.parametrize("cap", CAPS, ids=_cap_id)
def test_device_entry_in_place(pkg, oracle, cap):
    """level 0 read from the caller's image: rows padded by 16 bytes, frames by 160"""
    for k, names in enumerate(cc.batches(NAMES, 3, seed=4)):
        refs = [sc.reference(oracle, ("fast cells", n), cc.cases()[n].img, cc.ARGS) for n in names]
        for n, r in zip(names, refs):       # the helper compares with the oracle's candidates: they are the numpy reference's
            cc.assert_candidates(cc.as_tuples(r["cands"][0]), cc.numpy_candidates(n), n)
        sched = _device_batch(pkg, refs, len(refs), "in place, batch %d (%s), %s" % (k, "; ".join(names), _cap_id(cap)), -1,
                              row_pad=16, frame_pad=160, corner_cap=cap)
        assert sched & 16, "level 0 was not read in place"


@pytest.mark.parametrize("noise", cc.NOISE, ids=[n[0] for n in cc.NOISE])
@pytest.mark.parametrize("cap", CAPS, ids=_cap_id)
def test_noise_levels(pkg, oracle, noise, cap):
    """every level against the reference run on the DEVICE's level image: FAST on the upper levels, independently of the resize"""
    name, w, h, nlevels, seed = noise
    args = (500, 1.2, nlevels, cc.INI, cc.MIN)
    img = sc.noise_frame(w, h, seed)
    ref = sc.reference(oracle, ("fast cells", name), img, args)
    ex = pkg.Extractor(*args)
    try:
        if cap is not None:
            ex.debug_set_fast_corner_cap(cap)
        mono, kps, desc = ex(img, (0, 1000))
        for l in range(nlevels):
            lvl = ex.pyramid_level(l)
            assert lvl.shape == ref["sizes"][l][::-1] and (l > 0 or np.array_equal(lvl, img))
            if (name, l) not in _level_refs or not np.array_equal(_level_refs[name, l][0], lvl):      # (once for both corner caps)
                _level_refs[name, l] = (lvl, fr.level_candidates(lvl, cc.INI, cc.MIN))
            want = _level_refs[name, l][1]
            assert len(want) > 200, "%s level %d: the reference found %d candidates" % (name, l, len(want))
            cc.assert_candidates(cc.as_tuples(ex.candidates(l, cap=len(want) + 64)), want, "%s level %d, %s" % (name, l, _cap_id(cap)))
        sc.assert_same(ex, ref, mono, kps, desc, 0, "%s, %s" % (name, _cap_id(cap)))
    finally:
        ex.close()


def test_one_strip_per_cell_row():
    """every designed frame with a cell row as ONE strip of five cells, where the borders fall elsewhere (the strip width is read once
    per process: a process of its own)"""
    env = dict(os.environ, ORBX_STRIP_WIDTH="250")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fast_cells_cases.py")],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "wide strips ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
