"""Frames, strip geometry and the comparison with the CPU oracle that the tests of test_fast_strip_setup_gpu.py share.

The FAST strip kernel starts from a host-built record per strip (the tile's place in the pyramid, its size in 16-byte chunks, the cells'
columns and slots, the finished column -> cell row) and loads the tile with every chunk of a thread in flight at once, three at a time.
strips() restates the host's strip geometry (setup_geometry of csrc/orbx_extractor.hip) from the level sizes, so that a test can assert
that its frame really has the strips it was chosen for.

Run as a program it checks the frames whose strips need ORBX_STRIP_WIDTH = 250, which is read once per process."""
import importlib
import math
import os
import sys

import numpy as np

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
TILE_GROUP = 3          # chunks of the tile a thread has in flight at a time (orbx_fast_strips.inc)


def cells_of_level(w, h):
    """rows of cells (x0, x1, y0, y1) of a w x h pyramid level: the sub-images of ComputeKeyPointsOctTree (src/ORBextractor.cc:787-822)"""
    min_b, max_bx, max_by = 16, w - 16, h - 16
    width, height = float(max_bx - min_b), float(max_by - min_b)
    ncols, nrows = int(width / 35.0), int(height / 35.0)
    rows = []
    if ncols <= 0 or nrows <= 0:
        return rows
    wcell, hcell = int(math.ceil(width / ncols)), int(math.ceil(height / nrows))
    for i in range(nrows):
        y0 = min_b + i * hcell
        if y0 >= max_by - 3:
            continue
        y1 = min(y0 + hcell + 6, max_by)
        row = []
        for j in range(ncols):
            x0 = min_b + j * wcell
            if x0 >= max_bx - 6:
                continue
            x1 = min(x0 + wcell + 6, max_bx)
            if x1 - x0 - 6 > 0 and y1 - y0 - 6 > 0:
                row.append((x0, x1, y0, y1))
        if row:
            rows.append(row)
    return rows


def strips(level_sizes, strip_width=160):
    """every strip of a frame, in launch order (level, cell row, left to right): dicts with the numbers of the strip's record"""
    out = []
    for l, (w, h) in enumerate(level_sizes):
        for row in cells_of_level(w, h):
            n_row = len(row)
            w_cell = max(row[0][1] - row[0][0] - 6, 1)
            per = max(1, min(8, (strip_width - 6) // w_cell))
            n_strips = (n_row + per - 1) // per
            for k in range(n_strips):
                a, b = n_row * k // n_strips, n_row * (k + 1) // n_strips
                x0, x1, y0, y1 = row[a][0], row[b - 1][1], row[a][2], row[a][3]
                g0, g1 = (x0 + 3) >> 2, (x1 - 4) >> 2
                ngx = g1 - g0 + 1
                xa = (4 * (g0 - 1)) & ~15
                qoff = 4 * g0 - xa
                nch = (qoff + 4 * ngx + 4 + 15) >> 4
                th = y1 - y0
                out.append(dict(level=l, ncell=b - a, x0=x0, x1=x1, y0=y0, th=th, ngx=ngx, xa=xa, qoff=qoff, nch=nch, n_chunk=th * nch,
                                groups=-(-th * nch // (256 * TILE_GROUP))))
    return out


_references = {}


def reference(oracle, key, img, args):
    """the oracle's answer for one frame, computed once per key: mono index, key points, descriptors, the candidates and the size of
    every level"""
    if key not in _references:
        oex = oracle.extractor(*args)
        mono, kps, desc = oex.extract(img, (0, 1000))
        ref = dict(args=args, img=img, mono=mono, kps=kps, desc=desc, cands=[oex.level_candidates(l) for l in range(args[2])],
                   sizes=[tuple(oex.level_size(l)) for l in range(args[2])])
        for a in [img, kps, desc] + ref["cands"]:
            a.setflags(write=False)
        _references[key] = ref
    return _references[key]


def assert_same(ex, ref, mono, kps, desc, frame, what):
    """candidates of every level, key points and descriptors against the oracle, bit for bit (as fast_fallback_cases.assert_same does,
    from the shared reference)"""
    for l, oc in enumerate(ref["cands"]):
        gc = ex.candidates(l, frame=frame, cap=len(oc) + 64)
        assert len(oc) == len(gc), "%s level %d: %d vs %d candidates" % (what, l, len(gc), len(oc))
        for f in ("x", "y", "response"):
            np.testing.assert_array_equal(gc[f], oc[f], err_msg="%s level %d %s" % (what, l, f))
    assert mono == ref["mono"], "%s: mono index %d vs %d" % (what, mono, ref["mono"])
    assert len(kps) == len(ref["kps"]), "%s: %d vs %d key points" % (what, len(kps), len(ref["kps"]))
    for f in FIELDS:
        np.testing.assert_array_equal(kps[f], ref["kps"][f], err_msg="%s field %s" % (what, f))
    np.testing.assert_array_equal(desc, ref["desc"], err_msg=what)


def noise_frame(w, h, seed):
    """full-range noise: corners at iniThFAST everywhere"""
    return np.random.RandomState(seed).randint(0, 256, size=(h, w)).astype(np.uint8)


def faint_frame(w, h, seed):
    """steps of 10 grey levels: corners at minThFAST only, every cell falls back"""
    return (100 + 10 * (np.random.RandomState(seed).uniform(size=(h, w)) < 0.5)).astype(np.uint8)


# the frames of the wide-strip process: (name, width, height, levels, least number of key points, least number of chunk groups)
WIDE = [("tall 160x101", 160, 101, 2, 50, 1), ("tall 250x101", 250, 101, 2, 50, 2)]


def wide_frame(name, w, h, k):
    return faint_frame(w, h, 7 + k) if k == 0 else noise_frame(w, h, 31 + len(name))


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch  # noqa: F401  (before the package: one HIP runtime per process, see conftest.py)
    from oracle_api import Oracle
    pkg = importlib.import_module("orb_slam3-1_amd")
    assert os.environ.get("ORBX_STRIP_WIDTH") == "250"
    oracle = Oracle()
    for name, w, h, nlevels, min_kps, min_groups in WIDE:
        args = (500, 1.2, nlevels, 20, 7)
        imgs = np.stack([wide_frame(name, w, h, k) for k in range(2)])
        refs = [reference(oracle, (name, k), imgs[k], args) for k in range(2)]
        geo = strips(refs[0]["sizes"], 250)
        assert [s["ncell"] for s in geo if s["level"] == 0] == [(w - 32) // 35], "%s: level 0 is not one strip: %r" % (name, geo)
        assert max(s["groups"] for s in geo) >= min_groups, "%s: %r" % (name, geo)
        ex = pkg.Extractor(*args)
        try:
            mono, n, kps, desc = ex.extract_batch(imgs)
            for k in range(2):
                assert len(refs[k]["kps"]) > min_kps, "%s frame %d: the oracle found %d key points" % (name, k, len(refs[k]["kps"]))
                assert_same(ex, refs[k], mono[k], kps[k, :n[k]], desc[k, :n[k]], k, "%s, frame %d" % (name, k))
        finally:
            ex.close()
    print("wide strips ok")


if __name__ == "__main__":
    main()
