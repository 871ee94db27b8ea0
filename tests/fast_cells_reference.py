"""FAST over the cells of one pyramid level, in plain numpy from the definitions: what ComputeKeyPointsOctTree hands to the octree
(vToDistributeKeys, reference src/ORBextractor.cc:787-872) and what k_fast_strips must reproduce bit for bit.  Shares no code and no
evaluation order with oracle/*.cpp.

  * fast_definitional: FAST-9/16 (OpenCV features2d fast.cpp / fast_score.cpp).  A pixel is a corner at
    threshold t iff some contiguous arc of >= 9 of its 16 ring pixels is entirely brighter than v + t or entirely darker than v - t.
    With M = the largest over the sixteen 9-arcs of the arc's smallest contrast that is `M > t`, and the response is M - 1, the largest
    threshold at which the pixel is still a corner.  3x3 non-maximum suppression keeps strictly greater responses; non-corners and the
    3-pixel border of the image count as 0; emission is row-major.
  * level_candidates: the level is cut into cells (fast_strip_setup_cases.cells_of_level), cv::FAST runs on every cell's sub-image at
    iniThFAST, and again at minThFAST if that gave NOTHING (vKeysCell.empty(), :843: decided after the suppression, per cell); the keys
    are shifted to coordinates relative to minBorder (:865-866) and appended cell by cell, cells in row-major order.

level_candidates(..., variant=name) is a deliberately WRONG restatement, one single deviation each (VARIANTS): the mistakes a rewrite of
the kernel is likely to make.  tests/test_fast_cells_reference.py shows for each of them a designed frame of fast_cells_cases.py on which
it differs from the truth, i.e. a device kernel with that mistake fails the comparison of test_fast_cells_gpu.py.  The variants are
computed another way than the truth -- from one margin map of the whole level, in level coordinates -- and "same" is that computation
without a deviation, which the tests hold equal to the truth on every frame."""
import numpy as np

from fast_strip_setup_cases import cells_of_level

# the Bresenham ring of radius 3, (dx, dy) of ring pixel k, in cv::FAST's order
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
MIN_BORDER = 16         # EDGE_THRESHOLD - 3: vToDistributeKeys holds coordinates relative to it


def fast_definitional(img, t, want_map=False):
    """(x, y, score) of FAST-9/16 corners at threshold t with 3x3 NMS, row-major, straight from the definition"""
    h, w = img.shape
    v = img.astype(np.int32)
    H, W = h - 6, w - 6
    c = v[3:h - 3, 3:w - 3]
    d = np.stack([v[3 + dy:3 + dy + H, 3 + dx:3 + dx + W] - c for (dx, dy) in RING])       # ring - centre, [16, H, W]
    best = np.full((H, W), -1 << 20, np.int32)
    for k in range(16):
        arc = d[[(k + i) % 16 for i in range(9)]]
        best = np.maximum(best, np.maximum(arc.min(0), (-arc).min(0)))      # brighter arc / darker arc
    score = np.zeros((h, w), np.int32)
    sc = best - 1                       # largest threshold at which the pixel is a corner
    score[3:h - 3, 3:w - 3] = np.where(best > t, sc, 0)
    if want_map:
        return score
    out = []
    for y in range(3, h - 3):
        row = score[y]
        for x in np.nonzero(row[3:w - 3])[0] + 3:
            s = row[x]
            nb = score[y - 1:y + 2, x - 1:x + 2].copy()
            nb[1, 1] = -1
            if (s > nb).all():
                out.append((x, y, s))
    return out


# name -> the one thing it gets wrong
VARIANTS = {
    "same": "nothing: the computation of the variants without a deviation",
    "threshold_ge": "a corner is M >= t instead of M > t",
    "response_m": "the response is M instead of M - 1",
    "nms_ge": "the suppression keeps a response that is >= its neighbours instead of >",
    "nms_sub_threshold": "a neighbour that is no corner at the current threshold counts with the byte of the score map (M) instead of 0",
    "nms_across_border": "the suppression reads neighbours outside the cell's own interior",
    "fallback_before_nms": "a cell falls back when it has no corner before the suppression, not when it has no key after it",
    "fallback_per_row": "a cell falls back only when its whole cell row found nothing at iniThFAST",
    "fallback_adds": "the minThFAST keys are added to a cell that is not empty",
    "emit_column_major": "the keys of a cell are emitted column by column",
    "cells_column_major": "the cells are emitted column by column of the cell table",
}
# (nms_sub_threshold: a neighbour below the threshold that counted with its RESPONSE M' - 1 could never matter, M' <= t < M; a kernel goes
#  wrong here by comparing against the raw byte of its score map, which holds M for every scored pixel: then (21, 20) at t = 20 is
#  20 > 20 and drops the corner)


def margin_map(img):
    """M of every pixel that has its whole ring inside the image, 0 elsewhere and where no arc of nine is one-sided"""
    h, w = img.shape
    v = img.astype(np.int64)
    ring = np.zeros((16, h, w), np.int64)
    for k, (dx, dy) in enumerate(RING):
        ring[k, 3:h - 3, 3:w - 3] = v[3 + dy:h - 3 + dy, 3 + dx:w - 3 + dx]
    dark = v[None] - ring           # > 0: the ring pixel is darker than the centre
    m = np.zeros((h, w), np.int64)
    for k in range(16):
        arc = [(k + i) % 16 for i in range(9)]
        m = np.maximum(m, np.maximum(dark[arc].min(0), (-dark[arc]).min(0)))
    m[:3] = 0; m[h - 3:] = 0; m[:, :3] = 0; m[:, w - 3:] = 0
    return m


def _cell_keys(M, rect, t, variant):
    """keys of one cell at threshold t from the level's margin map, in coordinates relative to MIN_BORDER; and whether the cell's
    interior holds a corner at all"""
    x0, x1, y0, y1 = rect
    ix0, ix1, iy0, iy1 = x0 + 3, x1 - 3, y0 + 3, y1 - 3
    corner = (M >= t) if variant == "threshold_ge" else (M > t)
    nb = np.where(corner, M - 1, M if variant == "nms_sub_threshold" else 0)
    if variant != "nms_across_border":
        inside = np.zeros(M.shape, bool)
        inside[iy0:iy1, ix0:ix1] = True
        nb = np.where(inside, nb, 0)
    keys = []
    for y in range(iy0, iy1):
        for x in np.nonzero(corner[y, ix0:ix1])[0] + ix0:
            s = M[y, x] - 1
            n = nb[y - 1:y + 2, x - 1:x + 2].copy()
            n[1, 1] = -1
            if (s >= n).all() if variant == "nms_ge" else (s > n).all():
                keys.append((int(x) - MIN_BORDER, y - MIN_BORDER, int(M[y, x] if variant == "response_m" else s)))
    return keys, bool(corner[iy0:iy1, ix0:ix1].any())


def _variant_candidates(img, ini_th, min_th, variant):
    M = margin_map(img)
    rows = cells_of_level(img.shape[1], img.shape[0])
    per_cell = []
    for row in rows:
        at_ini = [_cell_keys(M, rect, ini_th, variant) for rect in row]
        row_found = any(keys for keys, _ in at_ini)
        out_row = []
        for rect, (keys, any_corner) in zip(row, at_ini):
            if variant == "fallback_before_nms":
                fall_back = not any_corner
            elif variant == "fallback_per_row":
                fall_back = not row_found
            else:
                fall_back = not keys
            if fall_back:
                keys = _cell_keys(M, rect, min_th, variant)[0]
            elif variant == "fallback_adds":
                keys = sorted(set(keys) | set(_cell_keys(M, rect, min_th, variant)[0]), key=lambda k: (k[1], k[0]))
            if variant == "emit_column_major":
                keys = sorted(keys, key=lambda k: (k[0], k[1]))
            out_row.append(keys)
        per_cell.append(out_row)
    if variant == "cells_column_major":
        order = [(i, j) for j in range(max(len(r) for r in per_cell)) for i in range(len(per_cell)) if j < len(per_cell[i])] if per_cell else []
    else:
        order = [(i, j) for i in range(len(per_cell)) for j in range(len(per_cell[i]))]
    return [k for i, j in order for k in per_cell[i][j]]


def level_candidates(img, ini_th, min_th, variant="exact"):
    """[(x, y, response)] of one pyramid level, coordinates relative to MIN_BORDER, in the order of vToDistributeKeys"""
    assert img.dtype == np.uint8 and img.ndim == 2
    if variant != "exact":
        assert variant in VARIANTS, variant
        return _variant_candidates(img, ini_th, min_th, variant)
    out = []
    for row in cells_of_level(img.shape[1], img.shape[0]):
        for x0, x1, y0, y1 in row:
            sub = img[y0:y1, x0:x1]
            keys = fast_definitional(sub, ini_th)
            if not keys:
                keys = fast_definitional(sub, min_th)
            out += [(int(x) + x0 - MIN_BORDER, int(y) + y0 - MIN_BORDER, int(s)) for x, y, s in keys]
    return out


def mask_words(img, cands):
    """a row-major restatement of the kernel's winner masks: per cell (row-major) the number of 32-bit words of its interior's bitmask,
    bit = y * interior width + x, and the set of words that hold a winner"""
    out = []
    for row in cells_of_level(img.shape[1], img.shape[0]):
        for x0, x1, y0, y1 in row:
            iw, ih = x1 - x0 - 6, y1 - y0 - 6
            used = set()
            for x, y, _ in cands:
                xl, yl = x + MIN_BORDER - (x0 + 3), y + MIN_BORDER - (y0 + 3)
                if 0 <= xl < iw and 0 <= yl < ih:
                    used.add((yl * iw + xl) >> 5)
            out.append(((iw * ih + 31) >> 5, used))
    return out
