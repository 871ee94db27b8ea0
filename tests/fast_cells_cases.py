"""Designed frames for the decisions of the FAST cell kernel (k_fast_strips) that whole-frame extraction of textured images reaches by
chance or not at all: the quick test's selectors and saturation, the strict thresholds, the per-cell fallback decided after the
suppression, the strict 3x3 suppression that stops at the cell interior, the ranking inside the row-major bitmask and the order of the
cells.  tests/test_fast_cells_reference.py (CPU) and tests/test_fast_cells_gpu.py share them.

Every frame has ONE pyramid level -- the pixels are exactly what is drawn here -- and the extractor arguments ARGS.  The size is
240 x 110: two cell rows (interior rows 19..57 and 58..90) of five cells whose interiors start at x = 19, 61, 103, 145 and 187, each cell
row two strips of 2 and 3 cells.  So one frame has a cell border inside a strip (x = 60|61, 144|145, 186|187), a strip border inside a
cell row (102|103) and a cell-row border (y = 57|58, another workgroup).  geometry() asserts all of this from the restated host set-up.

Two building blocks, on a flat background b:
  a DOT    one pixel at b - m: exactly one corner, M = m (all sixteen ring pixels are brighter by m), response m - 1.  A second dot does
           not change that unless it lies on the first one's ring, and ring offsets have a component of 3 (or are (+-2, +-2)): dots at
           distance 1, or with a component of 4 or more, have independently chosen scores.
  a STAMP  the nine ring pixels (rot + j) % 16, j < 9, of a centre at b +- m, optionally the other seven at b -+ m: the centre is a
           corner with M = m through an arc of exactly nine.  Stamps make by-product corners around them; the reference decides those.
           A uniform stamp with m = t is rejected by the quick test already, which sees ring pixels 0, 4, 8 and 12 only; a GRADED stamp
           has those one grey level further out than the rest of the arc, so that the score tree's M = t reaches `M > t`.

A case says what must happen in it (Case.expected: the whole list, for the frames of dots, worked out by hand when the frame is drawn;
Case.present / Case.absent / Case.empty for the stamps), and assert_design() holds the REFERENCE's own output to that: a case whose event does not
happen in the reference fails, whatever the device does.

Run as a program it checks every 240 x 110 frame with ORBX_STRIP_WIDTH = 250, where a cell row is ONE strip of five cells; the width is
read once per process, so that configuration needs a process of its own."""
import importlib
import os
import sys

import numpy as np

import fast_cells_reference as fr
import fast_strip_setup_cases as sc

W, H = 240, 110
INI, MIN = 20, 7
ARGS = (500, 1.2, 1, INI, MIN)
CELL_X = (19, 61, 103, 145, 187, 221)       # first interior column of the five cells, and the end of the last one
CELL_Y = (19, 58, 91)


def geometry(strip_width=160):
    """the cells and strips that every case relies on"""
    rows = sc.cells_of_level(W, H)
    assert [[(x0 + 3, x1 - 3, y0 + 3, y1 - 3) for x0, x1, y0, y1 in row] for row in rows] == \
        [[(CELL_X[j], CELL_X[j + 1], CELL_Y[i], CELL_Y[i + 1]) for j in range(5)] for i in range(2)], rows
    assert [row[j][0] for row in rows for j in range(5)] == [16, 58, 100, 142, 184] * 2
    geo = sc.strips([(W, H)], strip_width)
    assert [s["ncell"] for s in geo] == ([2, 3, 2, 3] if strip_width == 160 else [5, 5]), geo
    return rows


def cell_of(x, y):
    """(cell row, cell column) whose interior holds level pixel (x, y), or None"""
    if not (CELL_X[0] <= x < CELL_X[-1] and CELL_Y[0] <= y < CELL_Y[-1]):
        return None
    return (int(y >= CELL_Y[1]), max(j for j in range(5) if x >= CELL_X[j]))


class Case:
    def __init__(self, name, background=100):
        geometry()
        self.name = name
        self.img = np.full((H, W), background, np.uint8)
        self.dots = []          # (x, y, m, keep)
        self.present = []       # (x, y, response): must be in the reference's list
        self.absent = []        # (x, y, M): the pixel has exactly this M in the reference's margin map and is not in its list
        self.empty = False      # the reference's list must be empty
        self.only_dots = True
        self.extra = None       # further statement about the reference's list

    def dot(self, x, y, m, keep, sign=-1):
        """keep: the hand-made statement whether the reference reports this pixel (with response m - 1)"""
        b = int(self.img[y, x])
        assert all((px, py) != (x, y) and (px - x, py - y) not in fr.RING for px, py, _, _ in self.dots), "dot (%d, %d) collides" % (x, y)
        assert 0 <= b + sign * m <= 255
        self.img[y, x] = b + sign * m
        self.dots.append((x, y, m, keep))
        assert not keep or cell_of(x, y) is not None
        return self

    def stamp(self, cx, cy, rot, m, sign, opposite=False, compass=None):
        """compass: the margin of the arc's ring pixels 0, 4, 8 and 12, the ones the quick test looks at, if not m"""
        b = int(self.img[cy, cx])
        for k, (dx, dy) in enumerate(fr.RING):
            if (k - rot) % 16 < 9:
                self.img[cy + dy, cx + dx] = b + sign * (compass if compass is not None and k % 4 == 0 else m)
            elif opposite:
                self.img[cy + dy, cx + dx] = b - sign * m
        self.only_dots = False

    def expected(self):
        """the whole list of a frame of dots: the kept ones, cell by cell, row-major inside the cell, relative to the border of 16"""
        assert self.only_dots
        out = []
        for i in range(2):
            for j in range(5):
                mine = sorted((y, x, m) for x, y, m, keep in self.dots if keep and cell_of(x, y) == (i, j))
                out += [(x - 16, y - 16, m - 1) for y, x, m in mine]
        return out

    def finish(self):
        self.img.setflags(write=False)
        return self


def assert_design(case, cands):
    """cands: the REFERENCE's list for the case's frame.  The event the case was drawn for happens in it."""
    if case.only_dots:
        assert case.dots and cands == case.expected(), "%s: the reference gives\n%r\nthe case was drawn for\n%r" % (case.name, cands, case.expected())
    if case.empty:
        assert cands == [], "%s: %d keys in a frame drawn to have none" % (case.name, len(cands))
    else:
        assert cands, "%s: no key at all" % case.name
    have = set(cands)
    for x, y, r in case.present:
        assert (x - 16, y - 16, r) in have, "%s: (%d, %d) with response %d is not in the reference's list" % (case.name, x, y, r)
    if case.absent:
        M, at = fr.margin_map(case.img), set((x, y) for x, y, _ in cands)
        for x, y, m in case.absent:
            assert M[y, x] == m and (x - 16, y - 16) not in at, "%s: (%d, %d) has M = %d and is %s the list" % (
                case.name, x, y, M[y, x], "in" if (x - 16, y - 16) in at else "not in")
    if case.extra is not None:
        case.extra(cands)


def cells_with_keys(cands):
    return set(cell_of(x + 16, y + 16) for x, y, _ in cands)


ALL_CELLS = set((i, j) for i in range(2) for j in range(5))


# ---- stamp sheets: 16 rotations x every x mod 4 of the centre (x mod 4 = the pixel's place in the quick test's quad), both cell rows,
# every row of a wave (y mod 4) ----
def stamp_sheet(name, m, sign, background=100, opposite=False):
    c = Case(name, background)
    combos = set()
    for r in range(6):
        for i in range(16):
            cx, cy = 22 + 12 * i + (i & 3), 22 + 13 * r
            rot = ((i >> 2) + 4 * r + 2 * (r >> 2)) % 16
            c.stamp(cx, cy, rot, m, sign, opposite)
            combos.add((rot, cx & 3))
            if m > MIN:
                c.present.append((cx, cy, m - 1))
    assert len(combos) == 64
    c.empty = m <= MIN
    if opposite:            # (ring pixels 2 m apart: by-products above m)
        c.extra = lambda cands: _assert(cells_with_keys(cands) == ALL_CELLS and min(r for _, _, r in cands) >= INI, name)
    elif m == INI + 1:      # every cell has keys at iniThFAST, and no pixel has a larger margin than the stamps'
        c.extra = lambda cands: _assert(cells_with_keys(cands) == ALL_CELLS and set(r for _, _, r in cands) == {INI}, name)
    elif m > MIN:           # no corner at iniThFAST anywhere: every cell falls back, and finds its stamps
        c.extra = lambda cands: _assert(cells_with_keys(cands) == ALL_CELLS and max(r for _, _, r in cands) == m - 1 < INI, name)
    return c.finish()


def _assert(ok, what):
    assert ok, what


def graded_sheet(name, m, sign):
    """stamps whose ring pixels 0, 4, 8 and 12 -- all the quick test sees -- are one grey level further out than the rest of the arc:
    the quick test passes at t = m, the score tree gives M = m exactly, and `M > t` in stage 2 (and again in the scan after an overflow)
    is what decides.  The compass pixels themselves are dots with M = m + 1, so no cell is empty at that threshold: at m = iniThFAST
    and at m = minThFAST the centres are scored, held in the map and NOT reported; one above, they are."""
    c = Case(name)
    for r in range(6):
        for i in range(16):
            cx, cy = 22 + 12 * i + (i & 3), 22 + 13 * r
            c.stamp(cx, cy, ((i >> 2) + 4 * r + 2 * (r >> 2)) % 16, m, sign, compass=m + 1)
            if m in (INI, MIN):
                c.absent.append((cx, cy, m))
            else:
                c.present.append((cx, cy, m - 1))
    if m < INI:             # no corner at iniThFAST: every cell falls back
        c.extra = lambda cands: _assert(cells_with_keys(cands) == ALL_CELLS and max(r for _, _, r in cands) < INI, name)
    else:
        c.extra = lambda cands: _assert(cells_with_keys(cands) == ALL_CELLS and min(r for _, _, r in cands) >= INI, name)
    return c.finish()


def sheet_cases():
    out = []
    for m in (21, 20, 8, 7):
        for sign in (+1, -1):
            out.append(stamp_sheet("sheet m=%d %s" % (m, "bright" if sign > 0 else "dark"), m, sign))
    # the ends of the grey range, for the polarity that fits in a byte: v - t saturates at 0 below 20, v + t exceeds a byte above 235; at
    # 21 / 234 the ring itself is 0 / 255
    for b, sign in ((0, +1), (19, +1), (20, +1), (234, +1), (21, -1), (235, -1), (236, -1), (255, -1)):
        out.append(stamp_sheet("sheet m=21 on %d %s" % (b, "bright" if sign > 0 else "dark"), 21, sign, background=b))
    # both polarities of the quick test live at once: the other seven ring pixels on the opposite side by the same margin
    for sign in (+1, -1):
        out.append(stamp_sheet("sheet m=21 %s, rest opposite" % ("bright" if sign > 0 else "dark"), 21, sign, opposite=True))
    for m, sign in ((20, +1), (20, -1), (7, +1), (7, -1), (21, -1), (8, +1)):
        out.append(graded_sheet("graded sheet m=%d %s" % (m, "bright" if sign > 0 else "dark"), m, sign))
    return out


# ---- threshold and fallback per cell ----
def _slot(cell, k):
    """k-th place of a 5-pixel lattice inside a cell's interior"""
    i, j = cell
    return CELL_X[j] + 4 + 5 * (k % 6), CELL_Y[i] + 4 + 5 * (k // 6)


def threshold_case(name, A, B, Cs):
    """A: one dot with M = 21 among dots with M in 8..20 -> the single key.  B: only M <= 20, with M = 8 and M = 7 -> falls back, all but
    the M = 7.  C: an equal adjacent pair with M = 30 and a dot with M = 12 -> the pair empties the cell at iniThFAST, so it falls back."""
    c = Case(name)
    for k, m in enumerate((12, 20, 21, 8, 15, 19, 9)):
        c.dot(*_slot(A, k), m, keep=(m == 21))
    for k, m in enumerate((20, 8, 7, 13, 19, 9, 16)):
        c.dot(*_slot(B, k), m, keep=(m != 7))
    for C in Cs:
        x, y = _slot(C, 1)
        c.dot(x, y, 30, keep=False).dot(x + 1, y, 30, keep=False)
        c.dot(*_slot(C, 9), 12, keep=True)
    return c.finish()


# ---- suppression inside a cell ----
ORIENT = ((1, 0), (0, 1), (1, 1), (1, -1))


def _pair_slot(cell, k):
    i, j = cell
    return CELL_X[j] + 2 + 6 * (k % 6), CELL_Y[i] + 3 + 6 * (k // 6)


def pairs_case():
    """horizontal, vertical and both diagonal pairs, in both orders, for each pair of M: at iniThFAST in cells (0, 0) and (1, 3), in the
    fallback cells (0, 1) and (1, 2); chains of three in cells (0, 3) (iniThFAST) and (1, 0) (fallback)"""
    c = Case("pairs inside a cell")

    def pairs(cell, kinds):
        k = 0
        for ma, mb, keep_a, keep_b in kinds:
            for dx, dy in ORIENT:
                x, y = _pair_slot(cell, k)
                c.dot(x, y, ma, keep_a).dot(x + dx, y + dy, mb, keep_b)
                k += 1
        assert k <= 30          # (five rows of six places fit the lower cell row as well)
    # iniThFAST: equal; M and M + 1; 21 beside 20, which is no corner at 20 and counts as 0
    strong = [(25, 25, False, False), (25, 26, False, True), (26, 25, True, False), (21, 20, True, False), (20, 21, False, True),
              (21, 21, False, False), (22, 21, True, False)]
    pairs((0, 0), strong)
    pairs((1, 3), strong[::-1])
    # fallback cells: nothing above 20.  8 beside 7, which is no corner at 7; 15 beside 9, both corners
    faint = [(12, 12, False, False), (12, 13, False, True), (13, 12, True, False), (8, 7, True, False), (7, 8, False, True),
             (15, 9, True, False), (9, 15, False, True), (8, 8, False, False), (20, 20, False, False), (20, 19, True, False)]
    pairs((0, 1), faint[:7])
    pairs((1, 2), faint[3:])

    def chains(cell, lo):
        i, j = cell
        x, y = CELL_X[j] + 3, CELL_Y[i] + 3
        a, b, top = lo, lo + 1, lo + 10
        c.dot(x, y, a, False).dot(x + 1, y, b, False).dot(x + 2, y, top, True)                       # a < b < top in a row: only top
        c.dot(x + 8, y, b, True).dot(x + 9, y, a, False).dot(x + 10, y, b, True)                     # b a b: both b
        c.dot(x + 16, y, a, False).dot(x + 17, y, a, False).dot(x + 18, y, a, False)                 # a a a: none
        c.dot(x + 24, y, top, True).dot(x + 25, y, b, False).dot(x + 26, y, a, False)                # descending
        c.dot(x, y + 8, b, False).dot(x + 1, y + 8, a, False).dot(x, y + 9, top, True)               # an L: top under b, diagonal to a
        c.dot(x + 8, y + 8, a, False).dot(x + 8, y + 9, b, False).dot(x + 8, y + 10, top, True)      # a column
        # (three on a diagonal would put the third on the first one's ring, offset (2, 2))
        c.dot(x + 16, y + 8, top, True).dot(x + 17, y + 9, b, False).dot(x + 17, y + 10, a, False)   # a diagonal step, then down
        c.dot(x + 24, y + 10, a, False).dot(x + 25, y + 9, b, False).dot(x + 25, y + 8, b, False)    # the other diagonal, b b at its end
        c.dot(x, y + 16, b, True).dot(x + 1, y + 17, a, False).dot(x + 2, y + 16, b, True)           # a V: a under two b
    chains((0, 3), 30)
    chains((1, 0), 9)
    return c.finish()


# ---- suppression at every border ----
def border_case(name, lo, hi, equal_pairs_survive=True):
    """adjacent pairs (lo, lo) and (lo, hi) astride every kind of border -- both pixels survive, each in its own cell -- and one pixel
    to either side of it, where both lie in one interior and the suppression applies"""
    c = Case(name)
    for n, bx in enumerate(CELL_X[1:5]):            # 61: inside strip 0; 103: the strip border; 145, 187: inside strip 1
        y = CELL_Y[0] + 3
        # cell row 0: astride the border, left pixel bx - 1, right pixel bx
        c.dot(bx - 1, y, lo, True).dot(bx, y, lo, True)                         # horizontal, equal
        c.dot(bx - 1, y + 6, hi, True).dot(bx, y + 6, lo, True)                 # horizontal, unequal
        c.dot(bx - 1, y + 12, lo, True).dot(bx, y + 13, lo, True)               # diagonal, equal
        c.dot(bx - 1, y + 19, lo, True).dot(bx, y + 18, hi, True)               # other diagonal, unequal
        c.dot(bx - 1, y + 24, hi, True).dot(bx, y + 25, lo, True)               # diagonal, unequal
        c.dot(bx - 1, y + 31, lo, True).dot(bx, y + 30, lo, True)               # other diagonal, equal
        # cell row 1: the same pairs one pixel to the left (both in the left cell) and to the right (both in the right cell)
        y = CELL_Y[1] + 4
        c.dot(bx - 2, y, lo, False).dot(bx - 1, y, lo, False)
        c.dot(bx - 2, y + 6, lo, False).dot(bx - 1, y + 7, hi, True)
        c.dot(bx, y + 12, lo, False).dot(bx + 1, y + 12, hi, True)
        c.dot(bx, y + 19, lo, False).dot(bx + 1, y + 18, lo, False)
        c.dot(bx - 2, y + 24, hi, True).dot(bx - 1, y + 24, lo, False)
        # the point where four cells meet: diagonal pairs whose pixels lie in diagonally opposite cells
        yb = CELL_Y[1]
        if n % 2 == 0:
            c.dot(bx - 1, yb - 1, lo, True).dot(bx, yb, lo if n == 0 else hi, True)
        else:
            c.dot(bx, yb - 1, hi if n == 1 else lo, True).dot(bx - 1, yb, lo, True)
    # the cell-row border y = 57 | 58, per cell column: astride (cells 0, 2, 4: strip 0 and strip 1), one row up (cell 1), one row down (3)
    for j in range(5):
        x = CELL_X[j] + 8
        dy, keep = {0: (0, True), 1: (-1, False), 2: (0, True), 3: (+1, False), 4: (0, True)}[j]
        y = CELL_Y[1] - 1 + dy
        c.dot(x, y, lo, keep).dot(x, y + 1, lo, keep)                           # vertical, equal
        c.dot(x + 6, y, lo, keep).dot(x + 6, y + 1, hi, True)                   # vertical, unequal
        c.dot(x + 12, y, lo, keep).dot(x + 13, y + 1, lo, keep)                 # diagonal, equal
        c.dot(x + 19, y, hi, True).dot(x + 18, y + 1, lo, keep)                 # other diagonal, unequal
    return c.finish()


def edges_case(name, lo):
    """the first and last detection row and column (x = 19 and W - 20, y = 19 and H - 20) and one pixel outside, which is not reported
    and suppresses nothing although it is the stronger one"""
    c = Case(name)
    hi = lo + 9
    for x, y, m in ((19, 19, lo), (W - 20, 19, lo + 1), (19, H - 20, lo + 2), (W - 20, H - 20, lo + 3)):
        c.dot(x, y, m, True)
    c.dot(18, 30, hi, False).dot(19, 30, lo, True)
    c.dot(W - 19, 40, hi, False).dot(W - 20, 40, lo, True)
    c.dot(50, 18, hi, False).dot(50, 19, lo, True)
    c.dot(70, H - 19, hi, False).dot(70, H - 20, lo, True)
    c.dot(18, 18, hi, False).dot(W - 19, H - 19, hi, False)
    c.dot(18, 70, hi, False).dot(W - 19, 75, hi, False).dot(130, 18, hi, False).dot(150, H - 19, hi, False)
    c.dot(18, 50, hi, False).dot(19, 51, lo, True)                              # diagonal to a stronger pixel outside
    c.dot(170, H - 19, hi, False).dot(171, H - 20, lo, True)
    for j in range(5):                                                          # (no cell without a key)
        for i in range(2):
            c.dot(CELL_X[j] + 20, CELL_Y[i] + 15, lo + 4, True)
    return c.finish()


# ---- ranking ----
def ranking_case():
    """a lattice of dots with pitch 4 in x and 2 in y fills a cell: 220 winners (231 in the first column's cells), their bits spread over
    the words of the cell's row-major mask, so that a key's rank needs the word prefix and the popcount inside the word; the cell next
    to it has a single dot on its LAST interior pixel (the last bit of the mask).  Cell (0, 2) at iniThFAST, cell (1, 0) in the fallback.
    Pitch 2 in x and 4 in y leaves three rows in four empty and covers under 60 % of the words: cell (0, 4) has it as well, 170 winners,
    for the popcount inside densely set words, without the statement about the words."""
    c = Case("ranking")

    def lattice(cell, base, span, px=4, py=2):
        i, j = cell
        for iy, y in enumerate(range(CELL_Y[i], CELL_Y[i + 1], py)):
            for ix, x in enumerate(range(CELL_X[j], CELL_X[j + 1], px)):
                c.dot(x, y, base + (3 * ix + 5 * iy) % span, True)
    lattice((0, 2), 21, 40)
    lattice((0, 4), 21, 40, px=2, py=4)                     # sixteen winners to a word, three rows in four empty: 170
    c.dot(CELL_X[4] - 1, CELL_Y[1] - 1, 25, True)           # last interior pixel of cell (0, 3)
    lattice((1, 0), 8, 13)
    c.dot(CELL_X[2] - 1, CELL_Y[2] - 1, 9, True)            # last interior pixel of cell (1, 1)

    def spread(cands):
        words = fr.mask_words(c.img, cands)
        for cell in (2, 5):
            n_words, used = words[cell]
            assert 3 * len(used) >= 2 * n_words and 0 in used and n_words - 1 in used, "%d of %d mask words" % (len(used), n_words)
        for cell in (3, 6):
            n_words, used = words[cell]
            assert used == {n_words - 1}
        for cell in ((0, 2), (0, 4)):
            assert sum(1 for x, y, _ in cands if cell_of(x + 16, y + 16) == cell) > 100
    c.extra = spread
    return c.finish()


_cases = None


def cases():
    """every 240 x 110 frame, by name, in a fixed order"""
    global _cases
    if _cases is None:
        out = sheet_cases()
        out.append(threshold_case("threshold and fallback, one strip", A=(0, 0), B=(0, 1), Cs=[(0, 2)]))
        out.append(threshold_case("threshold and fallback, across strips", A=(1, 1), B=(1, 2), Cs=[(1, 4), (0, 0), (0, 3)]))
        out.append(pairs_case())
        out.append(border_case("borders at iniThFAST", 25, 31))
        out.append(border_case("borders in the fallback", 10, 16))
        out.append(edges_case("edges at iniThFAST", 30))
        out.append(edges_case("edges in the fallback", 9))
        out.append(ranking_case())
        _cases = dict((c.name, c) for c in out)
        assert len(_cases) == len(out)
    return _cases


_numpy = {}


def numpy_candidates(name):
    """the numpy reference's list for a case, computed once, with the case's own statement held against it"""
    if name not in _numpy:
        case = cases()[name]
        cands = fr.level_candidates(case.img, INI, MIN)
        assert_design(case, cands)
        _numpy[name] = tuple(cands)
    return list(_numpy[name])


def as_tuples(kp):
    """candidates as the device or the oracle returns them (KP_DTYPE) -> [(x, y, response)]; all three are integers held in floats"""
    for f in ("x", "y", "response"):
        assert np.array_equal(kp[f], np.round(kp[f]))
    return list(zip(kp["x"].astype(np.int64).tolist(), kp["y"].astype(np.int64).tolist(), kp["response"].astype(np.int64).tolist()))


def assert_candidates(got, want, what):
    """count, then x, y and response in order"""
    assert len(got) == len(want), "%s: %d candidates, the reference has %d" % (what, len(got), len(want))
    bad = [k for k in range(len(want)) if got[k] != want[k]]
    assert not bad, "%s: %d of %d candidates differ, first at %d: got %r, want %r" % (what, len(bad), len(want), bad[0], got[bad[0]], want[bad[0]])


# the noise frames: (name, width, height, levels, seed)
NOISE = [("noise 200x150, 3 levels", 200, 150, 3, 71), ("noise 320x240, 2 levels", 320, 240, 2, 72)]


def run_batch(pkg, oracle, names, what, corner_cap=None):
    """the frames `names` as one host batch: the candidates against the numpy reference, then candidates, key points and descriptors
    against the oracle"""
    refs = [sc.reference(oracle, ("fast cells", n), cases()[n].img, ARGS) for n in names]
    ex = pkg.Extractor(*ARGS)
    try:
        if corner_cap is not None:
            ex.debug_set_fast_corner_cap(corner_cap)
        mono, n, kps, desc = ex.extract_batch(np.stack([r["img"] for r in refs]))
        for b, name in enumerate(names):
            w = "%s, frame %d of %d (%s)" % (what, b, len(names), name)
            want = numpy_candidates(name)
            assert_candidates(as_tuples(ex.candidates(0, frame=b, cap=len(want) + 64)), want, w)
            sc.assert_same(ex, refs[b], mono[b], kps[b, :n[b]], desc[b, :n[b]], b, w)
    finally:
        ex.close()


def batches(names, size, seed=None):
    names = list(names)
    if seed is not None:
        names = [names[i] for i in np.random.RandomState(seed).permutation(len(names))]
    return [names[i:i + size] for i in range(0, len(names), size)]


def main():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for p in (root, os.path.join(root, "tests")):
        if p not in sys.path:
            sys.path.insert(0, p)
    import torch  # noqa: F401  (before the package: one HIP runtime per process, see conftest.py)
    from oracle_api import Oracle
    pkg = importlib.import_module("orb_slam3-1_amd")
    assert os.environ.get("ORBX_STRIP_WIDTH") == "250"
    geometry(250)           # a cell row is one strip: no strip border, four cell borders inside the strip
    oracle = Oracle()
    for cap in (None, 1):
        for k, names in enumerate(batches(cases(), 5, seed=5 if cap else None)):
            run_batch(pkg, oracle, names, "one strip per cell row, corner cap %r, batch %d" % (cap, k), corner_cap=cap)
    print("wide strips ok")


if __name__ == "__main__":
    main()
