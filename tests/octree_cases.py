"""Dot images that drive DistributeOctTree precisely through the public extractor (tests of the octree's waves).

An all-black image with isolated single bright pixels, at least 4 pixels apart and at least 24 from the border, gives a one-level
extractor `Extractor(N, 1.2, 1, 20, 7)` exactly one FAST candidate per dot, with response = value - 1: where the dots are fixes
every node's key count, and N fixes where the sorted phase cuts.

Geometry of level 0 of a w x h image: the tree covers [0, w - 32) x [0, h - 32) in coordinates relative to column / row 16;
nIni = round((w - 32) / (h - 32)) roots side by side; a node splits at ceil(half) of its sides.  320 x 240 has one root of 288 x 208
whose quadrants are 144 x 104, then 72 x 52, 36 x 26, 18 x 13."""
import numpy as np

ARGS_TAIL = (1.2, 1, 20, 7)
BORDER = 16


def block(rx, ry, n, cols, step=4):
    """n dots row-major in rows of `cols`, first at relative (rx, ry)"""
    return [(rx + step * (i % cols), ry + step * (i // cols)) for i in range(n)]


def grid(rx0, ry0, rx1, ry1, step=4):
    return [(x, y) for y in range(ry0, ry1, step) for x in range(rx0, rx1, step)]


def _value(x, y, mode):
    """mode 'flat': every response equal (ties inside every node: the first key must win); 'mixed': 50 .. 249"""
    return 200 if mode == "flat" else 50 + (x * 7 + y * 13 + (x * y) % 11) % 200


class Case:
    def __init__(self, name, w, h, N, dots, mode="mixed"):
        self.name, self.w, self.h, self.N, self.mode = name, w, h, N, mode
        self.dots = sorted(set(dots), key=lambda d: (d[1], d[0]))
        for x, y in self.dots:
            assert 8 <= x < w - 32 - 8 and 8 <= y < h - 32 - 8, (name, x, y)         # 24 pixels from the border
        pts = np.array(self.dots, int).reshape(-1, 2)
        if len(pts) > 1:
            d = np.abs(pts[:, None, :] - pts[None, :, :]).max(axis=2)
            np.fill_diagonal(d, 99)
            assert d.min() >= 4, name

    @property
    def args(self):
        return (self.N,) + ARGS_TAIL

    def image(self):
        img = np.zeros((self.h, self.w), np.uint8)
        for x, y in self.dots:
            img[y + BORDER, x + BORDER] = _value(x, y, self.mode)
        return img

    def candidates(self):
        """(x, y, response) of level 0's candidates in vToDistributeKeys order: cell row-major, row-major inside a cell"""
        def cell_of(v, n):
            width = n - 32
            ncell = max(width // 35, 1)
            wcell = -(-width // ncell)
            return min((v - 3) // wcell, ncell - 1) if v >= 3 else 0
        order = sorted(self.dots, key=lambda d: (cell_of(d[1], self.h), cell_of(d[0], self.w), d[1], d[0]))
        x = np.array([d[0] for d in order], np.float32)
        y = np.array([d[1] for d in order], np.float32)
        r = np.array([_value(d[0], d[1], self.mode) - 1 for d in order], np.float32)
        return x, y, r


def _quadrant_blocks(counts, cols=20):
    """one block of dots per quadrant of the 288 x 208 root (0 = none), in child order n1..n4"""
    org = [(8, 8), (148, 8), (8, 108), (148, 108)]
    dots = []
    for (ox, oy), n in zip(org, counts):
        dots += block(ox, oy, n, cols)
    return dots


def _sub_blocks(per_sub, cols=6):
    """per_sub[q][s]: dots in sub-quadrant s (72 x 52) of quadrant q of the 288 x 208 root"""
    dots = []
    for q, subs in enumerate(per_sub):
        qx, qy = 144 * (q & 1), 104 * (q >> 1)
        for s, n in enumerate(subs):
            ox, oy = qx + 72 * (s & 1) + 8, qy + 52 * (s >> 1) + 8
            dots += block(ox, oy, n, cols)
    return dots


def build_cases():
    c = []
    full = grid(8, 8, 280, 200)                 # 68 x 48 = 3264 dots
    # one-by-one key counts with at most 6 active lanes (every divisible node goes one by one)
    c.append(Case("quad_257_256_65_64", 320, 240, 40, _quadrant_blocks([257, 256, 65, 64])))
    c.append(Case("quad_33_32_2", 320, 240, 40, _quadrant_blocks([33, 32, 2, 0])))
    c.append(Case("quad_two", 320, 240, 40, _quadrant_blocks([40, 0, 0, 9])))
    # five, six and seven divisible nodes in one batch (both sides of the "at most 6" rule); a quadrant with ONE sub-block has three
    # empty children
    c.append(Case("sub_5", 320, 240, 60, _sub_blocks([[36, 35, 34, 40], [45, 0, 0, 0], [], []])))
    c.append(Case("sub_6", 320, 240, 60, _sub_blocks([[36, 35, 34, 40], [45, 33, 0, 0], [], []])))
    c.append(Case("sub_7", 320, 240, 60, _sub_blocks([[36, 35, 34, 40], [45, 33, 0, 20], [], []])))
    c.append(Case("sub_7_flat", 320, 240, 200, _sub_blocks([[54, 35, 34, 40], [45, 33, 5, 20], [3, 0, 0, 0], [0, 0, 0, 2]]), "flat"))
    # the sorted phase: 4 quadrants of 4 sub-blocks; N = 8 is reached by the second of four one-by-one nodes
    sixteen = _sub_blocks([[40, 36, 35, 34], [39, 38, 37, 33], [44, 43, 42, 41], [48, 47, 46, 45]])
    c.append(Case("sorted_cut_lane1", 320, 240, 8, sixteen))
    c.append(Case("sorted_cut_lane0", 320, 240, 6, sixteen))
    c.append(Case("first_pass_n", 320, 240, 3, sixteen))
    # the full grid: 64 one-by-one nodes in one batch, passes of several batches, N reached at lane 63 / lane 0 of a later batch
    c.append(Case("grid_n1000", 320, 240, 1000, full))
    c.append(Case("grid_n448_flat", 320, 240, 448, full, "flat"))
    c.append(Case("grid_n100_rounds", 320, 240, 100, full))
    c.append(Case("grid8_n2000", 320, 240, 2000, grid(8, 8, 280, 200, 8)))
    # 33 .. 35 dots in every 36 x 26 node: a FULL batch of 64 one-by-one nodes; in the upper half only: 32, then a pass of two batches
    def nodes(rows):
        d = []
        for j in range(rows):
            for i in range(8):
                d += block(36 * i + (8 if i == 0 else 0), 26 * j + (9 if j == 0 else 0 if j == 7 else 3), 33 + (i + j) % 3, 7)
        return d
    c.append(Case("nodes_64", 320, 240, 1000, nodes(8)))
    c.append(Case("nodes_32", 320, 240, 600, nodes(4), "flat"))
    # totals around one block of lanes; a lone key ends by size == prev_size
    c.append(Case("blank", 320, 240, 50, []))
    c.append(Case("one", 320, 240, 50, [(100, 60)]))
    c.append(Case("total_63", 320, 240, 50, block(8, 8, 63, 9, 8)))
    c.append(Case("total_64", 320, 240, 50, block(8, 8, 64, 8, 8), "flat"))
    c.append(Case("total_65", 320, 240, 500, block(8, 8, 65, 13, 8)))
    # wide images: nIni = 2 and 4, one root empty
    c.append(Case("wide2", 160, 96, 30, block(8, 8, 70, 10) + block(70, 12, 20, 5)))
    c.append(Case("wide2_empty_root", 160, 96, 30, block(8, 8, 70, 12)))
    c.append(Case("wide4_empty_root", 288, 96, 100, block(8, 8, 100, 13) + block(136, 8, 90, 13) + block(200, 8, 110, 12)))
    c.append(Case("wide4", 288, 96, 60, grid(8, 8, 248, 56), "flat"))
    return c


CASES = build_cases()
BY_NAME = {c.name: c for c in CASES}
