"""Hand-built inputs for k_orient_desc (orientation + steered BRIEF), each made to sit ON one of the kernel's decisions, and the
expected outputs from the restatement of tests/orient_desc_reference.py.

A Scene is what orbx_debug_orient_desc takes: per frame and level an unblurred and a blurred image (independent of each other), a
key list (x, y, response, output row), the output capacity and the number of guard rows.  Shapes are the smallest that reach every
path: 75 x 66 with 3 levels (level sizes 75x66, 62x55, 52x46: room for one or two disjoint 31 x 31 patches per level), one 4-level
117 x 257 scene, nfeatures 20 so that every level has 32 selection slots.  tests/test_orient_desc_reference.py holds the restatement
to the CPU oracle on every key of every scene and checks the pins (the outcome a case was built for);
tests/test_orient_desc_boundaries_gpu.py holds the kernel to the same expectations, bit for bit.
"""
import functools
import json
import os

import numpy as np

import orient_desc_reference as ref
from oracle_api import KP_DTYPE

F = np.float32
NFEATURES, SCALE, INI_TH, MIN_TH = 20, 1.2, 20, 7
GEO_SMALL, GEO_TALL = (75, 66, 3), (117, 257, 4)
SEL_CAP = 32
CANARY, PAD = 0xC3, 0xA5
STEERING_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "orient_desc_steering_pairs.json")


def scale_table(nlevels):
    """mvScaleFactor (:409-417): float32 entries, each the previous one times the double of the float factor"""
    s = [F(1.0)]
    for _ in range(1, nlevels):
        s.append(F(float(s[-1]) * float(F(SCALE))))
    return s


def level_sizes(w, h, nlevels):
    """ComputePyramid (:1175): (w_l, h_l) = cvRound(size * mvInvScaleFactor[l]) in float32"""
    out = []
    for s in scale_table(nlevels):
        inv = F(1.0) / s
        out.append((int(np.rint(F(w) * inv)), int(np.rint(F(h) * inv))))
    return out


def in_disc(u, v):
    return abs(v) <= 15 and abs(u) <= ref.UMAX[abs(v)]


DISC = np.array([[in_disc(u, v) for u in range(-15, 16)] for v in range(-15, 16)])


class Scene:
    def __init__(self, name, geo, frames, seed, cap=48, guard=4):
        self.name, self.geo, self.B, self.cap, self.guard = name, geo, frames, cap, guard
        self.sizes = level_sizes(*geo)
        rs = np.random.RandomState(seed)
        self.rs = rs
        self.raw = [[rs.randint(0, 256, (h, w)).astype(np.uint8) for (w, h) in self.sizes] for _ in range(frames)]
        self.blur = [[rs.randint(0, 256, (h, w)).astype(np.uint8) for (w, h) in self.sizes] for _ in range(frames)]
        self.keys = [[[] for _ in self.sizes] for _ in range(frames)]
        self.pins = []          # (frame, level, index in the level's list, {what the case pins})
        self._slot = 0

    # ---- placement of designed patches: disjoint squares of `spacing` px on a grid that starts at the first legal centre ----
    def slots(self, spacing):
        out = []
        for b in range(self.B):
            for l, (w, h) in enumerate(self.sizes):
                for y in range(19, h - 20 + 1, spacing):
                    for x in range(19, w - 20 + 1, spacing):
                        out.append((b, l, x, y))
        return out

    def add(self, b, l, x, y, resp=None, row=None, pin=None):
        w, h = self.sizes[l]
        assert 19 <= x <= w - 20 and 19 <= y <= h - 20, (self.name, l, x, y)
        k = len(self.keys[b][l])
        assert k < SEL_CAP
        if resp is None:
            resp = int(self.rs.randint(0, 256))
        if row is None:
            row = sum(len(q) for q in self.keys[b])
        self.keys[b][l].append([x, y, resp, row])
        if pin is not None:
            self.pins.append((b, l, k, pin))
        return k

    def place(self, slot, patch=None, window=None, extra=(), **kw):
        """a designed key at grid slot (b, l, x, y): the 31 x 31 unblurred patch, the 37 x 37 blurred window, and single pixels
        (u, v, value) of the unblurred level set afterwards (they may lie outside the patch)"""
        b, l, x, y = slot
        if patch is not None:
            self.raw[b][l][y - 15:y + 16, x - 15:x + 16] = patch
        for (u, v, val) in extra:
            self.raw[b][l][y + v, x + u] = val
        if window is not None:
            self.blur[b][l][y - 18:y + 19, x - 18:x + 19] = window
        return self.add(b, l, x, y, **kw)

    def freeze(self):
        for f in self.raw + self.blur:
            for im in f:
                im.flags.writeable = False
        self.rs = None
        return self

    def n_keys(self):
        return sum(len(q) for f in self.keys for q in f)

    def key_arrays(self):
        return [[np.array(q, np.int32).reshape(-1, 4) for q in f] for f in self.keys]


# ---- patches with designed moments ----
def axis_patch(m01, m10, rs=None, background=False):
    """31 x 31 patch with the given moments: q at (+-15, 0) and r < 15 at (+-1, 0) give m10 = +-(15 q + r), likewise on the v axis
    (0, +-15) -- inside the disc -- for m01.  background: a point-symmetric random texture I(u, v) = I(-u, -v) under it, which adds
    nothing to either moment.  With rs the corners outside the disc hold random bytes, which the disc mask must ignore."""
    p = np.zeros((31, 31), np.int32)
    if background:
        t = rs.randint(0, 100, (31, 31))
        p = np.where(np.arange(31 * 31).reshape(31, 31) <= 480, t, t[::-1, ::-1])       # p[i, j] == p[30 - i, 30 - j]
        assert (p == p[::-1, ::-1]).all()
    for m, axis in ((m10, 0), (m01, 1)):
        s, (q, r) = (1 if m >= 0 else -1), divmod(abs(m), 15)
        assert q <= 155
        for dist, val in ((15, q), (1, r)):
            u, v = (s * dist, 0) if axis == 0 else (0, s * dist)
            p[15 + v, 15 + u] += val
    if rs is not None:
        p = np.where(DISC, p, rs.randint(0, 256, (31, 31)))
    assert p.min() >= 0 and p.max() <= 255
    return p.astype(np.uint8)


def half_disc(direction):
    """255 on one half of the disc (u > 0, u < 0, v > 0 or v < 0), 0 on the other half and on the axis between them: the largest
    moment the disc can hold, both byte dot products of a row at their maxima"""
    u, v = np.meshgrid(np.arange(-15, 16), np.arange(-15, 16))
    sel = {"+u": u > 0, "-u": u < 0, "+v": v > 0, "-v": v < 0}[direction]
    return np.where(sel & DISC, 255, 0).astype(np.uint8)


M_HALF = sum(abs(u) * 255 for v in range(-15, 16) for u in range(1, ref.UMAX[abs(v)] + 1))          # |m10| of half_disc("+u")
assert M_HALF == sum(v * 255 * (2 * ref.UMAX[v] + 1) for v in range(1, 16))                          # = |m01| of half_disc("+v")


def scene_moments():
    pairs = [((0, 0), 0.0), ((0, -7), 180.0), ((0, 7), 0.0), ((5, 0), 90.0), ((-5, 0), 270.0), ((0, -2325), 180.0), ((2325, 0), 90.0)]
    pairs += [((sy * 37, sx * 37), None) for sy in (1, -1) for sx in (1, -1)]                   # |m01| == |m10|: the >= branch
    pairs += [((sy * 2324, sx * 2324), None) for sy in (1, -1) for sx in (1, -1)]
    pairs += [((sy * (37 + d), sx * 37), None) for sy in (1, -1) for sx in (1, -1) for d in (1, -1)]      # |m01| = |m10| +- 1
    pairs += [((sy * (600 + d), sx * 600), None) for sy in (1, -1) for sx in (1, -1) for d in (1, -1)]
    pairs += [((-1, 2325), None), ((1, -2325), None), ((2325, -1), None), ((-2325, 1), None)]
    n_keys = 2 * len(pairs) + 4 + 4
    per_frame = len(Scene("probe", GEO_SMALL, 1, 0).slots(33))
    sc = Scene("moments", GEO_SMALL, -(-n_keys // per_frame), 101)
    slots = iter(sc.slots(33))
    for background in (False, True):
        for (m01, m10), angle in pairs:
            pin = {"moments": (m01, m10), "what": "axis pixels, m01 %d m10 %d%s" % (m01, m10, ", symmetric background" if background else "")}
            if angle is not None:
                pin["angle"] = angle
            sc.place(next(slots), axis_patch(m01, m10, sc.rs, background), pin=pin)
    # saturated half discs, and m01 = -+1 beside the largest m10 the disc can hold (the smallest non-zero angle: 360 - a tiny a)
    for d, mom, angle in (("+u", (0, M_HALF), 0.0), ("-u", (0, -M_HALF), 180.0), ("+v", (M_HALF, 0), 90.0), ("-v", (-M_HALF, 0), 270.0)):
        sc.place(next(slots), half_disc(d), pin={"moments": mom, "angle": angle, "what": "saturated half disc " + d})
    for d, (u, v), mom in (("+u", (0, -1), (-1, M_HALF)), ("+u", (0, 1), (1, M_HALF)), ("-u", (0, -1), (-1, -M_HALF)), ("+v", (-1, 0), (M_HALF, -1))):
        p = half_disc(d)
        p[15 + v, 15 + u] = 1
        sc.place(next(slots), p, pin={"moments": mom, "what": "saturated half disc %s and one grey level at (%d, %d)" % (d, u, v)})
    return sc.freeze()


def scene_disc_mask():
    """a flat patch with one bright pixel inside; then a single 255 ON the rim of every row (must move the angle) and a single 255
    just OUTSIDE it (must not), column u = +16 -- the kernel's ninth dword -- and the corners of the 31 x 31 square included"""
    base = np.full((31, 31), 7, np.uint8)
    base[15 + 5, 15 + 3] = 200
    cases = [("base", (), None)]
    for v in range(-15, 16):
        um = ref.UMAX[abs(v)]
        for s in (1, -1):
            cases.append(("rim (%d, %d)" % (s * um, v), ((s * um, v, 255),), True))
            cases.append(("outside (%d, %d)" % (s * (um + 1), v), ((s * (um + 1), v, 255),), False))
    for (u, v) in ((15, 15), (-15, 15), (15, -15), (-15, -15)):
        cases.append(("corner (%d, %d)" % (u, v), ((u, v, 255),), False))
    per_frame = len(Scene("probe", GEO_SMALL, 1, 0).slots(34))
    sc = Scene("disc_mask", GEO_SMALL, -(-len(cases) // per_frame), 102)
    for slot, (what, extra, moves) in zip(sc.slots(34), cases):
        b, l, x, y = slot
        sc.raw[b][l][y - 17:y + 18, x - 17:x + 18] = 7          # (flat around the square too: the pixel outside is the only change)
        sc.place(slot, base, extra=extra, pin={"what": what, "moves": moves})
    return sc.freeze()


def scene_alignment():
    """one patch and one blurred window at 16 consecutive px (every (px - 18) & 15 and (px - 15) & 3) and two py"""
    sc = Scene("alignment", GEO_SMALL, 32, 103)
    patch = sc.rs.randint(0, 256, (31, 31)).astype(np.uint8)
    window = sc.rs.randint(0, 256, (37, 37)).astype(np.uint8)
    for i in range(32):
        sc.place((i, 0, 19 + i % 16, (19, 24)[i // 16]), patch, window, resp=200, pin={"what": "alignment", "same_as_first": True})
    return sc.freeze()


def scene_level_edges(geo, name, seed):
    """the four extreme key positions of every level, in every frame: the last level of the last frame ends the device buffers"""
    sc = Scene(name, geo, 2, seed)
    for b in range(2):
        for l, (w, h) in enumerate(sc.sizes):
            for (x, y) in ((19, 19), (w - 20, 19), (19, h - 20), (w - 20, h - 20)):
                sc.add(b, l, x, y, pin={"what": "level edge"})
    return sc.freeze()


def load_steering_pairs():
    with open(STEERING_JSON) as f:
        return json.load(f)


def scenes_steering():
    """the moment pairs of the steering fixture, each over a window of random blurred bytes.  A coordinate rounded the wrong way
    reads another byte, but flips its comparison only about one time in three: the window is re-seeded until every deviation the
    pair is listed for gives a different descriptor (tests/test_orient_desc_reference.py checks that again, from the scene)"""
    pairs = load_steering_pairs()["pairs"]
    pattern = ref.load_pattern()
    variants_of = {"half_up": ("half_up",), "fma": ("fma", "fma_other"), "cos+": ("cos+",), "cos-": ("cos-",), "sin+": ("sin+",), "sin-": ("sin-",),
                   "angle": ("angle+", "angle-")}
    per_frame = len(Scene("probe", GEO_SMALL, 1, 0).slots(37))
    out = []
    per_scene = 64 * per_frame
    for i in range(0, len(pairs), per_scene):
        part = pairs[i:i + per_scene]
        sc = Scene("steering_%d" % (i // per_scene), GEO_SMALL, -(-len(part) // per_frame), 200 + i)
        for slot, (m01, m10, classes) in zip(sc.slots(37), part):
            angle = ref.fast_atan2_f32(F(m01), F(m10))

            def reads(variant):
                (r0, c0), (r1, c1) = ref.steer(angle, pattern[:, 0:2], variant), ref.steer(angle, pattern[:, 2:4], variant)
                return (18 + r0[0]) * 37 + 18 + c0[0], (18 + r1[0]) * 37 + 18 + c1[0]
            good = reads("exact")
            wrong = [reads(v) for cls in classes for v in variants_of[cls]]
            wrong = [w for w in wrong if (w[0] != good[0]).any() or (w[1] != good[1]).any()]
            for _ in range(500):
                window = sc.rs.randint(0, 256, 37 * 37).astype(np.uint8)
                bits = window[good[0]] < window[good[1]]
                if all(((window[w[0]] < window[w[1]]) != bits).any() for w in wrong):
                    break
            else:
                raise AssertionError("no window tells the deviations of %r" % ((m01, m10, classes),))
            sc.place(slot, axis_patch(m01, m10, sc.rs), window.reshape(37, 37),
                     pin={"moments": (m01, m10), "classes": classes, "what": "steering %r" % (classes,)})
        out.append(sc.freeze())
    return out


def scene_comparison():
    """a constant blurred window (every t0 < t1 false), then windows that differ by +-1 at exactly one rotated pattern point"""
    pattern = ref.load_pattern()
    sc = Scene("comparison", GEO_SMALL, 8, 104)
    slots = [s for s in sc.slots(37)]
    cases = []
    for (m01, m10) in ((0, 0), (37, 37)):
        angle = ref.fast_atan2_f32(F(m01), F(m10))
        cases.append((m01, m10, None, 0, np.zeros(256, bool)))
        for pair, end, delta in ((0, 0, 1), (0, 1, 1), (17, 0, -1), (255, 1, -1), (100, 1, 1), (200, 0, -1)):
            r, c = ref.steer(angle, pattern[pair:pair + 1, 2 * end:2 * end + 2])
            r0, c0 = ref.steer(angle, pattern[:, 0:2])
            r1, c1 = ref.steer(angle, pattern[:, 2:4])
            first, second = (r0[0] == r[0, 0]) & (c0[0] == c[0, 0]), (r1[0] == r[0, 0]) & (c1[0] == c[0, 0])
            bits = (second & ~first) if delta > 0 else (first & ~second)        # t0 < t1 with the point brighter / darker
            cases.append((m01, m10, (int(r[0, 0]), int(c[0, 0])), delta, bits))
    for slot, (m01, m10, at, delta, bits) in zip(slots, cases):
        window = np.full((37, 37), 93, np.uint8)
        if at is not None:
            window[18 + at[0], 18 + at[1]] = 93 + delta
        sc.place(slot, axis_patch(m01, m10, sc.rs), window,
                 pin={"desc": np.packbits(bits.astype(np.uint8), bitorder="little"), "what": "constant window, %+d at %r" % (delta, at)})
    assert len(cases) <= len(slots)
    return sc.freeze()


def _random_keys(sc, b, l, n):
    w, h = sc.sizes[l]
    return [(int(sc.rs.randint(19, w - 19)), int(sc.rs.randint(19, h - 19))) for _ in range(n)]


def scene_bookkeeping(name, counts, seed, rows):
    """counts[frame][level] keys at random places of random images; rows(frame, n) gives the frame's output rows"""
    sc = Scene(name, GEO_SMALL, len(counts), seed, cap=44, guard=5)
    for b, per_level in enumerate(counts):
        order = rows(b, sum(per_level))
        i = 0
        for l, n in enumerate(per_level):
            for (x, y) in _random_keys(sc, b, l, n):
                sc.add(b, l, x, y, row=int(order[i]), pin={"what": "bookkeeping"})
                i += 1
    return sc.freeze()


def _rows_batch3(b, n):
    if b == 0:
        return np.arange(n)[::-1]                                   # reversed
    if b == 1:
        return (np.arange(n) * 5) % 12 + 20                         # scattered (12 keys, 5 is coprime to 12), not from row 0
    r = np.arange(n) + 3
    r[1::3] = -1                                                    # not written ...
    r[2::3] = 44 + np.arange(len(r[2::3])) * 7                      # ... nor these: at cap and beyond (some beyond the whole buffer)
    return r


@functools.lru_cache(maxsize=None)
def all_scenes():
    """every scene, built once; the images are read-only"""
    scenes = [scene_moments(), scene_disc_mask(), scene_alignment(),
              scene_level_edges(GEO_SMALL, "level_edges", 105), scene_level_edges(GEO_TALL, "level_edges_tall", 106),
              scene_comparison(),
              # per-level counts 32 (every slot), 0 between two others, 7 | 1, 9, 2 | 8, 0, 0: odd counts leave the upper half of the
              # last wave dead; three frames of 12 workgroups are not a multiple of the 8 the grid is padded to
              scene_bookkeeping("bookkeeping_batch3", [[32, 0, 7], [1, 9, 2], [8, 0, 0]], 107, _rows_batch3),
              scene_bookkeeping("bookkeeping_batch1", [[9, 1, 2]], 108, lambda b, n: np.arange(n)),
              scene_bookkeeping("bookkeeping_empty", [[0, 0, 0], [0, 2, 0]], 109, lambda b, n: np.arange(n))]
    scenes += scenes_steering()
    return {s.name: s for s in scenes}


# ---- expected outputs ----
def record(t):
    r = np.zeros(1, KP_DTYPE)
    r[0] = t
    return r


@functools.lru_cache(maxsize=None)
def expected(name):
    """what orbx_debug_orient_desc must return for the scene, from the restatement: (kps buffer, desc buffer, lvl[b][l]) exactly as
    Extractor.debug_orient_desc lays them out -- guard rows and unwritten rows hold CANARY bytes, unused level slots 0xFF bytes --
    and per key (frame, level, index, angle, descriptor) for the CPU comparison with the oracle"""
    sc = all_scenes()[name]
    pattern = ref.load_pattern()
    scales = scale_table(sc.geo[2])
    rows = 2 * sc.guard + sc.B * sc.cap
    kps = np.full(rows * KP_DTYPE.itemsize, CANARY, np.uint8).view(KP_DTYPE)
    desc = np.full((rows, 32), CANARY, np.uint8)
    lvl, per_key = [], []
    for b in range(sc.B):
        lvl.append([])
        for l in range(sc.geo[2]):
            slots = np.full(SEL_CAP * KP_DTYPE.itemsize, 0xFF, np.uint8).view(KP_DTYPE)
            for k, (x, y, resp, row) in enumerate(sc.keys[b][l]):
                rec_l, rec_f, d = ref.keypoint_reference(sc.raw[b][l], sc.blur[b][l], x, y, resp, l, scales[l], int(F(31) * scales[l]), pattern)
                slots[k] = rec_l
                if 0 <= row < sc.cap:
                    kps[sc.guard + b * sc.cap + row] = rec_f
                    desc[sc.guard + b * sc.cap + row] = d
                per_key.append((b, l, k, rec_l[3], d))
            lvl[-1].append(slots)
    return kps, desc, lvl, per_key
