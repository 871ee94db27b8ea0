"""Hand-built calls of Frame::ComputeStereoMatches (reference src/Frame.cc:931-1101), each left key point with the outcome it is built
to produce.  A test helper, not a test: tests/test_stereo_reference.py runs the cases through the restatement and the C++ oracle,
tests/test_stereo_boundaries_gpu.py through the two device entries.

The key points and descriptors are made by hand; the extractors only hold the pyramids.  Three image pairs ("sheets") of 320 x 240
are shared by all cases, and every geometry extracts all three in one batch, so sheet i is frame i of the batch:

* S0, S1: independent noise in both images with "sites" stamped in.  A site is an all-zero 11 x 11 patch in the left image at
  (ul, vl) and a 21 x 11 strip in the right image around (ur, vl).  With an all-zero left patch the SAD at shift s - 5 is the sum of
  strip columns s .. s + 10, so a wanted profile d[0..10] fixes column[s + 11] - column[s] = d[s + 1] - d[s] (strip_columns()).  At
  level 0 the pyramid is the image itself, so the eleven SADs of a site are exactly the profile it was given.
* TEX: a blocky texture; the right image is the left one moved by TEX_D columns, with a little noise.  Upper pyramid levels come out of the extractor's
  resize, so there the restatement says what happens; the stated codes of those probes were read off it once and are pinned here.

The median cut couples all matches of a call.  The calls that are not about the cut keep their best SADs within 100 .. 190 (a
single match of SAD 0 would be cut: thDist = 2.1f * 0, and 0 < 0 is false).

The |deltaR| > 1 gate (:1065) cannot fire: bestincR is a strict first minimum that is not at an end, so d1 > d2 and d3 >= d2, which
puts deltaR = (d1 - d3) / (2 (d1 + d3 - 2 d2)) into (-0.5, 0.5].  No case hunts for it; `parabola` pins the closed end 0.5.

`disparity = 0.01; bestuR = uL - 0.01` with float literals instead of the double ones gives the same two floats for every uL in
[0.125, 1024) (all of them tried), and an accepted match has uL >= 10 at the least (ten columns to the left of scaleduR0 must exist
on the level).  So that rewriting cannot be seen by any case; the clamp's values are still pinned by `final_gate`.

On import (CPU only) this module checks: every outcome code comes from at least two cases; every stated code equals the
restatement's; the per-probe expectations (winning right index, shift, deltaR, ...); that another rounding than round() changes
the rounding probes; that the median one rank lower or higher changes the result of every median case that has such a rank."""
import collections
import functools
import zlib

import numpy as np

import stereo_reference as ref
from fisheye_stereo_cases import flip_bits
from oracle_api import KP_DTYPE, Oracle
from stereo_reference import (ACCEPTED, ACCEPTED_CLAMPED, BEST_SHIFT_AT_END, CUT_BY_MEDIAN, DISPARITY_OUT_OF_RANGE, NO_CANDIDATE, OFF_LEVEL,
                              ORB_DISTANCE, WINDOW_PAST_RIGHT_EDGE, F)

W, H = 320, 240
GEOMS = {"g8": (500, 1.2, 8, 20, 7), "g2": (500, 2.0, 2, 20, 7), "g1": (500, 1.2, 1, 20, 7)}
MB, MBF = 0.2, 4.0                      # maxD = 20 unless a case says otherwise: the neighbouring cells lie outside the window
TEX_D = 6
CMAX = 11 * 255                         # the largest sum of one strip column
Site = collections.namedtuple("Site", "ul vl ur")


def strip_columns(d):
    """21 column sums in 0..CMAX whose sliding sums of 11 are d[0..10]"""
    d = [int(v) for v in d]
    assert len(d) == 11 and min(d) >= 0
    dl = [d[s + 1] - d[s] for s in range(10)]
    lo = [max(0, -x) for x in dl] + [0]
    hi = [min(CMAX, CMAX - x) for x in dl] + [CMAX]
    rest = d[0] - sum(lo)
    assert rest >= 0, "profile not reachable with an all-zero left patch"
    c = lo[:]
    while rest > 0:                     # spread what is left evenly
        room = [s for s in range(11) if c[s] < hi[s]]
        assert room, "profile not reachable with an all-zero left patch"
        share = max(rest // len(room), 1)
        for s in room:
            t = min(share, hi[s] - c[s], rest)
            c[s] += t; rest -= t
    c += [c[s] + dl[s] for s in range(10)]
    assert all(0 <= v <= CMAX for v in c) and [sum(c[s:s + 11]) for s in range(11)] == d
    return c


def vee(m, shift=0, slope=40):
    """a profile with its only minimum m at `shift`, symmetric about it where both sides exist"""
    return [m + slope * abs(s - 5 - shift) for s in range(11)]


class Sheet:
    """one image pair; sites are stamped until the first request for its pyramid freezes it"""

    def __init__(self, index, seed, textured=False):
        rs = np.random.RandomState(seed)
        self.index, self.frozen, self.next = index, False, 0
        if textured:
            t = np.zeros((H, W))
            for b, amp in ((4, 1.0), (12, 1.5), (40, 2.0)):
                t += amp * np.kron(rs.rand(H // b + 1, W // b + 1), np.ones((b, b)))[:H, :W]
            self.left = np.round(255 * (t - t.min()) / (t.max() - t.min())).astype(np.uint8)
            self.right = rs.randint(0, 256, (H, W)).astype(np.uint8)
            moved = self.left[:, TEX_D:].astype(np.int32) + rs.randint(-3, 4, (H, W - TEX_D))      # a little noise: no SAD of 0, which the cut drops
            self.right[:, :W - TEX_D] = np.clip(moved, 0, 255)
            self.frozen = True
        else:
            self.left = rs.randint(0, 256, (H, W)).astype(np.uint8)
            self.right = rs.randint(0, 256, (H, W)).astype(np.uint8)
        self.used_l = np.zeros((H, W), bool); self.used_r = np.zeros((H, W), bool)

    def site_at(self, ul, vl, ur, d):
        assert not self.frozen, "the sheet's pyramid was already taken"
        ys, xl, xr = slice(vl - 5, vl + 6), slice(ul - 5, ul + 6), slice(ur - 10, ur + 11)
        assert vl - 5 >= 0 and vl + 6 <= H and ul - 5 >= 0 and ul + 6 <= W and ur - 10 >= 0 and ur + 11 <= W
        assert not self.used_l[ys, xl].any() and not self.used_r[ys, xr].any(), "sites overlap"
        self.used_l[ys, xl] = True; self.used_r[ys, xr] = True
        self.left[ys, xl] = 0
        for j, c in enumerate(strip_columns(d)):
            q, r = divmod(c, 11)
            self.right[ys, ur - 10 + j] = [q + (i < r) for i in range(11)]
        return Site(ul, vl, ur)

    def site(self, d, D=8, dx=0, dy=0):
        """the next free cell of a 9 x 19 grid, moved by dx, dy (0 or 1); the left patch lies D columns to the right of the strip's centre"""
        k = self.next; self.next += 1
        assert k < 9 * 19 and 0 <= D <= 16 and dx in (0, 1) and dy in (0, 1)
        ur, vl = 16 + 32 * (k % 9) + dx, 10 + 12 * (k // 9) + dy
        return self.site_at(ur + D, vl, ur, d)


S0, S1, TEX = Sheet(0, 101), Sheet(1, 102), Sheet(2, 103, textured=True)
SHEETS = (S0, S1, TEX)


@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle()


@functools.lru_cache(maxsize=None)
def oracle_extractors(geom, sheet):
    """the two oracle extractors holding the pyramids of sheet `sheet` (an index) in geometry `geom`"""
    sh = SHEETS[sheet]
    sh.frozen = True
    exs = []
    for img in (sh.left, sh.right):
        ex = oracle().extractor(*GEOMS[geom])
        ex.extract(img, (0, 0))
        exs.append(ex)
    return tuple(exs)


@functools.lru_cache(maxsize=None)
def pyramid(geom, sheet):
    """(levels_l, levels_r) of the oracle extractors: what the restatement works on and what the device must hold as well"""
    exL, exR = oracle_extractors(geom, sheet)
    n = GEOMS[geom][2]
    return [exL.level_image(l) for l in range(n)], [exR.level_image(l) for l in range(n)]


@functools.lru_cache(maxsize=None)
def tables(geom):
    t = oracle_extractors(geom, 2)[0].tables()
    return t["scale"], t["inv_scale"]


def band(y, octave, geom="g8"):
    """(minr, maxr) of a right key point (:951-954)"""
    r = F(F(2.0) * tables(geom)[0][octave])
    return int(np.floor(F(F(y) - r))), int(np.ceil(F(F(y) + r)))


CASES = collections.OrderedDict()


class Call:
    """builder of one case: a call with its right and left key points"""

    def __init__(self, name, sheet, geom="g8", mb=MB, mbf=MBF, off_level=False, topic=None):
        self.name, self.sheet, self.geom, self.mb, self.mbf, self.off_level = name, sheet, geom, mb, mbf, off_level
        self.topic = topic or name
        self.rs = np.random.RandomState(zlib.crc32(name.encode()) & 0x7FFFFFFF)
        self.kr, self.dr, self.kl, self.dl, self.want, self.checks = [], [], [], [], [], []

    def desc(self):
        return self.rs.randint(0, 256, 32).astype(np.uint8)

    def near(self, d, bits):
        return flip_bits(self.rs, d, bits)

    def right(self, x, y, octave=0, desc=None):
        self.kr.append((x, y, octave)); self.dr.append(self.desc() if desc is None else desc)
        return len(self.kr) - 1

    def left(self, x, y, octave, desc, want, **checks):
        self.kl.append((x, y, octave)); self.dl.append(desc); self.want.append(want)
        self.checks.append(checks)
        return len(self.kl) - 1

    def probe(self, site, want, bits=20, octave=0, lx=None, ly=None, rx=None, ry=None, roct=None, **checks):
        """a left key point on the site's patch and a right key point on its strip, `bits` bits apart"""
        d = self.desc()
        ir = self.right(site.ur if rx is None else rx, site.vl if ry is None else ry, octave if roct is None else roct, self.near(d, bits))
        return self.left(site.ul if lx is None else lx, site.vl if ly is None else ly, octave, d, want, **checks), ir

    def tex_probe(self, x, y, octave, want, bits=20, ly=None, rx=None, ry=None, roct=None, **checks):
        """the same on the textured sheet, whose right image is the left one moved by TEX_D"""
        return self.probe(Site(x, y, x - TEX_D), want, bits, octave, ly=ly, rx=rx, ry=ry, roct=roct, **checks)

    def done(self):
        def kps(rows):
            k = np.zeros(len(rows), KP_DTYPE)
            for i, (x, y, o) in enumerate(rows):
                k[i] = (F(x), F(y), F(31.0), F(0.0), F(1.0), o, -1)
            return k
        assert self.name not in CASES
        c = dict(name=self.name, topic=self.topic, geom=self.geom, sheet=self.sheet.index, mb=self.mb, mbf=self.mbf, off_level=self.off_level,
                 kps_l=kps(self.kl), desc_l=np.array(self.dl, np.uint8).reshape(-1, 32), kps_r=kps(self.kr),
                 desc_r=np.array(self.dr, np.uint8).reshape(-1, 32), want=np.array(self.want, np.int8), checks=self.checks)
        assert (c["kps_l"]["x"] >= 0).all() and (c["kps_l"]["y"] >= 0).all() and (c["kps_l"]["y"] < H).all()
        CASES[self.name] = c
        return c


_TEX_GRID = [(x, y) for y in range(40, 201, 20) for x in range(60, 261, 40)]


def tex_xy(k):
    return _TEX_GRID[k]


def plain(k=0):
    """a symmetric profile whose minimum, 100 .. 190, lies at shift 0"""
    return vee(100 + 10 * (k % 10))


# ------------------------------------------------------------------------------------------------ row band (:951-957, :976)
c = Call("row_band_level0", S0, topic="row_band")
for k, (dy, want) in enumerate([(2, ACCEPTED),            # (int)vL == minr: r is exactly 2 at level 0
                                (3, NO_CANDIDATE),        # (int)vL == minr - 1
                                (-2, ACCEPTED),           # (int)vL == maxr
                                (-3, NO_CANDIDATE),       # (int)vL == maxr + 1
                                (2.5, ACCEPTED),          # fractional y: minr = floor(vl + 0.5) = vl
                                (2.9, ACCEPTED),          # floor, not ceil or round
                                (-2.9, ACCEPTED),         # maxr = ceil(vl - 0.9) = vl: ceil, not floor or round
                                (-3.0001, NO_CANDIDATE),
                                (3.0001, NO_CANDIDATE)]):
    s = S0.site(plain(k))
    c.probe(s, want, ry=s.vl + dy)
# a left vL with a fractional part: the row is (int)vL, the window's centre round(vL)
s = S0.site(plain(1)); c.probe(s, ACCEPTED, ly=s.vl - 0.4, ry=s.vl - 3)       # (int)vL = vl - 1 == maxr; round(vL) = vl would be outside
s = S0.site(plain(2)); c.probe(s, ACCEPTED, ly=s.vl - 0.4, ry=s.vl + 1)       # (int)vL = vl - 1 == minr
s = S0.site(plain(3)); c.probe(s, ACCEPTED, ly=s.vl + 0.4, ry=s.vl - 2.5)      # (int)vL = vl == maxr = ceil(vl - 0.5)
s = S0.site(plain(4)); c.probe(s, NO_CANDIDATE, ly=s.vl + 0.4, ry=s.vl - 3)    # (int)vL = vl == maxr + 1
# a better descriptor just outside the band loses to a worse one inside
s = S0.site(plain(5), D=10)
d = c.desc()
c.right(s.ur + 7, s.vl + 3, 0, c.near(d, 5))
inside = c.right(s.ur, s.vl + 2, 0, c.near(d, 40))
c.left(s.ul, s.vl, 0, d, ACCEPTED, best_r=inside)
c.done()

for lvl in (1, 3, 7):
    c = Call("row_band_level%d" % lvl, TEX, topic="row_band")
    for k, which in enumerate(("minr", "minr-1", "maxr", "maxr+1")):
        x, y = tex_xy(k + 4 * (lvl % 3))
        minr, maxr = band(y, lvl)
        vl = {"minr": minr, "minr-1": minr - 1, "maxr": maxr, "maxr+1": maxr + 1}[which]
        c.tex_probe(x, y, lvl, ACCEPTED if which in ("minr", "maxr") else NO_CANDIDATE, ly=vl, ry=y)
    c.done()

# ------------------------------------------------------------------------------------------------ octave window (:998)
for geom, levels in (("g8", (0, 3, 7)), ("g2", (0, 1)), ("g1", (0,))):
    c = Call("octave_window_" + geom, TEX, geom, topic="octave_window")
    k = 0
    for lvl in levels:
        for roct in range(lvl - 2, lvl + 3):
            if 0 <= roct < GEOMS[geom][2]:
                x, y = tex_xy(k); k += 1
                c.tex_probe(x, y, lvl, ACCEPTED if abs(roct - lvl) <= 1 else NO_CANDIDATE, roct=roct)
    c.done()

# a left octave that the pyramid does not have, too far from every right octave to find a candidate: defined in the reference too
c = Call("octave_outside", TEX, topic="octave_window")
for k, lvl in enumerate((-2, 9, 100)):
    x, y = tex_xy(k)
    d = c.desc()
    c.right(x - TEX_D, y, 0, d.copy()); c.right(x - TEX_D, y, 7, d.copy())
    c.left(x, y, lvl, d, NO_CANDIDATE)
c.tex_probe(*tex_xy(4), 0, ACCEPTED)
c.tex_probe(*tex_xy(5), 2, ACCEPTED)
c.done()
# ... and one that finds a candidate at nlevels - 1: there is no level to correlate on (the OFF_LEVEL contract)
c = Call("octave_outside_with_candidate", TEX, off_level=True, topic="octave_window")
c.tex_probe(*tex_xy(0), 8, OFF_LEVEL, roct=7)
c.tex_probe(*tex_xy(1), -1, OFF_LEVEL, roct=0)
c.tex_probe(*tex_xy(4), 0, ACCEPTED)
c.done()

# ------------------------------------------------------------------------------------------------ disparity window (:981-982, :1003)
_mb, _mbf = 0.3, 3.37                   # maxD = 11.2333..., not representable
_maxD = F(F(_mbf) / F(_mb))
assert float(_maxD) != 3.37 / 0.3 and 11 < _maxD < 11.5
c = Call("disparity_window", S0, mb=_mb, mbf=_mbf)
s = S0.site(plain(0), D=11); minU = F(F(s.ul) - _maxD)
c.probe(s, ACCEPTED, rx=minU)                                                   # x == minU
s = S0.site(plain(1), D=11); minU = F(F(s.ul) - _maxD)
c.probe(s, NO_CANDIDATE, rx=np.nextafter(minU, F(-np.inf)))
s = S0.site(plain(2), D=0)
c.probe(s, ACCEPTED_CLAMPED, rx=F(s.ul))                                        # x == uL; the profile refines to disparity 0
s = S0.site(vee(130, -2), D=0)
c.probe(s, ACCEPTED, rx=F(s.ul), shift=-2)                                      # x == uL, refined to disparity 2
s = S0.site(plain(4), D=0)
c.probe(s, NO_CANDIDATE, rx=np.nextafter(F(s.ul), F(np.inf)))
c.done()

# ------------------------------------------------------------------------------------------------ descriptor gate (:987, :1008, :1017)
_gate_sites = [S0.site(plain(k)) for k in range(5)]
for geom in ("g8", "g1"):
    c = Call("descriptor_gate_" + geom, S0, geom, topic="descriptor_gate")
    for s, (bits, want) in zip(_gate_sites, [(74, ACCEPTED), (75, ORB_DISTANCE), (99, ORB_DISTANCE), (100, ORB_DISTANCE), (0, ACCEPTED)]):
        c.probe(s, want, bits=bits)
    c.done()

# ------------------------------------------------------------------------------------------------ first minimum (:1008)
# 8192 right key points; every left key point sees about a seventh of them inside its band and window.  The tied key points carry
# different x, so the winner shows in u_right.  n_r > n_l.
c = Call("first_minimum", S0)
_N_R = 8192
_ties = [("i,i+1", 10, 11, 20), ("i,i+64", 100, 164, 20), ("i,i+65", 200, 265, 20), ("across 1024", 1000, 1030, 20), ("above 1024", 3000, 5000, 20),
         ("low against 8191", 5001, 8191, 20), ("8191 wins", 8191, 7, 10)]
_fm_sites = [S0.site(plain(k), D=10) for k in range(len(_ties))]
for i in range(_N_R):                                                           # fillers: random descriptors inside a probe's band and window
    s = _fm_sites[i % len(_ties)]
    c.right(s.ur + float(c.rs.randint(0, 11)), s.vl, 0)
for k, (what, win, lose, bits) in enumerate(_ties):
    s = _fm_sites[k]
    d = c.desc()
    if what == "8191 wins":                                                     # no tie: the better descriptor has the highest index there is
        c.kr[win] = (s.ur, s.vl, 0); c.dr[win] = c.near(d, 10)
        c.kr[lose] = (s.ur + 8, s.vl, 0); c.dr[lose] = c.near(d, 30)
    else:
        c.kr[win] = (s.ur, s.vl, 0); c.dr[win] = c.near(d, bits)
        c.kr[lose] = (s.ur + 8, s.vl, 0); c.dr[lose] = c.near(d, bits)
    c.left(s.ul, s.vl, 0, d, ACCEPTED, best_r=win)
c.done()

# ------------------------------------------------------------------------------------------------ rounding to the level (:1022-1024)
ROUNDING_CASES = []
c = Call("rounding_level0", S0, topic="rounding")


def _about_half(k):
    """the floats just below k + 0.5, at it and just above it, with the integer that round() makes of each"""
    h = F(k + 0.5)
    return (np.nextafter(h, F(0)), k), (h, k + 1), (np.nextafter(h, F(1e9)), k + 1)


for parity in (0, 1):                                                           # k + 0.5 for even and for odd k
    for j in range(3):
        s = S0.site(plain(j), D=8, dx=parity)                                   # uL
        x, to = _about_half(s.ul - 1)[j] if j else _about_half(s.ul)[j]
        assert to == s.ul == ref.c_round(x)
        c.probe(s, ACCEPTED, lx=x)
    for j in range(3):
        s = S0.site(plain(j + 3), dy=parity)                                    # vL; the row of the table is (int)vL
        y, to = _about_half(s.vl - 1)[j] if j else _about_half(s.vl)[j]
        assert to == s.vl == ref.c_round(y)
        c.probe(s, ACCEPTED, ly=y, ry=s.vl)
    # uR0: a wrong scaleduR0 moves bestincR the other way and the refined uR stays the same, unless the minimum then falls on an end
    for j, shift in enumerate((4, -4, -4)):
        s = S0.site(vee(100 + 10 * j, shift), D=14, dx=parity)
        x, to = _about_half(s.ur - 1)[j] if j else _about_half(s.ur)[j]
        assert to == s.ur == ref.c_round(x)
        c.probe(s, ACCEPTED, rx=x, shift=shift)
ROUNDING_CASES.append(c.done()["name"])


def half_points(inv, k):
    """float32 x with float32(x * inv) just below, exactly at and just above k + 0.5, or None if no x hits it exactly"""
    t = F(k + 0.5)
    x = F(t / inv)
    xs = [x]
    for _ in range(8):
        xs = [np.nextafter(xs[0], F(0))] + xs + [np.nextafter(xs[-1], F(1e9))]
    at = [v for v in xs if F(v * inv) == t]
    if not at:
        return None
    return max(v for v in xs if F(v * inv) < t), at[0], min(v for v in xs if F(v * inv) > t)


c = Call("rounding_level1", TEX, topic="rounding")                             # inv_scale 1 / 1.2f is no power of two
_inv1 = tables("g8")[1][1]
k = 0
for parity in (0, 1):
    for axis in ("uL", "vL", "uR0"):
        x, y = tex_xy(k); k += 1
        base = {"uL": x, "vL": y, "uR0": x - TEX_D + 4.8}[axis]               # (uR0: the true match four level columns away from the centre)
        kk = int(base * float(_inv1))
        kk += (kk - parity) % 2
        hp = None
        while hp is None:
            hp = half_points(_inv1, kk); kk += 2
        for j, v in enumerate(hp):
            if axis == "uL":
                c.tex_probe(x, y, 1, ACCEPTED, rx=x - TEX_D); c.kl[-1] = (v, y, 1)
            elif axis == "vL":
                c.tex_probe(x, y, 1, ACCEPTED, ly=v, ry=float(np.floor(v)))
            else:                                                               # (read off the restatement: rounding up puts the match on the end)
                c.tex_probe(x, y, 1, BEST_SHIFT_AT_END if parity == 0 and j else ACCEPTED, rx=v)
ROUNDING_CASES.append(c.done()["name"])

# ------------------------------------------------------------------------------------------------ window against the right edge (:1036-1039)
c = Call("right_edge_level0", S0, topic="right_edge")
s = S0.site_at(314, 220, 308, plain(3))
c.probe(s, ACCEPTED)                                                            # scaleduR0 + 11 == cols - 1
d = c.desc(); c.right(309, 200, 0, c.near(d, 10)); c.left(314, 200, 0, d, WINDOW_PAST_RIGHT_EDGE)      # scaleduR0 + 11 == cols
c.done()
c = Call("right_edge_level1_of_2", TEX, "g2", topic="right_edge")              # level 1 of scale factor 2 has 160 columns of its own
c.tex_probe(302, 100, 1, ACCEPTED, rx=296)                                      # round(296 / 2) + 11 == 159
c.tex_probe(302, 140, 1, WINDOW_PAST_RIGHT_EDGE, rx=298)                        # round(298 / 2) + 11 == 160
c.done()
# the OFF_LEVEL contract: cv::Mat::rowRange / colRange would assert.  The oracle returns -2 for the whole call; the kernel drops the key
# point and goes on, which the accepted probe next to it shows
for name, (lx, ly, rx) in (("off_level_xr_start", (15, 60, 9)), ("off_level_y0", (100, 4, 95)), ("off_level_y1", (100, 235, 95)),
                           ("off_level_xl1", (315, 60, 300))):
    c = Call(name, S0, off_level=True, topic="right_edge")
    d = c.desc(); c.right(rx, ly, 0, c.near(d, 10)); c.left(lx, ly, 0, d, OFF_LEVEL)
    c.probe(s, ACCEPTED)
    c.done()

# ------------------------------------------------------------------------------------------------ best shift (:1046-1056)
c = Call("best_shift", S0)
_tie_first_end = vee(120, 0, 10); _tie_first_end[0] = 120                              # equal minima at -5 and 0: the first wins, an end
_tie_last_end = vee(130, -2, 10); _tie_last_end[10] = 130; _tie_last_end[9] = 150   # equal minima at -2 and +5: the first wins
for k, (d, want, shift) in enumerate([(vee(110, -5), BEST_SHIFT_AT_END, -5), (vee(110, 5), BEST_SHIFT_AT_END, 5), (vee(140, -4), ACCEPTED, -4),
                                      (vee(150, 4), ACCEPTED, 4), (_tie_first_end, BEST_SHIFT_AT_END, -5), (_tie_last_end, ACCEPTED, -2),
                                      ([1000] * 11, BEST_SHIFT_AT_END, -5)]):
    c.probe(S0.site(d), want, shift=shift)
c.done()

# ------------------------------------------------------------------------------------------------ parabola (:1059-1063)
def _peak(d1, d2, d3, other):
    return [other] * 4 + [d1, d2, d3] + [other] * 4


c = Call("parabola", S0)
_third = S0.site(_peak(150, 100, 110, 400))
for s, delta in ((S0.site(_peak(300, 100, 100, 400)), 0.5),                     # d3 == d2: the closed end of (-0.5, 0.5]
                 (S0.site(_peak(180, 100, 180, 400)), 0.0),
                 (_third, F(F(40) / F(120))),                                   # 1 / 3 and 1 / 7, which float32 must round
                 (S0.site(_peak(190, 100, 150, 400)), F(F(40) / F(280)))):
    c.probe(s, ACCEPTED, shift=0, delta=delta)
c.done()
c = Call("parabola_large", S0, topic="parabola")                                # next to the largest SAD there is, 121 * 255 = 30855
c.probe(S0.site(_peak(30650, 30500, 30640, 30600)), ACCEPTED, shift=0, delta=F(F(10) / F(580)), sad=30500)
c.done()
c = Call("parabola_small", S0, topic="parabola")
c.probe(S0.site(_peak(9, 1, 4, 9)), ACCEPTED, shift=0, delta=F(F(5) / F(22)), sad=1)
c.done()
# the profile that the texture gives at level 3, stamped at level 0 as well: the same deltaR, multiplied by another scale
_x3, _y3 = tex_xy(7)
c = Call("parabola_level3", TEX, topic="parabola")
c.tex_probe(_x3, _y3, 3, ACCEPTED)
_c3 = c.done()
_r3 = ref.stereo_matches(*pyramid("g8", 2), *tables("g8"), _c3["kps_l"], _c3["desc_l"], _c3["kps_r"], _c3["desc_r"], MB, MBF)
assert _r3["code"][0] == ACCEPTED and -5 < _r3["shift"][0] < 5
_c3["checks"][0]["delta"] = _r3["delta"][0]
c = Call("parabola_level3_profile_at_level0", S0, topic="parabola")
c.probe(S0.site([int(v) for v in _r3["dists"][0]]), ACCEPTED, shift=int(_r3["shift"][0]), delta=_r3["delta"][0], sad=int(_r3["sad"][0]))
c.done()

# ------------------------------------------------------------------------------------------------ final disparity gate (:1071-1079)
c = Call("final_gate", S0)
s = S0.site(plain(0), D=0)
c.probe(s, ACCEPTED_CLAMPED, shift=0, delta=0.0, depth=F(F(MBF) / F(0.01)), u_right=F(np.float64(F(s.ul)) - 0.01))   # refined disparity exactly 0
c.probe(S0.site(vee(120, 2), D=0), DISPARITY_OUT_OF_RANGE, shift=2)            # a candidate at x == uL refined to disparity -2
c.probe(S0.site(plain(2), D=1), ACCEPTED, shift=0, u_right=None)
c.done()
_mb, _mbf = 0.25, 2.8125                # maxD == 11.25 exactly
c = Call("final_gate_max", S0, mb=_mb, mbf=_mbf, topic="final_gate")
assert F(F(_mbf) / F(_mb)) == 11.25
c.probe(S0.site(_peak(120, 100, 160, 400), D=11), DISPARITY_OUT_OF_RANGE, shift=0, delta=-0.25)          # disparity == maxD: 11 + 0.25
c.probe(S0.site(_peak(120, 100, 159, 400), D=11), ACCEPTED, shift=0)                                    # just below: 11 + 39 / 158
c.probe(S0.site(vee(110, -1), D=11), DISPARITY_OUT_OF_RANGE, shift=-1)                                  # 12, from a candidate inside the window
c.probe(S0.site(plain(3), D=11), ACCEPTED, shift=0)
c.done()

# ------------------------------------------------------------------------------------------------ median cut (:1087-1100)
X21 = F(F(1.5) * F(1.4))
_LOW, _MID, _HIGH = list(range(0, 101, 10)), [100, 220, 470], list(range(470, 601, 10))
_TH = next((m, int(F(X21 * F(m)))) for m in range(10, 300, 10) if F(X21 * F(m)) == int(F(X21 * F(m))))     # 2.1f * median lands on an integer
_MID_FINE, _HIGH_FINE = [100, 110, 120], [220, 240, 250] + list(range(120, 301, 10))
_ladder = sorted(set(list(range(0, 301, 10)) + _MID + _HIGH + [_TH[1] - 1, _TH[1]]))      # every multiple of 10 up to 300, SAD 0 included
LADDER = {m: S1.site(vee(m, 0, 60)) for m in _ladder}
MEDIAN_SIZES = (1, 2, 3, 4, 5, 7, 8, 9, 16, 17, 255, 256, 257, 1023, 1025, 4097, 8192)
MEDIAN_CASES = []


def _median_call(name, sads, n=None):
    """left key points on the ladder's sites with the best SADs `sads` (in this order), every third one unmatched (a descriptor far from
    its site's) until there are n; one right key point per site, so n_l > n_r for all but the smallest"""
    c = Call(name, S1, topic="median")
    site_desc, site_r = {}, {}
    for m in sorted(set(sads)) or [100]:
        site_desc[m] = c.desc(); site_r[m] = c.right(LADDER[m].ur, LADDER[m].vl, 0, site_desc[m])
    n = len(sads) if n is None else n
    sads = list(sads)
    th = F(X21 * F(sorted(sads)[len(sads) // 2])) if sads else None
    j = 0
    while len(c.kl) < n:
        unmatched = not sads or (len(c.kl) % 3 == 2 and n - len(c.kl) > len(sads))
        m = sads.pop(0) if not unmatched else sorted(site_desc)[j % len(site_desc)]
        j += 1
        s = LADDER[m]
        if unmatched:
            c.left(s.ul, s.vl, 0, c.desc(), ORB_DISTANCE)
        else:
            c.left(s.ul, s.vl, 0, c.near(site_desc[m], int(c.rs.randint(0, 40))), ACCEPTED if F(m) < th else CUT_BY_MEDIAN, sad=m, best_r=site_r[m])
    assert not sads
    return c.done()


def _median_sads(m):
    """m best SADs, sorted, such that a median one rank off changes what is cut.  From ten matches on, the ladder of every multiple of 10:
    the ranks below walk 0 .. 100, the three about the median are 100 | 110 | 120, the ranks above walk 120 .. 300; 2.1f * 100 cuts from
    210, 2.1f * 110 from 240, 2.1f * 120 from 260.  Fewer matches have no room for that and take 100 | 220 | 470 about the median and
    470 .. 600 above: 2.1f * 100 cuts 220, 2.1f * 220 cuts from 470, 2.1f * 470 cuts nothing"""
    r = m // 2
    mid, high = (_MID_FINE, _HIGH_FINE) if m >= 10 else (_MID, _HIGH)
    below = [_LOW[i % len(_LOW)] for i in range(max(r - 1, 0))]
    about = mid[(1 if r == 0 else 0):][:m - len(below)]
    above = [high[i % len(high)] for i in range(m - len(below) - len(about))]
    return sorted(below + about + above)


for n in MEDIAN_SIZES:
    m = n - n // 3
    sads = _median_sads(m)
    assert len(sads) == m
    order = np.random.RandomState(n).permutation(m)
    MEDIAN_CASES.append(_median_call("median_n%d" % n, [sads[i] for i in order], n)["name"])
_median_call("median_at_threshold", [0, 10, _TH[0], _TH[1] - 1, _TH[1]][::-1])  # a SAD equal to thDist goes, the one below stays
_median_call("median_zero", [50, 0, 60, 0, 0])                                  # thDist == 0: every match goes, the perfect ones too
_median_call("median_no_match", [], 5)                                          # m == 0: nothing is read, nothing changes

# ------------------------------------------------------------------------------------------------ entry-point shapes
c = Call("no_right_keypoints", S0, topic="entry")
for k in range(3):
    c.left(_fm_sites[k].ul, _fm_sites[k].vl, 0, c.desc(), NO_CANDIDATE)
c.done()
c = Call("no_left_keypoints", S0, topic="entry")
c.right(100, 100, 0)
c.done()


# ------------------------------------------------------------------------------------------------ the self-checks
@functools.lru_cache(maxsize=None)
def reference(name):
    """the restatement's result for a case; shared by the tests, which must not modify it"""
    c = CASES[name]
    return ref.stereo_matches(*pyramid(c["geom"], c["sheet"]), *tables(c["geom"]), c["kps_l"], c["desc_l"], c["kps_r"], c["desc_r"], c["mb"], c["mbf"])


def _names(code):
    return [ref.OUTCOMES[v] for v in code]


def _self_check():
    produced = collections.defaultdict(set)
    for name, c in CASES.items():
        r = reference(name)
        assert np.array_equal(r["code"], c["want"]), "%s: stated %s, the restatement says %s" % (name, _names(c["want"]), _names(r["code"]))
        for v in c["want"]:
            produced[int(v)].add(name)
        for i, chk in enumerate(c["checks"]):
            for key, want in chk.items():
                if want is not None:
                    got = r["uncut"][key][i] if key == "sad" else r[key][i]
                    assert got == want, "%s, left key point %d: %s is %r, built for %r" % (name, i, key, got, want)
        assert c["off_level"] == bool((c["want"] == OFF_LEVEL).any())
    for code in range(len(ref.OUTCOMES)):
        assert len(produced[code]) >= 2, "outcome %s comes from %d cases" % (ref.OUTCOMES[code], len(produced[code]))
    # the lowest index wins every tie, and the choice shows
    r = reference("first_minimum")
    assert len(set(r["u_right"].tolist())) == len(r["u_right"])
    # another rounding is seen
    for name in ROUNDING_CASES:
        c = CASES[name]
        alt = ref.stereo_matches(*pyramid(c["geom"], c["sheet"]), *tables(c["geom"]), c["kps_l"], c["desc_l"], c["kps_r"], c["desc_r"], c["mb"], c["mbf"],
                                 round_fn=lambda v: F(np.rint(v)))
        assert not np.array_equal(alt["u_right"], reference(name)["u_right"]), "%s: round-half-even gives the same result" % name
    # a median one rank lower or higher is seen
    for name in MEDIAN_CASES:
        r = reference(name)
        m = r["n_matches"]
        for sh in (-1, 1):
            if 0 <= m // 2 + sh < m:
                alt = ref.median_cut(r["uncut"], sh)
                assert not np.array_equal(alt["u_right"], r["u_right"]), "%s: the median at rank %d gives the same result" % (name, m // 2 + sh)
    r = reference("median_at_threshold")
    assert _names(r["code"]) == ["cut_by_median", "accepted", "accepted", "accepted", "accepted"]


TOPICS = collections.OrderedDict()
for _n, _c in CASES.items():
    TOPICS.setdefault(_c["topic"], []).append(_n)
OUTCOME_TABLE = {o: [n for n, c in CASES.items() if (c["want"] == i).any()] for i, o in enumerate(ref.OUTCOMES)}
_self_check()
