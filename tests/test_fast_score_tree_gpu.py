"""The FAST score tree of k_fast_strips, run alone on the device (orbx_debug_fast_scores), against OpenCV's definition restated in
numpy integers:  M = max(0, max_k min_{j<9} d[k+j], max_k min_{j<9} -d[k+j]),  d = centre - ring pixel k  (the corner score is M - 1).
The device computes it as one packed-f16 tree over (d, -d) with bytes read as subnormals; every case asserts equality of every M."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

# the Bresenham ring of radius 3, (dx, dy) of ring pixel k, in cv::FAST's order
RING = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0), (-3, 1), (-2, 2), (-1, 3)]
PITCHES = (16, 16 * 19)         # the smallest tile pitch, and an odd multiple of 16 above the widest strip's (64 quads + margins: 272)


def reference(patches):
    p = patches.astype(np.int32)
    d = np.stack([p[:, 3, 3] - p[:, 3 + dy, 3 + dx] for dx, dy in RING], axis=1)           # (n, 16)
    dd = np.concatenate([d, d[:, :8]], axis=1)
    lo = np.stack([dd[:, k:k + 9].min(axis=1) for k in range(16)], axis=1).max(axis=1)
    hi = np.stack([(-dd[:, k:k + 9]).min(axis=1) for k in range(16)], axis=1).max(axis=1)
    return np.maximum(np.maximum(lo, hi), 0).astype(np.int32)


def device(pkg, patches, pitch):
    patches = np.ascontiguousarray(patches, dtype=np.uint8)
    n = len(patches)
    assert patches.shape == (n, 7, 7)
    out = np.full(n, -1, np.int32)
    assert pkg.lib.orbx_debug_fast_scores(patches.ctypes.data, n, pitch, out.ctypes.data) == 0
    return out


def check(pkg, patches, want=None):
    ref = reference(patches)
    if want is not None:
        assert np.array_equal(ref, want), "the case's closed form disagrees with the definition"
    assert ref.any(), "the expected values are all zero"
    for pitch in PITCHES:
        got = device(pkg, patches, pitch)
        bad = np.flatnonzero(got != ref)
        assert bad.size == 0, "pitch %d: %d of %d differ, first at %d: got %d, want %d\n%s" % (
            pitch, bad.size, len(ref), bad[0], got[bad[0]], ref[bad[0]], patches[bad[0]])


def ring_patches(centre, ring, rng=None):
    """patches with the given centre (n,) and ring (n, 16); every other pixel random (the tree must not read them)"""
    n = len(centre)
    p = (rng.integers(0, 256, (n, 7, 7)) if rng is not None else np.zeros((n, 7, 7))).astype(np.uint8)
    p[:, 3, 3] = centre
    for k, (dx, dy) in enumerate(RING):
        p[:, 3 + dy, 3 + dx] = ring[:, k]
    return p


def test_uniform_ring_every_pair(pkg):
    """all 65 536 (centre, ring value) pairs: M = |v - r| -- every difference, +-1, +-255 and 0 included"""
    v, r = [a.ravel() for a in np.meshgrid(np.arange(256), np.arange(256), indexing="ij")]
    patches = ring_patches(v, np.repeat(r[:, None], 16, axis=1), np.random.default_rng(1))
    assert len(patches) == 65536
    check(pkg, patches, np.abs(v - r).astype(np.int32))


def test_arc_boundaries(pkg):
    """16 rotations x 2 polarities x arc lengths 8, 9, 10, 16 x 7 centres x 5 margins x (rest neutral | rest on the opposite side)"""
    cen, rings, want = [], [], []
    for c in (0, 1, 20, 128, 235, 254, 255):
        for sign in (+1, -1):           # ring = centre + sign * margin on the arc
            room = 255 - c if sign > 0 else c
            for margin in sorted({1, 2, 20, 21, room}):
                if margin < 1 or margin > room:
                    continue
                for length in (8, 9, 10, 16):
                    for rot in range(16):
                        arc = [(rot + j) % 16 for j in range(length)]
                        # the rest at the centre: an arc of 8 is no corner, an arc of 9 or more scores the margin
                        ring = np.full(16, c)
                        ring[arc] = c + sign * margin
                        cen.append(c); rings.append(ring); want.append(margin if length >= 9 else 0)
                        # the rest on the opposite side, as far as it goes (the complement has 16 - length pixels: a corner of the
                        # opposite polarity where that is 9 or more, i.e. never here; an arc of 8 leaves 8)
                        opp = min(margin, c if sign > 0 else 255 - c)
                        ring = np.full(16, c - sign * opp)
                        ring[arc] = c + sign * margin
                        cen.append(c); rings.append(ring); want.append(margin if length >= 9 else 0)
    cen, rings, want = np.array(cen), np.array(rings), np.array(want, np.int32)
    check(pkg, ring_patches(cen, rings), want)


@pytest.mark.parametrize("kind", ["uniform", "low_contrast", "two_valued"])
def test_random_patches(pkg, kind):
    """200 000 seeded random patches of each kind"""
    n = 200000
    rng = np.random.default_rng({"uniform": 11, "low_contrast": 12, "two_valued": 13}[kind])
    if kind == "uniform":
        p = rng.integers(0, 256, (n, 7, 7))
    elif kind == "low_contrast":
        c = rng.integers(3, 253, (n, 1, 1))
        p = c + rng.integers(-3, 4, (n, 7, 7))
        p[:, 3, 3] = c[:, 0, 0]
    else:
        p = 255 * rng.integers(0, 2, (n, 7, 7))
    check(pkg, p.astype(np.uint8))


def test_small_counts(pkg):
    """n no multiple of 64, in one workgroup and in several: lanes past the end stay idle"""
    rng = np.random.default_rng(21)
    for n in (1, 63, 65, 1000):
        p = (255 * rng.integers(0, 2, (n, 7, 7))).astype(np.uint8)
        p[:, 3, 3] = 0
        p[0, :, :] = 255; p[0, 3, 3] = 0          # a full bright ring: the expected values are not all zero
        check(pkg, p)
