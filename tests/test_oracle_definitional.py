"""Definitional cross-checks of the CPU ORACLE's feature stages on textured images (CPU only, no GPU).

The reference ships no fixture for cv::FAST / IC_Angle / computeOrbDescriptor (PARITY UNPINNED), and the
hand-made images of test_oracle_kat.py exercise a handful of pixels.  Here every pixel of textured 160x120 synthetic frames
goes through restatements written from the DEFINITIONS, sharing no code and no evaluation order with oracle/*.cpp:

  * FAST-9/16 (OpenCV features2d fast.cpp / fast_score.cpp): a pixel is a corner at threshold t iff
    some contiguous arc of >= 9 of its 16 ring pixels is entirely brighter than v + t or entirely darker than v - t; its
    score is the LARGEST t at which it is still a corner = max over the sixteen 9-arcs of the arc's minimum contrast, minus
    one; 3x3 non-maximum suppression keeps strictly greater scores, non-corners and the 3-pixel border count as 0; row-major
    emission.  (cornerScore's pairwise min/max ladder in the oracle is an optimisation of exactly this.)
  * IC_Angle (reference src/ORBextractor.cc:76-103): integer moments over the radius-15 disc given by umax, then
    cv::fastAtan2 (appendix A.4) in float32 without FMA, restated with numpy float32 scalars.
  * computeOrbDescriptor (:107-146): 256 comparisons of the blurred level at cvRound-ed rotated pattern points, float32
    products and sums without FMA, (float)cos / sin of the float angle.
"""
import numpy as np
import pytest

# the FAST restatement is shared with the tests of the device kernel's cells, tests/fast_cells_reference.py
from fast_cells_reference import RING, fast_definitional  # noqa: E402,F401


@pytest.mark.parametrize("seed,t", [(0, 20), (1, 20), (2, 7), (3, 7), (4, 12), (5, 40)])
def test_fast_against_the_definition(oracle, synth, seed, t):
    from oracle_api import KP_DTYPE
    img = np.ascontiguousarray(synth.make_frame(300 + seed, 160, 120))
    out = np.zeros(20000, KP_DTYPE)
    n = oracle.lib.orb_oracle_fast(img.ctypes.data, 160, 120, 160, t, 1, out.ctypes.data, 20000)
    got = [(int(k["x"]), int(k["y"]), int(k["response"])) for k in out[:n]]
    ref = fast_definitional(img, t)
    assert len(ref) > 50, "the image should have corners at this threshold"
    assert got == ref
    # without suppression (cv::FAST(..., false) reports response 0): the corners at t are the pixels whose definitional score
    # is >= t, row-major -- i.e. the score does not depend on the threshold it was computed at
    smap = fast_definitional(img, 0, want_map=True)
    for th in (t, t + 9):
        n_all = oracle.lib.orb_oracle_fast(img.ctypes.data, 160, 120, 160, th, 0, out.ctypes.data, 20000)
        ys, xs = np.nonzero(smap >= th)
        keep = (smap[ys, xs] > 0) | (th == 0)
        assert [(int(k["x"]), int(k["y"])) for k in out[:n_all]] == list(zip(xs[keep].tolist(), ys[keep].tolist()))


def test_fast_on_a_sub_image_with_stride(oracle, synth):
    """the extractor calls FAST on cell sub-images of a level (stride = level width): same corners as a cropped copy"""
    from oracle_api import KP_DTYPE
    img = np.ascontiguousarray(synth.make_frame(310, 160, 120))
    out = np.zeros(5000, KP_DTYPE)
    x0, y0, cw, ch = 16, 16, 41, 41
    n = oracle.lib.orb_oracle_fast(img.ctypes.data + y0 * 160 + x0, cw, ch, 160, 7, 1, out.ctypes.data, 5000)
    got = [(int(k["x"]), int(k["y"]), int(k["response"])) for k in out[:n]]
    assert got == fast_definitional(img[y0:y0 + ch, x0:x0 + cw], 7) and len(got) > 3


# ---- float32 restatements (numpy float32 scalars: every operation rounds to float32, nothing is contracted): shared with the
# tests of the device kernel, tests/orient_desc_reference.py ----
from orient_desc_reference import F, cv_round, descriptor_definitional, fast_atan2_f32, ic_angle_definitional, load_pattern  # noqa: E402,F401


def test_fast_atan2_restatement_matches_the_oracle(oracle):
    rs = np.random.RandomState(3)
    pts = [(0.0, 0.0), (0.0, 1.0), (1.0, 0.0), (-1.0, 0.0), (0.0, -1.0), (1.0, 1.0), (-1.0, -1.0), (3.0, -3.0)]
    pts += [(float(F(a)), float(F(b))) for a, b in rs.uniform(-1e5, 1e5, (3000, 2))]
    pts += [(float(a), float(b)) for a, b in rs.randint(-40000, 40000, (3000, 2))]
    oracle.lib.orb_oracle_fast_atan2.restype = __import__("ctypes").c_float
    for y, x in pts:
        assert F(oracle.lib.orb_oracle_fast_atan2(__import__("ctypes").c_float(y), __import__("ctypes").c_float(x))) == fast_atan2_f32(F(y), F(x)), (y, x)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_orientation_and_descriptors_against_the_definition(oracle, synth, seed):
    """every key point of a textured 160x120 frame: angle from the integer moments of the UNBLURRED level, descriptor bits from
    the blurred level, both restated above; the oracle's output order for a mono frame is the reversed level-major order"""
    img = synth.make_frame(320 + seed, 160, 120)
    ex = oracle.extractor(300, 1.2, 4, 20, 7)
    r, kps, desc = ex.extract(img, (0, 1000))
    assert r == 0 and len(kps) > 150
    pattern = load_pattern()
    j = 0
    n = len(kps)
    for level in range(4):
        lk = ex.level_keypoints(level)
        if len(lk) == 0:
            continue
        raw, blur = ex.level_image(level), ex.level_blurred(level)
        for k in lk:
            ang = ic_angle_definitional(raw, k["x"], k["y"])
            assert F(k["angle"]) == ang, (level, k)
            d = descriptor_definitional(blur, k["x"], k["y"], k["angle"], pattern)
            np.testing.assert_array_equal(desc[n - 1 - j], d, err_msg="level %d key point %r" % (level, k))
            assert kps[n - 1 - j]["angle"] == k["angle"] and kps[n - 1 - j]["octave"] == level
            j += 1
    assert j == n
