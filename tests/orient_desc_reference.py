"""IC_Angle and the steered BRIEF-256 descriptor restated from their DEFINITIONS in numpy float32, sharing no code and no evaluation
order with oracle/*.cpp or the HIP kernel.  One reference for tests/test_oracle_definitional.py (the oracle on textured frames),
tests/test_orient_desc_reference.py (restatement == oracle on the hand-built cases of orient_desc_cases.py) and
tests/test_orient_desc_boundaries_gpu.py (the kernel on the same cases), and for tools/find_steering_ties.py.

  * IC_Angle (reference src/ORBextractor.cc:76-103): integer moments over the radius-15 disc given by umax, then cv::fastAtan2
     in float32 without FMA.
  * computeOrbDescriptor (:107-146): 256 comparisons of the blurred level at cvRound-ed rotated pattern points, float32 products and
    sums without FMA, (float)cos / sin of the float angle.

Every float32 operation below is one numpy operation on float32 operands: it rounds once, and nothing is contracted.  The steering
also exists in deliberately WRONG variants (`steer(..., variant=...)`): the single deviations a rewrite of the kernel is likely to
make.  They classify the angles of tests/golden/orient_desc_steering_pairs.json and prove that a case can tell the deviation.
"""
import math
import os
import re

import numpy as np

F = np.float32
UMAX = [15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3]          # SURVEY.md 8 table (src/ORBextractor.cc:452-468)


def fast_atan2_f32(y, x):
    """cv::fastAtan2, degrees"""
    s = F(57.29577951308232)            # (float)(180 / pi)
    p1, p3, p5, p7 = F(0.9997878412794807) * s, F(-0.3258083974640975) * s, F(0.1555786518463281) * s, F(-0.04432655554792128) * s
    eps = F(2.220446049250313e-16)      # (float)DBL_EPSILON
    ax, ay = F(abs(x)), F(abs(y))
    if ax >= ay:
        c = ay / (ax + eps)
        c2 = c * c
        a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    else:
        c = ax / (ay + eps)
        c2 = c * c
        a = F(90.0) - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    if x < 0:
        a = F(180.0) - a
    if y < 0:
        a = F(360.0) - a
    return F(a)


def fast_atan2_f32_array(y, x):
    """fast_atan2_f32 over float32 arrays (the same operations, element by element)"""
    y, x = np.asarray(y, F), np.asarray(x, F)
    s = F(57.29577951308232)
    p1, p3, p5, p7 = F(0.9997878412794807) * s, F(-0.3258083974640975) * s, F(0.1555786518463281) * s, F(-0.04432655554792128) * s
    eps = F(2.220446049250313e-16)
    ax, ay = np.abs(x), np.abs(y)
    first = ax >= ay
    num, den = np.where(first, ay, ax), np.where(first, ax, ay) + eps
    c = num / den
    c2 = c * c
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c
    a = np.where(first, a, F(90.0) - a)
    a = np.where(x < 0, F(180.0) - a, a)
    a = np.where(y < 0, F(360.0) - a, a)
    assert a.dtype == F
    return a


def cv_round(v):
    """cvRound: round half to even"""
    return int(np.rint(np.float64(v)))


def moments_definitional(img, x, y):
    """(m01, m10) of the radius-15 disc around the key point, exact integers"""
    cx, cy = cv_round(x), cv_round(y)
    m01 = m10 = 0
    for v in range(-15, 16):
        d = UMAX[abs(v)]
        rowv = img[cy + v, cx - d:cx + d + 1].astype(np.int64)
        m10 += int((np.arange(-d, d + 1) * rowv).sum())
        m01 += v * int(rowv.sum())
    return m01, m10


def ic_angle_definitional(img, x, y):
    m01, m10 = moments_definitional(img, x, y)
    return fast_atan2_f32(F(m01), F(m10))


def load_pattern():
    txt = open(os.path.join(os.path.dirname(__file__), "..", "oracle", "orb_pattern_31.inc")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    vals = [int(t) for t in re.findall(r"-?\d+", txt)]
    assert len(vals) == 1024
    return np.array(vals, np.int32).reshape(256, 4)


def descriptor_definitional(blur, x, y, angle_deg, pattern):
    factor_pi = F(math.pi / F(180.0))               # (float)(CV_PI / 180.f)
    ang = F(angle_deg) * factor_pi
    a, b = F(math.cos(float(ang))), F(math.sin(float(ang)))
    cx, cy = cv_round(x), cv_round(y)

    def value(px, py):
        px, py = F(px), F(py)
        return int(blur[cy + cv_round(px * b + py * a), cx + cv_round(px * a - py * b)])
    bits = np.zeros(256, np.uint8)
    for i, (x0, y0, x1, y1) in enumerate(pattern):
        bits[i] = value(x0, y0) < value(x1, y1)
    return np.packbits(bits, bitorder="little")


# ---- the steering over arrays of angles, and its wrong variants ----
VARIANTS = ("exact", "half_up", "fma", "fma_other", "cos+", "cos-", "sin+", "sin-", "angle+", "angle-")


def _fma_f32(p, q, r):
    """float32 fma(p, q, r) for float32 arrays with |p| a small integer: p * q is exact in float64 and so is its sum with r
    unless q and r differ by more than 2^25 in magnitude, where the single rounding to float32 below is still the right one but for a
    double rounding at a float32 tie of the float64 sum (ignored)"""
    return (p.astype(np.float64) * q.astype(np.float64) + r.astype(np.float64)).astype(F)


def steer(angle_deg, points, variant="exact"):
    """(rows, cols) int32 arrays [n_angles, n_points]: the cvRound-ed rotated pattern points (points: [n, 2] integers x, y) for
    float32 angles in degrees, as computeOrbDescriptor computes them -- or with ONE deviation:
      half_up    floor(v + 0.5f) instead of half-to-even          fma / fma_other   one product of each sum fused into the add
      cos+ cos-  the cosine one float32 ulp up / down             sin+ sin-         the sine likewise
      angle+ angle-  the angle in degrees one ulp up / down"""
    assert variant in VARIANTS
    ang_deg = np.atleast_1d(np.asarray(angle_deg, F))
    if variant == "angle+":
        ang_deg = np.nextafter(ang_deg, F(np.inf))
    elif variant == "angle-":
        ang_deg = np.nextafter(ang_deg, F(-np.inf))
    factor_pi = F(math.pi / F(180.0))
    ang = ang_deg * factor_pi
    a, b = np.cos(ang.astype(np.float64)).astype(F), np.sin(ang.astype(np.float64)).astype(F)
    if variant[:3] == "cos":
        a = np.nextafter(a, F(np.inf) if variant[3] == "+" else F(-np.inf))
    if variant[:3] == "sin":
        b = np.nextafter(b, F(np.inf) if variant[3] == "+" else F(-np.inf))
    a, b = a[:, None], b[:, None]
    pts = np.asarray(points)
    x, y = pts[None, :, 0].astype(F), pts[None, :, 1].astype(F)
    if variant == "fma":                # fma(x, b, y * a), fma(x, a, -(y * b))
        vr, vc = _fma_f32(x, b, y * a), _fma_f32(x, a, -(y * b))
    elif variant == "fma_other":        # fma(y, a, x * b), fma(-y, b, x * a)
        vr, vc = _fma_f32(y, a, x * b), _fma_f32(-y, b, x * a)
    else:
        vr, vc = x * b + y * a, x * a - y * b
    assert vr.dtype == F and vc.dtype == F
    if variant == "half_up":
        return np.floor(vr + F(0.5)).astype(np.int32), np.floor(vc + F(0.5)).astype(np.int32)
    return np.rint(vr).astype(np.int32), np.rint(vc).astype(np.int32)


def cos_sin_f32(angle_deg):
    """the float32 cosine and sine computeOrbDescriptor steers with, scalars"""
    ang = F(angle_deg) * F(math.pi / F(180.0))
    return F(math.cos(float(ang))), F(math.sin(float(ang)))


def descriptor_array(blur, x, y, angle_deg, pattern, variant="exact"):
    """descriptor_definitional through steer(): one key point, all 256 pairs at once; `variant` as in steer()"""
    r0, c0 = steer(angle_deg, pattern[:, 0:2], variant)
    r1, c1 = steer(angle_deg, pattern[:, 2:4], variant)
    cx, cy = cv_round(x), cv_round(y)
    bits = blur[cy + r0[0], cx + c0[0]] < blur[cy + r1[0], cx + c1[0]]
    return np.packbits(bits.astype(np.uint8), bitorder="little")


def keypoint_reference(raw, blur, x, y, response, level, scale_l, patch_size, pattern):
    """what the kernel must write for one key of level coordinates (x, y): (level record, final record, descriptor) with the
    records as tuples (x, y, size, angle, response, octave, class_id) of float32 / int values (:880-895, :1149-1151)"""
    angle = ic_angle_definitional(raw, x, y)
    desc = descriptor_array(blur, x, y, angle, pattern)
    lvl = (F(x), F(y), F(patch_size), angle, F(response), int(level), -1)
    fin = lvl if level == 0 else (F(x) * F(scale_l), F(y) * F(scale_l)) + lvl[2:]
    return lvl, fin, desc
