#!/usr/bin/env python3
"""Searches the angles IC_Angle can produce from small integer moments for those at which ONE deviation in the steering of the BRIEF
pattern changes a rounded coordinate, and writes a selection to tests/golden/orient_desc_steering_pairs.json.

Every pair of integer moments |m01|, |m10| <= LIMIT gives an angle (cv::fastAtan2 in float32); for every distinct angle the 512
pattern points are rotated as computeOrbDescriptor does (tests/orient_desc_reference.py: steer) and rounded, once as defined and once
per deviation:

  half_up   floor(v + 0.5f) instead of round-half-to-even     fma     a product of x*b + y*a / x*a - y*b fused into the sum
  cos+ cos- the float32 cosine one ulp up / down              sin+ sin-   the sine likewise
  angle     the angle in degrees one ulp up or down

An angle belongs to a class when the deviation moves at least one of its 1 024 rounded coordinates.  A deviation moves a value by a
few float32 ulps at most (the angle's ulp, 3e-5 degrees at 360, times the pattern radius is 1e-5), so only angles with a coordinate
within 2^-14 of k + 0.5 are put through the variants.  CPU only, numpy only; about a minute.

    python tools/find_steering_ties.py            # prints the class counts, rewrites the fixture
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import orient_desc_reference as ref  # noqa: E402

LIMIT = 600
CLASSES = ("half_up", "fma", "cos+", "cos-", "sin+", "sin-", "angle")
VARIANTS_OF = {"half_up": ("half_up",), "fma": ("fma", "fma_other"), "cos+": ("cos+",), "cos-": ("cos-",), "sin+": ("sin+",), "sin-": ("sin-",),
               "angle": ("angle+", "angle-")}
KEEP = {"half_up": 10 ** 6, "fma": 10 ** 6, "cos+": 10 ** 6, "cos-": 10 ** 6, "sin+": 10 ** 6, "sin-": 10 ** 6, "angle": 120}
OUT = os.path.join(ROOT, "tests", "golden", "orient_desc_steering_pairs.json")


def pattern_points():
    p = ref.load_pattern()
    return np.unique(np.concatenate([p[:, 0:2], p[:, 2:4]]), axis=0)


def classes_of(angles, points):
    """{class: bool array over angles}: the deviation changes a rounded coordinate of some pattern point"""
    r0, c0 = ref.steer(angles, points)
    out = {}
    for cls in CLASSES:
        hit = np.zeros(len(angles), bool)
        for v in VARIANTS_OF[cls]:
            r, c = ref.steer(angles, points, v)
            hit |= ((r != r0) | (c != c0)).any(1)
        out[cls] = hit
    return out


def main():
    m = np.arange(-LIMIT, LIMIT + 1, dtype=np.int32)
    m01, m10 = [g.ravel() for g in np.meshgrid(m, m, indexing="ij")]
    ang = ref.fast_atan2_f32_array(m01.astype(np.float32), m10.astype(np.float32))
    # one pair per distinct angle: the one with the smallest moments
    order = np.lexsort((m10, m01, np.abs(m01) + np.abs(m10)))
    uniq, first = np.unique(ang[order], return_index=True)
    rep = order[first]
    print("%d moment pairs, %d distinct angles" % (len(ang), len(uniq)))
    points = pattern_points()
    factor_pi = np.float32(np.pi / np.float32(180.0))
    near = np.zeros(len(uniq), bool)
    ties = np.zeros(len(uniq), bool)
    n_tie_coords = set()
    x, y = points[None, :, 0].astype(np.float32), points[None, :, 1].astype(np.float32)
    for i in range(0, len(uniq), 8192):
        a_rad = uniq[i:i + 8192] * factor_pi
        a = np.cos(a_rad.astype(np.float64)).astype(np.float32)[:, None]
        b = np.sin(a_rad.astype(np.float64)).astype(np.float32)[:, None]
        for v in (x * b + y * a, x * a - y * b):
            d = np.abs(v - np.floor(v) - np.float32(0.5))
            near[i:i + 8192] |= (d < 2.0 ** -14).any(1)
            ties[i:i + 8192] |= (d == 0).any(1)
            n_tie_coords.update(np.unique(v[d == 0]).tolist())
    print("angles with a coordinate exactly k + 0.5: %d (%d distinct coordinates); within 2^-14 of one: %d" % (ties.sum(), len(n_tie_coords), near.sum()))
    idx = np.nonzero(near)[0]
    member = {c: np.zeros(len(idx), bool) for c in CLASSES}
    for i in range(0, len(idx), 4096):
        part = classes_of(uniq[idx[i:i + 4096]], points)
        for c in CLASSES:
            member[c][i:i + 4096] = part[c]
    counts = {c: int(member[c].sum()) for c in CLASSES}
    for c in CLASSES:
        print("class %-8s %5d angles" % (c, counts[c]))
    chosen = np.zeros(len(idx), bool)
    for c in CLASSES:
        hits = np.nonzero(member[c])[0]
        if len(hits) > KEEP[c]:
            hits = hits[np.linspace(0, len(hits) - 1, KEEP[c]).round().astype(int)]
        chosen[hits] = True
    pairs = []
    for j in np.nonzero(chosen)[0]:
        k = rep[idx[j]]
        pairs.append([int(m01[k]), int(m10[k]), [c for c in CLASSES if member[c][j]]])
    doc = {"limit": LIMIT, "distinct_angles": int(len(uniq)), "class_counts_of_the_search": counts, "pairs": pairs}
    with open(OUT, "w") as f:
        f.write(json.dumps(doc, separators=(",", ":")).replace("],[", "],\n[") + "\n")
    print("wrote %d pairs to %s (%d bytes)" % (len(pairs), os.path.relpath(OUT, ROOT), os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
