"""Synthetic fisheye rigs and scenes for the tests of ComputeStereoFishEyeMatches.  A test helper, not a test.

Everything is seeded and built once per process (functools.lru_cache): the tests share the cases and the reference's results and
must not modify them.

Tolerance of accepted pairs (tests/test_fisheye_stereo_gpu.py): depth and p3d agree with the `faithful` evaluation to
P3D_RTOL * |p3d|.  MEASURED_SPREAD is the largest |p3d_faithful - p3d_exact| / |p3d_exact| over the accepted pairs of every case
in this file (measure_spread(), asserted by tests/test_fisheye_stereo_reference.py); the device differs from `faithful` by
one-ulp transcendentals and by another null-vector algorithm, each of the size of the rounding that the spread measures, so the
tests allow 4 x the spread."""
import functools

import numpy as np

import fisheye_stereo_reference as ref

MEASURED_SPREAD = 6.2e-5        # measure_spread() gives 6.10e-5 (a pair near the parallax limit of the TUM-VI-like rig)
P3D_RTOL = 4 * MEASURED_SPREAD
BORDERLINE_CAP = 0.02           # borderline pairs may be left out of the code comparison, but may not exceed 2 % of any case

N_LEVELS = 8
_scale = [np.float32(1.0)]
for _ in range(N_LEVELS - 1):
    _scale.append(np.float32(_scale[-1] * np.float32(1.2)))
LEVEL_SIGMA2 = np.array([s * s for s in _scale], np.float32)      # mvLevelSigma2 of ORBextractor(.., 1.2, 8, ..)

f32 = lambda v: float(np.float32(v))


def _rot(w):
    w = np.asarray(w, np.float64)
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _cam(fx, fy, cx, cy, k):
    return dict(fx=f32(fx), fy=f32(fy), cx=f32(cx), cy=f32(cy), k=[f32(v) for v in k])


def _rig(left, right, w, t):
    return dict(left=left, right=right, precision_l=f32(1e-6), precision_r=f32(1e-6),
                Rlr=_rot(w).astype(np.float32), tlr=np.asarray(t, np.float32))


RIGS = {
    # a TUM-VI-like pair: 512 x 512, 0.101 m baseline, a relative rotation of a few hundredths of a radian
    "tumvi": _rig(_cam(190.978, 190.973, 254.932, 256.897, (0.0034, 0.0007, -0.0020, 0.0002)),
                  _cam(190.442, 190.434, 252.597, 254.917, (0.0034, 0.0018, -0.0027, 0.0004)), (0.02, -0.035, 0.012), (0.101, 0.0012, -0.0018)),
    # optical axes that diverge by 40 degrees: many points lie behind one camera's image plane for the other's ray
    "diverging": _rig(_cam(190.978, 190.973, 254.932, 256.897, (0.0034, 0.0007, -0.0020, 0.0002)),
                      _cam(190.442, 190.434, 252.597, 254.917, (0.0034, 0.0018, -0.0027, 0.0004)), (0.01, 0.70, -0.02), (0.12, 0.0, 0.01)),
}


def _project64(cam, X):
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    theta = np.arctan2(np.sqrt(x * x + y * y), z)
    psi = np.arctan2(y, x)
    k = cam["k"]
    t2 = theta * theta
    r = theta * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    return np.stack([cam["fx"] * r * np.cos(psi) + cam["cx"], cam["fy"] * r * np.sin(psi) + cam["cy"]], 1)


def _scene(rig, rs, n):
    """n points, log-uniform from 0.3 to 30 m, inside both fields of view; pixels with noise scaled by the level sigma: 70 % at 0.5,
    15 % at 1.5 and 15 % at 4 times it"""
    pts_l, pts_r, oct_l, oct_r = [], [], [], []
    R, t = rig["Rlr"].astype(np.float64), rig["tlr"].astype(np.float64)
    while len(pts_l) < n:
        d = np.exp(rs.uniform(np.log(0.3), np.log(30.0)))
        th, ph = rs.uniform(0, 1.2), rs.uniform(-np.pi, np.pi)
        Pl = d * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
        Pr = R.T @ (Pl - t)
        if np.arctan2(np.hypot(Pr[0], Pr[1]), Pr[2]) > 1.3:
            continue
        ol, orr = rs.randint(0, N_LEVELS), rs.randint(0, N_LEVELS)
        level = rs.choice([0.5, 1.5, 4.0], p=[0.7, 0.15, 0.15])
        ul = _project64(rig["left"], Pl[None])[0] + level * np.sqrt(LEVEL_SIGMA2[ol]) * rs.standard_normal(2)
        ur = _project64(rig["right"], Pr[None])[0] + level * np.sqrt(LEVEL_SIGMA2[orr]) * rs.standard_normal(2)
        pts_l.append(ul); pts_r.append(ur); oct_l.append(ol); oct_r.append(orr)
    return np.array(pts_l, np.float32), np.array(pts_r, np.float32), np.array(oct_l, np.int32), np.array(oct_r, np.int32)


@functools.lru_cache(maxsize=None)
def pair_case(name):
    """pixel pairs for the triangulation diagnostic: dict(rig, pts_l, pts_r, sigma_l, sigma_r).  The `_mismatch` cases pair a
    third of the left pixels with the right pixel of another point."""
    rig_name, seed, n, mismatch = {"tumvi_a": ("tumvi", 11, 700, False), "tumvi_mismatch": ("tumvi", 12, 500, True),
                                   "diverging_a": ("diverging", 13, 500, False), "diverging_mismatch": ("diverging", 14, 500, True)}[name]
    rs = np.random.RandomState(seed)
    rig = RIGS[rig_name]
    pl, pr, ol, orr = _scene(rig, rs, n)
    if mismatch:
        idx = np.arange(0, n, 3)
        pr[idx] = pr[np.roll(idx, 1)]; orr[idx] = orr[np.roll(idx, 1)]
    return dict(rig=rig, pts_l=pl, pts_r=pr, sigma_l=LEVEL_SIGMA2[ol], sigma_r=LEVEL_SIGMA2[orr])


PAIR_CASES = ("tumvi_a", "tumvi_mismatch", "diverging_a", "diverging_mismatch")


@functools.lru_cache(maxsize=None)
def pair_reference(name, mode):
    c = pair_case(name)
    return ref.triangulate_matches(c["rig"], c["pts_l"], c["pts_r"], c["sigma_l"], c["sigma_r"], ref.FAITHFUL if mode == "faithful" else ref.EXACT)


def geometry_references():
    """(case name, faithful, exact) of every committed case: the pair cases and the survivors of the frame cases"""
    for name in PAIR_CASES:
        yield name, pair_reference(name, "faithful"), pair_reference(name, "exact")
    for name in FRAME_CASES:
        yield name, frame_reference(name, "faithful")["geo"], frame_reference(name, "exact")["geo"]


def measure_spread():
    """the largest relative distance between the faithful and the exact point over the pairs both evaluations accept"""
    worst = 0.0
    for _, f, e in geometry_references():
        both = f["accepted"] & e["accepted"]
        if both.any():
            d = np.linalg.norm(f["p3d"][both].astype(np.float64) - e["p3d"][both], axis=1) / np.linalg.norm(e["p3d"][both], axis=1)
            worst = max(worst, float(d.max()))
    return worst


def assert_borderline_cap():
    """the condition under which borderline pairs may be left out: at most 2 % of any case (the reference alone, on the CPU)"""
    for name, _, e in geometry_references():
        b = ref.borderline(e)
        assert b.sum() <= BORDERLINE_CAP * max(len(b), 1), "%s: %d of %d pairs are borderline" % (name, b.sum(), len(b))


# ------------------------------------------------------------------------------------------------ descriptors
def _random_desc(rs, n):
    return rs.randint(0, 256, (n, 32)).astype(np.uint8)


def flip_bits(rs, desc, k):
    """`desc` (32 bytes) with k distinct bits flipped"""
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    pos = rs.choice(256, k, replace=False)
    bits[pos] ^= 1
    return np.packbits(bits)


BOUNDARY_RATIOS = [(7 * k + dd, 10 * k) for k in range(1, 11) for dd in (-1, 0, 1)]       # (d0, d1): 7k < 0.7 * 10k is false


@functools.lru_cache(maxsize=None)
def boundary_descriptors():
    """left descriptor i has exactly two near right descriptors, at BOUNDARY_RATIOS[i] bits; then three left descriptors whose two
    best right descriptors are exact duplicates of each other (a tie: no match).  Returns left, right, expected (d0, d1) per left"""
    rs = np.random.RandomState(21)
    left = _random_desc(rs, len(BOUNDARY_RATIOS) + 3)
    right, want = [], []
    for i, (d0, d1) in enumerate(BOUNDARY_RATIOS):
        right += [flip_bits(rs, left[i], d1), flip_bits(rs, left[i], d0)]
        want.append((d0, d1))
    for i in range(len(BOUNDARY_RATIOS), len(left)):
        twin = flip_bits(rs, left[i], 3 * (i - len(BOUNDARY_RATIOS)))       # 0, 3 and 6 bits away, twice each
        right += [twin, twin.copy()]
        want.append((3 * (i - len(BOUNDARY_RATIOS)),) * 2)
    return left, np.array(right, np.uint8), np.array(want, np.int32)


def _keypoints(pts, octv):
    return np.concatenate([np.asarray(pts, np.float64), np.asarray(octv, np.float64)[:, None]], 1)


@functools.lru_cache(maxsize=None)
def frame_case(name):
    """one rig frame in extractor order (non-lapping key points first): dict(rig, kps_l, desc_l, mono_l, kps_r, desc_r, mono_r), kps
    = (n, 3) of x, y, octave.  Lapping left key point j looks at lapping right key point perm[j] (a few bits flipped); the right side
    also holds distractors and exact duplicates of some matched descriptors; `many` left key points are noisy copies of one
    accepted pair (several left onto one right)."""
    rig_name, seed, lap_l, lap_r, mono_l, mono_r, many = {
        "frame_a": ("tumvi", 31, 130, 150, 37, 21, 4), "frame_b": ("tumvi", 32, 65, 65, 5, 60, 0), "frame_c": ("diverging", 33, 90, 129, 0, 3, 3),
        "frame_nolap_l": ("tumvi", 34, 0, 40, 50, 10, 0), "frame_nolap_r": ("tumvi", 35, 40, 0, 10, 50, 0), "frame_one_r": ("tumvi", 36, 20, 1, 3, 4, 0),
    }[name]
    rs = np.random.RandomState(seed)
    rig = RIGS[rig_name]
    n_pairs = min(lap_l, lap_r)
    pl, pr, ol, orr = _scene(rig, rs, max(n_pairs, 1))
    # keep most pairs close enough for parallax, so that a frame holds matches
    dl = _random_desc(rs, lap_l)
    dr = _random_desc(rs, lap_r)
    kl = np.zeros((lap_l, 3)); kr = np.zeros((lap_r, 3))
    kl[:, :2] = rs.uniform(20, 490, (lap_l, 2)); kr[:, :2] = rs.uniform(20, 490, (lap_r, 2))
    kl[:, 2] = rs.randint(0, N_LEVELS, lap_l); kr[:, 2] = rs.randint(0, N_LEVELS, lap_r)
    perm = rs.permutation(lap_r)[:n_pairs] if n_pairs else np.zeros(0, int)
    for j in range(n_pairs):
        kl[j] = (pl[j, 0], pl[j, 1], ol[j]); kr[perm[j]] = (pr[j, 0], pr[j, 1], orr[j])
        dr[perm[j]] = flip_bits(rs, dl[j], rs.randint(0, 25))
    free = [r for r in range(lap_r) if r not in set(perm.tolist())]
    for q, r in enumerate(free[: len(free) // 2]):                      # exact duplicates of matched right descriptors: a tie
        if n_pairs:
            dr[r] = dr[perm[(7 * q) % n_pairs]]
    src = None
    if many and n_pairs:
        probe = ref.triangulate_matches(rig, pl[:n_pairs], pr[:n_pairs], LEVEL_SIGMA2[ol[:n_pairs]], LEVEL_SIGMA2[orr[:n_pairs]])
        dup_of = {int(perm[(7 * q) % n_pairs]) for q in range(len(free) // 2)}
        good = [j for j in np.nonzero(probe["accepted"])[0] if int(perm[j]) not in dup_of]
        src = good[0]
        for q in range(many):                                           # the last `many` lapping left key points copy pair `src`
            j = lap_l - 1 - q
            kl[j] = kl[src]
            kl[j, :2] += 0.02 * (q + 1)
            dl[j] = flip_bits(rs, dl[src], q + 1)
    kps_l = np.concatenate([np.column_stack([rs.uniform(20, 490, (mono_l, 2)), rs.randint(0, N_LEVELS, mono_l)]).reshape(mono_l, 3), kl])
    kps_r = np.concatenate([np.column_stack([rs.uniform(20, 490, (mono_r, 2)), rs.randint(0, N_LEVELS, mono_r)]).reshape(mono_r, 3), kr])
    kps_l[:, :2] = kps_l[:, :2].astype(np.float32); kps_r[:, :2] = kps_r[:, :2].astype(np.float32)
    desc_l = np.concatenate([_random_desc(rs, mono_l), dl]); desc_r = np.concatenate([_random_desc(rs, mono_r), dr])
    return dict(rig=rig, kps_l=kps_l, desc_l=desc_l, mono_l=mono_l, kps_r=kps_r, desc_r=desc_r, mono_r=mono_r,
                many_onto=None if src is None else int(perm[src]) + mono_r, many_from=[mono_l + lap_l - 1 - q for q in range(many)] + ([mono_l + src] if src is not None else []))


FRAME_CASES = ("frame_a", "frame_b", "frame_c", "frame_nolap_l", "frame_nolap_r", "frame_one_r")


@functools.lru_cache(maxsize=None)
def frame_reference(name, mode="faithful"):
    c = frame_case(name)
    return ref.stereo_fisheye(c["rig"], c["kps_l"], c["desc_l"], c["mono_l"], c["kps_r"], c["desc_r"], c["mono_r"], LEVEL_SIGMA2,
                              ref.FAITHFUL if mode == "faithful" else ref.EXACT)


def knn_case(lap_l, lap_r, mono_l=3, mono_r=5, seed=41):
    """descriptors for the exact k-NN test: the boundary and duplicate descriptors first (as far as they fit), the rest random with a
    near copy on the other side"""
    rs = np.random.RandomState(seed + 1000 * lap_l + lap_r)
    bl, br, _ = boundary_descriptors()
    dl, dr = _random_desc(rs, lap_l), _random_desc(rs, lap_r)
    l0, r0 = (len(bl), len(br)) if lap_l >= len(bl) and lap_r >= len(br) else (0, 0)
    dl[:l0] = bl[:l0]; dr[:r0] = br[:r0]
    for j in range(l0, min(lap_l, l0 + (lap_r - r0) // 2)):
        dr[r0 + j - l0] = flip_bits(rs, dl[j], rs.randint(0, 60))
    return np.concatenate([_random_desc(rs, mono_l), dl]), mono_l, np.concatenate([_random_desc(rs, mono_r), dr]), mono_r


def rig_floats(rig):
    """the 30 floats of tests/fisheye_geometry_check.cpp: both cameras with their precision, Rlr row major, tlr"""
    cam = lambda c, p: [c["fx"], c["fy"], c["cx"], c["cy"]] + list(c["k"]) + [p]
    return np.array(cam(rig["left"], rig["precision_l"]) + cam(rig["right"], rig["precision_r"]) + list(rig["Rlr"].reshape(-1)) + list(rig["tlr"]), np.float32)


def check_geometry(name, code, p3d, faithful, exact):
    """`code` [n] and `p3d` [n, 3] of an implementation against the faithful evaluation: the outcome equal outside the borderline band
    of the exact evaluation, depth and point of the pairs both accept within P3D_RTOL * |p3d|; prints the figures before asserting"""
    code, p3d = np.asarray(code, np.float32), np.asarray(p3d, np.float32).reshape(-1, 3)
    band = ref.borderline(exact)
    got, want = ref.outcome(code), ref.outcome(faithful["code"])
    both = (got == 0) & (want == 0)
    scale = np.linalg.norm(faithful["p3d"][both].astype(np.float64), axis=1)
    dp = np.linalg.norm(p3d[both].astype(np.float64) - faithful["p3d"][both], axis=1) / scale if both.any() else np.zeros(0)
    dz = np.abs(code[both].astype(np.float64) - faithful["code"][both]) / scale if both.any() else np.zeros(0)
    print("%s: %d pairs, %d borderline, %d outcomes differ outside the band, %d accepted, worst point %.3g depth %.3g (allowed %.3g)" %
          (name, len(code), band.sum(), ((got != want) & ~band).sum(), both.sum(), dp.max() if len(dp) else 0.0, dz.max() if len(dz) else 0.0, P3D_RTOL))
    assert band.sum() <= BORDERLINE_CAP * max(len(band), 1)
    assert np.array_equal(got[~band], want[~band]), "%s: outcomes differ outside the borderline band at %s" % (name, np.nonzero((got != want) & ~band)[0][:10])
    rejected = got != 0
    assert not p3d[rejected].any(), "%s: a rejected pair has a point" % name
    assert (dp <= P3D_RTOL).all() and (dz <= P3D_RTOL).all(), "%s: accepted pairs differ by %.3g / %.3g of |p3d|" % (name, dp.max(), dz.max())
