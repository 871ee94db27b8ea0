"""Plain sequential restatement of LocalMapping::CreateNewMapPoints for two-camera KannalaBrandt8 rigs, written from the
reference's text (src/LocalMapping.cc:392-716 with mpCamera2 set on both key frames, src/MapPoint.cc:426-494), in float32
(fsr.FAITHFUL) and float64 (fsr.EXACT).  A test helper, not a test; the product never imports it.

Built on rig_bow_reference (the rig SearchForTriangulation and its gate), fisheye_stereo_reference (KannalaBrandt8 unproject /
project) and newpoints_reference (Triangulate, the guard bands).  The Ow1 state is explicit: `state` is 0 while the reference's
Ow1 holds key frame 1's left centre and 1 while it holds the right one (:423 declares Ow1 outside the neighbour loop, :512 / 522 /
532 / 542 overwrite it per match).

Measured on the CPU in the session that wrote this file (tests/test_rig_newpoints_reference.py prints and bounds the live values):
  SPREAD_F32       the point metric between the float32 and the float64 run of this reference over every scene of
                   rig_newpoints_cases.py: 3.45e-7 at most (scene three_neighbours; the two random scenes 2.50e-7 and
                   2.22e-7).  The conventional call's figure is 1.02e-7: the fisheye unprojection adds a Newton iteration and a
                   tangent, and rays up to about 60 degrees off the axis enter Triangulate's matrix with |xn| up to about 1.8.
  the bar for the device and the host build of the header is 4 x SPREAD_F32 = 1.38e-6, the margin DESIGN.md section 4c gives
  worst sigma1 / sigma3 of Triangulate's matrix over the accepted pairs of these scenes: 23 (bound: TRI_COND_MAX)"""
import numpy as np

import fisheye_stereo_reference as fsr
import newpoints_reference as nr
import rig_bow_reference as rbr

GUARD_COS, GUARD_REL, GUARD_DEPTH = nr.GUARD_COS, nr.GUARD_REL, nr.GUARD_DEPTH
GUARD_BASELINE = 1e-3           # relative, |baseline / mb - 1|: a baseline test inside it is not compared
CAP_PAIRS, CAP_FEATURES = 0.01, 0.02

SPREAD_F32 = 3.46e-7
# As newpoints_common.TRI_DOUBLE_BOUND: against the float64 null vector of the SAME float matrix the differences are the rounding
# of the coordinates to float (2^-24 relative each) and the double eigen-solve, eps64 * (sigma1 / sigma3)^2.  Fisheye rays reach
# |xn| = tan(75 deg) = 3.7, which scales rows of the matrix; the argument holds while (sigma1 / sigma3)^2 <= 1e6, i.e. the ratio
# of the largest to the third singular value stays below TRI_COND_MAX (the no-GPU test asserts it on every scene; 23 is the
# worst seen), and the absolute term keeps section 4c's factor of ten on top.
TRI_DOUBLE_BOUND_REL, TRI_DOUBLE_BOUND_ABS = 2.0 ** -24, 2.2e-9
TRI_COND_MAX = 1e3


def side_of(kf, right):
    """pose, centre and camera of the left / right camera of a rig key frame"""
    r = int(bool(right))
    c = np.asarray(kf["cam"], np.float32).reshape(2, 9)[r]
    return dict(Rcw=np.asarray(kf["Rcw"], np.float32).reshape(2, 3, 3)[r], tcw=np.asarray(kf["tcw"], np.float32).reshape(2, 3)[r],
                Ow=np.asarray(kf["Ow"], np.float32).reshape(2, 3)[r],
                cam=dict(fx=float(c[0]), fy=float(c[1]), cx=float(c[2]), cy=float(c[3]), k=[float(v) for v in c[4:8]]), precision=float(c[8]))


def obs_of(kf, i):
    o = int(kf["octave"][i])
    return dict(x=kf["x"][i], y=kf["y"][i], sigma2=kf["level_sigma2"][o], scale=kf["scale_factors"][o])


def _norm(v, T):
    """Eigen's norm of a fixed-size 3-vector: sqrt(a0 a0 + (a1 a1 + a2 a2))"""
    v = np.asarray(v, T)
    return T(np.sqrt(v[0] * v[0] + (v[1] * v[1] + v[2] * v[2])))


def baseline(Ow1, Ow2, T):
    """(Ow2 - Ow1).norm() (:449-450)"""
    return _norm(np.asarray(Ow2, np.float32).astype(T) - np.asarray(Ow1, np.float32).astype(T), T)


def pair_geometry(S1, o1, S2, o2, rule, dtype=np.float64, matrix_dtype=None):
    """One match through :561-695 with bStereo1 = bStereo2 = false.  Returns dict(accept, x3d, margins=[(gate, signed margin,
    guard)], undecided, sin_parallax, cond); a margin is positive when the pair passes that comparison the way it went.
    matrix_dtype = np.float32 builds Triangulate's matrix in float (as the reference and the kernel do) and takes its null vector
    in `dtype`."""
    T = dtype
    margins = []
    out = dict(accept=False, x3d=None, margins=margins, sin_parallax=None, cond=None)

    def finish():
        out["undecided"] = any(abs(m) < g for _, m, g in margins)
        return out

    def gate(name, value, guard):
        margins.append((name, float(value), guard))
        return value > 0

    def cmp(name, a, b):        # a < b
        r = a < b
        margins.append((name, float(b - a) if r else float(a - b), GUARD_COS))
        return r

    def rays(M):
        xn1 = fsr.unproject(S1["cam"], S1["precision"], np.array([[o1["x"], o1["y"]]], M), M)[0]
        xn2 = fsr.unproject(S2["cam"], S2["precision"], np.array([[o2["x"], o2["y"]]], M), M)[0]
        return xn1, xn2

    R1, t1, C1 = S1["Rcw"].astype(T), S1["tcw"].astype(T), S1["Ow"].astype(T)
    R2, t2, C2 = S2["Rcw"].astype(T), S2["tcw"].astype(T), S2["Ow"].astype(T)
    xn1, xn2 = rays(T)
    ray1, ray2 = R1.T @ xn1, R2.T @ xn2
    cosR = T(ray1.dot(ray2) / (np.linalg.norm(ray1) * np.linalg.norm(ray2)))
    out["sin_parallax"] = float(np.sqrt(max(0.0, 1.0 - float(cosR) ** 2)))
    # cosParallaxStereo = cosParallaxRays + 1: the first comparison of :586 always holds for a finite cosine and has no margin
    if not cmp("cosRays>0", T(0), cosR):
        return finish()
    if not cmp("cosRays<bound", float(cosR), 0.9996 if rule["inertial"] else 0.9998):
        return finish()
    if matrix_dtype is not None:
        M = matrix_dtype
        m1, m2 = rays(M)
        A = nr.triangulation_matrix(m1, m2, np.c_[S1["Rcw"].astype(M), S1["tcw"].astype(M)], np.c_[S2["Rcw"].astype(M), S2["tcw"].astype(M)], M).astype(T)
    else:
        A = nr.triangulation_matrix(xn1, xn2, np.c_[R1, t1], np.c_[R2, t2], T)
    sv = np.linalg.svd(A.astype(np.float64), compute_uv=False)
    out["cond"] = float(sv[0] / sv[2])
    v = nr.null_vector_svd(A)
    if v[3] == 0:
        return finish()
    x3D = (v[:3] / v[3]).astype(T)
    out["x3d"] = x3D

    d1, d2 = T(np.linalg.norm(x3D - C1)), T(np.linalg.norm(x3D - C2))              # from the SIDES' centres
    z1 = T(R1[2].dot(x3D) + t1[2])
    if not gate("z1>0", z1 / max(d1, T(1e-30)), GUARD_DEPTH):
        return finish()
    z2 = T(R2[2].dot(x3D) + t2[2])
    if not gate("z2>0", z2 / max(d2, T(1e-30)), GUARD_DEPTH):
        return finish()

    def reproj(tag, S, R, t, o, z):
        X = np.array([[T(R[0].dot(x3D) + t[0]), T(R[1].dot(x3D) + t[1]), z]], T)
        uv = fsr.project(S["cam"], X, T)[0]
        ex, ey = uv[0] - T(o["x"]), uv[1] - T(o["y"])
        return gate(tag, 1.0 - float(T(ex * ex + ey * ey)) / nr.chi2_threshold(5.991, o["sigma2"]), GUARD_REL)

    if not reproj("reproj1", S1, R1, t1, o1, z1):
        return finish()
    if not reproj("reproj2", S2, R2, t2, o2, z2):
        return finish()
    if d1 == 0 or d2 == 0:
        return finish()
    if rule["far_points"]:
        th_far = float(np.float32(rule["th_far"]))
        if not (gate("far1", 1.0 - float(d1) / th_far, GUARD_REL) and gate("far2", 1.0 - float(d2) / th_far, GUARD_REL)):
            return finish()
    ratioDist = T(d2 / d1)
    ratioFactor = T(np.float32(1.5) * np.float32(rule["scale_factor_1"]))
    ratioOctave = T(T(o1["scale"]) / T(o2["scale"]))
    if not gate("scale_lo", float(ratioDist * ratioFactor) / float(ratioOctave) - 1.0, GUARD_REL):
        return finish()
    if not gate("scale_hi", 1.0 - float(ratioDist) / float(ratioOctave * ratioFactor), GUARD_REL):
        return finish()
    out["accept"] = True
    return finish()


def normal_and_depth(x3d, Ow_side1, Ow_side2, Ow_left1, level_scale, last_scale, T=np.float64):
    """MapPoint::UpdateNormalAndDepth of the new point: the normal from the centres of the two observing SIDES, the distance
    from pRefKF->GetCameraCenter(), key frame 1's LEFT centre (:468)"""
    x3d, a, b, c = (np.asarray(v, np.float32).astype(T) if i else np.asarray(v, T) for i, v in enumerate((x3d, Ow_side1, Ow_side2, Ow_left1)))
    n = (x3d - a) / np.linalg.norm(x3d - a) + (x3d - b) / np.linalg.norm(x3d - b)
    mx = np.linalg.norm(x3d - c) * T(level_scale)
    return n / 2, mx, mx / T(last_scale)


def search_scene(scene, j, has_mp1):
    kf1, kf2 = scene["kf1"], scene["neighbours"][j]
    return dict(kf1=dict(kf1, has_mp=np.ascontiguousarray(has_mp1, np.uint8)), kf2=kf2, geom=scene["pairs"][j]["geom"],
                sigma2_1=kf1["level_sigma2"], sigma2_2=kf2["level_sigma2"])


def search_tables(scene, j, dtype):
    """of neighbour j with key frame 1's ORIGINAL has_mp (a superset of every later search's candidates): the gate outcome of
    every Hamming survivor under `dtype`, which features have a survivor, and which have one inside the borderline band of the
    float64 gate.  Cached on the scene."""
    cache = scene.setdefault("_tables", {})
    key = (j, np.dtype(dtype).name)
    if key not in cache:
        n1 = len(scene["kf1"]["x"])
        s = search_scene(scene, j, scene["kf1"]["has_mp"])
        sv = rbr.survivors(s)
        has_sv, band, passes = np.zeros(n1, bool), np.zeros(n1, bool), {}
        for (a, _, _, _) in sv:
            has_sv[a] = True
        if sv and not scene["pairs"][j]["coarse"]:
            g = rbr.gate(s, sv, dtype)
            passes = {(a, b): bool(dtype(c) > dtype(rbr.GATE_Z)) for (a, b, _, _), c in zip(sv, g["code"])}
            for (a, _, _, _), flag in zip(sv, fsr.borderline(rbr.gate(s, sv, fsr.EXACT))):
                band[a] |= bool(flag)
        cache[key] = (passes, has_sv, band)
    return cache[key]


def search(scene, j, has_mp1, dtype):
    """SearchForTriangulation(kf1, neighbour j, false, coarse) with ORBmatcher(0.6, false): match12"""
    passes, _, _ = search_tables(scene, j, dtype)
    return rbr.search_for_triangulation_rig(search_scene(scene, j, has_mp1), coarse=bool(scene["pairs"][j]["coarse"]), passes=passes)[1]


def baseline_tests(scene, T=np.float32):
    """per neighbour: (baseline from the left centre, from the right centre, mb of the neighbour) and the two skip decisions"""
    kf1 = scene["kf1"]
    Ow = np.asarray(kf1["Ow"], np.float32).reshape(2, 3)
    rows = []
    for kf2 in scene["neighbours"]:
        Ow2 = np.asarray(kf2["Ow"], np.float32).reshape(2, 3)[0]        # the neighbour's LEFT centre, fresh per neighbour (:448)
        rows.append((baseline(Ow[0], Ow2, T), baseline(Ow[1], Ow2, T), T(np.float32(kf2["mb"]))))
    b = np.array(rows, np.float64).reshape(-1, 3)
    return b, b[:, 0] < b[:, 2], b[:, 1] < b[:, 2]


def create_new_map_points_rig(scene, dtype=np.float64):
    """The sequential loop.  Per feature: neighbour, idx2, x3d, normal, max_dist, min_dist, undecided_from (first neighbour at
    which the feature met a borderline search candidate or an undecided pair, or -1); per neighbour: skipped, n_matched,
    n_created, match12, state_after (the Ow1 state after the neighbour), and for the comparison under the guard bands
    matched_certain / matched_open and created_certain / created_open (features whose outcome at that neighbour the bands leave
    open); pairs = [(idx1, j, idx2, accept, undecided, sin_parallax, x3d, margins)]; state_open_at = the first neighbour whose
    baseline test differs between the two centres AND reads a state that an open feature may have decided, or -1; baseline_open =
    neighbours whose own baseline test lies inside GUARD_BASELINE."""
    T = dtype
    kf1, nbs, rule = scene["kf1"], scene["neighbours"], scene["params"]
    n1, nb, n_left = len(kf1["x"]), len(nbs), int(kf1["n_left"])
    has_mp = np.ascontiguousarray(kf1["has_mp"]).copy()
    res = dict(neighbour=np.full(n1, -1, np.int32), idx2=np.full(n1, -1, np.int32), x3d=np.zeros((n1, 3), T), point_stereo=np.zeros(n1, np.uint8),
               normal=np.zeros((n1, 3), T), max_dist=np.zeros(n1, T), min_dist=np.zeros(n1, T), undecided_from=np.full(n1, -1, np.int32),
               skipped=np.zeros(nb, np.uint8), n_matched=np.zeros(nb, np.int32), n_created=np.zeros(nb, np.int32), match12=[], state_after=[],
               matched_certain=np.zeros(nb, np.int32), matched_open=np.zeros(nb, np.int32), created_certain=np.zeros(nb, np.int32),
               created_open=np.zeros(nb, np.int32), pairs=[], state_open_at=-1, baseline_open=[], cond_max=0.0)
    Ow = np.asarray(kf1["Ow"], np.float32).reshape(2, 3)
    b, skipL, skipR = baseline_tests(scene, T)
    und = res["undecided_from"]
    state, state_open = 0, False                                        # Ow1 = GetCameraCenter() before any match (:423)
    for j, kf2 in enumerate(nbs):
        if min(abs(b[j, 0] / max(b[j, 2], 1e-30) - 1), abs(b[j, 1] / max(b[j, 2], 1e-30) - 1)) < GUARD_BASELINE:
            res["baseline_open"].append(j)
        if skipL[j] != skipR[j] and state_open and res["state_open_at"] < 0:
            res["state_open_at"] = j
        res["state_after"].append(state)
        if (skipR if state else skipL)[j]:                              # if(baseline < pKF2->mb) continue;
            res["skipped"][j] = 1
            res["match12"].append(np.full(n1, -1, np.int32))
            continue
        m12 = np.asarray(search(scene, j, has_mp, T))
        _, has_sv, band = search_tables(scene, j, fsr.EXACT)
        reach = ~has_mp.astype(bool) & has_sv
        open_before = reach & (und >= 0)                                # left the comparison at an earlier neighbour
        open_here = reach & ~open_before & band
        und[open_here] = j
        certain = (m12 >= 0) & ~open_before & ~open_here
        res["match12"].append(m12.copy())
        res["n_matched"][j] = int((m12 >= 0).sum())
        res["matched_certain"][j] = int(certain.sum())
        res["matched_open"][j] = int((open_before | open_here).sum())
        cm = int(np.nonzero(certain)[0].max()) if certain.any() else -1
        um = int(np.nonzero(open_before | open_here)[0].max()) if (open_before | open_here).any() else -1
        if um > cm:
            state_open = True
        elif cm >= 0:
            state_open = False
        for i1 in np.nonzero(m12 >= 0)[0]:                              # ascending idx1 (src/ORBmatcher.cc:1138-1143)
            i2 = int(m12[i1])
            r1, r2 = i1 >= n_left, i2 >= int(kf2["n_left"])
            state = int(r1)                                             # Ow1 = the centre of this match's side, accepted or not
            S1, S2 = side_of(kf1, r1), side_of(kf2, r2)
            g = pair_geometry(S1, obs_of(kf1, i1), S2, obs_of(kf2, i2), rule, T)
            res["pairs"].append((int(i1), j, i2, g["accept"], g["undecided"], g["sin_parallax"], g["x3d"], g["margins"]))
            if g["undecided"] and und[i1] < 0:
                und[i1] = j
            if g["accept"]:
                res["cond_max"] = max(res["cond_max"], g["cond"])
                has_mp[i1] = 1
                res["neighbour"][i1], res["idx2"][i1], res["x3d"][i1] = j, i2, g["x3d"]
                res["normal"][i1], res["max_dist"][i1], res["min_dist"][i1] = normal_and_depth(
                    g["x3d"], S1["Ow"], S2["Ow"], Ow[0], kf1["scale_factors"][kf1["octave"][i1]], kf1["scale_factors"][-1], T)
                res["n_created"][j] += 1
                if und[i1] < 0:
                    res["created_certain"][j] += 1
        res["created_open"][j] = int((reach & (und >= 0)).sum())
        res["state_after"][-1] = state
    return res


def chain(scene, skipped, dtype=np.float64):
    """The chain reading the kernel implements: GIVEN which neighbours are skipped, a feature of key frame 1 depends on nothing
    but its own chain -- every search runs with the ORIGINAL has_mp, and a feature walks the neighbours until the first one that
    accepts it.  Returns neighbour, idx2, n_matched, n_created, match12, max_matched_idx1."""
    kf1, nbs, rule = scene["kf1"], scene["neighbours"], scene["params"]
    n1, nb, n_left = len(kf1["x"]), len(nbs), int(kf1["n_left"])
    stale = [None if skipped[j] else np.asarray(search(scene, j, kf1["has_mp"], dtype)) for j in range(nb)]
    out = dict(neighbour=np.full(n1, -1, np.int32), idx2=np.full(n1, -1, np.int32), n_matched=np.zeros(nb, np.int32), n_created=np.zeros(nb, np.int32),
               match12=np.full((nb, n1), -1, np.int32), max_matched_idx1=np.full(nb, -1, np.int32))
    for i1 in range(n1):
        for j in range(nb):
            if stale[j] is None or stale[j][i1] < 0:
                continue
            i2 = int(stale[j][i1])
            kf2 = nbs[j]
            out["n_matched"][j] += 1
            out["match12"][j, i1] = i2
            out["max_matched_idx1"][j] = max(out["max_matched_idx1"][j], i1)
            g = pair_geometry(side_of(kf1, i1 >= n_left), obs_of(kf1, i1), side_of(kf2, i2 >= int(kf2["n_left"])), obs_of(kf2, i2), rule, dtype)
            if g["accept"]:
                out["neighbour"][i1], out["idx2"][i1] = j, i2
                out["n_created"][j] += 1
                break
    return out


def shares(ref):
    """(share of reached pairs that are undecided, share of key frame 1's features that are undecided)"""
    u = sum(1 for p in ref["pairs"] if p[4]) + int(sum(ref["matched_open"]))
    return u / max(len(ref["pairs"]), 1), float((ref["undecided_from"] >= 0).mean()) if len(ref["undecided_from"]) else 0.0


def point_error(x_dev, x_ref, Ow_side1, sin_parallax):
    """|x_dev - x_ref| / |x_ref - Ow_side1| * sin(parallax)"""
    x_ref = np.asarray(x_ref, np.float64)
    return float(np.linalg.norm(np.asarray(x_dev, np.float64) - x_ref) / np.linalg.norm(x_ref - np.asarray(Ow_side1, np.float64)) * sin_parallax)


def compare(ref, dev, scene, label=""):
    """ref = the float64 sequential reference, dev = dict(neighbour, idx2, x3d [, point_stereo, skipped, n_matched, n_created,
    match12, normal, max_dist, min_dist]) of the implementation under test.  Integer results are compared exactly for every
    feature outside the guard bands; returns the point errors of the pairs both sides accept."""
    kf1 = scene["kf1"]
    n1, n_left = len(kf1["x"]), int(kf1["n_left"])
    assert n1 == len(dev["neighbour"]), label
    assert ref["state_open_at"] < 0 and not ref["baseline_open"], "%s: a baseline test of this scene hangs on a guard band: change the scene" % label
    und_from = ref["undecided_from"]
    decided = und_from < 0
    if "skipped" in dev:
        assert np.array_equal(np.asarray(dev["skipped"]), ref["skipped"]), "%s skipped: dev %s ref %s" % (label, dev["skipped"], ref["skipped"])
    for k in ("neighbour", "idx2", "point_stereo"):
        if k not in dev:
            continue
        bad = np.nonzero(decided & (np.asarray(dev[k]) != ref[k]))[0]
        assert len(bad) == 0, "%s %s differs outside the guard band at features %s: dev %s ref %s" % (
            label, k, bad[:8], np.asarray(dev[k])[bad[:8]], ref[k][bad[:8]])
    early = [i for i in np.nonzero(~decided)[0] if 0 <= dev["neighbour"][i] < und_from[i]]
    assert not early, "%s features %s accepted before their first undecided pair" % (label, early[:8])
    if dev.get("match12") is not None:
        for j, m_ref in enumerate(ref["match12"]):
            reach = (ref["neighbour"] < 0) | (ref["neighbour"] >= j)           # not yet a map point when neighbour j is searched
            reach &= ~np.asarray(kf1["has_mp"], bool)
            ok = reach & (decided | (und_from > j))
            bad = np.nonzero(ok & (np.asarray(dev["match12"])[j] != m_ref))[0]
            assert len(bad) == 0, "%s neighbour %d: match differs at features %s" % (label, j, bad[:8])
    for k, c, o in (("n_matched", "matched_certain", "matched_open"), ("n_created", "created_certain", "created_open")):
        if k in dev:
            d = np.asarray(dev[k])
            assert ((d >= ref[c]) & (d <= ref[c] + ref[o])).all(), "%s %s: dev %s outside [%s, + %s]" % (label, k, d, ref[c], ref[o])
    errs = []
    Ow = np.asarray(kf1["Ow"], np.float32).reshape(2, 3)
    for (i1, j, i2, accept, undecided, sinp, x3d, _) in ref["pairs"]:
        if accept and dev["neighbour"][i1] == j and dev["idx2"][i1] == i2:
            errs.append(point_error(dev["x3d"][i1], x3d, Ow[int(i1 >= n_left)], sinp))
            if "normal" in dev and decided[i1]:
                assert np.abs(np.asarray(dev["normal"][i1], np.float64) - ref["normal"][i1]).max() < 1e-5, (label, i1)
                assert abs(float(dev["max_dist"][i1]) / ref["max_dist"][i1] - 1) < 1e-5 and abs(float(dev["min_dist"][i1]) / ref["min_dist"][i1] - 1) < 1e-5, (label, i1)
    return errs


def pack_pairs(scene, triples):
    """float32 records for tests/rig_newpoints_geometry_check.cpp, one per (idx1, j, idx2): two sides of 24 floats (Rcw, tcw, Ow,
    camera), two observations of 4, the rule of 4, key frame 1's left centre, level scale and last scale"""
    kf1, rule = scene["kf1"], scene["params"]
    rows = []
    for (i1, j, i2) in triples:
        kf2 = scene["neighbours"][j]
        row = []
        for kf, i in ((kf1, i1), (kf2, i2)):
            r = int(i >= int(kf["n_left"]))
            row += list(np.asarray(kf["Rcw"], np.float32).reshape(2, 9)[r]) + list(np.asarray(kf["tcw"], np.float32).reshape(2, 3)[r])
            row += list(np.asarray(kf["Ow"], np.float32).reshape(2, 3)[r]) + list(np.asarray(kf["cam"], np.float32).reshape(2, 9)[r])
        for kf, i in ((kf1, i1), (kf2, i2)):
            o = obs_of(kf, i)
            row += [o["x"], o["y"], o["sigma2"], o["scale"]]
        row += [float(rule["inertial"]), float(rule["far_points"]), rule["th_far"], np.float32(1.5) * np.float32(rule["scale_factor_1"])]
        row += list(np.asarray(kf1["Ow"], np.float32).reshape(2, 3)[0]) + [kf1["scale_factors"][kf1["octave"][i1]], kf1["scale_factors"][-1]]
        rows.append(row)
    return np.asarray(rows, np.float32).reshape(-1, 65)
