"""Plain-loop restatements of the two vocabulary-guided searches of ORBmatcher for two-camera fisheye rigs, written from the
reference's text (src/ORBmatcher.cc): SearchByBoW(KeyFrame*, Frame&) with F.Nleft != -1 (:223-425, the `else` branches at :296-323
and :357-386) and SearchForTriangulation with both key frames rigs (:907-1146).  A test helper, not a test.

Feature indices run over the concatenated arrays of a rig: the left features first, right feature j at Nleft + j."""
import numpy as np

import fisheye_stereo_reference as fsr
from matcher_reference import HISTO_LENGTH, TH_LOW, _common_nodes, _drop_bins, f32, hamming, rot_bin

GATE_Z = np.float32(0.0001)         # KannalaBrandt8::epipolarConstrain: TriangulateMatches(...) > 0.0001f


def search_by_bow_rig(dKF, validKF, angKF, fvKF, dF, n_left, angF, fvF, nnratio=0.7, check_ori=True):
    """(nmatches, match[nF] = KF feature or -1).  Two (best, second, index) triples per key-frame feature; everything under the
    LEFT best <= TH_LOW (:327); the right ratio test is `|| true` (:359); one histogram of slot indices over both sides."""
    match = np.full(len(dF), -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for (k0, k1), (f0, f1) in _common_nodes(fvKF, fvF):
        for real_kf in fvKF[2][k0:k1]:
            real_kf = int(real_kf)
            if not validKF[real_kf]:                                   # !pMP || pMP->isBad() (:257-261)
                continue
            best1, best_f, best2 = 256, -1, 256
            best1r, best_fr, best2r = 256, -1, 256
            for real_f in fvF[2][f0:f1]:
                real_f = int(real_f)
                if match[real_f] >= 0:                                 # :299
                    continue
                dist = hamming(dKF[real_kf], dF[real_f])
                if real_f < n_left and dist < best1:                   # :306
                    best2 = best1; best1 = dist; best_f = real_f
                elif real_f < n_left and dist < best2:
                    best2 = dist
                if real_f >= n_left and dist < best1r:                 # :315
                    best2r = best1r; best1r = dist; best_fr = real_f
                elif real_f >= n_left and dist < best2r:
                    best2r = dist
            if best1 <= TH_LOW:                                        # :327
                if f32(best1) < f32(nnratio) * f32(best2):             # :329
                    match[best_f] = real_kf
                    if check_ori:
                        hist[rot_bin(angKF[real_kf], angF[best_f])].append(best_f)
                    nmatches += 1
                if best1r <= TH_LOW:                                   # :357
                    if f32(best1r) < f32(nnratio) * f32(best2r) or True:       # :359
                        match[best_fr] = real_kf
                        if check_ori:
                            hist[rot_bin(angKF[real_kf], angF[best_fr])].append(best_fr)
                        nmatches += 1
    if check_ori:
        for j in _drop_bins(hist):
            match[j] = -1
            nmatches -= 1
    return nmatches, match


def pair_rigs(geom):
    """the four (camera 1, camera 2, R12, t12) records of an OrbmRigTriGeometry-like dict as rig dicts of
    fisheye_stereo_reference.triangulate_matches, in the order ll, lr, rl, rr"""
    cam = np.asarray(geom["cam"], np.float32).reshape(4, 9)
    R12 = np.asarray(geom["R12"], np.float32).reshape(4, 3, 3)
    t12 = np.asarray(geom["t12"], np.float32).reshape(4, 3)
    as_cam = lambda c: dict(fx=float(c[0]), fy=float(c[1]), cx=float(c[2]), cy=float(c[3]), k=[float(v) for v in c[4:8]])
    rigs = []
    for c in range(4):
        c1, c2 = cam[c >> 1], cam[2 + (c & 1)]
        rigs.append(dict(left=as_cam(c1), right=as_cam(c2), precision_l=float(c1[8]), precision_r=float(c2[8]), Rlr=R12[c], tlr=t12[c]))
    return rigs


def survivors(s):
    """the (idx1, idx2, dist, position of idx2 in its node) of every candidate the Hamming test lets through to the gate (:1004-1018
    without the running bestDist, which the set-function reading drops), in the reference's visiting order"""
    k1, k2 = s["kf1"], s["kf2"]
    out = []
    for (a0, a1), (b0, b1) in _common_nodes(k1["fv"], k2["fv"]):
        for idx1 in k1["fv"][2][a0:a1]:
            idx1 = int(idx1)
            if k1["has_mp"][idx1]:
                continue
            for pos, idx2 in enumerate(k2["fv"][2][b0:b1]):
                idx2 = int(idx2)
                if k2["has_mp"][idx2]:
                    continue
                dist = hamming(k1["desc"][idx1], k2["desc"][idx2])
                if dist <= TH_LOW:
                    out.append((idx1, idx2, dist, pos))
    return out


def gate(s, pairs, dtype=fsr.FAITHFUL):
    """TriangulateMatches of (idx1, idx2) pairs, each under the record of its (bRight1, bRight2) and with the level sigmas of its two
    octaves: dict of code and the gate quantities per pair (as fisheye_stereo_reference.triangulate_matches), and `sel`"""
    k1, k2 = s["kf1"], s["kf2"]
    i1 = np.array([p[0] for p in pairs], np.int64); i2 = np.array([p[1] for p in pairs], np.int64)
    sel = 2 * (i1 >= k1["n_left"]) + (i2 >= k2["n_left"])
    keys = ("code", "cos", "z1", "z2", "e1", "e2", "gate1", "gate2")
    out = {k: np.full(len(pairs), np.nan) for k in keys}
    rigs = pair_rigs(s["geom"])
    for c in range(4):
        w = np.nonzero(sel == c)[0]
        if not len(w):
            continue
        p1 = np.stack([k1["x"][i1[w]], k1["y"][i1[w]]], 1); p2 = np.stack([k2["x"][i2[w]], k2["y"][i2[w]]], 1)
        r = fsr.triangulate_matches(rigs[c], p1, p2, s["sigma2_1"][k1["octave"][i1[w]]], s["sigma2_2"][k2["octave"][i2[w]]], dtype)
        for k in keys:
            out[k][w] = r[k]
    out["sel"] = sel
    return out


def search_for_triangulation_rig(s, only_stereo=False, coarse=False, check_ori=False, passes=None):
    """(nmatches, match12[n1]) by the reference's sequential loop (:963-1112): bestDist starts at TH_LOW, a candidate with dist <=
    bestDist that passes the gate becomes the holder.  `passes`: {(idx1, idx2): bool} of precomputed gate outcomes (default: the
    faithful float32 evaluation of every Hamming survivor)."""
    k1, k2 = s["kf1"], s["kf2"]
    n1 = len(k1["x"])
    match12 = np.full(n1, -1, np.int32)
    if only_stereo:                                                    # bStereo1 is false for a rig key frame (:979-983)
        return 0, match12
    if passes is None and not coarse:
        sv = survivors(s)
        g = gate(s, sv)
        passes = {(a, b): bool(np.float32(c) > GATE_Z) for (a, b, _, _), c in zip(sv, g["code"])}
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for (a0, a1), (b0, b1) in _common_nodes(k1["fv"], k2["fv"]):
        for idx1 in k1["fv"][2][a0:a1]:
            idx1 = int(idx1)
            if k1["has_mp"][idx1]:
                continue
            best_dist, best_idx2 = TH_LOW, -1
            for idx2 in k2["fv"][2][b0:b1]:
                idx2 = int(idx2)
                if k2["has_mp"][idx2]:
                    continue
                dist = hamming(k1["desc"][idx1], k2["desc"][idx2])
                if dist > TH_LOW or dist > best_dist:
                    continue
                if coarse or passes[(idx1, idx2)]:
                    best_idx2 = idx2; best_dist = dist
            if best_idx2 >= 0:
                match12[idx1] = best_idx2
                nmatches += 1
                if check_ori:
                    hist[rot_bin(k1["angle"][idx1], k2["angle"][best_idx2])].append(idx1)
    if check_ori:
        for i in _drop_bins(hist):
            match12[i] = -1
            nmatches -= 1
    return nmatches, match12


def undecided(s):
    """key-frame-1 features with a Hamming survivor inside the borderline band of the float64 evaluation: bool [n1]"""
    sv = survivors(s)
    out = np.zeros(len(s["kf1"]["x"]), bool)
    if sv:
        b = fsr.borderline(gate(s, sv, fsr.EXACT))
        for (idx1, _, _, _), flag in zip(sv, b):
            out[idx1] |= bool(flag)
    return out
