"""Numpy restatements of the ORBmatcher searches that had no second restatement, written from the reference text
(src/ORBmatcher.cc, src/Frame.cc:744-822, src/KeyFrame.cc:704-748, src/CameraModels/Pinhole.cpp:107-129) and from nothing
else: not from oracle/ and not from the kernels.  A test helper, not a test.

Plain loops; float expressions in np.float32 in the order the reference writes them, double where C++ promotes (the 5.99,
7.8 and 3.84*sigma2 literals, `rot<0.0`).  Every function takes the argument dicts of the `oracle.*` wrapper of the same
name.  Conventional cameras only (Nleft == -1, mpCamera2 == NULL), as the oracle and the kernels.

The two tracking searches have had their restatement since tests/test_projection_oracle.py; they are re-exported here."""
import math

import numpy as np

from test_projection_oracle import numpy_search_last, numpy_search_mp, _visit_order, _window  # noqa: F401

TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30     # src/ORBmatcher.cc:35-37
INT_MAX = 2 ** 31 - 1
f32 = np.float32


def c_round(v):
    """C round(): to nearest, halves away from zero, on the exact value of a float"""
    v = float(v)
    return int(math.floor(v + 0.5)) if v >= 0 else int(math.ceil(v - 0.5))


def hamming(a, b):
    """DescriptorDistance (:2058-2074): number of differing bits of two 256-bit descriptors"""
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def rot_bin(a1, a2):
    """:345-350 and its copies: rot = a1-a2; if(rot<0.0) rot+=360.0f; bin = round(rot*factor), factor = 1.0f/HISTO_LENGTH;
    bin == HISTO_LENGTH wraps to 0"""
    factor = f32(1.0) / f32(HISTO_LENGTH)
    rot = f32(a1) - f32(a2)
    if float(rot) < 0.0:
        rot = f32(rot + f32(360.0))
    b = c_round(f32(rot * factor))
    return 0 if b == HISTO_LENGTH else b


def three_maxima(counts):
    """ComputeThreeMaxima (:2012-2053) on the bin sizes: (ind1, ind2, ind3), -1 where there is none"""
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(counts):
        s = int(s)
        if s > max1:
            max3 = max2; max2 = max1; max1 = s
            ind3 = ind2; ind2 = ind1; ind1 = i
        elif s > max2:
            max3 = max2; max2 = s
            ind3 = ind2; ind2 = i
        elif s > max3:
            max3 = s; ind3 = i
    if f32(max2) < f32(0.1) * f32(max1):
        ind2 = -1; ind3 = -1
    elif f32(max3) < f32(0.1) * f32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def _drop_bins(hist):
    """entries of the bins that ComputeThreeMaxima does not keep, in the order of the clean-up loops (:412-421)"""
    keep = three_maxima([len(h) for h in hist])
    return [e for i in range(HISTO_LENGTH) if i not in keep for e in hist[i]]


# ---- the grid: Frame::AssignFeaturesToGrid / PosInGrid / GetFeaturesInArea ------------------------------------------------

class Grid:
    """mGrid[ix][iy] as Frame::AssignFeaturesToGrid fills it (src/Frame.cc:472-503): PosInGrid (:812-822) rounds
    (kp.pt.x-mnMinX)*mfGridElementWidthInv and drops what falls outside; features enter their cell in index order."""

    def __init__(self, g):
        self.g = g
        self.cols, self.rows = int(g.get("cols", 64)), int(g.get("rows", 48))
        self.min_x, self.min_y, self.max_x, self.max_y = (f32(g[k]) for k in ("min_x", "min_y", "max_x", "max_y"))
        self.winv = f32(self.cols) / f32(self.max_x - self.min_x)
        self.hinv = f32(self.rows) / f32(self.max_y - self.min_y)
        self.cells = {}
        for i in range(len(g["x"])):
            px = c_round(f32(f32(g["x"][i]) - self.min_x) * self.winv)
            py = c_round(f32(f32(g["y"][i]) - self.min_y) * self.hinv)
            if px < 0 or px >= self.cols or py < 0 or py >= self.rows:
                continue
            self.cells.setdefault((px, py), []).append(i)

    def features_in_area(self, x, y, r, min_level=-1, max_level=-1):
        """Frame::GetFeaturesInArea (src/Frame.cc:744-810); with min_level = max_level = -1 it is
        KeyFrame::GetFeaturesInArea (src/KeyFrame.cc:704-748), which has the same cells and no level filter"""
        g = self.g
        x, y, r = f32(x), f32(y), f32(r)
        out = []
        n_min_x = max(0, int(math.floor(f32(f32(f32(x - self.min_x) - r) * self.winv))))
        if n_min_x >= self.cols:
            return out
        n_max_x = min(self.cols - 1, int(math.ceil(f32(f32(f32(x - self.min_x) + r) * self.winv))))
        if n_max_x < 0:
            return out
        n_min_y = max(0, int(math.floor(f32(f32(f32(y - self.min_y) - r) * self.hinv))))
        if n_min_y >= self.rows:
            return out
        n_max_y = min(self.rows - 1, int(math.ceil(f32(f32(f32(y - self.min_y) + r) * self.hinv))))
        if n_max_y < 0:
            return out
        check_levels = (min_level > 0) or (max_level >= 0)
        for ix in range(n_min_x, n_max_x + 1):
            for iy in range(n_min_y, n_max_y + 1):
                for j in self.cells.get((ix, iy), ()):
                    if check_levels:
                        if g["octave"][j] < min_level:
                            continue
                        if max_level >= 0 and g["octave"][j] > max_level:
                            continue
                    distx = f32(g["x"][j]) - x
                    disty = f32(g["y"][j]) - y
                    if abs(distx) < r and abs(disty) < r:
                        out.append(j)
        return out


# ---- the vocabulary walk shared by the three BoW searches -----------------------------------------------------------------

def _common_nodes(fv1, fv2):
    """the while loop over two FeatureVectors (:244-402): the (slice1, slice2) of every node id both hold; lower_bound on a
    std::map is the first id not less than the key"""
    n1, o1, _ = fv1
    n2, o2, _ = fv2
    a = b = 0
    while a < len(n1) and b < len(n2):
        if n1[a] == n2[b]:
            yield (int(o1[a]), int(o1[a + 1])), (int(o2[b]), int(o2[b + 1]))
            a += 1; b += 1
        elif n1[a] < n2[b]:
            a = int(np.searchsorted(n1, n2[b], side="left"))
        else:
            b = int(np.searchsorted(n2, n1[a], side="left"))


def search_by_bow(dKF, validKF, angKF, fvKF, dF, angF, fvF, nnratio=0.7, check_ori=True):
    """SearchByBoW(KeyFrame*, Frame&, vpMapPointMatches) (:223-425), F.Nleft == -1: (nmatches, match[nF] = KF feature or -1)"""
    match = np.full(len(dF), -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for (k0, k1), (f0, f1) in _common_nodes(fvKF, fvF):
        for real_kf in fvKF[2][k0:k1]:
            real_kf = int(real_kf)
            if not validKF[real_kf]:                                   # !pMP || pMP->isBad() (:257-261)
                continue
            best1, best_f, best2 = 256, -1, 256
            for real_f in fvF[2][f0:f1]:
                real_f = int(real_f)
                if match[real_f] >= 0:                                 # :278
                    continue
                dist = hamming(dKF[real_kf], dF[real_f])
                if dist < best1:
                    best2 = best1; best1 = dist; best_f = real_f
                elif dist < best2:
                    best2 = dist
            if best1 <= TH_LOW:                                        # :327
                if f32(best1) < f32(nnratio) * f32(best2):             # :329
                    match[best_f] = real_kf
                    if check_ori:
                        hist[rot_bin(angKF[real_kf], angF[best_f])].append(best_f)
                    nmatches += 1
    if check_ori:
        for j in _drop_bins(hist):
            match[j] = -1
            nmatches -= 1
    return nmatches, match


def search_by_bow_kfkf(d1, valid1, ang1, fv1, d2, valid2, ang2, fv2, nnratio=0.7, check_ori=True):
    """SearchByBoW(KeyFrame*, KeyFrame*, vpMatches12) (:765-905): (nmatches, match12[n1] = feature of KF2 or -1)"""
    match12 = np.full(len(d1), -1, np.int32)
    matched2 = np.zeros(len(d2), bool)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for (a0, a1), (b0, b1) in _common_nodes(fv1, fv2):
        for idx1 in fv1[2][a0:a1]:
            idx1 = int(idx1)
            if not valid1[idx1]:                                       # :805-808
                continue
            best1, best_idx2, best2 = 256, -1, 256
            for idx2 in fv2[2][b0:b1]:
                idx2 = int(idx2)
                if matched2[idx2] or not valid2[idx2]:                 # :826-830
                    continue
                dist = hamming(d1[idx1], d2[idx2])
                if dist < best1:
                    best2 = best1; best1 = dist; best_idx2 = idx2
                elif dist < best2:
                    best2 = dist
            if best1 < TH_LOW:                                         # :848, strict
                if f32(best1) < f32(nnratio) * f32(best2):             # :850
                    match12[idx1] = best_idx2
                    matched2[best_idx2] = True
                    if check_ori:
                        hist[rot_bin(ang1[idx1], ang2[best_idx2])].append(idx1)
                    nmatches += 1
    if check_ori:
        for i in _drop_bins(hist):
            match12[i] = -1
            nmatches -= 1
    return nmatches, match12


def search_for_triangulation(k1, k2, ep, F12, sigma2_2, scale_2, only_stereo, coarse, check_ori):
    """SearchForTriangulation (:907-1146) with Pinhole::epipolarConstrain (Pinhole.cpp:107-129); F12(r, c) = F12[3*r + c].
    vbMatched2 is never set in the reference's loop, so a feature of KF2 may serve several of KF1."""
    n1 = len(k1["x"])
    match12 = np.full(n1, -1, np.int32)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    F = np.asarray(F12, np.float32)
    for (a0, a1), (b0, b1) in _common_nodes(k1["fv"], k2["fv"]):
        for idx1 in k1["fv"][2][a0:a1]:
            idx1 = int(idx1)
            if k1["has_mp"][idx1]:                                     # :974
                continue
            stereo1 = bool(k1["stereo"][idx1])                         # mvuRight[idx1]>=0
            if only_stereo and not stereo1:
                continue
            best_dist, best_idx2 = TH_LOW, -1                          # :994
            for idx2 in k2["fv"][2][b0:b1]:
                idx2 = int(idx2)
                if k2["has_mp"][idx2]:                                 # :1004
                    continue
                stereo2 = bool(k2["stereo"][idx2])
                if only_stereo and not stereo2:
                    continue
                dist = hamming(k1["desc"][idx1], k2["desc"][idx2])
                if dist > TH_LOW or dist > best_dist:                  # :1017
                    continue
                x2, y2, o2 = f32(k2["x"][idx2]), f32(k2["y"][idx2]), int(k2["octave"][idx2])
                if not stereo1 and not stereo2:                        # :1026-1034
                    distex = f32(ep[0]) - x2
                    distey = f32(ep[1]) - y2
                    if f32(f32(distex * distex) + f32(distey * distey)) < f32(100) * f32(scale_2[o2]):
                        continue
                ok = bool(coarse)
                if not ok:
                    x1, y1 = f32(k1["x"][idx1]), f32(k1["y"][idx1])
                    a = f32(f32(f32(x1 * F[0]) + f32(y1 * F[3])) + F[6])
                    b = f32(f32(f32(x1 * F[1]) + f32(y1 * F[4])) + F[7])
                    c = f32(f32(f32(x1 * F[2]) + f32(y1 * F[5])) + F[8])
                    num = f32(f32(f32(a * x2) + f32(b * y2)) + c)
                    den = f32(f32(a * a) + f32(b * b))
                    if den != 0:
                        dsqr = f32(f32(num * num) / den)
                        ok = float(dsqr) < 3.84 * float(f32(sigma2_2[o2]))
                if ok:
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


# ---- searches over the grid ----------------------------------------------------------------------------------------------

def search_by_projection_kf(g, dF, angF, scale, pts, th, orb_dist, check_ori, assign, occupied):
    """SearchByProjection(Frame&, KeyFrame*, sAlreadyFound, th, ORBdist) (:1889-2010); pts["valid"] stands for :1908-1910 and
    :1931, (u, v, level) for project() and PredictScale.  assign / occupied are CurrentFrame.mvpMapPoints, in and out."""
    grid = Grid(g)
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i in range(len(pts["u"])):
        if not pts["valid"][i]:
            continue
        u, v = f32(pts["u"][i]), f32(pts["v"][i])
        if u < grid.min_x or u > grid.max_x:                           # :1918
            continue
        if v < grid.min_y or v > grid.max_y:                           # :1920
            continue
        lvl = int(pts["level"][i])
        radius = f32(th) * f32(scale[lvl])                             # :1937
        best_dist, best_idx2 = 256, -1
        for i2 in grid.features_in_area(u, v, radius, lvl - 1, lvl + 1):
            if occupied[i2]:                                           # :1952
                continue
            dist = hamming(pts["desc"][i], dF[i2])
            if dist < best_dist:
                best_dist = dist; best_idx2 = i2
        if best_dist <= int(orb_dist):                                 # :1966
            assign[best_idx2] = i; occupied[best_idx2] = 1
            nmatches += 1
            if check_ori:
                hist[rot_bin(pts["angle"][i], angF[best_idx2])].append(best_idx2)
    if check_ori:
        for j in _drop_bins(hist):
            assign[j] = -1; occupied[j] = 0
            nmatches -= 1
    return nmatches


def search_by_projection_sim3(g, dKF, scale, pts, th, ratio_hamming, assign, occupied):
    """SearchByProjection(KeyFrame*, Sim3f&, vpPoints, vpMatched, th, ratioHamming) (:427-532); pts["valid"] stands for the
    prelude :451-484.  th is an int, TH_LOW*ratioHamming a float."""
    grid = Grid(g)
    nmatches = 0
    for i in range(len(pts["u"])):
        if not pts["valid"][i]:
            continue
        lvl = int(pts["level"][i])
        radius = f32(int(th)) * f32(scale[lvl])                        # :489
        best_dist, best_idx = 256, -1
        for idx in grid.features_in_area(pts["u"][i], pts["v"][i], radius):
            if occupied[idx]:                                          # :504
                continue
            kp_level = int(g["octave"][idx])
            if kp_level < lvl - 1 or kp_level > lvl:                   # :509
                continue
            dist = hamming(pts["desc"][i], dKF[idx])
            if dist < best_dist:
                best_dist = dist; best_idx = idx
        if f32(best_dist) <= f32(TH_LOW) * f32(ratio_hamming):         # :523
            assign[best_idx] = i; occupied[best_idx] = 1
            nmatches += 1
    return nmatches


def fuse_search(g, dKF, scale, u_right, inv_sigma2, pts, th, chi2_check=True):
    """The search core of Fuse(KeyFrame*, vpMapPoints, th, bRight=false) (:1148-1338, chi2_check) and of
    Fuse(KeyFrame*, Sim3f&, vpPoints, th, vpReplacePoint) (:1340-1455): (bestIdx, bestDist) per point, (-1, 256) where no
    candidate is left.  The second overload starts bestDist at INT_MAX (:1415) where the first starts at 256 (:1258); the
    two differ only for a candidate at distance 256, which neither fuses (`bestDist<=TH_LOW`), and the flattened interface
    reports the first overload's (-1, 256) for both."""
    grid = Grid(g)
    n = len(pts["u"])
    best_i = np.full(n, -1, np.int32); best_d = np.full(n, 256, np.int32)
    for i in range(n):
        if not pts["valid"][i]:
            continue
        lvl = int(pts["level"][i])
        u, v = f32(pts["u"][i]), f32(pts["v"][i])
        radius = f32(th) * f32(scale[lvl])                             # :1244
        best_dist, best_idx = 256, -1
        for idx in grid.features_in_area(u, v, radius):
            kp_level = int(g["octave"][idx])
            if kp_level < lvl - 1 or kp_level > lvl:                   # :1269
                continue
            if chi2_check:
                kpx, kpy = f32(g["x"][idx]), f32(g["y"][idx])
                ex = u - kpx
                ey = v - kpy
                if u_right[idx] >= 0:                                  # :1272
                    er = f32(pts["ur"][i]) - f32(u_right[idx])
                    e2 = f32(f32(f32(ex * ex) + f32(ey * ey)) + f32(er * er))
                    if float(f32(e2 * f32(inv_sigma2[kp_level]))) > 7.8:       # :1283
                        continue
                else:
                    e2 = f32(f32(ex * ex) + f32(ey * ey))
                    if float(f32(e2 * f32(inv_sigma2[kp_level]))) > 5.99:      # :1294
                        continue
            dist = hamming(pts["desc"][i], dKF[idx])
            if dist < best_dist:                                       # :1304
                best_dist = dist; best_idx = idx
        best_i[i] = best_idx; best_d[i] = best_dist
    return best_i, best_d


def search_for_initialization(f1, g2, d2, ang2, window_size, nnratio, check_ori):
    """SearchForInitialization (:648-763): (nmatches, vnMatches12)"""
    grid = Grid(g2)
    n1, n2 = len(f1["octave"]), len(g2["x"])
    match12 = np.full(n1, -1, np.int32)
    matched_distance = [INT_MAX] * n2
    match21 = [-1] * n2
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i1 in range(n1):
        level1 = int(f1["octave"][i1])
        if level1 > 0:                                                 # :665
            continue
        best_dist, best_dist2, best_idx2 = INT_MAX, INT_MAX, -1
        for i2 in grid.features_in_area(f1["prev_x"][i1], f1["prev_y"][i1], f32(int(window_size)), level1, level1):
            dist = hamming(f1["desc"][i1], d2[i2])
            if matched_distance[i2] <= dist:                           # :687
                continue
            if dist < best_dist:
                best_dist2 = best_dist; best_dist = dist; best_idx2 = i2
            elif dist < best_dist2:
                best_dist2 = dist
        if best_dist <= TH_LOW:                                        # :702
            if f32(best_dist) < f32(best_dist2) * f32(nnratio):        # :704
                if match21[best_idx2] >= 0:
                    match12[match21[best_idx2]] = -1
                    nmatches -= 1
                match12[i1] = best_idx2
                match21[best_idx2] = i1
                matched_distance[best_idx2] = best_dist
                nmatches += 1
                if check_ori:
                    hist[rot_bin(f1["angle"][i1], ang2[best_idx2])].append(i1)
    if check_ori:
        for idx1 in _drop_bins(hist):
            if match12[idx1] >= 0:                                     # :747
                match12[idx1] = -1
                nmatches -= 1
    return nmatches, match12
