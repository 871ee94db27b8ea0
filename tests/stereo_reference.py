"""Frame::ComputeStereoMatches (reference src/Frame.cc:931-1101) restated in numpy, one key point at a time.  A test helper, not a
test.  Written from the reference source: every arithmetic step is an np.float32 operation in the reference's order and with its
mixed types (float against int compares, the two double literals of the clamp), so that the result can be compared bit for bit.

What the reference leaves undefined, and what this project does there (oracle and kernel follow the same contracts):

* A correlation window that leaves the level image.  cv::Mat::rowRange / colRange assert there.  The kernel gives that left key
  point no match and goes on; the oracle gives up on the whole call and returns -2.  Here: outcome OFF_LEVEL, no match.  The left
  window (:1028) is cut before the test against the right edge (:1038), the right windows (:1043) after it, so a left window off
  the level is OFF_LEVEL whatever the right edge says.  A left octave that the pyramid does not have is OFF_LEVEL as well when a
  candidate passes the descriptor gate (there is no level image at all).
* No accepted match at all.  The reference would read vDistIdx[0] of an empty vector.  Oracle and kernel leave every output as it
  is (-1); so does this.
* A row band of a right key point that leaves 0..rows-1.  The reference indexes vRowIndices unchecked; the rows that exist are
  filled, the others dropped.

`if (maxU < 0) continue` (:984) cannot change a result for uL >= 0: maxU == uL - 0.0f == uL.  The kernel has no such test and
relies on it; every case keeps uL >= 0 and 0 <= (int)vL < rows.

Outcome codes, one per left key point: see OUTCOMES."""
import numpy as np

F = np.float32

OUTCOMES = ("no_candidate",               # no right key point passed the row band, the octave window and the disparity window
            "orb_distance",               # some did, but the best descriptor distance is >= 75 (those >= 100 never become the best)
            "window_past_right_edge",     # endu >= cols of the level
            "off_level",                  # the contract above
            "best_shift_at_end",          # the first SAD minimum lies at shift -5 or +5
            "disparity_out_of_range",     # the |deltaR| > 1 gate, or not (0 <= disparity < maxD)
            "accepted",
            "accepted_clamped",           # disparity <= 0 became 0.01
            "cut_by_median")
(NO_CANDIDATE, ORB_DISTANCE, WINDOW_PAST_RIGHT_EDGE, OFF_LEVEL, BEST_SHIFT_AT_END, DISPARITY_OUT_OF_RANGE, ACCEPTED, ACCEPTED_CLAMPED,
 CUT_BY_MEDIAN) = range(len(OUTCOMES))

TH_HIGH, TH_LOW = 100, 50                 # ORBmatcher::TH_HIGH / TH_LOW
INT_MAX = 2 ** 31 - 1

_POP = np.array([bin(i).count("1") for i in range(256)], np.int32)


def descriptor_distance(a, b):
    """ORBmatcher::DescriptorDistance: the number of differing bits of two 32-byte descriptors"""
    return int(_POP[np.bitwise_xor(a, b)].sum())


def c_round(x):
    """round() of a float: to the nearest integer, halves away from zero (np.round / rint go to even).  The sum is taken in
    float64, where |x| + 0.5 is exact for every float32 below 2^52"""
    x = F(x)
    return F(np.copysign(np.floor(np.abs(np.float64(x)) + 0.5), np.float64(x)))


def c_int(x):
    """(int) of a float: truncation towards zero"""
    return int(np.trunc(np.float64(x)))


def _sad(il, ir):
    """cv::norm(IL, IR, NORM_L1) of two 8-bit windows: an exact integer, returned as the float the reference stores"""
    return F(int(np.abs(il.astype(np.int32) - ir.astype(np.int32)).sum()))


def stereo_matches(levels_l, levels_r, scale, inv_scale, kps_l, desc_l, kps_r, desc_r, mb, mbf, round_fn=c_round):
    """levels_l / levels_r: mvImagePyramid of the left / right extractor (lists of uint8 images); scale / inv_scale: mvScaleFactors /
    mvInvScaleFactors (float32); kps: records with x, y, octave (mvKeys / mvKeysRight); desc: [n, 32] uint8; mb, mbf: floats.
    Returns dict(u_right, depth (float32, -1 where there is no match), sad (int32 best SAD of every match that reached the median
    cut, else -1), code (int8 index into OUTCOMES), best_r (the right index the descriptor search chose, else -1), shift (bestincR
    of those that got that far, else -99), dists (vDists of those), delta (deltaR, else nan), n_matches (the matches before the cut), uncut (the same dict
    before the median cut, for median_cut()).
    round_fn stands for the reference's round(); the case builders pass another rounding to show that it would be seen."""
    scale = np.asarray(scale, F); inv_scale = np.asarray(inv_scale, F)
    mb, mbf = F(mb), F(mbf)
    N, Nr = len(kps_l), len(kps_r)
    n_levels = len(levels_l)
    u_right = np.full(N, -1, F); depth = np.full(N, -1, F)
    sad = np.full(N, -1, np.int32); code = np.full(N, NO_CANDIDATE, np.int8)
    best_r = np.full(N, -1, np.int64); shift = np.full(N, -99, np.int32); delta = np.full(N, np.nan, F)
    dists = np.full((N, 11), -1, F)

    thOrbDist = (TH_HIGH + TH_LOW) // 2
    nRows = levels_l[0].shape[0]

    # assign key points to the row table (:941-958)
    vRowIndices = [[] for _ in range(nRows)]
    xr = np.asarray(kps_r["x"], F); yr = np.asarray(kps_r["y"], F); octr = np.asarray(kps_r["octave"], np.int64)
    for iR in range(Nr):
        kpY = yr[iR]
        r = F(F(2.0) * scale[octr[iR]])
        maxr = int(np.ceil(F(kpY + r)))
        minr = int(np.floor(F(kpY - r)))
        for yi in range(max(minr, 0), min(maxr, nRows - 1) + 1):
            vRowIndices[yi].append(iR)

    # limits of the search (:961-963)
    minZ = mb
    minD = F(0)
    maxD = F(mbf / minZ)

    vDistIdx = []
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for iL in range(N):
            levelL = int(kps_l["octave"][iL])
            vL = F(kps_l["y"][iL]); uL = F(kps_l["x"][iL])
            vCandidates = vRowIndices[c_int(vL)]
            if not vCandidates:
                continue
            minU = F(uL - maxD)
            maxU = F(uL - minD)
            if maxU < 0:
                continue
            bestDist = TH_HIGH
            bestIdxR = 0
            seen = False
            dL = desc_l[iL]
            for iR in vCandidates:
                if octr[iR] < levelL - 1 or octr[iR] > levelL + 1:
                    continue
                uR = xr[iR]
                if uR >= minU and uR <= maxU:
                    seen = True
                    dist = descriptor_distance(dL, desc_r[iR])
                    if dist < bestDist:
                        bestDist = dist
                        bestIdxR = iR
            if not seen:
                continue
            if not bestDist < thOrbDist:
                code[iL] = ORB_DISTANCE
                continue
            best_r[iL] = bestIdxR
            if levelL < 0 or levelL >= n_levels:
                code[iL] = OFF_LEVEL
                continue

            # sub-pixel match by correlation: coordinates in the image pyramid at the key point's scale (:1020-1024)
            uR0 = xr[bestIdxR]
            scaleFactor = inv_scale[levelL]
            scaleduL = round_fn(F(uL * scaleFactor))
            scaledvL = round_fn(F(vL * scaleFactor))
            scaleduR0 = round_fn(F(uR0 * scaleFactor))
            w = 5
            imL, imR = levels_l[levelL], levels_r[levelL]
            rows, cols = imL.shape
            y0, y1 = c_int(F(scaledvL - F(w))), c_int(F(F(scaledvL + F(w)) + F(1)))
            xl0, xl1 = c_int(F(scaleduL - F(w))), c_int(F(F(scaleduL + F(w)) + F(1)))
            if y0 < 0 or y1 > rows or xl0 < 0 or xl1 > cols:          # rowRange / colRange of IL (:1028)
                code[iL] = OFF_LEVEL
                continue
            IL = imL[y0:y1, xl0:xl1]
            bestDistS = INT_MAX
            bestincR = 0
            L = 5
            vDists = np.zeros(2 * L + 1, F)
            iniu = F(F(scaleduR0 + F(L)) - F(w))
            endu = F(F(F(scaleduR0 + F(L)) + F(w)) + F(1))
            if iniu < 0 or endu >= F(imR.shape[1]):
                code[iL] = WINDOW_PAST_RIGHT_EDGE
                continue
            off = False
            for incR in range(-L, L + 1):
                x0 = c_int(F(F(scaleduR0 + F(incR)) - F(w)))
                x1 = c_int(F(F(F(scaleduR0 + F(incR)) + F(w)) + F(1)))
                if x0 < 0 or x1 > imR.shape[1] or y1 > imR.shape[0]:
                    off = True
                    break
                dist = _sad(IL, imR[y0:y1, x0:x1])
                if dist < F(bestDistS):
                    bestDistS = c_int(dist)
                    bestincR = incR
                vDists[L + incR] = dist
            if off:
                code[iL] = OFF_LEVEL
                continue
            shift[iL] = bestincR
            dists[iL] = vDists
            if bestincR == -L or bestincR == L:
                code[iL] = BEST_SHIFT_AT_END
                continue

            # parabola fitting (:1059-1066)
            dist1 = vDists[L + bestincR - 1]
            dist2 = vDists[L + bestincR]
            dist3 = vDists[L + bestincR + 1]
            deltaR = F(F(dist1 - dist3) / F(F(2.0) * F(F(dist1 + dist3) - F(F(2.0) * dist2))))
            delta[iL] = deltaR
            if deltaR < -1 or deltaR > 1:
                code[iL] = DISPARITY_OUT_OF_RANGE
                continue

            # re-scaled coordinate (:1069-1083)
            bestuR = F(scale[levelL] * F(F(scaleduR0 + F(bestincR)) + deltaR))
            disparity = F(uL - bestuR)
            if disparity >= minD and disparity < maxD:
                code[iL] = ACCEPTED
                if disparity <= 0:
                    disparity = F(0.01)
                    bestuR = F(np.float64(uL) - 0.01)
                    code[iL] = ACCEPTED_CLAMPED
                depth[iL] = F(mbf / disparity)
                u_right[iL] = bestuR
                sad[iL] = bestDistS
                vDistIdx.append((bestDistS, iL))
            else:
                code[iL] = DISPARITY_OUT_OF_RANGE

    uncut = dict(u_right=u_right, depth=depth, sad=sad, code=code, best_r=best_r, shift=shift, delta=delta, dists=dists, n_matches=len(vDistIdx))
    res = median_cut(uncut)
    res["uncut"] = uncut
    return res


def median_cut(uncut, rank_shift=0):
    """the outlier cut of :1087-1100 on the matches of `uncut`; returns a new dict.  rank_shift moves the rank of the median (0 is
    the reference's size / 2); the case builders use it to show that a wrong rank would be seen."""
    res = {k: (v.copy() if isinstance(v, np.ndarray) else v) for k, v in uncut.items()}
    u_right, depth, code = res["u_right"], res["depth"], res["code"]
    vDistIdx = [(int(res["sad"][iL]), iL) for iL in range(len(code)) if code[iL] in (ACCEPTED, ACCEPTED_CLAMPED)]
    if vDistIdx:                                                       # (the reference reads vDistIdx[0] of an empty vector)
        vDistIdx.sort()
        rank = min(max(len(vDistIdx) // 2 + rank_shift, 0), len(vDistIdx) - 1)
        median = F(vDistIdx[rank][0])
        thDist = F(F(F(1.5) * F(1.4)) * median)
        for i in range(len(vDistIdx) - 1, -1, -1):
            if F(vDistIdx[i][0]) < thDist:
                break
            iL = vDistIdx[i][1]
            u_right[iL] = -1
            depth[iL] = -1
            code[iL] = CUT_BY_MEDIAN
    return res
