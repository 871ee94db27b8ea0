"""Numpy restatements of the two tracking searches for a two-camera fisheye rig frame (F.Nleft != -1), written from the
reference text (src/ORBmatcher.cc:43-213 and :1676-1887, Frame::GetFeaturesInArea src/Frame.cc:744-810) and from nothing
else: not from oracle/ (which has no rig branch) and not from the kernels.  A test helper, not a test.

Plain loops, one Grid per side (mGrid over mvKeys, mGridRight over mvKeysRight), ONE slot array: left slots first, right
slot j at Nleft + j.  A rig is dict(left, right (grid dicts with "desc" and "angle"), scale, left_to_right, right_to_left);
the point dicts carry the arrays of OrbmRigMapPoints / OrbmRigLastPoints under the names of the C struct.

`stats`, when given, counts the events the seeded random set must contain (tests/test_rig_match_reference.py)."""
import numpy as np

from matcher_reference import Grid, hamming, rot_bin, three_maxima, TH_HIGH, HISTO_LENGTH

f32 = np.float32


def _radius_by_viewing_cos(view_cos):
    """:215-221: `viewCos>0.998` compares a float with a double literal"""
    return f32(2.5) if float(f32(view_cos)) > 0.998 else f32(4.0)


def _best_two(idxs, octave, desc, d, occupied, slot0):
    """the candidate loops :84-120 / :164-190: (bestDist, bestLevel, bestDist2, bestLevel2, bestIdx)"""
    best = best2 = 256
    lev = lev2 = -1
    bi = -1
    for idx in idxs:
        if occupied[slot0 + idx]:
            continue
        dist = hamming(d, desc[idx])
        if dist < best:
            best2 = best; best = dist; lev2 = lev; lev = int(octave[idx]); bi = int(idx)
        elif dist < best2:
            lev2 = int(octave[idx]); best2 = dist
    return best, lev, best2, lev2, bi


def _bump(stats, key):
    if stats is not None:
        stats[key] = stats.get(key, 0) + 1


def numpy_search_mp_rig(rig, mp, th, nnratio, assign, occupied, far_points=False, th_far=0.0, stats=None):
    """SearchByProjection(Frame& F, const vector<MapPoint*>&, th, bFarPoints, thFarPoints), F.Nleft != -1 (:43-213)"""
    L, R = rig["left"], rig["right"]
    gl, gr = Grid(L), Grid(R)
    scale = rig["scale"]
    nl = len(L["x"])
    l2r, r2l = rig["left_to_right"], rig["right_to_left"]
    nmatches = 0
    b_factor = float(f32(th)) != 1.0                                   # :47
    for i in range(int(mp.get("n", len(mp["proj_u"])))):
        if not mp["in_view"][i] and not mp["in_view_r"][i]:            # :52
            continue
        if far_points and f32(mp["track_depth"][i]) > f32(th_far):     # :55
            continue
        if mp["bad"][i]:                                               # :58
            continue
        ho = mp["has_obs"][i]
        d = mp["desc"][i]
        wrote_partner = -1
        occ_before = None
        if mp["in_view"][i]:                                           # :61
            lvl = int(mp["pred_level"][i])
            r = _radius_by_viewing_cos(mp["view_cos"][i])
            if b_factor:
                r = f32(r * f32(th))
            idxs = gl.features_in_area(mp["proj_u"][i], mp["proj_v"][i], f32(r * f32(scale[lvl])), lvl - 1, lvl)
            if idxs:                                                   # :74
                best, lev, best2, lev2, bi = _best_two(idxs, L["octave"], L["desc"], d, occupied, 0)
                if best <= TH_HIGH:                                    # :123
                    if lev == lev2 and f32(best) > f32(nnratio) * f32(best2):      # :125-126: continue -- the right pass goes with it
                        if mp["in_view_r"][i] and int(mp["pred_level_r"][i]) != -1:
                            _bump(stats, "right_cancelled_by_left_ratio")
                        continue
                    assign[bi] = i; occupied[bi] = ho                  # :129
                    if l2r[bi] != -1:                                  # :131-135
                        wrote_partner = int(l2r[bi])
                        occ_before = occupied[nl + wrote_partner]
                        assign[nl + wrote_partner] = i; occupied[nl + wrote_partner] = ho
                        nmatches += 1
                        _bump(stats, "partner_l2r")
                    nmatches += 1
                    _bump(stats, "left")
        if mp["in_view_r"][i]:                                         # :144
            lvl = int(mp["pred_level_r"][i])
            if lvl != -1:                                              # :146
                r = _radius_by_viewing_cos(mp["view_cos_r"][i])        # :147: th is not applied
                idxs = gr.features_in_area(mp["proj_u_r"][i], mp["proj_v_r"][i], f32(r * f32(scale[lvl])), lvl - 1, lvl)
                if not idxs:                                           # :152
                    continue
                if stats is not None and wrote_partner >= 0 and ho and not occ_before:
                    was = occupied.copy(); was[nl + wrote_partner] = 0
                    if _best_two(idxs, R["octave"], R["desc"], d, was, nl)[4] == wrote_partner:
                        _bump(stats, "right_research")
                best, lev, best2, lev2, bi = _best_two(idxs, R["octave"], R["desc"], d, occupied, nl)
                if best <= TH_HIGH:                                    # :193
                    if lev == lev2 and f32(best) > f32(nnratio) * f32(best2):      # :195
                        continue
                    if r2l[bi] != -1:                                  # :198-202
                        assign[int(r2l[bi])] = i; occupied[int(r2l[bi])] = ho
                        nmatches += 1
                        _bump(stats, "partner_r2l")
                    assign[nl + bi] = i; occupied[nl + bi] = ho        # :205
                    nmatches += 1
                    _bump(stats, "right")
    return nmatches


def _level_window(lw, octave):
    """:1728-1733: bForward -> (octave, -1), bBackward -> (0, octave), else (octave-1, octave+1)"""
    return {0: (octave - 1, octave + 1), 1: (octave, -1), 2: (0, octave)}[int(lw)]


def numpy_search_last_rig(rig, last, th, check_ori, assign, occupied, stats=None):
    """SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono), CurrentFrame.Nleft != -1 (:1676-1887);
    last["valid"] stands for :1698-1711, proj_* for the two project() calls, level_window for bForward / bBackward"""
    L, R = rig["left"], rig["right"]
    gl, gr = Grid(L), Grid(R)
    scale = rig["scale"]
    nl = len(L["x"])
    lw = int(last.get("level_window", 0))
    hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for i in range(int(last.get("n", len(last["proj_u"])))):
        if not last["valid"][i]:
            continue
        u, v = f32(last["proj_u"][i]), f32(last["proj_v"][i])
        if u < gl.min_x or u > gl.max_x:                               # :1715
            continue
        if v < gl.min_y or v > gl.max_y:                               # :1717
            continue
        octave = int(last["octave"][i])
        radius = f32(f32(th) * f32(scale[octave]))                     # :1724
        lo, hi = _level_window(lw, octave)
        idxs = gl.features_in_area(u, v, radius, lo, hi)
        if not idxs:                                                   # :1735
            _bump(stats, "right_cancelled_by_empty_window")
            continue
        d = last["desc"][i]
        ho = last["has_obs"][i]
        best, bi = 256, -1
        for i2 in idxs:                                                # :1743-1768
            if occupied[i2]:
                continue
            dist = hamming(d, L["desc"][i2])
            if dist < best:
                best = dist; bi = i2
        if best <= TH_HIGH:                                            # :1770
            assign[bi] = i; occupied[bi] = ho
            nmatches += 1
            _bump(stats, "left")
            if check_ori:
                hist[rot_bin(last["angle"][i], L["angle"][bi])].append(bi)
        # :1794-1859: always, once the left window was not empty; no bounds test, no empty-window exit
        idxs = gr.features_in_area(last["proj_u_r"][i], last["proj_v_r"][i], radius, lo, hi)
        best, bi = 256, -1
        for i2 in idxs:
            if occupied[nl + i2]:
                continue
            dist = hamming(d, R["desc"][i2])
            if dist < best:
                best = dist; bi = i2
        if best <= TH_HIGH:                                            # :1836
            assign[nl + bi] = i; occupied[nl + bi] = ho
            nmatches += 1
            _bump(stats, "right")
            if check_ori:
                hist[rot_bin(last["angle"][i], R["angle"][bi])].append(nl + bi)
    if check_ori:                                                      # :1865-1884: ONE histogram over both sides
        keep = three_maxima([len(h) for h in hist])
        for b in range(HISTO_LENGTH):
            if b not in keep:
                for slot in hist[b]:
                    assign[slot] = -1; occupied[slot] = 0
                    nmatches -= 1
                    _bump(stats, "drop_left" if slot < nl else "drop_right")
    return nmatches
