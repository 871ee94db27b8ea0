"""The calls of the rig SearchByBoW / SearchForTriangulation tests: hand-built calls with the outcome written next to them by hand,
shape calls and seeded random calls.  A test helper, not a test.  Everything is built once per process (functools.lru_cache): the
tests share the calls and the reference's results and must not modify them.

A BoW call is dict(dKF, validKF, angKF, fvKF, dF, n_left, angF, fvF); a triangulation call dict(kf1, kf2, geom, sigma2_1, sigma2_2)
with kf = dict(desc, has_mp, x, y, octave, angle, fv, n_left) -- what Matcher.search_by_bow_rig / search_for_triangulation_rig
take.  Feature vectors are (node ids, offsets, features) triples."""
import functools

import numpy as np

import fisheye_stereo_cases as fsc
import rig_bow_reference as ref

NNRATIO = 0.6
LEVEL_SIGMA2 = fsc.LEVEL_SIGMA2


# ------------------------------------------------------------------------------------------------ descriptors and feature vectors
def base_desc(seed):
    return np.random.RandomState(1000 + seed).randint(0, 256, 32).astype(np.uint8)


def at(base, k, start=0):
    """`base` with the k bits start .. start + k - 1 flipped: at(b, i) and at(b, j) are |i - j| apart"""
    bits = np.unpackbits(np.asarray(base, np.uint8))
    bits[start:start + k] ^= 1
    return np.packbits(bits)


def make_fv(nodes):
    """{node id: [features in insertion order]} -> (node ids ascending, offsets, features)"""
    ids = sorted(nodes)
    off = np.zeros(len(ids) + 1, np.int32)
    feat = []
    for i, k in enumerate(ids):
        feat += list(nodes[k])
        off[i + 1] = len(feat)
    return np.array(ids, np.uint32), off, np.array(feat, np.uint32)


def bow_call(kf, frame, n_left, node_kf, node_f, ang_kf=None, ang_f=None, valid=None):
    """kf / frame: lists of descriptors; node_kf / node_f: {node: [indices]}"""
    dKF = np.array(kf, np.uint8).reshape(-1, 32); dF = np.array(frame, np.uint8).reshape(-1, 32)
    return dict(dKF=dKF, validKF=np.ones(len(dKF), np.uint8) if valid is None else np.array(valid, np.uint8),
                angKF=np.zeros(len(dKF), np.float32) if ang_kf is None else np.array(ang_kf, np.float32), fvKF=make_fv(node_kf),
                dF=dF, n_left=int(n_left), angF=np.zeros(len(dF), np.float32) if ang_f is None else np.array(ang_f, np.float32), fvF=make_fv(node_f))


# ------------------------------------------------------------------------------------------------ hand-built SearchByBoW calls
@functools.lru_cache(maxsize=None)
def bow_hand_cases():
    """name -> dict(call, nnratio, check_ori, want_n, want_match): the outcome is written by hand from the reference's text.  All
    key-frame features of a case share one descriptor B, a frame feature at(B, k) is k bits from each of them."""
    B = base_desc(1)
    C = {}

    def case(name, call, want_match, nnratio=NNRATIO, check_ori=False):
        want = np.array(want_match, np.int32)
        C[name] = dict(call=call, nnratio=nnratio, check_ori=check_ori, want_match=want, want_n=int((want >= 0).sum()))

    one = {7: [0]}
    # the left best is 51: :327 fails, the right candidate at distance 0 is never looked at
    case("left_51_right_0", bow_call([B], [at(B, 51), at(B, 0)], 1, one, {7: [0, 1]}), [-1, -1])
    # the node holds no left candidate (the frame's left feature sits in a node the key frame does not have): bestDist1 stays 256
    case("no_left_candidate", bow_call([B], [at(B, 3), at(B, 0)], 1, one, {7: [1], 9: [0]}), [-1, -1])
    # ... nor with n_left = 0: every candidate is a right one
    case("n_left_zero", bow_call([B], [at(B, 0), at(B, 2)], 0, one, {7: [0, 1]}), [-1, -1])
    # key-frame feature 0 takes the only left slot and right slot 1; for feature 1 the left side is consumed (best1 = 256), so
    # right slot 2 at distance 1 is ignored
    case("left_consumed", bow_call([B, B], [at(B, 5), at(B, 0), at(B, 1)], 1, {7: [0, 1]}, {7: [0, 1, 2]}), [0, 0, -1])
    # the issue's figures: best1 = 30, best2 = 50, nnratio = 0.6.  In float 0.6f * 50.f = 30.000002 (0.6f is 0.60000002), so
    # 30 < 30.000002 holds and the LEFT slot is written too: the count is 2 ...
    case("ratio_30_50_at_0.6", bow_call([B], [at(B, 30), at(B, 50), at(B, 10)], 2, one, {7: [0, 1, 2]}), [0, -1, 0])
    # ... and an exact float equality: 25 < 0.5f * 50.f = 25 fails while best1 <= TH_LOW: only the right slot is written, count 1
    case("ratio_equal_right_only", bow_call([B], [at(B, 25), at(B, 50), at(B, 10)], 2, one, {7: [0, 1, 2]}), [-1, -1, 0], nnratio=0.5)
    # 31 < 30.000002 fails: right only as well
    case("ratio_31_50_at_0.6", bow_call([B], [at(B, 31), at(B, 50), at(B, 10)], 2, one, {7: [0, 1, 2]}), [-1, -1, 0])
    # two equally distant right candidates (7 bits each, different bits): the first is written, no ratio test; with the left: 2
    case("two_equal_right", bow_call([B], [at(B, 4), at(B, 7), at(B, 7, start=100)], 1, one, {7: [0, 1, 2]}), [0, 0, -1])
    # left 2 and 3 fail the ratio for both key-frame features (2 < 0.6 * 3 is false): the left side stays untouched; feature 0 takes
    # right slot 2 (1 bit), which feature 1 does not see any more: it takes slot 3 (6 bits)
    case("right_taken_next", bow_call([B, B], [at(B, 2), at(B, 3), at(B, 1), at(B, 6)], 2, {7: [0, 1]}, {7: [0, 1, 2, 3]}), [-1, -1, 0, 1])
    # a right candidate (5) closer than every left one (20, 40) does not enter the left top-2: left 20 < 0.6 * 40 is written, right 5 too
    # (had it entered: best1 = 5 at slot 2, slot 0 unwritten)
    case("right_not_in_left_top2", bow_call([B], [at(B, 20), at(B, 40), at(B, 5)], 2, one, {7: [2, 0, 1]}), [0, -1, 0])
    # the converse: the left 5 does not enter the right side, whose best is 30 at slot 2
    case("left_not_in_right", bow_call([B], [at(B, 5), at(B, 45), at(B, 30)], 2, one, {7: [0, 2, 1]}), [0, -1, 0])
    # the right 11 is no second best of the left side: with it the left 10 would fail the ratio (10 < 0.6 * 11 is false); the left best
    # stands alone (second 256) and is written, the right 11 too
    case("right_not_left_second", bow_call([B], [at(B, 10), at(B, 11), at(B, 40)], 1, one, {7: [0, 1, 2]}), [0, 0, -1])
    # TH_LOW on each side: 50 is accepted, 51 is not
    case("left_50_right_50", bow_call([B], [at(B, 50), at(B, 50, start=100)], 1, one, {7: [0, 1]}), [0, 0])
    case("left_51_right_50", bow_call([B], [at(B, 51), at(B, 50, start=100)], 1, one, {7: [0, 1]}), [-1, -1])
    case("left_10_right_51", bow_call([B], [at(B, 10), at(B, 51)], 1, one, {7: [0, 1]}), [0, -1])
    # an invalid key-frame feature (no map point) is skipped, the next one matches
    case("invalid_kf_feature", bow_call([B, B], [at(B, 1), at(B, 2)], 1, {7: [0, 1]}, {7: [0, 1]}, valid=[0, 1]), [1, 1])
    # ONE histogram: nodes 0 .. 5 give left matches in bins 0, 0, 1, 1, 2, 2; node 6 a left match in bin 0 and a right match in bin 3.
    # Combined: 3, 2, 2, 1 -- bin 3 is not among the three maxima and the right match is dropped (count 7).  A histogram of the right
    # side alone would hold bin 3 only and keep it.
    kf, fr, nkf, nf = [], [], {}, {}
    ang_kf = [0, 0, 30, 30, 60, 60, 90]
    for i in range(7):
        Bi = base_desc(10 + i)
        kf.append(Bi); fr.append(at(Bi, 3)); nkf[i] = [i]; nf[i] = [i]
    fr.append(at(base_desc(16), 2)); nf[6] = [6, 7]
    ang_f = [0, 0, 0, 0, 0, 0, 90, 0]
    case("one_histogram", bow_call(kf, fr, 7, nkf, nf, ang_kf, ang_f), [0, 1, 2, 3, 4, 5, 6, -1], check_ori=True)
    # the same without orientation checking keeps it
    case("one_histogram_off", bow_call(kf, fr, 7, nkf, nf, ang_kf, ang_f), [0, 1, 2, 3, 4, 5, 6, 6])
    return C


# ------------------------------------------------------------------------------------------------ shapes and random SearchByBoW calls
def random_bow_call(seed, n_kf, n_f, n_left, n_nodes, big_nodes=()):
    """frame features are noisy copies (0 .. 69 bits) of key-frame features, mostly in the copied feature's node; angles mostly
    agree up to a common rotation.  big_nodes: (node, n_frame_features, n_kf_features) forced sizes, taken from the front."""
    rs = np.random.RandomState(seed)
    dKF = rs.randint(0, 256, (n_kf, 32)).astype(np.uint8)
    node_kf = rs.randint(0, max(n_nodes, 1), n_kf) * 3
    src = rs.randint(0, max(n_kf, 1), n_f)
    dF = np.zeros((n_f, 32), np.uint8)
    node_f = np.zeros(n_f, np.int64)
    for j in range(n_f):
        if n_kf:
            dF[j] = fsc.flip_bits(rs, dKF[src[j]], rs.randint(0, 70))
            node_f[j] = node_kf[src[j]] if rs.rand() < 0.85 else rs.randint(0, max(n_nodes, 1)) * 3 + rs.randint(0, 2)
        else:
            dF[j] = rs.randint(0, 256, 32)
    kf_pos = f_pos = 0
    for node, nf_, nk_ in big_nodes:
        node_f[f_pos:f_pos + nf_] = node; f_pos += nf_
        node_kf[kf_pos:kf_pos + nk_] = node; kf_pos += nk_
    order_f = rs.permutation(n_f)               # which slot a frame feature gets: the sides are mixed inside every node
    slot = np.empty(n_f, np.int64); slot[order_f] = np.arange(n_f)
    dF2 = np.zeros_like(dF); dF2[slot] = dF
    angKF = rs.uniform(0, 360, n_kf).astype(np.float32)
    angF = np.zeros(n_f, np.float32)
    for j in range(n_f):
        a = (angKF[src[j]] if n_kf else 0.0) - 40.0 + rs.normal(0, 8) if rs.rand() < 0.8 else rs.uniform(0, 360)
        angF[slot[j]] = np.float32(a % 360.0)
    nodes_kf, nodes_f = {}, {}
    for i in rs.permutation(n_kf):
        nodes_kf.setdefault(int(node_kf[i]), []).append(int(i))
    for j in rs.permutation(n_f):
        nodes_f.setdefault(int(node_f[j]), []).append(int(slot[j]))
    valid = (rs.rand(n_kf) < 0.9).astype(np.uint8)
    return dict(dKF=dKF, validKF=valid, angKF=angKF, fvKF=make_fv(nodes_kf), dF=dF2, n_left=int(n_left), angF=angF, fvF=make_fv(nodes_f))


NODE_SIZES = (1, 16, 17, 32, 33, 64, 65, 96, 97, 513)
KF_NODE_SIZES = (1, 16, 17)


def splits(n):
    """the numbers of left features a frame node of n features is given: every one for the sizes up to 97 (all the register forms and the
    memory form at its smallest).  For 513 (the one-lane form, which runs the reference's loops as they are written and owns no lanes)
    every split would be 514 nodes of 513 features -- 264 k descriptors to build and 2.9 M distances in the Python reference, beyond the
    few seconds a test may take --, so the left counts are the multiples of 31 (31 = -1 mod 16: seventeen counts that visit every residue
    modulo the 16 lanes of a group) and the two counts next to either end."""
    if n <= 97:
        return list(range(n + 1))
    return sorted(set(range(0, n + 1, 31)) | {0, 1, n - 1, n})


def node_split_call(n, seed=0):
    """one node per split of a frame node of n features (left features first in the slot array, mixed in node order), key-frame node
    sizes 1, 16, 17 in turn; the key-frame features of a node are near copies of one descriptor, so that they compete for the slots"""
    rs = np.random.RandomState(500 + 7 * n + seed)
    kf, valid, fr_l, fr_r, nodes_kf = [], [], [], [], {}
    per_node = []
    for q, n_l in enumerate(splits(n)):
        Bq = rs.randint(0, 256, 32).astype(np.uint8)
        nk = KF_NODE_SIZES[q % 3]
        nodes_kf[q] = list(range(len(kf), len(kf) + nk))
        for _ in range(nk):
            kf.append(fsc.flip_bits(rs, Bq, rs.randint(0, 12))); valid.append(rs.rand() < 0.9)
        side = np.array([0] * n_l + [1] * (n - n_l)); rs.shuffle(side)
        per_node.append(side)
        for s in side:
            (fr_r if s else fr_l).append(fsc.flip_bits(rs, Bq, rs.randint(0, 64)))
    nl = len(fr_l)
    nodes_f, il, ir = {}, 0, 0
    for q, side in enumerate(per_node):
        nodes_f[q] = []
        for s in side:
            if s:
                nodes_f[q].append(nl + ir); ir += 1
            else:
                nodes_f[q].append(il); il += 1
    ang_kf = rs.uniform(0, 360, len(kf)); ang_f = rs.uniform(0, 360, nl + len(fr_r))
    return bow_call(kf, fr_l + fr_r, nl, nodes_kf, nodes_f, ang_kf, ang_f, valid)


@functools.lru_cache(maxsize=None)
def bow_shape_cases():
    """name -> (call, check_ori)"""
    C = {}
    for n in NODE_SIZES:
        C["node_%d" % n] = (node_split_call(n), n % 2 == 0)
    C["n_left_0"] = (random_bow_call(61, 150, 160, 0, 12), True)
    C["n_left_all"] = (random_bow_call(62, 150, 160, 160, 12), True)
    C["empty_kf_fv"] = (dict(random_bow_call(63, 20, 30, 10, 3), fvKF=make_fv({})), False)
    C["empty_frame_fv"] = (dict(random_bow_call(64, 20, 30, 10, 3), fvF=make_fv({})), True)
    d = random_bow_call(65, 40, 40, 20, 4)
    C["disjoint_fv"] = (dict(d, fvF=(d["fvF"][0] + np.uint32(1), d["fvF"][1], d["fvF"][2])), True)
    C["no_features"] = (random_bow_call(66, 0, 0, 0, 0), True)
    C["kf_only"] = (random_bow_call(67, 12, 0, 0, 3), False)
    C["2000_a_side"] = (random_bow_call(68, 2000, 2000, 1000, 180, big_nodes=((1, 120, 20), (2, 70, 33))), True)
    # a feature in two nodes: the nodes interact through the slots and the device walks them in order
    e = random_bow_call(69, 60, 60, 30, 5)
    ids, off, feat = e["fvF"]
    feat2 = feat.copy(); feat2[off[1]] = feat[0]
    C["feature_in_two_nodes"] = (dict(e, fvF=(ids, off, feat2)), True)
    return C


RANDOM_BOW = tuple((seed, n_kf, n_f, n_left, nodes) for seed, n_kf, n_f, n_left, nodes in
                   ((71, 300, 320, 170, 25), (72, 257, 199, 64, 9), (73, 90, 400, 333, 4), (74, 500, 480, 1, 60), (75, 33, 35, 34, 2)))


@functools.lru_cache(maxsize=None)
def bow_random_cases():
    return {"random_%d" % s[0]: (random_bow_call(*s), i % 2 == 0) for i, s in enumerate(RANDOM_BOW)}


@functools.lru_cache(maxsize=None)
def bow_expected(group, name):
    """the reference loop's (nmatches, match) of a shape or random call"""
    call, ori = {"shape": bow_shape_cases, "random": bow_random_cases}[group]()[name]
    return ref.search_by_bow_rig(nnratio=NNRATIO, check_ori=ori, **call)


# ------------------------------------------------------------------------------------------------ rig key-frame pairs
def _rot(w):
    return fsc._rot(w)


def scene_geometry(rig_name="tumvi", w2=(0.25, -0.3, 0.2), c2=(0.06, 0.35, 0.08)):
    """two rig key frames: key frame 1's left camera at the world origin, key frame 2's left camera rotated by w2 with centre c2
    (mostly along y: the rigs' own baselines run along x, so a wrong pose record moves a pixel off its epipolar line).  Returns
    dict(cams [4] (kf1 l, kf1 r, kf2 l, kf2 r), poses [4] of (Rcw, tcw) in float64, geom)."""
    rig = fsc.RIGS[rig_name]
    Rlr, tlr = rig["Rlr"].astype(np.float64), rig["tlr"].astype(np.float64)
    right_of = lambda R, t: (Rlr.T @ R, Rlr.T @ (t - tlr))              # x_r = Rlr^T (x_l - tlr)
    R1, t1 = np.eye(3), np.zeros(3)
    R2 = _rot(w2); t2 = -R2 @ np.asarray(c2, np.float64)
    poses = [(R1, t1), right_of(R1, t1), (R2, t2), right_of(R2, t2)]
    cams = [rig["left"], rig["right"], rig["left"], rig["right"]]
    prec = [rig["precision_l"], rig["precision_r"]] * 2
    cam_rows = [[c["fx"], c["fy"], c["cx"], c["cy"]] + list(c["k"]) + [p] for c, p in zip(cams, prec)]
    R12, t12 = [], []
    for c in range(4):
        (Ra, ta), (Rb, tb) = poses[c >> 1], poses[2 + (c & 1)]
        R = Ra @ Rb.T
        R12.append(R.astype(np.float32)); t12.append((ta - R @ tb).astype(np.float32))
    geom = dict(cam=np.array(cam_rows, np.float32), R12=np.array(R12, np.float32).reshape(4, 9), t12=np.array(t12, np.float32))
    return dict(cams=cams, poses=poses, geom=geom)


def observe(G, cam_index, Pw):
    """the pixel (float64) of world point Pw in camera cam_index (0 .. 3)"""
    R, t = G["poses"][cam_index]
    return fsc._project64(G["cams"][cam_index], (R @ np.asarray(Pw, np.float64) + t)[None])[0]


def tri_side(feats):
    """feats: list of dict(right (bool), px, octave, desc, has_mp, angle, node) in NODE order.  The arrays hold the left features
    first; returns (kf dict, index of every feat in the arrays)"""
    order = [i for i, f in enumerate(feats) if not f["right"]] + [i for i, f in enumerate(feats) if f["right"]]
    index = {i: k for k, i in enumerate(order)}
    n_left = sum(1 for f in feats if not f["right"])
    nodes = {}
    for i, f in enumerate(feats):
        nodes.setdefault(f["node"], []).append(index[i])
    pick = lambda key, dt: np.array([feats[i][key] for i in order], dt)
    kf = dict(desc=np.array([feats[i]["desc"] for i in order], np.uint8).reshape(-1, 32), has_mp=pick("has_mp", np.uint8),
              x=np.array([feats[i]["px"][0] for i in order], np.float32), y=np.array([feats[i]["px"][1] for i in order], np.float32),
              octave=pick("octave", np.int32), angle=pick("angle", np.float32), fv=make_fv(nodes), n_left=n_left)
    return kf, [index[i] for i in range(len(feats))]


def feat(G, kf, right, Pw, desc, node=5, octave=0, has_mp=0, angle=0.0, shift=(0.0, 0.0)):
    px = observe(G, 2 * kf + int(right), Pw) + np.asarray(shift, np.float64)
    return dict(right=bool(right), px=px, octave=octave, desc=desc, has_mp=has_mp, angle=angle, node=node)


FAR = (0.0, 40.0)       # a pixel shift that no gate accepts (the level-0 gate is 2.4 px, the level-7 one 8.8 px)
P0 = (0.4, -0.2, 2.5)   # a world point in front of all four cameras


@functools.lru_cache(maxsize=None)
def tri_hand_cases():
    """name -> dict(call, only_stereo, coarse, check_ori, want_match, want_n, [only_record]): outcomes written by hand"""
    G = scene_geometry("diverging")         # optical axes 40 degrees apart: a wrong camera or pose record is no near miss
    B = base_desc(2)
    C = {}

    def case(name, f1, f2, want, only_stereo=False, coarse=False, check_ori=False, sigma=(LEVEL_SIGMA2, LEVEL_SIGMA2), **extra):
        k1, i1 = tri_side(f1)
        k2, i2 = tri_side(f2)
        m = np.full(len(f1), -1, np.int32)
        for a, b in want.items():                                       # in terms of the positions in the lists
            m[i1[a]] = i2[b]
        C[name] = dict(call=dict(kf1=k1, kf2=k2, geom=G["geom"], sigma2_1=sigma[0], sigma2_2=sigma[1]), only_stereo=only_stereo, coarse=coarse,
                       check_ori=check_ori, want_match=m, want_n=len(want), **extra)

    good = lambda kf, d, **kw: feat(G, kf, False, P0, at(B, d), **kw)
    bad = lambda kf, d, **kw: feat(G, kf, False, P0, at(B, d), shift=FAR, **kw)
    # a later candidate at the same distance replaces the holder (dist > bestDist is false at equality)
    case("later_equal_wins", [good(0, 0)], [good(1, 10), feat(G, 1, False, P0, at(B, 10, start=100))], {0: 1})
    # the earlier, closer candidate fails the gate and leaves bestDist alone: the later, farther one is taken
    case("closer_fails_farther_passes", [good(0, 0)], [bad(1, 5), good(1, 20)], {0: 1})
    # the earlier, farther candidate holds; the later closer one fails the gate and changes nothing
    case("farther_passes_closer_fails", [good(0, 0)], [good(1, 20), bad(1, 5)], {0: 0})
    # the last of three equal ones fails: the middle one stays
    case("last_equal_fails", [good(0, 0)], [good(1, 9), feat(G, 1, False, P0, at(B, 9, start=60)), feat(G, 1, False, P0, at(B, 9, start=120), shift=FAR)], {0: 1})
    # one pair per (bRight1, bRight2): its pixels are those of P0 in its own two cameras, which only its own record accepts
    for c, name in enumerate(("ll", "lr", "rl", "rr")):
        case("record_" + name, [feat(G, 0, c >> 1, P0, at(B, 0))], [feat(G, 1, c & 1, P0, at(B, 6))], {0: 0}, only_record=c)
    # 9.5 px off in key frame 1 at octave 6, key frame 2 at octave 5: inside the gates of those levels, outside those of level 0
    case("octave_sigmas", [feat(G, 0, False, P0, at(B, 0), octave=6, shift=(9.5, 0.0))], [feat(G, 1, False, P0, at(B, 3), octave=5)], {0: 0}, own_octaves=True)
    # ... and not accepted at level 0
    case("octave_sigmas_level0", [feat(G, 0, False, P0, at(B, 0), octave=0, shift=(9.5, 0.0))], [feat(G, 1, False, P0, at(B, 3), octave=0)], {})
    # a key-frame-1 feature with a map point is skipped; a key-frame-2 candidate with one is not a candidate
    case("has_mp_1", [good(0, 0, has_mp=1), good(0, 1)], [good(1, 4)], {1: 0})
    case("has_mp_2", [good(0, 0)], [good(1, 0, has_mp=1), good(1, 10)], {0: 1})
    # TH_LOW: 50 is a candidate, 51 is not
    case("dist_50_51", [good(0, 0, node=5), feat(G, 0, False, P0, at(base_desc(3), 0), node=6)],
         [good(1, 50, node=5), feat(G, 1, False, P0, at(base_desc(3), 51), node=6)], {0: 0})
    # the candidate sits AT the epipole (the image of key frame 1's centre): a rig pair has no epipole test (:1026, !pKF1->mpCamera2).
    # Coarse on purpose: a ray through the other camera's centre has no parallax to triangulate, so the geometric gate rejects this
    # candidate whatever an epipole test would do (the host build of the gate counts 0 passes for it) -- only without the gate does the
    # case tell whether an epipole test ran.  The non-coarse path is NOT covered here; `not_coarse` and the gate cases cover it.
    ep = observe(G, 2, np.zeros(3))
    at_ep = dict(right=False, px=ep, octave=0, desc=at(B, 2), has_mp=0, angle=0.0, node=5)
    case("epipole_coarse", [good(0, 0)], [at_ep], {0: 0}, coarse=True)
    # coarse: no gate at all
    case("coarse", [good(0, 0)], [bad(1, 5)], {0: 0}, coarse=True)
    case("not_coarse", [good(0, 0)], [bad(1, 5)], {})
    # bStereo1 is false for every feature of a rig key frame
    case("only_stereo", [good(0, 0)], [good(1, 5)], {}, only_stereo=True)
    # the histogram over all key-frame-1 features: bins 0, 0, 1, 1, 2, 2 and a single match in bin 3, which is dropped
    f1, f2, want = [], [], {}
    for i, a in enumerate((0, 0, 30, 30, 60, 60, 90)):
        Bi = base_desc(30 + i)
        f1.append(feat(G, 0, i % 2 == 1, P0, Bi, node=i, angle=a)); f2.append(feat(G, 1, i % 3 == 1, P0, at(Bi, 4), node=i))
        if a != 90:
            want[i] = i
    case("histogram", f1, f2, want, check_ori=True)
    case("histogram_off", f1, f2, {i: i for i in range(7)})
    return C


def random_tri_call(seed, n_pts, rig_name="tumvi", extra=40, noise=0.25, total=None):
    """n_pts world points, each seen by one camera of either key frame (sides at random), pixels with noise of `noise` level sigmas
    (well inside the gate of 2.45 sigmas); per point a few decoy candidates in the same node: near descriptors at pixels 25 .. 60 px
    away (no gate accepts them), exact copies (ties at equal distance) and some with map points.  `extra` features without partner on
    either side, or as many as bring each key frame to `total` features."""
    rs = np.random.RandomState(seed)
    G = scene_geometry(rig_name)
    f1, f2 = [], []
    n_nodes = max(n_pts // 6, 1)
    for p in range(n_pts):
        while True:
            d = np.exp(rs.uniform(np.log(0.8), np.log(8.0)))
            th, ph = rs.uniform(0, 0.9), rs.uniform(-np.pi, np.pi)
            Pw = d * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
            if all((R @ Pw + t)[2] > 0.3 for R, t in G["poses"]):
                break
        Bp = rs.randint(0, 256, 32).astype(np.uint8)
        node = int(rs.randint(0, n_nodes)) * 2
        o1, o2 = int(rs.randint(0, 8)), int(rs.randint(0, 8))
        ang = float(rs.uniform(0, 360))
        jit = lambda o: noise * np.sqrt(LEVEL_SIGMA2[o]) * rs.standard_normal(2)
        f1.append(feat(G, 0, rs.rand() < 0.5, Pw, Bp, node=node, octave=o1, has_mp=int(rs.rand() < 0.1), angle=ang, shift=jit(o1)))
        cands = [feat(G, 1, rs.rand() < 0.5, Pw, fsc.flip_bits(rs, Bp, rs.randint(0, 58)), node=node, octave=o2, has_mp=int(rs.rand() < 0.1),
                      angle=(ang - 25 + rs.normal(0, 6)) % 360, shift=jit(o2))]
        for _ in range(rs.randint(0, 3)):
            far = rs.uniform(25, 60) * np.array([np.cos(ph), np.sin(ph)]) * (1 if rs.rand() < 0.5 else -1)
            cands.append(feat(G, 1, rs.rand() < 0.5, Pw, fsc.flip_bits(rs, Bp, rs.randint(0, 40)), node=node, octave=int(rs.randint(0, 8)),
                              angle=float(rs.uniform(0, 360)), shift=far))
        if rs.rand() < 0.3:
            cands.append(dict(cands[0], has_mp=0))                      # an exact copy: equal distance, the later one wins
        rs.shuffle(cands)
        f2 += cands
    lone = lambda: dict(right=rs.rand() < 0.5, px=rs.uniform(60, 450, 2), octave=int(rs.randint(0, 8)), desc=rs.randint(0, 256, 32).astype(np.uint8), has_mp=0,
                        angle=float(rs.uniform(0, 360)), node=int(rs.randint(0, n_nodes + 3)) * 2 + int(rs.rand() < 0.3))
    if total is not None:
        assert len(f1) <= total and len(f2) <= total
        f1 += [lone() for _ in range(total - len(f1))]; f2 += [lone() for _ in range(total - len(f2))]
        extra = 0
    for _ in range(extra):
        f1.append(dict(right=rs.rand() < 0.5, px=rs.uniform(60, 450, 2), octave=int(rs.randint(0, 8)), desc=rs.randint(0, 256, 32).astype(np.uint8), has_mp=0,
                       angle=float(rs.uniform(0, 360)), node=int(rs.randint(0, n_nodes + 3)) * 2 + int(rs.rand() < 0.3)))
        f2.append(dict(right=rs.rand() < 0.5, px=rs.uniform(60, 450, 2), octave=int(rs.randint(0, 8)), desc=rs.randint(0, 256, 32).astype(np.uint8), has_mp=0,
                       angle=float(rs.uniform(0, 360)), node=int(rs.randint(0, n_nodes + 3)) * 2 + int(rs.rand() < 0.3)))
    p1 = rs.permutation(len(f1)); p2 = rs.permutation(len(f2))
    k1, _ = tri_side([f1[i] for i in p1])
    k2, _ = tri_side([f2[i] for i in p2])
    return dict(kf1=k1, kf2=k2, geom=G["geom"], sigma2_1=LEVEL_SIGMA2, sigma2_2=LEVEL_SIGMA2)


RANDOM_TRI = {"tri_tumvi_a": (81, 260, "tumvi"), "tri_tumvi_b": (82, 130, "tumvi"), "tri_diverging": (83, 200, "diverging"), "tri_one_node": (84, 5, "tumvi")}


@functools.lru_cache(maxsize=None)
def tri_random_case(name):
    return random_tri_call(*RANDOM_TRI[name])


@functools.lru_cache(maxsize=None)
def tri_random_expected(name, coarse=False, check_ori=False):
    """(nmatches, match12, undecided [n1]) of the reference loop on a random call"""
    s = tri_random_case(name)
    n, m = ref.search_for_triangulation_rig(s, coarse=coarse, check_ori=check_ori)
    return n, m, (np.zeros(len(m), bool) if coarse else ref.undecided(s))


def with_has_mp(s, seed):
    """the same pair with another has_mp on key frame 1: what one key frame against several neighbours passes per pair"""
    rs = np.random.RandomState(seed)
    return dict(s, kf1=dict(s["kf1"], has_mp=(rs.rand(len(s["kf1"]["x"])) < 0.2).astype(np.uint8)))
