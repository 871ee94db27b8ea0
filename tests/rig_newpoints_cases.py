"""The calls of the rig CreateNewMapPoints tests: hand-built scenes with the outcome written next to them by hand, shape scenes and
seeded random scenes.  A test helper, not a test.  Everything is built once per process (functools.lru_cache): the tests share the
scenes and the reference's results and must not modify them."""
import functools
import importlib

import numpy as np

import rig_newpoints_reference as R

try:                            # torch before anything of the package: a process must end up with ONE HIP runtime (tests/conftest.py: _torch_first),
    import torch  # noqa: F401   and this module loads the package when a test file that imports it is collected
except Exception:
    pass
S = importlib.import_module("orb_slam3-1_amd.synth_rig_mapping")

P0 = (0.4, -0.2, 2.5)           # a world point in front of all cameras of every hand-built key frame
P1 = (-0.3, 0.25, 2.2)
P2 = (0.1, 0.3, 2.5)
OFF = (8.0, 0.0)                # 8 px across the epipolar lines of NB0 (which run along y): Triangulate splits it, about 4 px a side, past the level-0 gate
NB0 = (S.rot((0.02, -0.03, 0.01)), np.array([0.0, 0.4, 0.05]))     # 0.4 m away: four baselines of the rig
NB1 = (S.rot((-0.01, 0.02, 0.0)), np.array([0.05, -0.45, 0.02]))
# 0.13 m from key frame 1's left centre (mb = 0.101: 29 % above) and 0.029 m from its right centre at (0.101, 0.0012, -0.0018)
# (71 % below): the baseline test of this neighbour depends on which centre Ow1 holds
AMBIGUOUS = (np.eye(3), np.array([0.13, 0.0, 0.0]))


def build(rig_name, feats1, neighbours, **kw):
    """feats1: features of key frame 1 as (right, Pw, desc, options); neighbours: [((R, c), [features])].  Returns the scene and
    the array index of every listed feature: idx1[k], idx2[j][k]."""
    rig = S.RIGS[rig_name]
    p1 = S.rig_poses(rig, np.eye(3), np.zeros(3))
    k1, i1 = S.key_frame(rig, np.eye(3), np.zeros(3), [S.feat(rig, p1, r, P, d, **o) for (r, P, d, o) in feats1])
    nbs, i2 = [], []
    for (Rj, cj), fs in neighbours:
        pj = S.rig_poses(rig, Rj, cj)
        kj, ij = S.key_frame(rig, Rj, cj, [S.feat(rig, pj, r, P, d, **o) for (r, P, d, o) in fs])
        nbs.append(kj); i2.append(ij)
    return S.scene(k1, nbs, **kw), i1, i2


@functools.lru_cache(maxsize=None)
def hand_cases():
    """name -> dict(scene, neighbour, idx2 [n1], n_matched, n_created, skipped [n_neighbours] [, extra]): the outcome is written by
    hand from the reference's text, in terms of the positions in the feature lists (translated to array indices here)."""
    B = [S.base_desc(k) for k in range(6)]
    C = {}

    def case(name, built, neighbour, idx2, n_matched, n_created, skipped, **extra):
        sc, i1, i2 = built
        n1 = len(sc["kf1"]["x"])
        nb_arr, i2_arr = np.full(n1, -1, np.int32), np.full(n1, -1, np.int32)
        for k, (j, q) in enumerate(zip(neighbour, idx2)):
            nb_arr[i1[k]] = j
            i2_arr[i1[k]] = i2[j][q] if j >= 0 else -1
        C[name] = dict(scene=sc, neighbour=nb_arr, idx2=i2_arr, n_matched=np.array(n_matched, np.int32), n_created=np.array(n_created, np.int32),
                       skipped=np.array(skipped, np.uint8), idx1=i1, idx2_of=i2, **extra)

    # 1. accepted by neighbour 0: a map point from there on, neighbour 1 (which holds a perfect partner too) does not search it
    case("accepted_once", build("tumvi", [(0, P0, B[0], {})], [(NB0, [(0, P0, S.at(B[0], 4), {})]), (NB1, [(0, P0, S.at(B[0], 2), {})])]),
         [0], [0], [1, 0], [1, 0], [0, 0])
    # 2. neighbour 0 is searched coarse, so its candidate 8 px off its epipolar line is a match; the geometry rejects it (reprojection); neighbour 1 accepts
    case("rejected_then_accepted", build("tumvi", [(0, P0, B[0], {})], [(NB0, [(0, P0, S.at(B[0], 4), dict(shift=OFF))]), (NB1, [(0, P0, S.at(B[0], 6), {})])],
                                         coarse=(0,)),
         [1], [0], [1, 1], [0, 1], [0, 0], rejected_by={(0, 0): ("reproj1", "reproj2")})
    # 3. one pair per (bRight1, bRight2); the diverging rig: only its own pose and camera records accept a pair
    pts = [P0, (0.2, 0.1, 2.0), (0.5, 0.0, 2.2), (0.3, -0.1, 3.0)]
    case("four_records", build("diverging", [(c >> 1, pts[c], B[c], dict(node=c)) for c in range(4)],
                               [(NB0, [(c & 1, pts[c], S.at(B[c], 5), dict(node=c)) for c in range(4)])]),
         [0, 0, 0, 0], [0, 1, 2, 3], [4], [4], [0])
    # 4. a RIGHT observation: max_dist = |x - LEFT centre| * scale.  The point lies along the rig's baseline, where the two
    # readings differ most: |P - Ow_left| = 2.193, |P - Ow_right| = 2.122 (3.3 % apart)
    PX = (1.6, 0.0, 1.5)
    case("dist_from_left_centre", build("tumvi", [(1, PX, B[0], dict(octave=2))], [(NB0, [(1, PX, S.at(B[0], 3), dict(octave=2))])]),
         [0], [0], [1], [1], [0], max_dist_left=float(np.linalg.norm(PX)) * 1.44, max_dist_right=float(np.linalg.norm(np.array(PX) - [0.101, 0.0012, -0.0018])) * 1.44)
    # 5. stale Ow1.  Key frame 1: L (left), T (right), G (left).  Neighbour 0 holds partners of L and T, the AMBIGUOUS neighbour 1 one of G.
    kf1 = [(0, P0, B[0], dict(node=5)), (1, P1, B[1], dict(node=6)), (0, P2, B[2], dict(node=7))]
    nb1 = (AMBIGUOUS, [(0, P2, S.at(B[2], 3), dict(node=7))])
    # T matches at neighbour 0 and has the highest idx1 (right features come last): Ow1 is the RIGHT centre, neighbour 1 is 0.029 m away: skipped
    case("stale_right", build("tumvi", kf1, [(NB0, [(0, P0, S.at(B[0], 4), dict(node=5)), (1, P1, S.at(B[1], 4), dict(node=6))]), nb1]),
         [0, 0, -1], [0, 1, -1], [2, 0], [2, 0], [0, 1])
    # the same, but T's partner is 51 bits away: no match, the last match is L's: Ow1 is the LEFT centre, neighbour 1 is 0.13 m away: searched
    case("stale_left", build("tumvi", kf1, [(NB0, [(0, P0, S.at(B[0], 4), dict(node=5)), (1, P1, S.at(B[1], 51), dict(node=6))]), nb1]),
         [0, -1, 1], [0, -1, 0], [1, 1], [1, 1], [0, 0])
    # neighbour 0 without any match: Ow1 keeps the left centre it started with
    case("stale_matchless", build("tumvi", kf1, [(NB0, [(0, P0, S.at(B[0], 51), dict(node=5)), (1, P1, S.at(B[1], 51), dict(node=6))]), nb1]),
         [-1, -1, 1], [-1, -1, 0], [0, 1], [0, 1], [0, 0])
    # T's match (coarse search, partner 8 px off its epipolar line) fails its gates: no map point, but Ow1 was overwritten before the gates: skipped
    case("stale_right_rejected", build("tumvi", kf1, [(NB0, [(0, P0, S.at(B[0], 4), dict(node=5)), (1, P1, S.at(B[1], 4), dict(node=6, shift=OFF))]), nb1], coarse=(0,)),
         [0, -1, -1], [0, -1, -1], [2, 0], [1, 0], [0, 1])
    # 6. far points: |PF - centres| = 5.1 m; bound 4 rejects, bound 6 accepts
    PF = (0.8, -0.4, 5.0)
    far = lambda th: build("tumvi", [(0, PF, B[0], {})], [(NB0, [(0, PF, S.at(B[0], 4), {})])], far_points=True, th_far=th)
    case("far_rejected", far(4.0), [-1], [-1], [1], [0], [0], rejected_by={(0, 0): ("far1",)})
    case("far_accepted", far(6.0), [0], [0], [1], [1], [0])
    # the scale gate: dist2 / dist1 = 1.005, ratioFactor = 1.8; 1.2^3 = 1.728 passes at both ends, 1.2^4 = 2.074 fails at both
    for name, o1, o2, ok, gate in (("scale_3_0", 3, 0, True, None), ("scale_4_0", 4, 0, False, "scale_lo"), ("scale_0_3", 0, 3, True, None), ("scale_0_4", 0, 4, False, "scale_hi")):
        b = build("tumvi", [(0, P0, B[0], dict(octave=o1))], [(NB0, [(0, P0, S.at(B[0], 4), dict(octave=o2))])])
        case(name, b, [0 if ok else -1], [0 if ok else -1], [1], [1 if ok else 0], [0], **({} if ok else dict(rejected_by={(0, 0): (gate,)})))
    return C


# ------------------------------------------------------------------------------------------------ shape and random scenes
ALL_SKIPPED = {0: (np.eye(3), np.array([0.0, 0.01, 0.0])), 1: (np.eye(3), np.array([0.02, 0.0, 0.0])), 2: (np.eye(3), np.array([0.04, 0.0, 0.005]))}
AMBIGUOUS_2 = (S.rot((0.0, 0.01, 0.0)), np.array([0.125, 0.01, 0.0]))          # 0.1254 m / 0.0258 m from the two centres

SHAPES = {
    # (n_left_1, n_left_2) in {0, n, in between}
    "left_left": dict(seed=101, n_pts=60, n_neighbours=2, right_frac_1=0.0, right_frac_2=0.0),
    "left_right": dict(seed=102, n_pts=60, n_neighbours=2, right_frac_1=0.0, right_frac_2=1.0),
    "right_left": dict(seed=103, n_pts=60, n_neighbours=2, right_frac_1=1.0, right_frac_2=0.0),
    "right_mixed": dict(seed=104, n_pts=60, n_neighbours=2, right_frac_1=1.0, right_frac_2=0.5),
    "mixed_right": dict(seed=105, n_pts=60, n_neighbours=2, right_frac_1=0.5, right_frac_2=1.0),
    # 1, 2, 3 neighbours, and 64 of 40 features each
    "one_neighbour": dict(seed=111, n_pts=80, n_neighbours=1),
    "two_neighbours": dict(seed=112, n_pts=80, n_neighbours=2),
    "three_neighbours": dict(seed=113, n_pts=80, n_neighbours=3, inertial=True),
    "64_neighbours": dict(seed=114, n_pts=24, n_neighbours=64, total=40, see=0.5),
    # an empty neighbour, coarse on one pair only, far points
    "empty_neighbour": dict(seed=121, n_pts=60, n_neighbours=3, empty_neighbours=(1,)),
    "coarse_one_pair": dict(seed=122, n_pts=120, n_neighbours=3, coarse=(1,), far_points=True, th_far=6.0),
    # the baseline test: every neighbour skipped; an ambiguous neighbour at position 1, two in a row, one last -- with right
    # features in key frame 1 (the state turns "right") and without (it stays "left")
    "all_skipped": dict(seed=131, n_pts=50, n_neighbours=3, poses=ALL_SKIPPED),
    "ambiguous_at_1": dict(seed=132, n_pts=80, n_neighbours=3, poses={1: AMBIGUOUS}),
    "ambiguous_at_1_left_only": dict(seed=133, n_pts=80, n_neighbours=3, poses={1: AMBIGUOUS}, right_frac_1=0.0),
    "ambiguous_twice": dict(seed=134, n_pts=80, n_neighbours=4, poses={1: AMBIGUOUS, 2: AMBIGUOUS_2}),
    "ambiguous_twice_left_only": dict(seed=135, n_pts=80, n_neighbours=4, poses={1: AMBIGUOUS, 2: AMBIGUOUS_2}, right_frac_1=0.0),
    "ambiguous_last": dict(seed=136, n_pts=80, n_neighbours=3, poses={2: AMBIGUOUS}, right_frac_1=0.0),
    "ambiguous_after_skipped": dict(seed=137, n_pts=80, n_neighbours=4, poses={1: ALL_SKIPPED[1], 2: AMBIGUOUS}),
}
# a neighbour node of 1 .. 130 candidates split across the sides: the lane-group boundaries of 16 and 64 lanes
NODE_SIZES = (1, 15, 16, 17, 63, 64, 65, 130)
for _n in NODE_SIZES:
    SHAPES["node_%d" % _n] = dict(seed=140 + _n, n_pts=12, n_neighbours=2, node_size={0: _n}, see=0.9)

RANDOM = {
    "random_3": dict(seed=201, n_pts=230, n_neighbours=3, total=600, far_points=True, th_far=7.0),
    "random_10": dict(seed=202, n_pts=230, n_neighbours=10, total=600, inertial=True, coarse=(4,), poses={6: AMBIGUOUS}),
}


@functools.lru_cache(maxsize=None)
def shape_scene(name):
    return S.make_rig_mapping_scene(**{**SHAPES, **RANDOM}[name])


@functools.lru_cache(maxsize=None)
def expected(name, faithful=False):
    """the sequential reference of a hand-built, shape or random scene in float64 (or float32)"""
    sc = hand_cases()[name]["scene"] if name in hand_cases() else shape_scene(name)
    return R.create_new_map_points_rig(sc, np.float32 if faithful else np.float64)


def scene_of(name):
    return hand_cases()[name]["scene"] if name in hand_cases() else shape_scene(name)


def all_names():
    return list(hand_cases()) + list(SHAPES) + list(RANDOM)


def special_scenes():
    """scenes no generator builds: key frame 1 without features, and no vocabulary node in common"""
    sc = {f: v for f, v in shape_scene("two_neighbours").items() if f != "_tables"}     # (the reference caches its search tables on a scene)
    k = sc["kf1"]
    empty = dict(sc, kf1=dict(k, desc=np.zeros((0, 32), np.uint8), fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)), n_left=0,
                              **{f: k[f][:0] for f in ("x", "y", "octave", "has_mp", "angle")}))
    nbs = [dict(q) for q in sc["neighbours"]]
    for q in nbs:
        nodes, off, feat = q["fv"]
        q["fv"] = ((nodes + np.uint32(1000)).astype(np.uint32), off, feat)  # beyond every node of key frame 1
    return dict(kf1_empty=empty, no_common_node=dict(sc, neighbours=nbs))
