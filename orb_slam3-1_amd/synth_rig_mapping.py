"""Synthetic scenes for LocalMapping::CreateNewMapPoints with two-camera KannalaBrandt8 rigs: a rig key frame, k rig neighbours on
a trajectory and world points seen by all four (bRight1, bRight2) combinations, with pixel noise of 0.25 level sigmas and decoys
in the neighbours' vocabulary nodes (near descriptors at far pixels, exact copies, features with map points).

A key frame is dict(desc, has_mp, x, y, octave, angle, fv, n_left, Rcw [2][3][3], tcw [2][3], Ow [2][3], cam [2][9], mb,
level_sigma2, scale_factors) over the concatenated arrays -- the left features first, right feature j at n_left + j; index 0 of
the poses is the left camera.  A scene is dict(kf1, neighbours, pairs=[dict(geom, coarse)], params) -- what
Matcher.create_new_map_points_rig takes.  Everything is seeded; float64 ground truth stays in the private keys "_poses"."""
import numpy as np

N_LEVELS = 8
_scale = [np.float32(1.0)]
for _ in range(N_LEVELS - 1):
    _scale.append(np.float32(_scale[-1] * np.float32(1.2)))
SCALE_FACTORS = np.array(_scale, np.float32)                        # mvScaleFactors of ORBextractor(.., 1.2, 8, ..)
LEVEL_SIGMA2 = np.array([s * s for s in _scale], np.float32)        # mvLevelSigma2

f32 = lambda v: float(np.float32(v))


def rot(w):
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
    return dict(left=left, right=right, precision_l=f32(1e-6), precision_r=f32(1e-6), Rlr=rot(w).astype(np.float32), tlr=np.asarray(t, np.float32))


RIGS = {
    # a TUM-VI-like pair: 512 x 512, 0.101 m baseline, a relative rotation of a few hundredths of a radian
    "tumvi": _rig(_cam(190.978, 190.973, 254.932, 256.897, (0.0034, 0.0007, -0.0020, 0.0002)),
                  _cam(190.442, 190.434, 252.597, 254.917, (0.0034, 0.0018, -0.0027, 0.0004)), (0.02, -0.035, 0.012), (0.101, 0.0012, -0.0018)),
    # optical axes that diverge by 40 degrees: a wrong camera or pose record is no near miss
    "diverging": _rig(_cam(190.978, 190.973, 254.932, 256.897, (0.0034, 0.0007, -0.0020, 0.0002)),
                      _cam(190.442, 190.434, 252.597, 254.917, (0.0034, 0.0018, -0.0027, 0.0004)), (0.01, 0.70, -0.02), (0.12, 0.0, 0.01)),
}


def project(cam, X):
    """KannalaBrandt8 projection of camera-frame points (n, 3) in float64"""
    X = np.asarray(X, np.float64).reshape(-1, 3)
    x, y, z = X[:, 0], X[:, 1], X[:, 2]
    theta = np.arctan2(np.sqrt(x * x + y * y), z)
    psi = np.arctan2(y, x)
    k = cam["k"]
    t2 = theta * theta
    r = theta * (1 + t2 * (k[0] + t2 * (k[1] + t2 * (k[2] + t2 * k[3]))))
    return np.stack([cam["fx"] * r * np.cos(psi) + cam["cx"], cam["fy"] * r * np.sin(psi) + cam["cy"]], 1)


def rig_poses(rig, R, c):
    """[(Rcw, tcw) of the left camera, of the right camera] in float64 for a left camera with rotation R and centre c:
    x_right = Rlr^T (x_left - tlr)"""
    R = np.asarray(R, np.float64)
    t = -R @ np.asarray(c, np.float64)
    Rlr, tlr = rig["Rlr"].astype(np.float64), rig["tlr"].astype(np.float64)
    return [(R, t), (Rlr.T @ R, Rlr.T @ (t - tlr))]


def rig_mb(rig):
    """the stereo baseline of the rig as the settings compute it: the length of the left-to-right translation"""
    return np.float32(np.linalg.norm(rig["tlr"].astype(np.float64)))


def flip_bits(rs, desc, k):
    bits = np.unpackbits(np.asarray(desc, np.uint8))
    if k > 0:
        bits[rs.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def at(base, k, start=0):
    """`base` with the k bits start .. start + k - 1 flipped"""
    bits = np.unpackbits(np.asarray(base, np.uint8))
    bits[start:start + k] ^= 1
    return np.packbits(bits)


def base_desc(seed):
    return np.random.RandomState(7000 + seed).randint(0, 256, 32).astype(np.uint8)


def make_fv(nodes):
    """{node id: [features in insertion order]} -> (node ids ascending, offsets, features)"""
    ids = sorted(nodes)
    off = np.zeros(len(ids) + 1, np.int32)
    feat = []
    for i, k in enumerate(ids):
        feat += list(nodes[k])
        off[i + 1] = len(feat)
    return np.array(ids, np.uint32), off, np.array(feat, np.uint32)


def observe(rig, poses, right, Pw):
    R, t = poses[int(right)]
    return project(rig["right" if right else "left"], (R @ np.asarray(Pw, np.float64) + t)[None])[0]


def feat(rig, poses, right, Pw, desc, node=5, octave=0, has_mp=0, shift=(0.0, 0.0)):
    """a feature: the pixel of world point Pw in the left / right camera of the key frame with `poses`, moved by `shift`"""
    return dict(right=bool(right), px=observe(rig, poses, right, Pw) + np.asarray(shift, np.float64), octave=int(octave), desc=desc,
                has_mp=int(has_mp), node=int(node))


def key_frame(rig, R, c, feats):
    """a rig key frame from features in NODE order (dicts of right, px, octave, desc, has_mp, node): the arrays hold the left
    features first.  Returns (key frame, index of every feature in the arrays)."""
    order = [i for i, f in enumerate(feats) if not f["right"]] + [i for i, f in enumerate(feats) if f["right"]]
    index = {i: k for k, i in enumerate(order)}
    nodes = {}
    for i, f in enumerate(feats):
        nodes.setdefault(f["node"], []).append(index[i])
    poses = rig_poses(rig, R, c)
    cams = [rig["left"], rig["right"]]
    prec = [rig["precision_l"], rig["precision_r"]]
    n = len(feats)
    kf = dict(desc=np.array([feats[i]["desc"] for i in order], np.uint8).reshape(-1, 32), has_mp=np.array([feats[i]["has_mp"] for i in order], np.uint8),
              x=np.array([feats[i]["px"][0] for i in order], np.float32), y=np.array([feats[i]["px"][1] for i in order], np.float32),
              octave=np.array([feats[i]["octave"] for i in order], np.int32), angle=np.zeros(n, np.float32), fv=make_fv(nodes),
              n_left=sum(1 for f in feats if not f["right"]),
              Rcw=np.array([p[0] for p in poses], np.float32), tcw=np.array([p[1] for p in poses], np.float32),
              Ow=np.array([-p[0].T @ p[1] for p in poses], np.float32),
              cam=np.array([[cm["fx"], cm["fy"], cm["cx"], cm["cy"]] + list(cm["k"]) + [p] for cm, p in zip(cams, prec)], np.float32),
              mb=rig_mb(rig), level_sigma2=LEVEL_SIGMA2.copy(), scale_factors=SCALE_FACTORS.copy(), _poses=poses, _rig=rig)
    return kf, [index[i] for i in range(n)]


def pair_geometry(kf1, kf2):
    """OrbmRigTriGeometry of (kf1, kf2): cam = kf1 left, kf1 right, kf2 left, kf2 right; R12 / t12 of T1w*Tw2, T1w*Twr2, Tr1w*Tw2,
    Tr1w*Twr2 (ll, lr, rl, rr), computed in float64 and rounded"""
    R12, t12 = [], []
    for c in range(4):
        (Ra, ta), (Rb, tb) = kf1["_poses"][c >> 1], kf2["_poses"][c & 1]
        R = Ra @ Rb.T
        R12.append(R.astype(np.float32)); t12.append((ta - R @ tb).astype(np.float32))
    return dict(cam=np.concatenate([kf1["cam"], kf2["cam"]]).astype(np.float32), R12=np.array(R12, np.float32).reshape(4, 9), t12=np.array(t12, np.float32))


def scene(kf1, neighbours, coarse=(), inertial=False, far_points=False, th_far=0.0):
    return dict(kf1=kf1, neighbours=list(neighbours), pairs=[dict(geom=pair_geometry(kf1, k), coarse=j in coarse) for j, k in enumerate(neighbours)],
                params=dict(inertial=bool(inertial), far_points=bool(far_points), th_far=float(th_far), scale_factor_1=1.2))


def trajectory(n_neighbours, seed=0):
    """[(R, c)]: centres 0.25 .. 1.15 m from key frame 1's left camera on a spiral, rotations of up to 0.15 rad.  Every centre is
    at least 0.13 m from either camera of key frame 1, so no baseline test (bound: 0.101 or 0.12 m) is near its bound"""
    rs = np.random.RandomState(9000 + seed)
    out = []
    for j in range(n_neighbours):
        r, phi = 0.25 + 0.1 * (j % 10), 0.7 * j + 0.3
        out.append((rot(rs.uniform(-0.09, 0.09, 3)), np.array([r * np.cos(phi), r * np.sin(phi), 0.05 * np.sin(1.3 * j)])))
    return out


def _visible(poses, right, Pw):
    R, t = poses[int(right)]
    X = R @ Pw + t
    return X[2] > 0.2 and np.arctan2(np.hypot(X[0], X[1]), X[2]) < 1.3


def make_rig_mapping_scene(seed, n_pts, n_neighbours, rig="tumvi", total=None, right_frac_1=0.5, right_frac_2=0.5, poses=None, coarse=(),
                           inertial=False, far_points=False, th_far=0.0, noise=0.25, see=0.7, node_size=None, empty_neighbours=()):
    """n_pts world points, each seen by one camera of key frame 1 and, with probability `see`, by one camera of every neighbour;
    per sighting a few decoys in the same vocabulary node.  right_frac_*: the share of right-camera features (0 and 1 give n_left = n
    and 0).  poses: {j: (R, c)} overrides of the trajectory.  total: lone features bring every key frame to that many.  node_size:
    {j: n} puts n candidates (near descriptors at far pixels, plus the true sighting) into ONE node of neighbour j that all points share.
    empty_neighbours: neighbours without features."""
    rs = np.random.RandomState(seed)
    R = RIGS[rig]
    traj = trajectory(n_neighbours, seed)
    for j, p in (poses or {}).items():
        traj[j] = p
    p1 = rig_poses(R, np.eye(3), np.zeros(3))
    pn = [rig_poses(R, Rj, cj) for Rj, cj in traj]
    n_nodes = max(n_pts // 6, 1)
    node_size = node_size or {}
    f1, fn = [], [[] for _ in range(n_neighbours)]
    jit = lambda o: noise * np.sqrt(float(LEVEL_SIGMA2[o])) * rs.standard_normal(2)
    for p in range(n_pts):
        while True:
            d = np.exp(rs.uniform(np.log(0.8), np.log(8.0)))
            th, ph = rs.uniform(0, 0.9), rs.uniform(-np.pi, np.pi)
            Pw = d * np.array([np.sin(th) * np.cos(ph), np.sin(th) * np.sin(ph), np.cos(th)])
            right1 = rs.rand() < right_frac_1
            if _visible(p1, right1, Pw):
                break
        Bp = rs.randint(0, 256, 32).astype(np.uint8)
        node = int(rs.randint(0, n_nodes)) * 2
        o1 = int(rs.randint(0, N_LEVELS))
        f1.append(feat(R, p1, right1, Pw, Bp, node=node, octave=o1, has_mp=int(rs.rand() < 0.1), shift=jit(o1)))
        for j in range(n_neighbours):
            if j in empty_neighbours or rs.rand() >= see:
                continue
            right2 = rs.rand() < right_frac_2
            if not _visible(pn[j], right2, Pw):
                continue
            delta = int(rs.choice([-1, 0, 0, 0, 1])) if rs.rand() < 0.85 else int(rs.choice([-5, -4, 4, 5]))
            o2 = int(np.clip(o1 + delta, 0, N_LEVELS - 1))
            nd = 0 if j in node_size else node
            cands = [feat(R, pn[j], right2, Pw, flip_bits(rs, Bp, rs.randint(0, 58)), node=nd, octave=o2, has_mp=int(rs.rand() < 0.1), shift=jit(o2))]
            for _ in range(rs.randint(0, 3)):
                far = rs.uniform(25, 60) * np.array([np.cos(ph), np.sin(ph)]) * (1 if rs.rand() < 0.5 else -1)
                cands.append(feat(R, pn[j], rs.rand() < right_frac_2, Pw, flip_bits(rs, Bp, rs.randint(0, 40)), node=nd, octave=int(rs.randint(0, N_LEVELS)), shift=far))
            if rs.rand() < 0.3:
                cands.append(dict(cands[0], has_mp=0))                  # an exact copy: equal distance, the later one wins
            rs.shuffle(cands)
            fn[j] += cands
    lone = lambda rf: dict(right=rs.rand() < rf, px=rs.uniform(60, 450, 2), octave=int(rs.randint(0, N_LEVELS)), desc=rs.randint(0, 256, 32).astype(np.uint8),
                           has_mp=0, node=int(rs.randint(0, n_nodes + 3)) * 2 + int(rs.rand() < 0.3))
    for j, n in node_size.items():                                       # one node of exactly n candidates in neighbour j; key frame 1's points share it
        for f in f1:
            f["node"] = 0
        fn[j] = fn[j][:n]
        while len(fn[j]) < n:
            src = f1[rs.randint(0, len(f1))]
            fn[j].append(dict(right=rs.rand() < right_frac_2, px=rs.uniform(60, 450, 2), octave=int(rs.randint(0, N_LEVELS)),
                              desc=flip_bits(rs, src["desc"], rs.randint(0, 56)), has_mp=int(rs.rand() < 0.1), node=0))
        rs.shuffle(fn[j])
    if total is not None:
        f1 += [lone(right_frac_1) for _ in range(max(total - len(f1), 0))]
        for j in range(n_neighbours):
            if j not in empty_neighbours and j not in node_size:
                fn[j] += [lone(right_frac_2) for _ in range(max(total - len(fn[j]), 0))]
    else:
        extra = max(n_pts // 8, 2)
        f1 += [lone(right_frac_1) for _ in range(extra)]
        for j in range(n_neighbours):
            if j not in empty_neighbours and j not in node_size:
                fn[j] += [lone(right_frac_2) for _ in range(extra)]
    k1, _ = key_frame(R, np.eye(3), np.zeros(3), [f1[i] for i in rs.permutation(len(f1))])
    nbs = []
    for j in range(n_neighbours):
        kj, _ = key_frame(R, traj[j][0], traj[j][1], [fn[j][i] for i in rs.permutation(len(fn[j]))])
        nbs.append(kj)
    return scene(k1, nbs, coarse, inertial, far_points, th_far)
