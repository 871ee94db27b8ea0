"""Seeded scenes for LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:392-716): a 3-D point cloud, the current
key frame and its covisible neighbours, as the arrays orbm_create_new_map_points takes (capi.Matcher.create_new_map_points)."""
import numpy as np

from . import synth

W, H = 752.0, 480.0


def _rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def _flip(rs, d, p):
    bits = np.unpackbits(d, axis=-1)
    return np.packbits(bits ^ (rs.uniform(size=bits.shape) < p).astype(np.uint8), axis=-1)


def _distort(x, y, cam, k1):
    """mvKeys from mvKeysUn: one radial term, enough to move a key point by a few pixels towards the image corners"""
    xn, yn = (x - cam["cx"]) / cam["fx"], (y - cam["cy"]) / cam["fy"]
    f = 1.0 + k1 * (xn * xn + yn * yn)
    return (cam["fx"] * xn * f + cam["cx"]).astype(np.float32), (cam["fy"] * yn * f + cam["cy"]).astype(np.float32)


def epipole_and_F12(kf1, kf2):
    """ep = mpCamera->project(T2w * Cw1) and F12 = K1^-T [t12]x R12 K2^-1 with T12 = T1w * Tw2, as include/orbslam3_hip.h defines
    them for orbm_search_for_triangulation (src/ORBmatcher.cc:914-931, src/CameraModels/Pinhole.cpp:109-112)"""
    R1, t1 = np.asarray(kf1["Rcw"], np.float64).reshape(3, 3), np.asarray(kf1["tcw"], np.float64)
    R2, t2 = np.asarray(kf2["Rcw"], np.float64).reshape(3, 3), np.asarray(kf2["tcw"], np.float64)
    C2 = R2 @ np.asarray(kf1["Ow"], np.float64) + t2
    ep = (kf2["fx"] * C2[0] / C2[2] + kf2["cx"], kf2["fy"] * C2[1] / C2[2] + kf2["cy"])
    R12 = R1 @ R2.T
    t12 = t1 - R12 @ t2
    tx = np.array([[0, -t12[2], t12[1]], [t12[2], 0, -t12[0]], [-t12[1], t12[0], 0]])
    K1 = np.array([[kf1["fx"], 0, kf1["cx"]], [0, kf1["fy"], kf1["cy"]], [0, 0, 1.0]])
    K2 = np.array([[kf2["fx"], 0, kf2["cx"]], [0, kf2["fy"], kf2["cy"]], [0, 0, 1.0]])
    F12 = np.linalg.inv(K1).T @ tx @ R12 @ np.linalg.inv(K2)
    return (np.float32(ep[0]), np.float32(ep[1])), np.ascontiguousarray(F12, np.float32).reshape(9)


def _key_frame(rs, cam, R, t, Xw, desc_w, octave_ref, noise_px, stereo_frac, has_mp_frac, off_octave_frac, distortion, tree, scale, keep_order):
    """observe the world points Xw (row i carries descriptor desc_w[i]) from the pose (R, t); returns the key-frame dict and
    src[n] = the world point of every feature"""
    nlevels = len(scale)
    Xc = Xw @ R.T + t
    z = Xc[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        u = cam["fx"] * Xc[:, 0] / z + cam["cx"]
        v = cam["fy"] * Xc[:, 1] / z + cam["cy"]
    vis = (z > 0.3) & (u >= 0) & (u < W) & (v >= 0) & (v < H)
    src = np.nonzero(vis)[0]
    if not keep_order:
        src = rs.permutation(src)
    n = len(src)
    dist = np.linalg.norm(Xc[src], axis=1)
    octave = np.rint(np.log(np.maximum(dist / octave_ref, 1e-6)) / np.log(1.2)).astype(np.int64)
    off = rs.uniform(size=n) < off_octave_frac
    octave = np.clip(octave + np.where(off, rs.choice([-2, -1, 1, 2], n), 0), 0, nlevels - 1).astype(np.int32)
    sig = scale[octave]
    x = (u[src] + rs.normal(0, noise_px, n) * sig).astype(np.float32)
    y = (v[src] + rs.normal(0, noise_px, n) * sig).astype(np.float32)
    is_st = rs.uniform(size=n) < stereo_frac
    ur_true = u[src] - cam["mbf"] / z[src]
    u_right = np.where(is_st, ur_true + rs.normal(0, noise_px, n) * sig, -1.0).astype(np.float32)
    is_st &= (u_right >= 0) & (x - u_right > 0.5)
    u_right = np.where(is_st, u_right, np.float32(-1.0)).astype(np.float32)
    depth = np.where(is_st, np.float32(cam["mbf"]) / np.maximum(x - u_right, np.float32(1e-3)), np.float32(-1.0)).astype(np.float32)    # mvDepth = mbf / disparity
    desc = _flip(rs, desc_w[src], 0.03)
    nodes, offs, feat = synth.feature_vector(synth.assign_nodes(desc, tree))
    Ow = -R.T @ t
    kf = dict(desc=np.ascontiguousarray(desc), x=x, y=y, octave=octave, angle=rs.uniform(0, 360, n).astype(np.float32),
              has_mp=(rs.uniform(size=n) < has_mp_frac).astype(np.uint8), stereo=is_st.astype(np.uint8), fv=(nodes, offs, feat),
              u_right=u_right, depth=depth, key_x=None, key_y=None,
              Rcw=np.ascontiguousarray(R, np.float32), tcw=t.astype(np.float32), Ow=Ow.astype(np.float32),
              fx=np.float32(cam["fx"]), fy=np.float32(cam["fy"]), cx=np.float32(cam["cx"]), cy=np.float32(cam["cy"]),
              invfx=np.float32(1.0) / np.float32(cam["fx"]), invfy=np.float32(1.0) / np.float32(cam["fy"]),
              mb=np.float32(cam["mb"]), mbf=np.float32(cam["mbf"]),
              level_sigma2=(scale * scale).astype(np.float32), scale_factors=scale.astype(np.float32))
    if distortion:
        kf["key_x"], kf["key_y"] = _distort(x, y, cam, distortion)
    return kf, src


def make_mapping_scene(seed, n=1000, n_neighbours=10, stereo_frac=0.0, nlevels=8, noise_px=0.7, wrong_frac=0.1, has_mp_frac=0.25,
                       off_octave_frac=0.15, clutter_frac=0.2, distortion=0.0, inertial=False, far_points=False, th_far=9.0,
                       coarse_neighbour=None, max_baseline=0.6):
    """A real 3-D scene.  World points at depths 2-12 in front of the current key frame; n_neighbours poses whose baselines
    spread from a few centimetres to max_baseline, so that the parallax gate cuts both ways; projections carry pixel noise
    scaled by the octave; octaves follow the distance (off by one or two levels for off_octave_frac of the observations, which
    the scale gate then rejects or not); descriptors sit near the level-2 centroids of synth.make_tree, a new draw of 3 % of the
    bits per observation; has_mp_frac of the features already hold map points; stereo_frac of the key points carry a
    consistent u_right / depth; wrong_frac of a neighbour's observations carry the descriptor of a point seen at a wrong depth
    along the same ray of key frame 1 (on its epipolar line: the search accepts it, the geometry has to judge it); clutter_frac
    more features per neighbour match nothing.  Returns dict(kf1, neighbours, pairs, params, truth)."""
    rs = np.random.RandomState(424242 + seed)
    tree = synth.make_tree(seed)
    scale = (1.2 ** np.arange(nlevels)).astype(np.float32)
    fx = 458.0
    cam = dict(fx=fx, fy=457.0, cx=367.0, cy=248.0, mb=0.11, mbf=0.11 * fx)
    R1 = _rot(rs.normal(0, 0.05, 3))
    t1 = rs.normal(0, 0.3, 3)
    # world points through key frame 1's pixels
    u, v, z = rs.uniform(5, W - 5, n), rs.uniform(5, H - 5, n), rs.uniform(2.0, 12.0, n)
    Xc1 = np.stack([(u - cam["cx"]) / cam["fx"] * z, (v - cam["cy"]) / cam["fy"] * z, z], 1)
    Xw = (Xc1 - t1) @ R1
    l2 = tree[1]
    desc_w = _flip(rs, l2[rs.randint(0, len(l2), n)], 0.2)
    kf1, src1 = _key_frame(rs, cam, R1, t1, Xw, desc_w, 2.0, noise_px, stereo_frac, has_mp_frac, off_octave_frac, distortion, tree, scale, True)
    Ow1 = -R1.T @ t1
    neighbours, pairs, truth = [], [], []
    base = rs.permutation(np.geomspace(0.02, max_baseline, max(n_neighbours, 1)))
    for j in range(n_neighbours):
        d = rs.normal(0, 1, 3) * np.array([1.0, 0.4, 0.6])
        Ow2 = Ow1 + R1.T @ (d / np.linalg.norm(d) * base[j])
        R2 = _rot(rs.normal(0, 0.03, 3)) @ R1
        t2 = -R2 @ Ow2
        # the wrong ones: a point of the cloud moved along its key-frame-1 ray keeps its descriptor
        wrong = rs.uniform(size=n) < wrong_frac
        Xj = np.where(wrong[:, None], Ow1 + (Xw - Ow1) * rs.choice([0.35, 0.6, 1.7, 2.6], n)[:, None], Xw)
        n_cl = int(clutter_frac * n)
        Xcl = np.stack([rs.uniform(-6, 6, n_cl), rs.uniform(-4, 4, n_cl), rs.uniform(2, 12, n_cl)], 1)
        dcl = _flip(rs, l2[rs.randint(0, len(l2), n_cl)], 0.2)
        kf2, src2 = _key_frame(rs, cam, R2, t2, np.concatenate([Xj, (Xcl - t1) @ R1]), np.concatenate([desc_w, dcl]), 2.0,
                               noise_px, stereo_frac, has_mp_frac, off_octave_frac, distortion, tree, scale, False)
        ep, F12 = epipole_and_F12(kf1, kf2)
        neighbours.append(kf2)
        pairs.append(dict(ep=ep, F12=F12, coarse=(j == coarse_neighbour)))
        truth.append(dict(point=np.where(src2 < n, src2, -1), wrong=np.where(src2 < n, wrong[np.minimum(src2, n - 1)], False)))
    params = dict(inertial=bool(inertial), far_points=bool(far_points), th_far=float(th_far), scale_factor_1=1.2)
    return dict(kf1=kf1, neighbours=neighbours, pairs=pairs, params=params, truth=dict(Xw=Xw, point1=src1, neighbours=truth))
