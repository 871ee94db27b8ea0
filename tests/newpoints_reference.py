"""Independent numpy restatement of the per-match geometry of LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:
561-695, GeometricTools::Triangulate src/GeometricTools.cc:47-66, KeyFrame::UnprojectStereo src/KeyFrame.cc:755-772), written
from the reference source and parameterised by dtype.  Besides the decision it returns the signed margin of every gate the
pair reaches, so that a test can tell a decision that hangs on the last bits of a float from one that does not.

Test infrastructure only: the product never imports it."""
import numpy as np

# guard bands (a float cosine carries a few 6e-8; the other gates are ratios of float expressions of a few operations)
GUARD_COS = 1e-6        # absolute, on every comparison between parallax cosines
GUARD_REL = 1e-3        # relative (value / threshold - 1) on the reprojection, far-point and scale gates
GUARD_DEPTH = 1e-3      # z / distance on the two depth signs

QUIRKS = dict(mbf_of_kf1=True,          # :669: the neighbour's right-image error uses key frame 1's mbf
              else_if_stereo2=True,     # :575: cosParallaxStereo2 is not computed when key point 1 is stereo
              unproject_distorted=True, # KeyFrame.cc:760-761: UnprojectStereo reads mvKeys, not mvKeysUn
              double_thresholds=True)   # :637 / :649: 5.991 and 7.8 are doubles, the comparison runs in double


def camera_of(kf):
    return {k: kf[k] for k in ("Rcw", "tcw", "Ow", "fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")}


def obs_of(kf, i):
    o = int(kf["octave"][i])
    kx = kf["x"][i] if kf.get("key_x") is None else kf["key_x"][i]
    ky = kf["y"][i] if kf.get("key_y") is None else kf["key_y"][i]
    return dict(x=kf["x"][i], y=kf["y"][i], ur=kf["u_right"][i], depth=kf["depth"][i], kx=kx, ky=ky,
                sigma2=kf["level_sigma2"][o], scale=kf["scale_factors"][o])


def null_vector_svd(A):
    """svd.matrixV().col(3)"""
    return np.linalg.svd(A)[2][3]


def null_vector_eig_longdouble(A, sweeps=12):
    """eigenvector of the smallest eigenvalue of A^T A by cyclic Jacobi in long double (numpy has no long-double LAPACK)"""
    M = A.astype(np.longdouble).T @ A.astype(np.longdouble)
    V = np.eye(4, dtype=np.longdouble)
    for _ in range(sweeps):
        for p in range(3):
            for q in range(p + 1, 4):
                if M[p, q] == 0:
                    continue
                th = (M[q, q] - M[p, p]) / (2 * M[p, q])
                t = np.sign(th) / (abs(th) + np.sqrt(th * th + 1)) if th != 0 else np.longdouble(1)
                c = 1 / np.sqrt(t * t + 1)
                s = t * c
                J = np.eye(4, dtype=np.longdouble)
                J[p, p] = c; J[q, q] = c; J[p, q] = s; J[q, p] = -s
                M = J.T @ M @ J
                V = V @ J
    return V[:, int(np.argmin(np.diag(M)))]


def chi2_threshold(chi, sigma2, double_thresholds=True):
    """5.991 * sigmaSquare as the reference evaluates it: the literal is a double, so the float sigma is promoted (:637, :649)"""
    return chi * float(sigma2) if double_thresholds else float(np.float32(chi) * np.float32(sigma2))


def triangulation_matrix(xn1, xn2, T1, T2, T):
    return np.stack([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]]).astype(T)


def triangulate(xn1, xn2, T1, T2, T):
    A = triangulation_matrix(xn1, xn2, T1, T2, T)
    v = null_vector_svd(A)
    if v[3] == 0:
        return None
    return (v[:3] / v[3]).astype(T)


def _unproject_stereo(C, o, T, distorted):
    z = T(o["depth"])
    if not z > 0:
        return None
    u, v = (T(o["kx"]), T(o["ky"])) if distorted else (T(o["x"]), T(o["y"]))
    x3Dc = np.array([(u - C["cx"]) * z * C["invfx"], (v - C["cy"]) * z * C["invfy"], z], T)
    return (C["Rcw"].T @ x3Dc + C["Ow"]).astype(T)


def _cast(C, T):
    c = {k: T(C[k]) for k in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf")}
    c["Rcw"] = np.asarray(C["Rcw"], np.float32).reshape(3, 3).astype(T)
    c["tcw"] = np.asarray(C["tcw"], np.float32).astype(T)
    c["Ow"] = np.asarray(C["Ow"], np.float32).astype(T)
    return c


def pair_geometry(cam1, obs1, cam2, obs2, rule, dtype=np.float64, quirks=None, matrix_dtype=None):
    """One (key frame 1 feature, neighbour feature) match through :561-695.  rule = dict(inertial, far_points, th_far,
    scale_factor_1).  Returns dict(accept, x3d, point_stereo, margins=[(gate, signed margin, guard)], undecided, sin_parallax);
    a margin is positive when the pair passes that comparison the way it went.  matrix_dtype = np.float32 builds Triangulate's
    4x4 matrix in float (as the reference and the kernel do) and takes its null vector in `dtype`."""
    T = dtype
    q = dict(QUIRKS)
    q.update(quirks or {})
    C1, C2 = _cast(cam1, T), _cast(cam2, T)
    o1 = {k: T(v) for k, v in obs1.items()}
    o2 = {k: T(v) for k, v in obs2.items()}
    margins = []
    out = dict(accept=False, x3d=None, point_stereo=False, margins=margins, sin_parallax=None)

    def finish():
        out["undecided"] = any(abs(m) < g for _, m, g in margins)
        return out

    def gate(name, value, guard):
        """records `value` (> 0 means the condition holds) and returns whether it holds"""
        margins.append((name, float(value), guard))
        return value > 0

    bS1, bS2 = o1["ur"] >= 0, o2["ur"] >= 0
    xn1 = np.array([(o1["x"] - C1["cx"]) / C1["fx"], (o1["y"] - C1["cy"]) / C1["fy"], T(1)], T)
    xn2 = np.array([(o2["x"] - C2["cx"]) / C2["fx"], (o2["y"] - C2["cy"]) / C2["fy"], T(1)], T)
    ray1, ray2 = C1["Rcw"].T @ xn1, C2["Rcw"].T @ xn2
    cosR = T(ray1.dot(ray2) / (np.linalg.norm(ray1) * np.linalg.norm(ray2)))
    out["sin_parallax"] = float(np.sqrt(max(0.0, 1.0 - float(cosR) ** 2)))
    cosS1 = cosS2 = T(cosR + T(1))
    if bS1:
        cosS1 = T(np.cos(T(2) * np.arctan2(C1["mb"] / T(2), o1["depth"])))
    if bS2 and (not bS1 or not q["else_if_stereo2"]):
        cosS2 = T(np.cos(T(2) * np.arctan2(C2["mb"] / T(2), o2["depth"])))
    cosS = min(cosS1, cosS2)

    # the three-way branch (:586-608); every cosine comparison it evaluates is recorded with the sign it came out with
    def cmp(name, a, b):        # a < b
        r = a < b
        margins.append((name, float(b - a) if r else float(a - b), GUARD_COS))
        return r

    x3D = None
    tri = cmp("cosRays<cosStereo", cosR, cosS) and cmp("cosRays>0", T(0), cosR)
    if tri and not (bS1 or bS2):
        bound = 0.9996 if rule["inertial"] else 0.9998
        tri = cmp("cosRays<bound", float(cosR), bound)
    if tri:
        T1 = np.concatenate([C1["Rcw"], C1["tcw"][:, None]], 1)
        T2 = np.concatenate([C2["Rcw"], C2["tcw"][:, None]], 1)
        if matrix_dtype is not None:
            M = matrix_dtype
            a1, a2 = _cast(cam1, M), _cast(cam2, M)
            m1 = np.array([(M(obs1["x"]) - a1["cx"]) / a1["fx"], (M(obs1["y"]) - a1["cy"]) / a1["fy"]], M)
            m2 = np.array([(M(obs2["x"]) - a2["cx"]) / a2["fx"], (M(obs2["y"]) - a2["cy"]) / a2["fy"]], M)
            A = triangulation_matrix(m1, m2, np.concatenate([a1["Rcw"], a1["tcw"][:, None]], 1), np.concatenate([a2["Rcw"], a2["tcw"][:, None]], 1), M)
            v = null_vector_svd(A.astype(T))
            x3D = None if v[3] == 0 else (v[:3] / v[3]).astype(T)
        else:
            x3D = triangulate(xn1, xn2, T1, T2, T)
        if x3D is None:
            return finish()
    elif bS1 and cmp("cosStereo1<cosStereo2", cosS1, cosS2):
        out["point_stereo"] = True
        x3D = _unproject_stereo(C1, o1, T, q["unproject_distorted"])
    elif bS2 and cmp("cosStereo2<cosStereo1", cosS2, cosS1):
        out["point_stereo"] = True
        x3D = _unproject_stereo(C2, o2, T, q["unproject_distorted"])
    if x3D is None:
        return finish()
    out["x3d"] = x3D

    d1, d2 = T(np.linalg.norm(x3D - C1["Ow"])), T(np.linalg.norm(x3D - C2["Ow"]))
    z1 = T(C1["Rcw"][2].dot(x3D) + C1["tcw"][2])
    if not gate("z1>0", z1 / max(d1, T(1e-30)), GUARD_DEPTH):
        return finish()
    z2 = T(C2["Rcw"][2].dot(x3D) + C2["tcw"][2])
    if not gate("z2>0", z2 / max(d2, T(1e-30)), GUARD_DEPTH):
        return finish()

    def reproj(tag, C, o, stereo, z, mbf):
        x = T(C["Rcw"][0].dot(x3D) + C["tcw"][0])
        y = T(C["Rcw"][1].dot(x3D) + C["tcw"][1])
        if not stereo:
            ex = T(C["fx"] * x / z + C["cx"]) - o["x"]
            ey = T(C["fy"] * y / z + C["cy"]) - o["y"]
            e2, chi = T(ex * ex + ey * ey), 5.991
        else:
            invz = T(1.0 / float(z))
            u = T(C["fx"] * x * invz + C["cx"])
            ex, ey, er = u - o["x"], T(C["fy"] * y * invz + C["cy"]) - o["y"], T(u - mbf * invz) - o["ur"]
            e2, chi = T(ex * ex + ey * ey + er * er), 7.8
        th = chi2_threshold(chi, o["sigma2"], q["double_thresholds"])
        return gate(tag, 1.0 - float(e2) / th, GUARD_REL)      # passes when NOT e2 > th

    if not reproj("reproj1", C1, o1, bS1, z1, C1["mbf"]):
        return finish()
    if not reproj("reproj2", C2, o2, bS2, z2, C1["mbf"] if q["mbf_of_kf1"] else C2["mbf"]):
        return finish()
    if d1 == 0 or d2 == 0:
        return finish()
    if rule["far_points"]:
        th_far = T(np.float32(rule["th_far"]))
        if not (gate("far1", 1.0 - float(d1) / float(th_far), GUARD_REL) and gate("far2", 1.0 - float(d2) / float(th_far), GUARD_REL)):
            return finish()
    ratioDist = T(d2 / d1)
    ratioFactor = T(np.float32(1.5) * np.float32(rule["scale_factor_1"]))
    ratioOctave = T(o1["scale"] / o2["scale"])
    if not gate("scale_lo", float(ratioDist * ratioFactor) / float(ratioOctave) - 1.0, GUARD_REL):       # NOT ratioDist*ratioFactor < ratioOctave
        return finish()
    if not gate("scale_hi", 1.0 - float(ratioDist) / float(ratioOctave * ratioFactor), GUARD_REL):       # NOT ratioDist > ratioOctave*ratioFactor
        return finish()
    out["accept"] = True
    return finish()


def normal_and_depth(x3d, Ow1, Ow2, level_scale, last_scale, T=np.float64):
    """MapPoint::UpdateNormalAndDepth with the observations (kf1, neighbour), pRefKF = kf1"""
    x3d, Ow1, Ow2 = np.asarray(x3d, T), np.asarray(Ow1, T), np.asarray(Ow2, T)
    n = (x3d - Ow1) / np.linalg.norm(x3d - Ow1) + (x3d - Ow2) / np.linalg.norm(x3d - Ow2)
    mx = np.linalg.norm(x3d - Ow1) * T(level_scale)
    return n / 2, mx, mx / T(last_scale)


def create_new_map_points(scene, search, dtype=np.float64, quirks=None):
    """The composite reference: for each neighbour in order, search(j, has_mp1) -> match12 with the current has_mp of key frame
    1, then pair_geometry on the matches, then has_mp for the accepted ones.  Returns per-feature arrays (neighbour, idx2, x3d,
    point_stereo, undecided_from = first neighbour at which the feature met an undecided pair or -1), per-neighbour n_matched /
    n_created, and the list of reached pairs: (idx1, j, idx2, accept, undecided, sin_parallax, x3d, margins)."""
    kf1, nbs, rule = scene["kf1"], scene["neighbours"], scene["params"]
    n1 = len(kf1["x"])
    has_mp = np.ascontiguousarray(kf1["has_mp"]).copy()
    res = dict(neighbour=np.full(n1, -1, np.int32), idx2=np.full(n1, -1, np.int32), x3d=np.zeros((n1, 3), dtype),
               point_stereo=np.zeros(n1, np.uint8), undecided_from=np.full(n1, -1, np.int32),
               n_matched=np.zeros(len(nbs), np.int32), n_created=np.zeros(len(nbs), np.int32), pairs=[], match12=[])
    C1 = camera_of(kf1)
    for j, kf2 in enumerate(nbs):
        m12 = np.asarray(search(j, has_mp))
        res["match12"].append(m12.copy())
        res["n_matched"][j] = int((m12 >= 0).sum())
        C2 = camera_of(kf2)
        for i1 in np.nonzero(m12 >= 0)[0]:
            i2 = int(m12[i1])
            g = pair_geometry(C1, obs_of(kf1, i1), C2, obs_of(kf2, i2), rule, dtype, quirks)
            res["pairs"].append((int(i1), j, i2, g["accept"], g["undecided"], g["sin_parallax"], g["x3d"], g["margins"]))
            if g["undecided"] and res["undecided_from"][i1] < 0:
                res["undecided_from"][i1] = j
            if g["accept"]:
                has_mp[i1] = 1
                res["neighbour"][i1], res["idx2"][i1], res["x3d"][i1], res["point_stereo"][i1] = j, i2, g["x3d"], g["point_stereo"]
                res["n_created"][j] += 1
    return res


def numpy_search(scene):
    """SearchForTriangulation (src/ORBmatcher.cc:907-1146, bOnlyStereo = false, no rotation histogram) in plain numpy: the
    sequential `dist > bestDist -> continue` loop, for scenes measured where the C++ oracle is not at hand"""
    kf1 = scene["kf1"]
    bits1 = np.unpackbits(kf1["desc"], axis=1)

    def search(j, has_mp1):
        kf2, pr = scene["neighbours"][j], scene["pairs"][j]
        F = np.asarray(pr["F12"], np.float32)
        bits2 = np.unpackbits(kf2["desc"], axis=1)
        m12 = np.full(len(kf1["x"]), -1, np.int32)
        n2, o2, f2 = kf2["fv"]
        at2 = {int(k): a for a, k in enumerate(n2)}
        n1, o1, f1 = kf1["fv"]
        for a, node in enumerate(n1):
            if int(node) not in at2:
                continue
            b = at2[int(node)]
            for i1 in f1[o1[a]:o1[a + 1]]:
                if has_mp1[i1]:
                    continue
                x, y = kf1["x"][i1], kf1["y"][i1]
                la = np.float32(x * F[0] + y * F[3]) + F[6]
                lb = np.float32(x * F[1] + y * F[4]) + F[7]
                lc = np.float32(x * F[2] + y * F[5]) + F[8]
                den = np.float32(la * la + lb * lb)
                best, besti = 50, -1
                for i2 in f2[o2[b]:o2[b + 1]]:
                    if kf2["has_mp"][i2]:
                        continue
                    dist = int((bits1[i1] != bits2[i2]).sum())
                    if dist > 50 or dist > best:
                        continue
                    kx, ky, oc = kf2["x"][i2], kf2["y"][i2], kf2["octave"][i2]
                    if not kf1["stereo"][i1] and not kf2["stereo"][i2]:
                        ex, ey = np.float32(pr["ep"][0]) - kx, np.float32(pr["ep"][1]) - ky
                        if np.float32(ex * ex + ey * ey) < np.float32(100) * kf2["scale_factors"][oc]:
                            continue
                    ok = bool(pr["coarse"])
                    if not ok and den != 0:
                        num = np.float32(np.float32(la * kx + lb * ky) + lc)
                        ok = float(np.float32(num * num / den)) < 3.84 * float(kf2["level_sigma2"][oc])
                    if ok:
                        best, besti = dist, int(i2)
                m12[i1] = besti
        return m12

    return search
