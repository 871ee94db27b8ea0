"""float32 numpy restatement of what include/orbslam3_hip_track_project.h computes, written from the reference sources -- one numpy
operation per reference operation, vectorised over rows:
  frame_pose     src/Optimizer.cc:1108-1111 (cast, Sophus::SO3f's normalising constructor, Thirdparty/Sophus/sophus/so3.hpp:297-303)
                 and Frame::UpdatePoseMatrices, src/Frame.cc:559-566 (SE3f::inverse, se3.hpp:208-211; Eigen's toRotationMatrix and
                 _transformVector)
  frustum        Frame::isInFrustum, src/Frame.cc:599-661, inside the loop of Tracking::SearchLocalPoints, src/Tracking.cc:3512-3530,
                 with MapPoint::PredictScale, src/MapPoint.cc:531-546, and Get{Min,Max}DistanceInvariance, :502-512
  project_last   src/ORBmatcher.cc:1695-1718
  handover       src/Tracking.cc:3055-3079 and :3490-3507
Conventions a real Eigen build leaves unpinned (stated in the public header): a fixed-size reduction of three terms is
a0*b0 + (a1*b1 + a2*b2); Quaternionf::norm() sums its squares as (x*x + z*z) + (y*y + w*w).

Test infrastructure only: the product never imports it."""
import numpy as np

F32 = np.float32
INT_MIN = -2 ** 31
LEVEL_TIE = 2.0 ** -16          # rows with |q - rint(q)| <= LEVEL_TIE * max(1, |q|) may take either neighbouring level


def _f(a):
    return np.asarray(a, F32)


def dot3(a0, a1, a2, b0, b1, b2):
    return a0 * b0 + (a1 * b1 + a2 * b2)


def norm3(a0, a1, a2):
    return np.sqrt(a0 * a0 + (a1 * a1 + a2 * a2))


def norm4(q):
    return np.sqrt((q[..., 0] * q[..., 0] + q[..., 2] * q[..., 2]) + (q[..., 1] * q[..., 1] + q[..., 3] * q[..., 3]))


def quat_rotate(q, v):
    """Eigen QuaternionBase::_transformVector: uv = q.vec().cross(v); uv += uv; v + q.w()*uv + q.vec().cross(uv)"""
    q0, q1, q2, q3 = (q[..., i] for i in range(4))
    v0, v1, v2 = (v[..., i] for i in range(3))
    ux = q1 * v2 - q2 * v1; uy = q2 * v0 - q0 * v2; uz = q0 * v1 - q1 * v0
    ux = ux + ux; uy = uy + uy; uz = uz + uz
    return np.stack([v0 + q3 * ux + (q1 * uz - q2 * uy),
                     v1 + q3 * uy + (q2 * ux - q0 * uz),
                     v2 + q3 * uz + (q0 * uy - q1 * ux)], -1)


def quat_to_R(q):
    """Eigen QuaternionBase::toRotationMatrix, row major [..., 9]"""
    x, y, z, w = (q[..., i] for i in range(4))
    two = F32(2); one = F32(1)
    tx = two * x; ty = two * y; tz = two * z
    twx = tx * w; twy = ty * w; twz = tz * w
    txx = tx * x; txy = ty * x; txz = tz * x
    tyy = ty * y; tyz = tz * y; tzz = tz * z
    return np.stack([one - (tyy + tzz), txy - twz, txz + twy,
                     txy + twz, one - (txx + tzz), tyz - twx,
                     txz - twy, tyz + twx, one - (txx + tyy)], -1)


def frame_pose(pose7, normalise):
    """[batch][7] double -> dict(q [batch][4], Rcw [batch][9], tcw, Ow [batch][3]) float32"""
    pose7 = np.asarray(pose7, np.float64)
    q = pose7[:, :4].astype(F32)                        # .cast<float>()
    tcw = pose7[:, 4:].astype(F32)
    if normalise:
        q = q / norm4(q)[:, None]                       # SO3f(quaternion): coeffs() /= norm()
    c = q * _f([-1, -1, -1, 1])                         # conjugate (a sign flip is exact)
    c = c / norm4(c)[:, None]                           # SO3f(conjugate) normalises again
    Ow = quat_rotate(c, tcw * F32(-1))
    return dict(q=q, Rcw=quat_to_R(q), tcw=tcw, Ow=Ow)


def frame_pose_record(fp):
    """the OrbmFramePose records as a [batch][19] float32 array"""
    return np.ascontiguousarray(np.concatenate([fp["q"], fp["Rcw"], fp["tcw"], fp["Ow"]], 1), F32)


def predict_scale(max_distance, dist, log_scale_factor, n_levels):
    """MapPoint::PredictScale(currentDist, Frame*): (level, q) with q the float64 quotient, for the tie rule"""
    ratio = max_distance / dist
    s = np.ceil(np.log(ratio) / F32(log_scale_factor))
    assert s.dtype == F32
    inside = (s >= F32(-2.0 ** 31)) & (s < F32(2.0 ** 31))     # cvttss2si: NaN and out-of-range give INT_MIN
    n = np.where(inside, np.where(inside, s, 0).astype(np.int64), INT_MIN)
    n = np.where(n < 0, 0, np.where(n >= n_levels, n_levels - 1, n))
    with np.errstate(all="ignore"):
        q = np.log(ratio.astype(np.float64)) / np.float64(F32(log_scale_factor))
    return n.astype(np.int32), q


def frustum(case, fp=None, normalise=1):
    """the loop :3512-3530 over every frame's rows; returns the arrays of OrbmFrustumOut plus level_q (float64 log quotient, NaN
    where the row never reached PredictScale) and PcZ"""
    cam = case["cam"]
    fp = fp or frame_pose(case["pose7"], normalise)
    B, pcap = case["skip"].shape
    P = _f(case["xyz"]); Pn = _f(case["normal"])
    R = fp["Rcw"][:, None, :]; t = fp["tcw"][:, None, :]; Ow = fp["Ow"][:, None, :]
    live = (np.arange(pcap)[None, :] < np.asarray(case["n"])[:, None]) & (case["skip"] == 0) & (case["bad"] == 0)
    with np.errstate(all="ignore"):
        Pc0 = dot3(R[..., 0], R[..., 1], R[..., 2], P[..., 0], P[..., 1], P[..., 2]) + t[..., 0]
        Pc1 = dot3(R[..., 3], R[..., 4], R[..., 5], P[..., 0], P[..., 1], P[..., 2]) + t[..., 1]
        PcZ = dot3(R[..., 6], R[..., 7], R[..., 8], P[..., 0], P[..., 1], P[..., 2]) + t[..., 2]
        Pc_dist = norm3(Pc0, Pc1, PcZ)
        invz = F32(1.0) / PcZ
        alive = live & ~(PcZ < F32(0.0))                                    # if(PcZ<0.0f) return false;
        uv0 = cam["fx"] * Pc0 / PcZ + cam["cx"]
        uv1 = cam["fy"] * Pc1 / PcZ + cam["cy"]
        alive = alive & ~((uv0 < cam["min_x"]) | (uv0 > cam["max_x"]))
        alive = alive & ~((uv1 < cam["min_y"]) | (uv1 > cam["max_y"]))
        stored = alive.copy()                                               # mTrackProjX / Y = uv (:626-627)
        maxDistance = F32(1.2) * _f(case["max_distance"])
        minDistance = F32(0.8) * _f(case["min_distance"])
        PO = P - Ow
        dist = norm3(PO[..., 0], PO[..., 1], PO[..., 2])
        alive = alive & ~((dist < minDistance) | (dist > maxDistance))
        viewCos = dot3(PO[..., 0], PO[..., 1], PO[..., 2], Pn[..., 0], Pn[..., 1], Pn[..., 2]) / dist
        alive = alive & ~(viewCos < F32(case["cos_limit"]))
        level, q = predict_scale(_f(case["max_distance"]), dist, cam["log_scale_factor"], cam["n_levels"])
        ur = uv0 - cam["bf"] * invz
    for a in (Pc0, uv0, dist, viewCos, ur):
        assert a.dtype == F32
    z = np.zeros((B, pcap), F32)
    return dict(valid=alive.astype(np.uint8), u=np.where(stored, uv0, F32(-1)), v=np.where(stored, uv1, F32(-1)),
                octave=np.where(alive, level, -1).astype(np.int32), view_cos=np.where(alive, viewCos, z), track_depth=np.where(alive, Pc_dist, z),
                proj_ur=np.where(alive, ur, z), n_to_match=alive.sum(1).astype(np.int32), level_q=np.where(alive, q, np.nan), PcZ=PcZ)


def project_last(case, fp=None, normalise=1, through_matrix=False):
    """:1695-1718 per last-frame feature; through_matrix = True computes x3Dc as Rcw*x + tcw instead (NOT what the reference does:
    the GPU test uses it to show that the two forms differ)"""
    cam = case["cam"]
    fp = fp or frame_pose(case["pose7"], normalise)
    B, cap = case["has_point"].shape
    x = _f(case["xyz"])
    live = (np.arange(cap)[None, :] < np.asarray(case["n"])[:, None]) & (case["has_point"] != 0)
    with np.errstate(all="ignore"):
        if through_matrix:
            R = fp["Rcw"][:, None, :]
            xc = np.stack([dot3(R[..., 3 * r], R[..., 3 * r + 1], R[..., 3 * r + 2], x[..., 0], x[..., 1], x[..., 2]) for r in range(3)], -1) + fp["tcw"][:, None, :]
        else:
            xc = quat_rotate(fp["q"][:, None, :], x) + fp["tcw"][:, None, :]       # Tcw * x3Dw
        invzc = (1.0 / xc[..., 2].astype(np.float64)).astype(F32)
        alive = live & ~(invzc < 0)
        uv0 = cam["fx"] * xc[..., 0] / xc[..., 2] + cam["cx"]
        uv1 = cam["fy"] * xc[..., 1] / xc[..., 2] + cam["cy"]
        alive = alive & ~((uv0 < cam["min_x"]) | (uv0 > cam["max_x"]))
        alive = alive & ~((uv1 < cam["min_y"]) | (uv1 > cam["max_y"]))
        ur = uv0 - cam["bf"] * invzc
    assert uv0.dtype == F32 and ur.dtype == F32
    return dict(valid=alive.astype(np.uint8), u=np.where(alive, uv0, F32(-1)), v=np.where(alive, uv1, F32(-1)),
                proj_ur=np.where(alive, ur, F32(0)), x3Dc=xc)


def handover(assign, outlier, n_cur, last_local, bad, has_obs):
    """the sequential loops :3057-3079 and :3490-3507 for [batch][...] arrays"""
    B, cap = assign.shape
    pcap = bad.shape[1]
    assign_local = np.full((B, cap), -1, np.int32); occupied = np.zeros((B, cap), np.uint8)
    skip = np.zeros((B, pcap), np.uint8); dropped = np.zeros(B, np.int32)
    for b in range(B):
        for i in range(min(int(n_cur[b]), cap)):
            a = int(assign[b, i])
            if a < 0:
                continue                                    # mvpMapPoints[i] == NULL
            row = int(last_local[b, a]) if a < last_local.shape[1] else -1
            if row < 0 or row >= pcap:
                dropped[b] += 1
                continue
            # mnLastFrameSeen = mCurrentFrame.mnId: :3073 for outliers, :3502 for the rest.  (A bad point is not stamped by the
            # reference; the entry stamps it too, which changes nothing: the loop :3518 skips a bad point anyway.)
            skip[b, row] = 1
            if outlier[b, i]:
                continue                                    # mvpMapPoints[i] = NULL (:3065)
            if bad[b, row]:
                continue                                    # *vit = NULL (:3497)
            assign_local[b, i] = row
            occupied[b, i] = 1 if has_obs[b, row] else 0
    return dict(assign_local=assign_local, occupied=occupied, skip=skip, n_dropped=dropped)


def level_mismatches(level, ref, n_levels):
    """Levels against a frustum() result.  A row whose quotient q = log(ratio)/log_scale_factor lies within LEVEL_TIE of an integer
    k is a tie: float logs that differ in the last bit may put ceil() on either side, so it may hold level k or k + 1 (clamped).
    Returns (rows that are wrong, tie rows)."""
    q = ref["level_q"]
    with np.errstate(all="ignore"):
        tie = (ref["valid"] != 0) & np.isfinite(q) & (np.abs(q - np.rint(q)) <= LEVEL_TIE * np.maximum(1.0, np.abs(q)))
    k = np.where(tie, np.rint(np.where(tie, q, 0)), 0)
    lo = np.clip(k, 0, n_levels - 1); hi = np.clip(k + 1, 0, n_levels - 1)
    wrong = np.where(tie, (level != lo) & (level != hi), level != ref["octave"])
    return int(wrong.sum()), int(tie.sum())
