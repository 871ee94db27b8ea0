"""float32 numpy restatement of what include/orbslam3_hip_track_project_rig.h computes, written from the reference sources -- one
numpy operation per reference operation, vectorised over rows:
  rig_frame_pose   Frame::UpdatePoseMatrices (src/Frame.cc:559-566: mRwc is the matrix of Twc's quaternion, the renormalised
                   conjugate) and the set-up of Frame::isInFrustumChecks for the right camera (:1294-1299)
  frustum          the Nleft != -1 branch of Frame::isInFrustum (:662-672) with isInFrustumChecks (:1288-1362) for both cameras,
                   inside the loop of Tracking::SearchLocalPoints (src/Tracking.cc:3490-3530), with the STALE STATE explicit: the
                   MapPoint members come in as case["state"] and go out as the result
  project_last     src/ORBmatcher.cc:1695-1718 and :1794-1796
  unproject        Frame::UnprojectStereoFishEye (src/Frame.cc:1364)
KannalaBrandt8::project is fisheye_stereo_reference.project: atan2 / sin / cos are the float rounding of the float64 function.

Every comparison returns a signed margin (positive: it went the way that keeps the row alive) and a guard; a row is OPEN when a
comparison it reached lies inside its guard.  Comparisons without a transcendental are float operations that every build repeats bit
for bit: guard 0.  The image-bounds tests compare u = fx*r*cos(psi) + cx: implementations agree on atan2 / sin / cos to a float ulp,
which the polynomial and the products carry into u; the bar for KannalaBrandt8 projections is the project's 4 x SPREAD_F32
(rig_newpoints_reference), relative to the magnitudes that are added: guard = 4 * SPREAD_F32 * (|u - cx| + |cx|).  Where r == 0 (a
point on the optical axis: atan2(0, z) = 0 exactly in every libm) u == cx exactly and the guard is 0.

Test infrastructure only: the product never imports it."""
import numpy as np

import fisheye_stereo_reference as fsr
import rig_newpoints_reference as rnr
import track_project_reference as R

F32 = np.float32
KB8_BAR = 4 * rnr.SPREAD_F32
STALE = ("proj_u", "proj_v", "view_cos", "track_depth")


def _f(a):
    return np.asarray(a, F32)


def cam_dict(p8):
    p8 = _f(p8)
    return dict(fx=p8[0], fy=p8[1], cx=p8[2], cy=p8[3], k=[p8[4], p8[5], p8[6], p8[7]])


def _matvec(M, v):
    """M [..., 9] row major times v [..., 3] in Eigen's three-term order"""
    return np.stack([R.dot3(M[..., 3 * r], M[..., 3 * r + 1], M[..., 3 * r + 2], v[..., 0], v[..., 1], v[..., 2]) for r in range(3)], -1)


def rig_frame_pose(cam, pose7, normalise):
    fp = R.frame_pose(pose7, normalise)
    q = fp["q"]
    c = q * _f([-1, -1, -1, 1])
    c = c / R.norm4(c)[:, None]
    Rwc = R.quat_to_R(c)
    Rrl = _f(cam["Rrl"]).reshape(9)
    Rcw = fp["Rcw"]
    R_r = np.stack([R.dot3(Rrl[3 * r], Rrl[3 * r + 1], Rrl[3 * r + 2], Rcw[:, k], Rcw[:, 3 + k], Rcw[:, 6 + k]) for r in range(3) for k in range(3)], -1)
    t_r = _matvec(Rrl[None, :], fp["tcw"]) + _f(cam["trl"])[None, :]
    Ow_r = _matvec(Rwc, _f(cam["tlr"])[None, :]) + fp["Ow"]
    for a in (Rwc, R_r, t_r, Ow_r):
        assert a.dtype == F32
    return dict(left=fp, Rwc=Rwc, R_r=R_r, t_r=t_r, Ow_r=Ow_r)


def rig_frame_pose_record(rp):
    """the OrbmRigFramePose records as a [batch][43] float32 array"""
    return np.ascontiguousarray(np.concatenate([R.frame_pose_record(rp["left"]), rp["Rwc"], rp["R_r"], rp["t_r"], rp["Ow_r"]], 1), F32)


def _project(p8, X):
    """KannalaBrandt8::project on [..., 3] -> u, v, guard_u, guard_v"""
    shape = X.shape[:-1]
    uv = fsr.project(cam_dict(p8), X.reshape(-1, 3), F32)
    assert uv.dtype == F32
    u, v = uv[:, 0].reshape(shape), uv[:, 1].reshape(shape)
    cx, cy = _f(p8)[2], _f(p8)[3]
    on_axis = (X[..., 0] == 0) & (X[..., 1] == 0) & ~np.signbit(X[..., 2])
    gu = np.where(on_axis, 0.0, KB8_BAR * (np.abs(u.astype(np.float64) - cx) + abs(float(cx))))
    gv = np.where(on_axis, 0.0, KB8_BAR * (np.abs(v.astype(np.float64) - cy) + abs(float(cy))))
    return u, v, gu, gv


class Gates:
    """the comparisons of one side: (name, margin, guard, reached)"""

    def __init__(self, live):
        self.alive = live.copy()
        self.items = []

    def fails_if(self, name, fails, margin, guard):
        self.items.append((name, np.asarray(margin, np.float64), np.broadcast_to(np.asarray(guard, np.float64), self.alive.shape), self.alive.copy()))
        self.alive = self.alive & ~fails

    def open(self):
        o = np.zeros(self.alive.shape, bool)
        for _, m, g, reached in self.items:
            with np.errstate(invalid="ignore"):
                o |= reached & (np.abs(m) < g)
        return o


def _bounds(g, cam, u, v, gu, gv):
    with np.errstate(invalid="ignore"):
        g.fails_if("min_x", u < cam["min_x"], u.astype(np.float64) - float(cam["min_x"]), gu)
        g.alive = g.items[-1][3] & ~((u < cam["min_x"]) | (u > cam["max_x"]))         # (one `if` in the reference: both halves are reached together)
        g.items.append(("max_x", float(cam["max_x"]) - u.astype(np.float64), gu, g.items[-1][3]))
        reached = g.alive.copy()
        g.items.append(("min_y", v.astype(np.float64) - float(cam["min_y"]), gv, reached))
        g.items.append(("max_y", float(cam["max_y"]) - v.astype(np.float64), gv, reached))
        g.alive = g.alive & ~((v < cam["min_y"]) | (v > cam["max_y"]))


def _side(case, cam, p8, mR, mt, twc, live):
    """isInFrustumChecks for one camera over [B][pcap]: dict(valid, u, v, level, view_cos, depth, level_q, PcZ, gates)"""
    P = _f(case["xyz"]); Pn = _f(case["normal"])
    mR = mR[:, None, :]; mt = mt[:, None, :]; twc = twc[:, None, :]
    with np.errstate(all="ignore"):
        Pc = _matvec(mR, P) + mt
        Pc_dist = R.norm3(Pc[..., 0], Pc[..., 1], Pc[..., 2])
        PcZ = Pc[..., 2]
        g = Gates(live)
        g.fails_if("depth", PcZ < F32(0.0), PcZ, 0.0)
        u, v, gu, gv = _project(p8, Pc)
        _bounds(g, cam, u, v, gu, gv)
        maxDistance = F32(1.2) * _f(case["max_distance"])
        minDistance = F32(0.8) * _f(case["min_distance"])
        PO = P - twc
        dist = R.norm3(PO[..., 0], PO[..., 1], PO[..., 2])
        g.fails_if("dist", (dist < minDistance) | (dist > maxDistance), np.minimum(dist.astype(np.float64) - minDistance, maxDistance.astype(np.float64) - dist), 0.0)
        viewCos = R.dot3(PO[..., 0], PO[..., 1], PO[..., 2], Pn[..., 0], Pn[..., 1], Pn[..., 2]) / dist
        g.fails_if("view_cos", viewCos < F32(case["cos_limit"]), viewCos.astype(np.float64) - float(case["cos_limit"]), 0.0)
        level, q = R.predict_scale(_f(case["max_distance"]), dist, cam["log_scale_factor"], cam["n_levels"])
    for a in (Pc, Pc_dist, dist, viewCos):
        assert a.dtype == F32
    return dict(valid=g.alive, u=u, v=v, level=level, view_cos=viewCos, depth=Pc_dist, level_q=np.where(g.alive, q, np.nan), PcZ=PcZ, gates=g)


def frustum(case, rp=None, normalise=1, state=None):
    """Returns the twelve arrays of OrbmRigFrustumOut after the call, n_to_match, and for the comparison: open [B][pcap], left /
    right (the per-side dicts of _side)."""
    cam = case["cam"]
    rp = rp or rig_frame_pose(cam, case["pose7"], normalise)
    B, pcap = case["skip"].shape
    live = (np.arange(pcap)[None, :] < np.asarray(case["n"])[:, None]) & (case["skip"] == 0) & (case["bad"] == 0)
    L = _side(case, cam, cam["left"], rp["left"]["Rcw"], rp["left"]["tcw"], rp["left"]["Ow"], live)
    Rt = _side(case, cam, cam["right"], rp["R_r"], rp["t_r"], rp["Ow_r"], live)
    out = {k: np.array(v, copy=True) for k, v in (state if state is not None else case["state"]).items()}
    for s, sfx in ((L, ""), (Rt, "_r")):
        ok = s["valid"]
        out["in_view" + sfx] = ok.astype(np.uint8)                                   # skipped rows: false (:3490-3507); live rows: the verdict
        out["pred_level" + sfx] = np.where(live, np.where(ok, s["level"], -1), out["pred_level" + sfx]).astype(np.int32)
        for k, src in (("proj_u", "u"), ("proj_v", "v"), ("view_cos", "view_cos"), ("track_depth", "depth")):
            out[k + sfx] = np.where(ok, s[src], out[k + sfx]).astype(F32)
    seen = L["valid"] | Rt["valid"]
    out["n_to_match"] = seen.sum(1).astype(np.int32)
    out["open"] = L["gates"].open() | Rt["gates"].open()
    out["left"], out["right"], out["live"] = L, Rt, live
    return out


def level_mismatches(level, ref, side, n_levels):
    """track_project_reference.level_mismatches for one side of a frustum() result"""
    s = ref[side]
    return R.level_mismatches(level, dict(level_q=s["level_q"], valid=s["valid"].astype(np.uint8), octave=np.where(s["valid"], s["level"], -1)), n_levels)


def project_last(case, rp=None, normalise=1, right_camera_for_uvr=False):
    """per last-frame entry; right_camera_for_uvr = True projects x3Dr with mpCamera2 (NOT what the reference does: the tests use it
    to show that the two are told apart).  Returns valid, proj_u/v, proj_u_r/v_r, open, guards"""
    cam = case["cam"]
    rp = rp or rig_frame_pose(cam, case["pose7"], normalise)
    fp = rp["left"]
    B, cap = case["has_point"].shape
    x = _f(case["xyz"])
    live = (np.arange(cap)[None, :] < np.asarray(case["n"])[:, None]) & (case["has_point"] != 0)
    with np.errstate(all="ignore"):
        xc = R.quat_rotate(fp["q"][:, None, :], x) + fp["tcw"][:, None, :]
        invzc = (1.0 / xc[..., 2].astype(np.float64)).astype(F32)
        g = Gates(live)
        g.fails_if("invzc", invzc < 0, invzc, 0.0)
        u, v, gu, gv = _project(cam["left"], xc)
        _bounds(g, cam, u, v, gu, gv)
        xr = R.quat_rotate(_f(cam["q_rl"])[None, None, :], xc) + _f(cam["trl"])[None, None, :]
        ur, vr, gur, gvr = _project(cam["right"] if right_camera_for_uvr else cam["left"], xr)
    assert xc.dtype == F32 and xr.dtype == F32
    ok = g.alive
    m1 = F32(-1)
    return dict(valid=ok.astype(np.uint8), proj_u=np.where(ok, u, m1), proj_v=np.where(ok, v, m1), proj_u_r=np.where(ok, ur, m1), proj_v_r=np.where(ok, vr, m1),
                open=g.open(), guard=dict(proj_u=gu, proj_v=gv, proj_u_r=gur, proj_v_r=gvr), x3Dc=xc, x3Dr=xr, gates=g)


def unproject(rp, points, valid, n, world):
    """mRwc * p + mOw where valid and below n; other rows of `world` kept"""
    B, cap = np.asarray(valid).shape
    live = (np.arange(cap)[None, :] < np.asarray(n)[:, None]) & (np.asarray(valid) != 0)
    w = _matvec(rp["Rwc"][:, None, :], _f(points)) + rp["left"]["Ow"][:, None, :]
    assert w.dtype == F32
    return np.where(live[..., None], w, _f(world))


def value_guard(ref, side):
    """the bar on proj_u / proj_v of a passing row of frustum(): the guard of its bounds comparisons"""
    it = {name: g for name, _, g, _ in ref[side]["gates"].items}
    return it["min_x"], it["min_y"]
