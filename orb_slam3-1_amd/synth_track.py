"""Synthetic inputs of the projection entries of include/orbslam3_hip_track_project.h: frame poses, local maps around them
(Tracking::SearchLocalPoints) and last-frame map-point tables (SearchByProjection(CurrentFrame, LastFrame)); and the same for the
two-camera KannalaBrandt8 rig frames of include/orbslam3_hip_track_project_rig.h.  numpy only."""
import numpy as np

F32 = np.float32


def camera(fx=458.654, fy=457.296, cx=367.215, cy=248.375, bf=47.9, size=(752, 480), scale_factor=1.2, n_levels=8):
    """OrbmTrackCamera as a dict of float32 values; log_scale_factor = log(mfScaleFactor) as Frame computes it (a float log)"""
    return dict(fx=F32(fx), fy=F32(fy), cx=F32(cx), cy=F32(cy), bf=F32(bf), min_x=F32(0), min_y=F32(0), max_x=F32(size[0]), max_y=F32(size[1]),
                log_scale_factor=np.log(F32(scale_factor)), n_levels=int(n_levels))


def make_poses(seed, batch, max_angle=0.6, max_t=1.5, unnormalised_every=3):
    """[batch][7] double Tcw (qx qy qz qw tx ty tz) as pose_optimize_batch_device writes them; every `unnormalised_every`-th has a
    quaternion of norm != 1.  The first is the identity."""
    rs = np.random.RandomState(seed)
    p = np.zeros((batch, 7))
    for b in range(batch):
        axis = rs.normal(size=3); axis /= np.linalg.norm(axis)
        ang = rs.uniform(-max_angle, max_angle) if b else 0.0
        p[b, :3] = axis * np.sin(ang / 2); p[b, 3] = np.cos(ang / 2)
        p[b, 4:] = rs.uniform(-max_t, max_t, 3) if b else 0.0
        if unnormalised_every and b % unnormalised_every == unnormalised_every - 1:
            p[b, :4] *= rs.uniform(0.7, 1.4)
    return p


def _rotation(q):
    x, y, z, w = q / np.linalg.norm(q)
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def _world_points(rs, pose, cam, n, behind_frac):
    """n world points seen by `pose` over 1.3 x the image, depths 0.4 .. 25, a share of them behind the camera"""
    w, h = float(cam["max_x"]), float(cam["max_y"])
    u = rs.uniform(-0.15 * w, 1.15 * w, n); v = rs.uniform(-0.15 * h, 1.15 * h, n)
    z = np.exp(rs.uniform(np.log(0.4), np.log(25.0), n))
    z[rs.uniform(size=n) < behind_frac] *= -1
    pc = np.stack([(u - float(cam["cx"])) / float(cam["fx"]) * z, (v - float(cam["cy"])) / float(cam["fy"]) * z, z], 1)
    R = _rotation(pose[:4])
    return (pc - pose[4:]) @ R, -R.T @ pose[4:]         # R^T (pc - t), camera centre


def make_local_map_case(seed, batch, pcap, cam=None, poses=None, full=False):
    """one call of orbm_frustum_batch(_device): dict(cam, pose7, xyz, normal, min_distance, max_distance, skip, bad, n, cos_limit).
    Every gate of Frame::isInFrustum rejects a share of the rows."""
    rs = np.random.RandomState(seed)
    cam = cam or camera()
    poses = make_poses(seed + 1000, batch) if poses is None else poses
    xyz = np.zeros((batch, pcap, 3), F32); normal = np.zeros((batch, pcap, 3), F32)
    mind = np.zeros((batch, pcap), F32); maxd = np.zeros((batch, pcap), F32)
    for b in range(batch):
        pw, ow = _world_points(rs, poses[b], cam, pcap, 0.08)
        d = np.linalg.norm(pw - ow, axis=1)
        nrm = (pw - ow) / d[:, None] + rs.normal(0, 0.5, (pcap, 3))          # mean viewing direction: up to ~60 degrees off
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        mx = d * np.exp(rs.uniform(np.log(0.7), np.log(6.0), pcap))
        mn = mx / 1.2 ** 7 * rs.uniform(0.5, 1.6, pcap)
        xyz[b], normal[b], mind[b], maxd[b] = pw, nrm, mn, mx
    n = np.full(batch, pcap, np.int32) if full else rs.randint(0, pcap + 1, batch).astype(np.int32)
    return dict(cam=cam, pose7=poses, xyz=xyz, normal=normal, min_distance=mind, max_distance=maxd,
                skip=(rs.uniform(size=(batch, pcap)) < 0.06).astype(np.uint8), bad=(rs.uniform(size=(batch, pcap)) < 0.04).astype(np.uint8),
                n=n, cos_limit=F32(0.5))


def make_last_frame_case(seed, batch, cap, cam=None, poses=None, full=False):
    """one call of orbm_project_last_batch(_device): dict(cam, pose7, xyz [batch][cap][3], has_point, n)"""
    rs = np.random.RandomState(seed)
    cam = cam or camera()
    poses = make_poses(seed + 2000, batch) if poses is None else poses
    xyz = np.zeros((batch, cap, 3), F32)
    for b in range(batch):
        xyz[b] = _world_points(rs, poses[b], cam, cap, 0.05)[0]
    n = np.full(batch, cap, np.int32) if full else rs.randint(0, cap + 1, batch).astype(np.int32)
    return dict(cam=cam, pose7=poses, xyz=xyz, has_point=(rs.uniform(size=(batch, cap)) < 0.8).astype(np.uint8), n=n)


# ---- two-camera KannalaBrandt8 rig frames (include/orbslam3_hip_track_project_rig.h) ----
RIG_STATE = (("in_view", np.uint8), ("proj_u", F32), ("proj_v", F32), ("pred_level", np.int32), ("view_cos", F32), ("in_view_r", np.uint8),
             ("proj_u_r", F32), ("proj_v_r", F32), ("pred_level_r", np.int32), ("view_cos_r", F32), ("track_depth", F32), ("track_depth_r", F32))


def rig_camera(yaw=0.45, baseline=0.11, size=(512, 512), scale_factor=1.2, n_levels=8,
               left=(190.98, 190.97, 254.93, 256.90, 0.0034, 0.00072, -0.0020, 0.00020),
               right=(188.20, 189.10, 252.70, 255.50, 0.0030, 0.00080, -0.0024, 0.00031)):
    """OrbmTrackRigCamera as a dict: two DIFFERENT KannalaBrandt8 parameter sets (fx fy cx cy k0..k3), the right camera `baseline`
    to the right of the left one and turned outwards by `yaw` about y, so that the two fields of view (about +-75 degrees each)
    overlap in the middle and each camera sees a part the other does not.  Rrl / trl / q_rl describe mTrl, tlr = mTlr.translation()."""
    h = 0.5 * yaw
    q_lr = np.array([0.0, np.sin(h), 0.0, np.cos(h)])                 # Tlr: right-camera coordinates -> left-camera coordinates
    Rlr = _rotation(q_lr)
    tlr = np.array([baseline, 0.002, -0.004])
    q_rl = (q_lr * [-1, -1, -1, 1]).astype(F32)
    Rrl = _rotation(q_rl.astype(np.float64))
    return dict(left=np.asarray(left, F32), right=np.asarray(right, F32), Rrl=Rrl.astype(F32).reshape(9), trl=(-Rrl @ tlr).astype(F32), tlr=tlr.astype(F32),
                q_rl=q_rl, min_x=F32(0), min_y=F32(0), max_x=F32(size[0]), max_y=F32(size[1]), log_scale_factor=np.log(F32(scale_factor)), n_levels=int(n_levels))


def _rig_world_points(rs, pose, cam, n, all_round_frac=0.35):
    """n world points around the rig of `pose`: most within 110 degrees of the left optical axis (in front of one camera, of both,
    or beside both images), the rest anywhere on the sphere (behind both cameras too); depths 0.4 .. 25"""
    d = rs.normal(size=(n, 3)); d /= np.linalg.norm(d, axis=1)[:, None]
    cone = rs.uniform(size=n) >= all_round_frac
    ang = rs.uniform(0, np.radians(110), n); phi = rs.uniform(0, 2 * np.pi, n)
    d[cone] = np.stack([np.sin(ang) * np.cos(phi), np.sin(ang) * np.sin(phi), np.cos(ang)], 1)[cone]
    pc = d * np.exp(rs.uniform(np.log(0.4), np.log(25.0), n))[:, None]
    R = _rotation(pose[:4])
    return (pc - pose[4:]) @ R, -R.T @ pose[4:]


def make_rig_state(seed, batch, pcap):
    """the MapPoint members an EARLIER frame left behind, as the twelve [batch][pcap] arrays of OrbmRigFrustumOut"""
    rs = np.random.RandomState(seed)
    st = {}
    for k, dt in RIG_STATE:
        if dt == np.uint8:
            st[k] = rs.randint(0, 2, (batch, pcap)).astype(dt)
        elif dt == np.int32:
            st[k] = rs.randint(-1, 8, (batch, pcap)).astype(dt)
        else:
            st[k] = rs.uniform(-900, -100, (batch, pcap)).astype(dt)        # (negative: no projection, cosine or depth of this frame)
    return st


def make_rig_local_map_case(seed, batch, pcap, cam=None, poses=None, full=False):
    """one call of orbm_frustum_rig_batch(_device): the dict of make_local_map_case with a rig camera, plus `state`"""
    rs = np.random.RandomState(seed)
    cam = cam or rig_camera()
    poses = make_poses(seed + 1000, batch) if poses is None else poses
    xyz = np.zeros((batch, pcap, 3), F32); normal = np.zeros((batch, pcap, 3), F32)
    mind = np.zeros((batch, pcap), F32); maxd = np.zeros((batch, pcap), F32)
    for b in range(batch):
        pw, ow = _rig_world_points(rs, poses[b], cam, pcap)
        d = np.linalg.norm(pw - ow, axis=1)
        nrm = (pw - ow) / d[:, None] + rs.normal(0, 0.5, (pcap, 3))
        nrm /= np.linalg.norm(nrm, axis=1)[:, None]
        mx = d * np.exp(rs.uniform(np.log(0.7), np.log(6.0), pcap))
        mn = mx / 1.2 ** 7 * rs.uniform(0.5, 1.6, pcap)
        xyz[b], normal[b], mind[b], maxd[b] = pw, nrm, mn, mx
    n = np.full(batch, pcap, np.int32) if full else rs.randint(0, pcap + 1, batch).astype(np.int32)
    return dict(cam=cam, pose7=poses, xyz=xyz, normal=normal, min_distance=mind, max_distance=maxd,
                skip=(rs.uniform(size=(batch, pcap)) < 0.06).astype(np.uint8), bad=(rs.uniform(size=(batch, pcap)) < 0.04).astype(np.uint8),
                n=n, cos_limit=F32(0.5), state=make_rig_state(seed + 3000, batch, pcap))


def make_rig_last_frame_case(seed, batch, cap, cam=None, poses=None, full=False):
    """one call of orbm_project_last_rig_batch(_device): dict(cam, pose7, xyz [batch][cap][3], has_point, n); cap = Nleft + Nright"""
    rs = np.random.RandomState(seed)
    cam = cam or rig_camera()
    poses = make_poses(seed + 2000, batch) if poses is None else poses
    xyz = np.zeros((batch, cap, 3), F32)
    for b in range(batch):
        xyz[b] = _rig_world_points(rs, poses[b], cam, cap)[0]
    n = np.full(batch, cap, np.int32) if full else rs.randint(0, cap + 1, batch).astype(np.int32)
    return dict(cam=cam, pose7=poses, xyz=xyz, has_point=(rs.uniform(size=(batch, cap)) < 0.8).astype(np.uint8), n=n)
