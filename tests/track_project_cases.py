"""Cases of the projection entries (include/orbslam3_hip_track_project.h) shared by the CPU and GPU tests: random local maps and
last frames from the package's generator, and hand-built rows that sit exactly ON every decision boundary of Frame::isInFrustum
and of the last-frame projection.  The boundary frames use the identity pose with tcw = -0 and a camera with power-of-two focal
lengths, so that every float of a boundary row is exact: Pc == P, dist == |Z| for points on the axis, uv == 256*X/Z + 320.

Test infrastructure only."""
import importlib

import numpy as np

import track_project_reference as R

try:                    # torch before anything of the package: a process must end up with one HIP runtime (conftest._torch_first)
    import torch  # noqa: F401
except Exception:
    pass

F32 = np.float32
ST = importlib.import_module("orb_slam3-1_amd.synth_track")

IDENTITY_POSE = np.array([0.0, 0.0, 0.0, 1.0, -0.0, -0.0, -0.0])


def boundary_camera():
    """log_scale_factor = log(1.1f): with it no hand-built level sits near an integer quotient"""
    return ST.camera(fx=256, fy=256, cx=320, cy=240, bf=32, size=(640, 480), scale_factor=1.1, n_levels=8)


def _unit(p):
    p = np.asarray(p, np.float64)
    n = np.linalg.norm(p)
    return (p / n if n > 0 else np.array([0.0, 0.0, 1.0])).astype(F32)


def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


D_MIN = F32(0.8) * F32(2.5)         # GetMinDistanceInvariance() of mfMinDistance = 2.5, in float
D_MAX = F32(1.2) * F32(2.5)

# name, P, normal (None = along P), mfMinDistance, mfMaxDistance, skip, bad, in view?, level (None = not in view)
FRUSTUM_ROWS = [
    ("behind", (0.1, 0.1, -2.0), None, 0.01, 1000, 0, 0, 0, None),
    ("left_of_min_x", (-1.26, 0, 1), None, 0.01, 1000, 0, 0, 0, None),
    ("right_of_max_x", (1.26, 0, 1), None, 0.01, 1000, 0, 0, 0, None),
    ("above_min_y", (0, -0.94, 1), None, 0.01, 1000, 0, 0, 0, None),
    ("below_max_y", (0, 0.94, 1), None, 0.01, 1000, 0, 0, 0, None),
    ("on_min_x", (-1.25, 0, 1), None, 0.01, 1000, 0, 0, 1, 7),          # uv(0) == mnMinX: `<` keeps it
    ("on_max_x", (1.25, 0, 1), None, 0.01, 1000, 0, 0, 1, 7),
    ("on_min_y", (0, -0.9375, 1), None, 0.01, 1000, 0, 0, 1, 7),
    ("on_max_y", (0, 0.9375, 1), None, 0.01, 1000, 0, 0, 1, 7),
    ("ulp_left_of_min_x", (_down(-1.25), 0, 1), None, 0.01, 1000, 0, 0, 0, None),
    ("step_right_of_max_x", (1.25 + 2.0 ** -22, 0, 1), None, 0.01, 1000, 0, 0, 0, None),   # uv(0) = 640 + one ulp of 640
    ("ulp_above_min_y", (0, _down(-0.9375), 1), None, 0.01, 1000, 0, 0, 0, None),
    ("step_below_max_y", (0, 0.9375 + 2.0 ** -23, 1), None, 0.01, 1000, 0, 0, 0, None),    # uv(1) = 480 + one ulp of 480
    ("nearer_than_min", (0, 0, 2), None, 3.0, 1000, 0, 0, 0, None),
    ("farther_than_max", (0, 0, 2), None, 0.01, 1.5, 0, 0, 0, None),
    ("dist_on_min", (0, 0, D_MIN), None, 2.5, 1000, 0, 0, 1, 7),        # dist == 0.8f*min: kept
    ("dist_ulp_under_min", (0, 0, _down(D_MIN)), None, 2.5, 1000, 0, 0, 0, None),
    ("dist_on_max", (0, 0, D_MAX), None, 0.01, 2.5, 0, 0, 1, 0),        # dist == 1.2f*max: kept; quotient -1.91 -> level 0
    ("dist_ulp_over_max", (0, 0, _up(D_MAX)), None, 0.01, 2.5, 0, 0, 0, None),
    ("cos_on_limit", (0, 0, 2), (0, 0, 0.5), 0.01, 1000, 0, 0, 1, 7),   # viewCos == 0.5 exactly: kept
    ("cos_ulp_under_limit", (0, 0, 2), (0, 0, _down(0.5)), 0.01, 1000, 0, 0, 0, None),
    ("beyond_angle", (0, 0, 2), (1, 0, 0), 0.01, 1000, 0, 0, 0, None),
    ("level_below_0", (0, 0, 1.15), None, 0.01, 1.0, 0, 0, 1, 0),       # quotient -1.47: ceil -1, clamped to 0
    ("level_above_top", (0, 0, 1), None, 0.01, 100.0, 0, 0, 1, 7),      # quotient 48.3: clamped to n_levels - 1
    ("level_inside", (0, 0, 2), None, 0.01, 3.0, 0, 0, 1, 5),           # quotient 4.25
    ("z_plus0_x0", (0.0, 0.0, 0.0), (0, 0, 1), 0.0, 1.0, 0, 0, 1, 0),   # uv = NaN fails no test; dist 0, viewCos NaN, ratio inf
    ("z_plus0_x1", (1.0, 0.0, 0.0), None, 0.0, 10.0, 0, 0, 0, None),    # uv(0) = +inf
    ("z_minus0_x0", (-0.0, -0.0, -0.0), (0, 0, 1), 0.0, 1.0, 0, 0, 1, 0),   # PcZ = -0.0f is not < 0.0f
    ("z_minus0_x1", (-1.0, -0.0, -0.0), None, 0.0, 10.0, 0, 0, 0, None),    # PcZ = -0: uv(0) = -1/-0 = +inf
    ("skipped", (0.1, 0.1, 2), None, 0.01, 1000, 1, 0, 0, None),
    ("bad", (0.1, 0.1, 2), None, 0.01, 1000, 0, 1, 0, None),
]
MINUS_ZERO_ROWS = ("z_minus0_x0", "z_minus0_x1")


def frustum_boundary_case():
    """three frames, pcap = 300, live rows 0 / 1 / 257 (an empty frame, a single lane, a tail that is no multiple of 64); frame 2
    holds FRUSTUM_ROWS first and random rows behind them; the rows past n are live-looking garbage that must come out dead"""
    cam = boundary_camera()
    B, pcap = 3, 300
    c = ST.make_local_map_case(11, B, pcap, cam=cam, poses=np.tile(IDENTITY_POSE, (B, 1)))
    c["skip"][:2] = 0; c["bad"][:2] = 0
    c["n"] = np.array([0, 1, 257], np.int32)
    c["xyz"][1, 0] = (0.3, 0.2, 3.0); c["normal"][1, 0] = _unit((0.3, 0.2, 3.0)); c["min_distance"][1, 0] = 0.5; c["max_distance"][1, 0] = 9.0
    for i, (_, P, Pn, mn, mx, skip, bad, _, _) in enumerate(FRUSTUM_ROWS):
        c["xyz"][2, i] = np.asarray(P, F32)
        c["normal"][2, i] = _unit(P) if Pn is None else np.asarray(Pn, F32)
        c["min_distance"][2, i] = mn; c["max_distance"][2, i] = mx
        c["skip"][2, i] = skip; c["bad"][2, i] = bad
    c["boundary_frame"] = 2
    return c


def check_frustum_boundary_rows(out, case):
    """the hand-built rows of `out` (any implementation's outputs) hold exactly what they were built for"""
    b = case["boundary_frame"]
    for i, (name, _, _, _, _, _, _, in_view, level) in enumerate(FRUSTUM_ROWS):
        assert out["valid"][b, i] == in_view, name
        assert out["octave"][b, i] == (level if in_view else -1), name


LAST_ROWS = [
    # name, x3Dw, has_point, valid
    ("behind", (0.1, 0.1, -2.0), 1, 0),
    ("left_of_min_x", (-1.26, 0, 1), 1, 0), ("right_of_max_x", (1.26, 0, 1), 1, 0), ("above_min_y", (0, -0.94, 1), 1, 0), ("below_max_y", (0, 0.94, 1), 1, 0),
    ("on_min_x", (-1.25, 0, 1), 1, 1), ("on_max_x", (1.25, 0, 1), 1, 1), ("on_min_y", (0, -0.9375, 1), 1, 1), ("on_max_y", (0, 0.9375, 1), 1, 1),
    ("ulp_left_of_min_x", (_down(-1.25), 0, 1), 1, 0), ("step_right_of_max_x", (1.25 + 2.0 ** -22, 0, 1), 1, 0),
    ("ulp_above_min_y", (0, _down(-0.9375), 1), 1, 0), ("step_below_max_y", (0, 0.9375 + 2.0 ** -23, 1), 1, 0),
    ("z_plus0_x0", (0.0, 0.0, 0.0), 1, 1),              # invzc = +inf is not < 0; uv = NaN
    ("z_plus0_x1", (1.0, 0.0, 0.0), 1, 0),
    ("z_minus0_x0", (-0.0, -0.0, -0.0), 1, 1),          # _transformVector turns -0 into +0 (v + w*uv + ...): the same as z_plus0
    ("z_minus0_x1", (-1.0, -0.0, -0.0), 1, 0),
    ("tiny_negative_z", (0.0, 0.0, -1e-30), 1, 0),      # invzc = -1e30 < 0
    ("no_point", (0.1, 0.1, 2), 0, 0),
    ("in_view", (0.1, 0.1, 2), 1, 1),
]


def last_boundary_case():
    """two frames, cap = 300: frame 0 (identity, 257 live rows) holds LAST_ROWS and random rows, frame 1 is rotated by 0.5 rad, so
    that Rcw*x and the quaternion's _transformVector differ in the last bit on some of its points"""
    cam = boundary_camera()
    poses = np.stack([IDENTITY_POSE, ST.make_poses(5, 2, max_angle=0.5)[1]])
    ang = 0.5
    poses[1, :4] = np.array([0.2, -0.5, 0.3, 0.0]) / np.linalg.norm([0.2, -0.5, 0.3]) * np.sin(ang / 2); poses[1, 3] = np.cos(ang / 2)
    c = ST.make_last_frame_case(12, 2, 300, cam=cam, poses=poses, full=True)
    c["n"] = np.array([257, 300], np.int32)
    for i, (_, x, has, _) in enumerate(LAST_ROWS):
        c["xyz"][0, i] = np.asarray(x, F32); c["has_point"][0, i] = has
    c["boundary_frame"] = 0
    return c


def check_last_boundary_rows(out, case):
    b = case["boundary_frame"]
    for i, (name, _, _, valid) in enumerate(LAST_ROWS):
        assert out["valid"][b, i] == valid, name


def random_frustum_cases():
    return [ST.make_local_map_case(31, 4, 300), ST.make_local_map_case(32, 2, 1000, cam=ST.camera(n_levels=12, scale_factor=1.15))]


def random_last_cases():
    return [ST.make_last_frame_case(41, 4, 300), ST.make_last_frame_case(42, 2, 1000)]


def pose_cases():
    """eight poses: the identity, rotations up to 0.6 rad, three of them with a double quaternion of norm != 1"""
    p = ST.make_poses(51, 8)
    assert (np.abs(np.linalg.norm(p[:, :4], axis=1) - 1) > 0.01).sum() >= 2
    return p


def handover_case():
    """one frame, cap = 70 (64 live), pcap = 40: inliers, discarded outliers, a bad point, a point without observations, two
    features on one row, one feature whose point has no row, and a dead feature holding a stale assignment"""
    cap, pcap, last_cap = 70, 40, 70
    assign = np.full((1, cap), -1, np.int32); outlier = np.zeros((1, cap), np.uint8)
    last_local = np.full((1, last_cap), -1, np.int32)
    bad = np.zeros((1, pcap), np.uint8); has_obs = np.ones((1, pcap), np.uint8)
    rs = np.random.RandomState(3)
    feats = rs.permutation(64)[:19]                     # the features that hold a point, anywhere in the live range
    for k, f in enumerate(feats):
        assign[0, f] = 30 + k                           # last-frame feature 30 + k ...
        last_local[0, 30 + k] = 2 * k                   # ... whose map point is local row 2k
    outlier[0, feats[10:14]] = 1
    bad[0, 2 * 14] = 1
    has_obs[0, 2 * 15] = 0
    last_local[0, 30 + 17] = 2 * 16                     # features 16 and 17 hold the same map point
    last_local[0, 30 + 18] = -1                         # no row: n_dropped = 1
    assign[0, 66] = 30                                  # beyond n_cur
    return dict(assign=assign, outlier=outlier, n_cur=np.array([64], np.int32), last_local=last_local, bad=bad, has_obs=has_obs)


def pack(mode, case, normalise):
    """the input file of tests/track_project_geometry_check.cpp: mode 0 = frustum, 1 = last-frame projection"""
    cam = case["cam"]
    B, rows = (case["skip"] if mode == 0 else case["has_point"]).shape
    head = np.array([mode, B, rows, normalise, cam["n_levels"]], np.int32).tobytes()
    head += np.array([cam[k] for k in ("fx", "fy", "cx", "cy", "bf", "min_x", "min_y", "max_x", "max_y", "log_scale_factor")] +
                     [case.get("cos_limit", 0.0)], F32).tobytes()
    parts = [np.ascontiguousarray(case["pose7"], np.float64), np.ascontiguousarray(case["n"], np.int32), np.ascontiguousarray(case["xyz"], F32)]
    if mode == 0:
        parts += [np.ascontiguousarray(case[k], F32) for k in ("normal", "min_distance", "max_distance")]
        parts += [np.ascontiguousarray(case[k], np.uint8) for k in ("skip", "bad")]
    else:
        parts += [np.ascontiguousarray(case["has_point"], np.uint8)]
    return head + b"".join(p.tobytes() for p in parts)


def unpack(mode, case, blob):
    """the check program's output -> (pose records [B][19], dict of outputs)"""
    B, rows = (case["skip"] if mode == 0 else case["has_point"]).shape
    a = np.frombuffer(blob, np.uint8)
    off = [0]

    def take(dtype, shape):
        n = int(np.prod(shape)) * 4
        v = a[off[0]:off[0] + n].view(dtype).reshape(shape).copy()
        off[0] += n
        return v
    poses = take(F32, (B, 19))
    names = [("valid", np.int32), ("u", F32), ("v", F32), ("octave", np.int32), ("view_cos", F32), ("track_depth", F32), ("proj_ur", F32)] if mode == 0 else \
            [("valid", np.int32), ("u", F32), ("v", F32), ("proj_ur", F32)]
    out = {k: take(dt, (B, rows)) for k, dt in names}
    if mode == 0:
        out["n_to_match"] = take(np.int32, (B,))
    assert off[0] == len(a)
    return poses, out


def assert_frustum_equal(out, ref, n_levels, max_tie_share=None, what=""):
    """every output bit for bit (NaN equals NaN), levels by the tie rule of track_project_reference.level_mismatches"""
    for k in ("valid", "u", "v", "view_cos", "track_depth", "proj_ur", "n_to_match"):
        np.testing.assert_array_equal(np.asarray(out[k]).astype(ref[k].dtype), ref[k], err_msg="%s %s" % (what, k))
    wrong, ties = R.level_mismatches(np.asarray(out["octave"]), ref, n_levels)
    print("%s: %d rows, %d in view, %d level ties" % (what, ref["valid"].size, int(ref["valid"].sum()), ties))
    assert wrong == 0, what
    if max_tie_share is not None:
        assert ties <= max_tie_share * ref["valid"].size, what


def assert_last_equal(out, ref, what=""):
    for k in ("valid", "u", "v", "proj_ur"):
        np.testing.assert_array_equal(np.asarray(out[k]).astype(ref[k].dtype), ref[k], err_msg="%s %s" % (what, k))
