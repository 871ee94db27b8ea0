"""Cases of the rig projection entries (include/orbslam3_hip_track_project_rig.h) shared by the CPU and GPU tests: seeded random rig
scenes from the package's generator, and hand-built rows whose expected outputs are stated literally.

The hand-built frames use the identity pose with tcw = -0 and a rig whose two cameras sit at ONE centre (trl = tlr = -0), the left
looking along +z and the right along +x: Rrl = [[0,0,-1],[0,1,0],[1,0,0]], so Pc_right = (-Z, Y, X) exactly.  A point on an optical
axis projects to exactly (cx, cy) of that camera (atan2(0, z) = 0, r = 0), which pins the strict image-bounds comparisons without a
guard band.  Left: fx = fy = 256, c = (512, 256); right: fx = 200, fy = 210, c = (500, 260), other distortion: the cameras differ, so
a projection with the wrong camera is told apart.  Image 1024 x 512.

Test infrastructure only."""
import importlib

import numpy as np

import track_project_rig_reference as RR

try:                    # torch before anything of the package: a process must end up with one HIP runtime
    import torch  # noqa: F401
except Exception:
    pass

F32 = np.float32
ST = importlib.import_module("orb_slam3-1_amd.synth_track")

IDENTITY_POSE = np.array([0.0, 0.0, 0.0, 1.0, -0.0, -0.0, -0.0])
S = np.sqrt(0.5)
SENT = dict(proj_u=F32(-701), proj_v=F32(-702), view_cos=F32(-703), track_depth=F32(-704), proj_u_r=F32(-711), proj_v_r=F32(-712), view_cos_r=F32(-713),
            track_depth_r=F32(-714), pred_level=3, pred_level_r=4, in_view=1, in_view_r=1)
PCAP, CAP, N_SHAPE = 70, 67, np.array([70, 0, 1], np.int32)
NLEFT = 40              # of the last-frame entries: rows >= NLEFT are key points of the right camera (projected like any other)


def boundary_rig(swap_centres=False, **bounds):
    left = [256, 256, 512, 256, 0.004, 0.0007, -0.002, 0.0002]
    right = [200, 210, 500, 260, 0.003, 0.0008, -0.0024, 0.0003]
    if swap_centres:
        left[2:4], right[2:4] = right[2:4], left[2:4]
    cam = dict(left=np.asarray(left, F32), right=np.asarray(right, F32), Rrl=np.asarray([0, 0, -1, 0, 1, 0, 1, 0, 0], F32),
               trl=np.asarray([-0.0, -0.0, -0.0], F32), tlr=np.asarray([-0.0, -0.0, -0.0], F32), q_rl=np.asarray([0, -S, 0, S], F32),
               min_x=F32(0), min_y=F32(0), max_x=F32(1024), max_y=F32(512), log_scale_factor=np.log(F32(1.1)), n_levels=8)
    cam.update({k: F32(v) for k, v in bounds.items()})
    return cam


def _unit(p):
    p = np.asarray(p, np.float64)
    n = np.linalg.norm(p)
    return (p / n if n > 0 else np.array([0.0, 0.0, 1.0])).astype(F32)


def _up(x):
    return np.nextafter(F32(x), F32(np.inf))


def _down(x):
    return np.nextafter(F32(x), F32(-np.inf))


TINY_NEG = np.nextafter(F32(-0.0), F32(-1))         # the smallest negative float
D_MIN = F32(0.8) * F32(2.5)
D_MAX = F32(1.2) * F32(2.5)

# name, P, normal (None = along P), mfMinDistance, mfMaxDistance, skip, bad, (in_view, pred_level), (in_view_r, pred_level_r)
# pred_level None = the row is skipped by SearchLocalPoints and keeps the sentinel level
FRUSTUM_ROWS = [
    ("front_of_left_behind_right", (-1, 0.2, 2), None, 0.01, 1000, 0, 0, (1, 7), (0, -1)),
    ("front_of_right_behind_left", (2, 0.2, -1), None, 0.01, 1000, 0, 0, (0, -1), (1, 7)),
    ("front_of_both", (2, 0.1, 2), None, 0.01, 1000, 0, 0, (1, 7), (1, 7)),
    ("behind_both", (-1, 0, -1), None, 0.01, 1000, 0, 0, (0, -1), (0, -1)),
    ("left_z_minus0", (-2, -1, -0.0), None, 0.01, 1000, 0, 0, (1, 7), (0, -1)),             # PcZ = -0.0f is not < 0.0f; right: PcZ = -2
    ("left_z_smallest_negative", (-2, -1, TINY_NEG), None, 0.01, 1000, 0, 0, (0, -1), (0, -1)),
    ("right_z_minus0", (-0.0, -1, -1), None, 0.01, 1000, 0, 0, (0, -1), (1, 7)),            # right PcZ = X = -0; left: PcZ = -1
    ("right_z_smallest_negative", (TINY_NEG, -1, -1), None, 0.01, 1000, 0, 0, (0, -1), (0, -1)),
    ("left_on_axis", (0, 0, 2), None, 0.01, 1000, 0, 0, (1, 7), (1, 7)),                    # right sees it at PcZ = +0, 90 degrees off axis
    ("right_on_axis", (2, 0, 0), None, 0.01, 1000, 0, 0, (1, 7), (1, 7)),
    ("below_left_image", (0.1, 3, 1), None, 0.01, 1000, 0, 0, (0, -1), (0, -1)),            # v = 256 + 256 * 1.25: right PcZ = 0.1, v_r beyond 512 too
    ("nearer_than_min", (0, 0, 2), None, 3.0, 1000, 0, 0, (0, -1), (0, -1)),
    ("farther_than_max", (0, 0, 2), None, 0.01, 1.5, 0, 0, (0, -1), (0, -1)),
    ("dist_on_min", (0, 0, D_MIN), None, 2.5, 1000, 0, 0, (1, 7), (1, 7)),                  # dist == 0.8f*min: kept (one centre: both cameras)
    ("dist_ulp_under_min", (0, 0, _down(D_MIN)), None, 2.5, 1000, 0, 0, (0, -1), (0, -1)),
    ("dist_on_max", (0, 0, D_MAX), None, 0.01, 2.5, 0, 0, (1, 0), (1, 0)),                  # dist == 1.2f*max: kept; PredictScale takes the RAW max: quotient -1.91
    ("dist_ulp_over_max", (0, 0, _up(D_MAX)), None, 0.01, 2.5, 0, 0, (0, -1), (0, -1)),
    ("cos_on_limit", (0, 0, 2), (0, 0, 0.5), 0.01, 1000, 0, 0, (1, 7), (1, 7)),             # viewCos == 0.5 exactly: kept
    ("cos_ulp_under_limit", (0, 0, 2), (0, 0, _down(0.5)), 0.01, 1000, 0, 0, (0, -1), (0, -1)),
    ("level_below_0", (0, 0, 1.15), None, 0.01, 1.0, 0, 0, (1, 0), (1, 0)),                 # quotient -1.47: ceil -1, clamped to 0
    ("level_above_top", (0, 0, 1), None, 0.01, 100.0, 0, 0, (1, 7), (1, 7)),                # quotient 48.3: clamped to n_levels - 1
    ("level_inside", (0, 0, 2), None, 0.01, 3.0, 0, 0, (1, 5), (1, 5)),                     # quotient 4.25
    ("level_nan", (0.0, 0.0, 0.0), (0, 0, 1), 0.0, 0.0, 0, 0, (1, 0), (1, 0)),              # dist 0, max 0: ratio 0/0, the NaN quotient gives 0
    ("skipped", (2, 0.1, 2), None, 0.01, 1000, 1, 0, (0, None), (0, None)),
    ("bad", (2, 0.1, 2), None, 0.01, 1000, 0, 1, (0, None), (0, None)),
]
N_TO_MATCH_ROWS = sum(1 for r in FRUSTUM_ROWS if r[7][0] or r[8][0])      # a point counts once, seen by both cameras or by one


def sentinel_state(B, pcap):
    dt = dict(ST.RIG_STATE)
    return {k: np.full((B, pcap), SENT[k], dt[k]) for k in dt}


def frustum_hand_case(cam=None):
    """three frames, pcap = 70 (no multiple of the wave), n = [70, 0, 1]: frame 0 holds FRUSTUM_ROWS and random rows behind them,
    frame 1 is empty, frame 2 has one live row; rows past n are live-looking garbage.  The state is the sentinel everywhere."""
    cam = cam or boundary_rig()
    B = 3
    c = ST.make_rig_local_map_case(11, B, PCAP, cam=cam, poses=np.tile(IDENTITY_POSE, (B, 1)))
    c["skip"][:] = 0; c["bad"][:] = 0
    c["n"] = N_SHAPE.copy()
    for i, (_, P, Pn, mn, mx, skip, bad, _, _) in enumerate(FRUSTUM_ROWS):
        c["xyz"][0, i] = np.asarray(P, F32)
        c["normal"][0, i] = _unit(P) if Pn is None else np.asarray(Pn, F32)
        c["min_distance"][0, i] = mn; c["max_distance"][0, i] = mx
        c["skip"][0, i] = skip; c["bad"][0, i] = bad
    c["xyz"][2, 0] = (2, 0.1, 2); c["normal"][2, 0] = _unit((2, 0.1, 2)); c["min_distance"][2, 0] = 0.01; c["max_distance"][2, 0] = 1000
    c["state"] = sentinel_state(B, PCAP)
    return c


def check_frustum_hand_rows(out, case):
    """the hand-built rows of `out` (any implementation's arrays after the call) hold exactly what they were built for"""
    for i, (name, _, _, _, _, _, _, left, right) in enumerate(FRUSTUM_ROWS):
        for (seen, level), sfx in ((left, ""), (right, "_r")):
            assert out["in_view" + sfx][0, i] == seen, name + sfx
            assert out["pred_level" + sfx][0, i] == (SENT["pred_level" + sfx] if level is None else level), name + sfx
            for k in RR.STALE:
                kept = out[k + sfx][0, i] == SENT[k + sfx]
                assert kept == (not seen), "%s: %s%s %s" % (name, k, sfx, "overwritten" if seen == 0 else "not written")
    names = [r[0] for r in FRUSTUM_ROWS]
    lc, rc = case["cam"]["left"], case["cam"]["right"]
    i = names.index("left_on_axis")
    assert out["proj_u"][0, i] == lc[2] and out["proj_v"][0, i] == lc[3] and out["track_depth"][0, i] == 2 and out["view_cos"][0, i] == 1
    i = names.index("right_on_axis")
    assert out["proj_u_r"][0, i] == rc[2] and out["proj_v_r"][0, i] == rc[3] and out["track_depth_r"][0, i] == 2
    i = names.index("front_of_right_behind_left")       # only the right camera sees it: the LEFT mTrackDepth stays what an earlier frame wrote
    assert out["track_depth"][0, i] == SENT["track_depth"] and out["track_depth_r"][0, i] > 2
    # dead rows: verdicts cleared, everything else as it was
    for b, n in enumerate(N_SHAPE):
        for k in SENT:
            want = 0 if k.startswith("in_view") else SENT[k]
            assert (out[k][b, n:] == want).all(), (b, k)
    assert out["n_to_match"][0] >= N_TO_MATCH_ROWS and out["n_to_match"][1] == 0 and out["n_to_match"][2] == 1


def bounds_cases():
    """[(name, case, in_view of the left-axis row, in_view_r of the right-axis row)]: batch 1, pcap = 70, two live rows -- (0, 0, 2)
    on the left axis projects to exactly the left (cx, cy), (2, 0, 0) on the right axis to exactly the right (cx, cy).  With the
    centres (512, 256) / (500, 260) the window min = (500, 256), max = (512, 260) puts the left point ON max_x and min_y and the right
    point ON min_x and max_y; with the centres swapped, on the other four.  One ulp tighter on one bound, that camera loses its point."""
    res = []
    for swap in (False, True):
        window = dict(min_x=500, min_y=256, max_x=512, max_y=260)
        # (bound, the side whose point sits on it)
        on = dict(max_x="left", min_y="left", min_x="right", max_y="right") if not swap else dict(min_x="left", max_y="left", max_x="right", min_y="right")
        variants = [("on_all_four", window, 1, 1)]
        for bound, side in on.items():
            w = dict(window)
            w[bound] = _up(w[bound]) if bound.startswith("min") else _down(w[bound])
            variants.append(("%s_one_ulp_inside_%s" % (side, bound), w, int(side != "left"), int(side != "right")))
        for name, w, seen_l, seen_r in variants:
            c = ST.make_rig_local_map_case(12, 1, PCAP, cam=boundary_rig(swap_centres=swap, **w), poses=IDENTITY_POSE[None, :].copy())
            c["skip"][:] = 0; c["bad"][:] = 0; c["n"] = np.array([2], np.int32)
            for i, P in enumerate(((0, 0, 2), (2, 0, 0))):
                c["xyz"][0, i] = P; c["normal"][0, i] = _unit(P); c["min_distance"][0, i] = 0.01; c["max_distance"][0, i] = 1000
            c["state"] = sentinel_state(1, PCAP)
            res.append((("swapped_" if swap else "") + name, c, seen_l, seen_r))
    return res


def check_bounds_case(out, seen_l, seen_r, name):
    # row 0 is seen by the left camera alone (the right one has it 90 degrees off its axis, outside the narrow window), row 1 by the right
    assert out["in_view"][0, 0] == seen_l and out["in_view_r"][0, 1] == seen_r, name
    assert out["in_view_r"][0, 0] == 0 and out["in_view"][0, 1] == 0, name
    assert out["n_to_match"][0] == seen_l + seen_r, name


# name, x3Dw, has_point, valid
LAST_ROWS = [
    ("behind", (0.1, 0.1, -2.0), 1, 0),
    ("tiny_negative_z", (0.0, 0.0, -1e-30), 1, 0),      # invzc = -1e30 < 0
    ("z_plus0", (0.0, 0.0, 0.0), 1, 1),                 # invzc = +inf is not < 0; on the axis: (cx, cy)
    ("on_axis", (0, 0, 2), 1, 1),
    ("left_out_of_bounds_cancels_right", (0.1, 3, 1), 1, 0),
    ("right_far_outside_stays_valid", (-2, 1.5, 1), 1, 1),   # x3Dr = (-1, 1.5, -2): v_r = 256 + 256 * 2.4 * 0.83, no bounds test on it
    ("no_point", (0.1, 0.1, 2), 0, 0),
    ("in_view", (0.1, 0.1, 2), 1, 1),
]


def last_hand_case():
    """three frames, cap = 67, n = [67, 0, 1]: frame 0 holds LAST_ROWS among its left entries and again from NLEFT on (entries of
    right key points), random rows elsewhere"""
    B = 3
    c = ST.make_rig_last_frame_case(13, B, CAP, cam=boundary_rig(), poses=np.tile(IDENTITY_POSE, (B, 1)), full=True)
    c["n"] = np.array([67, 0, 1], np.int32)
    for base in (0, NLEFT):
        for i, (_, x, has, _) in enumerate(LAST_ROWS):
            c["xyz"][0, base + i] = np.asarray(x, F32); c["has_point"][0, base + i] = has
    c["xyz"][2, 0] = (0.1, 0.1, 2); c["has_point"][2, 0] = 1
    return c


def check_last_hand_rows(out, case):
    names = [r[0] for r in LAST_ROWS]
    lc = case["cam"]["left"]
    for base in (0, NLEFT):
        for i, (name, _, _, valid) in enumerate(LAST_ROWS):
            assert out["valid"][0, base + i] == valid, name
            if not valid:
                assert all(out[k][0, base + i] == -1 for k in ("proj_u", "proj_v", "proj_u_r", "proj_v_r")), name
        for nm in ("z_plus0", "on_axis"):
            i = base + names.index(nm)
            assert out["proj_u"][0, i] == lc[2] and out["proj_v"][0, i] == lc[3], nm
        assert out["proj_v_r"][0, base + names.index("right_far_outside_stays_valid")] > float(case["cam"]["max_y"]) + 100
    for b, n in enumerate(case["n"]):
        assert (out["valid"][b, n:] == 0).all() and all((out[k][b, n:] == -1).all() for k in ("proj_u", "proj_v", "proj_u_r", "proj_v_r"))
    assert out["valid"][2, 0] == 1


def random_frustum_cases():
    """at most 3 frames x 200 points; the second has every row live"""
    return [ST.make_rig_local_map_case(31, 3, 200), ST.make_rig_local_map_case(32, 2, 200, cam=ST.rig_camera(yaw=0.8, n_levels=12, scale_factor=1.15), full=True)]


def random_last_cases():
    return [ST.make_rig_last_frame_case(41, 3, 200), ST.make_rig_last_frame_case(42, 2, 200, cam=ST.rig_camera(yaw=0.8), full=True)]


def pose_cases():
    p = ST.make_poses(51, 8)
    assert (np.abs(np.linalg.norm(p[:, :4], axis=1) - 1) > 0.01).sum() >= 2
    return p


def unproject_case(seed=61, B=3, cap=CAP):
    rs = np.random.RandomState(seed)
    return dict(cam=ST.rig_camera(), pose7=ST.make_poses(seed, B), points=rs.uniform(-5, 5, (B, cap, 3)).astype(F32),
                valid=(rs.uniform(size=(B, cap)) < 0.7).astype(np.uint8), n=np.array([cap, 0, 1], np.int32), world=np.full((B, cap, 3), -555, F32))


def pack(mode, case, normalise):
    """the input file of tests/track_project_rig_geometry_check.cpp: mode 0 = frustum, 1 = last-frame projection, 2 = unproject"""
    cam = case["cam"]
    B, rows = (case["skip"] if mode == 0 else case["has_point"] if mode == 1 else case["valid"]).shape
    head = np.array([mode, B, rows, normalise, cam["n_levels"]], np.int32).tobytes()
    head += np.concatenate([np.asarray(cam[k], F32).reshape(-1) for k in ("left", "right", "Rrl", "trl", "tlr", "q_rl")] +
                           [np.asarray([cam[k] for k in ("min_x", "min_y", "max_x", "max_y", "log_scale_factor")] + [case.get("cos_limit", 0.0)], F32)]).tobytes()
    parts = [np.ascontiguousarray(case["pose7"], np.float64), np.ascontiguousarray(case["n"], np.int32)]
    if mode == 0:
        parts += [np.ascontiguousarray(case[k], F32) for k in ("xyz", "normal", "min_distance", "max_distance")]
        parts += [np.ascontiguousarray(case[k], np.uint8) for k in ("skip", "bad")]
        parts += [np.ascontiguousarray(case["state"][k], np.int32 if dt != F32 else F32) for k, dt in ST.RIG_STATE]
    elif mode == 1:
        parts += [np.ascontiguousarray(case["xyz"], F32), np.ascontiguousarray(case["has_point"], np.uint8)]
    else:
        parts += [np.ascontiguousarray(case["points"], F32), np.ascontiguousarray(case["valid"], np.uint8), np.ascontiguousarray(case["world"], F32)]
    return head + b"".join(p.tobytes() for p in parts)


def unpack(mode, case, blob):
    """the check program's output -> (rig pose records [B][43], dict of outputs)"""
    B, rows = (case["skip"] if mode == 0 else case["has_point"] if mode == 1 else case["valid"]).shape
    a = np.frombuffer(blob, np.uint8)
    off = [0]

    def take(dtype, shape):
        n = int(np.prod(shape)) * 4
        v = a[off[0]:off[0] + n].view(dtype).reshape(shape).copy()
        off[0] += n
        return v
    poses = take(F32, (B, 43))
    if mode == 0:
        out = {k: take(np.int32 if dt != F32 else F32, (B, rows)) for k, dt in ST.RIG_STATE}
        out["n_to_match"] = take(np.int32, (B,))
    elif mode == 1:
        out = {k: take(np.int32 if k == "valid" else F32, (B, rows)) for k in ("valid", "proj_u", "proj_v", "proj_u_r", "proj_v_r")}
    else:
        out = dict(world=take(F32, (B, rows, 3)))
    assert off[0] == len(a)
    return poses, out


def compare_frustum(out, ref, n_levels, what=""):
    """`out` (an implementation's arrays after the call) against RR.frustum: decisions, levels (tie rule) and the preserved stale
    state on every row that is not open; values of passing rows within the KannalaBrandt8 bar (proj_u / proj_v) or exactly
    (view_cos, track_depth: no transcendental).  Returns (worst |du| / guard over the passing rows, rows that differ at all from the
    reference in proj_u / proj_v)."""
    closed = ~ref["open"]
    worst, differ = 0.0, 0
    for side, sfx in (("left", ""), ("right", "_r")):
        s = ref[side]
        np.testing.assert_array_equal(np.asarray(out["in_view" + sfx])[closed], ref["in_view" + sfx][closed], err_msg="%s in_view%s" % (what, sfx))
        agree = closed & (np.asarray(out["in_view" + sfx]) == ref["in_view" + sfx])
        lv = np.where(closed, out["pred_level" + sfx], ref["pred_level" + sfx])
        # rows not in view hold -1 or (skipped rows) the incoming level on both sides: exact; rows in view follow the tie rule
        seen = ref["in_view" + sfx] != 0
        np.testing.assert_array_equal(lv[~seen], ref["pred_level" + sfx][~seen], err_msg="%s pred_level%s of rows not in view" % (what, sfx))
        wrong, ties = RR.level_mismatches(np.where(seen, lv, -1), ref, side, n_levels)
        assert wrong == 0, "%s: %d levels%s wrong (%d ties)" % (what, wrong, sfx, ties)
        gu, gv = RR.value_guard(ref, side)
        passing = agree & seen
        for k, g in (("proj_u", gu), ("proj_v", gv)):
            d = np.abs(np.asarray(out[k + sfx], np.float64) - ref[k + sfx])
            keep = agree & ~seen
            np.testing.assert_array_equal(np.asarray(out[k + sfx])[keep], ref[k + sfx][keep], err_msg="%s stale %s%s" % (what, k, sfx))
            assert (d[passing] <= g[passing]).all(), "%s %s%s: %g above the bar" % (what, k, sfx, (d[passing] - g[passing]).max())
            with np.errstate(all="ignore"):
                ratio = np.where(passing & (g > 0), d / np.where(g > 0, g, 1), 0.0)
            worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
            differ += int((d[passing] != 0).sum())
        for k in ("view_cos", "track_depth"):
            np.testing.assert_array_equal(np.asarray(out[k + sfx])[agree].view(np.uint32), ref[k + sfx][agree].view(np.uint32), err_msg="%s %s%s" % (what, k, sfx))
    lo = (ref["left"]["valid"] | ref["right"]["valid"]) & closed
    n = np.asarray(out["n_to_match"])
    assert ((n >= lo.sum(1)) & (n <= lo.sum(1) + ref["open"].sum(1))).all(), "%s n_to_match %s" % (what, n)
    return worst, differ


def compare_last(out, ref, what=""):
    closed = ~ref["open"]
    np.testing.assert_array_equal(np.asarray(out["valid"])[closed], ref["valid"][closed], err_msg=what + " valid")
    agree = closed & (np.asarray(out["valid"]) == ref["valid"])
    ok = agree & (ref["valid"] != 0)
    worst, differ = 0.0, 0
    for k in ("proj_u", "proj_v", "proj_u_r", "proj_v_r"):
        np.testing.assert_array_equal(np.asarray(out[k])[agree & ~ok], ref[k][agree & ~ok], err_msg="%s %s of invalid rows" % (what, k))
        d = np.abs(np.asarray(out[k], np.float64) - ref[k]); g = ref["guard"][k]
        assert (d[ok] <= g[ok]).all(), "%s %s: %g above the bar" % (what, k, (d[ok] - g[ok]).max())
        with np.errstate(all="ignore"):
            ratio = np.where(ok & (g > 0), d / np.where(g > 0, g, 1), 0.0)
        worst = max(worst, float(ratio.max()) if ratio.size else 0.0)
        differ += int((d[ok] != 0).sum())
    return worst, differ
