"""Calls of the two rig-frame tracking searches (include/orbslam3_hip_rig_match.h) for tests/test_rig_match_reference.py (CPU)
and tests/test_rig_match_gpu.py: hand-built calls with their expected arrays stated literally, shape calls and seeded random
rigs.  A test helper, not a test; it imports nothing of the package.

Hand-built frames have a handful of features on the reference's 64 x 48 grid over a 640 x 480 image (cells of 10 x 10 px).
Descriptors are built bit by bit: flip(D, k) differs from D in exactly k bits, and two flips of one base by a and b bits in
DISJOINT ranges differ by a + b.  UNTOUCHED (-7) marks a slot no call may have written; the last-frame search writes -1 into
a slot the rotation check nulled.

A call is dict(kind "mp" | "last", rig, pts, th, nnratio, far_points, th_far, check_ori, assign, occupied[, expect]) with
expect = dict(n, assign, occupied)."""
import numpy as np

f32 = np.float32
W, H, COLS, ROWS, NLEVELS = 640.0, 480.0, 64, 48, 8
SCALE = (1.2 ** np.arange(NLEVELS)).astype(np.float32)
UNTOUCHED = -7
TH_HIGH = 100


def base_desc(tag):
    return np.random.default_rng(1000 + tag).integers(0, 256, 32).astype(np.uint8)


def flip(d, k, start=0):
    """d with bits [start, start + k) flipped"""
    bits = np.unpackbits(d)
    bits[start:start + k] ^= 1
    return np.packbits(bits)


class Side:
    def __init__(self, w=W, h=H):
        self.x, self.y, self.octave, self.angle, self.desc = [], [], [], [], []
        self.w, self.h = w, h

    def add(self, x, y, desc, octave=0, angle=0.0):
        self.x.append(x); self.y.append(y); self.octave.append(octave); self.angle.append(angle); self.desc.append(desc)
        return len(self.x) - 1

    def grid(self):
        n = len(self.x)
        return dict(x=np.array(self.x, np.float32), y=np.array(self.y, np.float32), octave=np.array(self.octave, np.int32),
                    angle=np.array(self.angle, np.float32), desc=np.array(self.desc, np.uint8).reshape(n, 32),
                    min_x=0.0, min_y=0.0, max_x=float(self.w), max_y=float(self.h), cols=COLS, rows=ROWS)


def make_rig(left, right, l2r=None, r2l=None, scale=SCALE):
    nl, nr = len(left.x), len(right.x)
    a = np.full(nl, -1, np.int32); b = np.full(nr, -1, np.int32)
    for k, v in (l2r or {}).items():
        a[k] = v
    for k, v in (r2l or {}).items():
        b[k] = v
    return dict(left=left.grid(), right=right.grid(), scale=scale.copy(), left_to_right=a, right_to_left=b)


MP_DEFAULT = dict(in_view=1, proj_u=0.0, proj_v=0.0, pred_level=0, view_cos=1.0, in_view_r=0, proj_u_r=0.0, proj_v_r=0.0, pred_level_r=0, view_cos_r=1.0,
                  track_depth=1.0, bad=0, has_obs=1)
MP_TYPES = dict(in_view=np.uint8, proj_u=f32, proj_v=f32, pred_level=np.int32, view_cos=f32, in_view_r=np.uint8, proj_u_r=f32, proj_v_r=f32,
                pred_level_r=np.int32, view_cos_r=f32, track_depth=f32, bad=np.uint8, has_obs=np.uint8)
LAST_DEFAULT = dict(valid=1, proj_u=0.0, proj_v=0.0, proj_u_r=0.0, proj_v_r=0.0, octave=0, angle=0.0, has_obs=1)
LAST_TYPES = dict(valid=np.uint8, proj_u=f32, proj_v=f32, proj_u_r=f32, proj_v_r=f32, octave=np.int32, angle=f32, has_obs=np.uint8)


def _points(rows, default, types):
    out = {k: np.array([dict(default, **r)[k] for r in rows], t) for k, t in types.items()}
    out["desc"] = np.array([r["desc"] for r in rows], np.uint8).reshape(len(rows), 32)
    out["n"] = len(rows)
    return out


def mp_points(rows):
    return _points(rows, MP_DEFAULT, MP_TYPES)


def last_points(rows, level_window=0):
    p = _points(rows, LAST_DEFAULT, LAST_TYPES)
    p["level_window"] = level_window
    return p


def _call(kind, rig, pts, expect=None, th=None, nnratio=0.8, far_points=False, th_far=0.0, check_ori=True, occupied=None, assign=None):
    slots = len(rig["left"]["x"]) + len(rig["right"]["x"])
    occ = np.zeros(slots, np.uint8)
    for s in occupied or ():
        occ[s] = 1
    c = dict(kind=kind, rig=rig, pts=pts, th=float((1.0 if kind == "mp" else 7.0) if th is None else th), nnratio=float(nnratio), far_points=bool(far_points),
             th_far=float(th_far), check_ori=bool(check_ori), assign=np.full(slots, UNTOUCHED, np.int32) if assign is None else assign, occupied=occ)
    if expect is not None:
        n, a, o = expect
        c["expect"] = dict(n=n, assign=np.array(a, np.int32), occupied=np.array(o, np.uint8))
    return c


U = UNTOUCHED


def hand_built():
    """name -> call.  Radii: RadiusByViewingCos(1.0) = 2.5, (0.5) = 4.0, level 0 -> scale 1; last frame: th 7 * scale."""
    D, X = base_desc(1), base_desc(2)
    assert int(np.unpackbits(D ^ X).sum()) > 101
    c = {}

    # ---- Frame x map points ----
    l, r = Side(), Side()
    l.add(100, 100, D); r.add(300, 200, X)
    c["mp_left_match_with_partner"] = _call("mp", make_rig(l, r, l2r={0: 0}), mp_points([dict(proj_u=101, proj_v=100, desc=flip(D, 5))]),
                                            expect=(2, [0, 0], [1, 1]))

    l, r = Side(), Side()
    l.add(100, 100, X); r.add(300, 200, D)
    c["mp_right_match_with_r2l_partner"] = _call("mp", make_rig(l, r, r2l={0: 0}),
                                                 mp_points([dict(in_view=0, in_view_r=1, proj_u_r=301, proj_v_r=200, desc=flip(D, 5))]),
                                                 expect=(2, [0, 0], [1, 1]))

    # left: 10 and 11 bits on one octave, 10 > 0.8 * 11 -> `continue`; the right feature is a perfect match
    l, r = Side(), Side()
    l.add(100, 100, flip(D, 10)); l.add(101, 101, flip(D, 11, 100)); r.add(300, 200, D)
    pt = dict(proj_u=100.5, proj_v=100.5, in_view_r=1, proj_u_r=300, proj_v_r=200, desc=D)
    c["mp_left_ratio_exit_cancels_right"] = _call("mp", make_rig(l, r), mp_points([pt]), expect=(0, [U, U, U], [0, 0, 0]))
    l2 = Side()
    l2.add(200, 100, flip(D, 10)); l2.add(201, 101, flip(D, 11, 100))        # the same features, outside the window
    c["mp_empty_left_window_right_runs"] = _call("mp", make_rig(l2, r), mp_points([pt]), expect=(1, [U, U, 0], [0, 0, 1]))

    # th = 3: left radius 7.5, right radius 2.5; both features 5 px from their projection
    l, r = Side(), Side()
    l.add(105, 100, D); r.add(305, 200, D)
    c["mp_th_not_applied_on_the_right"] = _call("mp", make_rig(l, r), mp_points([dict(proj_u=100, proj_v=100, in_view_r=1, proj_u_r=300, proj_v_r=200, desc=D)]),
                                                th=3.0, expect=(1, [0, U], [1, 0]))

    l, r = Side(), Side()
    l.add(100, 100, X); r.add(300, 200, D)
    c["mp_no_right_level"] = _call("mp", make_rig(l, r), mp_points([dict(in_view=0, in_view_r=1, pred_level_r=-1, proj_u_r=300, proj_v_r=200, desc=D)]),
                                   expect=(0, [U, U], [0, 0]))

    # the left match writes its partner slot (right 0); the right window holds right 0 (0 bits, octave 0) and right 1 (8 bits, octave 1)
    l, r = Side(), Side()
    l.add(100, 100, D); r.add(300, 200, D, octave=0); r.add(301, 201, flip(D, 8), octave=1)
    pt = dict(proj_u=100, proj_v=100, in_view_r=1, pred_level_r=1, proj_u_r=300, proj_v_r=200, desc=D)
    c["mp_partner_write_with_obs_blocks_right_best"] = _call("mp", make_rig(l, r, l2r={0: 0}), mp_points([dict(pt, has_obs=1)]),
                                                             expect=(3, [0, 0, 0], [1, 1, 1]))
    c["mp_partner_write_without_obs_right_takes_it_again"] = _call("mp", make_rig(l, r, l2r={0: 0}), mp_points([dict(pt, has_obs=0)]),
                                                                   expect=(3, [0, 0, U], [0, 0, 0]))

    # right 0 alone, occupied before the call: the partner write without observations FREES the slot, and the right pass of the same
    # point then finds it (a window searched against the occupancy before the point would see nothing)
    l2, r2 = Side(), Side()
    l2.add(100, 100, D); r2.add(300, 200, D)
    c["mp_partner_write_frees_an_occupied_slot"] = _call("mp", make_rig(l2, r2, l2r={0: 0}), mp_points([dict(pt, has_obs=0)]), occupied=[1],
                                                         expect=(3, [0, 0], [0, 0]))

    # point 0 takes right 0 (with observations); point 1 matches left 0, whose partner write takes the slot over and frees it
    l, r = Side(), Side()
    l.add(100, 100, D); r.add(300, 200, X)
    c["mp_partner_write_overwrites_earlier_point"] = _call(
        "mp", make_rig(l, r, l2r={0: 0}),
        mp_points([dict(in_view=0, in_view_r=1, proj_u_r=300, proj_v_r=200, desc=X, has_obs=1), dict(proj_u=100, proj_v=100, desc=D, has_obs=0)]),
        expect=(3, [1, 1], [0, 0]))

    l, r = Side(), Side()
    l.add(100, 100, D); r.add(300, 200, D)
    c["mp_right_view_only"] = _call("mp", make_rig(l, r), mp_points([dict(in_view=0, in_view_r=1, proj_u=100, proj_v=100, proj_u_r=300, proj_v_r=200, desc=D)]),
                                    expect=(1, [U, 0], [0, 1]))

    l, r = Side(), Side()
    for k in range(3):
        l.add(100 + 100 * k, 100, flip(base_desc(10 + k), 0))
    pts = [dict(proj_u=100 + 100 * k, proj_v=100, desc=base_desc(10 + k)) for k in range(3)]
    pts[0]["track_depth"] = 50.0; pts[1]["bad"] = 1; pts[2]["track_depth"] = 40.0          # 40 > 40 is false
    c["mp_far_and_bad_points"] = _call("mp", make_rig(l, r), mp_points(pts), far_points=True, th_far=40.0, expect=(1, [U, U, 2], [0, 0, 1]))
    c["mp_far_points_off"] = _call("mp", make_rig(l, r), mp_points(pts), far_points=False, th_far=40.0, expect=(2, [0, U, 2], [1, 0, 1]))

    for name, oct1, exp in (("equal_octaves", 0, (0, [U, U], [0, 0])), ("different_octaves", 1, (1, [0, U], [1, 0]))):
        l, r = Side(), Side()
        r.add(300, 200, flip(D, 10), octave=0); r.add(301, 201, flip(D, 11, 100), octave=oct1)
        c["mp_right_ratio_" + name] = _call("mp", make_rig(l, r),
                                            mp_points([dict(in_view=0, in_view_r=1, pred_level_r=1, proj_u_r=300.5, proj_v_r=200.5, desc=D)]), expect=exp)

    for bits, exp in ((TH_HIGH, (1, [0], [1])), (TH_HIGH + 1, (0, [U], [0]))):
        l, r = Side(), Side()
        r.add(300, 200, flip(D, bits))
        c["mp_right_best_%d" % bits] = _call("mp", make_rig(l, r), mp_points([dict(in_view=0, in_view_r=1, proj_u_r=300, proj_v_r=200, desc=D)]), expect=exp)

    # nnratio 0.5: 10 > 0.5 * 20 is false (match), 11 > 10 is true (exit); once on each side
    for side in ("left", "right"):
        for bits, exp in ((10, (1, [0, U], [1, 0])), (11, (0, [U, U], [0, 0]))):
            l, r = Side(), Side()
            s = l if side == "left" else r
            s.add(300, 200, flip(D, bits)); s.add(301, 201, flip(D, 20, 100))
            pt = dict(proj_u=300.5, proj_v=200.5, desc=D) if side == "left" else dict(in_view=0, in_view_r=1, proj_u_r=300.5, proj_v_r=200.5, desc=D)
            c["mp_%s_ratio_boundary_%d_of_20" % (side, bits)] = _call("mp", make_rig(l, r), mp_points([pt]), nnratio=0.5, expect=exp)

    # ---- last frame ----
    l, r = Side(), Side()
    l.add(634, 100, D); r.add(300, 200, D)                            # (x = 634 rounds into the last grid column, 63)
    outside = float(np.nextafter(f32(W), f32(np.inf)))
    c["last_left_projection_one_ulp_outside"] = _call("last", make_rig(l, r), last_points([dict(proj_u=outside, proj_v=100, proj_u_r=300, proj_v_r=200, desc=D)]),
                                                      expect=(0, [U, U], [0, 0]))
    c["last_left_projection_on_the_bound"] = _call("last", make_rig(l, r), last_points([dict(proj_u=W, proj_v=100, proj_u_r=300, proj_v_r=200, desc=D)]),
                                                   expect=(2, [0, 0], [1, 1]))

    pt = dict(proj_u=100, proj_v=100, proj_u_r=300, proj_v_r=200, desc=D)
    l, r = Side(), Side()
    l.add(120, 100, D); r.add(300, 200, D)                            # 20 px away: radius 7
    c["last_left_window_empty_skips_right"] = _call("last", make_rig(l, r), last_points([pt]), expect=(0, [U, U], [0, 0]))
    l, r = Side(), Side()
    l.add(101, 100, D, octave=3); r.add(300, 200, D)                  # levels -1 .. 1
    c["last_left_window_filtered_levels_skips_right"] = _call("last", make_rig(l, r), last_points([pt]), expect=(0, [U, U], [0, 0]))
    l, r = Side(), Side()
    l.add(101, 100, D); r.add(300, 200, D)
    c["last_left_window_all_occupied_right_runs"] = _call("last", make_rig(l, r), last_points([pt]), occupied=[0], expect=(1, [U, 0], [1, 1]))

    l, r = Side(), Side()
    l.add(101, 100, D); r.add(2, 100, D)
    c["last_right_projection_outside_the_image"] = _call("last", make_rig(l, r), last_points([dict(proj_u=100, proj_v=100, proj_u_r=-3, proj_v_r=100, desc=D)]),
                                                         expect=(2, [0, 0], [1, 1]))

    # entry octave 2 (radius 7 * 1.44); right 0: octave 1, 0 bits; right 1: octave 3, 5 bits; the left feature passes every window
    for lw, name, exp in ((0, "around", [0, 0, U]), (1, "forward", [0, U, 0]), (2, "backward", [0, 0, U])):
        l, r = Side(), Side()
        l.add(101, 100, flip(D, 3), octave=2); r.add(300, 200, D, octave=1); r.add(301, 201, flip(D, 5), octave=3)
        c["last_level_window_" + name] = _call("last", make_rig(l, r), last_points([dict(pt, octave=2)], level_window=lw),
                                               expect=(2, exp, [1 if v == 0 else 0 for v in exp]))

    # seven entries, one left feature each: rotation bins 0 0 0 1 1 2 2; entries 0 and 1 also match on the right, bins 0 and 7.
    # Both sides together: bins 0 (4), 1 (2), 2 (2), 7 (1) -> bin 7 is dropped; the right side alone (1, 1) would keep it.
    l, r = Side(), Side()
    left_angle = [300, 300, 300, 270, 270, 240, 240]
    rows = []
    for k in range(7):
        Dk = base_desc(20 + k)
        l.add(50 + 60 * k, 100, Dk, angle=left_angle[k])
        rows.append(dict(proj_u=50 + 60 * k, proj_v=100, proj_u_r=50 + 60 * k, proj_v_r=300, angle=300.0, desc=Dk))
    r.add(50, 300, base_desc(20), angle=300); r.add(110, 300, base_desc(21), angle=90)
    c["last_shared_histogram_drops_right_minority_bin"] = _call("last", make_rig(l, r), last_points(rows),
                                                                expect=(8, [0, 1, 2, 3, 4, 5, 6, 0, -1], [1, 1, 1, 1, 1, 1, 1, 1, 0]))
    c["last_no_orientation_check"] = _call("last", make_rig(l, r), last_points(rows), check_ori=False,
                                           expect=(9, [0, 1, 2, 3, 4, 5, 6, 0, 1], [1] * 9))

    # right 0 in grid column 21, right 1 in column 20, both 4 bits away: column 20 is visited first
    l, r = Side(), Side()
    l.add(101, 100, D); r.add(208, 100, flip(D, 4)); r.add(202, 100, flip(D, 4, 100))
    c["last_right_tie_by_visiting_order"] = _call("last", make_rig(l, r), last_points([dict(proj_u=100, proj_v=100, proj_u_r=205, proj_v_r=100, desc=D)]),
                                                  expect=(2, [0, U, 0], [1, 0, 1]))
    return c


# ---- seeded random rigs ------------------------------------------------------------------------------------------------------

def _noisy(rng, d, max_bits):
    bits = np.unpackbits(d)
    k = int(rng.integers(0, max_bits + 1))
    if k:
        bits[rng.choice(256, k, replace=False)] ^= 1
    return np.packbits(bits)


def random_rig(seed, nl=200, nr=180, partner_frac=0.4, w=W, h=H, twin_frac=0.15, spread=None):
    """A rig frame: about partner_frac of the left features have a stereo partner on the right (a near copy of the descriptor,
    both match tables set); twin_frac of the left features have a twin next to them on the same octave (ratio exits)."""
    rng = np.random.default_rng(seed)
    l, r = Side(w, h), Side(w, h)
    lo, hi = (0.03, 0.97) if spread is None else spread
    while len(l.x) < nl:
        x, y = rng.uniform(lo * w, hi * w), rng.uniform(lo * h, hi * h)
        d = rng.integers(0, 256, 32).astype(np.uint8)
        o = int(rng.choice(4, p=[0.4, 0.3, 0.2, 0.1]))
        a = float(rng.uniform(0, 360))
        l.add(x, y, d, o, a)
        if rng.random() < twin_frac and len(l.x) < nl:
            l.add(x + rng.uniform(-1, 1), y + rng.uniform(-1, 1), _noisy(rng, d, 6), o, a)
    l2r, r2l = {}, {}
    for i in range(nl):
        if len(r.x) < nr and rng.random() < partner_frac:
            j = r.add(min(max(l.x[i] - rng.uniform(5, 40) * w / W, 0.0), w), l.y[i] + rng.uniform(-1, 1) * h / H, _noisy(rng, l.desc[i], 10), l.octave[i],
                      (l.angle[i] + rng.uniform(-3, 3)) % 360.0)
            l2r[i] = j; r2l[j] = i
    while len(r.x) < nr:
        r.add(rng.uniform(lo * w, hi * w), rng.uniform(lo * h, hi * h), rng.integers(0, 256, 32).astype(np.uint8), int(rng.choice(4, p=[0.4, 0.3, 0.2, 0.1])),
              float(rng.uniform(0, 360)))
    return make_rig(l, r, l2r, r2l)


def _start(rig, rng, occupied_frac=0.08):
    slots = len(rig["left"]["x"]) + len(rig["right"]["x"])
    return np.full(slots, -1, np.int32), (rng.random(slots) < occupied_frac).astype(np.uint8)


def random_mp_call(seed, nl=200, nr=180, n_pts=150, th=1.0, rig=None, jitter=1.5, **kw):
    rng = np.random.default_rng(seed + 77)
    rig = random_rig(seed, nl, nr, **kw) if rig is None else rig
    L, R = rig["left"], rig["right"]
    nl, nr = len(L["x"]), len(R["x"])
    rows = []
    for _ in range(n_pts):
        row = dict(in_view=int(rng.random() < 0.85), in_view_r=int(rng.random() < 0.7), view_cos=float(rng.choice([0.9, 0.9995])),
                   view_cos_r=float(rng.choice([0.9, 0.9995])), track_depth=float(rng.uniform(1, 60)), bad=int(rng.random() < 0.03), has_obs=int(rng.random() < 0.8),
                   proj_u=float(rng.uniform(0, L["max_x"])), proj_v=float(rng.uniform(0, L["max_y"])), proj_u_r=float(rng.uniform(0, L["max_x"])),
                   proj_v_r=float(rng.uniform(0, L["max_y"])), pred_level=int(rng.integers(0, 4)), pred_level_r=int(rng.integers(0, 4)),
                   desc=rng.integers(0, 256, 32).astype(np.uint8))
        j = -1
        if nl and rng.random() < 0.9:
            i = int(rng.integers(nl))
            row.update(proj_u=float(L["x"][i] + rng.uniform(-jitter, jitter)), proj_v=float(L["y"][i] + rng.uniform(-jitter, jitter)),
                       pred_level=int(L["octave"][i]) + int(rng.random() < 0.3), desc=_noisy(rng, L["desc"][i], 40))
            j = int(rig["left_to_right"][i])
        if nr and (j >= 0 or rng.random() < 0.6):
            j = j if j >= 0 else int(rng.integers(nr))
            row.update(proj_u_r=float(R["x"][j] + rng.uniform(-jitter, jitter)), proj_v_r=float(R["y"][j] + rng.uniform(-jitter, jitter)),
                       pred_level_r=int(R["octave"][j]) + int(rng.random() < 0.3))
            if rng.random() < 0.3:
                row["desc"] = _noisy(rng, R["desc"][j], 40)
        if rng.random() < 0.05:
            row["pred_level_r"] = -1
        rows.append(row)
    assign, occ = _start(rig, rng)
    return dict(kind="mp", rig=rig, pts=mp_points(rows) if rows else mp_points_empty(), th=float(th), nnratio=0.8, far_points=True, th_far=55.0, check_ori=True,
                assign=assign, occupied=occ)


def mp_points_empty():
    p = {k: np.zeros(0, t) for k, t in MP_TYPES.items()}
    p["desc"] = np.zeros((0, 32), np.uint8); p["n"] = 0
    return p


def last_points_empty(level_window=0):
    p = {k: np.zeros(0, t) for k, t in LAST_TYPES.items()}
    p["desc"] = np.zeros((0, 32), np.uint8); p["n"] = 0; p["level_window"] = level_window
    return p


def random_last_call(seed, nl=200, nr=180, n_pts=150, th=7.0, level_window=0, check_ori=True, rig=None, jitter=3.0, octave=None, **kw):
    rng = np.random.default_rng(seed + 99)
    rig = random_rig(seed, nl, nr, **kw) if rig is None else rig
    L, R = rig["left"], rig["right"]
    nl, nr = len(L["x"]), len(R["x"])
    turn = float(rng.uniform(0, 360))                                 # the camera's roll between the two frames
    rows = []
    for _ in range(n_pts):
        row = dict(valid=int(rng.random() < 0.9), has_obs=int(rng.random() < 0.8), proj_u=float(rng.uniform(-20, L["max_x"] + 20)),
                   proj_v=float(rng.uniform(-20, L["max_y"] + 20)), proj_u_r=float(rng.uniform(-20, L["max_x"] + 20)), proj_v_r=float(rng.uniform(-20, L["max_y"] + 20)),
                   octave=int(rng.integers(0, 4)), angle=float(rng.uniform(0, 360)), desc=rng.integers(0, 256, 32).astype(np.uint8))
        j = -1
        if nl and rng.random() < 0.85:
            i = int(rng.integers(nl))
            noise = rng.uniform(-8, 8) if rng.random() < 0.8 else rng.uniform(0, 360)
            row.update(proj_u=float(L["x"][i] + rng.uniform(-jitter, jitter)), proj_v=float(L["y"][i] + rng.uniform(-jitter, jitter)), octave=int(L["octave"][i]),
                       angle=float((L["angle"][i] + turn + noise) % 360.0), desc=_noisy(rng, L["desc"][i], 40))
            j = int(rig["left_to_right"][i])
        if nr and (j >= 0 or rng.random() < 0.6):
            if j < 0:
                j = int(rng.integers(nr))
                if rng.random() < 0.5:
                    row.update(desc=_noisy(rng, R["desc"][j], 40), octave=int(R["octave"][j]),
                               angle=float((R["angle"][j] + turn + (rng.uniform(-8, 8) if rng.random() < 0.8 else rng.uniform(0, 360))) % 360.0))
            row.update(proj_u_r=float(R["x"][j] + rng.uniform(-jitter, jitter)), proj_v_r=float(R["y"][j] + rng.uniform(-jitter, jitter)))
        if octave is not None:
            row["octave"] = octave
        rows.append(row)
    assign, occ = _start(rig, rng)
    return dict(kind="last", rig=rig, pts=last_points(rows, level_window) if rows else last_points_empty(level_window), th=float(th), nnratio=0.8, far_points=False,
                th_far=0.0, check_ori=bool(check_ori), assign=assign, occupied=occ)


RANDOM_SEEDS = (1, 2, 3)


def random_calls():
    c = {}
    for s in RANDOM_SEEDS:
        c["mp_random_%d" % s] = random_mp_call(s, th=(1.0, 3.0, 1.0)[s % 3])
        c["last_random_%d" % s] = random_last_call(s, level_window=s % 3)
    return c


# ---- shapes ------------------------------------------------------------------------------------------------------------------

# The dispatcher stages both sides in LDS when  align16(nl + nr) + 48 * (nl + nr) + 2 * align16(4 * (cells + 1))  fits its budget of
# 160 KB - max(static LDS of the kernel, 4 KB) - 1 KB.  With 2000 features a side the frame alone needs 48 * 4000 = 192 000 B, more
# than the whole 160 KB = 163 840 B whatever the static part is: the launch takes the unstaged path.  (1000 a side, 122.6 KB, is staged.)
UNSTAGED_N = 2000
# A side of 8193 features is one more than the device's grid sort takes: the grids of the whole launch are built on the host.  By the
# same sum 8193 + 300 features need 48 * 8493 = 407 664 B: unstaged as well.
HOST_GRID_N = (8193, 300)


def _crowded_rig(seed):
    """70 features of each side in ONE grid cell (more candidates than the wave has lanes), the rest spread out"""
    rng = np.random.default_rng(seed)
    l, r = Side(), Side()
    D = base_desc(40)
    for s, (cx, cy) in ((l, (200.0, 150.0)), (r, (400.0, 250.0))):
        for k in range(70):
            s.add(cx + rng.uniform(-4, 4), cy + rng.uniform(-4, 4), _noisy(rng, D, 60), int(rng.integers(0, 2)) + (2 if s is r else 0), float(rng.uniform(0, 360)))
        for k in range(30):
            s.add(rng.uniform(20, 620), rng.uniform(20, 460), rng.integers(0, 256, 32).astype(np.uint8), int(rng.integers(0, 3)), float(rng.uniform(0, 360)))
    return make_rig(l, r, {k: 69 - k for k in range(0, 70, 3)}, {69 - k: k for k in range(0, 70, 3)}), D


def shape_calls():
    """name -> call, or name -> list of calls (a batch, ONE launch)"""
    c = {}
    for kind, make in (("mp", random_mp_call), ("last", random_last_call)):
        c[kind + "_no_left_features"] = make(11, nl=0, nr=60, n_pts=40, partner_frac=0.0)
        c[kind + "_no_right_features"] = make(12, nl=60, nr=0, n_pts=40, partner_frac=0.0)
        c[kind + "_no_points"] = make(13, nl=40, nr=30, n_pts=0)
        c[kind + "_65_points"] = make(14, nl=80, nr=70, n_pts=65)
        c[kind + "_129_points"] = make(15, nl=120, nr=100, n_pts=129)
        c[kind + "_unstaged_%d_a_side" % UNSTAGED_N] = make(16, nl=UNSTAGED_N, nr=UNSTAGED_N, n_pts=60)
        c[kind + "_host_grid_%d_and_%d" % HOST_GRID_N] = make(20, nl=HOST_GRID_N[0], nr=HOST_GRID_N[1], n_pts=60)
        c[kind + "_batch_of_3"] = [make(17, nl=90, nr=60, n_pts=70), make(18, nl=0, nr=0, n_pts=10, partner_frac=0.0), make(19, nl=150, nr=170, n_pts=40)]
    rig, D = _crowded_rig(5)
    rng = np.random.default_rng(6)
    rows = [dict(proj_u=200 + rng.uniform(-2, 2), proj_v=150 + rng.uniform(-2, 2), in_view_r=1, proj_u_r=400 + rng.uniform(-2, 2), proj_v_r=250 + rng.uniform(-2, 2),
                 pred_level=1, pred_level_r=3, view_cos=0.9, view_cos_r=0.9, has_obs=int(k % 4 != 0), desc=_noisy(rng, D, 50)) for k in range(40)]
    c["mp_70_features_in_one_cell"] = _call("mp", rig, mp_points(rows), th=2.0)
    rows = [dict(proj_u=200 + rng.uniform(-2, 2), proj_v=150 + rng.uniform(-2, 2), proj_u_r=400 + rng.uniform(-2, 2), proj_v_r=250 + rng.uniform(-2, 2),
                 octave=3, angle=float(rng.uniform(0, 360)), has_obs=int(k % 4 != 0), desc=_noisy(rng, D, 50)) for k in range(40)]
    c["last_70_features_in_one_cell"] = _call("last", rig, last_points(rows, level_window=2), th=7.0)          # levels 0 .. 3: the whole cell
    # Windows wider than 16 grid columns (search_window's other path).  Last frame: every entry on octave 7, th 30: radius 30 * 3.58 =
    # 107 px -> 22 columns of 10 px on both sides.  Map points: the right radius is at most 4 * scale[7] = 14.3 px whatever th is, so
    # the frame is a 64 x 48 px image (cells of 1 px): 29 columns on the right, the whole image on the left (th = 3: 43 px).
    wide = random_rig(21, nl=150, nr=150)
    for g in (wide["left"], wide["right"]):
        g["octave"][:] = np.where(np.arange(len(g["octave"])) % 2 == 0, 7, 6)
    c["last_window_wider_than_16_columns"] = random_last_call(21, rig=wide, n_pts=40, th=30.0, octave=7)
    small = random_rig(22, nl=150, nr=150, w=64.0, h=48.0)
    for g in (small["left"], small["right"]):
        g["octave"][:] = np.where(np.arange(len(g["octave"])) % 2 == 0, 7, 6)
    call = random_mp_call(22, rig=small, n_pts=40, th=3.0, jitter=0.3)
    call["pts"]["pred_level"][:] = 7; call["pts"]["pred_level_r"][:] = 7
    c["mp_window_wider_than_16_columns"] = call
    return c
