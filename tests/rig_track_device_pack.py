"""Packs calls of tests/rig_match_cases.py into the [batch][cap] arrays of include/orbslam3_hip_rig_track_device.h and runs the two
device-resident rig searches on them.  A test helper, not a test (tools/rig_track_device_timing.py uses it too).

cap = the largest count of the batch (at least 1).  Every array has `spare` rows beyond the batch; rows beyond a frame's count, slots
beyond n_l + n_r and the spare rows hold sentinels chosen so that an implementation that reads them shows in the result: the key
points lie inside the image, the points are valid and in view, the levels are out of the table and the partner entries out of range."""
import numpy as np

import rig_match_cases as MC

F32 = np.float32
SLOT_EXTRA = 8                      # slots of a row beyond cap_l + cap_r
ASSIGN_SENTINEL, OCC_SENTINEL, COUNT_SENTINEL = -99, 0x5a, -12345
LAST_FIELDS = (("d_valid", "valid"), ("d_u", "proj_u"), ("d_v", "proj_v"), ("d_u_r", "proj_u_r"), ("d_v_r", "proj_v_r"), ("d_octave", "octave"),
               ("d_angle", "angle"), ("d_has_obs", "has_obs"))
MP_FIELDS = (("d_in_view", "in_view"), ("d_u", "proj_u"), ("d_v", "proj_v"), ("d_pred_level", "pred_level"), ("d_view_cos", "view_cos"),
             ("d_in_view_r", "in_view_r"), ("d_u_r", "proj_u_r"), ("d_v_r", "proj_v_r"), ("d_pred_level_r", "pred_level_r"), ("d_view_cos_r", "view_cos_r"),
             ("d_track_depth", "track_depth"), ("d_bad", "bad"), ("d_has_obs", "has_obs"))
POINT_FILL = dict(valid=1, in_view=1, in_view_r=1, proj_u=100.0, proj_v=100.0, proj_u_r=100.0, proj_v_r=100.0, octave=99, pred_level=99, pred_level_r=99,
                  view_cos=1.0, view_cos_r=1.0, track_depth=1.0, bad=0, has_obs=1, angle=0.0)


def key_points(side, cap, rows):
    """[rows][cap] OrbxKeyPoint records (7 x 4 bytes: x y size angle response | octave class_id) as a float32 array"""
    k = np.zeros((rows, cap, 7), F32)
    k[:, :, 0] = 100.0; k[:, :, 1] = 100.0                          # fill: inside the image, octave 0
    k.view(np.int32)[:, :, 6] = -1
    for b, g in enumerate(side):
        n = len(g["x"])
        k[b, :n, 0] = g["x"]; k[b, :n, 1] = g["y"]; k[b, :n, 2] = 31.0; k[b, :n, 3] = g["angle"]
        k.view(np.int32)[b, :n, 5] = g["octave"]
    return k


def pack(calls, spare=1):
    """list of calls of one kind and one set of launch parameters -> dict(kind, B, cap_l, cap_r, cap, slot_cap, host arrays by field name,
    frames / points: the non-array fields)"""
    kind, B = calls[0]["kind"], len(calls)
    rows = B + spare
    L, R = [c["rig"]["left"] for c in calls], [c["rig"]["right"] for c in calls]
    nl, nr, npt = [len(g["x"]) for g in L], [len(g["x"]) for g in R], [int(c["pts"]["n"]) for c in calls]
    cap_l, cap_r, cap = max(nl + [1]), max(nr + [1]), max(npt + [1])
    slot_cap = cap_l + cap_r + SLOT_EXTRA
    h = dict(d_kps_l=key_points(L, cap_l, rows), d_kps_r=key_points(R, cap_r, rows))
    for name, side, c_, ns in (("d_desc_l", L, cap_l, nl), ("d_desc_r", R, cap_r, nr)):
        d = np.full((rows, c_, 32), 0xa5, np.uint8)
        for b, g in enumerate(side):
            d[b, :ns[b]] = g["desc"].reshape(ns[b], 32)
        h[name] = d
    h["d_n_l"] = np.array(nl + [COUNT_SENTINEL] * spare, np.int32); h["d_n_r"] = np.array(nr + [COUNT_SENTINEL] * spare, np.int32)
    h["d_n"] = np.array(npt + [COUNT_SENTINEL] * spare, np.int32)
    h["d_left_to_right"] = np.full((rows, cap_l), 7777, np.int32); h["d_right_to_left"] = np.full((rows, cap_r), 7777, np.int32)
    for b, c in enumerate(calls):
        h["d_left_to_right"][b, :nl[b]] = c["rig"]["left_to_right"]; h["d_right_to_left"][b, :nr[b]] = c["rig"]["right_to_left"]
    types = MC.LAST_TYPES if kind == "last" else MC.MP_TYPES
    for dev, key in (LAST_FIELDS if kind == "last" else MP_FIELDS):
        a = np.full((rows, cap), POINT_FILL[key], types[key])
        for b, c in enumerate(calls):
            a[b, :npt[b]] = c["pts"][key]
        h[dev] = a
    d = np.full((rows, cap, 32), 0x3c, np.uint8)
    for b, c in enumerate(calls):
        d[b, :npt[b]] = c["pts"]["desc"].reshape(npt[b], 32)
    h["d_desc"] = d
    if kind == "last":
        h["d_level_window"] = np.array([int(c["pts"].get("level_window", 0)) for c in calls] + [0] * spare, np.int32)
    h["assign"] = np.full((rows, slot_cap), ASSIGN_SENTINEL, np.int32); h["occupied"] = np.full((rows, slot_cap), OCC_SENTINEL, np.uint8)
    for b, c in enumerate(calls):
        h["assign"][b, :nl[b] + nr[b]] = c["assign"]; h["occupied"][b, :nl[b] + nr[b]] = c["occupied"]
    h["n_matches"] = np.full(rows, COUNT_SENTINEL, np.int32); h["n_slots"] = np.full(rows, COUNT_SENTINEL, np.int32)
    g = L[0]
    frames = dict(cap_l=cap_l, cap_r=cap_r, slot_cap=slot_cap, min_x=g["min_x"], min_y=g["min_y"], max_x=g["max_x"], max_y=g["max_y"],
                  grid_cols=g["cols"], grid_rows=g["rows"], scale_factors=calls[0]["rig"]["scale"])
    for c in calls:
        for s in (c["rig"]["left"], c["rig"]["right"]):
            assert all(s[k] == g[k] for k in ("min_x", "min_y", "max_x", "max_y", "cols", "rows")) and np.array_equal(c["rig"]["scale"], calls[0]["rig"]["scale"])
        assert (c["kind"], c["th"], c["nnratio"], c["far_points"], c["th_far"], c["check_ori"]) == tuple(calls[0][k] for k in ("kind", "th", "nnratio", "far_points", "th_far", "check_ori"))
    return dict(kind=kind, B=B, rows=rows, nl=nl, nr=nr, cap=cap, slot_cap=slot_cap, host=h, frames=frames, call=calls[0])


FRAME_ARRAYS = ("d_kps_l", "d_desc_l", "d_n_l", "d_kps_r", "d_desc_r", "d_n_r", "d_left_to_right", "d_right_to_left")
OUT_ARRAYS = ("assign", "occupied", "n_matches", "n_slots")


class Resident:
    """a pack()ed batch in device memory (torch only allocates and copies)"""

    def __init__(self, torch, p):
        self.torch, self.p = torch, p
        self.dev = torch.device("cuda", 0)
        self.t = {k: self.up(a) for k, a in p["host"].items()}
        self.stream = torch.cuda.current_stream().cuda_stream

    def up(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(self.dev)

    def down(self, k):
        h = self.p["host"][k]
        return self.t[k].cpu().numpy().view(h.dtype).reshape(h.shape).copy()

    def reset_outputs(self):
        for k in OUT_ARRAYS:
            self.t[k].copy_(self.up(self.p["host"][k]))

    def launch(self, m, level_window=True, has_obs=True, n_slots=True):
        """one device-resident search over the batch; only enqueues"""
        p, t = self.p, self.t
        c = p["call"]
        frames = dict(p["frames"], **{k: t[k].data_ptr() for k in FRAME_ARRAYS})
        names = LAST_FIELDS if p["kind"] == "last" else MP_FIELDS
        pts = {dev: t[dev].data_ptr() for dev, _ in names}
        pts.update(d_desc=t["d_desc"].data_ptr(), d_n=t["d_n"].data_ptr(), cap=p["cap"])
        out = (t["assign"].data_ptr(), t["occupied"].data_ptr(), t["n_matches"].data_ptr(), t["n_slots"].data_ptr() if n_slots else None, self.stream)
        m.nnratio, m.check_ori = c["nnratio"], c["check_ori"]
        if p["kind"] == "last":
            if level_window:
                pts["d_level_window"] = t["d_level_window"].data_ptr()
            if not has_obs:
                del pts["d_has_obs"]
            m.search_by_projection_last_rig_batch_device(frames, pts, p["B"], c["th"], *out)
        else:
            m.search_by_projection_rig_batch_device(frames, pts, p["B"], c["th"], *out, far_points=c["far_points"], th_far=c["th_far"])

    def results(self):
        """after a synchronise: per frame (n_matches, assign, occupied) of the live slots, and the four output arrays whole"""
        self.torch.cuda.synchronize()
        raw = {k: self.down(k) for k in OUT_ARRAYS}
        p = self.p
        per = [(int(raw["n_matches"][b]), raw["assign"][b, :p["nl"][b] + p["nr"][b]].copy(), raw["occupied"][b, :p["nl"][b] + p["nr"][b]].copy()) for b in range(p["B"])]
        return per, raw


def check_untouched(p, raw, n_slots=True):
    """slots at or beyond n_l + n_r, the spare rows and the counts of the spare rows hold their sentinels; n_slots = n_l + n_r (or, for
    a call without d_n_slots, its sentinel)"""
    for b in range(p["rows"]):
        live = p["nl"][b] + p["nr"][b] if b < p["B"] else 0
        assert (raw["assign"][b, live:] == ASSIGN_SENTINEL).all() and (raw["occupied"][b, live:] == OCC_SENTINEL).all(), "row %d written beyond its %d slots" % (b, live)
        if b < p["B"]:
            assert raw["n_slots"][b] == (live if n_slots else COUNT_SENTINEL), (b, raw["n_slots"][b], live)
        else:
            assert raw["n_slots"][b] == COUNT_SENTINEL and raw["n_matches"][b] == COUNT_SENTINEL
