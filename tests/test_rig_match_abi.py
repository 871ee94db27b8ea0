"""The rig-frame tracking searches' part of the C ABI (include/orbslam3_hip_rig_match.h, which include/orbslam3_hip.h includes; no
GPU): the functions are declared there and exported, the ctypes mirrors have the layout of the C structs, every refusal of the
host-only argument check is answered with ORBX_ERR_ARG before anything touches a device, and the four search entries refuse a
NULL handle."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import rig_match_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "orbslam3_hip.h")
HEADER_RIG = os.path.join(ROOT, "include", "orbslam3_hip_rig_match.h")
EXPECTED = sorted(["orbm_rig_search_check", "orbm_search_by_projection_rig", "orbm_search_by_projection_last_rig", "orbm_search_by_projection_rig_batch",
                   "orbm_search_by_projection_last_rig_batch", "orbm_rig_search_last_kernel_ms"])
ERR_ARG = -3


@pytest.fixture(scope="module")
def capi(pkg):
    m = importlib.import_module("orb_slam3-1_amd.capi")
    m._rig_match_argtypes()
    return m


def test_symbols_declared_and_exported(pkg, capi):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_RIG).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(orb[mx]_[a-z0-9_]+)\s*\(", src))) == EXPECTED
    assert '#include "orbslam3_hip_rig_match.h"' in open(HEADER).read()
    for n in EXPECTED:
        assert hasattr(pkg.lib, n), "symbol %s declared in include/orbslam3_hip_rig_match.h is not exported" % n
    for n in ("search_by_projection_rig", "search_by_projection_last_rig", "search_by_projection_rig_batch", "search_by_projection_last_rig_batch",
              "rig_search_last_kernel_ms"):
        assert callable(getattr(pkg.Matcher, n)), n


def test_struct_layouts_match_header(capi):
    names = ("OrbmRigFrame", "OrbmRigMapPoints", "OrbmRigLastPoints", "OrbmRigMapQuery", "OrbmRigLastQuery")
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbslam3_hip.h"', "int main(void) {"]
    for s in names:
        lines.append('printf("%s.size %%zu\\n", sizeof(%s));' % (s, s))
        for f, _ in getattr(capi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        seen = dict(l.split() for l in subprocess.check_output([exe], text=True).strip().splitlines())
    for s in names:
        cls = getattr(capi, s)
        assert int(seen[s + ".size"]) == C.sizeof(cls), s
        for f, _ in cls._fields_:
            assert int(seen["%s.%s" % (s, f)]) == getattr(cls, f).offset, (s, f)
    assert C.sizeof(capi.OrbmRigFrame) == 2 * C.sizeof(capi.Frame) + 16


def _good():
    c = cases.random_mp_call(31, nl=6, nr=5, n_pts=4)
    d = cases.random_last_call(31, nl=6, nr=5, n_pts=4)
    for p in (c["pts"], d["pts"]):
        for k in ("in_view", "in_view_r", "valid"):
            if k in p:
                p[k][:] = 1
    c["pts"]["pred_level_r"][0] = -1                                  # the reference's "no level": legal
    return c, d


def _side(rig, side, **kw):
    return dict(rig, **{side: dict(rig[side], **kw)})


def test_every_refusal_of_the_check(pkg, capi):
    c, d = _good()
    rig, mp, last, a, o = c["rig"], c["pts"], d["pts"], c["assign"], c["occupied"]
    chk = lambda rig=rig, mp=mp, last=None, a=a, o=o: capi.rig_search_check(rig, mp, last, a, o)
    assert chk() == 0 and chk(mp=None, last=last) == 0
    with_u_right = _side(rig, "left", u_right=np.zeros(6, np.float32))
    other_scale = _side(rig, "right", scale=(rig["scale"] * np.float32(1.01)).astype(np.float32))
    l2r_hi, l2r_lo, r2l_hi = rig["left_to_right"].copy(), rig["left_to_right"].copy(), rig["right_to_left"].copy()
    l2r_hi[2] = 5; l2r_lo[1] = -2; r2l_hi[0] = 6
    lvl_hi, lvl_neg, lvl_r_low, lvl_r_hi = (dict(mp) for _ in range(4))
    lvl_hi["pred_level"] = mp["pred_level"].copy(); lvl_hi["pred_level"][1] = cases.NLEVELS
    lvl_neg["pred_level"] = mp["pred_level"].copy(); lvl_neg["pred_level"][2] = -1             # -1 is legal on the right only
    lvl_r_low["pred_level_r"] = mp["pred_level_r"].copy(); lvl_r_low["pred_level_r"][1] = -2
    lvl_r_hi["pred_level_r"] = mp["pred_level_r"].copy(); lvl_r_hi["pred_level_r"][3] = cases.NLEVELS
    oct_hi = dict(last, octave=last["octave"].copy()); oct_hi["octave"][0] = cases.NLEVELS
    oct_neg = dict(last, octave=last["octave"].copy()); oct_neg["octave"][3] = -1
    bad = {
        "rig NULL": dict(rig=None), "assign NULL": dict(a=None), "occupied NULL": dict(o=None),
        "neither map points nor last": dict(mp=None), "both map points and last": dict(last=last),
        "left.u_right set": dict(rig=with_u_right),
        "left x NULL": dict(rig=_side(rig, "left", x=None)), "right y NULL": dict(rig=_side(rig, "right", y=None)),
        "left octave NULL": dict(rig=_side(rig, "left", octave=None)), "right desc NULL": dict(rig=_side(rig, "right", desc=None)),
        "left scale NULL": dict(rig=_side(rig, "left", scale=None, n_levels=8)), "left_to_right NULL": dict(rig=dict(rig, left_to_right=None)),
        "right_to_left NULL": dict(rig=dict(rig, right_to_left=None)),
        "min_x differs": dict(rig=_side(rig, "right", min_x=1.0)), "min_y differs": dict(rig=_side(rig, "right", min_y=1.0)),
        "max_x differs": dict(rig=_side(rig, "right", max_x=641.0)), "max_y differs": dict(rig=_side(rig, "left", max_y=479.0)),
        "grid_cols differ": dict(rig=_side(rig, "right", cols=32)), "grid_rows differ": dict(rig=_side(rig, "left", rows=24)),
        "n_levels differ": dict(rig=_side(rig, "right", scale=rig["scale"][:7].copy())), "scale factors differ": dict(rig=other_scale),
        "no levels": dict(rig=dict(_side(_side(rig, "left", n_levels=0), "right", n_levels=0))),
        "left_to_right == right.n": dict(rig=dict(rig, left_to_right=l2r_hi)), "left_to_right < -1": dict(rig=dict(rig, left_to_right=l2r_lo)),
        "right_to_left == left.n": dict(rig=dict(rig, right_to_left=r2l_hi)),
        "level == n_levels": dict(mp=lvl_hi), "left level -1": dict(mp=lvl_neg), "right level -2": dict(mp=lvl_r_low), "right level == n_levels": dict(mp=lvl_r_hi),
        "octave == n_levels": dict(mp=None, last=oct_hi), "octave -1": dict(mp=None, last=oct_neg),
        "negative point count": dict(mp=dict(mp, n=-1)), "negative entry count": dict(mp=None, last=dict(last, n=-1)),
    }
    for k in ("in_view", "proj_u", "proj_v", "pred_level", "view_cos", "in_view_r", "proj_u_r", "proj_v_r", "pred_level_r", "view_cos_r", "track_depth", "bad",
              "has_obs", "desc"):
        bad["map points: %s NULL" % k] = dict(mp=dict(mp, **{k: None}))
    for k in ("valid", "proj_u", "proj_v", "proj_u_r", "proj_v_r", "octave", "has_obs", "desc"):
        bad["last: %s NULL" % k] = dict(mp=None, last=dict(last, **{k: None}))
    for name, change in bad.items():
        assert chk(**change) == ERR_ARG and pkg.lib.orbx_last_error(), name
    # what is legal: a level out of range on a point that is not in view, NULL arrays with an empty side or no points, a NULL angle
    dead = dict(lvl_hi, in_view=mp["in_view"].copy()); dead["in_view"][1] = 0
    assert chk(mp=dead) == 0
    assert chk(mp=None, last=dict(last, angle=None)) == 0
    assert chk(mp=dict({k: None for k in mp}, n=0)) == 0
    e = cases.random_mp_call(32, nl=0, nr=0, n_pts=3, partner_frac=0.0)
    none = dict(e["rig"], left_to_right=None, right_to_left=None)
    for s in ("left", "right"):
        none = _side(none, s, x=None, y=None, octave=None, desc=None, angle=None)
    one = np.zeros(1, np.int32)                                        # (assign / occupied must be addresses even where there is no slot)
    assert capi.rig_search_check(none, e["pts"], None, one, one.view(np.uint8)) == 0


def test_search_entries_refuse_a_null_handle(pkg, capi):
    c, d = _good()
    r, _ = capi.rig_frame(c["rig"])
    mp, last = capi.rig_map_points(c["pts"]), capi.rig_last_points(d["pts"])
    a, o = c["assign"].ctypes.data_as(C.c_void_p), c["occupied"].ctypes.data_as(C.c_void_p)
    assert pkg.lib.orbm_search_by_projection_rig(None, C.byref(r), C.byref(mp), 1.0, 0, 0.0, 0.8, a, o) == ERR_ARG
    assert b"NULL matcher" in pkg.lib.orbx_last_error()
    assert pkg.lib.orbm_search_by_projection_last_rig(None, C.byref(r), C.byref(last), 7.0, 0, 1, a, o) == ERR_ARG
    qm = (capi.OrbmRigMapQuery * 1)(capi.OrbmRigMapQuery(C.pointer(r), C.pointer(mp), a.value, o.value, 0))
    ql = (capi.OrbmRigLastQuery * 1)(capi.OrbmRigLastQuery(C.pointer(r), C.pointer(last), 0, a.value, o.value, 0))
    assert pkg.lib.orbm_search_by_projection_rig_batch(None, qm, 1, 1.0, 0, 0.0, 0.8) == ERR_ARG
    assert pkg.lib.orbm_search_by_projection_last_rig_batch(None, ql, 1, 7.0, 1) == ERR_ARG
    assert pkg.lib.orbm_rig_search_last_kernel_ms(None) == 0.0
