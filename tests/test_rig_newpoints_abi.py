"""The rig CreateNewMapPoints part of the C ABI (include/orbslam3_hip_rig_newpoints.h, which include/orbslam3_hip.h includes; no
GPU): the functions are declared there and exported, the ctypes mirrors have the layout of the C structs, every refusal of the
host-only argument check is answered with ORBX_ERR_ARG before anything touches a device, a call with nothing to do returns 0
without a device, and the entry refuses a NULL handle."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import rig_newpoints_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "orbslam3_hip.h")
HEADER_RIG = os.path.join(ROOT, "include", "orbslam3_hip_rig_newpoints.h")
EXPECTED = sorted(["orbm_create_new_map_points_rig", "orbm_create_new_map_points_rig_check", "orbm_create_new_map_points_rig_last_kernel_ms",
                   "orbm_create_new_map_points_rig_last_launches"])
ERR_ARG = -3


@pytest.fixture(scope="module")
def capi(pkg):
    m = importlib.import_module("orb_slam3-1_amd.capi")
    m._rig_newpoints_argtypes()
    return m


def test_symbols_declared_and_exported(pkg, capi):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_RIG).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(orb[mx]_[a-z0-9_]+)\s*\(", src))) == EXPECTED
    text = open(HEADER).read()
    assert text.index('#include "orbslam3_hip_rig_bow.h"') < text.index('#include "orbslam3_hip_rig_newpoints.h"')
    for n in EXPECTED:
        assert hasattr(pkg.lib, n), "symbol %s declared in include/orbslam3_hip_rig_newpoints.h is not exported" % n
    for n in ("create_new_map_points_rig", "create_new_map_points_rig_prepare", "create_new_map_points_rig_launch", "create_new_map_points_rig_last"):
        assert callable(getattr(pkg.Matcher, n)), n
    assert callable(capi.create_new_map_points_rig_check)


def test_struct_layouts_match_header(capi):
    names = ("OrbmRigMapKeyFrame", "OrbmRigMapPair", "OrbmMapParams", "OrbmNewPoints")
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
    k = capi.OrbmRigMapKeyFrame
    assert k.Rcw.size == 72 and k.tcw.size == 24 and k.Ow.size == 24 and k.cam.size == 72


def _fv(ids, off, feat):
    return (np.array(ids, np.uint32), np.array(off, np.int32), np.array(feat, np.uint32))


def test_every_refusal_of_the_check(pkg, capi):
    sc = cases.shape_scene("two_neighbours")
    kf1, nbs, pairs, params = sc["kf1"], sc["neighbours"], sc["pairs"], sc["params"]
    n1, n2 = len(kf1["x"]), len(nbs[1]["x"])

    def chk(k1=None, nb1=None, pair1=None, **kw):
        """the check with changes to key frame 1, to neighbour 1, to pair 1"""
        a = None if k1 == "NULL" else dict(kf1, **(k1 or {}))
        b = [nbs[0], dict(nbs[1], **(nb1 or {}))]
        p = [pairs[0], dict(pairs[1], **(pair1 or {}))]
        return capi.create_new_map_points_rig_check(a, b, p, params, **kw)

    assert chk() == 0 and chk(k1=dict(n_left=0)) == 0 and chk(nb1=dict(n_left=n2)) == 0 and chk(nb1=dict(mb=0.0)) == 0
    oct_hi = kf1["octave"].copy(); oct_hi[2] = 8
    oct_neg = nbs[1]["octave"].copy(); oct_neg[0] = -1
    twice = _fv([1, 2], [0, 1, 2], [0, 0])
    big = np.zeros(65536, np.uint32)
    bad = {
        "kf1 NULL": dict(k1="NULL"), "params NULL": dict(null_args=("params",)), "out NULL": dict(null_args=("out",)),
        "neighbours NULL": dict(null_args=("neighbours",)), "pairs NULL": dict(null_args=("pairs",)), "geom NULL": dict(pair1=dict(geom=None)),
        "n_neighbours -1": dict(n_neighbours=-1), "n_neighbours 65": dict(n_neighbours=capi.ORBM_MAX_NEIGHBOURS + 1),
        "negative n1": dict(k1=dict(n=-1)), "negative n2": dict(nb1=dict(n=-1)),
        "n_left_1 < 0": dict(k1=dict(n_left=-1)), "n_left_1 > n": dict(k1=dict(n_left=n1 + 1)), "n_left_2 < 0": dict(nb1=dict(n_left=-1)), "n_left_2 > n": dict(nb1=dict(n_left=n2 + 1)),
        "no levels": dict(k1=dict(n_levels=0)), "33 levels": dict(nb1=dict(n_levels=33)), "octave == n_levels": dict(k1=dict(octave=oct_hi)), "octave -1": dict(nb1=dict(octave=oct_neg)),
        "octave beyond fewer levels": dict(nb1=dict(n_levels=1)), "sigma2 NULL": dict(k1=dict(level_sigma2=None, n_levels=8)), "scale NULL": dict(nb1=dict(scale_factors=None, n_levels=8)),
        "mb NaN": dict(k1=dict(mb=float("nan"))), "mb negative": dict(nb1=dict(mb=-0.1)),
        "fv1 negative node count": dict(k1=dict(fv=kf1["fv"] + (-1,))), "fv2 node ids NULL": dict(nb1=dict(fv=(None,) + nbs[1]["fv"][1:] + (len(nbs[1]["fv"][0]),))),
        "fv1 node ids equal": dict(k1=dict(fv=_fv([4, 4], [0, 1, 2], [0, 1]))), "fv2 node ids descending": dict(nb1=dict(fv=_fv([5, 4], [0, 1, 2], [0, 1]))),
        "fv2 offsets not monotone": dict(nb1=dict(fv=_fv([1, 2], [0, 2, 1], [0, 1]))), "fv2 offsets do not start at 0": dict(nb1=dict(fv=_fv([1], [1, 2], [0, 1]))),
        "fv1 offsets do not start at 0": dict(k1=dict(fv=_fv([1], [1, 2], [0, 1]))),
        "fv1 feature index == n": dict(k1=dict(fv=_fv([1], [0, 1], [n1]))), "fv2 feature index == n": dict(nb1=dict(fv=_fv([1], [0, 1], [n2]))),
        "fv2 node of 65536 features": dict(nb1=dict(fv=_fv([1], [0, 65536], big))), "fv1 node of 65536 features": dict(k1=dict(fv=_fv([1], [0, 65536], big))),
        "fv1 feature in two nodes": dict(k1=dict(fv=twice)),
        "n_matched NULL": dict(null=("n_matched",)), "n_created NULL": dict(null=("n_created",)),
        "normal alone NULL": dict(null=("normal",)), "max_dist and min_dist NULL": dict(null=("max_dist", "min_dist")),
    }
    for k in ("desc", "has_mp", "x", "y", "octave"):
        bad["kf1 %s NULL" % k] = dict(k1={k: None, "n": n1})
        bad["neighbour %s NULL" % k] = dict(nb1={k: None, "n": n2})
    for k in ("neighbour", "idx2", "x3d", "point_stereo"):
        bad["out %s NULL" % k] = dict(null=(k,))
    for name, change in bad.items():
        assert chk(**change) == ERR_ARG and pkg.lib.orbx_last_error(), name
    # what is legal: a repeated feature in a NEIGHBOUR's vector (only read: a candidate twice), a node of 65 535 features, no normal
    # outputs at all, no match12, NULL arrays without features, `stereo` and `angle` always NULL
    assert chk(nb1=dict(fv=twice)) == 0
    assert chk(nb1=dict(fv=_fv([1], [0, 65535], np.zeros(65535, np.uint32)))) == 0
    assert chk(null=("normal", "max_dist", "min_dist")) == 0 and chk(null=("match12",)) == 0
    empty = dict(desc=None, has_mp=None, x=None, y=None, octave=None, fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)), n_left=0)
    assert chk(k1=empty, null=("neighbour", "idx2", "x3d", "point_stereo", "normal", "max_dist", "min_dist")) == 0
    assert chk(nb1=empty) == 0


def test_nothing_to_do_returns_0_without_a_device(pkg, capi):
    sc = cases.shape_scene("two_neighbours")
    p = capi.rig_new_points_args(sc["kf1"], [], [], sc["params"])
    assert capi.create_new_map_points_rig_launch(None, p) == 0                      # n_neighbours = 0
    r = capi.rig_new_points_result(p, 0)
    assert (r["neighbour"] == -1).all() and (r["idx2"] == -1).all() and (r["x3d"] == 0).all() and len(r["n_matched"]) == 0 and len(r["skipped"]) == 0
    k = sc["kf1"]
    empty = dict(k, desc=np.zeros((0, 32), np.uint8), fv=(np.zeros(0, np.uint32), np.zeros(1, np.int32), np.zeros(0, np.uint32)), n_left=0,
                 **{f: k[f][:0] for f in ("x", "y", "octave", "has_mp")})
    p = capi.rig_new_points_args(empty, sc["neighbours"], sc["pairs"], sc["params"])
    assert capi.create_new_map_points_rig_launch(None, p) == 0                      # key frame 1 without features
    assert (p["arrays"]["n_matched"] == 0).all() and (p["skipped"] == 0).all()
    # ... and the baseline test still reports: nothing can match, so Ow1 stays the left centre
    sk = cases.shape_scene("all_skipped")
    p = capi.rig_new_points_args(dict(empty, Ow=sk["kf1"]["Ow"]), sk["neighbours"], sk["pairs"], sk["params"])
    assert capi.create_new_map_points_rig_launch(None, p) == 0 and (p["skipped"][:3] == 1).all()


def test_entry_refuses_a_null_handle_and_bad_arguments_before_any_device_call(pkg, capi):
    sc = cases.shape_scene("two_neighbours")
    lib = pkg.lib
    p = capi.rig_new_points_args(sc["kf1"], sc["neighbours"], sc["pairs"], sc["params"])
    call = lambda h, q: lib.orbm_create_new_map_points_rig(h, C.byref(q["kfs"]), C.byref(q["kfs"], C.sizeof(capi.OrbmRigMapKeyFrame)), q["n_neighbours"],
                                                           C.byref(q["pairs"]), C.byref(q["params"]), C.byref(q["out"]), q["skipped"].ctypes.data)
    assert call(None, p) in (ERR_ARG, -4)              # no handle: ORBX_ERR_NO_DEVICE where there is no device, else "NULL matcher"
    assert lib.orbm_create_new_map_points_rig_last_kernel_ms(None) == 0.0 and lib.orbm_create_new_map_points_rig_last_launches(None) == 0
    # a handle that is no handle: the checks come before it is touched
    fake = C.c_void_p(8)
    bad = capi.rig_new_points_args(dict(sc["kf1"], n_left=-1), sc["neighbours"], sc["pairs"], sc["params"])
    assert call(fake, bad) == ERR_ARG
    bad = capi.rig_new_points_args(sc["kf1"], sc["neighbours"], sc["pairs"], sc["params"], n_neighbours=capi.ORBM_MAX_NEIGHBOURS + 1)
    assert call(fake, bad) == ERR_ARG
