"""The stereo-fisheye part of the C ABI (include/orbslam3_hip_fisheye.h, which include/orbslam3_hip.h includes; no GPU): the functions
are declared there and exported, the ctypes mirror has the layout of the C struct, every refusal of the host-only argument check is
answered with ORBX_ERR_ARG before anything touches a device (orbm_stereo_fisheye_check, and both entries on a NULL handle), and
without a device orbm_create fails loudly."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import fisheye_stereo_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "orbslam3_hip.h")
HEADER_FISHEYE = os.path.join(ROOT, "include", "orbslam3_hip_fisheye.h")
EXPECTED = sorted(["orbm_stereo_fisheye_check", "orbm_stereo_fisheye", "orbm_stereo_fisheye_last_kernel_ms", "orbm_stereo_fisheye_batch_device",
                   "orbx_kb8_triangulate_matches"])
ERR_ARG, ERR_NO_DEVICE = -3, -4


@pytest.fixture(scope="module")
def capi(pkg):
    m = importlib.import_module("orb_slam3-1_amd.capi")
    m._fisheye_argtypes()
    return m


def test_symbols_declared_and_exported(pkg, capi):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_FISHEYE).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(orb[mx]_[a-z0-9_]+)\s*\(", src))) == EXPECTED
    assert '#include "orbslam3_hip_fisheye.h"' in open(HEADER).read()
    for n in EXPECTED:
        assert hasattr(pkg.lib, n), "symbol %s declared in include/orbslam3_hip_fisheye.h is not exported" % n
    assert callable(pkg.Matcher.stereo_fisheye) and callable(pkg.Matcher.stereo_fisheye_device) and callable(pkg.kb8_triangulate_matches)
    assert "one call at a time" in open(HEADER_FISHEYE).read().lower()            # the header says how a handle and streams go together
    assert int(re.search(r"#define ORBM_FISHEYE_KNN_CHUNK (\d+)", open(HEADER_FISHEYE).read()).group(1)) == pkg.ORBM_FISHEYE_KNN_CHUNK


def test_struct_layout_matches_header(capi):
    cls = capi.OrbxFisheyeRig
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbslam3_hip.h"', "int main(void) {", 'printf("size %zu\\n", sizeof(OrbxFisheyeRig));']
    for f, _ in cls._fields_:
        lines.append('printf("%s %%zu\\n", offsetof(OrbxFisheyeRig, %s));' % (f, f))
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        seen = dict(l.split() for l in subprocess.check_output([exe], text=True).strip().splitlines())
    assert int(seen["size"]) == C.sizeof(cls) == 184
    for f, _ in cls._fields_:
        assert int(seen[f]) == getattr(cls, f).offset, f
    rig = capi.fisheye_rig(cases.RIGS["tumvi"])
    raw = bytes(rig)
    assert np.frombuffer(raw[:64], np.float64)[0] == cases.RIGS["tumvi"]["left"]["fx"] and np.frombuffer(raw[64:128], np.float64)[7] == cases.RIGS["tumvi"]["right"]["k"][3]
    assert np.array_equal(np.frombuffer(raw[136:172], np.float32), cases.RIGS["tumvi"]["Rlr"].reshape(-1))
    assert np.array_equal(np.frombuffer(raw[172:184], np.float32), cases.RIGS["tumvi"]["tlr"]) and np.frombuffer(raw[128:136], np.float32).tolist() == [np.float32(1e-6)] * 2


def _frame(capi, n_l=6, n_r=5):
    kl, kr = np.zeros(n_l, capi.KP_DTYPE), np.zeros(n_r, capi.KP_DTYPE)
    kl["octave"] = np.arange(n_l) % cases.N_LEVELS; kr["octave"] = (np.arange(n_r) + 3) % cases.N_LEVELS
    return dict(kps_l=kl, desc_l=np.zeros((n_l, 32), np.uint8), n_l=n_l, mono_l=2, kps_r=kr, desc_r=np.zeros((n_r, 32), np.uint8), n_r=n_r, mono_r=1,
                level_sigma2=cases.LEVEL_SIGMA2.copy(), n_levels=cases.N_LEVELS, rig=cases.RIGS["tumvi"])


def _codes(pkg, capi, a):
    """the check, and the host entry on a NULL handle (so nothing can have run): the two codes and the message of the second"""
    p = lambda v: None if v is None else v.ctypes.data_as(C.c_void_p)
    rig = None if a["rig"] is None else C.byref(capi.fisheye_rig(a["rig"]))
    args = [p(a["kps_l"]), p(a["desc_l"]), a["n_l"], a["mono_l"], p(a["kps_r"]), p(a["desc_r"]), a["n_r"], a["mono_r"], p(a["level_sigma2"]), a["n_levels"], rig]
    chk = pkg.lib.orbm_stereo_fisheye_check(*args)
    run = pkg.lib.orbm_stereo_fisheye(None, *(args + [None] * 7))
    return chk, run, pkg.lib.orbx_last_error()


def _after_the_checks(pkg):
    return ERR_ARG if pkg.device_count() > 0 else ERR_NO_DEVICE           # a NULL handle: "NULL matcher", or no device at all


def test_every_refusal_of_the_check(pkg, capi):
    good = _frame(capi)
    chk, run, msg = _codes(pkg, capi, good)
    assert chk == 0 and run == _after_the_checks(pkg) and (b"NULL matcher" in msg or b"no HIP device" in msg)      # refused as such, after every check has passed
    oct_l, oct_r = good["kps_l"].copy(), good["kps_r"].copy()
    oct_l["octave"][4] = cases.N_LEVELS; oct_r["octave"][0] = -1
    nan = float("nan")
    cam = lambda side, **kw: dict(good["rig"], **{side: dict(good["rig"][side], **kw)})
    bad = {
        "negative n_l": dict(n_l=-1), "negative n_r": dict(n_r=-2), "negative mono_l": dict(mono_l=-1), "negative mono_r": dict(mono_r=-1),
        "mono_l above n_l": dict(mono_l=7), "mono_r above n_r": dict(mono_r=6),
        "left octave out of range": dict(kps_l=oct_l), "right octave negative": dict(kps_r=oct_r),
        "octave beyond a shorter table": dict(n_levels=4),
        "fx left zero": dict(rig=cam("left", fx=0.0)), "fy left negative": dict(rig=cam("left", fy=-190.0)), "fx right nan": dict(rig=cam("right", fx=nan)),
        "fy right zero": dict(rig=cam("right", fy=0.0)),
        "precision_l zero": dict(rig=dict(good["rig"], precision_l=0.0)), "precision_r negative": dict(rig=dict(good["rig"], precision_r=-1e-6)),
        "precision_r nan": dict(rig=dict(good["rig"], precision_r=nan)),
        "kps_l NULL": dict(kps_l=None), "desc_l NULL": dict(desc_l=None), "kps_r NULL": dict(kps_r=None), "desc_r NULL": dict(desc_r=None),
        "level_sigma2 NULL": dict(level_sigma2=None), "rig NULL": dict(rig=None), "no levels": dict(n_levels=0), "too many levels": dict(n_levels=33),
    }
    for name, change in bad.items():
        chk, run, msg = _codes(pkg, capi, dict(good, **change))
        assert chk == ERR_ARG and run == ERR_ARG and msg, name
    # mono == n (no lapping area) and empty sides are fine, and NULL arrays go with an empty side
    for change in (dict(mono_l=6), dict(mono_r=5), dict(n_l=0, mono_l=0, kps_l=None, desc_l=None), dict(n_r=0, mono_r=0, kps_r=None, desc_r=None)):
        assert _codes(pkg, capi, dict(good, **change))[0] == 0
    assert capi.stereo_fisheye_check(good["rig"], None, None, 0, 0, None, None, 0, 0, good["level_sigma2"], cases.N_LEVELS) == 0


def test_device_entry_and_diagnostic_check_before_touching_a_device(pkg, capi):
    sig = cases.LEVEL_SIGMA2.copy()
    p = sig.ctypes.data_as(C.c_void_p)
    rig = capi.fisheye_rig(cases.RIGS["tumvi"])
    bad_rig = capi.fisheye_rig(dict(cases.RIGS["tumvi"], precision_l=0.0))
    one = C.c_void_p(16)            # a non-NULL, aligned address that is never read: every call below is refused by the checks or by the NULL handle
    dev = lambda **kw: pkg.lib.orbm_stereo_fisheye_batch_device(None, kw.get("batch", 1), kw.get("cap", 8), one, kw.get("desc", one), one, one, one, one, one, one,
                                                                kw.get("sig", p), kw.get("levels", cases.N_LEVELS), C.byref(kw.get("rig", rig)),
                                                                kw.get("ltr", one), one, one, one, None, None, None, None)
    assert dev() == _after_the_checks(pkg)
    for kw in (dict(batch=-1), dict(cap=-1), dict(batch=70000), dict(levels=0), dict(sig=None), dict(rig=bad_rig), dict(ltr=None), dict(desc=C.c_void_p(8))):
        assert dev(**kw) == ERR_ARG, kw
    z = np.zeros(4, np.float32)
    q = z.ctypes.data_as(C.c_void_p)
    assert pkg.lib.orbx_kb8_triangulate_matches(0, C.byref(bad_rig), q, q, q, q, 1, q, q) == ERR_ARG
    assert pkg.lib.orbx_kb8_triangulate_matches(0, C.byref(rig), q, q, q, q, -1, q, q) == ERR_ARG
    assert pkg.lib.orbx_kb8_triangulate_matches(0, C.byref(rig), None, q, q, q, 1, q, q) == ERR_ARG
    assert pkg.lib.orbx_kb8_triangulate_matches(0, None, q, q, q, q, 1, q, q) == ERR_ARG


def test_create_without_a_device_fails_loudly(pkg):
    h = C.c_void_p()
    pkg.lib.orbm_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
    pkg.lib.orbm_destroy.argtypes = [C.c_void_p]
    rc = pkg.lib.orbm_create(0, C.byref(h))
    if pkg.device_count() > 0:
        assert rc == 0 and h.value
        pkg.lib.orbm_destroy(h)
    else:
        assert rc == ERR_NO_DEVICE and not h.value and b"no HIP device" in pkg.lib.orbx_last_error()
        with pytest.raises(pkg.OrbxError):
            pkg.Matcher()
        with pytest.raises(pkg.OrbxError):
            pkg.kb8_triangulate_matches(cases.RIGS["tumvi"], np.zeros((1, 2)), np.zeros((1, 2)), np.ones(1), np.ones(1))
