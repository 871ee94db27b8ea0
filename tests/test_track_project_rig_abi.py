"""The rig projection part of the C ABI (include/orbslam3_hip_track_project_rig.h, a header of its own that nothing includes; no GPU):
the functions are declared there and exported, the ctypes mirrors have the layout of the C structs, OrbmRigFrustumOut / OrbmRigLastProjOut
carry the fields of OrbmRigMapPoints / OrbmRigLastPoints under the same names and types, the host-only check refuses what the header
says it refuses, and every entry makes its checks before it touches a handle or a device."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "orbslam3_hip_track_project_rig.h")
EXPECTED = sorted(["orbm_rig_frame_pose_batch_device", "orbm_frustum_rig_batch_device", "orbm_project_last_rig_batch_device",
                   "orbm_unproject_stereo_fisheye_batch_device", "orbm_frustum_rig_batch", "orbm_project_last_rig_batch", "orbm_unproject_stereo_fisheye_batch",
                   "orbm_track_project_rig_check", "orbm_track_project_rig_last_kernel_ms"])
ERR_CAPACITY, ERR_ARG = -2, -3
STRUCTS = dict(OrbmTrackRigCamera="TrackRigCamera", OrbmRigFramePose="RigFramePose", OrbmRigFrustumOut="RigFrustumOut", OrbmRigLastProjOut="RigLastProjOut")
IN_OUT = ("proj_u", "proj_v", "view_cos", "track_depth", "proj_u_r", "proj_v_r", "view_cos_r", "track_depth_r")


@pytest.fixture(scope="module")
def capi(pkg):
    return importlib.import_module("orb_slam3-1_amd.capi")


def test_symbols_declared_and_exported(pkg, capi):
    text = open(HEADER).read()
    src = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    assert sorted(set(re.findall(r"\b(orbm_[a-z0-9_]+)\s*\(", src))) == EXPECTED
    for n in EXPECTED:
        assert hasattr(pkg.lib, n), "symbol %s declared in include/orbslam3_hip_track_project_rig.h is not exported" % n
    for n in ("rig_frame_pose_batch_device", "frustum_rig_batch_device", "project_last_rig_batch_device", "unproject_stereo_fisheye_batch_device", "frustum_rig_batch",
              "project_last_rig_batch", "unproject_stereo_fisheye_batch", "track_project_rig_last_kernel_ms"):
        assert callable(getattr(pkg.Matcher, n)), n
    # a header of its own: no other header includes it (the adapter does), and the hand-over entry is used as it is, not redeclared
    for f in os.listdir(os.path.join(ROOT, "include")):
        if f != os.path.basename(HEADER) and f != "orbslam3_shim_track_project_rig.hpp":
            assert "orbslam3_hip_track_project_rig.h" not in open(os.path.join(ROOT, "include", f)).read(), f
    assert "orbm_track_handover_batch_device" in text and "orbm_track_handover_batch_device" not in src


def test_struct_layouts_match_header(capi):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbslam3_hip_track_project_rig.h"', "int main(void) {"]
    for s, py in STRUCTS.items():
        lines.append('printf("%s.size %%zu\\n", sizeof(%s));' % (s, s))
        for f, _ in getattr(capi, py)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    # the pinhole header came along: its types and limits are visible
    lines.append('printf("max_batch %d\\nmax_levels %d\\npose %zu\\n", ORBM_TRACK_MAX_BATCH, ORBM_TRACK_MAX_LEVELS, sizeof(OrbmFramePose));')
    # the outputs are the search's inputs: same names, and types that convert without a cast
    lines.append("OrbmRigFrustumOut o = {0}; OrbmRigLastProjOut l = {0}; OrbmRigMapPoints mp; OrbmRigLastPoints lp;")
    for f in ("in_view", "proj_u", "proj_v", "pred_level", "view_cos", "in_view_r", "proj_u_r", "proj_v_r", "pred_level_r", "view_cos_r", "track_depth"):
        lines.append("mp.%s = o.%s;" % (f, f))
    for f in ("valid", "proj_u", "proj_v", "proj_u_r", "proj_v_r"):
        lines.append("lp.%s = l.%s;" % (f, f))
    lines.append("(void)mp; (void)lp; return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        seen = dict(l.split() for l in subprocess.check_output([exe], text=True).strip().splitlines())
    for s, py in STRUCTS.items():
        cls = getattr(capi, py)
        assert int(seen[s + ".size"]) == C.sizeof(cls), s
        for f, _ in cls._fields_:
            assert int(seen["%s.%s" % (s, f)]) == getattr(cls, f).offset, (s, f)
    assert C.sizeof(capi.RigFramePose) == 43 * 4 and C.sizeof(capi.TrackRigCamera) == 41 * 4     # the records the tests move around as float32 arrays
    assert int(seen["max_batch"]) == capi.TRACK_MAX_BATCH and int(seen["max_levels"]) == capi.TRACK_MAX_LEVELS and int(seen["pose"]) == 19 * 4


def _args(capi, **change):
    cam = capi.TrackRigCamera()
    cam.n_levels = 8
    pts = capi.LocalPoints(*([8] * 7), 100)             # (pointers are only compared with NULL)
    out = capi.RigFrustumOut(*([8] * 13))
    a = dict(cam=cam, poses=8, pts=pts, out=out, batch=4)
    for k, v in change.items():
        if "." in k:
            s, f = k.split(".")
            setattr(a[s], f, v)
        else:
            a[k] = v
    return a["cam"], a["poses"], a["pts"], a["out"], a["batch"]


def test_every_refusal_of_the_check(pkg, capi):
    chk = lambda **kw: capi.track_project_rig_check(*_args(capi, **kw))
    assert chk() == 0
    assert chk(**{"cam.n_levels": 1}) == 0 and chk(**{"cam.n_levels": capi.TRACK_MAX_LEVELS}) == 0
    assert chk(batch=1) == 0 and chk(batch=capi.TRACK_MAX_BATCH) == 0 and chk(**{"pts.pcap": 1}) == 0
    bad = {"cam NULL": dict(cam=None), "poses NULL": dict(poses=None), "pts NULL": dict(pts=None), "out NULL": dict(out=None),
           "pcap 0": {"pts.pcap": 0}, "pcap -1": {"pts.pcap": -1}, "no levels": {"cam.n_levels": 0}, "17 levels": {"cam.n_levels": capi.TRACK_MAX_LEVELS + 1},
           "batch 0": dict(batch=0), "batch -1": dict(batch=-1)}
    for f, _ in capi.LocalPoints._fields_[:7]:
        bad["pts.%s NULL" % f] = {"pts." + f: None}
    for f, _ in capi.RigFrustumOut._fields_:
        bad["out.%s NULL" % f] = {"out." + f: None}
    assert all("out.%s NULL" % f in bad for f in IN_OUT)             # a NULL in/out array is refused like a NULL output
    for name, change in bad.items():
        assert chk(**change) == ERR_ARG and pkg.lib.orbx_last_error(), name
    assert chk(batch=capi.TRACK_MAX_BATCH + 1) == ERR_CAPACITY and pkg.lib.orbx_last_error()


def test_entries_check_before_they_touch_the_handle(pkg, capi):
    lib = pkg.lib
    P, I = C.c_void_p, C.c_int
    lib.orbm_frustum_rig_batch_device.argtypes = [P, P, P, P, C.c_float, P, I, P]
    lib.orbm_frustum_rig_batch.argtypes = [P, P, P, P, C.c_float, P, I]
    lib.orbm_project_last_rig_batch_device.argtypes = [P, P, P, P, P, P, I, P, I, P]
    lib.orbm_project_last_rig_batch.argtypes = [P, P, P, P, P, P, I, P, I]
    lib.orbm_rig_frame_pose_batch_device.argtypes = [P, P, P, I, I, P, P]
    lib.orbm_unproject_stereo_fisheye_batch_device.argtypes = [P, P, P, P, P, I, P, I, P]
    lib.orbm_unproject_stereo_fisheye_batch.argtypes = [P, P, P, P, P, I, P, I]
    lib.orbm_track_project_rig_last_kernel_ms.restype = C.c_float
    lib.orbm_track_project_rig_last_kernel_ms.argtypes = [P]
    fake = C.c_void_p(8)                                # a handle that is no handle: the checks come before it is read
    cam, poses, pts, out, batch = _args(capi)
    assert lib.orbm_frustum_rig_batch_device(None, C.byref(cam), poses, C.byref(pts), 0.5, C.byref(out), batch, None) == ERR_ARG
    assert lib.orbm_frustum_rig_batch(None, C.byref(cam), poses, C.byref(pts), 0.5, C.byref(out), batch) == ERR_ARG
    cam17 = _args(capi, **{"cam.n_levels": 17})[0]
    assert lib.orbm_frustum_rig_batch_device(fake, C.byref(cam17), poses, C.byref(pts), 0.5, C.byref(out), batch, None) == ERR_ARG
    assert lib.orbm_frustum_rig_batch(fake, C.byref(cam), poses, C.byref(pts), 0.5, C.byref(out), capi.TRACK_MAX_BATCH + 1) == ERR_CAPACITY
    stale = _args(capi, **{"out.track_depth": None})[3]
    assert lib.orbm_frustum_rig_batch_device(fake, C.byref(cam), poses, C.byref(pts), 0.5, C.byref(stale), batch, None) == ERR_ARG
    lo = capi.RigLastProjOut(8, 8, 8, 8, 8)
    assert lib.orbm_project_last_rig_batch_device(fake, C.byref(cam), 8, 8, 8, 8, 0, C.byref(lo), 2, None) == ERR_ARG          # cap 0
    assert lib.orbm_project_last_rig_batch_device(fake, C.byref(cam), 8, 8, None, 8, 10, C.byref(lo), 2, None) == ERR_ARG      # has_point NULL
    assert lib.orbm_project_last_rig_batch(fake, C.byref(cam17), 8, 8, 8, 8, 10, C.byref(lo), 2) == ERR_ARG
    assert lib.orbm_project_last_rig_batch(fake, C.byref(cam), 8, 8, 8, 8, 10, C.byref(capi.RigLastProjOut(8, 8, 8, None, 8)), 2) == ERR_ARG
    assert lib.orbm_rig_frame_pose_batch_device(fake, None, 8, 2, 1, 8, None) == ERR_ARG
    assert lib.orbm_rig_frame_pose_batch_device(fake, C.byref(cam), None, 2, 1, 8, None) == ERR_ARG
    assert lib.orbm_rig_frame_pose_batch_device(fake, C.byref(cam), 8, 0, 1, 8, None) == ERR_ARG
    assert lib.orbm_rig_frame_pose_batch_device(fake, C.byref(cam), 8, capi.TRACK_MAX_BATCH + 1, 1, 8, None) == ERR_CAPACITY
    assert lib.orbm_unproject_stereo_fisheye_batch_device(fake, 8, 8, 8, 8, 0, 8, 2, None) == ERR_ARG                          # cap 0
    assert lib.orbm_unproject_stereo_fisheye_batch_device(fake, 8, 8, None, 8, 10, 8, 2, None) == ERR_ARG                      # valid NULL
    assert lib.orbm_unproject_stereo_fisheye_batch(fake, 8, 8, 8, 8, 10, 8, capi.TRACK_MAX_BATCH + 1) == ERR_CAPACITY
    assert lib.orbm_unproject_stereo_fisheye_batch(None, 8, 8, 8, 8, 10, 8, 2) == ERR_ARG
    assert lib.orbm_track_project_rig_last_kernel_ms(None) == 0.0
