"""The IMU pre-integration additions of the C ABI (include/orbslam3_hip_imu_preint.h, which include/orbslam3_hip.h includes; no GPU):
the functions are declared there and exported, the ctypes mirrors have the layout of the C structs, every refusal of the host-only
argument checks is answered with its code before anything touches a device (imu_preint_check, and the host entries on a NULL
handle), and without a device imu_preint_create fails loudly."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import imu_preint_cases as cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "orbslam3_hip.h")
HEADER_PREINT = os.path.join(ROOT, "include", "orbslam3_hip_imu_preint.h")
EXPECTED = sorted(["imu_preint_create", "imu_preint_destroy", "imu_preint_check", "imu_preint_last_device_ms",
                   "imu_preintegrate_batch", "imu_preintegrate_batch_device", "imu_frame_measurements_batch", "imu_frame_measurements_batch_device",
                   "imu_links_batch", "imu_links_batch_device", "imu_predict_state_batch", "imu_predict_state_batch_device"])
STRUCTS = ("ImuMeasurement", "ImuPreintState", "ImuPreintJob", "ImuLinkSpec", "ImuPredictJob", "ImuPredictOut")
ERR_ARG = -3


@pytest.fixture(scope="module")
def capi(pkg):
    return importlib.import_module("orb_slam3-1_amd.capi")


def test_symbols_declared_and_exported(pkg, capi):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_PREINT).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(imu_[a-z0-9_]+)\s*\(", src))) == EXPECTED
    assert '#include "orbslam3_hip_imu_preint.h"' in open(HEADER).read()
    for n in EXPECTED:
        assert hasattr(pkg.lib, n), "symbol %s declared in include/orbslam3_hip_imu_preint.h is not exported" % n
    assert callable(pkg.ImuPreintegrator.preintegrate) and callable(pkg.ImuPreintegrator.links) and callable(pkg.ImuPreintegrator.predict)
    assert "stays on the host" not in open(HEADER).read()


def test_struct_layout_matches_header(capi):
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbslam3_hip.h"', "int main(void) {"]
    for s in STRUCTS:
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f, _ in getattr(capi, s)._fields_:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    lines.append('printf("LibaLink %zu\\n", sizeof(LibaLink));')
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        seen = dict(l.split() for l in subprocess.check_output([exe], text=True).strip().splitlines())
    for s in STRUCTS:
        cls = getattr(capi, s)
        assert int(seen[s]) == C.sizeof(cls), s
        for f, _ in cls._fields_:
            assert int(seen["%s.%s" % (s, f)]) == getattr(cls, f).offset, "%s.%s" % (s, f)
    for cls, dt in ((capi.ImuMeasurement, capi.IMU_MEAS_DTYPE), (capi.ImuPreintState, capi.IMU_STATE_DTYPE), (capi.ImuPreintJob, capi.IMU_JOB_DTYPE),
                    (capi.ImuLinkSpec, capi.IMU_LINK_SPEC_DTYPE), (capi.ImuPredictJob, capi.IMU_PREDICT_JOB_DTYPE), (capi.ImuPredictOut, capi.IMU_PREDICT_OUT_DTYPE),
                    (capi._LibaLink, capi.LIBA_LINK_DTYPE)):
        assert dt.itemsize == C.sizeof(cls) and [dt.fields[f][1] for f, _ in cls._fields_] == [getattr(cls, f).offset for f, _ in cls._fields_]
    assert int(seen["LibaLink"]) == capi.LIBA_LINK_DTYPE.itemsize and int(seen["ImuPreintState"]) == 1268 and int(seen["ImuMeasurement"]) == 28


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _codes(pkg, states, jobs, meas, n=None):
    """imu_preint_check and imu_preintegrate_batch on a NULL handle (so nothing can have run): the two codes and the message"""
    ns, nj, nm = n or (len(states), len(jobs), len(meas))
    st = np.zeros(max(nj, 1), np.int32)
    a = pkg.lib.imu_preint_check(_p(states), ns, _p(jobs), nj, _p(meas), nm)
    b = pkg.lib.imu_preintegrate_batch(None, _p(states), ns, _p(jobs), nj, _p(meas), nm, _p(st))
    return a, b, pkg.lib.orbx_last_error()


def test_every_refusal_of_the_check(pkg, capi):
    states, jobs, meas = cases.pack(capi, ["n3_a", "n7_a"], extra_states=1)
    a, b, msg = _codes(pkg, states, jobs, meas)
    assert a == 0 and b == ERR_ARG and b"handle is NULL" in msg               # refused as such, after every check has passed

    def refused(text, states=states, jobs=jobs, meas=meas, n=None):
        a, b, msg = _codes(pkg, states, jobs, meas, n)
        assert (a, b) == (ERR_ARG, ERR_ARG) and text.encode() in msg, (text, a, b, msg)

    def job(i, **change):
        j = jobs.copy()
        for k, v in change.items():
            j[k][i] = v
        return j

    sizes = (len(states), len(jobs), len(meas))
    refused("pointer is NULL", states=None, n=sizes)
    refused("pointer is NULL", jobs=None, n=sizes)
    refused("pointer is NULL", meas=None, n=sizes)
    refused("negative size", n=(len(states), -1, len(meas)))
    refused("state 3 out of range", jobs=job(1, state=3))
    refused("state -1 out of range", jobs=job(0, state=-1))
    refused("out of range", jobs=job(1, first=4, count=7))                      # 4 + 7 > 10 measurements
    refused("out of range", jobs=job(0, first=-1))
    refused("out of range", jobs=job(0, count=-1))
    refused("out of range", jobs=job(0, first=2 ** 31 - 1, count=2 ** 31 - 1))  # no overflow of first + count
    refused("state 0 has two writers", jobs=job(1, state=0))
    for field, value in (("a", np.nan), ("w", np.inf), ("dt", np.nan)):
        m = meas.copy()
        if field == "dt":
            m["dt"][5] = value
        else:
            m[field][5, 2] = value
        refused("measurement 5 is not finite", meas=m)
    for value in (0.0, -0.005):
        m = meas.copy()
        m["dt"][9] = value
        refused("measurement 9 has dt <= 0", meas=m)
    bad = jobs.copy()
    bad["bias"][1, 4] = np.nan
    refused("bias is not finite", jobs=bad)
    m = meas.copy()                                                             # a measurement that no job reads is not looked at
    m["dt"][0] = 0.0
    j = jobs.copy()
    j["first"][0], j["count"][0] = 1, 2
    assert _codes(pkg, states, j, m)[0] == 0
    st = np.zeros(2, np.int32)
    assert pkg.lib.imu_preintegrate_batch(None, _p(states), len(states), _p(jobs), len(jobs), _p(meas), len(meas), None) == ERR_ARG


def test_refusals_of_the_other_host_entries(pkg, capi):
    states = capi.imu_state_new(2, cases.NGA, cases.NGA_WALK)
    spec = np.zeros(1, capi.IMU_LINK_SPEC_DTYPE)
    links, st = np.zeros(1, capi.LIBA_LINK_DTYPE), np.zeros(1, np.int32)
    lib = pkg.lib
    assert lib.imu_links_batch(None, _p(states), 2, _p(spec), 1, _p(links), _p(st)) == ERR_ARG and b"handle is NULL" in lib.orbx_last_error()
    for change in (dict(state=2), dict(state=-1), dict(walk_state=2), dict(walk_state=-2)):
        s = spec.copy()
        for k, v in change.items():
            s[k] = v
        assert lib.imu_links_batch(None, _p(states), 2, _p(s), 1, _p(links), _p(st)) == ERR_ARG and b"out of range" in lib.orbx_last_error()
    assert lib.imu_links_batch(None, _p(states), 2, _p(spec), 1, None, _p(st)) == ERR_ARG and b"pointer is NULL" in lib.orbx_last_error()
    assert lib.imu_links_batch(None, None, 2, _p(spec), 1, _p(links), _p(st)) == ERR_ARG
    pj, po = np.zeros(1, capi.IMU_PREDICT_JOB_DTYPE), np.zeros(1, capi.IMU_PREDICT_OUT_DTYPE)
    assert lib.imu_predict_state_batch(None, _p(states), 2, _p(pj), 1, _p(po), _p(st)) == ERR_ARG and b"handle is NULL" in lib.orbx_last_error()
    pj["state"] = 2
    assert lib.imu_predict_state_batch(None, _p(states), 2, _p(pj), 1, _p(po), _p(st)) == ERR_ARG and b"state 2 out of range" in lib.orbx_last_error()
    assert lib.imu_predict_state_batch(None, _p(states), 2, _p(pj), 1, _p(po), None) == ERR_ARG
    smp, n_imu, t = np.zeros((1, 4), capi.IMU_DTYPE), np.array([2], np.int32), np.zeros(1, np.int64)
    meas, cnt = np.zeros((1, 4), capi.IMU_MEAS_DTYPE), np.zeros(1, np.int32)
    assert lib.imu_frame_measurements_batch(None, _p(smp), _p(n_imu), _p(t), _p(t), 1, 4, _p(meas), _p(cnt)) == ERR_ARG and b"handle is NULL" in lib.orbx_last_error()
    for bad in (5, -1):
        assert lib.imu_frame_measurements_batch(None, _p(smp), _p(np.array([bad], np.int32)), _p(t), _p(t), 1, 4, _p(meas), _p(cnt)) == ERR_ARG
        assert b"outside 0 .. 4" in lib.orbx_last_error()
    assert lib.imu_frame_measurements_batch(None, None, _p(n_imu), _p(t), _p(t), 1, 4, _p(meas), _p(cnt)) == ERR_ARG
    assert lib.imu_frame_measurements_batch(None, _p(smp), _p(n_imu), _p(t), _p(t), 1, 0, _p(meas), _p(cnt)) == ERR_ARG
    # the device entries check shapes on the host
    assert lib.imu_preintegrate_batch_device(None, None, 1, None, 1, None, 0, None, None) == ERR_ARG and b"pointer is NULL" in lib.orbx_last_error()
    assert lib.imu_links_batch_device(None, None, 1, None, 1, None, None, None) == ERR_ARG
    assert lib.imu_predict_state_batch_device(None, None, 1, None, 1, None, None, None) == ERR_ARG
    assert lib.imu_frame_measurements_batch_device(None, None, None, None, None, 1, 4, None, None, None) == ERR_ARG


def test_create_without_a_device_fails_loudly(pkg):
    h = C.c_void_p()
    rc = pkg.lib.imu_preint_create(0, C.byref(h))
    if pkg.device_count() > 0:
        assert rc == 0 and h.value
        pkg.lib.imu_preint_destroy(h)
    else:
        assert rc == -4 and not h.value and b"no HIP device" in pkg.lib.orbx_last_error()
        with pytest.raises(pkg.OrbxError):
            pkg.ImuPreintegrator()
    assert pkg.lib.imu_preint_create(0, None) == ERR_ARG
