"""The IMU-initialisation additions of the C ABI (include/orbslam3_hip_imu_init.h, which include/orbslam3_hip.h includes; no GPU):
the functions are declared there and exported, the ctypes mirrors have the layout of the C structs, every argument check of
imu_init_optimize_batch answers with its code and message before anything touches a device, and without a device imu_init_create
fails loudly."""
import ctypes as C
import importlib
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "orbslam3_hip.h")
HEADER_IMU_INIT = os.path.join(ROOT, "include", "orbslam3_hip_imu_init.h")
EXPECTED = ["imu_init_check", "imu_init_create", "imu_init_destroy", "imu_init_last_device_ms", "imu_init_optimize_batch"]


@pytest.fixture(scope="module")
def capi(pkg):
    return importlib.import_module("orb_slam3-1_amd.capi")


@pytest.fixture(scope="module")
def sy(pkg):
    return importlib.import_module("orb_slam3-1_amd.synth_imuinit")


def test_symbols_declared_and_exported(pkg, capi):
    src = re.sub(r"/\*.*?\*/", "", open(HEADER_IMU_INIT).read(), flags=re.S)
    assert sorted(set(re.findall(r"\b(imu_init_[a-z0-9_]+)\s*\(", src))) == EXPECTED
    assert '#include "orbslam3_hip_imu_init.h"' in open(HEADER).read()
    for n in EXPECTED:
        assert hasattr(pkg.lib, n), "symbol %s declared in include/orbslam3_hip_imu_init.h is not exported" % n
    assert callable(pkg.ImuInit.optimize) and callable(pkg.ImuInit.optimize_batch)
    assert (capi.IMU_INIT_MAX_KF, capi.IMU_INIT_MAX_BATCH) == (256, 64)
    assert "#define IMU_INIT_MAX_KF 256" in src and "#define IMU_INIT_MAX_BATCH 64" in src


def test_struct_layout_matches_header(capi):
    structs = {"ImuInitProblem": ["n_kf", "Rwb", "twb", "vel", "bg", "ba", "Rwg", "scale", "n_links", "links", "free_vel", "free_bias", "free_gdir",
                                  "free_scale", "prior_g", "prior_a", "huber_delta", "gauss_newton", "lambda_init", "max_iters"],
               "ImuInitResult": ["vel_out", "bg_out", "ba_out", "Rwg_out", "scale_out", "chi2_initial", "chi2_final", "stats"]}
    lines = ['#include <stddef.h>', '#include <stdio.h>', '#include "orbslam3_hip.h"', "int main(void) {"]
    for s, fields in structs.items():
        lines.append('printf("%s %%zu\\n", sizeof(%s));' % (s, s))
        for f in fields:
            lines.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (s, f, s, f))
    lines.append('printf("LibaLink %zu\\n", sizeof(LibaLink));')
    lines.append("return 0; }")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.c"), os.path.join(d, "layout")
        open(src, "w").write("\n".join(lines))
        subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", exe, src])
        out = subprocess.check_output([exe], text=True)
    seen = dict(l.split() for l in out.strip().splitlines())
    for s, fields in structs.items():
        cls = getattr(capi, s)
        assert [f for f, _ in cls._fields_] == fields
        assert int(seen[s]) == C.sizeof(cls), s
        for f in fields:
            assert int(seen["%s.%s" % (s, f)]) == getattr(cls, f).offset, "%s.%s" % (s, f)
    assert int(seen["LibaLink"]) == C.sizeof(capi._LibaLink)


def _problem(sy, **kw):
    return sy.make_imu_init(5, 12, **kw)[0]


def _both(pkg, prep, n=1):
    """imu_init_check and imu_init_optimize_batch on a NULL handle (so nothing can have run): the two codes"""
    a = pkg.lib.imu_init_check(prep["problems"], prep["results"])
    msg = pkg.lib.orbx_last_error()
    b = pkg.lib.imu_init_optimize_batch(None, prep["problems"], n, prep["results"])
    return a, b, msg, pkg.lib.orbx_last_error()


def test_check_accepts_good_problems(pkg, capi, sy):
    for kw in (dict(), dict(variant="scale_refine"), dict(variant="bias"), dict(variant="fixed_vel"), dict(n_paths=3, n_isolated=2, shuffle=True)):
        prep = capi.imu_init_prepare([_problem(sy, **kw)])
        assert pkg.lib.imu_init_check(prep["problems"], prep["results"]) == 0, kw
    empty = dict(_problem(sy), links=[])               # zero links: valid, the inputs come back
    prep = capi.imu_init_prepare([empty])
    assert prep["problems"][0].links is None and pkg.lib.imu_init_check(prep["problems"], prep["results"]) == 0


def test_every_argument_check(pkg, capi, sy):
    """each refusal of the header with the message that names it"""
    good = capi.imu_init_prepare([_problem(sy)])
    assert pkg.lib.imu_init_check(None, good["results"]) == -3 and b"NULL" in pkg.lib.orbx_last_error()
    assert pkg.lib.imu_init_check(good["problems"], None) == -3 and b"NULL" in pkg.lib.orbx_last_error()
    assert pkg.lib.imu_init_optimize_batch(None, None, 1, good["results"]) == -3 and b"NULL" in pkg.lib.orbx_last_error()
    assert pkg.lib.imu_init_optimize_batch(None, good["problems"], 1, None) == -3 and b"NULL" in pkg.lib.orbx_last_error()
    # valid arguments and no handle: refused as such, after every check of the problem has passed
    assert pkg.lib.imu_init_optimize_batch(None, good["problems"], 1, good["results"]) == -3 and b"solver is NULL" in pkg.lib.orbx_last_error()

    def refused(change, text, code=-3, **kw):
        prep = capi.imu_init_prepare([_problem(sy, **kw)])
        change(prep["problems"][0], prep["results"][0], prep["arrays"][0])
        a, b, m1, m2 = _both(pkg, prep)
        assert (a, b) == (code, code), (text, a, b)
        assert text.encode() in m1 and text.encode() in m2, (text, m1, m2)

    def link(k, field, value):
        return lambda p, r, a: setattr(a["links"][k], field, value)

    for f in ("Rwb", "twb", "vel"):
        refused(lambda p, r, a, f=f: setattr(p, f, None), "Rwb, twb or vel is NULL")
    refused(lambda p, r, a: setattr(r, "vel_out", None), "vel_out is NULL")
    refused(lambda p, r, a: setattr(p, "links", None), "links is NULL")
    refused(lambda p, r, a: setattr(p, "n_kf", -1), "negative size")
    refused(lambda p, r, a: setattr(p, "n_links", -1), "negative size")
    refused(link(4, "kf2", 12), "key-frame index out of range")
    refused(link(4, "kf1", -1), "key-frame index out of range")
    refused(link(4, "kf2", 4), "kf1 == kf2")                                    # link 4 is 4 -> 5
    refused(link(6, "kf1", 2), "kf1 of more than one link")                     # 2 -> 3 exists
    refused(link(6, "kf2", 3), "kf2 of more than one link")
    refused(link(10, "kf2", 0), "cycle")                                        # 10 -> 11 becomes 10 -> 0: 0 -> 1 -> ... -> 10 -> 0
    refused(lambda p, r, a: setattr(p, "scale", 0.0), "scale is not finite and positive")
    refused(lambda p, r, a: setattr(p, "scale", -1.0), "scale is not finite and positive")
    refused(lambda p, r, a: setattr(p, "scale", float("inf")), "scale is not finite and positive")
    refused(lambda p, r, a: setattr(p, "scale", float("nan")), "scale is not finite and positive")
    refused(lambda p, r, a: p.bg.__setitem__(1, float("nan")), "bg, ba or Rwg is not finite")
    refused(lambda p, r, a: p.Rwg.__setitem__(8, float("inf")), "bg, ba or Rwg is not finite")
    for k in ("Rwb", "twb", "vel"):
        refused(lambda p, r, a, k=k: a[k].__setitem__((5, 2), np.nan), "key-frame value is not finite")
    for f in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bias0", "info9"):
        refused(lambda p, r, a, f=f: getattr(a["links"][7], f).__setitem__(2, float("nan")), "a value of link 7 is not finite")
    refused(link(7, "dT", float("inf")), "a value of link 7 is not finite")
    refused(lambda p, r, a: setattr(p, "huber_delta", float("nan")), "huber_delta is not finite")      # also without a robust link
    refused(lambda p, r, a: setattr(p, "lambda_init", -1.0), "lambda_init")
    refused(lambda p, r, a: setattr(p, "lambda_init", float("nan")), "lambda_init")
    refused(lambda p, r, a: setattr(p, "max_iters", -1), "max_iters")
    refused(lambda p, r, a: setattr(p, "max_iters", 1001), "max_iters")
    refused(lambda p, r, a: setattr(p, "gauss_newton", 2), "gauss_newton")
    refused(lambda p, r, a: setattr(p, "prior_g", -1.0), "prior is negative")
    refused(lambda p, r, a: setattr(p, "prior_a", float("nan")), "prior is negative")
    refused(lambda p, r, a: [setattr(p, f, 0) for f in ("free_vel", "free_bias", "free_gdir", "free_scale")], "nothing is free")
    refused(lambda p, r, a: setattr(p, "huber_delta", 0.0), "huber_delta", variant="scale_refine")
    refused(lambda p, r, a: setattr(p, "n_kf", 257), "capacity", code=-2)


def test_capacity_and_batch_size(pkg, capi, sy):
    pr = sy.make_imu_init(1, 256, variant="bias")[0]
    prep = capi.imu_init_prepare([pr])
    assert pkg.lib.imu_init_check(prep["problems"], prep["results"]) == 0        # exactly the capacity
    pr = sy.make_imu_init(1, 257, variant="bias")[0]
    prep = capi.imu_init_prepare([pr])
    assert _both(pkg, prep)[:2] == (-2, -2) and b"257 key frames" in pkg.lib.orbx_last_error()
    small = capi.imu_init_prepare([sy.make_imu_init(2, 3)[0]] * 65)
    assert pkg.lib.imu_init_optimize_batch(None, small["problems"], 65, small["results"]) == -3 and b"n_problems 65" in pkg.lib.orbx_last_error()
    assert pkg.lib.imu_init_optimize_batch(None, small["problems"], 0, small["results"]) == -3 and b"n_problems 0" in pkg.lib.orbx_last_error()
    bad = [sy.make_imu_init(2, 3)[0] for _ in range(3)]
    bad[2]["scale"] = -1.0                          # the message names the problem of a batch
    prep = capi.imu_init_prepare(bad)
    assert pkg.lib.imu_init_optimize_batch(None, prep["problems"], 3, prep["results"]) == -3 and b"problem 2" in pkg.lib.orbx_last_error()


def test_create_without_a_device_fails_loudly(pkg):
    h = C.c_void_p()
    rc = pkg.lib.imu_init_create(0, C.byref(h))
    if pkg.device_count() > 0:
        assert rc == 0 and h.value
        pkg.lib.imu_init_destroy(h)
    else:
        assert rc == -4 and not h.value and b"no HIP device" in pkg.lib.orbx_last_error()
        with pytest.raises(pkg.OrbxError):
            pkg.ImuInit()
    assert pkg.lib.imu_init_create(0, None) == -3


def test_generator_is_seeded_and_consistent(sy):
    a, b, c = sy.make_imu_init(5, 12)[0], sy.make_imu_init(5, 12)[0], sy.make_imu_init(6, 12)[0]
    for k in ("Rwb", "twb", "vel", "Rwg"):
        assert np.array_equal(a[k], b[k]), k
    assert not np.array_equal(a["twb"], c["twb"])
    assert [(l["kf1"], l["kf2"]) for l in a["links"]] == [(i, i + 1) for i in range(11)]
    m, gt = sy.make_imu_init(7, 130, n_paths=3, n_isolated=2, shuffle=True)
    k1, k2 = [l["kf1"] for l in m["links"]], [l["kf2"] for l in m["links"]]
    assert len(m["links"]) == 130 - 2 - 3 and len(set(k1)) == len(k1) and len(set(k2)) == len(k2)
    assert len(set(range(130)) - set(k1) - set(k2)) == 2                         # the isolated key frames
    assert [(l["kf1"], l["kf2"]) for l in m["links"]] != sorted((l["kf1"], l["kf2"]) for l in m["links"])
