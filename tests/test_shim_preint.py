"""The pre-integration adapter (include/orbslam3_shim_preint.hpp: PreintegrateIMUHIP, ReintegrateHIP, preint_detail::to_state /
from_state) against the stand-in of tests/stubs/standin_imu_preint.hpp.  Without a GPU: it compiles against the stand-ins with
-Wall -Wextra -Werror, and to_state / from_state carry every member of the stand-in there and back (tests/stubs/shim_preint_toy.cpp).
On the GPU: ReintegrateHIP on one object per case of tests/imu_preint_cases.py (one call for all of them) and PreintegrateIMUHIP on
a frame of 8 samples are held to truth by the bounds of tests/test_imu_preint_gpu.py; the interpolated measurements equal the float32
restatement bit for bit."""
import os
import subprocess

import numpy as np
import pytest

import imu_preint_cases as cases
import imu_preint_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "orb_slam3-1_amd")
NAMES = list(cases.CASES)
MEMBERS = ["dT", "C", "Nga", "NgaWalk", "b", "bu", "dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "avgA", "avgW"]
FIELDS = (("dT", 1), ("b", 6), ("bu", 6), ("nga", 6), ("nga_walk", 6), ("dR", 9), ("dV", 3), ("dP", 3), ("JRg", 9), ("JVg", 9), ("JVa", 9), ("JPg", 9),
          ("JPa", 9), ("avgA", 3), ("avgW", 3), ("C", 225))


def test_preint_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_imu_preint.hpp"\n#include "orbslam3_shim_preint.hpp"\n'
                   "using namespace ORB_SLAM3;\n"
                   "int main() { IMU::PiPreintegrated a, b; std::vector<IMU::PiPoint> v; std::vector<IMU::PiPreintegrated*> w;\n"
                   "             return PreintegrateIMUHIP(v, 0.0, 1.0, &a, &b) && ReintegrateHIP(w) ? 0 : 1; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory, pkg):
    exe = tmp_path_factory.mktemp("shim_preint") / "shim_preint_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_preint_toy.cpp"),
                           "-o", str(exe), "-L", LIBDIR, "-lorbslam3_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def test_to_state_from_state_round_trip_every_member(toy):
    lines = [l.split() for l in subprocess.check_output([toy, "roundtrip"], text=True).splitlines()]
    assert ["layout", "1"] in lines and ["n_meas", "5"] in lines and ["cleared", "1"] in lines
    assert [l[1] for l in lines if l[0] == "member"] == MEMBERS and all(l[2] == "1" for l in lines if l[0] == "member")
    assert [l[1:] for l in lines if l[0] == "kept"] == [["Info", "1"], ["db", "1"], ["mvMeasurements", "1"]]


def _fl(a):
    return " ".join(repr(float(x)) for x in np.asarray(a, np.float64).ravel())


def _parse(out):
    objs, meas = {}, {}
    for ln in out.splitlines():
        f = ln.split()
        if f[0] in ("object", "kf", "frame"):
            v = np.array([float.fromhex(x) for x in f[2:2 + 316]], np.float64)
            s, at = {}, 0
            for k, n in FIELDS:
                s[k] = v[at:at + n].astype(np.float32)
                at += n
            for k in ("dR", "JRg", "JVg", "JVa", "JPg", "JPa"):
                s[k] = s[k].reshape(3, 3)
            s["C"] = s["C"].reshape(15, 15)
            s["dT"] = s["dT"][0]
            s.update(n_meas=int(f[318]), info=float.fromhex(f[319]), db=float.fromhex(f[320]))
            objs[(f[0], int(f[1]))] = s
        elif f[0] == "meas":
            meas.setdefault((f[1], int(f[2])), []).append([float.fromhex(x) for x in f[3:10]])
    return objs, {k: np.array(v, np.float32) for k, v in meas.items()}


@pytest.mark.gpu
def test_reintegrate_hip_within_budget(toy, tmp_path):
    lines = ["%d" % len(NAMES)]
    for name in NAMES:
        c = cases.make_case(name)
        lines += ["%s %s %s %d" % (_fl(c["bias"]), _fl(c["nga"]), _fl(c["nga_walk"]), c["n"])]
        lines += ["%s %s %s" % (_fl(c["a"][i]), _fl(c["w"][i]), _fl(c["dt"][i])) for i in range(c["n"])]
    path = tmp_path / "objects.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([toy, "reintegrate", str(path)], text=True)
    assert out.splitlines()[0] == "accepted 1"
    objs, meas = _parse(out)
    for i, name in enumerate(NAMES):
        c, s = cases.make_case(name), objs[("object", i)]
        cases.check_against_truth(name, ref.blocks(s), ref.BLOCKS, "adapter")
        assert ref.zero_blocks_are_zero(s["C"]) and np.array_equal(s["b"], c["bias"]) and np.array_equal(s["bu"], c["bias"])
        assert np.array_equal(s["nga"], c["nga"]) and np.array_equal(s["nga_walk"], c["nga_walk"])
        assert s["n_meas"] == c["n"] and s["info"] == 0 and s["db"] == 0                  # Initialize() clears Info and db; the list is kept
        assert np.array_equal(meas[("object", i)], np.c_[c["a"], c["w"], c["dt"]])


@pytest.mark.gpu
def test_preintegrate_imu_hip_within_budget(toy, tmp_path):
    rng = np.random.default_rng(11)
    n = 8
    t = 1403636579.763555 + np.cumsum(0.005 + rng.normal(0, 2e-5, n))
    t_prev, t_cur = t[0] + 0.0012, t[-1] - 0.0023
    acce = (np.array([0.3, -0.2, 9.79]) + rng.normal(0, 1.5, (n, 3))).astype(np.float32)
    gyro = rng.normal(0, 0.4, (n, 3)).astype(np.float32)
    b_kf, b_fr = (rng.normal(0, 0.03, 6)).astype(np.float32), (rng.normal(0, 0.03, 6)).astype(np.float32)
    lines = [_fl(b_kf), _fl(b_fr), _fl(cases.NGA) + " " + _fl(cases.NGA_WALK), "%r %r %d" % (float(t_prev), float(t_cur), n)]
    lines += ["%r %s %s" % (float(t[i]), _fl(acce[i]), _fl(gyro[i])) for i in range(n)]
    path = tmp_path / "frame.txt"
    path.write_text("\n".join(lines) + "\n")
    out = subprocess.check_output([toy, "frame", str(path)], text=True)
    assert out.splitlines()[0] == "accepted 1"
    objs, meas = _parse(out)
    a, w, dt = ref.frame_measurements_seconds(t, gyro, acce, t_prev, t_cur)
    assert len(dt) == 7 and (dt > 0).all()
    want = np.c_[a, w, dt]
    assert meas[("kf", 0)].tobytes() == want.tobytes() and meas[("frame", 0)].tobytes() == want.tobytes()     # the frame's stale list was cleared
    d = cases.reference_data()
    for tag, bias in (("kf", b_kf), ("frame", b_fr)):
        c = dict(a=a, w=w, dt=dt, bias=bias, nga=cases.NGA, nga_walk=cases.NGA_WALK)
        truth = ref.blocks(ref.truth(c))
        s = ref.blocks(objs[(tag, 0)])
        for k in ref.BLOCKS:
            # the budget of length 7, this case -- a case of that length -- included
            budget = max([d["budget"][7][k]] + [ref.block_error(ref.blocks(ref.integrate(c, np.float32, **opt))[k], truth[k]) for opt in ref.VARIANTS.values()])
            e = ref.block_error(s[k], truth[k])
            print("%-6s %-6s adapter %.2e  budget %.2e  bound %.2e" % (tag, k, e, budget, cases.bound(budget)))
            assert e <= cases.bound(budget), (tag, k, e, budget)
        assert objs[(tag, 0)]["n_meas"] == 7 and np.array_equal(objs[(tag, 0)]["b"], bias)
    assert objs[("frame", 0)]["info"] == 0 and objs[("frame", 0)]["db"] == 0
