"""The FullInertialBA adapter (include/orbslam3_shim_fullba.hpp: FullInertialBAHIP with the reference's signature) against the
stand-in types of tests/stubs/: it compiles against them with -Wall -Wextra -Werror, and on a toy map (tests/stubs/shim_fullba_toy.cpp,
with a recording fake of fiba_solve) the problem it hands over -- which key frames get a slot and which are fixed, which links exist
and in what order, what SetNewBias did, the informations without the factor 1e-2, the shared bias of the last key frame visited, the
edges and which points have only fixed observers -- equals an independent restatement of the walk of src/Optimizer.cc:394-719 in Python;
both write-back branches (:730-808) write what the fake returned; a raised stop flag and fewer than three non-fixed key frames return
without a call and without a write; a second camera reaches the reference class.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "orb_slam3-1_amd")
F32 = np.float32
MAX_ID = 6
ORDER = [3, 0, 5, 1, 7, 4, 2, 6]                       # GetAllKeyFrames(), deliberately not in id order
PREV = {1: 0, 2: 1, 3: 2, 4: 3, 5: 4, 7: 5, 6: 7}       # mPrevKF


def test_fullba_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_fullba.hpp"\n#include "orbslam3_shim_fullba.hpp"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory, pkg):
    exe = tmp_path_factory.mktemp("shim_fullba") / "shim_fullba_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_fullba_toy.cpp"),
                           "-o", str(exe), "-L", LIBDIR, "-lorbslam3_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def _rot(rs):
    q, _ = np.linalg.qr(rs.normal(size=(3, 3)))
    return q * np.sign(np.linalg.det(q))


def make_map(seed=4, camera2=False, mostly_fixed=False):
    """Ids 0..7 with the chain 0 <- 1 <- 2 <- 3 <- 4 <- 5 <- 7 <- 6.  Key frame 7 is above maxKFid = 6: no vertex, and its successor 6 has
    no link.  Key frame 4 is bad: its own link is skipped, the link 4 -> 5 stays, and it is still a vertex that is written back.  Key
    frame 2 has no IMU: the links 1 -> 2 and 2 -> 3 do not exist.  That leaves the links 4 -> 5 and 0 -> 1, in GetAllKeyFrames() order of
    their second key frame.  Under bFixLocal (maxKFid - 1 = 5) key frame 0 is fixed through mnBAFixedForKF, key frame 1 through
    mnBALocalForKF; mostly_fixed fixes all but 3 and 5."""
    rs = np.random.RandomState(seed)
    kfs = []
    for i in ORDER:
        kf = dict(id=i, bad=int(i == 4), prev=PREV.get(i, -1), imu=int(i != 2), cam2=int(camera2 and i == 5), bal=5 if i == 1 else 0, baf=6 if i == 0 else 0,
                  Rwb=_rot(rs).astype(F32), twb=rs.normal(0, 2, 3).astype(F32), vel=rs.normal(0, 1, 3).astype(F32), bias=rs.normal(0, 0.02, 6).astype(F32),
                  keys=[(float(F32(rs.uniform(0, 640))), float(F32(rs.uniform(0, 480))), int(rs.randint(0, 3)), float(F32(rs.uniform(0, 600))) if j % 2 else -1.0) for j in range(3)])
        if mostly_fixed and i not in (3, 5):
            kf["bal"] = 6
        if kf["prev"] >= 0:
            A = rs.normal(size=(15, 15))
            kf["pre"] = dict(dT=F32(0.2 + 0.01 * i), dR=_rot(rs).astype(F32), dV=rs.normal(0, 1, 3).astype(F32), dP=rs.normal(0, 1, 3).astype(F32),
                             JRg=rs.normal(0, .1, (3, 3)).astype(F32), JVg=rs.normal(0, .1, (3, 3)).astype(F32), JVa=rs.normal(0, .1, (3, 3)).astype(F32),
                             JPg=rs.normal(0, .1, (3, 3)).astype(F32), JPa=rs.normal(0, .1, (3, 3)).astype(F32), b=rs.normal(0, 0.02, 6).astype(F32),
                             C=(A @ A.T * 1e-6 + np.eye(15) * 1e-5).astype(F32))
        kfs.append(kf)
    # point 0: key frames 0 (mono) and 1 (stereo), both fixed under bFixLocal; 1: key frames 3, 7 (above maxKFid) and 4 (bad); 2: one observation
    # without a left index, so no edge at all; 3: the key frame without IMU
    mps = [dict(id=10 + k, X=rs.normal(0, 3, 3).astype(F32), obs=o) for k, o in enumerate([[(0, 0), (1, 1)], [(3, 2), (7, 0), (4, 1)], [(5, -1)], [(2, 0), (6, 1)]])]
    return dict(kfs=kfs, mps=mps)


def write_case(path, m):
    fl = lambda a: " ".join(repr(float(x)) for x in np.asarray(a, np.float64).ravel())
    lines = ["%d %d %d" % (len(m["kfs"]), MAX_ID, len(m["mps"]))]
    for k in m["kfs"]:
        keys = " ".join("%r %r %d %r" % q for q in k["keys"])
        lines.append("%d %d %d %d %d %d %d %d %s %s %s %s %d %s" % (k["id"], k["bad"], k["prev"], k["imu"], k["cam2"], k["bal"], k["baf"], int("pre" in k), fl(k["Rwb"]),
                                                                     fl(k["twb"]), fl(k["vel"]), fl(k["bias"]), len(k["keys"]), keys))
        if "pre" in k:
            p = k["pre"]
            lines.append(" ".join([fl(p["dT"])] + [fl(p[f]) for f in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b", "C")]))
    for p in m["mps"]:
        lines.append("%d %s %d %s" % (p["id"], fl(p["X"]), len(p["obs"]), " ".join("%d %d" % o for o in p["obs"])))
    path.write_text("\n".join(lines) + "\n")


def run(toy, tmp_path, m, its=7, fix_local=0, loop_id=0, stop=-1, init=0, prior_g=100.0, prior_a=1e6):
    case = tmp_path / "case.txt"
    write_case(case, m)
    out = subprocess.check_output([toy, str(case), str(its), str(fix_local), str(loop_id), str(stop), str(init), repr(prior_g), repr(prior_a)], text=True)
    hx = lambda t: [float.fromhex(x) for x in t]
    r = dict(kf=[], link=[], edge=[], state={}, bu=[], point={})
    for line in out.splitlines():
        t = line.split()
        if t[0] == "call" and t[1] == "n_kf":
            r["head"] = dict(n_kf=int(t[2]), n_points=int(t[4]), n_edges=int(t[6]), n_links=int(t[8]), shared=int(t[10]), its=int(t[12]), lam=float.fromhex(t[14]),
                             priors=hx(t[16:18]), stop=int(t[19]), huber=hx(t[21:24]), cam=hx(t[25:30]))
        elif t[0] == "call" and t[1] == "shared_bias":
            r["shared"] = hx(t[2:8])
        elif t[0] == "call" and t[1] == "kf":
            r["kf"].append((int(t[3]), int(t[4]), int(t[5]), hx(t[6:])))
        elif t[0] == "call" and t[1] == "link":
            r["link"].append((int(t[2]), int(t[3]), int(t[4]), hx(t[5:])))
        elif t[0] == "call" and t[1] == "edge":
            r["edge"].append((int(t[2]), int(t[3])) + tuple(hx(t[4:8])) + (int(t[8]),))
        elif t[0] == "calls":
            r["calls"] = (int(t[2]), int(t[4]), int(t[6]))
        elif t[0] == "state":
            r["state"][int(t[1])] = dict(writes=tuple(int(x) for x in t[2:5]), gba=int(t[5]), v=hx(t[6:]))
        elif t[0] == "bu":
            r["bu"].append(hx(t[1:]))
        elif t[0] == "point":
            r["point"][int(t[1])] = (int(t[2]), int(t[3]), hx(t[4:]))
    return r


def expected_walk(m, fix_local):
    """src/Optimizer.cc:394-719 restated on the toy map"""
    by_id = {k["id"]: k for k in m["kfs"]}
    slot = {}
    for k in m["kfs"]:
        if k["id"] <= MAX_ID:
            slot[k["id"]] = len(slot)
    fixed = {i: bool(fix_local) and (by_id[i]["bal"] >= MAX_ID - 1 or by_id[i]["baf"] >= MAX_ID - 1) for i in slot}
    links = []
    for k in m["kfs"]:
        p = k["prev"]
        if p < 0 or k["id"] > MAX_ID or k["bad"] or p > MAX_ID or not (k["imu"] and by_id[p]["imu"]):
            continue
        links.append((p, k["id"]))
    edges, not_included = [], []
    for j, mp in enumerate(m["mps"]):
        all_fixed = True
        for kid, li in mp["obs"]:
            k = by_id[kid]
            if kid > MAX_ID or k["bad"] or li == -1:
                continue
            x, y, octv, ur = k["keys"][li]
            all_fixed = all_fixed and fixed[kid]
            edges.append((slot[kid], j, x, y, ur if ur >= 0 else -1.0, [1.0, 0.5, 0.25][octv], int(ur >= 0)))
        not_included.append(all_fixed)
    return slot, fixed, links, edges, not_included


def info9(C):
    I = np.linalg.inv(np.asarray(C, np.float64)[:9, :9])
    I = (I + I.T) / 2
    w, V = np.linalg.eigh(I)
    w[w < 1e-12] = 0
    return V @ np.diag(w) @ V.T


@pytest.mark.parametrize("init,fix_local", [(1, 0), (0, 0), (0, 1)])
def test_flattening(toy, tmp_path, init, fix_local):
    m = make_map()
    r = run(toy, tmp_path, m, its=100, init=init, fix_local=fix_local, stop=0)
    slot, fixed, links, edges, _ = expected_walk(m, fix_local)
    by_id = {k["id"]: k for k in m["kfs"]}
    assert links == [(4, 5), (0, 1)] and list(slot) == [3, 0, 5, 1, 4, 2, 6]
    h = r["head"]
    assert (h["n_kf"], h["n_points"], h["n_links"], h["n_edges"], h["shared"], h["its"], h["stop"]) == (7, 4, 2, len(edges), init, 100, 0)
    assert h["lam"] == 1e-5 and h["huber"] == [float(F32(np.sqrt(5.991))), float(F32(np.sqrt(7.815))), float(np.sqrt(16.92))] and h["cam"] == [400.0, 410.0, 320.0, 240.0, 40.0]
    last = by_id[6]["bias"].astype(np.float64)                       # pIncKF = the last key frame visited with mnId <= maxKFid
    assert (r["shared"] == (list(last[3:]) + list(last[:3]) if init else [0.0] * 6)) and h["priors"] == ([100.0, 1e6] if init else [0.0, 0.0])
    for (pf, hi, imf, v), kid in zip(r["kf"], slot):
        k = by_id[kid]
        assert (pf, hi, imf) == (int(fixed[kid]), k["imu"], int(fixed[kid])), kid
        b = k["bias"].astype(np.float64) if k["imu"] else np.zeros(6)
        vel = k["vel"].astype(np.float64) if k["imu"] else np.zeros(3)
        assert v == list(k["Rwb"].astype(np.float64).ravel()) + list(k["twb"].astype(np.float64)) + list(vel) + list(b[3:]) + list(b[:3]), kid
    for (k1, k2, robust, v), (a, b) in zip(r["link"], links):
        p = by_id[b]["pre"]
        assert (k1, k2, robust) == (slot[a], slot[b], 1)
        flat = np.concatenate([[p["dT"]]] + [np.asarray(p[f], np.float64).ravel() for f in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "b")])
        assert v[:67] == list(flat.astype(np.float64))
        np.testing.assert_allclose(np.array(v[67:148]).reshape(9, 9), info9(p["C"]), rtol=1e-7, atol=1e-7 * np.abs(info9(p["C"])).max())      # no factor 1e-2
        C = np.asarray(p["C"], np.float64)
        np.testing.assert_allclose(np.array(v[148:157]).reshape(3, 3), np.linalg.inv(C[9:12, 9:12]), rtol=1e-9)
        np.testing.assert_allclose(np.array(v[157:166]).reshape(3, 3), np.linalg.inv(C[12:15, 12:15]), rtol=1e-9)
    assert sorted(r["edge"]) == sorted(edges)                       # (within a point the order is that of a map keyed by pointers)
    assert [e[1] for e in r["edge"]] == sorted(e[1] for e in edges)
    # SetNewBias(mPrevKF->GetImuBias()) on exactly the links' pre-integrations
    for k, bu in zip(m["kfs"], r["bu"]):
        want = by_id[k["prev"]]["bias"].astype(np.float64) if (k["prev"], k["id"]) in links else np.zeros(6)
        assert bu == list(want), k["id"]


def _pose(k, shift):
    R = k["Rwb"].astype(np.float64)
    t = k["twb"].astype(np.float64) + shift
    return np.concatenate([R.T.ravel(), -R.T @ t])


@pytest.mark.parametrize("loop_id,init,fix_local", [(0, 1, 0), (5, 0, 0), (0, 0, 1), (9, 1, 1)])
def test_write_back(toy, tmp_path, loop_id, init, fix_local):
    m = make_map()
    r = run(toy, tmp_path, m, loop_id=loop_id, init=init, fix_local=fix_local)
    _, _, _, _, not_included = expected_walk(m, fix_local)
    assert r["calls"] == (1, 0, 1)
    shared = next(k for k in m["kfs"] if k["id"] == 6)["bias"].astype(np.float64)
    for k in m["kfs"]:
        s = r["state"][k["id"]]
        v = np.array(s["v"])
        pose, pose_gba, vel, vel_gba, bias, bias_gba = v[0:12], v[12:24], v[24:27], v[27:30], v[30:36], v[36:42]
        in_problem = k["id"] <= MAX_ID
        b_in = k["bias"].astype(np.float64)
        b_out = ((shared if init else b_in) + np.array([0.0625] * 3 + [0.125] * 3)).astype(F32).astype(np.float64)
        v_out = (k["vel"].astype(np.float64) + 0.25).astype(F32).astype(np.float64)
        wrote_imu = in_problem and k["imu"]
        if loop_id == 0:
            assert s["writes"] == (int(in_problem), int(wrote_imu), int(wrote_imu)) and s["gba"] == 0
            if in_problem:
                np.testing.assert_allclose(pose, _pose(k, 0.5), rtol=0, atol=2e-6)
            assert list(vel) == list(v_out if wrote_imu else k["vel"].astype(np.float64)) and list(bias) == list(b_out if wrote_imu else b_in)
        else:
            assert s["writes"] == (0, 0, 0) and s["gba"] == (loop_id if in_problem else 0)
            if in_problem:
                np.testing.assert_allclose(pose_gba, _pose(k, 0.5), rtol=0, atol=2e-6)
            assert list(vel) == list(k["vel"].astype(np.float64)) and list(bias) == list(b_in)
            if wrote_imu:
                assert list(vel_gba) == list(v_out) and list(bias_gba) == list(b_out)
    assert not_included == ([True, False, True, False] if fix_local else [False, False, True, False])
    for mp, skip in zip(m["mps"], not_included):
        n_upd, gba, v = r["point"][mp["id"]]
        X = mp["X"].astype(np.float64)
        moved = list((X + 1.0).astype(F32).astype(np.float64))
        if skip:
            assert (n_upd, gba) == (0, 0) and v[:3] == list(X)
        elif loop_id == 0:
            assert (n_upd, gba) == (1, 0) and v[:3] == moved
        else:
            assert (n_upd, gba) == (0, loop_id) and v[:3] == list(X) and v[3:] == moved


def _untouched(m, r):
    for k in m["kfs"]:
        s = r["state"][k["id"]]
        assert s["writes"] == (0, 0, 0) and s["gba"] == 0 and s["v"][24:27] == list(k["vel"].astype(np.float64)), k["id"]
    for mp in m["mps"]:
        assert r["point"][mp["id"]][:2] == (0, 0) and r["point"][mp["id"]][2][:3] == list(mp["X"].astype(np.float64))


def test_raised_stop_flag_returns_without_a_call_or_a_write(toy, tmp_path):
    m = make_map()
    r = run(toy, tmp_path, m, stop=1, init=1)
    assert r["calls"] == (0, 0, 0)
    _untouched(m, r)
    assert sum(any(b) for b in r["bu"]) == 2                       # the links were visited before (:491 comes before :721)


def test_fewer_than_three_non_fixed_key_frames_return_early(toy, tmp_path):
    m = make_map(mostly_fixed=True)
    r = run(toy, tmp_path, m, fix_local=1)
    assert r["calls"] == (0, 0, 0)
    _untouched(m, r)
    assert not any(any(b) for b in r["bu"])                         # :468-472 comes before the links
    r = run(toy, tmp_path, m, fix_local=0)                          # without bFixLocal the markers are not read
    assert r["calls"] == (1, 0, 1) and not any(f for f, _, _, _ in r["kf"])


def test_second_camera_reaches_the_reference(toy, tmp_path):
    m = make_map(camera2=True)
    r = run(toy, tmp_path, m, init=1)
    assert r["calls"] == (0, 1, 0)
    _untouched(m, r)
    assert not any(any(b) for b in r["bu"])
