"""The inertial pose-graph adapter of include/orbslam3_shim_loop.hpp (OptimizeEssentialGraph4DoFHIP) against the stand-ins of
tests/stubs/: it compiles against them, and on a toy map the graph it hands to essg_optimize_4dof -- which key frames become
vertices, which one is fixed, each vertex's camera pose, body pose and calibration by either constructor, vScw, every edge with
its Tij in the reference's order, the map points with their reference vertex -- equals an independent restatement of the walk of
src/Optimizer.cc:5322-5539 written here in Python.  Covered: the edge order (loop connections, then per key frame inertial, loop,
covisibility), the absent spanning-tree edge, the (current, loop) weight exception, the sInsertedEdges filter, the mPrevKF /
mNextKF / child / loop-edge exclusions, NonCorrectedSim3, the CorrectedSim3 constructor with a scale that stays in scw and is
dropped from the vertex, and the fallbacks to the reference: a bad key frame's missing vertex, input the checks refuse, capacity.
Glue, not numerics; no GPU: the walk is host code and refusals come from the argument checks, which run before a device is asked for."""
import os
import subprocess

import numpy as np
import pytest

import posegraph_reference as ref
from test_shim_essential import _pose_sim3, _rand_q

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "orb_slam3-1_amd")
F32 = np.float32


def test_essential4dof_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_essential4dof.hpp"\n#include "orbslam3_shim_loop.hpp"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory, pkg):
    exe = tmp_path_factory.mktemp("shim_essential4dof") / "shim_essential4dof_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_essential4dof_toy.cpp"),
                           "-o", str(exe), "-L", LIBDIR, "-lorbslam3_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def _R32(q):
    """the float rotation matrix a float pose holds"""
    return ref.quat_to_R(np.asarray(q, F32)[None])[0]


def make_case(seed, n=12, bad=()):
    rs = np.random.RandomState(seed)
    ids = [3 * k + 1 for k in range(n)]
    qcb, tcb = _rand_q(rs), rs.normal(0, 0.1, 3)
    kfs = []
    for k in range(n):
        q, t = _rand_q(rs), rs.normal(0, 2, 3)
        # the body pose KeyFrame::SetPose derives in float: Rwb = Rwc Rcb, twb = Rwc tcb + twc
        Rwc = _R32(q).T
        twc = -(Rwc @ t.astype(F32))
        kfs.append(dict(id=ids[k], bad=int(k in bad), parent=ids[k - 1] if k else -1, prev=ids[k - 1] if k and k != 6 else -1,
                        next=ids[k + 1] if k + 1 < n and k != 5 else -1, q=q, t=t, qcb=qcb, tcb=tcb,
                        rwb=(Rwc @ _R32(qcb)).astype(F32), twb=(Rwc @ tcb.astype(F32) + twc).astype(F32)))
    weights = {}
    for k in range(n):
        for j in range(max(0, k - 4), k):
            weights[(ids[k], ids[j])] = int(rs.choice([30, 99, 100, 150, 400]))
    weights[(ids[6], ids[5])] = 500                                     # the parent, but neither mPrevKF nor mNextKF (the chain is cut there):
    weights[(ids[n - 1], ids[0])] = 60                                  # the loop pair itself is below minFeat: kept by the id rule
    weights[(ids[n - 2], ids[1])] = 50                                  # another loop connection below minFeat: dropped
    weights[(ids[n - 2], ids[0])] = 120                                 # a loop connection that is also a covisibility pair: sInsertedEdges
    weights[(ids[3], ids[2])] = 400                                     # mPrevKF / mNextKF of each other: never a covisibility edge
    loops = [(ids[8], ids[2]), (ids[9], ids[7])]
    weights[(ids[9], ids[7])] = 300                                     # a loop edge is never a covisibility edge as well
    sim3 = lambda: np.concatenate([_rand_q(rs), rs.normal(0, 2, 3), [rs.uniform(0.8, 1.2)]])
    non_corrected = {ids[k]: sim3() for k in (n - 1, n - 2, 5)}
    corrected = {ids[k]: sim3() for k in (n - 1, n - 2)}
    conn = [(ids[n - 1], ids[0]), (ids[n - 1], ids[1]), (ids[n - 2], ids[1]), (ids[n - 2], ids[0])]
    mps = [dict(bad=int(m == 2), ref=ids[int(rs.randint(0, n))], p=rs.normal(0, 3, 3).astype(F32)) for m in range(9)]
    return dict(ids=ids, kfs=kfs, weights=weights, loops=loops, non_corrected=non_corrected, corrected=corrected, conn=conn, mps=mps,
                loop=ids[0], cur=ids[n - 1])


def write_case(c, path):
    f = lambda v: " ".join(repr(float(x)) for x in np.asarray(v).ravel())
    with open(path, "w") as o:
        o.write("%d %d %d\n" % (len(c["kfs"]), c["loop"], c["cur"]))
        for k in c["kfs"]:
            o.write("%d %d %d %d %d %s %s %s %s %s %s\n" % (k["id"], k["bad"], k["parent"], k["prev"], k["next"], f(k["q"]), f(k["t"]), f(k["qcb"]), f(k["tcb"]),
                                                        f(k["rwb"]), f(k["twb"])))
        o.write("%d\n" % len(c["weights"]) + "".join("%d %d %d\n" % (a, b, w) for (a, b), w in c["weights"].items()))
        o.write("%d\n" % len(c["loops"]) + "".join("%d %d\n" % p for p in c["loops"]))
        for m in (c["non_corrected"], c["corrected"]):
            o.write("%d\n" % len(m) + "".join("%d %s\n" % (i, f(s)) for i, s in m.items()))
        o.write("%d\n" % len(c["conn"]) + "".join("%d %d\n" % p for p in c["conn"]))
        o.write("%d\n" % len(c["mps"]) + "".join("%d %d %s\n" % (m["bad"], m["ref"], f(m["p"])) for m in c["mps"]))


def run_toy(toy, c, tmp):
    path = os.path.join(tmp, "case.txt")
    write_case(c, path)
    r = subprocess.run([toy, "walk", path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    V, E, P, head = [], [], [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "vertices": head = dict(zip(w[0::2], map(int, w[1::2])))
        else: {"v": V, "e": E, "p": P}[w[0]].append((int(w[1]), int(w[2]), np.array([float.fromhex(x) for x in w[3:]])))
    return head, V, E, P


def _w(c, a, b):
    return c["weights"].get((a, b), c["weights"].get((b, a), 0))


def _covisibles(c, a, min_w=100):
    """KeyFrame::GetCovisiblesByWeight as the stand-in orders it: by descending weight, then by id"""
    nb = [(w, (y if x == a else x)) for (x, y), w in c["weights"].items() if a in (x, y) and w >= min_w]
    return [i for w, i in sorted(nb, key=lambda p: (-p[0], p[1]))]


def _tij(Si, Sj):
    """rotation matrix and translation of Sij = Siw * Sjw^-1; the product's scale stays in the translation"""
    S = ref.sim3_mul(Si[None], ref.sim3_inv(Sj[None]))[0]
    return np.concatenate([ref.quat_to_R(S[None, :4])[0].ravel(), S[4:7]])


def walk(c):
    """:5322-5539, restated: vertices (id, fixed, rcw tcw rwb twb rcb tcb scw), edges (i, j, dRij dtij), points, dropped edges"""
    kf = {k["id"]: k for k in c["kfs"]}
    V, scw = [], {}
    for k in c["kfs"]:
        if k["bad"]:
            continue
        Rcb, tcb = _R32(k["qcb"]).astype(np.float64), k["tcb"].astype(F32).astype(np.float64)
        s = c["corrected"].get(k["id"])
        if s is None:       # ImuCamPose(KeyFrame*): the float members, each cast to double
            s = _pose_sim3(k["q"], k["t"])
            Rcw, tcw = _R32(k["q"]).astype(np.float64), k["t"].astype(F32).astype(np.float64)
            Rwb, twb = k["rwb"].astype(np.float64), k["twb"].astype(np.float64)
        else:               # ImuCamPose(Rwc, twc, pKF) with Rwc, twc of Scw.inverse(): the scale divides twc and is gone
            s = np.asarray(s)
            Swc = ref.sim3_inv(s[None])[0]
            Rwc, twc = ref.quat_to_R(Swc[None, :4])[0], Swc[4:7]
            Rcw, tcw, Rwb, twb = Rwc.T, -Rwc.T @ twc, Rwc @ Rcb, Rwc @ tcb + twc
        scw[k["id"]] = s
        V.append((k["id"], int(k["id"] == c["loop"]), np.concatenate([Rcw.ravel(), tcw, Rwb.ravel(), twb, Rcb.ravel(), tcb, s])))
    ident = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    S = lambda i: scw.get(i, ident)
    NC = lambda i: np.asarray(c["non_corrected"][i]) if i in c["non_corrected"] else S(i)
    E, inserted = [], set()
    by_i = {}
    for a, b in c["conn"]:
        by_i.setdefault(a, []).append(b)
    for a in sorted(by_i, key=lambda i: c["ids"].index(i)):            # std::map / std::set of pointers into one deque: address order = index order
        for b in sorted(by_i[a], key=lambda i: c["ids"].index(i)):
            if (a != c["cur"] or b != c["loop"]) and _w(c, a, b) < 100:
                continue
            E.append((a, b, _tij(S(a), S(b))))
            inserted.add((min(a, b), max(a, b)))
    for k in c["kfs"]:
        i = k["id"]
        if k["prev"] >= 0:
            E.append((i, k["prev"], _tij(NC(i), NC(k["prev"]))))
        mine = sorted([(y if x == i else x) for x, y in c["loops"] if i in (x, y)], key=lambda j: c["ids"].index(j))
        for j in mine:
            if j < i:
                E.append((i, j, _tij(NC(i), NC(j))))
        children = [q["id"] for q in c["kfs"] if q["parent"] == i]
        for j in _covisibles(c, i):
            if j not in (k["prev"], k["next"]) and j not in children and j not in mine and not kf[j]["bad"] and j < i:
                if (min(i, j), max(i, j)) in inserted:
                    continue
                E.append((i, j, _tij(NC(i), NC(j))))
    have = {v[0] for v in V}
    dropped = sum(1 for e in E if e[0] not in have or e[1] not in have)
    E = [e for e in E if e[0] in have and e[1] in have]
    P = [(m, mp["ref"] if mp["ref"] in have else -1, mp["p"].astype(np.float64)) for m, mp in enumerate(c["mps"]) if not mp["bad"]]
    return V, E, P, dropped


def _same(got, want, what):
    assert [g[:2] for g in got] == [w[:2] for w in want], what
    for g, w in zip(got, want):
        assert g[2].shape == w[2].shape and np.abs(g[2] - w[2]).max() < 1e-5, (what, g[:2])      # poses pass through float rotation matrices on both sides


def test_graph_of_the_walk(toy, tmp_path):
    c = make_case(3)
    ids = c["ids"]
    head, V, E, P = run_toy(toy, c, str(tmp_path))
    Vr, Er, Pr, dropped = walk(c)
    assert head["dropped"] == dropped == 0 and head["vertices"] == 12
    _same(V, Vr, "vertices"); _same(E, Er, "edges"); _same(P, Pr, "points")
    pairs = [e[:2] for e in E]
    # loop connections first, in the order of the map and its sets; (current, loop) is below minFeat and kept because it is the loop itself
    assert pairs[:2] == [(ids[-2], ids[0]), (c["cur"], c["loop"])] and _w(c, c["cur"], c["loop"]) < 100
    after = pairs[2:]
    assert (ids[-2], ids[1]) not in pairs                               # below minFeat: dropped
    assert pairs.count((ids[-2], ids[0])) == 1                          # loop connection and covisible: sInsertedEdges keeps it single
    assert pairs.count((ids[9], ids[7])) == 1                           # a loop edge is not repeated as a covisibility edge
    assert pairs.count((ids[3], ids[2])) == 1                           # mPrevKF: the inertial edge alone
    # no spanning-tree edge: key frame 6 has a parent but no mPrevKF, so the pair appears once, as the covisibility edge the
    # Sim3 walk would have excluded for being the parent
    assert pairs.count((ids[6], ids[5])) == 1
    # per key frame: inertial, then loop, then covisibility
    of8 = [p for p in after if p[0] == ids[8]]
    assert of8[0] == (ids[8], ids[7]) and of8[1] == (ids[8], ids[2])
    assert sum(v[1] for v in V) == 1 and V[0][1] == 1
    # the CorrectedSim3 constructor: scw is the map's entry bit for bit, scale included; the vertex's tcw is t / s
    cur = [v for v in V if v[0] == c["cur"]][0][2]
    s = np.asarray(c["corrected"][c["cur"]])
    assert np.array_equal(cur[36:44], s) and abs(s[7] - 1) > 1e-3
    assert np.abs(cur[9:12] - s[4:7] / s[7]).max() < 1e-12
    Rcw, tcw, Rwb, twb, Rcb, tcb = cur[0:9].reshape(3, 3), cur[9:12], cur[12:21].reshape(3, 3), cur[21:24], cur[24:33].reshape(3, 3), cur[33:36]
    assert np.abs(Rcb @ Rwb.T - Rcw).max() < 1e-6 and np.abs(Rcb @ (-Rwb.T @ twb) + tcb - tcw).max() < 1e-5        # (Rcb is a float matrix: orthonormal to 1e-7)
    # NonCorrectedSim3 replaces the pose of key frame 5 in its edges, not in its vertex
    e65 = [e for e in E if e[:2] == (ids[6], ids[5])][0][2]
    kf5 = c["kfs"][5]
    assert np.abs(e65 - _tij(_pose_sim3(c["kfs"][6]["q"], c["kfs"][6]["t"]), np.asarray(c["non_corrected"][ids[5]]))).max() < 1e-5
    assert np.abs(e65 - _tij(_pose_sim3(c["kfs"][6]["q"], c["kfs"][6]["t"]), _pose_sim3(kf5["q"], kf5["t"]))).max() > 1e-2
    v5 = [v for v in V if v[0] == ids[5]][0][2]
    assert np.abs(v5[9:12] - kf5["t"].astype(F32)).max() == 0 and np.array_equal(v5[12:21], kf5["rwb"].astype(np.float64).ravel())


def test_bad_key_frame_falls_back(toy, tmp_path):
    c = make_case(4, bad=(6,))
    head, V, E, P = run_toy(toy, c, str(tmp_path))
    Vr, Er, Pr, dropped = walk(c)
    assert c["ids"][6] not in [v[0] for v in V] and len(V) == 11
    assert head["dropped"] == dropped >= 1                              # the inertial edge of the key frame after it
    _same(V, Vr, "vertices"); _same(E, Er, "edges"); _same(P, Pr, "points")
    r = subprocess.run([toy, "fallback", os.path.join(str(tmp_path), "case.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "reference calls 1 pose writes 0 map changes 0" in r.stdout, r.stdout + r.stderr


def test_fallback_on_input_the_device_refuses(toy, tmp_path):
    """a corrected pose with scale 0 (its inverse, from which the vertex comes, is not finite): refused by the argument checks, so
    the reference class is called and nothing is written"""
    c = make_case(6)
    c["corrected"][c["cur"]] = np.array([0, 0, 0, 1, 0.5, 0, 0, 0.0])
    write_case(c, os.path.join(str(tmp_path), "case.txt"))
    r = subprocess.run([toy, "fallback", os.path.join(str(tmp_path), "case.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "reference calls 1 pose writes 0 map changes 0" in r.stdout, r.stdout + r.stderr


def test_fallback_above_the_capacity(toy):
    """1025 free key frames: ORBX_ERR_CAPACITY from the checks, the reference class is called and nothing is written"""
    r = subprocess.run([toy, "capacity", "1026"], capture_output=True, text=True)
    assert r.returncode == 0 and "reference calls 1 pose writes 0 map changes 0" in r.stdout, r.stdout + r.stderr
