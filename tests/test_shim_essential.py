"""The pose-graph adapters of include/orbslam3_shim_loop.hpp (OptimizeEssentialGraphHIP, both overloads) against the stand-ins of
tests/stubs/: they compile against them, and on a toy map the graph they hand to essg_optimize -- which key frames become
vertices, which are fixed, every edge with its measurement in the reference's order, the map points with their reference
vertex -- equals an independent restatement of the walk of src/Optimizer.cc:1517-1726 and :1806-2051 written here in Python.
Covered: both overloads, a bad key frame (its edges are refused, the adapter falls back), a duplicate edge (a loop edge that is
also a covisibility edge), NonCorrectedSim3 / CorrectedSim3, the weight rule of the loop connections, and the fallbacks to the
reference for input the device refuses.  Glue, not numerics; no GPU: the walk is host code and refusals come from the argument
checks, which run before a device is asked for."""
import os
import subprocess

import numpy as np
import pytest

import posegraph_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "orb_slam3-1_amd")
F32 = np.float32


def test_essential_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_essential.hpp"\n#include "orbslam3_shim_loop.hpp"\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory, pkg):
    exe = tmp_path_factory.mktemp("shim_essential") / "shim_essential_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_essential_toy.cpp"),
                           "-o", str(exe), "-L", LIBDIR, "-lorbslam3_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def _rand_q(rs):
    q = rs.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    return q if q[3] > 0 else -q


def _pose_sim3(q, t):
    """g2o::Sim3(Tcw.unit_quaternion(), Tcw.translation(), 1.0) of a float pose held as a rotation matrix"""
    qf = np.asarray(q, F32)
    R = ref.quat_to_R(qf[None])[0].astype(np.float64)
    return np.concatenate([ref.quat_from_R(R[None])[0], np.asarray(t, F32).astype(np.float64), [1.0]])


def make_case(seed, n=12, bad=(), fix_scale=False):
    rs = np.random.RandomState(seed)
    ids = [3 * k + 1 for k in range(n)]
    kfs = []
    for k in range(n):
        kfs.append(dict(id=ids[k], bad=int(k in bad), parent=ids[k - 1] if k else -1, imu=int(k == 4), prev=ids[3] if k == 4 else -1,
                        group=0 if k < 3 else (1 if k < 5 else 2), q=_rand_q(rs), t=rs.normal(0, 2, 3), qb=_rand_q(rs), tb=rs.normal(0, 2, 3)))
    weights = {}
    for k in range(n):
        for j in range(max(0, k - 4), k):
            weights[(ids[k], ids[j])] = int(rs.choice([30, 99, 100, 150, 400]))
    weights[(ids[n - 1], ids[0])] = 60                                  # the loop pair itself is below minFeat: kept by the id rule
    weights[(ids[n - 2], ids[1])] = 50                                  # another loop connection below minFeat: dropped
    weights[(ids[n - 2], ids[0])] = 120
    loops = [(ids[8], ids[2]), (ids[9], ids[7])]                        # the second is also a covisibility pair: a duplicate edge
    weights[(ids[9], ids[7])] = 300
    sim3 = lambda: np.concatenate([_rand_q(rs), rs.normal(0, 2, 3), [1.0 if fix_scale else rs.uniform(0.8, 1.2)]])
    non_corrected = {ids[k]: sim3() for k in (n - 1, n - 2, 5)}
    corrected = {ids[k]: sim3() for k in (n - 1, n - 2)}
    conn = [(ids[n - 1], ids[0]), (ids[n - 1], ids[1]), (ids[n - 2], ids[1]), (ids[n - 2], ids[0])]
    mps = [dict(bad=int(m == 2), ref=ids[int(rs.randint(0, n))], by=ids[n - 1] if m % 3 == 0 else 0, cref=ids[int(rs.randint(0, n))],
                p=rs.normal(0, 3, 3).astype(F32)) for m in range(9)]
    return dict(ids=ids, kfs=kfs, weights=weights, loops=loops, non_corrected=non_corrected, corrected=corrected, conn=conn, mps=mps,
                init=ids[0], loop=ids[0], cur=ids[n - 1], fix_scale=int(fix_scale))


def write_case(c, path):
    f = lambda v: " ".join(repr(float(x)) for x in v)
    with open(path, "w") as o:
        o.write("%d %d %d %d %d\n" % (len(c["kfs"]), c["init"], c["loop"], c["cur"], c["fix_scale"]))
        for k in c["kfs"]:
            o.write("%d %d %d %d %d %d %s %s %s %s\n" % (k["id"], k["bad"], k["parent"], k["imu"], k["prev"], k["group"], f(k["q"]), f(k["t"]), f(k["qb"]), f(k["tb"])))
        o.write("%d\n" % len(c["weights"]) + "".join("%d %d %d\n" % (a, b, w) for (a, b), w in c["weights"].items()))
        o.write("%d\n" % len(c["loops"]) + "".join("%d %d\n" % p for p in c["loops"]))
        for m in (c["non_corrected"], c["corrected"]):
            o.write("%d\n" % len(m) + "".join("%d %s\n" % (i, f(s)) for i, s in m.items()))
        o.write("%d\n" % len(c["conn"]) + "".join("%d %d\n" % p for p in c["conn"]))
        o.write("%d\n" % len(c["mps"]) + "".join("%d %d %d %d %s\n" % (m["bad"], m["ref"], m["by"], m["cref"], f(m["p"])) for m in c["mps"]))


def run_toy(toy, mode, c, tmp):
    path = os.path.join(tmp, "case.txt")
    write_case(c, path)
    r = subprocess.run([toy, mode, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    V, E, P, head = [], [], [], None
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "vertices": head = dict(zip(w[0::2], map(int, w[1::2])))
        elif w[0] == "v": V.append((int(w[1]), int(w[2]), np.array([float.fromhex(x) for x in w[3:]])))
        elif w[0] == "e": E.append((int(w[1]), int(w[2]), np.array([float.fromhex(x) for x in w[3:]])))
        elif w[0] == "p": P.append((int(w[1]), int(w[2]), np.array([float.fromhex(x) for x in w[3:]])))
    return head, V, E, P, r.stdout


def _w(c, a, b):
    return c["weights"].get((a, b), c["weights"].get((b, a), 0))


def _covisibles(c, a, min_w=100):
    """KeyFrame::GetCovisiblesByWeight as the stand-in orders it: by descending weight, then by id"""
    nb = [(w, (y if x == a else x)) for (x, y), w in c["weights"].items() if a in (x, y) and w >= min_w]
    return [i for w, i in sorted(nb, key=lambda p: (-p[0], p[1]))]


def _mulinv(Sj, Si):
    return ref.sim3_mul(Sj[None], ref.sim3_inv(Si[None]))[0]


def walk_loop(c):
    """:1517-1726, restated: returns vertices, edges (i, j, Sji) or None for an edge g2o refuses, and the points"""
    kf = {k["id"]: k for k in c["kfs"]}
    V, scw = [], {}
    for k in c["kfs"]:
        if k["bad"]:
            continue
        s = c["corrected"].get(k["id"])
        s = _pose_sim3(k["q"], k["t"]) if s is None else np.asarray(s)
        scw[k["id"]] = s
        V.append((k["id"], int(k["id"] == c["init"]), s))
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
            E.append((a, b, _mulinv(S(b), S(a))))
            inserted.add((min(a, b), max(a, b)))
    for k in c["kfs"]:
        i = k["id"]
        Swi_of = NC(i)
        if k["parent"] >= 0:
            E.append((i, k["parent"], _mulinv(NC(k["parent"]), Swi_of)))
        mine = sorted([(y if x == i else x) for x, y in c["loops"] if i in (x, y)], key=lambda j: c["ids"].index(j))
        for j in mine:
            if j < i:
                E.append((i, j, _mulinv(NC(j), Swi_of)))
        children = [q["id"] for q in c["kfs"] if q["parent"] == i]
        for j in _covisibles(c, i):
            if j != k["parent"] and j not in children and not kf[j]["bad"] and j < i:
                if (min(i, j), max(i, j)) in inserted:
                    continue
                E.append((i, j, _mulinv(NC(j), Swi_of)))
        if k["imu"] and k["prev"] >= 0:
            E.append((i, k["prev"], _mulinv(NC(k["prev"]), Swi_of)))
    have = {v[0] for v in V}
    dropped = sum(1 for e in E if e[0] not in have or e[1] not in have)
    E = [e for e in E if e[0] in have and e[1] in have]
    P = []
    for m, mp in enumerate(c["mps"]):
        if mp["bad"]:
            continue
        r = mp["cref"] if mp["by"] == c["cur"] else mp["ref"]
        P.append((m, r if r in have else -1, mp["p"].astype(np.float64)))
    return V, E, P, dropped


def walk_merge(c):
    """:1806-2051, restated"""
    kf = {k["id"]: k for k in c["kfs"]}
    groups = [[k for k in c["kfs"] if k["group"] == g] for g in range(3)]
    V, scw, cswc, good, bad = [], {}, {}, {}, {}
    for k in groups[0]:
        if k["bad"]: continue
        s = _pose_sim3(k["q"], k["t"]); cswc[k["id"]] = ref.sim3_inv(s[None])[0]; V.append((k["id"], 1, s)); good[k["id"]], bad[k["id"]] = True, False
    for k in groups[1]:
        if k["bad"]: continue
        s = _pose_sim3(k["q"], k["t"]); cswc[k["id"]] = ref.sim3_inv(s[None])[0]; scw[k["id"]] = _pose_sim3(k["qb"], k["tb"])
        V.append((k["id"], 1, s)); good[k["id"]], bad[k["id"]] = True, True
    for k in groups[2]:
        if k["bad"]: continue
        s = _pose_sim3(k["q"], k["t"]); scw[k["id"]] = s; V.append((k["id"], 0, s)); good[k["id"]], bad[k["id"]] = False, True
    ident = np.array([0, 0, 0, 1, 0, 0, 0, 1.0])
    allk = groups[0] + groups[1] + groups[2]
    ids = {k["id"] for k in allk}
    E = []

    def rel(i, j):
        if good.get(i) and good.get(j): return ref.sim3_inv(cswc.get(j, ident)[None])[0]
        if bad.get(i) and bad.get(j): return scw.get(j, ident)
        return None
    for k in allk:
        i = k["id"]
        Swi = ref.sim3_inv(scw.get(i, ident)[None])[0] if bad.get(i) else ident
        edge = lambda j, Sjw: E.append((i, j, ref.sim3_mul(Sjw[None], Swi[None])[0]))
        if k["parent"] >= 0 and k["parent"] in ids and rel(i, k["parent"]) is not None:
            edge(k["parent"], rel(i, k["parent"]))
        mine = sorted([(y if x == i else x) for x, y in c["loops"] if i in (x, y)], key=lambda j: c["ids"].index(j))
        for j in mine:
            if j in ids and j < i and rel(i, j) is not None:
                edge(j, rel(i, j))
        children = [q["id"] for q in c["kfs"] if q["parent"] == i]
        for j in _covisibles(c, i):
            if j != k["parent"] and j not in children and j not in mine and j in ids and not kf[j]["bad"] and j < i and rel(i, j) is not None:
                edge(j, rel(i, j))
    have = {v[0] for v in V}
    dropped = sum(1 for e in E if e[0] not in have or e[1] not in have)
    return V, [e for e in E if e[0] in have and e[1] in have], dropped


def _same(got, want, what):
    assert [g[:2] for g in got] == [w[:2] for w in want], what
    for g, w in zip(got, want):
        assert np.abs(g[2] - w[2]).max() < 1e-5, (what, g[:2])          # poses pass through float rotation matrices on both sides


@pytest.mark.parametrize("fix_scale", [False, True])
def test_loop_overload_graph(toy, tmp_path, fix_scale):
    c = make_case(3, fix_scale=fix_scale)
    head, V, E, P, _ = run_toy(toy, "loop", c, str(tmp_path))
    Vr, Er, Pr, dropped = walk_loop(c)
    assert head["fix_scale"] == int(fix_scale) and head["dropped"] == dropped == 0
    _same(V, Vr, "vertices"); _same(E, Er, "edges"); _same(P, Pr, "points")
    pairs = [e[:2] for e in E]
    assert (c["cur"], c["loop"]) in pairs                               # below minFeat, kept because it is the loop itself
    assert (c["ids"][-2], c["ids"][1]) not in pairs                     # below minFeat: dropped
    assert pairs.count((c["ids"][9], c["ids"][7])) == 2                 # a loop edge that is also a covisibility edge: twice
    assert (c["ids"][4], c["ids"][3]) in pairs and pairs.count((c["ids"][4], c["ids"][3])) == 2       # parent and mPrevKF (inertial edge)
    assert sum(v[1] for v in V) == 1 and V[0][1] == 1
    cur = [v for v in V if v[0] == c["cur"]][0]
    assert np.array_equal(cur[2], c["corrected"][c["cur"]])             # CorrectedSim3 is the estimate, bit for bit


def test_loop_overload_bad_key_frame(toy, tmp_path):
    c = make_case(4, bad=(6,))
    head, V, E, P, _ = run_toy(toy, "loop", c, str(tmp_path))
    Vr, Er, Pr, dropped = walk_loop(c)
    assert c["ids"][6] not in [v[0] for v in V] and len(V) == 11
    assert head["dropped"] == dropped >= 2                              # its own spanning-tree edge and its child's
    _same(V, Vr, "vertices"); _same(E, Er, "edges"); _same(P, Pr, "points")
    r = subprocess.run([toy, "fallback", os.path.join(str(tmp_path), "case.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "reference calls 1 pose writes 0 map changes 0" in r.stdout, r.stdout + r.stderr


def test_merge_overload_graph(toy, tmp_path):
    c = make_case(5)
    head, V, E, P, _ = run_toy(toy, "merge", c, str(tmp_path))
    Vr, Er, dropped = walk_merge(c)
    assert head["fix_scale"] == 0 and head["dropped"] == dropped == 0 and not P
    _same(V, Vr, "vertices"); _same(E, Er, "edges")
    fixed = {v[0]: v[1] for v in V}
    assert sum(fixed.values()) == 5
    assert any(fixed[a] and fixed[b] for a, b, _ in E)                  # edges between two fixed vertices stay in the graph
    # a relation needs two corrected or two uncorrected poses: nothing joins the first group to the third
    g = {k["id"]: k["group"] for k in c["kfs"]}
    assert not any({g[a], g[b]} == {0, 2} for a, b, _ in E)


def test_fallback_on_input_the_device_refuses(toy, tmp_path):
    """a corrected pose with scale 0: refused by the argument checks, so the reference class is called and nothing is written"""
    c = make_case(6)
    c["corrected"][c["cur"]] = np.array([0, 0, 0, 1, 0, 0, 0, 0.0])
    write_case(c, os.path.join(str(tmp_path), "case.txt"))
    r = subprocess.run([toy, "fallback", os.path.join(str(tmp_path), "case.txt")], capture_output=True, text=True)
    assert r.returncode == 0 and "reference calls 1 pose writes 0 map changes 0" in r.stdout, r.stdout + r.stderr
