"""include/orbslam3_shim_mapping.hpp (CreateNewMapPointsHIP) against the stand-ins of tests/stubs/: it compiles against them (no
GPU), refuses key frames with a second camera before any device call, and on a toy map its glue -- what it flattens from the
key frames, the epipole and F12 per neighbour, the creation order of the candidates -- gives what the Python mirror gives on
the same arrays (GPU).  Glue, not numerics: neither an oracle nor a build of the reference."""
import os
import subprocess

import numpy as np
import pytest

import newpoints_common as NC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
LIBDIR = os.path.join(ROOT, "orb_slam3-1_amd")
CASE = dict(seed=41, n=160, n_neighbours=4, stereo_frac=0.5, distortion=-0.03, far_points=True, th_far=10.0)


def test_mapping_shim_compiles_against_standins(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_mapping.hpp"\n#include "orbslam3_shim_mapping.hpp"\n'
                   'template bool ORB_SLAM3::CreateNewMapPointsHIP<ORB_SLAM3::MappingKeyFrame>(ORB_SLAM3::MappingKeyFrame*, '
                   'const std::vector<ORB_SLAM3::MappingKeyFrame*>&, bool, bool, bool, float, '
                   'std::vector<ORB_SLAM3::NewMapPointCandidateT<ORB_SLAM3::MappingKeyFrame> >&);\nint main() { return 0; }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    src.write_text('#include "orbslam3_shim_mapping.hpp"\nint main() { return 0; }\n')    # without the macro: the POD half only
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory, pkg):
    exe = tmp_path_factory.mktemp("shim_mapping") / "shim_mapping_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_mapping_toy.cpp"),
                           "-o", str(exe), "-L", LIBDIR, "-lorbslam3_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
    return str(exe)


def _write_case(sc, path, coarse):
    pr = sc["params"]
    with open(path, "w") as f:
        f.write("%d %d %d %d %r\n" % (1 + len(sc["neighbours"]), pr["inertial"], coarse, pr["far_points"], float(np.float32(pr["th_far"]))))
        for kf in [sc["kf1"]] + sc["neighbours"]:
            n, nl = len(kf["x"]), len(kf["scale_factors"])
            f.write("%d " % n + " ".join(repr(float(kf[k])) for k in ("fx", "fy", "cx", "cy", "mb", "mbf")) + " %r %d\n" % (float(np.float32(pr["scale_factor_1"])), nl))
            f.write(" ".join(repr(float(v)) for v in list(np.asarray(kf["Rcw"]).reshape(-1)) + list(kf["tcw"])) + "\n")
            f.write(" ".join(repr(float(v)) for v in kf["level_sigma2"]) + "\n" + " ".join(repr(float(v)) for v in kf["scale_factors"]) + "\n")
            nodes, off, feat = kf["fv"]
            node_of = np.zeros(n, np.int64)
            for a in range(len(nodes)):
                node_of[feat[off[a]:off[a + 1]]] = nodes[a]
            kx = kf["x"] if kf.get("key_x") is None else kf["key_x"]
            ky = kf["y"] if kf.get("key_y") is None else kf["key_y"]
            for i in range(n):
                f.write("%d %r %r %d %r %r %r %r %d " % (kf["has_mp"][i], float(kf["x"][i]), float(kf["y"][i]), kf["octave"][i], float(kf["u_right"][i]),
                                                         float(kf["depth"][i]), float(kx[i]), float(ky[i]), node_of[i]))
                f.write(" ".join(str(int(b)) for b in kf["desc"][i]) + "\n")


def _run(toy, mode, sc, tmp_path, coarse=0):
    path = str(tmp_path / "case.txt")
    _write_case(sc, path, coarse)
    r = subprocess.run(["timeout", "-k", "10", "120", toy, mode, path], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    d = dict(Ow=[], pair=[], cand=[])
    for line in r.stdout.strip().splitlines():
        tok = line.split()
        if tok[0] == "handled":
            d["handled"], d["n"] = int(tok[1]), int(tok[3])
        elif tok[0] == "cand":
            d["cand"].append([int(v) for v in tok[2:6]] + [float.fromhex(v) for v in tok[6:]])
        else:
            d[tok[0]].append([float.fromhex(v) for v in tok[2:]])
    return d


def test_toy_builds_and_second_cameras_go_to_the_reference(toy, tmp_path):
    """no device needed: the adapter reports an unsupported rig before any device call"""
    r = subprocess.run([toy], capture_output=True, text=True)
    assert r.returncode == 2 and "usage" in r.stderr
    d = _run(toy, "fallback", NC.make_scene(dict(CASE, n=40)), tmp_path)
    assert d["handled"] == 0 and d["n"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("coarse", [0, 1])
def test_adapter_equals_python_mirror(toy, pkg, tmp_path, coarse):
    sc = NC.make_scene(CASE)
    d = _run(toy, "run", sc, tmp_path, coarse)
    assert d["handled"] == 1 and d["n"] == len(d["cand"]) > 30
    # what the adapter derived from the poses agrees with the generator's own values to float accuracy ...
    kfs = [sc["kf1"]] + sc["neighbours"]
    for kf, Ow in zip(kfs, d["Ow"]):
        assert np.allclose(Ow, kf["Ow"], rtol=0, atol=1e-5)
    for pr, row in zip(sc["pairs"], d["pair"]):
        F, Fa = np.asarray(pr["F12"], np.float64), np.asarray(row[2:])
        assert np.abs(F - Fa).max() <= 1e-4 * np.abs(F).max()
        assert abs(row[0] - pr["ep"][0]) <= 1e-3 * max(1.0, abs(pr["ep"][0])) and abs(row[1] - pr["ep"][1]) <= 1e-3 * max(1.0, abs(pr["ep"][1]))
    # ... and the mirror on exactly those arrays gives exactly the adapter's candidates, in its order
    same = dict(sc)
    same["kf1"] = dict(sc["kf1"], Ow=np.asarray(d["Ow"][0], np.float32))
    same["neighbours"] = [dict(k, Ow=np.asarray(o, np.float32)) for k, o in zip(sc["neighbours"], d["Ow"][1:])]
    same["pairs"] = [dict(ep=(np.float32(r[0]), np.float32(r[1])), F12=np.asarray(r[2:], np.float32), coarse=bool(coarse)) for r in d["pair"]]
    for k in [same["kf1"]] + same["neighbours"]:
        if k.get("key_x") is None:
            k["key_x"], k["key_y"] = k["x"], k["y"]
    m = pkg.Matcher(0.6, False)
    try:
        r = m.create_new_map_points(same["kf1"], same["neighbours"], same["pairs"], same["params"])
    finally:
        m.close()
    order = [(j, i) for j in range(len(sc["neighbours"])) for i in np.nonzero(r["neighbour"] == j)[0]]
    assert [(c[1], c[0]) for c in d["cand"]] == order
    for c in d["cand"]:
        i = c[0]
        assert c[2] == r["idx2"][i] and c[3] == r["point_stereo"][i]
        got = np.asarray(c[4:], np.float32)
        want = np.concatenate([r["x3d"][i], r["normal"][i], [r["max_dist"][i], r["min_dist"][i]]]).astype(np.float32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
