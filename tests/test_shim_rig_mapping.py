"""The rig adapter of CreateNewMapPoints (include/orbslam3_shim_rig_mapping.hpp: CreateNewMapPointsRigHIP) against the stand-in types
of tests/stubs/ and a recording fake of the C entry points (tests/stubs/shim_rig_mapping_toy.cpp): the header compiles with -Wall
-Wextra -Werror; the routing on NLeft (all conventional: the existing entry; all fisheye rigs: the rig entry; a mixed pair or a rig of
other cameras: false before any C call); the flattened key frames (raw key points of both lists, both poses and centres, both
cameras); the four pose products per neighbour; the candidates in creation order and the skipped flags.  No GPU: routing,
marshalling and write-back are host code."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUBS = os.path.join(ROOT, "tests", "stubs")
INC = os.path.join(ROOT, "include")
f32 = np.float32


def test_rig_mapping_shim_compiles_against_standins_next_to_the_existing_adapters(tmp_path):
    src = tmp_path / "t.cpp"
    src.write_text('#define ORBSLAM3_HIP_WITH_REFERENCE\n#include "standin_rig_mapping.hpp"\n#include "orbslam3_shim_rig_map.hpp"\n#include "orbslam3_shim_rig_mapping.hpp"\n'
                   'using namespace ORB_SLAM3;\n'
                   'int main() { RigMappingKeyFrame K; std::vector<RigMappingKeyFrame*> nb; std::vector<NewMapPointCandidateT<RigMappingKeyFrame> > c;\n'
                   '  return CreateNewMapPointsRigHIP<RigMappingKeyFrame, KannalaBrandt8Rig>(&K, nb, false, false, false, 0.f, c)\n'
                   '         + CreateNewMapPointsHIP(&K, nb, false, false, false, 0.f, c); }\n')
    r = subprocess.run(["g++", "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, str(src)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


@pytest.fixture(scope="module")
def toy(tmp_path_factory):
    exe = tmp_path_factory.mktemp("shim_rig_mapping") / "shim_rig_mapping_toy"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", STUBS, "-I", INC, os.path.join(STUBS, "shim_rig_mapping_toy.cpp"), "-o", str(exe)])

    def run(scenario):
        r = subprocess.run([str(exe), scenario], check=True, capture_output=True, text=True)
        out = [ln.split() for ln in r.stdout.splitlines()]
        rows = {ln[0]: (None if ln[1:] == ["NULL"] else [float.fromhex(v) for v in ln[1:]]) for ln in out if len(ln) > 1 and not ln[0].startswith(("orbm_", "handled", "cand"))}
        calls = [ln for ln in out if ln[0].startswith("orbm_")]
        handled = [ln for ln in out if ln[0] == "handled"][0]
        cands = [ln[1:] for ln in out if ln[0] == "cand"]
        return calls, rows, handled, cands
    return run


def _desc(rows, seed):
    return [float((i * 7 + seed) & 0xFF) for i in range(rows * 32)]


T = [(np.eye(3), np.array([0.25, -0.5, 0.75])), (np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([1.5, 0.125, -0.375])),
     (np.eye(3), np.array([-1.0, 0.5, 2.0])), (np.array([[0.0, -1, 0], [1, 0, 0], [0, 0, 1]]), np.array([0.5, -2.0, 0.25]))]
TRL = [np.array([-0.125, 0.015625, 0.03125])] + [np.array([-0.25, 0.0625, 0.5])] * 3
CAMS1 = [[190.5, 190.25, 254.5, 256.75, 0.003, 0.0007, -0.002, 0.0002, 1e-6], [191.5, 191.25, 252.5, 254.75, 0.004, 0.0018, -0.0027, 0.0004, 2e-6]]
CAMS2 = [[290.5, 290.25, 354.5, 356.75, 0.013, 0.0107, -0.012, 0.0102, 3e-6], [291.5, 291.25, 352.5, 354.75, 0.014, 0.0118, -0.0127, 0.0104, 4e-6]]
flat32 = lambda cams: [float(f32(v)) for c in cams for v in c]


def test_rig_key_frames_go_to_the_rig_entry_flattened(toy):
    calls, rows, handled, cands = toy("rig")
    assert [c[0] for c in calls] == ["orbm_create", "orbm_create_new_map_points_rig"]
    h = dict(zip(calls[1][1::2], calls[1][2::2]))
    assert h["handle"] == "1" and h["n_neighbours"] == "3" and h["inertial"] == "1" and h["far_points"] == "1" and float.fromhex(h["th_far"]) == 7.5
    assert float.fromhex(h["scale_factor_1"]) == float(f32(1.2)) and h["match12"] == "NULL" and h["skipped"] == "set"
    for q, name in enumerate(("kf1", "nb0", "nb1", "nb2")):
        R, t = T[q]
        assert rows[name + ".n_nleft_nlevels"] == [5.0, 3.0, 3.0]
        assert rows[name + ".has_mp"] == [1.0, 0.0, 0.0, 1.0, 0.0] and rows[name + ".stereo"] is None and rows[name + ".angle"] is None
        # the raw key points of mvKeys then mvKeysRight (mvKeysUn holds 900 / 800 / octave 2)
        assert rows[name + ".x"] == [100.5 + q, 110.5 + q, 120.5 + q, 300.0 + q, 301.0 + q] and rows[name + ".y"] == [50.25, 51.25, 52.25, 250.0, 249.0]
        assert rows[name + ".octave"] == [0.0, 1.0, 0.0, 2.0, 1.0] and rows[name + ".desc"] == _desc(5, q)
        assert rows[name + ".fv.node"] == [3.0, 8.0] and rows[name + ".fv.offset"] == [0.0, 2.0, 5.0] and rows[name + ".fv.feat"] == [0.0, 3.0, 1.0, 2.0, 4.0]
        # index 0 GetPose / GetCameraCenter, index 1 GetRightPose = Trl * Tcw / GetRightCameraCenter
        tr = t + TRL[q]
        assert rows[name + ".Rcw"] == list(R.reshape(-1)) * 2
        assert rows[name + ".tcw"] == list(t) + list(tr)
        assert rows[name + ".Ow"] == list(-(R.T @ t)) + list(-(R.T @ tr))
        assert rows[name + ".cam"] == flat32(CAMS1 if q == 0 else CAMS2)
        assert rows[name + ".mb"] == [0.125 + 0.0625 * q]
        assert rows[name + ".level_sigma2"] == [1.0, float(f32(1.44)), float(f32(2.0736))] and rows[name + ".scale_factors"] == [1.0, float(f32(1.2)), float(f32(1.44))]
    # the four pose products per neighbour: T1w*Tw2, T1w*Twr2, Tr1w*Tw2, Tr1w*Twr2 (ll, lr, rl, rr)
    inv = lambda R, t: (R.T, -(R.T @ t))
    left1, right1 = (T[0][0], T[0][1]), (T[0][0], T[0][1] + TRL[0])
    for j in range(3):
        R2, t2 = T[1 + j]
        w2, wr2 = inv(R2, t2), inv(R2, t2 + TRL[1 + j])
        want_R, want_t = [], []
        for (Ra, ta), (Rb, tb) in ((left1, w2), (left1, wr2), (right1, w2), (right1, wr2)):
            want_R += list((Ra @ Rb).reshape(-1)); want_t += list(Ra @ tb + ta)
        assert rows["pair%d.R12" % j] == [float(v) for v in want_R] and rows["pair%d.t12" % j] == [float(v) for v in want_t], j
        assert rows["pair%d.cam" % j] == flat32(CAMS1 + CAMS2) and rows["pair%d.coarse" % j] == [1.0]
    # the fake: features 2 and 4 by neighbour 0, features 0 and 1 by neighbour 2, neighbour 1 skipped.  Creation order: (neighbour, idx1) ascending
    assert handled == ["handled", "1", "candidates", "4", "skipped", "0", "1", "0"]
    assert [c[:4] for c in cands] == [["2", "0", "3", "0"], ["4", "0", "1", "0"], ["0", "2", "0", "0"], ["1", "2", "4", "0"]]
    for c in cands:
        i = int(c[0])
        vals = [float.fromhex(v) for v in c[4:]]
        assert vals == [10.0 * i, 10.0 * i + 1, 10.0 * i + 2, 0.125 * i, 0.125 * (i + 1), 0.125 * (i + 2), 100.0 + i, 50.0 + i]


def test_conventional_key_frames_keep_the_existing_entry(toy):
    calls, _, handled, cands = toy("conv")
    assert [c[0] for c in calls] == ["orbm_create", "orbm_create_new_map_points"]
    assert calls[1][1:] == ["handle", "1", "n1", "4", "n_neighbours", "3"]
    assert handled[:4] == ["handled", "1", "candidates", "0"] and handled[4:] == ["skipped", "0", "0", "0"] and not cands


@pytest.mark.parametrize("scenario", ["mixed_kf1", "mixed_neighbour", "pinhole_rig"])
def test_mixed_pairs_and_other_rigs_are_refused_before_any_call(toy, scenario):
    """false, no candidates, no C call at all (not even a handle): the caller falls back to the reference's loop"""
    calls, _, handled, cands = toy(scenario)
    assert calls == [] and handled[:4] == ["handled", "0", "candidates", "0"] and not cands
