"""The plain-loop restatements of the rig SearchByBoW / SearchForTriangulation (tests/rig_bow_reference.py), the calls of
tests/rig_bow_cases.py and the host build of the geometry path of k_tri_rig (tests/rig_bow_geometry_check.cpp, compiled with
-fsanitize=address,undefined and run directly) against each other.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import fisheye_stereo_cases as fsc
import fisheye_stereo_reference as fsr
import matcher_reference as mref
import rig_bow_cases as cases
import rig_bow_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(cases.bow_hand_cases()))
def test_hand_built_bow_case_gives_the_outcome_written_next_to_it(name):
    c = cases.bow_hand_cases()[name]
    n, m = ref.search_by_bow_rig(nnratio=c["nnratio"], check_ori=c["check_ori"], **c["call"])
    assert m.tolist() == c["want_match"].tolist() and n == c["want_n"]


def test_the_issues_ratio_example_passes_in_float_and_an_exact_equality_does_not():
    f = np.float32
    assert f(30) < f(0.6) * f(50) and not f(25) < f(0.5) * f(50) and not f(31) < f(0.6) * f(50)


@pytest.mark.parametrize("name", sorted(cases.tri_hand_cases()))
def test_hand_built_triangulation_case_gives_the_outcome_written_next_to_it(name):
    c = cases.tri_hand_cases()[name]
    n, m = ref.search_for_triangulation_rig(c["call"], c["only_stereo"], c["coarse"], c["check_ori"])
    assert m.tolist() == c["want_match"].tolist() and n == c["want_n"]
    if not c["coarse"]:
        assert not ref.undecided(c["call"]).any(), "a hand-built case may not hold a borderline survivor"


def test_record_cases_are_accepted_under_their_own_record_only():
    for name, c in cases.tri_hand_cases().items():
        if "only_record" not in c:
            continue
        s = c["call"]
        sv = ref.survivors(s)
        assert len(sv) == 1
        for other in range(4):
            # the same two pixels judged under record `other`: move the features to the sides that select it
            k1 = dict(s["kf1"], n_left=0 if other >> 1 else 1)
            k2 = dict(s["kf2"], n_left=0 if other & 1 else 1)
            t = dict(s, kf1=k1, kf2=k2)
            g = ref.gate(t, sv)
            e = ref.gate(t, sv, fsr.EXACT)
            assert int(g["sel"][0]) == other and not fsr.borderline(e)[0]
            assert bool(np.float32(g["code"][0]) > ref.GATE_Z) == (other == c["only_record"]), (name, other, g["code"])


def test_octave_case_needs_the_sigmas_of_its_own_two_levels():
    s = cases.tri_hand_cases()["octave_sigmas"]["call"]
    sv = ref.survivors(s)
    own = ref.gate(s, sv)
    assert np.float32(own["code"][0]) > ref.GATE_Z
    # both errors lie above the level-0 gate: indexing either sigma table with 0, or with the other key point's octave where that
    # is the smaller one, rejects the pair
    assert own["e1"][0] > fsr.CHI2 * cases.LEVEL_SIGMA2[0] and own["e2"][0] > fsr.CHI2 * cases.LEVEL_SIGMA2[0]
    for o1, o2 in ((0, 5), (6, 0), (0, 0)):
        t = dict(s, kf1=dict(s["kf1"], octave=np.array([o1], np.int32)), kf2=dict(s["kf2"], octave=np.array([o2], np.int32)))
        assert not np.float32(ref.gate(t, sv)["code"][0]) > ref.GATE_Z, (o1, o2)


def test_with_every_slot_on_the_left_the_rig_loop_is_the_monocular_one():
    calls = [c for c, _ in cases.bow_random_cases().values()] + [cases.bow_shape_cases()[k][0] for k in ("n_left_all", "node_17", "node_65")]
    differ = 0
    for call in calls:
        for ori in (False, True):
            mono = dict(call); mono.pop("n_left")
            a = ref.search_by_bow_rig(nnratio=cases.NNRATIO, check_ori=ori, **dict(call, n_left=len(call["dF"])))
            b = mref.search_by_bow(nnratio=cases.NNRATIO, check_ori=ori, **mono)
            assert a[0] == b[0] and np.array_equal(a[1], b[1])
            c = ref.search_by_bow_rig(nnratio=cases.NNRATIO, check_ori=ori, **call)
            differ += int(not np.array_equal(c[1], b[1]))
    assert differ > 0, "the split calls must differ from the monocular reading somewhere, or they test nothing"


def test_set_function_reading_of_the_candidate_loop():
    """min of (dist << 16) | (0xFFFF - position) over the passing survivors is the sequential loop's winner"""
    for name in cases.RANDOM_TRI:
        s = cases.tri_random_case(name)
        sv = ref.survivors(s)
        g = ref.gate(s, sv)
        best = {}
        for (i1, i2, d, pos), code in zip(sv, g["code"]):
            if np.float32(code) > ref.GATE_Z:
                key = (d << 16) | (0xFFFF - pos)
                if key < best.get(i1, (1 << 32, -1))[0]:
                    best[i1] = (key, i2)
        m = np.full(len(s["kf1"]["x"]), -1, np.int32)
        for i1, (_, i2) in best.items():
            m[i1] = i2
        assert np.array_equal(m, cases.tri_random_expected(name)[1]), name


def test_borderline_cap_holds_for_every_random_triangulation_case():
    for name in cases.RANDOM_TRI:
        n, m, und = cases.tri_random_expected(name)
        print("%s: %d features, %d matched, %d undecided" % (name, len(m), n, und.sum()))
        assert und.sum() <= fsc.BORDERLINE_CAP * len(und), "%s: %d of %d key-frame-1 features are undecided" % (name, und.sum(), len(und))
        assert n >= 0.3 * (len(m) - 40) or len(m) < 60, "%s: the scene must produce matches (%d of %d)" % (name, n, len(m))


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("rig_bow_geometry")
    exe = str(d / "rig_bow_geometry_check")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "orb_slam3-1_amd", "csrc"), "-o", exe,
                           os.path.join(ROOT, "tests", "rig_bow_geometry_check.cpp")])

    def run(s, pairs):
        k1, k2 = s["kf1"], s["kf2"]
        rec = np.zeros(len(pairs), np.dtype([("sel", np.int32), ("q", np.float32, 6)]))
        for r, (i1, i2, _, _) in zip(rec, pairs):
            r["sel"] = 2 * int(i1 >= k1["n_left"]) + int(i2 >= k2["n_left"])
            r["q"] = (k1["x"][i1], k1["y"][i1], k2["x"][i2], k2["y"][i2], s["sigma2_1"][k1["octave"][i1]], s["sigma2_2"][k2["octave"][i2]])
        with open(d / "in.bin", "wb") as f:
            for rig in ref.pair_rigs(s["geom"]):
                f.write(fsc.rig_floats(rig).tobytes())
            f.write(np.int32(len(pairs)).tobytes()); f.write(rec.tobytes())
        r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
        raw = open(d / "out.bin", "rb").read()
        return np.frombuffer(raw[:4 * len(pairs)], np.float32), np.frombuffer(raw[4 * len(pairs):], np.uint8).astype(bool)
    return run


def test_host_build_of_the_gate_agrees_with_the_python_evaluation(host_check):
    calls = [(n, cases.tri_random_case(n)) for n in cases.RANDOM_TRI] + [(n, c["call"]) for n, c in cases.tri_hand_cases().items()]
    seen = np.zeros(4, int)
    for name, s in calls:
        sv = ref.survivors(s)
        if not sv:
            continue
        code, ok = host_check(s, sv)
        f, e = ref.gate(s, sv), ref.gate(s, sv, fsr.EXACT)
        band = fsr.borderline(e)
        want = f["code"].astype(np.float32) > ref.GATE_Z
        print("%s: %d survivors, %d borderline, %d pass" % (name, len(sv), band.sum(), want.sum()))
        assert np.array_equal(ok, code > ref.GATE_Z)
        assert np.array_equal(ok[~band], want[~band]), name
        assert np.array_equal(fsr.outcome(code)[~band], fsr.outcome(f["code"])[~band]), name
        seen += np.bincount(f["sel"], minlength=4)
    assert (seen > 20).all(), "every record must be exercised: %s" % seen
