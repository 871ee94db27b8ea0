"""The numpy restatement of ComputeStereoFishEyeMatches (tests/fisheye_stereo_reference.py), the synthetic cases
(tests/fisheye_stereo_cases.py) and the host build of csrc/kb8_stereo_geometry.h (tests/fisheye_geometry_check.cpp, compiled with
-fsanitize=address,undefined and run directly) against each other.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import fisheye_stereo_cases as cases
import fisheye_stereo_reference as ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_every_outcome_occurs_in_the_cases():
    total = np.zeros(6, int)
    for _, f, _ in cases.geometry_references():
        total += np.bincount(-ref.outcome(f["code"]), minlength=6)
    assert (total >= 8).all(), "outcomes accepted, -1 .. -5 occur %s times" % total


def test_borderline_pairs_stay_under_the_cap_and_the_two_evaluations_agree_outside_the_band():
    cases.assert_borderline_cap()
    for name, f, e in cases.geometry_references():
        band = ref.borderline(e)
        assert np.array_equal(ref.outcome(f["code"])[~band], ref.outcome(e["code"])[~band]), name


def test_measured_spread_is_the_recorded_one():
    spread = cases.measure_spread()
    print("largest faithful - exact spread of an accepted point: %.4g of |p3d|" % spread)
    assert 0.8 * cases.MEASURED_SPREAD <= spread <= cases.MEASURED_SPREAD
    assert cases.P3D_RTOL == 4 * cases.MEASURED_SPREAD


def test_ratio_test_at_the_exact_boundaries():
    for d0, d1 in cases.BOUNDARY_RATIOS:
        assert bool(ref.ratio_ok(d0, d1)) == (float(np.float32(d0)) < float(np.float32(d1)) * 0.7), (d0, d1)
    for k in range(1, 11):
        assert ref.ratio_ok(7 * k - 1, 10 * k) and not ref.ratio_ok(7 * k + 1, 10 * k)
    left, right, want = cases.boundary_descriptors()
    d0, d1, idx, ok = ref.knn2(left, right)
    assert np.array_equal(np.stack([d0, d1], 1), want)                  # the constructed distances are the two smallest
    nb = len(cases.BOUNDARY_RATIOS)
    assert np.array_equal(ok[:nb], ref.ratio_ok(want[:nb, 0], want[:nb, 1])) and ok[:nb].sum() >= 10
    assert np.array_equal(idx[:nb], 2 * np.arange(nb) + 1)              # the nearer descriptor was stored second


def test_duplicates_tie_and_do_not_match():
    left, right, want = cases.boundary_descriptors()
    nb = len(cases.BOUNDARY_RATIOS)
    d0, d1, _, ok = ref.knn2(left, right)
    assert np.array_equal(d0[nb:], d1[nb:]) and d0[nb] == 0 and not ok[nb:].any()
    for name in ("frame_a", "frame_c"):                                 # the duplicated right descriptors of the frames: no survivor looks at one
        c, r = cases.frame_case(name), cases.frame_reference(name)
        dr = c["desc_r"][c["mono_r"]:]
        twins = {i + c["mono_r"] for i in range(len(dr)) for j in range(len(dr)) if i != j and np.array_equal(dr[i], dr[j])}
        assert twins and not twins & set(r["knn_right"][r["knn_right"] >= 0].tolist())


def test_knn_without_two_neighbours_matches_nothing():
    rs = np.random.RandomState(5)
    d = rs.randint(0, 256, (4, 32)).astype(np.uint8)
    d0, d1, idx, ok = ref.knn2(d, d[:1])
    assert d0[0] == 0 and (d1 == -1).all() and not ok.any()
    d0, d1, idx, ok = ref.knn2(d, d[:0])
    assert (d0 == -1).all() and (idx == -1).all() and not ok.any()
    for name in ("frame_nolap_l", "frame_nolap_r", "frame_one_r"):
        r = cases.frame_reference(name)
        assert (r["left_to_right"] == -1).all() and (r["right_to_left"] == -1).all() and (r["depth"] == -1).all() and not r["p3d"].any()


def test_many_left_onto_one_right_keeps_the_highest_left_index():
    for name in ("frame_a", "frame_c"):
        c, r = cases.frame_case(name), cases.frame_reference(name)
        onto, frm = c["many_onto"], c["many_from"]
        assert len(frm) >= 4 and (r["left_to_right"][frm] == onto).all()
        assert r["right_to_left"][onto] == max(frm)
        assert c["mono_l"] != c["mono_r"] and (c["mono_l"] > 0 or c["mono_r"] > 0)


@pytest.fixture(scope="module")
def host_check(tmp_path_factory):
    d = tmp_path_factory.mktemp("fisheye_geometry")
    exe = str(d / "fisheye_geometry_check")
    subprocess.check_call(["g++", "-O1", "-g", "-ffp-contract=off", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "orb_slam3-1_amd", "csrc"), "-o", exe, os.path.join(ROOT, "tests", "fisheye_geometry_check.cpp")])

    def run(rig, pts_l, pts_r, sigma_l, sigma_r, ratios):
        n, m = len(pts_l), len(ratios)
        with open(d / "in.bin", "wb") as f:
            f.write(np.int32(n).tobytes()); f.write(cases.rig_floats(rig).tobytes())
            f.write(np.column_stack([pts_l, pts_r, sigma_l, sigma_r]).astype(np.float32).tobytes())
            f.write(np.int32(m).tobytes()); f.write(np.asarray(ratios, np.int32).reshape(m, 2).tobytes())
        r = subprocess.run([exe, str(d / "in.bin"), str(d / "out.bin")], capture_output=True, text=True)
        assert r.returncode == 0 and not r.stderr, r.stderr[-4000:]
        raw = open(d / "out.bin", "rb").read()
        out = np.frombuffer(raw[:16 * n], np.float32).reshape(n, 4)
        return out[:, 0], out[:, 1:], np.frombuffer(raw[16 * n:], np.uint8).astype(bool)
    return run


def test_host_build_of_the_shared_header_agrees_with_the_faithful_evaluation(host_check):
    ratios = [(a, b) for a in range(0, 257, 1) for b in (0, 1, 10, 20, 30, 50, 70, 90, 100, 101, 128, 200, 256)] + cases.BOUNDARY_RATIOS
    for name in cases.PAIR_CASES:
        c = cases.pair_case(name)
        code, p3d, ok = host_check(c["rig"], c["pts_l"], c["pts_r"], c["sigma_l"], c["sigma_r"], ratios)
        cases.check_geometry(name, code, p3d, cases.pair_reference(name, "faithful"), cases.pair_reference(name, "exact"))
        assert np.array_equal(ok, ref.ratio_ok([a for a, _ in ratios], [b for _, b in ratios]))
