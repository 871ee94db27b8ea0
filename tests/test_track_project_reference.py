"""The HOST build of csrc/track_project_geometry.h (the text the projection kernels compile, through
tests/track_project_geometry_check.cpp) against the numpy restatement of the reference, tests/track_project_reference.py: frame pose
records, Frame::isInFrustum and the last-frame projection on random cases and on rows built ON every decision boundary.  Exact
equality, except levels on rows whose log quotient is within 2^-16 of an integer (glibc's logf and numpy's float32 log may differ in
the last bit there).  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import track_project_cases as TC
import track_project_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tpj") / "track_project_geometry_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "track_project_geometry_check.cpp")])
    return exe


def run_host(exe, tmp, mode, case, normalise):
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(TC.pack(mode, case, normalise))
    subprocess.check_call([exe, src, dst])
    with open(dst, "rb") as f:
        return TC.unpack(mode, case, f.read())


def test_reference_on_the_boundary_rows():
    """the reference itself decides the hand-built rows as they were built, and the -0 rows really reach the depth gate with -0"""
    case = TC.frustum_boundary_case()
    ref = R.frustum(case)
    TC.check_frustum_boundary_rows(ref, case)
    names = [r[0] for r in TC.FRUSTUM_ROWS]
    b = case["boundary_frame"]
    for name in TC.MINUS_ZERO_ROWS:
        z = ref["PcZ"][b, names.index(name)]
        assert z == 0 and np.signbit(z), name
    assert np.isnan(ref["u"][b, names.index("z_plus0_x0")]) and ref["valid"][b, names.index("z_plus0_x0")] == 1
    # rows that fail after the bounds test keep the projection the reference had stored
    i = names.index("farther_than_max")
    assert ref["valid"][b, i] == 0 and ref["u"][b, i] == 320 and ref["v"][b, i] == 240
    assert list(ref["n_to_match"][:2]) == [0, 1]
    last = TC.last_boundary_case()
    TC.check_last_boundary_rows(R.project_last(last), last)
    # every gate rejects somewhere in the random cases, and plenty of rows survive
    for c in TC.random_frustum_cases():
        r = R.frustum(c)
        share = r["valid"].sum() / max(int(c["n"].sum()), 1)
        print("in view: %.3f of the live rows" % share)
        assert 0.1 < share < 0.7 and (r["valid"].sum(1) == r["n_to_match"]).all()


def test_pose_records(check_exe, tmp_path):
    poses = TC.pose_cases()
    case =TC.ST.make_last_frame_case(43, len(poses), 8, poses=poses)
    for normalise in (0, 1):
        rec, _ = run_host(check_exe, tmp_path, 1, case, normalise)
        fp = R.frame_pose(poses, normalise)
        np.testing.assert_array_equal(rec, R.frame_pose_record(fp))
        if normalise:                                   # and it is a pose: R orthonormal, Ow = -R^T t
            Rm = fp["Rcw"].reshape(-1, 3, 3).astype(np.float64)
            assert np.abs(Rm @ Rm.transpose(0, 2, 1) - np.eye(3)).max() < 1e-6
            assert np.abs(fp["Ow"] + np.einsum("bji,bj->bi", Rm, fp["tcw"].astype(np.float64))).max() < 1e-5
    assert not np.array_equal(R.frame_pose(poses, 0)["q"], R.frame_pose(poses, 1)["q"])


def test_frustum_host_build(check_exe, tmp_path):
    case = TC.frustum_boundary_case()
    _, out = run_host(check_exe, tmp_path, 0, case, 1)
    TC.check_frustum_boundary_rows(out, case)           # the hand-built rows: exact, no tie rule
    TC.assert_frustum_equal(out, R.frustum(case), case["cam"]["n_levels"], what="boundaries")
    for k, c in enumerate(TC.random_frustum_cases()):
        _, out = run_host(check_exe, tmp_path, 0, c, 1)
        TC.assert_frustum_equal(out, R.frustum(c), c["cam"]["n_levels"], max_tie_share=0.001, what="random %d" % k)


def test_last_projection_host_build(check_exe, tmp_path):
    case = TC.last_boundary_case()
    _, out = run_host(check_exe, tmp_path, 1, case, 1)
    TC.check_last_boundary_rows(out, case)
    TC.assert_last_equal(out, R.project_last(case), "boundaries")
    for k, c in enumerate(TC.random_last_cases()):
        _, out = run_host(check_exe, tmp_path, 1, c, 1)
        TC.assert_last_equal(out, R.project_last(c), "random %d" % k)
    # the quaternion form is what the reference computes, and it is not Rcw*x bit for bit
    a, b = R.project_last(case), R.project_last(case, through_matrix=True)
    assert (a["x3Dc"][1] != b["x3Dc"][1]).any()


def test_level_tie_rule_excuses_little():
    """float32 log against float64 log rounded to float on random ratios: the tie band holds well under 0.1 % of the rows"""
    rs = np.random.RandomState(9)
    ratio = np.exp(rs.uniform(np.log(0.8), np.log(5.0), 200000)).astype(np.float32)
    lsf = np.log(np.float32(1.2))
    q = np.log(ratio.astype(np.float64)) / np.float64(lsf)
    tie = np.abs(q - np.rint(q)) <= R.LEVEL_TIE * np.maximum(1.0, np.abs(q))
    assert tie.mean() < 0.001
    a = np.ceil(np.log(ratio) / lsf); b = np.ceil(np.log(ratio.astype(np.float64)).astype(np.float32) / lsf)
    assert (a[~tie] == b[~tie]).all()
