"""The numpy restatement tests/track_project_rig_reference.py on its own (hand-built rows decide as they were built; few rows of
the random scenes hang on a guard band), and the HOST build of csrc/track_project_rig_geometry.h (the text the rig projection
kernels compile, through tests/track_project_rig_geometry_check.cpp) against it.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import track_project_rig_cases as TC
import track_project_rig_reference as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPEN_CAP = 0.05


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("tpr") / "track_project_rig_geometry_check")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unknown-pragmas", "-I", os.path.join(ROOT, "include"),
                           "-o", exe, os.path.join(ROOT, "tests", "track_project_rig_geometry_check.cpp")])
    return exe


def run_host(exe, tmp, mode, case, normalise=1):
    src, dst = os.path.join(str(tmp), "in.bin"), os.path.join(str(tmp), "out.bin")
    with open(src, "wb") as f:
        f.write(TC.pack(mode, case, normalise))
    subprocess.check_call([exe, src, dst])
    with open(dst, "rb") as f:
        return TC.unpack(mode, case, f.read())


def test_reference_decides_the_hand_built_rows():
    case = TC.frustum_hand_case()
    ref = RR.frustum(case)
    TC.check_frustum_hand_rows(ref, case)
    k = len(TC.FRUSTUM_ROWS)
    assert not ref["open"][0, :k].any()                 # none of them hangs on a guard band
    names = [r[0] for r in TC.FRUSTUM_ROWS]
    for name, side in (("left_z_minus0", "left"), ("right_z_minus0", "right")):
        z = ref[side]["PcZ"][0, names.index(name)]
        assert z == 0 and np.signbit(z), name            # the row really reaches the depth gate with -0
    for name, side in (("left_z_smallest_negative", "left"), ("right_z_smallest_negative", "right")):
        assert ref[side]["PcZ"][0, names.index(name)] == TC.TINY_NEG, name
    assert np.isnan(ref["left"]["level_q"][0, names.index("level_nan")])
    seen = (ref["in_view"] != 0) | (ref["in_view_r"] != 0)
    assert (ref["n_to_match"] == seen.sum(1)).all() and seen[0, :k].sum() == TC.N_TO_MATCH_ROWS
    both = (ref["in_view"][0, :k] != 0) & (ref["in_view_r"][0, :k] != 0)
    assert both.sum() >= 5 and (seen[0, :k] & ~both).sum() >= 4        # counted once either way
    for name, c, seen_l, seen_r in TC.bounds_cases():
        r = RR.frustum(c)
        TC.check_bounds_case(r, seen_l, seen_r, name)
        assert not r["open"][0, :2].any(), name
    last = TC.last_hand_case()
    rl = RR.project_last(last)
    TC.check_last_hand_rows(rl, last)
    assert not rl["open"][0, :len(TC.LAST_ROWS)].any()
    # uv_r comes from the LEFT camera's parameters: the right camera's would land pixels away
    alt = RR.project_last(last, right_camera_for_uvr=True)
    i = [r[0] for r in TC.LAST_ROWS].index("in_view")
    assert abs(float(rl["proj_u_r"][0, i]) - float(alt["proj_u_r"][0, i])) > 5


def test_few_rows_of_the_random_scenes_are_open():
    for k, c in enumerate(TC.random_frustum_cases()):
        assert c["skip"].shape[0] <= 3 and c["skip"].shape[1] <= 200
        r = RR.frustum(c)
        live = int(r["live"].sum())
        l, rt = r["left"]["valid"], r["right"]["valid"]
        print("frustum %d: %d live rows, left only %d, right only %d, both %d, neither %d, open %d" % (
            k, live, (l & ~rt).sum(), (rt & ~l).sum(), (l & rt).sum(), (r["live"] & ~l & ~rt).sum(), r["open"].sum()))
        assert r["open"].sum() <= OPEN_CAP * r["open"].size
        # the generator puts points in front of one camera only, of both and of neither
        assert min((l & ~rt).sum(), (rt & ~l).sum(), (l & rt).sum(), (r["live"] & ~l & ~rt).sum()) >= 0.03 * live
        for side in ("left", "right"):
            reached = {name: int((reach & r["live"]).sum()) for name, _, _, reach in r[side]["gates"].items}
            assert reached["view_cos"] > 0.05 * live and reached["depth"] == live, (side, reached)
    for k, c in enumerate(TC.random_last_cases()):
        r = RR.project_last(c)
        print("last %d: %d valid of %d, open %d" % (k, r["valid"].sum(), r["valid"].size, r["open"].sum()))
        assert r["open"].sum() <= OPEN_CAP * r["open"].size and r["valid"].sum() > 0.1 * r["valid"].size


def test_pose_records(check_exe, tmp_path):
    poses = TC.pose_cases()
    case = TC.ST.make_rig_last_frame_case(43, len(poses), 8, poses=poses)
    for normalise in (0, 1):
        rec, _ = run_host(check_exe, tmp_path, 1, case, normalise)
        rp = RR.rig_frame_pose(case["cam"], poses, normalise)
        np.testing.assert_array_equal(rec, RR.rig_frame_pose_record(rp))
        if normalise:                                   # and it is a rig: Rwc = Rcw^T, the right camera's centre is tlr seen from the world
            Rcw = rp["left"]["Rcw"].reshape(-1, 3, 3).astype(np.float64); Rwc = rp["Rwc"].reshape(-1, 3, 3).astype(np.float64)
            assert np.abs(Rwc - Rcw.transpose(0, 2, 1)).max() < 1e-6
            Rr = rp["R_r"].reshape(-1, 3, 3).astype(np.float64)
            assert np.abs(rp["Ow_r"] + np.einsum("bji,bj->bi", Rr, rp["t_r"].astype(np.float64))).max() < 1e-5
    # mRwc is the matrix of the renormalised conjugate, not the transpose of Rcw bit for bit
    rp = RR.rig_frame_pose(case["cam"], poses, 1)
    assert (rp["Rwc"].reshape(-1, 3, 3) != rp["left"]["Rcw"].reshape(-1, 3, 3).transpose(0, 2, 1)).any()


def test_frustum_host_build(check_exe, tmp_path):
    case = TC.frustum_hand_case()
    _, out = run_host(check_exe, tmp_path, 0, case)
    TC.check_frustum_hand_rows(out, case)
    TC.compare_frustum(out, RR.frustum(case), case["cam"]["n_levels"], "hand-built")
    for name, c, seen_l, seen_r in TC.bounds_cases():
        _, out = run_host(check_exe, tmp_path, 0, c)
        TC.check_bounds_case(out, seen_l, seen_r, name)
    for k, c in enumerate(TC.random_frustum_cases()):
        _, out = run_host(check_exe, tmp_path, 0, c)
        worst, differ = TC.compare_frustum(out, RR.frustum(c), c["cam"]["n_levels"], "random %d" % k)
        print("random %d: worst |d| / bar %.3f, %d projections differ from the reference at all" % (k, worst, differ))


def test_last_projection_host_build(check_exe, tmp_path):
    case = TC.last_hand_case()
    _, out = run_host(check_exe, tmp_path, 1, case)
    TC.check_last_hand_rows(out, case)
    TC.compare_last(out, RR.project_last(case), "hand-built")
    for k, c in enumerate(TC.random_last_cases()):
        _, out = run_host(check_exe, tmp_path, 1, c)
        worst, differ = TC.compare_last(out, RR.project_last(c), "random %d" % k)
        print("random %d: worst |d| / bar %.3f, %d projections differ from the reference at all" % (k, worst, differ))


def test_unproject_host_build(check_exe, tmp_path):
    case = TC.unproject_case()
    _, out = run_host(check_exe, tmp_path, 2, case)
    rp = RR.rig_frame_pose(case["cam"], case["pose7"], 1)
    want = RR.unproject(rp, case["points"], case["valid"], case["n"], case["world"])
    np.testing.assert_array_equal(out["world"].view(np.uint32), want.view(np.uint32))      # bit-exact: no transcendentals
    assert (want[1] == -555).all() and (want[0] != -555).any()
