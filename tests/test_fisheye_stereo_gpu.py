"""Frame::ComputeStereoFishEyeMatches on the device (include/orbslam3_hip_fisheye.h, csrc/stereo_fisheye.hip) against the numpy
restatement tests/fisheye_stereo_reference.py on the cases of tests/fisheye_stereo_cases.py: the k-NN search as integers, the
many-to-one rule, the geometry under the borderline band and the tolerance that the cases file derives, the whole function, the
device-resident batch bit for bit against the host entry, and the adapter on a toy frame."""
import importlib

import numpy as np
import pytest

import fisheye_stereo_cases as cases
import fisheye_stereo_reference as ref
import shim_fisheye_common as common

pytestmark = pytest.mark.gpu

OUTPUTS = ("left_to_right", "right_to_left", "depth", "p3d", "knn_right", "knn_d0", "knn_d1")


@pytest.fixture(scope="module")
def capi(pkg):
    return importlib.import_module("orb_slam3-1_amd.capi")


@pytest.fixture(scope="module")
def matcher(pkg):
    m = pkg.Matcher()
    yield m
    m.close()


def _run(matcher, capi, c):
    return matcher.stereo_fisheye(c["rig"], common.keypoints(capi, c["kps_l"]), c["desc_l"], c["mono_l"], common.keypoints(capi, c["kps_r"]), c["desc_r"], c["mono_r"],
                                  cases.LEVEL_SIGMA2)


@pytest.fixture(scope="module")
def frames(matcher, capi):
    """the host entry on every frame case, once"""
    return {name: _run(matcher, capi, cases.frame_case(name)) for name in cases.FRAME_CASES}


def test_knn_is_exact(matcher, capi, pkg):
    chunk = pkg.ORBM_FISHEYE_KNN_CHUNK
    assert chunk + 1 <= 300
    shapes = [(65, r) for r in (0, 1, 2, 63, 64, 65, chunk + 1)] + [(l, chunk + 1) for l in (0, 1, 65, 130)] + [(130, 2 * chunk + 3)]
    nb = len(cases.BOUNDARY_RATIOS)
    seen_boundary = 0
    for lap_l, lap_r in shapes:
        for mono_l, mono_r in ((3, 5), (0, 0)):
            dl, ml, dr, mr = cases.knn_case(lap_l, lap_r, mono_l, mono_r)
            kl, kr = np.zeros((len(dl), 3)), np.zeros((len(dr), 3))
            kl[:, :2] = 200.0; kr[:, :2] = 210.0
            got = matcher.stereo_fisheye(cases.RIGS["tumvi"], common.keypoints(capi, kl), dl, ml, common.keypoints(capi, kr), dr, mr, cases.LEVEL_SIGMA2)
            d0, d1, idx, ok = ref.knn2(dl[ml:], dr[mr:])
            want_right = np.full(len(dl), -1, np.int32)
            want_right[ml:][ok] = idx[ok] + mr
            want_d0, want_d1 = np.full(len(dl), -1, np.int32), np.full(len(dl), -1, np.int32)
            want_d0[ml:], want_d1[ml:] = d0, d1
            where = "lapping %d x %d, mono %d / %d" % (lap_l, lap_r, ml, mr)
            assert np.array_equal(got["knn_d0"], want_d0) and np.array_equal(got["knn_d1"], want_d1), where
            assert np.array_equal(got["knn_right"], want_right), where
            assert (got["left_to_right"][got["knn_right"] < 0] == -1).all(), where
            if lap_l >= nb + 3 and lap_r >= 2 * (nb + 3):                        # the boundary ratios and the duplicates are in
                _, _, want = cases.boundary_descriptors()
                assert np.array_equal(np.stack([got["knn_d0"], got["knn_d1"]], 1)[ml:ml + nb + 3], want), where
                assert np.array_equal(got["knn_right"][ml:ml + nb] >= 0, ref.ratio_ok(want[:nb, 0], want[:nb, 1])), where
                assert (got["knn_right"][ml + nb:ml + nb + 3] == -1).all(), where       # a tie: no match
                seen_boundary += 1
    assert seen_boundary >= 4


def test_many_left_onto_one_right_keeps_the_highest_left_index_and_runs_repeat(matcher, capi, frames):
    for name in ("frame_a", "frame_c"):
        c, got = cases.frame_case(name), frames[name]
        onto, frm = c["many_onto"], c["many_from"]
        assert (got["left_to_right"][frm] == onto).all() and got["right_to_left"][onto] == max(frm), name
        again = _run(matcher, capi, c)
        for k in OUTPUTS:
            assert got[k].tobytes() == again[k].tobytes(), (name, k)
        assert got["matches"] == again["matches"] == (got["left_to_right"] >= 0).sum()


@pytest.mark.parametrize("name", cases.PAIR_CASES)
def test_triangulate_matches_against_the_faithful_evaluation(pkg, name):
    c = cases.pair_case(name)
    code, p3d = pkg.kb8_triangulate_matches(c["rig"], c["pts_l"], c["pts_r"], c["sigma_l"], c["sigma_r"])
    cases.check_geometry(name, code, p3d, cases.pair_reference(name, "faithful"), cases.pair_reference(name, "exact"))
    code2, p3d2 = pkg.kb8_triangulate_matches(c["rig"], c["pts_l"], c["pts_r"], c["sigma_l"], c["sigma_r"])
    assert code.tobytes() == code2.tobytes() and p3d.tobytes() == p3d2.tobytes()


@pytest.mark.parametrize("name", cases.FRAME_CASES)
def test_whole_function_against_the_reference(frames, name):
    c, got, want = cases.frame_case(name), frames[name], cases.frame_reference(name, "faithful")
    exact = cases.frame_reference(name, "exact")["geo"]
    n_l, n_r = len(c["kps_l"]), len(c["kps_r"])
    assert [len(got[k]) for k in OUTPUTS] == [n_l, n_r, n_l, n_l, n_l, n_l, n_l]
    for k in ("knn_right", "knn_d0", "knn_d1"):
        assert np.array_equal(got[k], want[k]), k
    # the geometry of the survivors under the rules of the diagnostic: a survivor the device accepted carries its depth as the code
    left = want["geo"]["left"]
    band = ref.borderline(exact)
    assert band.sum() <= cases.BORDERLINE_CAP * max(len(band), 1)
    acc_got, acc_want = got["left_to_right"][left] >= 0, want["left_to_right"][left] >= 0
    assert np.array_equal(acc_got[~band], acc_want[~band])
    both = acc_got & acc_want
    if both.any():
        scale = np.linalg.norm(want["p3d"][left[both]].astype(np.float64), axis=1)
        dp = np.linalg.norm(got["p3d"][left[both]].astype(np.float64) - want["p3d"][left[both]], axis=1) / scale
        dz = np.abs(got["depth"][left[both]].astype(np.float64) - want["depth"][left[both]]) / scale
        print("%s: %d survivors, %d borderline, %d accepted, worst point %.3g depth %.3g (allowed %.3g)" % (name, len(left), band.sum(), both.sum(), dp.max(), dz.max(), cases.P3D_RTOL))
        assert (dp <= cases.P3D_RTOL).all() and (dz <= cases.P3D_RTOL).all()
        assert np.array_equal(got["depth"][left[both]], got["p3d"][left[both], 2])          # the depth is z1 of the point
    assert np.array_equal(got["left_to_right"][left[acc_got]], want["knn_right"][left[acc_got]])
    # unmatched entries: -1 / -1 / -1.0 / zeros; the right side holds the highest accepted left index
    off = got["left_to_right"] < 0
    assert (got["depth"][off] == -1.0).all() and not got["p3d"][off].any() and (got["depth"][~off] > 1e-4).all()
    rtl = np.full(n_r, -1, np.int32)
    for i in np.nonzero(~off)[0]:
        rtl[got["left_to_right"][i]] = i
    assert np.array_equal(got["right_to_left"], rtl)
    if not band.any():
        assert np.array_equal(got["left_to_right"], want["left_to_right"]) and np.array_equal(got["right_to_left"], want["right_to_left"])
    # the offsets: nothing outside the lapping areas is matched
    assert (got["left_to_right"][:c["mono_l"]] == -1).all() and (got["right_to_left"][:c["mono_r"]] == -1).all()
    assert (got["left_to_right"][~off] >= c["mono_r"]).all()
    assert got["matches"] == (~off).sum()


def test_frames_hold_matches_and_offsets_differ(frames):
    a = cases.frame_case("frame_a")
    assert a["mono_l"] > 0 and a["mono_r"] > 0 and a["mono_l"] != a["mono_r"] and frames["frame_a"]["matches"] >= 30
    for name in ("frame_nolap_l", "frame_nolap_r", "frame_one_r"):
        assert frames[name]["matches"] == 0 and (frames[name]["knn_right"] == -1).all()


def test_device_batch_equals_the_host_entry_bit_for_bit(matcher, capi, frames):
    import torch
    names = ("frame_a", "frame_b", "frame_c")
    cap, B = 256, len(names)
    dev = torch.device("cuda", 0)
    kps = {s: np.zeros((B, cap), capi.KP_DTYPE) for s in "lr"}
    desc = {s: np.zeros((B, cap, 32), np.uint8) for s in "lr"}
    n = {s: np.zeros(B, np.int32) for s in "lr"}
    mono = {s: np.zeros(B, np.int32) for s in "lr"}
    rs = np.random.RandomState(3)
    for b, name in enumerate(names):
        c = cases.frame_case(name)
        for s in "lr":
            k = common.keypoints(capi, c["kps_" + s])
            assert len(k) < cap
            n[s][b], mono[s][b] = len(k), c["mono_" + s]
            kps[s][b, :len(k)] = k
            desc[s][b] = rs.randint(0, 256, (cap, 32))                  # what lies beyond n must not be read as a descriptor
            desc[s][b, :len(k)] = c["desc_" + s]
            kps[s][b, len(k):]["octave"] = 99                           # ... nor as a key point
    up = lambda a: torch.from_numpy(a.view(np.uint8).reshape(-1).copy()).to(dev)
    d = {k + s: up(v[s]) for k, v in (("kps", kps), ("desc", desc), ("n", n), ("mono", mono)) for s in "lr"}
    fill = dict(left_to_right=np.int32(-7), right_to_left=np.int32(-8), depth=np.float32(123.0), p3d=np.float32(7.5), knn_right=np.int32(-9),
                knn_d0=np.int32(-10), knn_d1=np.int32(-11))
    host = {k: np.full((B, cap, 3) if k == "p3d" else (B, cap), v) for k, v in fill.items()}
    out = {k: up(v) for k, v in host.items()}
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream().cuda_stream
    p = lambda t: t.data_ptr()
    matcher.stereo_fisheye_device(cases.RIGS["tumvi"], B, cap, p(d["kpsl"]), p(d["descl"]), p(d["nl"]), p(d["monol"]), p(d["kpsr"]), p(d["descr"]), p(d["nr"]),
                                  p(d["monor"]), cases.LEVEL_SIGMA2, p(out["left_to_right"]), p(out["right_to_left"]), p(out["depth"]), p(out["p3d"]),
                                  p(out["knn_right"]), p(out["knn_d0"]), p(out["knn_d1"]), stream)
    torch.cuda.synchronize()
    got = {k: out[k].cpu().numpy().view(host[k].dtype).reshape(host[k].shape) for k in OUTPUTS}
    for b, name in enumerate(names):
        if cases.frame_case(name)["rig"] is not cases.RIGS["tumvi"]:
            continue                                                    # one rig per call: frame_c is compared below, with its own
        for k in OUTPUTS:
            m = n["r"][b] if k == "right_to_left" else n["l"][b]
            assert got[k][b, :m].tobytes() == frames[name][k].tobytes(), (name, k)
            assert (got[k][b, m:] == fill[k]).all(), (name, k, "entries beyond n were written")
    # frame_c's rig, the diagnostics left out: the same bits, and the untouched rows stay untouched
    out2 = {k: up(host[k]) for k in OUTPUTS[:4]}
    torch.cuda.synchronize()
    matcher.stereo_fisheye_device(cases.RIGS["diverging"], B, cap, p(d["kpsl"]), p(d["descl"]), p(d["nl"]), p(d["monol"]), p(d["kpsr"]), p(d["descr"]), p(d["nr"]),
                                  p(d["monor"]), cases.LEVEL_SIGMA2, p(out2["left_to_right"]), p(out2["right_to_left"]), p(out2["depth"]), p(out2["p3d"]), stream=stream)
    torch.cuda.synchronize()
    b = names.index("frame_c")
    for k in OUTPUTS[:4]:
        g = out2[k].cpu().numpy().view(host[k].dtype).reshape(host[k].shape)
        m = n["r"][b] if k == "right_to_left" else n["l"][b]
        assert g[b, :m].tobytes() == frames["frame_c"][k].tobytes(), k
        assert (g[b, m:] == fill[k]).all(), k


def test_adapter_on_the_toy_frame_equals_the_host_entry(frames, capi, tmp_path):
    exe = common.build_toy(tmp_path, real=True)
    for name, scenario in (("frame_a", "rig"), ("frame_c", "noncontiguous")):
        out = common.run_toy(exe, scenario, common.case_bytes(capi, cases.frame_case(name)), tmp_path)
        got = frames[name]
        assert out["reference_calls"] == 0 and out["close"] == 0
        assert np.array_equal(out["left_to_right"], got["left_to_right"]) and np.array_equal(out["right_to_left"], got["right_to_left"])
        assert out["depth"].tobytes() == got["depth"].tobytes() and out["p3d"].tobytes() == got["p3d"].tobytes()
        assert (out["u_right"] == -1).all()
