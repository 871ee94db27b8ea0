"""HIP Frame::ComputeStereoMatches (k_stereo_match / k_stereo_median) at its exact decision boundaries: every hand-built case of
tests/stereo_boundary_cases.py through both device entries, kernel == numpy restatement (tests/stereo_reference.py) == the outcome
codes the cases state, float for float and without a tolerance.  The restatement itself is held against the C++ oracle on the
CPU by tests/test_stereo_reference.py."""
import itertools

import numpy as np
import pytest

import stereo_boundary_cases as bc
import stereo_reference as ref

pytestmark = pytest.mark.gpu

SENTINEL = np.float32(12345.0)
MATCHED = (ref.ACCEPTED, ref.ACCEPTED_CLAMPED)


@pytest.fixture(scope="module")
def rigs(pkg):
    """per geometry the two extractors after ONE extract_batch of the three sheets: sheet i is frame i"""
    out = {}
    try:
        for geom, params in bc.GEOMS.items():
            pair = []
            for side in ("left", "right"):
                ex = pkg.Extractor(*params)
                pair.append(ex)
                ex.extract_batch(np.stack([getattr(sh, side) for sh in bc.SHEETS]), (0, 0))
            out[geom] = tuple(pair)
        yield out
    finally:
        for pair in out.values():
            for ex in pair:
                ex.close()


def _check(name, want, ur, dp):
    np.testing.assert_array_equal(ur, want["u_right"], err_msg=name)
    np.testing.assert_array_equal(dp, want["depth"], err_msg=name)
    assert ur.dtype == dp.dtype == np.float32
    assert np.array_equal(ur >= 0, np.isin(want["code"], MATCHED)) and np.array_equal(ur >= 0, dp > 0), name


@pytest.mark.parametrize("geom", list(bc.GEOMS))
def test_device_pyramids_equal_the_restatements(rigs, geom):
    """the cases' expectations were computed on the oracle extractor's levels; the device must hold the same ones"""
    scale, inv_scale = bc.tables(geom)
    np.testing.assert_array_equal(rigs[geom][0].GetScaleFactors(), scale)
    np.testing.assert_array_equal(rigs[geom][0].GetInverseScaleFactors(), inv_scale)
    for sheet in range(len(bc.SHEETS)):
        for side in (0, 1):
            for level, want in enumerate(bc.pyramid(geom, sheet)[side]):
                np.testing.assert_array_equal(rigs[geom][side].pyramid_level(level, frame=sheet), want)


@pytest.mark.parametrize("name", list(bc.CASES))
def test_host_entry_equals_restatement(rigs, name):
    c = bc.CASES[name]
    want = bc.reference(name)
    assert np.array_equal(want["code"], c["want"])
    exL, exR = rigs[c["geom"]]
    ur, dp = exL.stereo_matches(exR, c["kps_l"], c["desc_l"], c["kps_r"], c["desc_r"], c["mb"], c["mbf"], frame=c["sheet"])
    _check(name, want, ur, dp)


def test_more_than_8192_keypoints_is_an_argument_error(pkg, rigs):
    exL, exR = rigs["g8"]
    c = bc.CASES["best_shift"]
    big_k = np.resize(c["kps_l"], 8193); big_d = np.resize(c["desc_l"], (8193, 32))
    for args in ((big_k, big_d, c["kps_r"], c["desc_r"]), (c["kps_l"], c["desc_l"], big_k, big_d)):
        with pytest.raises(pkg.capi.OrbxError) as e:
            exL.stereo_matches(exR, *args, c["mb"], c["mbf"], frame=c["sheet"])
        assert e.value.code == pkg.capi.ORBX_ERR_ARG
    ur, dp = exL.stereo_matches(exR, c["kps_l"], c["desc_l"], c["kps_r"], c["desc_r"], c["mb"], c["mbf"], frame=c["sheet"])       # the handle is still usable
    _check("best_shift", bc.reference("best_shift"), ur, dp)


def test_frame_of_a_batch_equals_the_single_pair(pkg, rigs):
    """stereo_matches(..., frame=2) on the batch of three different pairs against extractors that saw only the third pair"""
    name = "octave_window_g8"
    c = bc.CASES[name]
    assert c["sheet"] == 2
    exL, exR = pkg.Extractor(*bc.GEOMS["g8"]), pkg.Extractor(*bc.GEOMS["g8"])
    try:
        exL(bc.TEX.left, (0, 0)); exR(bc.TEX.right, (0, 0))
        single = exL.stereo_matches(exR, c["kps_l"], c["desc_l"], c["kps_r"], c["desc_r"], c["mb"], c["mbf"])
    finally:
        exL.close(); exR.close()
    batch = rigs["g8"][0].stereo_matches(rigs["g8"][1], c["kps_l"], c["desc_l"], c["kps_r"], c["desc_r"], c["mb"], c["mbf"], frame=2)
    np.testing.assert_array_equal(single[0], batch[0]); np.testing.assert_array_equal(single[1], batch[1])
    _check(name, bc.reference(name), *batch)


# ------------------------------------------------------------------------------------------------ device batch entry
def _launch(rig, frames, cap, mb, mbf):
    """one stereo_matches_device launch: frames[b] = (kps_l, desc_l, kps_r, desc_r, n_l, n_r), the arrays already cut to `cap` rows, n
    as the device is told.  Returns u_right, depth [B, cap] from buffers that were filled with SENTINEL."""
    import torch
    dev = torch.device("cuda", 0)
    B = len(frames)
    side = []
    for k_i, d_i in ((0, 1), (2, 3)):
        kps = np.zeros((B, cap), bc.KP_DTYPE); desc = np.zeros((B, cap, 32), np.uint8)
        for b, f in enumerate(frames):
            kps[b, :len(f[k_i])] = f[k_i]; desc[b, :len(f[d_i])] = f[d_i]
        side.append((torch.from_numpy(kps.view(np.uint8).reshape(-1)).to(dev), torch.from_numpy(desc.reshape(-1)).to(dev)))
    n_l = torch.tensor([f[4] for f in frames], dtype=torch.int32, device=dev)
    n_r = torch.tensor([f[5] for f in frames], dtype=torch.int32, device=dev)
    d_ur = torch.full((B * cap,), float(SENTINEL), dtype=torch.float32, device=dev); d_dp = torch.full((B * cap,), float(SENTINEL), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rig[0].stereo_matches_device(rig[1], B, side[0][0].data_ptr(), side[0][1].data_ptr(), n_l.data_ptr(), side[1][0].data_ptr(), side[1][1].data_ptr(),
                                 n_r.data_ptr(), cap, mb, mbf, d_ur.data_ptr(), d_dp.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return d_ur.cpu().numpy().reshape(B, cap), d_dp.cpu().numpy().reshape(B, cap)


_EMPTY = (np.zeros(0, bc.KP_DTYPE), np.zeros((0, 32), np.uint8)) * 2 + (0, 0)


def _device_launches():
    """every case with at most 1100 key points a side, one frame per sheet and launch (sheet i is frame i), the cases of a launch sharing
    geometry, mb and mbf.  cap is no power of two: 300 (bitonic size 512) while the cases fit, 1100 (2048) for the larger ones"""
    launches = []
    keyf = lambda c: (c["geom"], c["mb"], c["mbf"], 300 if max(len(c["kps_l"]), len(c["kps_r"])) <= 300 else 1100)
    fit = sorted((c for c in bc.CASES.values() if max(len(c["kps_l"]), len(c["kps_r"])) <= 1100), key=keyf)
    for key, group in itertools.groupby(fit, keyf):
        per_sheet = [[], [], []]
        for c in group:
            per_sheet[c["sheet"]].append(c["name"])
        for names in itertools.zip_longest(*per_sheet):
            launches.append(key + (names,))
    return launches


DEVICE_LAUNCHES = _device_launches()


def test_device_launches_cover_the_cases():
    names = [n for l in DEVICE_LAUNCHES for n in l[4] if n]
    assert len(names) == len(set(names)) and set(bc.CASES) - set(names) == {"first_minimum", "median_n4097", "median_n8192"}
    sizes = [[len(bc.CASES[n]["kps_l"]) for n in l[4] if n] for l in DEVICE_LAUNCHES]
    assert any(len(set(s)) == 3 for s in sizes)                    # frames of one launch with different n_l
    assert any(bc.reference(n)["n_matches"] == 0 for n in names)  # a frame without a match


@pytest.mark.parametrize("launch", DEVICE_LAUNCHES, ids=lambda l: "%s-cap%d-%s" % (l[0], l[3], "+".join(n or "empty" for n in l[4])))
def test_device_entry_equals_restatement(rigs, launch):
    geom, mb, mbf, cap, names = launch
    frames = []
    for n in names:
        c = bc.CASES[n] if n else None
        frames.append(_EMPTY if c is None else (c["kps_l"], c["desc_l"], c["kps_r"], c["desc_r"], len(c["kps_l"]), len(c["kps_r"])))
    ur, dp = _launch(rigs[geom], frames, cap, mb, mbf)
    for b, n in enumerate(names):
        k = frames[b][4]
        if n:
            _check(n, bc.reference(n), ur[b, :k], dp[b, :k])
        assert (ur[b, k:] == SENTINEL).all() and (dp[b, k:] == SENTINEL).all(), "rows past n_l were written"


def test_device_entry_clamps_to_cap(rigs):
    """nL[frame] > cap: the first cap key points are matched and the rows of the other frames stay untouched.  Of the other two frames
    one has no match at all and one a handful of key points, so the frames' bitonic sizes (4, 512, 16) all lie below the launch's"""
    cap = 300
    big, none, tex = bc.CASES["median_n1023"], bc.CASES["no_right_keypoints"], bc.CASES["octave_window_g8"]
    assert (big["sheet"], none["sheet"], tex["sheet"]) == (1, 0, 2) and len(big["kps_r"]) <= cap
    want_big = ref.stereo_matches(*bc.pyramid("g8", 1), *bc.tables("g8"), big["kps_l"][:cap], big["desc_l"][:cap], big["kps_r"], big["desc_r"], bc.MB, bc.MBF)
    assert want_big["n_matches"] > 100
    assert not np.array_equal(want_big["u_right"], bc.reference("median_n1023")["u_right"][:cap])       # another median than that of all 1023
    frames = [(none["kps_l"], none["desc_l"], none["kps_r"], none["desc_r"], len(none["kps_l"]), 0),
              (big["kps_l"][:cap], big["desc_l"][:cap], big["kps_r"], big["desc_r"], len(big["kps_l"]), len(big["kps_r"])),
              (tex["kps_l"], tex["desc_l"], tex["kps_r"], tex["desc_r"], len(tex["kps_l"]), len(tex["kps_r"]))]
    ur, dp = _launch(rigs["g8"], frames, cap, bc.MB, bc.MBF)
    _check("no_right_keypoints", bc.reference("no_right_keypoints"), ur[0, :len(none["kps_l"])], dp[0, :len(none["kps_l"])])
    _check("median_n1023 cut to cap", want_big, ur[1], dp[1])
    _check("octave_window_g8", bc.reference("octave_window_g8"), ur[2, :len(tex["kps_l"])], dp[2, :len(tex["kps_l"])])
    for b, k in ((0, len(none["kps_l"])), (2, len(tex["kps_l"]))):
        assert (ur[b, k:] == SENTINEL).all() and (dp[b, k:] == SENTINEL).all()
