"""k_resize / k_resize_tail / k_blur at the smallest shapes where their tiling can go wrong: every pyramid level and every blurred
level of every case, byte for byte.

  117 x 257, 4 levels   last blur tile column one pixel wide; width not a multiple of 4; last tile row one pixel high
  175 x 259, 6 levels   level widths 259, 216, 180, 150, 125, 104: the last quads of a resize row
  121 x 193, 5 levels   the top level, 93 x 58, is exactly one blur tile high
   75 x  66, 3 levels   levels 66, 55 and 46 wide: both reflected edges in one tile, narrower than a tile

The pyramid is compared with the oracle's.  The oracle blurs a level only where it has key points, so the reference of the blurred
levels is a numpy restatement of the 7x7 Q8.8 filter (taps 18 34 48 56 48 34 18, BORDER_REFLECT_101, (v + 0x8000) >> 16) applied to
the oracle's (= the verified) pyramid level; the restatement itself is checked against the oracle on every level the oracle blurs.
Each case runs through the host entry, through extract_batch_device with row stride = width (level 0 copied) and with the row stride
rounded up to 16 (level 0 read in place); 117 x 257 also with 64 frames, the batch size from which the fused resize tail and the
side-stream schedule run."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CASES = {"117x257": (117, 257, 4), "175x259": (175, 259, 6), "121x193": (121, 193, 5), "75x66": (75, 66, 3)}
N_DISTINCT = 2
NFEATURES = 500
TAPS = np.array([18, 34, 48, 56, 48, 34, 18], np.uint32)


def blur_restatement(img):
    """cv::GaussianBlur(7x7, sigma 2, BORDER_REFLECT_101) on 8-bit pixels, fixed point: rows to Q8.8, columns to Q16.16, one rounding"""
    h, w = img.shape
    p = np.pad(img.astype(np.uint32), ((0, 0), (3, 3)), mode="reflect")
    hor = sum(TAPS[k] * p[:, k:k + w] for k in range(7))
    assert hor.max() <= 255 * 256
    p = np.pad(hor, ((3, 3), (0, 0)), mode="reflect")
    ver = sum(TAPS[k] * p[k:k + h, :] for k in range(7))
    return ((ver + 0x8000) >> 16).astype(np.uint8)


_reference = {}


def reference(case, oracle, synth):
    """(frames, per frame and level the oracle's pyramid level, per frame and level the blurred level), computed once per case"""
    if case not in _reference:
        h, w, nlevels = CASES[case]
        frames = [synth.make_frame(4100 + 10 * list(CASES).index(case) + i, w, h) for i in range(N_DISTINCT)]
        pyr, blur = [], []
        for im in frames:
            oex = oracle.extractor(NFEATURES, 1.2, nlevels, 20, 7)
            oex.extract(im, (0, 1000))
            lv = [oex.level_image(l) for l in range(nlevels)]
            assert np.array_equal(lv[0], im)
            bl = [blur_restatement(x) for x in lv]
            # (with these frames the oracle has key points on, and blurs, every level of 104 x 70 and more and none of 93 x 58 and less:
            # no level of the 75 x 66 case)
            for l in range(nlevels):
                ob = oex.level_blurred(l)
                if ob is not None:
                    np.testing.assert_array_equal(bl[l], ob, "numpy restatement of the blur differs from the oracle, level %d" % l)
            pyr.append(lv); blur.append(bl)
        for a in frames + [x for f in pyr + blur for x in f]:
            a.setflags(write=False)
        _reference[case] = (frames, pyr, blur)
    return _reference[case]


def check_levels(ex, case, ref, frame, which, what):
    h, w, nlevels = CASES[case]
    _, pyr, blur = ref
    for l in range(nlevels):
        assert ex.level_size(l) == (pyr[which][l].shape[1], pyr[which][l].shape[0])
        np.testing.assert_array_equal(ex.pyramid_level(l, frame), pyr[which][l], "%s %s: pyramid level %d of frame %d" % (case, what, l, frame))
        np.testing.assert_array_equal(ex.blurred_level(l, frame), blur[which][l], "%s %s: blurred level %d of frame %d" % (case, what, l, frame))


def run_device(pkg, case, ref, B, in_place, what):
    import torch
    h, w, nlevels = CASES[case]
    frames = ref[0]
    stride = (w + 15) // 16 * 16 if in_place else w
    host = np.zeros((B, h, stride), np.uint8)
    host[:, :, w:] = 0xA5                   # row padding: never a pixel
    for b in range(B):
        host[b, :, :w] = frames[b % N_DISTINCT]
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(host).to(dev)
    ex = pkg.Extractor(NFEATURES, 1.2, nlevels, 20, 7)
    try:
        cap = max(ex.max_keypoints, ex.max_keypoints_for(w, h))
        d_kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device=dev); d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(B, dtype=torch.int32, device=dev); d_mono = torch.zeros(B, dtype=torch.int32, device=dev); d_st = torch.zeros(B, dtype=torch.int32, device=dev)
        ex.extract_batch_device(d_img.data_ptr(), B, w, h, stride, h * stride, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                                d_n.data_ptr(), d_mono.data_ptr(), d_st.data_ptr(), (0, 1000), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(d_st.abs().sum().item()) == 0
        sched = ex.debug_last_schedule()
        print("%s %s: schedule %d" % (case, what, sched))
        assert bool(sched & 16) == in_place, "level 0 read in place: %d, expected %d" % (bool(sched & 16), in_place)
        for b in range(B):
            check_levels(ex, case, ref, b, b % N_DISTINCT, what)
        return sched
    finally:
        ex.close()


@pytest.mark.parametrize("case", list(CASES))
def test_host_entry(pkg, oracle, synth, case):
    ref = reference(case, oracle, synth)
    ex = pkg.Extractor(NFEATURES, 1.2, CASES[case][2], 20, 7)
    try:
        for i, im in enumerate(ref[0]):
            ex(im)
            check_levels(ex, case, ref, 0, i, "host entry")
    finally:
        ex.close()


@pytest.mark.parametrize("case", list(CASES))
def test_device_entry_level0_copied(pkg, oracle, synth, case):
    run_device(pkg, case, reference(case, oracle, synth), 3, False, "device entry, stride = width")


@pytest.mark.parametrize("case", list(CASES))
def test_device_entry_level0_in_place(pkg, oracle, synth, case):
    run_device(pkg, case, reference(case, oracle, synth), 3, True, "device entry, stride rounded up to 16")


def test_64_frames_take_the_resize_tail(pkg, oracle, synth, monkeypatch):
    """64 frames and more: the upper levels are one k_resize_tail launch on the side stream.  The tail starts at level 4 by default and
    this case has 4 levels, so the test moves its start to level 2 (ORBX_RESIZE_TAIL, read when the handle is made)."""
    monkeypatch.setenv("ORBX_RESIZE_TAIL", "2")
    sched = run_device(pkg, "117x257", reference("117x257", oracle, synth), 64, True, "64 frames")
    assert sched & 32, "the resize tail did not run on the side stream: schedule %d" % sched
