"""The stream hand-offs of the extractor's large-batch schedule: the blur in two launches by level range with the
resize tail's levels blurred on the tail's own queue, events recorded as the stop event of the launch they follow, the status words
cleared by the first FAST launch.  640 x 480 with the bench's extractor parameters, B = 64 (the smallest batch with the fused resize
tail) and B = 96 (above 64 the scratch-key octree runs), 8 distinct frames repeated, the bench's entry point (device pointers, level 0
read in place).  Key points, descriptors, counts, mono index and status against the CPU oracle bit for bit; the oracle's results are
computed once per module.

Not marked gpu: the cut of the blur's tile list between the two launches, on the host."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")
PARAMS = (1000, 1.2, 8, 20, 7)
W, H = 640, 480
TAIL_LEVEL = 4                                  # first level of the fused resize tail (ORBX_RESIZE_TAIL's default)
SPLIT, BOUND, STATUS = 1, 2, 4                  # bits of debug_last_handoffs
SWITCHES = ("ORBX_BLUR_SPLIT", "ORBX_BIND_RECORDS", "ORBX_STATUS_IN_FAST")
ERR_CAPACITY = -2


@pytest.fixture(scope="module")
def frames(synth):
    return [synth.make_frame(970 + i) for i in range(8)]


@pytest.fixture(scope="module")
def ref(oracle, frames):
    oex = oracle.extractor(*PARAMS)
    return [oex.extract(im, (0, 1000)) for im in frames]


def _expected_schedule(B):
    # as tests/test_extractor_gpu.py::test_large_batch_device_api_in_place expects it with the resize chain beside FAST on level 0
    return (3 if B <= 64 else 2) | 4 | 8 | 16 | 32 | 64


def _run_twice(pkg, frames, ref, B, env, monkeypatch, handoffs, tail_delay=0, cap=None):
    """two calls on one handle, the second with the frames rolled by one (stale levels of any buffer then belong to another frame);
    d_status is pre-filled with a non-zero value before each.  With `cap` below a frame's count: only counts and status."""
    import torch
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(np.stack([frames[i % 8] for i in range(B)])).to(dev)
    ex = pkg.Extractor(*PARAMS)
    try:
        full = cap is None
        cap = ex.max_keypoints if full else cap
        d_kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device=dev); d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(B, dtype=torch.int32, device=dev); d_mono = torch.zeros(B, dtype=torch.int32, device=dev)
        st = torch.cuda.current_stream().cuda_stream
        if tail_delay:
            ex.debug_set_tail_delay(tail_delay)
        for rep in range(2):
            if rep == 1:
                d_img = torch.roll(d_img, 1, 0).contiguous()
            d_st = torch.full((B,), 0x5A5A, dtype=torch.int32, device=dev)
            ex.extract_batch_device(d_img.data_ptr(), B, W, H, W, W * H, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                                    d_n.data_ptr(), d_mono.data_ptr(), d_st.data_ptr(), (0, 1000), st)
            torch.cuda.synchronize()
            assert ex.debug_last_schedule() == _expected_schedule(B), "not the expected schedule: %d" % ex.debug_last_schedule()
            assert ex.debug_last_handoffs() == handoffs, "hand-offs %d, expected %d" % (ex.debug_last_handoffs(), handoffs)
            n = d_n.cpu().numpy(); mono = d_mono.cpu().numpy(); status = d_st.cpu().numpy()
            kps = d_kps.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap); desc = d_desc.cpu().numpy().reshape(B, cap, 32)
            for b in range(B):
                r0, k0, d0 = ref[(b - rep) % 8]
                what = "call %d frame %d" % (rep, b)
                assert mono[b] == r0 and n[b] == len(k0), what
                assert status[b] == (ERR_CAPACITY if len(k0) > cap else 0), "%s: status %d with %d key points, cap %d" % (what, status[b], len(k0), cap)
                if full:
                    for f in FIELDS:
                        assert np.array_equal(kps[b, :n[b]][f], k0[f]), "%s: field %s" % (what, f)
                    assert np.array_equal(desc[b, :n[b]], d0), "%s: descriptors" % what
    finally:
        ex.close()


@gpu
@pytest.mark.parametrize("B", [64, 96])
def test_new_schedule_ran(pkg, frames, ref, monkeypatch, B):
    """the defaults: all three hand-offs reported, the schedule getter unchanged, results and a zero status on both calls"""
    _run_twice(pkg, frames, ref, B, {}, monkeypatch, SPLIT | BOUND | STATUS)


@gpu
@pytest.mark.parametrize("B", [64, 96])
def test_tail_level_blur_waits_for_the_tail_and_descriptors_for_it(pkg, frames, ref, monkeypatch, B):
    """a spin kernel holds the resize tail back by 0.4 ms, far longer than FAST and the blur of the lower levels: a k_orient_desc that
    starts before the side queue's blur of the tail's levels, that blur in front of the tail, or a launch-stream blur that still reads
    those levels, sees the previous call's pixels -- another frame's -- and the upper levels' key points and descriptors differ"""
    _run_twice(pkg, frames, ref, B, {}, monkeypatch, SPLIT | BOUND | STATUS, tail_delay=400)


@gpu
@pytest.mark.parametrize("B", [64, 96])
def test_status_is_cleared_and_capacity_reported_per_frame(pkg, frames, ref, monkeypatch, B):
    """d_status pre-filled with a non-zero value: 0 after a clean call (test_new_schedule_ran), and with `cap` between the counts of
    the frames ORBX_ERR_CAPACITY exactly for the frames with more key points, on both calls of the handle"""
    counts = sorted(len(k0) for _, k0, _ in ref)
    cap = counts[3]
    assert counts[0] <= cap < counts[-1], "the eight frames' counts do not straddle a capacity: %r" % counts
    _run_twice(pkg, frames, ref, B, {}, monkeypatch, SPLIT | BOUND | STATUS, cap=cap)


@gpu
@pytest.mark.parametrize("B", [64, 96])
@pytest.mark.parametrize("on,handoffs", [(None, 0), ("ORBX_BLUR_SPLIT", SPLIT), ("ORBX_BIND_RECORDS", BOUND), ("ORBX_STATUS_IN_FAST", STATUS)])
def test_switches(pkg, frames, ref, monkeypatch, B, on, handoffs):
    """every switch off: the schedule without the hand-offs (getter 0); each switch on alone: that bit alone; the oracle's bits always.
    The tail is delayed here too, so that a switch combination that loses an ordering shows"""
    env = {k: ("1" if k == on else "0") for k in SWITCHES}
    _run_twice(pkg, frames, ref, B, env, monkeypatch, handoffs, tail_delay=400)


def _level_sizes(w, h, scale_factor, nlevels):
    """ComputePyramid's level sizes with the extractor's float scale chain (a float scale times the double scale factor)"""
    sf = float(np.float32(scale_factor))
    scale, sizes = np.float32(1.0), []
    for l in range(nlevels):
        if l > 0:
            scale = np.float32(float(scale) * sf)
        inv = np.float32(1.0) / scale
        sizes.append((int(np.rint(np.float32(w) * inv)), int(np.rint(np.float32(h) * inv))))
    return sizes


@pytest.mark.parametrize("w,h,nlevels,level", [(640, 480, 8, 4), (752, 480, 8, 4), (640, 480, 2, 1), (640, 480, 8, 2), (97, 131, 3, 2)])
def test_blur_tile_ranges_partition_the_tile_list(pkg, w, h, nlevels, level):
    """the two launches' tile ranges [0, split) and [split, n): every tile once, the first range exactly the levels below `level`,
    the second exactly the levels from it on; tile counts per level from the level sizes (64 x 58 outputs per tile)"""
    lv = np.full(4096, -1, np.int16)
    split = C.c_int(-1)
    n = pkg.lib.orbx_debug_blur_tile_split(1.2, nlevels, w, h, level, lv.ctypes.data, lv.size, C.byref(split))
    per_level = [((lw + 63) // 64) * ((lh + 57) // 58) for lw, lh in _level_sizes(w, h, 1.2, nlevels)]
    assert n == sum(per_level)
    assert np.array_equal(lv[:n], np.repeat(np.arange(nlevels), per_level))
    assert split.value == sum(per_level[:level]) and 0 < split.value < n
    assert (lv[:split.value] < level).all() and (lv[split.value:n] >= level).all()
