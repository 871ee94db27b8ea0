"""The table-driven pyramid resize with the rows uniform per wave (k_resize / k_resize_tail, resize_band): the lanes of a wave are
the quads of one column strip in FOUR frames (one frame for batches below four), a wave walks a band of output rows and keeps the
horizontal sums of the previous row's two source rows, and the clamp to 255 is dropped where the coefficient sums prove it dead.

Every pyramid level of every frame is compared with the oracle's level_image, byte for byte; row padding of the input is 0xA5.

  frame-to-lane mapping   B = 1, 2, 3, 4, 5, 7, 9, every frame different; 75 x 66 (3 levels) and 117 x 257 (4 levels); level 0 copied
                          and read in place
  band boundaries         image heights 76, 77, 78 (66 wide): level 1 is 63, 64 and 65 rows = 4 R - 1, 4 R, 4 R + 1 for the band of
                          R = 16 rows that is built.  The host table says that a band of these levels starts on a reused row (plan 1)
                          and that one starts right after a skipped source row (plan 0): both asserted
  clamped rows            first and last row of every level are part of every comparison, and the replay below checks every row's
                          plan against its clamped source rows; 70 x 157 and 70 x 310: level 1 is 131 and 258 pixels wide, one quad
                          in the last strip of four frames per wave (64-pixel strips) and of one (256-pixel strips)
  scale factors           1.1, 1.5, 1.99 (every level table-driven) and 2.0 on 257 x 117 (level 1 takes k_resize_generic), told
                          apart by a numpy replay of the column table
  extremes                all-255, 1-pixel and 2-pixel checkerboards of 0 / 255: the extremes of the dropped clamp
  the tail                B = 65 and 67 with ORBX_RESIZE_TAIL=2 on 117 x 257, schedule bit 32
  small batches           k_resize serves batches of 64 frames and more, so every case above runs with ORBX_RESIZE_BAND_MIN=1 and
                          asserts that a level went through k_resize (debug_resize_bands); B = 1 and 5 also run the default
                          schedule (k_resize_tiles) on the extreme frames

CPU (not marked gpu): the row table of orbx_debug_resize_rows replayed in numpy -- walking bands, reusing exactly what the kernels
reuse, no clamp -- reproduces the oracle's pyramid on the shapes above; the share of fresh source rows per output row on
640 x 480 x 8 levels is 1.20 +- 0.01."""
import ctypes as C

import numpy as np
import pytest

gpu = pytest.mark.gpu

NFEATURES = 500
BAND = 16                    # rows of a band as built (asserted against the library)


# ------------------------------------------------------------------------------------------------ host restatement
def level_sizes(w, h, sf, nlevels):
    """(w, h) per level as the extractor computes them: float scale table, round to nearest even"""
    s = [np.float32(1)]
    for _ in range(1, nlevels):
        s.append(np.float32(float(s[-1]) * float(np.float32(sf))))
    return [(int(np.rint(np.float32(w) * (np.float32(1) / x))), int(np.rint(np.float32(h) * (np.float32(1) / x)))) for x in s]


def row_table(pkg, src_h, dst_h):
    """(rows[dst_h, 4] = sy0 | sy1 << 16, b0 << 12, b1 << 12, plan; coefficient sums <= 2048)"""
    rows = np.zeros(4 * dst_h, np.uint32)
    band = C.c_int(0)
    r = pkg.lib.orbx_debug_resize_rows(src_h, dst_h, rows.ctypes.data, C.byref(band))
    assert r >= 0 and band.value == BAND
    return rows.reshape(dst_h, 4), bool(r)


def column_table(src_w, dst_w):
    """cv::resize INTER_LINEAR 8UC1: xofs, the two coefficients per column (float arithmetic as the host's)"""
    scale = 1. / (dst_w / src_w)
    fx = ((np.arange(dst_w) + 0.5) * scale - 0.5).astype(np.float32)
    sx = np.floor(fx).astype(np.int64)
    fx = fx - sx.astype(np.float32)
    fx[sx < 0] = 0; sx[sx < 0] = 0
    fx[sx >= src_w - 1] = 0; sx[sx >= src_w - 1] = src_w - 1
    a0 = np.rint((np.float32(1) - fx) * np.float32(2048)).astype(np.int64)
    a1 = np.rint(fx * np.float32(2048)).astype(np.int64)
    return sx, a0, a1


def takes_generic(src_w, dst_w):
    """a quad of destination columns spans more than the 8-byte window of the table-driven kernel"""
    sx, _, _ = column_table(src_w, dst_w)
    return any(sx[min(4 * q + 3, dst_w - 1)] - sx[4 * q] > 6 for q in range((dst_w + 3) // 4))


def replay_level(pkg, src, dst_w, dst_h):
    """the level as resize_band computes it: bands of BAND rows, the previous bottom row reused where the plan says so, every other
    row filtered afresh, no clamp.  Returns (level, fresh source rows as the kernel takes them, fresh source rows by the plan)"""
    src_h, src_w = src.shape
    rows, rows_ok = row_table(pkg, src_h, dst_h)
    sx, a0, a1 = column_table(src_w, dst_w)
    assert rows_ok and (a0 + a1 <= 2048).all(), "coefficient sums above 2048: the level would take the saturating kernel"
    sx1 = np.minimum(sx + 1, src_w - 1)
    s = src.astype(np.int64)

    def hsum(sy):
        return (s[sy, sx] * a0 + s[sy, sx1] * a1) & ~15

    out = np.zeros((dst_h, dst_w), np.uint8)
    fresh_kernel = fresh_plan = 0
    ht = hb = None
    p0 = p1 = -1
    for y in range(dst_h):
        sy0, sy1 = int(rows[y, 0] & 0xFFFF), int(rows[y, 0] >> 16)
        b0, b1, plan = int(rows[y, 1] >> 12), int(rows[y, 2] >> 12), int(rows[y, 3])
        assert 0 <= sy0 <= sy1 < src_h
        # the plan is consistent with the clamped source rows
        assert (plan & 3) in (0, 1, 2) and ((plan & 3) != 1 or sy0 == p1) and ((plan & 3) != 2 or sy0 == p0) and (bool(plan & 4) == (sy1 == sy0))
        assert (plan & 3) != 0 or (sy0 != p1 and sy0 != p0)
        fresh_plan += ((plan & 3) == 0) + (not plan & 4)
        if y % BAND and (plan & 3) == 1:
            ht = hb
        else:
            ht = hsum(sy0); fresh_kernel += 1
        hb = hsum(sy1); fresh_kernel += 1
        v = (((b0 << 12) * ht) >> 32) + (((b1 << 12) * hb) >> 32) + 2 >> 2
        assert v.max() <= 255
        out[y] = v
        p0, p1 = sy0, sy1
    return out, fresh_kernel, fresh_plan


# ------------------------------------------------------------------------------------------------ frames and references
def special_frame(kind, w, h):
    yy, xx = np.mgrid[0:h, 0:w]
    if kind == "white":
        return np.full((h, w), 255, np.uint8)
    if kind == "checker1":
        return (((xx + yy) & 1) * 255).astype(np.uint8)
    if kind == "checker1i":
        return (((xx + yy + 1) & 1) * 255).astype(np.uint8)
    assert kind == "checker2"
    return ((((xx >> 1) + (yy >> 1)) & 1) * 255).astype(np.uint8)


_pyramids = {}


def oracle_pyramid(oracle, synth, w, h, sf, nlevels, which):
    """the oracle's pyramid of frame `which` (a seed, or the name of a special frame) of a shape, computed once"""
    key = (w, h, sf, nlevels, which)
    if key not in _pyramids:
        im = special_frame(which, w, h) if isinstance(which, str) else synth.make_frame(5200 + 37 * which + w + h, w, h)
        oex = oracle.extractor(NFEATURES, sf, nlevels, 20, 7)
        oex.extract(im, (0, 1000))
        lv = [oex.level_image(l) for l in range(nlevels)]
        assert np.array_equal(lv[0], im)
        for a in lv:
            a.setflags(write=False)
        _pyramids[key] = lv
    return _pyramids[key]


def run_device(pkg, oracle, synth, w, h, sf, nlevels, frames, in_place, what, bands=True):
    """`frames`: a seed or special-frame name per frame of the batch.  Every level of every frame against the oracle.
    `bands`: whether the batch is expected to take k_resize (None: not checked)."""
    import torch
    B = len(frames)
    ref = [oracle_pyramid(oracle, synth, w, h, sf, nlevels, f) for f in frames]
    stride = (w + 15) // 16 * 16 if in_place else w
    host = np.full((B, h, stride), 0xA5, np.uint8)       # row padding: never a pixel
    for b in range(B):
        host[b, :, :w] = ref[b][0]
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(host).to(dev)
    ex = pkg.Extractor(NFEATURES, sf, nlevels, 20, 7)
    try:
        cap = max(ex.max_keypoints, ex.max_keypoints_for(w, h))
        d_kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device=dev); d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(B, dtype=torch.int32, device=dev); d_mono = torch.zeros(B, dtype=torch.int32, device=dev); d_st = torch.zeros(B, dtype=torch.int32, device=dev)
        ex.extract_batch_device(d_img.data_ptr(), B, w, h, stride, h * stride, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                                d_n.data_ptr(), d_mono.data_ptr(), d_st.data_ptr(), (0, 1000), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(d_st.abs().sum().item()) == 0
        sched = ex.debug_last_schedule()
        assert bool(sched & 16) == in_place, "level 0 read in place: %d, expected %d" % (bool(sched & 16), in_place)
        sizes = level_sizes(w, h, sf, nlevels)
        if bands is not None:       # did a level go through k_resize?  (a level of scale >= 2 takes k_resize_generic whatever the batch)
            l_tail = 2 if sched & 32 else nlevels
            table_driven = any(not takes_generic(sizes[l - 1][0], sizes[l][0]) for l in range(1, l_tail))
            assert ex.debug_resize_bands() == (bands and table_driven), "k_resize ran: %d, expected %d" % (ex.debug_resize_bands(), bands and table_driven)
        for l in range(nlevels):
            assert ex.level_size(l) == sizes[l] == (ref[0][l].shape[1], ref[0][l].shape[0])
            for b in range(B):
                np.testing.assert_array_equal(ex.pyramid_level(l, b), ref[b][l], "%s: pyramid level %d of frame %d of %d" % (what, l, b, B))
        return sched
    finally:
        ex.close()


def both_entries(pkg, oracle, synth, w, h, sf, nlevels, frames, what):
    run_device(pkg, oracle, synth, w, h, sf, nlevels, frames, False, what + ", level 0 copied")
    run_device(pkg, oracle, synth, w, h, sf, nlevels, frames, True, what + ", level 0 in place")


SHAPES = {"75x66": (66, 75, 3), "117x257": (257, 117, 4)}        # rows x columns -> (w, h, levels)


@pytest.fixture
def bands_for_every_batch(monkeypatch):
    """k_resize serves batches of 64 frames and more; the tests run it at every batch size (ORBX_RESIZE_BAND_MIN, read when the
    handle is made) and run_device asserts that it ran"""
    monkeypatch.setenv("ORBX_RESIZE_BAND_MIN", "1")


# ------------------------------------------------------------------------------------------------ GPU
@gpu
@pytest.mark.parametrize("B", [1, 2, 3, 4, 5, 7, 9])
@pytest.mark.parametrize("shape", list(SHAPES))
def test_frames_across_the_lanes(pkg, oracle, synth, shape, B, bands_for_every_batch):
    w, h, nlevels = SHAPES[shape]
    both_entries(pkg, oracle, synth, w, h, 1.2, nlevels, list(range(B)), "%s, %d frames" % (shape, B))


BAND_HEIGHTS = (76, 77, 78)


def band_start_plans(pkg, w, h, nlevels):
    """per level from 1 on: (rows of the level, the plan's top-row field of every row that starts a band but the first)"""
    sizes = level_sizes(w, h, 1.2, nlevels)
    out = []
    for l in range(1, nlevels):
        rows, _ = row_table(pkg, sizes[l - 1][1], sizes[l][1])
        out.append((sizes[l][1], [int(rows[y, 3] & 3) for y in range(BAND, sizes[l][1], BAND)]))
    return out


@gpu
@pytest.mark.parametrize("B", [3, 5])
def test_band_boundaries(pkg, oracle, synth, B, bands_for_every_batch):
    heights, starts = [], []
    for h in BAND_HEIGHTS:
        for lh, st in band_start_plans(pkg, 66, h, 3):
            heights.append(lh); starts += st
        both_entries(pkg, oracle, synth, 66, h, 1.2, 3, list(range(B)), "66 x %d, %d frames" % (h, B))
    assert {4 * BAND - 1, 4 * BAND, 4 * BAND + 1} <= set(heights), heights
    assert 1 in starts, "no band of these levels starts on a reused row"
    assert 0 in starts, "no band of these levels starts right after a skipped source row"


@gpu
@pytest.mark.parametrize("w,B", [(157, 4), (157, 6), (310, 1), (310, 3)])
def test_one_quad_in_the_last_strip(pkg, oracle, synth, w, B, bands_for_every_batch):
    lw = level_sizes(w, 70, 1.2, 2)[1][0]
    strip = 64 if B >= 4 else 256
    assert 1 <= lw % strip <= 4, "level 1 is %d pixels wide" % lw
    both_entries(pkg, oracle, synth, w, 70, 1.2, 2, list(range(B)), "%d x 70, %d frames" % (w, B))


@gpu
@pytest.mark.parametrize("sf,w,h,nlevels,generic", [(1.1, 257, 117, 4, False), (1.5, 257, 117, 3, False), (1.99, 257, 117, 2, False), (2.0, 117, 257, 2, True)])
def test_scale_factors(pkg, oracle, synth, sf, w, h, nlevels, generic, bands_for_every_batch):
    sizes = level_sizes(w, h, sf, nlevels)
    g = [takes_generic(sizes[l - 1][0], sizes[l][0]) for l in range(1, nlevels)]
    assert any(g) == generic, "levels that take k_resize_generic at scale %g: %s" % (sf, g)
    both_entries(pkg, oracle, synth, w, h, sf, nlevels, [0, 1, 2, 3, 4], "scale %g" % sf)
    both_entries(pkg, oracle, synth, w, h, sf, nlevels, [0, 1], "scale %g" % sf)


@gpu
@pytest.mark.parametrize("B", [2, 5])
def test_extremes_of_the_dropped_clamp(pkg, oracle, synth, B, bands_for_every_batch):
    frames = ["white", "checker1", "checker2", "checker1i", 0][:B]
    for shape in SHAPES:
        w, h, nlevels = SHAPES[shape]
        both_entries(pkg, oracle, synth, w, h, 1.2, nlevels, frames, "%s extremes, %d frames" % (shape, B))


@gpu
@pytest.mark.parametrize("B", [65, 67])
def test_the_tail(pkg, oracle, synth, monkeypatch, B):
    """64 frames and more: the upper levels are one k_resize_tail launch on the side stream; the tail starts at level 4 by default
    and the case has 4 levels, so the test moves its start to level 2 (ORBX_RESIZE_TAIL, read when the handle is made)"""
    monkeypatch.setenv("ORBX_RESIZE_TAIL", "2")
    w, h, nlevels = SHAPES["117x257"]
    sched = run_device(pkg, oracle, synth, w, h, 1.2, nlevels, list(range(B)), True, "%d frames" % B)
    assert sched & 32, "the resize tail did not run on the side stream: schedule %d" % sched


@gpu
@pytest.mark.parametrize("B", [1, 5])
def test_small_batches_take_the_tile_kernel(pkg, oracle, synth, B):
    """below 64 frames a level is one k_resize_tiles launch (a short wave per four rows: the latency of a small batch), with the
    clamp dropped in the same way"""
    for shape in SHAPES:
        w, h, nlevels = SHAPES[shape]
        frames = (["white", "checker1", "checker2", "checker1i", 0] if B == 5 else [0])
        run_device(pkg, oracle, synth, w, h, 1.2, nlevels, frames, False, "%s, %d frames, default schedule" % (shape, B), bands=False)
        run_device(pkg, oracle, synth, w, h, 1.2, nlevels, frames, True, "%s, %d frames, default schedule" % (shape, B), bands=False)


# ------------------------------------------------------------------------------------------------ CPU
CPU_CASES = [(66, 75, 1.2, 3), (257, 117, 1.2, 4), (66, 76, 1.2, 3), (66, 77, 1.2, 3), (66, 78, 1.2, 3), (157, 70, 1.2, 2), (310, 70, 1.2, 2),
             (257, 117, 1.1, 4), (257, 117, 1.5, 3), (257, 117, 1.99, 2), (117, 257, 2.0, 2)]


@pytest.mark.parametrize("w,h,sf,nlevels", CPU_CASES)
def test_row_plan_replayed_in_numpy_is_the_oracle_pyramid(pkg, oracle, synth, w, h, sf, nlevels):
    sizes = level_sizes(w, h, sf, nlevels)
    frames = [0, 1] + (["white", "checker1", "checker2"] if sf == 1.2 else [])
    replayed = 0
    for f in frames:
        ref = oracle_pyramid(oracle, synth, w, h, sf, nlevels, f)
        for l in range(1, nlevels):
            assert (ref[l].shape[1], ref[l].shape[0]) == sizes[l]
            if takes_generic(sizes[l - 1][0], sizes[l][0]):
                continue
            got, _, _ = replay_level(pkg, ref[l - 1], sizes[l][0], sizes[l][1])
            np.testing.assert_array_equal(got, ref[l], "%d x %d scale %g frame %s level %d" % (w, h, sf, f, l))
            replayed += 1
    assert replayed == len(frames) * (nlevels - 1) or sf == 2.0


def test_fresh_rows_per_output_row_at_640x480(pkg):
    sizes = level_sizes(640, 480, 1.2, 8)
    rows_out = fresh_plan = fresh_kernel = 0
    for l in range(1, 8):
        src = np.zeros((sizes[l - 1][1], sizes[l - 1][0]), np.uint8)
        _, fk, fp = replay_level(pkg, src, sizes[l][0], sizes[l][1])
        rows_out += sizes[l][1]; fresh_plan += fp; fresh_kernel += fk
    print("640 x 480 x 8 levels: %d output rows, %.4f fresh source rows per output row by the plan, %.4f as the kernel walks bands of %d" %
          (rows_out, fresh_plan / rows_out, fresh_kernel / rows_out, BAND))
    assert abs(fresh_plan / rows_out - 1.20) <= 0.01
    # a band's first row loads its top row whatever the plan says: at most one more row per band
    assert fresh_plan <= fresh_kernel <= fresh_plan + sum((sizes[l][1] + BAND - 1) // BAND for l in range(1, 8))
