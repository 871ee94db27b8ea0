"""The set-up of the FAST strip kernel: one host-built record per strip, the tile's 16-byte chunks loaded three per thread with all of
them in flight, the clears and the copy of the cells' table under the loads, one workgroup barrier.  Candidates of every level, key points
and descriptors against the CPU oracle, bit for bit, at the smallest shapes where that set-up can go wrong (fast_strip_setup_cases.py
restates the strip geometry, so that every case asserts that its frame has the strips it was chosen for):

  67 x 67, 67 x 100      the narrowest strips there are: one cell, 4 chunks per tile row; 140 chunks, fewer than threads, and 272, a
                         second one for 16 threads (a thread without a chunk of its own loads the last one again and stores nothing)
  320 x 240, 336 x 240   8 levels: strips that start at every alignment of the first quad inside its 16-byte chunk.  320 x 240 has the
                         tile bytes 8, 12 and 16; byte 4 needs a strip whose first column is 1 .. 4 mod 16, which 336 x 240 has (all four)
  160 x 101              2 levels, a cell row of 63 interior rows: three chunks per thread, the whole first group
  160 x 101, 250 x 101   with ORBX_STRIP_WIDTH = 250 (read once per process: a process of its own); the 250-wide strip has 1035 chunks,
                         more than one group per thread
  level 0                read in place with a row stride larger than the width and a frame stride larger than the frame; copied by
                         k_copy_level0 from an unaligned base; uploaded by the host entry -- two different frames per batch
  64 frames              the three launches of the large-batch schedule: the strip table is read at the offsets of level 1 and of the tail

Every case asserts that the oracle found key points, so that none passes on an empty frame."""
import os
import subprocess
import sys

import numpy as np
import pytest

import fast_strip_setup_cases as sc

pytestmark = pytest.mark.gpu

ARGS8 = (500, 1.2, 8, 20, 7)


def _refs(oracle, synth, w, h, args=ARGS8):
    """two different synthetic frames of w x h and the oracle's answers"""
    return [sc.reference(oracle, ("synth", w, h, args, k), synth.make_frame(8200 + k, w, h), args) for k in range(2)]


def _host_batch(pkg, refs, what, min_kps):
    args = refs[0]["args"]
    ex = pkg.Extractor(*args)
    try:
        mono, n, kps, desc = ex.extract_batch(np.stack([r["img"] for r in refs]))
        assert not ex.debug_last_schedule() & 16
        for b, r in enumerate(refs):
            assert len(r["kps"]) > min_kps, "%s frame %d: the oracle found %d key points" % (what, b, len(r["kps"]))
            sc.assert_same(ex, r, mono[b], kps[b, :n[b]], desc[b, :n[b]], b, "%s, frame %d" % (what, b))
    finally:
        ex.close()


def _device_batch(pkg, refs, B, what, min_kps, row_pad=0, frame_pad=0, misalign=0, corner_cap=None):
    """B frames (refs in turn) through extract_batch_device; returns the schedule bits.  corner_cap: the FAST kernel's corner lists
    shrunk to that many entries (its overflow path)"""
    import torch
    args = refs[0]["args"]
    h, w = refs[0]["img"].shape
    stride = w + row_pad
    frame_stride = h * stride + frame_pad
    host = np.full(misalign + B * frame_stride, 0xA5, np.uint8)          # padding: never a pixel
    for b in range(B):
        rows = host[misalign + b * frame_stride:misalign + b * frame_stride + h * stride].reshape(h, stride)
        rows[:, :w] = refs[b % len(refs)]["img"]
    dev = torch.device("cuda", 0)
    d_img = torch.from_numpy(host).to(dev)
    ex = pkg.Extractor(*args)
    try:
        if corner_cap is not None:
            ex.debug_set_fast_corner_cap(corner_cap)
        cap = max(ex.max_keypoints, ex.max_keypoints_for(w, h))
        d_kps = torch.zeros(B * cap * 28, dtype=torch.uint8, device=dev); d_desc = torch.zeros(B * cap * 32, dtype=torch.uint8, device=dev)
        d_n = torch.zeros(B, dtype=torch.int32, device=dev); d_mono = torch.zeros(B, dtype=torch.int32, device=dev)
        d_st = torch.full((B,), 77, dtype=torch.int32, device=dev)         # (a call leaves the status of every frame at zero)
        ex.extract_batch_device(d_img.data_ptr() + misalign, B, w, h, stride, frame_stride, d_kps.data_ptr(), d_desc.data_ptr(), cap,
                                d_n.data_ptr(), d_mono.data_ptr(), d_st.data_ptr(), (0, 1000), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        assert int(d_st.abs().sum().item()) == 0
        sched = ex.debug_last_schedule()
        n = d_n.cpu().numpy(); mono = d_mono.cpu().numpy()
        kps = d_kps.cpu().numpy().view(pkg.KP_DTYPE).reshape(B, cap); desc = d_desc.cpu().numpy().reshape(B, cap, 32)
        for b in range(B):
            r = refs[b % len(refs)]
            assert len(r["kps"]) > min_kps, "%s frame %d: the oracle found %d key points" % (what, b, len(r["kps"]))
            sc.assert_same(ex, r, mono[b], kps[b, :n[b]], desc[b, :n[b]], b, "%s, frame %d" % (what, b))
        return sched
    finally:
        ex.close()


@pytest.mark.parametrize("size", [(67, 67, 1, 255), (67, 100, 257, 511)])
def test_narrowest_strips(pkg, oracle, size):
    """67 x 67: fewer chunks than threads; 67 x 100: a second chunk for a few threads of the first wave only"""
    w, h, least, most = size
    args = (500, 1.2, 2, 20, 7)
    refs = [sc.reference(oracle, ("noise", w, h, k), sc.noise_frame(w, h, 50 + k), args) for k in range(2)]
    geo = sc.strips(refs[0]["sizes"])
    assert geo and all(s["ncell"] == 1 and s["nch"] == 4 and least <= s["n_chunk"] <= most for s in geo), repr(geo)
    _host_batch(pkg, refs, "%d x %d" % (w, h), 50)


def test_strips_start_at_every_alignment(pkg, oracle, synth):
    seen = set()
    for w, want in ((320, {8, 12, 16}), (336, {4, 8, 12, 16})):
        refs = _refs(oracle, synth, w, 240)
        qoffs = set(s["qoff"] for s in sc.strips(refs[0]["sizes"]))
        assert qoffs == want, "%d x 240: first quads at the tile bytes %r" % (w, sorted(qoffs))
        seen |= qoffs
        sched = _device_batch(pkg, refs, 3, "%d x 240" % w, 100)
        assert sched & 16, "level 0 was not read in place"
    assert seen == {4, 8, 12, 16}


def test_tall_cell_fills_the_first_group(pkg, oracle):
    args = (500, 1.2, 2, 20, 7)
    refs = [sc.reference(oracle, ("tall", k), sc.wide_frame("tall 160x101", 160, 101, k), args) for k in range(2)]
    geo = sc.strips(refs[0]["sizes"])
    assert max(s["n_chunk"] for s in geo) > 512 and max(s["groups"] for s in geo) == 1, repr(geo)      # three chunks per thread
    _host_batch(pkg, refs, "160 x 101", 50)


def test_wide_strips_take_a_second_group():
    """one strip per cell row (the strip width is read once per process: a process of its own)"""
    env = dict(os.environ, ORBX_STRIP_WIDTH="250")
    r = subprocess.run([sys.executable, os.path.join(os.path.dirname(os.path.abspath(__file__)), "fast_strip_setup_cases.py")],
                       env=env, capture_output=True, text=True)
    assert r.returncode == 0 and "wide strips ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]


@pytest.mark.parametrize("path", ["in place, padded rows", "copied, unaligned base", "host entry"])
def test_both_level0_paths(pkg, oracle, synth, path):
    refs = _refs(oracle, synth, 320, 240)
    assert not np.array_equal(refs[0]["img"], refs[1]["img"])
    if path == "host entry":
        _host_batch(pkg, refs, path, 100)
    elif path == "in place, padded rows":
        assert _device_batch(pkg, refs, 3, path, 100, row_pad=16, frame_pad=160) & 16, "level 0 was not read in place"
    else:
        assert not _device_batch(pkg, refs, 3, path, 100, misalign=4) & 16, "level 0 was read in place from an unaligned base"


def test_status_of_a_single_frame_is_cleared(pkg, oracle, synth):
    """(the status buffer holds 77 before the call: _device_batch)"""
    assert _device_batch(pkg, _refs(oracle, synth, 320, 240)[1:], 1, "one frame", 100) & 16


def test_three_launches_read_the_table_at_their_offsets(pkg, oracle, synth):
    """64 frames: FAST runs as three launches -- level 0, the levels up to the resize tail, and the tail's levels on the side stream --,
    each from its own first strip"""
    refs = _refs(oracle, synth, 320, 240)
    levels = [s["level"] for s in sc.strips(refs[0]["sizes"])]
    assert levels == sorted(levels) and {0, 1, 4} <= set(levels)         # (level order: the launches are ranges of the table)
    sched = _device_batch(pkg, refs, 64, "64 frames", 100)
    assert sched & 32 and sched & 64, "the tail and the resize chain did not run beside FAST: schedule %d" % sched
