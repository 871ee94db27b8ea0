"""k_orient_desc -- IC_Angle and the steered BRIEF-256 descriptor, two key points per wave -- at its exact decision boundaries.

The production kernel runs through orbx_debug_orient_desc (the launch the pipeline itself uses) on the hand-built scenes of
tests/orient_desc_cases.py; everything it writes is compared BYTE FOR BYTE with the numpy restatement of
tests/orient_desc_reference.py, which tests/test_orient_desc_reference.py has held to the CPU oracle on the same keys: the angle as its
bit pattern, x, y, size, response, octave, class_id, all 32 descriptor bytes, the per-level records, and every byte the kernel must
NOT write (guard rows on both sides of the outputs, rows of keys whose row is -1 or >= cap, selection slots beyond a level's count).
DESIGN.md lists the one-token mutations of the kernel this file was run against.
"""
import numpy as np
import pytest

import orient_desc_cases as cases

pytestmark = pytest.mark.gpu

FIELDS = ("x", "y", "size", "angle", "response", "octave", "class_id")


@pytest.fixture(scope="module")
def extractors(pkg):
    """one handle per geometry"""
    ex = {geo: pkg.Extractor(cases.NFEATURES, cases.SCALE, geo[2], cases.INI_TH, cases.MIN_TH) for geo in (cases.GEO_SMALL, cases.GEO_TALL)}
    yield ex
    for e in ex.values():
        e.close()


def run(ex, sc, pad=cases.PAD):
    return ex.debug_orient_desc(sc.geo[0], sc.geo[1], sc.raw, sc.blur, sc.key_arrays(), sc.cap, sc.guard, cases.CANARY, pad)


def describe(rec):
    return ", ".join("%s %r" % (f, rec[f]) for f in FIELDS) + " (angle bits %08x)" % rec["angle"].view(np.uint32)


def check(ex, name, pad=cases.PAD):
    sc = cases.all_scenes()[name]
    want_kps, want_desc, want_lvl, _ = cases.expected(name)
    kps, desc, lvl = run(ex, sc, pad)
    assert sc.n_keys() > 0 or name == "bookkeeping_empty"
    for b in range(sc.B):
        for l in range(sc.geo[2]):
            assert len(lvl[b][l]) == cases.SEL_CAP
            got, want = lvl[b][l].view(np.uint8).reshape(cases.SEL_CAP, -1), want_lvl[b][l].view(np.uint8).reshape(cases.SEL_CAP, -1)
            bad = np.flatnonzero((got != want).any(1))
            assert bad.size == 0, "%s frame %d level %d slot %d of %d keys (%r)\n got  %s\n want %s" % (
                name, b, l, bad[0], len(sc.keys[b][l]), sc.keys[b][l][bad[0]] if bad[0] < len(sc.keys[b][l]) else "unused slot",
                describe(lvl[b][l][bad[0]]), describe(want_lvl[b][l][bad[0]]))
    got, want = kps.view(np.uint8).reshape(len(desc), -1), want_kps.view(np.uint8).reshape(len(desc), -1)
    bad = np.flatnonzero((got != want).any(1))
    assert bad.size == 0, "%s: %d output rows differ, first buffer row %d (guard %d, cap %d)\n got  %s\n want %s" % (
        name, bad.size, bad[0], sc.guard, sc.cap, describe(kps[bad[0]]), describe(want_kps[bad[0]]))
    bad = np.flatnonzero((desc != want_desc).any(1))
    assert bad.size == 0, "%s: %d descriptors differ, first buffer row %d (guard %d, cap %d): %d bits\n got  %s\n want %s" % (
        name, bad.size, bad[0], sc.guard, sc.cap, int(np.unpackbits(desc[bad[0]] ^ want_desc[bad[0]]).sum()), desc[bad[0]], want_desc[bad[0]])


def test_geometry_is_the_one_the_cases_assume(extractors):
    for geo, ex in extractors.items():
        sc = cases.all_scenes()["level_edges" if geo == cases.GEO_SMALL else "level_edges_tall"]
        _, _, lvl = run(ex, sc)
        assert [ex.level_size(l) for l in range(geo[2])] == cases.level_sizes(*geo)
        assert [s.view(np.uint32) for s in ex.GetScaleFactors()] == [s.view(np.uint32) for s in cases.scale_table(geo[2])]
        assert all(len(lvl[0][l]) == cases.SEL_CAP for l in range(geo[2]))


def test_moments_and_angle(extractors):
    """0, 90, 180, 270 degrees, |m01| == |m10| in four quadrants (the >= of fastAtan2), +-1 beside it, saturated half discs, one grey
    level beside the largest moment; bare and over a point-symmetric background"""
    check(extractors[cases.GEO_SMALL], "moments")


def test_disc_mask(extractors):
    """a single 255 on the rim of every patch row moves the angle, one just outside (column +16 and the corners included) does not"""
    check(extractors[cases.GEO_SMALL], "disc_mask")


def test_every_alignment_of_the_patch_loads(extractors):
    """16 consecutive px, two py: every byte alignment of the intensity-centroid rows and of the LDS window"""
    check(extractors[cases.GEO_SMALL], "alignment")


@pytest.mark.parametrize("name,geo", [("level_edges", cases.GEO_SMALL), ("level_edges_tall", cases.GEO_TALL)])
def test_level_edges_and_padding(extractors, name, geo):
    """the extreme key positions of every level; row padding, level gaps and buffer tails filled with 0xA5, 0x00 or 0xFF: no result
    depends on them"""
    for pad in (cases.PAD, 0x00, 0xFF):
        check(extractors[geo], name, pad)


def test_comparison(extractors):
    """a constant window gives the zero descriptor; +-1 at one rotated pattern point flips the pairs that read it, no other"""
    check(extractors[cases.GEO_SMALL], "comparison")


@pytest.mark.parametrize("name", ["bookkeeping_batch3", "bookkeeping_batch1", "bookkeeping_empty"])
def test_bookkeeping(extractors, name):
    """counts 0, 1, 2, 7, 8, 9, 32 per level, an empty level between two others, dead upper halves, 1 / 2 / 3 frames (grid padding, the
    XCD remap), rows reversed, scattered, -1 and >= cap: only the rows of live keys with a row inside [0, cap) change"""
    check(extractors[cases.GEO_SMALL], name)


@pytest.mark.parametrize("name", sorted(n for n in cases.all_scenes() if n.startswith("steering_")))
def test_steering_roundings(extractors, name):
    """the angles of tests/golden/orient_desc_steering_pairs.json: exact ties where half-to-even and half-up differ, and coordinates
    that a contracted multiply-add, one ulp of the cosine, the sine or the angle rounds the other way"""
    check(extractors[cases.GEO_SMALL], name)


def test_arguments_that_could_leave_a_level_are_rejected(pkg, extractors):
    ex = extractors[cases.GEO_SMALL]
    sc = cases.all_scenes()["bookkeeping_batch1"]
    sizes = sc.sizes
    for level, (x, y, resp) in [(0, (18, 30, 1)), (0, (sizes[0][0] - 19, 30, 1)), (1, (30, 18, 1)), (2, (30, sizes[2][1] - 19, 1)), (0, (30, 30, 256)), (0, (30, 30, -1))]:
        keys = [[np.zeros((0, 4), np.int32) for _ in sizes]]
        keys[0][level] = np.array([[x, y, resp, 0]], np.int32)
        with pytest.raises(pkg.OrbxError) as e:
            ex.debug_orient_desc(sc.geo[0], sc.geo[1], sc.raw, sc.blur, keys, sc.cap)
        assert e.value.code == -3
    keys = [[np.zeros((0, 4), np.int32) for _ in sizes]]
    keys[0][1] = np.array([[30, 30, 1, i] for i in range(cases.SEL_CAP + 1)], np.int32)
    with pytest.raises(pkg.OrbxError) as e:
        ex.debug_orient_desc(sc.geo[0], sc.geo[1], sc.raw, sc.blur, keys, sc.cap)
    assert e.value.code == -3
    check(ex, "bookkeeping_batch1")         # the handle is as good as before


def test_debug_entry_reproduces_the_pipeline(pkg, synth):
    """a textured frame through the whole extractor, then its pyramid, blurred levels and per-level key points through the debug
    entry: the same key points, descriptors and per-level records (rows: the reversed level-major order of a mono frame)"""
    img = synth.make_frame(331, 160, 120)
    ex = pkg.Extractor(300, 1.2, 4, 20, 7)
    try:
        mono, kps, desc = ex(img)
        n = len(kps)
        assert n > 150
        raw = [[ex.pyramid_level(l) for l in range(4)]]
        blur = [[ex.blurred_level(l) for l in range(4)]]
        lk = [ex.level_keypoints(l) for l in range(4)]
        assert sum(len(k) for k in lk) == n
        keys, j = [[]], 0
        for l in range(4):
            rows = n - 1 - (j + np.arange(len(lk[l])))
            keys[0].append(np.stack([lk[l]["x"], lk[l]["y"], lk[l]["response"], rows], axis=1).astype(np.int32).reshape(-1, 4))
            j += len(lk[l])
        kps2, desc2, lvl2 = ex.debug_orient_desc(160, 120, raw, blur, keys, n)
        assert np.array_equal(kps2.view(np.uint8), kps.view(np.uint8)) and np.array_equal(desc2, desc)
        for l in range(4):
            assert np.array_equal(lvl2[0][l][:len(lk[l])].view(np.uint8), lk[l].view(np.uint8))
            assert (lvl2[0][l][len(lk[l]):].view(np.uint8) == 0xFF).all()
    finally:
        ex.close()
