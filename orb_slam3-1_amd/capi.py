"""ctypes mirror of include/orbslam3_hip.h.  Names, argument meaning and error behaviour follow the C ABI,
which in turn follows the reference's ORBextractor / ORBmatcher / Optimizer signatures."""
import ctypes as C
import os

import numpy as np

_PKG_DIR = os.path.dirname(os.path.abspath(__file__))
_LIB_PATH = os.path.join(_PKG_DIR, "liborbslam3_hip.so")

KP_DTYPE = np.dtype([("x", "f4"), ("y", "f4"), ("size", "f4"), ("angle", "f4"), ("response", "f4"),
                     ("octave", "i4"), ("class_id", "i4")])
assert KP_DTYPE.itemsize == 28

ORBX_OK, ORBX_ERR_EMPTY, ORBX_ERR_CAPACITY, ORBX_ERR_ARG, ORBX_ERR_NO_DEVICE, ORBX_ERR_HIP, ORBX_ERR_INTERNAL = 0, -1, -2, -3, -4, -5, -6


class OrbxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("orbslam3_hip error %d: %s" % (code, msg))
        self.code = code


class FeatVec(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("node_id", C.c_void_p), ("offset", C.c_void_p), ("feat", C.c_void_p)]


class BowPair(C.Structure):
    _fields_ = [("desc_kf", C.c_void_p), ("n_kf", C.c_int32), ("valid_kf", C.c_void_p), ("angle_kf", C.c_void_p), ("fv_kf", FeatVec),
                ("desc_f", C.c_void_p), ("n_f", C.c_int32), ("angle_f", C.c_void_p), ("fv_f", FeatVec),
                ("match_f2kf", C.c_void_p), ("n_matches", C.c_int32)]


class Frame(C.Structure):
    _fields_ = [("n", C.c_int32), ("x", C.c_void_p), ("y", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p),
                ("desc", C.c_void_p), ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("scale_factors", C.c_void_p), ("n_levels", C.c_int32),
                ("u_right", C.c_void_p)]


class LbaProblem(C.Structure):
    _fields_ = [("n_poses", C.c_int32), ("pose_q", C.c_void_p), ("pose_t", C.c_void_p), ("pose_fixed", C.c_void_p),
                ("n_points", C.c_int32), ("points", C.c_void_p),
                ("n_edges", C.c_int32), ("edge_point", C.c_void_p), ("edge_pose", C.c_void_p), ("edge_obs", C.c_void_p),
                ("edge_inv_sigma2", C.c_void_p), ("edge_stereo", C.c_void_p),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double),
                ("huber_mono", C.c_double), ("huber_stereo", C.c_double)]


class LbaStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("stop_reason", C.c_int32),
                ("lambda_", C.c_double), ("chi2_initial", C.c_double), ("chi2_final", C.c_double),
                ("chi2_trace", C.c_double * 16)]


def _load():
    if not os.path.exists(_LIB_PATH):
        raise ImportError("%s not found: build it with __graft_entry__.build() (hipcc, gfx950). "
                          "There is no CPU fallback." % _LIB_PATH)
    return C.CDLL(_LIB_PATH)


lib = _load()
lib.orbx_last_error.restype = C.c_char_p
lib.orbx_create.argtypes = [C.c_int, C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_void_p)]
lib.orbx_destroy.argtypes = [C.c_void_p]
lib.orbx_extract.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                             C.c_void_p, C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.orbx_extract_batch.argtypes = [C.c_void_p, C.POINTER(C.c_void_p), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                   C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
lib.orbx_extract_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int, C.c_int,
                                          C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
lib.orbx_max_keypoints.argtypes = [C.c_void_p]
lib.orbx_max_keypoints_for.argtypes = [C.c_void_p, C.c_int, C.c_int]
lib.orbx_levels.argtypes = [C.c_void_p]
lib.orbx_scale_factor.argtypes = [C.c_void_p]
lib.orbx_scale_factor.restype = C.c_float
lib.orbx_scale_tables.argtypes = [C.c_void_p] + [C.c_void_p] * 4
lib.orbx_features_per_level.argtypes = [C.c_void_p, C.c_void_p]
lib.orbx_pyramid_level_size.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int)]
lib.orbx_pyramid_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
lib.orbx_debug_blurred_level.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int]
lib.orbx_debug_candidates.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
lib.orbx_debug_level_keypoints.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
lib.orbx_debug_set_tail_delay.argtypes = [C.c_void_p, C.c_int]
lib.orbx_debug_last_schedule.argtypes = [C.c_void_p]
lib.orbx_debug_last_handoffs.argtypes = [C.c_void_p]
lib.orbx_debug_blur_tile_split.argtypes = [C.c_float, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.POINTER(C.c_int)]
lib.orbx_debug_octree_waves.argtypes = [C.c_void_p, C.c_int]
lib.orbx_debug_octree_table.argtypes = [C.c_void_p, C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_void_p, C.c_int]
lib.orbx_debug_resize_bands.argtypes = [C.c_void_p]
lib.orbx_debug_resize_rows.argtypes = [C.c_int, C.c_int, C.c_void_p, C.POINTER(C.c_int)]
lib.orbx_debug_introsort.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.orbx_debug_wave_sort.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
lib.orbx_debug_fast_scores.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p]
lib.orbx_debug_orient_desc.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                       C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
lib.orbx_debug_fast_atan2.restype = C.c_float
lib.orbx_debug_fast_atan2.argtypes = [C.c_float, C.c_float]
lib.orbx_debug_sincos.argtypes = [C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_float)]


def _p(a):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def _check(code):
    if code < 0:
        raise OrbxError(code, (lib.orbx_last_error() or b"").decode())
    return code


def device_count():
    return lib.orbx_device_count()


class Extractor:
    """ORB_SLAM3::ORBextractor (reference include/ORBextractor.h:44-109)."""

    def __init__(self, nfeatures=1000, scale_factor=1.2, nlevels=8, ini_th_fast=20, min_th_fast=7, device=0):
        h = C.c_void_p()
        _check(lib.orbx_create(nfeatures, scale_factor, nlevels, ini_th_fast, min_th_fast, device, C.byref(h)))
        self._h = h
        self.nlevels = nlevels
        self.max_keypoints = lib.orbx_max_keypoints(h)

    def close(self):
        if getattr(self, "_h", None):
            lib.orbx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # getters (include/ORBextractor.h:61-81)
    def GetLevels(self):
        return lib.orbx_levels(self._h)

    def GetScaleFactor(self):
        return lib.orbx_scale_factor(self._h)

    def _tables(self):
        n = self.nlevels
        t = [np.zeros(n, np.float32) for _ in range(4)]
        _check(lib.orbx_scale_tables(self._h, *[_p(a) for a in t]))
        return t

    def GetScaleFactors(self):
        return self._tables()[0]

    def GetInverseScaleFactors(self):
        return self._tables()[1]

    def GetScaleSigmaSquares(self):
        return self._tables()[2]

    def GetInverseScaleSigmaSquares(self):
        return self._tables()[3]

    def features_per_level(self):
        out = np.zeros(self.nlevels, np.int32)
        _check(lib.orbx_features_per_level(self._h, _p(out)))
        return out

    def __call__(self, image, lapping_area=(0, 1000)):
        """operator(): returns (monoIndex, keypoints[KP_DTYPE], descriptors[n,32]); monoIndex == -1 for an empty image."""
        if image is None or image.size == 0:
            return -1, np.zeros(0, KP_DTYPE), np.zeros((0, 32), np.uint8)
        assert image.dtype == np.uint8 and image.ndim == 2       # assert(image.type() == CV_8UC1)
        img = image if image.strides[1] == 1 else np.ascontiguousarray(image)
        h, w = img.shape
        cap = self.max_keypoints
        kps = np.zeros(cap, KP_DTYPE)
        desc = np.zeros((cap, 32), np.uint8)
        n, mono = C.c_int(), C.c_int()
        _check(lib.orbx_extract(self._h, _p(img), w, h, img.strides[0], lapping_area[0], lapping_area[1],
                                _p(kps), _p(desc), cap, C.byref(n), C.byref(mono)))
        return mono.value, kps[:n.value].copy(), desc[:n.value].copy()

    def max_keypoints_for(self, width, height):
        """orbx_max_keypoints_for: the key-point bound for one image size (very wide images with tiny per-level budgets)"""
        return int(lib.orbx_max_keypoints_for(self._h, int(width), int(height)))

    def extract_batch(self, images, lapping_area=(0, 1000)):
        """images: uint8 array [B, H, W] (host).  Returns (mono[B], n[B], kps[B,cap], desc[B,cap,32])."""
        imgs = np.ascontiguousarray(images)
        B, h, w = imgs.shape
        cap = max(self.max_keypoints, self.max_keypoints_for(w, h))
        kps = np.zeros((B, cap), KP_DTYPE)
        desc = np.zeros((B, cap, 32), np.uint8)
        n = np.zeros(B, np.int32)
        mono = np.zeros(B, np.int32)
        ptrs = (C.c_void_p * B)(*[imgs[b].ctypes.data for b in range(B)])
        _check(lib.orbx_extract_batch(self._h, ptrs, B, w, h, imgs.strides[1], lapping_area[0], lapping_area[1],
                                      _p(kps), _p(desc), cap, _p(n), _p(mono)))
        return mono, n, kps, desc

    def extract_batch_device(self, d_imgs_ptr, batch, w, h, row_stride, frame_stride, d_kps_ptr, d_desc_ptr, cap,
                             d_n_ptr, d_mono_ptr, d_status_ptr, lapping_area=(0, 1000), stream=None):
        """Raw device-pointer variant (pointers as ints, e.g. torch.Tensor.data_ptr()); asynchronous."""
        _check(lib.orbx_extract_batch_device(self._h, d_imgs_ptr, batch, w, h, row_stride, frame_stride,
                                             lapping_area[0], lapping_area[1], d_kps_ptr, d_desc_ptr, cap,
                                             d_n_ptr, d_mono_ptr, d_status_ptr, stream))

    def stereo_matches(self, right, kps_l, desc_l, kps_r, desc_r, mb, mbf, frame=0):
        """Frame::ComputeStereoMatches with self = left extractor, `right` = right extractor (pyramids of their last calls)."""
        kps_l = np.ascontiguousarray(kps_l); kps_r = np.ascontiguousarray(kps_r)
        desc_l = np.ascontiguousarray(desc_l); desc_r = np.ascontiguousarray(desc_r)
        n = len(kps_l)
        ur = np.full(max(n, 1), -1, np.float32); dp = np.full(max(n, 1), -1, np.float32)
        _check(lib.orbx_stereo_matches(self._h, right._h, int(frame), _p(kps_l), _p(desc_l), n, _p(kps_r), _p(desc_r), len(kps_r),
                                       C.c_float(mb), C.c_float(mbf), _p(ur), _p(dp)))
        return ur[:n], dp[:n]

    def stereo_matches_device(self, right, batch, d_kps_l, d_desc_l, d_n_l, d_kps_r, d_desc_r, d_n_r, cap, mb, mbf, d_u_right, d_depth, stream=None):
        _check(lib.orbx_stereo_matches_device(self._h, right._h, int(batch), C.c_void_p(d_kps_l), C.c_void_p(d_desc_l), C.c_void_p(d_n_l),
                                              C.c_void_p(d_kps_r), C.c_void_p(d_desc_r), C.c_void_p(d_n_r), int(cap), C.c_float(mb), C.c_float(mbf),
                                              C.c_void_p(d_u_right), C.c_void_p(d_depth), C.c_void_p(stream or 0)))

    def profile_enable(self, on=True):
        lib.orbx_profile_enable.argtypes = [C.c_void_p, C.c_int]
        _check(lib.orbx_profile_enable(self._h, int(on)))

    STAGES = ("copy_level0", "resize", "fast_strips", "octree", "index", "blur", "orient_desc")

    def profile_read(self):
        """per-stage device milliseconds of the last call (HIP events on the launch stream)"""
        lib.orbx_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        ms = np.zeros(7, np.float32)
        _check(lib.orbx_profile_read(self._h, _p(ms), 7))
        return dict(zip(self.STAGES, ms.tolist()))

    # mvImagePyramid replacement + stage introspection
    def level_size(self, level):
        w, h = C.c_int(), C.c_int()
        _check(lib.orbx_pyramid_level_size(self._h, level, C.byref(w), C.byref(h)))
        return w.value, h.value

    def pyramid_level(self, level, frame=0, border=0):
        w, h = self.level_size(level)
        out = np.zeros((h + 2 * border, w + 2 * border), np.uint8)
        _check(lib.orbx_pyramid_level(self._h, frame, level, border, _p(out), out.strides[0]))
        return out

    def blurred_level(self, level, frame=0):
        w, h = self.level_size(level)
        out = np.zeros((h, w), np.uint8)
        _check(lib.orbx_debug_blurred_level(self._h, frame, level, _p(out), out.strides[0]))
        return out

    def debug_set_fast_corner_cap(self, cap):
        """test hook: shrink the FAST kernel's per-wave corner lists so that its overflow path runs"""
        lib.orbx_debug_set_fast_corner_cap.argtypes = [C.c_void_p, C.c_int]
        _check(lib.orbx_debug_set_fast_corner_cap(self._h, int(cap)))

    def debug_set_tail_delay(self, microseconds):
        _check(lib.orbx_debug_set_tail_delay(self._h, int(microseconds)))

    def debug_resize_bands(self):
        """test hook: did the last extract call resize a level with k_resize (bands of rows, frames across the lanes)?"""
        return bool(lib.orbx_debug_resize_bands(self._h))

    def debug_last_schedule(self):
        """bits: 0-1 octree instantiation (0 node pool in HBM, 1 keys + nodes in LDS, 2 keys in the scratch), 4 two octree launches,
        8 level-0 octree early, 16 level 0 read in place, 32 resize tail on the side stream"""
        return int(lib.orbx_debug_last_schedule(self._h))

    def debug_last_handoffs(self):
        """bits: 1 the blur in two launches by level range, 2 events bound to the launches they follow, 4 status cleared by the first
        FAST launch (large batches; 0 otherwise)"""
        return int(lib.orbx_debug_last_handoffs(self._h))

    def debug_octree_waves(self, launch):
        """waves per workgroup of the last call's octree launch: 0 level 0 started early, 1 the lower (or all) levels, 2 the upper
        levels; 0 when there was no such launch"""
        return int(lib.orbx_debug_octree_waves(self._h, launch))

    def debug_octree_table(self, level):
        """the octree's bucket table of `level` as the device holds it (image size of the last call): (D, n_ini, x boundaries as an
        array of n_ini rows of 2^D + 1, y boundaries)"""
        depth, n_ini = C.c_int(), C.c_int()
        out = np.zeros(2 * 65537, np.int16)      # (roots + 1) * (2^D + 1) with roots * 4^D <= 65536: largest at D = 0
        n = _check(lib.orbx_debug_octree_table(self._h, level, C.byref(depth), C.byref(n_ini), _p(out), out.size))
        nb = (1 << depth.value) + 1
        assert n == (n_ini.value + 1) * nb or n == 0
        return depth.value, n_ini.value, out[:n_ini.value * nb].reshape(n_ini.value, nb).copy(), out[n_ini.value * nb:n].copy()

    def candidates(self, level, frame=0, cap=200000):
        out = np.zeros(cap, KP_DTYPE)
        n = C.c_int()
        _check(lib.orbx_debug_candidates(self._h, frame, level, _p(out), cap, C.byref(n)))
        return out[:min(n.value, cap)].copy()

    def level_keypoints(self, level, frame=0, cap=20000):
        out = np.zeros(cap, KP_DTYPE)
        n = C.c_int()
        _check(lib.orbx_debug_level_keypoints(self._h, frame, level, _p(out), cap, C.byref(n)))
        return out[:min(n.value, cap)].copy()

    def debug_orient_desc(self, width, height, raw, blurred, keys, cap, guard_rows=0, canary=0xC3, pad_byte=0xA5):
        """orbx_debug_orient_desc: the orientation + descriptor kernel alone, through the pipeline's own launch.
        raw, blurred: [frame][level] uint8 images of the level sizes of a width x height image; keys: [frame][level] integer arrays
        [n, 4] of (x, y, response, row).  Returns (kps, desc, lvl) with kps / desc the whole output buffers, guard_rows + B * cap +
        guard_rows rows that held `canary` bytes before the launch, and lvl[frame][level] every selection slot of the level (0xFF
        bytes where the kernel wrote nothing)."""
        B, nl = len(raw), self.nlevels
        assert len(blurred) == B and len(keys) == B and all(len(a) == nl for a in list(raw) + list(blurred) + list(keys))
        inv = self.GetInverseScaleFactors()         # the level sizes of ComputePyramid: what the library will read of each image
        for l in range(nl):
            shape = (int(np.rint(np.float32(height) * inv[l])), int(np.rint(np.float32(width) * inv[l])))
            assert all(tuple(raw[b][l].shape) == shape == tuple(blurred[b][l].shape) for b in range(B)), (l, shape)
        pack = lambda fr: np.concatenate([np.ascontiguousarray(im, np.uint8).ravel() for f in fr for im in f])
        raw_b, blur_b = pack(raw), pack(blurred)
        ks = [np.asarray(k, np.int32).reshape(-1, 4) for f in keys for k in f]
        counts = np.array([len(k) for k in ks], np.int32)
        flat = np.ascontiguousarray(np.concatenate(ks)) if ks else np.zeros((0, 4), np.int32)
        rows = 2 * guard_rows + B * cap
        kps = np.full(rows * KP_DTYPE.itemsize, canary, np.uint8).view(KP_DTYPE)
        desc = np.full((rows, 32), canary, np.uint8)
        lvl_cap = max(64, self.max_keypoints)
        lvl = np.zeros((B, nl, lvl_cap), KP_DTYPE)
        caps = np.zeros(nl, np.int32)
        _check(lib.orbx_debug_orient_desc(self._h, int(width), int(height), B, _p(raw_b), _p(blur_b), int(pad_byte), _p(counts), _p(flat),
                                          int(cap), int(guard_rows), _p(kps), _p(desc), _p(lvl), lvl_cap, _p(caps)))
        return kps, desc, [[lvl[b, l, :caps[l]].copy() for l in range(nl)] for b in range(B)]


def hamming(a, b):
    """ORBmatcher::DescriptorDistance."""
    lib.orbm_hamming.argtypes = [C.c_void_p, C.c_void_p]
    return lib.orbm_hamming(_p(np.ascontiguousarray(a)), _p(np.ascontiguousarray(b)))


def _fv(fv):
    nodes, offs, feat = [np.ascontiguousarray(a) for a in fv]
    s = FeatVec(len(nodes), nodes.ctypes.data, offs.ctypes.data, feat.ctypes.data)
    s._keep = (nodes, offs, feat)
    return s


class FramePose(C.Structure):
    """OrbmFramePose (include/orbslam3_hip_track_project.h): 19 floats"""
    _fields_ = [("q", C.c_float * 4), ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3)]


class TrackCamera(C.Structure):
    _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("bf", C.c_float),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("log_scale_factor", C.c_float), ("n_levels", C.c_int32)]


class LocalPoints(C.Structure):
    _fields_ = [("xyz", C.c_void_p), ("normal", C.c_void_p), ("min_distance", C.c_void_p), ("max_distance", C.c_void_p),
                ("skip", C.c_void_p), ("bad", C.c_void_p), ("n", C.c_void_p), ("pcap", C.c_int32)]


class FrustumOut(C.Structure):
    _fields_ = [("valid", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("octave", C.c_void_p), ("view_cos", C.c_void_p),
                ("track_depth", C.c_void_p), ("proj_ur", C.c_void_p), ("n_to_match", C.c_void_p)]


class LastProjOut(C.Structure):
    _fields_ = [("valid", C.c_void_p), ("u", C.c_void_p), ("v", C.c_void_p), ("proj_ur", C.c_void_p)]


TRACK_MAX_BATCH, TRACK_MAX_LEVELS = 65535, 16


def track_project_check(cam, poses, pts, out, batch):
    """orbm_track_project_check (host only): cam / pts / out are TrackCamera / LocalPoints / FrustumOut or None, poses an address or
    None.  Returns the code (ORBX_OK, ORBX_ERR_ARG = -3, ORBX_ERR_CAPACITY = -2)."""
    lib.orbm_track_project_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    ref = lambda s: C.cast(C.pointer(s), C.c_void_p) if s is not None else None
    return lib.orbm_track_project_check(ref(cam), C.c_void_p(poses) if poses else None, ref(pts), ref(out), int(batch))


class TrackRigCamera(C.Structure):
    """OrbmTrackRigCamera (include/orbslam3_hip_track_project_rig.h)"""
    _fields_ = [("left", C.c_float * 8), ("right", C.c_float * 8), ("Rrl", C.c_float * 9), ("trl", C.c_float * 3), ("tlr", C.c_float * 3),
                ("q_rl", C.c_float * 4), ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                ("log_scale_factor", C.c_float), ("n_levels", C.c_int32)]


class RigFramePose(C.Structure):
    """OrbmRigFramePose: 43 floats"""
    _fields_ = [("left", FramePose), ("Rwc", C.c_float * 9), ("R_r", C.c_float * 9), ("t_r", C.c_float * 3), ("Ow_r", C.c_float * 3)]


class RigFrustumOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("in_view", "proj_u", "proj_v", "pred_level", "view_cos", "in_view_r", "proj_u_r", "proj_v_r", "pred_level_r",
                                          "view_cos_r", "track_depth", "track_depth_r", "n_to_match")]


class RigLastProjOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("valid", "proj_u", "proj_v", "proj_u_r", "proj_v_r")]


RIG_FRUSTUM_DTYPES = dict(in_view=np.uint8, proj_u=np.float32, proj_v=np.float32, pred_level=np.int32, view_cos=np.float32, in_view_r=np.uint8,
                          proj_u_r=np.float32, proj_v_r=np.float32, pred_level_r=np.int32, view_cos_r=np.float32, track_depth=np.float32,
                          track_depth_r=np.float32)
RIG_LAST_DTYPES = dict(valid=np.uint8, proj_u=np.float32, proj_v=np.float32, proj_u_r=np.float32, proj_v_r=np.float32)


def track_rig_camera(cam):
    """a rig camera dict (synth_track.rig_camera) -> TrackRigCamera"""
    c = TrackRigCamera()
    for k in ("left", "right", "Rrl", "trl", "tlr", "q_rl"):
        a = np.asarray(cam[k], np.float32).reshape(-1)
        getattr(c, k)[:] = [float(v) for v in a]
    for k in ("min_x", "min_y", "max_x", "max_y", "log_scale_factor"):
        setattr(c, k, float(cam[k]))
    c.n_levels = int(cam["n_levels"])
    return c


def track_project_rig_check(cam, poses, pts, out, batch):
    """orbm_track_project_rig_check (host only): cam / pts / out are TrackRigCamera / LocalPoints / RigFrustumOut or None, poses an
    address or None.  Returns the code."""
    lib.orbm_track_project_rig_check.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int]
    ref = lambda s: C.cast(C.pointer(s), C.c_void_p) if s is not None else None
    return lib.orbm_track_project_rig_check(ref(cam), C.c_void_p(poses) if poses else None, ref(pts), ref(out), int(batch))


class Matcher:
    """ORB_SLAM3::ORBmatcher (reference include/ORBmatcher.h:40-106): ORBmatcher(nnratio=0.6, checkOri=true)."""
    TH_HIGH, TH_LOW, HISTO_LENGTH = 100, 50, 30

    def __init__(self, nnratio=0.6, check_orientation=True, device=0):
        self.nnratio = float(nnratio)
        self.check_ori = bool(check_orientation)
        lib.orbm_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.orbm_destroy.argtypes = [C.c_void_p]
        lib.orbm_search_by_bow.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(FeatVec),
                                           C.c_void_p, C.c_int, C.c_void_p, C.POINTER(FeatVec), C.c_float, C.c_int, C.c_void_p]
        lib.orbm_search_by_bow_batch.argtypes = [C.c_void_p, C.POINTER(BowPair), C.c_int, C.c_float, C.c_int]
        lib.orbm_search_by_bow_kfkf.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(FeatVec),
                                                C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(FeatVec),
                                                C.c_float, C.c_int, C.c_void_p]
        lib.orbm_search_by_projection.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int] + [C.c_void_p] * 10 + \
            [C.c_float, C.c_int, C.c_float, C.c_float, C.c_void_p, C.c_void_p]
        lib.orbm_search_by_projection_last.argtypes = [C.c_void_p, C.POINTER(Frame), C.c_int] + [C.c_void_p] * 8 + \
            [C.c_float, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        h = C.c_void_p()
        _check(lib.orbm_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.orbm_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def DescriptorDistance(a, b):
        return hamming(a, b)

    def SearchByBoW(self, dKF, validKF, angKF, fvKF, dF, angF, fvF):
        """SearchByBoW(KeyFrame*, Frame&, vector<MapPoint*>&): returns (nmatches, match_f2kf[nF])."""
        dKF, dF = np.ascontiguousarray(dKF), np.ascontiguousarray(dF)
        match = np.full(len(dF), -1, np.int32)
        a, b = _fv(fvKF), _fv(fvF)
        n = _check(lib.orbm_search_by_bow(self._h, _p(dKF), len(dKF), _p(validKF), _p(angKF), C.byref(a),
                                          _p(dF), len(dF), _p(angF), C.byref(b), self.nnratio, int(self.check_ori), _p(match)))
        return n, match

    def SearchByBoW_batch(self, sets):
        """sets: list of dicts as synth.make_match_set.  Returns list of (nmatches, match)."""
        P = len(sets)
        arr = (BowPair * P)()
        keep = []
        outs = []
        for i, s in enumerate(sets):
            dKF, dF = np.ascontiguousarray(s["dKF"]), np.ascontiguousarray(s["dF"])
            a, b = _fv(s["fvKF"]), _fv(s["fvF"])
            m = np.full(len(dF), -1, np.int32)
            keep.append((dKF, dF, a, b, m))
            outs.append(m)
            arr[i] = BowPair(dKF.ctypes.data, len(dKF), s["validKF"].ctypes.data, s["angKF"].ctypes.data, a,
                             dF.ctypes.data, len(dF), s["angF"].ctypes.data, b, m.ctypes.data, 0)
        _check(lib.orbm_search_by_bow_batch(self._h, arr, P, self.nnratio, int(self.check_ori)))
        return [(arr[i].n_matches, outs[i]) for i in range(P)]

    def bow_plan(self, sets):
        """Uploads the pairs once; returns a BowPlan whose run() only launches the kernel."""
        return BowPlan(self, sets)

    def SearchByBoW_KFKF(self, d1, valid1, ang1, fv1, d2, valid2, ang2, fv2):
        match = np.full(len(d1), -1, np.int32)
        a, b = _fv(fv1), _fv(fv2)
        n = _check(lib.orbm_search_by_bow_kfkf(self._h, _p(d1), len(d1), _p(valid1), _p(ang1), C.byref(a),
                                               _p(d2), len(d2), _p(valid2), _p(ang2), C.byref(b),
                                               self.nnratio, int(self.check_ori), _p(match)))
        return n, match

    @staticmethod
    def _frame(g, desc, scale_factors, angle=None):
        f = Frame(len(g["x"]), g["x"].ctypes.data, g["y"].ctypes.data, g["octave"].ctypes.data,
                  angle.ctypes.data if angle is not None else None, desc.ctypes.data,
                  g["min_x"], g["min_y"], g["max_x"], g["max_y"], g.get("cols", 64), g.get("rows", 48),
                  scale_factors.ctypes.data, len(scale_factors),
                  g["u_right"].ctypes.data if g.get("u_right") is not None else None)      # mvuRight: rectified stereo / RGB-D frames
        return f

    def SearchByProjection(self, g, dF, scale_factors, mp, th, assign, occupied, far_points=False, th_far=0.0):
        """SearchByProjection(Frame&, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)."""
        f = self._frame(g, dF, scale_factors)
        return _check(lib.orbm_search_by_projection(
            self._h, C.byref(f), len(mp["u"]), _p(mp["in_view"]), _p(mp["u"]), _p(mp["v"]), _p(mp.get("ur")), _p(mp["level"]),
            _p(mp["view_cos"]), _p(mp["depth"]), _p(mp["desc"]), _p(mp["has_obs"]), _p(mp["bad"]),
            th, int(far_points), th_far, self.nnratio, _p(assign), _p(occupied)))

    def SearchByProjection_last(self, g, dF, angF, scale_factors, last, th, assign, occupied):
        """SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono): last["level_window"] carries
        bForward (1) / bBackward (2), last["ur"] the predicted right-image columns of a rectified-stereo frame."""
        f = self._frame(g, dF, scale_factors, angF)
        return _check(lib.orbm_search_by_projection_last(
            self._h, C.byref(f), len(last["u"]), _p(last["valid"]), _p(last["u"]), _p(last["v"]), _p(last.get("ur")), _p(last["octave"]),
            _p(last["angle"]), _p(last["desc"]), _p(last["has_obs"]), th, int(last.get("level_window", 0)), int(self.check_ori),
            _p(assign), _p(occupied)))

    def SearchByProjection_kf(self, g, dF, angF, scale_factors, pts, th, orb_dist, assign, occupied):
        """SearchByProjection(Frame& CurrentFrame, KeyFrame* pKF, sAlreadyFound, th, ORBdist) (relocalisation)."""
        f = self._frame(g, dF, scale_factors, angF)
        return _check(lib.orbm_search_by_projection_kf(
            self._h, C.byref(f), len(pts["u"]), _p(pts["valid"]), _p(pts["u"]), _p(pts["v"]), _p(pts["level"]),
            _p(pts["angle"]), _p(pts["desc"]), C.c_float(th), int(orb_dist), int(self.check_ori), _p(assign), _p(occupied)))

    def SearchByProjection_sim3(self, g, dKF, scale_factors, pts, th, ratio_hamming, assign, occupied):
        """SearchByProjection(KeyFrame* pKF, Sim3f& Scw, vpPoints, vpMatched, th, ratioHamming) (loop closing)."""
        f = self._frame(g, dKF, scale_factors)
        return _check(lib.orbm_search_by_projection_sim3(
            self._h, C.byref(f), len(pts["u"]), _p(pts["valid"]), _p(pts["u"]), _p(pts["v"]), _p(pts["level"]),
            _p(pts["desc"]), int(th), C.c_float(ratio_hamming), _p(assign), _p(occupied)))

    def FuseSearch(self, g, dKF, scale_factors, u_right, inv_sigma2, pts, th, chi2_check=True):
        """search core of both ORBmatcher::Fuse overloads: (best_idx, best_dist) per candidate map point"""
        f = self._frame(g, dKF, scale_factors)
        n = len(pts["u"])
        bi = np.full(max(n, 1), -1, np.int32); bd = np.full(max(n, 1), 256, np.int32)
        _check(lib.orbm_fuse_search(self._h, C.byref(f), _p(u_right), _p(inv_sigma2), n, _p(pts["valid"]), _p(pts["u"]), _p(pts["v"]),
                                    _p(pts["ur"]), _p(pts["level"]), _p(pts["desc"]), C.c_float(th), int(chi2_check), _p(bi), _p(bd)))
        return bi[:n], bd[:n]

    def DistinctiveDescriptors(self, desc, off):
        """MapPoint::ComputeDistinctiveDescriptors for a batch of map points: (BestIdx, BestMedian) per point"""
        desc = np.ascontiguousarray(desc, np.uint8); off = np.ascontiguousarray(off, np.int32)
        P = len(off) - 1
        bi = np.zeros(max(P, 1), np.int32); bm = np.zeros(max(P, 1), np.int32)
        _check(lib.orbm_distinctive_descriptors(self._h, _p(desc), _p(off), P, _p(bi), _p(bm)))
        return bi[:P], bm[:P]

    def UpdateNormalAndDepth(self, pos, centers, off, ref_center, level_scale, last_level_scale):
        """MapPoint::UpdateNormalAndDepth for a batch of map points: (normal [P][3], max_dist, min_dist)"""
        pos = np.ascontiguousarray(pos, np.float32); centers = np.ascontiguousarray(centers, np.float32); off = np.ascontiguousarray(off, np.int32)
        ref_center = np.ascontiguousarray(ref_center, np.float32); level_scale = np.ascontiguousarray(level_scale, np.float32)
        P = len(off) - 1
        nrm = np.zeros((max(P, 1), 3), np.float32); mx = np.zeros(max(P, 1), np.float32); mn = np.zeros(max(P, 1), np.float32)
        _check(lib.orbm_update_normal_and_depth(self._h, _p(pos), _p(centers), _p(off), _p(ref_center), _p(level_scale),
                                                C.c_float(last_level_scale), P, _p(nrm), _p(mx), _p(mn)))
        return nrm[:P], mx[:P], mn[:P]

    class _ProjQuery(C.Structure):
        _fields_ = [("frame", C.c_void_p), ("n_pts", C.c_int32), ("valid", C.c_void_p), ("proj_u", C.c_void_p), ("proj_v", C.c_void_p),
                    ("proj_ur", C.c_void_p), ("level", C.c_void_p), ("level_window", C.c_int32), ("view_cos", C.c_void_p), ("track_depth", C.c_void_p), ("mp_bad", C.c_void_p), ("angle", C.c_void_p),
                    ("desc_mp", C.c_void_p), ("mp_has_obs", C.c_void_p), ("assign", C.c_void_p), ("occupied", C.c_void_p), ("n_matches", C.c_int32)]

    def prepare_last_batch(self, cases):
        """cases: list of (g, dF, angF, scale_factors, last, assign, occupied) as for SearchByProjection_last"""
        n = len(cases)
        qs = (self._ProjQuery * n)()
        frames = []
        for i, (g, dF, angF, scale, last, assign, occ) in enumerate(cases):
            f = self._frame(g, dF, scale, angF)
            frames.append(f)
            q = qs[i]
            q.frame = C.addressof(f); q.n_pts = len(last["u"])
            q.valid, q.proj_u, q.proj_v, q.level = (last[k].ctypes.data for k in ("valid", "u", "v", "octave"))
            q.proj_ur = last["ur"].ctypes.data if last.get("ur") is not None else None
            q.level_window = int(last.get("level_window", 0))
            q.angle = last["angle"].ctypes.data; q.desc_mp = last["desc"].ctypes.data; q.mp_has_obs = last["has_obs"].ctypes.data
            q.assign = assign.ctypes.data; q.occupied = occ.ctypes.data
        return dict(qs=qs, frames=frames, cases=cases, n=n)

    def run_last_batch(self, prep, th):
        """SearchByProjection(CurrentFrame, LastFrame, th, bMono=true) for every case in one launch; returns n_matches per case"""
        _check(lib.orbm_search_by_projection_last_batch(self._h, prep["qs"], prep["n"], C.c_float(th), int(self.check_ori)))
        return [q.n_matches for q in prep["qs"]]

    class _DevFrames(C.Structure):
        _fields_ = [("d_kps", C.c_void_p), ("d_desc", C.c_void_p), ("d_n", C.c_void_p), ("cap", C.c_int32),
                    ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float),
                    ("grid_cols", C.c_int32), ("grid_rows", C.c_int32), ("scale_factors", C.c_void_p), ("n_levels", C.c_int32)]

    class _DevLastPoints(C.Structure):
        _fields_ = [("d_valid", C.c_void_p), ("d_u", C.c_void_p), ("d_v", C.c_void_p), ("d_octave", C.c_void_p), ("d_angle", C.c_void_p),
                    ("d_desc", C.c_void_p), ("d_n", C.c_void_p), ("cap", C.c_int32), ("d_has_obs", C.c_void_p)]

    def SearchByProjection_last_batch_device(self, cur, last, batch, th, d_assign, d_occupied, d_n_matches, stream=None, bounds=(0.0, 0.0, 640.0, 480.0),
                                             scale_factors=None, grid=(64, 48)):
        """cur = (d_kps, d_desc, d_n, cap) as orbx_extract_batch_device left them; last = (d_valid, d_u, d_v, d_octave, d_angle, d_desc, d_n, cap);
        every d_* a device pointer.  Only enqueues."""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        self._dev_keep = sf
        cf = self._DevFrames(cur[0], cur[1], cur[2], int(cur[3]), bounds[0], bounds[1], bounds[2], bounds[3], grid[0], grid[1], sf.ctypes.data, len(sf))
        lp = self._DevLastPoints(last[0], last[1], last[2], last[3], last[4], last[5], last[6], int(last[7]), last[8] if len(last) > 8 else None)
        lib.orbm_search_by_projection_last_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(lib.orbm_search_by_projection_last_batch_device(self._h, C.byref(cf), C.byref(lp), int(batch), C.c_float(th), int(self.check_ori),
                                                               C.c_void_p(d_assign), C.c_void_p(d_occupied), C.c_void_p(d_n_matches), C.c_void_p(stream or 0)))

    class _DevMpExtras(C.Structure):
        _fields_ = [("d_view_cos", C.c_void_p), ("d_track_depth", C.c_void_p), ("d_bad", C.c_void_p), ("th_far", C.c_float), ("nnratio", C.c_float), ("far_points", C.c_int32)]

    def SearchByProjection_batch_device(self, cur, pts, extras, batch, th, d_assign, d_occupied, d_n_matches, stream=None, bounds=(0.0, 0.0, 640.0, 480.0),
                                        scale_factors=None, grid=(64, 48), far_points=False, th_far=0.0):
        """Frame x map points on device arrays: cur as above; pts = (d_valid, d_u, d_v, d_level, 0, d_desc, d_n, cap, d_has_obs);
        extras = (d_view_cos, d_track_depth, d_bad)"""
        sf = np.ascontiguousarray(scale_factors, np.float32)
        self._dev_keep = sf
        cf = self._DevFrames(cur[0], cur[1], cur[2], int(cur[3]), bounds[0], bounds[1], bounds[2], bounds[3], grid[0], grid[1], sf.ctypes.data, len(sf))
        lp = self._DevLastPoints(pts[0], pts[1], pts[2], pts[3], pts[4] or None, pts[5], pts[6], int(pts[7]), pts[8])
        ex = self._DevMpExtras(extras[0], extras[1], extras[2], float(th_far), self.nnratio, int(far_points))
        lib.orbm_search_by_projection_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _check(lib.orbm_search_by_projection_batch_device(self._h, C.byref(cf), C.byref(lp), C.byref(ex), int(batch), C.c_float(th),
                                                          C.c_void_p(d_assign), C.c_void_p(d_occupied), C.c_void_p(d_n_matches), C.c_void_p(stream or 0)))

    # ---- include/orbslam3_hip_track_project.h: the projections in front of the two searches above ----
    @staticmethod
    def _track_camera(cam):
        return TrackCamera(*[float(cam[k]) for k in ("fx", "fy", "cx", "cy", "bf", "min_x", "min_y", "max_x", "max_y", "log_scale_factor")], int(cam["n_levels"]))

    def frame_pose_batch_device(self, d_pose, batch, normalise, d_frame_pose, stream=None):
        """orbm_frame_pose_batch_device: d_pose [batch][7] double -> d_frame_pose [batch] FramePose records.  Only enqueues."""
        lib.orbm_frame_pose_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        _check(lib.orbm_frame_pose_batch_device(self._h, C.c_void_p(d_pose), int(batch), int(normalise), C.c_void_p(d_frame_pose), C.c_void_p(stream or 0)))

    def frustum_batch_device(self, cam, d_frame_pose, pts, cos_limit, out, batch, stream=None):
        """orbm_frustum_batch_device: cam a dict as synth_track.camera(); pts = (d_xyz, d_normal, d_min_distance, d_max_distance, d_skip,
        d_bad, d_n, pcap); out = (d_valid, d_u, d_v, d_octave, d_view_cos, d_track_depth, d_proj_ur, d_n_to_match).  Only enqueues."""
        lib.orbm_frustum_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
        c, p, o = self._track_camera(cam), LocalPoints(*pts[:7], int(pts[7])), FrustumOut(*out)
        _check(lib.orbm_frustum_batch_device(self._h, C.byref(c), C.c_void_p(d_frame_pose), C.byref(p), C.c_float(cos_limit), C.byref(o), int(batch), C.c_void_p(stream or 0)))

    def project_last_batch_device(self, cam, d_frame_pose, d_mp_xyz, d_has_point, d_n, cap, out, batch, stream=None):
        """orbm_project_last_batch_device: out = (d_valid, d_u, d_v, d_proj_ur).  Only enqueues."""
        lib.orbm_project_last_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        c, o = self._track_camera(cam), LastProjOut(*out)
        _check(lib.orbm_project_last_batch_device(self._h, C.byref(c), C.c_void_p(d_frame_pose), C.c_void_p(d_mp_xyz), C.c_void_p(d_has_point), C.c_void_p(d_n),
                                                  int(cap), C.byref(o), int(batch), C.c_void_p(stream or 0)))

    def track_handover_batch_device(self, d_assign, d_outlier, d_n_cur, cap, d_last_local, last_cap, d_bad, d_has_obs, pcap,
                                    d_assign_local, d_occupied, d_skip, d_n_dropped, batch, stream=None):
        """orbm_track_handover_batch_device.  Only enqueues."""
        lib.orbm_track_handover_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int,
                                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _check(lib.orbm_track_handover_batch_device(self._h, C.c_void_p(d_assign), C.c_void_p(d_outlier), C.c_void_p(d_n_cur), int(cap), C.c_void_p(d_last_local),
                                                    int(last_cap), C.c_void_p(d_bad), C.c_void_p(d_has_obs), int(pcap), C.c_void_p(d_assign_local),
                                                    C.c_void_p(d_occupied), C.c_void_p(d_skip), C.c_void_p(d_n_dropped), int(batch), C.c_void_p(stream or 0)))

    def frustum_batch(self, case, frame_poses):
        """orbm_frustum_batch on host arrays: case as synth_track.make_local_map_case, frame_poses [batch][19] float32 FramePose records.
        Returns dict(valid, u, v, octave, view_cos, track_depth, proj_ur, n_to_match)."""
        lib.orbm_frustum_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int]
        B, pcap = case["skip"].shape
        fp = np.ascontiguousarray(frame_poses, np.float32).reshape(B, 19)
        keep = [np.ascontiguousarray(case[k], np.float32) for k in ("xyz", "normal", "min_distance", "max_distance")] + \
               [np.ascontiguousarray(case[k], np.uint8) for k in ("skip", "bad")] + [np.ascontiguousarray(case["n"], np.int32)]
        res = dict(valid=np.zeros((B, pcap), np.uint8), u=np.zeros((B, pcap), np.float32), v=np.zeros((B, pcap), np.float32), octave=np.zeros((B, pcap), np.int32),
                   view_cos=np.zeros((B, pcap), np.float32), track_depth=np.zeros((B, pcap), np.float32), proj_ur=np.zeros((B, pcap), np.float32),
                   n_to_match=np.zeros(B, np.int32))
        c, p, o = self._track_camera(case["cam"]), LocalPoints(*[a.ctypes.data for a in keep], pcap), FrustumOut(*[a.ctypes.data for a in res.values()])
        _check(lib.orbm_frustum_batch(self._h, C.byref(c), _p(fp), C.byref(p), C.c_float(case["cos_limit"]), C.byref(o), B))
        return res

    def project_last_batch(self, case, frame_poses):
        """orbm_project_last_batch on host arrays: case as synth_track.make_last_frame_case.  Returns dict(valid, u, v, proj_ur)."""
        lib.orbm_project_last_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        B, cap = case["has_point"].shape
        fp = np.ascontiguousarray(frame_poses, np.float32).reshape(B, 19)
        xyz, has, n = np.ascontiguousarray(case["xyz"], np.float32), np.ascontiguousarray(case["has_point"], np.uint8), np.ascontiguousarray(case["n"], np.int32)
        res = dict(valid=np.zeros((B, cap), np.uint8), u=np.zeros((B, cap), np.float32), v=np.zeros((B, cap), np.float32), proj_ur=np.zeros((B, cap), np.float32))
        c, o = self._track_camera(case["cam"]), LastProjOut(*[a.ctypes.data for a in res.values()])
        _check(lib.orbm_project_last_batch(self._h, C.byref(c), _p(fp), _p(xyz), _p(has), _p(n), cap, C.byref(o), B))
        return res

    def track_project_last_kernel_ms(self):
        lib.orbm_track_project_last_kernel_ms.restype = C.c_float
        lib.orbm_track_project_last_kernel_ms.argtypes = [C.c_void_p]
        return float(lib.orbm_track_project_last_kernel_ms(self._h))

    # ---- include/orbslam3_hip_track_project_rig.h: the same projections for two-camera fisheye rig frames ----
    def rig_frame_pose_batch_device(self, cam, d_pose, batch, normalise, d_rig_pose, stream=None):
        """orbm_rig_frame_pose_batch_device: d_pose [batch][7] double -> d_rig_pose [batch] RigFramePose records.  Only enqueues."""
        lib.orbm_rig_frame_pose_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
        c = track_rig_camera(cam)
        _check(lib.orbm_rig_frame_pose_batch_device(self._h, C.byref(c), C.c_void_p(d_pose), int(batch), int(normalise), C.c_void_p(d_rig_pose), C.c_void_p(stream or 0)))

    def frustum_rig_batch_device(self, cam, d_rig_pose, pts, cos_limit, out, batch, stream=None):
        """orbm_frustum_rig_batch_device: pts as frustum_batch_device; out = the 13 device addresses in the order of RigFrustumOut."""
        lib.orbm_frustum_rig_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int, C.c_void_p]
        c, p, o = track_rig_camera(cam), LocalPoints(*pts[:7], int(pts[7])), RigFrustumOut(*out)
        _check(lib.orbm_frustum_rig_batch_device(self._h, C.byref(c), C.c_void_p(d_rig_pose), C.byref(p), C.c_float(cos_limit), C.byref(o), int(batch), C.c_void_p(stream or 0)))

    def project_last_rig_batch_device(self, cam, d_rig_pose, d_mp_xyz, d_has_point, d_n, cap, out, batch, stream=None):
        """orbm_project_last_rig_batch_device: out = (d_valid, d_proj_u, d_proj_v, d_proj_u_r, d_proj_v_r).  Only enqueues."""
        lib.orbm_project_last_rig_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        c, o = track_rig_camera(cam), RigLastProjOut(*out)
        _check(lib.orbm_project_last_rig_batch_device(self._h, C.byref(c), C.c_void_p(d_rig_pose), C.c_void_p(d_mp_xyz), C.c_void_p(d_has_point), C.c_void_p(d_n),
                                                      int(cap), C.byref(o), int(batch), C.c_void_p(stream or 0)))

    def unproject_stereo_fisheye_batch_device(self, d_rig_pose, d_points, d_valid, d_n, cap, d_world, batch, stream=None):
        """orbm_unproject_stereo_fisheye_batch_device.  Only enqueues."""
        lib.orbm_unproject_stereo_fisheye_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _check(lib.orbm_unproject_stereo_fisheye_batch_device(self._h, C.c_void_p(d_rig_pose), C.c_void_p(d_points), C.c_void_p(d_valid), C.c_void_p(d_n), int(cap),
                                                              C.c_void_p(d_world), int(batch), C.c_void_p(stream or 0)))

    def frustum_rig_batch(self, case, rig_poses, state):
        """orbm_frustum_rig_batch on host arrays: case as synth_track.make_rig_local_map_case, rig_poses [batch][43] float32, state a
        dict of the twelve [batch][pcap] arrays of RIG_FRUSTUM_DTYPES as the caller holds them (copied, not modified).  Returns
        the arrays after the call plus n_to_match."""
        lib.orbm_frustum_rig_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_int]
        B, pcap = case["skip"].shape
        fp = np.ascontiguousarray(rig_poses, np.float32).reshape(B, 43)
        keep = [np.ascontiguousarray(case[k], np.float32) for k in ("xyz", "normal", "min_distance", "max_distance")] + \
               [np.ascontiguousarray(case[k], np.uint8) for k in ("skip", "bad")] + [np.ascontiguousarray(case["n"], np.int32)]
        res = {k: np.array(state[k], dt, order="C").reshape(B, pcap) for k, dt in RIG_FRUSTUM_DTYPES.items()}
        res["n_to_match"] = np.zeros(B, np.int32)
        c, p, o = track_rig_camera(case["cam"]), LocalPoints(*[a.ctypes.data for a in keep], pcap), RigFrustumOut(*[a.ctypes.data for a in res.values()])
        _check(lib.orbm_frustum_rig_batch(self._h, C.byref(c), _p(fp), C.byref(p), C.c_float(case["cos_limit"]), C.byref(o), B))
        return res

    def project_last_rig_batch(self, case, rig_poses):
        """orbm_project_last_rig_batch on host arrays: case as synth_track.make_rig_last_frame_case"""
        lib.orbm_project_last_rig_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        B, cap = case["has_point"].shape
        fp = np.ascontiguousarray(rig_poses, np.float32).reshape(B, 43)
        xyz, has, n = np.ascontiguousarray(case["xyz"], np.float32), np.ascontiguousarray(case["has_point"], np.uint8), np.ascontiguousarray(case["n"], np.int32)
        res = {k: np.zeros((B, cap), dt) for k, dt in RIG_LAST_DTYPES.items()}
        c, o = track_rig_camera(case["cam"]), RigLastProjOut(*[a.ctypes.data for a in res.values()])
        _check(lib.orbm_project_last_rig_batch(self._h, C.byref(c), _p(fp), _p(xyz), _p(has), _p(n), cap, C.byref(o), B))
        return res

    def unproject_stereo_fisheye_batch(self, rig_poses, points, valid, n, world):
        """orbm_unproject_stereo_fisheye_batch on host arrays; `world` [batch][cap][3] float32 is copied and returned"""
        lib.orbm_unproject_stereo_fisheye_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
        B, cap = np.asarray(valid).shape
        fp = np.ascontiguousarray(rig_poses, np.float32).reshape(B, 43)
        pts, val, nn = np.ascontiguousarray(points, np.float32), np.ascontiguousarray(valid, np.uint8), np.ascontiguousarray(n, np.int32)
        w = np.array(world, np.float32, order="C").reshape(B, cap, 3)
        _check(lib.orbm_unproject_stereo_fisheye_batch(self._h, _p(fp), _p(pts), _p(val), _p(nn), cap, _p(w), B))
        return w

    def track_project_rig_last_kernel_ms(self):
        lib.orbm_track_project_rig_last_kernel_ms.restype = C.c_float
        lib.orbm_track_project_rig_last_kernel_ms.argtypes = [C.c_void_p]
        return float(lib.orbm_track_project_rig_last_kernel_ms(self._h))

    class _TriSide(C.Structure):
        _fields_ = [("n", C.c_int32), ("desc", C.c_void_p), ("has_mp", C.c_void_p), ("stereo", C.c_void_p), ("x", C.c_void_p),
                    ("y", C.c_void_p), ("octave", C.c_void_p), ("angle", C.c_void_p), ("fv", FeatVec)]

    def SearchForTriangulation(self, k1, k2, ep, F12, sigma2_2, scale_2, only_stereo=False, coarse=False):
        """SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse): returns (nmatches, match12)"""
        sides = []
        for k in (k1, k2):
            fv = _fv(k["fv"])
            sides.append((self._TriSide(len(k["x"]), k["desc"].ctypes.data, k["has_mp"].ctypes.data, k["stereo"].ctypes.data,
                                        k["x"].ctypes.data, k["y"].ctypes.data, k["octave"].ctypes.data, k["angle"].ctypes.data, fv), fv))
        m12 = np.full(max(len(k1["x"]), 1), -1, np.int32)
        n = _check(lib.orbm_search_for_triangulation(self._h, C.byref(sides[0][0]), C.byref(sides[1][0]), C.c_float(ep[0]), C.c_float(ep[1]),
                                                     _p(F12), _p(sigma2_2), _p(scale_2), len(scale_2), int(only_stereo), int(coarse),
                                                     int(self.check_ori), _p(m12)))
        return n, m12[:len(k1["x"])]

    def SearchForInitialization(self, f1, g2, d2, ang2, scale_factors, window_size=100):
        """SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize): returns (nmatches, vnMatches12)"""
        f = self._frame(g2, d2, scale_factors, ang2)
        n1 = len(f1["octave"])
        m12 = np.full(max(n1, 1), -1, np.int32)
        n = _check(lib.orbm_search_for_initialization(self._h, _p(f1["desc"]), n1, _p(f1["octave"]), _p(f1["angle"]), _p(f1["prev_x"]),
                                                      _p(f1["prev_y"]), C.byref(f), int(window_size), C.c_float(self.nnratio),
                                                      int(self.check_ori), _p(m12)))
        return n, m12[:n1]


    def create_new_map_points_prepare(self, kf1, neighbours, pairs, params):
        """flatten the arguments of orbm_create_new_map_points once (no device needed).  kf1 / neighbours[j]: dict(desc, has_mp,
        stereo, x, y, octave, fv, u_right, depth, [key_x, key_y], Rcw, tcw, Ow, fx, fy, cx, cy, invfx, invfy, mb, mbf, level_sigma2,
        scale_factors); pairs[j]: dict(ep, F12, coarse); params: dict(inertial, far_points, th_far, scale_factor_1)."""
        if len(pairs) != len(neighbours):
            raise ValueError("%d pairs for %d neighbours" % (len(pairs), len(neighbours)))
        keep = []
        kfs = (OrbmMapKeyFrame * (1 + len(neighbours)))()
        for q, k in enumerate([kf1] + list(neighbours)):
            _fill_map_key_frame(kfs[q], k, keep, "kf1" if q == 0 else "neighbour %d" % (q - 1))
        prs = (OrbmMapPair * max(len(pairs), 1))()
        for j, w in enumerate(pairs):
            F12 = np.ascontiguousarray(w["F12"], np.float32).reshape(-1)
            if F12.shape != (9,):
                raise ValueError("pair %d: F12 is not 3x3" % j)
            prs[j].ep_x, prs[j].ep_y = float(w["ep"][0]), float(w["ep"][1])
            prs[j].F12[:] = [float(v) for v in F12]
            prs[j].coarse = int(bool(w.get("coarse", False)))
        par = OrbmMapParams(int(bool(params["inertial"])), int(bool(params["far_points"])), float(params["th_far"]), float(params["scale_factor_1"]))
        n1, nb = kfs[0].side.n, len(neighbours)
        o = dict(neighbour=np.full(max(n1, 1), -1, np.int32), idx2=np.full(max(n1, 1), -1, np.int32), x3d=np.zeros((max(n1, 1), 3), np.float32),
                 point_stereo=np.zeros(max(n1, 1), np.uint8), normal=np.zeros((max(n1, 1), 3), np.float32), max_dist=np.zeros(max(n1, 1), np.float32),
                 min_dist=np.zeros(max(n1, 1), np.float32), n_matched=np.zeros(max(nb, 1), np.int32), n_created=np.zeros(max(nb, 1), np.int32),
                 match12=np.full((max(nb, 1), max(n1, 1)), -1, np.int32))
        out = OrbmNewPoints(*[o[f].ctypes.data for f, _ in OrbmNewPoints._fields_])
        return dict(kfs=kfs, pairs=prs, params=par, out=out, arrays=o, n1=n1, n_neighbours=nb, keep=keep)

    def create_new_map_points_launch(self, prep):
        """the C call alone: one upload, one kernel launch, one download"""
        lib.orbm_create_new_map_points.argtypes = [C.c_void_p] * 3 + [C.c_int] + [C.c_void_p] * 3
        nbs = C.byref(prep["kfs"], C.sizeof(OrbmMapKeyFrame)) if prep["n_neighbours"] else None
        return _check(lib.orbm_create_new_map_points(self._h, C.byref(prep["kfs"]), nbs, prep["n_neighbours"],
                                                     C.byref(prep["pairs"]), C.byref(prep["params"]), C.byref(prep["out"])))

    def create_new_map_points(self, kf1, neighbours, pairs, params):
        """LocalMapping::CreateNewMapPoints: dict(created, neighbour, idx2, x3d, point_stereo, normal, max_dist, min_dist [n1],
        n_matched, n_created [n_neighbours], match12 [n_neighbours][n1]); (neighbour, idx1) ascending over neighbour >= 0 is the reference's creation order"""
        prep = self.create_new_map_points_prepare(kf1, neighbours, pairs, params)
        created = self.create_new_map_points_launch(prep)
        a, n1, nb = prep["arrays"], prep["n1"], prep["n_neighbours"]
        r = {k: (a[k][:nb] if k in ("n_matched", "n_created") else a[k][:nb, :n1] if k == "match12" else a[k][:n1]).copy() for k in a}
        r["created"] = created
        return r

    def create_new_map_points_last_kernel_ms(self):
        lib.orbm_create_new_map_points_last_kernel_ms.restype = C.c_float
        lib.orbm_create_new_map_points_last_kernel_ms.argtypes = [C.c_void_p]
        return float(lib.orbm_create_new_map_points_last_kernel_ms(self._h))

    # ---- Frame::ComputeStereoFishEyeMatches (include/orbslam3_hip_fisheye.h) ----
    def stereo_fisheye(self, rig, kps_l, desc_l, mono_l, kps_r, desc_r, mono_r, level_sigma2):
        """orbm_stereo_fisheye on host arrays: kps = KP_DTYPE arrays (mvKeys / mvKeysRight), mono = monoLeft / monoRight, rig as
        fisheye_rig() takes it.  Returns dict(matches, left_to_right, right_to_left, depth, p3d, knn_right, knn_d0, knn_d1)."""
        kps_l = np.ascontiguousarray(kps_l, KP_DTYPE); kps_r = np.ascontiguousarray(kps_r, KP_DTYPE)
        desc_l = np.ascontiguousarray(desc_l, np.uint8); desc_r = np.ascontiguousarray(desc_r, np.uint8)
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        n_l, n_r = len(kps_l), len(kps_r)
        out = dict(left_to_right=np.full(n_l, -1, np.int32), right_to_left=np.full(n_r, -1, np.int32), depth=np.full(n_l, -1, np.float32),
                   p3d=np.zeros((n_l, 3), np.float32), knn_right=np.full(n_l, -1, np.int32), knn_d0=np.full(n_l, -1, np.int32),
                   knn_d1=np.full(n_l, -1, np.int32))
        _fisheye_argtypes()
        out["matches"] = _check(lib.orbm_stereo_fisheye(self._h, _p(kps_l), _p(desc_l), n_l, int(mono_l), _p(kps_r), _p(desc_r), n_r, int(mono_r),
                                                        _p(sig), len(sig), C.byref(fisheye_rig(rig)), _p(out["left_to_right"]), _p(out["right_to_left"]),
                                                        _p(out["depth"]), _p(out["p3d"]), _p(out["knn_right"]), _p(out["knn_d0"]), _p(out["knn_d1"])))
        return out

    def stereo_fisheye_last_kernel_ms(self):
        _fisheye_argtypes()
        return float(lib.orbm_stereo_fisheye_last_kernel_ms(self._h))

    def stereo_fisheye_device(self, rig, batch, cap, d_kps_l, d_desc_l, d_n_l, d_mono_l, d_kps_r, d_desc_r, d_n_r, d_mono_r, level_sigma2,
                              d_left_to_right, d_right_to_left, d_depth, d_p3d, d_knn_right=None, d_knn_d0=None, d_knn_d1=None, stream=None):
        """orbm_stereo_fisheye_batch_device: raw device pointers (ints, e.g. torch.Tensor.data_ptr()); asynchronous"""
        sig = np.ascontiguousarray(level_sigma2, np.float32)
        _fisheye_argtypes()
        v = lambda q: C.c_void_p(q or 0)
        _check(lib.orbm_stereo_fisheye_batch_device(self._h, int(batch), int(cap), v(d_kps_l), v(d_desc_l), v(d_n_l), v(d_mono_l), v(d_kps_r), v(d_desc_r),
                                                    v(d_n_r), v(d_mono_r), _p(sig), len(sig), C.byref(fisheye_rig(rig)), v(d_left_to_right),
                                                    v(d_right_to_left), v(d_depth), v(d_p3d), v(d_knn_right), v(d_knn_d0), v(d_knn_d1), v(stream)))


    # ---- the tracking searches of a two-camera fisheye rig frame, Nleft != -1 (include/orbslam3_hip_rig_match.h) ----
    def search_by_projection_rig(self, rig, mp, th, assign, occupied, far_points=False, th_far=0.0):
        """SearchByProjection(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints) of a rig frame.  rig: dict(left, right
        (grid dicts as _frame takes them, with "desc" and optionally "angle"), scale, left_to_right, right_to_left); mp: dict of
        the OrbmRigMapPoints arrays.  assign / occupied: in/out, left.n + right.n slots.  Returns nmatches."""
        _rig_match_argtypes()
        r, keep = rig_frame(rig)
        p = rig_map_points(mp)
        return _check(lib.orbm_search_by_projection_rig(self._h, C.byref(r), C.byref(p), th, int(far_points), th_far, self.nnratio, _p(assign), _p(occupied)))

    def search_by_projection_last_rig(self, rig, last, th, assign, occupied):
        """SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) of a rig frame; last: dict of the
        OrbmRigLastPoints arrays and "level_window".  Returns nmatches."""
        _rig_match_argtypes()
        r, keep = rig_frame(rig)
        p = rig_last_points(last)
        return _check(lib.orbm_search_by_projection_last_rig(self._h, C.byref(r), C.byref(p), th, int(last.get("level_window", 0)), int(self.check_ori),
                                                             _p(assign), _p(occupied)))

    def search_by_projection_rig_batch(self, queries, th, far_points=False, th_far=0.0):
        """queries: list of dict(rig, pts, assign, occupied) -> list of nmatches; ONE launch"""
        _rig_match_argtypes()
        arr = (OrbmRigMapQuery * len(queries))()
        keep = []
        for i, q in enumerate(queries):
            r, k = rig_frame(q["rig"]); p = rig_map_points(q["pts"])
            keep.append((r, k, p))
            arr[i] = OrbmRigMapQuery(C.pointer(r), C.pointer(p), q["assign"].ctypes.data, q["occupied"].ctypes.data, 0)
        _check(lib.orbm_search_by_projection_rig_batch(self._h, arr, len(queries), th, int(far_points), th_far, self.nnratio))
        return [int(arr[i].n_matches) for i in range(len(queries))]

    def search_by_projection_last_rig_batch(self, queries, th):
        """queries: list of dict(rig, pts (with "level_window"), assign, occupied) -> list of nmatches; ONE launch"""
        _rig_match_argtypes()
        arr = (OrbmRigLastQuery * len(queries))()
        keep = []
        for i, q in enumerate(queries):
            r, k = rig_frame(q["rig"]); p = rig_last_points(q["pts"])
            keep.append((r, k, p))
            arr[i] = OrbmRigLastQuery(C.pointer(r), C.pointer(p), int(q["pts"].get("level_window", 0)), q["assign"].ctypes.data, q["occupied"].ctypes.data, 0)
        _check(lib.orbm_search_by_projection_last_rig_batch(self._h, arr, len(queries), th, int(self.check_ori)))
        return [int(arr[i].n_matches) for i in range(len(queries))]

    def rig_search_last_kernel_ms(self):
        _rig_match_argtypes()
        return float(lib.orbm_rig_search_last_kernel_ms(self._h))

    # ---- the same two searches on device arrays (include/orbslam3_hip_rig_track_device.h) ----
    def search_by_projection_last_rig_batch_device(self, frames, last, batch, th, d_assign, d_occupied, d_n_matches, d_n_slots=None, stream=None):
        """orbm_search_by_projection_last_rig_batch_device.  frames / last: dicts keyed by the fields of OrbmDeviceRigFrames /
        OrbmDeviceRigLastPoints (device addresses as ints; scale_factors a host float array; optional fields may be absent).
        Only enqueues."""
        _rig_track_device_argtypes()
        f, keep = device_rig_frames(frames)
        p = device_rig_points(OrbmDeviceRigLastPoints, last)
        _check(lib.orbm_search_by_projection_last_rig_batch_device(self._h, C.byref(f), C.byref(p), int(batch), th, int(self.check_ori), d_assign, d_occupied,
                                                                   d_n_matches, d_n_slots, stream))

    def search_by_projection_rig_batch_device(self, frames, points, batch, th, d_assign, d_occupied, d_n_matches, d_n_slots=None, stream=None,
                                              far_points=False, th_far=0.0):
        """orbm_search_by_projection_rig_batch_device.  points: dict keyed by the array fields of OrbmDeviceRigMapPoints and cap; nnratio is
        the handle's.  Only enqueues."""
        _rig_track_device_argtypes()
        f, keep = device_rig_frames(frames)
        p = device_rig_points(OrbmDeviceRigMapPoints, dict(points, th_far=float(th_far), nnratio=self.nnratio, far_points=int(far_points)))
        _check(lib.orbm_search_by_projection_rig_batch_device(self._h, C.byref(f), C.byref(p), int(batch), th, d_assign, d_occupied, d_n_matches, d_n_slots, stream))


    # ---- SearchByBoW and SearchForTriangulation for two-camera fisheye rigs (include/orbslam3_hip_rig_bow.h) ----
    def search_by_bow_rig(self, s):
        """SearchByBoW(KeyFrame*, Frame&, ...) with F.Nleft != -1.  s: dict(dKF, validKF, angKF, fvKF, dF, n_left, angF, fvF), all over
        the concatenated (left, then right) arrays.  Returns (nmatches, match_f2kf[nF])."""
        _rig_bow_argtypes()
        p, keep = bow_rig_pair(s)
        a, b = p.fv_kf, p.fv_f
        n = _check(lib.orbm_search_by_bow_rig(self._h, p.desc_kf, p.n_kf, p.valid_kf, p.angle_kf, C.byref(a), p.desc_f, p.n_f, p.n_left_f, p.angle_f, C.byref(b),
                                              self.nnratio, int(self.check_ori), p.match_f2kf))
        return n, keep["match"][:p.n_f]

    def search_by_bow_rig_batch(self, sets):
        """sets: list of dicts as search_by_bow_rig takes -> list of (nmatches, match_f2kf); ONE launch"""
        _rig_bow_argtypes()
        arr = (OrbmBowRigPair * len(sets))()
        keep = []
        for i, s in enumerate(sets):
            arr[i], k = bow_rig_pair(s)
            keep.append(k)
        _check(lib.orbm_search_by_bow_rig_batch(self._h, arr, len(sets), self.nnratio, int(self.check_ori)))
        return [(int(arr[i].n_matches), keep[i]["match"][:arr[i].n_f]) for i in range(len(sets))]

    def search_for_triangulation_rig(self, s, only_stereo=False, coarse=False):
        """SearchForTriangulation(pKF1, pKF2, ...) of two rig key frames.  s: dict(kf1, kf2 (dicts of desc, has_mp, x, y, octave, angle, fv,
        n_left over the concatenated lists), geom=dict(cam [4][9], R12 [4][9], t12 [4][3]), sigma2_1, sigma2_2).  Returns (nmatches, match12)."""
        _rig_bow_argtypes()
        p, keep = rig_tri_pair(s)
        n = _check(lib.orbm_search_for_triangulation_rig(self._h, p.kf1, p.n_left_1, p.kf2, p.n_left_2, p.geom, p.level_sigma2_1, p.level_sigma2_2, p.n_levels,
                                                         int(only_stereo), int(coarse), int(self.check_ori), p.match12))
        return n, keep["match"][:p.kf1.contents.n]

    def search_for_triangulation_rig_batch(self, sets, only_stereo=False, coarse=False):
        """sets: list of dicts as search_for_triangulation_rig takes -> list of (nmatches, match12); ONE search launch"""
        _rig_bow_argtypes()
        arr = (OrbmRigTriPair * len(sets))()
        keep = []
        for i, s in enumerate(sets):
            arr[i], k = rig_tri_pair(s)
            keep.append(k)
        _check(lib.orbm_search_for_triangulation_rig_batch(self._h, arr, len(sets), int(only_stereo), int(coarse), int(self.check_ori)))
        return [(int(arr[i].n_matches), keep[i]["match"][:arr[i].kf1.contents.n]) for i in range(len(sets))]

    def rig_bow_last_kernel_ms(self):
        _rig_bow_argtypes()
        return float(lib.orbm_rig_bow_last_kernel_ms(self._h))


class OrbmRigFrame(C.Structure):
    """OrbmRigFrame of include/orbslam3_hip_rig_match.h"""
    _fields_ = [("left", Frame), ("right", Frame), ("left_to_right", C.c_void_p), ("right_to_left", C.c_void_p)]


class OrbmRigMapPoints(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(k, C.c_void_p) for k in (
        "in_view", "proj_u", "proj_v", "pred_level", "view_cos", "in_view_r", "proj_u_r", "proj_v_r", "pred_level_r", "view_cos_r",
        "track_depth", "bad", "has_obs", "desc")]


class OrbmRigLastPoints(C.Structure):
    _fields_ = [("n", C.c_int32)] + [(k, C.c_void_p) for k in ("valid", "proj_u", "proj_v", "proj_u_r", "proj_v_r", "octave", "angle", "has_obs", "desc")]


class OrbmRigMapQuery(C.Structure):
    _fields_ = [("rig", C.POINTER(OrbmRigFrame)), ("pts", C.POINTER(OrbmRigMapPoints)), ("assign", C.c_void_p), ("occupied", C.c_void_p), ("n_matches", C.c_int32)]


class OrbmRigLastQuery(C.Structure):
    _fields_ = [("rig", C.POINTER(OrbmRigFrame)), ("pts", C.POINTER(OrbmRigLastPoints)), ("level_window", C.c_int32), ("assign", C.c_void_p),
                ("occupied", C.c_void_p), ("n_matches", C.c_int32)]


def _rig_match_argtypes():
    lib.orbm_rig_search_check.argtypes = [C.POINTER(OrbmRigFrame), C.POINTER(OrbmRigMapPoints), C.POINTER(OrbmRigLastPoints), C.c_void_p, C.c_void_p]
    lib.orbm_search_by_projection_rig.argtypes = [C.c_void_p, C.POINTER(OrbmRigFrame), C.POINTER(OrbmRigMapPoints), C.c_float, C.c_int, C.c_float, C.c_float,
                                                  C.c_void_p, C.c_void_p]
    lib.orbm_search_by_projection_last_rig.argtypes = [C.c_void_p, C.POINTER(OrbmRigFrame), C.POINTER(OrbmRigLastPoints), C.c_float, C.c_int, C.c_int,
                                                       C.c_void_p, C.c_void_p]
    lib.orbm_search_by_projection_rig_batch.argtypes = [C.c_void_p, C.POINTER(OrbmRigMapQuery), C.c_int, C.c_float, C.c_int, C.c_float, C.c_float]
    lib.orbm_search_by_projection_last_rig_batch.argtypes = [C.c_void_p, C.POINTER(OrbmRigLastQuery), C.c_int, C.c_float, C.c_int]
    lib.orbm_rig_search_last_kernel_ms.restype = C.c_float
    lib.orbm_rig_search_last_kernel_ms.argtypes = [C.c_void_p]


def _ptr(a):
    return None if a is None else a.ctypes.data


def rig_frame(rig):
    """dict(left, right, scale, left_to_right, right_to_left) -> (OrbmRigFrame, the arrays it points to).  A side is a grid dict
    (x, y, octave, min_x .. max_y, cols, rows) with "desc" and optionally "angle"; a side may carry its own "scale"."""
    sides = []
    for s in ("left", "right"):
        g = rig[s]
        sc = g.get("scale", rig.get("scale"))
        n = int(g["n"]) if "n" in g else next((len(g[k]) for k in ("x", "y", "octave", "desc") if g.get(k) is not None), 0)
        sides.append(Frame(n, _ptr(g["x"]), _ptr(g["y"]), _ptr(g["octave"]), _ptr(g.get("angle")), _ptr(g["desc"]),
                           g["min_x"], g["min_y"], g["max_x"], g["max_y"], g.get("cols", 64), g.get("rows", 48), _ptr(sc), g.get("n_levels", 0 if sc is None else len(sc)),
                           _ptr(g.get("u_right"))))
    return OrbmRigFrame(sides[0], sides[1], _ptr(rig["left_to_right"]), _ptr(rig["right_to_left"])), rig


def rig_map_points(mp):
    return OrbmRigMapPoints(int(mp.get("n", len(mp["proj_u"]) if mp.get("proj_u") is not None else 0)),
                            *[_ptr(mp.get(k)) for k, _ in OrbmRigMapPoints._fields_[1:]])


def rig_last_points(last):
    return OrbmRigLastPoints(int(last.get("n", len(last["proj_u"]) if last.get("proj_u") is not None else 0)),
                             *[_ptr(last.get(k)) for k, _ in OrbmRigLastPoints._fields_[1:]])


def rig_search_check(rig, mp=None, last=None, assign=None, occupied=None):
    """orbm_rig_search_check with the arguments as given (dicts, ctypes structs or None): the code"""
    _rig_match_argtypes()
    r = None if rig is None else C.byref(rig if isinstance(rig, OrbmRigFrame) else rig_frame(rig)[0])
    a = None if mp is None else C.byref(rig_map_points(mp))
    b = None if last is None else C.byref(rig_last_points(last))
    return int(lib.orbm_rig_search_check(r, a, b, _p(assign), _p(occupied)))


# ---- include/orbslam3_hip_rig_track_device.h: the rig searches and the rig PoseOptimization on device arrays ----
class OrbmDeviceRigFrames(C.Structure):
    _fields_ = [("d_kps_l", C.c_void_p), ("d_desc_l", C.c_void_p), ("d_n_l", C.c_void_p), ("cap_l", C.c_int32),
                ("d_kps_r", C.c_void_p), ("d_desc_r", C.c_void_p), ("d_n_r", C.c_void_p), ("cap_r", C.c_int32),
                ("d_left_to_right", C.c_void_p), ("d_right_to_left", C.c_void_p),
                ("min_x", C.c_float), ("min_y", C.c_float), ("max_x", C.c_float), ("max_y", C.c_float), ("grid_cols", C.c_int32), ("grid_rows", C.c_int32),
                ("scale_factors", C.c_void_p), ("n_levels", C.c_int32), ("slot_cap", C.c_int32)]


class OrbmDeviceRigLastPoints(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("d_valid", "d_u", "d_v", "d_u_r", "d_v_r", "d_octave", "d_angle", "d_has_obs", "d_desc", "d_n")] + \
               [("cap", C.c_int32), ("d_level_window", C.c_void_p)]


class OrbmDeviceRigMapPoints(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("d_in_view", "d_u", "d_v", "d_pred_level", "d_view_cos", "d_in_view_r", "d_u_r", "d_v_r", "d_pred_level_r",
                                         "d_view_cos_r", "d_track_depth", "d_bad", "d_has_obs", "d_desc", "d_n")] + \
               [("cap", C.c_int32), ("th_far", C.c_float), ("nnratio", C.c_float), ("far_points", C.c_int32)]


class PoseDeviceRigFrames(C.Structure):
    _fields_ = [("d_kps_l", C.c_void_p), ("d_n_l", C.c_void_p), ("cap_l", C.c_int32), ("d_kps_r", C.c_void_p), ("d_n_r", C.c_void_p), ("cap_r", C.c_int32),
                ("d_assign", C.c_void_p), ("slot_cap", C.c_int32), ("d_mp_xyz", C.c_void_p), ("mp_cap", C.c_int32), ("d_pose", C.c_void_p),
                ("inv_level_sigma2", C.c_void_p), ("n_levels", C.c_int32), ("huber_mono", C.c_double)]


def _rig_track_device_argtypes():
    P, I = C.c_void_p, C.c_int
    lib.orbm_rig_search_device_check.argtypes = [P, P, P, I]
    lib.orbm_search_by_projection_last_rig_batch_device.argtypes = [P, P, P, I, C.c_float, I, P, P, P, P, P]
    lib.orbm_search_by_projection_rig_batch_device.argtypes = [P, P, P, I, C.c_float, P, P, P, P, P]
    lib.pose_optimize_rig_batch_device.argtypes = [P, P, I, P, P, P, P, P]


def device_rig_frames(fr):
    """dict keyed by the fields of OrbmDeviceRigFrames -> (the struct, the host scale array it points to).  scale_factors is a host
    float array (n_levels defaults to its length), grid_cols / grid_rows default to 64 x 48, slot_cap to cap_l + cap_r."""
    sf = None if fr.get("scale_factors") is None else np.ascontiguousarray(fr["scale_factors"], np.float32)
    v = dict(fr, scale_factors=_ptr(sf))
    v.setdefault("n_levels", 0 if sf is None else len(sf))
    v.setdefault("grid_cols", 64); v.setdefault("grid_rows", 48)
    v.setdefault("slot_cap", int(fr.get("cap_l", 0)) + int(fr.get("cap_r", 0)))
    return OrbmDeviceRigFrames(*[v.get(k, 0 if t is not C.c_void_p else None) for k, t in OrbmDeviceRigFrames._fields_]), sf


def device_rig_points(cls, pts):
    """dict keyed by the fields of OrbmDeviceRigLastPoints / OrbmDeviceRigMapPoints -> the struct; an absent address is NULL"""
    return cls(*[pts.get(k, 0 if t is not C.c_void_p else None) for k, t in cls._fields_])


def rig_search_device_check(frames, last=None, mp=None, batch=1):
    """orbm_rig_search_device_check with the arguments as given (dicts or None): the code"""
    _rig_track_device_argtypes()
    f = None if frames is None else C.byref(device_rig_frames(frames)[0])
    a = None if last is None else C.byref(device_rig_points(OrbmDeviceRigLastPoints, last))
    b = None if mp is None else C.byref(device_rig_points(OrbmDeviceRigMapPoints, mp))
    return int(lib.orbm_rig_search_device_check(f, a, b, int(batch)))


class OrbmBowRigPair(C.Structure):
    """OrbmBowRigPair of include/orbslam3_hip_rig_bow.h"""
    _fields_ = [("desc_kf", C.c_void_p), ("n_kf", C.c_int32), ("valid_kf", C.c_void_p), ("angle_kf", C.c_void_p), ("fv_kf", FeatVec),
                ("desc_f", C.c_void_p), ("n_f", C.c_int32), ("n_left_f", C.c_int32), ("angle_f", C.c_void_p), ("fv_f", FeatVec),
                ("match_f2kf", C.c_void_p), ("n_matches", C.c_int32)]


class OrbmRigTriGeometry(C.Structure):
    _fields_ = [("cam", (C.c_float * 9) * 4), ("R12", (C.c_float * 9) * 4), ("t12", (C.c_float * 3) * 4)]


class OrbmRigTriPair(C.Structure):
    _fields_ = [("kf1", C.POINTER(Matcher._TriSide)), ("n_left_1", C.c_int32), ("kf2", C.POINTER(Matcher._TriSide)), ("n_left_2", C.c_int32),
                ("geom", C.POINTER(OrbmRigTriGeometry)), ("level_sigma2_1", C.c_void_p), ("level_sigma2_2", C.c_void_p), ("n_levels", C.c_int32),
                ("match12", C.c_void_p), ("n_matches", C.c_int32)]


def _rig_bow_argtypes():
    lib.orbm_rig_bow_check.argtypes = [C.POINTER(OrbmBowRigPair), C.POINTER(OrbmRigTriPair), C.c_int]
    lib.orbm_search_by_bow_rig.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.POINTER(FeatVec),
                                           C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.POINTER(FeatVec), C.c_float, C.c_int, C.c_void_p]
    lib.orbm_search_by_bow_rig_batch.argtypes = [C.c_void_p, C.POINTER(OrbmBowRigPair), C.c_int, C.c_float, C.c_int]
    lib.orbm_search_for_triangulation_rig.argtypes = [C.c_void_p, C.POINTER(Matcher._TriSide), C.c_int, C.POINTER(Matcher._TriSide), C.c_int,
                                                      C.POINTER(OrbmRigTriGeometry), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p]
    lib.orbm_search_for_triangulation_rig_batch.argtypes = [C.c_void_p, C.POINTER(OrbmRigTriPair), C.c_int, C.c_int, C.c_int, C.c_int]
    lib.orbm_rig_bow_last_kernel_ms.restype = C.c_float
    lib.orbm_rig_bow_last_kernel_ms.argtypes = [C.c_void_p]


def _fv_opt(fv):
    """_fv for a (node ids, offsets, features) triple whose arrays may be None; a 4-tuple gives n_nodes itself"""
    if fv is None:
        return FeatVec(0, None, None, None), ()
    arrs = [None if a is None else np.ascontiguousarray(a) for a in fv[:3]]
    n = int(fv[3]) if len(fv) > 3 else (0 if arrs[0] is None else len(arrs[0]))
    return FeatVec(n, _ptr(arrs[0]), _ptr(arrs[1]), _ptr(arrs[2])), arrs


def _len(a):
    return 0 if a is None else len(a)


def bow_rig_pair(s):
    """dict(dKF, validKF, angKF, fvKF, dF, n_left, angF, fvF [, n_kf, n_f, match]) -> (OrbmBowRigPair, what it points to).  Arrays may be
    None and the counts may be given, for the argument checks."""
    dKF = None if s.get("dKF") is None else np.ascontiguousarray(s["dKF"])
    dF = None if s.get("dF") is None else np.ascontiguousarray(s["dF"])
    n_kf, n_f = int(s.get("n_kf", _len(dKF))), int(s.get("n_f", _len(dF)))
    a, ka = _fv_opt(s.get("fvKF"))
    b, kb = _fv_opt(s.get("fvF"))
    match = s["match"] if "match" in s else np.full(max(n_f, 1), -1, np.int32)
    keep = dict(arrays=(dKF, dF, ka, kb, s), match=match)
    return OrbmBowRigPair(_ptr(dKF), n_kf, _ptr(s.get("validKF")), _ptr(s.get("angKF")), a, _ptr(dF), n_f, int(s.get("n_left", n_f)), _ptr(s.get("angF")), b,
                          _ptr(match), 0), keep


def _rig_tri_side(k):
    fv, kf = _fv_opt(k.get("fv"))
    n = int(k["n"]) if "n" in k else next((len(k[q]) for q in ("x", "y", "octave", "desc") if k.get(q) is not None), 0)
    return Matcher._TriSide(n, _ptr(k.get("desc")), _ptr(k.get("has_mp")), _ptr(k.get("stereo")), _ptr(k.get("x")), _ptr(k.get("y")), _ptr(k.get("octave")),
                            _ptr(k.get("angle")), fv), kf


def rig_tri_geometry(g):
    geo = OrbmRigTriGeometry()
    for name, w in (("cam", 9), ("R12", 9), ("t12", 3)):
        a = np.ascontiguousarray(g[name], np.float32).reshape(4, w)
        for c in range(4):
            for i in range(w):
                getattr(geo, name)[c][i] = float(a[c, i])
    return geo


def rig_tri_pair(s):
    """dict(kf1, kf2, geom, sigma2_1, sigma2_2 [, n_levels, match]) -> (OrbmRigTriPair, what it points to); kf1 / kf2 / geom / the sigmas
    may be None, for the argument checks"""
    sides, keep = [], dict(arrays=[s])
    for q in ("kf1", "kf2"):
        if s.get(q) is None:
            sides.append((None, 0))
        else:
            t, kf = _rig_tri_side(s[q])
            keep["arrays"] += [t, kf]
            sides.append((C.pointer(t), int(s[q].get("n_left", t.n))))
    geo = None if s.get("geom") is None else rig_tri_geometry(s["geom"])
    n1 = sides[0][0].contents.n if sides[0][0] else 0
    match = s["match"] if "match" in s else np.full(max(n1, 1), -1, np.int32)
    keep["match"] = match
    keep["arrays"].append(geo)
    n_levels = int(s.get("n_levels", _len(s.get("sigma2_1"))))
    return OrbmRigTriPair(sides[0][0], sides[0][1], sides[1][0], sides[1][1], None if geo is None else C.pointer(geo), _ptr(s.get("sigma2_1")), _ptr(s.get("sigma2_2")),
                          n_levels, _ptr(match), 0), keep


def rig_bow_check(bow=None, tri=None, check_orientation=0):
    """orbm_rig_bow_check with the arguments as given (dicts or None): the code"""
    _rig_bow_argtypes()
    a = None if bow is None else bow_rig_pair(bow)
    b = None if tri is None else rig_tri_pair(tri)
    return int(lib.orbm_rig_bow_check(None if a is None else C.byref(a[0]), None if b is None else C.byref(b[0]), int(check_orientation)))


ORBM_MAX_NEIGHBOURS = 64


class OrbmMapKeyFrame(C.Structure):
    _fields_ = [("side", Matcher._TriSide), ("u_right", C.c_void_p), ("depth", C.c_void_p), ("key_x", C.c_void_p), ("key_y", C.c_void_p),
                ("Rcw", C.c_float * 9), ("tcw", C.c_float * 3), ("Ow", C.c_float * 3),
                ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("invfx", C.c_float), ("invfy", C.c_float),
                ("mb", C.c_float), ("mbf", C.c_float),
                ("level_sigma2", C.c_void_p), ("scale_factors", C.c_void_p), ("n_levels", C.c_int32)]


class OrbmMapPair(C.Structure):
    _fields_ = [("ep_x", C.c_float), ("ep_y", C.c_float), ("F12", C.c_float * 9), ("coarse", C.c_int32)]


class OrbmMapParams(C.Structure):
    _fields_ = [("inertial", C.c_int32), ("far_points", C.c_int32), ("th_far", C.c_float), ("scale_factor_1", C.c_float)]


class OrbmNewPoints(C.Structure):
    _fields_ = [("neighbour", C.c_void_p), ("idx2", C.c_void_p), ("x3d", C.c_void_p), ("point_stereo", C.c_void_p),
                ("normal", C.c_void_p), ("max_dist", C.c_void_p), ("min_dist", C.c_void_p), ("n_matched", C.c_void_p), ("n_created", C.c_void_p),
                ("match12", C.c_void_p)]


def _fill_map_key_frame(s, k, keep, name):
    """one OrbmMapKeyFrame from a dict; the C side copies n rows of every per-feature array, so unequal lengths are refused here"""
    a = dict(desc=np.ascontiguousarray(k["desc"], np.uint8), has_mp=np.ascontiguousarray(k["has_mp"], np.uint8),
             stereo=np.ascontiguousarray(k["stereo"], np.uint8), x=np.ascontiguousarray(k["x"], np.float32),
             y=np.ascontiguousarray(k["y"], np.float32), octave=np.ascontiguousarray(k["octave"], np.int32),
             u_right=np.ascontiguousarray(k["u_right"], np.float32), depth=np.ascontiguousarray(k["depth"], np.float32))
    for f in ("key_x", "key_y"):
        if k.get(f) is not None:
            a[f] = np.ascontiguousarray(k[f], np.float32)
    n = len(a["x"])
    for f, v in a.items():
        if v.shape != ((n, 32) if f == "desc" else (n,)):
            raise ValueError("%s: %s does not hold %d features" % (name, f, n))
    sig, sc = np.ascontiguousarray(k["level_sigma2"], np.float32), np.ascontiguousarray(k["scale_factors"], np.float32)
    if sig.shape != sc.shape or sig.ndim != 1:
        raise ValueError("%s: level_sigma2 and scale_factors differ in length" % name)
    fv = _fv(k["fv"])
    keep.append((a, sig, sc, fv))
    s.side = Matcher._TriSide(n, a["desc"].ctypes.data, a["has_mp"].ctypes.data, a["stereo"].ctypes.data, a["x"].ctypes.data,
                              a["y"].ctypes.data, a["octave"].ctypes.data, None, fv)
    s.u_right, s.depth = a["u_right"].ctypes.data, a["depth"].ctypes.data
    s.key_x = a["key_x"].ctypes.data if "key_x" in a else None
    s.key_y = a["key_y"].ctypes.data if "key_y" in a else None
    for f, m in (("Rcw", 9), ("tcw", 3), ("Ow", 3)):
        v = np.asarray(k[f], np.float32).reshape(-1)
        if v.shape != (m,):
            raise ValueError("%s: %s does not hold %d values" % (name, f, m))
        getattr(s, f)[:] = [float(t) for t in v]
    for f in ("fx", "fy", "cx", "cy", "invfx", "invfy", "mb", "mbf"):
        setattr(s, f, float(k[f]))
    s.level_sigma2, s.scale_factors, s.n_levels = sig.ctypes.data, sc.ctypes.data, len(sc)


class OrbmRigMapKeyFrame(C.Structure):
    """OrbmRigMapKeyFrame of include/orbslam3_hip_rig_newpoints.h"""
    _fields_ = [("side", Matcher._TriSide), ("n_left", C.c_int32), ("Rcw", (C.c_float * 9) * 2), ("tcw", (C.c_float * 3) * 2),
                ("Ow", (C.c_float * 3) * 2), ("cam", (C.c_float * 9) * 2), ("mb", C.c_float),
                ("level_sigma2", C.c_void_p), ("scale_factors", C.c_void_p), ("n_levels", C.c_int32)]


class OrbmRigMapPair(C.Structure):
    _fields_ = [("geom", C.POINTER(OrbmRigTriGeometry)), ("coarse", C.c_int32)]


def _rig_newpoints_argtypes():
    lib.orbm_create_new_map_points_rig_check.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orbm_create_new_map_points_rig.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.orbm_create_new_map_points_rig_last_kernel_ms.restype = C.c_float
    lib.orbm_create_new_map_points_rig_last_kernel_ms.argtypes = [C.c_void_p]
    lib.orbm_create_new_map_points_rig_last_launches.argtypes = [C.c_void_p]


def _fill_rig_map_key_frame(s, k, keep):
    """one OrbmRigMapKeyFrame from dict(desc, has_mp, x, y, octave, fv, n_left, Rcw [2][9], tcw [2][3], Ow [2][3], cam [2][9], mb,
    level_sigma2, scale_factors [, n, n_levels]); arrays may be None and the counts may be given, for the argument checks"""
    typed = dict(desc=np.uint8, has_mp=np.uint8, x=np.float32, y=np.float32, octave=np.int32)
    a = {f: None if k.get(f) is None else np.ascontiguousarray(k[f], t) for f, t in typed.items()}
    n = int(k["n"]) if "n" in k else next((len(a[f]) for f in ("x", "y", "octave", "desc") if a[f] is not None), 0)
    if "n" not in k:
        for f, v in a.items():
            if v is not None and len(v) != n:
                raise ValueError("%s does not hold %d features" % (f, n))
    sig = None if k.get("level_sigma2") is None else np.ascontiguousarray(k["level_sigma2"], np.float32)
    sc = None if k.get("scale_factors") is None else np.ascontiguousarray(k["scale_factors"], np.float32)
    fv, kfv = _fv_opt(k.get("fv"))
    keep.append((a, sig, sc, kfv))
    s.side = Matcher._TriSide(n, _ptr(a["desc"]), _ptr(a["has_mp"]), None, _ptr(a["x"]), _ptr(a["y"]), _ptr(a["octave"]), None, fv)
    s.n_left = int(k.get("n_left", n))
    for f, w in (("Rcw", 9), ("tcw", 3), ("Ow", 3), ("cam", 9)):
        v = np.asarray(k[f], np.float32).reshape(2, w)
        for c in range(2):
            getattr(s, f)[c][:] = [float(t) for t in v[c]]
    s.mb = float(k["mb"])
    s.level_sigma2, s.scale_factors, s.n_levels = _ptr(sig), _ptr(sc), int(k.get("n_levels", _len(sc)))


def rig_new_points_args(kf1, neighbours, pairs, params, n_neighbours=None, null=()):
    """the arguments of orbm_create_new_map_points_rig flattened once (no device needed).  kf1 / neighbours[j]: dicts as
    _fill_rig_map_key_frame takes (kf1 may be None); pairs[j]: dict(geom, coarse) (geom may be None); params: dict(inertial,
    far_points, th_far, scale_factor_1).  n_neighbours overrides the count, `null` names output arrays to pass as NULL."""
    if len(pairs) != len(neighbours):
        raise ValueError("%d pairs for %d neighbours" % (len(pairs), len(neighbours)))
    keep = []
    kfs = (OrbmRigMapKeyFrame * (1 + max(len(neighbours), 1)))()
    for q, k in enumerate([kf1] + list(neighbours)):
        if k is not None:
            _fill_rig_map_key_frame(kfs[q], k, keep)
    prs = (OrbmRigMapPair * max(len(pairs), 1))()
    for j, w in enumerate(pairs):
        if w.get("geom") is not None:
            g = rig_tri_geometry(w["geom"])
            keep.append(g)
            prs[j].geom = C.pointer(g)
        prs[j].coarse = int(bool(w.get("coarse", False)))
    par = OrbmMapParams(int(bool(params["inertial"])), int(bool(params["far_points"])), float(params["th_far"]), float(params["scale_factor_1"]))
    n1 = kfs[0].side.n if kf1 is not None else 0
    nb = len(neighbours) if n_neighbours is None else int(n_neighbours)
    m1, mb = max(n1, 1), max(len(neighbours), 1)
    o = dict(neighbour=np.full(m1, -1, np.int32), idx2=np.full(m1, -1, np.int32), x3d=np.zeros((m1, 3), np.float32),
             point_stereo=np.zeros(m1, np.uint8), normal=np.zeros((m1, 3), np.float32), max_dist=np.zeros(m1, np.float32),
             min_dist=np.zeros(m1, np.float32), n_matched=np.zeros(mb, np.int32), n_created=np.zeros(mb, np.int32),
             match12=np.full((mb, m1), -1, np.int32))
    out = OrbmNewPoints(*[None if f in null else o[f].ctypes.data for f, _ in OrbmNewPoints._fields_])
    skipped = np.zeros(mb, np.uint8)
    return dict(kfs=kfs, pairs=prs, params=par, out=out, arrays=o, skipped=skipped, n1=n1, n_neighbours=nb, keep=keep, has_kf1=kf1 is not None)


def create_new_map_points_rig_check(kf1, neighbours, pairs, params, n_neighbours=None, null=(), null_args=()):
    """orbm_create_new_map_points_rig_check with the arguments as given: the code.  null_args names whole arguments to pass as
    NULL: "neighbours", "pairs", "params", "out"."""
    _rig_newpoints_argtypes()
    p = rig_new_points_args(kf1, neighbours, pairs, params, n_neighbours, null)
    nbs = None if "neighbours" in null_args else C.byref(p["kfs"], C.sizeof(OrbmRigMapKeyFrame))
    return int(lib.orbm_create_new_map_points_rig_check(C.byref(p["kfs"]) if p["has_kf1"] else None, nbs, p["n_neighbours"],
                                                        None if "pairs" in null_args else C.byref(p["pairs"]),
                                                        None if "params" in null_args else C.byref(p["params"]),
                                                        None if "out" in null_args else C.byref(p["out"])))


def create_new_map_points_rig_launch(handle, prep):
    """the C call alone on a matcher handle (None: no handle)"""
    _rig_newpoints_argtypes()
    nbs = C.byref(prep["kfs"], C.sizeof(OrbmRigMapKeyFrame))
    return _check(lib.orbm_create_new_map_points_rig(handle, C.byref(prep["kfs"]), nbs, prep["n_neighbours"], C.byref(prep["pairs"]),
                                                     C.byref(prep["params"]), C.byref(prep["out"]), prep["skipped"].ctypes.data))


def rig_new_points_result(prep, created):
    a, n1, nb = prep["arrays"], prep["n1"], prep["n_neighbours"]
    r = {k: (a[k][:nb] if k in ("n_matched", "n_created") else a[k][:nb, :n1] if k == "match12" else a[k][:n1]).copy() for k in a}
    r["created"] = created
    r["skipped"] = prep["skipped"][:nb].copy()
    return r


def _matcher_create_new_map_points_rig(self, kf1, neighbours, pairs, params):
    """LocalMapping::CreateNewMapPoints for rig key frames: dict(created, neighbour, idx2, x3d, point_stereo, normal, max_dist,
    min_dist [n1], n_matched, n_created, skipped [n_neighbours], match12 [n_neighbours][n1]); (neighbour, idx1) ascending over
    neighbour >= 0 is the reference's creation order"""
    prep = rig_new_points_args(kf1, neighbours, pairs, params)
    return rig_new_points_result(prep, create_new_map_points_rig_launch(self._h, prep))


def _matcher_rig_new_points_last(self):
    """(device milliseconds, launches) of the last create_new_map_points_rig on this handle"""
    _rig_newpoints_argtypes()
    return float(lib.orbm_create_new_map_points_rig_last_kernel_ms(self._h)), int(lib.orbm_create_new_map_points_rig_last_launches(self._h))


Matcher.create_new_map_points_rig_prepare = staticmethod(rig_new_points_args)
Matcher.create_new_map_points_rig_launch = lambda self, prep: create_new_map_points_rig_launch(self._h, prep)
Matcher.create_new_map_points_rig = _matcher_create_new_map_points_rig
Matcher.create_new_map_points_rig_last = _matcher_rig_new_points_last


class _BowSideDevice(C.Structure):
    _fields_ = [("desc", C.c_void_p), ("kps", C.c_void_p), ("n", C.c_void_p), ("cap", C.c_int32), ("valid", C.c_void_p),
                ("fv_node", C.c_void_p), ("fv_off", C.c_void_p), ("fv_feat", C.c_void_p), ("n_fv_nodes", C.c_void_p)]


class _BowPairDevice(C.Structure):
    _fields_ = [("kf", _BowSideDevice), ("f", _BowSideDevice), ("match_f2kf", C.c_void_p), ("n_matches", C.c_void_p)]


class DeviceBowPlan:
    """SearchByBoW on device-resident pairs: sides = dicts of device addresses (desc, kps, n, cap, fv_node, fv_off, fv_feat,
    n_fv_nodes[, valid]) as produced by Extractor.extract_batch_device + Vocabulary.transform_batch_device."""

    def __init__(self, matcher, pairs):
        n = len(pairs)
        arr = (_BowPairDevice * n)()
        for i, (kf, f, match_ptr, nm_ptr) in enumerate(pairs):
            for side, d in ((arr[i].kf, kf), (arr[i].f, f)):
                side.desc, side.kps, side.n, side.cap = d["desc"], d["kps"], d["n"], int(d["cap"])
                side.valid = d.get("valid") or None
                side.fv_node, side.fv_off, side.fv_feat, side.n_fv_nodes = d["fv_node"], d["fv_off"], d["fv_feat"], d["n_fv_nodes"]
            arr[i].match_f2kf = match_ptr; arr[i].n_matches = nm_ptr
        h = C.c_void_p()
        _check(lib.orbm_bow_plan_create_device(matcher._h, arr, n, C.byref(h)))
        self._h, self._m = h, matcher

    def run(self, stream=None):
        _check(lib.orbm_bow_plan_run(self._h, C.c_float(self._m.nnratio), int(self._m.check_ori), C.c_void_p(stream or 0)))

    def close(self):
        if getattr(self, "_h", None):
            lib.orbm_bow_plan_destroy.argtypes = [C.c_void_p]
            lib.orbm_bow_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class BowPlan:
    def __init__(self, matcher, sets):
        lib.orbm_bow_plan_create.argtypes = [C.c_void_p, C.POINTER(BowPair), C.c_int, C.POINTER(C.c_void_p)]
        lib.orbm_bow_plan_run.argtypes = [C.c_void_p, C.c_float, C.c_int, C.c_void_p]
        lib.orbm_bow_plan_fetch.argtypes = [C.c_void_p, C.POINTER(BowPair), C.c_void_p]
        lib.orbm_bow_plan_destroy.argtypes = [C.c_void_p]
        self.m = matcher
        P = self.P = len(sets)
        self.arr = (BowPair * P)()
        self.keep, self.outs = [], []
        for i, s in enumerate(sets):
            dKF, dF = np.ascontiguousarray(s["dKF"]), np.ascontiguousarray(s["dF"])
            a, b = _fv(s["fvKF"]), _fv(s["fvF"])
            m = np.full(len(dF), -1, np.int32)
            self.keep.append((dKF, dF, a, b, s["validKF"], s["angKF"], s["angF"]))
            self.outs.append(m)
            self.arr[i] = BowPair(dKF.ctypes.data, len(dKF), s["validKF"].ctypes.data, s["angKF"].ctypes.data, a,
                                  dF.ctypes.data, len(dF), s["angF"].ctypes.data, b, m.ctypes.data, 0)
        h = C.c_void_p()
        _check(lib.orbm_bow_plan_create(matcher._h, self.arr, P, C.byref(h)))
        self._h = h

    def run(self, stream=None):
        _check(lib.orbm_bow_plan_run(self._h, self.m.nnratio, int(self.m.check_ori), stream))

    def fetch(self, stream=None):
        _check(lib.orbm_bow_plan_fetch(self._h, self.arr, stream))
        return [(self.arr[i].n_matches, self.outs[i]) for i in range(self.P)]

    def close(self):
        if getattr(self, "_h", None):
            lib.orbm_bow_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class OrbxKB8(C.Structure):
    """OrbxKB8 of include/orbslam3_hip_kb8.h: KannalaBrandt8::mvParameters[0..7], floats promoted to double"""
    _fields_ = [("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("k", C.c_double * 4)]


def _kb8(cam):
    """dict(fx, fy, cx, cy, k=[k0..k3]) -> OrbxKB8"""
    c = OrbxKB8(float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]))
    c.k[:] = [float(v) for v in cam["k"]]
    return c


def _set_camera_kb8(fn, handle, cam):
    fn.argtypes = [C.c_void_p, C.POINTER(OrbxKB8)]
    _check(fn(handle, C.byref(_kb8(cam)) if cam is not None else None))


class OrbxKB8Rig(C.Structure):
    """OrbxKB8Rig of include/orbslam3_hip_kb8.h: mpCamera, mpCamera2 and GetRelativePoseTrl() as a g2o::SE3Quat (q xyzw, t)"""
    _fields_ = [("left", OrbxKB8), ("right", OrbxKB8), ("q_rl", C.c_double * 4), ("t_rl", C.c_double * 3)]


EDGE_RIGHT = 2      # ORBX_EDGE_RIGHT: the stereo byte of a right-camera edge while a rig is set


def _kb8_rig(rig):
    """dict(left, right (as _kb8 takes them), q_rl (xyzw), t_rl) -> OrbxKB8Rig"""
    r = OrbxKB8Rig(_kb8(rig["left"]), _kb8(rig["right"]))
    r.q_rl[:] = [float(v) for v in rig["q_rl"]]
    r.t_rl[:] = [float(v) for v in rig["t_rl"]]
    return r


def _set_rig_kb8(fn, handle, rig):
    fn.argtypes = [C.c_void_p, C.POINTER(OrbxKB8Rig)]
    _check(fn(handle, C.byref(_kb8_rig(rig)) if rig is not None else None))


def kb8_project(cam, Xc, want_jac=True, device=0):
    """orbx_kb8_project: KannalaBrandt8::project (and projectJac, 2 x 3 row-major) of camera-frame points on the device"""
    lib.orbx_kb8_project.argtypes = [C.c_int, C.POINTER(OrbxKB8), C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    X = np.ascontiguousarray(Xc, np.float64).reshape(-1, 3)
    uv = np.zeros((len(X), 2))
    jac = np.zeros((len(X), 6)) if want_jac else None
    _check(lib.orbx_kb8_project(device, C.byref(_kb8(cam)), _p(X), len(X), _p(uv), _p(jac)))
    return (uv, jac.reshape(-1, 2, 3)) if want_jac else uv


class OrbxFisheyeRig(C.Structure):
    """OrbxFisheyeRig of include/orbslam3_hip_fisheye.h: mpCamera, mpCamera2, their precision, mRlr (row major), mtlr"""
    _fields_ = [("left", OrbxKB8), ("right", OrbxKB8), ("precision_l", C.c_float), ("precision_r", C.c_float), ("Rlr", C.c_float * 9), ("tlr", C.c_float * 3)]


ORBM_FISHEYE_KNN_CHUNK = 128        # right key points the k-NN kernel stages per pass (include/orbslam3_hip_fisheye.h)


def fisheye_rig(rig):
    """dict(left, right (as _kb8 takes them), precision_l, precision_r, Rlr (3, 3), tlr (3,)) -> OrbxFisheyeRig"""
    if isinstance(rig, OrbxFisheyeRig):
        return rig
    r = OrbxFisheyeRig(_kb8(rig["left"]), _kb8(rig["right"]), float(rig.get("precision_l", 1e-6)), float(rig.get("precision_r", 1e-6)))
    r.Rlr[:] = [float(v) for v in np.asarray(rig["Rlr"], np.float32).reshape(9)]
    r.tlr[:] = [float(v) for v in np.asarray(rig["tlr"], np.float32).reshape(3)]
    return r


def _fisheye_argtypes():
    side = [C.c_void_p, C.c_void_p, C.c_int, C.c_int]
    lib.orbm_stereo_fisheye_check.argtypes = side + side + [C.c_void_p, C.c_int, C.POINTER(OrbxFisheyeRig)]
    lib.orbm_stereo_fisheye.argtypes = [C.c_void_p] + side + side + [C.c_void_p, C.c_int, C.POINTER(OrbxFisheyeRig)] + [C.c_void_p] * 7
    lib.orbm_stereo_fisheye_last_kernel_ms.restype = C.c_float
    lib.orbm_stereo_fisheye_last_kernel_ms.argtypes = [C.c_void_p]
    lib.orbm_stereo_fisheye_batch_device.argtypes = [C.c_void_p, C.c_int, C.c_int] + [C.c_void_p] * 9 + [C.c_int, C.POINTER(OrbxFisheyeRig)] + [C.c_void_p] * 8
    lib.orbx_kb8_triangulate_matches.argtypes = [C.c_int, C.POINTER(OrbxFisheyeRig)] + [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p]


def stereo_fisheye_check(rig, kps_l, desc_l, n_l, mono_l, kps_r, desc_r, n_r, mono_r, level_sigma2, n_levels):
    """orbm_stereo_fisheye_check with the arguments as given (arrays or None; rig a dict, an OrbxFisheyeRig or None): the code"""
    _fisheye_argtypes()
    return int(lib.orbm_stereo_fisheye_check(_p(kps_l), _p(desc_l), int(n_l), int(mono_l), _p(kps_r), _p(desc_r), int(n_r), int(mono_r), _p(level_sigma2),
                                             int(n_levels), None if rig is None else C.byref(fisheye_rig(rig))))


def kb8_triangulate_matches(rig, pts_l, pts_r, sigma_l, sigma_r, device=0):
    """orbx_kb8_triangulate_matches: KannalaBrandt8::TriangulateMatches of n pixel pairs on the device -> (code or depth [n], p3d [n, 3])"""
    pl = np.ascontiguousarray(pts_l, np.float32).reshape(-1, 2); pr = np.ascontiguousarray(pts_r, np.float32).reshape(-1, 2)
    sl = np.ascontiguousarray(sigma_l, np.float32); sr = np.ascontiguousarray(sigma_r, np.float32)
    n = len(pl)
    assert len(pr) == len(sl) == len(sr) == n
    code = np.zeros(n, np.float32); p3d = np.zeros((n, 3), np.float32)
    _fisheye_argtypes()
    _check(lib.orbx_kb8_triangulate_matches(device, C.byref(fisheye_rig(rig)), _p(pl), _p(pr), _p(sl), _p(sr), n, _p(code), _p(p3d)))
    return code, p3d


def _lba_problem(w):
    keep = {k: np.ascontiguousarray(w[k]) for k in ("pose_q", "pose_t", "pose_fixed", "points", "edge_point",
                                                      "edge_pose", "edge_obs", "edge_inv_sigma2", "edge_stereo")}
    pr = LbaProblem(len(keep["pose_q"]), keep["pose_q"].ctypes.data, keep["pose_t"].ctypes.data, keep["pose_fixed"].ctypes.data,
                    len(keep["points"]), keep["points"].ctypes.data, len(keep["edge_point"]), keep["edge_point"].ctypes.data,
                    keep["edge_pose"].ctypes.data, keep["edge_obs"].ctypes.data, keep["edge_inv_sigma2"].ctypes.data,
                    keep["edge_stereo"].ctypes.data, w["fx"], w["fy"], w["cx"], w["cy"], w["bf"], w["huber_mono"], w["huber_stereo"])
    pr._keep = keep
    return pr


def _stats_dict(st):
    return dict(iterations=st.iterations, trials=st.trials, stop_reason=st.stop_reason, lambda_=st.lambda_,
                chi2_initial=st.chi2_initial, chi2_final=st.chi2_final, chi2_trace=list(st.chi2_trace))


class LbaSolver:
    """Numerical core of Optimizer::LocalBundleAdjustment (reference src/Optimizer.cc:1116-1498)."""

    def __init__(self, device=0):
        lib.lba_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.lba_destroy.argtypes = [C.c_void_p]
        lib.lba_solve.argtypes = [C.c_void_p, C.POINTER(LbaProblem), C.c_void_p, C.c_int, C.c_double,
                                  C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(LbaStats)]
        h = C.c_void_p()
        _check(lib.lba_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.lba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_camera_kb8(self, cam):
        """lba_set_camera_kb8: dict(fx, fy, cx, cy, k) or None (back to the pinhole camera of the windows)"""
        _set_camera_kb8(lib.lba_set_camera_kb8, self._h, cam)

    def set_rig_kb8(self, rig):
        """lba_set_rig_kb8: dict(left, right, q_rl, t_rl) or None (back to the pinhole camera); edge_stereo then holds 0 or EDGE_RIGHT"""
        _set_rig_kb8(lib.lba_set_rig_kb8, self._h, rig)

    def solve(self, w, max_iters=10, lambda_init=0.0, stop_flag=None):
        pr = _lba_problem(w)
        k = pr._keep
        q = np.zeros_like(k["pose_q"]); t = np.zeros_like(k["pose_t"]); pts = np.zeros_like(k["points"])
        chi2 = np.zeros(len(k["edge_point"])); dpos = np.zeros(len(k["edge_point"]), np.uint8)
        st = LbaStats()
        _check(lib.lba_solve(self._h, C.byref(pr), _p(stop_flag), max_iters, lambda_init,
                             _p(q), _p(t), _p(pts), _p(chi2), _p(dpos), C.byref(st)))
        return dict(pose_q=q, pose_t=t, points=pts, chi2=chi2, depth_positive=dpos, stats=_stats_dict(st))


class LbaOutputs(C.Structure):
    _fields_ = [("pose_q", C.c_void_p), ("pose_t", C.c_void_p), ("points", C.c_void_p), ("chi2_per_edge", C.c_void_p), ("depth_positive", C.c_void_p)]


class LbaBatch:
    """lba_solve_batch: many LocalBundleAdjustment windows (one per map / client session) per launch."""

    def __init__(self, device=0):
        lib.lba_batch_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.lba_batch_destroy.argtypes = [C.c_void_p]
        lib.lba_solve_batch.argtypes = [C.c_void_p, C.POINTER(LbaProblem), C.POINTER(LbaOutputs), C.c_int, C.c_void_p, C.c_int, C.c_double, C.POINTER(LbaStats)]
        lib.lba_batch_last_device_ms.argtypes = [C.c_void_p]
        lib.lba_batch_last_device_ms.restype = C.c_double
        h = C.c_void_p()
        _check(lib.lba_batch_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.lba_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_camera_kb8(self, cam):
        """lba_batch_set_camera_kb8: one fisheye camera for every window of a call, or None"""
        _set_camera_kb8(lib.lba_batch_set_camera_kb8, self._h, cam)

    def set_rig_kb8(self, rig):
        """lba_batch_set_rig_kb8: one rig of two fisheye cameras for every window of a call, or None"""
        _set_rig_kb8(lib.lba_batch_set_rig_kb8, self._h, rig)

    def prepare(self, windows, want_outputs=True):
        """marshal once (a benchmark re-solves the same windows): problem structs, output arrays, stats"""
        n = len(windows)
        prs = [_lba_problem(w) for w in windows]
        arr = (LbaProblem * n)(*prs)
        outs, oarr = [], (LbaOutputs * n)()
        for i, pr in enumerate(prs):
            k = pr._keep
            o = dict(pose_q=np.zeros_like(k["pose_q"]), pose_t=np.zeros_like(k["pose_t"]), points=np.zeros_like(k["points"]),
                     chi2=np.zeros(len(k["edge_point"])), depth_positive=np.zeros(len(k["edge_point"]), np.uint8))
            outs.append(o)
            if want_outputs:
                oarr[i] = LbaOutputs(_p(o["pose_q"]), _p(o["pose_t"]), _p(o["points"]), _p(o["chi2"]), _p(o["depth_positive"]))
        return dict(n=n, prs=prs, arr=arr, outs=outs, oarr=oarr, stats=(LbaStats * n)(), want=want_outputs)

    def run(self, prep, max_iters=10, lambda_init=0.0, stop_flags=None):
        flags = None
        if stop_flags is not None:
            flags = (C.c_void_p * prep["n"])(*[(f.ctypes.data if f is not None else None) for f in stop_flags])
        _check(lib.lba_solve_batch(self._h, prep["arr"], prep["oarr"] if prep["want"] else None, prep["n"], flags, max_iters, lambda_init, prep["stats"]))
        return [dict(o, stats=_stats_dict(prep["stats"][i])) for i, o in enumerate(prep["outs"])]

    def solve(self, windows, max_iters=10, lambda_init=0.0, stop_flags=None):
        return self.run(self.prepare(windows), max_iters, lambda_init, stop_flags)

    def last_device_ms(self):
        return float(lib.lba_batch_last_device_ms(self._h))


class LbaShard:
    """One rank's share of a landmark-sharded global BA; see INTEGRATION.md."""

    def __init__(self, w, device=0):
        lib.lba_shard_create.argtypes = [C.c_int, C.POINTER(LbaProblem), C.POINTER(C.c_void_p)]
        lib.lba_shard_destroy.argtypes = [C.c_void_p]
        lib.lba_shard_reduce_len.argtypes = [C.c_void_p]
        lib.lba_shard_reduce_len.restype = C.c_int64
        lib.lba_shard_reduce_buffer.argtypes = [C.c_void_p]
        lib.lba_shard_reduce_buffer.restype = C.c_void_p
        lib.lba_shard_linearize.argtypes = [C.c_void_p] + [C.POINTER(C.c_double)] * 3
        lib.lba_shard_reduce.argtypes = [C.c_void_p, C.c_double]
        lib.lba_shard_finish.argtypes = [C.c_void_p, C.c_double] + [C.POINTER(C.c_double)] * 3
        lib.lba_shard_accept.argtypes = [C.c_void_p, C.c_int]
        lib.lba_shard_download.argtypes = [C.c_void_p] + [C.c_void_p] * 5
        self._pr = _lba_problem(w)
        h = C.c_void_p()
        _check(lib.lba_shard_create(device, C.byref(self._pr), C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.lba_shard_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reduce_len(self):
        return lib.lba_shard_reduce_len(self._h)

    def reduce_buffer_ptr(self):
        return lib.lba_shard_reduce_buffer(self._h)

    def set_local(self, local=True):
        lib.lba_shard_set_local.argtypes = [C.c_void_p, C.c_int]
        _check(lib.lba_shard_set_local(self._h, int(local)))

    def set_reduce_buffer(self, device_ptr):
        lib.lba_shard_set_reduce_buffer.argtypes = [C.c_void_p, C.c_void_p]
        _check(lib.lba_shard_set_reduce_buffer(self._h, device_ptr))

    def hint_lambda(self, lam):
        """the lambda of the first trial after the next linearize(): lets it fold the landmark side of the Schur complement in"""
        _check(lib.lba_shard_hint_lambda(self._h, C.c_double(lam)))

    def linearize(self):
        """returns (chi2_local, max_diag_poses_local, max_diag_landmarks_local)"""
        chi, mp, ml = C.c_double(), C.c_double(), C.c_double()
        _check(lib.lba_shard_linearize(self._h, C.byref(chi), C.byref(mp), C.byref(ml)))
        return chi.value, mp.value, ml.value

    def reduce(self, lam):
        _check(lib.lba_shard_reduce(self._h, lam))

    def finish(self, lam):
        """returns (solved, chi2_local_new, scale_poses, scale_landmarks_local)"""
        chi, sp, sl = C.c_double(), C.c_double(), C.c_double()
        r = lib.lba_shard_finish(self._h, lam, C.byref(chi), C.byref(sp), C.byref(sl))
        _check(min(r, 0))
        return r, chi.value, sp.value, sl.value

    def accept(self, ok):
        _check(lib.lba_shard_accept(self._h, int(ok)))

    STAGES = ("linearize", "schur", "factor", "solve", "update", "reduce", "gaps")
    STAGE_KERNEL = {"linearize": "k_lin_all", "schur": "k_schur_blocks", "factor": "k_chol_flow", "solve": "k_chol_solve_update",
                    "update": "k_update_errors", "reduce": "k_reduce", "gaps": None}

    def profile_enable(self, on=True):
        lib.lba_shard_profile_enable.argtypes = [C.c_void_p, C.c_int]
        _check(lib.lba_shard_profile_enable(self._h, int(on)))

    def profile_read(self):
        """milliseconds per stage (HIP events on the shard's stream) accumulated since profile_enable(True)"""
        lib.lba_shard_profile_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        ms = np.zeros(len(self.STAGES), np.float32)
        _check(lib.lba_shard_profile_read(self._h, _p(ms), len(ms)))
        return dict(zip(self.STAGES, [float(v) for v in ms]))

    def fence_out(self, other_stream):
        lib.lba_shard_fence_out.argtypes = [C.c_void_p, C.c_void_p]
        _check(lib.lba_shard_fence_out(self._h, C.c_void_p(other_stream)))

    def fence_in(self, other_stream):
        lib.lba_shard_fence_in.argtypes = [C.c_void_p, C.c_void_p]
        _check(lib.lba_shard_fence_in(self._h, C.c_void_p(other_stream)))

    def set_async_reduce(self, on=True):
        lib.lba_shard_set_async_reduce.argtypes = [C.c_void_p, C.c_int]
        _check(lib.lba_shard_set_async_reduce(self._h, int(on)))

    def reset(self):
        lib.lba_shard_reset.argtypes = [C.c_void_p]
        _check(lib.lba_shard_reset(self._h))

    ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p)

    def optimize(self, allreduce=None, world=1, max_iters=10, lambda_init=0.0, stop_flag=None):
        """lba_shard_optimize: the whole Levenberg loop in the library.  `allreduce(device_ptr, count, op, hip_stream) -> int` is
        called for every exchange (op 0 = sum, 1 = max; reduce `count` doubles at `device_ptr` in place over all ranks, ordered on
        `hip_stream`); None = world size 1.  Returns the stats dict."""
        lib.lba_shard_optimize.argtypes = [C.c_void_p, self.ALLREDUCE_FN, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.POINTER(LbaStats)]
        err = []

        def tramp(user, buf, count, op, stream):
            try:
                return int(allreduce(buf, int(count), int(op), stream) or 0)
            except Exception as e:  # noqa: BLE001  (an exception must not cross the C frame)
                err.append(e)
                return 1
        cb = self.ALLREDUCE_FN(tramp) if allreduce is not None else C.cast(None, self.ALLREDUCE_FN)
        st = LbaStats()
        rc = lib.lba_shard_optimize(self._h, cb, None, int(world), int(max_iters), float(lambda_init), _p(stop_flag), C.byref(st))
        if err:
            raise err[0]
        _check(rc)
        return _stats_dict(st)

    def download(self):
        k = self._pr._keep
        q = np.zeros_like(k["pose_q"]); t = np.zeros_like(k["pose_t"]); pts = np.zeros_like(k["points"])
        chi2 = np.zeros(len(k["edge_point"])); dpos = np.zeros(len(k["edge_point"]), np.uint8)
        _check(lib.lba_shard_download(self._h, _p(q), _p(t), _p(pts), _p(chi2), _p(dpos)))
        return dict(pose_q=q, pose_t=t, points=pts, chi2=chi2, depth_positive=dpos)


class PoseProblem(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("n", C.c_int32), ("Xw", C.c_void_p), ("obs", C.c_void_p),
                ("inv_sigma2", C.c_void_p), ("stereo", C.c_void_p),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double),
                ("huber_mono", C.c_double), ("huber_stereo", C.c_double)]


class PoseResult(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("inliers", C.c_int32), ("n_bad", C.c_int32),
                ("iterations", C.c_int32 * 4), ("trials", C.c_int32 * 4), ("chi2", C.c_double * 4)]


class PoseDeviceFrames(C.Structure):
    _fields_ = [("d_kps", C.c_void_p), ("d_n", C.c_void_p), ("d_u_right", C.c_void_p), ("cap", C.c_int32),
                ("d_assign", C.c_void_p), ("d_mp_xyz", C.c_void_p), ("mp_cap", C.c_int32), ("d_pose", C.c_void_p),
                ("inv_level_sigma2", C.c_void_p), ("n_levels", C.c_int32),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double),
                ("huber_mono", C.c_double), ("huber_stereo", C.c_double)]


def _pose_problem(w, pr):
    keep = [np.ascontiguousarray(w["Xw"], np.float64), np.ascontiguousarray(w["obs"], np.float64),
            np.ascontiguousarray(w["inv_sigma2"], np.float64), np.ascontiguousarray(w["stereo"], np.uint8)]
    pr.q[:] = [float(v) for v in w["q"]]
    pr.t[:] = [float(v) for v in w["t"]]
    pr.n = len(keep[0])
    pr.Xw, pr.obs, pr.inv_sigma2, pr.stereo = (a.ctypes.data for a in keep)
    for k in ("fx", "fy", "cx", "cy", "bf", "huber_mono", "huber_stereo"):
        setattr(pr, k, float(w[k]))
    return keep


class PoseSolver:
    """Optimizer::PoseOptimization (reference src/Optimizer.cc:814-1115): motion-only BA, one workgroup per frame."""

    def __init__(self, device=0):
        lib.pose_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.pose_destroy.argtypes = [C.c_void_p]
        lib.pose_optimize_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        h = C.c_void_p()
        _check(lib.pose_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.pose_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_camera_kb8(self, cam):
        """pose_set_camera_kb8: dict(fx, fy, cx, cy, k) or None (back to the pinhole camera of the problems)"""
        _set_camera_kb8(lib.pose_set_camera_kb8, self._h, cam)

    def set_rig_kb8(self, rig):
        """pose_set_rig_kb8: dict(left, right, q_rl, t_rl) or None (back to the pinhole camera); stereo then holds 0 or EDGE_RIGHT"""
        _set_rig_kb8(lib.pose_set_rig_kb8, self._h, rig)

    def optimize_one(self, w):
        """pose_optimize: the single-frame entry"""
        lib.pose_optimize.argtypes = [C.c_void_p, C.POINTER(PoseProblem), C.POINTER(PoseResult), C.c_void_p]
        pr, r = PoseProblem(), PoseResult()
        keep = _pose_problem(w, pr)
        outl = np.zeros(max(pr.n, 1), np.uint8)
        _check(lib.pose_optimize(self._h, C.byref(pr), C.byref(r), _p(outl)))
        del keep
        return dict(q=np.array(r.q[:]), t=np.array(r.t[:]), inliers=r.inliers, n_bad=r.n_bad, iterations=list(r.iterations),
                    trials=list(r.trials), chi2=list(r.chi2), outlier=outl[:pr.n].copy())

    def prepare(self, problems):
        """flatten a list of frames once (benchmarks re-run the same batch)"""
        n = len(problems)
        prs = (PoseProblem * n)()
        keep = [_pose_problem(w, prs[i]) for i, w in enumerate(problems)]
        outl = [np.zeros(max(prs[i].n, 1), np.uint8) for i in range(n)]
        ptrs = (C.c_void_p * n)(*[o.ctypes.data for o in outl])
        return dict(n=n, prs=prs, keep=keep, outl=outl, ptrs=ptrs, res=(PoseResult * n)())

    def launch(self, prep):
        """the C call alone: upload, one kernel launch, download"""
        _check(lib.pose_optimize_batch(self._h, prep["prs"], prep["n"], prep["res"], prep["ptrs"]))

    def results(self, prep):
        return [dict(q=np.array(r.q[:]), t=np.array(r.t[:]), inliers=r.inliers, n_bad=r.n_bad,
                     iterations=list(r.iterations), trials=list(r.trials), chi2=list(r.chi2),
                     outlier=prep["outl"][i][:prep["prs"][i].n].copy()) for i, r in enumerate(prep["res"])]

    def run(self, prep):
        self.launch(prep)
        return self.results(prep)

    def optimize_batch_device(self, batch, cap, d_kps, d_n, d_assign, d_mp_xyz, mp_cap, d_pose, inv_level_sigma2, cam, d_pose_out, d_inliers,
                              d_outlier, stream, d_u_right=None, d_results=None):
        """pose_optimize_batch_device: every d_* argument is a device address (int); `cam` = dict(fx, fy, cx, cy, bf[, huber_mono,
        huber_stereo]); inv_level_sigma2 a host float array.  Only enqueues on `stream`."""
        lib.pose_optimize_batch_device.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        isig = np.ascontiguousarray(inv_level_sigma2, np.float32)
        f = PoseDeviceFrames(d_kps, d_n, d_u_right, cap, d_assign, d_mp_xyz, mp_cap, d_pose, isig.ctypes.data, len(isig),
                             float(cam["fx"]), float(cam["fy"]), float(cam["cx"]), float(cam["cy"]), float(cam.get("bf", 0.0)),
                             float(cam.get("huber_mono", np.float32(np.sqrt(5.991)))), float(cam.get("huber_stereo", np.float32(np.sqrt(7.815)))))
        _check(lib.pose_optimize_batch_device(self._h, C.byref(f), batch, d_pose_out, d_inliers, d_outlier, d_results, stream))

    def optimize_rig_batch_device(self, frames, batch, d_pose_out=None, d_inliers=None, d_outlier=None, d_results=None, stream=None):
        """pose_optimize_rig_batch_device on a handle with a rig set: frames a dict keyed by the fields of PoseDeviceRigFrames (device
        addresses as ints; inv_level_sigma2 a host float array; huber_mono defaults to sqrt(5.991) as a float).  Only enqueues."""
        _rig_track_device_argtypes()
        isig = np.ascontiguousarray(frames["inv_level_sigma2"], np.float32)
        v = dict(frames, inv_level_sigma2=isig.ctypes.data)
        v.setdefault("n_levels", len(isig)); v.setdefault("huber_mono", float(np.float32(np.sqrt(5.991))))
        v.setdefault("slot_cap", int(frames["cap_l"]) + int(frames["cap_r"]))
        f = PoseDeviceRigFrames(*[v.get(k) for k, _ in PoseDeviceRigFrames._fields_])
        _check(lib.pose_optimize_rig_batch_device(self._h, C.byref(f), int(batch), d_pose_out, d_inliers, d_outlier, d_results, stream))

    def last_kernel_ms(self):
        lib.pose_last_kernel_ms.restype = C.c_float
        lib.pose_last_kernel_ms.argtypes = [C.c_void_p]
        return float(lib.pose_last_kernel_ms(self._h))

    def optimize_batch(self, problems):
        return self.run(self.prepare(problems))

    def optimize(self, w):
        return self.optimize_batch([w])[0]


class OrbvVocabulary(C.Structure):
    _fields_ = [("n_nodes", C.c_int32), ("L", C.c_int32), ("child_off", C.c_void_p), ("child_id", C.c_void_p),
                ("desc", C.c_void_p), ("weight", C.c_void_p), ("word_id", C.c_void_p)]


def vocabulary_struct(voc, cls=OrbvVocabulary):
    keep = [np.ascontiguousarray(voc["child_off"], np.int32), np.ascontiguousarray(voc["child_id"], np.uint32),
            np.ascontiguousarray(voc["desc"], np.uint8), np.ascontiguousarray(voc["weight"], np.float64),
            np.ascontiguousarray(voc["word_id"], np.int32)]
    s = cls(int(voc["n_nodes"]), int(voc["L"]), *[a.ctypes.data for a in keep])
    s._keep = keep
    return s


class Vocabulary:
    """DBoW2 TemplatedVocabulary::transform for ORB descriptors (TF_IDF, L1) on a device-resident tree."""

    def __init__(self, voc, device=0):
        s = vocabulary_struct(voc)
        h = C.c_void_p()
        _check(lib.orbv_create(device, C.byref(s), C.byref(h)))
        self._h = h
        lib.orbv_destroy.argtypes = [C.c_void_p]

    def close(self):
        if getattr(self, "_h", None):
            lib.orbv_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def transform_features(self, desc, levelsup=4):
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(desc)
        word = np.zeros(max(n, 1), np.uint32); weight = np.zeros(max(n, 1)); node = np.zeros(max(n, 1), np.uint32)
        _check(lib.orbv_transform_features(self._h, _p(desc), n, int(levelsup), _p(word), _p(weight), _p(node)))
        return word[:n], weight[:n], node[:n]

    def transform(self, desc, levelsup=4):
        """returns (bow_id, bow_val), (fv_node, fv_off, fv_feat)"""
        desc = np.ascontiguousarray(desc, np.uint8)
        n = len(desc)
        m = max(n, 1)
        bi = np.zeros(m, np.uint32); bv = np.zeros(m); fn = np.zeros(m, np.uint32); fo = np.zeros(m + 1, np.int32); ff = np.zeros(m, np.uint32)
        nb, nf = C.c_int32(), C.c_int32()
        used = _check(lib.orbv_transform(self._h, _p(desc), n, int(levelsup), _p(bi), _p(bv), C.byref(nb), _p(fn), _p(fo), _p(ff), C.byref(nf)))
        return (bi[:nb.value], bv[:nb.value]), (fn[:nf.value], fo[:nf.value + 1], ff[:used])

    def transform_batch_device(self, d_desc, d_n, batch, cap, levelsup, d_bow_id, d_bow_val, d_n_bow, d_fv_node, d_fv_off, d_fv_feat,
                               d_n_fv, stream=None):
        _check(lib.orbv_transform_batch_device(self._h, C.c_void_p(d_desc), C.c_void_p(d_n), int(batch), int(cap), int(levelsup),
                                               C.c_void_p(d_bow_id), C.c_void_p(d_bow_val), C.c_void_p(d_n_bow), C.c_void_p(d_fv_node),
                                               C.c_void_p(d_fv_off), C.c_void_p(d_fv_feat), C.c_void_p(d_n_fv), C.c_void_p(stream or 0)))


IMU_DTYPE = np.dtype([("ts", "i8"), ("gyro", "f4", (3,)), ("acce", "f4", (3,))])      # OrbeImuSample, the 32-byte wire record


class PacketCodec:
    """The fork's edge-SLAM packets (class SlamPktVI, reference include/Socket/slampkt_vi.h) packed / unpacked on the device."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib.orbe_create(device, C.byref(h)))
        self._h = h
        lib.orbe_destroy.argtypes = [C.c_void_p]

    def close(self):
        if getattr(self, "_h", None):
            lib.orbe_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def packet_bytes(n_pts, n_imu=0):
        return lib.orbe_packet_bytes(int(n_pts), int(n_imu))

    def pack_batch(self, kps, desc, n, frame_id, timestamp, imu=None, imu_off=None, stride=None):
        """kps [B][cap] KP_DTYPE, desc [B][cap][32], n [B]; returns (payload [B][stride] u8, len [B], head [B][2], status [B])"""
        kps = np.ascontiguousarray(kps, KP_DTYPE); desc = np.ascontiguousarray(desc, np.uint8)
        B, cap = kps.shape
        n = np.ascontiguousarray(n, np.int32); frame_id = np.ascontiguousarray(frame_id, np.int32)
        timestamp = np.ascontiguousarray(timestamp, np.int64)
        assert desc.shape == (B, cap, 32) and n.shape == (B,) and frame_id.shape == (B,) and timestamp.shape == (B,)
        if imu is not None:
            imu = np.ascontiguousarray(imu, IMU_DTYPE); imu_off = np.ascontiguousarray(imu_off, np.int32)
            assert imu_off.shape == (B + 1,) and imu_off[-1] <= len(imu)
            max_imu = int(np.diff(imu_off).max()) if B else 0
        else:
            max_imu = 0
        if stride is None:
            stride = (self.packet_bytes(int(n.max()) if B else 0, max_imu) + 3) & ~3
        payload = np.zeros((B, stride), np.uint8); ln = np.zeros(B, np.int32); head = np.zeros((B, 2), np.uint8); st = np.zeros(B, np.int32)
        _check(lib.orbe_pack_batch(self._h, _p(kps), _p(desc), _p(n), B, cap, _p(frame_id), _p(timestamp),
                                   _p(imu) if imu is not None else None, _p(imu_off) if imu is not None else None,
                                   _p(payload), int(stride), _p(ln), _p(head), _p(st)))
        return payload, ln, head, st

    def unpack_batch(self, payload, ln, cap, imu_cap=0):
        """payload [B][stride] u8, ln [B]; returns dict(kps, desc, n, frame_id, timestamp, imu, n_imu, status)"""
        payload = np.ascontiguousarray(payload, np.uint8); ln = np.ascontiguousarray(ln, np.int32)
        B, stride = payload.shape
        kps = np.zeros((B, cap), KP_DTYPE); desc = np.zeros((B, cap, 32), np.uint8); n = np.zeros(B, np.int32)
        fid = np.zeros(B, np.int32); ts = np.zeros(B, np.int64); imu = np.zeros((B, max(imu_cap, 1)), IMU_DTYPE)
        ni = np.zeros(B, np.int32); st = np.zeros(B, np.int32)
        _check(lib.orbe_unpack_batch(self._h, _p(payload), int(stride), _p(ln), B, int(cap), int(imu_cap), _p(kps), _p(desc), _p(n),
                                     _p(fid), _p(ts), _p(imu) if imu_cap > 0 else None, _p(ni), _p(st)))
        return dict(kps=kps, desc=desc, n=n, frame_id=fid, timestamp=ts, imu=imu, n_imu=ni, status=st)

    def pack_batch_device(self, d_kps, d_desc, d_n, batch, cap, d_frame_id, d_timestamp, d_imu, d_imu_off, d_payload, stride, d_len, d_head,
                          d_status, stream=None):
        _check(lib.orbe_pack_batch_device(self._h, C.c_void_p(d_kps), C.c_void_p(d_desc), C.c_void_p(d_n), int(batch), int(cap),
                                          C.c_void_p(d_frame_id), C.c_void_p(d_timestamp), C.c_void_p(d_imu or 0), C.c_void_p(d_imu_off or 0),
                                          C.c_void_p(d_payload), int(stride), C.c_void_p(d_len), C.c_void_p(d_head or 0), C.c_void_p(d_status),
                                          C.c_void_p(stream or 0)))

    class _Camera(C.Structure):
        _fields_ = [("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float), ("k", C.c_float * 5),
                    ("fx_new", C.c_float), ("fy_new", C.c_float), ("cx_new", C.c_float), ("cy_new", C.c_float)]

    def undistort_batch_device(self, d_kps, d_n, batch, cap, K, dist, Knew, d_kps_un, stream=None):
        """Frame::UndistortKeyPoints on device arrays: K / Knew = (fx, fy, cx, cy), dist = (k1, k2, p1, p2, k3)"""
        cam = self._Camera(float(K[0]), float(K[1]), float(K[2]), float(K[3]), (C.c_float * 5)(*[float(v) for v in dist]),
                           float(Knew[0]), float(Knew[1]), float(Knew[2]), float(Knew[3]))
        _check(lib.orbe_undistort_batch_device(self._h, C.c_void_p(d_kps), C.c_void_p(d_n), int(batch), int(cap), C.byref(cam), C.c_void_p(d_kps_un),
                                               C.c_void_p(stream or 0)))

    def unpack_batch_device(self, d_payload, stride, d_len, batch, cap, imu_cap, d_kps, d_desc, d_n, d_frame_id, d_timestamp, d_imu, d_n_imu,
                            d_status, stream=None):
        _check(lib.orbe_unpack_batch_device(self._h, C.c_void_p(d_payload), int(stride), C.c_void_p(d_len), int(batch), int(cap), int(imu_cap),
                                            C.c_void_p(d_kps), C.c_void_p(d_desc), C.c_void_p(d_n), C.c_void_p(d_frame_id),
                                            C.c_void_p(d_timestamp), C.c_void_p(d_imu or 0), C.c_void_p(d_n_imu), C.c_void_p(d_status),
                                            C.c_void_p(stream or 0)))


class _LibaLink(C.Structure):
    _fields_ = [("kf1", C.c_int32), ("kf2", C.c_int32), ("dR", C.c_float * 9), ("dV", C.c_float * 3), ("dP", C.c_float * 3),
                ("JRg", C.c_float * 9), ("JVg", C.c_float * 9), ("JVa", C.c_float * 9), ("JPg", C.c_float * 9), ("JPa", C.c_float * 9),
                ("dT", C.c_float), ("bias0", C.c_float * 6), ("info9", C.c_double * 81), ("info_gyro", C.c_double * 9), ("info_acc", C.c_double * 9),
                ("robust", C.c_uint8)]


class _LibaProblem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("Rwb", C.c_void_p), ("twb", C.c_void_p), ("vel", C.c_void_p), ("bg", C.c_void_p), ("ba", C.c_void_p),
                ("pose_fixed", C.c_void_p), ("has_imu", C.c_void_p), ("imu_fixed", C.c_void_p),
                ("Rcb", C.c_double * 9), ("tcb", C.c_double * 3), ("tbc", C.c_double * 3),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double),
                ("n_points", C.c_int32), ("points", C.c_void_p), ("n_edges", C.c_int32), ("edge_kf", C.c_void_p), ("edge_point", C.c_void_p),
                ("edge_obs", C.c_void_p), ("edge_inv_sigma2", C.c_void_p), ("edge_stereo", C.c_void_p),
                ("n_links", C.c_int32), ("links", C.c_void_p),
                ("huber_mono", C.c_double), ("huber_stereo", C.c_double), ("huber_inertial", C.c_double), ("lambda_init", C.c_double), ("max_iters", C.c_int32)]


class _LibaStats(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("trials", C.c_int32), ("stop_reason", C.c_int32),
                ("lambda_", C.c_double), ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("chi2_trace", C.c_double * 16)]


def _liba_problem(pr):
    dt = dict(Rwb=np.float64, twb=np.float64, vel=np.float64, bg=np.float64, ba=np.float64, pose_fixed=np.uint8, has_imu=np.uint8, imu_fixed=np.uint8,
              points=np.float64, edge_kf=np.int32, edge_point=np.int32, edge_obs=np.float64, edge_inv_sigma2=np.float64, edge_stereo=np.uint8)
    keep = {k: np.ascontiguousarray(pr[k], t) for k, t in dt.items()}
    links = (_LibaLink * max(len(pr["links"]), 1))()
    for L, d in zip(links, pr["links"]):
        L.kf1, L.kf2, L.dT, L.robust = int(d["kf1"]), int(d["kf2"]), float(d["dT"]), int(d["robust"])
        for name in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bias0"):
            getattr(L, name)[:] = np.asarray(d[name], np.float32).ravel().tolist()
        for name in ("info9", "info_gyro", "info_acc"):
            getattr(L, name)[:] = np.asarray(d[name], np.float64).ravel().tolist()
    s = _LibaProblem()
    s.n_kf = int(pr["n_kf"])
    for k in dt:
        setattr(s, k, keep[k].ctypes.data)
    s.Rcb[:] = np.asarray(pr["Rcb"], np.float64).ravel().tolist(); s.tcb[:] = list(map(float, pr["tcb"])); s.tbc[:] = list(map(float, pr["tbc"]))
    s.fx, s.fy, s.cx, s.cy, s.bf = pr["fx"], pr["fy"], pr["cx"], pr["cy"], pr["bf"]
    s.n_points = len(keep["points"]); s.n_edges = len(keep["edge_kf"]); s.n_links = len(pr["links"]); s.links = C.addressof(links)
    s.huber_mono, s.huber_stereo, s.huber_inertial = pr["huber_mono"], pr["huber_stereo"], pr["huber_inertial"]
    s.lambda_init, s.max_iters = float(pr["lambda_init"]), int(pr["max_iters"])
    s._keep = (keep, links)
    return s


class InertialSolver:
    """The numerical core of Optimizer::LocalInertialBA (reference src/Optimizer.cc:2383-2958) on the device."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib.liba_create(device, C.byref(h)))
        self._h = h
        lib.liba_destroy.argtypes = [C.c_void_p]

    def close(self):
        if getattr(self, "_h", None):
            lib.liba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, pr):
        s = _liba_problem(pr)
        n, m, ne = s.n_kf, s.n_points, s.n_edges
        Rwb = np.zeros((n, 3, 3)); twb = np.zeros((n, 3)); vel = np.zeros((n, 3)); bg = np.zeros((n, 3)); ba = np.zeros((n, 3))
        pts = np.zeros((max(m, 1), 3)); chi2 = np.zeros(max(ne, 1)); dpos = np.zeros(max(ne, 1), np.uint8)
        st = _LibaStats()
        _check(lib.liba_solve(self._h, C.byref(s), _p(Rwb), _p(twb), _p(vel), _p(bg), _p(ba), _p(pts), _p(chi2), _p(dpos), C.byref(st)))
        stats = dict(iterations=st.iterations, trials=st.trials, stop_reason=st.stop_reason, lambda_=st.lambda_, chi2_initial=st.chi2_initial,
                     chi2_final=st.chi2_final)
        return dict(Rwb=Rwb, twb=twb, vel=vel, bg=bg, ba=ba, points=pts[:m], chi2=chi2[:ne], depth_positive=dpos[:ne], stats=stats)


class LibaOutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("Rwb", "twb", "vel", "bg", "ba", "points", "chi2_per_edge", "depth_positive")]


class LibaBatch:
    """liba_solve_batch: many LocalInertialBA windows (one per map / client session) per launch."""

    def __init__(self, device=0):
        lib.liba_batch_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.liba_batch_destroy.argtypes = [C.c_void_p]
        lib.liba_solve_batch.argtypes = [C.c_void_p, C.POINTER(_LibaProblem), C.POINTER(LibaOutputs), C.c_int, C.POINTER(_LibaStats)]
        lib.liba_batch_last_device_ms.argtypes = [C.c_void_p]
        lib.liba_batch_last_device_ms.restype = C.c_double
        h = C.c_void_p()
        _check(lib.liba_batch_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.liba_batch_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def prepare(self, windows, want_outputs=True):
        """marshal once (a benchmark re-solves the same windows)"""
        n = len(windows)
        prs = [_liba_problem(w) for w in windows]
        arr = (_LibaProblem * n)(*prs)
        outs, oarr = [], (LibaOutputs * n)()
        for i, s in enumerate(prs):
            nk, m, ne = s.n_kf, s.n_points, s.n_edges
            o = dict(Rwb=np.zeros((nk, 3, 3)), twb=np.zeros((nk, 3)), vel=np.zeros((nk, 3)), bg=np.zeros((nk, 3)), ba=np.zeros((nk, 3)),
                     points=np.zeros((max(m, 1), 3)), chi2=np.zeros(max(ne, 1)), depth_positive=np.zeros(max(ne, 1), np.uint8))
            outs.append(o)
            if want_outputs:
                oarr[i] = LibaOutputs(*[o[k].ctypes.data for k in ("Rwb", "twb", "vel", "bg", "ba", "points", "chi2", "depth_positive")])
        return dict(n=n, prs=prs, arr=arr, outs=outs, oarr=oarr, stats=(_LibaStats * n)(), want=want_outputs)

    def run(self, prep):
        _check(lib.liba_solve_batch(self._h, prep["arr"], prep["oarr"] if prep["want"] else None, prep["n"], prep["stats"]))
        res = []
        for i, o in enumerate(prep["outs"]):
            s, st = prep["prs"][i], prep["stats"][i]
            stats = dict(iterations=st.iterations, trials=st.trials, stop_reason=st.stop_reason, lambda_=st.lambda_, chi2_initial=st.chi2_initial,
                         chi2_final=st.chi2_final)
            res.append(dict(Rwb=o["Rwb"], twb=o["twb"], vel=o["vel"], bg=o["bg"], ba=o["ba"], points=o["points"][:s.n_points], chi2=o["chi2"][:s.n_edges],
                            depth_positive=o["depth_positive"][:s.n_edges], stats=stats))
        return res

    def solve(self, windows):
        return self.run(self.prepare(windows))

    def last_device_ms(self):
        return float(lib.liba_batch_last_device_ms(self._h))


class _LibaPoseProblem(C.Structure):
    _fields_ = [("Rwb", C.c_double * 18), ("twb", C.c_double * 6), ("vel", C.c_double * 6), ("bg", C.c_double * 6), ("ba", C.c_double * 6),
                ("Rcb", C.c_double * 9), ("tcb", C.c_double * 3), ("tbc", C.c_double * 3),
                ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double), ("cy", C.c_double), ("bf", C.c_double),
                ("n", C.c_int32), ("Xw", C.c_void_p), ("obs", C.c_void_p), ("inv_sigma2", C.c_void_p), ("stereo", C.c_void_p), ("close_point", C.c_void_p),
                ("link", _LibaLink), ("huber_mono", C.c_double), ("huber_stereo", C.c_double), ("rec_init", C.c_int32),
                ("last_frame", C.c_int32), ("prior_Rwb", C.c_double * 9), ("prior_twb", C.c_double * 3), ("prior_vel", C.c_double * 3),
                ("prior_bg", C.c_double * 3), ("prior_ba", C.c_double * 3), ("prior_H", C.c_double * 225)]


def _fill_liba_pose(s, pr, keep):
    arrs = {k: np.ascontiguousarray(pr[k], t) for k, t in (("Xw", np.float64), ("obs", np.float64), ("inv_sigma2", np.float64), ("stereo", np.uint8),
                                                           ("close_point", np.uint8))}
    keep.append(arrs)
    for k, m in (("Rwb", 18), ("twb", 6), ("vel", 6), ("bg", 6), ("ba", 6), ("Rcb", 9), ("tcb", 3), ("tbc", 3)):
        getattr(s, k)[:] = np.asarray(pr[k], np.float64).ravel().tolist()
    s.fx, s.fy, s.cx, s.cy, s.bf = pr["fx"], pr["fy"], pr["cx"], pr["cy"], pr["bf"]
    s.n = len(arrs["Xw"])
    for k in arrs:
        setattr(s, k, arrs[k].ctypes.data)
    d, L = pr["link"], s.link
    L.kf1, L.kf2, L.dT, L.robust = int(d["kf1"]), int(d["kf2"]), float(d["dT"]), int(d["robust"])
    for name in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bias0"):
        getattr(L, name)[:] = np.asarray(d[name], np.float32).ravel().tolist()
    for name in ("info9", "info_gyro", "info_acc"):
        getattr(L, name)[:] = np.asarray(d[name], np.float64).ravel().tolist()
    s.huber_mono, s.huber_stereo, s.rec_init = pr["huber_mono"], pr["huber_stereo"], int(pr["rec_init"])
    s.last_frame = int(pr.get("last_frame", 0))
    if s.last_frame:
        for k in ("prior_Rwb", "prior_twb", "prior_vel", "prior_bg", "prior_ba", "prior_H"):
            getattr(s, k)[:] = np.asarray(pr[k], np.float64).ravel().tolist()


def _pose_inertial_prepare(self, problems):
    """flatten a list of frames once (what a C++ caller holds anyway; benchmarks re-run the same batch)"""
    B = len(problems)
    arr = (_LibaPoseProblem * B)()
    keep = []
    for s, pr in zip(arr, problems):
        _fill_liba_pose(s, pr, keep)
    tot = sum(int(s.n) for s in arr)
    N = 30 if int(problems[0].get("last_frame", 0)) else 15         # last-frame variant: the 30 x 30 Hessian before Optimizer::Marginalize
    return dict(B=B, arr=arr, keep=keep, tot=tot, Rwb=np.zeros((B, 3, 3)), twb=np.zeros((B, 3)), vel=np.zeros((B, 3)), bg=np.zeros((B, 3)),
                ba=np.zeros((B, 3)), out=np.zeros(max(tot, 1), np.uint8), H=np.zeros((B, N, N)), inl=np.zeros(B, np.int32), nb=np.zeros(B, np.int32))


def _pose_inertial_launch(self, q):
    """the C call alone: one copy in, one kernel launch, one copy out"""
    _check(lib.liba_pose_optimize_batch(self._h, q["arr"], q["B"], _p(q["Rwb"]), _p(q["twb"]), _p(q["vel"]), _p(q["bg"]), _p(q["ba"]),
                                        _p(q["out"]), _p(q["H"]), _p(q["inl"]), _p(q["nb"])))


def _pose_inertial_results(self, q):
    res, o = [], 0
    for b in range(q["B"]):
        n = int(q["arr"][b].n)
        res.append(dict(Rwb=q["Rwb"][b].copy(), twb=q["twb"][b].copy(), vel=q["vel"][b].copy(), bg=q["bg"][b].copy(), ba=q["ba"][b].copy(),
                        outlier=q["out"][o:o + n].copy(), H=q["H"][b].copy(), n_bad=int(q["nb"][b]), inliers=int(q["inl"][b])))
        o += n
    return res


def _pose_inertial_batch(self, problems):
    """Optimizer::PoseInertialOptimizationLastKeyFrame for a batch of frames: list of dict(Rwb, twb, vel, bg, ba, outlier, H, n_bad, inliers)"""
    q = _pose_inertial_prepare(self, problems)
    _pose_inertial_launch(self, q)
    return _pose_inertial_results(self, q)


InertialSolver.pose_prepare = _pose_inertial_prepare
InertialSolver.pose_launch = _pose_inertial_launch
InertialSolver.pose_results = _pose_inertial_results
InertialSolver.pose_optimize_batch = _pose_inertial_batch


class Sim3RansacProblem(C.Structure):
    _fields_ = [("n", C.c_int32), ("X1c", C.c_void_p), ("X2c", C.c_void_p), ("max_err1", C.c_void_p), ("max_err2", C.c_void_p),
                ("fx1", C.c_float), ("fy1", C.c_float), ("cx1", C.c_float), ("cy1", C.c_float),
                ("fx2", C.c_float), ("fy2", C.c_float), ("cx2", C.c_float), ("cy2", C.c_float),
                ("fix_scale", C.c_int32), ("min_inliers", C.c_int32), ("n_hyp", C.c_int32), ("triples", C.c_void_p)]


class Sim3RansacResult(C.Structure):
    _fields_ = [("converged", C.c_int32), ("index", C.c_int32), ("scored", C.c_int32),
                ("count", C.c_void_p), ("T12", C.c_void_p), ("mask", C.c_void_p)]


class Sim3OptProblem(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("n", C.c_int32),
                ("X1c", C.c_void_p), ("X2c", C.c_void_p), ("obs1", C.c_void_p), ("obs2", C.c_void_p),
                ("inv_sigma2_1", C.c_void_p), ("inv_sigma2_2", C.c_void_p),
                ("fx1", C.c_double), ("fy1", C.c_double), ("cx1", C.c_double), ("cy1", C.c_double),
                ("fx2", C.c_double), ("fy2", C.c_double), ("cx2", C.c_double), ("cy2", C.c_double),
                ("th2", C.c_double), ("huber_delta", C.c_double), ("fix_scale", C.c_int32)]


class Sim3OptResult(C.Structure):
    _fields_ = [("q", C.c_double * 4), ("t", C.c_double * 3), ("s", C.c_double), ("n_in", C.c_int32), ("n_bad", C.c_int32),
                ("iterations", C.c_int32 * 2), ("trials", C.c_int32 * 2), ("stop_reason", C.c_int32 * 2), ("chi2", C.c_double * 2)]


SIM3_LDS_CORRESPONDENCES = 1024
SIM3_MAX_HYPOTHESES = 1024


def sim3_draw_triples(seed, n, n_hyp):
    """sim3_draw_triples: the draw-three-without-replacement of Sim3Solver::iterate (src/Sim3Solver.cc:172-186) with the
    header's splitmix64 generator; host only (needs no device).  Returns int32 [n_hyp][3]."""
    lib.sim3_draw_triples.argtypes = [C.c_uint64, C.c_int, C.c_int, C.c_void_p]
    out = np.zeros((max(n_hyp, 0), 3), np.int32)
    _check(lib.sim3_draw_triples(int(seed), int(n), int(n_hyp), _p(out)))
    return out


class Sim3Solver:
    """Sim3Solver::iterate (reference src/Sim3Solver.cc) and Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381): one workgroup
    per problem, a batch per launch."""

    def __init__(self, device=0):
        lib.sim3_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.sim3_destroy.argtypes = [C.c_void_p]
        lib.sim3_ransac_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        lib.sim3_optimize_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        lib.sim3_last_kernel_ms.restype = C.c_float
        lib.sim3_last_kernel_ms.argtypes = [C.c_void_p]
        h = C.c_void_p()
        _check(lib.sim3_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.sim3_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def last_kernel_ms(self):
        return float(lib.sim3_last_kernel_ms(self._h))

    def ransac_prepare(self, problems):
        """flatten a list of problems once: dict(X1c, X2c [n][3], max_err1, max_err2 [n], K1, K2 (fx fy cx cy), fix_scale,
        min_inliers, triples [H][3])"""
        B = len(problems)
        prs, res = (Sim3RansacProblem * B)(), (Sim3RansacResult * B)()
        keep, outs = [], []
        for i, w in enumerate(problems):
            a = [np.ascontiguousarray(w["X1c"], np.float32).reshape(-1, 3), np.ascontiguousarray(w["X2c"], np.float32).reshape(-1, 3),
                 np.ascontiguousarray(w["max_err1"], np.float32), np.ascontiguousarray(w["max_err2"], np.float32),
                 np.ascontiguousarray(w["triples"], np.int32).reshape(-1, 3)]
            n = len(a[0])
            if not (a[1].shape == (n, 3) and a[2].shape == (n,) and a[3].shape == (n,)):     # the C side copies n rows of each array
                raise ValueError("problem %d: X2c / max_err1 / max_err2 do not hold %d correspondences" % (i, n))
            keep.append(a)
            p = prs[i]
            p.n, p.n_hyp = n, len(a[4])
            p.X1c, p.X2c, p.max_err1, p.max_err2, p.triples = (x.ctypes.data for x in a)
            p.fx1, p.fy1, p.cx1, p.cy1 = (float(v) for v in w["K1"])
            p.fx2, p.fy2, p.cx2, p.cy2 = (float(v) for v in w["K2"])
            p.fix_scale, p.min_inliers = int(bool(w["fix_scale"])), int(w["min_inliers"])
            o = dict(count=np.zeros(p.n_hyp, np.int32), T12=np.zeros((p.n_hyp, 13), np.float32),
                     mask=np.zeros((p.n_hyp, (p.n + 63) // 64), np.uint64))
            res[i].count, res[i].T12, res[i].mask = o["count"].ctypes.data, o["T12"].ctypes.data, o["mask"].ctypes.data
            outs.append(o)
        return dict(B=B, prs=prs, res=res, keep=keep, outs=outs)

    def ransac_launch(self, prep):
        """the C call alone: upload, one kernel launch, download"""
        _check(lib.sim3_ransac_batch(self._h, prep["prs"], prep["B"], prep["res"]))

    def ransac_results(self, prep):
        return [dict(converged=int(r.converged), index=int(r.index), scored=int(r.scored), count=o["count"].copy(), T12=o["T12"].copy(),
                     mask=o["mask"].copy()) for r, o in zip(prep["res"], prep["outs"])]

    def ransac_batch(self, problems):
        prep = self.ransac_prepare(problems)
        self.ransac_launch(prep)
        return self.ransac_results(prep)

    def ransac(self, w):
        return self.ransac_batch([w])[0]

    def optimize_prepare(self, problems):
        """flatten a list of problems once: dict(q (x y z w), t, s, X1c, X2c [n][3], obs1, obs2 [n][2], inv_sigma2_1/2 [n], K1, K2,
        th2, huber_delta, fix_scale)"""
        B = len(problems)
        prs, res = (Sim3OptProblem * B)(), (Sim3OptResult * B)()
        keep, outs = [], []
        for i, w in enumerate(problems):
            a = [np.ascontiguousarray(w[k], np.float64) for k in ("X1c", "X2c", "obs1", "obs2", "inv_sigma2_1", "inv_sigma2_2")]
            n = len(a[4])
            if [x.size for x in a] != [3 * n, 3 * n, 2 * n, 2 * n, n, n]:                    # the C side copies n rows of each array
                raise ValueError("problem %d: the arrays do not hold %d edge pairs each" % (i, n))
            keep.append(a)
            p = prs[i]
            p.q[:] = [float(v) for v in w["q"]]
            p.t[:] = [float(v) for v in w["t"]]
            p.s = float(w["s"])
            p.n = len(a[4])
            p.X1c, p.X2c, p.obs1, p.obs2, p.inv_sigma2_1, p.inv_sigma2_2 = (x.ctypes.data for x in a)
            p.fx1, p.fy1, p.cx1, p.cy1 = (float(v) for v in w["K1"])
            p.fx2, p.fy2, p.cx2, p.cy2 = (float(v) for v in w["K2"])
            p.th2, p.huber_delta, p.fix_scale = float(w["th2"]), float(w["huber_delta"]), int(bool(w["fix_scale"]))
            outs.append(np.zeros(max(p.n, 1), np.uint8))
        ptrs = (C.c_void_p * B)(*[o.ctypes.data for o in outs])
        return dict(B=B, prs=prs, res=res, keep=keep, outs=outs, ptrs=ptrs)

    def optimize_launch(self, prep):
        _check(lib.sim3_optimize_batch(self._h, prep["prs"], prep["B"], prep["res"], prep["ptrs"]))

    def optimize_results(self, prep):
        return [dict(q=np.array(r.q[:]), t=np.array(r.t[:]), s=float(r.s), n_in=int(r.n_in), n_bad=int(r.n_bad),
                     iterations=list(r.iterations), trials=list(r.trials), stop_reason=list(r.stop_reason), chi2=list(r.chi2),
                     keep=prep["outs"][i][:prep["prs"][i].n].astype(bool)) for i, r in enumerate(prep["res"])]

    def optimize_batch(self, problems):
        prep = self.optimize_prepare(problems)
        self.optimize_launch(prep)
        return self.optimize_results(prep)

    def optimize(self, w):
        return self.optimize_batch([w])[0]


ESSG_MAX_FREE_VERTICES = 1024


class EssgProblem(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("sim3", C.c_void_p), ("fixed", C.c_void_p),
                ("n_edges", C.c_int32), ("edge_vertices", C.c_void_p), ("edge_measurement", C.c_void_p),
                ("fix_scale", C.c_int32), ("max_iters", C.c_int32), ("lambda_init", C.c_double),
                ("n_points", C.c_int32), ("points", C.c_void_p), ("point_ref", C.c_void_p)]


class EssgResult(C.Structure):
    _fields_ = [("sim3_out", C.c_void_p), ("pose_q", C.c_void_p), ("pose_t", C.c_void_p), ("points_out", C.c_void_p),
                ("stats", LbaStats)]


def essg_prepare(w):
    """EssgProblem / EssgResult of a graph dictionary (synth_posegraph.make_posegraph) with the arrays they point to"""
    k = dict(sim3=np.ascontiguousarray(w["sim3"], np.float64).reshape(-1, 8), fixed=np.ascontiguousarray(w["fixed"], np.uint8),
             ev=np.ascontiguousarray(w["edge_vertices"], np.int32).reshape(-1, 2),
             meas=np.ascontiguousarray(w["edge_measurement"], np.float64).reshape(-1, 8),
             points=np.ascontiguousarray(w.get("points", np.zeros((0, 3))), np.float32).reshape(-1, 3),
             ref=np.ascontiguousarray(w.get("point_ref", np.zeros(0)), np.int32))
    nv, ne, npt = len(k["sim3"]), len(k["ev"]), len(k["points"])
    if len(k["fixed"]) != nv or len(k["meas"]) != ne or len(k["ref"]) != npt:
        raise ValueError("essential graph arrays of unequal length")
    k.update(sim3_out=np.zeros((nv, 8)), pose_q=np.zeros((nv, 4), np.float32), pose_t=np.zeros((nv, 3), np.float32),
             points_out=np.zeros((npt, 3), np.float32))
    pr = EssgProblem(nv, k["sim3"].ctypes.data, k["fixed"].ctypes.data, ne, k["ev"].ctypes.data if ne else None,
                     k["meas"].ctypes.data if ne else None, int(w.get("fix_scale", 0)), int(w.get("max_iters", 20)),
                     float(w.get("lambda_init", 1e-16)), npt, k["points"].ctypes.data if npt else None, k["ref"].ctypes.data if npt else None)
    res = EssgResult(k["sim3_out"].ctypes.data, k["pose_q"].ctypes.data, k["pose_t"].ctypes.data,
                     k["points_out"].ctypes.data if npt else None)
    return dict(problem=pr, result=res, arrays=k)


class Essg4DofProblem(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("rcw", C.c_void_p), ("tcw", C.c_void_p), ("rwb", C.c_void_p), ("twb", C.c_void_p),
                ("rcb", C.c_void_p), ("tcb", C.c_void_p), ("fixed", C.c_void_p),
                ("n_edges", C.c_int32), ("edge_vertices", C.c_void_p), ("edge_rot", C.c_void_p), ("edge_trans", C.c_void_p),
                ("information", C.c_double * 36), ("max_iters", C.c_int32), ("lambda_init", C.c_double),
                ("n_points", C.c_int32), ("points", C.c_void_p), ("point_ref", C.c_void_p), ("scw", C.c_void_p)]


class Essg4DofResult(C.Structure):
    _fields_ = [("rcw_out", C.c_void_p), ("tcw_out", C.c_void_p), ("pose_q", C.c_void_p), ("pose_t", C.c_void_p),
                ("points_out", C.c_void_p), ("stats", LbaStats)]


ESSG4DOF_INFORMATION = np.diag([1e3, 1e3, 1.0, 1.0, 1.0, 1.0])      # matLambda of Optimizer::OptimizeEssentialGraph4DoF


def essg4dof_prepare(w):
    """Essg4DofProblem / Essg4DofResult of a graph dictionary (synth_posegraph.make_posegraph4dof) with the arrays they point to"""
    f8 = lambda key, shape: np.ascontiguousarray(w[key], np.float64).reshape(shape)
    k = dict(rcw=f8("rcw", (-1, 9)), tcw=f8("tcw", (-1, 3)), rwb=f8("rwb", (-1, 9)), twb=f8("twb", (-1, 3)), rcb=f8("rcb", (-1, 9)),
             tcb=f8("tcb", (-1, 3)), fixed=np.ascontiguousarray(w["fixed"], np.uint8),
             ev=np.ascontiguousarray(w["edge_vertices"], np.int32).reshape(-1, 2), edge_rot=f8("edge_rot", (-1, 9)),
             edge_trans=f8("edge_trans", (-1, 3)),
             points=np.ascontiguousarray(w.get("points", np.zeros((0, 3))), np.float32).reshape(-1, 3),
             ref=np.ascontiguousarray(w.get("point_ref", np.zeros(0)), np.int32),
             information=np.ascontiguousarray(w.get("information", ESSG4DOF_INFORMATION), np.float64).reshape(36))
    nv, ne, npt = len(k["rcw"]), len(k["ev"]), len(k["points"])
    k["scw"] = np.ascontiguousarray(w["scw"], np.float64).reshape(-1, 8) if npt else np.zeros((0, 8))
    if any(len(k[key]) != nv for key in ("tcw", "rwb", "twb", "rcb", "tcb", "fixed")) or len(k["edge_rot"]) != ne or len(k["edge_trans"]) != ne \
            or len(k["ref"]) != npt or (npt and len(k["scw"]) != nv):
        raise ValueError("4-DoF essential graph arrays of unequal length")
    k.update(rcw_out=np.zeros((nv, 3, 3)), tcw_out=np.zeros((nv, 3)), pose_q=np.zeros((nv, 4), np.float32), pose_t=np.zeros((nv, 3), np.float32),
             points_out=np.zeros((npt, 3), np.float32))
    ptr = lambda key, present=True: k[key].ctypes.data if present else None
    pr = Essg4DofProblem(nv, ptr("rcw"), ptr("tcw"), ptr("rwb"), ptr("twb"), ptr("rcb"), ptr("tcb"), ptr("fixed"),
                         ne, ptr("ev", ne), ptr("edge_rot", ne), ptr("edge_trans", ne), (C.c_double * 36)(*k["information"]),
                         int(w.get("max_iters", 20)), float(w.get("lambda_init", 0.0)), npt, ptr("points", npt), ptr("ref", npt), ptr("scw", npt))
    res = Essg4DofResult(ptr("rcw_out"), ptr("tcw_out"), ptr("pose_q"), ptr("pose_t"), ptr("points_out", npt))
    return dict(problem=pr, result=res, arrays=k)


lib.essg_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
lib.essg_destroy.argtypes = [C.c_void_p]
lib.essg_optimize.argtypes = [C.c_void_p, C.POINTER(EssgProblem), C.POINTER(EssgResult), C.c_void_p]
lib.essg_last_device_ms.argtypes = [C.c_void_p, C.c_void_p]
lib.essg_check.argtypes = [C.POINTER(EssgProblem), C.POINTER(EssgResult)]
lib.essg_last_device_ms.restype = C.c_double
lib.essg_optimize_4dof.argtypes = [C.c_void_p, C.POINTER(Essg4DofProblem), C.POINTER(Essg4DofResult), C.c_void_p]
lib.essg_check_4dof.argtypes = [C.POINTER(Essg4DofProblem), C.POINTER(Essg4DofResult)]


class EssentialGraph:
    """Optimizer::OptimizeEssentialGraph between building the graph and writing the map back (reference src/Optimizer.cc:1729-1779):
    essg_optimize of include/orbslam3_hip.h.  One handle serves one call at a time."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib.essg_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.essg_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optimize(self, w, stop_flag=None):
        prep = essg_prepare(w)
        _check(lib.essg_optimize(self._h, C.byref(prep["problem"]), C.byref(prep["result"]), _p(stop_flag)))
        k = prep["arrays"]
        return dict(sim3_out=k["sim3_out"], pose_q=k["pose_q"], pose_t=k["pose_t"], points_out=k["points_out"],
                    stats=_stats_dict(prep["result"].stats))

    def optimize_4dof(self, pr, stop_flag=None):
        """Optimizer::OptimizeEssentialGraph4DoF between building the graph and writing the map back (reference
        src/Optimizer.cc:5541-5586): essg_optimize_4dof of include/orbslam3_hip.h on this handle"""
        prep = essg4dof_prepare(pr)
        _check(lib.essg_optimize_4dof(self._h, C.byref(prep["problem"]), C.byref(prep["result"]), _p(stop_flag)))
        k = prep["arrays"]
        return dict(rcw_out=k["rcw_out"], tcw_out=k["tcw_out"], pose_q=k["pose_q"], pose_t=k["pose_t"], points_out=k["points_out"],
                    stats=_stats_dict(prep["result"].stats))

    def last_device_ms(self):
        st = (C.c_double * 3)()
        ms = lib.essg_last_device_ms(self._h, st)
        return ms, dict(structure_upload=st[0], rounds=st[1], epilogue_download=st[2])


# ---- IMU initialisation: the three Optimizer::InertialOptimization overloads (include/orbslam3_hip_imu_init.h) ----
IMU_INIT_MAX_KF = 256
IMU_INIT_MAX_BATCH = 64


class ImuInitProblem(C.Structure):
    _fields_ = [("n_kf", C.c_int32), ("Rwb", C.c_void_p), ("twb", C.c_void_p), ("vel", C.c_void_p),
                ("bg", C.c_double * 3), ("ba", C.c_double * 3), ("Rwg", C.c_double * 9), ("scale", C.c_double),
                ("n_links", C.c_int32), ("links", C.c_void_p),
                ("free_vel", C.c_uint8), ("free_bias", C.c_uint8), ("free_gdir", C.c_uint8), ("free_scale", C.c_uint8),
                ("prior_g", C.c_double), ("prior_a", C.c_double), ("huber_delta", C.c_double), ("gauss_newton", C.c_int32),
                ("lambda_init", C.c_double), ("max_iters", C.c_int32)]


class ImuInitResult(C.Structure):
    _fields_ = [("vel_out", C.c_void_p), ("bg_out", C.c_double * 3), ("ba_out", C.c_double * 3), ("Rwg_out", C.c_double * 9),
                ("scale_out", C.c_double), ("chi2_initial", C.c_double), ("chi2_final", C.c_double), ("stats", LbaStats)]


def imu_init_fill(pr, res, w):
    """fills one ImuInitProblem / ImuInitResult from a problem dictionary (synth_imuinit.make_imu_init); returns the arrays they point to"""
    f8 = lambda key, shape: np.ascontiguousarray(w[key], np.float64).reshape(shape)
    k = dict(Rwb=f8("Rwb", (-1, 9)), twb=f8("twb", (-1, 3)), vel=f8("vel", (-1, 3)))
    n = len(k["Rwb"])
    if len(k["twb"]) != n or len(k["vel"]) != n:
        raise ValueError("IMU initialisation arrays of unequal length")
    links = (_LibaLink * max(len(w["links"]), 1))()
    for L, d in zip(links, w["links"]):
        L.kf1, L.kf2, L.dT, L.robust = int(d["kf1"]), int(d["kf2"]), float(d["dT"]), int(d["robust"])
        for name in ("dR", "dV", "dP", "JRg", "JVg", "JVa", "JPg", "JPa", "bias0"):
            getattr(L, name)[:] = np.asarray(d[name], np.float32).ravel().tolist()
        L.info9[:] = np.asarray(d["info9"], np.float64).ravel().tolist()
    k.update(links=links, vel_out=np.zeros((n, 3)))
    pr.n_kf = n
    pr.Rwb, pr.twb, pr.vel = (k[key].ctypes.data if n else None for key in ("Rwb", "twb", "vel"))
    pr.bg[:] = [float(v) for v in w["bg"]]; pr.ba[:] = [float(v) for v in w["ba"]]
    pr.Rwg[:] = np.asarray(w["Rwg"], np.float64).ravel().tolist(); pr.scale = float(w["scale"])
    pr.n_links = len(w["links"]); pr.links = C.addressof(links) if len(w["links"]) else None
    pr.free_vel, pr.free_bias, pr.free_gdir, pr.free_scale = (int(bool(w[key])) for key in ("free_vel", "free_bias", "free_gdir", "free_scale"))
    pr.prior_g, pr.prior_a, pr.huber_delta = float(w.get("prior_g", 0.0)), float(w.get("prior_a", 0.0)), float(w.get("huber_delta", 0.0))
    pr.gauss_newton, pr.lambda_init, pr.max_iters = int(w.get("gauss_newton", 0)), float(w.get("lambda_init", 0.0)), int(w.get("max_iters", 200))
    res.vel_out = k["vel_out"].ctypes.data if n else None
    return k


def imu_init_prepare(problems):
    """arrays of ImuInitProblem / ImuInitResult for a list of problem dictionaries, with everything they point to"""
    n = len(problems)
    prs, ress = (ImuInitProblem * max(n, 1))(), (ImuInitResult * max(n, 1))()
    keep = [imu_init_fill(prs[i], ress[i], w) for i, w in enumerate(problems)]
    return dict(problems=prs, results=ress, arrays=keep, n=n)


def imu_init_results(prep):
    out = []
    for i in range(prep["n"]):
        r = prep["results"][i]
        out.append(dict(vel=prep["arrays"][i]["vel_out"], bg=np.array(r.bg_out[:]), ba=np.array(r.ba_out[:]), Rwg=np.array(r.Rwg_out[:]).reshape(3, 3),
                        scale=r.scale_out, chi2_initial=r.chi2_initial, chi2_final=r.chi2_final, stats=_stats_dict(r.stats)))
    return out


lib.imu_init_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
lib.imu_init_destroy.argtypes = [C.c_void_p]
lib.imu_init_check.argtypes = [C.POINTER(ImuInitProblem), C.POINTER(ImuInitResult)]
lib.imu_init_optimize_batch.argtypes = [C.c_void_p, C.POINTER(ImuInitProblem), C.c_int, C.POINTER(ImuInitResult)]
lib.imu_init_last_device_ms.argtypes = [C.c_void_p]
lib.imu_init_last_device_ms.restype = C.c_double


class ImuInit:
    """The three Optimizer::InertialOptimization overloads (reference src/Optimizer.cc:3042, :3227, :3389) between the walk over
    the map and the write-back: imu_init_optimize_batch of include/orbslam3_hip_imu_init.h.  One handle serves one call at a time."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib.imu_init_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.imu_init_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def optimize_batch(self, problems):
        """one launch for up to IMU_INIT_MAX_BATCH problem dictionaries; a list of result dictionaries"""
        prep = imu_init_prepare(problems)
        _check(lib.imu_init_optimize_batch(self._h, prep["problems"], prep["n"], prep["results"]))
        return imu_init_results(prep)

    def optimize(self, problem):
        return self.optimize_batch([problem])[0]

    def last_device_ms(self):
        return lib.imu_init_last_device_ms(self._h)


FIBA_MAX_UNKNOWNS = 15732
FIBA_MAX_KF = 4096


class FibaProblem(C.Structure):
    _fields_ = list(_LibaProblem._fields_) + [("shared_bias", C.c_uint8), ("shared_bg", C.c_double * 3), ("shared_ba", C.c_double * 3),
                                              ("prior_g", C.c_double), ("prior_a", C.c_double), ("stop_flag", C.c_void_p)]


class FibaOutputs(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in ("Rwb", "twb", "vel", "bg", "ba", "points")]


def fiba_problem(pr, stop_flag=None):
    """a FibaProblem from a problem dictionary (synth_fullba.make_full_map): the keys of a LocalInertialBA window plus shared_bias,
    shared_bg, shared_ba, prior_g, prior_a; stop_flag: a uint8 array of one element, or None"""
    base = _liba_problem(pr)
    s = FibaProblem()
    C.memmove(C.addressof(s), C.addressof(base), C.sizeof(_LibaProblem))
    s.shared_bias = int(bool(pr.get("shared_bias", 0)))
    s.shared_bg[:] = [float(v) for v in pr.get("shared_bg", (0, 0, 0))]; s.shared_ba[:] = [float(v) for v in pr.get("shared_ba", (0, 0, 0))]
    s.prior_g, s.prior_a = float(pr.get("prior_g", 0.0)), float(pr.get("prior_a", 0.0))
    s.stop_flag = None if stop_flag is None else stop_flag.ctypes.data
    s._keep = (base, stop_flag)
    return s


class FullInertialBA:
    """The numerical core of Optimizer::FullInertialBA (reference src/Optimizer.cc:392-811) on the device: fiba_solve of
    include/orbslam3_hip_fullba.h.  One handle serves one call at a time."""

    def __init__(self, device=0):
        lib.fiba_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
        lib.fiba_destroy.argtypes = [C.c_void_p]
        lib.fiba_solve.argtypes = [C.c_void_p, C.POINTER(FibaProblem), C.POINTER(FibaOutputs), C.POINTER(LbaStats)]
        lib.fiba_check.argtypes = [C.POINTER(FibaProblem)]
        lib.fiba_last_device_ms.argtypes = [C.c_void_p]
        lib.fiba_last_device_ms.restype = C.c_double
        h = C.c_void_p()
        _check(lib.fiba_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.fiba_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, pr, stop_flag=None):
        s = fiba_problem(pr, stop_flag)
        n, m = s.n_kf, s.n_points
        out = dict(Rwb=np.zeros((n, 3, 3)), twb=np.zeros((n, 3)), vel=np.zeros((n, 3)), bg=np.zeros((n, 3)), ba=np.zeros((n, 3)), points=np.zeros((max(m, 1), 3)))
        o = FibaOutputs(*[out[k].ctypes.data for k in ("Rwb", "twb", "vel", "bg", "ba", "points")])
        st = LbaStats()
        _check(lib.fiba_solve(self._h, C.byref(s), C.byref(o), C.byref(st)))
        out["points"] = out["points"][:m]
        out["stats"] = _stats_dict(st)
        return out

    def last_device_ms(self):
        return lib.fiba_last_device_ms(self._h)


# ---- IMU pre-integration on the device (include/orbslam3_hip_imu_preint.h) ----
class ImuMeasurement(C.Structure):
    _fields_ = [("a", C.c_float * 3), ("w", C.c_float * 3), ("dt", C.c_float)]


class ImuPreintState(C.Structure):
    _fields_ = [("dT", C.c_float), ("b", C.c_float * 6), ("bu", C.c_float * 6), ("nga", C.c_float * 6), ("nga_walk", C.c_float * 6),
                ("dR", C.c_float * 9), ("dV", C.c_float * 3), ("dP", C.c_float * 3), ("JRg", C.c_float * 9), ("JVg", C.c_float * 9),
                ("JVa", C.c_float * 9), ("JPg", C.c_float * 9), ("JPa", C.c_float * 9), ("avgA", C.c_float * 3), ("avgW", C.c_float * 3),
                ("C", C.c_float * 225), ("n_meas", C.c_int32)]


class ImuPreintJob(C.Structure):
    _fields_ = [("state", C.c_int32), ("first", C.c_int32), ("count", C.c_int32), ("reset", C.c_uint8), ("bias", C.c_float * 6)]


class ImuLinkSpec(C.Structure):
    _fields_ = [("state", C.c_int32), ("walk_state", C.c_int32), ("kf1", C.c_int32), ("kf2", C.c_int32), ("info_scale", C.c_double),
                ("robust", C.c_uint8)]


class ImuPredictJob(C.Structure):
    _fields_ = [("state", C.c_int32), ("Rwb1", C.c_float * 9), ("twb1", C.c_float * 3), ("Vwb1", C.c_float * 3), ("bias", C.c_float * 6)]


class ImuPredictOut(C.Structure):
    _fields_ = [("Rwb2", C.c_float * 9), ("twb2", C.c_float * 3), ("Vwb2", C.c_float * 3)]


def _np_dtype(cls, shapes=None):
    """the numpy record of a ctypes struct: same offsets, same size"""
    names, formats, offsets = [], [], []
    for name, ct in cls._fields_:
        names.append(name); offsets.append(getattr(cls, name).offset)
        if hasattr(ct, "_length_"):
            n = ct._length_
            shape = (shapes or {}).get(name, (n,))
            formats.append((np.dtype(ct._type_), shape))
        else:
            formats.append(np.dtype(ct))
    return np.dtype(dict(names=names, formats=formats, offsets=offsets, itemsize=C.sizeof(cls)))


_M33 = {k: (3, 3) for k in ("dR", "JRg", "JVg", "JVa", "JPg", "JPa", "Rwb1", "Rwb2")}
IMU_MEAS_DTYPE = _np_dtype(ImuMeasurement)
IMU_STATE_DTYPE = _np_dtype(ImuPreintState, dict(_M33, C=(15, 15)))
IMU_JOB_DTYPE = _np_dtype(ImuPreintJob)
IMU_LINK_SPEC_DTYPE = _np_dtype(ImuLinkSpec)
IMU_PREDICT_JOB_DTYPE = _np_dtype(ImuPredictJob, _M33)
IMU_PREDICT_OUT_DTYPE = _np_dtype(ImuPredictOut, _M33)
LIBA_LINK_DTYPE = _np_dtype(_LibaLink, dict(_M33, info9=(9, 9), info_gyro=(3, 3), info_acc=(3, 3)))

lib.imu_preint_create.argtypes = [C.c_int, C.POINTER(C.c_void_p)]
lib.imu_preint_destroy.argtypes = [C.c_void_p]
lib.imu_preint_last_device_ms.argtypes = [C.c_void_p]
lib.imu_preint_last_device_ms.restype = C.c_double
lib.imu_preint_check.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
lib.imu_preintegrate_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p]
lib.imu_preintegrate_batch_device.argtypes = lib.imu_preintegrate_batch.argtypes + [C.c_void_p]
lib.imu_frame_measurements_batch.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p]
lib.imu_frame_measurements_batch_device.argtypes = lib.imu_frame_measurements_batch.argtypes + [C.c_void_p]
lib.imu_links_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
lib.imu_links_batch_device.argtypes = lib.imu_links_batch.argtypes + [C.c_void_p]
lib.imu_predict_state_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
lib.imu_predict_state_batch_device.argtypes = lib.imu_predict_state_batch.argtypes + [C.c_void_p]


def imu_state_new(n, nga, nga_walk):
    """n states as Preintegrated(Bias(), calib) leaves them: Initialize(0), nga / nga_walk = the diagonals of Calib::Cov / CovWalk"""
    s = np.zeros(n, IMU_STATE_DTYPE)
    s["nga"] = np.asarray(nga, np.float32); s["nga_walk"] = np.asarray(nga_walk, np.float32)
    s["dR"] = np.eye(3, dtype=np.float32)
    return s


def imu_preint_check(states, jobs, meas):
    """the host-only argument checks of imu_preintegrate_batch: the ORBX code"""
    return lib.imu_preint_check(_p(states), len(states), _p(jobs), len(jobs), _p(meas), len(meas))


class ImuPreintegrator:
    """IMU::Preintegrated on the device (include/orbslam3_hip_imu_preint.h): Initialize / IntegrateNewMeasurement batched over states,
    the interpolation loop of Tracking::PreintegrateIMU, the LibaLink of a state and Tracking::PredictStateIMU.  The host entries
    take numpy records (IMU_STATE_DTYPE, IMU_JOB_DTYPE, ...); the *_device entries take device addresses (int) and only enqueue.
    One handle serves one call at a time."""

    def __init__(self, device=0):
        h = C.c_void_p()
        _check(lib.imu_preint_create(device, C.byref(h)))
        self._h = h

    def close(self):
        if getattr(self, "_h", None):
            lib.imu_preint_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def preintegrate(self, states, jobs, meas):
        """states is updated in place; returns the per-job status"""
        assert states.dtype == IMU_STATE_DTYPE and states.flags.c_contiguous
        jobs = np.ascontiguousarray(jobs, IMU_JOB_DTYPE); meas = np.ascontiguousarray(meas, IMU_MEAS_DTYPE)
        st = np.zeros(len(jobs), np.int32)
        _check(lib.imu_preintegrate_batch(self._h, _p(states), len(states), _p(jobs), len(jobs), _p(meas), len(meas), _p(st)))
        return st

    def preintegrate_device(self, d_states, n_states, d_jobs, n_jobs, d_meas, n_meas, d_status, stream=None):
        _check(lib.imu_preintegrate_batch_device(self._h, C.c_void_p(d_states), int(n_states), C.c_void_p(d_jobs), int(n_jobs), C.c_void_p(d_meas or 0),
                                                 int(n_meas), C.c_void_p(d_status), C.c_void_p(stream or 0)))

    def frame_measurements(self, samples, n_imu, t_prev_ns, t_cur_ns):
        """samples [B][imu_cap] IMU_DTYPE; returns (meas [B][imu_cap] IMU_MEAS_DTYPE, count [B])"""
        samples = np.ascontiguousarray(samples, IMU_DTYPE)
        B, cap = samples.shape
        n_imu = np.ascontiguousarray(n_imu, np.int32); tp = np.ascontiguousarray(t_prev_ns, np.int64); tc = np.ascontiguousarray(t_cur_ns, np.int64)
        assert n_imu.shape == tp.shape == tc.shape == (B,)
        meas = np.zeros((B, cap), IMU_MEAS_DTYPE); cnt = np.zeros(B, np.int32)
        _check(lib.imu_frame_measurements_batch(self._h, _p(samples), _p(n_imu), _p(tp), _p(tc), B, cap, _p(meas), _p(cnt)))
        return meas, cnt

    def frame_measurements_device(self, d_samples, d_n_imu, d_t_prev_ns, d_t_cur_ns, batch, imu_cap, d_meas_out, d_count_out, stream=None):
        _check(lib.imu_frame_measurements_batch_device(self._h, C.c_void_p(d_samples), C.c_void_p(d_n_imu), C.c_void_p(d_t_prev_ns), C.c_void_p(d_t_cur_ns),
                                                       int(batch), int(imu_cap), C.c_void_p(d_meas_out), C.c_void_p(d_count_out), C.c_void_p(stream or 0)))

    def links(self, states, specs):
        """returns (links LIBA_LINK_DTYPE [n], status [n])"""
        assert states.dtype == IMU_STATE_DTYPE and states.flags.c_contiguous
        specs = np.ascontiguousarray(specs, IMU_LINK_SPEC_DTYPE)
        out = np.zeros(len(specs), LIBA_LINK_DTYPE); st = np.zeros(len(specs), np.int32)
        _check(lib.imu_links_batch(self._h, _p(states), len(states), _p(specs), len(specs), _p(out), _p(st)))
        return out, st

    def links_device(self, d_states, n_states, d_specs, n_links, d_links_out, d_status, stream=None):
        _check(lib.imu_links_batch_device(self._h, C.c_void_p(d_states), int(n_states), C.c_void_p(d_specs), int(n_links), C.c_void_p(d_links_out),
                                          C.c_void_p(d_status), C.c_void_p(stream or 0)))

    def predict(self, states, jobs):
        """returns (out IMU_PREDICT_OUT_DTYPE [n], status [n])"""
        assert states.dtype == IMU_STATE_DTYPE and states.flags.c_contiguous
        jobs = np.ascontiguousarray(jobs, IMU_PREDICT_JOB_DTYPE)
        out = np.zeros(len(jobs), IMU_PREDICT_OUT_DTYPE); st = np.zeros(len(jobs), np.int32)
        _check(lib.imu_predict_state_batch(self._h, _p(states), len(states), _p(jobs), len(jobs), _p(out), _p(st)))
        return out, st

    def predict_device(self, d_states, n_states, d_jobs, n_jobs, d_out, d_status, stream=None):
        _check(lib.imu_predict_state_batch_device(self._h, C.c_void_p(d_states), int(n_states), C.c_void_p(d_jobs), int(n_jobs), C.c_void_p(d_out),
                                                  C.c_void_p(d_status), C.c_void_p(stream or 0)))

    def last_device_ms(self):
        return lib.imu_preint_last_device_ms(self._h)
