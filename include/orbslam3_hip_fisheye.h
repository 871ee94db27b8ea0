/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- void Frame::ComputeStereoFishEyeMatches() (src/Frame.cc:1246-1286): stereo for a two-camera fisheye rig ----
 * A rig frame (Nleft != -1, two KannalaBrandt8 cameras: every TUM-VI stereo sequence) matches the left key points of the lapping
 * area against the right ones and triangulates the pairs that pass:
 *   1. BFmatcher.knnMatch(left[mono_l:], right[mono_r:], 2), NORM_HAMMING: for every lapping left descriptor the smallest and the
 *      second smallest distance over all lapping right descriptors.  It passes when there are at least two right descriptors
 *      and (double)(float)d0 < (double)(float)d1 * 0.7 (:1271).  Two equally good right descriptors give d0 == d1: no match.
 *   2. KannalaBrandt8::TriangulateMatches (src/CameraModels/KannalaBrandt8.cpp:306-375) of the pair: -1 low parallax
 *      (cos > 0.9998), -2 / -3 behind the left / right camera, -4 / -5 reprojection error^2 above 5.991 * level sigma^2 of the
 *      left / right key point, else the depth z1 in the left camera.
 *   3. where depth > 0.0001f: mvLeftToRightMatch, mvRightToLeftMatch, mvDepth, mvStereo3Dpoints.  Several left key points may be
 *      accepted onto one right key point; mvRightToLeftMatch then holds the HIGHEST left index, which is what the reference's
 *      loop leaves behind.  mvuRight stays -1 everywhere and is the caller's to fill.
 * Indices are those of the whole arrays (mono_l / mono_r already added).  Entries the reference leaves unset are -1 (matches),
 * -1.0 (depth) and zeros (p3d).  The geometry follows the reference's float operation order (csrc/kb8_stereo_geometry.h says
 * where it cannot: one-ulp transcendentals and the null vector); DESIGN.md 4i gives the measured spread.
 * Two calls with the same inputs return the same bits.
 *
 * A handle serves ONE call at a time: the host entry packs into the handle's pinned buffer and runs on the handle's stream, the
 * device entry enqueues on the caller's stream and must not overlap another call on the same handle from another thread or
 * stream.  Use one orbm_matcher per stream. */
typedef struct OrbxFisheyeRig {
    OrbxKB8 left, right;               /* mpCamera, mpCamera2: mvParameters[0..7], floats promoted to double */
    float precision_l, precision_r;    /* KannalaBrandt8::precision (1e-6 by default) */
    float Rlr[9];                      /* mRlr, row major */
    float tlr[3];                      /* mtlr */
} OrbxFisheyeRig;

/* right key points the k-NN kernel stages per pass (tests put lapping counts on both sides of it) */
#define ORBM_FISHEYE_KNN_CHUNK 128

/* The argument checks alone (host only, no device needed): ORBX_OK or ORBX_ERR_ARG for a negative count, mono > n, a NULL
 * array of a non-empty side, n_levels outside [1, 32], a NULL level_sigma2 or rig, an octave outside [0, n_levels), fx or fy <= 0
 * and precision <= 0 (NaN included).  Both entries below call it before touching a device; the handle stays usable. */
int orbm_stereo_fisheye_check(const OrbxKeyPoint* kps_l, const uint8_t* desc_l, int n_l, int mono_l,
                              const OrbxKeyPoint* kps_r, const uint8_t* desc_r, int n_r, int mono_r,
                              const float* level_sigma2, int n_levels, const OrbxFisheyeRig* rig);

/* Host buffers.  kps_l / desc_l = mvKeys / mDescriptors (n_l = Nleft, mono_l = monoLeft), likewise the right side; level_sigma2 =
 * mvLevelSigma2 of the LEFT extractor, used for both octaves (:1275).  Any output may be NULL.  knn_right / knn_d0 / knn_d1 are
 * exact diagnostics of step 1: the right index of a left key point that passed the ratio test (else -1), and its two distances
 * (-1 where there was no first / second neighbour or the key point is outside the lapping area).
 * Returns the number of matches (nMatches of the reference), or < 0. */
int orbm_stereo_fisheye(orbm_matcher* m,
                        const OrbxKeyPoint* kps_l, const uint8_t* desc_l, int n_l, int mono_l,
                        const OrbxKeyPoint* kps_r, const uint8_t* desc_r, int n_r, int mono_r,
                        const float* level_sigma2, int n_levels, const OrbxFisheyeRig* rig,
                        int32_t* left_to_right /*[n_l]*/, int32_t* right_to_left /*[n_r]*/, float* depth /*[n_l]*/, float* p3d /*[n_l][3]*/,
                        int32_t* knn_right /*[n_l]*/, int32_t* knn_d0 /*[n_l]*/, int32_t* knn_d1 /*[n_l]*/);
/* device time of the two kernels of the LAST orbm_stereo_fisheye call on this handle (HIP events), milliseconds */
float orbm_stereo_fisheye_last_kernel_ms(const orbm_matcher* m);

/* Device-resident batch: the [batch][cap] outputs of orbx_extract_batch_device of both extractors with d_n and d_mono per frame
 * (DEVICE pointers, descriptors 16-byte aligned); the four outputs are [batch][cap] device arrays and required, the three
 * diagnostics may be NULL.  Frame b writes entries [0, n) of its rows and leaves the rest untouched, and equals the host entry on
 * frame b bit for bit.  A count outside [0, cap] is clamped, an octave outside the table reads its nearest entry.  Only
 * enqueues on `stream` (a hipStream_t, NULL = default stream). */
int orbm_stereo_fisheye_batch_device(orbm_matcher* m, int batch, int cap,
                                     const OrbxKeyPoint* d_kps_l, const uint8_t* d_desc_l, const int32_t* d_n_l, const int32_t* d_mono_l,
                                     const OrbxKeyPoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_n_r, const int32_t* d_mono_r,
                                     const float* level_sigma2 /*host*/, int n_levels, const OrbxFisheyeRig* rig,
                                     int32_t* d_left_to_right, int32_t* d_right_to_left, float* d_depth, float* d_p3d,
                                     int32_t* d_knn_right, int32_t* d_knn_d0, int32_t* d_knn_d1, void* stream);

/* diagnostic, in the spirit of orbx_kb8_project: TriangulateMatches of n given pixel pairs with the device function the
 * entries above use.  pts_l / pts_r [n][2], sigma_l / sigma_r [n] (level sigma^2).  code_or_depth[n] receives -1 .. -5 or z1,
 * p3d[n][3] the point of an accepted pair (zeros otherwise). */
int orbx_kb8_triangulate_matches(int device, const OrbxFisheyeRig* rig, const float* pts_l, const float* pts_r,
                                 const float* sigma_l, const float* sigma_r, int n, float* code_or_depth, float* p3d);
