/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- the vocabulary-guided searches of ORBmatcher for two-camera fisheye rigs (Nleft != -1, mpCamera2 != NULL) ----
 *   int ORBmatcher::SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches), F.Nleft != -1
 *       (src/ORBmatcher.cc:223-425, the `else` branches at :296-323 and :357-386 that orbm_search_by_bow leaves out), and
 *   int ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, ..., bOnlyStereo, bCoarse), both key frames rigs (:907-1146).
 * Feature indices on every side run over the concatenated arrays of a rig: the left features first, right feature j at Nleft + j.
 * mDescriptors is stored that way (src/Frame.cc:1233) and the feature vectors index it, so a feature sits in exactly one
 * vocabulary node and nodes do not interact.  Angles, positions and octaves are those of mvKeys followed by mvKeysRight.
 *
 * What the reference does, and these calls restate (integer-equal to the sequential loops):
 *  SearchByBoW, per common node, per valid key-frame feature in order: the frame features of the node are visited in order, slots
 *   already written are skipped (:299), and TWO (best, second, index) triples are kept -- one over candidates < n_left_f, one over
 *   candidates >= n_left_f.  Everything then sits inside `if(bestDist1 <= TH_LOW)` (:327) on the LEFT best: with no live left
 *   candidate in the node (none at all, or all consumed: bestDist1 stays 256), or a left best of 51 or more, nothing is written --
 *   a right candidate at distance 0 included.  Inside it the left slot is written when (float)best1 < nnratio * (float)best2
 *   (:329), and, independently of that ratio test, the right slot is written when bestDist1R <= TH_LOW: its own ratio test is
 *   `|| true` (:359), so the first of equally near right candidates is taken.  The return value counts both writes.  A slot
 *   written on either side is invisible to the later key-frame features of the node; the sides consume independently.
 *   check_orientation: ONE histogram over both sides (:404-422) logs every written slot once, with rot_bin(angle_kf[kf feature],
 *   angle_f[slot]); a slot outside the three kept bins is cleared and takes one off the count.
 *  SearchForTriangulation: bStereo1 / bStereo2 are false for rig key frames (:979, :1007), so only_stereo yields 0 matches and the
 *   epipole-distance test (:1026-1034, `!pKF1->mpCamera2`) never runs: a candidate at the epipole matches like any other.
 *   (bRight1, bRight2) select one of four relative poses and camera pairs (:1036-1070): ll, lr, rl, rr.  The gate is
 *   KannalaBrandt8::epipolarConstrain = TriangulateMatches(pCamera2, kp1, kp2, R12, t12, mvLevelSigma2_1[kp1.octave],
 *   mvLevelSigma2_2[kp2.octave], p3D) > 0.0001f (KannalaBrandt8.cpp:216-220), skipped when coarse.  vbMatched2 is never written,
 *   so key-frame-1 features do not interact, and the candidate loop (:997-1077) is an order-free set function: among the
 *   candidates without a map point, with dist <= TH_LOW and a passing gate, the winner has the smallest dist, and among equal
 *   distances it is the LAST in node order (a later candidate with dist <= bestDist replaces the holder; a failing candidate
 *   changes nothing).  check_orientation: one histogram over all key-frame-1 features (:1114-1133).
 *
 * A handle serves one call at a time (see orbslam3_hip_fisheye.h): use one orbm_matcher per stream. */
typedef struct OrbmBowRigPair {
    const uint8_t* desc_kf; int32_t n_kf; const uint8_t* valid_kf; const float* angle_kf; OrbmFeatVec fv_kf;   /* as OrbmBowPair; a rig key frame's angles concatenated */
    const uint8_t* desc_f;  int32_t n_f;  int32_t n_left_f;        /* F.Nleft: slots [0, n_left_f) are the left camera's */
    const float* angle_f;   OrbmFeatVec fv_f;
    int32_t* match_f2kf;    /* out [n_f] */
    int32_t n_matches;      /* out */
} OrbmBowRigPair;

/* the cameras and relative poses of a rig key-frame pair.  cam: key frame 1 left, key frame 1 right, key frame 2 left, key
 * frame 2 right, each fx fy cx cy k0..k3 precision.  R12 (row major) / t12 in the order ll, lr, rl, rr: rotationMatrix() and
 * translation() of T1w*Tw2, T1w*Twr2, Tr1w*Tw2, Tr1w*Twr2, computed by the caller with the reference's float expressions. */
typedef struct OrbmRigTriGeometry {
    float cam[4][9];
    float R12[4][9];
    float t12[4][3];
} OrbmRigTriGeometry;

/* one (key frame 1, key frame 2) pair.  kf1 / kf2: x, y, octave, angle of mvKeys then mvKeysRight, has_mp[i] = GetMapPoint(i) !=
 * NULL, desc = mDescriptors, fv = mFeatVec; `stereo` is not read and may be NULL; angle may be NULL without orientation checking. */
typedef struct OrbmRigTriPair {
    const OrbmTriSide* kf1; int32_t n_left_1;
    const OrbmTriSide* kf2; int32_t n_left_2;
    const OrbmRigTriGeometry* geom;
    const float* level_sigma2_1; const float* level_sigma2_2; int32_t n_levels;     /* mvLevelSigma2 of the two key frames */
    int32_t* match12;       /* out [kf1->n]: key-frame-2 feature or -1 */
    int32_t n_matches;      /* out */
} OrbmRigTriPair;

/* The argument checks alone (host only, no device needed).  Exactly one of bow / tri is given.  ORBX_OK, or ORBX_ERR_ARG for:
 * a NULL array where its count is positive (angle_* / angle alone may be NULL when check_orientation is 0; `stereo` always); a
 * NULL kf1, kf2, geom, level_sigma2_* ; a negative count; n_left outside [0, n]; n_levels outside [1, 32]; an octave outside [0,
 * n_levels); a feature vector with a negative node count, node ids not strictly ascending, offsets that do not start at 0 or are
 * not monotone, a feature index >= n, or a node of more than 65 535 features (the position field of the kernels' keys); for tri,
 * a feature of key frame 1 that appears in two nodes (key frame 2's may).  Every entry below calls it first, for every pair. */
int orbm_rig_bow_check(const OrbmBowRigPair* bow, const OrbmRigTriPair* tri, int check_orientation);

/* SearchByBoW(KeyFrame*, Frame&, ...), F.Nleft != -1.  match_f2kf[n_f] and the return value as orbm_search_by_bow. */
int orbm_search_by_bow_rig(orbm_matcher* m,
                           const uint8_t* desc_kf, int n_kf, const uint8_t* valid_kf, const float* angle_kf, const OrbmFeatVec* fv_kf,
                           const uint8_t* desc_f, int n_f, int n_left_f, const float* angle_f, const OrbmFeatVec* fv_f,
                           float nnratio, int check_orientation, int32_t* match_f2kf);
/* n_pairs independent pairs in ONE launch, a workgroup per pair */
int orbm_search_by_bow_rig_batch(orbm_matcher* m, OrbmBowRigPair* pairs, int n_pairs, float nnratio, int check_orientation);

/* SearchForTriangulation(pKF1, pKF2, ...), both rigs.  only_stereo != 0: 0 matches, match12 all -1, no launch.  Returns nmatches. */
int orbm_search_for_triangulation_rig(orbm_matcher* m, const OrbmTriSide* kf1, int n_left_1, const OrbmTriSide* kf2, int n_left_2,
                                      const OrbmRigTriGeometry* geom, const float* level_sigma2_1, const float* level_sigma2_2, int n_levels,
                                      int only_stereo, int coarse, int check_orientation, int32_t* match12);
/* n_pairs pairs in ONE search launch (one key frame against its neighbours: has_mp is per pair); n_matches is written per pair */
int orbm_search_for_triangulation_rig_batch(orbm_matcher* m, OrbmRigTriPair* pairs, int n_pairs, int only_stereo, int coarse, int check_orientation);

/* device time of the kernels of the LAST of these searches on this handle (HIP events), milliseconds */
float orbm_rig_bow_last_kernel_ms(const orbm_matcher* m);
