/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- void LocalMapping::CreateNewMapPoints() for two-camera fisheye rigs (Nleft != -1, mpCamera2 != NULL) in one call ----
 * src/LocalMapping.cc:392-716 with both key frames rigs: orbm_create_new_map_points (conventional cameras) and
 * orbm_search_for_triangulation_rig (a rig's search alone) fused.  Feature indices run over the concatenated arrays of a rig, as in
 * orbslam3_hip_rig_bow.h: the left features first, right feature j at n_left + j; key points are the raw mvKeys / mvKeysRight.
 *
 * What the reference does, and this call restates:
 *  Per neighbour in order: SearchForTriangulation(kf1, neighbour, bOnlyStereo = false, coarse) with ORBmatcher(0.6, false) (no
 *   rotation histogram) exactly as orbm_search_for_triangulation_rig, with the map points created so far visible as has_mp of key
 *   frame 1; then the matches in ascending idx1 (src/ORBmatcher.cc:1138-1143).
 *  The baseline test is INSIDE the call, because it carries state.  A rig is a stereo sensor, so the test is
 *   `if(baseline < pKF2->mb) continue;` with baseline = (Ow2 - Ow1).norm() (:447-455).  Ow2 is the neighbour's LEFT centre, fresh
 *   per neighbour (:448).  Ow1 is declared OUTSIDE the neighbour loop (:423) and overwritten per match (:512/522/532/542): from the
 *   second neighbour on it is the centre of the side of the LAST match -- the one with the highest idx1, whether or not it passed
 *   the later gates -- of the most recent neighbour that had a match: the right-camera centre iff that idx1 >= n_left.  It is the
 *   left centre before any match; skipped or matchless neighbours leave it alone.  The two centres are mb apart, so the two
 *   readings can disagree.  The caller cannot decide this before the call; `skipped` reports what was decided.
 *  Per match (:509-559): (bRight1, bRight2) select pose, centre and camera of each side.  bStereo1 = bStereo2 = false (mpCamera2
 *   is set): no UnprojectStereo, no 7.8 gate, point_stereo is written 0.  mvuRight[idx] (read past the end of an NLeft-long array
 *   for a right index, never used) is not read.
 *  Geometry: KannalaBrandt8::unprojectEig of the side's camera, the parallax cosine (bound 0.9996 with inertial, else 0.9998),
 *   GeometricTools::Triangulate on the two sides' world poses (null vector in double), z1 > 0, z2 > 0, the monocular 5.991 gate on
 *   both sides through KannalaBrandt8::project, dist1 / dist2 from the SIDES' centres, far-point and scale-consistency gates.
 *  MapPoint::UpdateNormalAndDepth of the new point (src/MapPoint.cc:426-494): the normal is the mean of the two unit vectors from
 *   the centres of the observing sides; the distance is taken from key frame 1's LEFT centre, also for a right observation (:468);
 *   the level is the octave of feature idx1.
 * Stays with the caller, as for orbm_create_new_map_points: CheckNewKeyFrames() (:440) once before the call, and the pointer
 * surgery (:698-713) in (neighbour, idx1) ascending order.
 *
 * OrbmRigMapKeyFrame: side = desc, has_mp, x, y, octave, fv over the concatenated arrays (`stereo` and `angle` are not read and may
 * be NULL); index 0 of Rcw / tcw / Ow is GetPose() / GetCameraCenter(), index 1 GetRightPose() / GetRightCameraCenter() (Rcw row
 * major); cam[0] / cam[1] = mpCamera / mpCamera2 as fx fy cx cy k0..k3 precision (the layout of OrbmRigTriGeometry::cam).
 * OrbmRigMapPair (one per neighbour): geom = the search's four relative poses and camera pairs of (kf1, neighbour), computed by the
 * caller as for orbm_search_for_triangulation_rig; coarse.  OrbmMapParams and OrbmNewPoints as orbm_create_new_map_points defines
 * them; the device keeps one launch unless a neighbour's baseline test differs between the two centres of key frame 1, where the
 * call is cut before that neighbour and only the counters of the segment are read back. */
typedef struct OrbmRigMapKeyFrame {
    OrbmTriSide side;
    int32_t n_left;
    float Rcw[2][9]; float tcw[2][3]; float Ow[2][3];
    float cam[2][9];
    float mb;
    const float* level_sigma2; const float* scale_factors; int32_t n_levels;
} OrbmRigMapKeyFrame;
typedef struct OrbmRigMapPair {
    const OrbmRigTriGeometry* geom;
    int32_t coarse;
} OrbmRigMapPair;

/* The argument checks alone (host only, no device needed); every call runs them first.  ORBX_OK, or ORBX_ERR_ARG for: a NULL
 * kf1, params or out; n_neighbours outside [0, ORBM_MAX_NEIGHBOURS]; NULL neighbours / pairs / out->n_matched / out->n_created
 * with n_neighbours > 0; a NULL geom; and for every key frame: a NULL array where its count is positive, a negative count, n_left
 * outside [0, n], n_levels outside [1, 32], NULL level tables, an octave outside [0, n_levels), mb NaN or negative, a feature
 * vector with a negative node count, node ids not strictly ascending, offsets that do not start at 0 or are not monotone, a
 * feature index >= n or a node of more than 65 535 features; a feature of key frame 1 in two nodes; NULL per-feature outputs
 * with features in key frame 1; normal / max_dist / min_dist not given together. */
int orbm_create_new_map_points_rig_check(const OrbmRigMapKeyFrame* kf1, const OrbmRigMapKeyFrame* neighbours, int n_neighbours,
                                         const OrbmRigMapPair* pairs, const OrbmMapParams* params, const OrbmNewPoints* out);

/* Returns the number of points created, or ORBX_ERR_ARG (the handle stays usable) / ORBX_ERR_NO_DEVICE / ORBX_ERR_HIP.
 * skipped[n_neighbours] (may be NULL): 1 where the baseline test skipped the neighbour. */
int orbm_create_new_map_points_rig(orbm_matcher* m, const OrbmRigMapKeyFrame* kf1, const OrbmRigMapKeyFrame* neighbours, int n_neighbours,
                                   const OrbmRigMapPair* pairs, const OrbmMapParams* params, OrbmNewPoints* out, uint8_t* skipped);

/* device time of the launches of the last orbm_create_new_map_points_rig on this handle (HIP events; 0 before the first) */
float orbm_create_new_map_points_rig_last_kernel_ms(const orbm_matcher* m);
/* the number of launches that call took (1 unless a neighbour's baseline test was ambiguous; 0 when there was nothing to do) */
int orbm_create_new_map_points_rig_last_launches(const orbm_matcher* m);
