/* Part of the C ABI of orbslam3_hip.h, which includes this file at its end: include that header, not this one.
 *
 * ---- the two tracking searches of ORBmatcher for a two-camera fisheye rig frame (Nleft != -1) ----
 *   int ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th, bFarPoints, thFarPoints)
 *       (src/ORBmatcher.cc:43-213, the branches orbm_search_by_projection leaves out), and
 *   int ORBmatcher::SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono) (:1676-1887).
 * A rig frame has two key-point lists (mvKeys[0..Nleft), mvKeysRight[0..Nright), neither undistorted), two grids (mGrid,
 * mGridRight) and ONE slot array mvpMapPoints[0 .. Nleft+Nright): left slots first, right slot j at Nleft + j.
 * assign / occupied are in/out arrays of left.n + right.n entries in that slot order, with the meaning they have in
 * orbm_search_by_projection(_last): assign[slot] = index of the point the slot now holds (untouched where the call assigned
 * nothing; in the last-frame search -1 marks a slot the rotation check nulled), occupied[slot] = mvpMapPoints[slot] &&
 * Observations() > 0.  A match by point i writes occupied[slot] = has_obs[i].
 *
 * What the reference does, and these calls restate (integer-equal to the sequential loop):
 *  map points, per point in order: skipped when neither in_view nor in_view_r, when far_points && track_depth > th_far, when bad.
 *   Left pass (in_view): radius RadiusByViewingCos(view_cos) (* th when th != 1) * scale[pred_level], levels pred_level-1 ..
 *   pred_level on the left grid, occupied left slots skipped, no u_right gate.  best <= TH_HIGH and both on one level and
 *   best > nnratio * second: `continue` (:125-126) -- the RIGHT pass of the point is cancelled with it.  Otherwise, best <=
 *   TH_HIGH: the left slot is written, and when left_to_right[best] != -1 the partner slot left.n + l2r too, unconditionally
 *   (:131-135).  An empty left window does not cancel the right pass.  Right pass (in_view_r and pred_level_r != -1):
 *   radius RadiusByViewingCos(view_cos_r) * scale[pred_level_r] -- th is NOT applied (:147) --, right grid, slot left.n + idx
 *   decides occupancy (the partner slot the left pass of this very point wrote included), octaves of the right key points;
 *   on a match the slot right_to_left[best] (when != -1) is written first, then left.n + best (:198-207).  The return value
 *   counts WRITES: a slot written twice counts twice.
 *  last frame, per entry in order: skipped when !valid, when the LEFT projection is outside [min_x, max_x] x [min_y, max_y],
 *   and when the left window is empty (:1735; empty by cells, levels and |dx|,|dy| < r -- not by occupancy); each of these
 *   cancels the right pass too.  Radius th * scale[octave], levels by level_window (ORBM_LEVELS_*).  Left best <= TH_HIGH:
 *   slot written, logged with rot_bin(angle[i], left.angle[best]).  The right pass then always runs: NO image-bounds test on
 *   proj_u_r / proj_v_r, same radius and levels on the right grid, occupancy of slot left.n + idx, logged with right.angle.
 *   check_orientation: ONE histogram over both sides (:1865-1884); every logged slot outside the three kept bins gets
 *   assign = -1, occupied = 0 and takes one off the count.
 * Ties between equal distances go to the first candidate in the reference's visiting order (grid columns outer, rows inner,
 * insertion order in a cell).
 *
 * A handle serves one call at a time (see orbslam3_hip_fisheye.h): use one orbm_matcher per stream. */
typedef struct OrbmRigFrame {
    OrbmFrame left;    /* mvKeys[0..Nleft): x, y, octave, angle of the RAW key points; desc = mDescriptors rows [0, Nleft); u_right must be NULL */
    OrbmFrame right;   /* mvKeysRight[0..Nright); desc = mDescriptors rows [Nleft, Nleft+Nright) */
    const int32_t* left_to_right;   /* mvLeftToRightMatch, [left.n], -1 = none, else an index into right */
    const int32_t* right_to_left;   /* mvRightToLeftMatch, [right.n] */
} OrbmRigFrame;

/* the map points of SearchByProjection(Frame&, vector<MapPoint*>&, ...): per point the left mbTrackInView, mTrackProjX/Y,
 * mnTrackScaleLevel, mTrackViewCos, the ...R members of the right camera, mTrackDepth, isBad(), Observations() > 0 and
 * GetDescriptor().  pred_level_r may be -1: the reference's "no level" (:146), which skips the right pass of that point. */
typedef struct OrbmRigMapPoints {
    int32_t n;
    const uint8_t* in_view; const float* proj_u; const float* proj_v; const int32_t* pred_level; const float* view_cos;
    const uint8_t* in_view_r; const float* proj_u_r; const float* proj_v_r; const int32_t* pred_level_r; const float* view_cos_r;
    const float* track_depth; const uint8_t* bad; const uint8_t* has_obs;
    const uint8_t* desc;            /* n x 32 */
} OrbmRigMapPoints;

/* the entries of LastFrame.mvpMapPoints: the caller projects with the reference's own float expressions (x3Dc = Tcw * x3Dw,
 * proj_u/v = mpCamera->project(x3Dc), proj_u_r/v_r = mpCamera->project(GetRelativePoseTrl() * x3Dc) -- the LEFT camera's
 * project, as :1795-1796 calls it) and clears valid where the point is NULL, an outlier or invzc < 0.  octave / angle are
 * those of LastFrame's key point i (:1720, :1777-1779); angle may be NULL when orientation is not checked. */
typedef struct OrbmRigLastPoints {
    int32_t n;
    const uint8_t* valid; const float* proj_u; const float* proj_v; const float* proj_u_r; const float* proj_v_r;
    const int32_t* octave; const float* angle; const uint8_t* has_obs;
    const uint8_t* desc;            /* n x 32 */
} OrbmRigLastPoints;

/* The argument checks alone (host only, no device needed).  Exactly one of mp / last is given.  ORBX_OK, or ORBX_ERR_ARG for:
 * a NULL rig, assign or occupied; a NULL array where its n > 0 (a NULL left_to_right / right_to_left of a non-empty side
 * included; `angle` alone may be NULL); left.u_right != NULL; a negative n; the two sides disagreeing in min_x .. max_y,
 * grid_cols, grid_rows, n_levels or the values of scale_factors; n_levels outside [1, 32]; an entry of left_to_right outside
 * [-1, right.n) or of right_to_left outside [-1, left.n); a level of a live point outside [0, n_levels) -- pred_level where
 * in_view, pred_level_r where in_view_r (there -1 is legal), octave where valid.  Every entry below calls it first. */
int orbm_rig_search_check(const OrbmRigFrame* rig, const OrbmRigMapPoints* mp, const OrbmRigLastPoints* last,
                          const int32_t* assign, const uint8_t* occupied);

/* SearchByProjection(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints), F.Nleft != -1.  Returns nmatches, or < 0. */
int orbm_search_by_projection_rig(orbm_matcher* m, const OrbmRigFrame* rig, const OrbmRigMapPoints* pts,
                                  float th, int far_points, float th_far, float nnratio,
                                  int32_t* assign, uint8_t* occupied);

/* SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono), CurrentFrame.Nleft != -1.  level_window is one
 * of ORBM_LEVELS_*; with check_orientation both sides' angle arrays and pts->angle are required.  Returns nmatches, or < 0. */
int orbm_search_by_projection_last_rig(orbm_matcher* m, const OrbmRigFrame* rig, const OrbmRigLastPoints* pts,
                                       float th, int level_window, int check_orientation,
                                       int32_t* assign, uint8_t* occupied);

/* Batched forms: n_frames independent rig frames in ONE launch, a workgroup per frame (as OrbmProjQuery for conventional
 * frames); n_matches is written per query. */
typedef struct OrbmRigMapQuery {
    const OrbmRigFrame* rig;
    const OrbmRigMapPoints* pts;
    int32_t* assign; uint8_t* occupied;     /* in/out, left.n + right.n entries */
    int32_t n_matches;                      /* out */
} OrbmRigMapQuery;
typedef struct OrbmRigLastQuery {
    const OrbmRigFrame* rig;
    const OrbmRigLastPoints* pts;
    int32_t level_window;                   /* ORBM_LEVELS_*: bForward / bBackward depend on each stream's own motion */
    int32_t* assign; uint8_t* occupied;     /* in/out, left.n + right.n entries */
    int32_t n_matches;                      /* out */
} OrbmRigLastQuery;
int orbm_search_by_projection_rig_batch(orbm_matcher* m, OrbmRigMapQuery* queries, int n_frames,
                                        float th, int far_points, float th_far, float nnratio);
int orbm_search_by_projection_last_rig_batch(orbm_matcher* m, OrbmRigLastQuery* queries, int n_frames, float th, int check_orientation);

/* device time of the kernels (grid build + search) of the LAST rig search on this handle (HIP events), milliseconds */
float orbm_rig_search_last_kernel_ms(const orbm_matcher* m);
