/* Device-resident tracking of two-camera fisheye rig frames (Nleft != -1): the two projection searches of orbslam3_hip_rig_match.h
 * and PoseOptimization with rig edges (orbslam3_hip_kb8.h), fed by arrays that never left HBM.  A header of its own:
 * it includes orbslam3_hip.h, and nothing includes it.  With the rig projection entries and the hand-over, a rig tracker runs
 *
 *   rig frame pose -> last-frame projection -> orbm_search_by_projection_last_rig_batch_device -> pose_optimize_rig_batch_device
 *       -> orbm_track_handover_batch_device -> rig frame pose -> frustum projection
 *       -> orbm_search_by_projection_rig_batch_device -> pose_optimize_rig_batch_device
 *
 * between the two extractions and the pose TrackLocalMap leaves without a visit to the host.
 *
 * SLOTS.  Row b of d_assign / d_occupied / d_outlier ([batch][slot_cap]) holds the reference's mvpMapPoints[0 .. Nleft+Nright) of
 * frame b compactly: left slot i at i, right slot j at d_n_l[b] + j -- the order of the host entries, of
 * orbm_track_handover_batch_device and of the rows a rig last frame hands to the last-frame projection.  The searches never write a
 * slot at or beyond n_l + n_r; d_n_slots[b] = n_l + n_r is what the hand-over takes as d_n_cur.
 *
 * RESULTS.  assign, occupied and n_matches of frame b are integer for integer those of orbm_search_by_projection(_last)_rig_batch
 * on frame b's arrays, every quirk listed in orbslam3_hip_rig_match.h included: the same kernel runs behind both.
 *
 * CLAMPS.  The host entries refuse bad contents; a device entry cannot read them, so it clamps instead:
 *   - a count (d_n_l, d_n_r, d_n) outside [0, cap] is clamped to it;
 *   - an entry of d_left_to_right outside [-1, n_r) or of d_right_to_left outside [-1, n_l) counts as -1;
 *   - a level (d_octave, d_pred_level, d_pred_level_r) outside [0, n_levels) counts as the nearest level; d_pred_level_r == -1 keeps
 *     its meaning (no right pass);
 *   - a d_level_window entry that is none of ORBM_LEVELS_* counts as ORBM_LEVELS_AROUND.
 *
 * Every entry makes its argument checks on the host before it touches the handle or a device, and then only enqueues on `stream`;
 * the one exception is the handle's workspace, which grows on demand (a device synchronise, first call or a larger batch only).
 * A handle serves one call at a time. */
#ifndef ORBSLAM3_HIP_RIG_TRACK_DEVICE_H
#define ORBSLAM3_HIP_RIG_TRACK_DEVICE_H

#include "orbslam3_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct OrbmDeviceRigFrames {           /* what the two extractors and orbm_stereo_fisheye_batch_device left in HBM */
    const OrbxKeyPoint* d_kps_l; const uint8_t* d_desc_l; const int32_t* d_n_l; int32_t cap_l;   /* [batch][cap_l]: mvKeys, rows [0,Nleft) of mDescriptors */
    const OrbxKeyPoint* d_kps_r; const uint8_t* d_desc_r; const int32_t* d_n_r; int32_t cap_r;   /* mvKeysRight */
    const int32_t* d_left_to_right;            /* [batch][cap_l] */
    const int32_t* d_right_to_left;            /* [batch][cap_r] */
    float min_x, min_y, max_x, max_y; int32_t grid_cols, grid_rows;
    const float* scale_factors; int32_t n_levels;          /* HOST array, 1..32 */
    int32_t slot_cap;                          /* row stride of d_assign / d_occupied, >= cap_l + cap_r */
} OrbmDeviceRigFrames;
typedef struct OrbmDeviceRigLastPoints {       /* fields of OrbmRigLastPoints, [batch][cap] */
    const uint8_t* d_valid; const float* d_u; const float* d_v; const float* d_u_r; const float* d_v_r;   /* what OrbmRigLastProjOut wrote */
    const int32_t* d_octave; const float* d_angle; const uint8_t* d_has_obs;   /* d_has_obs NULL = all 1; d_angle required with check_orientation */
    const uint8_t* d_desc; const int32_t* d_n; int32_t cap;
    const int32_t* d_level_window;             /* [batch] ORBM_LEVELS_*, NULL = ORBM_LEVELS_AROUND; bForward/bBackward stay with the caller */
} OrbmDeviceRigLastPoints;
typedef struct OrbmDeviceRigMapPoints {        /* fields of OrbmRigMapPoints, [batch][cap]: the arrays of OrbmRigFrustumOut plus the map's own */
    const uint8_t* d_in_view; const float* d_u; const float* d_v; const int32_t* d_pred_level; const float* d_view_cos;
    const uint8_t* d_in_view_r; const float* d_u_r; const float* d_v_r; const int32_t* d_pred_level_r; const float* d_view_cos_r;
    const float* d_track_depth; const uint8_t* d_bad; const uint8_t* d_has_obs; const uint8_t* d_desc; const int32_t* d_n; int32_t cap;
    float th_far, nnratio; int32_t far_points;
} OrbmDeviceRigMapPoints;

/* The argument and capacity checks of the two searches alone (host only, no device needed; pointers are only compared with NULL).
 * Exactly one of last / mp is given.  ORBX_ERR_ARG: a NULL frames, neither or both of last / mp, batch < 1, a NULL array (d_angle,
 * d_has_obs and d_level_window of the last-frame points may be NULL), cap_l, cap_r or cap below 1, slot_cap < cap_l + cap_r,
 * n_levels outside [1, 32], grid_cols or grid_rows below 1 or more than 2^20 cells, max_x <= min_x or max_y <= min_y.
 * ORBX_ERR_CAPACITY: cap_l or cap_r above 8192 (the grid is sorted in LDS), or cap_l + cap_r + 256 bytes beyond the search kernel's
 * LDS (the occupancy table; out of reach while the first limit holds). */
int orbm_rig_search_device_check(const OrbmDeviceRigFrames* frames, const OrbmDeviceRigLastPoints* last, const OrbmDeviceRigMapPoints* mp, int batch);

/* SearchByProjection(CurrentFrame, LastFrame, th, bMono) for batch rig frames.  d_assign / d_occupied [batch][frames->slot_cap] are
 * in/out, d_n_matches [batch] out, d_n_slots [batch] out or NULL.  ORBX_ERR_ARG besides the check's: a NULL d_assign, d_occupied,
 * d_n_matches or handle, check_orientation without d_angle.  Launches: setup, grid (2 x batch sides), search. */
int orbm_search_by_projection_last_rig_batch_device(orbm_matcher* m, const OrbmDeviceRigFrames* frames, const OrbmDeviceRigLastPoints* last, int batch,
        float th, int check_orientation, int32_t* d_assign, uint8_t* d_occupied, int32_t* d_n_matches, int32_t* d_n_slots, void* stream);

/* SearchByProjection(Frame&, vector<MapPoint*>&, th, bFarPoints, thFarPoints) for batch rig frames; far_points, th_far and nnratio
 * travel in `points`.  Arguments, errors and launches as above. */
int orbm_search_by_projection_rig_batch_device(orbm_matcher* m, const OrbmDeviceRigFrames* frames, const OrbmDeviceRigMapPoints* points, int batch,
        float th, int32_t* d_assign, uint8_t* d_occupied, int32_t* d_n_matches, int32_t* d_n_slots, void* stream);

/* Optimizer::PoseOptimization of batch rig frames on a handle with a rig set (pose_set_rig_kb8).  The edges are gathered on the
 * device in slot order, the order in which the reference walks a rig frame (src/Optimizer.cc:935-990): slot s < n_l with
 * d_assign[b][s] in [0, mp_cap) is a left edge (kind 0) observing d_kps_l[b][s], any other such slot a right edge (ORBX_EDGE_RIGHT)
 * observing d_kps_r[b][s - n_l]; information inv_level_sigma2[octave of that key point] (octave clamped to the table), Xw =
 * (double)d_mp_xyz[b][assign].  An assign outside [0, mp_cap) means no point.  Results are bit for bit those of pose_optimize_batch
 * on the same handle for these edges when both take the same kernel variant: this entry chooses it by slot_cap > 512, the host entry
 * by the largest edge count > 512.
 * d_pose [batch][7] (q xyzw, t) is the initial pose.  Outputs, each may be NULL: d_pose_out [batch][7], d_inliers [batch], d_outlier
 * [batch][slot_cap] (every row written whole: mvbOutlier of the slot, 0 for a slot without a point), d_results [batch].
 * ORBX_ERR_ARG: a NULL frames, array or handle, batch < 1, cap_l, cap_r or mp_cap below 1, slot_cap < cap_l + cap_r, n_levels outside
 * [1, 16], a handle whose camera is not a rig. */
typedef struct PoseDeviceRigFrames {
    const OrbxKeyPoint* d_kps_l; const int32_t* d_n_l; int32_t cap_l;
    const OrbxKeyPoint* d_kps_r; const int32_t* d_n_r; int32_t cap_r;
    const int32_t* d_assign; int32_t slot_cap;             /* [batch][slot_cap] */
    const float* d_mp_xyz; int32_t mp_cap; const double* d_pose;
    const float* inv_level_sigma2; int32_t n_levels;       /* HOST, <= 16 */
    double huber_mono;
} PoseDeviceRigFrames;
int pose_optimize_rig_batch_device(pose_solver* s, const PoseDeviceRigFrames* frames, int batch, double* d_pose_out, int32_t* d_inliers,
        uint8_t* d_outlier /*[batch][slot_cap]*/, PoseResult* d_results, void* stream);

#ifdef __cplusplus
}
#endif
#endif
