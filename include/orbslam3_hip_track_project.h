/* Projection of map points into a frame on the device: the step between the device-resident tracking searches and pose
 * optimisations of orbslam3_hip.h.  A header of its own (it includes orbslam3_hip.h; nothing includes it); the entry points live on
 * the orbm_matcher handle.  Pinhole frames only (Nleft == -1: monocular and rectified stereo).
 *
 *   extract -> orbm_frame_pose_batch_device -> orbm_project_last_batch_device -> orbm_search_by_projection_last_batch_device
 *           -> pose_optimize_batch_device -> orbm_track_handover_batch_device -> orbm_frame_pose_batch_device
 *           -> orbm_frustum_batch_device -> orbm_search_by_projection_batch_device -> pose_optimize_batch_device
 * runs on one stream with one synchronisation at the end.
 *
 * All float arithmetic is that of csrc/track_project_geometry.h, compiled with -ffp-contract=off.  Eigen's fixed-size reductions
 * of three terms are a0*b0 + (a1*b1 + a2*b2); the four-term sum of Quaternionf::norm() is (x*x + z*z) + (y*y + w*w), the order
 * of Eigen's 4-wide packet reduction (parity to a real Eigen build is unpinned). */
#ifndef ORBSLAM3_HIP_TRACK_PROJECT_H
#define ORBSLAM3_HIP_TRACK_PROJECT_H

#include "orbslam3_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define ORBM_TRACK_MAX_BATCH 65535      /* frames per call (one grid row each) */
#define ORBM_TRACK_MAX_LEVELS 16        /* as pose_optimize_batch_device */

/* What Frame::mTcw (q, tcw), mRcw, mtcw and mOw hold (src/Frame.cc:559-566).  Host callers fill it from the Frame. */
typedef struct OrbmFramePose {
    float q[4];         /* mTcw.unit_quaternion(): x y z w */
    float Rcw[9];       /* row major */
    float tcw[3];
    float Ow[3];
} OrbmFramePose;

/* d_pose[batch][7] double (qx qy qz qw tx ty tz, as pose_optimize_batch_device writes) -> d_frame_pose[batch].
 * normalise != 0 restates src/Optimizer.cc:1108-1111: cast to float, then Sophus::SO3f's constructor divides the quaternion by its
 * float norm.  normalise == 0 takes the cast quaternion as it is: a pose that already is an mTcw (the motion-model prediction);
 * renormalising a unit float quaternion can move it by an ulp.  Then Frame::UpdatePoseMatrices: Rcw = toRotationMatrix(q),
 * Ow = SE3f::inverse().translation() = normalised(conjugate(q)) rotating tcw * -1 (Eigen's _transformVector).  Only enqueues. */
int orbm_frame_pose_batch_device(orbm_matcher* m, const double* d_pose, int batch, int normalise, OrbmFramePose* d_frame_pose, void* stream);

/* the frames' camera and pyramid, one for the call */
typedef struct OrbmTrackCamera {
    float fx, fy, cx, cy, bf;                   /* Pinhole parameters, mbf */
    float min_x, min_y, max_x, max_y;           /* mnMinX .. mnMaxY */
    float log_scale_factor;                     /* mfLogScaleFactor, as the host computed it */
    int32_t n_levels;                           /* mnScaleLevels, 1 .. ORBM_TRACK_MAX_LEVELS */
} OrbmTrackCamera;

/* the local map of every frame, [batch][pcap] rows of which n[b] are live (mvpLocalMapPoints) */
typedef struct OrbmLocalPoints {
    const float* xyz;               /* [batch][pcap][3] GetWorldPos(): the table PoseDeviceFrames::d_mp_xyz reads */
    const float* normal;            /* [batch][pcap][3] GetNormal() */
    const float* min_distance;      /* raw mfMinDistance: the call applies 0.8f * (GetMinDistanceInvariance) */
    const float* max_distance;      /* raw mfMaxDistance: 1.2f * for the gate, raw in PredictScale */
    const uint8_t* skip;            /* mnLastFrameSeen == mCurrentFrame.mnId (orbm_track_handover_batch_device writes it) */
    const uint8_t* bad;             /* isBad() */
    const int32_t* n;               /* [batch] */
    int32_t pcap;
} OrbmLocalPoints;

/* [batch][pcap] each, every row written.  valid / u / v / octave are OrbmDeviceLastPoints::d_valid / d_u / d_v / d_octave
 * (mbTrackInView, mTrackProjX, mTrackProjY, mnTrackScaleLevel), view_cos / track_depth are OrbmDeviceMapPointExtras'. */
typedef struct OrbmFrustumOut {
    uint8_t* valid; float* u; float* v; int32_t* octave;
    float* view_cos; float* track_depth;
    float* proj_ur;                 /* mTrackProjXR = uv(0) - mbf*invz */
    int32_t* n_to_match;            /* [batch] nToMatch of Tracking::SearchLocalPoints */
} OrbmFrustumOut;

/* Frame::isInFrustum (src/Frame.cc:599-661) inside the loop of Tracking::SearchLocalPoints (src/Tracking.cc:3512-3530), statement
 * by statement: Pc = Rcw*P + tcw; PcZ < 0.0f returns (-0.0f passes); uv = fx*X/Z + cx (NaN for X = Z = 0 fails neither bounds
 * test); uv outside [min, max] returns; dist = |P - Ow| against 0.8f*min_distance and 1.2f*max_distance; viewCos = PO.Pn/dist
 * against viewing_cos_limit; level = ceil(logf(max_distance/dist)/log_scale_factor) clamped to [0, n_levels) (a quotient that is
 * NaN or outside int gives 0, what the reference's conversion gives on x86-64).  All comparisons are strict, as written there.
 * Rows not in view: valid 0, level -1, view_cos / track_depth / proj_ur 0, and u = v = -1 -- except rows that fail after the
 * bounds test, which keep uv as the reference stored it (:626-627).  Skipped, bad and dead (>= n[b]) rows: valid 0, u = v = -1.
 * Only enqueues on `stream` (a clear of n_to_match and one kernel). */
int orbm_frustum_batch_device(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* d_frame_pose, const OrbmLocalPoints* pts,
                              float viewing_cos_limit, const OrbmFrustumOut* out, int batch, void* stream);

/* [batch][cap] each, every row written: OrbmDeviceLastPoints::d_valid / d_u / d_v, and proj_ur = uv(0) - mbf*invzc */
typedef struct OrbmLastProjOut {
    uint8_t* valid; float* u; float* v; float* proj_ur;
} OrbmLastProjOut;

/* Lines :1686-1718 of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame) (src/ORBmatcher.cc): per last-frame feature i with
 * has_point[b][i] (= LastFrame.mvpMapPoints[i] && !mvbOutlier[i]) x3Dc = Tcw * x3Dw through the QUATERNION (Eigen's
 * _transformVector(q, x) + t, which is not Rcw*x bit for bit), invzc = (float)(1.0/(double)z), invzc < 0 skips, uv = project(x3Dc),
 * uv outside the bounds skips.  Rows that are skipped, without a point or dead: valid 0, u = v = -1, proj_ur 0.  Octave, angle and
 * descriptors of OrbmDeviceLastPoints are the last frame's own arrays; bForward / bBackward stay with the caller. */
int orbm_project_last_batch_device(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* d_frame_pose,
                                   const float* d_mp_xyz, const uint8_t* d_has_point, const int32_t* d_n, int cap,
                                   const OrbmLastProjOut* out, int batch, void* stream);

/* The hand-over from TrackWithMotionModel to TrackLocalMap (src/Tracking.cc:3055-3079 and :3490-3507).
 * In: d_assign[batch][cap] of the last-frame search (last-frame feature index, -1 = none) and d_outlier[batch][cap] of the pose
 * optimisation behind it, d_n_cur[batch] live features; d_last_local[batch][last_cap] = local-map row of that last-frame feature's
 * map point (-1 = not in the table); d_bad / d_has_obs [batch][pcap] of the local map.
 * Out: d_assign_local[batch][cap] = the row, or -1 for an unmatched feature, a discarded outlier or a bad point; d_occupied =
 * assign_local >= 0 && has_obs[row]; d_skip[batch][pcap] cleared and then set for the row of EVERY feature that held a point,
 * discarded outliers included (:3073, :3502); d_n_dropped[batch] = held features whose point has no row (index outside
 * [0, last_cap) or d_last_local outside [0, pcap)): the caller appends the last frame's points to its local table, so this is 0.
 * Rows of features >= d_n_cur[b] get -1 / 0.  Only enqueues. */
int orbm_track_handover_batch_device(orbm_matcher* m, const int32_t* d_assign, const uint8_t* d_outlier, const int32_t* d_n_cur, int cap,
                                     const int32_t* d_last_local, int last_cap, const uint8_t* d_bad, const uint8_t* d_has_obs, int pcap,
                                     int32_t* d_assign_local, uint8_t* d_occupied, uint8_t* d_skip, int32_t* d_n_dropped,
                                     int batch, void* stream);

/* Host-array forms: the same structures holding HOST pointers, `poses` from the caller.  Each stages its arrays in one blob,
 * makes the same launch and copies back; results are bit-identical to the device entries.  Synchronous. */
int orbm_frustum_batch(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* poses, const OrbmLocalPoints* pts,
                       float viewing_cos_limit, const OrbmFrustumOut* out, int batch);
int orbm_project_last_batch(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* poses,
                            const float* mp_xyz, const uint8_t* has_point, const int32_t* n, int cap,
                            const OrbmLastProjOut* out, int batch);

/* The argument and capacity checks of the frustum entries alone (host only, no device needed; pointers are only compared with
 * NULL).  ORBX_ERR_ARG: a NULL cam, poses, pts or out, a NULL array in pts or out, pts->pcap <= 0, cam->n_levels outside
 * [1, ORBM_TRACK_MAX_LEVELS], batch < 1.  ORBX_ERR_CAPACITY: batch > ORBM_TRACK_MAX_BATCH. */
int orbm_track_project_check(const OrbmTrackCamera* cam, const OrbmFramePose* poses, const OrbmLocalPoints* pts,
                             const OrbmFrustumOut* out, int batch);

/* device time of the kernel of the LAST orbm_frustum_batch / orbm_project_last_batch on this handle (HIP events), milliseconds */
float orbm_track_project_last_kernel_ms(const orbm_matcher* m);

#ifdef __cplusplus
}
#endif
#endif
