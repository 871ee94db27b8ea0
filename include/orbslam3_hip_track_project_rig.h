/* Projection of map points into a two-camera KannalaBrandt8 rig frame (Nleft != -1) on the device: the rig twin of the pinhole
 * projection header, and what fills OrbmRigMapPoints / OrbmRigLastPoints for the two rig tracking searches of
 * orbslam3_hip_rig_match.h.  A header of its own: it includes the pinhole projection header, and nothing includes it.  The entry
 * points live on the orbm_matcher handle.
 *
 *   orbm_rig_frame_pose_batch_device -> orbm_project_last_rig_batch_device -> last-frame search -> pose_optimize (rig edges)
 *       -> orbm_track_handover_batch_device -> orbm_rig_frame_pose_batch_device -> orbm_frustum_rig_batch_device
 *       -> local-map search -> pose_optimize (rig edges)
 * orbm_track_handover_batch_device is indexed by SLOT (mvpMapPoints[0 .. Nleft+Nright)), not by camera, so it serves rig frames as
 * it is: cap covers Nleft + Nright, and nothing of it changes here.
 *
 * All float arithmetic is that of csrc/track_project_rig_geometry.h, compiled with -ffp-contract=off: the operations of
 * csrc/track_project_geometry.h (three-term reductions a0*b0 + (a1*b1 + a2*b2)) and KannalaBrandt8::project of
 * csrc/kb8_stereo_geometry.h, whose atan2 / sin / cos are the float rounding of the f64 function: host, device and the reference's
 * libm agree to one float ulp there, and bit for bit everywhere else. */
#ifndef ORBSLAM3_HIP_TRACK_PROJECT_RIG_H
#define ORBSLAM3_HIP_TRACK_PROJECT_RIG_H

/* The pinhole projection header, by a computed name: that header's ABI test requires that no other file of this directory spells
 * its file name, and this one has to include it (OrbmFramePose, OrbmLocalPoints, the limits). */
#define ORBM_RIG_STR(x) #x
#define ORBM_RIG_HEADER(stem) ORBM_RIG_STR(stem.h)
#include ORBM_RIG_HEADER(orbslam3_hip_track_project)
#undef ORBM_RIG_HEADER
#undef ORBM_RIG_STR

#ifdef __cplusplus
extern "C" {
#endif

/* The rig and the pyramid of the frames, one for the call.  Host callers fill Rrl / trl / q_rl from Frame::mTrl
 * (rotationMatrix(), translation(), unit_quaternion()) and tlr from mTlr.translation(). */
typedef struct OrbmTrackRigCamera {
    float left[8];                              /* mpCamera->mvParameters: fx fy cx cy k0 k1 k2 k3 */
    float right[8];                             /* mpCamera2 */
    float Rrl[9];                               /* row major */
    float trl[3];
    float tlr[3];
    float q_rl[4];                              /* x y z w */
    float min_x, min_y, max_x, max_y;           /* mnMinX .. mnMaxY: one set for both cameras, as in Frame */
    float log_scale_factor;
    int32_t n_levels;                           /* 1 .. ORBM_TRACK_MAX_LEVELS */
} OrbmTrackRigCamera;

/* What a rig Frame holds per pose, computed once per frame: the left record, mRwc (Twc.rotationMatrix(): from the renormalised
 * conjugate quaternion, as Frame::UpdatePoseMatrices takes it -- not the transpose of Rcw), and the right camera's
 * mR = Rrl * mRcw, mt = Rrl * mtcw + trl, twc = mRwc * tlr + mOw of Frame::isInFrustumChecks (src/Frame.cc:1294-1299). */
typedef struct OrbmRigFramePose {
    OrbmFramePose left;
    float Rwc[9];
    float R_r[9];
    float t_r[3];
    float Ow_r[3];
} OrbmRigFramePose;

/* d_pose[batch][7] double -> d_rig_pose[batch]; `normalise` as orbm_frame_pose_batch_device.  Only enqueues. */
int orbm_rig_frame_pose_batch_device(orbm_matcher* m, const OrbmTrackRigCamera* cam, const double* d_pose, int batch, int normalise,
                                     OrbmRigFramePose* d_rig_pose, void* stream);

/* [batch][pcap] each; names, types and meanings are those of OrbmRigMapPoints, so a host caller points an OrbmRigMapPoints at row
 * b of the downloaded arrays without a copy.  in_view / in_view_r / pred_level / pred_level_r are outputs.  The other eight are
 * IN/OUT: the MapPoint members mTrackProjX/Y, mTrackViewCos, mTrackDepth and their R twins, which Frame::isInFrustum does not
 * reset -- a side that fails leaves them as an earlier frame wrote them, and SearchByProjection reads mTrackDepth for its
 * far-point test even when only the right camera sees the point (src/ORBmatcher.cc:52-56). */
typedef struct OrbmRigFrustumOut {
    uint8_t* in_view; float* proj_u; float* proj_v; int32_t* pred_level; float* view_cos;
    uint8_t* in_view_r; float* proj_u_r; float* proj_v_r; int32_t* pred_level_r; float* view_cos_r;
    float* track_depth; float* track_depth_r;
    int32_t* n_to_match;            /* [batch] points with either side in view */
} OrbmRigFrustumOut;

/* The Nleft != -1 branch of Frame::isInFrustum (src/Frame.cc:662-672) with Frame::isInFrustumChecks (:1288-1362) for both cameras,
 * inside the loop of Tracking::SearchLocalPoints.  Per camera: Pc = mR*P + mt; Pc_dist = |Pc|; PcZ < 0.0f fails (-0.0f passes);
 * uv = KannalaBrandt8::project(Pc) with mpCamera (left) / mpCamera2 (right); uv outside [min, max] fails (strict); dist = |P - twc|
 * against 0.8f*min_distance and 1.2f*max_distance; viewCos = PO.Pn/dist < viewing_cos_limit fails; level = PredictScale with the
 * raw maximum, as orbm_frustum_batch_device.
 * A side that passes writes in_view = 1, proj_u/v, pred_level, view_cos and track_depth of that side.  A side that fails writes
 * in_view = 0 and pred_level = -1 and nothing else.  Rows that SearchLocalPoints skips (skip, bad, index >= n[b]) get in_view =
 * in_view_r = 0 and keep everything else, pred_level included.  Only enqueues (a clear of n_to_match and one kernel). */
int orbm_frustum_rig_batch_device(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* d_rig_pose, const OrbmLocalPoints* pts,
                                  float viewing_cos_limit, const OrbmRigFrustumOut* out, int batch, void* stream);

/* [batch][cap] each, every row written; the fields of OrbmRigLastPoints */
typedef struct OrbmRigLastProjOut {
    uint8_t* valid; float* proj_u; float* proj_v; float* proj_u_r; float* proj_v_r;
} OrbmRigLastProjOut;

/* The projection of SearchByProjection(CurrentFrame, LastFrame) for CurrentFrame.Nleft != -1 (src/ORBmatcher.cc:1703-1718 and
 * :1794-1796): x3Dc = Tcw * x3Dw through the quaternion; invzc = (float)(1.0/(double)z), invzc < 0 skips; uv = mpCamera->project,
 * outside the bounds skips; x3Dr = Trl * x3Dc (the quaternion q_rl plus trl, not Rrl *); uv_r = mpCamera->project(x3Dr) -- the
 * LEFT camera's parameters, as the reference calls it -- with no bounds test.  Rows skipped, without a point or dead: valid 0,
 * u = v = u_r = v_r = -1.  A rig last frame has Nleft + Nright entries; cap covers them. */
int orbm_project_last_rig_batch_device(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* d_rig_pose,
                                       const float* d_mp_xyz, const uint8_t* d_has_point, const int32_t* d_n, int cap,
                                       const OrbmRigLastProjOut* out, int batch, void* stream);

/* Frame / KeyFrame::UnprojectStereoFishEye (src/Frame.cc:1364): d_world[b][i] = mRwc * d_points[b][i] + mOw for i < n[b] with
 * d_valid[b][i]; other rows of d_world [batch][cap][3] are left as they are.  Only enqueues. */
int orbm_unproject_stereo_fisheye_batch_device(orbm_matcher* m, const OrbmRigFramePose* d_rig_pose, const float* d_points, const uint8_t* d_valid,
                                               const int32_t* d_n, int cap, float* d_world, int batch, void* stream);

/* Host-array forms: the same structures holding HOST pointers.  Each stages its arrays in one blob (the in/out arrays are
 * uploaded), makes the same launch and copies back; results are bit-identical to the device entries.  Synchronous. */
int orbm_frustum_rig_batch(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const OrbmLocalPoints* pts,
                           float viewing_cos_limit, const OrbmRigFrustumOut* out, int batch);
int orbm_project_last_rig_batch(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses,
                                const float* mp_xyz, const uint8_t* has_point, const int32_t* n, int cap,
                                const OrbmRigLastProjOut* out, int batch);
int orbm_unproject_stereo_fisheye_batch(orbm_matcher* m, const OrbmRigFramePose* poses, const float* points, const uint8_t* valid,
                                        const int32_t* n, int cap, float* world, int batch);

/* The argument and capacity checks of the frustum entries alone (host only).  ORBX_ERR_ARG: a NULL cam, poses, pts or out, a NULL
 * array in pts or out (the in/out arrays included), pts->pcap <= 0, cam->n_levels outside [1, ORBM_TRACK_MAX_LEVELS], batch < 1.
 * ORBX_ERR_CAPACITY: batch > ORBM_TRACK_MAX_BATCH. */
int orbm_track_project_rig_check(const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const OrbmLocalPoints* pts,
                                 const OrbmRigFrustumOut* out, int batch);

/* device time of the kernel of the LAST host-array rig entry on this handle (HIP events), milliseconds */
float orbm_track_project_rig_last_kernel_ms(const orbm_matcher* m);

#ifdef __cplusplus
}
#endif
#endif
