// The float arithmetic of include/orbslam3_hip_track_project_rig.h: the rig part of Frame::UpdatePoseMatrices and of
// Frame::isInFrustumChecks' set-up (reference src/Frame.cc:559-566, :1294-1299), Frame::isInFrustumChecks for one camera
// (:1307-1361) inside the Nleft != -1 branch of Frame::isInFrustum (:662-672), the projection of
// ORBmatcher::SearchByProjection(CurrentFrame, LastFrame) for a rig frame (src/ORBmatcher.cc:1703-1718, :1794-1796) and
// Frame::UnprojectStereoFishEye (src/Frame.cc:1364).  Plain C++ without device builtins: the same text is the body of the kernels
// of orbm_track_project_rig.hip, of the host check tests/track_project_rig_geometry_check.cpp and of the one-core baseline
// tools/track_project_rig_cpu.cpp.  Built on tpj:: (track_project_geometry.h) and on kb8s::project (kb8_stereo_geometry.h), the
// one KannalaBrandt8 projection of the library; one operation per reference operation, -ffp-contract=off.
#pragma once
#include "kb8_stereo_geometry.h"
#include "track_project_geometry.h"
#include "../../include/orbslam3_hip_track_project_rig.h"

namespace tpr {

TPJ_HD kb8s::Cam kb8_cam(const float* p) { return kb8s::Cam{p[0], p[1], p[2], p[3], {p[4], p[5], p[6], p[7]}, 0.f}; }   // (precision: unproject's, unused)

// pose[7] double -> the rig frame record
TPJ_HD void rig_frame_pose(const OrbmTrackRigCamera& C, const double* pose, int normalise, OrbmRigFramePose* F)
{
    tpj::frame_pose(pose, normalise, &F->left);
    const OrbmFramePose& L = F->left;
    // Twc = mTcw.inverse(); mRwc = Twc.rotationMatrix(): the matrix of the conjugate, which SO3f's constructor normalised
    float c[4] = {-L.q[0], -L.q[1], -L.q[2], L.q[3]};
    const float length = tpj::norm4(c);
    c[0] = c[0] / length; c[1] = c[1] / length; c[2] = c[2] / length; c[3] = c[3] / length;
    tpj::quat_to_R(c, F->Rwc);
    for (int r = 0; r < 3; r++) {
        const float* a = C.Rrl + 3 * r;
        for (int k = 0; k < 3; k++) F->R_r[3 * r + k] = tpj::dot3(a[0], a[1], a[2], L.Rcw[k], L.Rcw[3 + k], L.Rcw[6 + k]);     // mR = Rrl * mRcw
        F->t_r[r] = tpj::dot3(a[0], a[1], a[2], L.tcw[0], L.tcw[1], L.tcw[2]) + C.trl[r];                                      // mt = Rrl * mtcw + trl
        F->Ow_r[r] = tpj::dot3(F->Rwc[3 * r], F->Rwc[3 * r + 1], F->Rwc[3 * r + 2], C.tlr[0], C.tlr[1], C.tlr[2]) + L.Ow[r];   // twc = mRwc * tlr + mOw
    }
}

struct Side {           // what isInFrustumChecks leaves behind for one camera; the five values only where valid
    int valid, level;
    float u, v, view_cos, depth;
};

// Frame::isInFrustumChecks(pMP, viewingCosLimit, bRight) with mR / mt / twc and the camera of that side
TPJ_HD Side frustum_side(const OrbmTrackRigCamera& C, const float* cam8, const float* mR, const float* mt, const float* twc,
                         const float* P, const float* Pn, float min_distance_raw, float max_distance_raw, float viewingCosLimit)
{
    Side s{0, -1, 0.f, 0.f, 0.f, 0.f};
    float Pc[3];
    for (int r = 0; r < 3; r++) Pc[r] = tpj::dot3(mR[3 * r], mR[3 * r + 1], mR[3 * r + 2], P[0], P[1], P[2]) + mt[r];
    const float Pc_dist = tpj::norm3(Pc[0], Pc[1], Pc[2]);
    if (Pc[2] < 0.0f) return s;
    float uv[2];
    kb8s::project(kb8_cam(cam8), Pc, uv);               // the f64 transcendentals: only behind the depth test
    if (uv[0] < C.min_x || uv[0] > C.max_x) return s;
    if (uv[1] < C.min_y || uv[1] > C.max_y) return s;
    const float maxDistance = 1.2f * max_distance_raw;
    const float minDistance = 0.8f * min_distance_raw;
    const float PO0 = P[0] - twc[0], PO1 = P[1] - twc[1], PO2 = P[2] - twc[2];
    const float dist = tpj::norm3(PO0, PO1, PO2);
    if (dist < minDistance || dist > maxDistance) return s;
    const float viewCos = tpj::dot3(PO0, PO1, PO2, Pn[0], Pn[1], Pn[2]) / dist;
    if (viewCos < viewingCosLimit) return s;
    s.level = tpj::predict_scale(max_distance_raw, dist, C.log_scale_factor, C.n_levels);
    s.valid = 1;
    s.u = uv[0]; s.v = uv[1];
    s.view_cos = viewCos;
    s.depth = Pc_dist;
    return s;
}

TPJ_HD Side frustum_left(const OrbmTrackRigCamera& C, const OrbmRigFramePose& F, const float* P, const float* Pn, float mn, float mx, float limit)
{
    return frustum_side(C, C.left, F.left.Rcw, F.left.tcw, F.left.Ow, P, Pn, mn, mx, limit);
}
TPJ_HD Side frustum_right(const OrbmTrackRigCamera& C, const OrbmRigFramePose& F, const float* P, const float* Pn, float mn, float mx, float limit)
{
    return frustum_side(C, C.right, F.R_r, F.t_r, F.Ow_r, P, Pn, mn, mx, limit);
}

struct LastRow { int valid; float u, v, ur, vr; };

// src/ORBmatcher.cc:1703-1718 and :1794-1796 for one last-frame map point
TPJ_HD LastRow project_last_rig_row(const OrbmTrackRigCamera& C, const OrbmRigFramePose& F, const float* x3Dw)
{
    LastRow r{0, -1.f, -1.f, -1.f, -1.f};
    float x3Dc[3];
    tpj::quat_rotate(F.left.q, x3Dw, x3Dc);             // Tcw * x3Dw = so3 * p + translation
    x3Dc[0] = x3Dc[0] + F.left.tcw[0]; x3Dc[1] = x3Dc[1] + F.left.tcw[1]; x3Dc[2] = x3Dc[2] + F.left.tcw[2];
    const float invzc = (float)(1.0 / (double)x3Dc[2]);
    if (invzc < 0) return r;
    const kb8s::Cam cam = kb8_cam(C.left);
    float uv[2];
    kb8s::project(cam, x3Dc, uv);
    if (uv[0] < C.min_x || uv[0] > C.max_x) return r;
    if (uv[1] < C.min_y || uv[1] > C.max_y) return r;
    float x3Dr[3], uvr[2];
    tpj::quat_rotate(C.q_rl, x3Dc, x3Dr);               // GetRelativePoseTrl() * x3Dc
    x3Dr[0] = x3Dr[0] + C.trl[0]; x3Dr[1] = x3Dr[1] + C.trl[1]; x3Dr[2] = x3Dr[2] + C.trl[2];
    kb8s::project(cam, x3Dr, uvr);                      // CurrentFrame.mpCamera: the left camera, no bounds test
    r.valid = 1;
    r.u = uv[0]; r.v = uv[1]; r.ur = uvr[0]; r.vr = uvr[1];
    return r;
}

// Frame::UnprojectStereoFishEye: mRwc * mvStereo3Dpoints[i] + mOw
TPJ_HD void unproject_stereo_fisheye(const OrbmRigFramePose& F, const float* p, float* w)
{
    for (int r = 0; r < 3; r++) w[r] = tpj::dot3(F.Rwc[3 * r], F.Rwc[3 * r + 1], F.Rwc[3 * r + 2], p[0], p[1], p[2]) + F.left.Ow[r];
}

}  // namespace tpr
