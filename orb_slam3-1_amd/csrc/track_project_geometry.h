// The float arithmetic of include/orbslam3_hip_track_project.h: Frame::UpdatePoseMatrices (reference src/Frame.cc:559-566) behind
// the pose hand-over of Optimizer::PoseOptimization (src/Optimizer.cc:1108-1111), Frame::isInFrustum (src/Frame.cc:599-661) with
// MapPoint::PredictScale (src/MapPoint.cc:531-546), and the projection of ORBmatcher::SearchByProjection(CurrentFrame, LastFrame)
// (src/ORBmatcher.cc:1703-1718).  Plain C++ without device builtins, so that the same text is the body of the kernels of
// orbm_track_project.hip and of the host check tests/track_project_geometry_check.cpp.  One operation per reference operation;
// the library is built with -ffp-contract=off.
#pragma once
#include <math.h>

#include "../../include/orbslam3_hip_track_project.h"

#ifdef __HIPCC__
#define TPJ_HD __host__ __device__ __forceinline__
#else
#define TPJ_HD inline
#endif

namespace tpj {

TPJ_HD float dot3(float a0, float a1, float a2, float b0, float b1, float b2) { return a0 * b0 + (a1 * b1 + a2 * b2); }   // Eigen's fixed-size redux
TPJ_HD float norm3(float a0, float a1, float a2) { return sqrtf(a0 * a0 + (a1 * a1 + a2 * a2)); }
// Quaternionf::norm(): the four squares summed as Eigen's 4-wide packet reduction does, lanes (0 + 2) + (1 + 3)
TPJ_HD float norm4(const float* q) { return sqrtf((q[0] * q[0] + q[2] * q[2]) + (q[1] * q[1] + q[3] * q[3])); }

TPJ_HD void quat_rotate(const float* q, const float* v, float* out)        // Eigen QuaternionBase::_transformVector
{
    float ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux += ux; uy += uy; uz += uz;
    out[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
    out[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
    out[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}

TPJ_HD void quat_to_R(const float* q, float* R)                             // Eigen QuaternionBase::toRotationMatrix
{
    const float tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const float twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const float txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const float tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

// pose[7] = qx qy qz qw tx ty tz in double -> the frame's pose record
TPJ_HD void frame_pose(const double* pose, int normalise, OrbmFramePose* F)
{
    float q[4] = {(float)pose[0], (float)pose[1], (float)pose[2], (float)pose[3]};
    if (normalise) {                                    // Sophus::SO3f(quaternion): coeffs() /= norm()
        const float length = norm4(q);
        q[0] = q[0] / length; q[1] = q[1] / length; q[2] = q[2] / length; q[3] = q[3] / length;
    }
    for (int i = 0; i < 4; i++) F->q[i] = q[i];
    for (int i = 0; i < 3; i++) F->tcw[i] = (float)pose[4 + i];
    quat_to_R(q, F->Rcw);
    // SE3f::inverse(): invR = SO3f(conjugate), which normalises again; translation = invR * (translation() * -1)
    float c[4] = {-q[0], -q[1], -q[2], q[3]};
    const float length = norm4(c);
    c[0] = c[0] / length; c[1] = c[1] / length; c[2] = c[2] / length; c[3] = c[3] / length;
    const float mt[3] = {F->tcw[0] * -1.f, F->tcw[1] * -1.f, F->tcw[2] * -1.f};
    quat_rotate(c, mt, F->Ow);
}

// MapPoint::PredictScale(currentDist, Frame*).  The reference converts ceil()'s float to int unchecked; a NaN or a value outside
// int converts to INT_MIN on x86-64, which the clamp turns into level 0: restated, so that host and device agree.
TPJ_HD int predict_scale(float max_distance, float dist, float log_scale_factor, int n_levels)
{
    const float ratio = max_distance / dist;
    const float s = ceilf(logf(ratio) / log_scale_factor);
    int nScale = (s >= -2147483648.f && s < 2147483648.f) ? (int)s : (-2147483647 - 1);
    if (nScale < 0)
        nScale = 0;
    else if (nScale >= n_levels)
        nScale = n_levels - 1;
    return nScale;
}

struct Row {            // what one map point leaves behind
    int valid, level;
    float u, v, ur, view_cos, depth;
};

TPJ_HD Row row_none() { return Row{0, -1, -1.f, -1.f, 0.f, 0.f, 0.f}; }

// Frame::isInFrustum(pMP, viewingCosLimit), Nleft == -1
TPJ_HD Row frustum_row(const OrbmTrackCamera& C, const OrbmFramePose& F, const float* P, const float* Pn,
                       float min_distance_raw, float max_distance_raw, float viewingCosLimit)
{
    Row r = row_none();
    const float Pc0 = dot3(F.Rcw[0], F.Rcw[1], F.Rcw[2], P[0], P[1], P[2]) + F.tcw[0];
    const float Pc1 = dot3(F.Rcw[3], F.Rcw[4], F.Rcw[5], P[0], P[1], P[2]) + F.tcw[1];
    const float PcZ = dot3(F.Rcw[6], F.Rcw[7], F.Rcw[8], P[0], P[1], P[2]) + F.tcw[2];
    const float Pc_dist = norm3(Pc0, Pc1, PcZ);
    const float invz = 1.0f / PcZ;
    if (PcZ < 0.0f) return r;
    const float uv0 = C.fx * Pc0 / PcZ + C.cx;          // Pinhole::project
    const float uv1 = C.fy * Pc1 / PcZ + C.cy;
    if (uv0 < C.min_x || uv0 > C.max_x) return r;
    if (uv1 < C.min_y || uv1 > C.max_y) return r;
    r.u = uv0; r.v = uv1;
    const float maxDistance = 1.2f * max_distance_raw;
    const float minDistance = 0.8f * min_distance_raw;
    const float PO0 = P[0] - F.Ow[0], PO1 = P[1] - F.Ow[1], PO2 = P[2] - F.Ow[2];
    const float dist = norm3(PO0, PO1, PO2);
    if (dist < minDistance || dist > maxDistance) return r;
    const float viewCos = dot3(PO0, PO1, PO2, Pn[0], Pn[1], Pn[2]) / dist;
    if (viewCos < viewingCosLimit) return r;
    r.level = predict_scale(max_distance_raw, dist, C.log_scale_factor, C.n_levels);
    r.valid = 1;
    r.ur = uv0 - C.bf * invz;
    r.depth = Pc_dist;
    r.view_cos = viewCos;
    return r;
}

// src/ORBmatcher.cc:1703-1718 for one last-frame map point
TPJ_HD Row project_last_row(const OrbmTrackCamera& C, const OrbmFramePose& F, const float* x3Dw)
{
    Row r = row_none();
    float x3Dc[3];
    quat_rotate(F.q, x3Dw, x3Dc);                       // Tcw * x3Dw = so3 * p + translation
    x3Dc[0] = x3Dc[0] + F.tcw[0]; x3Dc[1] = x3Dc[1] + F.tcw[1]; x3Dc[2] = x3Dc[2] + F.tcw[2];
    const float invzc = (float)(1.0 / (double)x3Dc[2]);
    if (invzc < 0) return r;
    const float uv0 = C.fx * x3Dc[0] / x3Dc[2] + C.cx;
    const float uv1 = C.fy * x3Dc[1] / x3Dc[2] + C.cy;
    if (uv0 < C.min_x || uv0 > C.max_x) return r;
    if (uv1 < C.min_y || uv1 > C.max_y) return r;
    r.valid = 1;
    r.u = uv0; r.v = uv1;
    r.ur = uv0 - C.bf * invzc;
    return r;
}

}  // namespace tpj
