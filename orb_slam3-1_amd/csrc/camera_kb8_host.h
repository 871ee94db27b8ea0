// camera_kb8_host.h -- host side of the KannalaBrandt8 rig (OrbxKB8Rig of the C ABI -> kb8::Rig of the kernels), shared by
// pose_solver.hip and lba_solver.hip.  The checks of the setters are made here, before anything touches a device.
#pragma once
#include <cmath>

#include "../../include/orbslam3_hip.h"
#include "camera_kb8.h"
#include "hip_check.h"

namespace kb8 {

inline void cam_from_abi(const OrbxKB8& a, Cam* c)
{
    c->fx = a.fx; c->fy = a.fy; c->cx = a.cx; c->cy = a.cy;
    for (int k = 0; k < 4; k++) c->k[k] = a.k[k];
}

// q_rl is normalised as the g2o::SE3Quat constructor normalises it (w made non-negative, divided by the norm) and turned into the
// rotation matrix with Eigen's toRotationMatrix expressions
inline int rig_from_abi(const OrbxKB8Rig* rig, Rig* out)
{
    if (!(rig->left.fx > 0) || !(rig->left.fy > 0) || !(rig->right.fx > 0) || !(rig->right.fy > 0))
        return fail(ORBX_ERR_ARG, "KannalaBrandt8 focal lengths must be positive in both cameras of a rig");
    double q[4] = {rig->q_rl[0], rig->q_rl[1], rig->q_rl[2], rig->q_rl[3]};
    const double nrm = std::sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
    if (!(nrm > 0) || !std::isfinite(nrm)) return fail(ORBX_ERR_ARG, "the rig's quaternion q_rl has zero or non-finite norm");
    for (int k = 0; k < 3; k++)
        if (!std::isfinite(rig->t_rl[k])) return fail(ORBX_ERR_ARG, "the rig's translation t_rl is not finite");
    if (q[3] < 0) for (int k = 0; k < 4; k++) q[k] = -q[k];
    for (int k = 0; k < 4; k++) q[k] /= nrm;
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double tx = 2 * x, ty = 2 * y, tz = 2 * z;
    const double twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x, tyy = ty * y, tyz = tz * y, tzz = tz * z;
    cam_from_abi(rig->left, &out->left);
    cam_from_abi(rig->right, &out->right);
    double* R = out->R_rl;
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
    for (int k = 0; k < 3; k++) out->t_rl[k] = rig->t_rl[k];
    out->kind = nullptr; out->kind_tab = nullptr;
    return ORBX_OK;
}

// The camera of a solver handle: pinhole (the figures every problem brings) until a setter names a fisheye camera or a rig of two.
// NULL resets to pinhole, the last setter wins, a refused argument leaves the choice as it was.
struct CameraChoice {
    enum Kind { kPinhole, kFisheye, kRig } kind = kPinhole;
    Cam cam;
    Rig rig;        // (rig.kind / rig.kind_tab: the per-edge cameras of an LBA window, filled in by its shard / its batch)
    int set(const OrbxKB8* a)
    {
        if (!a) { kind = kPinhole; return ORBX_OK; }
        if (!(a->fx > 0) || !(a->fy > 0)) return fail(ORBX_ERR_ARG, "KannalaBrandt8 focal lengths must be positive");
        cam_from_abi(*a, &cam);
        kind = kFisheye;
        return ORBX_OK;
    }
    int set(const OrbxKB8Rig* a)
    {
        if (!a) { kind = kPinhole; return ORBX_OK; }
        Rig g;
        if (int r = rig_from_abi(a, &g)) return r;
        rig = g;
        kind = kRig;
        return ORBX_OK;
    }
};

// f() for the pinhole camera, f(cam) for the fisheye one, f(rig) for the rig: a launch site passes a generic lambda over a pack,
// [&](auto... cam) { hipLaunchKernelGGL((k<decltype(cam)...>), ..., cam..., ...); }
template <class F>
inline void with_camera(const CameraChoice& c, F&& f)
{
    switch (c.kind) {
    case CameraChoice::kFisheye: f(c.cam); break;
    case CameraChoice::kRig: f(c.rig); break;
    default: f();
    }
}

}  // namespace kb8
