// camera_kb8.h -- the Kannala-Brandt fisheye camera (reference src/CameraModels/KannalaBrandt8.cpp) for the edge bodies of
// lba_solver.hip and pose_solver.hip: project(Vector3d) (:46-65) and projectJac (:145-175), restated in the reference's operation
// order (the library is built with -ffp-contract=off).  Device only.
//
// The reference evaluates theta and psi of project() with the host's atan2f / sqrtf on float-rounded arguments.  Here both
// arctangents are the float rounding of the f64 atan2 of the float-rounded arguments: that is the correctly rounded float apart
// from double-rounding cases, which stay within one ulp, and glibc documents atan2f as within one ulp -- so theta and psi differ
// from the host's by at most one float ulp.  (The device's own atan2f has a looser bound and is not used.)  The square root is
// the float rounding of the f64 square root of a float, which is the IEEE float square root exactly (53 >= 2 * 24 + 2).
#pragma once
#include <hip/hip_runtime.h>

namespace kb8 {

struct Cam { double fx, fy, cx, cy, k[4]; };       // mvParameters[0..7], floats promoted to double (OrbxKB8 of the C ABI)

__device__ __forceinline__ double atan2_as_float(float y, float x) { return (double)(float)atan2((double)y, (double)x); }

// KannalaBrandt8::project(const Eigen::Vector3d&): uv[2]
__device__ __forceinline__ void project(const Cam& c, const double* X, double* uv)
{
    const double x2_plus_y2 = X[0] * X[0] + X[1] * X[1];
    const float rho = (float)sqrt((double)(float)x2_plus_y2);               // sqrtf(x2_plus_y2)
    const double theta = atan2_as_float(rho, (float)X[2]);
    const double psi = atan2_as_float((float)X[1], (float)X[0]);
    const double theta2 = theta * theta;
    const double theta3 = theta * theta2;
    const double theta5 = theta3 * theta2;
    const double theta7 = theta5 * theta2;
    const double theta9 = theta7 * theta2;
    const double r = theta + c.k[0] * theta3 + c.k[1] * theta5 + c.k[2] * theta7 + c.k[3] * theta9;
    uv[0] = c.fx * r * cos(psi) + c.cx;
    uv[1] = c.fy * r * sin(psi) + c.cy;
}

// KannalaBrandt8::projectJac: J[6] = the 2 x 3 matrix, row major.  All double; the divisions by r2 and r3 make the optical axis
// singular here as in the reference.
__device__ __forceinline__ void project_jac(const Cam& c, const double* X, double* J)
{
    const double x2 = X[0] * X[0], y2 = X[1] * X[1], z2 = X[2] * X[2];
    const double r2 = x2 + y2;
    const double r = sqrt(r2);
    const double r3 = r2 * r;
    const double theta = atan2(r, X[2]);
    const double theta2 = theta * theta, theta3 = theta2 * theta;
    const double theta4 = theta2 * theta2, theta5 = theta4 * theta;
    const double theta6 = theta2 * theta4, theta7 = theta6 * theta;
    const double theta8 = theta4 * theta4, theta9 = theta8 * theta;
    const double f = theta + theta3 * c.k[0] + theta5 * c.k[1] + theta7 * c.k[2] + theta9 * c.k[3];
    const double fd = 1 + 3 * c.k[0] * theta2 + 5 * c.k[1] * theta4 + 7 * c.k[2] * theta6 + 9 * c.k[3] * theta8;
    J[0] = c.fx * (fd * X[2] * x2 / (r2 * (r2 + z2)) + f * y2 / r3);
    J[3] = c.fy * (fd * X[2] * X[1] * X[0] / (r2 * (r2 + z2)) - f * X[1] * X[0] / r3);
    J[1] = c.fx * (fd * X[2] * X[1] * X[0] / (r2 * (r2 + z2)) - f * X[1] * X[0] / r3);
    J[4] = c.fy * (fd * X[2] * y2 / (r2 * (r2 + z2)) + f * x2 / r3);
    J[2] = -c.fx * fd * X[0] / (r2 + z2);
    J[5] = -c.fy * fd * X[1] / (r2 + z2);
}

// -projectJac(Xc) * [0 z -y 1 0 0; -z 0 x 0 1 0; y -x 0 0 0 1]: the two pose rows of EdgeSE3ProjectXYZ(OnlyPose)::linearizeOplus,
// Jj[12] row major; N[6] receives -projectJac for the caller's point Jacobian
__device__ __forceinline__ void pose_rows(const Cam& c, const double* Xc, double* N, double* Jj)
{
    double J[6];
    project_jac(c, Xc, J);
    for (int k = 0; k < 6; k++) N[k] = -J[k];
    const double x = Xc[0], y = Xc[1], z = Xc[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const double a0 = N[3 * q], a1 = N[3 * q + 1], a2 = N[3 * q + 2];
        Jj[6 * q + 0] = a1 * (-z) + a2 * y;
        Jj[6 * q + 1] = a0 * z + a2 * (-x);
        Jj[6 * q + 2] = a0 * (-y) + a1 * x;
        Jj[6 * q + 3] = a0; Jj[6 * q + 4] = a1; Jj[6 * q + 5] = a2;
    }
}

// ---- a rig of two such cameras: the right-camera edges EdgeSE3ProjectXYZOnlyPoseToBody / EdgeSE3ProjectXYZToBody
// (src/OptimizableTypes.cpp:91-107, 192-213): error obs - right.project(X_r), X_r = Trl X_l; pose Jacobian
// -right.projectJac(X_r) R_rl SE3deriv(X_l); point Jacobian -right.projectJac(X_r) R_rl R_lw ----
struct Rig {
    Cam left, right;                    // mpCamera, mpCamera2
    double R_rl[9], t_rl[3];            // GetRelativePoseTrl(), the rotation row major
    const uint8_t* kind;                // LBA: [nE] camera of an edge, 0 left, else right (the pose solver reads the problem's stereo byte)
    const uint8_t* const* kind_tab;     // batched LBA: the kind array of window w at kind_tab[w]
};
struct RigEdge { const Rig& g; bool right; };      // the camera argument of one edge

// The camera and the camera-frame point of one edge, by selection: a wave that holds left and right edges then makes ONE pass through
// the f64 atan2 / sincos / polynomial code of project and project_jac instead of two under divergence.  A left edge gets the left
// camera and X_l untouched, so it computes what the monocular kb8 edge computes, bit for bit.
__device__ __forceinline__ void rig_select(const Rig& g, bool right, const double* Xl, Cam& c, double* Xp)
{
    c.fx = right ? g.right.fx : g.left.fx; c.fy = right ? g.right.fy : g.left.fy;
    c.cx = right ? g.right.cx : g.left.cx; c.cy = right ? g.right.cy : g.left.cy;
#pragma unroll
    for (int k = 0; k < 4; k++) c.k[k] = right ? g.right.k[k] : g.left.k[k];
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const double xr = g.R_rl[3 * a] * Xl[0] + g.R_rl[3 * a + 1] * Xl[1] + g.R_rl[3 * a + 2] * Xl[2] + g.t_rl[a];
        Xp[a] = right ? xr : Xl[a];
    }
}

// project of the edge's own camera; Xp[3] receives the point in that camera's frame (isDepthPositive reads Xp[2])
__device__ __forceinline__ void rig_project(const Rig& g, bool right, const double* Xl, double* Xp, double* uv)
{
    Cam c;
    rig_select(g, right, Xl, c, Xp);
    project(c, Xp, uv);
}

// N[6] = -projectJac(Xp), times R_rl on a right edge; Jj[12] = N * SE3deriv(X_l).  The caller's point Jacobian is N * R_lw for both kinds.
__device__ __forceinline__ void rig_pose_rows(const Rig& g, bool right, const double* Xl, double* N, double* Jj)
{
    Cam c;
    double Xp[3], J[6];
    rig_select(g, right, Xl, c, Xp);
    project_jac(c, Xp, J);
    for (int k = 0; k < 6; k++) N[k] = -J[k];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const double a0 = N[3 * q], a1 = N[3 * q + 1], a2 = N[3 * q + 2];
#pragma unroll
        for (int k = 0; k < 3; k++) {
            const double m = a0 * g.R_rl[k] + a1 * g.R_rl[3 + k] + a2 * g.R_rl[6 + k];
            N[3 * q + k] = right ? m : N[3 * q + k];
        }
    }
    const double x = Xl[0], y = Xl[1], z = Xl[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const double a0 = N[3 * q], a1 = N[3 * q + 1], a2 = N[3 * q + 2];
        Jj[6 * q + 0] = a1 * (-z) + a2 * y;
        Jj[6 * q + 1] = a0 * z + a2 * (-x);
        Jj[6 * q + 2] = a0 * (-y) + a1 * x;
        Jj[6 * q + 3] = a0; Jj[6 * q + 4] = a1; Jj[6 * q + 5] = a2;
    }
}

}  // namespace kb8
