// The per-pair geometry of Frame::ComputeStereoFishEyeMatches (reference src/Frame.cc:1246-1286): KannalaBrandt8::unproject
// (src/CameraModels/KannalaBrandt8.cpp:116-143), project(Vector3f) (:67-93), Triangulate (:394-406) and TriangulateMatches
// (:306-375), restated for one (left key point, right key point) pair.  Plain C++ without device builtins, so that the same text
// is the body of k_fisheye_geometry (stereo_fisheye.hip), of the host check tests/fisheye_geometry_check.cpp and of the one-core
// baseline tools/fisheye_stereo_cpu.cpp.  Float expressions follow the reference's operation order (the library is built with
// -ffp-contract=off); only the null vector of Triangulate's 4x4 matrix is computed in double (nmp::null_vector).
//
// Transcendentals, as csrc/camera_kb8.h: tan, atan2, sin and cos are the float rounding of the f64 function of the float
// argument.  That is the correctly rounded float apart from double-rounding cases, glibc documents its float functions as
// within one ulp, and the host's and the device's f64 functions agree to an ulp of a double -- so host and device here, and the
// reference's libm calls, agree to one float ulp.
// The reference's unqualified cos(psi) / sin(psi) on a float psi (:81-82) resolve to the float overload where <cmath> declares
// ::cos(float), as libstdc++ does, and to the double function otherwise.  This header takes the FLOAT overload: r * cos(psi) is
// a float product.  The tolerance band of the tests covers the other reading.
#pragma once
#include <math.h>

#include "orbm_new_points_geometry.h"

#define KB8S_HD NMP_HD

namespace kb8s {

struct Cam { float fx, fy, cx, cy, k[4], precision; };      // mvParameters[0..7] and KannalaBrandt8::precision
struct Rig { Cam l, r; float R12[9], t12[3]; };             // mpCamera, mpCamera2, mRlr (row major), mtlr

// a rig from 30 floats: left fx fy cx cy k0..k3 precision, the same of the right, Rlr row major, tlr (the layout of the host programs' files)
KB8S_HD Rig rig_from_floats(const float* r)
{
    Rig g;
    Cam* cams[2] = {&g.l, &g.r};
    for (int c = 0; c < 2; c++) {
        const float* p = r + 9 * c;
        cams[c]->fx = p[0]; cams[c]->fy = p[1]; cams[c]->cx = p[2]; cams[c]->cy = p[3];
        for (int k = 0; k < 4; k++) cams[c]->k[k] = p[4 + k];
        cams[c]->precision = p[8];
    }
    for (int k = 0; k < 9; k++) g.R12[k] = r[18 + k];
    for (int k = 0; k < 3; k++) g.t12[k] = r[27 + k];
    return g;
}

KB8S_HD float tan_f(float x) { return (float)tan((double)x); }
KB8S_HD float sin_f(float x) { return (float)sin((double)x); }
KB8S_HD float cos_f(float x) { return (float)cos((double)x); }
KB8S_HD float atan2_f(float y, float x) { return (float)atan2((double)y, (double)x); }

// KannalaBrandt8::unproject: the ray (x, y, 1) of a pixel.  Newton on theta, at most 10 steps
KB8S_HD void unproject(const Cam& c, float u, float v, float* ray)
{
    const float pwx = (u - c.cx) / c.fx, pwy = (v - c.cy) / c.fy;
    float scale = 1.f;
    float theta_d = sqrtf(pwx * pwx + pwy * pwy);
    const float half_pi = (float)(3.1415926535897932384626433832795 / 2.0);     // CV_PI / 2.f, a double, through fmaxf's float parameter
    theta_d = fminf(fmaxf(-half_pi, theta_d), half_pi);
    if ((double)theta_d > 1e-8) {
        float theta = theta_d;
        for (int j = 0; j < 10; j++) {
            const float theta2 = theta * theta, theta4 = theta2 * theta2, theta6 = theta4 * theta2, theta8 = theta4 * theta4;
            const float k0_theta2 = c.k[0] * theta2, k1_theta4 = c.k[1] * theta4;
            const float k2_theta6 = c.k[2] * theta6, k3_theta8 = c.k[3] * theta8;
            const float theta_fix = (theta * (1 + k0_theta2 + k1_theta4 + k2_theta6 + k3_theta8) - theta_d) /
                                    (1 + 3 * k0_theta2 + 5 * k1_theta4 + 7 * k2_theta6 + 9 * k3_theta8);
            theta = theta - theta_fix;
            if (fabsf(theta_fix) < c.precision) break;
        }
        scale = tan_f(theta) / theta_d;
    }
    ray[0] = pwx * scale; ray[1] = pwy * scale; ray[2] = 1.f;
}

// KannalaBrandt8::project(const Eigen::Vector3f&)
KB8S_HD void project(const Cam& c, const float* X, float* uv)
{
    const float x2_plus_y2 = X[0] * X[0] + X[1] * X[1];
    const float theta = atan2_f(sqrtf(x2_plus_y2), X[2]);
    const float psi = atan2_f(X[1], X[0]);
    const float theta2 = theta * theta;
    const float theta3 = theta * theta2;
    const float theta5 = theta3 * theta2;
    const float theta7 = theta5 * theta2;
    const float theta9 = theta7 * theta2;
    const float r = theta + c.k[0] * theta3 + c.k[1] * theta5 + c.k[2] * theta7 + c.k[3] * theta9;
    uv[0] = c.fx * r * cos_f(psi) + c.cx;
    uv[1] = c.fy * r * sin_f(psi) + c.cy;
}

// KannalaBrandt8::Triangulate with Tcw1 = [I | 0], Tcw2 = [R21 | t21] (row major): the null vector of the float 4x4, rounded to
// float component by component (svd.matrixV() is a float matrix), then the float division by its last component
KB8S_HD void triangulate(float p1x, float p1y, float p2x, float p2y, const float* R21, const float* t21, float* x3D)
{
    float A[16];
    for (int c = 0; c < 4; c++) {
        const float t10 = c == 0 ? 1.f : 0.f, t11 = c == 1 ? 1.f : 0.f, t12 = c == 2 ? 1.f : 0.f;
        const float t20 = c < 3 ? R21[c] : t21[0], t21c = c < 3 ? R21[3 + c] : t21[1], t22 = c < 3 ? R21[6 + c] : t21[2];
        A[c] = p1x * t12 - t10;
        A[4 + c] = p1y * t12 - t11;
        A[8 + c] = p2x * t22 - t20;
        A[12 + c] = p2y * t22 - t21c;
    }
    double v[4];
    nmp::null_vector(A, v);
    const float h0 = (float)v[0], h1 = (float)v[1], h2 = (float)v[2], h3 = (float)v[3];
    x3D[0] = h0 / h3; x3D[1] = h1 / h3; x3D[2] = h2 / h3;
}

// KannalaBrandt8::TriangulateMatches(pCamera2, kp1, kp2, R12, t12, sigmaLevel, unc, p3D): -1 low parallax, -2 / -3 behind the
// left / right camera, -4 / -5 reprojection error in the left / right image, else z1 with p3D written.  sigma1 and sigma2 are
// the level sigma^2 of the two key points (src/Frame.cc:1275)
KB8S_HD float triangulate_matches(const Rig& g, float u1, float v1, float u2, float v2, float sigma1, float sigma2, float* p3D)
{
    float r1[3], r2[3], r21[3];
    unproject(g.l, u1, v1, r1);
    unproject(g.r, u2, v2, r2);
    for (int r = 0; r < 3; r++) r21[r] = nmp::dot3(g.R12[3 * r], g.R12[3 * r + 1], g.R12[3 * r + 2], r2[0], r2[1], r2[2]);
    const float cosParallaxRays = nmp::dot3(r1[0], r1[1], r1[2], r21[0], r21[1], r21[2]) /
                                  (nmp::norm3(r1[0], r1[1], r1[2]) * nmp::norm3(r21[0], r21[1], r21[2]));
    if ((double)cosParallaxRays > 0.9998) return -1.f;

    float R21[9], t21[3];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) R21[3 * r + c] = g.R12[3 * c + r];
    for (int r = 0; r < 3; r++) t21[r] = nmp::dot3(-R21[3 * r], -R21[3 * r + 1], -R21[3 * r + 2], g.t12[0], g.t12[1], g.t12[2]);   // -R21 * t12
    float x3D[3];
    triangulate(r1[0], r1[1], r2[0], r2[1], R21, t21, x3D);

    const float z1 = x3D[2];
    if (z1 <= 0) return -2.f;
    const float z2 = nmp::dot3(R21[6], R21[7], R21[8], x3D[0], x3D[1], x3D[2]) + t21[2];
    if (z2 <= 0) return -3.f;

    float uv1[2];
    project(g.l, x3D, uv1);
    const float errX1 = uv1[0] - u1, errY1 = uv1[1] - v1;
    if ((double)(errX1 * errX1 + errY1 * errY1) > 5.991 * (double)sigma1) return -4.f;

    float x3D2[3], uv2[2];
    for (int r = 0; r < 3; r++) x3D2[r] = nmp::dot3(R21[3 * r], R21[3 * r + 1], R21[3 * r + 2], x3D[0], x3D[1], x3D[2]) + t21[r];
    project(g.r, x3D2, uv2);
    const float errX2 = uv2[0] - u2, errY2 = uv2[1] - v2;
    if ((double)(errX2 * errX2 + errY2 * errY2) > 5.991 * (double)sigma2) return -5.f;

    p3D[0] = x3D[0]; p3D[1] = x3D[1]; p3D[2] = x3D[2];
    return z1;
}

// Lowe's ratio of src/Frame.cc:1271 on two Hamming distances: cv::DMatch::distance is a float, 0.7 a double
KB8S_HD bool ratio_ok(int d0, int d1) { return (double)(float)d0 < (double)(float)d1 * 0.7; }

}  // namespace kb8s
