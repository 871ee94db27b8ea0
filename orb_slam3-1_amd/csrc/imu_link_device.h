// SO(3) helpers (3x3 row major) and the bias-corrected deltas of a pre-integrated link, shared by the inertial solvers
// (inertial_solver.inc) and the IMU initialisation (imu_init_group.h); g++ compiles the same text for the CPU side of a timing tool.
#pragma once
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#else           // a host build (g++) of the same text
#include <cmath>
#endif

#include "../../include/orbslam3_hip.h"

#ifdef __HIPCC__
#define IML_FN __device__ inline
#else
#define IML_FN inline
#endif

namespace liba {

#ifndef __HIPCC__
using std::acos; using std::cos; using std::fabs; using std::fmax; using std::isfinite; using std::sin; using std::sqrt;
#endif

// ---- small dense helpers (3x3 row major) ----
IML_FN void mmul(const double* A, const double* B, double* C)
{
    double t[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) t[3 * i + j] = A[3 * i] * B[j] + A[3 * i + 1] * B[3 + j] + A[3 * i + 2] * B[6 + j];
#pragma unroll
    for (int k = 0; k < 9; k++) C[k] = t[k];
}
IML_FN void mtr(const double* A, double* T)
{
    double t[9];
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) t[3 * i + j] = A[3 * j + i];
#pragma unroll
    for (int k = 0; k < 9; k++) T[k] = t[k];
}
IML_FN void mvec(const double* A, const double* v, double* o)
{
    const double t0 = A[0] * v[0] + A[1] * v[1] + A[2] * v[2], t1 = A[3] * v[0] + A[4] * v[1] + A[5] * v[2], t2 = A[6] * v[0] + A[7] * v[1] + A[8] * v[2];
    o[0] = t0; o[1] = t1; o[2] = t2;
}
IML_FN bool minv3(const double* A, double* Ai)
{
    const double c00 = A[4] * A[8] - A[5] * A[7], c01 = A[5] * A[6] - A[3] * A[8], c02 = A[3] * A[7] - A[4] * A[6];
    const double det = A[0] * c00 + A[1] * c01 + A[2] * c02;
    if (det == 0.0 || !isfinite(det)) return false;
    const double id = 1.0 / det;
    Ai[0] = c00 * id; Ai[1] = (A[2] * A[7] - A[1] * A[8]) * id; Ai[2] = (A[1] * A[5] - A[2] * A[4]) * id;
    Ai[3] = c01 * id; Ai[4] = (A[0] * A[8] - A[2] * A[6]) * id; Ai[5] = (A[2] * A[3] - A[0] * A[5]) * id;
    Ai[6] = c02 * id; Ai[7] = (A[1] * A[6] - A[0] * A[7]) * id; Ai[8] = (A[0] * A[4] - A[1] * A[3]) * id;
    return true;
}
// NormalizeRotation (G2oTypes.h:67-71: U V^T of the SVD) = the orthogonal polar factor, by Newton iteration
IML_FN void normalize_rotation(double* R)
{
    for (int it = 0; it < 6; it++) {
        double Ri[9], Rit[9];
        if (!minv3(R, Ri)) return;
        mtr(Ri, Rit);
        double delta = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) { const double n = 0.5 * (R[k] + Rit[k]); delta = fmax(delta, fabs(n - R[k])); R[k] = n; }
        if (delta < 1e-16) break;
    }
}
IML_FN void skew3(const double* w, double* W) { W[0] = 0; W[1] = -w[2]; W[2] = w[1]; W[3] = w[2]; W[4] = 0; W[5] = -w[0]; W[6] = -w[1]; W[7] = w[0]; W[8] = 0; }
IML_FN void exp_so3(const double* w, double* R)             // G2oTypes.cc:782-798
{
    const double d2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2], d = sqrt(d2);
    double W[9], W2[9];
    skew3(w, W);
    mmul(W, W, W2);
    const double a = d < 1e-5 ? 1.0 : sin(d) / d, b = d < 1e-5 ? 0.5 : (1.0 - cos(d)) / d2;
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = ((k % 4 == 0) ? 1.0 : 0.0) + W[k] * a + W2[k] * b;
    normalize_rotation(R);
}
IML_FN void log_so3(const double* R, double* w)             // :800-814
{
    const double tr = R[0] + R[4] + R[8];
    w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
    const double costheta = (tr - 1.0) * 0.5f;
    if (costheta > 1 || costheta < -1) return;
    const double theta = acos(costheta), s = sin(theta);
    if (fabs(s) < 1e-5) return;
#pragma unroll
    for (int k = 0; k < 3; k++) w[k] = theta * w[k] / s;
}
IML_FN void inv_right_jac(const double* v, double* J)       // :821-832
{
    const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
    double W[9], W2[9];
    skew3(v, W);
    mmul(W, W, W2);
#pragma unroll
    for (int k = 0; k < 9; k++) J[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (d < 1e-5) return;
    const double c = 1.0 / d2 - (1.0 + cos(d)) / (2.0 * d * sin(d));
#pragma unroll
    for (int k = 0; k < 9; k++) J[k] += W[k] / 2 + W2[k] * c;
}
IML_FN void right_jac(const double* v, double* J)           // :839-854
{
    const double d2 = v[0] * v[0] + v[1] * v[1] + v[2] * v[2], d = sqrt(d2);
    double W[9], W2[9];
    skew3(v, W);
    mmul(W, W, W2);
#pragma unroll
    for (int k = 0; k < 9; k++) J[k] = (k % 4 == 0) ? 1.0 : 0.0;
    if (d < 1e-5) return;
    const double a = (1.0 - cos(d)) / d2, b = (d - sin(d)) / (d2 * d);
#pragma unroll
    for (int k = 0; k < 9; k++) J[k] += -W[k] * a + W2[k] * b;
}

// Preintegrated::GetDelta*(b) (ImuTypes.cc:276-307) at the bias (bg, ba): FLOAT expressions on a FLOAT bias; the float product
// dR * exp is re-orthonormalised and rounded to float as in the oracle
IML_FN void link_delta(const LibaLink& L, const double* bg, const double* ba, double* dR, double* dV, double* dP, double* dbg_out)
{
    float dbg[3], dba[3];
    for (int i = 0; i < 3; i++) { dbg[i] = (float)bg[i] - L.bias0[3 + i]; dba[i] = (float)ba[i] - L.bias0[i]; }
    float w[3];
    for (int i = 0; i < 3; i++) w[i] = L.JRg[3 * i] * dbg[0] + L.JRg[3 * i + 1] * dbg[1] + L.JRg[3 * i + 2] * dbg[2];
    const double wd[3] = {w[0], w[1], w[2]};
    const double th2 = wd[0] * wd[0] + wd[1] * wd[1] + wd[2] * wd[2], th = sqrt(th2);
    const double imag = th < 1e-5 ? 0.5 - th2 / 48.0 : sin(0.5 * th) / th, real = th < 1e-5 ? 1.0 - th2 / 8.0 : cos(0.5 * th);
    const double qx = imag * wd[0], qy = imag * wd[1], qz = imag * wd[2], qw = real;
    float E[9];
    E[0] = (float)(1 - 2 * (qy * qy + qz * qz)); E[1] = (float)(2 * (qx * qy - qz * qw)); E[2] = (float)(2 * (qx * qz + qy * qw));
    E[3] = (float)(2 * (qx * qy + qz * qw)); E[4] = (float)(1 - 2 * (qx * qx + qz * qz)); E[5] = (float)(2 * (qy * qz - qx * qw));
    E[6] = (float)(2 * (qx * qz - qy * qw)); E[7] = (float)(2 * (qy * qz + qx * qw)); E[8] = (float)(1 - 2 * (qx * qx + qy * qy));
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) dR[3 * i + j] = (double)(L.dR[3 * i] * E[j] + L.dR[3 * i + 1] * E[3 + j] + L.dR[3 * i + 2] * E[6 + j]);
    normalize_rotation(dR);
    for (int k = 0; k < 9; k++) dR[k] = (double)(float)dR[k];
    for (int i = 0; i < 3; i++) {
        const float dv = L.dV[i] + (L.JVg[3 * i] * dbg[0] + L.JVg[3 * i + 1] * dbg[1] + L.JVg[3 * i + 2] * dbg[2]) +
                         (L.JVa[3 * i] * dba[0] + L.JVa[3 * i + 1] * dba[1] + L.JVa[3 * i + 2] * dba[2]);
        const float dp = L.dP[i] + (L.JPg[3 * i] * dbg[0] + L.JPg[3 * i + 1] * dbg[1] + L.JPg[3 * i + 2] * dbg[2]) +
                         (L.JPa[3 * i] * dba[0] + L.JPa[3 * i + 1] * dba[1] + L.JPa[3 * i + 2] * dba[2]);
        dV[i] = dv; dP[i] = dp;
    }
    for (int i = 0; i < 3; i++) dbg_out[i] = dbg[i];
}

}  // namespace liba
