// Sim(3) group arithmetic of the pose-graph solver (essential_graph.inc, which includes this header itself), restating g2o::Sim3 (reference
// Thirdparty/g2o/g2o/types/sim3.h) and the Eigen formulas it relies on: exp (:70-142), log (:148-230), inverse (:233-236), the
// product (:266-272), map (:144-146); VertexSim3Expmap::oplusImpl and EdgeSim3::computeError (types_seven_dof_expmap.h:60-69,
// :106-114) and the numeric Jacobian of a binary edge (core/base_binary_edge.hpp:147-196).  A Sim3 is 8 doubles: the rotation
// quaternion x y z w (used as given: g2o::Sim3 never normalises it), the translation, the scale.  A tangent vector is
// (omega, upsilon, sigma).  Plain C++ behind DLM_FN: g++ compiles it for tests/test_posegraph_geometry.py.
#pragma once
#include "dense_lm_device.h"

namespace sim3g {

#ifndef __HIPCC__
using std::acos; using std::cos; using std::exp; using std::fabs; using std::log; using std::sin; using std::sqrt;
#endif

constexpr double kEps = 0.00001;                    // the branch threshold of exp and log (sim3.h:90, :165)
constexpr double kDelta = 1e-9;                     // numeric Jacobian step (base_binary_edge.hpp:147)
constexpr double kScalar = 1.0 / (2 * kDelta);      // (:148)
// one edge's record: Ji^T Ji, Ji^T Jj, Jj^T Jj (7 x 7 row-major each), -Ji^T e, -Jj^T e, chi2
constexpr int kRecHii = 0, kRecHij = 49, kRecHjj = 98, kRecBi = 147, kRecBj = 154, kRecChi = 161, kRec = 162;

DLM_FN void quat_rotate(const double* q, const double* v, double* out)      // Eigen QuaternionBase::_transformVector
{
    double ux = q[1] * v[2] - q[2] * v[1], uy = q[2] * v[0] - q[0] * v[2], uz = q[0] * v[1] - q[1] * v[0];
    ux += ux; uy += uy; uz += uz;
    out[0] = v[0] + q[3] * ux + (q[1] * uz - q[2] * uy);
    out[1] = v[1] + q[3] * uy + (q[2] * ux - q[0] * uz);
    out[2] = v[2] + q[3] * uz + (q[0] * uy - q[1] * ux);
}

DLM_FN void quat_to_R(const double* q, double* R)                           // Eigen QuaternionBase::toRotationMatrix
{
    const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1 - (tyy + tzz); R[1] = txy - twz;       R[2] = txz + twy;
    R[3] = txy + twz;       R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;       R[7] = tyz + twx;       R[8] = 1 - (txx + tyy);
}

DLM_FN void quat_from_R(const double* R, double* q)                         // Eigen Quaternion(Matrix3d)
{
    double t = R[0] + R[4] + R[8];
    if (t > 0) {
        t = sqrt(t + 1.0);
        q[3] = 0.5 * t;
        t = 0.5 / t;
        q[0] = (R[7] - R[5]) * t; q[1] = (R[2] - R[6]) * t; q[2] = (R[3] - R[1]) * t;
        return;
    }
    const int i = (R[8] > (R[4] > R[0] ? R[4] : R[0])) ? 2 : (R[4] > R[0] ? 1 : 0);
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = sqrt(R[i * 3 + i] - R[j * 3 + j] - R[k * 3 + k] + 1.0);
    double v[3];
    v[i] = 0.5 * t;
    t = 0.5 / t;
    q[3] = (R[k * 3 + j] - R[j * 3 + k]) * t;
    v[j] = (R[j * 3 + i] + R[i * 3 + j]) * t;
    v[k] = (R[k * 3 + i] + R[i * 3 + k]) * t;
    q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
}

DLM_FN void skew2(const double* om, double* O, double* O2)
{
    O[0] = 0; O[1] = -om[2]; O[2] = om[1]; O[3] = om[2]; O[4] = 0; O[5] = -om[0]; O[6] = -om[1]; O[7] = om[0]; O[8] = 0;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
}

// the coefficients of W = A Omega + B Omega^2 + C I that exp and log share (:92-135, :169-213); sn, cs = sin, cos of theta
DLM_FN void w_coefficients(double sigma, double s, bool small_angle, double theta, double sn, double cs, double& A, double& B, double& C)
{
    if (fabs(sigma) < kEps) {
        C = 1;
        if (small_angle) { A = 1. / 2.; B = 1. / 6.; }
        else { const double theta2 = theta * theta; A = (1 - cs) / theta2; B = (theta - sn) / (theta2 * theta); }
    } else {
        C = (s - 1) / sigma;
        const double sigma2 = sigma * sigma;
        if (small_angle) {
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, theta2 = theta * theta, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
}

// Sim3(const Vector7d& update)
DLM_FN void exp_map(const double* u, double* S)
{
    const double om[3] = {u[0], u[1], u[2]};
    const double sigma = u[6];
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    double O[9], O2[9], R[9];
    skew2(om, O, O2);
    const double s = exp(sigma);
    const bool small_angle = theta < kEps;
    double sn = 0, cs = 1;
    if (small_angle) {
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + O[i] + O2[i];       // (:99, :117)
    } else {
        sn = sin(theta); cs = cos(theta);
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * O[i] + b * O2[i];
    }
    double A, B, C;
    w_coefficients(sigma, s, small_angle, theta, sn, cs, A, B, C);
    quat_from_R(R, S);
    for (int i = 0; i < 3; i++) {
        double v = 0;
        for (int j = 0; j < 3; j++) v += ((A * O[i * 3 + j] + B * O2[i * 3 + j]) + ((i == j) ? C : 0.0)) * u[3 + j];
        S[4 + i] = v;
    }
    S[7] = s;
}

// x = W^-1 t as PartialPivLU does it (Eigen/src/LU/PartialPivLU.h, unblocked): per column the row of the largest magnitude
// becomes the pivot, the column below is divided by it, the trailing block takes the rank-1 update
DLM_FN void lu_solve3(double* W, const double* t, double* x)
{
    int perm[3] = {0, 1, 2};
    for (int k = 0; k < 3; k++) {
        int p = k;
        double best = fabs(W[perm[k] * 3 + k]);
        for (int r = k + 1; r < 3; r++) { const double v = fabs(W[perm[r] * 3 + k]); if (v > best) { best = v; p = r; } }
        const int tmp = perm[k]; perm[k] = perm[p]; perm[p] = tmp;
        const double piv = W[perm[k] * 3 + k];
        for (int r = k + 1; r < 3; r++) {
            double* row = W + perm[r] * 3;
            row[k] /= piv;
            for (int c = k + 1; c < 3; c++) row[c] -= row[k] * W[perm[k] * 3 + c];
        }
    }
    double y[3];
    for (int r = 0; r < 3; r++) {
        double v = t[perm[r]];
        for (int c = 0; c < r; c++) v -= W[perm[r] * 3 + c] * y[c];
        y[r] = v;
    }
    for (int r = 2; r >= 0; r--) {
        double v = y[r];
        for (int c = r + 1; c < 3; c++) v -= W[perm[r] * 3 + c] * x[c];
        x[r] = v / W[perm[r] * 3 + r];
    }
}

// Sim3::log.  margins (may be null): [0] = |sigma| - eps, [1] = (1 - eps) - d, the signed distances of the two branch
// conditions from their thresholds (what tests/posegraph_reference.py reports for its own evaluations)
DLM_FN void log_map(const double* S, double* u, double* margins = nullptr)
{
    const double s = S[7];
    const double sigma = log(s);
    double R[9];
    quat_to_R(S, R);
    const double d = 0.5 * (R[0] + R[4] + R[8] - 1);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};
    const bool small_angle = d > 1 - kEps;
    double om[3], theta = 0, sn = 0, cs = 1;
    if (small_angle) {
        for (int i = 0; i < 3; i++) om[i] = 0.5 * dR[i];
    } else {
        theta = acos(d);
        const double f = theta / (2 * sqrt(1 - d * d));
        for (int i = 0; i < 3; i++) om[i] = f * dR[i];
        sn = sin(theta); cs = cos(theta);
    }
    double A, B, C;
    w_coefficients(sigma, s, small_angle, theta, sn, cs, A, B, C);
    double O[9], O2[9], W[9];
    skew2(om, O, O2);
    for (int i = 0; i < 9; i++) W[i] = (A * O[i] + B * O2[i]) + ((i % 4 == 0) ? C : 0.0);
    lu_solve3(W, S + 4, u + 3);
    u[0] = om[0]; u[1] = om[1]; u[2] = om[2];
    u[6] = sigma;
    if (margins) { margins[0] = fabs(sigma) - kEps; margins[1] = (1 - kEps) - d; }
}

// Sim3::operator*: r = a.r * b.r, t = a.s * (a.r * b.t) + a.t, s = a.s * b.s
DLM_FN void mul(const double* a, const double* b, double* o)
{
    double rt[3];
    quat_rotate(a, b + 4, rt);
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    for (int i = 0; i < 3; i++) o[4 + i] = a[7] * rt[i] + a[4 + i];
    o[7] = a[7] * b[7];
}

// Sim3::inverse: (r*, r* ((-1/s) t), 1/s)
DLM_FN void inv(const double* a, double* o)
{
    const double m = -1. / a[7];
    const double v[3] = {m * a[4], m * a[5], m * a[6]};
    o[0] = -a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = a[3];
    quat_rotate(o, v, o + 4);
    o[7] = 1. / a[7];
}

// Sim3::map: s (r x) + t
DLM_FN void map(const double* S, const double* x, double* out)
{
    double r[3];
    quat_rotate(S, x, r);
    for (int i = 0; i < 3; i++) out[i] = S[7] * r[i] + S[4 + i];
}

// VertexSim3Expmap::oplusImpl: est <- exp(update) * est; with _fix_scale the update's seventh entry is zeroed before exp
DLM_FN void oplus(const double* est, const double* update, bool fix_scale, double* out)
{
    double u[7], E[8];
    for (int i = 0; i < 7; i++) u[i] = update[i];
    if (fix_scale) u[6] = 0;
    exp_map(u, E);
    mul(E, est, out);
}

// EdgeSim3::computeError: log(C * v0 * v1^-1)
DLM_FN void edge_error(const double* C, const double* Si, const double* Sj, double* e, double* margins = nullptr)
{
    double A[8], Ji[8], B[8];
    mul(C, Si, A);
    inv(Sj, Ji);
    mul(A, Ji, B);
    log_map(B, e, margins);
}

// the error with vertex `side` (0: vertex 0, 1: vertex 1) moved by +-delta along dimension dim (linearizeOplus, :152-197)
// dim < 0: nobody moves (the error itself)
DLM_FN void edge_error_perturbed(const double* C, const double* Si, const double* Sj, int side, int dim, bool minus, bool fix_scale, double* e)
{
    double add[7], P[8];
    const bool moved = dim >= 0;
    if (moved) {
        for (int i = 0; i < 7; i++) add[i] = (i == dim) ? (minus ? -kDelta : kDelta) : 0.0;
        oplus(side ? Sj : Si, add, fix_scale, P);
    }
    edge_error(C, (moved && !side) ? P : Si, (moved && side) ? P : Sj, e);
}

// entry o of an edge's record from J (7 rows x 14 columns, row-major: columns 0-6 vertex 0, 7-13 vertex 1; the columns of a
// fixed vertex are zero) and the error e.  The sums run over the error's components in order.
DLM_FN double record_entry(const double* J, const double* e, int o)
{
    double v = 0;
    if (o < kRecBi) {
        const int blk = o / 49, r = (o % 49) / 7, c = o % 7;
        const int ca = (blk == 2 ? 7 : 0) + r, cb = (blk == 0 ? 0 : 7) + c;
        for (int k = 0; k < 7; k++) v += J[k * 14 + ca] * J[k * 14 + cb];
    } else if (o < kRecChi) {
        const int ca = o - kRecBi;
        for (int k = 0; k < 7; k++) v += J[k * 14 + ca] * -e[k];
    } else {
        for (int k = 0; k < 7; k++) v += e[k] * e[k];
    }
    return v;
}

// one edge, serially: its error, numeric Jacobian and record (the kernel k_essg_linearize spreads the same calls over 32 lanes)
DLM_FN void edge_linearize(const double* C, const double* Si, const double* Sj, bool fixed_i, bool fixed_j, bool fix_scale,
                           double* e, double* J, double* rec)
{
    edge_error(C, Si, Sj, e);
    for (int i = 0; i < 98; i++) J[i] = 0;
    for (int side = 0; side < 2; side++) {
        if (side ? fixed_j : fixed_i) continue;
        for (int dim = 0; dim < 7; dim++) {
            double ep[7], em[7];
            edge_error_perturbed(C, Si, Sj, side, dim, false, fix_scale, ep);
            edge_error_perturbed(C, Si, Sj, side, dim, true, fix_scale, em);
            for (int k = 0; k < 7; k++) J[k * 14 + 7 * side + dim] = kScalar * (ep[k] - em[k]);
        }
    }
    for (int o = 0; o < kRec; o++) rec[o] = record_entry(J, e, o);
}

}  // namespace sim3g
