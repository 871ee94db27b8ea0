// Yaw + translation pose arithmetic of the 4-DoF pose-graph solver (essential_graph_4dof.inc), restating what
// Optimizer::OptimizeEssentialGraph4DoF relies on (reference src/G2oTypes.cc): ExpSO3 (:782-798), LogSO3 (:800-814),
// ImuCamPose::UpdateW (:222-256) as VertexPose4DoF::oplusImpl calls it (include/G2oTypes.h:178-188), Edge4DoF::computeError
// (:831-836) and the numeric Jacobian of a binary edge (g2o core/base_binary_edge.hpp:147-196) with an information matrix.
// UpdateW only ever multiplies DR by ExpSO3(0, 0, z), whose result is block diagonal with exact zeros and an exact one, so DR is a
// rotation about z and is carried as its (cos, sin) pair.  Plain C++ behind DLM_FN: g++ compiles it for tools/posegraph_cpu.cpp.
#pragma once
#include "dense_lm_device.h"

namespace p4g {

#ifndef __HIPCC__
using std::acos; using std::cos; using std::fabs; using std::sin; using std::sqrt;
#endif

constexpr double kDelta = 1e-9;                     // numeric Jacobian step (base_binary_edge.hpp:147)
constexpr double kScalar = 1.0 / (2 * kDelta);      // (:148)
// a vertex's estimate: DR as (cos, sin), twb, the number of accepted updates since the last clean-up of DR (its), Rcw[0], tcw[0]
constexpr int kC = 0, kS = 1, kTwb = 2, kIts = 5, kRcw = 6, kTcw = 15, kState = 18;
// what an update leaves alone: Rwb0, Rcb, tcb
constexpr int kRwb0 = 0, kRcb = 9, kTcb = 18, kConst = 21;
// one edge's record: Ji^T W Ji, Ji^T W Jj, Jj^T W Jj (4 x 4 row-major each), -Ji^T W e, -Jj^T W e, e^T W e
constexpr int kRecHii = 0, kRecHij = 16, kRecHjj = 32, kRecBi = 48, kRecBj = 52, kRecChi = 56, kRec = 57;

// ExpSO3(0, 0, z) as (cos, sin): the upper-left block [[a, -b], [b, a]] of I + W + W^2 / 2 (d < 1e-5) or of Rodrigues' formula,
// then NormalizeRotation -- the nearest rotation of a scaled rotation is the block divided by its norm
DLM_FN void exp_z(double z, double& c, double& s)
{
    const double d2 = z * z, d = sqrt(d2);
    double a, b;
    if (d < 1e-5) { a = 1.0 + 0.5 * -d2; b = z; }
    else { a = 1.0 + (-d2 * (1.0 - cos(d))) / d2; b = (z * sin(d)) / d; }
    const double nrm = sqrt(a * a + b * b);
    c = a / nrm; s = b / nrm;
}

// LogSO3 with both early returns: costheta outside [-1, 1], |sin theta| < 1e-5
DLM_FN void log_so3(const double* R, double* w)
{
    const double tr = R[0] + R[4] + R[8];
    w[0] = (R[7] - R[5]) / 2; w[1] = (R[2] - R[6]) / 2; w[2] = (R[3] - R[1]) / 2;
    const double costheta = (tr - 1.0) * 0.5;
    if (costheta > 1 || costheta < -1) return;
    const double theta = acos(costheta);
    const double s = sin(theta);
    if (fabs(s) < 1e-5) return;
    for (int i = 0; i < 3; i++) w[i] = theta * w[i] / s;
}

// the camera pose of UpdateW's last lines: Rwb = DR Rwb0, Rbw = Rwb^T, tbw = -Rbw twb, Rcw = Rcb Rbw, tcw = Rcb tbw + tcb
DLM_FN void camera_pose(double c, double s, const double* twb, const double* K, double* Rcw, double* tcw)
{
    const double* R0 = K + kRwb0;
    const double* Rcb = K + kRcb;
    double Rwb[9], tbw[3];
    for (int j = 0; j < 3; j++) { Rwb[j] = c * R0[j] - s * R0[3 + j]; Rwb[3 + j] = s * R0[j] + c * R0[3 + j]; Rwb[6 + j] = R0[6 + j]; }
    for (int i = 0; i < 3; i++) tbw[i] = -(Rwb[i] * twb[0] + Rwb[3 + i] * twb[1] + Rwb[6 + i] * twb[2]);
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) Rcw[3 * i + j] = Rcb[3 * i] * Rwb[3 * j] + Rcb[3 * i + 1] * Rwb[3 * j + 1] + Rcb[3 * i + 2] * Rwb[3 * j + 2];
        tcw[i] = (Rcb[3 * i] * tbw[0] + Rcb[3 * i + 1] * tbw[1] + Rcb[3 * i + 2] * tbw[2]) + K[kTcb + i];
    }
}

// VertexPose4DoF::oplusImpl(u = yaw, tx, ty, tz): UpdateW with ur = (0, 0, u0), ut = (u1, u2, u3).  The camera pose comes from
// the DR of before the clean-up, as there; every fifth update zeroes DR's off-block entries (they are zero) and replaces its block
// [[p, q], [r, s]] by the nearest rotation [[p + s, q - r], [r - q, p + s]] / norm.
DLM_FN void oplus(const double* X, const double* K, const double* u, double* out)
{
    double dc, ds;
    exp_z(u[0], dc, ds);
    double c = dc * X[kC] - ds * X[kS], s = ds * X[kC] + dc * X[kS];
    for (int i = 0; i < 3; i++) out[kTwb + i] = X[kTwb + i] + u[1 + i];
    camera_pose(c, s, out + kTwb, K, out + kRcw, out + kTcw);
    double its = X[kIts] + 1;
    if (its >= 5) {
        const double a = c + c, b = s + s, nrm = sqrt(a * a + b * b);
        c = a / nrm; s = b / nrm;
        its = 0;
    }
    out[kC] = c; out[kS] = s; out[kIts] = its;
}

// Edge4DoF::computeError: LogSO3(Ri Rj^T dRij^T), Ri (-Rj^T tj) + ti - dtij; M = dRij[9], dtij[3]
DLM_FN void edge_error(const double* M, const double* Ri, const double* ti, const double* Rj, const double* tj, double* e)
{
    double A[9], B[9], v[3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) A[3 * i + j] = Ri[3 * i] * Rj[3 * j] + Ri[3 * i + 1] * Rj[3 * j + 1] + Ri[3 * i + 2] * Rj[3 * j + 2];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) B[3 * i + j] = A[3 * i] * M[3 * j] + A[3 * i + 1] * M[3 * j + 1] + A[3 * i + 2] * M[3 * j + 2];
    log_so3(B, e);
    for (int i = 0; i < 3; i++) v[i] = -(Rj[i] * tj[0] + Rj[3 + i] * tj[1] + Rj[6 + i] * tj[2]);
    for (int i = 0; i < 3; i++) e[3 + i] = (Ri[3 * i] * v[0] + Ri[3 * i + 1] * v[1] + Ri[3 * i + 2] * v[2]) + ti[i] - M[9 + i];
}

// the error with vertex `side` moved by +-delta along dimension dim (linearizeOplus), dim < 0: nobody moves.  The vertex that
// does not move contributes its stored Rcw / tcw; the one that moves the pose UpdateW recomputes from (DR, Rwb0, twb, Rcb, tcb).
DLM_FN void edge_error_perturbed(const double* M, const double* Xi, const double* Ki, const double* Xj, const double* Kj, int side, int dim, bool minus, double* e)
{
    if (dim < 0) { edge_error(M, Xi + kRcw, Xi + kTcw, Xj + kRcw, Xj + kTcw, e); return; }
    double u[4] = {0, 0, 0, 0}, P[kState];
    u[dim] = minus ? -kDelta : kDelta;
    oplus(side ? Xj : Xi, side ? Kj : Ki, u, P);
    if (side) edge_error(M, Xi + kRcw, Xi + kTcw, P + kRcw, P + kTcw, e);
    else edge_error(M, P + kRcw, P + kTcw, Xj + kRcw, Xj + kTcw, e);
}

// entry o of an edge's record from J (6 rows x 8 columns, row-major: columns 0-3 vertex 0, 4-7 vertex 1; the columns of a fixed
// vertex are zero), WJ = W J (6 x 8), the error e and We = W e.  The sums run over the error's components in order.
DLM_FN double record_entry(const double* J, const double* WJ, const double* e, const double* We, int o)
{
    double v = 0;
    if (o < kRecBi) {
        const int blk = o >> 4, r = (o >> 2) & 3, c = o & 3;
        const int ca = (blk == 2 ? 4 : 0) + r, cb = (blk == 0 ? 0 : 4) + c;
        for (int k = 0; k < 6; k++) v += J[k * 8 + ca] * WJ[k * 8 + cb];
    } else if (o < kRecChi) {
        const int ca = o - kRecBi;
        for (int k = 0; k < 6; k++) v += J[k * 8 + ca] * -We[k];
    } else {
        for (int k = 0; k < 6; k++) v += e[k] * We[k];
    }
    return v;
}

DLM_FN double weighted(const double* W, const double* col, int stride, int k)        // (W x)[k] for x[m] = col[m * stride]
{
    double v = 0;
    for (int m = 0; m < 6; m++) v += W[6 * k + m] * col[m * stride];
    return v;
}

// one edge, serially: its error, numeric Jacobian and record (k_essg4_linearize spreads the same calls over 32 lanes)
DLM_FN void edge_linearize(const double* M, const double* W, const double* Xi, const double* Ki, const double* Xj, const double* Kj,
                           bool fixed_i, bool fixed_j, double* rec)
{
    double e[6], We[6], J[48], WJ[48];
    edge_error_perturbed(M, Xi, Ki, Xj, Kj, 0, -1, false, e);
    for (int i = 0; i < 48; i++) J[i] = 0;
    for (int side = 0; side < 2; side++) {
        if (side ? fixed_j : fixed_i) continue;
        for (int dim = 0; dim < 4; dim++) {
            double ep[6], em[6];
            edge_error_perturbed(M, Xi, Ki, Xj, Kj, side, dim, false, ep);
            edge_error_perturbed(M, Xi, Ki, Xj, Kj, side, dim, true, em);
            for (int k = 0; k < 6; k++) J[k * 8 + 4 * side + dim] = kScalar * (ep[k] - em[k]);
        }
    }
    for (int k = 0; k < 6; k++) {
        We[k] = weighted(W, e, 1, k);
        for (int c = 0; c < 8; c++) WJ[k * 8 + c] = weighted(W, J + c, 8, k);
    }
    for (int o = 0; o < kRec; o++) rec[o] = record_entry(J, WJ, e, We, o);
}

// e^T W e
DLM_FN double chi2(const double* W, const double* e)
{
    double v = 0;
    for (int k = 0; k < 6; k++) v += e[k] * weighted(W, e, 1, k);
    return v;
}

}  // namespace p4g
