// sim3_solver.hip -- gfx950 kernels + C ABI for the geometry between the two loop-closing searches
// (LoopClosing::DetectCommonRegionsFromBoW, reference src/LoopClosing.cc:640-830): the RANSAC of Sim3Solver
// (src/Sim3Solver.cc:149-294 iterate, :311-412 ComputeSim3, :415-439 CheckInliers) and Optimizer::OptimizeSim3
// (src/Optimizer.cc:2115-2381; second half of this file).
//
// MI355X mapping: a problem is a few hundred correspondences and up to 300 independent three-point hypotheses, each scored
// against every correspondence.  ONE 256-thread workgroup runs a whole problem: the correspondences are staged once in LDS,
// phase A gives every hypothesis a LANE (Horn's closed form: ~4 k flops of straight-line code), phase B gives every
// hypothesis a WAVE (64 correspondences per step, __ballot delivers the 64 inlier bits as the output word, popcount counts),
// phase C is the selection rule.  A batch (one problem per candidate key frame / per client) is one launch.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbslam3_hip.h"
#include "batch_stage.h"
#include "dense_lm_device.h"
#include "se3_device.h"

namespace sim3 {

// LDS budget: 12 floats per correspondence (X1c, X2c, their pinhole projections, both thresholds) = 48 B; 1024 of them are
// 48 KiB, + 4 KiB of counts = 52 KiB of the 64 KiB a workgroup may declare statically (three workgroups fit the CU's 160 KiB).
// Problems with more correspondences read them from global memory (L2) instead -- same arithmetic, same results.
constexpr int kLdsN = SIM3_LDS_CORRESPONDENCES;
constexpr int kMaxHyp = SIM3_MAX_HYPOTHESES;

struct RansacDev {
    int32_t n, n_hyp, fix_scale, min_inliers;
    float K1[4], K2[4];                     // fx fy cx cy of key frame 1 / 2
    const float* X1; const float* X2; const float* e1; const float* e2;
    const int32_t* triples;
    int32_t* count; float* T12; unsigned long long* mask; int32_t* sel;
};

// GeometricCamera::project(Eigen::Vector3f) of a pinhole (src/CameraModels/Pinhole.cpp:43-49)
__device__ __forceinline__ void project(const float* K, const float* X, float* p)
{
    p[0] = K[0] * X[0] / X[2] + K[2];
    p[1] = K[1] * X[1] / X[2] + K[3];
}

// one Jacobi rotation of the symmetric 4x4 A in the (P, Q) plane, accumulated into V (columns = eigenvectors).
// Only + - * / sqrt; an exactly zero off-diagonal entry is skipped; a huge theta gives t = 0 through 1/inf.
template <int P, int Q>
__device__ __forceinline__ void jacobi_rot(double (&A)[4][4], double (&V)[4][4])
{
    const double apq = A[P][Q];
    if (apq == 0.0) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    const double app = A[P][P], aqq = A[Q][Q];
    A[P][P] = app - t * apq;
    A[Q][Q] = aqq + t * apq;
    A[P][Q] = 0.0; A[Q][P] = 0.0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        if (r != P && r != Q) {
            const double arp = A[r][P], arq = A[r][Q];
            const double np_ = c * arp - s * arq, nq = s * arp + c * arq;
            A[r][P] = np_; A[P][r] = np_;
            A[r][Q] = nq; A[Q][r] = nq;
        }
        const double vrp = V[r][P], vrq = V[r][Q];
        V[r][P] = c * vrp - s * vrq;
        V[r][Q] = s * vrp + c * vrq;
    }
}

constexpr int kJacobiSweeps = 8;    // a 4x4 converges quadratically: 6 sweeps reach double rounding, 8 leave a margin

// Sim3Solver::ComputeSim3 (src/Sim3Solver.cc:311-412) for the point triple a (key frame 1) / b (key frame 2).
// The inputs and the results (R, t, s) are float like the reference's; the closed form in between runs in DOUBLE.  The
// eigenvector of N is only as accurate as (rounding of N) / (eigen-gap): in float a triple with a gap of 7e-3 moved the
// error ratio of a correspondence by 1.6e-3 (the float run of the numpy reference: 1.2e-3), which no guard band of 1e-3
// around the inlier threshold absorbs; in double T12 is exact to the rounding of its float outputs whatever the gap, and
// 300 lanes of ~4 k f64 operations are not what the kernel's time goes to.
// The rotation is formed from the unit quaternion directly: the reference's atan2 + SO3::exp of 2*ang*axis (:362-368) is the
// same rotation, also when the eigenvector comes out negated (ang -> pi - ang, axis -> -axis).
__device__ __forceinline__ void horn(const float (&a)[3][3], const float (&b)[3][3], bool fix_scale, float* Rf, float* tf, float& sf)
{
    double O1[3], O2[3], A1[3][3], B2[3][3];    // [point][axis]
#pragma unroll
    for (int k = 0; k < 3; k++) {               // ComputeCentroid (:302-308)
        O1[k] = (((double)a[0][k] + (double)a[1][k]) + (double)a[2][k]) / 3.0;
        O2[k] = (((double)b[0][k] + (double)b[1][k]) + (double)b[2][k]) / 3.0;
#pragma unroll
        for (int p = 0; p < 3; p++) { A1[p][k] = (double)a[p][k] - O1[k]; B2[p][k] = (double)b[p][k] - O2[k]; }
    }
    double M[3][3];                             // M = Pr2 * Pr1^T (:328)
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = (B2[0][i] * A1[0][j] + B2[1][i] * A1[1][j]) + B2[2][i] * A1[2][j];
    double N[4][4];                             // (:335-349)
    N[0][0] = M[0][0] + M[1][1] + M[2][2];
    N[0][1] = M[1][2] - M[2][1];
    N[0][2] = M[2][0] - M[0][2];
    N[0][3] = M[0][1] - M[1][0];
    N[1][1] = M[0][0] - M[1][1] - M[2][2];
    N[1][2] = M[0][1] + M[1][0];
    N[1][3] = M[2][0] + M[0][2];
    N[2][2] = -M[0][0] + M[1][1] - M[2][2];
    N[2][3] = M[1][2] + M[2][1];
    N[3][3] = -M[0][0] - M[1][1] + M[2][2];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < i; j++) N[i][j] = N[j][i];
    double V[4][4];
#pragma unroll
    for (int i = 0; i < 4; i++)
#pragma unroll
        for (int j = 0; j < 4; j++) V[i][j] = (i == j) ? 1.0 : 0.0;
#pragma unroll 1
    for (int sweep = 0; sweep < kJacobiSweeps; sweep++) {
        jacobi_rot<0, 1>(N, V); jacobi_rot<0, 2>(N, V); jacobi_rot<0, 3>(N, V);
        jacobi_rot<1, 2>(N, V); jacobi_rot<1, 3>(N, V); jacobi_rot<2, 3>(N, V);
    }
    // eigenvector of the largest eigenvalue (:359-362; maxCoeff keeps the first maximum)
    double best = N[0][0], q[4] = {V[0][0], V[1][0], V[2][0], V[3][0]};
#pragma unroll
    for (int k = 1; k < 4; k++)
        if (N[k][k] > best) { best = N[k][k]; q[0] = V[0][k]; q[1] = V[1][k]; q[2] = V[2][k]; q[3] = V[3][k]; }
    const double qn = sqrt((q[0] * q[0] + q[1] * q[1]) + (q[2] * q[2] + q[3] * q[3]));
    const double qw = q[0] / qn, qx = q[1] / qn, qy = q[2] / qn, qz = q[3] / qn;
    double R[9];
    R[0] = 1.0 - 2.0 * (qy * qy + qz * qz); R[1] = 2.0 * (qx * qy - qz * qw); R[2] = 2.0 * (qx * qz + qy * qw);
    R[3] = 2.0 * (qx * qy + qz * qw); R[4] = 1.0 - 2.0 * (qx * qx + qz * qz); R[5] = 2.0 * (qy * qz - qx * qw);
    R[6] = 2.0 * (qx * qz - qy * qw); R[7] = 2.0 * (qy * qz + qx * qw); R[8] = 1.0 - 2.0 * (qx * qx + qy * qy);
    double s = 1.0;
    if (!fix_scale) {                           // P3 = R * Pr2, s = <Pr1, P3> / <P3, P3> (:371-385)
        double nom = 0.0, den = 0.0;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int i = 0; i < 3; i++) {
                const double p3 = (R[3 * i] * B2[p][0] + R[3 * i + 1] * B2[p][1]) + R[3 * i + 2] * B2[p][2];
                nom += A1[p][i] * p3;
                den += p3 * p3;
            }
        s = nom / den;
    }
#pragma unroll
    for (int i = 0; i < 3; i++)                 // t = O1 - s * R * O2 (:391)
        tf[i] = (float)(O1[i] - s * ((R[3 * i] * O2[0] + R[3 * i + 1] * O2[1]) + R[3 * i + 2] * O2[2]));
#pragma unroll
    for (int i = 0; i < 9; i++) Rf[i] = (float)R[i];
    sf = (float)s;
}

__global__ __launch_bounds__(256) void k_sim3_ransac(const RansacDev* __restrict__ problems)
{
    __shared__ float s_c[12][kLdsN];            // SoA: X1 (0-2), X2 (3-5), p1 (6-7), p2 (8-9), max_err1, max_err2
    __shared__ int s_count[kMaxHyp];
    const RansacDev P = problems[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = P.n, H = P.n_hyp, W = (n + 63) >> 6;
    const bool scored = n >= 3 && n >= P.min_inliers;         // N < mRansacMinInliers: bNoMore, nothing is scored (:155-159)
    if (!scored) {
        for (int h = tid; h < H; h += 256) {
            P.count[h] = 0;
            for (int k = 0; k < 13; k++) P.T12[13 * (size_t)h + k] = 0.0f;
        }
        for (size_t k = tid; k < (size_t)H * W; k += 256) P.mask[k] = 0ull;
        if (tid == 0) { P.sel[0] = 0; P.sel[1] = -1; P.sel[2] = 0; P.sel[3] = 0; }
        return;
    }
    const bool staged = n <= kLdsN;
    auto fetch = [&](int i, float* c) {         // the 12 floats of correspondence i
        if (staged) {
#pragma unroll
            for (int k = 0; k < 12; k++) c[k] = s_c[k][i];
        } else {
#pragma unroll
            for (int k = 0; k < 3; k++) { c[k] = P.X1[3 * (size_t)i + k]; c[3 + k] = P.X2[3 * (size_t)i + k]; }
            project(P.K1, c, c + 6);            // FromCameraToImage (:117-118, :477-487)
            project(P.K2, c + 3, c + 8);
            c[10] = P.e1[i]; c[11] = P.e2[i];
        }
    };
    if (staged) {
        for (int i = tid; i < n; i += 256) {
            float c[12];
#pragma unroll
            for (int k = 0; k < 3; k++) { c[k] = P.X1[3 * (size_t)i + k]; c[3 + k] = P.X2[3 * (size_t)i + k]; }
            project(P.K1, c, c + 6);
            project(P.K2, c + 3, c + 8);
            c[10] = P.e1[i]; c[11] = P.e2[i];
#pragma unroll
            for (int k = 0; k < 12; k++) s_c[k][i] = c[k];
        }
        __syncthreads();
    }
    // ---- phase A: one lane per hypothesis ----
    for (int h = tid; h < H; h += 256) {
        float a[3][3], b[3][3];
#pragma unroll
        for (int p = 0; p < 3; p++) {
            const int i = P.triples[3 * (size_t)h + p];      // validated on the host: 0 <= i < n
            float c[12];
            fetch(i, c);
#pragma unroll
            for (int k = 0; k < 3; k++) { a[p][k] = c[k]; b[p][k] = c[3 + k]; }
        }
        float R[9], t[3], s;
        horn(a, b, P.fix_scale != 0, R, t, s);
        float* o = P.T12 + 13 * (size_t)h;
#pragma unroll
        for (int k = 0; k < 9; k++) o[k] = R[k];
        o[9] = t[0]; o[10] = t[1]; o[11] = t[2]; o[12] = s;
    }
    __syncthreads();                            // T12 rows (global) are visible to the whole workgroup behind the barrier
    // ---- phase B: one wave per hypothesis (CheckInliers, :415-439) ----
    for (int h = wave; h < H; h += 4) {
        const float* o = P.T12 + 13 * (size_t)h;
        const float s = o[12], is = 1.0f / s;
        float sR[9], sRi[9], t[3], ti[3];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) { sR[3 * i + j] = s * o[3 * i + j]; sRi[3 * i + j] = is * o[3 * j + i]; }     // (:398, :405)
#pragma unroll
        for (int i = 0; i < 3; i++) t[i] = o[9 + i];
#pragma unroll
        for (int i = 0; i < 3; i++) ti[i] = -((sRi[3 * i] * t[0] + sRi[3 * i + 1] * t[1]) + sRi[3 * i + 2] * t[2]);   // (:410)
        int cnt = 0;
        for (int j = 0; j < W; j++) {
            const int i = 64 * j + lane;
            bool in = false;
            if (i < n) {
                float c[12], Y[3], Z[3], u[2], v[2];
                fetch(i, c);
#pragma unroll
                for (int r = 0; r < 3; r++) {   // Project (:461-475): Rcw * X + tcw
                    Y[r] = ((sR[3 * r] * c[3] + sR[3 * r + 1] * c[4]) + sR[3 * r + 2] * c[5]) + t[r];
                    Z[r] = ((sRi[3 * r] * c[0] + sRi[3 * r + 1] * c[1]) + sRi[3 * r + 2] * c[2]) + ti[r];
                }
                project(P.K1, Y, u);
                project(P.K2, Z, v);
                const float d1x = c[6] - u[0], d1y = c[7] - u[1], d2x = v[0] - c[8], d2y = v[1] - c[9];
                const float err1 = d1x * d1x + d1y * d1y, err2 = d2x * d2x + d2y * d2y;
                in = err1 < c[10] && err2 < c[11];
            }
            const unsigned long long bal = __ballot(in);
            cnt += __popcll(bal);
            if (lane == 0) P.mask[(size_t)h * W + j] = bal;
        }
        if (lane == 0) { s_count[h] = cnt; P.count[h] = cnt; }
    }
    __syncthreads();
    // ---- phase C: the selection of iterate (:192-209) with mnBestInliers starting at 0 ----
    if (wave == 0) {
        int first = INT_MAX, best = -1, best_h = -1;
        for (int h = lane; h < H; h += 64) {
            const int c = s_count[h];
            if (c > P.min_inliers && h < first) first = h;
            if (c >= best) { best = c; best_h = h; }        // ascending h: the last maximum of this lane
        }
        for (int o = 32; o > 0; o >>= 1) {
            const int f2 = __shfl_xor(first, o), b2 = __shfl_xor(best, o), h2 = __shfl_xor(best_h, o);
            first = min(first, f2);
            if (b2 > best || (b2 == best && h2 > best_h)) { best = b2; best_h = h2; }
        }
        if (lane == 0) {
            const bool conv = first != INT_MAX;
            P.sel[0] = conv ? 1 : 0; P.sel[1] = conv ? first : best_h; P.sel[2] = 1; P.sel[3] = 0;
        }
    }
}


// ---------------------------------------------------------------------------------------------------------------------
// Optimizer::OptimizeSim3 (src/Optimizer.cc:2115-2381) in double: one workgroup runs both rounds of g2o's Levenberg.
// A similarity is 8 doubles: qx qy qz qw tx ty tz s (g2o::Sim3, Thirdparty/g2o/g2o/types/sim3.h).
// ---------------------------------------------------------------------------------------------------------------------
struct OptDev {
    double S[8];
    int32_t n, fix_scale;
    const double* X1; const double* X2; const double* o1; const double* o2; const double* w1; const double* w2;
    double K1[4], K2[4], th2, delta;
    double* err;            // [4n] scratch: _error of e12 and e21 as last computed
    uint8_t* keep;          // [n] out: 1 while the pair is in the graph / was not nulled in vpMatches1
    Sim3OptResult* result;
};

// Sim3(const Vector7d& update) (sim3.h:70-142): update = (omega, upsilon, sigma); the quaternion is Quaterniond(R), not normalised
__device__ inline void sim3_exp(const double* u, double* S)
{
    const double om[3] = {u[0], u[1], u[2]};
    const double sigma = u[6];
    const double theta = sqrt(om[0] * om[0] + om[1] * om[1] + om[2] * om[2]);
    const double O[9] = {0, -om[2], om[1], om[2], 0, -om[0], -om[1], om[0], 0};
    double O2[9];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) O2[i * 3 + j] = O[i * 3] * O[j] + O[i * 3 + 1] * O[3 + j] + O[i * 3 + 2] * O[6 + j];
    const double s = exp(sigma);
    const double eps = 0.00001;
    double A, B, C, R[9];
    double sn = 0, cs = 1;
    const bool small_theta = theta < eps;
    if (small_theta) {
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + O[i] + O2[i];       // (:99, :117)
    } else {
        sn = sin(theta); cs = cos(theta);
        const double a = sn / theta, b = (1 - cs) / (theta * theta);
        for (int i = 0; i < 9; i++) R[i] = ((i % 4 == 0) ? 1.0 : 0.0) + a * O[i] + b * O2[i];
    }
    if (fabs(sigma) < eps) {
        C = 1;
        if (small_theta) { A = 1. / 2.; B = 1. / 6.; }
        else { const double theta2 = theta * theta; A = (1 - cs) / theta2; B = (theta - sn) / (theta2 * theta); }
    } else {
        C = (s - 1) / sigma;
        if (small_theta) {
            const double sigma2 = sigma * sigma;
            A = ((sigma - 1) * s + 1) / sigma2;
            B = ((0.5 * sigma2 - sigma + 1) * s) / (sigma2 * sigma);
        } else {
            const double a = s * sn, b = s * cs, theta2 = theta * theta, sigma2 = sigma * sigma, c = theta2 + sigma2;
            A = (a * sigma + (1 - b) * theta) / (theta * c);
            B = (C - ((b - 1) * sigma + a * theta) / c) * 1. / theta2;
        }
    }
    se3::quat_from_R(R, S);
    for (int i = 0; i < 3; i++) {
        double v = 0;
        for (int j = 0; j < 3; j++) v += ((A * O[i * 3 + j] + B * O2[i * 3 + j]) + ((i == j) ? C : 0.0)) * u[3 + j];
        S[4 + i] = v;
    }
    S[7] = s;
}

// Sim3::operator* (:266-272): r = a.r * b.r, t = a.s * (a.r * b.t) + a.t, s = a.s * b.s
__device__ inline void sim3_mul(const double* a, const double* b, double* o)
{
    double rt[3];
    se3::quat_rotate(a, b + 4, rt);
    o[3] = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
    o[0] = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
    o[1] = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
    o[2] = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
    for (int i = 0; i < 3; i++) o[4 + i] = a[7] * rt[i] + a[4 + i];
    o[7] = a[7] * b[7];
}

// Sim3::inverse (:233-236)
__device__ inline void sim3_inv(const double* a, double* o)
{
    const double m = -1. / a[7];
    const double v[3] = {m * a[4], m * a[5], m * a[6]};
    o[0] = -a[0]; o[1] = -a[1]; o[2] = -a[2]; o[3] = a[3];
    se3::quat_rotate(o, v, o + 4);
    o[7] = 1. / a[7];
}

// obs - project(S.map(X)) (OptimizableTypes.h:183-190, :204-211; Sim3::map :144-146; Pinhole.cpp:35-41)
__device__ __forceinline__ void sim3_edge_error(const double* S, const double* K, const double* X, const double* obs, double* r)
{
    double Y[3];
    se3::quat_rotate(S, X, Y);
    for (int i = 0; i < 3; i++) Y[i] = S[7] * Y[i] + S[4 + i];
    r[0] = obs[0] - (K[0] * Y[0] / Y[2] + K[2]);
    r[1] = obs[1] - (K[1] * Y[1] / Y[2] + K[3]);
}

constexpr int kOptAcc = 36;         // H upper triangle (28), b (7), robust chi2 (1)

// The Levenberg state (estimate, lambda, chi2, counters) and the 7x7 solve are replicated in every thread, as in k_pose_opt:
// the only synchronisation is inside the block reductions and around the shared perturbed similarities.
__global__ __launch_bounds__(256) void k_sim3_optimize(const OptDev* __restrict__ problems)
{
    __shared__ double s_part[kOptAcc][4];
    __shared__ double s_pert[14][2][8];         // exp(+-delta e_d) * S and its inverse, d = 0..6 (+) and 7..13 (-)
    const OptDev P = problems[blockIdx.x];
    const int tid = threadIdx.x, n = P.n;
    const double dsq = P.delta * P.delta;
    double T[8];
    for (int k = 0; k < 8; k++) T[k] = P.S[k];
    for (int e = tid; e < n; e += 256) { P.keep[e] = 1; for (int k = 0; k < 4; k++) P.err[4 * (size_t)e + k] = 0; }
    int iters[2] = {0, 0}, trials[2] = {0, 0}, reason[2] = {0, 0};
    double chis[2] = {0, 0};
    int nBad = 0, nIn = 0;
    bool done = false;
#pragma unroll 1
    for (int round = 0; round < 2 && !done; round++) {
        const bool robust = round == 0;                          // setRobustKernel(0) on the survivors (:2338-2339)
        const int max_it = (round == 0) ? 5 : (nBad > 0 ? 10 : 5);  // (:2308, :2342-2353)
        const int n_active = n - nBad;
        int r_iters = 0, r_trials = 0, r_reason = 0;             // this round's statistics (constant indices below: registers only)
        double r_chi = 0;
        if (n_active > 0) {
            double lambda = 0, ni = 2;
            int nbad_lm = 0;
#pragma unroll 1
            for (int it = 0; it < max_it; it++) {
                // the 14 perturbed estimates of the numeric Jacobian (base_binary_edge.hpp:147-196 through
                // VertexSim3Expmap::oplusImpl, OptimizableTypes.h:158-167), once per linearisation
                double Ti[8];
                sim3_inv(T, Ti);
                __syncthreads();
                if (tid < 14) {
                    double u[7], E[8], Sp[8], Spi[8];
                    const int d = tid % 7;
#pragma unroll
                    for (int k = 0; k < 7; k++) u[k] = (k == d) ? ((tid < 7) ? 1e-9 : -1e-9) : 0.0;     // no dynamic index: registers only
                    if (P.fix_scale) u[6] = 0;
                    sim3_exp(u, E);
                    sim3_mul(E, T, Sp);
                    sim3_inv(Sp, Spi);
                    for (int k = 0; k < 8; k++) { s_pert[tid][0][k] = Sp[k]; s_pert[tid][1][k] = Spi[k]; }
                }
                __syncthreads();
                // computeActiveErrors + activeRobustChi2 + buildSystem on the current estimate
                double acc[kOptAcc];
                for (int k = 0; k < kOptAcc; k++) acc[k] = 0;
                for (int e = tid; e < n; e += 256) {
                    if (!P.keep[e]) continue;
#pragma unroll 1
                    for (int side = 0; side < 2; side++) {
                        // side 0: e12 = obs1 - project1(S12 * X2c); side 1: e21 = obs2 - project2(S12^-1 * X1c)
                        const double* X = (side == 0 ? P.X2 : P.X1) + 3 * (size_t)e;
                        const double* obs = (side == 0 ? P.o1 : P.o2) + 2 * (size_t)e;
                        const double* K = side == 0 ? P.K1 : P.K2;
                        const double w = side == 0 ? P.w1[e] : P.w2[e];
                        const double Xe[3] = {X[0], X[1], X[2]}, oe[2] = {obs[0], obs[1]};
                        double r[2], J[2][7], Ss[8];
#pragma unroll
                        for (int k = 0; k < 8; k++) Ss[k] = side == 0 ? T[k] : Ti[k];       // a select per value keeps T / Ti in registers
                        sim3_edge_error(Ss, K, Xe, oe, r);
                        P.err[4 * (size_t)e + 2 * side] = r[0]; P.err[4 * (size_t)e + 2 * side + 1] = r[1];
                        for (int d = 0; d < 7; d++) {
                            double rp[2], rm[2];
                            sim3_edge_error(s_pert[d][side], K, Xe, oe, rp);
                            sim3_edge_error(s_pert[7 + d][side], K, Xe, oe, rm);
                            J[0][d] = (1.0 / (2 * 1e-9)) * (rp[0] - rm[0]);
                            J[1][d] = (1.0 / (2 * 1e-9)) * (rp[1] - rm[1]);
                        }
                        const double chi = r[0] * (w * r[0]) + r[1] * (w * r[1]);
                        double rho0, rho1;
                        dlm::huber(robust, chi, P.delta, dsq, rho0, rho1);
                        acc[35] += rho0;
                        const double rw = rho1 * w;
                        const double wr0 = rho1 * (-(w * r[0])), wr1 = rho1 * (-(w * r[1]));
#pragma unroll
                        for (int a = 0; a < 7; a++) {
#pragma unroll
                            for (int c = a; c < 7; c++) acc[a * 7 - (a * (a - 1)) / 2 + (c - a)] += J[0][a] * rw * J[0][c] + J[1][a] * rw * J[1][c];
                            acc[28 + a] += J[0][a] * wr0 + J[1][a] * wr1;
                        }
                    }
                }
                dlm::block_sum<kOptAcc>(acc, s_part);
                const double* Hu = acc;
                const double* b = acc + 28;
                double cur = acc[35];
                const double ini = cur;
                if (it == 0) { lambda = dlm::lambda_init<7>(Hu); ni = 2; nbad_lm = 0; }
                // ---- LM trial loop (optimization_algorithm_levenberg.cpp:102-149) ----
                int qmax = 0;
                double rho = 0;
#pragma unroll 1
                do {
                    double x[7], Tt[8], Tti[8];
                    const bool ok2 = dlm::ldlt_solve<7, false>(Hu, lambda, b, x);
                    if (ok2) {
                        double u[7], E[8];
                        for (int k = 0; k < 7; k++) u[k] = x[k];
                        if (P.fix_scale) u[6] = 0;
                        sim3_exp(u, E);
                        sim3_mul(E, T, Tt);
                    } else {
                        for (int k = 0; k < 8; k++) Tt[k] = T[k];
                        for (int k = 0; k < 7; k++) x[k] = 0;
                    }
                    sim3_inv(Tt, Tti);
                    double tchi = 0;
                    for (int e = tid; e < n; e += 256) {
                        if (!P.keep[e]) continue;
#pragma unroll 1
                        for (int side = 0; side < 2; side++) {
                            const double* X = (side == 0 ? P.X2 : P.X1) + 3 * (size_t)e;
                            const double* obs = (side == 0 ? P.o1 : P.o2) + 2 * (size_t)e;
                            const double w = side == 0 ? P.w1[e] : P.w2[e];
                            const double Xe[3] = {X[0], X[1], X[2]}, oe[2] = {obs[0], obs[1]};
                            double r[2], rho0, rho1, Ss[8];
#pragma unroll
                            for (int k = 0; k < 8; k++) Ss[k] = side == 0 ? Tt[k] : Tti[k];
                            sim3_edge_error(Ss, side == 0 ? P.K1 : P.K2, Xe, oe, r);
                            P.err[4 * (size_t)e + 2 * side] = r[0]; P.err[4 * (size_t)e + 2 * side + 1] = r[1];
                            dlm::huber(robust, r[0] * (w * r[0]) + r[1] * (w * r[1]), P.delta, dsq, rho0, rho1);
                            tchi += rho0;
                        }
                    }
                    const double tempChi = dlm::block_sum(tchi, s_part[0]);
                    double scale = 0;
                    for (int j = 0; j < 7; j++) scale += x[j] * (lambda * x[j] + b[j]);
                    if (dlm::trial(ok2, tempChi, scale, lambda, ni, cur, rho))
                        for (int k = 0; k < 8; k++) T[k] = Tt[k];     // discardTop(); after pop() the estimate stays
                    qmax++;
                } while (dlm::more_trials(rho, qmax));
                r_iters++; r_trials += qmax; r_chi = cur;
                r_reason = dlm::stop_reason(qmax, rho, ini, cur, nbad_lm);
                if (r_reason) break;
            }
        }
        __syncthreads();
        if (round == 0) { iters[0] = r_iters; trials[0] = r_trials; reason[0] = r_reason; chis[0] = r_chi; }
        else { iters[1] = r_iters; trials[1] = r_trials; reason[1] = r_reason; chis[1] = r_chi; }
        if (round == 0) {
            // chi2 of the errors as last computed against th2 (:2313-2340); the dropped pairs leave the graph
            double bad = 0;
            for (int e = tid; e < n; e += 256) {
                const double* r = P.err + 4 * (size_t)e;
                const double w1 = P.w1[e], w2 = P.w2[e];
                const double c12 = r[0] * (w1 * r[0]) + r[1] * (w1 * r[1]), c21 = r[2] * (w2 * r[2]) + r[3] * (w2 * r[3]);
                if (c12 > P.th2 || c21 > P.th2) { P.keep[e] = 0; bad += 1.0; }
            }
            nBad = (int)dlm::block_sum(bad, s_part[0]);
            if (n - nBad < 10) {                                 // return 0; g2oS12 is not written (:2348-2349)
                for (int k = 0; k < 8; k++) T[k] = P.S[k];
                nIn = 0;
                done = true;
            }
        } else {
            // computeError on the final estimate, chi2 against th2 (:2357-2374)
            double Ti[8], in = 0;
            sim3_inv(T, Ti);
            for (int e = tid; e < n; e += 256) {
                if (!P.keep[e]) continue;
                const double X1[3] = {P.X1[3 * (size_t)e], P.X1[3 * (size_t)e + 1], P.X1[3 * (size_t)e + 2]};
                const double X2[3] = {P.X2[3 * (size_t)e], P.X2[3 * (size_t)e + 1], P.X2[3 * (size_t)e + 2]};
                const double o1[2] = {P.o1[2 * (size_t)e], P.o1[2 * (size_t)e + 1]}, o2[2] = {P.o2[2 * (size_t)e], P.o2[2 * (size_t)e + 1]};
                double r1[2], r2[2];
                sim3_edge_error(T, P.K1, X2, o1, r1);
                sim3_edge_error(Ti, P.K2, X1, o2, r2);
                const double w1 = P.w1[e], w2 = P.w2[e];
                const double c12 = r1[0] * (w1 * r1[0]) + r1[1] * (w1 * r1[1]), c21 = r2[0] * (w2 * r2[0]) + r2[1] * (w2 * r2[1]);
                if (c12 > P.th2 || c21 > P.th2) P.keep[e] = 0;
                else in += 1.0;
            }
            nIn = (int)dlm::block_sum(in, s_part[0]);
        }
    }
    if (tid == 0) {
        Sim3OptResult R;
        for (int k = 0; k < 4; k++) R.q[k] = T[k];
        for (int k = 0; k < 3; k++) R.t[k] = T[4 + k];
        R.s = T[7];
        R.n_in = nIn; R.n_bad = nBad;
        for (int k = 0; k < 2; k++) { R.iterations[k] = iters[k]; R.trials[k] = trials[k]; R.stop_reason[k] = reason[k]; R.chi2[k] = chis[k]; }
        *P.result = R;
    }
}

}  // namespace sim3

struct sim3_solver : stage::Batch {};     // staging: [descriptors | inputs] up, [outputs] down

namespace {
int ransac_batch(sim3_solver* s, const Sim3RansacProblem* problems, int n_problems, Sim3RansacResult* results)
{
    if (!s || !problems || !results || n_problems < 1) return fail(ORBX_ERR_ARG, "bad arguments");
    ORBX_HIP(hipSetDevice(s->device));
    // layout: [RansacDev x P][per problem: X1 X2 e1 e2 triples]  ||  [per problem: sel count T12 mask]
    struct Off { size_t X1, X2, e1, e2, tri, sel, cnt, T, mask; };
    std::vector<Off> offs(n_problems);
    stage::Cursor cur;
    cur.take(sizeof(sim3::RansacDev) * (size_t)n_problems);
    for (int i = 0; i < n_problems; i++) {
        const Sim3RansacProblem& p = problems[i];
        if (p.n < 0 || p.n_hyp < 1 || p.n_hyp > SIM3_MAX_HYPOTHESES) return fail(ORBX_ERR_ARG, "problem %d: n %d / n_hyp %d out of range", i, p.n, p.n_hyp);
        if (!p.triples || (p.n > 0 && (!p.X1c || !p.X2c || !p.max_err1 || !p.max_err2))) return fail(ORBX_ERR_ARG, "problem %d: NULL arrays", i);
        if (p.n >= 3 && p.n >= p.min_inliers)               // the kernel indexes the correspondences by these: check the bounds here
            for (int k = 0; k < 3 * p.n_hyp; k++)
                if (p.triples[k] < 0 || p.triples[k] >= p.n) return fail(ORBX_ERR_ARG, "problem %d: triple index %d out of [0, %d)", i, p.triples[k], p.n);
        const size_t n = (size_t)p.n, H = (size_t)p.n_hyp;
        Off& o = offs[i];
        o.X1 = cur.take(12 * n);
        o.X2 = cur.take(12 * n);
        o.e1 = cur.take(4 * n);
        o.e2 = cur.take(4 * n);
        o.tri = cur.take(12 * H);
    }
    const size_t up_bytes = cur.pos;
    for (int i = 0; i < n_problems; i++) {
        const size_t H = (size_t)problems[i].n_hyp, W = ((size_t)problems[i].n + 63) / 64;
        Off& o = offs[i];
        o.sel = cur.take(16);
        o.cnt = cur.take(4 * H);
        o.T = cur.take(52 * H);
        o.mask = cur.take(8 * H * W);
    }
    const int rc = stage::reserve(*s, cur.pos, cur.pos);
    if (rc != ORBX_OK) return rc;
    uint8_t* base = s->d_blob;
    sim3::RansacDev* descs = (sim3::RansacDev*)s->h_blob;
    for (int i = 0; i < n_problems; i++) {
        const Sim3RansacProblem& p = problems[i];
        const Off& o = offs[i];
        const size_t n = (size_t)p.n;
        if (n) {
            std::memcpy(s->h_blob + o.X1, p.X1c, 12 * n); std::memcpy(s->h_blob + o.X2, p.X2c, 12 * n);
            std::memcpy(s->h_blob + o.e1, p.max_err1, 4 * n); std::memcpy(s->h_blob + o.e2, p.max_err2, 4 * n);
        }
        std::memcpy(s->h_blob + o.tri, p.triples, 12 * (size_t)p.n_hyp);
        sim3::RansacDev d;
        d.n = p.n; d.n_hyp = p.n_hyp; d.fix_scale = p.fix_scale; d.min_inliers = p.min_inliers;
        d.K1[0] = p.fx1; d.K1[1] = p.fy1; d.K1[2] = p.cx1; d.K1[3] = p.cy1;
        d.K2[0] = p.fx2; d.K2[1] = p.fy2; d.K2[2] = p.cx2; d.K2[3] = p.cy2;
        d.X1 = (const float*)(base + o.X1); d.X2 = (const float*)(base + o.X2);
        d.e1 = (const float*)(base + o.e1); d.e2 = (const float*)(base + o.e2);
        d.triples = (const int32_t*)(base + o.tri);
        d.sel = (int32_t*)(base + o.sel); d.count = (int32_t*)(base + o.cnt); d.T12 = (float*)(base + o.T);
        d.mask = (unsigned long long*)(base + o.mask);
        descs[i] = d;
    }
    const int rr = stage::run(*s, up_bytes, up_bytes, cur.pos, [&] {
        hipLaunchKernelGGL(sim3::k_sim3_ransac, dim3(n_problems), dim3(256), 0, s->stream, (const sim3::RansacDev*)base);
    });
    if (rr != ORBX_OK) return rr;
    for (int i = 0; i < n_problems; i++) {
        const Off& o = offs[i];
        const size_t H = (size_t)problems[i].n_hyp, W = ((size_t)problems[i].n + 63) / 64;
        const int32_t* sel = (const int32_t*)(s->h_blob + o.sel);
        Sim3RansacResult& r = results[i];
        r.converged = sel[0]; r.index = sel[1]; r.scored = sel[2];
        if (r.count) std::memcpy(r.count, s->h_blob + o.cnt, 4 * H);
        if (r.T12) std::memcpy(r.T12, s->h_blob + o.T, 52 * H);
        if (r.mask && W) std::memcpy(r.mask, s->h_blob + o.mask, 8 * H * W);
    }
    return ORBX_OK;
}

int optimize_batch(sim3_solver* s, const Sim3OptProblem* problems, int n_problems, Sim3OptResult* results, uint8_t* const* keep_out)
{
    if (!s || !problems || !results || n_problems < 1) return fail(ORBX_ERR_ARG, "bad arguments");
    ORBX_HIP(hipSetDevice(s->device));
    // layout: [OptDev x P][per problem: X1 X2 obs1 obs2 w1 w2]  ||  [Sim3OptResult x P][per problem: keep]  ||  err scratch
    struct Off { size_t X1, X2, o1, o2, w1, w2, keep, err; };
    std::vector<Off> offs(n_problems);
    stage::Cursor cur;
    cur.take(sizeof(sim3::OptDev) * (size_t)n_problems);
    for (int i = 0; i < n_problems; i++) {
        const Sim3OptProblem& p = problems[i];
        if (p.n < 0 || (p.n > 0 && (!p.X1c || !p.X2c || !p.obs1 || !p.obs2 || !p.inv_sigma2_1 || !p.inv_sigma2_2)))
            return fail(ORBX_ERR_ARG, "problem %d: NULL arrays", i);
        const size_t n = (size_t)p.n;
        Off& o = offs[i];
        o.X1 = cur.take(24 * n);
        o.X2 = cur.take(24 * n);
        o.o1 = cur.take(16 * n);
        o.o2 = cur.take(16 * n);
        o.w1 = cur.take(8 * n);
        o.w2 = cur.take(8 * n);
    }
    const size_t up_bytes = cur.pos;
    const size_t res_off = cur.take(sizeof(Sim3OptResult) * (size_t)n_problems);
    for (int i = 0; i < n_problems; i++) offs[i].keep = cur.take((size_t)std::max(problems[i].n, 1));
    const size_t down_end = cur.pos;
    for (int i = 0; i < n_problems; i++) offs[i].err = cur.take(32 * (size_t)std::max(problems[i].n, 1));
    const int rc = stage::reserve(*s, cur.pos, cur.pos);
    if (rc != ORBX_OK) return rc;
    uint8_t* base = s->d_blob;
    sim3::OptDev* descs = (sim3::OptDev*)s->h_blob;
    for (int i = 0; i < n_problems; i++) {
        const Sim3OptProblem& p = problems[i];
        const Off& o = offs[i];
        const size_t n = (size_t)p.n;
        if (n) {
            std::memcpy(s->h_blob + o.X1, p.X1c, 24 * n); std::memcpy(s->h_blob + o.X2, p.X2c, 24 * n);
            std::memcpy(s->h_blob + o.o1, p.obs1, 16 * n); std::memcpy(s->h_blob + o.o2, p.obs2, 16 * n);
            std::memcpy(s->h_blob + o.w1, p.inv_sigma2_1, 8 * n); std::memcpy(s->h_blob + o.w2, p.inv_sigma2_2, 8 * n);
        }
        sim3::OptDev d;
        for (int k = 0; k < 4; k++) d.S[k] = p.q[k];
        for (int k = 0; k < 3; k++) d.S[4 + k] = p.t[k];
        d.S[7] = p.s;
        d.n = p.n; d.fix_scale = p.fix_scale;
        d.X1 = (const double*)(base + o.X1); d.X2 = (const double*)(base + o.X2);
        d.o1 = (const double*)(base + o.o1); d.o2 = (const double*)(base + o.o2);
        d.w1 = (const double*)(base + o.w1); d.w2 = (const double*)(base + o.w2);
        d.K1[0] = p.fx1; d.K1[1] = p.fy1; d.K1[2] = p.cx1; d.K1[3] = p.cy1;
        d.K2[0] = p.fx2; d.K2[1] = p.fy2; d.K2[2] = p.cx2; d.K2[3] = p.cy2;
        d.th2 = p.th2; d.delta = p.huber_delta;
        d.err = (double*)(base + o.err); d.keep = base + o.keep;
        d.result = (Sim3OptResult*)(base + res_off) + i;
        descs[i] = d;
    }
    const int rr = stage::run(*s, up_bytes, res_off, down_end, [&] {
        hipLaunchKernelGGL(sim3::k_sim3_optimize, dim3(n_problems), dim3(256), 0, s->stream, (const sim3::OptDev*)base);
    });
    if (rr != ORBX_OK) return rr;
    std::memcpy(results, s->h_blob + res_off, sizeof(Sim3OptResult) * (size_t)n_problems);
    if (keep_out)
        for (int i = 0; i < n_problems; i++)
            if (keep_out[i] && problems[i].n > 0) std::memcpy(keep_out[i], s->h_blob + offs[i].keep, (size_t)problems[i].n);
    return ORBX_OK;
}
}  // namespace

extern "C" {

int sim3_create(int device, sim3_solver** out) { return stage::open(device, out); }

void sim3_destroy(sim3_solver* s) { stage::close(s); }

float sim3_last_kernel_ms(const sim3_solver* s) { return s ? s->last_kernel_ms : 0.0f; }

int sim3_ransac_batch(sim3_solver* s, const Sim3RansacProblem* problems, int n_problems, Sim3RansacResult* results)
{
    return stage::guarded("sim3_ransac_batch", [&] { return ransac_batch(s, problems, n_problems, results); });
}

int sim3_optimize_batch(sim3_solver* s, const Sim3OptProblem* problems, int n_problems, Sim3OptResult* results, uint8_t* const* keep_out)
{
    return stage::guarded("sim3_optimize_batch", [&] { return optimize_batch(s, problems, n_problems, results, keep_out); });
}

// The reference draws with DUtils::Random::RandomInt (libc rand); here the generator is part of the interface: splitmix64
// (Steele, Lea, Flood 2014), state = seed, one step per draw, randi = x % (number of indices still available).  The procedure
// is the reference's (src/Sim3Solver.cc:172-186): pick a slot of the available list, move the last entry into it, shrink.
int sim3_draw_triples(uint64_t seed, int n, int n_hyp, int32_t* out)
{
    if (n < 3 || n_hyp < 1 || !out) return fail(ORBX_ERR_ARG, "sim3_draw_triples: n %d (>= 3) / n_hyp %d (>= 1) / out", n, n_hyp);
    return stage::guarded("sim3_draw_triples", [&] {
        std::vector<int32_t> all(n), avail;
        for (int i = 0; i < n; i++) all[i] = i;
        uint64_t state = seed;
        for (int h = 0; h < n_hyp; h++) {
            avail = all;
            for (int k = 0; k < 3; k++) {
                state += 0x9E3779B97F4A7C15ull;
                uint64_t z = state;
                z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
                z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
                z ^= z >> 31;
                const size_t r = (size_t)(z % (uint64_t)avail.size());
                out[3 * (size_t)h + k] = avail[r];
                avail[r] = avail.back();
                avail.pop_back();
            }
        }
        return ORBX_OK;
    });
}

}  // extern "C"
