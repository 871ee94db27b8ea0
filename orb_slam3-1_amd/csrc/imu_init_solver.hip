// imu_init_solver.hip -- gfx950 kernel + C ABI for the three Optimizer::InertialOptimization overloads (reference
// src/Optimizer.cc:3042, :3227, :3389; EdgeInertialGS src/G2oTypes.cc:596-718, VertexGDir / VertexScale include/G2oTypes.h:257-317):
// gravity direction, scale, biases and key-frame velocities of a map whose poses stay fixed (include/orbslam3_hip_imu_init.h).
//
// Structure: three unknowns per key frame (its velocity), coupled only along the mPrevKF chain, and at most nine unknowns shared
// by every link (gyro bias 3, accelerometer bias 3, gravity direction 2, log-scale 1).  With the key frames numbered along their
// paths (imu_init_structure.h) the normal equations are block tridiagonal in 3 x 3 blocks with a 9-wide border:
//
//     [ T   B ] [xv]   [rv]        T = tridiag(E_p^T, D_p, E_{p+1}),  B_p 3 x 9
//     [ B^T C ] [xb] = [rb]
//
// MI355X mapping: ONE 256-thread workgroup runs the whole optimisation of a problem (up to 200 iterations of up to 10 trials: a
// host-driven loop would be all launch latency), a batch is one launch with one workgroup per problem.  Thread p owns chain
// position p: it linearises the link INTO p (one writer per slot), gathers the at most two links of its key frame in a fixed
// order (in, then out), and the border is an ordered block sum.  The chain is eliminated forward by wave 0 (the 3 x 3 pivots
// replicated in every lane, lanes 0-9 on the ten right-hand columns: nine border columns and the right-hand side), the 9 x 9 Schur
// complement is an ordered block sum over the key frames and is solved replicated in every thread, and the back-substitution
// walks every path on the thread of its tail.  No atomics, no accumulation into memory: two runs agree bit for bit.
// The per-key-frame blocks (136 doubles of a link's quadratic form, 108 of the elimination) live in a global arena of the
// handle, which stays in L2 (256 key frames: 0.5 MB); LDS holds the velocities and what the two serial passes read.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbslam3_hip.h"
#include "batch_stage.h"
#include "dense_lm_device.h"
#include "imu_init_group.h"
#include "imu_init_structure.h"

namespace imuinit {

constexpr int kThreads = 256;

struct Out {
    double bg[3], ba[3], Rwg[9], scale, chi2_initial, chi2_final, lambda;
    int32_t iterations, trials, stop_reason, pad;
    double trace[16];
};

struct Dev {
    int32_t n_chain, n_links;
    const double* Rwb; const double* twb; const double* vel;    // by key frame
    const int32_t* order; const int32_t* link_in;               // [n_chain]
    const LibaLink* links;
    double bg[3], ba[3], Rwg[9], scale;
    double prior_g, prior_a, lambda_init;
    int32_t max_iters, gauss_newton;
    Cfg cfg;
    double* slot;       // [n_chain][kSlot]
    double* D;          // [n_chain][9]   diagonal block of position p
    double* E;          // [n_chain][9]   H[p - 1][p]
    double* Y0;         // [n_chain][30]  3 x 10: the border block of p and, in column 9, its right-hand side
    double* Y;          // [n_chain][30]  forward-eliminated
    double* Z;          // [n_chain][30]  pivot^-1 Y
    double* vel_out;    // [n_chain][3]
    Out* out;
};

__device__ __forceinline__ double block_max(double v, double (&s_part)[4])
{
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) s_part[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmax(fmax(s_part[0], s_part[1]), fmax(s_part[2], s_part[3]));
}

__global__ __launch_bounds__(kThreads) void k_imu_init(const Dev* __restrict__ problems)
{
    __shared__ double s_v[kThreads][3], s_vt[kThreads][3];      // accepted / trial velocity of every position
    __shared__ double s_L[kThreads][9];                         // E_p^T pivot_{p-1}^-1 of the forward pass
    __shared__ double s_w[kThreads][3], s_x[kThreads][3];
    __shared__ double s_part[55][4];
    __shared__ int s_in[kThreads + 1];                          // link into position p (-1: none); [n_chain] = -1
    __shared__ int s_ok;
    const Dev d = problems[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, nC = d.n_chain;

    Border X;
    for (int k = 0; k < 3; k++) { X.bg[k] = d.bg[k]; X.ba[k] = d.ba[k]; }
    for (int k = 0; k < 9; k++) X.Rwg[k] = d.Rwg[k];
    X.s = d.scale;
    if (nC == 0 || d.n_links == 0) {        // no active edge: the inputs come back (uniform over the workgroup)
        if (tid == 0) {
            Out o;
            memset(&o, 0, sizeof(o));
            for (int k = 0; k < 3; k++) { o.bg[k] = X.bg[k]; o.ba[k] = X.ba[k]; }
            for (int k = 0; k < 9; k++) o.Rwg[k] = X.Rwg[k];
            o.scale = X.s;
            *d.out = o;
        }
        return;
    }
    const bool active = tid < nC;
    const int lin = active ? d.link_in[tid] : -1;
    s_in[tid] = lin;
    if (tid == 0) s_in[kThreads] = -1;
    const bool has_in = lin >= 0;
    Geom G;
    memset(&G, 0, sizeof(G));
    if (active) {
        const int k2 = d.order[tid];
        for (int k = 0; k < 3; k++) s_v[tid][k] = d.vel[3 * k2 + k];
        if (has_in) {
            const int k1 = d.order[tid - 1];
            for (int k = 0; k < 9; k++) { G.Rwb1[k] = d.Rwb[9 * k1 + k]; G.Rwb2[k] = d.Rwb[9 * k2 + k]; }
            for (int k = 0; k < 3; k++) { G.twb1[k] = d.twb[3 * k1 + k]; G.twb2[k] = d.twb[3 * k2 + k]; }
        }
    } else {
        for (int k = 0; k < 3; k++) s_v[tid][k] = 0.0;
    }
    for (int k = 0; k < 3; k++) s_vt[tid][k] = 0.0;
    __syncthreads();
    const bool has_out = active && s_in[tid + 1] >= 0 && tid + 1 < nC;
    const LibaLink& L = d.links[has_in ? lin : 0];
    double* const slot = d.slot + (size_t)kSlot * tid;
    const double* const slot_out = d.slot + (size_t)kSlot * (tid + 1);
    const bool priors = d.cfg.free_bias != 0;

    auto prior_chi2 = [&](const Border& b) -> double {
        if (!priors) return 0.0;
        double cg = 0, ca = 0;
        for (int k = 0; k < 3; k++) { cg += b.bg[k] * d.prior_g * b.bg[k]; ca += b.ba[k] * d.prior_a * b.ba[k]; }
        return ca + cg;
    };
    // active robust chi2 at (velocities vv, border b)
    auto total_chi2 = [&](const double (*vv)[3], const Border& b) -> double {
        double c = 0;
        if (has_in) c = gs_chi2(d.cfg, L, G, vv[tid - 1], vv[tid], b);
        return dlm::block_sum(c, s_part[0]) + prior_chi2(b);
    };

    const double chi2_initial = total_chi2(s_v, X);
    double cur = chi2_initial, lambda = 0, ni = 2;
    int nbad = 0, iterations = 0, trials = 0, stop = 0;
    double trace[16];
    for (int k = 0; k < 16; k++) trace[k] = 0;
    const bool free_b[9] = {priors, priors, priors, priors, priors, priors, d.cfg.free_gdir != 0, d.cfg.free_gdir != 0, d.cfg.free_scale != 0};

#pragma unroll 1
    for (int it = 0; it < d.max_iters; it++) {
        // ---- computeActiveErrors + buildSystem on the accepted estimate ----
        if (has_in) gs_linearize(d.cfg, L, G, s_v[tid - 1], s_v[tid], X, slot);
        __syncthreads();
        double acc[55];                     // this link's share of the border: C (45, packed upper), rb (9), chi2
        for (int k = 0; k < 55; k++) acc[k] = 0.0;
        if (has_in) {
            for (int a = 0; a < 9; a++) {
                for (int c = a; c < 9; c++) acc[a * 9 - (a * (a - 1)) / 2 + (c - a)] = slot[up15(6 + a, 6 + c)];
                acc[45 + a] = slot[120 + 6 + a];
            }
            acc[54] = slot[135];
        }
        double dmax = 0;
        if (active && d.cfg.free_vel) {         // the key frame's blocks: the link into it, then the link out of it
            double Dp[9], Ep[9], Yp[30];
            for (int i = 0; i < 3; i++) {
                for (int j = 0; j < 3; j++) {
                    double v = 0;
                    if (has_in) v = slot[sym15(3 + i, 3 + j)];
                    if (has_out) v += slot_out[sym15(i, j)];
                    Dp[3 * i + j] = v;
                    Ep[3 * i + j] = has_in ? slot[up15(i, 3 + j)] : 0.0;
                }
                for (int c = 0; c < 9; c++) {
                    double v = 0;
                    if (has_in) v = slot[up15(3 + i, 6 + c)];
                    if (has_out) v += slot_out[up15(i, 6 + c)];
                    Yp[10 * i + c] = v;
                }
                double v = 0;
                if (has_in) v = slot[120 + 3 + i];
                if (has_out) v += slot_out[120 + i];
                Yp[10 * i + 9] = v;
                dmax = fmax(dmax, fabs(Dp[4 * i]));
            }
            for (int k = 0; k < 9; k++) { d.D[9 * (size_t)tid + k] = Dp[k]; d.E[9 * (size_t)tid + k] = Ep[k]; }
            for (int k = 0; k < 30; k++) d.Y0[30 * (size_t)tid + k] = Yp[k];
        }
        dlm::block_sum<55>(acc, s_part);
        double C[45], rb[9];
        for (int k = 0; k < 45; k++) C[k] = acc[k];
        for (int k = 0; k < 9; k++) rb[k] = acc[45 + k];
        if (priors)                         // EdgePriorGyro / EdgePriorAcc: error = estimate - 0, information prior x I
            for (int k = 0; k < 3; k++) {
                C[k * 9 - (k * (k - 1)) / 2] += d.prior_g; rb[k] -= d.prior_g * X.bg[k];
                C[(3 + k) * 9 - ((3 + k) * (2 + k)) / 2] += d.prior_a; rb[3 + k] -= d.prior_a * X.ba[k];
            }
        cur = acc[54] + prior_chi2(X);
        const double ini = cur;
        if (it == 0 && !d.gauss_newton) {
            if (d.lambda_init > 0) lambda = d.lambda_init;
            else {                          // computeLambdaInit: 1e-5 * max diag H over the free unknowns
                double m = block_max(dmax, s_part[0]);
                for (int a = 0; a < 9; a++) m = fmax(m, fabs(C[a * 9 - (a * (a - 1)) / 2]));
                lambda = 1e-5 * m;
            }
            ni = 2; nbad = 0;
        }
        // ---- the trials of this iteration (levenberg.cpp:102-149); Gauss-Newton: one solve at lambda = 0, always taken ----
        int qmax = 0;
        double rho = 0;
        bool gn_failed = false;
#pragma unroll 1
        do {
            __syncthreads();
            if (tid == 0) s_ok = 1;
            if (d.cfg.free_vel && tid < 64) {
                // forward elimination of the chain: pivot_p = D_p + lambda I - Lm E_p, Lm = E_p^T pivot_{p-1}^-1; column c of the
                // right-hand sides follows on lane c
                const int c = lane < 10 ? lane : 9;
                double Pi[9], yp[3] = {0, 0, 0};
                for (int k = 0; k < 9; k++) Pi[k] = 0;
                bool ok = true;
                double nD[9], nE[9], ny[3];
                int nin = s_in[0];
                for (int k = 0; k < 9; k++) { nD[k] = d.D[k]; nE[k] = d.E[k]; }
                for (int i = 0; i < 3; i++) ny[i] = d.Y0[10 * i + c];
#pragma unroll 1
                for (int p = 0; p < nC; p++) {
                    double Dp[9], Ep[9], y[3];
                    const int in = nin;
                    for (int k = 0; k < 9; k++) { Dp[k] = nD[k]; Ep[k] = nE[k]; }
                    for (int i = 0; i < 3; i++) y[i] = ny[i];
                    if (p + 1 < nC) {       // the next position's blocks are on their way while this one is eliminated
                        nin = s_in[p + 1];
                        for (int k = 0; k < 9; k++) { nD[k] = d.D[9 * (size_t)(p + 1) + k]; nE[k] = d.E[9 * (size_t)(p + 1) + k]; }
                        for (int i = 0; i < 3; i++) ny[i] = d.Y0[30 * (size_t)(p + 1) + 10 * i + c];
                    }
                    for (int i = 0; i < 3; i++) Dp[4 * i] += lambda;
                    if (in >= 0) {
                        double Lm[9];
                        for (int i = 0; i < 3; i++)
                            for (int j = 0; j < 3; j++) Lm[3 * i + j] = Ep[i] * Pi[j] + Ep[3 + i] * Pi[3 + j] + Ep[6 + i] * Pi[6 + j];
                        for (int i = 0; i < 3; i++)
                            for (int j = i; j < 3; j++) {
                                const double v = Dp[3 * i + j] - (Lm[3 * i] * Ep[j] + Lm[3 * i + 1] * Ep[3 + j] + Lm[3 * i + 2] * Ep[6 + j]);
                                Dp[3 * i + j] = v; Dp[3 * j + i] = v;
                            }
                        double t[3];
                        mvec(Lm, yp, t);
                        for (int i = 0; i < 3; i++) y[i] -= t[i];
                        if (lane == 0) for (int k = 0; k < 9; k++) s_L[p][k] = Lm[k];
                    }
                    ok = spd_inv3(Dp, Pi) && ok;
                    double z[3];
                    mvec(Pi, y, z);
                    if (lane < 10)
                        for (int i = 0; i < 3; i++) { d.Y[30 * (size_t)p + 10 * i + c] = y[i]; d.Z[30 * (size_t)p + 10 * i + c] = z[i]; }
                    for (int i = 0; i < 3; i++) yp[i] = y[i];
                }
                if (lane == 0 && !ok) s_ok = 0;
            }
            __syncthreads();
            // ---- Schur complement of the border: an ordered sum over the key frames ----
            double sc[54];
            for (int k = 0; k < 54; k++) sc[k] = 0.0;
            if (active && d.cfg.free_vel) {
                double Yp[30], Zp[30];
                for (int k = 0; k < 30; k++) { Yp[k] = d.Y[30 * (size_t)tid + k]; Zp[k] = d.Z[30 * (size_t)tid + k]; }
                for (int a = 0; a < 9; a++) {
                    for (int c = a; c < 9; c++)
                        sc[a * 9 - (a * (a - 1)) / 2 + (c - a)] = Yp[a] * Zp[c] + Yp[10 + a] * Zp[10 + c] + Yp[20 + a] * Zp[20 + c];
                    sc[45 + a] = Yp[a] * Zp[9] + Yp[10 + a] * Zp[19] + Yp[20 + a] * Zp[29];
                }
            }
            if (d.cfg.free_vel) dlm::block_sum<54>(sc, s_part);
            double S[45], rs[9], xb[9];
            for (int k = 0; k < 45; k++) S[k] = C[k] - sc[k];
            for (int a = 0; a < 9; a++) rs[a] = rb[a] - sc[45 + a];
            for (int a = 0; a < 9; a++)
                if (!free_b[a]) {           // a fixed border unknown: identity row and column, zero right-hand side
                    for (int c = 0; c < 9; c++) if (c != a) S[c <= a ? c * 9 - (c * (c - 1)) / 2 + (a - c) : a * 9 - (a * (a - 1)) / 2 + (c - a)] = 0.0;
                    S[a * 9 - (a * (a - 1)) / 2] = 1.0; rs[a] = 0.0;
                }
            bool solved = dlm::ldlt_solve<9, false>(S, lambda, rs, xb);
            solved = solved && s_ok != 0;
            for (int a = 0; a < 9; a++) if (!free_b[a] || !solved) xb[a] = 0.0;
            // ---- back-substitution: w_p = Z_p (b - B xb) per key frame, then every path from its tail to its head ----
            double xv[3] = {0, 0, 0}, bv[3] = {0, 0, 0};
            if (d.cfg.free_vel) {
                if (active) {
                    const double* Zp = d.Z + 30 * (size_t)tid;
                    for (int i = 0; i < 3; i++) {
                        double w = Zp[10 * i + 9];
                        for (int c = 0; c < 9; c++) w -= Zp[10 * i + c] * xb[c];
                        s_w[tid][i] = w;
                        bv[i] = d.Y0[30 * (size_t)tid + 10 * i + 9];
                    }
                }
                __syncthreads();
                if (active && !has_out) {
                    double x[3] = {s_w[tid][0], s_w[tid][1], s_w[tid][2]};
                    for (int k = 0; k < 3; k++) s_x[tid][k] = x[k];
#pragma unroll 1
                    for (int q = tid - 1; q >= 0 && s_in[q + 1] >= 0; q--) {
                        const double* Lm = s_L[q + 1];
                        const double x0 = s_w[q][0] - (Lm[0] * x[0] + Lm[3] * x[1] + Lm[6] * x[2]);
                        const double x1 = s_w[q][1] - (Lm[1] * x[0] + Lm[4] * x[1] + Lm[7] * x[2]);
                        const double x2 = s_w[q][2] - (Lm[2] * x[0] + Lm[5] * x[1] + Lm[8] * x[2]);
                        x[0] = x0; x[1] = x1; x[2] = x2;
                        for (int k = 0; k < 3; k++) s_x[q][k] = x[k];
                    }
                }
                __syncthreads();
                if (active && solved) for (int k = 0; k < 3; k++) xv[k] = s_x[tid][k];
            }
            // ---- the trial estimate (oplus) and its chi2 ----
            Border Xt = X;
            if (solved) {
                if (priors) for (int k = 0; k < 3; k++) { Xt.bg[k] = X.bg[k] + xb[k]; Xt.ba[k] = X.ba[k] + xb[3 + k]; }
                if (d.cfg.free_gdir) {          // GDirection::Update: Rwg <- Rwg ExpSO3(u0, u1, 0)
                    const double u[3] = {xb[6], xb[7], 0.0};
                    double Ex[9];
                    exp_so3(u, Ex);
                    mmul(X.Rwg, Ex, Xt.Rwg);
                }
                if (d.cfg.free_scale) Xt.s = X.s * exp(xb[8]);
            }
            for (int k = 0; k < 3; k++) s_vt[tid][k] = s_v[tid][k] + xv[k];
            __syncthreads();
            double two[2] = {0.0, 0.0};
            if (has_in) two[0] = gs_chi2(d.cfg, L, G, s_vt[tid - 1], s_vt[tid], Xt);
            for (int k = 0; k < 3; k++) two[1] += xv[k] * (lambda * xv[k] + bv[k]);
            dlm::block_sum<2>(two, s_part);
            const double chi_new = two[0] + prior_chi2(Xt);
            double scale = two[1];
            for (int a = 0; a < 9; a++) scale += xb[a] * (lambda * xb[a] + rb[a]);
            bool take;
            if (d.gauss_newton) { take = solved; gn_failed = !solved; cur = solved ? chi_new : cur; }
            else take = dlm::trial(solved, chi_new, scale, lambda, ni, cur, rho);
            if (take) {
                X = Xt;
                for (int k = 0; k < 3; k++) s_v[tid][k] = s_vt[tid][k];
            }
            qmax++;
        } while (!d.gauss_newton && dlm::more_trials(rho, qmax));
        __syncthreads();
        iterations++; trials += qmax;
        if (it < 16) trace[it] = cur;
        if (d.gauss_newton) { if (gn_failed) { stop = 4; break; } }
        else if ((stop = dlm::stop_reason(qmax, rho, ini, cur, nbad)) != 0) break;
    }
    if (active) for (int k = 0; k < 3; k++) d.vel_out[3 * (size_t)tid + k] = s_v[tid][k];
    if (tid == 0) {
        Out o;
        for (int k = 0; k < 3; k++) { o.bg[k] = X.bg[k]; o.ba[k] = X.ba[k]; }
        for (int k = 0; k < 9; k++) o.Rwg[k] = X.Rwg[k];
        o.scale = X.s; o.chi2_initial = chi2_initial; o.chi2_final = cur; o.lambda = lambda;
        o.iterations = iterations; o.trials = trials; o.stop_reason = stop; o.pad = 0;
        for (int k = 0; k < 16; k++) o.trace[k] = trace[k];
        *d.out = o;
    }
}

}  // namespace imuinit

struct imu_init_solver : stage::Batch {};

namespace {

bool all_finite(const double* v, size_t n)
{
    for (size_t i = 0; i < n; i++) if (!std::isfinite(v[i])) return false;
    return true;
}

// every argument check of one problem; st (may be NULL) receives the chain order
int check_problem(const ImuInitProblem* p, const ImuInitResult* r, int idx, imuinit::Structure* st)
{
    if (!p || !r) return fail(ORBX_ERR_ARG, "problem %d: problem or result is NULL", idx);
    if (p->n_kf < 0 || p->n_links < 0) return fail(ORBX_ERR_ARG, "problem %d: negative size", idx);
    if (p->n_kf > IMU_INIT_MAX_KF) return fail(ORBX_ERR_CAPACITY, "problem %d: %d key frames, the capacity is %d", idx, p->n_kf, IMU_INIT_MAX_KF);
    if (p->n_kf > 0 && (!p->Rwb || !p->twb || !p->vel)) return fail(ORBX_ERR_ARG, "problem %d: Rwb, twb or vel is NULL", idx);
    if (p->n_kf > 0 && !r->vel_out) return fail(ORBX_ERR_ARG, "problem %d: vel_out is NULL", idx);
    if (p->n_links > 0 && !p->links) return fail(ORBX_ERR_ARG, "problem %d: links is NULL", idx);
    if (!(p->scale > 0) || !std::isfinite(p->scale)) return fail(ORBX_ERR_ARG, "problem %d: the scale is not finite and positive", idx);
    if (!all_finite(p->bg, 3) || !all_finite(p->ba, 3) || !all_finite(p->Rwg, 9)) return fail(ORBX_ERR_ARG, "problem %d: bg, ba or Rwg is not finite", idx);
    if (!all_finite(p->Rwb, 9 * (size_t)p->n_kf) || !all_finite(p->twb, 3 * (size_t)p->n_kf) || !all_finite(p->vel, 3 * (size_t)p->n_kf))
        return fail(ORBX_ERR_ARG, "problem %d: a key-frame value is not finite", idx);
    if (!(p->lambda_init >= 0) || !std::isfinite(p->lambda_init)) return fail(ORBX_ERR_ARG, "problem %d: lambda_init is negative or not finite", idx);
    if (p->max_iters < 0 || p->max_iters > 1000) return fail(ORBX_ERR_ARG, "problem %d: max_iters %d outside 0 .. 1000", idx, p->max_iters);
    if (p->gauss_newton != 0 && p->gauss_newton != 1) return fail(ORBX_ERR_ARG, "problem %d: gauss_newton is neither 0 nor 1", idx);
    if (!(p->prior_g >= 0) || !(p->prior_a >= 0) || !std::isfinite(p->prior_g) || !std::isfinite(p->prior_a))
        return fail(ORBX_ERR_ARG, "problem %d: a prior is negative or not finite", idx);
    if (!p->free_vel && !p->free_bias && !p->free_gdir && !p->free_scale) return fail(ORBX_ERR_ARG, "problem %d: nothing is free", idx);
    std::vector<int> kf1((size_t)p->n_links), kf2((size_t)p->n_links);
    bool robust = false;
    for (int l = 0; l < p->n_links; l++) { kf1[l] = p->links[l].kf1; kf2[l] = p->links[l].kf2; robust = robust || p->links[l].robust; }
    if (!std::isfinite(p->huber_delta)) return fail(ORBX_ERR_ARG, "problem %d: huber_delta is not finite", idx);
    if (robust && !(p->huber_delta > 0)) return fail(ORBX_ERR_ARG, "problem %d: huber_delta is not positive with a robust link", idx);
    for (int l = 0; l < p->n_links; l++) {          // the float members as doubles, then info9
        const LibaLink& L = p->links[l];
        const float* f[] = {L.dR, L.dV, L.dP, L.JRg, L.JVg, L.JVa, L.JPg, L.JPa, &L.dT, L.bias0};
        const int nf[] = {9, 3, 3, 9, 9, 9, 9, 9, 1, 6};
        bool ok = all_finite(L.info9, 81);
        for (int a = 0; a < 10 && ok; a++)
            for (int k = 0; k < nf[a]; k++) ok = ok && std::isfinite(f[a][k]);
        if (!ok) return fail(ORBX_ERR_ARG, "problem %d: a value of link %d is not finite", idx, l);
    }
    imuinit::Structure s = imuinit::build_structure(p->n_kf, p->n_links, kf1.data(), kf2.data());
    if (s.error) return fail(ORBX_ERR_ARG, "problem %d, link %d: %s", idx, s.bad_link, imuinit::structure_error_text(s.error));
    if (st) *st = std::move(s);
    return ORBX_OK;
}

int optimize_batch(imu_init_solver* s, const ImuInitProblem* problems, int n_problems, ImuInitResult* results)
{
    if (!problems || !results) return fail(ORBX_ERR_ARG, "problems or results is NULL");
    if (n_problems < 1 || n_problems > IMU_INIT_MAX_BATCH) return fail(ORBX_ERR_ARG, "n_problems %d outside 1 .. %d", n_problems, IMU_INIT_MAX_BATCH);
    std::vector<imuinit::Structure> sts((size_t)n_problems);
    for (int i = 0; i < n_problems; i++)
        if (int rc = check_problem(problems + i, results + i, i, &sts[i])) return rc;
    if (!s) return fail(ORBX_ERR_ARG, "the solver is NULL");
    ORBX_HIP(hipSetDevice(s->device));
    // layout: [Dev x N][per problem: Rwb twb vel order link_in links]  ||  [Out x N][per problem: vel of the chain]  ||  scratch
    struct Off { size_t Rwb, twb, vel, order, link_in, links, vout, slot, D, E, Y0, Y, Z; };
    std::vector<Off> offs((size_t)n_problems);
    stage::Cursor cur;
    cur.take(sizeof(imuinit::Dev) * (size_t)n_problems);
    for (int i = 0; i < n_problems; i++) {
        const size_t n = (size_t)problems[i].n_kf, nc = sts[i].order.size();
        Off& o = offs[i];
        o.Rwb = cur.take(72 * n); o.twb = cur.take(24 * n); o.vel = cur.take(24 * n);
        o.order = cur.take(4 * nc); o.link_in = cur.take(4 * nc);
        o.links = cur.take(sizeof(LibaLink) * (size_t)problems[i].n_links);
    }
    const size_t up_bytes = cur.pos;
    const size_t res_off = cur.take(sizeof(imuinit::Out) * (size_t)n_problems);
    for (int i = 0; i < n_problems; i++) offs[i].vout = cur.take(24 * sts[i].order.size());
    const size_t down_end = cur.pos;
    for (int i = 0; i < n_problems; i++) {
        const size_t nc = sts[i].order.size() + 1;          // (+ 1: the slot a last position's thread forms an address of)
        Off& o = offs[i];
        o.slot = cur.take(8 * imuinit::kSlot * nc);
        o.D = cur.take(72 * nc); o.E = cur.take(72 * nc);
        o.Y0 = cur.take(240 * nc); o.Y = cur.take(240 * nc); o.Z = cur.take(240 * nc);
    }
    if (int rc = stage::reserve(*s, down_end, cur.pos)) return rc;
    uint8_t* const base = s->d_blob;
    imuinit::Dev* const descs = (imuinit::Dev*)s->h_blob;
    for (int i = 0; i < n_problems; i++) {
        const ImuInitProblem& p = problems[i];
        const Off& o = offs[i];
        const size_t n = (size_t)p.n_kf, nc = sts[i].order.size();
        if (n) { std::memcpy(s->h_blob + o.Rwb, p.Rwb, 72 * n); std::memcpy(s->h_blob + o.twb, p.twb, 24 * n); std::memcpy(s->h_blob + o.vel, p.vel, 24 * n); }
        if (nc) { std::memcpy(s->h_blob + o.order, sts[i].order.data(), 4 * nc); std::memcpy(s->h_blob + o.link_in, sts[i].link_in.data(), 4 * nc); }
        if (p.n_links) std::memcpy(s->h_blob + o.links, p.links, sizeof(LibaLink) * (size_t)p.n_links);
        imuinit::Dev d;
        std::memset(&d, 0, sizeof(d));
        d.n_chain = (int32_t)nc; d.n_links = p.n_links;
        d.Rwb = (const double*)(base + o.Rwb); d.twb = (const double*)(base + o.twb); d.vel = (const double*)(base + o.vel);
        d.order = (const int32_t*)(base + o.order); d.link_in = (const int32_t*)(base + o.link_in);
        d.links = (const LibaLink*)(base + o.links);
        for (int k = 0; k < 3; k++) { d.bg[k] = p.bg[k]; d.ba[k] = p.ba[k]; }
        for (int k = 0; k < 9; k++) d.Rwg[k] = p.Rwg[k];
        d.scale = p.scale;
        d.prior_g = p.prior_g; d.prior_a = p.prior_a; d.cfg.huber_delta = p.huber_delta; d.lambda_init = p.lambda_init;
        d.max_iters = p.max_iters; d.gauss_newton = p.gauss_newton;
        d.cfg.free_vel = p.free_vel ? 1 : 0; d.cfg.free_bias = p.free_bias ? 1 : 0; d.cfg.free_gdir = p.free_gdir ? 1 : 0; d.cfg.free_scale = p.free_scale ? 1 : 0;
        d.slot = (double*)(base + o.slot); d.D = (double*)(base + o.D); d.E = (double*)(base + o.E);
        d.Y0 = (double*)(base + o.Y0); d.Y = (double*)(base + o.Y); d.Z = (double*)(base + o.Z);
        d.vel_out = (double*)(base + o.vout);
        d.out = (imuinit::Out*)(base + res_off) + i;
        descs[i] = d;
    }
    const int rr = stage::run(*s, up_bytes, res_off, down_end, [&] {
        hipLaunchKernelGGL(imuinit::k_imu_init, dim3(n_problems), dim3(imuinit::kThreads), 0, s->stream, (const imuinit::Dev*)base);
    });
    if (rr != ORBX_OK) return rr;
    for (int i = 0; i < n_problems; i++) {
        const ImuInitProblem& p = problems[i];
        ImuInitResult& r = results[i];
        const imuinit::Out& o = ((const imuinit::Out*)(s->h_blob + res_off))[i];
        // a key frame in no link has no active edge: its velocity comes back as it went in
        if (p.n_kf && r.vel_out != p.vel) std::memmove(r.vel_out, p.vel, 24 * (size_t)p.n_kf);
        const double* vo = (const double*)(s->h_blob + offs[i].vout);
        if (p.n_links && p.free_vel)
            for (size_t q = 0; q < sts[i].order.size(); q++) std::memcpy(r.vel_out + 3 * (size_t)sts[i].order[q], vo + 3 * q, 24);
        for (int k = 0; k < 3; k++) { r.bg_out[k] = o.bg[k]; r.ba_out[k] = o.ba[k]; }
        for (int k = 0; k < 9; k++) r.Rwg_out[k] = o.Rwg[k];
        r.scale_out = o.scale; r.chi2_initial = o.chi2_initial; r.chi2_final = o.chi2_final;
        std::memset(&r.stats, 0, sizeof(r.stats));
        r.stats.iterations = o.iterations; r.stats.trials = o.trials; r.stats.stop_reason = o.stop_reason;
        r.stats.lambda = o.lambda; r.stats.chi2_initial = o.chi2_initial; r.stats.chi2_final = o.chi2_final;
        for (int k = 0; k < 16; k++) r.stats.chi2_trace[k] = o.trace[k];
    }
    return ORBX_OK;
}

}  // namespace

extern "C" {

int imu_init_create(int device, imu_init_solver** out) { return stage::open(device, out); }

void imu_init_destroy(imu_init_solver* s) { stage::close(s); }

int imu_init_check(const ImuInitProblem* problem, const ImuInitResult* result)
{
    return stage::guarded("imu_init_check", [&] { return check_problem(problem, result, 0, nullptr); });
}

int imu_init_optimize_batch(imu_init_solver* s, const ImuInitProblem* problems, int n_problems, ImuInitResult* results)
{
    return stage::guarded("imu_init_optimize_batch", [&] { return optimize_batch(s, problems, n_problems, results); });
}

double imu_init_last_device_ms(const imu_init_solver* s) { return s ? (double)s->last_kernel_ms : 0.0; }

}  // extern "C"
