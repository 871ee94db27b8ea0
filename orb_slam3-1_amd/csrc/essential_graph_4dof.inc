// essential_graph_4dof.inc -- the pose graph of loop closing in an inertial map: Optimizer::OptimizeEssentialGraph4DoF (reference
// src/Optimizer.cc:5292-5588) between "the graph is built" and "the map is written back".  Included by lba_solver.hip right
// after essential_graph.inc, whose handle (essg_solver: stream, scratch buffers, host-mapped scalars, flow flags) and whose host
// driver (essg_validate_graph, essg_stage, essg_levenberg, essg_finish) it shares: here are the kernels, their Dev, the packing
// of the inputs and the checks of this model alone.
//
// Every vertex is a VertexPose4DoF (yaw about the world's z and a world-frame translation of the body: 4 unknowns), every edge
// an Edge4DoF (6 error components, one information matrix for all, no robust kernel, g2o's numeric Jacobian).  H is a symmetric
// matrix of 4 x 4 blocks over the free vertices, assembled densely, (n + 1) x n with the right-hand side as row n;
// n = 4 * free vertices is even, so the system needs no padding.
//
// One Levenberg trial:  memset S -> k_essg4_assemble(lambda) -> factorisation -> k_chol_solve -> k_essg4_update_errors ->
// k_essg4_reduce -> the host reads chi2, dx^T (lambda dx + b) and the failure flag and lm::Levenberg decides.
// One linearisation: k_essg4_linearize writes a record per edge (no atomics); the assembly sums a block's records in the order of
// a CSR the host builds once per call (pose_graph_structure.h).  The first linearisation's reduction also returns max diag H,
// from which lambda_0 comes when the caller sets none (computeLambdaInit: the reference sets no user lambda here).

#include "pose4dof_group.h"

namespace essg4 {

constexpr int kRec = p4g::kRec, kState = p4g::kState, kConst = p4g::kConst;
constexpr int kLinGroups = 8;           // edges per 256-thread workgroup of k_essg4_linearize (32 lanes each)
constexpr int kAsmLanes = 20;           // lanes per block of k_essg4_assemble: 16 entries and, on the diagonal, 4 components of b
constexpr int kAsmSlots = 12;           // blocks per 256-thread workgroup (240 lanes at work)

struct Dev {
    int nV, nE, nF, n, nBlk, nP;
    const double* meas;         // [nE][12] dRij, dtij
    const double* konst;        // [nV][kConst] Rwb0, Rcb, tcb
    const int* ev;              // [nE][2]
    const int* col;             // [nV] index among the free vertices, -1: fixed
    double* rec;                // [nE][kRec]
    double* chi_e;              // [nE]
    double* part;               // [nF] dx^T (lambda dx + b) per free vertex
    const int* blk_i;           // [nBlk] block row / column (free-vertex indices, row >= column); the nF diagonal blocks first
    const int* blk_j;
    const int* blk_off;         // [nBlk + 1] into blk_ent
    const int* blk_ent;         // edge * 4 + kind: 0 Hii, 1 Hjj, 2 Hij, 3 its transpose
    double* x;                  // [n] the solution
    double* bfull;              // [n] b as assembled (the factorisation consumes row n of S)
    double* scal;               // [16]; [5] the factorisation's failure flag
    double W[36];               // the information matrix of every edge
};

// 32 lanes per edge: lanes 0-15 evaluate the error with one vertex moved by +-delta along one dimension (vertex, dimension,
// sign = lane / 8, lane % 8 / 2, lane & 1), lane 16 the error itself.  Neighbouring lanes exchange their errors to form a
// Jacobian column; J and e go through LDS, the lanes share the 54 entries of W J and W e, then the 57 entries of the record.
__global__ __launch_bounds__(256) void k_essg4_linearize(Dev d, const double* __restrict__ est)
{
    __shared__ double sJ[kLinGroups][48], sWJ[kLinGroups][48], sE[kLinGroups][6], sWe[kLinGroups][6];
    const int g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int e = blockIdx.x * kLinGroups + g;
    const bool live = e < d.nE;
    double err[6] = {0, 0, 0, 0, 0, 0};
    if (live) {
        const int vi = d.ev[2 * e], vj = d.ev[2 * e + 1];
        const int side = l >> 3, dim = (l & 7) >> 1;
        const bool fixed_side = (side ? d.col[vj] : d.col[vi]) < 0;
        if ((l < 16 && !fixed_side) || l == 16) {
            double M[12];
            for (int k = 0; k < 12; k++) M[k] = d.meas[12 * (size_t)e + k];
            p4g::edge_error_perturbed(M, est + kState * (size_t)vi, d.konst + kConst * (size_t)vi, est + kState * (size_t)vj, d.konst + kConst * (size_t)vj,
                                      side, l == 16 ? -1 : dim, l & 1, err);
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) {
        const double other = __shfl_xor(err[k], 1, 32);
        if (l < 16 && !(l & 1)) sJ[g][k * 8 + (l >> 1)] = p4g::kScalar * (err[k] - other);
        if (l == 16) sE[g][k] = err[k];
    }
    __syncthreads();
    for (int o = l; o < 54; o += 32) {
        if (o < 48) sWJ[g][o] = p4g::weighted(d.W, sJ[g] + (o & 7), 8, o >> 3);
        else sWe[g][o - 48] = p4g::weighted(d.W, sE[g], 1, o - 48);
    }
    __syncthreads();
    if (!live) return;
    for (int o = l; o < kRec; o += 32) {
        const double v = p4g::record_entry(sJ[g], sWJ[g], sE[g], sWe[g], o);
        d.rec[(size_t)e * kRec + o] = v;
        if (o == p4g::kRecChi) d.chi_e[e] = v;
    }
}

// entry (r, c) of diagonal block cf as the assembly sums it, before lambda is added
__device__ __forceinline__ double diag_entry(const Dev& d, int cf, int q)
{
    double v = 0;
    for (int k = d.blk_off[cf]; k < d.blk_off[cf + 1]; k++) {
        const int ent = d.blk_ent[k];
        v += d.rec[(size_t)(ent >> 2) * kRec + ((ent & 3) == 0 ? p4g::kRecHii : p4g::kRecHjj) + q];
    }
    return v;
}

// kAsmLanes lanes per block of the system, kAsmSlots blocks per workgroup: lanes 0-15 of a slot own an entry, lanes 16-19 of a
// diagonal block a component of b.  The last thread of the first workgroup (it has no slot) clears the failure flag of the trial.
__global__ __launch_bounds__(256) void k_essg4_assemble(Dev d, double* __restrict__ S, double lambda)
{
    const int t = threadIdx.x, slot = t / kAsmLanes, q = t - kAsmLanes * slot, n = d.n;
    if (blockIdx.x == 0 && t == 255) d.scal[5] = 0.0;
    const int b = blockIdx.x * kAsmSlots + slot;
    if (slot >= kAsmSlots || b >= d.nBlk) return;
    const int bi = d.blk_i[b], bj = d.blk_j[b];
    if (q < 16) {
        const int r = q >> 2, c = q & 3;
        double v = 0;
        if (bi == bj) {
            v = diag_entry(d, bi, q);
            if (r == c) v += lambda;
        } else {
            for (int k = d.blk_off[b]; k < d.blk_off[b + 1]; k++) {
                const int ent = d.blk_ent[k];
                v += d.rec[(size_t)(ent >> 2) * kRec + p4g::kRecHij + ((ent & 3) == 2 ? q : 4 * c + r)];
            }
            S[(size_t)(4 * bj + c) * n + 4 * bi + r] = v;
        }
        S[(size_t)(4 * bi + r) * n + 4 * bj + c] = v;
    } else if (bi == bj) {
        const int r = q - 16;
        double v = 0;
        for (int k = d.blk_off[b]; k < d.blk_off[b + 1]; k++) {
            const int ent = d.blk_ent[k];
            v += d.rec[(size_t)(ent >> 2) * kRec + ((ent & 3) == 0 ? p4g::kRecBi : p4g::kRecBj) + r];
        }
        S[(size_t)n * n + 4 * bi + r] = v;
        d.bfull[4 * bi + r] = v;
    }
}

// the trial state of vertex v: oplusImpl(dx) on the estimate, a fixed vertex as it is
__device__ __forceinline__ void trial_state(const Dev& d, const double* __restrict__ est, int v, double* out)
{
    const int col = d.col[v];
    if (col < 0) { for (int k = 0; k < kState; k++) out[k] = est[kState * (size_t)v + k]; return; }
    double u[4];
    for (int k = 0; k < 4; k++) u[k] = d.x[4 * (size_t)col + k];
    p4g::oplus(est + kState * (size_t)v, d.konst + kConst * (size_t)v, u, out);
}

// thread i: vertex i's trial state and its part of dx^T (lambda dx + b); edge i's chi2 at the trial state (it forms the trial
// states of its two vertices itself: the same calls on the same inputs, so no second launch has to wait for the first)
__global__ __launch_bounds__(256) void k_essg4_update_errors(Dev d, double lambda, const double* __restrict__ est, double* __restrict__ est_new)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.nV) {
        double T[kState];
        trial_state(d, est, i, T);
        for (int k = 0; k < kState; k++) est_new[kState * (size_t)i + k] = T[k];
        const int col = d.col[i];
        if (col >= 0) {
            double sc = 0;
            for (int a = 0; a < 4; a++) { const double xa = d.x[4 * (size_t)col + a]; sc += xa * (lambda * xa + d.bfull[4 * (size_t)col + a]); }
            d.part[col] = sc;
        }
    }
    if (i < d.nE) {
        double M[12], Ti[kState], Tj[kState], e[6];
        for (int k = 0; k < 12; k++) M[k] = d.meas[12 * (size_t)i + k];
        trial_state(d, est, d.ev[2 * i], Ti);
        trial_state(d, est, d.ev[2 * i + 1], Tj);
        p4g::edge_error(M, Ti + p4g::kRcw, Ti + p4g::kTcw, Tj + p4g::kRcw, Tj + p4g::kTcw, e);
        d.chi_e[i] = p4g::chi2(d.W, e);
    }
}

// chi2 over the edges, (what & 1) the scale sum over the free vertices, (what & 2) max diag H over the free unknowns; each
// thread a strided partial, then a fixed tree; published to the host like k_essg_reduce does
__global__ __launch_bounds__(1024) void k_essg4_reduce(Dev d, int what, double* __restrict__ hmap, unsigned long long seq)
{
    __shared__ double s_a[16], s_b[16], s_c[16];
    const int tid = threadIdx.x;
    double a = 0, b = 0, c = 0;
    for (int i = tid; i < d.nE; i += 1024) a += d.chi_e[i];
    if (what & 1) for (int i = tid; i < d.nF; i += 1024) b += d.part[i];
    if (what & 2) for (int i = tid; i < 4 * d.nF; i += 1024) c = fmax(c, fabs(diag_entry(d, i >> 2, 5 * (i & 3))));
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); c = fmax(c, __shfl_xor(c, o)); }
    if ((tid & 63) == 0) { s_a[tid >> 6] = a; s_b[tid >> 6] = b; s_c[tid >> 6] = c; }
    __syncthreads();
    if (tid == 0) {
        a = 0; b = 0; c = 0;
        for (int w = 0; w < 16; w++) { a += s_a[w]; b += s_b[w]; c = fmax(c, s_c[w]); }
        hmap[0] = a; hmap[3] = b; hmap[4] = c; hmap[5] = d.scal[5];
        __threadfence_system();
        __hip_atomic_store((unsigned long long*)(hmap + 8), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// per vertex Rcw[0], tcw[0] and the pose SetPose receives (:5555-5562): Quaterniond(Ri) normalised by Sophus::SO3d's constructor,
// cast to float and normalised again by SO3f's, the translation cast to float.  Per point (:5578-5583)
// Sim3(Ri, ti, 1).inverse().map(vScw[ref].map(P)) in double, cast to float; g2o::Sim3 uses Quaterniond(Ri) as it is.
__global__ __launch_bounds__(256) void k_essg4_epilogue(Dev d, const double* __restrict__ est, const double* __restrict__ scw,
                                                        double* __restrict__ rcw_out, double* __restrict__ tcw_out,
                                                        float* __restrict__ pose_q, float* __restrict__ pose_t,
                                                        const float* __restrict__ pts, const int* __restrict__ ref, float* __restrict__ pts_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.nV) {
        const double* X = est + kState * (size_t)i;
        double q[4];
        for (int k = 0; k < 9; k++) rcw_out[9 * (size_t)i + k] = X[p4g::kRcw + k];
        for (int k = 0; k < 3; k++) tcw_out[3 * (size_t)i + k] = X[p4g::kTcw + k];
        sim3g::quat_from_R(X + p4g::kRcw, q);
        const double nd = sqrt(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
        const float x = (float)(q[0] / nd), y = (float)(q[1] / nd), z = (float)(q[2] / nd), w = (float)(q[3] / nd);
        const float nrm = sqrtf(((x * x + y * y) + z * z) + w * w);
        pose_q[4 * i] = x / nrm; pose_q[4 * i + 1] = y / nrm; pose_q[4 * i + 2] = z / nrm; pose_q[4 * i + 3] = w / nrm;
        for (int k = 0; k < 3; k++) pose_t[3 * i + k] = (float)X[p4g::kTcw + k];
    }
    if (i < d.nP) {
        const int r = ref[i];
        const double* X = est + kState * (size_t)r;
        const double P[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        double Srw[8], Swr[8], Pc[3], Pw[3];
        sim3g::quat_from_R(X + p4g::kRcw, Srw);
        for (int k = 0; k < 3; k++) Srw[4 + k] = X[p4g::kTcw + k];
        Srw[7] = 1.0;
        sim3g::map(scw + 8 * (size_t)r, P, Pc);
        sim3g::inv(Srw, Swr);
        sim3g::map(Swr, Pc, Pw);
        for (int k = 0; k < 3; k++) pts_out[3 * i + k] = (float)Pw[k];
    }
}

}  // namespace essg4

static int essg4_validate(const Essg4DofProblem* p, const Essg4DofResult* r, int* n_free)
{
    return essg_validate_graph("essg_optimize_4dof", p, r, n_free,
        [&] { return !p->rcw || !p->tcw || !p->rwb || !p->twb || !p->rcb || !p->tcb || !p->fixed ? "vertex arrays"
                   : p->n_edges > 0 && (!p->edge_vertices || !p->edge_rot || !p->edge_trans) ? "edge arrays"
                   : p->n_points > 0 && (!p->points || !p->point_ref || !p->scw) ? "point arrays"
                   : !r->rcw_out || !r->tcw_out ? "rcw_out / tcw_out" : (const char*)nullptr; },
        [&] {
            if (!std::isfinite(p->lambda_init)) return fail(ORBX_ERR_ARG, "essg_optimize_4dof: lambda_init is not finite");
            for (int a = 0; a < 6; a++) {
                for (int b = 0; b < 6; b++) {
                    if (!std::isfinite(p->information[6 * a + b])) return fail(ORBX_ERR_ARG, "essg_optimize_4dof: the information matrix is not finite");
                    if (p->information[6 * a + b] != p->information[6 * b + a]) return fail(ORBX_ERR_ARG, "essg_optimize_4dof: the information matrix is not symmetric");
                }
                if (!(p->information[7 * a] > 0)) return fail(ORBX_ERR_ARG, "essg_optimize_4dof: the information matrix has a diagonal entry that is not positive");
            }
            return (int)ORBX_OK;
        },
        [&](int v) {
            const size_t v3 = 3 * (size_t)v, v9 = 9 * (size_t)v;
            const bool ok = essg_finite(p->rcw + v9, 9) && essg_finite(p->rwb + v9, 9) && essg_finite(p->rcb + v9, 9) &&
                            essg_finite(p->tcw + v3, 3) && essg_finite(p->twb + v3, 3) && essg_finite(p->tcb + v3, 3);
            return ok ? ORBX_OK : fail(ORBX_ERR_ARG, "essg_optimize_4dof: vertex %d is not finite", v);
        },
        [&](int e) {
            const bool ok = essg_finite(p->edge_rot + 9 * (size_t)e, 9) && essg_finite(p->edge_trans + 3 * (size_t)e, 3);
            return ok ? ORBX_OK : fail(ORBX_ERR_ARG, "essg_optimize_4dof: the measurement of edge %d is not finite", e);
        },
        [&] {
            int rc = ORBX_OK;
            for (int v = 0; v < p->n_vertices && p->n_points > 0 && !rc; v++) rc = essg_check_sim3("essg_optimize_4dof", p->scw + 8 * (size_t)v, "scw of vertex", v);
            return rc;
        });
}

extern "C" {

int essg_check_4dof(const Essg4DofProblem* p, const Essg4DofResult* res) { return essg4_validate(p, res, nullptr); }

int essg_optimize_4dof(essg_solver* s, const Essg4DofProblem* p, Essg4DofResult* res, const volatile uint8_t* stop_flag)
{
    int nF = 0;
    int r = essg4_validate(p, res, &nF);
    if (r) return r;
    EssgCall c{"essg_optimize_4dof"};
    const int nV = p->n_vertices, nE = p->n_edges, nP = p->n_points;
    constexpr int kState = essg4::kState, kConst = essg4::kConst;
    // ---- the vertices as the kernels take them: the estimate (DR = I, its = 0) and what stays constant; the edges' dRij | dtij ----
    std::vector<double> state((size_t)nV * kState), konst((size_t)nV * kConst), meas((size_t)nE * 12);
    for (int v = 0; v < nV; v++) {
        double* X = state.data() + (size_t)v * kState;
        double* K = konst.data() + (size_t)v * kConst;
        X[p4g::kC] = 1.0; X[p4g::kS] = 0.0; X[p4g::kIts] = 0.0;
        for (int k = 0; k < 3; k++) { X[p4g::kTwb + k] = p->twb[3 * (size_t)v + k]; X[p4g::kTcw + k] = p->tcw[3 * (size_t)v + k]; K[p4g::kTcb + k] = p->tcb[3 * (size_t)v + k]; }
        for (int k = 0; k < 9; k++) { X[p4g::kRcw + k] = p->rcw[9 * (size_t)v + k]; K[p4g::kRwb0 + k] = p->rwb[9 * (size_t)v + k]; K[p4g::kRcb + k] = p->rcb[9 * (size_t)v + k]; }
    }
    for (int e = 0; e < nE; e++) {
        for (int k = 0; k < 9; k++) meas[12 * (size_t)e + k] = p->edge_rot[9 * (size_t)e + k];
        for (int k = 0; k < 3; k++) meas[12 * (size_t)e + 9 + k] = p->edge_trans[3 * (size_t)e + k];
    }
    essg4::Dev d{};
    for (int k = 0; k < 36; k++) d.W[k] = p->information[k];
    double *scw = nullptr, *rcw_out = nullptr, *tcw_out = nullptr;
    r = essg_stage(s, p, 4 * nF, kState, essg4::kRec, d, c, [&](hipStream_t st) {
        using B = essg_solver;
        int q;
        if ((q = essg_reserve(s, B::kConst4, 8 * konst.size(), &d.konst)) || (q = essg_reserve(s, B::kMeas, 8 * meas.size(), &d.meas)) ||
            (q = essg_reserve(s, B::kRcwOut4, 72 * (size_t)nV, &rcw_out)) || (q = essg_reserve(s, B::kTcwOut4, 24 * (size_t)nV, &tcw_out)) ||
            (nP > 0 && (q = essg_reserve(s, B::kScw4, 64 * (size_t)nV, &scw))))
            return q;
        ORBX_HIP(hipMemcpyAsync(c.est[0], state.data(), 8 * state.size(), hipMemcpyHostToDevice, st));
        ORBX_HIP(hipMemcpyAsync((void*)d.konst, konst.data(), 8 * konst.size(), hipMemcpyHostToDevice, st));
        if (nE > 0) ORBX_HIP(hipMemcpyAsync((void*)d.meas, meas.data(), 8 * meas.size(), hipMemcpyHostToDevice, st));
        if (nP > 0) ORBX_HIP(hipMemcpyAsync(scw, p->scw, 64 * (size_t)nV, hipMemcpyHostToDevice, st));
        return (int)ORBX_OK;
    });
    if (r) return r;
    hipStream_t st = s->stream;
    r = essg_levenberg(s, d, c, p->max_iters, stop_flag, 2,
        [&](const double* est) { hipLaunchKernelGGL(essg4::k_essg4_linearize, dim3((nE + essg4::kLinGroups - 1) / essg4::kLinGroups), dim3(256), 0, st, d, est); },
        [&](int what) { hipLaunchKernelGGL(essg4::k_essg4_reduce, dim3(1), dim3(1024), 0, st, d, what, s->hs.d, ++s->hs.seq); },
        [&](double* S, double lambda) { hipLaunchKernelGGL(essg4::k_essg4_assemble, dim3((d.nBlk + essg4::kAsmSlots - 1) / essg4::kAsmSlots), dim3(256), 0, st, d, S, lambda); },
        [&](double lambda, const double* est, double* est_new) { hipLaunchKernelGGL(essg4::k_essg4_update_errors, dim3((std::max(nV, nE) + 255) / 256), dim3(256), 0, st, d, lambda, est, est_new); },
        [&](const double* h) { return lm::initial_lambda(p->lambda_init, h[4], 0.0); });      // max diag H of the first linearisation
    if (r) return r;
    hipLaunchKernelGGL(essg4::k_essg4_epilogue, dim3((std::max(nV, nP) + 255) / 256), dim3(256), 0, st, d, (const double*)c.est[c.cur], (const double*)scw,
                       rcw_out, tcw_out, c.pose_q, c.pose_t, (const float*)c.pts, (const int*)c.ref, c.pts_out);
    return essg_finish(s, c, nV, nP, res, {{res->rcw_out, rcw_out, 72 * (size_t)nV}, {res->tcw_out, tcw_out, 24 * (size_t)nV}});
}

}  // extern "C"
