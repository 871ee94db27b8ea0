// essential_graph.inc -- the pose-graph solver of loop closing and map merging: Optimizer::OptimizeEssentialGraph (reference
// src/Optimizer.cc:1501-1783, :1785-2113) between "the graph is built" and "the map is written back".  It stands on
// dense_chol.h (chol::enqueue_factor / enqueue_solve) and the host kit of batch_stage.h (stage::open / close, HostScalars), and is
// compiled as part of lba_solver.hip, the one translation unit that holds the k_chol_* kernels (dense_chol.h says why).
//
// Every vertex is a Sim3 pose (VertexSim3Expmap), every edge an EdgeSim3 with identity information and no robust kernel, so
// there is no Schur complement: H is a symmetric matrix of 7 x 7 blocks over the free vertices, assembled densely, (n + 1) x n
// with the right-hand side as row n, exactly the layout the factorisation takes.  n = 7 * free vertices, plus one decoupled
// unknown (diagonal 1, right-hand side 0) when that is odd: the factorisation loads pairs of doubles.
//
// One Levenberg trial:  memset S -> k_essg_assemble(lambda) -> factorisation -> k_chol_solve -> k_essg_update_errors ->
// k_essg_reduce -> the host reads chi2, dx^T (lambda dx + b) and the failure flag and lm::Levenberg decides.
// One linearisation: k_essg_linearize writes a record per edge (no atomics); the assembly sums a block's records in the order of
// a CSR the host builds once per call (pose_graph_structure.h), so results do not depend on scheduling.
//
// The host half of this file is the driver of BOTH pose graphs (essential_graph_4dof.inc is included after it and brings only its
// kernels, its Dev, its input packing and its own argument checks): essg_reserve, essg_validate_graph, essg_stage, essg_levenberg
// and essg_finish are templates over the Dev / problem / result types, which name what they share alike; essg_optimize below is
// their first user.

#include "batch_stage.h"
#include "dense_chol.h"
#include "lm_control.h"
#include "pose_graph_structure.h"
#include "sim3_group.h"

namespace essg {

constexpr int kRec = sim3g::kRec;
constexpr int kLinGroups = 8;           // edges per 256-thread workgroup of k_essg_linearize (32 lanes each)

struct Dev {
    int nV, nE, nF, n, nBlk, nP, fix_scale;
    const double* meas;         // [nE][8]
    const int* ev;              // [nE][2]
    const int* col;             // [nV] index among the free vertices, -1: fixed
    double* rec;                // [nE][kRec]
    double* chi_e;              // [nE]
    double* part;               // [nF] dx^T (lambda dx + b) per free vertex
    const int* blk_i;           // [nBlk] block row / column (free-vertex indices, row >= column); the nF diagonal blocks first
    const int* blk_j;
    const int* blk_off;         // [nBlk + 1] into blk_ent
    const int* blk_ent;         // edge * 4 + kind: 0 Ji^T Ji, 1 Jj^T Jj, 2 Ji^T Jj, 3 its transpose
    double* x;                  // [n] the solution
    double* bfull;              // [n] b as assembled (the factorisation consumes row n of S)
    double* scal;               // [16]; [5] the factorisation's failure flag
};

// 32 lanes per edge: lanes 0-27 evaluate the error with one vertex moved by +-delta along one dimension (vertex, dimension,
// sign = lane / 14, lane % 14 / 2, lane & 1), lane 28 the error itself.  Neighbouring lanes exchange their errors to form a
// Jacobian column; columns and error go through LDS, and the lanes share the 162 entries of the record.
__global__ __launch_bounds__(256) void k_essg_linearize(Dev d, const double* __restrict__ est)
{
    __shared__ double sJ[kLinGroups][98], sE[kLinGroups][7];
    const int g = threadIdx.x >> 5, l = threadIdx.x & 31;
    const int e = blockIdx.x * kLinGroups + g;
    const bool live = e < d.nE;
    double err[7] = {0, 0, 0, 0, 0, 0, 0};
    if (live) {
        const int vi = d.ev[2 * e], vj = d.ev[2 * e + 1];
        const int side = l / 14, dim = (l % 14) >> 1;
        const bool fixed_side = (side ? d.col[vj] : d.col[vi]) < 0;
        if ((l < 28 && !fixed_side) || l == 28) {
            double C[8], Si[8], Sj[8];
            for (int k = 0; k < 8; k++) { C[k] = d.meas[8 * (size_t)e + k]; Si[k] = est[8 * (size_t)vi + k]; Sj[k] = est[8 * (size_t)vj + k]; }
            sim3g::edge_error_perturbed(C, Si, Sj, side, l == 28 ? -1 : dim, l & 1, d.fix_scale != 0, err);
        }
    }
#pragma unroll
    for (int k = 0; k < 7; k++) {
        const double other = __shfl_xor(err[k], 1, 32);
        if (l < 28 && !(l & 1)) sJ[g][k * 14 + (l >> 1)] = sim3g::kScalar * (err[k] - other);
        if (l == 28) sE[g][k] = err[k];
    }
    __syncthreads();
    if (!live) return;
    for (int o = l; o < kRec; o += 32) {
        const double v = sim3g::record_entry(sJ[g], sE[g], o);
        d.rec[(size_t)e * kRec + o] = v;
        if (o == sim3g::kRecChi) d.chi_e[e] = v;
    }
}

// one 64-thread workgroup per block of the system: threads 0-48 own an entry, threads 49-55 of a diagonal block a component of
// b.  The last workgroup clears the failure flag of the trial and sets the decoupled unknown of an odd system.
__global__ __launch_bounds__(64) void k_essg_assemble(Dev d, double* __restrict__ S, double lambda)
{
    const int b = blockIdx.x, t = threadIdx.x, n = d.n;
    if (b == d.nBlk) {
        if (t == 0) {
            d.scal[5] = 0.0;
            if (n != 7 * d.nF) { S[(size_t)(n - 1) * n + n - 1] = 1.0; d.bfull[n - 1] = 0.0; }
        }
        return;
    }
    const int bi = d.blk_i[b], bj = d.blk_j[b];
    const int k0 = d.blk_off[b], k1 = d.blk_off[b + 1];
    if (t < 49) {
        const int r = t / 7, c = t - 7 * r;
        double v = 0;
        for (int k = k0; k < k1; k++) {
            const int ent = d.blk_ent[k], kind = ent & 3;
            const double* rec = d.rec + (size_t)(ent >> 2) * kRec;
            v += kind == 0 ? rec[sim3g::kRecHii + t] : kind == 1 ? rec[sim3g::kRecHjj + t] : kind == 2 ? rec[sim3g::kRecHij + t] : rec[sim3g::kRecHij + 7 * c + r];
        }
        if (bi == bj && r == c) v += lambda;
        S[(size_t)(7 * bi + r) * n + 7 * bj + c] = v;
        if (bi != bj) S[(size_t)(7 * bj + c) * n + 7 * bi + r] = v;
    } else if (t < 56 && bi == bj) {
        const int r = t - 49;
        double v = 0;
        for (int k = k0; k < k1; k++) {
            const int ent = d.blk_ent[k];
            const double* rec = d.rec + (size_t)(ent >> 2) * kRec;
            v += (ent & 3) == 0 ? rec[sim3g::kRecBi + r] : rec[sim3g::kRecBj + r];
        }
        S[(size_t)n * n + 7 * bi + r] = v;
        d.bfull[7 * bi + r] = v;
    }
}

// the trial state of vertex v: exp(dx) * estimate (oplusImpl), a fixed vertex as it is
__device__ __forceinline__ void trial_state(const Dev& d, const double* __restrict__ est, int v, double* out)
{
    const int col = d.col[v];
    if (col < 0) { for (int k = 0; k < 8; k++) out[k] = est[8 * (size_t)v + k]; return; }
    double S[8], u[7];
    for (int k = 0; k < 8; k++) S[k] = est[8 * (size_t)v + k];
    for (int k = 0; k < 7; k++) u[k] = d.x[7 * (size_t)col + k];
    sim3g::oplus(S, u, d.fix_scale != 0, out);
}

// thread i: vertex i's trial state and its part of dx^T (lambda dx + b); edge i's error at the trial state (it forms the trial
// states of its two vertices itself: the same calls on the same inputs, so no second launch has to wait for the first)
__global__ __launch_bounds__(256) void k_essg_update_errors(Dev d, double lambda, const double* __restrict__ est, double* __restrict__ est_new)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.nV) {
        double T[8];
        trial_state(d, est, i, T);
        for (int k = 0; k < 8; k++) est_new[8 * (size_t)i + k] = T[k];
        const int col = d.col[i];
        if (col >= 0) {
            double sc = 0;
            for (int a = 0; a < 7; a++) { const double xa = d.x[7 * (size_t)col + a]; sc += xa * (lambda * xa + d.bfull[7 * (size_t)col + a]); }
            d.part[col] = sc;
        }
    }
    if (i < d.nE) {
        double C[8], Ti[8], Tj[8], e[7];
        for (int k = 0; k < 8; k++) C[k] = d.meas[8 * (size_t)i + k];
        trial_state(d, est, d.ev[2 * i], Ti);
        trial_state(d, est, d.ev[2 * i + 1], Tj);
        sim3g::edge_error(C, Ti, Tj, e);
        double chi = 0;
        for (int k = 0; k < 7; k++) chi += e[k] * e[k];
        d.chi_e[i] = chi;
    }
}

// chi2 over the edges and (with_scale) the scale sum over the free vertices, each thread a strided partial, then a fixed tree;
// published to the host like k_reduce does
__global__ __launch_bounds__(1024) void k_essg_reduce(Dev d, int with_scale, double* __restrict__ hmap, unsigned long long seq)
{
    __shared__ double s_a[16], s_b[16];
    const int tid = threadIdx.x;
    double a = 0, b = 0;
    for (int i = tid; i < d.nE; i += 1024) a += d.chi_e[i];
    if (with_scale) for (int i = tid; i < d.nF; i += 1024) b += d.part[i];
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); b += __shfl_xor(b, o); }
    if ((tid & 63) == 0) { s_a[tid >> 6] = a; s_b[tid >> 6] = b; }
    __syncthreads();
    if (tid == 0) {
        a = 0; b = 0;
        for (int w = 0; w < 16; w++) { a += s_a[w]; b += s_b[w]; }
        hmap[0] = a; hmap[3] = b; hmap[5] = d.scal[5];
        __threadfence_system();
        __hip_atomic_store((unsigned long long*)(hmap + 8), seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

// SE3 recovery per vertex (:1735-1749: the float quaternion normalised as Sophus::SO3f's constructor does, the float
// translation divided by the scale converted to float) and the map-point correction per point (:1771-1776, in double)
__global__ __launch_bounds__(256) void k_essg_epilogue(Dev d, const double* __restrict__ est0, const double* __restrict__ est,
                                                       float* __restrict__ pose_q, float* __restrict__ pose_t,
                                                       const float* __restrict__ pts, const int* __restrict__ ref, float* __restrict__ pts_out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < d.nV) {
        const double* S = est + 8 * (size_t)i;
        const float x = (float)S[0], y = (float)S[1], z = (float)S[2], w = (float)S[3];
        const float nrm = sqrtf(((x * x + y * y) + z * z) + w * w);
        pose_q[4 * i] = x / nrm; pose_q[4 * i + 1] = y / nrm; pose_q[4 * i + 2] = z / nrm; pose_q[4 * i + 3] = w / nrm;
        const float s = (float)S[7];
        for (int k = 0; k < 3; k++) pose_t[3 * i + k] = (float)S[4 + k] / s;
    }
    if (i < d.nP) {
        const int r = ref[i];
        const double P[3] = {(double)pts[3 * i], (double)pts[3 * i + 1], (double)pts[3 * i + 2]};
        double Swr[8], Pc[3], Pw[3];
        sim3g::map(est0 + 8 * (size_t)r, P, Pc);
        sim3g::inv(est + 8 * (size_t)r, Swr);
        sim3g::map(Swr, Pc, Pw);
        for (int k = 0; k < 3; k++) pts_out[3 * i + k] = (float)Pw[k];
    }
}

}  // namespace essg

struct essg_solver : stage::Batch {      // its stream, the two events around the device work of a call
    stage::HostScalars hs;
    unsigned* flow = nullptr;
    unsigned flow_epoch = 0;
    double* scal = nullptr;
    struct Buf { void* p = nullptr; size_t cap = 0; };
    enum { kEst0, kEstA, kEstB, kMeas, kEv, kCol, kRecs, kChi, kPart, kBlkI, kBlkJ, kBlkOff, kBlkEnt, kX, kBfull, kS, kLp, kLinv,
           kPts, kRef, kPtsOut, kPoseQ, kPoseT,
           kConst4, kScw4, kRcwOut4, kTcwOut4,      // essential_graph_4dof.inc; it takes the others as they are sized per call
           kNumBufs };
    Buf buf[kNumBufs];
    double last_device_ms = 0.0;
    double stage_ms[3] = {0, 0, 0};
    ~essg_solver()
    {
        for (auto& b : buf) if (b.p) (void)hipFree(b.p);
        if (flow) (void)hipFree(flow);
        if (scal) (void)hipFree(scal);
        hs.release();
    }
};

template <class T>
static int essg_reserve(essg_solver* s, int which, size_t bytes, T** out)
{
    essg_solver::Buf& b = s->buf[which];
    bytes = std::max<size_t>(bytes, 16);
    if (b.cap < bytes) {
        if (b.p) { ORBX_HIP(hipStreamSynchronize(s->stream)); ORBX_HIP(hipFree(b.p)); b.p = nullptr; b.cap = 0; }
        ORBX_HIP(hipMalloc(&b.p, bytes));
        b.cap = bytes;
    }
    *out = (T*)b.p;
    return ORBX_OK;
}

// ---- the host driver of a pose-graph call: P / R are the problem and result structs of an entry point, Dev its kernels' argument ----

template <class T>
static bool essg_finite(const T* a, int n)
{
    for (int k = 0; k < n; k++) if (!std::isfinite(a[k])) return false;
    return true;
}

// a Sim3 among the arguments (q, t, s): finite, with a positive scale; `what` and i name it in the message
static int essg_check_sim3(const char* name, const double* S, const char* what, int i)
{
    if (!essg_finite(S, 8)) return fail(ORBX_ERR_ARG, "%s: %s %d is not finite", name, what, i);
    return S[7] > 0 ? ORBX_OK : fail(ORBX_ERR_ARG, "%s: %s %d has a scale that is not positive", name, what, i);
}

// Every check of the header, before anything touches a device, in the order the tests pin; *n_free (may be NULL) = number of free vertices.
// The model supplies arrays() = the group of its pointers that holds a NULL (or nullptr), constants() = its checks of scalars,
// vertex(v) / edge(e) = its checks of one vertex / of one edge's measurement, last() = what it checks after the points.
template <class P, class R, class Arrays, class Constants, class Vertex, class Edge, class Last>
static int essg_validate_graph(const char* name, const P* p, const R* r, int* n_free, Arrays&& arrays, Constants&& constants, Vertex&& vertex, Edge&& edge, Last&& last)
{
    if (!p) return fail(ORBX_ERR_ARG, "%s: NULL problem", name);
    if (!r) return fail(ORBX_ERR_ARG, "%s: NULL result", name);
    if (p->n_vertices < 1 || p->n_edges < 0 || p->n_points < 0) return fail(ORBX_ERR_ARG, "%s: bad problem sizes", name);
    if (const char* what = arrays()) return fail(ORBX_ERR_ARG, "%s: NULL %s", name, what);
    if (p->n_points > 0 && !r->points_out) return fail(ORBX_ERR_ARG, "%s: NULL points_out", name);
    if (p->max_iters < 0) return fail(ORBX_ERR_ARG, "%s: max_iters %d is negative", name, p->max_iters);
    int rc = constants(), nf = 0;
    if (rc) return rc;
    for (int v = 0; v < p->n_vertices; v++) {
        if ((rc = vertex(v))) return rc;
        nf += p->fixed[v] ? 0 : 1;
    }
    if (nf == 0) return fail(ORBX_ERR_ARG, "%s: no free vertex", name);
    for (int e = 0; e < p->n_edges; e++) {
        const int a = p->edge_vertices[2 * (size_t)e], b = p->edge_vertices[2 * (size_t)e + 1];
        if (a < 0 || a >= p->n_vertices || b < 0 || b >= p->n_vertices) return fail(ORBX_ERR_ARG, "%s: edge %d has a vertex index out of range", name, e);
        if (a == b) return fail(ORBX_ERR_ARG, "%s: edge %d joins vertex %d to itself", name, e, a);
        if ((rc = edge(e))) return rc;
    }
    for (int k = 0; k < p->n_points; k++) {
        if (p->point_ref[k] < 0 || p->point_ref[k] >= p->n_vertices) return fail(ORBX_ERR_ARG, "%s: point %d has a reference index out of range", name, k);
        if (!essg_finite(p->points + 3 * (size_t)k, 3)) return fail(ORBX_ERR_ARG, "%s: point %d is not finite", name, k);
    }
    if ((rc = last())) return rc;
    if (nf > ESSG_MAX_FREE_VERTICES) return fail(ORBX_ERR_CAPACITY, "%s: %d free vertices, capacity %d", name, nf, ESSG_MAX_FREE_VERTICES);
    if (n_free) *n_free = nf;
    return ORBX_OK;
}

// what a call holds besides its Dev: the system's size, the buffers both graphs use, the current estimate, the marks of its stages
struct EssgCall {
    const char* name;               // the entry point, for messages
    int n = 0, nblk = 0;            // unknowns (even: the factorisation loads pairs of doubles), Cholesky blocks
    size_t sys = 0;                 // doubles of S: (n + 1) x n
    double *est[2] = {nullptr, nullptr}, *S = nullptr, *Lp = nullptr, *Linv = nullptr;
    float *pts = nullptr, *pts_out = nullptr, *pose_q = nullptr, *pose_t = nullptr;
    int* ref = nullptr;
    int cur = 0;                    // est[cur] is the estimate
    LbaStats stats{};
    stage::Clock::time_point t_start = stage::Clock::now(), t_uploaded, t_solved;
};

// Structure + upload.  Sets the fields of d that do not depend on the model, reserves what they point to and the buffers of c
// (the estimates `state` doubles a vertex, the records `rec` doubles an edge, the system n unknowns), uploads the structure
// (pose_graph_structure.h), the edges' vertices and the points.  inputs(stream) reserves and enqueues the uploads of the model's
// own arrays; the host arrays of either go out of use at the synchronisation that ends the stage.
template <class Dev, class P, class Inputs>
static int essg_stage(essg_solver* s, const P* p, int n, int state, int rec, Dev& d, EssgCall& c, Inputs&& inputs)
{
    using B = essg_solver;
    int r = ORBX_OK;
    if (!s) return (r = stage::check_device(0)) ? r : fail(ORBX_ERR_ARG, "%s: NULL solver", c.name);      // no device is an error of its own
    ORBX_HIP(hipSetDevice(s->device));
    const size_t nV = p->n_vertices, nE = p->n_edges, nP = p->n_points;
    const pgraph::Structure g = pgraph::build_structure(p->n_vertices, p->fixed, p->n_edges, p->edge_vertices);
    const size_t nF = g.n_free, nBlk = g.blk_i.size(), nEnt = g.blk_ent.size();
    d.nV = (int)nV; d.nE = (int)nE; d.nF = (int)nF; d.n = n; d.nBlk = (int)nBlk; d.nP = (int)nP; d.scal = s->scal;
    c.n = n; c.nblk = (n + chol::NB - 1) / chol::NB; c.sys = ((size_t)n + 1) * (size_t)n;
    auto buf = [&](int which, size_t bytes, auto** out) { if (!r) r = essg_reserve(s, which, bytes, out); };
    buf(B::kEstA, 8 * state * nV, &c.est[0]); buf(B::kEstB, 8 * state * nV, &c.est[1]); buf(B::kEv, 8 * nE, &d.ev); buf(B::kCol, 4 * nV, &d.col);
    buf(B::kRecs, 8 * rec * nE, &d.rec); buf(B::kChi, 8 * nE, &d.chi_e); buf(B::kPart, 8 * nF, &d.part);
    buf(B::kBlkI, 4 * nBlk, &d.blk_i); buf(B::kBlkJ, 4 * nBlk, &d.blk_j); buf(B::kBlkOff, 4 * (nBlk + 1), &d.blk_off); buf(B::kBlkEnt, 4 * nEnt, &d.blk_ent);
    buf(B::kX, 8 * (size_t)n, &d.x); buf(B::kBfull, 8 * (size_t)n, &d.bfull); buf(B::kS, 8 * c.sys, &c.S);
    if (c.nblk <= chol::kFusedMaxBlocks) buf(B::kLp, 8 * c.sys, &c.Lp);
    buf(B::kLinv, 8 * (size_t)c.nblk * chol::NB * chol::NB, &c.Linv); buf(B::kPoseQ, 16 * nV, &c.pose_q); buf(B::kPoseT, 12 * nV, &c.pose_t);
    if (nP > 0) { buf(B::kPts, 12 * nP, &c.pts); buf(B::kRef, 4 * nP, &c.ref); buf(B::kPtsOut, 12 * nP, &c.pts_out); }
    if (r) return r;
    hipStream_t st = s->stream;
    if ((r = inputs(st))) return r;
    if (nE > 0) ORBX_HIP(hipMemcpyAsync((void*)d.ev, p->edge_vertices, 8 * nE, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync((void*)d.col, g.col.data(), 4 * nV, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync((void*)d.blk_i, g.blk_i.data(), 4 * nBlk, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync((void*)d.blk_j, g.blk_j.data(), 4 * nBlk, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync((void*)d.blk_off, g.blk_off.data(), 4 * (nBlk + 1), hipMemcpyHostToDevice, st));
    if (nEnt > 0) ORBX_HIP(hipMemcpyAsync((void*)d.blk_ent, g.blk_ent.data(), 4 * nEnt, hipMemcpyHostToDevice, st));
    if (nP > 0) {
        ORBX_HIP(hipMemcpyAsync(c.pts, p->points, 12 * nP, hipMemcpyHostToDevice, st));
        ORBX_HIP(hipMemcpyAsync(c.ref, p->point_ref, 4 * nP, hipMemcpyHostToDevice, st));
    }
    ORBX_HIP(hipStreamSynchronize(st));         // the host vectors above go out of use here
    c.t_uploaded = stage::Clock::now();
    ORBX_HIP(hipEventRecord(s->ev0, st));
    return ORBX_OK;
}

// The Levenberg rounds.  The model's launches on the solver's stream: linearize(est), reduce(what) (it publishes to s->hs under
// the next sequence number), assemble(S, lambda), update_errors(lambda, est, est_new); first_what = what the reduction after the
// first linearisation computes, lambda0(h) = the first lambda from its scalars.  Leaves c.cur, c.stats and c.t_solved.
template <class Dev, class Linearize, class Reduce, class Assemble, class Update, class Lambda0>
static int essg_levenberg(essg_solver* s, const Dev& d, EssgCall& c, int max_iters, const volatile uint8_t* stop_flag, int first_what,
                          Linearize&& linearize, Reduce&& reduce, Assemble&& assemble, Update&& update_errors, Lambda0&& lambda0)
{
    hipStream_t st = s->stream;
    int r;
    double chi_cur = 0, lambda_first = 0;
    bool have_chi = false;
    lm::Levenberg ctl(max_iters);
    while (!ctl.capped()) {
        if (!ctl.begin_iteration(stop_flag && *stop_flag)) break;
        if (d.nE > 0) linearize((const double*)c.est[c.cur]);
        if (!have_chi) {        // later iterations start from an accepted trial, whose chi2 is the same sum of the same terms
            reduce(first_what);
            ORBX_HIP(hipGetLastError());
            if ((r = s->hs.wait(st))) return r;
            chi_cur = s->hs.h[0];
            lambda_first = lambda0((const double*)s->hs.h);
            have_chi = true;
        }
        ctl.linearized(chi_cur, lambda_first);
        bool stopped = false;
        do {
            const double lambda = ctl.lambda();
            ORBX_HIP(hipMemsetAsync(c.S, 0, 8 * c.sys, st));
            assemble(c.S, lambda);
            chol::enqueue_factor(st, c.S, c.Lp, c.n, c.nblk, c.Linv, d.scal, s->flow, &s->flow_epoch);
            chol::enqueue_solve(st, c.S, c.Lp, c.n, c.nblk, c.Linv, d.x, d.scal);
            update_errors(lambda, (const double*)c.est[c.cur], c.est[1 - c.cur]);
            reduce(1);
            ORBX_HIP(hipGetLastError());
            if ((r = s->hs.wait(st))) return r;
            const double* h = s->hs.h;
            const lm::TrialStatus status = lm::trial_status(h[5]);
            if (status == lm::TrialStatus::kStalled) return fail(ORBX_ERR_INTERNAL, "%s: the factorisation stalled (a spin wait between workgroups expired)", c.name);
            if (ctl.trial(status == lm::TrialStatus::kSolved, h[0], h[3])) { c.cur = 1 - c.cur; chi_cur = h[0]; }
            stopped = stop_flag && *stop_flag;
        } while (ctl.more_trials(stopped));
        if (!ctl.end_iteration()) break;
    }
    c.stats = ctl.stats();
    c.t_solved = stage::Clock::now();
    return ORBX_OK;
}

// after the epilogue launch: the end of the device work, the downloads (the model's own, then what both graphs return), the wait
// for them, the times and the stats of the call
struct EssgDownload { void* to; const void* from; size_t bytes; };
template <class R>
static int essg_finish(essg_solver* s, const EssgCall& c, size_t n_vertices, size_t n_points, R* res, std::initializer_list<EssgDownload> own)
{
    hipStream_t st = s->stream;
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipEventRecord(s->ev1, st));
    for (const EssgDownload& x : own) ORBX_HIP(hipMemcpyAsync(x.to, x.from, x.bytes, hipMemcpyDeviceToHost, st));
    if (res->pose_q) ORBX_HIP(hipMemcpyAsync(res->pose_q, c.pose_q, 16 * n_vertices, hipMemcpyDeviceToHost, st));
    if (res->pose_t) ORBX_HIP(hipMemcpyAsync(res->pose_t, c.pose_t, 12 * n_vertices, hipMemcpyDeviceToHost, st));
    if (n_points > 0) ORBX_HIP(hipMemcpyAsync(res->points_out, c.pts_out, 12 * n_points, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    float ms = 0;
    ORBX_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->last_device_ms = ms;
    s->stage_ms[0] = stage::ms(c.t_start, c.t_uploaded); s->stage_ms[1] = stage::ms(c.t_uploaded, c.t_solved); s->stage_ms[2] = stage::ms(c.t_solved, stage::Clock::now());
    res->stats = c.stats;
    return ORBX_OK;
}

static int essg_validate(const EssgProblem* p, const EssgResult* r, int* n_free)
{
    return essg_validate_graph("essg_optimize", p, r, n_free,
        [&] { return !p->sim3 || !p->fixed ? "vertex arrays"
                   : p->n_edges > 0 && (!p->edge_vertices || !p->edge_measurement) ? "edge arrays"
                   : p->n_points > 0 && (!p->points || !p->point_ref) ? "point arrays"
                   : !r->sim3_out ? "sim3_out" : (const char*)nullptr; },
        [&] { return p->lambda_init > 0 && std::isfinite(p->lambda_init) ? ORBX_OK : fail(ORBX_ERR_ARG, "essg_optimize: lambda_init must be positive and finite"); },
        [&](int v) { return essg_check_sim3("essg_optimize", p->sim3 + 8 * (size_t)v, "vertex", v); },
        [&](int e) { return essg_check_sim3("essg_optimize", p->edge_measurement + 8 * (size_t)e, "the measurement of edge", e); },
        [] { return (int)ORBX_OK; });
}

extern "C" {

int essg_create(int device, essg_solver** out)
{
    int r = stage::open(device, out);
    if (r) return r;
    essg_solver* s = *out;
    bool ok = s->hs.alloc() == ORBX_OK;
    ok = ok && hipMalloc((void**)&s->flow, chol::kFlowFlags * sizeof(unsigned)) == hipSuccess;
    ok = ok && hipMalloc((void**)&s->scal, 16 * sizeof(double)) == hipSuccess;
    ok = ok && hipMemsetAsync(s->flow, 0, chol::kFlowFlags * sizeof(unsigned), s->stream) == hipSuccess;
    ok = ok && hipMemsetAsync(s->scal, 0, 16 * sizeof(double), s->stream) == hipSuccess;
    ok = ok && chol::raise_lds_limits(chol::kMaxUnknowns) == ORBX_OK;       // (the value shard_create_impl sets: one limit, whoever sets it)
    ok = ok && hipStreamSynchronize(s->stream) == hipSuccess;
    if (!ok) {
        stage::close(s);
        *out = nullptr;
        return fail(ORBX_ERR_HIP, "essg_create: stream / buffer creation failed");
    }
    return ORBX_OK;
}

void essg_destroy(essg_solver* s) { stage::close(s); }

int essg_check(const EssgProblem* p, const EssgResult* res) { return essg_validate(p, res, nullptr); }

double essg_last_device_ms(const essg_solver* s, double* stage_ms)
{
    if (!s) return 0.0;
    if (stage_ms) for (int k = 0; k < 3; k++) stage_ms[k] = s->stage_ms[k];
    return s->last_device_ms;
}

int essg_optimize(essg_solver* s, const EssgProblem* p, EssgResult* res, const volatile uint8_t* stop_flag)
{
    int nF = 0;
    int r = essg_validate(p, res, &nF);
    if (r) return r;
    EssgCall c{"essg_optimize"};
    const int nV = p->n_vertices, nE = p->n_edges, nP = p->n_points;
    essg::Dev d{};
    d.fix_scale = p->fix_scale ? 1 : 0;
    double* est0 = nullptr;
    r = essg_stage(s, p, 7 * nF + ((7 * nF) & 1), 8, essg::kRec, d, c, [&](hipStream_t st) {
        int q;
        if ((q = essg_reserve(s, essg_solver::kEst0, 64 * (size_t)nV, &est0)) || (q = essg_reserve(s, essg_solver::kMeas, 64 * (size_t)nE, &d.meas))) return q;
        ORBX_HIP(hipMemcpyAsync(est0, p->sim3, 64 * (size_t)nV, hipMemcpyHostToDevice, st));
        ORBX_HIP(hipMemcpyAsync(c.est[0], est0, 64 * (size_t)nV, hipMemcpyDeviceToDevice, st));
        if (nE > 0) ORBX_HIP(hipMemcpyAsync((void*)d.meas, p->edge_measurement, 64 * (size_t)nE, hipMemcpyHostToDevice, st));
        return (int)ORBX_OK;
    });
    if (r) return r;
    hipStream_t st = s->stream;
    r = essg_levenberg(s, d, c, p->max_iters, stop_flag, 0,
        [&](const double* est) { hipLaunchKernelGGL(essg::k_essg_linearize, dim3((nE + essg::kLinGroups - 1) / essg::kLinGroups), dim3(256), 0, st, d, est); },
        [&](int what) { hipLaunchKernelGGL(essg::k_essg_reduce, dim3(1), dim3(1024), 0, st, d, what, s->hs.d, ++s->hs.seq); },
        [&](double* S, double lambda) { hipLaunchKernelGGL(essg::k_essg_assemble, dim3(d.nBlk + 1), dim3(64), 0, st, d, S, lambda); },
        [&](double lambda, const double* est, double* est_new) { hipLaunchKernelGGL(essg::k_essg_update_errors, dim3((std::max(nV, nE) + 255) / 256), dim3(256), 0, st, d, lambda, est, est_new); },
        [&](const double*) { return p->lambda_init; });
    if (r) return r;
    hipLaunchKernelGGL(essg::k_essg_epilogue, dim3((std::max(nV, nP) + 255) / 256), dim3(256), 0, st, d, (const double*)est0, (const double*)c.est[c.cur],
                       c.pose_q, c.pose_t, (const float*)c.pts, (const int*)c.ref, c.pts_out);
    return essg_finish(s, c, nV, nP, res, {{res->sim3_out, c.est[c.cur], 64 * (size_t)nV}});
}

}  // extern "C"
