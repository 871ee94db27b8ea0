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
// a CSR the host builds once per call, so results do not depend on scheduling.

#include "batch_stage.h"
#include "dense_chol.h"
#include "lm_control.h"
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

static int essg_reserve(essg_solver* s, int which, size_t bytes, void** out)
{
    essg_solver::Buf& b = s->buf[which];
    bytes = std::max<size_t>(bytes, 16);
    if (b.cap < bytes) {
        if (b.p) { ORBX_HIP(hipStreamSynchronize(s->stream)); ORBX_HIP(hipFree(b.p)); b.p = nullptr; b.cap = 0; }
        ORBX_HIP(hipMalloc(&b.p, bytes));
        b.cap = bytes;
    }
    *out = b.p;
    return ORBX_OK;
}

// every check of the header, before anything touches a device; *n_free = number of free vertices
static int essg_validate(const EssgProblem* p, const EssgResult* r, int* n_free)
{
    if (!p) return fail(ORBX_ERR_ARG, "essg_optimize: NULL problem");
    if (!r) return fail(ORBX_ERR_ARG, "essg_optimize: NULL result");
    if (p->n_vertices < 1 || p->n_edges < 0 || p->n_points < 0) return fail(ORBX_ERR_ARG, "essg_optimize: bad problem sizes");
    if (!p->sim3 || !p->fixed) return fail(ORBX_ERR_ARG, "essg_optimize: NULL vertex arrays");
    if (p->n_edges > 0 && (!p->edge_vertices || !p->edge_measurement)) return fail(ORBX_ERR_ARG, "essg_optimize: NULL edge arrays");
    if (p->n_points > 0 && (!p->points || !p->point_ref)) return fail(ORBX_ERR_ARG, "essg_optimize: NULL point arrays");
    if (!r->sim3_out) return fail(ORBX_ERR_ARG, "essg_optimize: NULL sim3_out");
    if (p->n_points > 0 && !r->points_out) return fail(ORBX_ERR_ARG, "essg_optimize: NULL points_out");
    if (p->max_iters < 0) return fail(ORBX_ERR_ARG, "essg_optimize: max_iters %d is negative", p->max_iters);
    if (!(p->lambda_init > 0) || !std::isfinite(p->lambda_init)) return fail(ORBX_ERR_ARG, "essg_optimize: lambda_init must be positive and finite");
    int nf = 0;
    for (int v = 0; v < p->n_vertices; v++) {
        for (int k = 0; k < 8; k++)
            if (!std::isfinite(p->sim3[8 * (size_t)v + k])) return fail(ORBX_ERR_ARG, "essg_optimize: vertex %d is not finite", v);
        if (!(p->sim3[8 * (size_t)v + 7] > 0)) return fail(ORBX_ERR_ARG, "essg_optimize: vertex %d has a scale that is not positive", v);
        nf += p->fixed[v] ? 0 : 1;
    }
    if (nf == 0) return fail(ORBX_ERR_ARG, "essg_optimize: no free vertex");
    for (int e = 0; e < p->n_edges; e++) {
        const int a = p->edge_vertices[2 * (size_t)e], b = p->edge_vertices[2 * (size_t)e + 1];
        if (a < 0 || a >= p->n_vertices || b < 0 || b >= p->n_vertices) return fail(ORBX_ERR_ARG, "essg_optimize: edge %d has a vertex index out of range", e);
        if (a == b) return fail(ORBX_ERR_ARG, "essg_optimize: edge %d joins vertex %d to itself", e, a);
        for (int k = 0; k < 8; k++)
            if (!std::isfinite(p->edge_measurement[8 * (size_t)e + k])) return fail(ORBX_ERR_ARG, "essg_optimize: the measurement of edge %d is not finite", e);
        if (!(p->edge_measurement[8 * (size_t)e + 7] > 0)) return fail(ORBX_ERR_ARG, "essg_optimize: the measurement of edge %d has a scale that is not positive", e);
    }
    for (int k = 0; k < p->n_points; k++) {
        if (p->point_ref[k] < 0 || p->point_ref[k] >= p->n_vertices) return fail(ORBX_ERR_ARG, "essg_optimize: point %d has a reference index out of range", k);
        for (int a = 0; a < 3; a++)
            if (!std::isfinite(p->points[3 * (size_t)k + a])) return fail(ORBX_ERR_ARG, "essg_optimize: point %d is not finite", k);
    }
    if (nf > ESSG_MAX_FREE_VERTICES) return fail(ORBX_ERR_CAPACITY, "essg_optimize: %d free vertices, capacity %d", nf, ESSG_MAX_FREE_VERTICES);
    *n_free = nf;
    return ORBX_OK;
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

int essg_check(const EssgProblem* p, const EssgResult* res)
{
    int nF = 0;
    return essg_validate(p, res, &nF);
}

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
    if (!s) return (r = stage::check_device(0)) ? r : fail(ORBX_ERR_ARG, "essg_optimize: NULL solver");       // no device is an error of its own
    const auto t_start = stage::Clock::now();
    ORBX_HIP(hipSetDevice(s->device));
    const int nV = p->n_vertices, nE = p->n_edges, nP = p->n_points;
    // ---- structure: free-vertex columns and the block CSR (diagonal blocks first, then the off-diagonal ones in (row, column)
    // order; inside a block the edges in their own order) ----
    std::vector<int> col((size_t)nV);
    for (int v = 0, c = 0; v < nV; v++) col[v] = p->fixed[v] ? -1 : c++;
    std::vector<std::vector<int>> diag((size_t)nF);
    std::vector<std::pair<std::pair<int, int>, int>> off;       // ((row, column), entry)
    for (int e = 0; e < nE; e++) {
        const int ci = col[p->edge_vertices[2 * (size_t)e]], cj = col[p->edge_vertices[2 * (size_t)e + 1]];
        if (ci >= 0) diag[ci].push_back(4 * e);
        if (cj >= 0) diag[cj].push_back(4 * e + 1);
        if (ci >= 0 && cj >= 0) off.push_back(ci > cj ? std::make_pair(std::make_pair(ci, cj), 4 * e + 2) : std::make_pair(std::make_pair(cj, ci), 4 * e + 3));
    }
    std::stable_sort(off.begin(), off.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
    std::vector<int> blk_i, blk_j, blk_off, blk_ent;
    for (int c = 0; c < nF; c++) {
        blk_i.push_back(c); blk_j.push_back(c); blk_off.push_back((int)blk_ent.size());
        blk_ent.insert(blk_ent.end(), diag[c].begin(), diag[c].end());
    }
    for (size_t k = 0; k < off.size(); k++) {
        if (k == 0 || off[k].first != off[k - 1].first) { blk_i.push_back(off[k].first.first); blk_j.push_back(off[k].first.second); blk_off.push_back((int)blk_ent.size()); }
        blk_ent.push_back(off[k].second);
    }
    blk_off.push_back((int)blk_ent.size());
    const int nBlk = (int)blk_i.size();
    const int n = 7 * nF + ((7 * nF) & 1);
    const int nblk = (n + chol::NB - 1) / chol::NB;
    const bool fused = nblk <= chol::kFusedMaxBlocks;
    const size_t sys = ((size_t)n + 1) * (size_t)n;

    essg::Dev d{};
    d.nV = nV; d.nE = nE; d.nF = nF; d.n = n; d.nBlk = nBlk; d.nP = nP; d.fix_scale = p->fix_scale ? 1 : 0;
    double *est0, *estA, *estB, *S, *Lp = nullptr, *Linv;
    float *pts = nullptr, *pts_out = nullptr, *pose_q, *pose_t;
    int* ref = nullptr;
#define ESSG_BUF(which, bytes, ptr) do { void* q_ = nullptr; if ((r = essg_reserve(s, essg_solver::which, (bytes), &q_))) return r; ptr = (decltype(ptr))q_; } while (0)
    ESSG_BUF(kEst0, 64 * (size_t)nV, est0); ESSG_BUF(kEstA, 64 * (size_t)nV, estA); ESSG_BUF(kEstB, 64 * (size_t)nV, estB);
    ESSG_BUF(kMeas, 64 * (size_t)nE, d.meas); ESSG_BUF(kEv, 8 * (size_t)nE, d.ev); ESSG_BUF(kCol, 4 * (size_t)nV, d.col);
    ESSG_BUF(kRecs, 8 * (size_t)essg::kRec * nE, d.rec); ESSG_BUF(kChi, 8 * (size_t)nE, d.chi_e); ESSG_BUF(kPart, 8 * (size_t)nF, d.part);
    ESSG_BUF(kBlkI, 4 * (size_t)nBlk, d.blk_i); ESSG_BUF(kBlkJ, 4 * (size_t)nBlk, d.blk_j); ESSG_BUF(kBlkOff, 4 * ((size_t)nBlk + 1), d.blk_off);
    ESSG_BUF(kBlkEnt, 4 * blk_ent.size(), d.blk_ent);
    ESSG_BUF(kX, 8 * (size_t)n, d.x); ESSG_BUF(kBfull, 8 * (size_t)n, d.bfull);
    ESSG_BUF(kS, 8 * sys, S);
    if (fused) ESSG_BUF(kLp, 8 * sys, Lp);
    ESSG_BUF(kLinv, 8 * (size_t)nblk * chol::NB * chol::NB, Linv);
    ESSG_BUF(kPoseQ, 16 * (size_t)nV, pose_q); ESSG_BUF(kPoseT, 12 * (size_t)nV, pose_t);
    if (nP > 0) { ESSG_BUF(kPts, 12 * (size_t)nP, pts); ESSG_BUF(kRef, 4 * (size_t)nP, ref); ESSG_BUF(kPtsOut, 12 * (size_t)nP, pts_out); }
#undef ESSG_BUF
    d.scal = s->scal;
    hipStream_t st = s->stream;
    ORBX_HIP(hipMemcpyAsync(est0, p->sim3, 64 * (size_t)nV, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync(estA, est0, 64 * (size_t)nV, hipMemcpyDeviceToDevice, st));
    if (nE > 0) {
        ORBX_HIP(hipMemcpyAsync((void*)d.meas, p->edge_measurement, 64 * (size_t)nE, hipMemcpyHostToDevice, st));
        ORBX_HIP(hipMemcpyAsync((void*)d.ev, p->edge_vertices, 8 * (size_t)nE, hipMemcpyHostToDevice, st));
    }
    ORBX_HIP(hipMemcpyAsync((void*)d.col, col.data(), 4 * (size_t)nV, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync((void*)d.blk_i, blk_i.data(), 4 * (size_t)nBlk, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync((void*)d.blk_j, blk_j.data(), 4 * (size_t)nBlk, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync((void*)d.blk_off, blk_off.data(), 4 * ((size_t)nBlk + 1), hipMemcpyHostToDevice, st));
    if (!blk_ent.empty()) ORBX_HIP(hipMemcpyAsync((void*)d.blk_ent, blk_ent.data(), 4 * blk_ent.size(), hipMemcpyHostToDevice, st));
    if (nP > 0) {
        ORBX_HIP(hipMemcpyAsync(pts, p->points, 12 * (size_t)nP, hipMemcpyHostToDevice, st));
        ORBX_HIP(hipMemcpyAsync(ref, p->point_ref, 4 * (size_t)nP, hipMemcpyHostToDevice, st));
    }
    ORBX_HIP(hipStreamSynchronize(st));         // the host vectors above go out of use here
    const auto t_uploaded = stage::Clock::now();
    ORBX_HIP(hipEventRecord(s->ev0, st));

    double* est[2] = {estA, estB};
    int cur = 0;
    double chi_cur = 0;
    bool have_chi = false;
    const dim3 items((std::max(nV, nE) + 255) / 256);
    lm::Levenberg ctl(p->max_iters);
    while (!ctl.capped()) {
        if (!ctl.begin_iteration(stop_flag && *stop_flag)) break;
        if (nE > 0) hipLaunchKernelGGL(essg::k_essg_linearize, dim3((nE + essg::kLinGroups - 1) / essg::kLinGroups), dim3(256), 0, st, d, (const double*)est[cur]);
        if (!have_chi) {        // later iterations start from an accepted trial, whose chi2 is the same sum of the same terms
            hipLaunchKernelGGL(essg::k_essg_reduce, dim3(1), dim3(1024), 0, st, d, 0, s->hs.d, ++s->hs.seq);
            ORBX_HIP(hipGetLastError());
            if ((r = s->hs.wait(st))) return r;
            chi_cur = s->hs.h[0];
            have_chi = true;
        }
        ctl.linearized(chi_cur, p->lambda_init);
        bool stopped = false;
        do {
            const double lambda = ctl.lambda();
            ORBX_HIP(hipMemsetAsync(S, 0, 8 * sys, st));
            hipLaunchKernelGGL(essg::k_essg_assemble, dim3(nBlk + 1), dim3(64), 0, st, d, S, lambda);
            chol::enqueue_factor(st, S, Lp, n, nblk, Linv, d.scal, s->flow, &s->flow_epoch);
            chol::enqueue_solve(st, S, Lp, n, nblk, Linv, d.x, d.scal);
            hipLaunchKernelGGL(essg::k_essg_update_errors, items, dim3(256), 0, st, d, lambda, (const double*)est[cur], est[1 - cur]);
            hipLaunchKernelGGL(essg::k_essg_reduce, dim3(1), dim3(1024), 0, st, d, 1, s->hs.d, ++s->hs.seq);
            ORBX_HIP(hipGetLastError());
            if ((r = s->hs.wait(st))) return r;
            const double* h = s->hs.h;
            const lm::TrialStatus status = lm::trial_status(h[5]);
            if (status == lm::TrialStatus::kStalled) return fail(ORBX_ERR_INTERNAL, "essg_optimize: the factorisation stalled (a spin wait between workgroups expired)");
            if (ctl.trial(status == lm::TrialStatus::kSolved, h[0], h[3])) { cur = 1 - cur; chi_cur = h[0]; }
            stopped = stop_flag && *stop_flag;
        } while (ctl.more_trials(stopped));
        if (!ctl.end_iteration()) break;
    }
    const auto t_solved = stage::Clock::now();
    hipLaunchKernelGGL(essg::k_essg_epilogue, dim3((std::max(nV, nP) + 255) / 256), dim3(256), 0, st, d, (const double*)est0, (const double*)est[cur],
                       pose_q, pose_t, (const float*)pts, (const int*)ref, pts_out);
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipEventRecord(s->ev1, st));
    ORBX_HIP(hipMemcpyAsync(res->sim3_out, est[cur], 64 * (size_t)nV, hipMemcpyDeviceToHost, st));
    if (res->pose_q) ORBX_HIP(hipMemcpyAsync(res->pose_q, pose_q, 16 * (size_t)nV, hipMemcpyDeviceToHost, st));
    if (res->pose_t) ORBX_HIP(hipMemcpyAsync(res->pose_t, pose_t, 12 * (size_t)nV, hipMemcpyDeviceToHost, st));
    if (nP > 0) ORBX_HIP(hipMemcpyAsync(res->points_out, pts_out, 12 * (size_t)nP, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    float ms = 0;
    ORBX_HIP(hipEventElapsedTime(&ms, s->ev0, s->ev1));
    s->last_device_ms = ms;
    s->stage_ms[0] = stage::ms(t_start, t_uploaded); s->stage_ms[1] = stage::ms(t_uploaded, t_solved); s->stage_ms[2] = stage::ms(t_solved, stage::Clock::now());
    res->stats = ctl.stats();
    return ORBX_OK;
}

}  // extern "C"
