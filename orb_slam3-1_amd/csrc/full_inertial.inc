// full_inertial.inc -- gfx950 kernels + C ABI for the numerical core of Optimizer::FullInertialBA (reference
// src/Optimizer.cc:392-811): LocalInertialBA's edges over a whole map (include/orbslam3_hip_fullba.h).  Compiled into
// lba_solver.hip behind inertial_solver.inc, whose window setup (liba_window_setup with a LibaLayout), linearisation (ki_lin),
// landmark / pose-block gathers (system_body), Schur blocks (ki_schur_blocks), state initialisation and epilogue it launches as
// they are: none of them depends on how the biases are laid out or on how many rows there are.  New here:
//   kf_system         the entries of the reduced system outside the pose blocks (liba::entry_body<true>) with a third row class, "shared": the 6 rows of the
//                     map-wide gyro / accelerometer bias of bInit.  (key-frame row, shared column) entries are gathered over that
//                     key frame's links in link order; the 6 x 6 shared block and its 6 gradient rows are sums over ALL links plus
//                     the two priors, done by one workgroup in a reduction tree whose shape depends on n_links alone
//   kf_update         the trial state behind chol::enqueue_solve (ki_solve_update prefetches for at most 480 rows): the shared
//                     step reaches every key frame's copy of the bias, so link_delta keeps reading k1.bg / k1.ba, and enters the
//                     scale sum once
//   kf_points_errors  points_errors_body for any number of links (a workgroup per 256) with the priors counted once
// The invariant of inertial_solver.inc holds: every entry of the reduced system has ONE writer that gathers its terms in a fixed
// order; no atomics on data, no accumulation into memory.  The factorisation is chol::enqueue_factor / enqueue_solve: one launch
// up to kFusedMaxBlocks tiles, a diag / panel / update launch per block column beyond.
#include <climits>

#include "../../include/orbslam3_hip_fullba.h"

static_assert(FIBA_MAX_UNKNOWNS <= chol::kMaxUnknowns, "the substitution kernel keeps the solution in LDS");

namespace fiba {

using liba::Dev;
using liba::IDyn;
using liba::IWin;
using liba::KFState;
using liba::kIwErrors;
using liba::kIwLin;
using liba::kIwTrial;
using liba::exp_so3;
using liba::mmul;
using liba::mvec;
using liba::normalize_rotation;

struct Mode {
    int shared;                     // bInit: one bias pair for the map, rows off_shared .. off_shared + 5, row_kf = nKF
    int kb;                         // a key frame that holds a copy of the shared bias
    int off_shared, link_blocks;
    double prior_g, prior_a;
};
constexpr int kThreads = 256;

// the shared block: 36 entries and 6 gradient rows, each the sum over all links of the link's G1 / A1 part.  Thread t adds links
// t, t + 256, ... in that order, the 64 lanes of a wave a butterfly, thread 0 the four waves; then the prior (information
// prior I, error = estimate - 0) and lambda
__device__ __forceinline__ void shared_block_body(const IWin& w, const IDyn& y, const Mode& m)
{
    __shared__ double s_w[kThreads / 64];
    const Dev& d = w.d;
    const int tid = threadIdx.x, np = d.npad, os = m.off_shared;
    const KFState& kb = w.st[y.cur][m.kb];
    for (int q = 0; q < 42; q++) {
        const int a = q < 36 ? q / 6 : q - 36, c = q < 36 ? q - 6 * a : -1;
        double v = 0;
        for (int l = tid; l < d.nLinks; l += kThreads) v += c >= 0 ? d.lH[576 * (size_t)l + (9 + a) * 24 + 9 + c] : d.lb[24 * (size_t)l + 9 + a];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if ((tid & 63) == 0) s_w[tid >> 6] = v;
        __syncthreads();
        if (tid == 0) {
            double tot = ((s_w[0] + s_w[1]) + s_w[2]) + s_w[3];
            const double prior = a < 3 ? m.prior_g : m.prior_a;
            if (c >= 0) {
                if (a == c) tot += prior + y.lambda;
                w.S[(size_t)(os + a) * np + os + c] = tot;
            } else {
                tot -= prior * (a < 3 ? kb.bg[a] : kb.ba[a - 3]);
                w.S[(size_t)np * np + os + a] = tot; d.bp[os + a] = tot;
            }
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kThreads) void kf_system(const IWin* __restrict__ wins, IDyn y, Mode m)
{
    static_assert(kThreads == liba::kSysThreads, "system_body is written for kSysThreads");
    const IWin& w = wins[0];
    const int bx = (int)blockIdx.x, n_gather = w.lm_blocks + w.d.nKF;
    if (bx < n_gather) { liba::system_body(w, y, bx); return; }        // (its landmark and pose-block workgroups only)
    if (bx < n_gather + w.entry_blocks) { liba::entry_body<true>(w, y, (size_t)(bx - n_gather) * kThreads + threadIdx.x); return; }
    if (m.shared) shared_block_body(w, y, m);
}

// the trial state of every key frame (oplus into the other state buffer: ImuCamPose::Update, G2oTypes.cc:230-258) with its part of
// the scale sum dx (lambda dx + b); runs behind the substitution
__global__ __launch_bounds__(kThreads) void kf_update(const IWin* __restrict__ wins, IDyn y, Mode m)
{
    const IWin& w = wins[0];
    const Dev& d = w.d;
    const int i = blockIdx.x * kThreads + threadIdx.x;
    if (i >= d.nKF) return;
    const double lambda = y.lambda;
    KFState k = w.st[y.cur][i];
    double sc = 0;
    const int op = d.off_pose[i], ov = d.off_v[i], og = d.off_g[i], oa = d.off_a[i];
    if (op >= 0) {
        const double* pu = d.x + op;
        double t[3], dR[9];
        mvec(k.Rwb, pu + 3, t);
        for (int q = 0; q < 3; q++) k.twb[q] += t[q];
        exp_so3(pu, dR);
        mmul(k.Rwb, dR, k.Rwb);
        if (++k.its >= 3) { normalize_rotation(k.Rwb); k.its = 0; }
        liba::camera_from_body(d, k);
        for (int q = 0; q < 6; q++) sc += pu[q] * (lambda * pu[q] + d.bp[op + q]);
    }
    if (ov >= 0)
        for (int q = 0; q < 3; q++) { const double xv = d.x[ov + q]; k.v[q] += xv; sc += xv * (lambda * xv + d.bp[ov + q]); }
    if (og >= 0) {
        const bool count = !m.shared || i == m.kb;             // the shared step is one vertex's: counted once
        for (int q = 0; q < 3; q++) {
            const double xg = d.x[og + q], xa = d.x[oa + q];
            k.bg[q] += xg; k.ba[q] += xa;
            if (count) sc += xg * (lambda * xg + d.bp[og + q]) + xa * (lambda * xa + d.bp[oa + q]);
        }
    }
    w.st[1 - y.cur][i] = k;
    d.part[d.nL + i] = sc;
}

// liba::points_errors_body with a workgroup per 256 links and the priors; the hand-off between workgroups is the same (agent-scope
// stores / loads of exactly the handed-off words, a ticket, no device-wide fence)
__global__ __launch_bounds__(kThreads) void kf_points_errors(const IWin* __restrict__ wins, IDyn y, Mode m, int trial_i)
{
    static_assert(kThreads == liba::kPtThreads, "eight lanes per landmark, kPtLandmarks per workgroup");
    constexpr int kPtLandmarks = liba::kPtLandmarks;
    __shared__ double s_a[kThreads / 64], s_c[kThreads / 64], s_l[kThreads / 64];
    __shared__ unsigned int s_ticket;
    const bool trial = trial_i != 0;
    const IWin& w = wins[0];
    const Dev& d = w.d;
    const int tid = threadIdx.x, sub = tid & 7, bx = (int)blockIdx.x;
    const KFState* __restrict__ st = trial ? w.st[1 - y.cur] : w.st[y.cur];
    const double* __restrict__ pts = w.pts[y.cur];
    const int n_blocks = w.lm_blocks + m.link_blocks;
    if (bx >= w.lm_blocks) {
        const int l = (bx - w.lm_blocks) * kThreads + tid;
        if (l < d.nLinks) st_agent(d.lrho + l, liba::link_chi2(d, d.links[l], st));
    } else {
        const int l = bx * kPtLandmarks + (tid >> 3);
        const bool live = l < d.nL;
        int k0 = 0, k1 = 0;
        double Xn[3] = {0, 0, 0};
        if (live) { k0 = d.l_off[l]; k1 = d.l_off[l + 1]; for (int a = 0; a < 3; a++) Xn[a] = pts[3 * (size_t)l + a]; }
        if (trial) {
            double cs[3] = {0, 0, 0};
            for (int k = k0 + sub; k < k1; k += 8) {
                const int e = d.l_edge[k];
                const int o = d.off_pose[d.e_kf[e]];
                if (o < 0) continue;
                const double* W = d.W + 18 * (size_t)e;
                double xp[6];
                for (int r = 0; r < 6; r++) xp[r] = d.x[o + r];
#pragma unroll
                for (int q = 0; q < 3; q++) { double s2 = 0; for (int r = 0; r < 6; r++) s2 += W[3 * r + q] * xp[r]; cs[q] += s2; }
            }
            for (int q = 0; q < 3; q++)
                for (int o = 4; o > 0; o >>= 1) cs[q] += __shfl_xor(cs[q], o);
            if (live) {
                const double c[3] = {d.bl[3 * (size_t)l] - cs[0], d.bl[3 * (size_t)l + 1] - cs[1], d.bl[3 * (size_t)l + 2] - cs[2]};
                const double* Di = d.Dinv + 9 * (size_t)l;
                double sc = 0;
                for (int a = 0; a < 3; a++) {
                    const double xl = Di[3 * a] * c[0] + Di[3 * a + 1] * c[1] + Di[3 * a + 2] * c[2];
                    Xn[a] += xl;
                    sc += xl * (y.lambda * xl + d.bl[3 * (size_t)l + a]);
                }
                if (sub == 0) {
                    double* pn = w.pts[1 - y.cur] + 3 * (size_t)l;
                    pn[0] = Xn[0]; pn[1] = Xn[1]; pn[2] = Xn[2];
                    st_agent(d.part + l, sc);
                }
            }
        }
        double chi_l = 0;
        for (int k = k0 + sub; k < k1; k += 8) {
            const int e = d.l_edge[k];
            const KFState& kf = st[d.e_kf[e]];
            double Xc[3];
            mvec(kf.Rcw, Xn, Xc);
            for (int i = 0; i < 3; i++) Xc[i] += kf.tcw[i];
            const double u = d.fx * Xc[0] / Xc[2] + d.cx, v = d.fy * Xc[1] / Xc[2] + d.cy;
            const bool stereo = d.e_stereo[e] != 0;
            double r0 = d.e_obs[3 * (size_t)e] - u, r1 = d.e_obs[3 * (size_t)e + 1] - v, r2 = 0;
            if (stereo) r2 = d.e_obs[3 * (size_t)e + 2] - (u - d.bf * (1 / Xc[2]));
            d.err[3 * (size_t)e] = r0; d.err[3 * (size_t)e + 1] = r1; d.err[3 * (size_t)e + 2] = r2;
            const double c = d.e_w[e] * (r0 * r0 + r1 * r1 + r2 * r2);
            const double delta = stereo ? d.huber_stereo : d.huber_mono;
            chi_l += liba::huber_rho(c, delta);
            d.rho1[e] = c <= delta * delta ? 1.0 : delta / sqrt(c);
        }
        for (int o = 4; o > 0; o >>= 1) chi_l += __shfl_xor(chi_l, o);
        if (live && sub == 0) st_agent(d.chi_part + l, chi_l);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __syncthreads();
    if (tid == 0) s_ticket = __hip_atomic_fetch_add(d.ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __syncthreads();
    if (s_ticket != (unsigned)(n_blocks - 1)) return;
    double a = 0, c = 0, lk = 0;
    for (int i = tid; i < d.nL; i += kThreads) { a += ld_agent(d.chi_part + i); if (trial) c += ld_agent(d.part + i); }
    if (trial) for (int i = tid; i < d.nKF; i += kThreads) c += d.part[d.nL + i];            // (written by the previous launch)
    for (int i = tid; i < d.nLinks; i += kThreads) lk += ld_agent(d.lrho + i);
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); c += __shfl_xor(c, o); lk += __shfl_xor(lk, o); }
    if ((tid & 63) == 0) { s_a[tid >> 6] = a; s_c[tid >> 6] = c; s_l[tid >> 6] = lk; }
    __syncthreads();
    if (tid == 0) {
        lk = ((s_l[0] + s_l[1]) + s_l[2]) + s_l[3];
        if (m.shared) {             // EdgePriorGyro / EdgePriorAcc, once
            const KFState& kb = st[m.kb];
            lk += m.prior_g * (kb.bg[0] * kb.bg[0] + kb.bg[1] * kb.bg[1] + kb.bg[2] * kb.bg[2]);
            lk += m.prior_a * (kb.ba[0] * kb.ba[0] + kb.ba[1] * kb.ba[1] + kb.ba[2] * kb.ba[2]);
        }
        a = lk + (((s_a[0] + s_a[1]) + s_a[2]) + s_a[3]); c = ((s_c[0] + s_c[1]) + s_c[2]) + s_c[3];
        const double failed = ld_agent(d.scal + 5);
        __hip_atomic_store(d.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (trial) st_agent(d.scal + 5, 0.0);
        double* hmap = w.hmap;
        if (trial) { hmap[0] = a; hmap[3] = c; hmap[5] = failed; } else hmap[6] = a;
        __threadfence_system();
        if (trial || !(y.flags & kIwTrial)) __hip_atomic_store((unsigned long long*)(hmap + 8), y.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}

}  // namespace fiba

struct fiba_solver {
    liba_solver* slot = nullptr;    // stream, arena with its pinned mirror, host-mapped scalars, window table, result buffer
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    unsigned flow_epoch = 0;
    float last_device_ms = 0.f;
};

extern "C" {

void fiba_destroy(fiba_solver* s)
{
    if (!s) return;
    if (s->slot) (void)hipSetDevice(s->slot->device);
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    liba_destroy(s->slot);
    delete s;
}

int fiba_create(int device, fiba_solver** out)
{
    if (!out) return fail(ORBX_ERR_ARG, "out is NULL");
    *out = nullptr;
    fiba_solver* s = new (std::nothrow) fiba_solver();
    if (!s) return fail(ORBX_ERR_INTERNAL, "out of host memory");
    int r = liba_create(device, &s->slot);
    if (!r && (hipEventCreate(&s->ev0) != hipSuccess || hipEventCreate(&s->ev1) != hipSuccess)) r = fail(ORBX_ERR_HIP, "event creation failed");
    if (!r) r = chol::raise_lds_limits(chol::kMaxUnknowns);        // (one limit, whoever sets it)
    if (r) { fiba_destroy(s); return r; }
    *out = s;
    return ORBX_OK;
}

double fiba_last_device_ms(const fiba_solver* s) { return s ? (double)s->last_device_ms : 0.0; }

}  // extern "C"

// What the host takes out of the problem before the device sees it (g2o activates only vertices that have an edge): the IMU
// states of a key frame in no link, the pose of a key frame with neither an observation nor a link, and the points none of whose
// observers has a free pose, with their edges.  The rest as a LibaProblem: every link robust; with a shared bias no random walks
// and the shared value in every key frame that has IMU states.
struct FibaReduced {
    std::vector<uint8_t> pose_fixed, imu_fixed, edge_stereo;
    std::vector<double> bg, ba, points, edge_obs, edge_w;
    std::vector<int32_t> edge_kf, edge_point, kept;     // kept[j] = input index of device point j
    std::vector<LibaLink> links;
    LibaProblem q;
};
static void fiba_reduce(const FibaProblem* p, FibaReduced* o)
{
    const int nKF = p->n_kf;
    std::vector<char> linked((size_t)nKF, 0), seen((size_t)nKF, 0);
    for (int l = 0; l < p->n_links; l++) { linked[p->links[l].kf1] = 1; linked[p->links[l].kf2] = 1; }
    for (int e = 0; e < p->n_edges; e++) seen[p->edge_kf[e]] = 1;
    o->pose_fixed.resize(nKF); o->imu_fixed.resize(nKF);
    o->bg.assign(p->bg, p->bg + 3 * (size_t)nKF); o->ba.assign(p->ba, p->ba + 3 * (size_t)nKF);
    for (int i = 0; i < nKF; i++) {
        o->pose_fixed[i] = p->pose_fixed[i] || (!linked[i] && !seen[i]);
        o->imu_fixed[i] = p->imu_fixed[i] || !linked[i];
        if (p->shared_bias && p->has_imu[i])
            for (int k = 0; k < 3; k++) { o->bg[3 * (size_t)i + k] = p->shared_bg[k]; o->ba[3 * (size_t)i + k] = p->shared_ba[k]; }
    }
    std::vector<int32_t> new_index((size_t)p->n_points, -1);
    std::vector<char> keep((size_t)p->n_points, 0);
    for (int e = 0; e < p->n_edges; e++) if (!o->pose_fixed[p->edge_kf[e]]) keep[p->edge_point[e]] = 1;
    for (int l = 0; l < p->n_points; l++)
        if (keep[l]) {
            new_index[l] = (int32_t)o->kept.size();
            o->kept.push_back(l);
            o->points.insert(o->points.end(), p->points + 3 * (size_t)l, p->points + 3 * (size_t)l + 3);
        }
    for (int e = 0; e < p->n_edges; e++) {
        if (!keep[p->edge_point[e]]) continue;
        o->edge_kf.push_back(p->edge_kf[e]); o->edge_point.push_back(new_index[p->edge_point[e]]);
        o->edge_obs.insert(o->edge_obs.end(), p->edge_obs + 3 * (size_t)e, p->edge_obs + 3 * (size_t)e + 3);
        o->edge_w.push_back(p->edge_inv_sigma2[e]); o->edge_stereo.push_back(p->edge_stereo[e]);
    }
    o->links.assign(p->links, p->links + p->n_links);
    for (LibaLink& L : o->links) {
        L.robust = 1;
        if (p->shared_bias) for (int k = 0; k < 9; k++) { L.info_gyro[k] = 0.0; L.info_acc[k] = 0.0; }
    }
    LibaProblem& q = o->q;
    std::memset(&q, 0, sizeof(q));
    q.n_kf = nKF; q.Rwb = p->Rwb; q.twb = p->twb; q.vel = p->vel; q.bg = o->bg.data(); q.ba = o->ba.data();
    q.pose_fixed = o->pose_fixed.data(); q.has_imu = p->has_imu; q.imu_fixed = o->imu_fixed.data();
    std::memcpy(q.Rcb, p->Rcb, sizeof(q.Rcb)); std::memcpy(q.tcb, p->tcb, sizeof(q.tcb)); std::memcpy(q.tbc, p->tbc, sizeof(q.tbc));
    q.fx = p->fx; q.fy = p->fy; q.cx = p->cx; q.cy = p->cy; q.bf = p->bf;
    q.n_points = (int)o->kept.size(); q.points = o->points.data();
    q.n_edges = (int)o->edge_kf.size(); q.edge_kf = o->edge_kf.data(); q.edge_point = o->edge_point.data(); q.edge_obs = o->edge_obs.data();
    q.edge_inv_sigma2 = o->edge_w.data(); q.edge_stereo = o->edge_stereo.data();
    q.n_links = p->n_links; q.links = o->links.data();
    q.huber_mono = p->huber_mono; q.huber_stereo = p->huber_stereo; q.huber_inertial = p->huber_inertial;
    q.lambda_init = p->lambda_init; q.max_iters = p->max_iters;
}

static int fiba_validate(const FibaProblem* p)
{
    if (!p) return fail(ORBX_ERR_ARG, "NULL problem");
    LibaProblem v;                  // the fields the two problems share, checked as liba_solve checks them (without its bound on the links)
    std::memset(&v, 0, sizeof(v));
    v.n_kf = p->n_kf; v.Rwb = p->Rwb; v.twb = p->twb; v.vel = p->vel; v.bg = p->bg; v.ba = p->ba;
    v.pose_fixed = p->pose_fixed; v.has_imu = p->has_imu; v.imu_fixed = p->imu_fixed;
    v.n_points = p->n_points; v.points = p->points;
    v.n_edges = p->n_edges; v.edge_kf = p->edge_kf; v.edge_point = p->edge_point; v.edge_obs = p->edge_obs; v.edge_inv_sigma2 = p->edge_inv_sigma2;
    v.edge_stereo = p->edge_stereo;
    v.n_links = p->n_links; v.links = p->links; v.lambda_init = p->lambda_init; v.max_iters = p->max_iters;
    if (int r = liba_validate(&v, INT_MAX)) return r;
    if (p->shared_bias) {
        if (p->n_links == 0) return fail(ORBX_ERR_ARG, "a shared bias needs at least one link");
        if (!(p->prior_g >= 0) || !(p->prior_a >= 0) || !std::isfinite(p->prior_g) || !std::isfinite(p->prior_a)) return fail(ORBX_ERR_ARG, "bad bias priors");
    }
    return ORBX_OK;
}

// the reduced unknowns as fiba_reduce and liba_window_setup will count them
static long fiba_unknowns(const FibaProblem* p)
{
    std::vector<char> linked((size_t)p->n_kf, 0), seen((size_t)p->n_kf, 0);
    for (int l = 0; l < p->n_links; l++) { linked[p->links[l].kf1] = 1; linked[p->links[l].kf2] = 1; }
    for (int e = 0; e < p->n_edges; e++) seen[p->edge_kf[e]] = 1;
    long np = p->shared_bias ? 6 : 0;
    for (int i = 0; i < p->n_kf; i++) {
        if (!p->pose_fixed[i] && (linked[i] || seen[i])) np += 6;
        if (p->has_imu[i] && !p->imu_fixed[i] && linked[i]) np += p->shared_bias ? 3 : 9;
    }
    return np;
}

extern "C" int fiba_check(const FibaProblem* p)
{
    return stage::guarded("fiba_check", [&]() {
        if (int r = fiba_validate(p)) return r;
        // (the window setup keeps n_kf x n_kf pair-count tables on the host: bound the key frames as well, fixed ones included)
        if (p->n_kf > FIBA_MAX_KF) return fail(ORBX_ERR_CAPACITY, "%d key frames exceed FIBA_MAX_KF = %d", p->n_kf, FIBA_MAX_KF);
        const long np = fiba_unknowns(p);
        if (np == 0) return fail(ORBX_ERR_ARG, "nothing to optimise");
        if (np > FIBA_MAX_UNKNOWNS) return fail(ORBX_ERR_CAPACITY, "%ld reduced unknowns exceed FIBA_MAX_UNKNOWNS = %d", np, FIBA_MAX_UNKNOWNS);
        return (int)ORBX_OK;
    });
}

static void fiba_scatter(const FibaProblem* p, const FibaOutputs* o, const liba::KFState* st, const double* pts, const std::vector<int32_t>* kept)
{
    for (int k = 0; k < p->n_kf; k++) {
        if (o->Rwb) std::memcpy(o->Rwb + 9 * (size_t)k, st ? st[k].Rwb : p->Rwb + 9 * (size_t)k, 72);
        if (o->twb) std::memcpy(o->twb + 3 * (size_t)k, st ? st[k].twb : p->twb + 3 * (size_t)k, 24);
        if (o->vel) std::memcpy(o->vel + 3 * (size_t)k, st ? st[k].v : p->vel + 3 * (size_t)k, 24);
        if (o->bg) std::memcpy(o->bg + 3 * (size_t)k, st ? st[k].bg : p->bg + 3 * (size_t)k, 24);
        if (o->ba) std::memcpy(o->ba + 3 * (size_t)k, st ? st[k].ba : p->ba + 3 * (size_t)k, 24);
    }
    if (o->points && p->n_points > 0) {
        std::memcpy(o->points, p->points, 3 * (size_t)p->n_points * 8);
        if (pts) for (size_t j = 0; j < kept->size(); j++) std::memcpy(o->points + 3 * (size_t)(*kept)[j], pts + 3 * j, 24);
    }
}

static int fiba_run(fiba_solver* s, const FibaProblem* p, const FibaOutputs* outputs, LbaStats* stats_out)
{
    auto stop = [&]() { return p->stop_flag && *p->stop_flag != 0; };
    if (stop()) {                   // :721-723: nothing is written back
        if (stats_out) { std::memset(stats_out, 0, sizeof(*stats_out)); stats_out->stop_reason = 3; stats_out->lambda = p->lambda_init; }
        if (outputs) fiba_scatter(p, outputs, nullptr, nullptr, nullptr);
        return ORBX_OK;
    }
    FibaReduced red;
    fiba_reduce(p, &red);
    liba_solver* sv = s->slot;
    hipStream_t stream = sv->stream;
    ORBX_HIP(hipSetDevice(sv->device));
    sv->release();
    LibaWindow win;
    LibaLayout lay;
    lay.large = true; lay.shared_bias = p->shared_bias != 0; lay.max_unknowns = FIBA_MAX_UNKNOWNS;
    int r = liba_window_setup(sv, &red.q, &win, lay);
    if (r) { (void)hipStreamSynchronize(stream); sv->release(); return r; }
    liba::IWin w = win.w;
    const liba::Dev& d = w.d;
    stage::PinnedOut* io = &sv->io;
    io->clear();
    io->add((size_t)d.nKF * sizeof(liba::KFState), d.nL, d.nE);
    r = io->reserve(true);
    if (!r) {
        const stage::PinnedOut::Slice o = io->slice(io->d + io->off[0], (size_t)d.nKF * sizeof(liba::KFState), d.nL, d.nE);
        w.o_st = (liba::KFState*)o.state; w.o_pts = (double*)o.points; w.o_chi2 = (double*)o.chi2; w.o_depth = o.depth;
        if (hipMemsetAsync(win.zero_block, 0, win.zero_bytes, stream) != hipSuccess) r = fail(ORBX_ERR_HIP, "memset failed");
    }
    if (!r && hipMemcpyAsync(sv->d_wins, &w, sizeof(liba::IWin), hipMemcpyHostToDevice, stream) != hipSuccess) r = fail(ORBX_ERR_HIP, "window table upload failed");
    if (r) { (void)hipStreamSynchronize(stream); sv->release(); return r; }
    fiba::Mode m;
    std::memset(&m, 0, sizeof(m));
    m.shared = lay.shared_bias;
    m.kb = p->n_links > 0 ? p->links[0].kf1 : 0;
    m.off_shared = d.np - 6;
    m.link_blocks = std::max(1, (d.nLinks + fiba::kThreads - 1) / fiba::kThreads);
    m.prior_g = p->prior_g; m.prior_a = p->prior_a;
    const liba::IWin* dw = sv->d_wins;
    const int kf_blocks = (d.nKF + fiba::kThreads - 1) / fiba::kThreads;
    hipLaunchKernelGGL(liba::ki_init_states, dim3((d.nKF + 63) / 64, 1), dim3(64), 0, stream, dw);
    (void)hipEventRecord(s->ev0, stream);
    s->flow_epoch = 0;              // (the flags were zeroed with the window)

    lm::Levenberg c(p->max_iters, p->lambda_init);
    int cur = 0;
    bool err_current = false;
    liba::IDynAll dyn;
    std::memset(&dyn, 0, sizeof(dyn));
    liba::IDyn& y = dyn.w[0];
    for (;;) {
        y.flags = 0;
        if (c.step() == lm::Levenberg::kBegin && c.begin_iteration(stop())) {
            y.flags |= liba::kIwLin;
            if (!err_current) y.flags |= liba::kIwErrors;
        }
        if (c.step() == lm::Levenberg::kLinearize || c.step() == lm::Levenberg::kTrial) y.flags |= liba::kIwTrial;
        if (!y.flags) break;
        y.lambda = c.lambda(); y.cur = cur; y.seq = ++sv->hs.seq;
        if (y.flags & liba::kIwErrors) hipLaunchKernelGGL(fiba::kf_points_errors, dim3(w.lm_blocks + m.link_blocks), dim3(fiba::kThreads), 0, stream, dw, y, m, 0);
        if (y.flags & liba::kIwLin) hipLaunchKernelGGL(liba::ki_lin, dim3(std::max(1, d.nLinks + w.edge_blocks), 1), dim3(liba::kLinThreads), 0, stream, dw, dyn);
        hipLaunchKernelGGL(fiba::kf_system, dim3(w.lm_blocks + d.nKF + w.entry_blocks + 1), dim3(fiba::kThreads), 0, stream, dw, y, m);
        hipLaunchKernelGGL(liba::ki_schur_blocks, dim3(std::max(1, d.nBlocks), 1), dim3(1024), 0, stream, dw, dyn);
        chol::enqueue_factor(stream, w.S, w.Lp, d.npad, w.nblk, w.Linv, d.scal, w.flow, &s->flow_epoch);
        chol::enqueue_solve(stream, w.S, w.Lp, d.npad, w.nblk, w.Linv, d.x, d.scal);
        hipLaunchKernelGGL(fiba::kf_update, dim3(kf_blocks), dim3(fiba::kThreads), 0, stream, dw, y, m);
        hipLaunchKernelGGL(fiba::kf_points_errors, dim3(w.lm_blocks + m.link_blocks), dim3(fiba::kThreads), 0, stream, dw, y, m, 1);
        if (hipGetLastError() != hipSuccess) { r = fail(ORBX_ERR_HIP, "launch failed"); break; }
        if ((r = sv->hs.wait(stream))) break;
        const double* h = sv->hs.h;
        if (y.flags & liba::kIwErrors) err_current = true;
        if (y.flags & liba::kIwLin) c.linearized(c.iteration() == 0 ? h[6] : c.chi2(), p->lambda_init);
        const lm::TrialStatus ts = lm::trial_status(h[5]);
        if (ts == lm::TrialStatus::kStalled) { r = fail(ORBX_ERR_INTERNAL, "fiba_solve: the factorisation stalled (a spin wait between workgroups expired)"); break; }
        if (c.trial(ts == lm::TrialStatus::kSolved, h[0], h[3])) { cur = 1 - cur; err_current = true; }
        else err_current = false;
        if (!c.more_trials(stop())) c.end_iteration();
    }
    (void)hipEventRecord(s->ev1, stream);
    if (!r) {
        y.cur = cur;
        if (stats_out) *stats_out = c.stats();
        if (outputs) {
            const int epi = (std::max({d.nE, 3 * d.nL, d.nKF * (int)(sizeof(liba::KFState) / 8)}) + 255) / 256;
            hipLaunchKernelGGL(liba::ki_epilogue, dim3(epi, 1), dim3(256), 0, stream, dw, dyn);
            ORBX_HIP_FIRST(r, hipGetLastError());
            ORBX_HIP_FIRST(r, hipMemcpyAsync(io->h, io->d, io->total(), hipMemcpyDeviceToHost, stream));
        }
        ORBX_HIP_FIRST(r, hipStreamSynchronize(stream));
        if (!r) { float ms = 0.f; if (hipEventElapsedTime(&ms, s->ev0, s->ev1) == hipSuccess) s->last_device_ms = ms; }
        if (!r && outputs) {
            const stage::PinnedOut::Slice h = io->slice(io->h + io->off[0], (size_t)d.nKF * sizeof(liba::KFState), d.nL, d.nE);
            fiba_scatter(p, outputs, (const liba::KFState*)h.state, (const double*)h.points, &red.kept);
        }
    } else {
        (void)hipStreamSynchronize(stream);
    }
    sv->release();
    return r;
}

extern "C" int fiba_solve(fiba_solver* s, const FibaProblem* problem, const FibaOutputs* outputs, LbaStats* stats)
{
    if (int r = fiba_check(problem)) return r;             // (host only: before anything touches a device)
    if (!s || !s->slot) return fail(ORBX_ERR_ARG, "solver is NULL");
    return stage::guarded("fiba_solve", [&]() { return fiba_run(s, problem, outputs, stats); });
}
