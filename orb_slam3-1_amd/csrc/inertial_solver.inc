// inertial_solver.inc -- gfx950 kernels + C ABI for the numerical core of Optimizer::LocalInertialBA (reference
// src/Optimizer.cc:2383-2958; vertices / edges of src/G2oTypes.cc, include/G2oTypes.h).  It stands on dense_chol.h (its kernels
// wrap chol::chol_flow_body / chol_solve_body), device_scope.h and the host kit of batch_stage.h (HostScalars, for_each_window,
// PinnedOut), and is compiled as part of lba_solver.hip, the one translation unit that holds the Cholesky kernels.
//
// Unknowns per key frame: body pose (6, ImuCamPose::Update: twb += Rwb ut, Rwb <- Rwb Exp(ur)), velocity, gyro bias,
// accelerometer bias (3 each); landmarks are marginalised.  The reduced system has 15 unknowns per temporal key frame (<= 25
// key frames), so everything outside the visual edges is tiny: the inertial links are linearised by one thread each and
// accumulated in link order by one thread (deterministic), the visual edges by ordered gathers exactly as in LocalBA
// (per landmark, per key frame, per pair list of a Schur block).  First version: correctness and the shared factorisation;
// no tuning yet.
#include "batch_stage.h"
#include "dense_chol.h"
#include "device_scope.h"
#include "lm_control.h"
#include "se3_device.h"
#include "imu_link_device.h"

namespace liba {

using chol::NB;

struct KFState { double Rwb[9], twb[3], v[3], bg[3], ba[3], Rcw[9], tcw[3]; int its, pad; };

struct Dev {
    int nKF, nL, nE, nLinks, np, npad, nBlocks;
    const int* off_pose; const int* off_v; const int* off_g; const int* off_a;
    const int* row_kf; const int* row_loc;      // row of the reduced system -> key frame, local index (pose 0-5, v 6-8, bg 9-11, ba 12-14); padding: -1
    const int* kl_off; const int* kl_link;      // the links of a key frame, in link order
    const int* e_kf; const int* e_point; const double* e_obs; const double* e_w; const uint8_t* e_stereo;
    const int* l_off; const int* l_edge;        // edges of a landmark
    const int* k_off; const int* k_edge;        // edges of a key frame with a free pose (by key frame index)
    const int* b_i; const int* b_j; const int* b_off; const int2* b_pair;   // key-frame pairs (i <= j) and their (edge a, edge b) lists
    const LibaLink* links;
    double* bp; double* bl; double* W; double* Z; double* Dinv;
    double* err; double* rho1;                  // [nE][3], [nE] Huber weight
    double* lrho;                               // [nLinks] robust chi2 of a link incl. its random walks
    double* lH; double* lb;                     // [nLinks][24*24], [nLinks][24]
    double* eH; double* pH;                     // per visual edge: landmark part [12], key-frame part [27]
    double* x; double* part; double* chi_part; double* scal;
    unsigned* ticket;
    double Rcb[9], tcb[3], Rbc[9], tbc[3];
    double fx, fy, cx, cy, bf, huber_mono, huber_stereo, huber_inertial;
};

__device__ inline void camera_from_body(const Dev& d, KFState& k)      // ImuCamPose::Update tail (G2oTypes.cc:249-257)
{
    double Rbw[9], tbw[3];
    mtr(k.Rwb, Rbw);
    mvec(Rbw, k.twb, tbw);
    for (int i = 0; i < 3; i++) tbw[i] = -tbw[i];
    mmul(d.Rcb, Rbw, k.Rcw);
    mvec(d.Rcb, tbw, k.tcw);
    for (int i = 0; i < 3; i++) k.tcw[i] += d.tcb[i];
}
template <typename D>
__device__ inline void camera_from_body_pi(const D& d, KFState& k)
{
    double Rbw[9], tbw[3];
    mtr(k.Rwb, Rbw);
    mvec(Rbw, k.twb, tbw);
    for (int i = 0; i < 3; i++) tbw[i] = -tbw[i];
    mmul(d.Rcb, Rbw, k.Rcw);
    mvec(d.Rcb, tbw, k.tcw);
    for (int i = 0; i < 3; i++) k.tcw[i] += d.tcb[i];
}
__device__ inline double huber_rho(double c, double delta) { const double d2 = delta * delta; return c <= d2 ? c : 2 * sqrt(c) * delta - d2; }

// Preintegrated::GetDelta*(b1) at the bias of key frame k1 (imu_link_device.h)
__device__ inline void link_delta(const LibaLink& L, const KFState& k1, double* dR, double* dV, double* dP, double* dbg_out) { link_delta(L, k1.bg, k1.ba, dR, dV, dP, dbg_out); }

// EdgeInertial::computeError (G2oTypes.cc:520-540); also returns eR and Rbw1 for the Jacobians
__device__ inline void link_error(const LibaLink& L, const KFState& k1, const KFState& k2, double* e9, double* eR, double* Rbw1, double* dbg)
{
    double dR[9], dV[3], dP[3];
    link_delta(L, k1, dR, dV, dP, dbg);
    const double dt = L.dT, g[3] = {0, 0, -9.81};
    double dRt[9], t[9], a[3], b[3];
    mtr(k1.Rwb, Rbw1); mtr(dR, dRt);
    mmul(dRt, Rbw1, t); mmul(t, k2.Rwb, eR);
    log_so3(eR, e9);
    for (int i = 0; i < 3; i++) a[i] = k2.v[i] - k1.v[i] - g[i] * dt;
    mvec(Rbw1, a, e9 + 3);
    for (int i = 0; i < 3; i++) e9[3 + i] -= dV[i];
    for (int i = 0; i < 3; i++) b[i] = k2.twb[i] - k1.twb[i] - k1.v[i] * dt - g[i] * dt * dt / 2;
    mvec(Rbw1, b, e9 + 6);
    for (int i = 0; i < 3; i++) e9[6 + i] -= dP[i];
}

// ---------------------------------------------------------------------------------------------------------------------------
// Launch structure (round 3): every kernel takes the windows of a batch (grid.y = window; liba_solve is a batch of one) and the
// per-round state of each window by value.  A linearisation is ONE launch (ki_lin: a workgroup per inertial link beside the
// visual edges), a Levenberg trial FIVE (ki_system, ki_schur_blocks, the factorisation chol::chol_flow_body, ki_solve_update,
// ki_points_errors); the first version needed twelve plus a memset, and its link kernel (one workgroup for all links, then
// colour-ordered read-modify-write accumulation into a dense matrix) alone took 45 us.  No stage accumulates into memory any more:
// every entry of the reduced system has ONE writer that gathers its terms in a fixed order.
// ---------------------------------------------------------------------------------------------------------------------------
struct IWin {
    Dev d;
    KFState* st[2]; double* pts[2];
    double* S; double* Lp; double* Linv; unsigned* flow; double* hmap;
    KFState* o_st; double* o_pts; double* o_chi2; uint8_t* o_depth;        // this window's slice of the handle's result buffer
    int nblk, edge_blocks, lm_blocks, entry_blocks;
};
struct IDyn { double lambda; unsigned long long seq; int cur, flags; };
constexpr int kMaxIBatch = 64;
struct IDynAll { IDyn w[kMaxIBatch]; };
enum { kIwErrors = 1, kIwLin = 2, kIwTrial = 4 };
constexpr int kPtThreads = 256, kPtLandmarks = kPtThreads / 8;

// robust chi2 of link l (EdgeInertial + the two random walks) at the state `st`
__device__ __forceinline__ double link_chi2(const Dev& d, const LibaLink& L, const KFState* __restrict__ st)
{
    const KFState &k1 = st[L.kf1], &k2 = st[L.kf2];
    double e[9], eR[9], Rbw1[9], dbg[3], c = 0;
    link_error(L, k1, k2, e, eR, Rbw1, dbg);
    for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) c += e[i] * L.info9[9 * i + j] * e[j];
    double chi = L.robust ? huber_rho(c, d.huber_inertial) : c;
    double eg = 0, ea = 0, dg[3], da[3];
    for (int i = 0; i < 3; i++) { dg[i] = k2.bg[i] - k1.bg[i]; da[i] = k2.ba[i] - k1.ba[i]; }
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) { eg += dg[i] * L.info_gyro[3 * i + j] * dg[j]; ea += da[i] * L.info_acc[3 * i + j] * da[j]; }
    chi += eg; chi += ea;
    return chi;
}

// ---- ki_points_errors: the tail of a trial (TRIAL: back-substitution of the landmarks into the other point buffer, scale partials)
// and the errors + robust chi2 of every edge at that state; without TRIAL the errors of the accepted state (start of a solve, after
// a rejected trial).  Eight lanes per landmark (a landmark's edges are split over them; every edge belongs to one landmark), one
// extra workgroup for the inertial links; the workgroup that finishes last sums the partials in a fixed order and publishes the
// scalars to the host (chi2 in [0] for a trial, in [6] for the accepted state).  Cross-workgroup hand-off as in
// lba::update_errors_body (agent-scope stores / loads of exactly the handed-off words, no device-wide fence).
__device__ __forceinline__ void points_errors_body(const IWin& w, const IDyn& y, const bool trial, const int bx)
{
    __shared__ double s_a[kPtThreads / 64], s_c[kPtThreads / 64];
    __shared__ unsigned int s_ticket;
    const Dev& d = w.d;
    const int tid = threadIdx.x, sub = tid & 7;
    const KFState* __restrict__ st = trial ? w.st[1 - y.cur] : w.st[y.cur];
    const double* __restrict__ pts = w.pts[y.cur];
    const int n_blocks = w.lm_blocks + 1;
    if (bx == w.lm_blocks) {
        if (tid < d.nLinks) st_agent(d.lrho + tid, link_chi2(d, d.links[tid], st));
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
            chi_l += huber_rho(c, delta);
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
    double a = 0, c = 0;
    for (int i = tid; i < d.nL; i += kPtThreads) { a += ld_agent(d.chi_part + i); if (trial) c += ld_agent(d.part + i); }
    if (trial) for (int i = tid; i < d.nKF; i += kPtThreads) c += d.part[d.nL + i];           // (written by the previous launch)
    for (int o = 32; o > 0; o >>= 1) { a += __shfl_xor(a, o); c += __shfl_xor(c, o); }
    if ((tid & 63) == 0) { s_a[tid >> 6] = a; s_c[tid >> 6] = c; }
    __syncthreads();
    if (tid == 0) {
        double lk = 0;
        for (int l = 0; l < d.nLinks; l++) lk += ld_agent(d.lrho + l);
        a = lk + (((s_a[0] + s_a[1]) + s_a[2]) + s_a[3]); c = ((s_c[0] + s_c[1]) + s_c[2]) + s_c[3];
        const double failed = ld_agent(d.scal + 5);
        __hip_atomic_store(d.ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (trial) st_agent(d.scal + 5, 0.0);           // the failure flag of this trial has been handed over
        double* hmap = w.hmap;
        if (trial) { hmap[0] = a; hmap[3] = c; hmap[5] = failed; } else hmap[6] = a;
        __threadfence_system();
        // (the errors of the accepted state are followed by a trial in most rounds: the trial publishes the round's sequence number)
        if (trial || !(y.flags & kIwTrial)) __hip_atomic_store((unsigned long long*)(hmap + 8), y.seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
__global__ __launch_bounds__(kPtThreads) void ki_points_errors(const IWin* __restrict__ wins, IDynAll dyn, int trial)
{
    const IDyn y = dyn.w[blockIdx.y];
    if (!(y.flags & (trial ? kIwTrial : kIwErrors))) return;
    const IWin& w = wins[blockIdx.y];
    if ((int)blockIdx.x > w.lm_blocks) return;
    points_errors_body(w, y, trial != 0, (int)blockIdx.x);
}

// visual Jacobians of edge e (EdgeMono / EdgeStereo::linearizeOplus, G2oTypes.cc:349-420): Ji 3 x 3 (point), Jj 3 x 6 (body pose)
__device__ inline void visual_jac(const Dev& d, const KFState& k, const double* X, bool stereo, double* Ji, double* Jj)
{
    double Xc[3], Xb[3];
    mvec(k.Rcw, X, Xc);
    for (int i = 0; i < 3; i++) Xc[i] += k.tcw[i];
    mvec(d.Rbc, Xc, Xb);
    for (int i = 0; i < 3; i++) Xb[i] += d.tbc[i];
    const double iz = 1.0 / Xc[2], iz2 = 1.0 / (Xc[2] * Xc[2]);
    double pj[9] = {d.fx * iz, 0, -d.fx * Xc[0] * iz2, 0, d.fy * iz, -d.fy * Xc[1] * iz2, 0, 0, 0};
    if (stereo) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + d.bf * iz2; }
    double pr[9];
    mmul(pj, k.Rcw, Ji);
    for (int q = 0; q < 9; q++) Ji[q] = -Ji[q];
    mmul(pj, d.Rcb, pr);
    const double x = Xb[0], y = Xb[1], z = Xb[2];
    const double D[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 6; c++) Jj[6 * r + c] = pr[3 * r] * D[c] + pr[3 * r + 1] * D[6 + c] + pr[3 * r + 2] * D[12 + c];
}

// per visual edge: W_e = w Jj^T Ji (zero when the key frame's pose is fixed) and its contributions w Ji^T Ji, -w Ji^T r to the
// landmark and w Jj^T Jj (upper triangle), -w Jj^T r to the key frame; gathered in a fixed order by ki_system
__device__ __forceinline__ void lin_edge(const Dev& d, const KFState* __restrict__ st, const double* __restrict__ pts, const int e)
{
    const int ne = d.e_stereo[e] ? 3 : 2;
    double Ji[9], Jj[18];
    visual_jac(d, st[d.e_kf[e]], pts + 3 * (size_t)d.e_point[e], ne == 3, Ji, Jj);
    const double w = d.e_w[e] * d.rho1[e];
    const double* r = d.err + 3 * (size_t)e;
    double* eh = d.eH + 12 * (size_t)e;
    for (int a = 0; a < 3; a++) {
        for (int c = 0; c < 3; c++) { double s = 0; for (int q = 0; q < ne; q++) s += Ji[3 * q + a] * Ji[3 * q + c]; eh[3 * a + c] = w * s; }
        double s = 0; for (int q = 0; q < ne; q++) s += Ji[3 * q + a] * r[q];
        eh[9 + a] = -(w * s);
    }
    const bool free_pose = d.off_pose[d.e_kf[e]] >= 0;
    double* We = d.W + 18 * (size_t)e;
    for (int a = 0; a < 6; a++)
        for (int c = 0; c < 3; c++) { double t = 0; for (int q = 0; q < ne; q++) t += Jj[6 * q + a] * Ji[3 * q + c]; We[3 * a + c] = free_pose ? w * t : 0.0; }
    double* ph = d.pH + 27 * (size_t)e;
    int idx = 0;
    for (int a = 0; a < 6; a++)
        for (int c = a; c < 6; c++, idx++) { double s = 0; for (int q = 0; q < ne; q++) s += Jj[6 * q + a] * Jj[6 * q + c]; ph[idx] = w * s; }
    for (int a = 0; a < 6; a++) { double s = 0; for (int q = 0; q < ne; q++) s += Jj[6 * q + a] * r[q]; ph[21 + a] = -(w * s); }
}

// inertial link l -> its local 24 x 24 Hessian lH and gradient lb (P1 V1 G1 A1 P2 V2 = 6 3 3 3 6 3), one workgroup per link: lane 0
// walks the error chain with the link record in LDS, then lanes of three waves the rotation rows, the velocity / position rows and
// the Huber weight side by side (the 9 x 24 Jacobian lives in LDS), then rho1 info9 J (216 entries) and J^T (rho1 info9 J)
// (576 + 24) over the threads
constexpr int kLinThreads = 256;
__device__ __forceinline__ void lin_link(const Dev& d, const KFState* __restrict__ st, const int l)
{
    __shared__ __align__(16) unsigned char s_link_raw[sizeof(LibaLink)];
    __shared__ double s_J[216], s_OJ[216], s_Oe[10];
    const int tid = threadIdx.x;
    {
        const unsigned long long* src = (const unsigned long long*)(d.links + l);
        unsigned long long* dst = (unsigned long long*)s_link_raw;
        for (int i = tid; i < (int)(sizeof(LibaLink) / 8); i += kLinThreads) dst[i] = src[i];
        for (int i = tid; i < 216; i += kLinThreads) s_J[i] = 0.0;
    }
    __syncthreads();
    const LibaLink& L = *(const LibaLink*)s_link_raw;
    __shared__ double s_e[9], s_eR[9], s_Rbw1[9], s_dbg[3];
    if (tid == 0) {         // the error chain (bias-corrected deltas, eR = dR^T Rbw1 Rwb2, its logarithm)
        double e[9], eR[9], Rbw1[9], dbg[3];
        link_error(L, st[L.kf1], st[L.kf2], e, eR, Rbw1, dbg);
        for (int k = 0; k < 9; k++) { s_e[k] = e[k]; s_eR[k] = eR[k]; s_Rbw1[k] = Rbw1[k]; }
        for (int k = 0; k < 3; k++) s_dbg[k] = dbg[k];
    }
    __syncthreads();
    // J: 9 x 24, column offsets 0 (P1) 6 (V1) 9 (G1) 12 (A1) 15 (P2) 21 (V2); three independent chains on lanes of three waves
    auto set = [&](int r0, int c0, const double* B, double sc) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) s_J[(r0 + i) * 24 + c0 + j] = sc * B[3 * i + j];
    };
    if (tid == 0) {                 // the rotation rows
        const KFState &k1 = st[L.kf1], &k2 = st[L.kf2];
        double invJr[9], er[3] = {s_e[0], s_e[1], s_e[2]}, Rbw2[9], A[9], B[9];
        inv_right_jac(er, invJr);
        mtr(k2.Rwb, Rbw2);
        mmul(Rbw2, k1.Rwb, A); mmul(invJr, A, B);
        set(0, 0, B, -1.0);
        double JRg[9], wv[3], rj[9], eRt[9], eR[9], dbg[3], C[9], D[9];
        for (int k = 0; k < 9; k++) { JRg[k] = L.JRg[k]; eR[k] = s_eR[k]; }
        for (int k = 0; k < 3; k++) dbg[k] = s_dbg[k];
        mvec(JRg, dbg, wv); right_jac(wv, rj); mtr(eR, eRt);
        mmul(invJr, eRt, C); mmul(C, rj, D); mmul(D, JRg, C);
        set(0, 9, C, -1.0);
        set(0, 15, invJr, 1.0);
    } else if (tid == 64) {         // the velocity and position rows
        const KFState &k1 = st[L.kf1], &k2 = st[L.kf2];
        const double dt = L.dT, g[3] = {0, 0, -9.81};
        double Rbw1[9], h[9], a[3], b[3], ra[3], rb[3], A[9];
        for (int k = 0; k < 9; k++) Rbw1[k] = s_Rbw1[k];
        for (int i = 0; i < 3; i++) a[i] = k2.v[i] - k1.v[i] - g[i] * dt;
        mvec(Rbw1, a, ra); skew3(ra, h); set(3, 0, h, 1.0);
        for (int i = 0; i < 3; i++) b[i] = k2.twb[i] - k1.twb[i] - k1.v[i] * dt - 0.5 * g[i] * dt * dt;
        mvec(Rbw1, b, rb); skew3(rb, h); set(6, 0, h, 1.0);
        const double I3[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        set(6, 3, I3, -1.0);
        set(3, 6, Rbw1, -1.0); set(6, 6, Rbw1, -dt);
        double JVg[9], JVa[9], JPg[9], JPa[9];
        for (int k = 0; k < 9; k++) { JVg[k] = L.JVg[k]; JVa[k] = L.JVa[k]; JPg[k] = L.JPg[k]; JPa[k] = L.JPa[k]; }
        set(3, 9, JVg, -1.0); set(6, 9, JPg, -1.0);
        set(3, 12, JVa, -1.0); set(6, 12, JPa, -1.0);
        mmul(Rbw1, k2.Rwb, A); set(6, 18, A, 1.0);
        set(3, 21, Rbw1, 1.0);
    } else if (tid == 128) {        // the Huber weight and rho1 info9 e
        double e[9], c = 0;
        for (int k = 0; k < 9; k++) e[k] = s_e[k];
        for (int i = 0; i < 9; i++) for (int j = 0; j < 9; j++) c += e[i] * L.info9[9 * i + j] * e[j];
        const double d2 = d.huber_inertial * d.huber_inertial;
        const double rho1 = (L.robust && c > d2) ? d.huber_inertial / sqrt(c) : 1.0;
        for (int r = 0; r < 9; r++) { double t = 0; for (int q = 0; q < 9; q++) t += L.info9[9 * r + q] * e[q]; s_Oe[r] = rho1 * t; }
        s_Oe[9] = rho1;
    }
    __syncthreads();
    if (tid < 216) {        // OmJ = rho1 info9 J
        const int r = tid / 24, cc = tid - r * 24;
        double t = 0;
        for (int q = 0; q < 9; q++) t += L.info9[9 * r + q] * s_J[q * 24 + cc];
        s_OJ[tid] = s_Oe[9] * t;
    }
    __syncthreads();
    for (int idx = tid; idx < 600; idx += kLinThreads) {
        if (idx < 576) {
            const int a2 = idx / 24, cc = idx - a2 * 24;
            double sacc = 0;
            for (int r = 0; r < 9; r++) sacc += s_J[r * 24 + a2] * s_OJ[r * 24 + cc];
            d.lH[576 * (size_t)l + idx] = sacc;
        } else {
            const int a2 = idx - 576;
            double sacc = 0;
            for (int r = 0; r < 9; r++) sacc += s_J[r * 24 + a2] * s_Oe[r];
            d.lb[24 * (size_t)l + a2] = -sacc;
        }
    }
}
__global__ __launch_bounds__(kLinThreads) void ki_lin(const IWin* __restrict__ wins, IDynAll dyn)
{
    const IDyn y = dyn.w[blockIdx.y];
    if (!(y.flags & kIwLin)) return;
    const IWin& w = wins[blockIdx.y];
    const Dev& d = w.d;
    const int bx = blockIdx.x;
    if (bx < d.nLinks) { lin_link(d, w.st[y.cur], bx); return; }
    const int e = (bx - d.nLinks) * kLinThreads + threadIdx.x;
    if (e < d.nE) lin_edge(d, w.st[y.cur], w.pts[y.cur], e);
}

// ---- ki_system: everything of the reduced system that does not need a pair list, one writer per entry ----
//  landmark groups (8 lanes per landmark): Hll = sum of its edges' parts, D^-1 = (Hll + lambda I)^-1, bl, Z_e = W_e D^-1
//  key-frame workgroups: the 21 + 6 sums over a free key frame's edges, then its 6 x 6 pose block and 6 gradient rows
//  entry workgroups: every other entry of S / the right-hand side row (inertial links and random walks of the key frame's links,
//  in link order; lambda on the diagonal, the identity on the padding)
__device__ __forceinline__ int link_index24(const LibaLink& L, int kf, int loc)     // column of (kf, loc) in the link's 24 (or -1)
{
    if (kf == L.kf1) return loc;
    if (kf == L.kf2 && loc < 9) return 15 + loc;
    return -1;
}
// the links' part of entry (row of key frame kr, local lr; column of kc, lc); kc < 0: the gradient entry of the row
__device__ __forceinline__ double link_terms(const Dev& d, const KFState* __restrict__ st, int kr, int lr, int kc, int lc)
{
    double v = 0;
    for (int k = d.kl_off[kr]; k < d.kl_off[kr + 1]; k++) {
        const int l = d.kl_link[k];
        const LibaLink& L = d.links[l];
        const int li = link_index24(L, kr, lr);
        if (kc >= 0) {
            if (kc != L.kf1 && kc != L.kf2) continue;
            const int lj = link_index24(L, kc, lc);
            if (li >= 0 && lj >= 0) v += d.lH[576 * (size_t)l + li * 24 + lj];
            // random walks (EdgeGyroRW / EdgeAccRW): e = b2 - b1, J1 = -I, J2 = +I
            if (lr >= 9 && lc >= 9 && (lr - 9) / 3 == (lc - 9) / 3) {
                const double* Om3 = lr >= 12 ? L.info_acc : L.info_gyro;
                const double wv = Om3[3 * ((lr - 9) % 3) + (lc - 9) % 3];
                v += (kr == kc) ? wv : -wv;
            }
        } else {
            if (li >= 0) v += d.lb[24 * (size_t)l + li];
            if (lr >= 9) {
                const double* Om3 = lr >= 12 ? L.info_acc : L.info_gyro;
                const KFState &k1 = st[L.kf1], &k2 = st[L.kf2];
                double dd[3];
                for (int q = 0; q < 3; q++) dd[q] = lr >= 12 ? k2.ba[q] - k1.ba[q] : k2.bg[q] - k1.bg[q];
                const int i = (lr - 9) % 3;
                const double Od = Om3[3 * i] * dd[0] + Om3[3 * i + 1] * dd[1] + Om3[3 * i + 2] * dd[2];
                v += (kr == L.kf1) ? Od : -Od;
            }
        }
    }
    return v;
}
constexpr int kSysThreads = 256;
// the links' part of entry (row of key frame kr, local lr < 9; shared column sc in 9 .. 14) or of its transpose, over the key frame's
// links in link order (full_inertial.inc: ONE bias pair for the map): as P1 / V1 of a link the key frame meets the shared bias in the
// link's own G1 / A1 columns, as P2 / V2 too
__device__ __forceinline__ double border_terms(const Dev& d, int kr, int lr, int sc, bool kf_is_row)
{
    double v = 0;
    for (int k = d.kl_off[kr]; k < d.kl_off[kr + 1]; k++) {
        const int l = d.kl_link[k];
        const int li = link_index24(d.links[l], kr, lr);
        if (li >= 0) v += d.lH[576 * (size_t)l + (kf_is_row ? li * 24 + sc : sc * 24 + li)];
    }
    return v;
}
// entry idx of S / the right-hand side row outside the pose blocks.  SHARED (full_inertial.inc): rows with row_kf = nKF are the shared
// bias; the shared block and its gradient rows belong to another workgroup
template <bool SHARED>
__device__ __forceinline__ void entry_body(const IWin& w, const IDyn& y, const size_t idx)
{
    const Dev& d = w.d;
    const int np = d.npad;
    const double lambda = y.lambda;
    double* __restrict__ S = w.S;
    const KFState* __restrict__ st = w.st[y.cur];
    if (idx >= (size_t)np * np + np) return;
    const int r = (int)(idx / np), c = (int)(idx - (size_t)r * np);
    if (r == np) {          // the right-hand side row
        const int kc = d.row_kf[c];
        if (kc < 0) { S[idx] = 0.0; return; }
        const int lc = d.row_loc[c];
        if (SHARED && kc == d.nKF) return;
        if (lc < 6) return;                                     // a pose row: its key-frame workgroup writes it
        const double v = link_terms(d, st, kc, lc, -1, 0);
        S[idx] = v; d.bp[c] = v;
        return;
    }
    const int kr = d.row_kf[r], kc = d.row_kf[c];
    if (kr < 0 || kc < 0) { S[idx] = (r == c) ? 1.0 : 0.0; return; }
    const int lr = d.row_loc[r], lc = d.row_loc[c];
    if (SHARED) {
        if (kr == d.nKF && kc == d.nKF) return;
        if (kr == d.nKF) { S[idx] = border_terms(d, kc, lc, lr, false); return; }
        if (kc == d.nKF) { S[idx] = border_terms(d, kr, lr, lc, true); return; }
    }
    if (kr == kc && lr < 6 && lc < 6) return;                   // a pose block: its key-frame workgroup writes it
    double v = link_terms(d, st, kr, lr, kc, lc);
    if (r == c) v += lambda;
    S[idx] = v;
}
__device__ __forceinline__ void system_body(const IWin& w, const IDyn& y, const int bx)
{
    const Dev& d = w.d;
    const int tid = threadIdx.x, np = d.npad;
    const double lambda = y.lambda;
    double* __restrict__ S = w.S;
    const KFState* __restrict__ st = w.st[y.cur];
    if (bx < w.lm_blocks) {
        const int sub = tid & 7, l = bx * kPtLandmarks + (tid >> 3);
        const bool live = l < d.nL;
        int k0 = 0, k1 = 0;
        if (live) { k0 = d.l_off[l]; k1 = d.l_off[l + 1]; }
        double acc[12];
        for (int q = 0; q < 12; q++) acc[q] = 0.0;
        for (int k = k0 + sub; k < k1; k += 8) {
            const double* eh = d.eH + 12 * (size_t)d.l_edge[k];
            for (int q = 0; q < 12; q++) acc[q] += eh[q];
        }
        for (int q = 0; q < 12; q++)
            for (int o = 4; o > 0; o >>= 1) acc[q] += __shfl_xor(acc[q], o);
        if (!live) return;
        double A[9], Di[9];
        for (int k = 0; k < 9; k++) A[k] = acc[k] + ((k % 4 == 0) ? lambda : 0.0);
        if (!minv3(A, Di)) { for (int k = 0; k < 9; k++) Di[k] = 0.0; if (sub == 0) st_agent(d.scal + 5, 1.0); }
        if (sub == 0) {
            for (int k = 0; k < 9; k++) d.Dinv[9 * (size_t)l + k] = Di[k];
            for (int k = 0; k < 3; k++) d.bl[3 * (size_t)l + k] = acc[9 + k];
        }
        for (int k = k0 + sub; k < k1; k += 8) {
            const int e = d.l_edge[k];
            const double* We = d.W + 18 * (size_t)e;
            double* Ze = d.Z + 18 * (size_t)e;
            for (int r = 0; r < 6; r++)
                for (int c = 0; c < 3; c++) Ze[3 * r + c] = We[3 * r] * Di[c] + We[3 * r + 1] * Di[3 + c] + We[3 * r + 2] * Di[6 + c];
        }
        return;
    }
    if (bx < w.lm_blocks + d.nKF) {
        const int i = bx - w.lm_blocks;
        const int op = d.off_pose[i];
        if (op < 0) return;
        __shared__ double s_acc[kSysThreads / 64][28];
        double acc[27];
        for (int k = 0; k < 27; k++) acc[k] = 0.0;
        for (int k = d.k_off[i] + tid; k < d.k_off[i + 1]; k += kSysThreads) {
            const double* ph = d.pH + 27 * (size_t)d.k_edge[k];
            for (int q = 0; q < 27; q++) acc[q] += ph[q];
        }
        for (int q = 0; q < 27; q++) {
            double v = acc[q];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((tid & 63) == 0) s_acc[tid >> 6][q] = v;
        }
        __syncthreads();
        if (tid < 42) {
            const int a = tid < 36 ? tid / 6 : tid - 36, c = tid < 36 ? tid - 6 * a : -1;
            int idx;
            if (c >= 0) { const int lo = a < c ? a : c, hi = a < c ? c : a; idx = lo * 6 - lo * (lo - 1) / 2 + (hi - lo); }
            else idx = 21 + a;
            double v = ((s_acc[0][idx] + s_acc[1][idx]) + s_acc[2][idx]) + s_acc[3][idx];
            v += link_terms(d, st, i, a, c >= 0 ? i : -1, c);
            if (c >= 0) S[(size_t)(op + a) * np + op + c] = (a == c) ? v + lambda : v;
            else { S[(size_t)np * np + op + a] = v; d.bp[op + a] = v; }
        }
        return;
    }
    entry_body<false>(w, y, (size_t)(bx - w.lm_blocks - d.nKF) * kSysThreads + tid);
}
__global__ __launch_bounds__(kSysThreads) void ki_system(const IWin* __restrict__ wins, IDynAll dyn)
{
    const IDyn y = dyn.w[blockIdx.y];
    if (!(y.flags & kIwTrial)) return;
    const IWin& w = wins[blockIdx.y];
    if ((int)blockIdx.x >= w.lm_blocks + w.d.nKF + w.entry_blocks) return;
    system_body(w, y, (int)blockIdx.x);
}

// the visual Schur terms of a key-frame pair (i <= j): S_ij -= sum over the pair list of Z_a W_b^T; the diagonal pairs also take
// b_schur = bp - sum_e Z_e bl of their key frame
constexpr int kSchurGroups = 256;           // 256 groups of 4 lanes walk the pair list of a block, a lane owns a 3 x 3 corner of the 6 x 6 block
                                            // (round 3, as LocalBA's k_schur_blocks: 18 loaded doubles for 27 FMAs; 28 groups x 36 entries
                                            // walked ~20 pairs each through chains of dependent loads: 41 us for the 55 blocks of 10 key frames)
__device__ __forceinline__ void schur_blocks_body(const Dev& d, double* __restrict__ S, const int blk)
{
    __shared__ double s_part[16][37];
    const int i = d.b_i[blk], j = d.b_j[blk];
    const int oi = d.off_pose[i], oj = d.off_pose[j];
    const int np = d.npad;
    const int tid = threadIdx.x;
    {
        const int g = tid >> 2, q = tid & 3, rb = q >> 1, cb = q & 1;
        double acc[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
        for (int k = d.b_off[blk] + g; k < d.b_off[blk + 1]; k += kSchurGroups) {
            const int2 pr = d.b_pair[k];
            const double* Z = d.Z + 18 * (size_t)pr.x + 9 * rb;
            const double* W = d.W + 18 * (size_t)pr.y + 9 * cb;
            double z[9], w[9];
#pragma unroll
            for (int u = 0; u < 9; u++) { z[u] = Z[u]; w[u] = W[u]; }
#pragma unroll
            for (int a = 0; a < 3; a++)
#pragma unroll
                for (int b = 0; b < 3; b++) acc[a][b] += z[3 * a] * w[3 * b] + z[3 * a + 1] * w[3 * b + 1] + z[3 * a + 2] * w[3 * b + 2];
        }
        // the 16 groups of a wave first (fixed butterfly over the lanes with the same corner), then the 16 waves
#pragma unroll
        for (int a = 0; a < 3; a++)
#pragma unroll
            for (int b = 0; b < 3; b++) {
                double v = acc[a][b];
                v += __shfl_xor(v, 4); v += __shfl_xor(v, 8); v += __shfl_xor(v, 16); v += __shfl_xor(v, 32);
                if ((tid & 63) < 4) s_part[tid >> 6][(3 * rb + a) * 6 + 3 * cb + b] = v;
            }
    }
    // b_schur of this key frame: bp - sum_e Z_e bl, 6 rows x 160 groups over the key frame's edges (a key frame has a few hundred
    // edges and every term is a chain of three dependent loads: with 7 groups this part alone took longer than all the products)
    constexpr int kBGroups = 160;
    __shared__ double s_b[6][kBGroups];
    __syncthreads();
    if (i == j && tid < 6 * kBGroups) {
        const int r = tid / kBGroups, gg = tid - r * kBGroups;
        double bsum = 0;
        for (int k = d.k_off[i] + gg; k < d.k_off[i + 1]; k += kBGroups) {
            const int e = d.k_edge[k];
            const double* Z = d.Z + 18 * (size_t)e + r * 3;
            const double* b = d.bl + 3 * (size_t)d.e_point[e];
            bsum += Z[0] * b[0] + Z[1] * b[1] + Z[2] * b[2];
        }
        s_b[r][gg] = bsum;
    }
    if (tid < 36) {
        const int r = tid / 6, c = tid - r * 6;
        double sum = s_part[0][tid];
        for (int q = 1; q < 16; q++) sum += s_part[q][tid];
        S[(size_t)(oi + r) * np + oj + c] -= sum;
        if (i != j) S[(size_t)(oj + c) * np + oi + r] -= sum;
    }
    __syncthreads();
    if (i == j && tid < 6) {
        double sum = 0;
        for (int q = 0; q < kBGroups; q++) sum += s_b[tid][q];
        S[(size_t)np * np + oi + tid] -= sum;
    }
}
__global__ __launch_bounds__(1024) void ki_schur_blocks(const IWin* __restrict__ wins, IDynAll dyn)
{
    const IDyn y = dyn.w[blockIdx.y];
    if (!(y.flags & kIwTrial)) return;
    const IWin& w = wins[blockIdx.y];
    if ((int)blockIdx.x >= w.d.nBlocks) return;
    schur_blocks_body(w.d, w.S, (int)blockIdx.x);
}

// the factorisation: LocalBA's one-launch dataflow kernel (a workgroup per lower-triangle tile); `w0` = first window of this launch
// (the host keeps tiles x windows of a launch within what is resident at once)
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(1, 2))) void ki_chol_flow(const IWin* __restrict__ wins, IDynAll dyn, int w0)
{
    extern __shared__ __align__(16) double sm_step[];
    const IDyn y = dyn.w[w0 + blockIdx.y];
    if (!(y.flags & kIwTrial)) return;
    const IWin& w = wins[w0 + blockIdx.y];
    if ((int)blockIdx.x >= w.nblk * (w.nblk + 1) / 2) return;
    chol::chol_flow_body(w.S, w.Lp, w.d.npad, w.nblk, w.Linv, w.d.scal, w.flow, (unsigned)y.seq, (int)blockIdx.x, sm_step);
}

// substitution (LocalBA's single-workgroup kernel) and, by the same workgroup, the trial state of every key frame (oplus into the
// other state buffer: ImuCamPose::Update, G2oTypes.cc:230-258) with its part of the scale sum
__global__ __launch_bounds__(1024) void ki_solve_update(const IWin* __restrict__ wins, IDynAll dyn)
{
    extern __shared__ double sm[];
    const IDyn y = dyn.w[blockIdx.y];
    if (!(y.flags & kIwTrial)) return;
    const IWin& w = wins[blockIdx.y];
    const Dev& d = w.d;
    const int np = d.npad;
    chol::chol_solve_body<true>(w.Lp, np, w.Linv, w.Lp + (size_t)np * np, w.S + (size_t)np * np, d.x, d.scal, 1, 0, sm);
    __syncthreads();                // x is complete (global memory, same workgroup)
    const double lambda = y.lambda;
    const KFState* __restrict__ st = w.st[y.cur];
    KFState* __restrict__ st_new = w.st[1 - y.cur];
    for (int i = threadIdx.x; i < d.nKF; i += 1024) {
        KFState k = st[i];
        double sc = 0;
        const int op = d.off_pose[i];
        if (op >= 0) {
            const double* pu = d.x + op;
            double t[3], dR[9];
            mvec(k.Rwb, pu + 3, t);
            for (int q = 0; q < 3; q++) k.twb[q] += t[q];
            exp_so3(pu, dR);
            mmul(k.Rwb, dR, k.Rwb);
            if (++k.its >= 3) { normalize_rotation(k.Rwb); k.its = 0; }
            camera_from_body(d, k);
            for (int q = 0; q < 6; q++) sc += pu[q] * (lambda * pu[q] + d.bp[op + q]);
        }
        if (d.off_v[i] >= 0) {
            for (int q = 0; q < 3; q++) {
                const double xv = d.x[d.off_v[i] + q], xg = d.x[d.off_g[i] + q], xa = d.x[d.off_a[i] + q];
                k.v[q] += xv; k.bg[q] += xg; k.ba[q] += xa;
                sc += xv * (lambda * xv + d.bp[d.off_v[i] + q]) + xg * (lambda * xg + d.bp[d.off_g[i] + q]) + xa * (lambda * xa + d.bp[d.off_a[i] + q]);
            }
        }
        st_new[i] = k;
        d.part[d.nL + i] = sc;
    }
}

__global__ void ki_init_states(const IWin* __restrict__ wins)
{
    const IWin& w = wins[blockIdx.y];
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < w.d.nKF) { KFState k = w.st[0][i]; k.its = 0; camera_from_body(w.d, k); w.st[0][i] = k; }
}

// results of every window into ONE device buffer (a single copy to the host follows): the accepted states and points, and per
// visual edge chi2 (from the errors of the final state) and the depth sign
__global__ __launch_bounds__(256) void ki_epilogue(const IWin* __restrict__ wins, IDynAll dyn)
{
    const IWin& w = wins[blockIdx.y];
    const Dev& d = w.d;
    const int cur = dyn.w[blockIdx.y].cur;
    const KFState* __restrict__ st = w.st[cur];
    const double* __restrict__ pts = w.pts[cur];
    const int g = blockIdx.x * 256 + threadIdx.x;
    constexpr int kStWords = (int)(sizeof(KFState) / 8);
    if (g < d.nKF * kStWords) ((unsigned long long*)w.o_st)[g] = ((const unsigned long long*)st)[g];
    if (g < 3 * d.nL) w.o_pts[g] = pts[g];
    if (g < d.nE) {
        const int e = g;
        const double* r = d.err + 3 * (size_t)e;
        w.o_chi2[e] = d.e_w[e] * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        const KFState& k = st[d.e_kf[e]];
        const double* X = pts + 3 * (size_t)d.e_point[e];
        w.o_depth[e] = (k.Rcw[6] * X[0] + k.Rcw[7] * X[1] + k.Rcw[8] * X[2] + k.tcw[2]) > 0.0;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// Optimizer::PoseInertialOptimizationLastKeyFrame (reference src/Optimizer.cc:4491-4873): the per-frame optimisation of the
// inertial tracker, a batch of frames per launch (one 256-thread workgroup per frame, the whole 4 x 10 Gauss-Newton schedule in
// one launch like k_pose_opt).  15 unknowns: the visual edges are reduced over the workgroup (21 + 6 sums), the inertial edge's
// 9 x 9 part is spread over 81 threads, thread 0 does the link error / Jacobian, the 15 x 15 Cholesky and the update.
// Replicated quirk: chi2 of an ACTIVE edge after a round is the error from the start of the last iteration (g2o's Gauss-Newton
// never recomputes it after the last update), outlier edges are recomputed at the current state (:4723-4726).
// ---------------------------------------------------------------------------------------------------------------------------
struct PIFrameDev {
    KFState kf, fr;                 // [0] last key frame (fixed) or previous frame (free, LF), [1] current frame (initial estimate)
    LibaLink link;
    int n, rec_init;
    size_t edge0;                   // first edge of this frame in the packed edge arrays
    double prior_Rwb[9], prior_twb[3], prior_vel[3], prior_bg[3], prior_ba[3], prior_H[225];       // LF only: pFp->mpcpi
};
struct PIDev {
    const PIFrameDev* frames;
    const double* Xw; const double* obs; const double* w; const uint8_t* stereo; const uint8_t* close_pt;
    double* err;                    // [edges][3] scratch
    uint8_t* outlier;               // [edges] out
    KFState* out_state; double* Hout; int* n_bad;     // per frame (Hout: N x N)
    double Rcb[9], tcb[3], Rbc[9], tbc[3];
    double fx, fy, cx, cy, bf, huber_mono, huber_stereo;
};

// EdgeInertial at the current states: error and the 9 x 24 Jacobian (columns P1 0-5, V1 6-8, G1 9-11, A1 12-14, P2 15-20, V2 21-23).
// Split over two lanes of different waves for the last-frame variant (both states free).  Part A is the dependent
// chain through the rotation error: bias-corrected delta rotation -> eR -> log -> inverse right Jacobian -> the three blocks of
// the rotation rows.  Part B is everything that only needs Rbw1 and the float velocity / position deltas.  The blocks that depend
// on the link alone (-I, -JVg, -JPg, -JVa, -JPa) are written once per call (pi_link_const).
__device__ inline void pi_link_const(const LibaLink& L, double* Jm)
{
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            Jm[(6 + i) * 24 + 3 + j] = (i == j) ? -1.0 : 0.0;
            Jm[(3 + i) * 24 + 9 + j] = -(double)L.JVg[3 * i + j]; Jm[(6 + i) * 24 + 9 + j] = -(double)L.JPg[3 * i + j];
            Jm[(3 + i) * 24 + 12 + j] = -(double)L.JVa[3 * i + j]; Jm[(6 + i) * 24 + 12 + j] = -(double)L.JPa[3 * i + j];
        }
}
__device__ inline void pi_link_part_a(const LibaLink& L, const KFState& k1, const KFState& k2, double* e9, double* Jm)
{
    auto set = [&](int r0, int c0, const double* B, double s) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Jm[(r0 + i) * 24 + c0 + j] = s * B[3 * i + j];
    };
    double dR[9], dV[3], dP[3], dbg[3], Rbw1[9], dRt[9], t[9], eR[9], er[3];
    link_delta(L, k1, dR, dV, dP, dbg);
    mtr(k1.Rwb, Rbw1); mtr(dR, dRt);
    mmul(dRt, Rbw1, t); mmul(t, k2.Rwb, eR);
    log_so3(eR, er);
    e9[0] = er[0]; e9[1] = er[1]; e9[2] = er[2];
    double invJr[9], Rbw2[9], A[9], B[9];
    inv_right_jac(er, invJr);
    mtr(k2.Rwb, Rbw2);
    mmul(Rbw2, k1.Rwb, A); mmul(invJr, A, B);
    set(0, 0, B, -1.0);
    double JRg[9], w[3], rj[9], eRt[9], C[9], D[9];
    for (int k = 0; k < 9; k++) JRg[k] = L.JRg[k];
    mvec(JRg, dbg, w); right_jac(w, rj); mtr(eR, eRt);
    mmul(invJr, eRt, C); mmul(C, rj, D); mmul(D, JRg, C);
    set(0, 9, C, -1.0);
    set(0, 15, invJr, 1.0);
}
__device__ inline void pi_link_part_b(const LibaLink& L, const KFState& k1, const KFState& k2, double* e9, double* Jm)
{
    auto set = [&](int r0, int c0, const double* B, double s) {
        for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Jm[(r0 + i) * 24 + c0 + j] = s * B[3 * i + j];
    };
    // GetDeltaVelocity / GetDeltaPosition (ImuTypes.cc:289-307): the float part of link_delta
    float dbg[3], dba[3];
    for (int i = 0; i < 3; i++) { dbg[i] = (float)k1.bg[i] - L.bias0[3 + i]; dba[i] = (float)k1.ba[i] - L.bias0[i]; }
    double dV[3], dP[3];
    for (int i = 0; i < 3; i++) {
        const float dv = L.dV[i] + (L.JVg[3 * i] * dbg[0] + L.JVg[3 * i + 1] * dbg[1] + L.JVg[3 * i + 2] * dbg[2]) +
                         (L.JVa[3 * i] * dba[0] + L.JVa[3 * i + 1] * dba[1] + L.JVa[3 * i + 2] * dba[2]);
        const float dp = L.dP[i] + (L.JPg[3 * i] * dbg[0] + L.JPg[3 * i + 1] * dbg[1] + L.JPg[3 * i + 2] * dbg[2]) +
                         (L.JPa[3 * i] * dba[0] + L.JPa[3 * i + 1] * dba[1] + L.JPa[3 * i + 2] * dba[2]);
        dV[i] = dv; dP[i] = dp;
    }
    const double dt = L.dT, g[3] = {0, 0, -9.81};
    double Rbw1[9], a[3], b[3], ra[3], rb[3], h[9], A[9];
    mtr(k1.Rwb, Rbw1);
    for (int i = 0; i < 3; i++) a[i] = k2.v[i] - k1.v[i] - g[i] * dt;
    mvec(Rbw1, a, ra);
    for (int i = 0; i < 3; i++) e9[3 + i] = ra[i] - dV[i];
    for (int i = 0; i < 3; i++) b[i] = k2.twb[i] - k1.twb[i] - k1.v[i] * dt - g[i] * dt * dt / 2;
    mvec(Rbw1, b, rb);
    for (int i = 0; i < 3; i++) e9[6 + i] = rb[i] - dP[i];
    skew3(ra, h); set(3, 0, h, 1.0);
    // (the Jacobian uses 0.5 * g * dt * dt where the error uses g * dt * dt / 2, as the reference does)
    for (int i = 0; i < 3; i++) b[i] = k2.twb[i] - k1.twb[i] - k1.v[i] * dt - 0.5 * g[i] * dt * dt;
    mvec(Rbw1, b, rb); skew3(rb, h); set(6, 0, h, 1.0);
    set(3, 6, Rbw1, -1.0); set(6, 6, Rbw1, -dt);
    mmul(Rbw1, k2.Rwb, A); set(6, 18, A, 1.0);
    set(3, 21, Rbw1, 1.0);
}
// EdgePriorPoseImu (G2oTypes.cc:720-760) on the previous frame's states: error (er, et, ev, ebg, eba) and its 15 x 15 Jacobian
__device__ inline void pi_prior(const PIFrameDev& fr, const KFState& K0, double* e15, double* J15)
{
    double Rt[9], Rr[9], iJ[9];
    mtr(fr.prior_Rwb, Rt);
    mmul(Rt, K0.Rwb, Rr);
    log_so3(Rr, e15);
    const double dt3[3] = {K0.twb[0] - fr.prior_twb[0], K0.twb[1] - fr.prior_twb[1], K0.twb[2] - fr.prior_twb[2]};
    mvec(Rt, dt3, e15 + 3);
    for (int q = 0; q < 3; q++) { e15[6 + q] = K0.v[q] - fr.prior_vel[q]; e15[9 + q] = K0.bg[q] - fr.prior_bg[q]; e15[12 + q] = K0.ba[q] - fr.prior_ba[q]; }
    for (int q = 0; q < 225; q++) J15[q] = 0.0;
    inv_right_jac(e15, iJ);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { J15[15 * r + c] = iJ[3 * r + c]; J15[15 * (3 + r) + 3 + c] = Rr[3 * r + c]; }
    for (int q = 6; q < 15; q++) J15[15 * q + q] = 1.0;
}

__device__ __forceinline__ void wave_fence_lds()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
// ---- the per-frame solve: N x N SPD system on the first N lanes of one wave.  Lane i holds row i of the matrix in registers
// (static indices: every loop is fully unrolled); the right-looking factorisation broadcasts the scaled pivot column with
// v_readlane (SGPR operands of the update FMAs: no LDS round trip on the dependent chain), the back substitution sums a
// column over the lanes with DPP row rotations.  Returns false (uniformly) when a pivot is not positive.
template <int CTRL>
__device__ __forceinline__ double dpp_mov_f64(double v)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}
// (NOT a duplicate of chol::row16_sum, a __shfl_xor butterfly: the two add in different orders and differ in the last bits.)
__device__ __forceinline__ double row16_allsum(double v)       // every lane gets the sum over its row of 16 lanes
{
    v += dpp_mov_f64<0x121>(v);         // row_ror:1
    v += dpp_mov_f64<0x122>(v);         // row_ror:2
    v += dpp_mov_f64<0x124>(v);         // row_ror:4
    v += dpp_mov_f64<0x128>(v);         // row_ror:8
    return v;
}
template <int J>
__device__ __forceinline__ double readlane_f64(double v)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), J), __builtin_amdgcn_readlane(__double2loint(v), J));
}
template <int N, int J, int C>
struct CholRowUpdate {
    static __device__ __forceinline__ void run(double (&A)[N], double lij)
    {
        if constexpr (C < N) {
            A[C] = fma(-lij, readlane_f64<C>(lij), A[C]);          // a_ic -= l_ij l_cj (meaningful for i >= c)
            CholRowUpdate<N, J, C + 1>::run(A, lij);
        }
    }
};
template <int N, int J>
struct CholRowStep {
    static __device__ __forceinline__ void factor(double (&A)[N], double (&invd)[N], bool& ok)
    {
        if constexpr (J < N) {
            const double dj = readlane_f64<J>(A[J]);
            if (!(dj > 0.0) || !isfinite(dj)) ok = false;
            const double inv = chol::rsqrt_newton(dj);
            invd[J] = inv;
            const double lij = A[J] * inv;
            A[J] = lij;
            CholRowUpdate<N, J, J + 1>::run(A, lij);
            CholRowStep<N, J + 1>::factor(A, invd, ok);
        }
    }
    static __device__ __forceinline__ void forward(const double (&A)[N], const double (&invd)[N], double& y, int i)
    {
        if constexpr (J < N) {
            const double yj = readlane_f64<J>(y) * invd[J];
            y = (i == J) ? yj : ((i > J) ? fma(-A[J], yj, y) : y);
            CholRowStep<N, J + 1>::forward(A, invd, y, i);
        }
    }
    // x_j = (y_j - sum_{k > j} L[k][j] x_k) / L[j][j], j = N - 1 - J.  Row form (N <= 16): lane k holds L[k][j], the sum over the
    // lanes is a DPP row reduction.  Column form: lane i holds COLUMN i of the factor (LT[c] = L[c][i]) and the step is a broadcast
    // of x_j like the forward substitution.
    static __device__ __forceinline__ void backward_rows(const double (&A)[N], const double (&invd)[N], double& x, int i)
    {
        if constexpr (J < N) {
            constexpr int j = N - 1 - J;
            double t = (i > j && i < N) ? A[j] * x : 0.0;
            t = row16_allsum(t);
            if (i == j) x = (x - t) * invd[j];
            CholRowStep<N, J + 1>::backward_rows(A, invd, x, i);
        }
    }
    static __device__ __forceinline__ void backward_cols(const double (&LT)[N], const double (&invd)[N], double& x, int i)
    {
        if constexpr (J < N) {
            constexpr int j = N - 1 - J;
            const double xj = readlane_f64<j>(x) * invd[j];
            x = (i == j) ? xj : ((i < j) ? fma(-LT[j], xj, x) : x);
            CholRowStep<N, J + 1>::backward_cols(LT, invd, x, i);
        }
    }
};
template <int N>
__device__ inline bool chol_solve_rows(double* __restrict__ H, const double* __restrict__ b, double* __restrict__ x_out, int lane)
{
    static_assert(N <= 32, "rows live on the first two DPP rows of the wave");
    const int i = lane < N ? lane : N - 1;
    double A[N], invd[N];
#pragma unroll
    for (int c = 0; c < N; c++) A[c] = H[N * i + c];
    bool ok = true;
    CholRowStep<N, 0>::factor(A, invd, ok);
    double y = b[i];
    CholRowStep<N, 0>::forward(A, invd, y, lane < N ? lane : 64);
    if constexpr (N <= 16) {
        CholRowStep<N, 0>::backward_rows(A, invd, y, lane < N ? lane : 64);
    } else {
        // transpose the factor through the (now free) LDS copy of H
        if (lane < N) {
#pragma unroll
            for (int c = 0; c < N; c++) H[N * i + c] = A[c];
        }
        wave_fence_lds();
#pragma unroll
        for (int c = 0; c < N; c++) A[c] = H[N * c + i];
        CholRowStep<N, 0>::backward_cols(A, invd, y, lane < N ? lane : -1);
    }
    if (lane < N) x_out[lane] = y;
    return ok;
}

// One visual edge of the per-frame problem, held in registers by its thread
struct PIEdge { double X[3], o[3], w; bool st, cl; };
__device__ __forceinline__ PIEdge pi_load_edge(const PIDev& d, size_t e)
{
    PIEdge E;
    for (int q = 0; q < 3; q++) { E.X[q] = d.Xw[3 * e + q]; E.o[q] = d.obs[3 * e + q]; }
    E.w = d.w[e]; E.st = d.stereo[e] != 0; E.cl = d.close_pt[e] != 0;
    return E;
}
__device__ __forceinline__ void pi_edge_error_v(const PIDev& d, const KFState& F, const PIEdge& E, double* r)
{
    double Xc[3];
    mvec(F.Rcw, E.X, Xc);
    for (int i = 0; i < 3; i++) Xc[i] += F.tcw[i];
    const double u = d.fx * Xc[0] / Xc[2] + d.cx, v = d.fy * Xc[1] / Xc[2] + d.cy;
    r[0] = E.o[0] - u; r[1] = E.o[1] - v; r[2] = 0;
    if (E.st) r[2] = E.o[2] - (u - d.bf * (1 / Xc[2]));
}
__device__ __forceinline__ void pi_edge_jac_v(const PIDev& d, const KFState& F, const PIEdge& E, double* Jj)
{
    double Xc[3], Xb[3];
    mvec(F.Rcw, E.X, Xc);
    for (int i = 0; i < 3; i++) Xc[i] += F.tcw[i];
    mvec(d.Rbc, Xc, Xb);
    for (int i = 0; i < 3; i++) Xb[i] += d.tbc[i];
    const double iz = 1.0 / Xc[2], iz2 = 1.0 / (Xc[2] * Xc[2]);
    double pj[9] = {d.fx * iz, 0, -d.fx * Xc[0] * iz2, 0, d.fy * iz, -d.fy * Xc[1] * iz2, 0, 0, 0};
    if (E.st) { pj[6] = pj[0]; pj[7] = pj[1]; pj[8] = pj[2] + d.bf * iz2; }
    double pr[9];
    mmul(pj, d.Rcb, pr);
    const double x = Xb[0], y = Xb[1], z = Xb[2];
    const double D[18] = {0, z, -y, 1, 0, 0, -z, 0, x, 0, 1, 0, y, -x, 0, 0, 0, 1};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 6; c++) Jj[6 * r + c] = pr[3 * r] * D[c] + pr[3 * r + 1] * D[6 + c] + pr[3 * r + 2] * D[12 + c];
}
// error (kept by the caller for the stale-chi2 rule) and the edge's share of the 21 + 6 sums; weighted = with b and Huber
__device__ __forceinline__ void pi_edge_sums(const PIDev& d, const KFState& F, const PIEdge& E, bool robust, bool with_b, double* r, double* acc)
{
    if (with_b) pi_edge_error_v(d, F, E, r);
    constexpr int ne = 3;       // a mono edge's third row is all zeros (and so is its third error): static indices, no branches
    double w = E.w;
    if (with_b) {
        const double c = E.w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]);
        const double delta = E.st ? d.huber_stereo : d.huber_mono;
        w = E.w * ((robust && c > delta * delta) ? delta / sqrt(c) : 1.0);
    }
    double Jj[18];
    pi_edge_jac_v(d, F, E, Jj);
    int idx = 0;
#pragma unroll
    for (int a = 0; a < 6; a++)
#pragma unroll
        for (int c2 = a; c2 < 6; c2++, idx++) {
            double s2 = 0;
#pragma unroll
            for (int q = 0; q < ne; q++) s2 += Jj[6 * q + a] * Jj[6 * q + c2];
            acc[idx] += w * s2;
        }
    if (with_b) {
#pragma unroll
        for (int a = 0; a < 6; a++) {
            double s2 = 0;
#pragma unroll
            for (int q = 0; q < ne; q++) s2 += Jj[6 * q + a] * r[q];
            acc[21 + a] -= w * s2;
        }
    }
}

// EdgeInertial to a FIXED first state (the last key frame): everything that depends on the first state only is computed once
// per call; per Gauss-Newton iteration remain the rotation error, its inverse right Jacobian and the three Jacobian blocks of
// the second state's pose and velocity (columns 15-23; the first state's columns are never read: goff() < 0).
struct PILinkFixed { double M1[9], Rbw1[9], dV[3], dP[3]; };
__device__ inline void pi_link_fixed_init(const LibaLink& L, const KFState& k1, PILinkFixed& C, double* Jm)
{
    double dR[9], dbg[3], dRt[9];
    link_delta(L, k1, dR, C.dV, C.dP, dbg);
    mtr(k1.Rwb, C.Rbw1); mtr(dR, dRt);
    mmul(dRt, C.Rbw1, C.M1);
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) Jm[(3 + i) * 24 + 21 + j] = C.Rbw1[3 * i + j];      // d eV / d V2
}
// (two lanes of different waves: part A the chain through the rotation error, part B the velocity / position rows)
__device__ inline void pi_link_fixed_a(const PILinkFixed& C, const KFState& k2, double* e9, double* Jm)
{
    double eR[9], invJr[9], er[3];
    mmul(C.M1, k2.Rwb, eR);
    log_so3(eR, er);
    e9[0] = er[0]; e9[1] = er[1]; e9[2] = er[2];
    inv_right_jac(er, invJr);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Jm[i * 24 + 15 + j] = invJr[3 * i + j];
}
__device__ inline void pi_link_fixed_b(const LibaLink& L, const PILinkFixed& C, const KFState& k1, const KFState& k2, double* e9, double* Jm)
{
    const double dt = L.dT, g[3] = {0, 0, -9.81};
    double a[3], b[3], A[9];
    for (int i = 0; i < 3; i++) a[i] = k2.v[i] - k1.v[i] - g[i] * dt;
    mvec(C.Rbw1, a, e9 + 3);
    for (int i = 0; i < 3; i++) e9[3 + i] -= C.dV[i];
    for (int i = 0; i < 3; i++) b[i] = k2.twb[i] - k1.twb[i] - k1.v[i] * dt - g[i] * dt * dt / 2;
    mvec(C.Rbw1, b, e9 + 6);
    for (int i = 0; i < 3; i++) e9[6 + i] -= C.dP[i];
    mmul(C.Rbw1, k2.Rwb, A);
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) Jm[(6 + i) * 24 + 18 + j] = A[3 * i + j];
}

#ifdef LIBA_PI_TIMING     // cycle split of one workgroup's Gauss-Newton iterations (tools/pi_timing.py); never defined in the product build
__device__ unsigned long long d_pi_prof[16];
#define PI_TICK(k) if (blockIdx.x == 0 && tid == 0) { const long long t_now = clock64(); d_pi_prof[k] += (unsigned long long)(t_now - t_prev); t_prev = t_now; }
#else
#define PI_TICK(k)
#endif
constexpr int kPiAccRow = 264;      // 256 partials + one pad per 32 (bank spread for the strided second stage)
constexpr int kPiRegEdges = 2;      // edges per thread held in registers (n <= 512 never re-reads global memory)

// LF = false: PoseInertialOptimizationLastKeyFrame (15 unknowns).  LF = true: PoseInertialOptimizationLastFrame (:4875-5285): the
// previous frame's 15 unknowns come first (0-14), the current frame's follow (15-29); it adds the prior edge (Huber 5) and returns the
// 30 x 30 Hessian the shim hands to Optimizer::Marginalize.
// Waves 0-3 own the visual edges (two per thread in registers: data, last error, outlier flag); lane 0 of wave 4 does the
// rotation-error chain of the inertial link and lane 0 of wave 5 its velocity / position rows (LF: and the prior edge), beside them.  An iteration is five barriers: sums / link ->
// second reduction stage, Omega J -> H and b assembled entry by entry -> solve (wave 0) -> update.
template <bool LF>
__global__ __launch_bounds__(384) void k_pose_inertial(PIDev d)
{
    constexpr int N = LF ? 30 : 15, OC = LF ? 15 : 0;
    __shared__ KFState sF, sK;
    __shared__ double s_acc[27][kPiAccRow], s_out[27];
    __shared__ double s_H[N * N], s_b[N], s_x[N], s_Jm[216], s_OJ[216], s_e9[9], s_Oe[9];
    __shared__ double s_e15[15], s_Oe15[15], s_J15[LF ? 225 : 1], s_OJ15[LF ? 225 : 1];
    __shared__ PILinkFixed s_lc;
    __shared__ int s_bad, s_inl, s_fail;
    const PIFrameDev& fr = d.frames[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, n = fr.n;
    const bool edge_thread = tid < 256;
    const int link_tid = 256, prior_tid = 320;
    const size_t e0 = fr.edge0;
    if (tid == 0) { sF = fr.fr; sK = fr.kf; sF.its = 0; sK.its = 0; camera_from_body_pi(d, sF); camera_from_body_pi(d, sK); s_fail = 0; }
    for (int i = tid; i < 216; i += blockDim.x) s_Jm[i] = 0.0;
    PIEdge ce[kPiRegEdges];
    double cerr[kPiRegEdges][3];
    bool cvalid[kPiRegEdges], cout_[kPiRegEdges];
#pragma unroll
    for (int j = 0; j < kPiRegEdges; j++) {
        const int i = tid + 256 * j;
        cvalid[j] = edge_thread && i < n;
        if (cvalid[j]) ce[j] = pi_load_edge(d, e0 + i);
        else { ce[j].X[0] = 0; ce[j].X[1] = 0; ce[j].X[2] = 1; ce[j].o[0] = 0; ce[j].o[1] = 0; ce[j].o[2] = 0; ce[j].w = 0; ce[j].st = false; ce[j].cl = false; }
        cout_[j] = false; cerr[j][0] = 0; cerr[j][1] = 0; cerr[j][2] = 0;
    }
    const int i_rest = tid + 256 * kPiRegEdges;         // first edge of this thread that lives in global memory
    if (edge_thread) for (int i = i_rest; i < n; i += 256) d.outlier[e0 + i] = 0;
    __syncthreads();
    if (!LF && tid == link_tid) pi_link_fixed_init(fr.link, sK, s_lc, s_Jm);
    if (LF && tid == link_tid) pi_link_const(fr.link, s_Jm);
    bool robust = true;
    const float chi2Mono[4] = {LF ? 5.991f : 12.f, LF ? 5.991f : 7.5f, 5.991f, 5.991f}, chi2Stereo[4] = {15.6f, 9.8f, 7.815f, 7.815f};
    // unknown -> column of the link's 9 x 24 Jacobian (P1 0-5, V1 6-8, G1 9-11, A1 12-14, P2 15-20, V2 21-23), -1: none
    auto lcol = [&](int g) __attribute__((always_inline)) -> int {
        if (LF) return g < 15 ? g : (g < 24 ? g : -1);
        return g < 9 ? 15 + g : -1;
    };
    // the 21 + 6 sums of the visual edges over the workgroup, into s_acc (first stage: one partial per thread)
    auto visual_sums = [&](bool with_b) __attribute__((always_inline)) {
        double acc[27];
        for (int q = 0; q < 27; q++) acc[q] = 0.0;
#pragma unroll
        for (int j = 0; j < kPiRegEdges; j++)
            if (cvalid[j] && !cout_[j]) pi_edge_sums(d, sF, ce[j], robust, with_b, cerr[j], acc);
        for (int i = i_rest; i < n; i += 256) {
            const size_t e = e0 + i;
            if (d.outlier[e]) continue;                 // level 1
            const PIEdge E = pi_load_edge(d, e);
            double r[3];
            pi_edge_sums(d, sF, E, robust, with_b, r, acc);
            if (with_b) { d.err[3 * e] = r[0]; d.err[3 * e + 1] = r[1]; d.err[3 * e + 2] = r[2]; }
        }
#pragma unroll
        for (int q = 0; q < 27; q++) s_acc[q][tid + (tid >> 5)] = acc[q];
    };
    // second stage (27 x 8 threads) and the products with the information matrices
    auto reduce_and_weigh = [&](bool with_b) __attribute__((always_inline)) {
        if (tid < 216) {
            const int r = tid / 24, c = tid - r * 24;
            double s2 = 0;
            for (int q = 0; q < 9; q++) s2 += fr.link.info9[9 * r + q] * s_Jm[24 * q + c];
            s_OJ[tid] = s2;
            const int k = tid >> 3, part = tid & 7;
            const double* src = &s_acc[k][part * 33];
            double v = 0;
#pragma unroll 8
            for (int i = 0; i < 32; i++) v += src[i];
            v += __shfl_xor(v, 1); v += __shfl_xor(v, 2); v += __shfl_xor(v, 4);
            if (part == 0) s_out[k] = v;
        } else if (tid < 225) {
            const int r = tid - 216;
            double s2 = 0;
            for (int q = 0; q < 9; q++) s2 += fr.link.info9[9 * r + q] * s_e9[q];
            s_Oe[r] = s2;
        }
        if (LF) {
            const int t2 = tid - 128;                   // waves 2-5: the prior's products
            if (t2 >= 0 && t2 < 225) {
                const int r = t2 / 15, c = t2 - r * 15;
                double s2 = 0;
                for (int q = 0; q < 15; q++) s2 += fr.prior_H[15 * r + q] * s_J15[15 * q + c];
                s_OJ15[t2] = s2;
            } else if (with_b && t2 >= 225 && t2 < 240) {
                const int r = t2 - 225;
                double s2 = 0;
                for (int q = 0; q < 15; q++) s2 += fr.prior_H[15 * r + q] * s_e15[q];
                s_Oe15[r] = s2;
            }
        }
    };
    // H (and b) entry by entry: visual block + J^T (Omega J) of the link + the random walks + the prior
    auto assemble = [&](bool with_b) __attribute__((always_inline)) {
        double rho1p = 1.0;
        if (LF && with_b) {                             // Huber weight of the prior edge (delta 5); every thread on its own
            double c = 0;
            for (int q = 0; q < 15; q++) c += s_e15[q] * s_Oe15[q];
            rho1p = c > 25.0 ? 5.0 / sqrt(c) : 1.0;
        }
        const double* Og = fr.link.info_gyro; const double* Oa = fr.link.info_acc;
        auto rw = [&](int r, int c, int off2, const double* Om) __attribute__((always_inline)) -> double {     // e = b_cur - b_prev, J_prev = -I, J_cur = +I
            const int o2 = OC + off2, o1 = LF ? off2 : -100;
            const bool r2 = r >= o2 && r < o2 + 3, c2 = c >= o2 && c < o2 + 3, r1 = r >= o1 && r < o1 + 3, c1 = c >= o1 && c < o1 + 3;
            if (r2 && c2) return Om[3 * (r - o2) + c - o2];
            if (r1 && c1) return Om[3 * (r - o1) + c - o1];
            if (r1 && c2) return -Om[3 * (r - o1) + c - o2];
            if (r2 && c1) return -Om[3 * (r - o2) + c - o1];
            return 0.0;
        };
        // the solve only reads the lower triangle: N (N + 1) / 2 entries per iteration; the returned Hessian is built in full
        const int n_ent = with_b ? N * (N + 1) / 2 : N * N;
        for (int idx = tid; idx < n_ent; idx += blockDim.x) {
            int r, c;
            if (with_b) {
                r = (int)((sqrtf(8.f * (float)idx + 1.f) - 1.f) * 0.5f);
                while (r * (r + 1) / 2 > idx) r--;
                while ((r + 1) * (r + 2) / 2 <= idx) r++;
                c = idx - r * (r + 1) / 2;
            } else { r = idx / N; c = idx - r * N; }
            double v = 0;
            if (r >= OC && r < OC + 6 && c >= OC && c < OC + 6) {
                const int a = (r < c ? r : c) - OC, b2 = (r < c ? c : r) - OC;
                v += s_out[a * 6 - (a * (a - 1)) / 2 + (b2 - a)];
            }
            const int lr = lcol(r), lc = lcol(c);
            if (lr >= 0 && lc >= 0) { double s2 = 0; for (int q = 0; q < 9; q++) s2 += s_Jm[24 * q + lr] * s_OJ[24 * q + lc]; v += s2; }
            v += rw(r, c, 9, Og); v += rw(r, c, 12, Oa);
            if (LF && r < 15 && c < 15) { double s2 = 0; for (int q = 0; q < 15; q++) s2 += s_J15[15 * q + r] * s_OJ15[15 * q + c]; v += rho1p * s2; }
            s_H[N * r + c] = v;
        }
        if (with_b && tid >= 256 && tid < 256 + N) {
            const int r = tid - 256;
            double v = 0;
            if (r >= OC && r < OC + 6) v += s_out[21 + r - OC];
            const int lr = lcol(r);
            if (lr >= 0) { double s2 = 0; for (int q = 0; q < 9; q++) s2 += s_Jm[24 * q + lr] * s_Oe[q]; v -= s2; }
            for (int which = 0; which < 2; which++) {
                const int o2 = OC + (which ? 12 : 9), o1 = LF ? (which ? 12 : 9) : -100;
                const double* Om = which ? Oa : Og;
                const bool in2 = r >= o2 && r < o2 + 3, in1 = r >= o1 && r < o1 + 3;
                if (in2 || in1) {
                    const int a = in2 ? r - o2 : r - o1;
                    double Od = 0;
                    for (int q = 0; q < 3; q++) Od += Om[3 * a + q] * (which ? sF.ba[q] - sK.ba[q] : sF.bg[q] - sK.bg[q]);
                    v += in2 ? -Od : Od;
                }
            }
            if (LF && r < 15) { double s2 = 0; for (int q = 0; q < 15; q++) s2 += s_J15[15 * q + r] * s_Oe15[q]; v -= rho1p * s2; }
            s_b[r] = v;
        }
    };
    auto link_and_prior = [&]() __attribute__((always_inline)) {
        if (tid == link_tid) {
            if (LF) pi_link_part_a(fr.link, sK, sF, s_e9, s_Jm);
            else pi_link_fixed_a(s_lc, sF, s_e9, s_Jm);
        }
        if (tid == prior_tid) {
            if (LF) { pi_link_part_b(fr.link, sK, sF, s_e9, s_Jm); pi_prior(fr, sK, s_e15, s_J15); }
            else pi_link_fixed_b(fr.link, s_lc, sK, sF, s_e9, s_Jm);
        }
    };
    int nBad = 0, nInl = 0;
#ifdef LIBA_PI_TIMING
    long long t_prev = clock64();
#endif
    __syncthreads();
    for (int it = 0; it < 4; it++) {
        for (int k = 0; k < 10; k++) {
            if (edge_thread) visual_sums(true); else link_and_prior();
            PI_TICK(0)
            __syncthreads();
            PI_TICK(1)
            reduce_and_weigh(true);
            __syncthreads();
            assemble(true);
            __syncthreads();
            PI_TICK(3)
            if (tid < 64) {                                 // Cholesky solve by N lanes (rows in registers)
                const bool ok = chol_solve_rows<N>(s_H, s_b, s_x, lane);
                if (lane == 0) s_fail = ok ? 0 : 1;
            }
            __syncthreads();
            PI_TICK(4)
            // update (ImuCamPose::Update, G2oTypes.cc:230-258): thread 0 the frame, thread 64 the previous one -- two branches with
            // the state named in each (a reference picked by ?: between two LDS objects would be addressed through flat loads)
            auto apply = [&](KFState& S, const double* x) __attribute__((always_inline)) {
                double t[3], dR[9];
                mvec(S.Rwb, x + 3, t);
                for (int q = 0; q < 3; q++) S.twb[q] += t[q];
                exp_so3(x, dR);
                mmul(S.Rwb, dR, S.Rwb);
                if (++S.its >= 3) { normalize_rotation(S.Rwb); S.its = 0; }
                camera_from_body_pi(d, S);
                for (int q = 0; q < 3; q++) { S.v[q] += x[6 + q]; S.bg[q] += x[9 + q]; S.ba[q] += x[12 + q]; }
            };
            if (!s_fail) {
                if (tid == 0) apply(sF, s_x + OC);
                else if (LF && tid == 64) apply(sK, s_x);
            }
            __syncthreads();
            PI_TICK(5)
            if (s_fail) break;                              // uniform
        }
        // ---- classification (:4716-4789, :5122-5195): active edges keep the error from the start of the last iteration
        if (tid == 0) { s_bad = 0; s_inl = 0; }
        __syncthreads();
        const float chi2close = 1.5 * chi2Mono[it];
        auto classify = [&](const PIEdge& E, const double* r) __attribute__((always_inline)) -> bool {
            const float chi2 = (float)(E.w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
            if (E.st) return chi2 > chi2Stereo[it];
            const double z = sF.Rcw[6] * E.X[0] + sF.Rcw[7] * E.X[1] + sF.Rcw[8] * E.X[2] + sF.tcw[2];
            return (chi2 > chi2Mono[it] && !E.cl) || (E.cl && chi2 > chi2close) || !(z > 0.0);
        };
        int my_bad = 0, my_inl = 0;
#pragma unroll
        for (int j = 0; j < kPiRegEdges; j++) {
            if (!cvalid[j]) continue;
            if (cout_[j]) pi_edge_error_v(d, sF, ce[j], cerr[j]);
            cout_[j] = classify(ce[j], cerr[j]);
            if (cout_[j]) my_bad++; else my_inl++;
        }
        if (edge_thread)
            for (int i = i_rest; i < n; i += 256) {
                const size_t e = e0 + i;
                const PIEdge E = pi_load_edge(d, e);
                double r[3];
                if (d.outlier[e]) { pi_edge_error_v(d, sF, E, r); d.err[3 * e] = r[0]; d.err[3 * e + 1] = r[1]; d.err[3 * e + 2] = r[2]; }
                else { r[0] = d.err[3 * e]; r[1] = d.err[3 * e + 1]; r[2] = d.err[3 * e + 2]; }
                const bool bad = classify(E, r);
                d.outlier[e] = bad;
                if (bad) my_bad++; else my_inl++;
            }
        if (my_bad) atomicAdd(&s_bad, my_bad);
        if (my_inl) atomicAdd(&s_inl, my_inl);
        __syncthreads();
        nBad = s_bad; nInl = s_inl;
        if (it == 2) robust = false;
        __syncthreads();
        PI_TICK(6)
        if (n + (LF ? 4 : 3) < 10) break;
    }
    if (nInl < 30 && !fr.rec_init) {                        // recover not too bad points (:4802-4828)
        if (tid == 0) s_bad = 0;
        __syncthreads();
        int my_bad = 0;
        auto recover = [&](const PIEdge& E) __attribute__((always_inline)) -> bool {
            double r[3];
            pi_edge_error_v(d, sF, E, r);
            const float chi2 = (float)(E.w * (r[0] * r[0] + r[1] * r[1] + r[2] * r[2]));
            return !(chi2 < (E.st ? 24.f : 18.f));
        };
#pragma unroll
        for (int j = 0; j < kPiRegEdges; j++) {
            if (!cvalid[j]) continue;
            if (recover(ce[j])) my_bad++; else cout_[j] = false;        // an edge above the bound keeps its flag
        }
        if (edge_thread)
            for (int i = i_rest; i < n; i += 256) {
                const size_t e = e0 + i;
                if (recover(pi_load_edge(d, e))) my_bad++; else d.outlier[e] = 0;
            }
        if (my_bad) atomicAdd(&s_bad, my_bad);
        __syncthreads();
        nBad = s_bad;
    }
    // ---- Hessian of the new prior (:4837-4870, :5231-5280): no robust weights
    if (edge_thread) visual_sums(false); else link_and_prior();
    __syncthreads();
    reduce_and_weigh(false);
    __syncthreads();
    assemble(false);
    __syncthreads();
    for (int q = tid; q < N * N; q += blockDim.x) d.Hout[(size_t)N * N * blockIdx.x + q] = s_H[q];
#pragma unroll
    for (int j = 0; j < kPiRegEdges; j++)
        if (cvalid[j]) d.outlier[e0 + tid + 256 * j] = cout_[j] ? 1 : 0;
    PI_TICK(7)
    if (tid == 0) { d.out_state[blockIdx.x] = sF; d.n_bad[blockIdx.x] = nBad; }
}

}  // namespace liba

struct liba_solver {                // also a window slot of a liba_batch, with the batch's stream and a view of its scalars
    int device = 0;
    hipStream_t stream = nullptr;
    liba::IWin* d_wins = nullptr;   // the window table of liba_solve (one entry)
    stage::PinnedOut io;            // result buffer of the handle: device + pinned host
    std::vector<void*> allocs;
    // bump arena reused across calls (a window needs ~45 device buffers; without it the hipMalloc / hipFree pairs cost more
    // than the optimisation); buffers that do not fit fall back to hipMalloc and the arena grows for the next call
    uint8_t* arena = nullptr;
    size_t arena_cap = 0, arena_off = 0, wanted = 0;
    stage::HostScalars hs;          // scalars + sequence number at [8]
    uint8_t* h_mirror = nullptr;    // pinned mirror of the arena (stage / flush)
    size_t h_mirror_cap = 0;
    std::vector<std::pair<size_t, size_t> > pending;     // (arena offset, bytes) waiting for flush()
    uint8_t* h_stage = nullptr;     // pinned staging buffer of the per-frame optimisation (grown on demand)
    size_t h_stage_cap = 0;
    template <typename T>
    int dalloc(T** p, size_t count)
    {
        *p = nullptr;
        const size_t bytes = (std::max(count, (size_t)1) * sizeof(T) + 255) & ~(size_t)255;
        wanted += bytes;
        if (arena && arena_off + bytes <= arena_cap) { *p = (T*)(arena + arena_off); arena_off += bytes; return ORBX_OK; }
        ORBX_HIP(hipMalloc((void**)p, bytes));
        allocs.push_back(*p);
        return ORBX_OK;
    }
    template <typename T>
    int upload(const T** p, const T* src, size_t count)
    {
        T* q;
        int r = dalloc(&q, count);
        if (r) return r;
        *p = q;
        return stage(q, src, count * sizeof(T));
    }
    // Host-to-device data goes through a pinned mirror of the arena: a window's two dozen small arrays become one or two copies
    // (adjacent allocations merge) issued by flush() before the first kernel, instead of a pageable-memory copy each.
    // (lba_shard::put / flush_stage is NOT the same thing: a shard allocates everything it uploads first and sends the arena's
    // prefix in ONE copy; here uploads and scratch interleave, so segments are merged.  One for both would change the copies.)
    int stage(void* dev, const void* src, size_t bytes)
    {
        if (!bytes) return ORBX_OK;
        uint8_t* dp = (uint8_t*)dev;
        if (arena && h_mirror && h_mirror_cap >= arena_cap && dp >= arena && dp + bytes <= arena + arena_cap) {
            const size_t off = (size_t)(dp - arena);
            std::memcpy(h_mirror + off, src, bytes);
            if (!pending.empty() && pending.back().first + ((pending.back().second + 255) & ~(size_t)255) == off) pending.back().second = off + bytes - pending.back().first;
            else pending.push_back(std::make_pair(off, bytes));
            return ORBX_OK;
        }
        ORBX_HIP(hipMemcpyAsync(dev, src, bytes, hipMemcpyHostToDevice, stream));
        return ORBX_OK;
    }
    int flush()
    {
        for (const auto& sg : pending) ORBX_HIP(hipMemcpyAsync(arena + sg.first, h_mirror + sg.first, sg.second, hipMemcpyHostToDevice, stream));
        pending.clear();
        return ORBX_OK;
    }
    void release()
    {
        for (void* p : allocs) (void)hipFree(p);
        allocs.clear();
        pending.clear();
        if (wanted > arena_cap) {
            if (arena) (void)hipFree(arena);
            arena = nullptr; arena_cap = 0;
            const size_t cap = wanted + wanted / 4 + (1 << 20);
            if (hipMalloc((void**)&arena, cap) == hipSuccess) arena_cap = cap;
            if (h_mirror) (void)hipHostFree(h_mirror);
            h_mirror = nullptr; h_mirror_cap = 0;
            if (arena_cap && hipHostMalloc((void**)&h_mirror, arena_cap, hipHostMallocDefault) == hipSuccess) h_mirror_cap = arena_cap;
        }
        arena_off = 0; wanted = 0;
    }
    ~liba_solver()
    {
        release();
        if (arena) (void)hipFree(arena);
        if (h_stage) (void)hipHostFree(h_stage);
        if (h_mirror) (void)hipHostFree(h_mirror);
        if (d_wins) (void)hipFree(d_wins);
        hs.release();
        io.release();
    }
};

static int liba_kernel_attributes()
{
    int r = chol::allow_lds(liba::ki_chol_flow, chol::kStepLds);
    return r ? r : chol::allow_lds(liba::ki_solve_update, chol::kFusedSolveLds);
}

extern "C" {

int liba_create(int device, liba_solver** out)
{
    if (!out) return fail(ORBX_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (int r = stage::check_device(device)) return r;
    ORBX_HIP(hipSetDevice(device));
    liba_solver* s = new liba_solver();
    s->device = device;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess) { delete s; return fail(ORBX_ERR_HIP, "stream creation failed"); }
    if (s->hs.alloc() != ORBX_OK || hipMalloc((void**)&s->d_wins, sizeof(liba::IWin)) != hipSuccess || liba_kernel_attributes() != ORBX_OK) {
        liba_destroy(s);
        return fail(ORBX_ERR_HIP, "solver buffer creation failed");
    }
    *out = s;
    return ORBX_OK;
}

void liba_destroy(liba_solver* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
    delete s;
}

static int liba_validate(const LibaProblem* p, int max_links = 64)
{
    if (!p) return fail(ORBX_ERR_ARG, "NULL problem");
    if (p->n_kf < 1 || p->n_points < 0 || p->n_edges < 0 || p->n_links < 0 || p->n_links > max_links) return fail(ORBX_ERR_ARG, "bad sizes");
    if (!p->Rwb || !p->twb || !p->vel || !p->bg || !p->ba || !p->pose_fixed || !p->has_imu || !p->imu_fixed) return fail(ORBX_ERR_ARG, "NULL key-frame arrays");
    if (p->n_points > 0 && !p->points) return fail(ORBX_ERR_ARG, "NULL points");
    if (p->n_edges > 0 && (!p->edge_kf || !p->edge_point || !p->edge_obs || !p->edge_inv_sigma2 || !p->edge_stereo)) return fail(ORBX_ERR_ARG, "NULL edge arrays");
    if (p->n_links > 0 && !p->links) return fail(ORBX_ERR_ARG, "NULL links");
    for (int e = 0; e < p->n_edges; e++)
        if (p->edge_kf[e] < 0 || p->edge_kf[e] >= p->n_kf || p->edge_point[e] < 0 || p->edge_point[e] >= p->n_points) return fail(ORBX_ERR_ARG, "edge %d out of range", e);
    for (int l = 0; l < p->n_links; l++) {
        const LibaLink& L = p->links[l];
        if (L.kf1 < 0 || L.kf1 >= p->n_kf || L.kf2 < 0 || L.kf2 >= p->n_kf || L.kf1 == L.kf2) return fail(ORBX_ERR_ARG, "link %d out of range", l);
        if (!p->has_imu[L.kf1] || !p->has_imu[L.kf2]) return fail(ORBX_ERR_ARG, "link %d joins a key frame without IMU states", l);
    }
    if (p->max_iters < 0 || !(p->lambda_init > 0)) return fail(ORBX_ERR_ARG, "bad LM parameters");
    return ORBX_OK;
}

// ---- one window on one slot: structure (CSR lists, pair lists, link lists, row tables), arena allocation, staged upload ----
struct LibaWindow {
    liba::IWin w;
    void* zero_block = nullptr;
    size_t zero_bytes = 0;
};
// What full_inertial.inc asks of the setup beyond a local window: systems of more than kFusedMaxBlocks tiles (no panel copy Lp
// then: the launch-per-block-column factorisation works in place) and, with shared_bias, ONE gyro and ONE accelerometer bias for
// all key frames: their 6 rows come last, row_kf = n_kf, and off_g / off_a of every key frame with IMU states point there.
struct LibaLayout { bool large = false, shared_bias = false; int max_unknowns = 0; };
static int liba_window_setup(liba_solver* sv, const LibaProblem* p, LibaWindow* out, const LibaLayout& lay = LibaLayout())
{
    int r = ORBX_OK;
    liba::Dev d;
    std::memset(&d, 0, sizeof(d));
    const int nKF = p->n_kf, nL = p->n_points, nE = p->n_edges;
    d.nKF = nKF; d.nL = nL; d.nE = nE; d.nLinks = p->n_links;
    std::vector<int> off_pose(nKF, -1), off_v(nKF, -1), off_g(nKF, -1), off_a(nKF, -1);
    int np = 0;
    for (int i = 0; i < nKF; i++) {
        if (!p->pose_fixed[i]) { off_pose[i] = np; np += 6; }
        if (p->has_imu[i] && !p->imu_fixed[i]) {
            if (lay.shared_bias) { off_v[i] = np; np += 3; }
            else { off_v[i] = np; off_g[i] = np + 3; off_a[i] = np + 6; np += 9; }
        }
    }
    const int off_shared = np;
    if (lay.shared_bias) {
        np += 6;
        for (int i = 0; i < nKF; i++) if (p->has_imu[i]) { off_g[i] = off_shared; off_a[i] = off_shared + 3; }
    }
    if (np == 0) return fail(ORBX_ERR_ARG, "nothing to optimise");
    const int npad = (np + 1) & ~1;             // the factorisation kernels use 16-byte loads: an even leading dimension
    d.np = np; d.npad = npad;
    const int nblk = (npad + chol::NB - 1) / chol::NB;
    if (lay.large ? np > lay.max_unknowns : nblk > chol::kFusedMaxBlocks) return fail(ORBX_ERR_CAPACITY, "%d reduced unknowns exceed the inertial solver's limit", np);
    // row -> (key frame, local index: pose 0-5, velocity 6-8, gyro bias 9-11, accelerometer bias 12-14); padding rows: -1
    std::vector<int> row_kf(npad, -1), row_loc(npad, 0);
    for (int i = 0; i < nKF; i++) {
        if (off_pose[i] >= 0) for (int q = 0; q < 6; q++) { row_kf[off_pose[i] + q] = i; row_loc[off_pose[i] + q] = q; }
        if (off_v[i] >= 0) for (int q = 0; q < (lay.shared_bias ? 3 : 9); q++) { row_kf[off_v[i] + q] = i; row_loc[off_v[i] + q] = 6 + q; }
    }
    if (lay.shared_bias) for (int q = 0; q < 6; q++) { row_kf[off_shared + q] = nKF; row_loc[off_shared + q] = 9 + q; }
    // the links of a key frame, in link order
    std::vector<int> kl_off(nKF + 1, 0), kl_link(std::max(2 * p->n_links, 1));
    for (int l = 0; l < p->n_links; l++) { kl_off[p->links[l].kf1 + 1]++; kl_off[p->links[l].kf2 + 1]++; }
    for (int i = 0; i < nKF; i++) kl_off[i + 1] += kl_off[i];
    {
        std::vector<int> c(kl_off.begin(), kl_off.end() - 1);
        for (int l = 0; l < p->n_links; l++) { kl_link[c[p->links[l].kf1]++] = l; kl_link[c[p->links[l].kf2]++] = l; }
    }
    // CSR by landmark / by key frame (free poses), pair lists per key-frame pair
    std::vector<int> l_off(nL + 1, 0), k_off(nKF + 1, 0);
    for (int e = 0; e < nE; e++) { l_off[p->edge_point[e] + 1]++; if (off_pose[p->edge_kf[e]] >= 0) k_off[p->edge_kf[e] + 1]++; }
    for (int l = 0; l < nL; l++) l_off[l + 1] += l_off[l];
    for (int i = 0; i < nKF; i++) k_off[i + 1] += k_off[i];
    std::vector<int> l_edge(std::max(nE, 1)), k_edge(std::max(k_off[nKF], 1)), lc(l_off.begin(), l_off.end() - 1), kc(k_off.begin(), k_off.end() - 1);
    for (int e = 0; e < nE; e++) { l_edge[lc[p->edge_point[e]]++] = e; if (off_pose[p->edge_kf[e]] >= 0) k_edge[kc[p->edge_kf[e]]++] = e; }
    std::vector<int> cnt((size_t)nKF * nKF, 0);
    for (int l = 0; l < nL; l++)
        for (int a = l_off[l]; a < l_off[l + 1]; a++) {
            const int i = p->edge_kf[l_edge[a]];
            if (off_pose[i] < 0) continue;
            for (int b = l_off[l]; b < l_off[l + 1]; b++) {
                const int j = p->edge_kf[l_edge[b]];
                if (off_pose[j] >= 0 && j >= i) cnt[(size_t)i * nKF + j]++;
            }
        }
    std::vector<int> b_i, b_j, b_off(1, 0), blk_of((size_t)nKF * nKF, -1);
    for (int i = 0; i < nKF; i++)
        for (int j = i; j < nKF; j++)
            if (off_pose[i] >= 0 && off_pose[j] >= 0 && (i == j || cnt[(size_t)i * nKF + j] > 0)) {
                blk_of[(size_t)i * nKF + j] = (int)b_i.size();
                b_i.push_back(i); b_j.push_back(j);
                b_off.push_back(b_off.back() + cnt[(size_t)i * nKF + j]);
            }
    d.nBlocks = (int)b_i.size();
    std::vector<int2> pairs(std::max(b_off.back(), 1));
    std::vector<int> bc(b_off.begin(), b_off.end() - 1);
    for (int l = 0; l < nL; l++)
        for (int a = l_off[l]; a < l_off[l + 1]; a++) {
            const int ea = l_edge[a], i = p->edge_kf[ea];
            if (off_pose[i] < 0) continue;
            for (int b = l_off[l]; b < l_off[l + 1]; b++) {
                const int eb = l_edge[b], j = p->edge_kf[eb];
                if (off_pose[j] < 0 || j < i) continue;
                int2 pr; pr.x = ea; pr.y = eb;
                pairs[bc[blk_of[(size_t)i * nKF + j]]++] = pr;
            }
        }
    std::vector<liba::KFState> st0(nKF);
    for (int i = 0; i < nKF; i++) {
        std::memset(&st0[i], 0, sizeof(liba::KFState));
        std::memcpy(st0[i].Rwb, p->Rwb + 9 * i, 72); std::memcpy(st0[i].twb, p->twb + 3 * i, 24); std::memcpy(st0[i].v, p->vel + 3 * i, 24);
        std::memcpy(st0[i].bg, p->bg + 3 * i, 24); std::memcpy(st0[i].ba, p->ba + 3 * i, 24);
    }
#define LIBA_TRY(x) do { r = (x); if (r) return r; } while (0)
    LIBA_TRY(sv->upload(&d.off_pose, off_pose.data(), (size_t)nKF)); LIBA_TRY(sv->upload(&d.off_v, off_v.data(), (size_t)nKF));
    LIBA_TRY(sv->upload(&d.off_g, off_g.data(), (size_t)nKF)); LIBA_TRY(sv->upload(&d.off_a, off_a.data(), (size_t)nKF));
    LIBA_TRY(sv->upload(&d.row_kf, row_kf.data(), row_kf.size())); LIBA_TRY(sv->upload(&d.row_loc, row_loc.data(), row_loc.size()));
    LIBA_TRY(sv->upload(&d.kl_off, kl_off.data(), kl_off.size())); LIBA_TRY(sv->upload(&d.kl_link, kl_link.data(), kl_link.size()));
    LIBA_TRY(sv->upload(&d.e_kf, p->edge_kf, (size_t)nE)); LIBA_TRY(sv->upload(&d.e_point, p->edge_point, (size_t)nE));
    LIBA_TRY(sv->upload(&d.e_obs, p->edge_obs, 3 * (size_t)nE)); LIBA_TRY(sv->upload(&d.e_w, p->edge_inv_sigma2, (size_t)nE));
    LIBA_TRY(sv->upload(&d.e_stereo, p->edge_stereo, (size_t)nE));
    LIBA_TRY(sv->upload(&d.l_off, l_off.data(), l_off.size())); LIBA_TRY(sv->upload(&d.l_edge, l_edge.data(), l_edge.size()));
    LIBA_TRY(sv->upload(&d.k_off, k_off.data(), k_off.size())); LIBA_TRY(sv->upload(&d.k_edge, k_edge.data(), k_edge.size()));
    LIBA_TRY(sv->upload(&d.b_i, b_i.data(), b_i.size())); LIBA_TRY(sv->upload(&d.b_j, b_j.data(), b_j.size()));
    LIBA_TRY(sv->upload(&d.b_off, b_off.data(), b_off.size())); LIBA_TRY(sv->upload(&d.b_pair, pairs.data(), pairs.size()));
    LIBA_TRY(sv->upload(&d.links, p->links, (size_t)p->n_links));
    liba::IWin& w = out->w;
    std::memset(&w, 0, sizeof(w));
    for (int k = 0; k < 2; k++) { LIBA_TRY(sv->dalloc(&w.st[k], (size_t)nKF)); LIBA_TRY(sv->dalloc(&w.pts[k], 3 * (size_t)nL)); }
    LIBA_TRY(sv->stage(w.st[0], st0.data(), (size_t)nKF * sizeof(liba::KFState)));
    if (nL > 0) LIBA_TRY(sv->stage(w.pts[0], p->points, 3 * (size_t)nL * sizeof(double)));
    LIBA_TRY(sv->dalloc(&d.bp, (size_t)npad)); LIBA_TRY(sv->dalloc(&d.bl, 3 * (size_t)nL));
    LIBA_TRY(sv->dalloc(&d.W, 18 * (size_t)nE)); LIBA_TRY(sv->dalloc(&d.Z, 18 * (size_t)nE)); LIBA_TRY(sv->dalloc(&d.Dinv, 9 * (size_t)nL));
    LIBA_TRY(sv->dalloc(&d.err, 3 * (size_t)nE)); LIBA_TRY(sv->dalloc(&d.rho1, (size_t)nE));
    LIBA_TRY(sv->dalloc(&d.eH, 12 * (size_t)nE)); LIBA_TRY(sv->dalloc(&d.pH, 27 * (size_t)nE));
    LIBA_TRY(sv->dalloc(&d.lrho, (size_t)p->n_links)); LIBA_TRY(sv->dalloc(&d.lH, 576 * (size_t)p->n_links)); LIBA_TRY(sv->dalloc(&d.lb, 24 * (size_t)p->n_links));
    LIBA_TRY(sv->dalloc(&d.x, (size_t)npad)); LIBA_TRY(sv->dalloc(&d.part, (size_t)nL + nKF)); LIBA_TRY(sv->dalloc(&d.chi_part, (size_t)nL));
    {   // zeroed per call in one memset: the device scalars (failure flag in [5]), the ticket of ki_points_errors, the tile flags of the factorisation
        uint8_t* zb;
        const size_t zbytes = 16 * sizeof(double) + 64 + chol::kFlowFlags * sizeof(unsigned);
        LIBA_TRY(sv->dalloc(&zb, zbytes));
        d.scal = (double*)zb; d.ticket = (unsigned*)(zb + 16 * sizeof(double)); w.flow = (unsigned*)(zb + 16 * sizeof(double) + 64);
        out->zero_block = zb; out->zero_bytes = zbytes;
    }
    LIBA_TRY(sv->dalloc(&w.S, ((size_t)npad + 1) * npad)); LIBA_TRY(sv->dalloc(&w.Linv, (size_t)nblk * chol::NB * chol::NB));
    if (nblk <= chol::kFusedMaxBlocks) LIBA_TRY(sv->dalloc(&w.Lp, ((size_t)npad + 1) * npad));
#undef LIBA_TRY
    for (int k = 0; k < 9; k++) { d.Rcb[k] = p->Rcb[k]; d.Rbc[k] = p->Rcb[3 * (k % 3) + k / 3]; }
    for (int k = 0; k < 3; k++) { d.tcb[k] = p->tcb[k]; d.tbc[k] = p->tbc[k]; }
    d.fx = p->fx; d.fy = p->fy; d.cx = p->cx; d.cy = p->cy; d.bf = p->bf;
    d.huber_mono = p->huber_mono; d.huber_stereo = p->huber_stereo; d.huber_inertial = p->huber_inertial;
    w.d = d;
    w.hmap = sv->hs.d;
    w.nblk = nblk;
    w.edge_blocks = (nE + liba::kLinThreads - 1) / liba::kLinThreads;
    w.lm_blocks = (nL + liba::kPtLandmarks - 1) / liba::kPtLandmarks;
    w.entry_blocks = (int)(((size_t)npad * npad + npad + liba::kSysThreads - 1) / liba::kSysThreads);
    return sv->flush();
}

// The Levenberg loops of W windows side by side: SparseOptimizer::optimize driving OptimizationAlgorithmLevenberg::solve
// (levenberg.cpp:61-169) with the user lambda, one Levenberg controller (lm_control.h) per window, cut where the host waits for the device; a round =
// [errors of the accepted state where they are stale] [linearisation where an iteration starts] [one trial], every stage ONE launch
// for all windows.
static int liba_run(int device, hipStream_t stream, liba_solver* const* slots, liba::IWin* d_wins, stage::PinnedOut* io, const LibaProblem* problems,
                    const LibaOutputs* outputs, int W, LbaStats* stats_out, float* device_ms, hipEvent_t ev0, hipEvent_t ev1)
{
    static const bool timing = std::getenv("ORBX_LBA_TIMING") != nullptr;
    const auto t_start = stage::Clock::now();
    int r = ORBX_OK;
    for (int i = 0; i < W; i++) if ((r = liba_validate(&problems[i]))) return r;
    ORBX_HIP(hipSetDevice(device));
    for (int i = 0; i < W; i++) slots[i]->release();
    auto cleanup = [&]() { for (int i = 0; i < W; i++) slots[i]->release(); };
    std::vector<LibaWindow> win((size_t)W);
    if (W == 1) r = liba_window_setup(slots[0], &problems[0], &win[0]);        // (liba_solve: the window's own message stands)
    else r = stage::for_each_window(W, device, [&](int i) { return liba_window_setup(slots[i], &problems[i], &win[i]); });
    if (r) { (void)hipStreamSynchronize(stream); cleanup(); return r; }
    std::vector<liba::IWin> hw((size_t)W);
    int max_lin = 1, max_pt = 1, max_sys = 1, max_sb = 1, max_nblk = 1, max_kf = 1, max_epi = 1;
    io->clear();
    for (int i = 0; i < W; i++) io->add((size_t)win[i].w.d.nKF * sizeof(liba::KFState), win[i].w.d.nL, win[i].w.d.nE);
    r = io->reserve(true);
    for (int i = 0; i < W && !r; i++) {
        hw[i] = win[i].w;
        liba::IWin& w = hw[i];
        {
            const stage::PinnedOut::Slice o = io->slice(io->d + io->off[i], (size_t)w.d.nKF * sizeof(liba::KFState), w.d.nL, w.d.nE);
            w.o_st = (liba::KFState*)o.state; w.o_pts = (double*)o.points; w.o_chi2 = (double*)o.chi2; w.o_depth = o.depth;
        }
        max_lin = std::max(max_lin, w.d.nLinks + w.edge_blocks); max_pt = std::max(max_pt, w.lm_blocks + 1);
        max_sys = std::max(max_sys, w.lm_blocks + w.d.nKF + w.entry_blocks); max_sb = std::max(max_sb, w.d.nBlocks);
        max_nblk = std::max(max_nblk, w.nblk); max_kf = std::max(max_kf, w.d.nKF);
        max_epi = std::max(max_epi, (std::max({w.d.nE, 3 * w.d.nL, w.d.nKF * (int)(sizeof(liba::KFState) / 8)}) + 255) / 256);
        if (hipMemsetAsync(win[i].zero_block, 0, win[i].zero_bytes, stream) != hipSuccess) r = fail(ORBX_ERR_HIP, "memset failed");
    }
    if (!r && hipMemcpyAsync(d_wins, hw.data(), (size_t)W * sizeof(liba::IWin), hipMemcpyHostToDevice, stream) != hipSuccess) r = fail(ORBX_ERR_HIP, "window table upload failed");
    if (r) { cleanup(); return r; }
    hipLaunchKernelGGL(liba::ki_init_states, dim3((max_kf + 63) / 64, W), dim3(64), 0, stream, (const liba::IWin*)d_wins);
    if (ev0) (void)hipEventRecord(ev0, stream);
    const auto t_setup = stage::Clock::now();

    std::vector<lm::Levenberg> ctl;                 // one Levenberg controller per window (lm_control.h), started at the user lambda
    for (int i = 0; i < W; i++) ctl.emplace_back(problems[i].max_iters, problems[i].lambda_init);
    std::vector<int> cur((size_t)W, 0);             // index of the accepted state; 1 - cur holds the trial state
    std::vector<char> err_current((size_t)W, 0);    // the device's edge errors belong to the accepted state
    liba::IDynAll dyn;
    std::memset(&dyn, 0, sizeof(dyn));
    const int tiles = max_nblk * (max_nblk + 1) / 2;
    const int flow_windows = std::max(1, chol::kMaxFlowGroups / tiles);
    for (bool final_round = false;;) {
        bool any_lin = false, any_err = false, any_trial = false;
        for (int i = 0; i < W; i++) {
            lm::Levenberg& c = ctl[i];
            liba::IDyn& y = dyn.w[i];
            y.flags = 0;
            if (final_round) {
                if (!err_current[i]) { y.flags = liba::kIwErrors; err_current[i] = 1; }       // the epilogue reads the errors of the final state
            } else {
                if (c.step() == lm::Levenberg::kBegin && c.begin_iteration(false)) {         // (linearisation and first trial in one round)
                    y.flags |= liba::kIwLin;
                    if (!err_current[i]) y.flags |= liba::kIwErrors;
                }
                if (c.step() == lm::Levenberg::kLinearize || c.step() == lm::Levenberg::kTrial) y.flags |= liba::kIwTrial;
            }
            y.lambda = c.lambda(); y.cur = cur[i];
            if (y.flags) y.seq = ++slots[i]->hs.seq;
            any_lin |= (y.flags & liba::kIwLin) != 0; any_err |= (y.flags & liba::kIwErrors) != 0; any_trial |= (y.flags & liba::kIwTrial) != 0;
        }
        if (!any_lin && !any_trial && !any_err) { if (final_round) break; final_round = true; continue; }
        const liba::IWin* dw = d_wins;
        if (any_err) hipLaunchKernelGGL(liba::ki_points_errors, dim3(max_pt, W), dim3(liba::kPtThreads), 0, stream, dw, dyn, 0);
        if (any_lin) hipLaunchKernelGGL(liba::ki_lin, dim3(max_lin, W), dim3(liba::kLinThreads), 0, stream, dw, dyn);
        if (any_trial) {
            hipLaunchKernelGGL(liba::ki_system, dim3(max_sys, W), dim3(liba::kSysThreads), 0, stream, dw, dyn);
            hipLaunchKernelGGL(liba::ki_schur_blocks, dim3(max_sb, W), dim3(1024), 0, stream, dw, dyn);
            for (int w0 = 0; w0 < W; w0 += flow_windows)
                hipLaunchKernelGGL(liba::ki_chol_flow, dim3(tiles, std::min(flow_windows, W - w0)), dim3(256), chol::kStepLds, stream, dw, dyn, w0);
            hipLaunchKernelGGL(liba::ki_solve_update, dim3(1, W), dim3(1024), chol::kFusedSolveLds, stream, dw, dyn);
            hipLaunchKernelGGL(liba::ki_points_errors, dim3(max_pt, W), dim3(liba::kPtThreads), 0, stream, dw, dyn, 1);
        }
        if (hipGetLastError() != hipSuccess) { r = fail(ORBX_ERR_HIP, "launch failed"); break; }
        if (final_round) break;
        for (int i = 0; i < W && !r; i++)
            if (dyn.w[i].flags) r = slots[i]->hs.wait(stream);
        if (r) break;
        for (int i = 0; i < W; i++) {
            lm::Levenberg& c = ctl[i];
            const int f = dyn.w[i].flags;
            const double* h = slots[i]->hs.h;
            if (f & liba::kIwErrors) err_current[i] = 1;
            if (f & liba::kIwLin) c.linearized(c.iteration() == 0 ? h[6] : c.chi2(), problems[i].lambda_init);     // (chi2 of the initial state)
            if (!(f & liba::kIwTrial)) continue;
            const lm::TrialStatus ts = lm::trial_status(h[5]);
            if (ts == lm::TrialStatus::kStalled) { r = fail(ORBX_ERR_INTERNAL, "liba_run: window %d: the factorisation stalled (a spin wait between workgroups expired)", i); break; }
            if (c.trial(ts == lm::TrialStatus::kSolved, h[0], h[3])) {
                cur[i] = 1 - cur[i];            // discardTop(): the trial state (and its errors) become current
                err_current[i] = 1;
            } else {
                err_current[i] = 0;             // pop(): the old state stays; its errors are recomputed before the next linearisation
            }
            if (!c.more_trials(false)) c.end_iteration();
        }
        if (r) break;
    }
    if (ev1) (void)hipEventRecord(ev1, stream);
    const auto t_solved = stage::Clock::now();
    if (!r) {
        // results of all windows: one epilogue launch into the handle's device buffer, ONE copy, one synchronisation, then the scatter
        for (int i = 0; i < W; i++) {
            dyn.w[i].cur = cur[i];
            if (stats_out) stats_out[i] = ctl[i].stats();
        }
        if (outputs) {
            hipLaunchKernelGGL(liba::ki_epilogue, dim3(max_epi, W), dim3(256), 0, stream, (const liba::IWin*)d_wins, dyn);
            ORBX_HIP_FIRST(r, hipGetLastError());
            ORBX_HIP_FIRST(r, hipMemcpyAsync(io->h, io->d, io->total(), hipMemcpyDeviceToHost, stream));
        }
        ORBX_HIP_FIRST(r, hipStreamSynchronize(stream));
        if (!r && device_ms && ev0 && ev1) { float ms = 0.f; if (hipEventElapsedTime(&ms, ev0, ev1) == hipSuccess) *device_ms = ms; }
        for (int i = 0; i < W && !r && outputs; i++) {
            const liba::Dev& d = hw[i].d;
            const LibaOutputs& o = outputs[i];
            const stage::PinnedOut::Slice h = io->slice(io->h + io->off[i], (size_t)d.nKF * sizeof(liba::KFState), d.nL, d.nE);
            const liba::KFState* st = (const liba::KFState*)h.state;
            for (int k = 0; k < d.nKF; k++) {
                if (o.Rwb) std::memcpy(o.Rwb + 9 * k, st[k].Rwb, 72);
                if (o.twb) std::memcpy(o.twb + 3 * k, st[k].twb, 24);
                if (o.vel) std::memcpy(o.vel + 3 * k, st[k].v, 24);
                if (o.bg) std::memcpy(o.bg + 3 * k, st[k].bg, 24);
                if (o.ba) std::memcpy(o.ba + 3 * k, st[k].ba, 24);
            }
            if (o.points && d.nL > 0) std::memcpy(o.points, h.points, 3 * (size_t)d.nL * 8);
            if (o.chi2_per_edge && d.nE > 0) std::memcpy(o.chi2_per_edge, h.chi2, (size_t)d.nE * 8);
            if (o.depth_positive && d.nE > 0) std::memcpy(o.depth_positive, h.depth, (size_t)d.nE);
        }
    } else {
        (void)hipStreamSynchronize(stream);
    }
    if (timing) {
        using stage::ms;
        int its = 0, trials = 0;
        for (int i = 0; i < W; i++) { its += ctl[i].stats().iterations; trials += ctl[i].stats().trials; }
        std::fprintf(stderr, "[liba_solve] %d window(s): structure + upload %.3f ms, %d iterations / %d trials %.3f ms, download %.3f ms\n", W, ms(t_start, t_setup),
                     its, trials, ms(t_setup, t_solved), ms(t_solved, stage::Clock::now()));
    }
    cleanup();
    return r;
}

int liba_solve(liba_solver* sv, const LibaProblem* p, double* Rwb_out, double* twb_out, double* vel_out, double* bg_out, double* ba_out,
               double* points_out, double* chi2_per_edge, uint8_t* depth_positive, LbaStats* stats_out)
{
    if (!sv) return fail(ORBX_ERR_ARG, "NULL solver");
    if (!p) return fail(ORBX_ERR_ARG, "NULL problem");
    LibaOutputs o;
    o.Rwb = Rwb_out; o.twb = twb_out; o.vel = vel_out; o.bg = bg_out; o.ba = ba_out; o.points = points_out; o.chi2_per_edge = chi2_per_edge; o.depth_positive = depth_positive;
    liba_solver* slot = sv;
    return liba_run(sv->device, sv->stream, &slot, sv->d_wins, &sv->io, p, &o, 1, stats_out, nullptr, nullptr, nullptr);
}

struct liba_batch : stage::Batch {          // its stream, the two events around the Levenberg rounds
    std::vector<liba_solver*> slots;        // one arena per window
    stage::HostScalars hs;                  // [kMaxIBatch][16]
    liba::IWin* d_wins = nullptr;
    stage::PinnedOut io;
    float last_device_ms = 0.f;
    ~liba_batch()
    {
        for (liba_solver* s : slots) delete s;
        hs.release();
        if (d_wins) (void)hipFree(d_wins);
        io.release();
    }
};

int liba_batch_create(int device, liba_batch** out)
{
    int r = stage::open(device, out);
    if (r) return r;
    liba_batch* b = *out;
    if (b->hs.alloc(liba::kMaxIBatch) != ORBX_OK || hipMalloc((void**)&b->d_wins, (size_t)liba::kMaxIBatch * sizeof(liba::IWin)) != hipSuccess ||
        liba_kernel_attributes() != ORBX_OK) {
        stage::close(b);
        *out = nullptr;
        return fail(ORBX_ERR_HIP, "batch creation failed");
    }
    return ORBX_OK;
}

void liba_batch_destroy(liba_batch* b) { stage::close(b); }

int liba_solve_batch(liba_batch* b, const LibaProblem* problems, const LibaOutputs* outputs, int n_windows, LbaStats* stats_out)
{
    if (!b || !problems || n_windows < 0) return fail(ORBX_ERR_ARG, "NULL argument");
    if (n_windows > liba::kMaxIBatch) return fail(ORBX_ERR_CAPACITY, "at most %d windows per call", liba::kMaxIBatch);
    if (n_windows == 0) return ORBX_OK;
    while ((int)b->slots.size() < n_windows) {
        liba_solver* sv = new liba_solver();
        sv->device = b->device; sv->stream = b->stream;
        sv->hs = b->hs.view((int)b->slots.size());
        b->slots.push_back(sv);
    }
    return liba_run(b->device, b->stream, b->slots.data(), b->d_wins, &b->io, problems, outputs, n_windows, stats_out, &b->last_device_ms, b->ev0, b->ev1);
}

double liba_batch_last_device_ms(const liba_batch* b) { return b ? (double)b->last_device_ms : 0.0; }

int liba_pose_optimize_batch(liba_solver* sv, const LibaPoseProblem* probs, int batch, double* Rwb_out, double* twb_out, double* vel_out,
                             double* bg_out, double* ba_out, uint8_t* outlier_out, double* H15_out, int32_t* inliers_out, int32_t* n_bad_out)
{
    if (!sv || !probs || batch < 1) return fail(ORBX_ERR_ARG, "bad arguments");
    size_t total = 0;
    for (int b = 0; b < batch; b++) {
        const LibaPoseProblem& p = probs[b];
        if (p.n < 0 || (p.n > 0 && (!p.Xw || !p.obs || !p.inv_sigma2 || !p.stereo || !p.close_point))) return fail(ORBX_ERR_ARG, "frame %d: NULL edge arrays", b);
        for (int k = 0; k < 9; k++)
            if (p.Rcb[k] != probs[0].Rcb[k]) return fail(ORBX_ERR_ARG, "frame %d: one camera-body calibration per batch", b);
        if (p.fx != probs[0].fx || p.fy != probs[0].fy || p.cx != probs[0].cx || p.cy != probs[0].cy || p.bf != probs[0].bf)
            return fail(ORBX_ERR_ARG, "frame %d: one camera per batch", b);
        if ((p.last_frame != 0) != (probs[0].last_frame != 0)) return fail(ORBX_ERR_ARG, "frame %d: one variant (last key frame / last frame) per batch", b);
        total += (size_t)p.n;
    }
    const bool lf = probs[0].last_frame != 0;
    const int NN = lf ? 30 : 15;
    ORBX_HIP(hipSetDevice(sv->device));
    sv->release();
    hipStream_t stream = sv->stream;
    // One pinned staging buffer and one device buffer with the same layout: inputs first (one copy in), then the error scratch,
    // then the outputs back to back (one copy out) -- a single frame per call is what the tracker makes, and there the copies
    // and allocations cost as much as the optimisation.
    size_t off = 0;
    auto place = [&](size_t bytes) { const size_t o = off; off = (off + std::max(bytes, (size_t)1) + 255) & ~(size_t)255; return o; };
    const size_t o_frames = place((size_t)batch * sizeof(liba::PIFrameDev)), o_Xw = place(24 * total), o_obs = place(24 * total), o_w = place(8 * total);
    const size_t o_st = place(total), o_cl = place(total), in_bytes = off;
    const size_t o_err = place(24 * total);
    const size_t o_outl = place(total), o_state = place((size_t)batch * sizeof(liba::KFState)), o_nbad = place(4 * (size_t)batch), o_H = place(8 * (size_t)NN * NN * batch);
    const size_t all_bytes = off;
    if (all_bytes > sv->h_stage_cap) {
        if (sv->h_stage) (void)hipHostFree(sv->h_stage);
        sv->h_stage = nullptr; sv->h_stage_cap = 0;
        const size_t want = all_bytes + all_bytes / 2;
        if (hipHostMalloc((void**)&sv->h_stage, want, hipHostMallocDefault) != hipSuccess) return fail(ORBX_ERR_HIP, "pinned staging buffer of %zu bytes", want);
        sv->h_stage_cap = want;
    }
    uint8_t* const hs = sv->h_stage;
    liba::PIFrameDev* frames = (liba::PIFrameDev*)(hs + o_frames);
    double* Xw = (double*)(hs + o_Xw); double* obs = (double*)(hs + o_obs); double* w = (double*)(hs + o_w);
    uint8_t* st = hs + o_st; uint8_t* cl = hs + o_cl;
    size_t e0 = 0;
    for (int b = 0; b < batch; b++) {
        const LibaPoseProblem& p = probs[b];
        liba::PIFrameDev& f = frames[b];
        std::memset(&f, 0, sizeof(f));
        liba::KFState* ks[2] = {&f.kf, &f.fr};
        for (int i = 0; i < 2; i++) {
            std::memcpy(ks[i]->Rwb, p.Rwb + 9 * i, 72); std::memcpy(ks[i]->twb, p.twb + 3 * i, 24); std::memcpy(ks[i]->v, p.vel + 3 * i, 24);
            std::memcpy(ks[i]->bg, p.bg + 3 * i, 24); std::memcpy(ks[i]->ba, p.ba + 3 * i, 24);
        }
        f.link = p.link; f.n = p.n; f.rec_init = p.rec_init; f.edge0 = e0;
        if (lf) {
            std::memcpy(f.prior_Rwb, p.prior_Rwb, 72); std::memcpy(f.prior_twb, p.prior_twb, 24); std::memcpy(f.prior_vel, p.prior_vel, 24);
            std::memcpy(f.prior_bg, p.prior_bg, 24); std::memcpy(f.prior_ba, p.prior_ba, 24); std::memcpy(f.prior_H, p.prior_H, 1800);
        }
        if (p.n > 0) {
            std::memcpy(&Xw[3 * e0], p.Xw, 24 * (size_t)p.n); std::memcpy(&obs[3 * e0], p.obs, 24 * (size_t)p.n); std::memcpy(&w[e0], p.inv_sigma2, 8 * (size_t)p.n);
            std::memcpy(&st[e0], p.stereo, (size_t)p.n); std::memcpy(&cl[e0], p.close_point, (size_t)p.n);
        }
        e0 += (size_t)p.n;
    }
    uint8_t* dev = nullptr;
    int r = sv->dalloc(&dev, all_bytes);
    if (r) { sv->release(); return r; }
    liba::PIDev d;
    std::memset(&d, 0, sizeof(d));
    d.frames = (const liba::PIFrameDev*)(dev + o_frames);
    d.Xw = (const double*)(dev + o_Xw); d.obs = (const double*)(dev + o_obs); d.w = (const double*)(dev + o_w);
    d.stereo = dev + o_st; d.close_pt = dev + o_cl;
    d.err = (double*)(dev + o_err); d.outlier = dev + o_outl;
    d.out_state = (liba::KFState*)(dev + o_state); d.n_bad = (int*)(dev + o_nbad); d.Hout = (double*)(dev + o_H);
    const LibaPoseProblem& p0 = probs[0];
    for (int k = 0; k < 9; k++) { d.Rcb[k] = p0.Rcb[k]; d.Rbc[k] = p0.Rcb[3 * (k % 3) + k / 3]; }
    for (int k = 0; k < 3; k++) { d.tcb[k] = p0.tcb[k]; d.tbc[k] = p0.tbc[k]; }
    d.fx = p0.fx; d.fy = p0.fy; d.cx = p0.cx; d.cy = p0.cy; d.bf = p0.bf; d.huber_mono = p0.huber_mono; d.huber_stereo = p0.huber_stereo;
    hipError_t e1 = hipMemcpyAsync(dev, hs, in_bytes, hipMemcpyHostToDevice, stream);
    if (e1 == hipSuccess) {
        if (lf) hipLaunchKernelGGL(liba::k_pose_inertial<true>, dim3(batch), dim3(384), 0, stream, d);
        else hipLaunchKernelGGL(liba::k_pose_inertial<false>, dim3(batch), dim3(384), 0, stream, d);
        e1 = hipGetLastError();
    }
    if (e1 == hipSuccess) e1 = hipMemcpyAsync(hs + o_outl, dev + o_outl, all_bytes - o_outl, hipMemcpyDeviceToHost, stream);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(stream);
    sv->release();
    if (e1 != hipSuccess) return fail(ORBX_ERR_HIP, "pose-inertial batch: %s", hipGetErrorString(e1));
    const liba::KFState* out = (const liba::KFState*)(hs + o_state);
    const int* nbad = (const int*)(hs + o_nbad);
    if (H15_out) std::memcpy(H15_out, hs + o_H, 8 * (size_t)NN * NN * batch);
    if (outlier_out && total > 0) std::memcpy(outlier_out, hs + o_outl, total);
    for (int b = 0; b < batch; b++) {
        if (Rwb_out) std::memcpy(Rwb_out + 9 * b, out[b].Rwb, 72);
        if (twb_out) std::memcpy(twb_out + 3 * b, out[b].twb, 24);
        if (vel_out) std::memcpy(vel_out + 3 * b, out[b].v, 24);
        if (bg_out) std::memcpy(bg_out + 3 * b, out[b].bg, 24);
        if (ba_out) std::memcpy(ba_out + 3 * b, out[b].ba, 24);
        if (n_bad_out) n_bad_out[b] = nbad[b];
        if (inliers_out) inliers_out[b] = probs[b].n - nbad[b];
    }
    return ORBX_OK;
}

#ifdef LIBA_PI_TIMING
int liba_debug_pi_prof(unsigned long long* out16, int reset)
{
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(liba::d_pi_prof), 16 * sizeof(unsigned long long)) != hipSuccess) return ORBX_ERR_HIP;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(liba::d_pi_prof), z, sizeof(z)) != hipSuccess) return ORBX_ERR_HIP; }
    return ORBX_OK;
}
#endif

}  // extern "C"
