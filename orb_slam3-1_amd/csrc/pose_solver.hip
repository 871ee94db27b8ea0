// pose_solver.hip -- gfx950 kernel + C ABI for Optimizer::PoseOptimization (reference src/Optimizer.cc:814-1115):
// motion-only bundle adjustment of one frame.  SURVEY.md 8(f) rank 1 ("next" row): it runs every frame right after
// matching (src/Tracking.cc:2889,3053,3115).
//
// MI355X mapping: the problem is tiny (one 6-dof pose, a few hundred unary edges, a 6x6 system) and strictly sequential in
// its control flow (4 rounds x <=10 LM iterations x <=10 trials), so a launch per step would be pure latency.  Instead ONE
// 256-thread workgroup runs the whole optimisation of a frame on the device -- edges in registers/L2, ordered block
// reductions for chi2 / H / b, the 6x6 LDL^T, SE3 exp and all Levenberg and outlier bookkeeping -- and a batch of frames
// is one launch with one workgroup per frame (frames are independent: they shard over workgroups and GPUs alike).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbslam3_hip.h"
#include "../../include/orbslam3_hip_rig_track_device.h"
#include "batch_stage.h"
#include "camera_kb8.h"
#include "camera_kb8_host.h"
#include "dense_lm_device.h"
#include "se3_device.h"

namespace poseopt {

using namespace se3;

struct ProblemDev {
    double q[4], t[3];
    int32_t n;
    const double* Xw; const double* obs; const double* w; const uint8_t* stereo;
    double fx, fy, cx, cy, bf, huber_mono, huber_stereo;
    double* err;            // [3n] scratch: edge._error as last computed
    uint8_t* outlier;       // [n] out
    uint8_t* active;        // [n] scratch: level 0
    PoseResult* result;
};

// camera policies of the edge bodies: the pinhole one reads fx .. bf of the problem, the fisheye one carries its own eight parameters
// (monocular edges only; pose_set_camera_kb8)
struct Pinhole { static constexpr bool kFisheye = false, kRig = false; };
struct Fisheye { static constexpr bool kFisheye = true, kRig = false; kb8::Cam c; };
// a rig of two fisheye cameras (pose_set_rig_kb8): Edge::st is the camera of the edge, 0 left, ORBX_EDGE_RIGHT right; two residual rows
struct RigCam { static constexpr bool kFisheye = true, kRig = true; kb8::Rig g; };

// one edge in registers
struct Edge {
    double X[3], o[3], w;
    int st;
};

template <bool STEREO>
__device__ __forceinline__ Edge load_edge(const ProblemDev& P, int e)
{
    Edge d;
    const double* X = P.Xw + 3 * (size_t)e;
    const double* o = P.obs + 3 * (size_t)e;
    d.X[0] = X[0]; d.X[1] = X[1]; d.X[2] = X[2];
    d.o[0] = o[0]; d.o[1] = o[1]; d.o[2] = STEREO ? o[2] : 0.0;
    d.w = P.w[e];
    d.st = STEREO ? (int)P.stereo[e] : 0;
    return d;
}
template <bool STEREO, class CamT>
__device__ __forceinline__ Edge load_edge(const CamT&, const ProblemDev& P, int e)
{
    Edge d = load_edge<STEREO>(P, e);
    if constexpr (CamT::kRig) d.st = (int)P.stereo[e];
    return d;
}

// EdgeSE3ProjectXYZOnlyPose::computeError (include/OptimizableTypes.h:46-50) and
// EdgeStereoSE3ProjectXYZOnlyPose::computeError (types_six_dof_expmap.h:203-207, cam_project .cpp:339-346)
template <bool STEREO, class CamT>
__device__ __forceinline__ void edge_eval(const CamT& cam, const ProblemDev& P, const double* T, const Edge& d, double* Xc, double* r)
{
    pose_map(T, d.X, Xc);
    if constexpr (CamT::kRig) {                                 // a right edge: obs - pCamera->project(Trl Xc) (OptimizableTypes.h:69-73)
        double uv[2], Xp[3];
        kb8::rig_project(cam.g, d.st != 0, Xc, Xp, uv);
        r[0] = d.o[0] - uv[0]; r[1] = d.o[1] - uv[1]; r[2] = 0;
    } else if constexpr (CamT::kFisheye) {                      // obs - pCamera->project(Xc) (OptimizableTypes.h:46-50)
        double uv[2];
        kb8::project(cam.c, Xc, uv);
        r[0] = d.o[0] - uv[0]; r[1] = d.o[1] - uv[1]; r[2] = 0;
    } else if (!STEREO || !d.st) {
        r[0] = d.o[0] - (P.fx * Xc[0] / Xc[2] + P.cx);
        r[1] = d.o[1] - (P.fy * Xc[1] / Xc[2] + P.cy);
        r[2] = 0;
    } else {
        const float invz = (float)(1.0 / Xc[2]);             // 1.0f/double rounded to float (types_six_dof_expmap.cpp:340)
        const double u = Xc[0] * (double)invz * P.fx + P.cx;
        const double v = Xc[1] * (double)invz * P.fy + P.cy;
        r[0] = d.o[0] - u; r[1] = d.o[1] - v; r[2] = d.o[2] - (u - P.bf * (double)invz);
    }
}

template <bool STEREO>
__device__ __forceinline__ double edge_chi2(const Edge& d, const double* r)
{
    double c = r[0] * (d.w * r[0]) + r[1] * (d.w * r[1]);
    if (STEREO && d.st) c += r[2] * (d.w * r[2]);
    return c;
}

struct Robust {
    bool on;
    double delta_m, delta_s, dsq_m, dsq_s;
};

// computeError + robustify + linearizeOplus + constructQuadraticForm of one edge, accumulated into acc[28]
template <bool STEREO, class CamT>
__device__ __forceinline__ void edge_build(const CamT& cam, const ProblemDev& P, const double* T, const Edge& d, const Robust& rb, double* r, double* acc)
{
    constexpr int D = STEREO ? 3 : 2;
    double Xc[3], J[D * 6];
    edge_eval<STEREO>(cam, P, T, d, Xc, r);
    const double chi = edge_chi2<STEREO>(d, r);
    const double delta = (STEREO && d.st) ? rb.delta_s : rb.delta_m, dsq = (STEREO && d.st) ? rb.dsq_s : rb.dsq_m;
    double rho0, rho1;
    dlm::huber(rb.on, chi, delta, dsq, rho0, rho1);
    acc[27] += rho0;
    const double x = Xc[0], y = Xc[1], z = Xc[2];
    if constexpr (CamT::kRig) {                                 // -projectJac(X_r) * R_rl * SE3deriv(X_l) on a right edge (OptimizableTypes.cpp:91-107)
        double N[6];
        kb8::rig_pose_rows(cam.g, d.st != 0, Xc, N, J);
    } else if constexpr (CamT::kFisheye) {                      // -projectJac(Xc) * SE3deriv (OptimizableTypes.cpp:24-38)
        double N[6];
        kb8::pose_rows(cam.c, Xc, N, J);
    } else if (!STEREO || !d.st) {
        const double p00 = -(P.fx / z), p02 = P.fx * x / (z * z), p11 = -(P.fy / z), p12 = P.fy * y / (z * z);
        J[0] = p02 * y; J[1] = p00 * z + p02 * (-x); J[2] = p00 * (-y); J[3] = p00; J[4] = 0; J[5] = p02;
        J[6] = p11 * (-z) + p12 * y; J[7] = p12 * (-x); J[8] = p11 * x; J[9] = 0; J[10] = p11; J[11] = p12;
        if (STEREO) for (int k = 12; k < D * 6; k++) J[k] = 0;
    } else {
        const double invz = 1.0 / z, iz2 = invz * invz, fx = P.fx, fy = P.fy, bf = P.bf;
        J[0] = x * y * iz2 * fx; J[1] = -(1 + (x * x * iz2)) * fx; J[2] = y * invz * fx; J[3] = -invz * fx; J[4] = 0; J[5] = x * iz2 * fx;
        J[6] = (1 + y * y * iz2) * fy; J[7] = -x * y * iz2 * fy; J[8] = -x * invz * fy; J[9] = 0; J[10] = -invz * fy; J[11] = y * iz2 * fy;
        J[(D - 1) * 6 + 0] = J[0] - bf * y * iz2; J[(D - 1) * 6 + 1] = J[1] + bf * x * iz2; J[(D - 1) * 6 + 2] = J[2];
        J[(D - 1) * 6 + 3] = J[3]; J[(D - 1) * 6 + 4] = 0; J[(D - 1) * 6 + 5] = J[5] - bf * iz2;
    }
    // fixed trip counts (the third row of a mono edge is zero) so that everything stays in registers
    const double rw = rho1 * d.w;
    double wr[D];
#pragma unroll
    for (int q = 0; q < D; q++) wr[q] = d.w * r[q];
#pragma unroll
    for (int a = 0; a < 6; a++) {
#pragma unroll
        for (int c = a; c < 6; c++) {
            double h = 0;
#pragma unroll
            for (int q = 0; q < D; q++) h += J[q * 6 + a] * rw * J[q * 6 + c];
            acc[a * 6 - (a * (a - 1)) / 2 + (c - a)] += h;
        }
        double sv = 0;
#pragma unroll
        for (int q = 0; q < D; q++) sv += J[q * 6 + a] * wr[q];
        acc[21 + a] -= rho1 * sv;
    }
}

// computeError + robust chi2 of one edge under the trial pose
template <bool STEREO, class CamT>
__device__ __forceinline__ double edge_trial(const CamT& cam, const ProblemDev& P, const double* T, const Edge& d, const Robust& rb, double* r)
{
    double Xc[3];
    edge_eval<STEREO>(cam, P, T, d, Xc, r);
    const double chi = edge_chi2<STEREO>(d, r);
    const double delta = (STEREO && d.st) ? rb.delta_s : rb.delta_m, dsq = (STEREO && d.st) ? rb.dsq_s : rb.dsq_m;
    double rho0, rho1;
    dlm::huber(rb.on, chi, delta, dsq, rho0, rho1);
    return rho0;
}

// float chi2 against the 95 % thresholds (src/Optimizer.cc:1020-1034, 1049-1063)
template <bool STEREO>
__device__ __forceinline__ bool edge_is_outlier(const Edge& d, const double* r)
{
    const float chi2 = (float)edge_chi2<STEREO>(d, r);
    return chi2 > ((STEREO && d.st) ? 7.815f : 5.991f);
}

constexpr int kAccRow = 264;        // 256 partials + one pad per 32 (bank spread for the strided second stage)
// kRegEdges (template parameter R of the kernel): edges per thread held in registers -- 2 (n <= 512 never re-reads global memory) or,
// for frames with more edges (TrackWithMotionModel matches ~750 of 1000 features), 4; the per-thread summation order is the same.

// STEREO = the batch holds at least one stereo edge; the mono instantiation carries 2-row Jacobians only.
// The Levenberg state (pose, lambda, chi2, counters) and the 6x6 solve are REPLICATED in every thread: all lanes run the
// same scalar code on the same reduced values, so no broadcast barriers sit between the solve, the trial pass and the
// accept / reject decision -- the only synchronisation left is inside the two block reductions.
// The camera is a pack: empty for the pinhole kernels (no camera argument), else the one Fisheye / RigCam the kernel receives by value
// (monocular edges only, or left and right fisheye edges interleaved with the kind of an edge in the problem's stereo byte: kStereo is
// false in both).
__device__ __forceinline__ Pinhole camera_arg() { return Pinhole(); }
template <class C> __device__ __forceinline__ const C& camera_arg(const C& c) { return c; }
template <bool kStereo, int kRegEdges, class... CamT>
__global__ __launch_bounds__(256) void k_pose_opt(const ProblemDev* __restrict__ problems, CamT... cam_arg)
{
    constexpr bool STEREO = kStereo;
    const auto& cam = camera_arg(cam_arg...);
#include "pose_opt_body.inc"
}

// ---- device-resident entry (pose_optimize_batch_device): the frame's edges are gathered ON THE DEVICE from the arrays the extractor
// and the projection search left there, in feature order (the order Optimizer::PoseOptimization walks mvpMapPoints, :861-996) ----
struct GatherArgs {
    const OrbxKeyPoint* kps; const int32_t* n_kps; const float* u_right; const int32_t* assign; const float* mp_xyz; const double* pose;
    int32_t cap, mp_cap, n_levels;
    float inv_sigma2[16];
    double fx, fy, cx, cy, bf, huber_mono, huber_stereo;
    uint8_t* slots; size_t slot_bytes;              // per frame: [Xw | obs | w | err | idx | stereo | outl | act]
    size_t o_obs, o_w, o_err, o_idx, o_st, o_outl, o_act;
    ProblemDev* problems; PoseResult* results;
};

// one workgroup per frame: ordered compaction of the features that hold a map point (assign >= 0) into the solver's edge arrays;
// float -> double exactly as the reference casts them (obs << kpUn.pt.x ..., GetWorldPos().cast<double>(), mvInvLevelSigma2)
__global__ __launch_bounds__(256) void k_pose_gather(GatherArgs A)
{
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint8_t* slot = A.slots + (size_t)b * A.slot_bytes;
    double* Xw = (double*)slot; double* obs = (double*)(slot + A.o_obs); double* w = (double*)(slot + A.o_w);
    int32_t* idx = (int32_t*)(slot + A.o_idx); uint8_t* st = slot + A.o_st;
    const int n = min(max(A.n_kps[b], 0), A.cap);
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        int j = -1;
        if (i < n) { j = A.assign[(size_t)b * A.cap + i]; if (j >= A.mp_cap) j = -1; }
        const bool has = j >= 0;
        const unsigned long long bal = __ballot(has);
        const int in_wave = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = s_base;
        for (int q = 0; q < wave; q++) before += s_wave[q];
        if (has) {
            const int e = before + in_wave;
            const OrbxKeyPoint k = A.kps[(size_t)b * A.cap + i];
            const float* X = A.mp_xyz + 3 * ((size_t)b * A.mp_cap + j);
            const float ur = A.u_right ? A.u_right[(size_t)b * A.cap + i] : -1.0f;
            Xw[3 * (size_t)e] = (double)X[0]; Xw[3 * (size_t)e + 1] = (double)X[1]; Xw[3 * (size_t)e + 2] = (double)X[2];
            obs[3 * (size_t)e] = (double)k.x; obs[3 * (size_t)e + 1] = (double)k.y; obs[3 * (size_t)e + 2] = (double)ur;
            const int oc = min(max(k.octave, 0), A.n_levels - 1);
            w[e] = (double)A.inv_sigma2[oc];
            st[e] = (A.u_right && !(ur < 0.0f)) ? 1 : 0;          // mvuRight[i] < 0: monocular observation (:869)
            idx[e] = i;
        }
        __syncthreads();
        if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (tid == 0) {
        ProblemDev P;
        for (int k = 0; k < 4; k++) P.q[k] = A.pose[7 * (size_t)b + k];
        for (int k = 0; k < 3; k++) P.t[k] = A.pose[7 * (size_t)b + 4 + k];
        P.n = s_base;
        P.Xw = Xw; P.obs = obs; P.w = w; P.stereo = st;
        P.fx = A.fx; P.fy = A.fy; P.cx = A.cx; P.cy = A.cy; P.bf = A.bf; P.huber_mono = A.huber_mono; P.huber_stereo = A.huber_stereo;
        P.err = (double*)(slot + A.o_err); P.outlier = slot + A.o_outl; P.active = slot + A.o_act;
        P.result = A.results + b;
        A.problems[b] = P;
    }
}

// ---- device-resident entry for two-camera fisheye rig frames (pose_optimize_rig_batch_device) ----
struct RigGatherArgs {
    const OrbxKeyPoint* kps_l; const int32_t* n_l; const OrbxKeyPoint* kps_r; const int32_t* n_r; const int32_t* assign; const float* mp_xyz; const double* pose;
    int32_t cap_l, cap_r, slot_cap, mp_cap, n_levels;
    float inv_sigma2[16];
    double huber_mono;
    uint8_t* slots; size_t slot_bytes;              // per frame, as GatherArgs
    size_t o_obs, o_w, o_err, o_idx, o_st, o_outl, o_act;
    ProblemDev* problems; PoseResult* results;
};

// k_pose_gather over the SLOTS of a rig frame (mvpMapPoints[0 .. Nleft+Nright), right slot j at n_l + j): a slot below n_l that holds
// a point becomes a left edge observing mvKeys[s], any other a right edge (ORBX_EDGE_RIGHT) observing mvKeysRight[s - n_l] -- the order
// in which Optimizer::PoseOptimization walks a rig frame (:935-990)
__global__ __launch_bounds__(256) void k_pose_gather_rig(RigGatherArgs A)
{
    __shared__ int s_wave[4];
    __shared__ int s_base;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint8_t* slot = A.slots + (size_t)b * A.slot_bytes;
    double* Xw = (double*)slot; double* obs = (double*)(slot + A.o_obs); double* w = (double*)(slot + A.o_w);
    int32_t* idx = (int32_t*)(slot + A.o_idx); uint8_t* st = slot + A.o_st;
    const int nl = min(max(A.n_l[b], 0), A.cap_l), nr = min(max(A.n_r[b], 0), A.cap_r), n = nl + nr;
    if (tid == 0) s_base = 0;
    __syncthreads();
    for (int i0 = 0; i0 < n; i0 += 256) {
        const int i = i0 + tid;
        int j = -1;
        if (i < n) { j = A.assign[(size_t)b * A.slot_cap + i]; if (j >= A.mp_cap) j = -1; }
        const bool has = j >= 0;
        const unsigned long long bal = __ballot(has);
        const int in_wave = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
        if (lane == 0) s_wave[wave] = __popcll(bal);
        __syncthreads();
        int before = s_base;
        for (int q = 0; q < wave; q++) before += s_wave[q];
        if (has) {
            const int e = before + in_wave;
            const bool right = i >= nl;
            const OrbxKeyPoint k = right ? A.kps_r[(size_t)b * A.cap_r + (i - nl)] : A.kps_l[(size_t)b * A.cap_l + i];
            const float* X = A.mp_xyz + 3 * ((size_t)b * A.mp_cap + j);
            Xw[3 * (size_t)e] = (double)X[0]; Xw[3 * (size_t)e + 1] = (double)X[1]; Xw[3 * (size_t)e + 2] = (double)X[2];
            obs[3 * (size_t)e] = (double)k.x; obs[3 * (size_t)e + 1] = (double)k.y; obs[3 * (size_t)e + 2] = -1.0;
            const int oc = min(max(k.octave, 0), A.n_levels - 1);
            w[e] = (double)A.inv_sigma2[oc];
            st[e] = right ? ORBX_EDGE_RIGHT : 0;
            idx[e] = i;
        }
        __syncthreads();
        if (tid == 0) s_base += s_wave[0] + s_wave[1] + s_wave[2] + s_wave[3];
        __syncthreads();
    }
    if (tid == 0) {
        ProblemDev P;
        for (int k = 0; k < 4; k++) P.q[k] = A.pose[7 * (size_t)b + k];
        for (int k = 0; k < 3; k++) P.t[k] = A.pose[7 * (size_t)b + 4 + k];
        P.n = s_base;
        P.Xw = Xw; P.obs = obs; P.w = w; P.stereo = st;
        P.fx = P.fy = P.cx = P.cy = P.bf = 0.0;          // the rig's cameras are the kernel's argument
        P.huber_mono = A.huber_mono; P.huber_stereo = 0.0;
        P.err = (double*)(slot + A.o_err); P.outlier = slot + A.o_outl; P.active = slot + A.o_act;
        P.result = A.results + b;
        A.problems[b] = P;
    }
}

// results back into per-feature / per-frame arrays: mvbOutlier[i] (0 for a feature without a map point), the pose, the return value
__global__ __launch_bounds__(256) void k_pose_scatter(const ProblemDev* __restrict__ problems, const uint8_t* __restrict__ slots, size_t slot_bytes, size_t o_idx,
                                                      int cap, double* __restrict__ pose_out, int32_t* __restrict__ inliers, uint8_t* __restrict__ outlier,
                                                      PoseResult* __restrict__ results_out)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const ProblemDev& P = problems[b];
    const int32_t* idx = (const int32_t*)(slots + (size_t)b * slot_bytes + o_idx);
    if (outlier) {
        for (int i = tid; i < cap; i += 256) outlier[(size_t)b * cap + i] = 0;
        __syncthreads();
        for (int e = tid; e < P.n; e += 256) outlier[(size_t)b * cap + idx[e]] = P.outlier[e];
    }
    if (tid == 0) {
        const PoseResult R = *P.result;
        if (pose_out) { for (int k = 0; k < 4; k++) pose_out[7 * (size_t)b + k] = R.q[k]; for (int k = 0; k < 3; k++) pose_out[7 * (size_t)b + 4 + k] = R.t[k]; }
        if (inliers) inliers[b] = R.inliers;
        if (results_out) results_out[b] = R;
    }
}

// orbx_kb8_project: kb8::project and kb8::project_jac of n points
__global__ __launch_bounds__(256) void k_kb8_project(kb8::Cam c, const double* __restrict__ X, int n, double* __restrict__ uv, double* __restrict__ jac)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double x[3] = {X[3 * (size_t)i], X[3 * (size_t)i + 1], X[3 * (size_t)i + 2]};
    double o[2];
    kb8::project(c, x, o);
    uv[2 * (size_t)i] = o[0]; uv[2 * (size_t)i + 1] = o[1];
    if (jac) {
        double J[6];
        kb8::project_jac(c, x, J);
        for (int k = 0; k < 6; k++) jac[6 * (size_t)i + k] = J[k];
    }
}

}  // namespace poseopt

// staging: [descriptors | inputs] up, [results | outlier flags] down, scratch behind them on the device
struct pose_solver : stage::Batch {
    uint8_t* d_dev = nullptr;       // arena of the device-resident entry (edge slots, problem descriptors, results)
    size_t dev_cap = 0;
    kb8::CameraChoice camera;       // pose_set_camera_kb8: the fisheye camera replaces fx .. bf of every problem; pose_set_rig_kb8: two of them,
                                    // the stereo byte of an edge names its camera
    ~pose_solver() { if (d_dev) (void)hipFree(d_dev); }
};

namespace {
inline poseopt::Fisheye policy(const kb8::Cam& c) { return poseopt::Fisheye{c}; }
inline poseopt::RigCam policy(const kb8::Rig& g) { return poseopt::RigCam{g}; }

// cam: nothing (pinhole; the stereo instantiation if the batch holds a stereo edge), or the Fisheye / RigCam of the handle
template <class... CamT>
inline void pose_launch(bool stereo, bool many_edges, int n, hipStream_t st, const poseopt::ProblemDev* p, const CamT&... cam)
{
    if constexpr (sizeof...(CamT) == 0) {
        if (stereo) {
            if (many_edges) hipLaunchKernelGGL((poseopt::k_pose_opt<true, 4>), dim3(n), dim3(256), 0, st, p);
            else hipLaunchKernelGGL((poseopt::k_pose_opt<true, 2>), dim3(n), dim3(256), 0, st, p);
            return;
        }
    }
    if (many_edges) hipLaunchKernelGGL((poseopt::k_pose_opt<false, 4, CamT...>), dim3(n), dim3(256), 0, st, p, cam...);
    else hipLaunchKernelGGL((poseopt::k_pose_opt<false, 2, CamT...>), dim3(n), dim3(256), 0, st, p, cam...);
}

// The arena of the device-resident entries, sized by the capacity of a frame (features, or slots of a rig frame): per frame the edge
// slots [Xw | obs | w | err | idx | stereo | outl | act], then the problem descriptors and the results.  Fills the layout fields of A
// (GatherArgs / RigGatherArgs).  The arena grows on demand: the only synchronising step (first call / larger batch).
template <class Args>
int device_arena(pose_solver* s, size_t cap, int batch, Args& A)
{
    stage::Cursor slot;                 // Xw at 0
    slot.take(24 * cap);
    A.o_obs = slot.take(24 * cap);
    A.o_w = slot.take(8 * cap);
    A.o_err = slot.take(24 * cap);
    A.o_idx = slot.take(4 * cap);
    A.o_st = slot.take(cap);
    A.o_outl = slot.take(cap);
    A.o_act = slot.take(cap);
    A.slot_bytes = slot.pos;
    stage::Cursor arena;
    arena.take(A.slot_bytes * (size_t)batch);
    const size_t prob_off = arena.take(sizeof(poseopt::ProblemDev) * (size_t)batch);
    const size_t res_off = arena.take(sizeof(PoseResult) * (size_t)batch);
    const size_t total = arena.pos;
    if (total > s->dev_cap) {
        if (s->d_dev) { ORBX_HIP(hipDeviceSynchronize()); (void)hipFree(s->d_dev); }
        s->d_dev = nullptr; s->dev_cap = 0;
        ORBX_HIP(hipMalloc((void**)&s->d_dev, total));
        s->dev_cap = total;
    }
    A.slots = s->d_dev;
    A.problems = (poseopt::ProblemDev*)(s->d_dev + prob_off);
    A.results = (PoseResult*)(s->d_dev + res_off);
    return ORBX_OK;
}

int optimize_batch(pose_solver* s, const PoseProblem* problems, int n_problems, PoseResult* results, uint8_t* const* outlier_out)
{
    if (!s || !problems || !results || n_problems < 1) return fail(ORBX_ERR_ARG, "bad arguments");
    if (s->camera.kind == kb8::CameraChoice::kFisheye)          // a fisheye frame is monocular (or a two-camera rig, which this library does not take): before any device work
        for (int i = 0; i < n_problems; i++)
            for (int k = 0; k < problems[i].n && problems[i].stereo; k++)
                if (problems[i].stereo[k]) return fail(ORBX_ERR_ARG, "problem %d: edge %d is stereo, the handle's camera is KannalaBrandt8", i, k);
    if (s->camera.kind == kb8::CameraChoice::kRig)          // a rig frame holds left (0) and right (ORBX_EDGE_RIGHT) edges only: before any device work
        for (int i = 0; i < n_problems; i++)
            for (int k = 0; k < problems[i].n && problems[i].stereo; k++)
                if (problems[i].stereo[k] != 0 && problems[i].stereo[k] != ORBX_EDGE_RIGHT)
                    return fail(ORBX_ERR_ARG, "problem %d: edge %d has kind %d, the handle's camera is a KannalaBrandt8 rig (0 or %d)", i, k, (int)problems[i].stereo[k], ORBX_EDGE_RIGHT);
    ORBX_HIP(hipSetDevice(s->device));
    // layout: [ProblemDev x N][per problem: Xw obs w stereo]  ||  [PoseResult x N][per problem: outlier]  ||  scratch
    struct Off { size_t Xw, obs, w, st, outl, err, act; };
    std::vector<Off> offs(n_problems);
    stage::Cursor cur;
    cur.take(sizeof(poseopt::ProblemDev) * (size_t)n_problems);
    for (int i = 0; i < n_problems; i++) {
        const PoseProblem& p = problems[i];
        if (p.n < 0 || (p.n > 0 && (!p.Xw || !p.obs || !p.inv_sigma2 || !p.stereo))) return fail(ORBX_ERR_ARG, "problem %d: NULL arrays", i);
        const size_t n = (size_t)p.n;
        Off& o = offs[i];
        o.Xw = cur.take(24 * n);
        o.obs = cur.take(24 * n);
        o.w = cur.take(8 * n);
        o.st = cur.take(n);
    }
    const size_t up_bytes = cur.pos;
    const size_t res_off = cur.take(sizeof(PoseResult) * (size_t)n_problems);
    for (int i = 0; i < n_problems; i++) offs[i].outl = cur.take((size_t)std::max(problems[i].n, 1));
    const size_t down_end = cur.pos;
    for (int i = 0; i < n_problems; i++) {
        const size_t n = (size_t)std::max(problems[i].n, 1);
        offs[i].err = cur.take(24 * n);
        offs[i].act = cur.take(n);
    }
    const int rc = stage::reserve(*s, down_end, cur.pos);       // the scratch is never staged on the host
    if (rc != ORBX_OK) return rc;
    uint8_t* base = s->d_blob;
    poseopt::ProblemDev* descs = (poseopt::ProblemDev*)s->h_blob;
    bool any_stereo = false;
    int n_max = 0;
    for (int i = 0; i < n_problems; i++) {
        const PoseProblem& p = problems[i];
        const Off& o = offs[i];
        const size_t n = (size_t)p.n;
        n_max = std::max(n_max, p.n);
        for (size_t k = 0; k < n && !any_stereo; k++) any_stereo = p.stereo[k] != 0;
        if (n) {
            std::memcpy(s->h_blob + o.Xw, p.Xw, 24 * n); std::memcpy(s->h_blob + o.obs, p.obs, 24 * n);
            std::memcpy(s->h_blob + o.w, p.inv_sigma2, 8 * n); std::memcpy(s->h_blob + o.st, p.stereo, n);
        }
        poseopt::ProblemDev d;
        for (int k = 0; k < 4; k++) d.q[k] = p.q[k];
        for (int k = 0; k < 3; k++) d.t[k] = p.t[k];
        d.n = p.n;
        d.Xw = (const double*)(base + o.Xw); d.obs = (const double*)(base + o.obs); d.w = (const double*)(base + o.w); d.stereo = base + o.st;
        d.fx = p.fx; d.fy = p.fy; d.cx = p.cx; d.cy = p.cy; d.bf = p.bf; d.huber_mono = p.huber_mono; d.huber_stereo = p.huber_stereo;
        d.err = (double*)(base + o.err); d.outlier = base + o.outl; d.active = base + o.act;
        d.result = (PoseResult*)(base + res_off) + i;
        descs[i] = d;
    }
    const int rr = stage::run(*s, up_bytes, res_off, down_end, [&] {
        kb8::with_camera(s->camera, [&](const auto&... cam) { pose_launch(any_stereo, n_max > 512, n_problems, s->stream, (const poseopt::ProblemDev*)base, policy(cam)...); });
    });
    if (rr != ORBX_OK) return rr;
    std::memcpy(results, s->h_blob + res_off, sizeof(PoseResult) * (size_t)n_problems);
    if (outlier_out)
        for (int i = 0; i < n_problems; i++)
            if (outlier_out[i] && problems[i].n > 0) std::memcpy(outlier_out[i], s->h_blob + offs[i].outl, (size_t)problems[i].n);
    return ORBX_OK;
}
}  // namespace

extern "C" {

int pose_create(int device, pose_solver** out) { return stage::open(device, out); }

void pose_destroy(pose_solver* s) { stage::close(s); }

float pose_last_kernel_ms(const pose_solver* s) { return s ? s->last_kernel_ms : 0.0f; }

int pose_optimize_batch(pose_solver* s, const PoseProblem* problems, int n_problems, PoseResult* results, uint8_t* const* outlier_out)
{
    return stage::guarded("pose_optimize_batch", [&] { return optimize_batch(s, problems, n_problems, results, outlier_out); });
}

int pose_optimize_batch_device(pose_solver* s, const PoseDeviceFrames* f, int batch, double* d_pose_out, int32_t* d_inliers,
                               uint8_t* d_outlier, PoseResult* d_results, void* stream)
{
    if (!s || !f || batch < 1) return fail(ORBX_ERR_ARG, "bad arguments");
    if (s->camera.kind == kb8::CameraChoice::kRig) return fail(ORBX_ERR_ARG, "pose_optimize_batch_device has no KannalaBrandt8 rig path: reset the camera (pose_set_rig_kb8(s, NULL)) or use pose_optimize_batch");
    if (s->camera.kind == kb8::CameraChoice::kFisheye) return fail(ORBX_ERR_ARG, "pose_optimize_batch_device has no KannalaBrandt8 path: reset the camera (pose_set_camera_kb8(s, NULL)) or use pose_optimize_batch");
    if (!f->d_kps || !f->d_n || !f->d_assign || !f->d_mp_xyz || !f->d_pose || !f->inv_level_sigma2) return fail(ORBX_ERR_ARG, "NULL arrays");
    if (f->cap < 1 || f->mp_cap < 1 || f->n_levels < 1 || f->n_levels > 16) return fail(ORBX_ERR_ARG, "bad cap / mp_cap / n_levels");
    ORBX_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    poseopt::GatherArgs A;
    std::memset(&A, 0, sizeof(A));
    if (int r = device_arena(s, (size_t)f->cap, batch, A)) return r;
    A.kps = f->d_kps; A.n_kps = f->d_n; A.u_right = f->d_u_right; A.assign = f->d_assign; A.mp_xyz = f->d_mp_xyz; A.pose = f->d_pose;
    A.cap = f->cap; A.mp_cap = f->mp_cap; A.n_levels = f->n_levels;
    for (int l = 0; l < f->n_levels; l++) A.inv_sigma2[l] = f->inv_level_sigma2[l];
    A.fx = f->fx; A.fy = f->fy; A.cx = f->cx; A.cy = f->cy; A.bf = f->bf; A.huber_mono = f->huber_mono; A.huber_stereo = f->huber_stereo;
    hipLaunchKernelGGL(poseopt::k_pose_gather, dim3(batch), dim3(256), 0, st, A);
    pose_launch(f->d_u_right != nullptr, f->cap > 512, batch, st, (const poseopt::ProblemDev*)A.problems);
    hipLaunchKernelGGL(poseopt::k_pose_scatter, dim3(batch), dim3(256), 0, st, (const poseopt::ProblemDev*)A.problems, (const uint8_t*)s->d_dev, A.slot_bytes, A.o_idx,
                       f->cap, d_pose_out, d_inliers, d_outlier, d_results);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int pose_optimize_rig_batch_device(pose_solver* s, const PoseDeviceRigFrames* f, int batch, double* d_pose_out, int32_t* d_inliers,
                                   uint8_t* d_outlier, PoseResult* d_results, void* stream)
{
    if (!f || batch < 1) return fail(ORBX_ERR_ARG, "bad arguments");
    if (!f->d_kps_l || !f->d_n_l || !f->d_kps_r || !f->d_n_r || !f->d_assign || !f->d_mp_xyz || !f->d_pose || !f->inv_level_sigma2) return fail(ORBX_ERR_ARG, "NULL arrays");
    if (f->cap_l < 1 || f->cap_r < 1 || f->mp_cap < 1 || f->n_levels < 1 || f->n_levels > 16) return fail(ORBX_ERR_ARG, "bad cap_l / cap_r / mp_cap / n_levels");
    if ((int64_t)f->slot_cap < (int64_t)f->cap_l + f->cap_r) return fail(ORBX_ERR_ARG, "slot_cap %d below cap_l + cap_r = %d + %d", f->slot_cap, f->cap_l, f->cap_r);
    if (!s) return fail(ORBX_ERR_ARG, "NULL solver");
    if (s->camera.kind != kb8::CameraChoice::kRig) return fail(ORBX_ERR_ARG, "pose_optimize_rig_batch_device needs a handle with a KannalaBrandt8 rig (pose_set_rig_kb8)");
    ORBX_HIP(hipSetDevice(s->device));
    hipStream_t st = (hipStream_t)stream;
    poseopt::RigGatherArgs A;
    std::memset(&A, 0, sizeof(A));
    if (int r = device_arena(s, (size_t)f->slot_cap, batch, A)) return r;
    A.kps_l = f->d_kps_l; A.n_l = f->d_n_l; A.kps_r = f->d_kps_r; A.n_r = f->d_n_r; A.assign = f->d_assign; A.mp_xyz = f->d_mp_xyz; A.pose = f->d_pose;
    A.cap_l = f->cap_l; A.cap_r = f->cap_r; A.slot_cap = f->slot_cap; A.mp_cap = f->mp_cap; A.n_levels = f->n_levels;
    for (int l = 0; l < f->n_levels; l++) A.inv_sigma2[l] = f->inv_level_sigma2[l];
    A.huber_mono = f->huber_mono;
    hipLaunchKernelGGL(poseopt::k_pose_gather_rig, dim3(batch), dim3(256), 0, st, A);
    kb8::with_camera(s->camera, [&](const auto&... cam) { pose_launch(false, f->slot_cap > 512, batch, st, (const poseopt::ProblemDev*)A.problems, policy(cam)...); });
    hipLaunchKernelGGL(poseopt::k_pose_scatter, dim3(batch), dim3(256), 0, st, (const poseopt::ProblemDev*)A.problems, (const uint8_t*)s->d_dev, A.slot_bytes, A.o_idx,
                       f->slot_cap, d_pose_out, d_inliers, d_outlier, d_results);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int pose_set_camera_kb8(pose_solver* s, const OrbxKB8* cam) { return s ? s->camera.set(cam) : fail(ORBX_ERR_ARG, "NULL solver"); }
int pose_set_rig_kb8(pose_solver* s, const OrbxKB8Rig* rig) { return s ? s->camera.set(rig) : fail(ORBX_ERR_ARG, "NULL solver"); }

// diagnostic: the two device functions of camera_kb8.h on n points
int orbx_kb8_project(int device, const OrbxKB8* cam, const double* Xc, int n, double* uv, double* jac)
{
    if (!cam || n < 0 || (n > 0 && (!Xc || !uv))) return fail(ORBX_ERR_ARG, "bad arguments");
    if (!(cam->fx > 0) || !(cam->fy > 0)) return fail(ORBX_ERR_ARG, "KannalaBrandt8 focal lengths must be positive");
    if (int r = stage::check_device(device)) return r;
    if (n == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(device));
    kb8::Cam c;
    kb8::cam_from_abi(*cam, &c);
    double* d = nullptr;
    const size_t N = (size_t)n;
    ORBX_HIP(hipMalloc((void**)&d, 11 * N * sizeof(double)));          // [X 3n | uv 2n | jac 6n]
    hipError_t e = hipMemcpy(d, Xc, 3 * N * sizeof(double), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(poseopt::k_kb8_project, dim3((n + 255) / 256), dim3(256), 0, 0, c, (const double*)d, n, d + 3 * N, jac ? d + 5 * N : nullptr);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(uv, d + 3 * N, 2 * N * sizeof(double), hipMemcpyDeviceToHost);
    if (e == hipSuccess && jac) e = hipMemcpy(jac, d + 5 * N, 6 * N * sizeof(double), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(ORBX_ERR_HIP, "orbx_kb8_project: %s", hipGetErrorString(e));
    return ORBX_OK;
}

int pose_optimize(pose_solver* s, const PoseProblem* problem, PoseResult* result, uint8_t* outlier)
{
    uint8_t* outs[1] = {outlier};
    return pose_optimize_batch(s, problem, 1, result, outs);
}

}  // extern "C"
