// orbslam3_shim_imu_init.hpp -- drop-in adapters for the three Optimizer::InertialOptimization overloads (reference
// include/Optimizer.h, src/Optimizer.cc:3042, :3227, :3389) on top of imu_init_optimize_batch of orbslam3_hip_imu_init.h:
//
//   void InertialOptimizationHIP(Map*, Eigen::Matrix3d& Rwg, double& scale, Eigen::Vector3d& bg, Eigen::Vector3d& ba, bool bMono,
//                                Eigen::MatrixXd& covInertial, bool bFixedVel = false, bool bGauss = false,
//                                float priorG = 1e2, float priorA = 1e6)          LocalMapping::InitializeIMU, src/LocalMapping.cc:1271
//   void InertialOptimizationHIP(Map*, Eigen::Vector3d& bg, Eigen::Vector3d& ba, float priorG = 1e2, float priorA = 1e6)
//                                                                                 LoopClosing::MergeLocal2, src/LoopClosing.cc:1867
//   void InertialOptimizationHIP(Map*, Eigen::Matrix3d& Rwg, double& scale)       LocalMapping::ScaleRefinement, src/LocalMapping.cc:1465
//
// Like orbslam3_shim.hpp (which it includes) it is written against the reference's own types and compiles inside an ORB-SLAM3
// tree with ORBSLAM3_HIP_WITH_REFERENCE defined.  The walk over the map (FlattenInertialOptimization) and the write-back
// (imu_init_detail::write_back) are host code and are checked without a device by tests/test_shim_imu_init.py on stand-in types,
// which is why the map type is a template parameter.  Opt = the class whose InertialOptimization serves what the device does
// not: input imu_init_check refuses (ORBX_ERR_ARG: a key frame without pre-integration, links that are no disjoint paths, a value
// that is not finite) and maps of more than IMU_INIT_MAX_KF key frames (ORBX_ERR_CAPACITY).  Nothing is written before that call.
// covInertial is not touched: the reference does not touch it either.
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include <cstring>
#include <map>
#include <type_traits>

namespace ORB_SLAM3 {

// what the walk hands to the device, in the order the reference adds its vertices and edges
template <class KF>
struct ImuInitFlat {
    std::vector<KF*> kfs;                   // key frames with mnId <= maxKFid, in GetAllKeyFrames() order
    std::vector<double> Rwb, twb, vel;      // [9] row-major / [3] / [3] per key frame
    std::vector<LibaLink> links;            // one per EdgeInertialGS, in GetAllKeyFrames() order of its second key frame
    double bg[3], ba[3];                    // VertexGyroBias / VertexAccBias(vpKFs.front())
    bool refused = false;                   // a link's key frame has no mpImuPreintegrated: the reference dereferences it
};

// The walk of :3064-3176 (:3245-3350, :3405-3478 are the same walk): set_new_bias = the SetNewBias(mPrevKF->GetImuBias()) of the
// first two overloads, robust = the Huber kernel of the third.
template <class MapT, class KF>
void FlattenInertialOptimization(MapT* pMap, ImuInitFlat<KF>& g, bool set_new_bias, bool robust)
{
    const long unsigned int maxKFid = pMap->GetMaxKFid();
    const std::vector<KF*> vpKFs = pMap->GetAllKeyFrames();
    std::map<KF*, int> index;
    for (KF* pKFi : vpKFs) {
        if (pKFi->mnId > maxKFid) continue;
        index[pKFi] = (int)g.kfs.size();
        g.kfs.push_back(pKFi);
        const Eigen::Matrix3d R = pKFi->GetImuRotation().template cast<double>();
        const Eigen::Vector3d t = pKFi->GetImuPosition().template cast<double>(), v = pKFi->GetVelocity().template cast<double>();
        for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) g.Rwb.push_back(R(r, c)); g.twb.push_back(t[r]); g.vel.push_back(v[r]); }
    }
    for (int k = 0; k < 3; k++) { g.bg[k] = 0; g.ba[k] = 0; }
    if (!vpKFs.empty()) {
        const Eigen::Vector3d b_g = vpKFs.front()->GetGyroBias().template cast<double>(), b_a = vpKFs.front()->GetAccBias().template cast<double>();
        for (int k = 0; k < 3; k++) { g.bg[k] = b_g[k]; g.ba[k] = b_a[k]; }
    }
    for (KF* pKFi : vpKFs) {
        if (!pKFi->mPrevKF || pKFi->mnId > maxKFid) continue;
        if (pKFi->isBad() || pKFi->mPrevKF->mnId > maxKFid) continue;
        const auto i1 = index.find(pKFi->mPrevKF), i2 = index.find(pKFi);
        if (!pKFi->mpImuPreintegrated) { g.refused = true; continue; }
        auto* pInt = pKFi->mpImuPreintegrated;
        if (set_new_bias) pInt->SetNewBias(pKFi->mPrevKF->GetImuBias());                    // :3145 (before the vertex lookup)
        if (i1 == index.end() || i2 == index.end()) continue;                               // optimizer.vertex() == NULL: "Error", no edge
        g.links.push_back(orbslam3_hip::imu_link(pInt, i1->second, i2->second, 1.0, nullptr, robust));   // EdgeInertialGS: no factor 1e-2, no random-walk edges
    }
}

namespace imu_init_detail {

struct Settings {
    bool free_vel, free_bias, free_gdir, free_scale, gauss_newton;
    double prior_g, prior_a, huber_delta, lambda_init;
    int max_iters;
};

// the problem of a flattened map; vel_out: room for the velocities
template <class KF>
inline void fill(const ImuInitFlat<KF>& g, const Settings& s, const double* Rwg, double scale, std::vector<double>& vel_out, ImuInitProblem& p, ImuInitResult& r)
{
    std::memset(&p, 0, sizeof(p));
    std::memset(&r, 0, sizeof(r));
    p.n_kf = (int32_t)g.kfs.size();
    p.Rwb = g.Rwb.data(); p.twb = g.twb.data(); p.vel = g.vel.data();
    for (int k = 0; k < 3; k++) { p.bg[k] = g.bg[k]; p.ba[k] = g.ba[k]; }
    for (int k = 0; k < 9; k++) p.Rwg[k] = Rwg[k];
    p.scale = scale;
    p.n_links = (int32_t)g.links.size(); p.links = g.links.data();
    p.free_vel = s.free_vel; p.free_bias = s.free_bias; p.free_gdir = s.free_gdir; p.free_scale = s.free_scale;
    p.prior_g = s.prior_g; p.prior_a = s.prior_a; p.huber_delta = s.huber_delta; p.gauss_newton = s.gauss_newton;
    p.lambda_init = s.lambda_init; p.max_iters = s.max_iters;
    vel_out.assign(g.vel.size() + 3, 0.0);
    r.vel_out = vel_out.data();
}

// imu_init_optimize_batch on a flattened map; false when the device refuses it: the caller falls back
template <class KF>
inline bool run(const ImuInitFlat<KF>& g, const Settings& s, const double* Rwg, double scale, std::vector<double>& vel_out, ImuInitResult& r)
{
    if (g.refused) return false;
    ImuInitProblem p;
    fill(g, s, Rwg, scale, vel_out, p, r);
    const int ok = imu_init_check(&p, &r);              // before a handle (and with it a device) is asked for
    if (ok == ORBX_ERR_ARG || ok == ORBX_ERR_CAPACITY) return false;
    orbslam3_hip::check(imu_init_optimize_batch(orbslam3_hip::thread_handle<imu_init_solver, imu_init_create>(), &p, 1, &r));
    return true;
}

// :3201-3223 (:3368-3386): velocities, then the new bias, with a re-integration where the gyro bias moved by more than 0.01
template <class KF>
inline void write_back(const ImuInitFlat<KF>& g, const double* vel_out, const Eigen::Vector3d& bg, const Eigen::Vector3d& ba)
{
    const IMU::Bias b(ba[0], ba[1], ba[2], bg[0], bg[1], bg[2]);
    for (size_t k = 0; k < g.kfs.size(); k++) {
        KF* pKFi = g.kfs[k];
        const Eigen::Vector3d Vw(vel_out[3 * k], vel_out[3 * k + 1], vel_out[3 * k + 2]);
        pKFi->SetVelocity(Vw.template cast<float>());
        if ((pKFi->GetGyroBias() - bg.template cast<float>()).norm() > 0.01) {
            pKFi->SetNewBias(b);
            if (pKFi->mpImuPreintegrated) pKFi->mpImuPreintegrated->Reintegrate();
        } else
            pKFi->SetNewBias(b);
    }
}

inline void rwg_in(const Eigen::Matrix3d& Rwg, double* out) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) out[3 * r + c] = Rwg(r, c); }
inline void rwg_out(const double* in, Eigen::Matrix3d& Rwg) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) Rwg(r, c) = in[3 * r + c]; }

}  // namespace imu_init_detail

// void Optimizer::InertialOptimization(Map*, Eigen::Matrix3d& Rwg, double& scale, Eigen::Vector3d& bg, Eigen::Vector3d& ba, bool bMono,
//                                      Eigen::MatrixXd& covInertial, bool bFixedVel, bool bGauss, float priorG, float priorA)     :3042
template <class Opt = Optimizer, class MapT>
void InertialOptimizationHIP(MapT* pMap, Eigen::Matrix3d& Rwg, double& scale, Eigen::Vector3d& bg, Eigen::Vector3d& ba, bool bMono,
                             Eigen::MatrixXd& covInertial, bool bFixedVel = false, bool bGauss = false, float priorG = 1e2, float priorA = 1e6)
{
    typedef typename std::remove_pointer<typename decltype(pMap->GetAllKeyFrames())::value_type>::type KF;
    ImuInitFlat<KF> g;
    FlattenInertialOptimization(pMap, g, true, false);
    imu_init_detail::Settings s;
    s.free_vel = !bFixedVel; s.free_bias = !bFixedVel; s.free_gdir = true; s.free_scale = bMono; s.gauss_newton = false;   // (bGauss is not read, :3057)
    s.prior_g = priorG; s.prior_a = priorA; s.huber_delta = 0.0;
    s.lambda_init = priorG != 0.f ? 1e3 : 0.0;                                             // :3059-3060
    s.max_iters = 200;
    double R[9];
    imu_init_detail::rwg_in(Rwg, R);
    std::vector<double> vel_out;
    ImuInitResult r;
    if (!imu_init_detail::run(g, s, R, scale, vel_out, r)) {
        Opt::InertialOptimization(pMap, Rwg, scale, bg, ba, bMono, covInertial, bFixedVel, bGauss, priorG, priorA);
        return;
    }
    scale = r.scale_out;                                                                    // :3185-3199
    for (int k = 0; k < 3; k++) { bg[k] = r.bg_out[k]; ba[k] = r.ba_out[k]; }
    imu_init_detail::rwg_out(r.Rwg_out, Rwg);
    imu_init_detail::write_back(g, vel_out.data(), bg, ba);
}

// void Optimizer::InertialOptimization(Map*, Eigen::Vector3d& bg, Eigen::Vector3d& ba, float priorG, float priorA)                  :3227
template <class Opt = Optimizer, class MapT>
void InertialOptimizationHIP(MapT* pMap, Eigen::Vector3d& bg, Eigen::Vector3d& ba, float priorG = 1e2, float priorA = 1e6)
{
    typedef typename std::remove_pointer<typename decltype(pMap->GetAllKeyFrames())::value_type>::type KF;
    ImuInitFlat<KF> g;
    FlattenInertialOptimization(pMap, g, true, false);
    imu_init_detail::Settings s;
    s.free_vel = true; s.free_bias = true; s.free_gdir = false; s.free_scale = false; s.gauss_newton = false;
    s.prior_g = priorG; s.prior_a = priorA; s.huber_delta = 0.0;
    s.lambda_init = 1e3;                                                                    // :3243
    s.max_iters = 200;
    const double I[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
    std::vector<double> vel_out;
    ImuInitResult r;
    if (!imu_init_detail::run(g, s, I, 1.0, vel_out, r)) {
        Opt::InertialOptimization(pMap, bg, ba, priorG, priorA);
        return;
    }
    for (int k = 0; k < 3; k++) { bg[k] = r.bg_out[k]; ba[k] = r.ba_out[k]; }
    imu_init_detail::write_back(g, vel_out.data(), bg, ba);
}

// void Optimizer::InertialOptimization(Map*, Eigen::Matrix3d& Rwg, double& scale)                                                   :3389
template <class Opt = Optimizer, class MapT>
void InertialOptimizationHIP(MapT* pMap, Eigen::Matrix3d& Rwg, double& scale)
{
    typedef typename std::remove_pointer<typename decltype(pMap->GetAllKeyFrames())::value_type>::type KF;
    ImuInitFlat<KF> g;
    FlattenInertialOptimization(pMap, g, false, true);                                      // no SetNewBias here; Huber 1 on every link (:3468-3470)
    imu_init_detail::Settings s;
    s.free_vel = false; s.free_bias = false; s.free_gdir = true; s.free_scale = true; s.gauss_newton = true;
    s.prior_g = 0.0; s.prior_a = 0.0; s.huber_delta = 1.0; s.lambda_init = 0.0;
    s.max_iters = 10;
    double R[9];
    imu_init_detail::rwg_in(Rwg, R);
    std::vector<double> vel_out;
    ImuInitResult r;
    if (!imu_init_detail::run(g, s, R, scale, vel_out, r)) {
        Opt::InertialOptimization(pMap, Rwg, scale);
        return;
    }
    scale = r.scale_out;                                                                    // :3484-3485: nothing else is written
    imu_init_detail::rwg_out(r.Rwg_out, Rwg);
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
