// orbslam3_shim_fullba.hpp -- drop-in adapter for Optimizer::FullInertialBA (reference include/Optimizer.h, src/Optimizer.cc:392-811)
// on top of fiba_solve of orbslam3_hip_fullba.h:
//
//   void FullInertialBAHIP(Map*, int its, const bool bFixLocal = false, const unsigned long nLoopId = 0, bool* pbStopFlag = NULL,
//                          bool bInit = false, float priorG = 1e2, float priorA = 1e6)
//       LocalMapping::InitializeIMU, src/LocalMapping.cc:1311,1313; LoopClosing::RunGlobalBundleAdjustment, src/LoopClosing.cc:2290
//   (the reference's last two parameters, vSingVal and bHess, are read by nothing in the function)
//
// Like orbslam3_shim_imu_init.hpp it is written against the reference's own types, compiles inside an ORB-SLAM3 tree with
// ORBSLAM3_HIP_WITH_REFERENCE defined, and takes the map type as a template parameter so that the walk (FlattenFullInertialBA) and
// the write-back (fullba_detail::write_back) can be checked without a device on stand-in types (tests/test_shim_fullba.py).
// Opt = the class whose FullInertialBA serves what the device does not: a map with a second camera (mpCamera2), a link without a
// pre-integration or an observation by a key frame that has no vertex (the reference dereferences both), and whatever fiba_check
// refuses (ORBX_ERR_ARG, ORBX_ERR_CAPACITY).  Before that call only SetNewBias on the links' pre-integrations has happened, which
// the reference repeats with the same values.
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include <cmath>
#include <cstring>
#include <map>
#include <type_traits>

namespace ORB_SLAM3 {

// what the walk hands to the device, in the order the reference adds its vertices and edges
template <class KF, class MP>
struct FullBAFlat {
    std::vector<KF*> kfs;                               // key frames with mnId <= maxKFid, in GetAllKeyFrames() order
    std::vector<double> Rwb, twb, vel, bg, ba;          // [9] row-major / [3] per key frame
    std::vector<uint8_t> pose_fixed, has_imu, imu_fixed;
    std::vector<LibaLink> links;                        // one per EdgeInertial, in GetAllKeyFrames() order of its second key frame
    std::vector<MP*> mps;                               // GetAllMapPoints()
    std::vector<double> X;
    std::vector<bool> not_included;                     // vbNotIncludedMP: bAllFixed (:714-718)
    std::vector<int32_t> edge_kf, edge_point;           // in addEdge order
    std::vector<double> edge_obs, edge_w;
    std::vector<uint8_t> edge_stereo;
    KF* pIncKF = nullptr;                               // the last key frame visited with mnId <= maxKFid (:425)
    int nNonFixed = 0;
    bool camera2 = false, refused = false, too_few = false;
};

// The walk of :394-719.  too_few: bFixLocal with fewer than 3 non-fixed key frames (:468-472): the reference returns there, before
// any link is visited, and so does the walk.
template <class MapT, class KF, class MP>
void FlattenFullInertialBA(MapT* pMap, bool bFixLocal, FullBAFlat<KF, MP>& g)
{
    const long unsigned int maxKFid = pMap->GetMaxKFid();
    const std::vector<KF*> vpKFs = pMap->GetAllKeyFrames();
    const std::vector<MP*> vpMPs = pMap->GetAllMapPoints();
    for (KF* pKFi : vpKFs) if (pKFi->mpCamera2) g.camera2 = true;
    if (g.camera2) return;
    typedef typename std::remove_reference<decltype(vpMPs.front()->GetObservations())>::type ObsMap;
    typedef typename ObsMap::key_type ObsKF;                                        // the key-frame pointer type the observations hold
    std::map<ObsKF, int> index;
    for (KF* pKFi : vpKFs) {                                                        // :418-454
        if (pKFi->mnId > maxKFid) continue;
        index[static_cast<ObsKF>(pKFi)] = (int)g.kfs.size();
        g.kfs.push_back(pKFi);
        g.pIncKF = pKFi;
        bool bFixed = false;
        if (bFixLocal) {
            bFixed = (pKFi->mnBALocalForKF >= (maxKFid - 1)) || (pKFi->mnBAFixedForKF >= (maxKFid - 1));
            if (!bFixed) g.nNonFixed++;
        }
        const Eigen::Matrix3d R = pKFi->GetImuRotation().template cast<double>();
        const Eigen::Vector3d t = pKFi->GetImuPosition().template cast<double>();
        Eigen::Vector3d v, bgk, bak;
        for (int r = 0; r < 3; r++) { v[r] = 0; bgk[r] = 0; bak[r] = 0; }
        if (pKFi->bImu) { v = pKFi->GetVelocity().template cast<double>(); bgk = pKFi->GetGyroBias().template cast<double>(); bak = pKFi->GetAccBias().template cast<double>(); }
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) g.Rwb.push_back(R(r, c));
            g.twb.push_back(t[r]); g.vel.push_back(v[r]); g.bg.push_back(bgk[r]); g.ba.push_back(bak[r]);
        }
        g.pose_fixed.push_back(bFixed); g.imu_fixed.push_back(bFixed); g.has_imu.push_back(pKFi->bImu);
    }
    if (bFixLocal && g.nNonFixed < 3) { g.too_few = true; return; }
    for (KF* pKFi : vpKFs) {                                                        // :475-568
        if (!pKFi->mPrevKF) continue;
        if (pKFi->mnId > maxKFid) continue;
        if (pKFi->isBad() || pKFi->mPrevKF->mnId > maxKFid) continue;
        if (!(pKFi->bImu && pKFi->mPrevKF->bImu)) continue;
        if (!pKFi->mpImuPreintegrated) { g.refused = true; continue; }
        auto* pInt = pKFi->mpImuPreintegrated;
        pInt->SetNewBias(pKFi->mPrevKF->GetImuBias());                              // :491 (before the vertex lookup)
        const auto i1 = index.find(static_cast<ObsKF>(pKFi->mPrevKF)), i2 = index.find(static_cast<ObsKF>(pKFi));
        if (i1 == index.end() || i2 == index.end()) continue;                       // optimizer.vertex() == NULL: "Error", no edge
        g.links.push_back(orbslam3_hip::imu_link(pInt, i1->second, i2->second, 1.0, pInt, true));    // no factor 1e-2 in this function; Huber :540-542;
                                                                                                    // the random-walk informations :551, :559 are read without bInit only
    }
    g.not_included.assign(vpMPs.size(), false);
    for (size_t i = 0; i < vpMPs.size(); i++) {                                     // :599-719
        MP* pMP = vpMPs[i];
        g.mps.push_back(pMP);
        const Eigen::Vector3d Xd = pMP->GetWorldPos().template cast<double>();
        for (int r = 0; r < 3; r++) g.X.push_back(Xd[r]);
        bool bAllFixed = true;
        const ObsMap observations = pMP->GetObservations();
        for (const auto& obs : observations) {
            auto* pKFi = obs.first;
            if (pKFi->mnId > maxKFid) continue;
            if (pKFi->isBad()) continue;
            const int leftIndex = std::get<0>(obs.second);
            if (leftIndex == -1) continue;
            const auto it = index.find(pKFi);
            if (it == index.end()) { g.refused = true; continue; }                  // (the reference dereferences the missing vertex)
            if (!g.pose_fixed[it->second]) bAllFixed = false;
            const cv::KeyPoint& kpUn = pKFi->mvKeysUn[leftIndex];
            const float ur = pKFi->mvuRight[leftIndex];
            g.edge_kf.push_back(it->second); g.edge_point.push_back((int32_t)i);
            orbslam3_hip::push_edge_obs(kpUn, ur, g.edge_obs, g.edge_stereo);
            g.edge_w.push_back((double)pKFi->mvInvLevelSigma2[kpUn.octave]);       // (no uncertainty2 in this function)
        }
        if (bAllFixed) g.not_included[i] = true;
    }
}

namespace fullba_detail {

template <class KF, class MP>
inline void fill(const FullBAFlat<KF, MP>& g, int its, bool* pbStopFlag, bool bInit, float priorG, float priorA, FibaProblem& p)
{
    std::memset(&p, 0, sizeof(p));
    KF* k0 = g.pIncKF;
    p.n_kf = (int32_t)g.kfs.size();
    p.Rwb = g.Rwb.data(); p.twb = g.twb.data(); p.vel = g.vel.data(); p.bg = g.bg.data(); p.ba = g.ba.data();
    p.pose_fixed = g.pose_fixed.data(); p.has_imu = g.has_imu.data(); p.imu_fixed = g.imu_fixed.data();
    orbslam3_hip::imu_calib(k0->mImuCalib, p.Rcb, p.tcb, p.tbc);
    p.fx = k0->fx; p.fy = k0->fy; p.cx = k0->cx; p.cy = k0->cy; p.bf = k0->mbf;
    p.n_points = (int32_t)g.mps.size(); p.points = g.X.data();
    p.n_edges = (int32_t)g.edge_kf.size(); p.edge_kf = g.edge_kf.data(); p.edge_point = g.edge_point.data(); p.edge_obs = g.edge_obs.data();
    p.edge_inv_sigma2 = g.edge_w.data(); p.edge_stereo = g.edge_stereo.data();
    p.n_links = (int32_t)g.links.size(); p.links = g.links.data();
    p.huber_mono = orbslam3_hip::huber_mono(); p.huber_stereo = orbslam3_hip::huber_stereo(); p.huber_inertial = std::sqrt(16.92);   // :592-593
    p.lambda_init = 1e-5; p.max_iters = its;                                        // :407, :727
    p.shared_bias = bInit;
    if (bInit) {                                                                    // :456-466, :570-590
        const Eigen::Vector3d sg = k0->GetGyroBias().template cast<double>(), sa = k0->GetAccBias().template cast<double>();
        for (int r = 0; r < 3; r++) { p.shared_bg[r] = sg[r]; p.shared_ba[r] = sa[r]; }
        p.prior_g = priorG; p.prior_a = priorA;
    }
    p.stop_flag = reinterpret_cast<const volatile uint8_t*>(pbStopFlag);
}

// :730-810; p: the problem of g, for its camera-body calibration
template <class MapT, class KF, class MP>
inline void write_back(MapT* pMap, const FullBAFlat<KF, MP>& g, const FibaProblem& p, unsigned long nLoopId, const double* Ro, const double* to, const double* vo,
                       const double* go, const double* ao, const double* Xo)
{
    for (size_t i = 0; i < g.kfs.size(); i++) {
        KF* pKFi = g.kfs[i];
        const Sophus::SE3f Tcw = orbslam3_hip::camera_pose(p.Rcb, p.tcb, &Ro[9 * i], &to[3 * i]);
        if (nLoopId == 0) pKFi->SetPose(Tcw);
        else { pKFi->mTcwGBA = Tcw; pKFi->mnBAGlobalForKF = nLoopId; }
        if (!pKFi->bImu) continue;
        const Eigen::Vector3d Vw(vo[3 * i], vo[3 * i + 1], vo[3 * i + 2]);
        const IMU::Bias b(ao[3 * i], ao[3 * i + 1], ao[3 * i + 2], go[3 * i], go[3 * i + 1], go[3 * i + 2]);
        if (nLoopId == 0) { pKFi->SetVelocity(Vw.template cast<float>()); pKFi->SetNewBias(b); }
        else { pKFi->mVwbGBA = Vw.template cast<float>(); pKFi->mBiasGBA = b; }
    }
    for (size_t i = 0; i < g.mps.size(); i++) {
        if (g.not_included[i]) continue;
        MP* pMP = g.mps[i];
        const Eigen::Vector3d Xd(Xo[3 * i], Xo[3 * i + 1], Xo[3 * i + 2]);
        if (nLoopId == 0) { pMP->SetWorldPos(Xd.template cast<float>()); pMP->UpdateNormalAndDepth(); }
        else { pMP->mPosGBA = Xd.template cast<float>(); pMP->mnBAGlobalForKF = nLoopId; }
    }
    pMap->IncreaseChangeIndex();
}

}  // namespace fullba_detail

// void Optimizer::FullInertialBA(Map*, int its, const bool bFixLocal, const long unsigned int nLoopId, bool* pbStopFlag, bool bInit,
//                                float priorG, float priorA, Eigen::VectorXd* vSingVal, bool* bHess)                                 :392
template <class Opt = Optimizer, class MapT>
void FullInertialBAHIP(MapT* pMap, int its, const bool bFixLocal = false, const long unsigned int nLoopId = 0, bool* pbStopFlag = NULL, bool bInit = false,
                       float priorG = 1e2, float priorA = 1e6)
{
    typedef typename std::remove_pointer<typename decltype(pMap->GetAllKeyFrames())::value_type>::type KF;
    typedef typename std::remove_pointer<typename decltype(pMap->GetAllMapPoints())::value_type>::type MP;
    FullBAFlat<KF, MP> g;
    FlattenFullInertialBA(pMap, bFixLocal, g);
    if (g.too_few) return;                                                          // :468-472
    FibaProblem p;
    bool device = !g.camera2 && !g.refused && g.pIncKF;
    if (device) {
        fullba_detail::fill(g, its, pbStopFlag, bInit, priorG, priorA, p);
        const int ok = fiba_check(&p);                                              // before a handle (and with it a device) is asked for
        device = ok != ORBX_ERR_ARG && ok != ORBX_ERR_CAPACITY;
    }
    if (!device) { Opt::FullInertialBA(pMap, its, bFixLocal, nLoopId, pbStopFlag, bInit, priorG, priorA); return; }
    if (pbStopFlag && *pbStopFlag) return;                                          // :721-723: nothing is written
    std::vector<double> Ro(g.Rwb.size()), to(g.twb.size()), vo(g.vel.size()), go(g.bg.size()), ao(g.ba.size()), Xo(g.X.size() + 3);
    FibaOutputs o;
    o.Rwb = Ro.data(); o.twb = to.data(); o.vel = vo.data(); o.bg = go.data(); o.ba = ao.data(); o.points = Xo.data();
    LbaStats st;
    orbslam3_hip::check(fiba_solve(orbslam3_hip::thread_handle<fiba_solver, fiba_create>(), &p, &o, &st));
    fullba_detail::write_back(pMap, g, p, nLoopId, Ro.data(), to.data(), vo.data(), go.data(), ao.data(), Xo.data());
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
