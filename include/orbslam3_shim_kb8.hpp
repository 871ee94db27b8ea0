// orbslam3_shim_kb8.hpp -- drop-in adapters that add the monocular KannalaBrandt8 (fisheye) camera to the two visual optimisers:
//
//   int  PoseOptimizationAnyCamHIP(Frame*)                                              Optimizer::PoseOptimization, src/Optimizer.cc:814-1115
//   void LocalBundleAdjustmentAnyCamHIP(KeyFrame*, bool*, Map*, int&, int&, int&, int&) Optimizer::LocalBundleAdjustment, :1116-1498
//
// Device KB8 path: the frame -- or every key frame of the window, fixed cameras included -- has no mpCamera2 and one CAM_FISHEYE
// camera, with identical eight parameters across the window, and no observation with mvuRight >= 0 (the device's KB8 edges are
// monocular).  The adapter sets that camera on its solver handle
// (pose_set_camera_kb8 / lba_set_camera_kb8 of orbslam3_hip_kb8.h), runs the graph walk and the write-back of the pinhole adapters,
// and resets the camera.  Anything else goes to PoseOptimizationHIP / LocalBundleAdjustmentHIP of orbslam3_shim.hpp, which keep
// their own fallback to the reference (stereo-fisheye rigs with mpCamera2 end there).
// The walk of the window is LocalBundleAdjustmentGraph of orbslam3_shim.hpp itself; what is REPEATED here from the pinhole adapters,
// because they do it inside one function with their own solver handle, is the flattening of a frame's edges, the marshalling
// of the problem and the write-back.  The handles of this header are its own (one per thread).
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include "CameraModels/KannalaBrandt8.h"

namespace ORB_SLAM3 {

namespace kb8_detail {

// the eight parameters of a CAM_FISHEYE camera (mvParameters: fx fy cx cy k0 k1 k2 k3, floats) promoted to double; false for
// any other camera.  (getParameter is GeometricCamera's in the reference; the call goes through the derived class because the
// stand-in base class that the typed tests compile against does not have it, and a CAM_FISHEYE camera is a KannalaBrandt8.)
inline bool camera_of(GeometricCamera* pCamera, OrbxKB8& out)
{
    if (!pCamera || pCamera->GetType() != GeometricCamera::CAM_FISHEYE) return false;
    KannalaBrandt8* kb = static_cast<KannalaBrandt8*>(pCamera);
    out.fx = kb->getParameter(0); out.fy = kb->getParameter(1); out.cx = kb->getParameter(2); out.cy = kb->getParameter(3);
    for (int k = 0; k < 4; k++) out.k[k] = kb->getParameter(4 + k);
    return true;
}

inline bool same(const OrbxKB8& a, const OrbxKB8& b)
{
    return a.fx == b.fx && a.fy == b.fy && a.cx == b.cx && a.cy == b.cy && a.k[0] == b.k[0] && a.k[1] == b.k[1] && a.k[2] == b.k[2] && a.k[3] == b.k[3];
}

template <class KF>
inline bool is_mono_kb8(KF* p, const OrbxKB8* like, OrbxKB8& out)
{
    return !p->mpCamera2 && camera_of(p->mpCamera, out) && (!like || same(*like, out));
}

// sets the camera on a handle for the lifetime of the object; the reset must happen on every way out (check() throws)
template <class Handle, int (*Set)(Handle*, const OrbxKB8*)>
struct CameraScope {
    Handle* h;
    CameraScope(Handle* h_, const OrbxKB8& cam) : h(h_) { orbslam3_hip::check(Set(h, &cam)); }
    ~CameraScope() { (void)Set(h, nullptr); }
    CameraScope(const CameraScope&) = delete;
    CameraScope& operator=(const CameraScope&) = delete;
};

}  // namespace kb8_detail

inline int PoseOptimizationAnyCamHIP(Frame* pFrame)
{
    OrbxKB8 cam;
    bool kb8 = kb8_detail::is_mono_kb8(pFrame, nullptr, cam);
    for (int i = 0; kb8 && i < pFrame->N; i++)
        if (pFrame->mvpMapPoints[i] && pFrame->mvuRight[i] >= 0) kb8 = false;      // a stereo observation: not a monocular frame
    if (!kb8) return PoseOptimizationHIP(pFrame);
    // ---- as PoseOptimizationHIP: one edge per feature holding a MapPoint, in feature order; a monocular frame has mvuRight < 0 ----
    const int N = pFrame->N;
    std::vector<double> Xw, obs, w;
    std::vector<uint8_t> stereo;
    std::vector<int> feat;
    {
        std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);                  // :857
        for (int i = 0; i < N; i++) {
            MapPoint* pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            pFrame->mvbOutlier[i] = false;
            const cv::KeyPoint& kpUn = pFrame->mvKeysUn[i];
            const Eigen::Vector3d X = pMP->GetWorldPos().cast<double>();
            Xw.push_back(X.x()); Xw.push_back(X.y()); Xw.push_back(X.z());
            obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y); obs.push_back(-1.0);
            w.push_back((double)pFrame->mvInvLevelSigma2[kpUn.octave]);
            stereo.push_back(0);
            feat.push_back(i);
        }
    }
    PoseProblem pr;
    const Sophus::SE3<float> Tcw = pFrame->GetPose();
    const Eigen::Quaterniond qd = Tcw.unit_quaternion().cast<double>();
    const Eigen::Vector3d td = Tcw.translation().cast<double>();
    pr.q[0] = qd.x(); pr.q[1] = qd.y(); pr.q[2] = qd.z(); pr.q[3] = qd.w();
    pr.t[0] = td.x(); pr.t[1] = td.y(); pr.t[2] = td.z();
    pr.n = (int)feat.size(); pr.Xw = Xw.data(); pr.obs = obs.data(); pr.inv_sigma2 = w.data(); pr.stereo = stereo.data();
    pr.fx = cam.fx; pr.fy = cam.fy; pr.cx = cam.cx; pr.cy = cam.cy; pr.bf = 0.0;   // not read while the KB8 camera is set
    const float deltaMono = sqrt(5.991), deltaStereo = sqrt(7.815);                 // :838-839 (through float)
    pr.huber_mono = deltaMono; pr.huber_stereo = deltaStereo;
    static thread_local pose_solver* solver = nullptr;
    if (!solver) orbslam3_hip::check(pose_create(0, &solver));
    PoseResult res;
    std::vector<uint8_t> outlier(feat.size() + 1);
    {
        kb8_detail::CameraScope<pose_solver, pose_set_camera_kb8> scope(solver, cam);
        orbslam3_hip::check(pose_optimize(solver, &pr, &res, outlier.data()));
    }
    if (pr.n < 3) return 0;                                                         // :998-999 (pose untouched)
    for (size_t k = 0; k < feat.size(); k++) pFrame->mvbOutlier[feat[k]] = outlier[k] != 0;
    const Eigen::Quaterniond qo(res.q[3], res.q[0], res.q[1], res.q[2]);
    pFrame->SetPose(Sophus::SE3f(qo.cast<float>(), Eigen::Vector3d(res.t[0], res.t[1], res.t[2]).cast<float>()));   // :1107-1110
    return res.inliers;
}

inline void LocalBundleAdjustmentAnyCamHIP(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges)
{
    OrbxKB8 cam, other;
    bool kb8 = kb8_detail::is_mono_kb8(pKF, nullptr, cam);
    if (kb8)
        for (KeyFrame* pKFi : pKF->GetVectorCovisibleKeyFrames())
            if (!kb8_detail::is_mono_kb8(pKFi, &cam, other)) { kb8 = false; break; }
    if (!kb8) { LocalBundleAdjustmentHIP(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges); return; }
    LbaGraph g;
    const bool ok = LocalBundleAdjustmentGraph(pKF, pMap, g);
    // the fixed cameras only turn up in the walk (LocalBundleAdjustmentHIP says what the walk has touched by then, and why that is harmless)
    // and so do the observations: one with mvuRight >= 0 would be a stereo edge, which the device refuses for a KB8 camera
    for (KeyFrame* pKFi : g.kfs) kb8 = kb8 && kb8_detail::is_mono_kb8(pKFi, &cam, other);
    for (uint8_t st : g.eStereo) kb8 = kb8 && !st;
    if (!kb8) { LocalBundleAdjustmentHIP(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges); return; }
    (void)num_MPs;
    num_fixedKF = g.num_fixedKF;
    if (!ok) return;                                                                // :1182-1186
    num_OptKF = g.num_OptKF; num_edges = g.num_edges;
    if (pbStopFlag && *pbStopFlag) return;                                          // :1406-1408

    // ---- as LocalBundleAdjustmentHIP from here on, with the camera set around the solve ----
    LbaProblem pr;
    pr.n_poses = (int)g.kfs.size(); pr.pose_q = g.q.data(); pr.pose_t = g.t.data(); pr.pose_fixed = g.fixed.data();
    pr.n_points = (int)g.mps.size(); pr.points = g.X.data();
    pr.n_edges = num_edges; pr.edge_point = g.ePoint.data(); pr.edge_pose = g.ePose.data(); pr.edge_obs = g.eObs.data();
    pr.edge_inv_sigma2 = g.eW.data(); pr.edge_stereo = g.eStereo.data();
    pr.fx = cam.fx; pr.fy = cam.fy; pr.cx = cam.cx; pr.cy = cam.cy; pr.bf = 0.0;   // not read while the KB8 camera is set
    const float thHuberMono = sqrt(5.991), thHuberStereo = sqrt(7.815);             // :1275-1276 (through float)
    pr.huber_mono = thHuberMono; pr.huber_stereo = thHuberStereo;
    static thread_local lba_solver* solver = nullptr;
    if (!solver) orbslam3_hip::check(lba_create(0, &solver));
    std::vector<double> qo(g.q.size()), to(g.t.size()), Xo(g.X.size()), chi2(num_edges);
    std::vector<uint8_t> depthPos(num_edges);
    LbaStats st;
    {
        kb8_detail::CameraScope<lba_solver, lba_set_camera_kb8> scope(solver, cam);
        orbslam3_hip::check(lba_solve(solver, &pr, (const volatile uint8_t*)pbStopFlag, 10, pMap->IsInertial() ? 100.0 : 0.0,
                                      qo.data(), to.data(), Xo.data(), chi2.data(), depthPos.data(), &st));
    }
    std::vector<std::pair<KeyFrame*, MapPoint*> > vToErase;                         // :1413-1460 (monocular edges: 5.991)
    for (int e = 0; e < num_edges; e++) {
        if (g.eMP[e]->isBad()) continue;
        if (chi2[e] > 5.991 || !depthPos[e]) vToErase.push_back(std::make_pair(g.eKF[e], g.eMP[e]));
    }
    std::unique_lock<std::mutex> lock(pMap->mMutexMapUpdate);                       // :1464
    for (auto& er : vToErase) { er.first->EraseMapPointMatch(er.second); er.second->EraseObservation(er.first); }
    for (KeyFrame* pKFi : g.lLocalKeyFrames) {
        const int i = g.kfIndex.at(pKFi);
        const Eigen::Quaterniond qd(qo[4 * i + 3], qo[4 * i], qo[4 * i + 1], qo[4 * i + 2]);
        pKFi->SetPose(Sophus::SE3f(qd.cast<float>(), Eigen::Vector3d(to[3 * i], to[3 * i + 1], to[3 * i + 2]).cast<float>()));
    }
    for (MapPoint* pMP : g.lLocalMapPoints) {
        const int i = g.mpIndex.at(pMP);
        pMP->SetWorldPos(Eigen::Vector3d(Xo[3 * i], Xo[3 * i + 1], Xo[3 * i + 2]).cast<float>());
        pMP->UpdateNormalAndDepth();
    }
    pMap->IncreaseChangeIndex();
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
