// orbslam3_shim_rig.hpp -- drop-in adapters that add the two-camera KannalaBrandt8 rig (mpCamera, mpCamera2, GetRelativePoseTrl) to the
// two visual optimisers:
//
//   int  PoseOptimizationRigHIP(Frame*)                                              Optimizer::PoseOptimization, src/Optimizer.cc:814-1115
//   void LocalBundleAdjustmentRigHIP(KeyFrame*, bool*, Map*, int&, int&, int&, int&) Optimizer::LocalBundleAdjustment, :1116-1498
//
// Device rig path: the frame -- or every key frame of the window, fixed cameras included -- has two CAM_FISHEYE cameras, with the
// same sixteen parameters and the same GetRelativePoseTrl() across the window, and no edge-bearing observation with mvuRight >= 0.
// The rig is then set on this thread's solver handle around the solve (pose_set_rig_kb8 / lba_set_rig_kb8 of orbslam3_hip_kb8.h) and
// reset after it.  Anything else goes to PoseOptimizationAnyCamHIP / LocalBundleAdjustmentAnyCamHIP of orbslam3_shim_kb8.hpp, which keep
// their own routing.
// The edges follow the reference.  PoseOptimization (:929-991): feature i < Nleft is a left edge from mvKeys[i] (not mvKeysUn), feature
// i >= Nleft a right edge from mvKeysRight[i - Nleft]; one mvbOutlier[i] per edge, written back over both lists.
// LocalBundleAdjustment (:1296-1400), per observation: a left edge if leftIndex != -1 (from mvKeysUn[leftIndex]), then a right edge if
// rightIndex != -1 (from mvKeysRight[rightIndex - NLeft], with that key point's octave); the erase pass (:1417-1445) runs over the
// left edges, then the right ones, so a (key frame, point) pair may be erased twice, as in the reference.
// The walk of the window, the problems, the solves and the write-backs are the pinhole adapters' own steps in orbslam3_shim.hpp
// (LocalBundleAdjustmentGraph with this header's edge function, LocalBundleAdjustmentFinish, PoseOptimizationSolve /
// PoseOptimizationWriteBack); the handles are theirs too (thread_handle), which is how the rig set here reaches their solve.
// The frame and key-frame types are template parameters (Frame and KeyFrame in the reference tree, which have the rig members
// themselves; derived stand-ins in the typed tests): the rig members are reached through a static_cast to them.
#pragma once

#include "orbslam3_shim_kb8.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

namespace ORB_SLAM3 {

namespace rig_detail {

inline bool same(const OrbxKB8Rig& a, const OrbxKB8Rig& b)
{
    bool eq = kb8_detail::same(a.left, b.left) && kb8_detail::same(a.right, b.right);
    for (int k = 0; k < 4; k++) eq = eq && a.q_rl[k] == b.q_rl[k];
    for (int k = 0; k < 3; k++) eq = eq && a.t_rl[k] == b.t_rl[k];
    return eq;
}

// the rig of a frame or key frame with two CAM_FISHEYE cameras; false for anything else
template <class Fisheye, class T>
inline bool rig_of(T* p, const OrbxKB8Rig* like, OrbxKB8Rig& out)
{
    OrbxKB8 l, r;
    if (!kb8_detail::camera_of(p->mpCamera, l) || !kb8_detail::camera_of(p->mpCamera2, r)) return false;
    out = orbslam3_hip::kb8_rig_in(static_cast<Fisheye*>(p->mpCamera), static_cast<Fisheye*>(p->mpCamera2), p->GetRelativePoseTrl());
    return !like || same(*like, out);
}

inline void push_right_obs(const cv::KeyPoint& kp, std::vector<double>& obs, std::vector<uint8_t>& kind)
{
    obs.push_back(kp.pt.x); obs.push_back(kp.pt.y); obs.push_back(-1.0);
    kind.push_back(ORBX_EDGE_RIGHT);
}

}  // namespace rig_detail

template <class Fisheye = KannalaBrandt8, class FrameT = Frame>
inline int PoseOptimizationRigHIP(Frame* pFrame_)
{
    FrameT* pFrame = static_cast<FrameT*>(pFrame_);
    OrbxKB8Rig rig;
    bool ok = pFrame->Nleft >= 0 && rig_detail::rig_of<Fisheye>(pFrame, nullptr, rig);
    for (int i = 0; ok && i < pFrame->Nleft && i < (int)pFrame->mvuRight.size(); i++)
        if (pFrame->mvpMapPoints[i] && pFrame->mvuRight[i] >= 0) ok = false;       // a rectified-stereo observation: not a rig edge
    if (!ok) return PoseOptimizationAnyCamHIP(pFrame_);
    PoseGraph g;
    {
        std::unique_lock<std::mutex> lock(MapPoint::mGlobalMutex);                  // :857
        for (int i = 0; i < pFrame->N; i++) {
            MapPoint* pMP = pFrame->mvpMapPoints[i];
            if (!pMP) continue;
            pFrame->mvbOutlier[i] = false;                                          // :938, :968
            const bool right = i >= pFrame->Nleft;
            const cv::KeyPoint& kp = right ? pFrame->mvKeysRight[i - pFrame->Nleft] : pFrame->mvKeys[i];
            const Eigen::Vector3d X = pMP->GetWorldPos().template cast<double>();
            g.Xw.push_back(X.x()); g.Xw.push_back(X.y()); g.Xw.push_back(X.z());
            if (right) rig_detail::push_right_obs(kp, g.obs, g.stereo);
            else orbslam3_hip::push_edge_obs(kp, -1.f, g.obs, g.stereo);
            g.w.push_back((double)pFrame->mvInvLevelSigma2[kp.octave]);
            g.feat.push_back(i);
        }
    }
    PoseResult res;
    std::vector<uint8_t> outlier;
    {
        orbslam3_hip::RigScope<pose_solver, pose_set_rig_kb8> scope(orbslam3_hip::thread_handle<pose_solver, pose_create>(), &rig);
        PoseOptimizationSolve(pFrame, g, nullptr, res, outlier);                    // the handle it takes is the one the rig is set on
    }
    return PoseOptimizationWriteBack(pFrame, g, res, outlier);
}

template <class Fisheye = KannalaBrandt8, class KeyFrameT = KeyFrame>
inline void LocalBundleAdjustmentRigHIP(KeyFrame* pKF, bool* pbStopFlag, Map* pMap, int& num_fixedKF, int& num_OptKF, int& num_MPs, int& num_edges)
{
    OrbxKB8Rig rig, other;
    bool ok = rig_detail::rig_of<Fisheye>(static_cast<KeyFrameT*>(pKF), nullptr, rig);
    if (ok)
        for (KeyFrame* pKFi : pKF->GetVectorCovisibleKeyFrames())
            if (!rig_detail::rig_of<Fisheye>(static_cast<KeyFrameT*>(pKFi), &rig, other)) { ok = false; break; }
    if (!ok) { LocalBundleAdjustmentAnyCamHIP(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges); return; }
    LbaGraph g;
    const bool walked = LocalBundleAdjustmentGraph(pKF, pMap, g, [](KeyFrame* pKFi_, MapPoint* pMP, const std::tuple<int, int>& idx, LbaGraph& gr) {
        KeyFrameT* pKFi = static_cast<KeyFrameT*>(pKFi_);
        LbaConventionalEdge(pKFi, pMP, idx, gr);                                    // :1302-1364: the left edge (kind 0), or a stereo one (1), which is refused below
        int rightIndex = std::get<1>(idx);
        if (!pKFi->mpCamera2 || rightIndex == -1) return;                           // :1366-1369
        rightIndex -= pKFi->NLeft;
        const cv::KeyPoint& kp = pKFi->mvKeysRight[rightIndex];
        gr.ePoint.push_back(gr.mpIndex.at(pMP)); gr.ePose.push_back(gr.kfIndex.at(pKFi_));
        rig_detail::push_right_obs(kp, gr.eObs, gr.eStereo);
        gr.eW.push_back((double)pKFi->mvInvLevelSigma2[kp.octave]);
        gr.eKF.push_back(pKFi_); gr.eMP.push_back(pMP);
    });
    // the fixed cameras and the observations only turn up in the walk (LocalBundleAdjustmentHIP says what the walk has touched by then,
    // and why that is harmless)
    for (KeyFrame* pKFi : g.kfs) ok = ok && rig_detail::rig_of<Fisheye>(static_cast<KeyFrameT*>(pKFi), &rig, other);
    for (uint8_t kind : g.eStereo) ok = ok && kind != 1;
    if (!ok) { LocalBundleAdjustmentAnyCamHIP(pKF, pbStopFlag, pMap, num_fixedKF, num_OptKF, num_MPs, num_edges); return; }
    orbslam3_hip::RigScope<lba_solver, lba_set_rig_kb8> scope(orbslam3_hip::thread_handle<lba_solver, lba_create>(), &rig);
    LocalBundleAdjustmentFinish(g, walked, pbStopFlag, pMap, nullptr, num_fixedKF, num_OptKF, num_edges, true);
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
