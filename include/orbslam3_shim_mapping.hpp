// orbslam3_shim_mapping.hpp -- drop-in adapter for the numerical part of LocalMapping::CreateNewMapPoints (reference
// src/LocalMapping.cc:392-716), on top of orbm_create_new_map_points of orbslam3_hip.h:
//
//   bool CreateNewMapPointsHIP(KeyFrame* pKF, const std::vector<KeyFrame*>& vpNeighKFs, bool bInertial, bool bCoarse,
//                              bool bFarPoints, float thFarPoints, std::vector<NewMapPointCandidate>& vCandidates)
//
// The caller keeps the two host parts of the reference's loop: it passes the neighbours that survive the baseline test
// (:447-464, ComputeSceneMedianDepth walks map points) and checks CheckNewKeyFrames() once before the call (:440).  The
// adapter fills the POD structs from the reference's types, makes the one call and returns the candidates in the reference's
// creation order -- (neighbour, idx1) ascending -- for the caller to run the pointer surgery of :698-713 on: new MapPoint(x3D,
// pKF, map), the two AddObservation / AddMapPoint, ComputeDistinctiveDescriptors; UpdateNormalAndDepth is already in the
// candidate (normal, fMaxDistance, fMinDistance).  It returns false without touching the device when a key frame has a second
// camera (mpCamera2): the caller then runs the reference's own loop.
//
// Like orbslam3_shim_loop.hpp it is written against the reference's own types and compiles inside an ORB-SLAM3 tree with
// ORBSLAM3_HIP_WITH_REFERENCE defined.  The key-frame type is a template parameter (KeyFrame in the reference tree).
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include <algorithm>
#include <memory>

namespace ORB_SLAM3 {

template <class KF>
struct NewMapPointCandidateT {
    int idx1;                   // feature of the current key frame
    KF* pKF2;                   // the neighbour that accepted it
    int idx2;                   // feature of pKF2
    Eigen::Vector3f x3D;
    bool bPointStereo;
    Eigen::Vector3f normal;     // MapPoint::UpdateNormalAndDepth of the point with its two observations, pRefKF = pKF
    float fMaxDistance, fMinDistance;
};
typedef NewMapPointCandidateT<KeyFrame> NewMapPointCandidate;

namespace mapping_detail {

inline orbm_matcher* matcher() { return orbslam3_hip::thread_handle<orbm_matcher, orbm_create>(); }

template <class KF>
struct FlatKeyFrame {           // the arrays an OrbmMapKeyFrame points into
    std::vector<uint8_t> mp, st;
    std::vector<float> x, y, kx, ky;
    std::vector<int32_t> o;
    orbslam3_hip::FlatFeatVec<DBoW2::FeatureVector> fv;

    FlatKeyFrame(KF* k, OrbmMapKeyFrame& d) : fv(k->mFeatVec)
    {
        const int n = k->N;
        mp.resize(n); st.resize(n); x.resize(n); y.resize(n); kx.resize(n); ky.resize(n); o.resize(n);
        for (int i = 0; i < n; i++) {
            mp[i] = k->GetMapPoint(i) != NULL; st[i] = k->mvuRight[i] >= 0;
            const cv::KeyPoint& kp = k->mvKeysUn[i];
            x[i] = kp.pt.x; y[i] = kp.pt.y; o[i] = kp.octave;
            kx[i] = k->mvKeys[i].pt.x; ky[i] = k->mvKeys[i].pt.y;                   // KeyFrame::UnprojectStereo reads mvKeys (KeyFrame.cc:760-761)
        }
        d.side.n = n; d.side.desc = k->mDescriptors.data; d.side.has_mp = mp.data(); d.side.stereo = st.data();
        d.side.x = x.data(); d.side.y = y.data(); d.side.octave = o.data(); d.side.angle = NULL;
        d.side.fv = fv.view;
        d.u_right = k->mvuRight.data(); d.depth = k->mvDepth.data(); d.key_x = kx.data(); d.key_y = ky.data();
        const Sophus::SE3f Tcw = k->GetPose();
        const Eigen::Matrix3f R = Tcw.rotationMatrix();
        const Eigen::Vector3f t = Tcw.translation(), Ow = k->GetCameraCenter();
        for (int r = 0; r < 3; r++) {
            for (int c = 0; c < 3; c++) d.Rcw[3 * r + c] = R(r, c);
            d.tcw[r] = t(r); d.Ow[r] = Ow(r);
        }
        d.fx = k->fx; d.fy = k->fy; d.cx = k->cx; d.cy = k->cy; d.invfx = k->invfx; d.invfy = k->invfy; d.mb = k->mb; d.mbf = k->mbf;
        d.level_sigma2 = k->mvLevelSigma2.data(); d.scale_factors = k->mvScaleFactors.data(); d.n_levels = (int32_t)k->mvScaleFactors.size();
    }
    FlatKeyFrame(const FlatKeyFrame&) = delete;
    FlatKeyFrame& operator=(const FlatKeyFrame&) = delete;
};

}  // namespace mapping_detail

template <class KF>
bool CreateNewMapPointsHIP(KF* pKF, const std::vector<KF*>& vpNeighKFs, const bool bInertial, const bool bCoarse, const bool bFarPoints,
                           const float thFarPoints, std::vector<NewMapPointCandidateT<KF> >& vCandidates)
{
    vCandidates.clear();
    if (pKF->mpCamera2) return false;
    for (KF* k : vpNeighKFs)
        if (k->mpCamera2) return false;
    const int nn = (int)vpNeighKFs.size(), n1 = pKF->N;
    if (nn > ORBM_MAX_NEIGHBOURS) throw orbslam3_hip::Error(ORBX_ERR_CAPACITY);
    std::vector<OrbmMapKeyFrame> kfs(1 + nn);
    std::vector<std::unique_ptr<mapping_detail::FlatKeyFrame<KF> > > flat;
    flat.emplace_back(new mapping_detail::FlatKeyFrame<KF>(pKF, kfs[0]));
    std::vector<OrbmMapPair> pairs(std::max(nn, 1));
    const Sophus::SE3f T1w = pKF->GetPose();
    for (int j = 0; j < nn; j++) {
        KF* pKF2 = vpNeighKFs[j];
        flat.emplace_back(new mapping_detail::FlatKeyFrame<KF>(pKF2, kfs[1 + j]));
        const Eigen::Vector3f C2 = pKF2->GetPose() * pKF->GetCameraCenter();           // src/ORBmatcher.cc:914-920
        const Eigen::Vector2f ep = pKF2->mpCamera->project(C2);
        const Sophus::SE3f T12 = T1w * pKF2->GetPoseInverse();
        const Eigen::Matrix3f F12 = pKF->mpCamera->toK_().transpose().inverse() * Sophus::SO3f::hat(T12.translation()) * T12.rotationMatrix() *
                                    pKF2->mpCamera->toK_().inverse();                  // Pinhole.cpp:109-112
        pairs[j].ep_x = ep(0); pairs[j].ep_y = ep(1);
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) pairs[j].F12[r * 3 + c] = F12(r, c);
        pairs[j].coarse = bCoarse ? 1 : 0;
    }
    OrbmMapParams par;
    par.inertial = bInertial ? 1 : 0; par.far_points = bFarPoints ? 1 : 0; par.th_far = thFarPoints; par.scale_factor_1 = pKF->mfScaleFactor;
    const size_t m = (size_t)std::max(n1, 1);
    std::vector<int32_t> nb(m, -1), idx2(m, -1), n_matched(std::max(nn, 1), 0), n_created(std::max(nn, 1), 0);
    std::vector<float> x3d(3 * m, 0.f), normal(3 * m, 0.f), maxd(m, 0.f), mind(m, 0.f);
    std::vector<uint8_t> ps(m, 0);
    OrbmNewPoints out;
    out.neighbour = nb.data(); out.idx2 = idx2.data(); out.x3d = x3d.data(); out.point_stereo = ps.data();
    out.normal = normal.data(); out.max_dist = maxd.data(); out.min_dist = mind.data();
    out.n_matched = n_matched.data(); out.n_created = n_created.data(); out.match12 = NULL;
    const int created = orbslam3_hip::check(orbm_create_new_map_points(mapping_detail::matcher(), &kfs[0], nn ? &kfs[1] : NULL, nn, pairs.data(), &par, &out));
    vCandidates.reserve(created);
    for (int j = 0; j < nn; j++)                                                    // the reference's creation order: neighbour by neighbour,
        for (int i = 0; i < n1; i++) {                                              // vMatchedIndices in feature order (src/ORBmatcher.cc:1133-1143)
            if (nb[i] != j) continue;
            NewMapPointCandidateT<KF> c;
            c.idx1 = i; c.pKF2 = vpNeighKFs[j]; c.idx2 = idx2[i]; c.bPointStereo = ps[i] != 0;
            for (int r = 0; r < 3; r++) { c.x3D(r) = x3d[3 * i + r]; c.normal(r) = normal[3 * i + r]; }
            c.fMaxDistance = maxd[i]; c.fMinDistance = mind[i];
            vCandidates.push_back(c);
        }
    return true;
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
