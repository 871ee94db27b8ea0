// orbslam3_shim_rig_mapping.hpp -- drop-in adapter for the numerical part of LocalMapping::CreateNewMapPoints (reference
// src/LocalMapping.cc:392-716) when the key frames are two-camera fisheye rigs (NLeft != -1, mpCamera2 != NULL), on top of
// orbm_create_new_map_points_rig of orbslam3_hip_rig_newpoints.h:
//
//   bool CreateNewMapPointsRigHIP(KeyFrame* pKF, const std::vector<KeyFrame*>& vpNeighKFs, bool bInertial, bool bCoarse,
//                                 bool bFarPoints, float thFarPoints, std::vector<NewMapPointCandidate>& vCandidates,
//                                 std::vector<bool>* pvbSkipped = NULL)
//
// Routing on NLeft:
//   every key frame conventional (NLeft == -1): CreateNewMapPointsHIP of orbslam3_shim_mapping.hpp, with its contract -- the caller
//     passes the neighbours that survive the baseline test;
//   every key frame a rig of two CAM_FISHEYE cameras: orbm_create_new_map_points_rig.  The caller passes ALL neighbours: for a rig
//     the baseline test (:447-455) reads the centre that the last match of an earlier neighbour left in Ow1, so it runs inside the
//     call; *pvbSkipped reports which neighbours it skipped.  CheckNewKeyFrames() (:440) is checked once before the call;
//   a mixed pair (one key frame a rig, another not), or a rig of other cameras: false, without touching the device -- the caller
//     runs the reference's own loop.
// The adapter flattens the rig key frames (raw mvKeys followed by mvKeysRight, GetPose / GetRightPose and the two centres, the two
// cameras), computes per neighbour the four products T1w*Tw2, T1w*Twr2, Tr1w*Tw2, Tr1w*Twr2 as ORBmatcherRigMapHIP does for the
// search (src/ORBmatcher.cc:934-943), makes the one call and returns the candidates in the reference's creation order --
// (neighbour, idx1) ascending -- for the caller to run the pointer surgery of :698-713 on.  bPointStereo is false for every rig point.
//
// The key-frame and camera types are template parameters (KeyFrame and KannalaBrandt8 in the reference tree).
#pragma once

#include "orbslam3_shim_mapping.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include "CameraModels/KannalaBrandt8.h"

namespace ORB_SLAM3 {

namespace rig_mapping_detail {

template <class KF, class Fisheye>
struct FlatRigKeyFrame {        // the arrays an OrbmRigMapKeyFrame points into
    std::vector<uint8_t> mp;
    std::vector<float> x, y;
    std::vector<int32_t> o;
    orbslam3_hip::FlatFeatVec<DBoW2::FeatureVector> fv;

    FlatRigKeyFrame(KF* k, OrbmRigMapKeyFrame& d) : fv(k->mFeatVec)
    {
        const int n = k->N, nl = k->NLeft;
        mp.resize(n); x.resize(n); y.resize(n); o.resize(n);
        for (int i = 0; i < n; i++) {
            mp[i] = k->GetMapPoint(i) != NULL;
            const cv::KeyPoint& kp = i < nl ? k->mvKeys[i] : k->mvKeysRight[i - nl];        // :492-494, :500-502
            x[i] = kp.pt.x; y[i] = kp.pt.y; o[i] = kp.octave;
        }
        d.side.n = n; d.side.desc = k->mDescriptors.data; d.side.has_mp = mp.data(); d.side.stereo = NULL;
        d.side.x = x.data(); d.side.y = y.data(); d.side.octave = o.data(); d.side.angle = NULL;
        d.side.fv = fv.view;
        d.n_left = nl;
        const Sophus::SE3f T[2] = {k->GetPose(), k->GetRightPose()};
        const Eigen::Vector3f C[2] = {k->GetCameraCenter(), k->GetRightCameraCenter()};
        Fisheye* cam[2] = {static_cast<Fisheye*>(k->mpCamera), static_cast<Fisheye*>(k->mpCamera2)};
        for (int s = 0; s < 2; s++) {
            const Eigen::Matrix3f R = T[s].rotationMatrix();
            const Eigen::Vector3f t = T[s].translation();
            for (int r = 0; r < 3; r++) {
                for (int c = 0; c < 3; c++) d.Rcw[s][3 * r + c] = R(r, c);
                d.tcw[s][r] = t(r); d.Ow[s][r] = C[s](r);
            }
            for (int q = 0; q < 8; q++) d.cam[s][q] = cam[s]->getParameter(q);
            d.cam[s][8] = cam[s]->GetPrecision();
        }
        d.mb = k->mb;
        d.level_sigma2 = k->mvLevelSigma2.data(); d.scale_factors = k->mvScaleFactors.data();
        d.n_levels = (int32_t)std::min(k->mvLevelSigma2.size(), k->mvScaleFactors.size());
    }
    FlatRigKeyFrame(const FlatRigKeyFrame&) = delete;
    FlatRigKeyFrame& operator=(const FlatRigKeyFrame&) = delete;
};

template <class KF>
inline bool fisheye_rig(KF* k)
{
    return k->NLeft != -1 && k->mpCamera && k->mpCamera2 && k->mpCamera->GetType() == GeometricCamera::CAM_FISHEYE &&
           k->mpCamera2->GetType() == GeometricCamera::CAM_FISHEYE;
}

}  // namespace rig_mapping_detail

template <class KF, class Fisheye = KannalaBrandt8>
bool CreateNewMapPointsRigHIP(KF* pKF, const std::vector<KF*>& vpNeighKFs, const bool bInertial, const bool bCoarse, const bool bFarPoints,
                              const float thFarPoints, std::vector<NewMapPointCandidateT<KF> >& vCandidates, std::vector<bool>* pvbSkipped = NULL)
{
    namespace rd = rig_mapping_detail;
    vCandidates.clear();
    const int nn = (int)vpNeighKFs.size(), n1 = pKF->N;
    if (pvbSkipped) pvbSkipped->assign(nn, false);
    bool any_rig = pKF->NLeft != -1 || pKF->mpCamera2, all_rigs = rd::fisheye_rig(pKF);
    for (KF* k : vpNeighKFs) {
        any_rig = any_rig || k->NLeft != -1 || k->mpCamera2;
        all_rigs = all_rigs && rd::fisheye_rig(k);
    }
    if (!any_rig) return CreateNewMapPointsHIP(pKF, vpNeighKFs, bInertial, bCoarse, bFarPoints, thFarPoints, vCandidates);
    if (!all_rigs) return false;                                                    // a mixed pair, or a rig of other cameras
    if (nn > ORBM_MAX_NEIGHBOURS) throw orbslam3_hip::Error(ORBX_ERR_CAPACITY);
    std::vector<OrbmRigMapKeyFrame> kfs(1 + nn);
    std::vector<std::unique_ptr<rd::FlatRigKeyFrame<KF, Fisheye> > > flat;
    flat.emplace_back(new rd::FlatRigKeyFrame<KF, Fisheye>(pKF, kfs[0]));
    std::vector<OrbmRigTriGeometry> geom(std::max(nn, 1));
    std::vector<OrbmRigMapPair> pairs(std::max(nn, 1));
    const Sophus::SE3f T1w = pKF->GetPose(), Tr1w = pKF->GetRightPose();
    for (int j = 0; j < nn; j++) {
        KF* pKF2 = vpNeighKFs[j];
        flat.emplace_back(new rd::FlatRigKeyFrame<KF, Fisheye>(pKF2, kfs[1 + j]));
        OrbmRigTriGeometry& g = geom[j];
        for (int q = 0; q < 9; q++) { g.cam[0][q] = kfs[0].cam[0][q]; g.cam[1][q] = kfs[0].cam[1][q]; g.cam[2][q] = kfs[1 + j].cam[0][q]; g.cam[3][q] = kfs[1 + j].cam[1][q]; }
        const Sophus::SE3f Tw2 = pKF2->GetPoseInverse(), Twr2 = pKF2->GetRightPoseInverse();                     // src/ORBmatcher.cc:914-939
        const Sophus::SE3f T12[4] = {T1w * Tw2, T1w * Twr2, Tr1w * Tw2, Tr1w * Twr2};
        for (int c = 0; c < 4; c++) {
            const Eigen::Matrix3f R = T12[c].rotationMatrix();
            const Eigen::Vector3f t = T12[c].translation();
            for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) g.R12[c][3 * r + q] = R(r, q); g.t12[c][r] = t(r); }
        }
        pairs[j].geom = &g; pairs[j].coarse = bCoarse ? 1 : 0;
    }
    OrbmMapParams par;
    par.inertial = bInertial ? 1 : 0; par.far_points = bFarPoints ? 1 : 0; par.th_far = thFarPoints; par.scale_factor_1 = pKF->mfScaleFactor;
    const size_t m = (size_t)std::max(n1, 1);
    std::vector<int32_t> nb(m, -1), idx2(m, -1), n_matched(std::max(nn, 1), 0), n_created(std::max(nn, 1), 0);
    std::vector<float> x3d(3 * m, 0.f), normal(3 * m, 0.f), maxd(m, 0.f), mind(m, 0.f);
    std::vector<uint8_t> ps(m, 0), skipped(std::max(nn, 1), 0);
    OrbmNewPoints out;
    out.neighbour = nb.data(); out.idx2 = idx2.data(); out.x3d = x3d.data(); out.point_stereo = ps.data();
    out.normal = normal.data(); out.max_dist = maxd.data(); out.min_dist = mind.data();
    out.n_matched = n_matched.data(); out.n_created = n_created.data(); out.match12 = NULL;
    const int created = orbslam3_hip::check(orbm_create_new_map_points_rig(mapping_detail::matcher(), &kfs[0], nn ? &kfs[1] : NULL, nn, pairs.data(), &par, &out,
                                                                           skipped.data()));
    if (pvbSkipped)
        for (int j = 0; j < nn; j++) (*pvbSkipped)[j] = skipped[j] != 0;
    vCandidates.reserve(created);
    for (int j = 0; j < nn; j++)                                                    // the reference's creation order: neighbour by neighbour,
        for (int i = 0; i < n1; i++) {                                              // vMatchedIndices in feature order (src/ORBmatcher.cc:1138-1143)
            if (nb[i] != j) continue;
            NewMapPointCandidateT<KF> c;
            c.idx1 = i; c.pKF2 = vpNeighKFs[j]; c.idx2 = idx2[i]; c.bPointStereo = false;
            for (int r = 0; r < 3; r++) { c.x3D(r) = x3d[3 * i + r]; c.normal(r) = normal[3 * i + r]; }
            c.fMaxDistance = maxd[i]; c.fMinDistance = mind[i];
            vCandidates.push_back(c);
        }
    return true;
}

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
