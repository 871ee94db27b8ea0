// orbslam3_shim_rig_map.hpp -- drop-in adapter that finishes ORBmatcher for two-camera fisheye rigs (Nleft / NLeft != -1, mpCamera2 != NULL):
//
//   int SearchByBoW(KeyFrame* pKF, Frame& F, vector<MapPoint*>& vpMapPointMatches)                src/ORBmatcher.cc:223-425   (A)
//   int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, vector<MapPoint*>& vpMatches12)               src/ORBmatcher.cc:765-905   (D)
//   int SearchForTriangulation(pKF1, pKF2, vMatchedPairs, bOnlyStereo, bCoarse)                   src/ORBmatcher.cc:907-1146  (B)
//   int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th, bRight)                     src/ORBmatcher.cc:1148-1338 (C)
//
// ORBmatcherRigMapHIP owns an ORBmatcherRigHIP (orbslam3_shim_rig_match.hpp) for everything else -- rig() and matcher() -- and an
// orbm_matcher handle of its own.  Routing:
//   A  F.Nleft != -1: orbm_search_by_bow_rig, with the key frame's angles those of mvKeysUn (no mpCamera2) or of mvKeys followed by
//      mvKeysRight (:333-336), the frame's those of mvKeys followed by mvKeysRight.  F.Nleft == -1 with a rig key frame: the
//      reference (the monocular entry would read mvKeysUn beyond its NLeft entries).  Otherwise the owned matcher.
//   D  always orbm_search_by_bow_kfkf; for a rig key frame valid[i] = 0 for i >= mvKeysUn.size() (:800, :820), angles of mvKeysUn.
//   B  both key frames with two CAM_FISHEYE cameras: orbm_search_for_triangulation_rig with Tll = T1w*Tw2, Tlr = T1w*Twr2, Trl =
//      Tr1w*Tw2, Trr = Tr1w*Twr2 (:934-943).  Neither a rig: the owned matcher.  A mixed pair, or a rig of other cameras: the reference
//      (whose code leaves R12 unset for a mixed pair).
//   C  pKF->NLeft != -1: the prelude (:1176-1239) with the side's pose, centre and camera, orbm_fuse_search on the side's RAW key
//      points (mvKeys / mvKeysRight; KeyFrame::GetFeaturesInArea walks them, src/KeyFrame.cc:732-737) and the side's half of
//      mDescriptors, u_right an array of -1 -- a rig's mvuRight is NLeft entries of -1 (src/Frame.cc:1257), which the reference reads
//      with the side-local index, past its end for NRight > NLeft: the restatement is always the monocular gate 5.99 --, bestIdx +
//      NLeft for the right side (:1298), and the pointer surgery of :1312-1331 in order.  A conventional key frame: the owned matcher.
// The reference-tree types are template parameters (Frame, KeyFrame, MapPoint, KannalaBrandt8 and ORBmatcher there, which have the rig
// members themselves; derived stand-ins in the typed tests).
#pragma once

#include "orbslam3_shim_rig_match.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

#include "CameraModels/KannalaBrandt8.h"

namespace ORB_SLAM3 {

template <class FrameT = Frame, class KeyFrameT = KeyFrame, class MapPointT = MapPoint, class Fisheye = KannalaBrandt8, class ReferenceT = ORBmatcher>
class ORBmatcherRigMapHIP {
public:
    ORBmatcherRigMapHIP(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri), rig_(nnratio, checkOri)
    { orbslam3_hip::check(orbm_create(0, &m_)); }
    ~ORBmatcherRigMapHIP() { orbm_destroy(m_); }
    ORBmatcherRigMapHIP(const ORBmatcherRigMapHIP&) = delete;
    ORBmatcherRigMapHIP& operator=(const ORBmatcherRigMapHIP&) = delete;

    ORBmatcherRigHIP<FrameT, MapPointT>& rig() { return rig_; }    // the tracking searches
    ORBmatcherHIP& matcher() { return rig_.matcher(); }             // every other search

    int SearchByBoW(KeyFrame* pKF_, Frame& F_, std::vector<MapPoint*>& vpMapPointMatches)
    {
        KeyFrameT* pKF = static_cast<KeyFrameT*>(pKF_);
        if (F_.Nleft == -1) {
            if (pKF->NLeft != -1) return ReferenceT(mfNNratio, mbCheckOrientation).SearchByBoW(pKF_, F_, vpMapPointMatches);
            return matcher().SearchByBoW(pKF_, F_, vpMapPointMatches);
        }
        FrameT& F = static_cast<FrameT&>(F_);
        const std::vector<MapPoint*> vpMapPointsKF = pKF->GetMapPointMatches();
        const int nKF = (int)vpMapPointsKF.size(), nF = F.N;
        std::vector<uint8_t> valid(nKF);
        std::vector<float> angKF(nKF), angF(nF);
        for (int i = 0; i < nKF; i++) {
            valid[i] = vpMapPointsKF[i] && !vpMapPointsKF[i]->isBad();
            angKF[i] = !pKF->mpCamera2 ? pKF->mvKeysUn[i].angle : i >= pKF->NLeft ? pKF->mvKeysRight[i - pKF->NLeft].angle : pKF->mvKeys[i].angle;    // :333-336
        }
        for (int i = 0; i < nF; i++) angF[i] = i >= F.Nleft ? F.mvKeysRight[i - F.Nleft].angle : F.mvKeys[i].angle;                                    // :340-343, :370-373
        orbslam3_hip::FlatFeatVec<DBoW2::FeatureVector> fvKF(pKF->mFeatVec), fvF(F.mFeatVec);
        std::vector<int32_t> match(std::max(nF, 1), -1);
        const int n = orbslam3_hip::check(orbm_search_by_bow_rig(m_, pKF->mDescriptors.data, nKF, valid.data(), angKF.data(), &fvKF.view,
                                                                  F.mDescriptors.data, nF, F.Nleft, angF.data(), &fvF.view, mfNNratio, mbCheckOrientation, match.data()));
        vpMapPointMatches.assign(nF, static_cast<MapPoint*>(NULL));
        for (int f = 0; f < nF; f++) if (match[f] >= 0) vpMapPointMatches[f] = vpMapPointsKF[match[f]];
        return n;
    }

    int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12)
    {
        KeyFrame* kf[2] = {pKF1, pKF2};
        std::vector<MapPoint*> pts[2];
        std::vector<uint8_t> valid[2];
        std::vector<float> ang[2];
        for (int q = 0; q < 2; q++) {
            pts[q] = kf[q]->GetMapPointMatches();
            const int n = (int)pts[q].size(), nUn = (int)kf[q]->mvKeysUn.size();
            valid[q].assign(n, 0); ang[q].assign(n, 0.f);
            for (int i = 0; i < n; i++) {
                if (kf[q]->NLeft != -1 && i >= nUn) continue;                                   // :800, :820
                valid[q][i] = pts[q][i] && !pts[q][i]->isBad();
                if (i < nUn) ang[q][i] = kf[q]->mvKeysUn[i].angle;
            }
        }
        const int n1 = (int)pts[0].size(), n2 = (int)pts[1].size();
        orbslam3_hip::FlatFeatVec<DBoW2::FeatureVector> fv1(pKF1->mFeatVec), fv2(pKF2->mFeatVec);
        std::vector<int32_t> m12(std::max(n1, 1), -1);
        const int n = orbslam3_hip::check(orbm_search_by_bow_kfkf(m_, pKF1->mDescriptors.data, n1, valid[0].data(), ang[0].data(), &fv1.view,
                                                                   pKF2->mDescriptors.data, n2, valid[1].data(), ang[1].data(), &fv2.view,
                                                                   mfNNratio, mbCheckOrientation, m12.data()));
        vpMatches12.assign(n1, static_cast<MapPoint*>(NULL));
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vpMatches12[i] = pts[1][m12[i]];
        return n;
    }

    int SearchForTriangulation(KeyFrame* pKF1_, KeyFrame* pKF2_, std::vector<std::pair<size_t, size_t> >& vMatchedPairs, const bool bOnlyStereo, const bool bCoarse = false)
    {
        if (!pKF1_->mpCamera2 && !pKF2_->mpCamera2) return matcher().SearchForTriangulation(pKF1_, pKF2_, vMatchedPairs, bOnlyStereo, bCoarse);
        KeyFrameT* kf[2] = {static_cast<KeyFrameT*>(pKF1_), static_cast<KeyFrameT*>(pKF2_)};
        GeometricCamera* cams[4] = {kf[0]->mpCamera, kf[0]->mpCamera2, kf[1]->mpCamera, kf[1]->mpCamera2};
        bool fisheye_rigs = true;
        for (GeometricCamera* c : cams) fisheye_rigs = fisheye_rigs && c && c->GetType() == GeometricCamera::CAM_FISHEYE;
        if (!fisheye_rigs) return ReferenceT(mfNNratio, mbCheckOrientation).SearchForTriangulation(pKF1_, pKF2_, vMatchedPairs, bOnlyStereo, bCoarse);
        OrbmRigTriGeometry g;
        for (int c = 0; c < 4; c++) {
            Fisheye* cam = static_cast<Fisheye*>(cams[c]);
            for (int k = 0; k < 8; k++) g.cam[c][k] = cam->getParameter(k);
            g.cam[c][8] = cam->GetPrecision();
        }
        const Sophus::SE3f T1w = kf[0]->GetPose(), Tw2 = kf[1]->GetPoseInverse(), Tr1w = kf[0]->GetRightPose(), Twr2 = kf[1]->GetRightPoseInverse();     // :914-939
        const Sophus::SE3f T12[4] = {T1w * Tw2, T1w * Twr2, Tr1w * Tw2, Tr1w * Twr2};
        for (int c = 0; c < 4; c++) {
            const Eigen::Matrix3f R = T12[c].rotationMatrix();
            const Eigen::Vector3f t = T12[c].translation();
            for (int r = 0; r < 3; r++) { for (int q = 0; q < 3; q++) g.R12[c][3 * r + q] = R(r, q); g.t12[c][r] = t(r); }
        }
        struct Side { std::vector<uint8_t> mp; std::vector<float> x, y, a; std::vector<int32_t> o; };
        Side sd[2];
        OrbmTriSide ts[2];
        orbslam3_hip::FlatFeatVec<DBoW2::FeatureVector> fv1(kf[0]->mFeatVec), fv2(kf[1]->mFeatVec);
        for (int q = 0; q < 2; q++) {
            const int n = kf[q]->N, nl = kf[q]->NLeft;
            Side& s = sd[q];
            s.mp.resize(n); s.x.resize(n); s.y.resize(n); s.a.resize(n); s.o.resize(n);
            for (int i = 0; i < n; i++) {
                s.mp[i] = kf[q]->GetMapPoint(i) != NULL;
                const cv::KeyPoint& kp = i < nl ? kf[q]->mvKeys[i] : kf[q]->mvKeysRight[i - nl];        // :985-987, :1020-1022
                s.x[i] = kp.pt.x; s.y[i] = kp.pt.y; s.a[i] = kp.angle; s.o[i] = kp.octave;
            }
            ts[q].n = n; ts[q].desc = kf[q]->mDescriptors.data; ts[q].has_mp = s.mp.data(); ts[q].stereo = NULL;
            ts[q].x = s.x.data(); ts[q].y = s.y.data(); ts[q].octave = s.o.data(); ts[q].angle = s.a.data();
            ts[q].fv = q ? fv2.view : fv1.view;
        }
        const int n1 = kf[0]->N;
        // both sigma tables are read up to n_levels: the shorter one bounds it, and an octave beyond it is refused by the entry's check
        const int nLevels = (int)std::min(kf[0]->mvLevelSigma2.size(), kf[1]->mvLevelSigma2.size());
        std::vector<int32_t> m12(std::max(n1, 1), -1);
        const int n = orbslam3_hip::check(orbm_search_for_triangulation_rig(m_, &ts[0], kf[0]->NLeft, &ts[1], kf[1]->NLeft, &g, kf[0]->mvLevelSigma2.data(),
                                                                             kf[1]->mvLevelSigma2.data(), nLevels, bOnlyStereo, bCoarse,
                                                                             mbCheckOrientation, m12.data()));
        vMatchedPairs.clear();
        vMatchedPairs.reserve(n);
        for (int i = 0; i < n1; i++) if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));     // :1138-1143
        return n;
    }

    int Fuse(KeyFrame* pKF_, const std::vector<MapPoint*>& vpMapPoints, const float th = 3.0, const bool bRight = false)
    {
        if (pKF_->NLeft == -1) return matcher().Fuse(pKF_, vpMapPoints, th, bRight);
        KeyFrameT* pKF = static_cast<KeyFrameT*>(pKF_);
        const Sophus::SE3f Tcw = bRight ? pKF->GetRightPose() : pKF->GetPose();                    // :1154-1163
        const Eigen::Vector3f Ow = bRight ? pKF->GetRightCameraCenter() : pKF->GetCameraCenter();
        GeometricCamera* pCamera = bRight ? pKF->mpCamera2 : pKF->mpCamera;
        const float bf = pKF->mbf;
        const int nMPs = (int)vpMapPoints.size();
        std::vector<uint8_t> valid(nMPs, 0), desc((size_t)nMPs * 32, 0);
        std::vector<float> u(nMPs, 0.f), v(nMPs, 0.f), ur(nMPs, 0.f);
        std::vector<int32_t> lvl(nMPs, 0), bestIdx(std::max(nMPs, 1)), bestDist(std::max(nMPs, 1));
        for (int i = 0; i < nMPs; i++) {                                          // prelude :1176-1239
            MapPoint* pMP = vpMapPoints[i];
            if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
            const Eigen::Vector3f p3Dw = pMP->GetWorldPos();
            const Eigen::Vector3f p3Dc = Tcw * p3Dw;
            if (p3Dc(2) < 0.0f) continue;
            const float invz = 1 / p3Dc(2);
            const Eigen::Vector2f uv = pCamera->project(p3Dc);
            if (!pKF->IsInImage(uv(0), uv(1))) continue;
            const Eigen::Vector3f PO = p3Dw - Ow;
            const float dist3D = PO.norm();
            if (dist3D < pMP->GetMinDistanceInvariance() || dist3D > pMP->GetMaxDistanceInvariance()) continue;
            if (PO.dot(pMP->GetNormal()) < 0.5 * dist3D) continue;
            valid[i] = 1; u[i] = uv(0); v[i] = uv(1); ur[i] = uv(0) - bf * invz;
            lvl[i] = pMP->PredictScale(dist3D, pKF);
            const cv::Mat d = pMP->GetDescriptor();
            std::memcpy(&desc[(size_t)i * 32], d.data, 32);
        }
        const std::vector<cv::KeyPoint>& keys = bRight ? pKF->mvKeysRight : pKF->mvKeys;       // the side's RAW key points (src/KeyFrame.cc:732-737)
        const int nl = pKF->NLeft, nK = bRight ? pKF->N - nl : nl;
        std::vector<float> x(nK), y(nK), noRight(std::max(nK, 1), -1.f);
        std::vector<int32_t> o(nK);
        for (int i = 0; i < nK; i++) { x[i] = keys[i].pt.x; y[i] = keys[i].pt.y; o[i] = keys[i].octave; }
        OrbmFrame f;
        f.n = nK; f.x = x.data(); f.y = y.data(); f.octave = o.data(); f.angle = NULL;
        f.desc = pKF->mDescriptors.data + (bRight ? (size_t)nl * 32 : 0);
        f.min_x = pKF->mnMinX; f.min_y = pKF->mnMinY; f.max_x = pKF->mnMaxX; f.max_y = pKF->mnMaxY;
        f.grid_cols = pKF->mnGridCols; f.grid_rows = pKF->mnGridRows;
        f.scale_factors = pKF->mvScaleFactors.data(); f.n_levels = (int)pKF->mvScaleFactors.size(); f.u_right = NULL;
        orbslam3_hip::check(orbm_fuse_search(m_, &f, noRight.data(), pKF->mvInvLevelSigma2.data(), nMPs, valid.data(), u.data(), v.data(),
                                             ur.data(), lvl.data(), desc.data(), th, 1, bestIdx.data(), bestDist.data()));
        int nFused = 0;
        for (int i = 0; i < nMPs; i++) {                                          // :1311-1333, in order
            if (!valid[i] || bestIdx[i] < 0 || bestDist[i] > 50 /* TH_LOW */) continue;
            MapPoint* pMP = vpMapPoints[i];
            if (pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;    // :1187-1196 see the surgery of earlier iterations (duplicates, Replace)
            const int slot = bestIdx[i] + (bRight ? nl : 0);          // :1298
            MapPoint* pMPinKF = pKF->GetMapPoint(slot);
            if (pMPinKF) {
                if (!pMPinKF->isBad()) {
                    if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
                    else pMPinKF->Replace(pMP);
                }
            } else {
                pMP->AddObservation(pKF, slot);
                pKF->AddMapPoint(pMP, slot);
            }
            nFused++;
        }
        return nFused;
    }

private:
    float mfNNratio;
    bool mbCheckOrientation;
    ORBmatcherRigHIP<FrameT, MapPointT> rig_;
    orbm_matcher* m_ = nullptr;
};

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
