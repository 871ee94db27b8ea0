// orbslam3_shim_rig_match.hpp -- drop-in adapter that adds the two-camera fisheye rig (Nleft != -1) to the two tracking searches:
//
//   int SearchByProjection(Frame& F, const vector<MapPoint*>&, th, bFarPoints, thFarPoints)      src/ORBmatcher.cc:43-213
//   int SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)               src/ORBmatcher.cc:1676-1887
//
// ORBmatcherRigHIP owns an ORBmatcherHIP (orbslam3_shim.hpp) for every frame that is not a rig frame -- and everything else that
// class offers, through matcher() -- and an orbm_matcher handle of its own for the rig calls of orbslam3_hip_rig_match.h.
// A rig frame is viewed as an OrbmRigFrame: the RAW key points mvKeys[0..Nleft) and mvKeysRight[0..Nright) (a rig frame has no
// undistorted list), mDescriptors rows [0, Nleft) and [Nleft, N), mvLeftToRightMatch / mvRightToLeftMatch, and ONE slot array
// mvpMapPoints[0..N).  The last-frame overload projects as the reference does: x3Dc = Tcw * x3Dw, uv = mpCamera->project(x3Dc),
// and for the right pass mpCamera->project(GetRelativePoseTrl() * x3Dc) -- the LEFT camera's project (:1795-1796), not mpCamera2's.
// The frame and map-point types are template parameters (Frame and MapPoint in the reference tree, which have the rig members
// themselves; derived stand-ins in the typed tests): the rig members are reached through a static_cast to them.
#pragma once

#include "orbslam3_shim.hpp"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

namespace ORB_SLAM3 {

template <class FrameT = Frame, class MapPointT = MapPoint>
class ORBmatcherRigHIP {
public:
    ORBmatcherRigHIP(float nnratio = 0.6, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri), conventional_(nnratio, checkOri)
    { orbslam3_hip::check(orbm_create(0, &m_)); }
    ~ORBmatcherRigHIP() { orbm_destroy(m_); }
    ORBmatcherRigHIP(const ORBmatcherRigHIP&) = delete;
    ORBmatcherRigHIP& operator=(const ORBmatcherRigHIP&) = delete;

    ORBmatcherHIP& matcher() { return conventional_; }     // every other search

    int SearchByProjection(Frame& F_, const std::vector<MapPoint*>& vpMapPoints, const float th = 3, const bool bFarPoints = false, const float thFarPoints = 50.0f)
    {
        if (F_.Nleft == -1) return conventional_.SearchByProjection(F_, vpMapPoints, th, bFarPoints, thFarPoints);
        FrameT& F = static_cast<FrameT&>(F_);
        const int nMP = (int)vpMapPoints.size();
        std::vector<uint8_t> inView(nMP), inViewR(nMP), hasObs(nMP), bad(nMP), desc((size_t)nMP * 32);
        std::vector<float> u(nMP), v(nMP), vc(nMP), uR(nMP), vR(nMP), vcR(nMP), depth(nMP);
        std::vector<int32_t> lvl(nMP), lvlR(nMP);
        for (int i = 0; i < nMP; i++) {
            MapPointT* p = static_cast<MapPointT*>(vpMapPoints[i]);
            inView[i] = p->mbTrackInView; u[i] = p->mTrackProjX; v[i] = p->mTrackProjY; lvl[i] = p->mnTrackScaleLevel; vc[i] = p->mTrackViewCos;
            inViewR[i] = p->mbTrackInViewR; uR[i] = p->mTrackProjXR; vR[i] = p->mTrackProjYR; lvlR[i] = p->mnTrackScaleLevelR; vcR[i] = p->mTrackViewCosR;
            depth[i] = p->mTrackDepth; bad[i] = p->isBad(); hasObs[i] = p->Observations() > 0;
            const cv::Mat d = p->GetDescriptor();
            std::memcpy(&desc[(size_t)i * 32], d.data, 32);
        }
        RigView view(F);
        OrbmRigMapPoints pts;
        pts.n = nMP;
        pts.in_view = inView.data(); pts.proj_u = u.data(); pts.proj_v = v.data(); pts.pred_level = lvl.data(); pts.view_cos = vc.data();
        pts.in_view_r = inViewR.data(); pts.proj_u_r = uR.data(); pts.proj_v_r = vR.data(); pts.pred_level_r = lvlR.data(); pts.view_cos_r = vcR.data();
        pts.track_depth = depth.data(); pts.bad = bad.data(); pts.has_obs = hasObs.data(); pts.desc = desc.data();
        const int n = orbslam3_hip::check(orbm_search_by_projection_rig(m_, &view.rig, &pts, th, bFarPoints, thFarPoints, mfNNratio, view.assign.data(), view.occ.data()));
        for (size_t s = 0; s < view.assign.size(); s++)
            if (view.assign[s] >= 0) F.mvpMapPoints[s] = vpMapPoints[view.assign[s]];
        return n;
    }

    int SearchByProjection(Frame& CurrentFrame_, const Frame& LastFrame_, const float th, const bool bMono)
    {
        if (CurrentFrame_.Nleft == -1) return conventional_.SearchByProjection(CurrentFrame_, LastFrame_, th, bMono);
        FrameT& CurrentFrame = static_cast<FrameT&>(CurrentFrame_);
        const Frame& LastFrame = LastFrame_;
        const int nL = LastFrame.N;
        const Sophus::SE3f Tcw = CurrentFrame.GetPose();
        const Eigen::Vector3f twc = Tcw.inverse().translation();                   // :1686-1693
        const Sophus::SE3f Tlw = LastFrame.GetPose();
        const Eigen::Vector3f tlc = Tlw * twc;
        const bool bForward = tlc(2) > CurrentFrame.mb && !bMono;
        const bool bBackward = -tlc(2) > CurrentFrame.mb && !bMono;
        const int levelWindow = bForward ? ORBM_LEVELS_FORWARD : bBackward ? ORBM_LEVELS_BACKWARD : ORBM_LEVELS_AROUND;
        const Sophus::SE3f Trl = CurrentFrame.GetRelativePoseTrl();
        std::vector<uint8_t> valid(nL, 0);
        std::vector<float> u(nL, 0.f), v(nL, 0.f), uR(nL, 0.f), vR(nL, 0.f);
        for (int i = 0; i < nL; i++) {
            MapPoint* p = LastFrame.mvpMapPoints[i];
            if (!p || LastFrame.mvbOutlier[i]) continue;
            const Eigen::Vector3f x3Dc = Tcw * p->GetWorldPos();                   // the reference's own float expressions (:1703-1713)
            const float invzc = 1.0 / x3Dc(2);
            if (invzc < 0) continue;
            const Eigen::Vector2f uv = CurrentFrame.mpCamera->project(x3Dc);
            const Eigen::Vector3f x3Dr = Trl * x3Dc;                               // :1795
            const Eigen::Vector2f uvr = CurrentFrame.mpCamera->project(x3Dr);      // :1796: mpCamera, not mpCamera2
            valid[i] = 1; u[i] = uv(0); v[i] = uv(1); uR[i] = uvr(0); vR[i] = uvr(1);
        }
        return SearchByProjectionProjected(CurrentFrame_, LastFrame_, th, levelWindow, valid.data(), u.data(), v.data(), uR.data(), vR.data());
    }

    // The last-frame search of a rig frame behind its projection loop: valid / proj_u / proj_v / proj_u_r / proj_v_r [LastFrame.N] as
    // that loop (or orbm_project_last_rig_batch, through TrackProjectRigHIP) left them; level_window is one of ORBM_LEVELS_*.
    int SearchByProjectionProjected(Frame& CurrentFrame_, const Frame& LastFrame, const float th, const int levelWindow,
                                    const uint8_t* valid, const float* u, const float* v, const float* uR, const float* vR)
    {
        FrameT& CurrentFrame = static_cast<FrameT&>(CurrentFrame_);
        const int nL = LastFrame.N;
        std::vector<uint8_t> hasObs(nL, 0), desc((size_t)nL * 32, 0);
        std::vector<float> ang(nL, 0.f);
        std::vector<int32_t> oct(nL, 0);
        for (int i = 0; i < nL; i++) {
            if (!valid[i]) continue;
            MapPoint* p = LastFrame.mvpMapPoints[i];
            const bool lastRight = LastFrame.Nleft != -1 && i >= LastFrame.Nleft;
            if (lastRight) { const cv::KeyPoint& kp = LastFrame.mvKeysRight[i - LastFrame.Nleft]; oct[i] = kp.octave; ang[i] = kp.angle; }    // :1720-1721, :1777-1779
            else { oct[i] = LastFrame.mvKeys[i].octave; ang[i] = LastFrame.Nleft == -1 ? LastFrame.mvKeysUn[i].angle : LastFrame.mvKeys[i].angle; }
            hasObs[i] = p->Observations() > 0;
            const cv::Mat d = p->GetDescriptor();
            std::memcpy(&desc[(size_t)i * 32], d.data, 32);
        }
        RigView view(CurrentFrame);
        OrbmRigLastPoints pts;
        pts.n = nL;
        pts.valid = valid; pts.proj_u = u; pts.proj_v = v; pts.proj_u_r = uR; pts.proj_v_r = vR;
        pts.octave = oct.data(); pts.angle = ang.data(); pts.has_obs = hasObs.data(); pts.desc = desc.data();
        const int n = orbslam3_hip::check(orbm_search_by_projection_last_rig(m_, &view.rig, &pts, th, levelWindow, mbCheckOrientation, view.assign.data(), view.occ.data()));
        for (size_t s = 0; s < view.assign.size(); s++) {
            if (view.assign[s] >= 0) CurrentFrame.mvpMapPoints[s] = LastFrame.mvpMapPoints[view.assign[s]];
            else if (view.assign[s] == -1) CurrentFrame.mvpMapPoints[s] = static_cast<MapPoint*>(NULL);        // :1879
        }
        return n;
    }

private:
    // a rig frame as the C ABI takes it; the arrays live as long as the view
    struct RigView {
        OrbmRigFrame rig;
        std::vector<float> x[2], y[2], ang[2];
        std::vector<int32_t> oct[2], l2r, r2l, assign;      // assign: -2 = untouched, -1 = nulled by the rotation check
        std::vector<uint8_t> occ;
        explicit RigView(FrameT& F)
        {
            const int nl = F.Nleft, nr = F.N - F.Nleft;
            const std::vector<cv::KeyPoint>* keys[2] = {&F.mvKeys, &F.mvKeysRight};
            const int n[2] = {nl, nr};
            OrbmFrame* side[2] = {&rig.left, &rig.right};
            for (int s = 0; s < 2; s++) {
                x[s].resize(n[s]); y[s].resize(n[s]); ang[s].resize(n[s]); oct[s].resize(n[s]);
                for (int i = 0; i < n[s]; i++) {
                    const cv::KeyPoint& kp = (*keys[s])[i];
                    x[s][i] = kp.pt.x; y[s][i] = kp.pt.y; ang[s][i] = kp.angle; oct[s][i] = kp.octave;
                }
                OrbmFrame& f = *side[s];
                f.n = n[s]; f.x = x[s].data(); f.y = y[s].data(); f.octave = oct[s].data(); f.angle = ang[s].data();
                f.desc = F.mDescriptors.data + (s ? (size_t)nl * 32 : 0);
                f.min_x = F.mnMinX; f.min_y = F.mnMinY; f.max_x = F.mnMaxX; f.max_y = F.mnMaxY;
                f.grid_cols = FRAME_GRID_COLS; f.grid_rows = FRAME_GRID_ROWS;
                f.scale_factors = F.mvScaleFactors.data(); f.n_levels = (int)F.mvScaleFactors.size();
                f.u_right = NULL;
            }
            l2r.assign(F.mvLeftToRightMatch.begin(), F.mvLeftToRightMatch.begin() + nl);
            r2l.assign(F.mvRightToLeftMatch.begin(), F.mvRightToLeftMatch.begin() + nr);
            rig.left_to_right = l2r.data(); rig.right_to_left = r2l.data();
            assign.assign(std::max(F.N, 1), -2);
            occ.assign(std::max(F.N, 1), 0);
            for (int i = 0; i < F.N; i++) occ[i] = F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0;
            assign.resize(F.N); occ.resize(F.N);                // (the capacity stays: data() is an address even for an empty frame)
        }
    };

    float mfNNratio;
    bool mbCheckOrientation;
    ORBmatcherHIP conventional_;
    orbm_matcher* m_ = nullptr;
};

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
