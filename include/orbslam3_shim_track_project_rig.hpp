// orbslam3_shim_track_project_rig.hpp -- drop-in adapter for the two projection steps of tracking with a two-camera KannalaBrandt8
// rig frame (Nleft != -1), on orbslam3_hip_track_project_rig.h:
//
//   the loop of Tracking::SearchLocalPoints over mvpLocalMapPoints                      src/Tracking.cc:3512-3530
//       (the Nleft != -1 branch of Frame::isInFrustum, src/Frame.cc:662-672, with isInFrustumChecks for both cameras)
//   the projection loop of SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)     src/ORBmatcher.cc:1695-1718, :1794-1796
//
// Frame::isInFrustum of a rig frame resets only the two flags and the two levels of a map point: a camera that does not see the point
// leaves mTrackProjX/Y, mTrackViewCos and mTrackDepth (or their R twins) as an EARLIER frame wrote them, and the search reads
// mTrackDepth even when only the right camera sees the point.  So those eight members travel IN and out of the call.
// Frames that are no rig frames go to the owned TrackProjectHIP.  The frame and map-point types are template parameters, as there;
// MapPoint needs the same one line, `friend struct TrackProjectAccess;`.
#pragma once

#include "orbslam3_shim_track_project.hpp"
#include "orbslam3_shim_rig_match.hpp"
#include "orbslam3_hip_track_project_rig.h"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

namespace ORB_SLAM3 {

namespace track_project_detail {

// mpCamera / mpCamera2 (KannalaBrandt8: fx fy cx cy k0..k3), mTrl, mTlr's translation, the bounds and the pyramid of a rig frame
template <class FrameT>
inline OrbmTrackRigCamera rig_camera(FrameT& F)
{
    OrbmTrackRigCamera C;
    for (int k = 0; k < 8; k++) {
        C.left[k] = static_cast<KannalaBrandt8*>(F.mpCamera)->getParameter(k);
        C.right[k] = static_cast<KannalaBrandt8*>(F.mpCamera2)->getParameter(k);
    }
    const Sophus::SE3f Trl = F.GetRelativePoseTrl();
    const Eigen::Matrix3f Rrl = Trl.rotationMatrix();
    const Eigen::Quaternionf q = Trl.unit_quaternion();
    const Eigen::Vector3f trl = Trl.translation(), tlr = F.GetRelativePoseTlr_translation();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) C.Rrl[3 * r + c] = Rrl(r, c);
        C.trl[r] = trl(r); C.tlr[r] = tlr(r);
    }
    C.q_rl[0] = q.x(); C.q_rl[1] = q.y(); C.q_rl[2] = q.z(); C.q_rl[3] = q.w();
    C.min_x = F.mnMinX; C.min_y = F.mnMinY; C.max_x = F.mnMaxX; C.max_y = F.mnMaxY;
    C.log_scale_factor = F.mfLogScaleFactor; C.n_levels = F.mnScaleLevels;
    return C;
}

// the rig record from what Frame::UpdatePoseMatrices left in the frame, with the reference's own expressions for the right camera
// (src/Frame.cc:1294-1299)
template <class FrameT>
inline OrbmRigFramePose rig_frame_pose(FrameT& F)
{
    OrbmRigFramePose P;
    P.left = frame_pose(F);
    const Sophus::SE3f Tcw = F.GetPose(), Trl = F.GetRelativePoseTrl();
    const Eigen::Matrix3f Rwc = F.GetRotationInverse(), Rrl = Trl.rotationMatrix();
    const Eigen::Matrix3f mR = Rrl * Tcw.rotationMatrix();
    const Eigen::Vector3f mt = Rrl * Tcw.translation() + Trl.translation();
    const Eigen::Vector3f twc = Rwc * F.GetRelativePoseTlr_translation() + F.GetCameraCenter();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) { P.Rwc[3 * r + c] = Rwc(r, c); P.R_r[3 * r + c] = mR(r, c); }
        P.t_r[r] = mt(r); P.Ow_r[r] = twc(r);
    }
    return P;
}

}  // namespace track_project_detail

template <class FrameT = Frame, class MapPointT = MapPoint>
class TrackProjectRigHIP {
public:
    TrackProjectRigHIP(float nnratio = 0.9, bool checkOri = true) : pinhole_(nnratio, checkOri), rig_matcher_(nnratio, checkOri) { orbslam3_hip::check(orbm_create(0, &m_)); }
    ~TrackProjectRigHIP() { orbm_destroy(m_); }
    TrackProjectRigHIP(const TrackProjectRigHIP&) = delete;
    TrackProjectRigHIP& operator=(const TrackProjectRigHIP&) = delete;

    TrackProjectHIP<FrameT, MapPointT>& pinhole() { return pinhole_; }
    ORBmatcherRigHIP<FrameT, MapPointT>& matcher() { return rig_matcher_; }

    // The loop :3512-3530 of Tracking::SearchLocalPoints for a rig frame.  Of every point the reference would have passed to isInFrustum
    // it writes mbTrackInView(R) and mnTrackScaleLevel(R), and for a camera that sees the point mTrackProjX/Y, mTrackViewCos and
    // mTrackDepth (or the R twins); calls IncreaseVisible where either camera sees it, fills mmProjectPoints from the left camera, and
    // returns nToMatch.  Points the loop skips (seen in this frame, bad) are left alone.
    int SearchLocalPointsProjectHIP(Frame& F_, const std::vector<MapPoint*>& vpLocalMapPoints, float viewingCosLimit)
    {
        if (F_.Nleft == -1) return pinhole_.SearchLocalPointsProjectHIP(F_, vpLocalMapPoints, viewingCosLimit);
        FrameT& F = static_cast<FrameT&>(F_);
        const int n = (int)vpLocalMapPoints.size();
        if (n == 0) return 0;
        std::vector<float> xyz((size_t)n * 3), normal((size_t)n * 3), mind(n), maxd(n);
        std::vector<float> u(n), v(n), vcos(n), depth(n), uR(n), vR(n), vcosR(n), depthR(n);
        std::vector<uint8_t> skip(n), bad(n), seen(n), seenR(n);
        std::vector<int32_t> level(n), levelR(n);
        for (int i = 0; i < n; i++) {
            MapPointT* pMP = static_cast<MapPointT*>(vpLocalMapPoints[i]);
            const Eigen::Vector3f P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
            for (int k = 0; k < 3; k++) { xyz[(size_t)i * 3 + k] = P(k); normal[(size_t)i * 3 + k] = Pn(k); }
            TrackProjectAccess::distances(pMP, mind[i], maxd[i]);
            skip[i] = pMP->mnLastFrameSeen == F.mnId; bad[i] = pMP->isBad();
            // the stale members, in
            seen[i] = pMP->mbTrackInView; u[i] = pMP->mTrackProjX; v[i] = pMP->mTrackProjY; level[i] = pMP->mnTrackScaleLevel; vcos[i] = pMP->mTrackViewCos; depth[i] = pMP->mTrackDepth;
            seenR[i] = pMP->mbTrackInViewR; uR[i] = pMP->mTrackProjXR; vR[i] = pMP->mTrackProjYR; levelR[i] = pMP->mnTrackScaleLevelR; vcosR[i] = pMP->mTrackViewCosR;
            depthR[i] = pMP->mTrackDepthR;
        }
        const OrbmTrackRigCamera cam = track_project_detail::rig_camera(F);
        const OrbmRigFramePose pose = track_project_detail::rig_frame_pose(F);
        int32_t n_rows = n, nToMatch = 0;
        OrbmLocalPoints pts;
        pts.xyz = xyz.data(); pts.normal = normal.data(); pts.min_distance = mind.data(); pts.max_distance = maxd.data();
        pts.skip = skip.data(); pts.bad = bad.data(); pts.n = &n_rows; pts.pcap = n;
        OrbmRigFrustumOut out;
        out.in_view = seen.data(); out.proj_u = u.data(); out.proj_v = v.data(); out.pred_level = level.data(); out.view_cos = vcos.data();
        out.in_view_r = seenR.data(); out.proj_u_r = uR.data(); out.proj_v_r = vR.data(); out.pred_level_r = levelR.data(); out.view_cos_r = vcosR.data();
        out.track_depth = depth.data(); out.track_depth_r = depthR.data(); out.n_to_match = &nToMatch;
        orbslam3_hip::check(orbm_frustum_rig_batch(m_, &cam, &pose, &pts, viewingCosLimit, &out, 1));
        for (int i = 0; i < n; i++) {
            if (skip[i] || bad[i]) continue;            // :3516-3519: isInFrustum was never called
            MapPointT* pMP = static_cast<MapPointT*>(vpLocalMapPoints[i]);
            // the stale members, out: the library left the arrays of a camera that does not see the point as they came in
            pMP->mbTrackInView = seen[i] != 0; pMP->mTrackProjX = u[i]; pMP->mTrackProjY = v[i]; pMP->mnTrackScaleLevel = level[i]; pMP->mTrackViewCos = vcos[i];
            pMP->mTrackDepth = depth[i];
            pMP->mbTrackInViewR = seenR[i] != 0; pMP->mTrackProjXR = uR[i]; pMP->mTrackProjYR = vR[i]; pMP->mnTrackScaleLevelR = levelR[i]; pMP->mTrackViewCosR = vcosR[i];
            pMP->mTrackDepthR = depthR[i];
            if (seen[i] || seenR[i]) pMP->IncreaseVisible();
            if (seen[i]) F.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
        }
        return nToMatch;
    }

    // SearchByProjection(CurrentFrame, LastFrame, th, bMono) of a rig frame with the projection loop made by orbm_project_last_rig_batch;
    // the rest is the owned ORBmatcherRigHIP's (SearchByProjectionProjected).
    int SearchByProjection(Frame& CurrentFrame_, const Frame& LastFrame, const float th, const bool bMono)
    {
        if (CurrentFrame_.Nleft == -1) return pinhole_.SearchByProjection(CurrentFrame_, LastFrame, th, bMono);
        FrameT& CurrentFrame = static_cast<FrameT&>(CurrentFrame_);
        const int nL = LastFrame.N, rows = std::max(nL, 1);
        const Sophus::SE3f Tcw = CurrentFrame.GetPose();                           // :1686-1693
        const Eigen::Vector3f twc = Tcw.inverse().translation();
        const Eigen::Vector3f tlc = LastFrame.GetPose() * twc;
        const bool bForward = tlc(2) > CurrentFrame.mb && !bMono;
        const bool bBackward = -tlc(2) > CurrentFrame.mb && !bMono;
        const int levelWindow = bForward ? ORBM_LEVELS_FORWARD : bBackward ? ORBM_LEVELS_BACKWARD : ORBM_LEVELS_AROUND;
        std::vector<float> xyz((size_t)rows * 3, 0.f), u(rows, 0.f), v(rows, 0.f), uR(rows, 0.f), vR(rows, 0.f);
        std::vector<uint8_t> has(rows, 0), valid(rows, 0);
        for (int i = 0; i < nL; i++) {
            MapPoint* p = LastFrame.mvpMapPoints[i];
            if (!p || LastFrame.mvbOutlier[i]) continue;
            has[i] = 1;
            const Eigen::Vector3f x3Dw = p->GetWorldPos();
            for (int k = 0; k < 3; k++) xyz[(size_t)i * 3 + k] = x3Dw(k);
        }
        const OrbmTrackRigCamera cam = track_project_detail::rig_camera(CurrentFrame);
        const OrbmRigFramePose pose = track_project_detail::rig_frame_pose(CurrentFrame);
        const int32_t n_rows = nL;
        OrbmRigLastProjOut out;
        out.valid = valid.data(); out.proj_u = u.data(); out.proj_v = v.data(); out.proj_u_r = uR.data(); out.proj_v_r = vR.data();
        orbslam3_hip::check(orbm_project_last_rig_batch(m_, &cam, &pose, xyz.data(), has.data(), &n_rows, rows, &out, 1));
        return rig_matcher_.SearchByProjectionProjected(CurrentFrame, LastFrame, th, levelWindow, valid.data(), u.data(), v.data(), uR.data(), vR.data());
    }

private:
    TrackProjectHIP<FrameT, MapPointT> pinhole_;
    ORBmatcherRigHIP<FrameT, MapPointT> rig_matcher_;
    orbm_matcher* m_ = nullptr;
};

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
