// orbslam3_shim_track_project.hpp -- drop-in adapters for the two projection steps of tracking (orbslam3_hip_track_project.h):
//
//   the loop of Tracking::SearchLocalPoints over mvpLocalMapPoints                      src/Tracking.cc:3512-3530
//       (Frame::isInFrustum, src/Frame.cc:599-661, with IncreaseVisible and mmProjectPoints)
//   the projection loop of SearchByProjection(Frame& CurrentFrame, const Frame& LastFrame, th, bMono)     src/ORBmatcher.cc:1695-1718
//
// Pinhole frames (Nleft == -1) only: a rig frame goes to the reference.  The frame and map-point types are template parameters (Frame
// and MapPoint in the reference tree; derived stand-ins in the typed tests).  MapPoint::mfMinDistance / mfMaxDistance and mMutexPos are
// protected: every access is in TrackProjectAccess below, so MapPoint needs one line, `friend struct TrackProjectAccess;`.
#pragma once

#include "orbslam3_shim.hpp"
#include "orbslam3_hip_track_project.h"

#ifdef ORBSLAM3_HIP_WITH_REFERENCE

namespace ORB_SLAM3 {

struct TrackProjectAccess {
    template <class MapPointT>
    static void distances(MapPointT* p, float& min_distance, float& max_distance)        // raw: the library applies 0.8f / 1.2f itself
    {
        std::unique_lock<std::mutex> lock(p->mMutexPos);
        min_distance = p->mfMinDistance; max_distance = p->mfMaxDistance;
    }
};

namespace track_project_detail {

// what Frame::UpdatePoseMatrices left in the frame (src/Frame.cc:559-566): mTcw, mRcw = mTcw.rotationMatrix(), mtcw, mOw
template <class FrameT>
inline OrbmFramePose frame_pose(FrameT& F)
{
    OrbmFramePose P;
    const Sophus::SE3f Tcw = F.GetPose();
    const Eigen::Quaternionf q = Tcw.unit_quaternion();
    const Eigen::Matrix3f R = Tcw.rotationMatrix();
    const Eigen::Vector3f t = Tcw.translation(), Ow = F.GetCameraCenter();
    P.q[0] = q.x(); P.q[1] = q.y(); P.q[2] = q.z(); P.q[3] = q.w();
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) P.Rcw[3 * r + c] = R(r, c);
        P.tcw[r] = t(r); P.Ow[r] = Ow(r);
    }
    return P;
}

template <class FrameT>
inline OrbmTrackCamera camera(FrameT& F)
{
    OrbmTrackCamera C;
    C.fx = F.fx; C.fy = F.fy; C.cx = F.cx; C.cy = F.cy; C.bf = F.mbf;
    C.min_x = F.mnMinX; C.min_y = F.mnMinY; C.max_x = F.mnMaxX; C.max_y = F.mnMaxY;
    C.log_scale_factor = F.mfLogScaleFactor; C.n_levels = F.mnScaleLevels;
    return C;
}

}  // namespace track_project_detail

template <class FrameT = Frame, class MapPointT = MapPoint>
class TrackProjectHIP {
public:
    TrackProjectHIP(float nnratio = 0.9, bool checkOri = true) : matcher_(nnratio, checkOri) { orbslam3_hip::check(orbm_create(0, &m_)); }
    ~TrackProjectHIP() { orbm_destroy(m_); }
    TrackProjectHIP(const TrackProjectHIP&) = delete;
    TrackProjectHIP& operator=(const TrackProjectHIP&) = delete;

    ORBmatcherHIP& matcher() { return matcher_; }

    // The loop :3512-3530 of Tracking::SearchLocalPoints.  Writes mbTrackInView, mTrackProjX, mTrackProjY, mTrackProjXR, mTrackDepth,
    // mnTrackScaleLevel and mTrackViewCos of every point the reference would have passed to isInFrustum, calls IncreaseVisible where it
    // returned true, fills mmProjectPoints, and returns nToMatch.  Points the loop skips (seen in this frame, bad) are left alone.
    int SearchLocalPointsProjectHIP(Frame& F_, const std::vector<MapPoint*>& vpLocalMapPoints, float viewingCosLimit)
    {
        FrameT& F = static_cast<FrameT&>(F_);
        const int n = (int)vpLocalMapPoints.size();
        if (F.Nleft != -1) {                            // a rig frame: the reference's loop
            int nToMatch = 0;
            for (MapPoint* p_ : vpLocalMapPoints) {
                MapPointT* pMP = static_cast<MapPointT*>(p_);
                if (pMP->mnLastFrameSeen == F.mnId) continue;
                if (pMP->isBad()) continue;
                if (F.isInFrustum(pMP, viewingCosLimit)) { pMP->IncreaseVisible(); nToMatch++; }
                if (pMP->mbTrackInView) F.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
            }
            return nToMatch;
        }
        if (n == 0) return 0;
        std::vector<float> xyz((size_t)n * 3), normal((size_t)n * 3), mind(n), maxd(n), u(n), v(n), vcos(n), depth(n), ur(n);
        std::vector<uint8_t> skip(n), bad(n), valid(n);
        std::vector<int32_t> level(n);
        for (int i = 0; i < n; i++) {
            MapPointT* pMP = static_cast<MapPointT*>(vpLocalMapPoints[i]);
            const Eigen::Vector3f P = pMP->GetWorldPos(), Pn = pMP->GetNormal();
            for (int k = 0; k < 3; k++) { xyz[(size_t)i * 3 + k] = P(k); normal[(size_t)i * 3 + k] = Pn(k); }
            TrackProjectAccess::distances(pMP, mind[i], maxd[i]);
            skip[i] = pMP->mnLastFrameSeen == F.mnId; bad[i] = pMP->isBad();
        }
        const OrbmTrackCamera cam = track_project_detail::camera(F);
        const OrbmFramePose pose = track_project_detail::frame_pose(F);
        int32_t n_rows = n, nToMatch = 0;
        OrbmLocalPoints pts;
        pts.xyz = xyz.data(); pts.normal = normal.data(); pts.min_distance = mind.data(); pts.max_distance = maxd.data();
        pts.skip = skip.data(); pts.bad = bad.data(); pts.n = &n_rows; pts.pcap = n;
        OrbmFrustumOut out;
        out.valid = valid.data(); out.u = u.data(); out.v = v.data(); out.octave = level.data(); out.view_cos = vcos.data();
        out.track_depth = depth.data(); out.proj_ur = ur.data(); out.n_to_match = &nToMatch;
        orbslam3_hip::check(orbm_frustum_batch(m_, &cam, &pose, &pts, viewingCosLimit, &out, 1));
        for (int i = 0; i < n; i++) {
            if (skip[i] || bad[i]) continue;            // :3516-3519: isInFrustum was never called
            MapPointT* pMP = static_cast<MapPointT*>(vpLocalMapPoints[i]);
            pMP->mbTrackInView = valid[i] != 0;
            pMP->mTrackProjX = u[i]; pMP->mTrackProjY = v[i];
            if (valid[i]) {                             // :650-658
                pMP->mTrackProjXR = ur[i]; pMP->mTrackDepth = depth[i]; pMP->mnTrackScaleLevel = level[i]; pMP->mTrackViewCos = vcos[i];
                pMP->IncreaseVisible();
                F.mmProjectPoints[pMP->mnId] = cv::Point2f(pMP->mTrackProjX, pMP->mTrackProjY);
            }
        }
        return nToMatch;
    }

    // SearchByProjection(CurrentFrame, LastFrame, th, bMono) with the projection loop :1695-1718 made by orbm_project_last_batch; the
    // rest is the owned ORBmatcherHIP's (SearchByProjectionProjected).  Rig frames go there whole, and from there to the reference.
    int SearchByProjection(Frame& CurrentFrame_, const Frame& LastFrame, const float th, const bool bMono)
    {
        if (CurrentFrame_.Nleft != -1 || LastFrame.Nleft != -1) return matcher_.SearchByProjection(CurrentFrame_, LastFrame, th, bMono);
        FrameT& CurrentFrame = static_cast<FrameT&>(CurrentFrame_);
        const int nL = LastFrame.N, rows = std::max(nL, 1);
        std::vector<float> xyz((size_t)rows * 3, 0.f), u(rows, 0.f), v(rows, 0.f), ur(rows, 0.f);
        std::vector<uint8_t> has(rows, 0), valid(rows, 0);
        for (int i = 0; i < nL; i++) {
            MapPoint* p = LastFrame.mvpMapPoints[i];
            if (!p || LastFrame.mvbOutlier[i]) continue;
            has[i] = 1;
            const Eigen::Vector3f x3Dw = p->GetWorldPos();
            for (int k = 0; k < 3; k++) xyz[(size_t)i * 3 + k] = x3Dw(k);
        }
        const OrbmTrackCamera cam = track_project_detail::camera(CurrentFrame);
        const OrbmFramePose pose = track_project_detail::frame_pose(CurrentFrame);
        const int32_t n_rows = nL;
        OrbmLastProjOut out;
        out.valid = valid.data(); out.u = u.data(); out.v = v.data(); out.proj_ur = ur.data();
        orbslam3_hip::check(orbm_project_last_batch(m_, &cam, &pose, xyz.data(), has.data(), &n_rows, rows, &out, 1));
        return matcher_.SearchByProjectionProjected(CurrentFrame, LastFrame, th, bMono, valid.data(), u.data(), v.data(), ur.data());
    }

private:
    ORBmatcherHIP matcher_;
    orbm_matcher* m_ = nullptr;
};

}  // namespace ORB_SLAM3

#endif  // ORBSLAM3_HIP_WITH_REFERENCE
