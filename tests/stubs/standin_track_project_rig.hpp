// TEST INFRASTRUCTURE -- what include/orbslam3_shim_track_project_rig.hpp reads of a rig frame and of a map point beyond the
// stand-ins of standin_rig_match.hpp, added as derived classes so that those stay as they are: Frame::mnId, mnScaleLevels,
// mfLogScaleFactor, mmProjectPoints, GetCameraCenter, GetRotationInverse, GetRelativePoseTlr_translation and isInFrustum
// (include/Frame.h:105-150, :280-305), MapPoint::mTrackDepthR, mnLastFrameSeen, IncreaseVisible and mMutexPos
// (include/MapPoint.h:137, :174, :181, :246).  Holds only what the adapter touches.
#pragma once
#include "standin_rig_match.hpp"

namespace ORB_SLAM3 {

class TrackProjectRigMapPoint : public RigMatchMapPoint {
public:
    void IncreaseVisible(int n = 1) { nVisible += n; }
    float mTrackDepthR = 0;
    long unsigned int mnLastFrameSeen = 0;
    std::mutex mMutexPos;
    int nVisible = 0;               // toy state
};

class TrackProjectRigFrame : public RigMatchFrame {
public:
    Eigen::Vector3f GetCameraCenter() { return mOw; }
    Eigen::Matrix3f GetRotationInverse() { return mRwc; }
    Eigen::Vector3f GetRelativePoseTlr_translation() { return mtlr; }
    bool isInFrustum(MapPoint* pMP, float) { nReferenceFrustum++; pMP->mbTrackInView = true; pMP->mTrackProjX = 7.f; pMP->mTrackProjY = 8.f; return true; }
    long unsigned int mnId = 0;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0;
    std::map<long unsigned int, cv::Point2f> mmProjectPoints;
    Eigen::Vector3f mOw, mtlr;      // toy state (private in the reference)
    Eigen::Matrix3f mRwc;
    int nReferenceFrustum = 0;
};

}  // namespace ORB_SLAM3
