// TEST INFRASTRUCTURE -- what include/orbslam3_shim_track_project.hpp reads of a frame and of a map point beyond the stand-ins of
// standin_orbslam3.hpp, added as derived classes so that those stay as they are: Frame::mnId, mnScaleLevels, mfLogScaleFactor,
// mmProjectPoints, GetCameraCenter and isInFrustum (include/Frame.h:111, :143, :280-305), MapPoint::mnLastFrameSeen, IncreaseVisible
// and mMutexPos (include/MapPoint.h:137, :181, :246).  Holds only what the adapter touches.
#pragma once
#include "standin_orbslam3.hpp"

namespace ORB_SLAM3 {

class TrackProjectMapPoint : public MapPoint {
public:
    void IncreaseVisible(int n = 1) { nVisible += n; }
    long unsigned int mnLastFrameSeen = 0;
    std::mutex mMutexPos;
    int nVisible = 0;               // toy state
};

class TrackProjectFrame : public Frame {
public:
    Eigen::Vector3f GetCameraCenter() { return mOw; }
    bool isInFrustum(MapPoint* pMP, float) { nReferenceFrustum++; pMP->mbTrackInView = true; pMP->mTrackProjX = 7.f; pMP->mTrackProjY = 8.f; return true; }
    long unsigned int mnId = 0;
    int mnScaleLevels = 0;
    float mfLogScaleFactor = 0;
    std::map<long unsigned int, cv::Point2f> mmProjectPoints;
    Eigen::Vector3f mOw;            // toy state (private in the reference)
    int nReferenceFrustum = 0;
};

}  // namespace ORB_SLAM3
