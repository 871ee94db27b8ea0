// TEST INFRASTRUCTURE -- what include/orbslam3_shim_rig_map.hpp reads of a rig key frame and of the reference's matcher beyond the
// stand-ins of standin_orbslam3.hpp, standin_rig.hpp, standin_rig_match.hpp and standin_fisheye.hpp, added as derived classes so that
// those stay as they are: KeyFrame::mvKeys, GetRightPose, GetRightPoseInverse and GetRightCameraCenter (include/KeyFrame.h) on top of
// RigKeyFrame's mvKeysRight, and the two SearchByBoW overloads of ORBmatcher (include/ORBmatcher.h:61-62).  Holds only what the
// adapter touches.
#pragma once
#include "standin_fisheye.hpp"
#include "standin_rig_match.hpp"

namespace ORB_SLAM3 {

class RigMapKeyFrame : public RigKeyFrame {
public:
    Sophus::SE3f GetRightPose() { return mTrl * mTcw; }                 // src/KeyFrame.cc:1069-1073
    Sophus::SE3f GetRightPoseInverse() { return (mTrl * mTcw).inverse(); }
    Eigen::Vector3f GetRightCameraCenter() { return (mTrl * mTcw).inverse().translation(); }
    std::vector<cv::KeyPoint> mvKeys;
};

class RigMapReference : public ORBmatcher {
public:
    RigMapReference(float nnratio = 0.6, bool checkOri = true) : ORBmatcher(nnratio, checkOri) {}
    int SearchByBoW(KeyFrame* pKF, Frame& F, std::vector<MapPoint*>& vpMapPointMatches);
    int SearchByBoW(KeyFrame* pKF1, KeyFrame* pKF2, std::vector<MapPoint*>& vpMatches12);
};

}  // namespace ORB_SLAM3
