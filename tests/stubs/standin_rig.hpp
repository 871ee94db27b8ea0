// TEST INFRASTRUCTURE -- what include/orbslam3_shim_rig.hpp reads of a two-camera fisheye rig beyond the stand-ins of
// standin_orbslam3.hpp and standin_kb8.hpp, added as derived classes so that those stay as they are: Frame::GetRelativePoseTrl
// (include/Frame.h:341-361), KeyFrame::mvKeysRight and KeyFrame::GetRelativePoseTrl (include/KeyFrame.h).  Holds only what the adapter touches.
#pragma once
#include "standin_kb8.hpp"

namespace ORB_SLAM3 {

class RigPoseFrame : public Frame {
public:
    Sophus::SE3f GetRelativePoseTrl() { return mTrl; }
    Sophus::SE3f mTrl;          // toy state (mTrl is private in the reference)
};

class RigKeyFrame : public KeyFrame {
public:
    Sophus::SE3f GetRelativePoseTrl() { return mTrl; }
    std::vector<cv::KeyPoint> mvKeysRight;
    Sophus::SE3f mTrl;
};

}  // namespace ORB_SLAM3
