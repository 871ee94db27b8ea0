// TEST INFRASTRUCTURE -- what include/orbslam3_shim_fisheye.hpp reads and writes of a two-camera fisheye rig frame, added as
// classes of their own so that the stand-ins of standin_orbslam3.hpp and standin_kb8.hpp stay as they are: the camera with its
// Newton precision (include/CameraModels/KannalaBrandt8.h:42-59,102) and the rig members of Frame (include/Frame.h:102-103,255,294,
// 341-361).  Holds only what the adapter touches.
#pragma once
#include "standin_kb8.hpp"

namespace ORB_SLAM3 {

class KannalaBrandt8Rig : public KannalaBrandt8 {
public:
    explicit KannalaBrandt8Rig(const std::vector<float>& p, float precision_ = 1e-6f) : KannalaBrandt8(p), precision(precision_) {}
    float GetPrecision() { return precision; }

private:
    const float precision;
};

class RigFrame : public Frame {
public:
    Sophus::SE3f GetRelativePoseTlr() { return mTlr; }
    void ComputeStereoFishEyeMatches() { nReferenceCalls++; }      // the reference's own function: the adapter's fallback

    int Nright = -1, monoLeft = -1, monoRight = -1;
    int mnCloseMPs = -1;
    std::vector<float> mvLevelSigma2;
    std::vector<int> mvLeftToRightMatch, mvRightToLeftMatch;
    std::vector<Eigen::Vector3f> mvStereo3Dpoints;

    // toy state (not reference members)
    Sophus::SE3f mTlr;
    int nReferenceCalls = 0;
};

}  // namespace ORB_SLAM3
