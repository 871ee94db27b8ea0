// TEST INFRASTRUCTURE -- the members of the reference's KeyFrame that include/orbslam3_shim_mapping.hpp touches and the
// stand-in of standin_orbslam3.hpp lacks (include/KeyFrame.h: mvKeys, mvDepth, mb, invfx, invfy, mfScaleFactor), added by
// derivation so that the existing stand-in stays as it is.  The adapter takes the key-frame type as a template parameter.
#pragma once
#include "standin_orbslam3.hpp"

namespace ORB_SLAM3 {

class MappingKeyFrame : public KeyFrame {
public:
    std::vector<cv::KeyPoint> mvKeys;
    std::vector<float> mvDepth;
    float mb = 0, invfx = 0, invfy = 0, mfScaleFactor = 1.2f;
};

}  // namespace ORB_SLAM3
