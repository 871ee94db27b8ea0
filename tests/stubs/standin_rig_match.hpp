// TEST INFRASTRUCTURE -- what include/orbslam3_shim_rig_match.hpp reads of a rig frame and of a map point beyond the stand-ins of
// standin_orbslam3.hpp and standin_rig.hpp, added as derived classes so that those stay as they are: Frame::mvLeftToRightMatch /
// mvRightToLeftMatch (include/Frame.h:305) on top of RigPoseFrame's GetRelativePoseTrl, and the right-camera tracking members of
// MapPoint (include/MapPoint.h:142-160).  Holds only what the adapter touches.
#pragma once
#include "standin_rig.hpp"

namespace ORB_SLAM3 {

class RigMatchFrame : public RigPoseFrame {
public:
    std::vector<int> mvLeftToRightMatch, mvRightToLeftMatch;
};

class RigMatchMapPoint : public MapPoint {
public:
    float mTrackProjYR = 0, mTrackViewCosR = 0;
    int mnTrackScaleLevelR = 0;
};

}  // namespace ORB_SLAM3
