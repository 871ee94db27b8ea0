// TEST INFRASTRUCTURE -- what include/orbslam3_shim_rig_mapping.hpp reads of a key frame beyond the stand-ins of
// standin_rig_map.hpp (mvKeys, mvKeysRight, the right pose and centre): the members of include/KeyFrame.h that the conventional
// route needs as well (mvDepth, mb, invfx, invfy, mfScaleFactor), added by derivation so that the existing stand-ins stay as they are.
#pragma once
#include "standin_rig_map.hpp"

namespace ORB_SLAM3 {

class RigMappingKeyFrame : public RigMapKeyFrame {
public:
    std::vector<float> mvDepth;
    float mb = 0, invfx = 0, invfy = 0, mfScaleFactor = 1.2f;
};

}  // namespace ORB_SLAM3
