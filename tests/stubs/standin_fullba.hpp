// TEST INFRASTRUCTURE -- the members of the reference's KeyFrame and Map that the FullInertialBA adapter
// (include/orbslam3_shim_fullba.hpp) touches and the stand-ins of standin_orbslam3.hpp lack (include/KeyFrame.h: mVwbGBA, mBiasGBA;
// include/Map.h: GetMaxKFid), added by derivation so that the existing stand-ins stay as they are.  The adapter takes its key-frame
// type from the map, as a template parameter; the map points keep observing base-class key-frame pointers.
#pragma once
#include "standin_orbslam3.hpp"

namespace ORB_SLAM3 {

class FbaKeyFrame : public KeyFrame {
public:
    void SetVelocity(const Eigen::Vector3f& v) { KeyFrame::SetVelocity(v); nVelocityWrites++; }
    void SetNewBias(const IMU::Bias& b) { KeyFrame::SetNewBias(b); nBiasWrites++; }
    Eigen::Vector3f mVwbGBA;
    IMU::Bias mBiasGBA;
    int nVelocityWrites = 0, nBiasWrites = 0;   // toy-map state
};

class FbaMap : public Map {
public:
    long unsigned int GetMaxKFid() { return mnMaxKFid; }
    std::vector<FbaKeyFrame*> GetAllKeyFrames() { return kfs; }
    std::vector<FbaKeyFrame*> kfs;
    long unsigned int mnMaxKFid = 0;
};

}  // namespace ORB_SLAM3
