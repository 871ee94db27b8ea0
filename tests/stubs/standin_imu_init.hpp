// TEST INFRASTRUCTURE -- the members of the reference's KeyFrame, Map and IMU::Preintegrated that the IMU-initialisation adapter
// (include/orbslam3_shim_imu_init.hpp) touches and the stand-ins of standin_orbslam3.hpp lack (include/ImuTypes.h:
// Preintegrated::Reintegrate; include/Map.h: GetMaxKFid), added by derivation so that the existing stand-ins stay as they are.
// The derived key frame re-declares mPrevKF and mpImuPreintegrated with the derived types (the adapter takes its types from the
// map, as template parameters); everything else is the base stand-in's.
#pragma once
#include "standin_orbslam3.hpp"

namespace ORB_SLAM3 {

class ImiPreintegrated : public IMU::Preintegrated {
public:
    void Reintegrate() { nReintegrated++; }
    int nReintegrated = 0;      // toy-map state
};

class ImiKeyFrame : public KeyFrame {
public:
    void SetVelocity(const Eigen::Vector3f& v) { KeyFrame::SetVelocity(v); nVelocityWrites++; }
    void SetNewBias(const IMU::Bias& b) { KeyFrame::SetNewBias(b); nBiasWrites++; }
    ImiKeyFrame* mPrevKF = nullptr;
    ImiPreintegrated* mpImuPreintegrated = nullptr;
    int nVelocityWrites = 0, nBiasWrites = 0;   // toy-map state
};

class ImiMap : public Map {
public:
    long unsigned int GetMaxKFid() { return mnMaxKFid; }
    std::vector<ImiKeyFrame*> GetAllKeyFrames() { return kfs; }
    std::vector<ImiKeyFrame*> kfs;
    long unsigned int mnMaxKFid = 0;
};

}  // namespace ORB_SLAM3
