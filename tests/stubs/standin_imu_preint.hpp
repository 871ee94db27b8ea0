// TEST INFRASTRUCTURE -- the members of the reference's IMU::Preintegrated and IMU::Point (include/ImuTypes.h:46-59, :210-250) that
// the pre-integration adapter (include/orbslam3_shim_preint.hpp) marshals and the stand-ins of standin_orbslam3.hpp lack: members
// only, no arithmetic.  Everything is public here; in the reference bu, db, mvMeasurements and mMutex are private, which is what the
// friend line of INTEGRATION.md 4k is for.
#pragma once
#include <mutex>
#include <vector>

#include "standin_orbslam3.hpp"

namespace ORB_SLAM3 {
namespace IMU {

// Eigen::DiagonalMatrix<float, 6> as far as the adapter uses it
struct PiDiagonal6 {
    Eigen::Matrix<float, 6, 1> d;
    Eigen::Matrix<float, 6, 1>& diagonal() { return d; }
    const Eigen::Matrix<float, 6, 1>& diagonal() const { return d; }
};

class PiPoint {
public:
    PiPoint(const Eigen::Vector3f& a_, const Eigen::Vector3f& w_, double t_) : a(a_), w(w_), t(t_) {}
    Eigen::Vector3f a, w;
    double t;
};

class PiPreintegrated {
public:
    float dT = 0;
    Eigen::Matrix<float, 15, 15> C, Info;
    PiDiagonal6 Nga, NgaWalk;
    Bias b;
    Eigen::Matrix3f dR;
    Eigen::Vector3f dV, dP;
    Eigen::Matrix3f JRg, JVg, JVa, JPg, JPa;
    Eigen::Vector3f avgA, avgW;
    Bias bu;
    Eigen::Matrix<float, 6, 1> db;
    struct integrable {
        integrable() {}
        integrable(const Eigen::Vector3f& a_, const Eigen::Vector3f& w_, const float& t_) : a(a_), w(w_), t(t_) {}
        Eigen::Vector3f a, w;
        float t;
    };
    std::vector<integrable> mvMeasurements;
    std::mutex mMutex;
};

}  // namespace IMU
}  // namespace ORB_SLAM3
