// TEST INFRASTRUCTURE -- the fisheye camera class that include/orbslam3_shim_kb8.hpp reads its eight parameters from
// (include/CameraModels/KannalaBrandt8.h; getParameter is GeometricCamera's, include/CameraModels/GeometricCamera.h:84), added as
// a class of its own so that the stand-ins of standin_orbslam3.hpp stay as they are.  Holds only what the adapter touches.
#pragma once
#include "standin_orbslam3.hpp"

namespace ORB_SLAM3 {

class KannalaBrandt8 : public GeometricCamera {
public:
    explicit KannalaBrandt8(const std::vector<float>& p) : mvParameters(p) { mnType = CAM_FISHEYE; }
    float getParameter(const int i) { return mvParameters[i]; }
    Eigen::Vector2f project(const Eigen::Vector3f&) override { throw std::logic_error("the adapter never projects on the host"); }
    float uncertainty2(const Eigen::Matrix<double, 2, 1>&) override { return 1.0f; }
    Eigen::Matrix3f toK_() override { Eigen::Matrix3f K; K(0, 0) = mvParameters[0]; K(0, 2) = mvParameters[2]; K(1, 1) = mvParameters[1]; K(1, 2) = mvParameters[3]; K(2, 2) = 1.f; return K; }

private:
    std::vector<float> mvParameters;
};

}  // namespace ORB_SLAM3
