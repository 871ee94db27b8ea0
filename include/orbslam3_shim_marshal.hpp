// orbslam3_shim_marshal.hpp -- the marshalling every drop-in adapter of orbslam3_shim*.hpp shares: the solver handle of the calling
// thread, poses and calibrations between the reference's float types and the C ABI's doubles, one pre-integration as a LibaLink,
// one observation as an edge record, key points, descriptors and a fisheye rig as the C ABI reads them, the Huber deltas, the LbaProblem of a
// flattened window.
// Included by orbslam3_shim.hpp, after orbslam3_hip::check and the reference's headers (Eigen, Sophus, cv::KeyPoint): include that
// header, not this one.  Whatever touches a reference class takes it as a template parameter, so that the helpers serve the
// adapters that are templates themselves (orbslam3_shim_fullba.hpp, orbslam3_shim_imu_init.hpp) and compile against stand-in types.
// A problem struct holds raw pointers: a helper that returns one takes the arrays by reference, from an owner that has to outlive
// the solve -- never hand it a temporary.
#pragma once

#include <cmath>
#include <cstring>
#include <vector>

namespace orbslam3_hip {

// The one handle of a solver type on the calling thread, created on first use: a handle owns one stream and must not be shared
// between threads (orbslam3_hip.h).  Adapters that name the same Create share the handle.
template <class T, int (*Create)(int, T**)>
inline T* thread_handle()
{
    static thread_local T* h = nullptr;
    if (!h) check(Create(0, &h));
    return h;
}

// Sets a KannalaBrandt8 camera (or a rig of two: RigScope) on a handle for the lifetime of the object; with cam == nullptr nothing is set and the handle keeps
// its pinhole model.  The reset must happen on every way out (check() throws).
template <class Handle, class Cam, int (*Set)(Handle*, const Cam*)>
struct CameraScopeOf {
    Handle* h;
    CameraScopeOf(Handle* h_, const Cam* cam) : h(cam ? h_ : nullptr) { if (h) check(Set(h, cam)); }
    ~CameraScopeOf() { if (h) (void)Set(h, nullptr); }
    CameraScopeOf(const CameraScopeOf&) = delete;
    CameraScopeOf& operator=(const CameraScopeOf&) = delete;
};
template <class Handle, int (*Set)(Handle*, const OrbxKB8*)>
using CameraScope = CameraScopeOf<Handle, OrbxKB8, Set>;            // one KannalaBrandt8 camera (*_set_camera_kb8)
template <class Handle, int (*Set)(Handle*, const OrbxKB8Rig*)>
using RigScope = CameraScopeOf<Handle, OrbxKB8Rig, Set>;            // a rig of two (*_set_rig_kb8)

// Tcw -> q[4] (x y z w), t[3]: cast to double component by component, as g2o::SE3Quat is built from the float pose
inline void pose_in(const Sophus::SE3f& Tcw, double* q, double* t)
{
    const Eigen::Quaterniond qd = Tcw.unit_quaternion().cast<double>();
    const Eigen::Vector3d td = Tcw.translation().cast<double>();
    q[0] = qd.x(); q[1] = qd.y(); q[2] = qd.z(); q[3] = qd.w();
    t[0] = td.x(); t[1] = td.y(); t[2] = td.z();
}
inline Sophus::SE3f pose_out(const double* q, const double* t)
{
    const Eigen::Quaterniond qd(q[3], q[0], q[1], q[2]);
    return Sophus::SE3f(qd.cast<float>(), Eigen::Vector3d(t[0], t[1], t[2]).cast<float>());
}

inline Eigen::Vector3f point_out(const double* X) { return Eigen::Vector3d(X[0], X[1], X[2]).cast<float>(); }

template <class M>
inline void put3x3(const M& m, double* dst) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) dst[3 * r + c] = m(r, c); }

// IMU::Calib -> Rcb[9] (row major), tcb[3], tbc[3]
template <class Calib>
inline void imu_calib(const Calib& calib, double* Rcb, double* tcb, double* tbc)
{
    const Eigen::Matrix3d R = calib.mTcb.rotationMatrix().template cast<double>();
    const Eigen::Vector3d c = calib.mTcb.translation().template cast<double>(), b = calib.mTbc.translation().template cast<double>();
    put3x3(R, Rcb);
    for (int r = 0; r < 3; r++) { tcb[r] = c[r]; tbc[r] = b[r]; }
}

// ImuCamPose: the camera pose of a body pose, Rcw = Rcb Rbw, tcw = Rcb tbw + tcb
inline Sophus::SE3f camera_pose(const double* Rcb_, const double* tcb_, const double* Rwb, const double* twb)
{
    Eigen::Matrix3d Rcb, R;
    Eigen::Vector3d tcb, t;
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) { Rcb(r, c) = Rcb_[3 * r + c]; R(r, c) = Rwb[3 * r + c]; } tcb[r] = tcb_[r]; t[r] = twb[r]; }
    const Eigen::Matrix3d Rcw = Rcb * R.transpose();
    const Eigen::Vector3d tcw = Rcb * (-R.transpose() * t) + tcb;
    return Sophus::SE3f(Rcw.cast<float>(), tcw.cast<float>());
}

// One IMU::Preintegrated between the slots kf1 -> kf2 as a LibaLink: the pre-integrated terms, the original bias, and the
// EdgeInertial information of its constructor (G2oTypes.cc:510-518, EdgeInertialGS :604-612): C's 9 x 9 block cast to double,
// inverted, symmetrised, eigenvalues below 1e-12 set to 0; info_scale is the factor 1e-2 of Optimizer.cc:2651.
// random_walk_from = the pre-integration whose C gives the EdgeGyroRW / EdgeAccRW informations; nullptr leaves them zero.
template <class Pre>
inline LibaLink imu_link(Pre* pInt, int kf1, int kf2, double info_scale, decltype(pInt) random_walk_from, bool robust)
{
    LibaLink L;
    std::memset(&L, 0, sizeof(L));
    L.kf1 = kf1; L.kf2 = kf2;
    auto put = [](float* dst, const Eigen::Matrix3f& M) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) dst[3 * r + c] = M(r, c); };
    put(L.dR, pInt->dR); put(L.JRg, pInt->JRg); put(L.JVg, pInt->JVg); put(L.JVa, pInt->JVa); put(L.JPg, pInt->JPg); put(L.JPa, pInt->JPa);
    for (int r = 0; r < 3; r++) { L.dV[r] = pInt->dV(r); L.dP[r] = pInt->dP(r); }
    L.dT = pInt->dT;
    const auto b = pInt->GetOriginalBias();
    L.bias0[0] = b.bax; L.bias0[1] = b.bay; L.bias0[2] = b.baz; L.bias0[3] = b.bwx; L.bias0[4] = b.bwy; L.bias0[5] = b.bwz;
    Eigen::Matrix<double, 9, 9> Info = pInt->C.template block<9, 9>(0, 0).template cast<double>().inverse();
    Info = (Info + Info.transpose()) / 2;
    Eigen::SelfAdjointEigenSolver<Eigen::Matrix<double, 9, 9> > es(Info);
    Eigen::Matrix<double, 9, 1> eigs = es.eigenvalues();
    for (int k = 0; k < 9; k++) if (eigs[k] < 1e-12) eigs[k] = 0;
    Info = es.eigenvectors() * eigs.asDiagonal() * es.eigenvectors().transpose();
    Info *= info_scale;
    for (int r = 0; r < 9; r++) for (int c = 0; c < 9; c++) L.info9[9 * r + c] = Info(r, c);
    if (random_walk_from) {
        const Eigen::Matrix3d InfoG = random_walk_from->C.template block<3, 3>(9, 9).template cast<double>().inverse();
        const Eigen::Matrix3d InfoA = random_walk_from->C.template block<3, 3>(12, 12).template cast<double>().inverse();
        put3x3(InfoG, L.info_gyro); put3x3(InfoA, L.info_acc);
    }
    L.robust = robust;
    return L;
}

// one observation as an edge record: x, y, and the right coordinate of a stereo observation (mvuRight >= 0), else -1
inline void push_edge_obs(const cv::KeyPoint& kpUn, float ur, std::vector<double>& obs, std::vector<uint8_t>& stereo)
{
    obs.push_back(kpUn.pt.x); obs.push_back(kpUn.pt.y); obs.push_back(ur >= 0 ? (double)ur : -1.0);
    stereo.push_back(ur >= 0);
}

// mvKeys as the C ABI's key points: cv::KeyPoint has OrbxKeyPoint's layout (orbslam3_hip.h), so the vector is read in place
inline const OrbxKeyPoint* keypoints_in(const std::vector<cv::KeyPoint>& keys)
{
    static_assert(sizeof(cv::KeyPoint) == sizeof(OrbxKeyPoint), "cv::KeyPoint layout");
    return keys.empty() ? nullptr : reinterpret_cast<const OrbxKeyPoint*>(keys.data());
}

// the first n rows of a descriptor matrix (CV_8U, 32 columns) as one contiguous array: read in place where the rows already are,
// else copied into `copy`, which has to outlive the call that reads the pointer
inline const uint8_t* descriptors_in(const cv::Mat& desc, int n, std::vector<uint8_t>& copy)
{
    if (n <= 0) return nullptr;
    if (desc.isContinuous()) return desc.data;
    copy.resize((size_t)n * 32);
    for (int r = 0; r < n; r++) std::memcpy(copy.data() + (size_t)r * 32, desc.ptr<uint8_t>(r), 32);
    return copy.data();
}

// the eight parameters of a KannalaBrandt8 camera (mvParameters: fx fy cx cy k0 k1 k2 k3, floats) promoted to double
template <class Fisheye>
inline void kb8_in(Fisheye* kb, OrbxKB8& out)
{
    out.fx = kb->getParameter(0); out.fy = kb->getParameter(1); out.cx = kb->getParameter(2); out.cy = kb->getParameter(3);
    for (int k = 0; k < 4; k++) out.k[k] = kb->getParameter(4 + k);
}

// A two-camera fisheye rig as an OrbxFisheyeRig: the eight parameters of each camera (floats promoted to double), their Newton
// precision, and Tlr as mRlr (row major) and mtlr.  Fisheye = KannalaBrandt8 (getParameter, GetPrecision)
template <class Fisheye>
inline OrbxFisheyeRig fisheye_rig_in(Fisheye* left, Fisheye* right, const Sophus::SE3f& Tlr)
{
    OrbxFisheyeRig rig;
    std::memset(&rig, 0, sizeof(rig));
    kb8_in(left, rig.left); kb8_in(right, rig.right);
    rig.precision_l = left->GetPrecision(); rig.precision_r = right->GetPrecision();
    const Eigen::Matrix3f R = Tlr.rotationMatrix();
    const Eigen::Vector3f t = Tlr.translation();
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) rig.Rlr[3 * r + c] = R(r, c); rig.tlr[r] = t(r); }
    return rig;
}

// A two-camera fisheye rig as an OrbxKB8Rig: the eight parameters of each camera and Trl as the g2o::SE3Quat the reference builds
// from it (Trl.unit_quaternion().cast<double>(), Trl.translation().cast<double>(), src/Optimizer.cc:984, :1388-1389)
template <class Fisheye>
inline OrbxKB8Rig kb8_rig_in(Fisheye* left, Fisheye* right, const Sophus::SE3f& Trl)
{
    OrbxKB8Rig rig;
    kb8_in(left, rig.left); kb8_in(right, rig.right);
    pose_in(Trl, rig.q_rl, rig.t_rl);
    return rig;
}

// the reference keeps its Huber deltas in floats (const float thHuberMono = sqrt(5.991), Optimizer.cc:838-839, :1275-1276, ...)
inline double huber_mono() { const float d = std::sqrt(5.991); return d; }
inline double huber_stereo() { const float d = std::sqrt(7.815); return d; }

// The LbaProblem of a flattened window.  cam = fx fy cx cy bf.  The problem points into the arrays.
inline LbaProblem lba_problem(const std::vector<double>& q, const std::vector<double>& t, const std::vector<uint8_t>& fixed, const double* points, int n_points,
                              const std::vector<int32_t>& ePoint, const std::vector<int32_t>& ePose, const std::vector<double>& eObs, const std::vector<double>& eW,
                              const std::vector<uint8_t>& eStereo, const double (&cam)[5], double huber_mono_, double huber_stereo_)
{
    LbaProblem pr;
    pr.n_poses = (int)fixed.size(); pr.pose_q = q.data(); pr.pose_t = t.data(); pr.pose_fixed = fixed.data();
    pr.n_points = n_points; pr.points = points;
    pr.n_edges = (int)ePoint.size(); pr.edge_point = ePoint.data(); pr.edge_pose = ePose.data(); pr.edge_obs = eObs.data();
    pr.edge_inv_sigma2 = eW.data(); pr.edge_stereo = eStereo.data();
    pr.fx = cam[0]; pr.fy = cam[1]; pr.cx = cam[2]; pr.cy = cam[3]; pr.bf = cam[4];
    pr.huber_mono = huber_mono_; pr.huber_stereo = huber_stereo_;
    return pr;
}

}  // namespace orbslam3_hip
