// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_mapping.hpp (CreateNewMapPointsHIP) on a toy map made of the stand-in
// types (tests/stubs/standin_*.hpp).  Modes:
//   run <case.txt>       the adapter on the case (needs a HIP device); prints what it handed to the C entry per key frame
//                        (pose, camera centre, epipole, F12) and the candidates in creation order, floats in hex
//   fallback <case.txt>  the same call with a second camera on one neighbour: must return false before any device call
// tests/test_shim_mapping.py writes the case, parses the output and compares with the Python mirror on the same arrays.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_mapping.hpp"
#include "orbslam3_shim_mapping.hpp"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <fstream>
#include <string>

using namespace ORB_SLAM3;

std::mutex MapPoint::mGlobalMutex;

// the reference entry points orbslam3_shim.hpp names: never reached here
static void unreachable(const char* what) { std::fprintf(stderr, "reference fallback called: %s\n", what); std::exit(40); }
ORBmatcher::ORBmatcher(float, bool) {}
int ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&, const float, const bool, const float) { unreachable("SearchByProjection"); return 0; }
int ORBmatcher::SearchByProjection(Frame&, const Frame&, const float, const bool) { unreachable("SearchByProjection"); return 0; }
int ORBmatcher::Fuse(KeyFrame*, const std::vector<MapPoint*>&, const float, const bool) { unreachable("Fuse"); return 0; }
int ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, std::vector<std::pair<size_t, size_t> >&, const bool, const bool) { unreachable("SearchForTriangulation"); return 0; }
void Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*, int&, int&, int&, int&) { unreachable("LocalBundleAdjustment"); }
void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>&, const std::vector<MapPoint*>&, int, bool*, const unsigned long, const bool) { unreachable("BundleAdjustment"); }
void Optimizer::LocalInertialBA(KeyFrame*, bool*, Map*, int&, int&, int&, int&, bool, bool) { unreachable("LocalInertialBA"); }
int Optimizer::PoseOptimization(Frame*) { unreachable("PoseOptimization"); return 0; }
int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame*, bool) { unreachable("PoseInertialOptimizationLastKeyFrame"); return 0; }
int Optimizer::PoseInertialOptimizationLastFrame(Frame*, bool) { unreachable("PoseInertialOptimizationLastFrame"); return 0; }
Eigen::MatrixXd Optimizer::Marginalize(const Eigen::MatrixXd& H, const int&, const int&) { unreachable("Marginalize"); return H; }

// case file: "n_kf inertial coarse far th_far", then per key frame (the current one first)
//   "n fx fy cx cy mb mbf scale_factor n_levels"  "R[9] t[3]" (row-major Rcw, tcw)  "sigma2[n_levels]"  "scale[n_levels]"
//   n lines "has_mp x y octave u_right depth key_x key_y node desc[32]"
int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: shim_mapping_toy run|fallback case.txt\n"); return 2; }
    const std::string mode = argv[1];
    std::ifstream in(argv[2]);
    if (!in) return 2;
    int n_kf, inertial, coarse, far;
    float th_far;
    in >> n_kf >> inertial >> coarse >> far >> th_far;
    std::deque<MappingKeyFrame> kfs(n_kf);
    std::deque<Pinhole> cams;
    static MapPoint some_point;
    for (int q = 0; q < n_kf; q++) {
        MappingKeyFrame& k = kfs[q];
        int n, nl;
        in >> n >> k.fx >> k.fy >> k.cx >> k.cy >> k.mb >> k.mbf >> k.mfScaleFactor >> nl;
        k.N = n; k.mnId = 10 + q;
        k.invfx = 1.0f / k.fx; k.invfy = 1.0f / k.fy;
        cams.emplace_back(k.fx, k.fy, k.cx, k.cy);
        k.mpCamera = &cams.back();
        Eigen::Matrix3f R;
        Eigen::Vector3f t;
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) in >> R(r, c);
        for (int r = 0; r < 3; r++) in >> t(r);
        k.SetPose(Sophus::SE3f(R, t));
        k.mvLevelSigma2.resize(nl); k.mvScaleFactors.resize(nl);
        for (float& v : k.mvLevelSigma2) in >> v;
        for (float& v : k.mvScaleFactors) in >> v;
        k.mvKeysUn.resize(n); k.mvKeys.resize(n); k.mvuRight.resize(n); k.mvDepth.resize(n); k.mvpMapPoints.assign(n, nullptr);
        k.mDescriptors.create(n, 32, 0);
        for (int i = 0; i < n; i++) {
            int has_mp, node;
            in >> has_mp >> k.mvKeysUn[i].pt.x >> k.mvKeysUn[i].pt.y >> k.mvKeysUn[i].octave >> k.mvuRight[i] >> k.mvDepth[i] >> k.mvKeys[i].pt.x >>
                k.mvKeys[i].pt.y >> node;
            if (has_mp) k.mvpMapPoints[i] = &some_point;
            k.mFeatVec[(DBoW2::NodeId)node].push_back((unsigned)i);
            for (int b = 0; b < 32; b++) { int v; in >> v; k.mDescriptors.data[(size_t)i * 32 + b] = (unsigned char)v; }
        }
    }
    if (!in) { std::fprintf(stderr, "short case file\n"); return 2; }
    std::vector<MappingKeyFrame*> nbs;
    for (int q = 1; q < n_kf; q++) nbs.push_back(&kfs[q]);
    std::vector<NewMapPointCandidateT<MappingKeyFrame> > cand;
    if (mode == "fallback") {
        kfs[n_kf - 1].mpCamera2 = kfs[n_kf - 1].mpCamera;
        const bool ok = CreateNewMapPointsHIP(&kfs[0], nbs, inertial != 0, coarse != 0, far != 0, th_far, cand);
        std::printf("handled %d candidates %d\n", ok ? 1 : 0, (int)cand.size());
        return 0;
    }
    for (int q = 0; q < n_kf; q++) {
        const Eigen::Vector3f Ow = kfs[q].GetCameraCenter();
        std::printf("Ow 3 %a %a %a\n", (double)Ow(0), (double)Ow(1), (double)Ow(2));
        if (q == 0) continue;
        const Eigen::Vector2f ep = kfs[q].mpCamera->project(kfs[q].GetPose() * kfs[0].GetCameraCenter());
        const Sophus::SE3f T12 = kfs[0].GetPose() * kfs[q].GetPoseInverse();
        const Eigen::Matrix3f F12 = kfs[0].mpCamera->toK_().transpose().inverse() * Sophus::SO3f::hat(T12.translation()) * T12.rotationMatrix() *
                                    kfs[q].mpCamera->toK_().inverse();
        std::printf("pair 11 %a %a", (double)ep(0), (double)ep(1));
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) std::printf(" %a", (double)F12(r, c));
        std::printf("\n");
    }
    const bool ok = CreateNewMapPointsHIP(&kfs[0], nbs, inertial != 0, coarse != 0, far != 0, th_far, cand);
    std::printf("handled %d candidates %d\n", ok ? 1 : 0, (int)cand.size());
    for (const auto& c : cand)
        std::printf("cand 13 %d %d %d %d %a %a %a %a %a %a %a %a\n", c.idx1, (int)(c.pKF2->mnId - 11), c.idx2, c.bPointStereo ? 1 : 0,
                    (double)c.x3D(0), (double)c.x3D(1), (double)c.x3D(2), (double)c.normal(0), (double)c.normal(1), (double)c.normal(2),
                    (double)c.fMaxDistance, (double)c.fMinDistance);
    return 0;
}
