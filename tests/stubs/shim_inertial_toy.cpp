// TEST INFRASTRUCTURE -- drives LocalInertialBAHIP and PoseInertialOptimizationHIP of include/orbslam3_shim.hpp on a toy window and
// a toy frame made of the stand-in types (tests/stubs/standin_*.hpp) against a RECORDING FAKE of liba_create, liba_solve and
// liba_pose_optimize_batch defined here: every call dumps its whole problem through record_abi.hpp on stderr and returns the inputs
// moved by fixed amounts; Optimizer::Marginalize records its arguments.  What the adapter wrote back is printed on stdout.
//   shim_inertial_toy <scenario>
//     liba_window | liba_recinit | liba_large | liba_diverged | liba_large_diverged | liba_no_prev | liba_stop
//     pose_keyframe | pose_lastframe | pose_keyframe_recinit | pose_lastframe_recinit | pose_rig
// tests/test_shim_abi_golden.py compares both streams with tests/golden/shim_abi/shim_inertial_toy.txt.  No device is needed.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_orbslam3.hpp"
#include "orbslam3_shim.hpp"
#include "record_abi.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

using namespace ORB_SLAM3;

std::mutex MapPoint::mGlobalMutex;

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
int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame*, bool bRecInit) { std::printf("reference PoseInertialOptimizationLastKeyFrame %d\n", (int)bRecInit); return -7; }
int Optimizer::PoseInertialOptimizationLastFrame(Frame*, bool bRecInit) { std::printf("reference PoseInertialOptimizationLastFrame %d\n", (int)bRecInit); return -8; }
Eigen::MatrixXd Optimizer::Marginalize(const Eigen::MatrixXd& H, const int& start, const int& end)
{
    std::vector<double> flat;
    for (int r = 0; r < H.rows(); r++) for (int c = 0; c < H.cols(); c++) flat.push_back(H(r, c));
    std::printf("Marginalize %d x %d start %d end %d fnv %016llx\n", H.rows(), H.cols(), start, end, (unsigned long long)record_abi::fnv1a(flat.data(), flat.size() * sizeof(double)));
    Eigen::MatrixXd out = H;
    for (int r = 0; r < H.rows(); r++) for (int c = 0; c < H.cols(); c++) out(r, c) = H(r, c) + 0.25;
    return out;
}

// ---- the recording fake (these definitions take the place of the library's); handle 1, 2, ... in order of creation ----
static int g_handles = 0;
static double g_chi2_growth = 0.5;      // chi2_final = g_chi2_growth * chi2_initial
extern "C" const char* orbx_last_error(void) { return "fake"; }
extern "C" int liba_create(int, liba_solver** out) { *out = reinterpret_cast<liba_solver*>((size_t)++g_handles); std::printf("liba_create handle %d\n", g_handles); return 0; }
extern "C" int liba_solve(liba_solver* s, const LibaProblem* p, double* R, double* t, double* v, double* bg, double* ba, double* X, double* chi2, uint8_t* depth, LbaStats* st)
{
    std::printf("liba_solve handle %d\n", (int)reinterpret_cast<size_t>(s));
    record_abi::dump(*p);
    for (int i = 0; i < 9 * p->n_kf; i++) R[i] = p->Rwb[i];
    for (int i = 0; i < 3 * p->n_kf; i++) { t[i] = p->twb[i] + 0.5; v[i] = p->vel[i] + 0.25; bg[i] = p->bg[i] + 0.125; ba[i] = p->ba[i] + 0.0625; }
    for (int i = 0; i < 3 * p->n_points; i++) X[i] = p->points[i] + 1.0;
    // every edge of the window's points 1 and 2 lies between 5.991 and 1.5 x 5.991 (and below 7.815); the last edge is behind the camera
    for (int e = 0; e < p->n_edges; e++) { chi2[e] = p->edge_point[e] == 1 || p->edge_point[e] == 2 ? 7.0 : 1.0; depth[e] = e != p->n_edges - 1; }
    std::memset(st, 0, sizeof(*st));
    st->chi2_initial = 100.0; st->chi2_final = 100.0 * g_chi2_growth;
    return 0;
}
extern "C" int liba_pose_optimize_batch(liba_solver* s, const LibaPoseProblem* p, int batch, double* R, double* t, double* v, double* bg, double* ba, uint8_t* outlier, double* H,
                                        int32_t* inliers, int32_t* n_bad)
{
    std::printf("liba_pose_optimize_batch handle %d batch %d\n", (int)reinterpret_cast<size_t>(s), batch);
    record_abi::dump(*p);
    for (int i = 0; i < 9; i++) R[i] = p->Rwb[9 + i];
    for (int i = 0; i < 3; i++) { t[i] = p->twb[3 + i] + 0.5; v[i] = p->vel[3 + i] + 0.25; bg[i] = p->bg[3 + i] + 0.125; ba[i] = p->ba[3 + i] + 0.0625; }
    for (int i = 0; i < p->n; i++) outlier[i] = i % 3 == 1;
    const int m = p->last_frame ? 30 : 15;
    for (int i = 0; i < m * m; i++) H[i] = 1.0 + 0.001 * i;
    *n_bad = p->n / 3; *inliers = p->n - *n_bad;
    return 0;
}

// a small deterministic generator for the toy's numbers
static unsigned g_seed = 12345u;
static float rnd() { g_seed = g_seed * 1664525u + 1013904223u; return (float)((g_seed >> 8) & 0xffff) / 65536.f - 0.5f; }
static Eigen::Matrix3f rot(float a, float b)
{
    Eigen::Matrix3f Rz, Rx;
    Rz(0, 0) = std::cos(a); Rz(0, 1) = -std::sin(a); Rz(1, 0) = std::sin(a); Rz(1, 1) = std::cos(a); Rz(2, 2) = 1.f;
    Rx(0, 0) = 1.f; Rx(1, 1) = std::cos(b); Rx(1, 2) = -std::sin(b); Rx(2, 1) = std::sin(b); Rx(2, 2) = std::cos(b);
    return Rz * Rx;
}
static Eigen::Matrix3f small3() { Eigen::Matrix3f M; for (int i = 0; i < 9; i++) M[i] = 0.1f * rnd(); return M; }
static Eigen::Vector3f vec3(float s) { return Eigen::Vector3f(s * rnd(), s * rnd(), s * rnd()); }
static void fill(IMU::Preintegrated& p, int k)
{
    p.dT = 0.2f + 0.01f * k;
    p.dR = rot(0.05f * k, 0.02f); p.dV = vec3(1.f); p.dP = vec3(1.f);
    p.JRg = small3(); p.JVg = small3(); p.JVa = small3(); p.JPg = small3(); p.JPa = small3();
    p.b = IMU::Bias(0.02f * rnd(), 0.02f * rnd(), 0.02f * rnd(), 0.02f * rnd(), 0.02f * rnd(), 0.02f * rnd());
    Eigen::Matrix<float, 15, 15> A;
    for (int i = 0; i < 225; i++) A[i] = rnd();
    const Eigen::Matrix<float, 15, 15> AAt = A * A.transpose();
    for (int r = 0; r < 15; r++) for (int c = 0; c < 15; c++) p.C(r, c) = 1e-6f * AAt(r, c) + (r == c ? 1e-5f : 0.f);
}
static void fill(IMU::Calib& c)
{
    const Eigen::Matrix3f R = rot(0.3f, -0.2f);
    const Eigen::Vector3f t(0.05f, -0.02f, 0.01f);
    c.mTcb = Sophus::SE3<float>(R, t);
    c.mTbc = c.mTcb.inverse();
}
static void print3(const char* what, const Eigen::Vector3f& v) { std::printf(" %s %a %a %a", what, (double)v[0], (double)v[1], (double)v[2]); }
static void print_bias(const char* what, const IMU::Bias& b)
{ std::printf(" %s %a %a %a %a %a %a", what, (double)b.bax, (double)b.bay, (double)b.baz, (double)b.bwx, (double)b.bwy, (double)b.bwz); }

// Key frames 0 <- 1 <- 2 <- 3 <- 4 by mPrevKF, 4 the current one; the map counts 6 key frames, so 4 3 2 1 are optimisable and 0, the
// predecessor of the last optimisable one, is fixed: its link is the one with the factor 1e-2 and the Huber kernel.  Key frame 5 is
// outside the chain and sees the local point 3: the second fixed key frame.  Six map points; point 0 has one monocular and one stereo
// observation.  The window lists the points in the order 0 1 5 2 3 4, so the fake's chi2 of 7.0 goes to the edges of map point 1 (close:
// kept) and of map point 5 (far: its monocular edge is erased, its stereo edge stays below 7.815); the last edge, of map point 4, is
// behind the camera.
static int run_liba(const std::string& sc)
{
    Pinhole pin(458.f, 457.f, 367.f, 248.f);
    Map map;
    map.nKeyFrames = 6;
    std::vector<KeyFrame> kfs(6);
    std::vector<IMU::Preintegrated> pre(6);
    std::vector<MapPoint> mps(6);
    for (int i = 0; i < 6; i++) {
        KeyFrame& k = kfs[i];
        k.mnId = 10 + i; k.mpMap = &map; k.mpCamera = &pin; k.bImu = true;
        k.fx = 458.f; k.fy = 457.f; k.cx = 367.f; k.cy = 248.f; k.mbf = 47.9f;
        k.mvInvLevelSigma2 = {1.f, 0.69f, 0.48f};
        k.mvKeysUn.resize(6); k.mvuRight.assign(6, -1.f); k.mvpMapPoints.assign(6, nullptr);
        for (int j = 0; j < 6; j++) k.mvKeysUn[j] = cv::KeyPoint(100.f + 10.f * i + j + 0.3f, 50.f + 7.f * i + 2.f * j + 0.7f, 31.f, -1.f, 0.f, (i + j) % 3);
        k.mRwb = rot(0.1f * i, 0.05f * i); k.mtwb = vec3(2.f); k.mVw = vec3(1.f);
        k.mImuBias = IMU::Bias(0.02f * rnd(), 0.02f * rnd(), 0.02f * rnd(), 0.02f * rnd(), 0.02f * rnd(), 0.02f * rnd());
        fill(k.mImuCalib);
        if (i >= 1 && i <= 4) { k.mPrevKF = &kfs[i - 1]; fill(pre[i], i); k.mpImuPreintegrated = &pre[i]; }
    }
    for (int j = 0; j < 6; j++) { mps[j].mnId = 100 + j; mps[j].mpMap = &map; mps[j].mWorldPos = vec3(3.f); mps[j].mTrackDepth = 20.f; }
    mps[1].mTrackDepth = 5.f;
    auto see = [&](int kf, int mp) { kfs[kf].mvpMapPoints[mp] = &mps[mp]; mps[mp].AddObservation(&kfs[kf], mp); };
    see(4, 0); see(3, 0); kfs[3].mvuRight[0] = 95.5f;               // point 0: monocular in 4, stereo in 3
    see(4, 1); see(2, 1);
    see(3, 2); see(1, 2);
    see(2, 3); see(5, 3);                                           // key frame 5: fixed, found through the point
    see(1, 4); see(0, 4);
    see(4, 5); see(1, 5); kfs[1].mvuRight[5] = 120.25f;
    if (sc == "liba_no_prev") kfs[1].mPrevKF = nullptr;             // the chain ends at 1: it becomes the fixed key frame and gets no link
    if (sc == "liba_diverged" || sc == "liba_large_diverged") g_chi2_growth = 3.0;
    const bool bLarge = sc == "liba_large" || sc == "liba_large_diverged", bRecInit = sc == "liba_recinit";
    bool stop = sc == "liba_stop";
    int nf = -1, no = -1, nm = -1, ne = -1;
    LocalInertialBAHIP(&kfs[4], sc == "liba_stop" ? &stop : nullptr, &map, nf, no, nm, ne, bLarge, bRecInit);
    std::printf("counters %d %d %d %d change %d stop %d\n", nf, no, nm, ne, map.mnMapChange, (int)stop);
    for (int i = 0; i < 6; i++) {
        KeyFrame& k = kfs[i];
        std::printf("kf %d writes %d local %lu fixed %lu", i, k.nPoseWrites, k.mnBALocalForKF, k.mnBAFixedForKF);
        const Eigen::Matrix3f R = k.GetPose().rotationMatrix();
        std::printf(" R");
        for (int a = 0; a < 9; a++) std::printf(" %a", (double)R[a]);
        print3("t", k.GetPose().translation()); print3("v", k.mVw); print_bias("bias", k.mImuBias); print_bias("bu", pre[i].bu);
        std::printf("\n");
    }
    for (int j = 0; j < 6; j++) {
        std::printf("mp %d erased %d normals %d obs %d", j, mps[j].nErased, mps[j].nNormalUpdates, mps[j].nObs);
        print3("X", mps[j].mWorldPos);
        std::printf("\n");
    }
    return 0;
}

// Seven features, five with map points, one of those with a right coordinate; the second map point is close.
static int run_pose(const std::string& sc)
{
    const bool lastFrame = sc.find("lastframe") != std::string::npos, bRecInit = sc.find("recinit") != std::string::npos;
    Pinhole pin(458.f, 457.f, 367.f, 248.f);
    Frame F, prev;
    KeyFrame kf;
    IMU::Preintegrated preKF, preFrame;
    fill(preKF, 1); fill(preFrame, 2);
    F.N = 7;
    F.mvKeysUn.resize(7); F.mvuRight.assign(7, -1.f); F.mvpMapPoints.assign(7, nullptr); F.mvbOutlier.assign(7, true);
    F.mvInvLevelSigma2 = {1.f, 0.69f};
    F.fx = 458.f; F.fy = 457.f; F.cx = 367.f; F.cy = 248.f; F.mbf = 47.9f;
    F.mpCamera = &pin;
    std::vector<MapPoint> mps(5);
    const int at[5] = {0, 2, 3, 5, 6};
    for (int k = 0; k < 5; k++) {
        mps[k].mWorldPos = Eigen::Vector3f(0.1f * k + 0.03f, -0.2f * k, 2.f + k);
        mps[k].mTrackDepth = k == 1 ? 4.f : 15.f;
        F.mvpMapPoints[at[k]] = &mps[k];
        F.mvKeysUn[at[k]] = cv::KeyPoint(100.3f + at[k], 50.7f + at[k], 31.f, -1.f, 0.f, k % 2);
    }
    F.mvuRight[3] = 90.5f;
    F.mRwb = rot(0.4f, 0.1f); F.mtwb = vec3(2.f); F.mVw = vec3(1.f);
    F.mImuBias = IMU::Bias(0.011f, -0.012f, 0.013f, 0.001f, -0.002f, 0.003f);
    fill(F.mImuCalib);
    F.mpImuPreintegrated = &preKF; F.mpImuPreintegratedFrame = &preFrame;
    kf.mRwb = rot(0.3f, 0.05f); kf.mtwb = vec3(2.f); kf.mVw = vec3(1.f);
    kf.mImuBias = IMU::Bias(0.021f, -0.022f, 0.023f, 0.004f, -0.005f, 0.006f);
    F.mpLastKeyFrame = &kf;
    prev.mRwb = rot(0.35f, 0.08f); prev.mtwb = vec3(2.f); prev.mVw = vec3(1.f);
    prev.mImuBias = IMU::Bias(0.031f, -0.032f, 0.033f, 0.007f, -0.008f, 0.009f);
    Eigen::Matrix<double, 15, 15> Hp;
    for (int r = 0; r < 15; r++) for (int c = 0; c < 15; c++) Hp(r, c) = (r == c ? 10.0 : 0.0) + 0.01 * (r + c);
    prev.mpcpi = new ConstraintPoseImu(prev.mRwb.cast<double>(), prev.mtwb.cast<double>(), prev.mVw.cast<double>(), Eigen::Vector3d(0.007, -0.008, 0.009),
                                       Eigen::Vector3d(0.031, -0.032, 0.033), Hp);
    F.mpPrevFrame = &prev;
    if (sc == "pose_rig") F.Nleft = 4;
    const int n = PoseInertialOptimizationHIP(&F, bRecInit, lastFrame);
    std::printf("returned %d outliers", n);
    for (int i = 0; i < 7; i++) std::printf(" %d", (int)F.mvbOutlier[i]);
    std::printf("\nframe R");
    for (int a = 0; a < 9; a++) std::printf(" %a", (double)F.mRwb[a]);
    print3("t", F.mtwb); print3("v", F.mVw); print_bias("bias", F.mImuBias); print_bias("bu_kf", preKF.bu); print_bias("bu_frame", preFrame.bu);
    std::printf("\nprevious mpcpi %s\n", prev.mpcpi ? "kept" : "deleted");
    if (F.mpcpi) {
        const ConstraintPoseImu& c = *F.mpcpi;
        std::printf("mpcpi Rwb fnv %016llx H fnv %016llx H00 %a H1414 %a twb %a %a %a vwb %a %a %a bg %a %a %a ba %a %a %a\n",
                    (unsigned long long)record_abi::fnv1a(&c.Rwb(0, 0), 9 * sizeof(double)), (unsigned long long)record_abi::fnv1a(&c.H(0, 0), 225 * sizeof(double)), c.H(0, 0),
                    c.H(14, 14), c.twb[0], c.twb[1], c.twb[2], c.vwb[0], c.vwb[1], c.vwb[2], c.bg[0], c.bg[1], c.bg[2], c.ba[0], c.ba[1], c.ba[2]);
    } else
        std::printf("mpcpi none\n");
    delete F.mpcpi;
    delete prev.mpcpi;
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const std::string sc = argv[1];
    return sc.compare(0, 4, "pose") == 0 ? run_pose(sc) : run_liba(sc);
}
