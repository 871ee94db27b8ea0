// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_loop.hpp (Sim3SolverHIP, OptimizeSim3HIP) on a toy pair of key frames made
// of the stand-in types (tests/stubs/standin_*.hpp).  Modes (both need a HIP device):
//   ransac <case.txt>   the loop of src/LoopClosing.cc:710-714 on Sim3SolverHIP; prints the flattened problem and the results
//   opt <case.txt>      OptimizeSim3HIP; prints the return value, g2oS12, the nulled matches and mAcumHessian
//   fallback <case.txt> the same two calls with a non-pinhole camera: the supplied reference classes must be reached
// tests/test_shim_loop.py writes the case, parses the output and compares with the C ABI on the same data.
// Eigen does not zero a default-constructed fixed-size matrix; the stand-in does.  So that nothing the adapters return can lean
// on that, this translation unit turns the stand-in's zero fill into a NaN fill: the standard headers first (they stay
// untouched), then the stand-in with `fill` redirected.
#include <array>
#include <cmath>
#include <cstddef>
#include <limits>
#include <vector>
template <class T> inline T standin_poison() { return std::numeric_limits<T>::quiet_NaN(); }
#define fill(v) fill(standin_poison<T>())
#include "standin_eigen.hpp"
#undef fill

#define ORBSLAM3_HIP_WITH_REFERENCE
#include "orbslam3_shim_loop.hpp"

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

// what this translation unit supplies for the two template parameters of the adapters
namespace g2o {
struct Sim3 {                                           // Thirdparty/g2o/g2o/types/sim3.h: the members the adapter uses
    Sim3() : s(1.0) {}
    Sim3(const Eigen::Quaterniond& r_, const Eigen::Vector3d& t_, double s_) : r(r_), t(t_), s(s_) {}
    const Eigen::Quaterniond& rotation() const { return r; }
    const Eigen::Vector3d& translation() const { return t; }
    const double& scale() const { return s; }
    Eigen::Quaterniond r;
    Eigen::Vector3d t;
    double s;
};
}  // namespace g2o

static int g_ref_solver_calls = 0, g_ref_opt_calls = 0;
struct RefSolver {                                      // include/Sim3Solver.h:33-50
    RefSolver(KeyFrame*, KeyFrame*, const std::vector<MapPoint*>&, const bool, const std::vector<KeyFrame*>) { g_ref_solver_calls++; }
    void SetRansacParameters(double, int, int) { g_ref_solver_calls++; }
    Eigen::Matrix<float, 4, 4> iterate(int, bool& bNoMore, std::vector<bool>&, int& n) { g_ref_solver_calls++; bNoMore = true; n = 0; return Eigen::Matrix<float, 4, 4>(); }
    Eigen::Matrix<float, 4, 4> iterate(int, bool& bNoMore, std::vector<bool>&, int& n, bool& c) { g_ref_solver_calls++; bNoMore = true; c = false; n = 0; return Eigen::Matrix<float, 4, 4>(); }
    Eigen::Matrix<float, 4, 4> GetEstimatedTransformation() { return Eigen::Matrix<float, 4, 4>(); }
    Eigen::Matrix3f GetEstimatedRotation() { return Eigen::Matrix3f(); }
    Eigen::Vector3f GetEstimatedTranslation() { return Eigen::Vector3f(); }
    float GetEstimatedScale() { return -1.f; }
};
struct RefOptimizer {
    static int OptimizeSim3(KeyFrame*, KeyFrame*, std::vector<MapPoint*>&, g2o::Sim3&, const float, const bool, Eigen::Matrix<double, 7, 7>&, const bool)
    { g_ref_opt_calls++; return -7; }
};

class NotPinhole : public Pinhole {
public:
    NotPinhole() : Pinhole(1, 1, 0, 0) { mnType = CAM_FISHEYE; }
};

struct Toy {
    KeyFrame kf1, kf2;
    std::deque<MapPoint> mps1, mps2;
    std::vector<MapPoint*> matches;
    int fix_scale = 0, min_inliers = 6, max_its = 300, all_points = 0;
    unsigned long long seed = 0;
    float th2 = 10.f;
    double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0}, s = 1;
};

static void read_kf(std::ifstream& in, KeyFrame& k)
{
    float fx, fy, cx, cy;
    double q[4], t[3];
    in >> k.mnId >> fx >> fy >> cx >> cy >> q[0] >> q[1] >> q[2] >> q[3] >> t[0] >> t[1] >> t[2];
    k.fx = fx; k.fy = fy; k.cx = cx; k.cy = cy;
    k.mpCamera = new Pinhole(fx, fy, cx, cy);
    k.mTcw = Sophus::SE3f(Eigen::Quaternionf((float)q[3], (float)q[0], (float)q[1], (float)q[2]), Eigen::Vector3f((float)t[0], (float)t[1], (float)t[2]));
    k.mvLevelSigma2.resize(8); k.mvInvLevelSigma2.resize(8);
    for (float& v : k.mvLevelSigma2) in >> v;
    for (float& v : k.mvInvLevelSigma2) in >> v;
}

// per feature i of key frame 1: match present, point 1 present / bad / observed in KF1, point 2 bad / index in KF2 (-1: not
// observed), world positions, key points of both sides, the track level of point 2
static void load(const char* path, Toy& T)
{
    std::ifstream in(path);
    if (!in) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(41); }
    int n1, n2;
    in >> T.fix_scale >> T.min_inliers >> T.max_its >> T.seed >> T.all_points >> T.th2;
    in >> T.q[0] >> T.q[1] >> T.q[2] >> T.q[3] >> T.t[0] >> T.t[1] >> T.t[2] >> T.s;
    read_kf(in, T.kf1);
    read_kf(in, T.kf2);
    in >> n1 >> n2;
    T.kf1.mvKeysUn.resize(n1); T.kf1.mvpMapPoints.assign(n1, nullptr);
    T.kf2.mvKeysUn.resize(n2); T.kf2.mvpMapPoints.assign(n2, nullptr);
    T.mps1.resize(n1); T.mps2.resize(n1);
    T.matches.assign(n1, nullptr);
    for (int i = 0; i < n1; i++) {
        int has_match, has1, bad1, obs1, bad2, i2, oct1, oct2, lvl2;
        float X1[3], X2[3], u1, v1, u2, v2;
        in >> has_match >> has1 >> bad1 >> obs1 >> bad2 >> i2 >> X1[0] >> X1[1] >> X1[2] >> X2[0] >> X2[1] >> X2[2] >> u1 >> v1 >> oct1 >> u2 >> v2 >> oct2 >> lvl2;
        MapPoint& a = T.mps1[i];
        MapPoint& b = T.mps2[i];
        a.mbBad = bad1; a.mWorldPos = Eigen::Vector3f(X1[0], X1[1], X1[2]);
        b.mbBad = bad2; b.mWorldPos = Eigen::Vector3f(X2[0], X2[1], X2[2]); b.mnTrackScaleLevel = lvl2;
        T.kf1.mvKeysUn[i] = cv::KeyPoint(u1, v1, 31.f, 0.f, 1.f, oct1);
        if (has1) T.kf1.mvpMapPoints[i] = &a;
        if (obs1) a.AddObservation(&T.kf1, i);
        if (i2 >= 0) { T.kf2.mvKeysUn[i2] = cv::KeyPoint(u2, v2, 31.f, 0.f, 1.f, oct2); T.kf2.mvpMapPoints[i2] = &b; b.AddObservation(&T.kf2, i2); }
        if (has_match) T.matches[i] = &b;
    }
}

template <class V> static void dump(const char* name, const V& v)
{
    std::printf("%s %zu", name, (size_t)v.size());
    for (size_t i = 0; i < v.size(); i++) std::printf(" %a", (double)v[i]);
    std::printf("\n");
}

static int run_ransac(Toy& T)
{
    typedef Sim3SolverHIPT<RefSolver> Solver;
    Solver solver(&T.kf1, &T.kf2, T.matches, T.fix_scale != 0);
    solver.SetRansacParameters(0.99, T.min_inliers, T.max_its);
    solver.SetSeed(T.seed);
    if (solver.UsesReference()) return 50;
    std::printf("N %d H %d\n", solver.Correspondences(), solver.Hypotheses());
    dump("indices1", solver.Indices1());
    dump("X1c", solver.X3Dc1()); dump("X2c", solver.X3Dc2()); dump("max_err1", solver.MaxError1()); dump("max_err2", solver.MaxError2());
    bool bNoMore = false, bConverge = false;
    std::vector<bool> vbInliers;
    int nInliers = 0, calls = 0;
    Solver::Matrix4 Tm;
    while (!bConverge && !bNoMore) {                    // src/LoopClosing.cc:710-714
        Tm = solver.iterate(20, bNoMore, vbInliers, nInliers, bConverge);
        calls++;
    }
    std::printf("calls %d converge %d nomore %d ninliers %d\n", calls, (int)bConverge, (int)bNoMore, nInliers);
    std::vector<float> tm, rot, tr;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) tm.push_back(Tm(r, c));
    const Eigen::Matrix3f R = solver.GetEstimatedRotation();
    const Eigen::Vector3f t = solver.GetEstimatedTranslation();
    for (int r = 0; r < 3; r++) { for (int c = 0; c < 3; c++) rot.push_back(R(r, c)); tr.push_back(t[r]); }
    tr.push_back(solver.GetEstimatedScale());
    dump("T", tm); dump("R", rot); dump("ts", tr);
    std::vector<int> inl(vbInliers.begin(), vbInliers.end());
    dump("inliers", inl);
    // SetSeed() after a finished walk restarts it: the same seed gives the same answer again
    solver.SetSeed(T.seed);
    bool noMore2 = false, conv2 = false;
    std::vector<bool> inl2;
    int nIn2 = 0, calls2 = 0;
    Solver::Matrix4 Tm2;
    while (!conv2 && !noMore2) { Tm2 = solver.iterate(20, noMore2, inl2, nIn2, conv2); calls2++; }
    bool same = calls2 == calls && conv2 == bConverge && noMore2 == bNoMore && nIn2 == nInliers && inl2 == vbInliers;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) same = same && Tm2(r, c) == Tm(r, c);
    std::printf("reseed_same %d\n", (int)same);
    // the 4-argument overload and find() on a fresh solver: Identity unless converged
    Solver again(&T.kf1, &T.kf2, T.matches, T.fix_scale != 0);
    again.SetRansacParameters(0.99, T.min_inliers, T.max_its);
    again.SetSeed(T.seed);
    int n2 = 0;
    std::vector<bool> in2;
    const Solver::Matrix4 Tf = again.find(in2, n2);
    std::vector<float> tf;
    for (int r = 0; r < 4; r++) for (int c = 0; c < 4; c++) tf.push_back(Tf(r, c));
    dump("Tfind", tf);
    std::printf("find_ninliers %d\n", n2);
    return 0;
}

static int run_opt(Toy& T)
{
    g2o::Sim3 S(Eigen::Quaterniond(T.q[3], T.q[0], T.q[1], T.q[2]), Eigen::Vector3d(T.t[0], T.t[1], T.t[2]), T.s);
    Eigen::Matrix<double, 7, 7> H;
    for (int r = 0; r < 7; r++) for (int c = 0; c < 7; c++) H(r, c) = 3.0;
    std::vector<MapPoint*> matches = T.matches;
    const int ret = OptimizeSim3HIP<RefOptimizer>(&T.kf1, &T.kf2, matches, S, T.th2, T.fix_scale != 0, H, T.all_points != 0);
    if (g_ref_opt_calls) return 51;
    std::printf("ret %d\n", ret);
    std::vector<double> s12 = {S.r.x(), S.r.y(), S.r.z(), S.r.w(), S.t[0], S.t[1], S.t[2], S.s};
    dump("S12", s12);
    std::vector<int> nulled, was;
    for (size_t i = 0; i < matches.size(); i++) { nulled.push_back(matches[i] == nullptr); was.push_back(T.matches[i] == nullptr); }
    dump("null_after", nulled); dump("null_before", was);
    double hs = 0;
    for (int r = 0; r < 7; r++) for (int c = 0; c < 7; c++) hs += H(r, c);
    std::printf("hessian_sum %g\n", hs);
    return 0;
}

static int run_fallback(Toy& T)
{
    T.kf2.mpCamera = new NotPinhole();
    Sim3SolverHIPT<RefSolver> solver(&T.kf1, &T.kf2, T.matches, true);
    bool bNoMore = false, bConverge = false;
    std::vector<bool> in;
    int n = 0;
    solver.iterate(20, bNoMore, in, n, bConverge);
    g2o::Sim3 S;
    Eigen::Matrix<double, 7, 7> H;
    std::vector<MapPoint*> matches = T.matches;
    const int ret = OptimizeSim3HIP<RefOptimizer>(&T.kf1, &T.kf2, matches, S, 10.f, true, H, false);
    std::printf("uses_reference %d solver_calls %d opt_calls %d ret %d scale %g\n", (int)solver.UsesReference(), g_ref_solver_calls, g_ref_opt_calls, ret,
                (double)solver.GetEstimatedScale());
    return 0;
}

int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: %s ransac|opt|fallback <case.txt>\n", argv[0]); return 2; }
    Toy T;
    load(argv[2], T);
    const std::string mode = argv[1];
    try {
        if (mode == "ransac") return run_ransac(T);
        if (mode == "opt") return run_opt(T);
        if (mode == "fallback") return run_fallback(T);
    } catch (const orbslam3_hip::Error& e) {
        std::fprintf(stderr, "orbslam3_hip error %d: %s\n", e.code, e.what());
        return e.code == ORBX_ERR_NO_DEVICE ? 44 : 45;
    }
    return 2;
}
