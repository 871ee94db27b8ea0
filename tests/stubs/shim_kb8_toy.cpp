// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_kb8.hpp (PoseOptimizationAnyCamHIP, LocalBundleAdjustmentAnyCamHIP) on toy
// frames and a toy window made of the stand-in types (tests/stubs/standin_*.hpp) against a RECORDING FAKE of the C entry points
// defined here: every call prints a line (and dumps its whole argument on stderr through record_abi.hpp, for tests/test_shim_abi_golden.py),
// the solves return the inputs moved by fixed amounts.  No device is needed.
//   shim_kb8_toy <scenario>      pose_kb8 | pose_pinhole | pose_rig | pose_stereo_obs | lba_kb8 | lba_mixed | lba_rig | lba_fixed_pinhole | lba_stereo_obs
// tests/test_shim_kb8_typed.py checks the order of the calls, the camera parameters and what was written back.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_kb8.hpp"
#include "orbslam3_shim_kb8.hpp"
#include "record_abi.hpp"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>

using namespace ORB_SLAM3;

std::mutex MapPoint::mGlobalMutex;

static void unreachable(const char* what) { std::fprintf(stderr, "reference fallback called: %s\n", what); std::exit(40); }
ORBmatcher::ORBmatcher(float, bool) {}
int ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&, const float, const bool, const float) { unreachable("SearchByProjection"); return 0; }
int ORBmatcher::SearchByProjection(Frame&, const Frame&, const float, const bool) { unreachable("SearchByProjection"); return 0; }
int ORBmatcher::Fuse(KeyFrame*, const std::vector<MapPoint*>&, const float, const bool) { unreachable("Fuse"); return 0; }
int ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, std::vector<std::pair<size_t, size_t> >&, const bool, const bool) { unreachable("SearchForTriangulation"); return 0; }
void Optimizer::LocalBundleAdjustment(KeyFrame*, bool*, Map*, int&, int&, int&, int&) { std::printf("reference LocalBundleAdjustment\n"); }
void Optimizer::BundleAdjustment(const std::vector<KeyFrame*>&, const std::vector<MapPoint*>&, int, bool*, const unsigned long, const bool) { unreachable("BundleAdjustment"); }
void Optimizer::LocalInertialBA(KeyFrame*, bool*, Map*, int&, int&, int&, int&, bool, bool) { unreachable("LocalInertialBA"); }
int Optimizer::PoseOptimization(Frame*) { std::printf("reference PoseOptimization\n"); return -7; }
int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame*, bool) { unreachable("PoseInertialOptimizationLastKeyFrame"); return 0; }
int Optimizer::PoseInertialOptimizationLastFrame(Frame*, bool) { unreachable("PoseInertialOptimizationLastFrame"); return 0; }
Eigen::MatrixXd Optimizer::Marginalize(const Eigen::MatrixXd& H, const int&, const int&) { unreachable("Marginalize"); return H; }

// ---- the recording fake (these definitions take the place of the library's); handle 1, 2, ... in order of creation ----
static int g_handles = 0;
extern "C" const char* orbx_last_error(void) { return "fake"; }
static int id_of(const void* h) { return (int)reinterpret_cast<size_t>(h); }
static void print_camera(const char* what, const void* h, const OrbxKB8* c)
{
    record_abi::dump(c);
    if (!c) { std::printf("%s handle %d NULL\n", what, id_of(h)); return; }
    std::printf("%s handle %d %a %a %a %a %a %a %a %a\n", what, id_of(h), c->fx, c->fy, c->cx, c->cy, c->k[0], c->k[1], c->k[2], c->k[3]);
}
extern "C" int pose_create(int, pose_solver** out) { *out = reinterpret_cast<pose_solver*>((size_t)++g_handles); std::printf("pose_create handle %d\n", g_handles); return 0; }
extern "C" int lba_create(int, lba_solver** out) { *out = reinterpret_cast<lba_solver*>((size_t)++g_handles); std::printf("lba_create handle %d\n", g_handles); return 0; }
extern "C" int pose_set_camera_kb8(pose_solver* s, const OrbxKB8* c) { print_camera("pose_set_camera_kb8", s, c); return 0; }
extern "C" int lba_set_camera_kb8(lba_solver* s, const OrbxKB8* c) { print_camera("lba_set_camera_kb8", s, c); return 0; }
extern "C" int pose_optimize(pose_solver* s, const PoseProblem* p, PoseResult* r, uint8_t* outlier)
{
    int n_stereo = 0;
    record_abi::dump(*p);
    for (int i = 0; i < p->n; i++) n_stereo += p->stereo[i];
    std::printf("pose_optimize handle %d n %d stereo %d huber %a first_obs %a %a %a\n", id_of(s), p->n, n_stereo, p->huber_mono, p->n ? p->obs[0] : 0.0, p->n ? p->obs[1] : 0.0,
                p->n ? p->obs[2] : 0.0);
    for (int k = 0; k < 4; k++) r->q[k] = p->q[k];
    for (int k = 0; k < 3; k++) r->t[k] = p->t[k] + 0.5;
    for (int i = 0; i < p->n; i++) outlier[i] = i % 3 == 1;
    r->n_bad = p->n / 3; r->inliers = p->n - r->n_bad;
    return 0;
}
extern "C" int lba_solve(lba_solver* s, const LbaProblem* p, const volatile uint8_t*, int max_iters, double lambda_init, double* q, double* t, double* X, double* chi2,
                         uint8_t* depth, LbaStats*)
{
    int n_stereo = 0, n_fixed = 0;
    record_abi::dump(*p);
    record_abi::scalar("max_iters", max_iters); record_abi::scalar("lambda_init", lambda_init);
    for (int e = 0; e < p->n_edges; e++) n_stereo += p->edge_stereo[e];
    for (int i = 0; i < p->n_poses; i++) n_fixed += p->pose_fixed[i];
    std::printf("lba_solve handle %d poses %d fixed %d points %d edges %d stereo %d iters %d lambda %a\n", id_of(s), p->n_poses, n_fixed, p->n_points, p->n_edges, n_stereo, max_iters,
                lambda_init);
    for (int i = 0; i < 4 * p->n_poses; i++) q[i] = p->pose_q[i];
    for (int i = 0; i < 3 * p->n_poses; i++) t[i] = p->pose_t[i] + 0.5;
    for (int i = 0; i < 3 * p->n_points; i++) X[i] = p->points[i] + 1.0;
    for (int e = 0; e < p->n_edges; e++) { chi2[e] = e == 2 ? 6.5 : 1.0; depth[e] = e != 4; }      // edge 2 above 5.991 (below 7.815), edge 4 behind the camera
    return 0;
}

static const std::vector<float> kParams = {190.98f, 190.97f, 254.93f, 256.90f, 0.0034f, 0.0007f, -0.0020f, 0.0002f};

static int run_pose(const std::string& sc)
{
    KannalaBrandt8 kb(kParams), kb_right(kParams);
    Pinhole pin(458.f, 457.f, 367.f, 248.f);
    Frame F;
    F.N = 7;
    F.mvKeysUn.resize(7); F.mvuRight.assign(7, -1.f); F.mvpMapPoints.assign(7, nullptr); F.mvbOutlier.assign(7, true);
    F.mvInvLevelSigma2 = {1.f, 0.69f};
    F.fx = 458.f; F.fy = 457.f; F.cx = 367.f; F.cy = 248.f;
    std::deque<MapPoint> mps(5);
    const int at[5] = {0, 2, 3, 5, 6};
    for (int k = 0; k < 5; k++) {
        mps[k].mWorldPos = Eigen::Vector3f(0.1f * k, -0.2f * k, 2.f + k);
        F.mvpMapPoints[at[k]] = &mps[k];
        F.mvKeysUn[at[k]] = cv::KeyPoint(100.f + at[k], 50.f + at[k], 31.f, -1.f, 0.f, k % 2);
    }
    F.mpCamera = sc == "pose_pinhole" ? static_cast<GeometricCamera*>(&pin) : &kb;
    if (sc == "pose_rig") F.mpCamera2 = &kb_right;
    if (sc == "pose_stereo_obs") F.mvuRight[3] = 90.f;              // a feature with a map point and a right coordinate
    const int n = PoseOptimizationAnyCamHIP(&F);
    std::printf("returned %d t %a outliers", n, (double)F.GetPose().translation()(0));
    for (int i = 0; i < 7; i++) std::printf(" %d", (int)F.mvbOutlier[i]);
    std::printf("\n");
    if (sc == "pose_kb8") {     // a second frame on the same thread uses the same handle, and sets and resets the camera again
        const int n2 = PoseOptimizationAnyCamHIP(&F);
        std::printf("returned %d\n", n2);
    }
    return 0;
}

static int run_lba(const std::string& sc)
{
    KannalaBrandt8 kb(kParams), kb_right(kParams);
    std::vector<float> other = kParams;
    other[5] = 0.0008f;
    KannalaBrandt8 kb_other(other);
    Pinhole pin(458.f, 457.f, 367.f, 248.f);
    Map map;
    map.mnInitKFid = 0;
    std::deque<KeyFrame> kfs(4);          // 0 (the map's first, fixed), 1, 2 local; 3 sees a local point from outside: a fixed camera
    std::deque<MapPoint> mps(3);
    for (int i = 0; i < 4; i++) {
        kfs[i].mnId = i; kfs[i].mpMap = &map; kfs[i].mpCamera = &kb;
        kfs[i].mvKeysUn.resize(3); kfs[i].mvuRight.assign(3, -1.f); kfs[i].mvpMapPoints.assign(3, nullptr);
        kfs[i].mvInvLevelSigma2 = {1.f};
        for (int k = 0; k < 3; k++) kfs[i].mvKeysUn[k] = cv::KeyPoint(10.f * i + k, 20.f * i + k, 31.f);
    }
    for (int k = 0; k < 3; k++) { mps[k].mnId = 10 + k; mps[k].mpMap = &map; mps[k].mWorldPos = Eigen::Vector3f(1.f * k, 0.f, 3.f); }
    auto see = [&](int kf, int mp) { kfs[kf].mvpMapPoints[mp] = &mps[mp]; mps[mp].AddObservation(&kfs[kf], mp); };
    see(0, 0); see(1, 0); see(1, 1); see(2, 1); see(2, 2); see(3, 2); see(0, 2);
    KeyFrame* cur = &kfs[2];
    cur->mvpOrderedConnectedKeyFrames = {&kfs[1], &kfs[0]};
    if (sc == "lba_mixed") kfs[1].mpCamera = &kb_other;             // one coefficient differs
    if (sc == "lba_rig") kfs[1].mpCamera2 = &kb_right;
    if (sc == "lba_fixed_pinhole") kfs[3].mpCamera = &pin;          // only the walk finds this one
    if (sc == "lba_stereo_obs") kfs[3].mvuRight[2] = 12.f;          // an observation with a right coordinate, by the fixed camera
    int nf = -1, no = -1, nm = -1, ne = -1;
    LocalBundleAdjustmentAnyCamHIP(cur, nullptr, &map, nf, no, nm, ne);
    std::printf("counters %d %d %d %d change %d\n", nf, no, nm, ne, map.mnMapChange);
    for (int i = 0; i < 4; i++) std::printf("kf %d writes %d t %a\n", i, kfs[i].nPoseWrites, (double)kfs[i].GetPose().translation()(0));
    for (int k = 0; k < 3; k++) std::printf("mp %d x %a erased %d normals %d\n", k, (double)mps[k].mWorldPos(0), mps[k].nErased, mps[k].nNormalUpdates);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const std::string sc = argv[1];
    return sc.compare(0, 4, "pose") == 0 ? run_pose(sc) : run_lba(sc);
}
