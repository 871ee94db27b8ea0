// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_rig.hpp (PoseOptimizationRigHIP, LocalBundleAdjustmentRigHIP) on a toy frame and
// a toy window of a two-camera fisheye rig made of the stand-in types (tests/stubs/standin_*.hpp) against a RECORDING FAKE of the C
// entry points defined here: every call prints a line, every edge of a problem prints a line, the solves return the inputs moved by
// fixed amounts.  No device is needed.
//   shim_rig_toy <scenario>      pose_rig | pose_pinhole2 | pose_stereo_obs | lba_rig | lba_trl | lba_param | lba_pinhole2 | lba_stereo_obs
// tests/test_shim_rig_typed.py checks the order of the calls, the rig, the edges and what was written back.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_rig.hpp"
#include "orbslam3_shim_rig.hpp"

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
    if (!c) { std::printf("%s handle %d NULL\n", what, id_of(h)); return; }
    std::printf("%s handle %d %a %a %a %a %a %a %a %a\n", what, id_of(h), c->fx, c->fy, c->cx, c->cy, c->k[0], c->k[1], c->k[2], c->k[3]);
}
static void print_rig(const char* what, const void* h, const OrbxKB8Rig* r)
{
    if (!r) { std::printf("%s handle %d NULL\n", what, id_of(h)); return; }
    std::printf("%s handle %d", what, id_of(h));
    for (const OrbxKB8* c : {&r->left, &r->right}) std::printf(" %a %a %a %a %a %a %a %a", c->fx, c->fy, c->cx, c->cy, c->k[0], c->k[1], c->k[2], c->k[3]);
    std::printf(" %a %a %a %a %a %a %a\n", r->q_rl[0], r->q_rl[1], r->q_rl[2], r->q_rl[3], r->t_rl[0], r->t_rl[1], r->t_rl[2]);
}
extern "C" int pose_create(int, pose_solver** out) { *out = reinterpret_cast<pose_solver*>((size_t)++g_handles); std::printf("pose_create handle %d\n", g_handles); return 0; }
extern "C" int lba_create(int, lba_solver** out) { *out = reinterpret_cast<lba_solver*>((size_t)++g_handles); std::printf("lba_create handle %d\n", g_handles); return 0; }
extern "C" int pose_set_camera_kb8(pose_solver* s, const OrbxKB8* c) { print_camera("pose_set_camera_kb8", s, c); return 0; }
extern "C" int lba_set_camera_kb8(lba_solver* s, const OrbxKB8* c) { print_camera("lba_set_camera_kb8", s, c); return 0; }
extern "C" int pose_set_rig_kb8(pose_solver* s, const OrbxKB8Rig* r) { print_rig("pose_set_rig_kb8", s, r); return 0; }
extern "C" int lba_set_rig_kb8(lba_solver* s, const OrbxKB8Rig* r) { print_rig("lba_set_rig_kb8", s, r); return 0; }
extern "C" int pose_optimize(pose_solver* s, const PoseProblem* p, PoseResult* r, uint8_t* outlier)
{
    std::printf("pose_optimize handle %d n %d huber %a\n", id_of(s), p->n, p->huber_mono);
    for (int i = 0; i < p->n; i++)
        std::printf("pose_edge %d kind %d obs %a %a %a w %a X %a\n", i, (int)p->stereo[i], p->obs[3 * i], p->obs[3 * i + 1], p->obs[3 * i + 2], p->inv_sigma2[i], p->Xw[3 * i + 2]);
    for (int k = 0; k < 4; k++) r->q[k] = p->q[k];
    for (int k = 0; k < 3; k++) r->t[k] = p->t[k] + 0.5;
    for (int i = 0; i < p->n; i++) outlier[i] = i % 3 == 1;
    r->n_bad = p->n / 3; r->inliers = p->n - r->n_bad;
    return 0;
}
extern "C" int lba_solve(lba_solver* s, const LbaProblem* p, const volatile uint8_t*, int max_iters, double lambda_init, double* q, double* t, double* X, double* chi2,
                         uint8_t* depth, LbaStats*)
{
    int n_fixed = 0;
    for (int i = 0; i < p->n_poses; i++) n_fixed += p->pose_fixed[i];
    std::printf("lba_solve handle %d poses %d fixed %d points %d edges %d iters %d lambda %a\n", id_of(s), p->n_poses, n_fixed, p->n_points, p->n_edges, max_iters, lambda_init);
    for (int e = 0; e < p->n_edges; e++)
        std::printf("lba_edge %d pose %d point %d kind %d obs %a %a %a w %a\n", e, p->edge_pose[e], p->edge_point[e], (int)p->edge_stereo[e], p->edge_obs[3 * e], p->edge_obs[3 * e + 1],
                    p->edge_obs[3 * e + 2], p->edge_inv_sigma2[e]);
    for (int i = 0; i < 4 * p->n_poses; i++) q[i] = p->pose_q[i];
    for (int i = 0; i < 3 * p->n_poses; i++) t[i] = p->pose_t[i] + 0.5;
    for (int i = 0; i < 3 * p->n_points; i++) X[i] = p->points[i] + 1.0;
    // edge 2 (left) and edge 5 (right) above 5.991 but below 7.815: a right edge is held to the monocular threshold; edge 4 behind its camera
    for (int e = 0; e < p->n_edges; e++) { chi2[e] = (e == 2 || e == 5) ? 6.5 : 1.0; depth[e] = e != 4; }
    return 0;
}

static const std::vector<float> kLeft = {190.98f, 190.97f, 254.93f, 256.90f, 0.0034f, 0.0007f, -0.0020f, 0.0002f};
static const std::vector<float> kRight = {189.40f, 189.35f, 252.10f, 259.30f, 0.0030f, 0.0011f, -0.0017f, 0.00015f};

static Sophus::SE3f toy_Trl(float baseline)
{
    const float c = std::cos(0.05f), s = std::sin(0.05f);        // a rotation about y
    Eigen::Matrix3f R;
    R(0, 0) = c; R(0, 2) = s; R(1, 1) = 1.f; R(2, 0) = -s; R(2, 2) = c;
    return Sophus::SE3f(R, Eigen::Vector3f(-baseline, 0.001f, 0.002f));
}

static void print_Trl(const Sophus::SE3f& T)
{
    double q[4], t[3];
    orbslam3_hip::pose_in(T, q, t);
    std::printf("toy_trl %a %a %a %a %a %a %a\n", q[0], q[1], q[2], q[3], t[0], t[1], t[2]);
}

static int run_pose(const std::string& sc)
{
    KannalaBrandt8 kb(kLeft), kb_right(kRight);
    Pinhole pin(458.f, 457.f, 367.f, 248.f);
    RigPoseFrame F;
    F.N = 7; F.Nleft = 4;                                           // features 0..3 in the left image, 4..6 in the right one
    F.mvKeys.resize(4); F.mvKeysUn.resize(4); F.mvKeysRight.resize(3);
    F.mvuRight.assign(7, -1.f); F.mvpMapPoints.assign(7, nullptr); F.mvbOutlier.assign(7, true);
    F.mvInvLevelSigma2 = {1.f, 0.69f, 0.48f};
    F.fx = 458.f; F.fy = 457.f; F.cx = 367.f; F.cy = 248.f;
    F.mTrl = toy_Trl(0.1f);
    for (int i = 0; i < 4; i++) { F.mvKeys[i] = cv::KeyPoint(100.f + i, 50.f + i, 31.f, -1.f, 0.f, i % 2); F.mvKeysUn[i] = cv::KeyPoint(900.f + i, 800.f + i, 31.f, -1.f, 0.f, 0); }
    for (int i = 0; i < 3; i++) F.mvKeysRight[i] = cv::KeyPoint(300.f + i, 250.f + i, 31.f, -1.f, 0.f, 2 - i);
    std::deque<MapPoint> mps(5);
    const int at[5] = {0, 2, 3, 4, 6};
    for (int k = 0; k < 5; k++) {
        mps[k].mWorldPos = Eigen::Vector3f(0.1f * k, -0.2f * k, 2.f + k);
        F.mvpMapPoints[at[k]] = &mps[k];
    }
    F.mpCamera = &kb;
    F.mpCamera2 = sc == "pose_pinhole2" ? static_cast<GeometricCamera*>(&pin) : &kb_right;
    if (sc == "pose_stereo_obs") F.mvuRight[2] = 90.f;              // a left feature with a map point and a rectified right coordinate
    print_Trl(F.mTrl);
    const int n = PoseOptimizationRigHIP<KannalaBrandt8, RigPoseFrame>(&F);
    std::printf("returned %d t %a outliers", n, (double)F.GetPose().translation()(0));
    for (int i = 0; i < 7; i++) std::printf(" %d", (int)F.mvbOutlier[i]);
    std::printf("\n");
    return 0;
}

static int run_lba(const std::string& sc)
{
    KannalaBrandt8 kb(kLeft), kb_right(kRight);
    std::vector<float> other = kRight;
    other[5] = 0.0012f;
    KannalaBrandt8 kb_other(other);
    Pinhole pin(458.f, 457.f, 367.f, 248.f);
    Map map;
    map.mnInitKFid = 0;
    std::vector<RigKeyFrame> kfs(4);      // 0 (the map's first, fixed), 1, 2 local; 3 sees a local point from outside: a fixed camera.  (a vector: the observations of a
    std::deque<MapPoint> mps(3);          // map point are ordered by key-frame address, and the edge order is part of what is checked)
    for (int i = 0; i < 4; i++) {
        kfs[i].mnId = i; kfs[i].mpMap = &map; kfs[i].mpCamera = &kb; kfs[i].mpCamera2 = &kb_right; kfs[i].mTrl = toy_Trl(0.1f);
        kfs[i].N = 5; kfs[i].NLeft = 3;
        kfs[i].mvKeysUn.resize(3); kfs[i].mvKeysRight.resize(2); kfs[i].mvuRight.assign(3, -1.f); kfs[i].mvpMapPoints.assign(5, nullptr);
        kfs[i].mvInvLevelSigma2 = {1.f, 0.69f};
        for (int k = 0; k < 3; k++) kfs[i].mvKeysUn[k] = cv::KeyPoint(10.f * i + k, 20.f * i + k, 31.f, -1.f, 0.f, 0);
        for (int k = 0; k < 2; k++) kfs[i].mvKeysRight[k] = cv::KeyPoint(100.f + 10.f * i + k, 200.f + 20.f * i + k, 31.f, -1.f, 0.f, 1);
    }
    for (int k = 0; k < 3; k++) { mps[k].mnId = 10 + k; mps[k].mpMap = &map; mps[k].mWorldPos = Eigen::Vector3f(1.f * k, 0.f, 3.f); }
    auto see = [&](int kf, int mp, int left, int right) {          // right is an index into the frame's whole feature list (>= NLeft), as the reference keeps it
        if (left >= 0) kfs[kf].mvpMapPoints[left] = &mps[mp];
        if (right >= 0) kfs[kf].mvpMapPoints[right] = &mps[mp];
        mps[mp].mObservations[&kfs[kf]] = std::tuple<int, int>(left, right); mps[mp].nObs++;
    };
    see(0, 0, 0, -1); see(1, 0, -1, 3); see(1, 1, 1, 4); see(2, 1, 1, -1); see(2, 2, 2, 3); see(3, 2, 2, -1); see(0, 2, -1, 4);
    KeyFrame* cur = &kfs[2];
    cur->mvpOrderedConnectedKeyFrames = {&kfs[1], &kfs[0]};
    if (sc == "lba_trl") kfs[3].mTrl = toy_Trl(0.11f);              // only the walk finds the fixed camera
    if (sc == "lba_param") kfs[3].mpCamera2 = &kb_other;            // one coefficient of the right camera differs, on the fixed camera
    if (sc == "lba_pinhole2") kfs[1].mpCamera2 = &pin;
    if (sc == "lba_stereo_obs") kfs[3].mvuRight[2] = 12.f;          // an edge-bearing observation with a rectified right coordinate
    print_Trl(kfs[0].mTrl);
    int nf = -1, no = -1, nm = -1, ne = -1;
    LocalBundleAdjustmentRigHIP<KannalaBrandt8, RigKeyFrame>(cur, nullptr, &map, nf, no, nm, ne);
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
