// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_rig_mapping.hpp (CreateNewMapPointsRigHIP) on toy key frames made of the
// stand-in types (tests/stubs/standin_*.hpp) against a RECORDING FAKE of the C entry points defined here: every call prints a line on
// stdout and its arrays, element by element, on the lines after it.  The fake writes fixed results so that the creation order and the
// skipped flags show.  No device is needed.
//   shim_rig_mapping_toy <scenario>   rig | conv | mixed_kf1 | mixed_neighbour | pinhole_rig
// tests/test_shim_rig_mapping.py checks the routing, the arrays, the four pose products per neighbour and the creation order.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_rig_mapping.hpp"
#include "orbslam3_shim_rig_mapping.hpp"

#include <cstdio>
#include <cstdlib>
#include <deque>
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

// ---- the recording fake (these definitions take the place of the library's) ----
static int g_handles = 0;
extern "C" const char* orbx_last_error(void) { return "fake"; }
static int id_of(const void* h) { return (int)reinterpret_cast<size_t>(h); }
extern "C" int orbm_create(int, orbm_matcher** out) { *out = reinterpret_cast<orbm_matcher*>((size_t)++g_handles); std::printf("orbm_create handle %d\n", g_handles); return 0; }

template <class T>
static void row(const char* name, const T* p, int n)
{
    std::printf(" %s", name);
    if (!p) std::printf(" NULL");
    for (int i = 0; p && i < n; i++) std::printf(" %a", (double)p[i]);
    std::printf("\n");
}

extern "C" int orbm_create_new_map_points(orbm_matcher* m, const OrbmMapKeyFrame* kf1, const OrbmMapKeyFrame*, int n_neighbours, const OrbmMapPair*, const OrbmMapParams*,
                                          OrbmNewPoints*)
{
    std::printf("orbm_create_new_map_points handle %d n1 %d n_neighbours %d\n", id_of(m), kf1->side.n, n_neighbours);
    return 0;
}

static void print_kf(const char* name, const OrbmRigMapKeyFrame& k)
{
    char b[64];
    auto nm = [&](const char* f) { std::snprintf(b, sizeof(b), "%s.%s", name, f); return b; };
    const int head[3] = {k.side.n, k.n_left, k.n_levels};
    row(nm("n_nleft_nlevels"), head, 3);
    row(nm("desc"), k.side.desc, k.side.n * 32); row(nm("has_mp"), k.side.has_mp, k.side.n); row(nm("stereo"), k.side.stereo, k.side.n);
    row(nm("x"), k.side.x, k.side.n); row(nm("y"), k.side.y, k.side.n); row(nm("octave"), k.side.octave, k.side.n); row(nm("angle"), k.side.angle, k.side.n);
    row(nm("fv.node"), k.side.fv.node_id, k.side.fv.n_nodes); row(nm("fv.offset"), k.side.fv.offset, k.side.fv.n_nodes + 1);
    row(nm("fv.feat"), k.side.fv.feat, k.side.fv.n_nodes ? k.side.fv.offset[k.side.fv.n_nodes] : 0);
    row(nm("Rcw"), &k.Rcw[0][0], 18); row(nm("tcw"), &k.tcw[0][0], 6); row(nm("Ow"), &k.Ow[0][0], 6); row(nm("cam"), &k.cam[0][0], 18); row(nm("mb"), &k.mb, 1);
    row(nm("level_sigma2"), k.level_sigma2, k.n_levels); row(nm("scale_factors"), k.scale_factors, k.n_levels);
}

extern "C" int orbm_create_new_map_points_rig(orbm_matcher* m, const OrbmRigMapKeyFrame* kf1, const OrbmRigMapKeyFrame* neighbours, int n_neighbours,
                                              const OrbmRigMapPair* pairs, const OrbmMapParams* params, OrbmNewPoints* out, uint8_t* skipped)
{
    std::printf("orbm_create_new_map_points_rig handle %d n_neighbours %d inertial %d far_points %d th_far %a scale_factor_1 %a match12 %s skipped %s\n", id_of(m), n_neighbours,
                params->inertial, params->far_points, params->th_far, params->scale_factor_1, out->match12 ? "set" : "NULL", skipped ? "set" : "NULL");
    print_kf("kf1", *kf1);
    for (int j = 0; j < n_neighbours; j++) {
        char b[32];
        std::snprintf(b, sizeof(b), "nb%d", j);
        print_kf(b, neighbours[j]);
        std::snprintf(b, sizeof(b), "pair%d.cam", j); row(b, &pairs[j].geom->cam[0][0], 36);
        std::snprintf(b, sizeof(b), "pair%d.R12", j); row(b, &pairs[j].geom->R12[0][0], 36);
        std::snprintf(b, sizeof(b), "pair%d.t12", j); row(b, &pairs[j].geom->t12[0][0], 12);
        std::snprintf(b, sizeof(b), "pair%d.coarse", j); row(b, &pairs[j].coarse, 1);
    }
    // features 4 and 2 by neighbour 0, features 0 and 1 by neighbour 2; neighbour 1 skipped by the baseline test
    const int nb[5] = {2, 2, 0, -1, 0}, i2[5] = {0, 4, 3, -1, 1};
    for (int i = 0; i < 5; i++) {
        out->neighbour[i] = nb[i]; out->idx2[i] = i2[i];
        for (int c = 0; c < 3; c++) { out->x3d[3 * i + c] = 10.f * i + c; out->normal[3 * i + c] = 0.125f * (i + c); }
        out->max_dist[i] = 100.f + i; out->min_dist[i] = 50.f + i;
    }
    if (skipped && n_neighbours > 1) skipped[1] = 1;
    return 4;
}

// ---- the toy ----
static Sophus::SE3f shift(const Eigen::Vector3f& t) { return Sophus::SE3f(Sophus::SE3f().rotationMatrix(), t); }     // no rotation: R * x + t is x + t to the bit
static Sophus::SE3f quarter_turn(const Eigen::Vector3f& t)      // 90 degrees about z: products with 0 and +-1 are exact
{
    Eigen::Matrix3f R;
    R(0, 1) = -1.f; R(1, 0) = 1.f; R(2, 2) = 1.f;
    return Sophus::SE3f(R, t);
}

static void fill_desc(cv::Mat& d, int rows, int seed)
{
    d.create(rows, 32, CV_8U);
    for (int i = 0; i < rows * 32; i++) d.data[i] = (uint8_t)((i * 7 + seed) & 0xFF);
}

static MapPoint g_point;

// a rig key frame: slots 0 .. 2 left, 3 .. 4 right; mvKeysUn holds NLeft entries of its own that the adapter must not read
static void make_rig_kf(RigMappingKeyFrame& K, int seed, GeometricCamera* cam, GeometricCamera* cam2, const Sophus::SE3f& Tcw, const Eigen::Vector3f& trl)
{
    K.N = 5; K.NLeft = 3; K.mnId = 10 + seed;
    K.mvKeys.resize(3); K.mvKeysUn.resize(3); K.mvKeysRight.resize(2);
    for (int i = 0; i < 3; i++) { K.mvKeys[i] = cv::KeyPoint(100.5f + 10.f * i + seed, 50.25f + i, 31.f, 10.f + i, 0.f, i % 2); K.mvKeysUn[i] = cv::KeyPoint(900.f, 800.f, 31.f, 77.f, 0.f, 2); }
    for (int i = 0; i < 2; i++) K.mvKeysRight[i] = cv::KeyPoint(300.f + i + seed, 250.f - i, 31.f, 200.f + i, 0.f, 2 - i);
    fill_desc(K.mDescriptors, 5, seed);
    K.mFeatVec[3] = {0, 3}; K.mFeatVec[8] = {1, 2, 4};
    K.mvScaleFactors = {1.f, 1.2f, 1.44f}; K.mvLevelSigma2 = {1.f, 1.44f, 2.0736f};
    K.mvuRight.assign(3, -1.f); K.mvDepth.assign(3, -1.f);          // NLeft entries (src/Frame.cc:1257): the adapter must not index them with a right slot
    K.mb = 0.125f + 0.0625f * seed; K.mbf = 19.f; K.mfScaleFactor = 1.2f;
    K.mvpMapPoints = {&g_point, nullptr, nullptr, &g_point, nullptr};
    K.mpCamera = cam; K.mpCamera2 = cam2;
    K.mTcw = Tcw;
    K.mTrl = shift(trl);
}

static void make_conv_kf(RigMappingKeyFrame& K, int seed, GeometricCamera* cam)
{
    K.N = 4; K.NLeft = -1; K.mnId = 10 + seed;
    K.mvKeysUn.resize(4); K.mvKeys.resize(4);
    for (int i = 0; i < 4; i++) K.mvKeys[i] = K.mvKeysUn[i] = cv::KeyPoint(11.f + i, 21.f + i, 31.f, 46.f + i + seed, 0.f, i % 3);
    fill_desc(K.mDescriptors, 4, seed);
    K.mFeatVec[3] = {0, 1}; K.mFeatVec[9] = {2, 3};
    K.mvScaleFactors = {1.f, 1.2f, 1.44f}; K.mvLevelSigma2 = {1.f, 1.44f, 2.0736f};
    K.mvuRight.assign(4, -1.f); K.mvDepth.assign(4, -1.f);
    K.mvpMapPoints.assign(4, nullptr);
    K.fx = 458.f; K.fy = 457.f; K.cx = 367.f; K.cy = 248.f; K.invfx = 1.f / 458.f; K.invfy = 1.f / 457.f;
    K.mpCamera = cam;
    K.mTcw = shift(Eigen::Vector3f(0.125f * seed, 0.f, 0.f));
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const std::string sc = argv[1];
    Pinhole pin(458.f, 457.f, 367.f, 248.f), pin2(300.f, 301.f, 200.f, 201.f);
    KannalaBrandt8Rig fl({190.5f, 190.25f, 254.5f, 256.75f, 0.003f, 0.0007f, -0.002f, 0.0002f}, 1e-6f), fr({191.5f, 191.25f, 252.5f, 254.75f, 0.004f, 0.0018f, -0.0027f, 0.0004f}, 2e-6f);
    KannalaBrandt8Rig gl({290.5f, 290.25f, 354.5f, 356.75f, 0.013f, 0.0107f, -0.012f, 0.0102f}, 3e-6f), gr({291.5f, 291.25f, 352.5f, 354.75f, 0.014f, 0.0118f, -0.0127f, 0.0104f}, 4e-6f);
    const Eigen::Vector3f trl1(-0.125f, 0.015625f, 0.03125f), trl2(-0.25f, 0.0625f, 0.5f);
    std::deque<RigMappingKeyFrame> K(4);
    // all values dyadic so that every float operation of the pose products is exact
    const Sophus::SE3f T[4] = {shift(Eigen::Vector3f(0.25f, -0.5f, 0.75f)), quarter_turn(Eigen::Vector3f(1.5f, 0.125f, -0.375f)), shift(Eigen::Vector3f(-1.f, 0.5f, 2.f)),
                               quarter_turn(Eigen::Vector3f(0.5f, -2.f, 0.25f))};
    for (int q = 0; q < 4; q++) {
        const bool conv = sc == "conv" || (sc == "mixed_kf1" && q == 0) || (sc == "mixed_neighbour" && q == 2);
        if (conv) make_conv_kf(K[q], q, &pin);
        else if (sc == "pinhole_rig" && q == 1) make_rig_kf(K[q], q, &pin, &pin2, T[q], trl2);
        else make_rig_kf(K[q], q, q ? (GeometricCamera*)&gl : (GeometricCamera*)&fl, q ? (GeometricCamera*)&gr : (GeometricCamera*)&fr, T[q], q ? trl2 : trl1);
    }
    std::vector<RigMappingKeyFrame*> nbs = {&K[1], &K[2], &K[3]};
    std::vector<NewMapPointCandidateT<RigMappingKeyFrame> > cand(1);
    std::vector<bool> skipped(7, true);
    const bool ok = CreateNewMapPointsRigHIP<RigMappingKeyFrame, KannalaBrandt8Rig>(&K[0], nbs, true, true, true, 7.5f, cand, &skipped);
    std::printf("handled %d candidates %d skipped", ok ? 1 : 0, (int)cand.size());
    for (bool s : skipped) std::printf(" %d", (int)s);
    std::printf("\n");
    for (const auto& c : cand)
        std::printf("cand %d %d %d %d %a %a %a %a %a %a %a %a\n", c.idx1, (int)(c.pKF2->mnId - 11), c.idx2, c.bPointStereo ? 1 : 0, (double)c.x3D(0), (double)c.x3D(1),
                    (double)c.x3D(2), (double)c.normal(0), (double)c.normal(1), (double)c.normal(2), (double)c.fMaxDistance, (double)c.fMinDistance);
    return 0;
}
