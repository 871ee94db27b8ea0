// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_rig_map.hpp (ORBmatcherRigMapHIP) on toy frames and key frames made of the
// stand-in types (tests/stubs/standin_*.hpp) against a RECORDING FAKE of the C entry points defined here: every call prints a line on
// stdout and its arrays, element by element, on the lines after it.  The fakes write fixed matches so that the write-back shows.  No
// device is needed.
//   shim_rig_map_toy <scenario>   bow_rig | bow_rig_convkf | bow_conv_rigkf | bow_conv | kfkf_rig | kfkf_conv | tri_rig | tri_conv |
//                                 tri_mixed | tri_pinhole_rig | fuse_left | fuse_right | fuse_conv | fuse_conv_right
// tests/test_shim_rig_map.py checks the arrays byte for byte, the routing and what was written back.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_rig_map.hpp"
#include "orbslam3_shim_rig_map.hpp"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>

using namespace ORB_SLAM3;

std::mutex MapPoint::mGlobalMutex;

ORBmatcher::ORBmatcher(float, bool) {}
int ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&, const float, const bool, const float) { std::printf("reference SearchByProjection\n"); return -7; }
int ORBmatcher::SearchByProjection(Frame&, const Frame&, const float, const bool) { std::printf("reference SearchByProjection\n"); return -8; }
int ORBmatcher::Fuse(KeyFrame*, const std::vector<MapPoint*>&, const float, const bool bRight) { std::printf("reference Fuse bRight %d\n", (int)bRight); return -9; }
int ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, std::vector<std::pair<size_t, size_t> >&, const bool, const bool) { std::printf("reference SearchForTriangulation\n"); return -10; }
int RigMapReference::SearchByBoW(KeyFrame*, Frame&, std::vector<MapPoint*>&) { std::printf("reference SearchByBoW frame\n"); return -11; }
int RigMapReference::SearchByBoW(KeyFrame*, KeyFrame*, std::vector<MapPoint*>&) { std::printf("reference SearchByBoW key frames\n"); return -12; }

// ---- the recording fake (these definitions take the place of the library's); handle 1, 2, ... in order of creation ----
static int g_handles = 0;
extern "C" const char* orbx_last_error(void) { return "fake"; }
static int id_of(const void* h) { return (int)reinterpret_cast<size_t>(h); }
extern "C" int orbm_create(int, orbm_matcher** out) { *out = reinterpret_cast<orbm_matcher*>((size_t)++g_handles); std::printf("orbm_create handle %d\n", g_handles); return 0; }
extern "C" void orbm_destroy(orbm_matcher* m) { std::printf("orbm_destroy handle %d\n", id_of(m)); }

template <class T>
static void row(const char* name, const T* p, int n)
{
    std::printf(" %s", name);
    if (!p) std::printf(" NULL");
    for (int i = 0; p && i < n; i++) std::printf(" %a", (double)p[i]);
    std::printf("\n");
}

static void print_fv(const char* name, const OrbmFeatVec& fv)
{
    char b[64];
    std::snprintf(b, sizeof(b), "%s.node", name); row(b, fv.node_id, fv.n_nodes);
    std::snprintf(b, sizeof(b), "%s.offset", name); row(b, fv.offset, fv.n_nodes + 1);
    std::snprintf(b, sizeof(b), "%s.feat", name); row(b, fv.feat, fv.n_nodes ? fv.offset[fv.n_nodes] : 0);
}

extern "C" int orbm_search_by_bow(orbm_matcher* m, const uint8_t*, int n_kf, const uint8_t*, const float*, const OrbmFeatVec*, const uint8_t*, int n_f, const float*,
                                  const OrbmFeatVec*, float, int, int32_t*)
{
    std::printf("orbm_search_by_bow handle %d n_kf %d n_f %d\n", id_of(m), n_kf, n_f);
    return 0;
}

extern "C" int orbm_search_by_bow_rig(orbm_matcher* m, const uint8_t* desc_kf, int n_kf, const uint8_t* valid_kf, const float* angle_kf, const OrbmFeatVec* fv_kf,
                                      const uint8_t* desc_f, int n_f, int n_left_f, const float* angle_f, const OrbmFeatVec* fv_f, float nnratio, int check_orientation,
                                      int32_t* match_f2kf)
{
    std::printf("orbm_search_by_bow_rig handle %d n_kf %d n_f %d n_left_f %d nnratio %a check_orientation %d\n", id_of(m), n_kf, n_f, n_left_f, nnratio, check_orientation);
    row("desc_kf", desc_kf, n_kf * 32); row("valid_kf", valid_kf, n_kf); row("angle_kf", angle_kf, n_kf); print_fv("fv_kf", *fv_kf);
    row("desc_f", desc_f, n_f * 32); row("angle_f", angle_f, n_f); print_fv("fv_f", *fv_f); row("match", match_f2kf, n_f);
    match_f2kf[1] = 0; match_f2kf[n_f - 1] = 3;             // a left slot takes key-frame feature 0, the last right slot feature 3
    return 2;
}

extern "C" int orbm_search_by_bow_kfkf(orbm_matcher* m, const uint8_t* desc1, int n1, const uint8_t* valid1, const float* angle1, const OrbmFeatVec* fv1,
                                       const uint8_t* desc2, int n2, const uint8_t* valid2, const float* angle2, const OrbmFeatVec* fv2, float nnratio, int check_orientation,
                                       int32_t* match12)
{
    std::printf("orbm_search_by_bow_kfkf handle %d n1 %d n2 %d nnratio %a check_orientation %d\n", id_of(m), n1, n2, nnratio, check_orientation);
    row("desc1", desc1, n1 * 32); row("valid1", valid1, n1); row("angle1", angle1, n1); print_fv("fv1", *fv1);
    row("desc2", desc2, n2 * 32); row("valid2", valid2, n2); row("angle2", angle2, n2); print_fv("fv2", *fv2);
    match12[0] = 3; match12[n1 - 1] = 0;
    return 2;
}

extern "C" int orbm_search_for_triangulation(orbm_matcher* m, const OrbmTriSide* k1, const OrbmTriSide* k2, float, float, const float*, const float*, const float*, int,
                                             int, int, int, int32_t*)
{
    std::printf("orbm_search_for_triangulation handle %d n1 %d n2 %d\n", id_of(m), k1->n, k2->n);
    return 0;
}

static void print_side(const char* name, const OrbmTriSide* k)
{
    char b[64];
    auto nm = [&](const char* f) { std::snprintf(b, sizeof(b), "%s.%s", name, f); return b; };
    row(nm("desc"), k->desc, k->n * 32); row(nm("has_mp"), k->has_mp, k->n); row(nm("stereo"), k->stereo, k->n); row(nm("x"), k->x, k->n); row(nm("y"), k->y, k->n);
    row(nm("octave"), k->octave, k->n); row(nm("angle"), k->angle, k->n); print_fv(nm("fv"), k->fv);
}

extern "C" int orbm_search_for_triangulation_rig(orbm_matcher* m, const OrbmTriSide* kf1, int n_left_1, const OrbmTriSide* kf2, int n_left_2, const OrbmRigTriGeometry* geom,
                                                 const float* level_sigma2_1, const float* level_sigma2_2, int n_levels, int only_stereo, int coarse, int check_orientation,
                                                 int32_t* match12)
{
    std::printf("orbm_search_for_triangulation_rig handle %d n1 %d n_left_1 %d n2 %d n_left_2 %d n_levels %d only_stereo %d coarse %d check_orientation %d\n", id_of(m),
                kf1->n, n_left_1, kf2->n, n_left_2, n_levels, only_stereo, coarse, check_orientation);
    print_side("kf1", kf1); print_side("kf2", kf2);
    row("cam", &geom->cam[0][0], 36); row("R12", &geom->R12[0][0], 36); row("t12", &geom->t12[0][0], 12);
    row("level_sigma2_1", level_sigma2_1, n_levels); row("level_sigma2_2", level_sigma2_2, n_levels);
    match12[1] = 4; match12[3] = 0;
    return 2;
}

extern "C" int orbm_fuse_search(orbm_matcher* m, const OrbmFrame* kf, const float* u_right, const float* inv_level_sigma2, int n_pts, const uint8_t* valid, const float* proj_u,
                                const float* proj_v, const float* proj_ur, const int32_t* pred_level, const uint8_t* desc_mp, float th, int chi2_check, int32_t* best_idx,
                                int32_t* best_dist)
{
    std::printf("orbm_fuse_search handle %d n %d points %d th %a chi2_check %d grid %d %d bounds %a %a %a %a angle %s frame_u_right %s\n", id_of(m), kf->n, n_pts, th, chi2_check,
                kf->grid_cols, kf->grid_rows, kf->min_x, kf->min_y, kf->max_x, kf->max_y, kf->angle ? "set" : "NULL", kf->u_right ? "set" : "NULL");
    row("x", kf->x, kf->n); row("y", kf->y, kf->n); row("octave", kf->octave, kf->n); row("desc", kf->desc, kf->n * 32); row("scale_factors", kf->scale_factors, kf->n_levels);
    row("u_right", u_right, kf->n); row("inv_level_sigma2", inv_level_sigma2, kf->n_levels);
    row("valid", valid, n_pts); row("proj_u", proj_u, n_pts); row("proj_v", proj_v, n_pts); row("proj_ur", proj_ur, n_pts); row("pred_level", pred_level, n_pts);
    row("desc_mp", desc_mp, n_pts * 32);
    for (int i = 0; i < n_pts; i++) { best_idx[i] = -1; best_dist[i] = 256; }
    if (n_pts >= 3) { best_idx[0] = 1; best_dist[0] = 10; best_idx[1] = 0; best_dist[1] = 50; best_idx[2] = 0; best_dist[2] = 51; }
    return 0;
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

static std::deque<MapPoint> g_kf_points;

// a rig key frame: slots 0 .. 2 left, 3 .. 4 right; mvKeysUn holds NLeft entries with angles of its own
static void make_rig_kf(RigMapKeyFrame& K, int seed, GeometricCamera* cam, GeometricCamera* cam2, const Sophus::SE3f& Tcw)
{
    K.N = 5; K.NLeft = 3;
    K.mvKeys.resize(3); K.mvKeysUn.resize(3); K.mvKeysRight.resize(2);
    for (int i = 0; i < 3; i++) { K.mvKeys[i] = cv::KeyPoint(100.5f + 10.f * i + seed, 50.25f + i, 31.f, 10.f + i + seed, 0.f, i % 2); K.mvKeysUn[i] = cv::KeyPoint(900.f, 800.f, 31.f, 77.f + i, 0.f, 5); }
    for (int i = 0; i < 2; i++) K.mvKeysRight[i] = cv::KeyPoint(300.f + i + seed, 250.f - i, 31.f, 200.f + i + seed, 0.f, 2 - i);
    fill_desc(K.mDescriptors, 5, seed);
    K.mFeatVec[3] = {0, 3}; K.mFeatVec[8] = {1, 2, 4};
    K.mnMinX = 0.f; K.mnMinY = 0.f; K.mnMaxX = 752.f; K.mnMaxY = 480.f;
    K.mvScaleFactors = {1.f, 1.2f, 1.44f}; K.mvLevelSigma2 = {1.f, 1.44f, 2.0736f}; K.mvInvLevelSigma2 = {1.f, 0.5f + 0.1f * seed, 0.25f};
    K.mvuRight.assign(3, -1.f);                                         // NLeft entries of -1 (src/Frame.cc:1257)
    K.mbf = 19.f;
    const size_t first = g_kf_points.size();
    g_kf_points.resize(first + 4);
    g_kf_points[first + 1].mbBad = true;
    K.mvpMapPoints = {&g_kf_points[first], nullptr, &g_kf_points[first + 1], &g_kf_points[first + 2], &g_kf_points[first + 3]};
    K.mpCamera = cam; K.mpCamera2 = cam2;
    K.mTcw = Tcw;
    K.mTrl = shift(Eigen::Vector3f(-0.125f, 0.015625f, 0.03125f));
}

static void make_conv_kf(RigMapKeyFrame& K, int seed, GeometricCamera* cam)
{
    K.N = 4; K.NLeft = -1;
    K.mvKeysUn.resize(4);
    for (int i = 0; i < 4; i++) K.mvKeysUn[i] = cv::KeyPoint(11.f + i, 21.f + i, 31.f, 46.f + i + seed, 0.f, i % 3);
    fill_desc(K.mDescriptors, 4, seed);
    K.mFeatVec[3] = {0, 1}; K.mFeatVec[9] = {2, 3};
    K.mnMaxX = 752.f; K.mnMaxY = 480.f;
    K.mvScaleFactors = {1.f, 1.2f, 1.44f}; K.mvLevelSigma2 = {1.f, 1.44f, 2.0736f}; K.mvInvLevelSigma2 = {1.f, 0.5f, 0.25f};
    K.mvuRight.assign(4, -1.f);
    const size_t first = g_kf_points.size();
    g_kf_points.resize(first + 3);
    K.mvpMapPoints = {&g_kf_points[first], &g_kf_points[first + 1], nullptr, &g_kf_points[first + 2]};
    K.mpCamera = cam;
    K.mTcw = shift(Eigen::Vector3f(0.f, 0.f, 0.f));
}

static void make_rig_frame(RigMatchFrame& F, GeometricCamera* cam, GeometricCamera* cam2)
{
    F.N = 6; F.Nleft = 4;                                           // slots 0 .. 3 left, 4 .. 5 right
    F.mvKeys.resize(4); F.mvKeysRight.resize(2); F.mvKeysUn.resize(4);
    for (int i = 0; i < 4; i++) { F.mvKeys[i] = cv::KeyPoint(1.f, 2.f, 31.f, 20.f + i, 0.f, 0); F.mvKeysUn[i] = cv::KeyPoint(3.f, 4.f, 31.f, 120.f + i, 0.f, 0); }
    for (int i = 0; i < 2; i++) F.mvKeysRight[i] = cv::KeyPoint(5.f, 6.f, 31.f, 220.f + i, 0.f, 0);
    fill_desc(F.mDescriptors, 6, 5);
    F.mFeatVec[3] = {4, 0}; F.mFeatVec[7] = {1, 5, 2, 3};
    F.mvpMapPoints.assign(6, nullptr);
    F.mpCamera = cam; F.mpCamera2 = cam2;
}

static void make_conv_frame(Frame& F, GeometricCamera* cam)
{
    F.N = 2; F.Nleft = -1;
    F.mvKeys.resize(2); F.mvKeysUn.resize(2);
    fill_desc(F.mDescriptors, 2, 9);
    F.mFeatVec[3] = {0, 1};
    F.mvpMapPoints.assign(2, nullptr);
    F.mpCamera = cam;
}

static int id_in(const std::deque<MapPoint>& pts, MapPoint* p)
{
    for (size_t k = 0; k < pts.size(); k++) if (p == &pts[k]) return (int)k;
    return -1;
}

typedef ORBmatcherRigMapHIP<RigMatchFrame, RigMapKeyFrame, RigMatchMapPoint, KannalaBrandt8Rig, RigMapReference> Matcher;

static int run_bow(const std::string& sc)
{
    Pinhole pin(458.f, 457.f, 367.f, 248.f), pin2(300.f, 301.f, 200.f, 201.f);
    RigMapKeyFrame K;
    if (sc == "bow_rig" || sc == "bow_conv_rigkf") make_rig_kf(K, 1, &pin, &pin2, shift(Eigen::Vector3f(0.f, 0.f, 0.f)));
    else make_conv_kf(K, 1, &pin);
    Matcher matcher(0.75f, true);
    std::vector<MapPoint*> out(1, nullptr);
    if (sc == "bow_conv" || sc == "bow_conv_rigkf") {
        Frame F;
        make_conv_frame(F, &pin);
        std::printf("returned %d\n", matcher.SearchByBoW(&K, F, out));
        return 0;
    }
    RigMatchFrame F;
    make_rig_frame(F, &pin, &pin2);
    const int n = matcher.SearchByBoW(&K, F, out);
    std::printf("returned %d matches", n);
    for (MapPoint* p : out) std::printf(" %d", id_in(g_kf_points, p));
    std::printf("\n");
    return 0;
}

static int run_kfkf(const std::string& sc)
{
    Pinhole pin(458.f, 457.f, 367.f, 248.f), pin2(300.f, 301.f, 200.f, 201.f);
    RigMapKeyFrame K1, K2;
    if (sc == "kfkf_rig") { make_rig_kf(K1, 1, &pin, &pin2, shift(Eigen::Vector3f(0.f, 0.f, 0.f))); make_rig_kf(K2, 2, &pin, &pin2, shift(Eigen::Vector3f(0.f, 0.f, 0.f))); }
    else { make_conv_kf(K1, 1, &pin); make_conv_kf(K2, 2, &pin); }
    Matcher matcher(0.75f, true);
    std::vector<MapPoint*> out;
    const int n = matcher.SearchByBoW(&K1, &K2, out);
    std::printf("returned %d matches", n);
    for (MapPoint* p : out) std::printf(" %d", id_in(g_kf_points, p));
    std::printf("\n");
    return 0;
}

static int run_tri(const std::string& sc)
{
    Pinhole pin(458.f, 457.f, 367.f, 248.f), pin2(300.f, 301.f, 200.f, 201.f);
    KannalaBrandt8Rig fl({190.5f, 190.25f, 254.5f, 256.75f, 0.003f, 0.0007f, -0.002f, 0.0002f}, 1e-6f), fr({191.5f, 191.25f, 252.5f, 254.75f, 0.004f, 0.0018f, -0.0027f, 0.0004f}, 2e-6f);
    KannalaBrandt8Rig gl({290.5f, 290.25f, 354.5f, 356.75f, 0.013f, 0.0107f, -0.012f, 0.0102f}, 3e-6f), gr({291.5f, 291.25f, 352.5f, 354.75f, 0.014f, 0.0118f, -0.0127f, 0.0104f}, 4e-6f);
    RigMapKeyFrame K1, K2;
    const Sophus::SE3f T1 = shift(Eigen::Vector3f(0.25f, -0.5f, 0.75f)), T2 = quarter_turn(Eigen::Vector3f(1.5f, 0.125f, -0.375f));
    if (sc == "tri_rig") { make_rig_kf(K1, 1, &fl, &fr, T1); make_rig_kf(K2, 2, &gl, &gr, T2); }
    else if (sc == "tri_pinhole_rig") { make_rig_kf(K1, 1, &pin, &pin2, T1); make_rig_kf(K2, 2, &gl, &gr, T2); }
    else if (sc == "tri_mixed") { make_rig_kf(K1, 1, &fl, &fr, T1); make_conv_kf(K2, 2, &pin); }
    else { make_conv_kf(K1, 1, &pin); make_conv_kf(K2, 2, &pin); }
    K2.mTrl = shift(Eigen::Vector3f(-0.25f, 0.0625f, 0.5f));
    Matcher matcher(0.75f, false);
    std::vector<std::pair<size_t, size_t> > pairs(1);
    const int n = matcher.SearchForTriangulation(&K1, &K2, pairs, false, true);
    std::printf("returned %d pairs", n);
    for (const auto& p : pairs) std::printf(" %zu %zu", p.first, p.second);
    std::printf("\n");
    return 0;
}

static int run_fuse(const std::string& sc)
{
    Pinhole pin(458.f, 457.f, 367.f, 248.f), pin2(300.f, 301.f, 200.f, 201.f);
    RigMapKeyFrame K;
    if (sc == "fuse_left" || sc == "fuse_right") make_rig_kf(K, 1, &pin, &pin2, shift(Eigen::Vector3f(0.25f, -0.5f, -0.5f)));
    else make_conv_kf(K, 1, &pin);
    // four points: 0 and 1 visible, 2 visible but too far in descriptor space (the fake says 51), 3 behind the camera
    std::deque<MapPoint> pts(4);
    std::vector<MapPoint*> v;
    for (int k = 0; k < 4; k++) {
        pts[k].mWorldPos = Eigen::Vector3f(0.125f * k, -0.25f * k, k == 3 ? -2.f : 2.f + k);
        pts[k].mNormal = Eigen::Vector3f(0.f, 0.f, 1.f);
        pts[k].mnPredicted = k % 3; pts[k].nObs = k;
        fill_desc(pts[k].mDescriptor, 1, 60 + k);
        v.push_back(&pts[k]);
    }
    Matcher matcher(0.75f, true);
    const bool right = sc == "fuse_right" || sc == "fuse_conv_right";
    const int n = matcher.Fuse(&K, v, 2.5f, right);
    std::printf("returned %d slots", n);
    for (MapPoint* p : K.mvpMapPoints) std::printf(" %d", p ? (id_in(pts, p) >= 0 ? id_in(pts, p) : 100 + id_in(g_kf_points, p)) : -1);
    std::printf("\nreplaced");
    for (const MapPoint& p : g_kf_points) std::printf(" %d", p.mpReplaced ? id_in(pts, p.mpReplaced) : -1);
    std::printf("\nobservations");
    for (const MapPoint& p : pts) std::printf(" %d", p.mObservations.count(&K) ? std::get<0>(p.mObservations.at(&K)) : -1);
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const std::string sc = argv[1];
    if (sc.compare(0, 3, "bow") == 0) return run_bow(sc);
    if (sc.compare(0, 4, "kfkf") == 0) return run_kfkf(sc);
    if (sc.compare(0, 3, "tri") == 0) return run_tri(sc);
    return run_fuse(sc);
}
