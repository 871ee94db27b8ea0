// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_rig_match.hpp (ORBmatcherRigHIP) on toy frames made of the stand-in types
// (tests/stubs/standin_*.hpp) against a RECORDING FAKE of the C entry points defined here: every call prints a line on stdout and
// its arrays, element by element, on the lines after it; record_abi.hpp's length / hash / first / last lines go to stderr.  The
// fakes write fixed assignments so that the write-back shows.  No device is needed.
//   shim_rig_match_toy <scenario>    mp_rig | mp_conv | last_rig_rig | last_rig_conv | last_rig_mono | last_conv | last_conv_from_rig
// tests/test_shim_rig_match.py checks the arrays byte for byte, the delegation and what was written back.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_rig_match.hpp"
#include "orbslam3_shim_rig_match.hpp"
#include "record_abi.hpp"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>

using namespace ORB_SLAM3;

std::mutex MapPoint::mGlobalMutex;

static void unreachable(const char* what) { std::fprintf(stderr, "reference fallback called: %s\n", what); std::exit(40); }
ORBmatcher::ORBmatcher(float, bool) {}
int ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&, const float, const bool, const float) { std::printf("reference SearchByProjection map points\n"); return -7; }
int ORBmatcher::SearchByProjection(Frame&, const Frame&, const float, const bool) { std::printf("reference SearchByProjection last frame\n"); return -8; }
int ORBmatcher::Fuse(KeyFrame*, const std::vector<MapPoint*>&, const float, const bool) { unreachable("Fuse"); return 0; }
int ORBmatcher::SearchForTriangulation(KeyFrame*, KeyFrame*, std::vector<std::pair<size_t, size_t> >&, const bool, const bool) { unreachable("SearchForTriangulation"); return 0; }

// ---- the recording fake (these definitions take the place of the library's); handle 1, 2, ... in order of creation ----
static int g_handles = 0;
extern "C" const char* orbx_last_error(void) { return "fake"; }
static int id_of(const void* h) { return (int)reinterpret_cast<size_t>(h); }
extern "C" int orbm_create(int, orbm_matcher** out) { *out = reinterpret_cast<orbm_matcher*>((size_t)++g_handles); std::printf("orbm_create handle %d\n", g_handles); return 0; }
extern "C" void orbm_destroy(orbm_matcher* m) { std::printf("orbm_destroy handle %d\n", id_of(m)); }

template <class T>
static void row(const char* name, const T* p, int n)
{
    record_abi::array(name, p, (size_t)n);
    std::printf(" %s", name);
    if (!p) std::printf(" NULL");
    for (int i = 0; p && i < n; i++) std::printf(" %a", (double)p[i]);
    std::printf("\n");
}

static void print_frame(const char* name, const OrbmFrame& f)
{
    std::printf(" %s n %d bounds %a %a %a %a grid %d %d levels %d u_right %s\n", name, f.n, f.min_x, f.min_y, f.max_x, f.max_y, f.grid_cols, f.grid_rows, f.n_levels,
                f.u_right ? "set" : "NULL");
    row("x", f.x, f.n); row("y", f.y, f.n); row("octave", f.octave, f.n); row("angle", f.angle, f.n); row("desc", f.desc, f.n * 32);
    row("scale_factors", f.scale_factors, f.n_levels);
}

static void print_rig(const OrbmRigFrame* r, const int32_t* assign, const uint8_t* occupied)
{
    print_frame("left", r->left); print_frame("right", r->right);
    row("left_to_right", r->left_to_right, r->left.n); row("right_to_left", r->right_to_left, r->right.n);
    row("assign", assign, r->left.n + r->right.n); row("occupied", occupied, r->left.n + r->right.n);
}

extern "C" int orbm_search_by_projection_rig(orbm_matcher* m, const OrbmRigFrame* r, const OrbmRigMapPoints* p, float th, int far_points, float th_far, float nnratio,
                                             int32_t* assign, uint8_t* occupied)
{
    std::printf("orbm_search_by_projection_rig handle %d n %d th %a far %d th_far %a nnratio %a\n", id_of(m), p->n, th, far_points, th_far, nnratio);
    print_rig(r, assign, occupied);
    row("in_view", p->in_view, p->n); row("proj_u", p->proj_u, p->n); row("proj_v", p->proj_v, p->n); row("pred_level", p->pred_level, p->n); row("view_cos", p->view_cos, p->n);
    row("in_view_r", p->in_view_r, p->n); row("proj_u_r", p->proj_u_r, p->n); row("proj_v_r", p->proj_v_r, p->n); row("pred_level_r", p->pred_level_r, p->n);
    row("view_cos_r", p->view_cos_r, p->n); row("track_depth", p->track_depth, p->n); row("bad", p->bad, p->n); row("has_obs", p->has_obs, p->n);
    row("pts_desc", p->desc, p->n * 32);
    assign[0] = 2; assign[3] = 0; assign[4] = 1;            // left slot 0, right slots 0 and 1
    return 3;
}

extern "C" int orbm_search_by_projection_last_rig(orbm_matcher* m, const OrbmRigFrame* r, const OrbmRigLastPoints* p, float th, int level_window, int check_orientation,
                                                  int32_t* assign, uint8_t* occupied)
{
    std::printf("orbm_search_by_projection_last_rig handle %d n %d th %a level_window %d check_orientation %d\n", id_of(m), p->n, th, level_window, check_orientation);
    print_rig(r, assign, occupied);
    row("valid", p->valid, p->n); row("proj_u", p->proj_u, p->n); row("proj_v", p->proj_v, p->n); row("proj_u_r", p->proj_u_r, p->n); row("proj_v_r", p->proj_v_r, p->n);
    row("pts_octave", p->octave, p->n); row("pts_angle", p->angle, p->n); row("has_obs", p->has_obs, p->n); row("pts_desc", p->desc, p->n * 32);
    assign[1] = 0; assign[3] = -1;                          // left slot 1 takes entry 0; right slot 0 is nulled by the rotation check
    return 1;
}

extern "C" int orbm_search_by_projection(orbm_matcher* m, const OrbmFrame* f, int n_mp, const uint8_t*, const float*, const float*, const float*, const int32_t*, const float*,
                                         const float*, const uint8_t*, const uint8_t*, const uint8_t*, float th, int, float, float, int32_t*, uint8_t*)
{
    std::printf("orbm_search_by_projection handle %d n %d points %d th %a\n", id_of(m), f->n, n_mp, th);
    return 0;
}

extern "C" int orbm_search_by_projection_last(orbm_matcher* m, const OrbmFrame* cur, int n_last, const uint8_t*, const float*, const float*, const float*, const int32_t*,
                                              const float*, const uint8_t*, const uint8_t*, float th, int level_window, int, int32_t*, uint8_t*)
{
    std::printf("orbm_search_by_projection_last handle %d n %d entries %d th %a level_window %d\n", id_of(m), cur->n, n_last, th, level_window);
    return 0;
}

// ---- the toy ----
static Sophus::SE3f shift(const Eigen::Vector3f& t) { return Sophus::SE3f(Sophus::SE3f().rotationMatrix(), t); }     // no rotation: R * x + t is x + t to the bit

static void fill_desc(cv::Mat& d, int rows, int seed)
{
    d.create(rows, 32, CV_8U);
    for (int i = 0; i < rows * 32; i++) d.data[i] = (uint8_t)((i * 7 + seed) & 0xFF);
}

static void make_rig_frame(RigMatchFrame& F, std::deque<RigMatchMapPoint>& held, GeometricCamera* cam, GeometricCamera* cam2)
{
    F.N = 5; F.Nleft = 3;                                           // slots 0..2 left, 3..4 right
    F.mvKeys.resize(3); F.mvKeysRight.resize(2); F.mvKeysUn.resize(3);
    for (int i = 0; i < 3; i++) { F.mvKeys[i] = cv::KeyPoint(100.5f + 10.f * i, 50.25f + i, 31.f, 10.f + i, 0.f, i % 2); F.mvKeysUn[i] = cv::KeyPoint(900.f, 800.f, 31.f, 77.f, 0.f, 5); }
    for (int i = 0; i < 2; i++) F.mvKeysRight[i] = cv::KeyPoint(300.f + i, 250.f - i, 31.f, 200.f + i, 0.f, 2 - i);
    fill_desc(F.mDescriptors, 5, 3);
    F.mvLeftToRightMatch = {1, -1, 0}; F.mvRightToLeftMatch = {2, 0};
    F.mnMinX = 0.f; F.mnMinY = 0.f; F.mnMaxX = 512.f; F.mnMaxY = 512.f;
    F.mvScaleFactors = {1.f, 1.2f, 1.44f};
    F.mb = 0.1f; F.mbf = 19.f;
    F.mvuRight.assign(5, -1.f); F.mvbOutlier.assign(5, false); F.mvpMapPoints.assign(5, nullptr);
    held.resize(2);
    held[0].nObs = 2; held[1].nObs = 0;
    F.mvpMapPoints[1] = &held[0];                                   // occupied
    F.mvpMapPoints[4] = &held[1];                                   // held, but by a point without observations: not occupied
    F.mpCamera = cam; F.mpCamera2 = cam2;
    F.mTrl = shift(Eigen::Vector3f(-0.1f, 0.01f, 0.02f));
    F.SetPose(shift(Eigen::Vector3f(0.25f, -0.5f, -0.5f)));
}

static void make_conventional_frame(Frame& F, GeometricCamera* cam)
{
    F.N = 2; F.Nleft = -1;
    F.mvKeys.resize(2); F.mvKeysUn.resize(2);
    for (int i = 0; i < 2; i++) { F.mvKeys[i] = cv::KeyPoint(10.f + i, 20.f + i, 31.f, 45.f, 0.f, i); F.mvKeysUn[i] = cv::KeyPoint(11.f + i, 21.f + i, 31.f, 46.f + i, 0.f, i); }
    fill_desc(F.mDescriptors, 2, 9);
    F.mnMaxX = 512.f; F.mnMaxY = 512.f;
    F.mvScaleFactors = {1.f, 1.2f, 1.44f};
    F.mb = 0.1f; F.mbf = 19.f;
    F.mvuRight.assign(2, -1.f); F.mvbOutlier.assign(2, false); F.mvpMapPoints.assign(2, nullptr);
    F.mpCamera = cam;
    F.SetPose(shift(Eigen::Vector3f(0.f, 0.f, 0.f)));
}

static void print_slots(const char* what, int n, Frame& F, const std::deque<RigMatchMapPoint>& pts, const std::deque<RigMatchMapPoint>& held)
{
    std::printf("%s %d slots", what, n);
    for (MapPoint* p : F.mvpMapPoints) {
        int id = -1;                                                // NULL
        for (size_t k = 0; k < pts.size(); k++) if (p == &pts[k]) id = (int)k;
        for (size_t k = 0; k < held.size(); k++) if (p == &held[k]) id = 100 + (int)k;
        std::printf(" %d", id);
    }
    std::printf("\n");
}

static int run_mp(const std::string& sc)
{
    Pinhole pin(458.f, 457.f, 367.f, 248.f), pin2(300.f, 301.f, 200.f, 201.f);
    std::deque<RigMatchMapPoint> pts(3), held;
    std::vector<MapPoint*> v;
    for (int k = 0; k < 3; k++) {
        RigMatchMapPoint& p = pts[k];
        p.mbTrackInView = k != 1; p.mTrackProjX = 100.f + k; p.mTrackProjY = 50.f + k; p.mnTrackScaleLevel = k; p.mTrackViewCos = 0.9f + 0.03f * k;
        p.mbTrackInViewR = k != 0; p.mTrackProjXR = 300.f + k; p.mTrackProjYR = 250.f + k; p.mnTrackScaleLevelR = k - 1; p.mTrackViewCosR = 0.99f + 0.004f * k;
        p.mTrackDepth = 5.f + k; p.mbBad = k == 2; p.nObs = k;
        fill_desc(p.mDescriptor, 1, 40 + k);
        v.push_back(&p);
    }
    ORBmatcherRigHIP<RigMatchFrame, RigMatchMapPoint> matcher(0.8f, true);
    if (sc == "mp_conv") {
        Frame F;
        make_conventional_frame(F, &pin);
        const int n = matcher.SearchByProjection(F, v, 3.f, true, 40.f);
        std::printf("returned %d\n", n);
        return 0;
    }
    RigMatchFrame F;
    make_rig_frame(F, held, &pin, &pin2);
    const int n = matcher.SearchByProjection(F, v, 3.f, true, 40.f);
    print_slots("returned", n, F, pts, held);
    return 0;
}

static int run_last(const std::string& sc)
{
    Pinhole pin(458.f, 457.f, 367.f, 248.f), pin2(300.f, 301.f, 200.f, 201.f);
    std::deque<RigMatchMapPoint> pts(4), held, none;
    for (int k = 0; k < 4; k++) {
        pts[k].mWorldPos = Eigen::Vector3f(0.1f * k, -0.2f * k, k == 3 ? -2.f : 2.f + k);     // entry 3 ends up behind the camera
        pts[k].nObs = k % 2;
        fill_desc(pts[k].mDescriptor, 1, 60 + k);
    }
    // the last frame: a rig frame (entries 0, 1 from mvKeys, 2 .. 4 from mvKeysRight) or a conventional one (5 entries of mvKeys / mvKeysUn)
    const bool last_rig = sc == "last_rig_rig" || sc == "last_rig_mono" || sc == "last_conv_from_rig";
    RigMatchFrame Last;
    Last.N = 5; Last.Nleft = last_rig ? 2 : -1;
    Last.mvKeys.resize(last_rig ? 2 : 5); Last.mvKeysUn.resize(last_rig ? 2 : 5); Last.mvKeysRight.resize(last_rig ? 3 : 0);
    for (size_t i = 0; i < Last.mvKeys.size(); i++) { Last.mvKeys[i] = cv::KeyPoint(1.f, 2.f, 31.f, 30.f + i, 0.f, (int)i % 3); Last.mvKeysUn[i] = cv::KeyPoint(1.f, 2.f, 31.f, 130.f + i, 0.f, 7); }
    for (size_t i = 0; i < Last.mvKeysRight.size(); i++) Last.mvKeysRight[i] = cv::KeyPoint(3.f, 4.f, 31.f, 230.f + i, 0.f, 2 - (int)i % 3);
    Last.mvpMapPoints = {&pts[0], nullptr, &pts[1], &pts[2], &pts[3]};
    Last.mvbOutlier = {false, false, false, true, false};          // entry 1 has no point, entry 3 is an outlier, entry 4 is behind the camera
    Last.SetPose(shift(Eigen::Vector3f(0.f, 0.f, 0.f)));
    ORBmatcherRigHIP<RigMatchFrame, RigMatchMapPoint> matcher(0.8f, false);
    if (sc == "last_conv" || sc == "last_conv_from_rig") {
        Frame F;
        make_conventional_frame(F, &pin);
        const int n = matcher.SearchByProjection(F, Last, 7.f, false);
        std::printf("returned %d\n", n);
        return 0;
    }
    RigMatchFrame F;
    make_rig_frame(F, held, &pin, &pin2);
    const int n = matcher.SearchByProjection(F, Last, 7.f, sc == "last_rig_mono");
    print_slots("returned", n, F, pts, held);
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const std::string sc = argv[1];
    return sc.compare(0, 2, "mp") == 0 ? run_mp(sc) : run_last(sc);
}
