// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_track_project.hpp (TrackProjectHIP) on toy frames made of the stand-in types
// (tests/stubs/standin_*.hpp) against a RECORDING FAKE of the C entry points defined here: every call prints a line on stdout and
// its arrays, element by element, on the lines after it; record_abi.hpp's length / hash / first / last lines go to stderr.  The
// fakes write fixed results so that the write-back shows.  No device is needed.
//   shim_track_project_toy <scenario>    frustum | frustum_rig | frustum_empty | last | last_rig
// tests/test_shim_track_project.py checks the arrays byte for byte, the routing and what was written back.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_track_project.hpp"
#include "orbslam3_shim_track_project.hpp"
#include "record_abi.hpp"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <string>

using namespace ORB_SLAM3;

std::mutex MapPoint::mGlobalMutex;

static void unreachable(const char* what) { std::fprintf(stderr, "reference fallback called: %s\n", what); std::exit(40); }
ORBmatcher::ORBmatcher(float, bool) {}
int ORBmatcher::SearchByProjection(Frame&, const std::vector<MapPoint*>&, const float, const bool, const float) { unreachable("SearchByProjection map points"); return 0; }
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

static void print_camera_and_pose(const OrbmTrackCamera* c, const OrbmFramePose* p)
{
    const float cam[10] = {c->fx, c->fy, c->cx, c->cy, c->bf, c->min_x, c->min_y, c->max_x, c->max_y, c->log_scale_factor};
    row("camera", cam, 10);
    std::printf(" n_levels %d\n", c->n_levels);
    row("q", p->q, 4); row("Rcw", p->Rcw, 9); row("tcw", p->tcw, 3); row("Ow", p->Ow, 3);
}

extern "C" int orbm_frustum_batch(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* poses, const OrbmLocalPoints* pts, float viewing_cos_limit,
                                  const OrbmFrustumOut* out, int batch)
{
    const int n = pts->n[0];
    std::printf("orbm_frustum_batch handle %d batch %d pcap %d n %d cos_limit %a\n", id_of(m), batch, pts->pcap, n, viewing_cos_limit);
    print_camera_and_pose(cam, poses);
    row("xyz", pts->xyz, n * 3); row("normal", pts->normal, n * 3); row("min_distance", pts->min_distance, n); row("max_distance", pts->max_distance, n);
    row("skip", pts->skip, n); row("bad", pts->bad, n);
    // point 0 in view, point 1 rejected after the bounds test (its projection stays), point 2 outside the image; 3 and 4 are skipped / bad
    const uint8_t valid[5] = {1, 0, 0, 0, 0};
    const float u[5] = {101.5f, 202.5f, -1.f, -1.f, -1.f}, v[5] = {11.25f, 22.25f, -1.f, -1.f, -1.f};
    for (int i = 0; i < n && i < 5; i++) {
        out->valid[i] = valid[i]; out->u[i] = u[i]; out->v[i] = v[i]; out->octave[i] = valid[i] ? 3 : -1;
        out->view_cos[i] = valid[i] ? 0.75f : 0.f; out->track_depth[i] = valid[i] ? 4.5f : 0.f; out->proj_ur[i] = valid[i] ? 95.5f : 0.f;
    }
    out->n_to_match[0] = 1;
    return 0;
}

extern "C" int orbm_project_last_batch(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* poses, const float* mp_xyz, const uint8_t* has_point,
                                       const int32_t* n, int cap, const OrbmLastProjOut* out, int batch)
{
    std::printf("orbm_project_last_batch handle %d batch %d cap %d n %d\n", id_of(m), batch, cap, n[0]);
    print_camera_and_pose(cam, poses);
    row("xyz", mp_xyz, n[0] * 3); row("has_point", has_point, n[0]);
    for (int i = 0; i < n[0]; i++) { out->valid[i] = has_point[i] && i != 2; out->u[i] = out->valid[i] ? 50.5f + i : -1.f; out->v[i] = out->valid[i] ? 60.5f + i : -1.f; out->proj_ur[i] = out->valid[i] ? 40.5f + i : 0.f; }
    return 0;
}

extern "C" int orbm_search_by_projection_last(orbm_matcher* m, const OrbmFrame* cur, int n_last, const uint8_t* valid, const float* u, const float* v, const float* ur,
                                              const int32_t* octave, const float* angle, const uint8_t* desc, const uint8_t* has_obs, float th, int level_window,
                                              int check_orientation, int32_t* assign, uint8_t* occupied)
{
    std::printf("orbm_search_by_projection_last handle %d n %d entries %d th %a level_window %d check_orientation %d\n", id_of(m), cur->n, n_last, th, level_window, check_orientation);
    row("valid", valid, n_last); row("proj_u", u, n_last); row("proj_v", v, n_last); row("proj_ur", ur, n_last); row("pts_octave", octave, n_last);
    row("pts_angle", angle, n_last); row("has_obs", has_obs, n_last); row("pts_desc", desc, n_last * 32);
    row("cur_x", cur->x, cur->n); row("occupied", occupied, cur->n);
    assign[0] = 3; assign[1] = -1;                          // feature 0 takes entry 3; feature 1 is nulled by the rotation check
    return 1;
}

// ---- the toy ----
static void fill_desc(cv::Mat& d, int rows, int seed)
{
    d.create(rows, 32, CV_8U);
    for (int i = 0; i < rows * 32; i++) d.data[i] = (uint8_t)((i * 7 + seed) & 0xFF);
}

static void make_frame(TrackProjectFrame& F, GeometricCamera* cam, bool rig)
{
    F.N = 2; F.Nleft = rig ? 1 : -1;
    F.mvKeys.resize(2); F.mvKeysUn.resize(2);
    for (int i = 0; i < 2; i++) { F.mvKeys[i] = cv::KeyPoint(10.f + i, 20.f + i, 31.f, 45.f, 0.f, i); F.mvKeysUn[i] = cv::KeyPoint(11.5f + i, 21.f + i, 31.f, 46.f + i, 0.f, i); }
    fill_desc(F.mDescriptors, 2, 9);
    F.mnMinX = -3.f; F.mnMinY = -2.f; F.mnMaxX = 755.f; F.mnMaxY = 483.f;
    F.mvScaleFactors = {1.f, 1.2f, 1.44f};
    F.mnScaleLevels = 3; F.mfLogScaleFactor = 0.18232156f;
    F.fx = 458.5f; F.fy = 457.25f; F.cx = 367.125f; F.cy = 248.375f; F.mb = 0.1f; F.mbf = 47.75f;
    F.mvuRight.assign(2, -1.f); F.mvbOutlier.assign(2, false); F.mvpMapPoints.assign(2, nullptr);
    F.mpCamera = cam;
    F.mnId = 17;
    Eigen::Matrix3f R;                                              // a quarter turn about z: every entry and the quaternion's halves are exact
    R(0, 1) = -1.f; R(1, 0) = 1.f; R(2, 2) = 1.f;
    F.SetPose(Sophus::SE3f(R, Eigen::Vector3f(0.25f, -0.5f, 1.5f)));
    F.mOw = Eigen::Vector3f(0.5f, 0.25f, -1.5f);
}

static int run_frustum(const std::string& sc)
{
    Pinhole pin(458.5f, 457.25f, 367.125f, 248.375f);
    std::deque<TrackProjectMapPoint> pts(sc == "frustum_empty" ? 0 : 5);
    std::vector<MapPoint*> v;
    for (size_t k = 0; k < pts.size(); k++) {
        TrackProjectMapPoint& p = pts[k];
        p.mnId = 100 + k;
        p.mWorldPos = Eigen::Vector3f(0.5f * k, 1.f - 0.25f * k, 3.f + k); p.mNormal = Eigen::Vector3f(0.f, 0.6f, 0.8f - 0.125f * k);
        p.mfMinDistance = 0.5f + k; p.mfMaxDistance = 20.f + k;
        p.mnLastFrameSeen = k == 3 ? 17 : 16; p.mbBad = k == 4;
        p.mbTrackInView = true; p.mTrackProjX = 900.f; p.mTrackProjY = 901.f; p.mTrackProjXR = 902.f; p.mTrackDepth = 903.f; p.mnTrackScaleLevel = 9; p.mTrackViewCos = 0.125f;    // stale
        v.push_back(&p);
    }
    TrackProjectFrame F;
    make_frame(F, &pin, sc == "frustum_rig");
    TrackProjectHIP<TrackProjectFrame, TrackProjectMapPoint> tp(0.9f, true);
    const int n = tp.SearchLocalPointsProjectHIP(F, v, 0.5f);
    std::printf("returned %d reference_calls %d\n", n, F.nReferenceFrustum);
    for (const TrackProjectMapPoint& p : pts)
        std::printf(" point %lu in_view %d x %a y %a xr %a depth %a level %d cos %a visible %d\n", p.mnId, (int)p.mbTrackInView, p.mTrackProjX, p.mTrackProjY, p.mTrackProjXR,
                    p.mTrackDepth, p.mnTrackScaleLevel, p.mTrackViewCos, p.nVisible);
    for (const auto& kv : F.mmProjectPoints) std::printf(" project_point %lu %a %a\n", kv.first, kv.second.x, kv.second.y);
    return 0;
}

static int run_last(const std::string& sc)
{
    Pinhole pin(458.5f, 457.25f, 367.125f, 248.375f);
    std::deque<TrackProjectMapPoint> pts(4);
    for (int k = 0; k < 4; k++) {
        pts[k].mWorldPos = Eigen::Vector3f(0.1f * k, -0.2f * k, 2.f + k);
        pts[k].nObs = k % 2;
        fill_desc(pts[k].mDescriptor, 1, 60 + k);
    }
    TrackProjectFrame Last;
    make_frame(Last, &pin, false);
    Last.N = 5;
    Last.mvKeys.resize(5); Last.mvKeysUn.resize(5);
    for (int i = 0; i < 5; i++) { Last.mvKeys[i] = cv::KeyPoint(1.f, 2.f, 31.f, 30.f + i, 0.f, i % 3); Last.mvKeysUn[i] = cv::KeyPoint(1.f, 2.f, 31.f, 130.f + i, 0.f, 7); }
    Last.mvpMapPoints = {&pts[0], nullptr, &pts[1], &pts[2], &pts[3]};
    Last.mvbOutlier = {false, false, false, true, false};          // entry 1 has no point, entry 3 is an outlier
    Last.SetPose(Sophus::SE3f(Sophus::SE3f().rotationMatrix(), Eigen::Vector3f(0.f, 0.f, 0.f)));
    TrackProjectFrame F;
    make_frame(F, &pin, sc == "last_rig");
    std::deque<TrackProjectMapPoint> held(1);
    held[0].nObs = 2;
    F.mvpMapPoints[1] = &held[0];
    TrackProjectHIP<TrackProjectFrame, TrackProjectMapPoint> tp(0.9f, false);
    const int n = tp.SearchByProjection(F, Last, 7.f, sc == "last_mono");
    std::printf("returned %d slots", n);
    for (MapPoint* p : F.mvpMapPoints) {
        int id = -1;
        for (size_t k = 0; k < pts.size(); k++) if (p == &pts[k]) id = (int)k;
        if (p == &held[0]) id = 100;
        std::printf(" %d", id);
    }
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    const std::string sc = argv[1];
    return sc.compare(0, 7, "frustum") == 0 ? run_frustum(sc) : run_last(sc);
}
