// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_track_project_rig.hpp (TrackProjectRigHIP) on toy rig frames made of the
// stand-in types (tests/stubs/standin_*.hpp) against a RECORDING FAKE of the C entry points defined here: every call prints a line
// on stdout and its arrays, element by element, on the lines after it; record_abi.hpp's length / hash / first / last lines go to
// stderr.  The fakes write fixed results so that the write-back shows.  No device is needed.
//   shim_track_project_rig_toy <scenario>    frustum | frustum_pinhole | frustum_empty | last | last_mono
// tests/test_shim_track_project_rig.py checks the arrays byte for byte, the routing and what was written back.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_track_project_rig.hpp"
#include "orbslam3_shim_track_project_rig.hpp"
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
int ORBmatcher::SearchByProjection(Frame&, const Frame&, const float, const bool) { unreachable("SearchByProjection last frame"); return 0; }
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

static void print_camera_and_pose(const OrbmTrackRigCamera* c, const OrbmRigFramePose* p)
{
    row("cam_left", c->left, 8); row("cam_right", c->right, 8); row("Rrl", c->Rrl, 9); row("trl", c->trl, 3); row("tlr", c->tlr, 3); row("q_rl", c->q_rl, 4);
    const float b[5] = {c->min_x, c->min_y, c->max_x, c->max_y, c->log_scale_factor};
    row("bounds", b, 5);
    std::printf(" n_levels %d\n", c->n_levels);
    row("q", p->left.q, 4); row("Rcw", p->left.Rcw, 9); row("tcw", p->left.tcw, 3); row("Ow", p->left.Ow, 3);
    row("Rwc", p->Rwc, 9); row("R_r", p->R_r, 9); row("t_r", p->t_r, 3); row("Ow_r", p->Ow_r, 3);
}

extern "C" int orbm_frustum_rig_batch(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const OrbmLocalPoints* pts, float viewing_cos_limit,
                                      const OrbmRigFrustumOut* out, int batch)
{
    const int n = pts->n[0];
    std::printf("orbm_frustum_rig_batch handle %d batch %d pcap %d n %d cos_limit %a\n", id_of(m), batch, pts->pcap, n, viewing_cos_limit);
    print_camera_and_pose(cam, poses);
    row("xyz", pts->xyz, n * 3); row("normal", pts->normal, n * 3); row("min_distance", pts->min_distance, n); row("max_distance", pts->max_distance, n);
    row("skip", pts->skip, n); row("bad", pts->bad, n);
    // the stale members as they came in
    row("in_proj_u", out->proj_u, n); row("in_proj_v", out->proj_v, n); row("in_view_cos", out->view_cos, n); row("in_track_depth", out->track_depth, n);
    row("in_proj_u_r", out->proj_u_r, n); row("in_proj_v_r", out->proj_v_r, n); row("in_view_cos_r", out->view_cos_r, n); row("in_track_depth_r", out->track_depth_r, n);
    row("in_pred_level", out->pred_level, n); row("in_pred_level_r", out->pred_level_r, n);
    // as the library: point 0 seen by both cameras, 1 by the left only, 2 by the right only, 3 by neither; 4 and 5 are skipped / bad
    const int seen[6] = {1, 1, 0, 0, 0, 0}, seen_r[6] = {1, 0, 1, 0, 0, 0};
    for (int i = 0; i < n && i < 6; i++) {
        out->in_view[i] = seen[i]; out->in_view_r[i] = seen_r[i];
        if (i >= 4) continue;
        out->pred_level[i] = seen[i] ? 2 : -1; out->pred_level_r[i] = seen_r[i] ? 1 : -1;
        if (seen[i]) { out->proj_u[i] = 101.5f + i; out->proj_v[i] = 11.25f + i; out->view_cos[i] = 0.75f; out->track_depth[i] = 4.5f + i; }
        if (seen_r[i]) { out->proj_u_r[i] = 301.5f + i; out->proj_v_r[i] = 31.25f + i; out->view_cos_r[i] = 0.875f; out->track_depth_r[i] = 6.5f + i; }
    }
    out->n_to_match[0] = 3;
    return 0;
}

extern "C" int orbm_frustum_batch(orbm_matcher* m, const OrbmTrackCamera*, const OrbmFramePose*, const OrbmLocalPoints* pts, float, const OrbmFrustumOut* out, int)
{
    std::printf("orbm_frustum_batch handle %d n %d\n", id_of(m), pts->n[0]);
    for (int i = 0; i < pts->n[0]; i++) { out->valid[i] = 0; out->u[i] = -1.f; out->v[i] = -1.f; out->octave[i] = -1; }
    out->n_to_match[0] = 0;
    return 0;
}
extern "C" int orbm_project_last_batch(orbm_matcher*, const OrbmTrackCamera*, const OrbmFramePose*, const float*, const uint8_t*, const int32_t*, int, const OrbmLastProjOut*, int)
{ unreachable("orbm_project_last_batch"); return 0; }
extern "C" int orbm_search_by_projection_last(orbm_matcher*, const OrbmFrame*, int, const uint8_t*, const float*, const float*, const float*, const int32_t*, const float*,
                                              const uint8_t*, const uint8_t*, float, int, int, int32_t*, uint8_t*)
{ unreachable("orbm_search_by_projection_last"); return 0; }
extern "C" int orbm_search_by_projection_rig(orbm_matcher*, const OrbmRigFrame*, const OrbmRigMapPoints*, float, int, float, float, int32_t*, uint8_t*)
{ unreachable("orbm_search_by_projection_rig"); return 0; }

extern "C" int orbm_project_last_rig_batch(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const float* mp_xyz, const uint8_t* has_point,
                                           const int32_t* n, int cap, const OrbmRigLastProjOut* out, int batch)
{
    std::printf("orbm_project_last_rig_batch handle %d batch %d cap %d n %d\n", id_of(m), batch, cap, n[0]);
    print_camera_and_pose(cam, poses);
    row("xyz", mp_xyz, n[0] * 3); row("has_point", has_point, n[0]);
    for (int i = 0; i < n[0]; i++) {                    // entry 2 is behind the camera
        const bool ok = has_point[i] && i != 2;
        out->valid[i] = ok; out->proj_u[i] = ok ? 50.5f + i : -1.f; out->proj_v[i] = ok ? 60.5f + i : -1.f; out->proj_u_r[i] = ok ? 70.5f + i : -1.f; out->proj_v_r[i] = ok ? 80.5f + i : -1.f;
    }
    return 0;
}

extern "C" int orbm_search_by_projection_last_rig(orbm_matcher* m, const OrbmRigFrame* r, const OrbmRigLastPoints* p, float th, int level_window, int check_orientation,
                                                  int32_t* assign, uint8_t* occupied)
{
    std::printf("orbm_search_by_projection_last_rig handle %d left %d right %d entries %d th %a level_window %d check_orientation %d\n", id_of(m), r->left.n, r->right.n, p->n, th,
                level_window, check_orientation);
    row("valid", p->valid, p->n); row("proj_u", p->proj_u, p->n); row("proj_v", p->proj_v, p->n); row("proj_u_r", p->proj_u_r, p->n); row("proj_v_r", p->proj_v_r, p->n);
    row("pts_octave", p->octave, p->n); row("pts_angle", p->angle, p->n); row("has_obs", p->has_obs, p->n); row("pts_desc", p->desc, p->n * 32);
    row("occupied", occupied, r->left.n + r->right.n);
    assign[0] = 4; assign[2] = -1;                          // left slot 0 takes entry 4; right slot 2 is nulled by the rotation check
    return 1;
}

// ---- the toy ----
static void fill_desc(cv::Mat& d, int rows, int seed)
{
    d.create(rows, 32, CV_8U);
    for (int i = 0; i < rows * 32; i++) d.data[i] = (uint8_t)((i * 7 + seed) & 0xFF);
}

static void make_frame(TrackProjectRigFrame& F, GeometricCamera* cam, GeometricCamera* cam2, bool rig)
{
    F.N = 3; F.Nleft = rig ? 2 : -1;
    F.mvKeys.resize(rig ? 2 : 3); F.mvKeysUn.resize(rig ? 0 : 3); F.mvKeysRight.resize(rig ? 1 : 0);
    for (size_t i = 0; i < F.mvKeys.size(); i++) F.mvKeys[i] = cv::KeyPoint(10.f + i, 20.f + i, 31.f, 45.f, 0.f, (int)i);
    for (size_t i = 0; i < F.mvKeysUn.size(); i++) F.mvKeysUn[i] = cv::KeyPoint(11.5f + i, 21.f + i, 31.f, 46.f + i, 0.f, (int)i);
    for (size_t i = 0; i < F.mvKeysRight.size(); i++) F.mvKeysRight[i] = cv::KeyPoint(30.f + i, 40.f + i, 31.f, 47.f, 0.f, 1);
    fill_desc(F.mDescriptors, 3, 9);
    F.mvLeftToRightMatch.assign(2, -1); F.mvRightToLeftMatch.assign(1, -1);
    F.mnMinX = -3.f; F.mnMinY = -2.f; F.mnMaxX = 515.f; F.mnMaxY = 514.f;
    F.mvScaleFactors = {1.f, 1.2f, 1.44f};
    F.mnScaleLevels = 3; F.mfLogScaleFactor = 0.18232156f;
    F.mb = 0.1f; F.mbf = 19.f;
    F.mvuRight.assign(3, -1.f); F.mvbOutlier.assign(3, false); F.mvpMapPoints.assign(3, nullptr);
    F.mpCamera = cam; F.mpCamera2 = cam2;
    F.mnId = 17;
    Eigen::Matrix3f R;                                              // a quarter turn about z: every entry and the quaternion's halves are exact
    R(0, 1) = -1.f; R(1, 0) = 1.f; R(2, 2) = 1.f;
    F.SetPose(Sophus::SE3f(R, Eigen::Vector3f(0.25f, -0.5f, 1.5f)));
    F.mOw = Eigen::Vector3f(0.5f, 0.25f, -1.5f);
    F.mRwc = Eigen::Matrix3f();
    F.mRwc(0, 1) = 1.f; F.mRwc(1, 0) = -1.f; F.mRwc(2, 2) = 1.f;
    Eigen::Matrix3f Rrl;                                            // a quarter turn about y
    Rrl(0, 2) = -1.f; Rrl(1, 1) = 1.f; Rrl(2, 0) = 1.f;
    F.mTrl = Sophus::SE3f(Rrl, Eigen::Vector3f(-0.125f, 0.f, 0.0625f));
    F.mtlr = Eigen::Vector3f(0.0625f, 0.f, 0.125f);
}

static int run_frustum(const std::string& sc)
{
    KannalaBrandt8 left({190.5f, 191.5f, 254.f, 256.f, 0.5f, 0.25f, -0.125f, 0.0625f}), right({188.5f, 189.5f, 252.f, 255.f, 0.25f, 0.125f, -0.0625f, 0.03125f});
    std::deque<TrackProjectRigMapPoint> pts(sc == "frustum_empty" ? 0 : 6);
    std::vector<MapPoint*> v;
    for (size_t k = 0; k < pts.size(); k++) {
        TrackProjectRigMapPoint& p = pts[k];
        p.mnId = 100 + k;
        p.mWorldPos = Eigen::Vector3f(0.5f * k, 1.f - 0.25f * k, 3.f + k); p.mNormal = Eigen::Vector3f(0.f, 0.6f, 0.8f - 0.125f * k);
        p.mfMinDistance = 0.5f + k; p.mfMaxDistance = 20.f + k;
        p.mnLastFrameSeen = k == 4 ? 17 : 16; p.mbBad = k == 5;
        // what an earlier frame left behind
        p.mbTrackInView = true; p.mTrackProjX = 900.f + k; p.mTrackProjY = 910.f + k; p.mTrackDepth = 920.f + k; p.mnTrackScaleLevel = 9; p.mTrackViewCos = 0.125f;
        p.mbTrackInViewR = true; p.mTrackProjXR = 930.f + k; p.mTrackProjYR = 940.f + k; p.mTrackDepthR = 950.f + k; p.mnTrackScaleLevelR = 8; p.mTrackViewCosR = 0.25f;
        v.push_back(&p);
    }
    TrackProjectRigFrame F;
    make_frame(F, &left, &right, sc != "frustum_pinhole");
    TrackProjectRigHIP<TrackProjectRigFrame, TrackProjectRigMapPoint> tp(0.9f, true);
    const int n = tp.SearchLocalPointsProjectHIP(F, v, 0.5f);
    std::printf("returned %d reference_calls %d\n", n, F.nReferenceFrustum);
    for (const TrackProjectRigMapPoint& p : pts)
        std::printf(" point %lu in_view %d x %a y %a depth %a level %d cos %a in_view_r %d xr %a yr %a depth_r %a level_r %d cos_r %a visible %d\n", p.mnId, (int)p.mbTrackInView,
                    p.mTrackProjX, p.mTrackProjY, p.mTrackDepth, p.mnTrackScaleLevel, p.mTrackViewCos, (int)p.mbTrackInViewR, p.mTrackProjXR, p.mTrackProjYR, p.mTrackDepthR,
                    p.mnTrackScaleLevelR, p.mTrackViewCosR, p.nVisible);
    for (const auto& kv : F.mmProjectPoints) std::printf(" project_point %lu %a %a\n", kv.first, kv.second.x, kv.second.y);
    return 0;
}

static int run_last(const std::string& sc)
{
    KannalaBrandt8 left({190.5f, 191.5f, 254.f, 256.f, 0.5f, 0.25f, -0.125f, 0.0625f}), right({188.5f, 189.5f, 252.f, 255.f, 0.25f, 0.125f, -0.0625f, 0.03125f});
    std::deque<TrackProjectRigMapPoint> pts(4);
    for (int k = 0; k < 4; k++) {
        pts[k].mWorldPos = Eigen::Vector3f(0.1f * k, -0.2f * k, 2.f + k);
        pts[k].nObs = k % 2;
        fill_desc(pts[k].mDescriptor, 1, 60 + k);
    }
    TrackProjectRigFrame Last;                                      // a rig last frame: 3 left + 2 right entries
    make_frame(Last, &left, &right, true);
    Last.N = 5; Last.Nleft = 3;
    Last.mvKeys.resize(3); Last.mvKeysRight.resize(2);
    for (int i = 0; i < 3; i++) Last.mvKeys[i] = cv::KeyPoint(1.f, 2.f, 31.f, 30.f + i, 0.f, i % 3);
    for (int i = 0; i < 2; i++) Last.mvKeysRight[i] = cv::KeyPoint(1.f, 2.f, 31.f, 230.f + i, 0.f, 2 - i);
    Last.mvpMapPoints = {&pts[0], nullptr, &pts[1], &pts[2], &pts[3]};
    Last.mvbOutlier = {false, false, false, true, false};          // entry 1 has no point, entry 3 is an outlier
    Last.SetPose(Sophus::SE3f(Sophus::SE3f().rotationMatrix(), Eigen::Vector3f(0.f, 0.f, 0.f)));
    TrackProjectRigFrame F;
    make_frame(F, &left, &right, true);
    std::deque<TrackProjectRigMapPoint> held(1);
    held[0].nObs = 2;
    F.mvpMapPoints[1] = &held[0];
    TrackProjectRigHIP<TrackProjectRigFrame, TrackProjectRigMapPoint> tp(0.9f, false);
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
