// TEST INFRASTRUCTURE -- drives the graph walks of include/orbslam3_shim_loop.hpp (FlattenEssentialGraph, FlattenEssentialGraphMerge:
// what OptimizeEssentialGraphHIP hands to essg_optimize) on a toy map made of the stand-in types (tests/stubs/standin_*.hpp).
//   loop <case.txt>      the loop overload's graph        merge <case.txt>     the merge overload's graph
//   fallback <case.txt>  OptimizeEssentialGraphHIP (loop) on a case the device refuses: the supplied reference class must be reached
// Prints vertices (id fixed sim3[8]), edges (i j Sji[8]) and points (index ref xyz), doubles in hex.  No device is needed: the walk
// is host code, and the fallback case is refused by the argument checks before anything touches a device.
// tests/test_shim_essential.py writes the case and compares with its own restatement of the walk.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_essential.hpp"
#include "orbslam3_shim_loop.hpp"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <fstream>
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
int Optimizer::PoseInertialOptimizationLastKeyFrame(Frame*, bool) { unreachable("PoseInertialOptimizationLastKeyFrame"); return 0; }
int Optimizer::PoseInertialOptimizationLastFrame(Frame*, bool) { unreachable("PoseInertialOptimizationLastFrame"); return 0; }
Eigen::MatrixXd Optimizer::Marginalize(const Eigen::MatrixXd& H, const int&, const int&) { unreachable("Marginalize"); return H; }

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

typedef std::map<EssKeyFrame*, g2o::Sim3> KeyFrameAndPose;          // LoopClosing::KeyFrameAndPose (include/LoopClosing.h:51-52)
typedef std::map<EssKeyFrame*, std::set<EssKeyFrame*> > Connections;

static int g_ref_calls = 0;
struct RefOptimizer {
    static void OptimizeEssentialGraph(EssMap*, EssKeyFrame*, EssKeyFrame*, const KeyFrameAndPose&, const KeyFrameAndPose&, const Connections&, const bool&) { g_ref_calls++; }
    static void OptimizeEssentialGraph(EssKeyFrame*, std::vector<EssKeyFrame*>&, std::vector<EssKeyFrame*>&, std::vector<EssKeyFrame*>&, std::vector<EssMapPoint*>&) { g_ref_calls += 100; }
};

static void print(const EssentialGraphFlat& g)
{
    std::printf("vertices %zu edges %zu points %zu dropped %d fix_scale %d\n", g.id.size(), g.edges.size() / 2, g.point_ref.size(), g.dropped_edges, g.fix_scale);
    for (size_t k = 0; k < g.id.size(); k++) {
        std::printf("v %lu %d", g.id[k], (int)g.fixed[k]);
        for (int a = 0; a < 8; a++) std::printf(" %a", g.sim3[8 * k + a]);
        std::printf("\n");
    }
    for (size_t e = 0; e < g.edges.size() / 2; e++) {
        std::printf("e %lu %lu", g.id[g.edges[2 * e]], g.id[g.edges[2 * e + 1]]);
        for (int a = 0; a < 8; a++) std::printf(" %a", g.meas[8 * e + a]);
        std::printf("\n");
    }
    for (size_t k = 0; k < g.point_ref.size(); k++)
        std::printf("p %zu %ld %a %a %a\n", g.point_index[k], g.point_ref[k] < 0 ? -1L : (long)g.id[g.point_ref[k]], (double)g.points[3 * k], (double)g.points[3 * k + 1], (double)g.points[3 * k + 2]);
}

static g2o::Sim3 read_sim3(std::istream& in)
{
    double v[8];
    for (double& x : v) in >> x;
    return g2o::Sim3(Eigen::Quaterniond(v[3], v[0], v[1], v[2]), Eigen::Vector3d(v[4], v[5], v[6]), v[7]);
}

// case file: "n_kf init_id loop_id cur_id fix_scale", per key frame "id bad parent_id(-1) imu prev_id(-1) group  q[4](xyzw) t[3]  qb[4] tb[3]" (pose and
// mTcwBefMerge; group: 0 fixed, 1 fixed-corrected, 2 non-fixed, for the merge overload), then "n_w" lines "a b weight", "n_l" lines "a b" (loop edges,
// both directions), "n_nc" lines "id sim3[8]" (NonCorrectedSim3), "n_c" likewise (CorrectedSim3), "n_lc" lines "a b" (LoopConnections),
// "n_mp" lines "bad ref_id corrected_by corrected_reference x y z"
int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: shim_essential_toy loop|merge|fallback case.txt\n"); return 2; }
    const std::string mode = argv[1];
    std::ifstream in(argv[2]);
    if (!in) return 2;
    int n_kf;
    long init_id, loop_id, cur_id;
    int fix_scale;
    in >> n_kf >> init_id >> loop_id >> cur_id >> fix_scale;
    std::deque<EssKeyFrame> kfs(n_kf);
    std::map<long, EssKeyFrame*> by_id;
    std::vector<long> parent(n_kf), prev(n_kf);
    std::vector<int> group(n_kf);
    EssMap map;
    map.mnInitKFid = (unsigned long)init_id;
    for (int k = 0; k < n_kf; k++) {
        EssKeyFrame& kf = kfs[k];
        long id; int bad, imu;
        in >> id >> bad >> parent[k] >> imu >> prev[k] >> group[k];
        kf.mnId = (unsigned long)id; kf.mbBad = bad != 0; kf.bImu = imu != 0; kf.mpMap = &map;
        for (int which = 0; which < 2; which++) {
            double q[4], t[3];
            for (double& x : q) in >> x;
            for (double& x : t) in >> x;
            const Sophus::SE3f T(Eigen::Quaternionf((float)q[3], (float)q[0], (float)q[1], (float)q[2]), Eigen::Vector3f((float)t[0], (float)t[1], (float)t[2]));
            if (which == 0) kf.mTcw = T; else kf.mTcwBefMerge = T;
        }
        by_id[id] = &kf;
        map.kfs.push_back(&kf);
    }
    for (int k = 0; k < n_kf; k++) {
        if (parent[k] >= 0) { kfs[k].mpParent = by_id[parent[k]]; by_id[parent[k]]->mspChildrens.insert(&kfs[k]); }
        if (prev[k] >= 0) kfs[k].mPrevKF = by_id[prev[k]];
    }
    int n;
    in >> n;
    for (int k = 0; k < n; k++) { long a, b; int w; in >> a >> b >> w; by_id[a]->mConnectedKeyFrameWeights[by_id[b]] = w; by_id[b]->mConnectedKeyFrameWeights[by_id[a]] = w; }
    in >> n;
    for (int k = 0; k < n; k++) { long a, b; in >> a >> b; by_id[a]->mspLoopEdges.insert(by_id[b]); by_id[b]->mspLoopEdges.insert(by_id[a]); }
    KeyFrameAndPose non_corrected, corrected;
    in >> n;
    for (int k = 0; k < n; k++) { long a; in >> a; non_corrected[by_id[a]] = read_sim3(in); }
    in >> n;
    for (int k = 0; k < n; k++) { long a; in >> a; corrected[by_id[a]] = read_sim3(in); }
    Connections conn;
    in >> n;
    for (int k = 0; k < n; k++) { long a, b; in >> a >> b; conn[by_id[a]].insert(by_id[b]); }
    in >> n;
    std::deque<EssMapPoint> mps(n);
    for (int k = 0; k < n; k++) {
        int bad; long ref, by, cref; float x, y, z;
        in >> bad >> ref >> by >> cref >> x >> y >> z;
        mps[k].mbBad = bad != 0; mps[k].mpRefKF = by_id[ref]; mps[k].mnCorrectedByKF = (unsigned long)by; mps[k].mnCorrectedReference = (unsigned long)cref;
        mps[k].mWorldPos = Eigen::Vector3f(x, y, z);
        map.mps.push_back(&mps[k]);
    }
    if (!in) { std::fprintf(stderr, "short case file\n"); return 2; }
    EssentialGraphFlat g;
    if (mode == "loop") {
        FlattenEssentialGraph<EssKeyFrame, EssMapPoint>(&map, by_id[loop_id], by_id[cur_id], non_corrected, corrected, conn, fix_scale != 0, g);
        print(g);
    } else if (mode == "merge") {
        std::vector<EssKeyFrame*> grp[3];
        for (int k = 0; k < n_kf; k++) grp[group[k]].push_back(&kfs[k]);
        FlattenEssentialGraphMerge(by_id[cur_id], grp[0], grp[1], grp[2], g);
        print(g);
    } else if (mode == "fallback") {
        const bool fs = fix_scale != 0;
        OptimizeEssentialGraphHIP<RefOptimizer>(&map, by_id[loop_id], by_id[cur_id], non_corrected, corrected, conn, fs);
        std::printf("reference calls %d pose writes %d map changes %d\n", g_ref_calls, kfs[0].nPoseWrites, map.mnMapChange);
    } else {
        return 2;
    }
    return 0;
}
