// TEST INFRASTRUCTURE -- drives the graph walk of include/orbslam3_shim_loop.hpp for the inertial pose graph
// (FlattenEssentialGraph4DoF: what OptimizeEssentialGraph4DoFHIP hands to essg_optimize_4dof) on a toy map made of the stand-in
// types (tests/stubs/standin_*.hpp).
//   walk <case.txt>      the graph                 fallback <case.txt>  OptimizeEssentialGraph4DoFHIP on a case the device refuses
//   capacity <n>         OptimizeEssentialGraph4DoFHIP on a chain of n key frames (n - 1 free)
// fallback and capacity print how often the supplied reference class was reached and what was written to the map.
// Prints vertices (id fixed rcw[9] tcw[3] rwb[9] twb[3] rcb[9] tcb[3] scw[8]), edges (i j dRij[9] dtij[3]) and points (index ref
// xyz), doubles in hex.  No device is needed: the walk is host code, and the refusals come from the argument checks.
// tests/test_shim_essential4dof.py writes the case and compares with its own restatement of the walk.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_essential4dof.hpp"
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

typedef std::map<Ess4KeyFrame*, g2o::Sim3> KeyFrameAndPose;         // LoopClosing::KeyFrameAndPose (include/LoopClosing.h:51-52)
typedef std::map<Ess4KeyFrame*, std::set<Ess4KeyFrame*> > Connections;

static int g_ref_calls = 0;
struct RefOptimizer {
    static void OptimizeEssentialGraph4DoF(Ess4Map*, Ess4KeyFrame*, Ess4KeyFrame*, const KeyFrameAndPose&, const KeyFrameAndPose&, const Connections&) { g_ref_calls++; }
};

static void row(const std::vector<double>& v, size_t k, int w) { for (int a = 0; a < w; a++) std::printf(" %a", v[(size_t)w * k + a]); }

static void print(const EssentialGraph4DoFFlat& g)
{
    std::printf("vertices %zu edges %zu points %zu dropped %d\n", g.id.size(), g.edges.size() / 2, g.point_ref.size(), g.dropped_edges);
    for (size_t k = 0; k < g.id.size(); k++) {
        std::printf("v %lu %d", g.id[k], (int)g.fixed[k]);
        row(g.rcw, k, 9); row(g.tcw, k, 3); row(g.rwb, k, 9); row(g.twb, k, 3); row(g.rcb, k, 9); row(g.tcb, k, 3); row(g.scw, k, 8);
        std::printf("\n");
    }
    for (size_t e = 0; e < g.edges.size() / 2; e++) {
        std::printf("e %lu %lu", g.id[g.edges[2 * e]], g.id[g.edges[2 * e + 1]]);
        row(g.edge_rot, e, 9); row(g.edge_trans, e, 3);
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

static Sophus::SE3f read_pose(std::istream& in)
{
    double q[4], t[3];
    for (double& x : q) in >> x;
    for (double& x : t) in >> x;
    return Sophus::SE3f(Eigen::Quaternionf((float)q[3], (float)q[0], (float)q[1], (float)q[2]), Eigen::Vector3f((float)t[0], (float)t[1], (float)t[2]));
}

static int capacity(int n)
{
    std::deque<Ess4KeyFrame> kfs((size_t)n);
    Ess4Map map;
    for (int k = 0; k < n; k++) {
        kfs[k].mnId = (unsigned long)k; kfs[k].mpMap = &map;
        kfs[k].mRwb = kfs[k].mTcw.rotationMatrix();
        if (k) { kfs[k].mPrevKF = &kfs[k - 1]; kfs[k - 1].mNextKF = &kfs[k]; }
        map.kfs.push_back(&kfs[k]);
    }
    KeyFrameAndPose none;
    Connections conn;
    OptimizeEssentialGraph4DoFHIP<RefOptimizer>(&map, &kfs[0], &kfs[n - 1], none, none, conn);
    std::printf("reference calls %d pose writes %d map changes %d\n", g_ref_calls, kfs[1].nPoseWrites, map.mnMapChange);
    return 0;
}

// case file: "n_kf loop_id cur_id", per key frame "id bad parent_id(-1) prev_id(-1) next_id(-1)  q[4](xyzw) t[3] (pose)  q[4] t[3] (Tcb)
// Rwb[9] twb[3] (row-major)", then "n_w" lines "a b weight", "n_l" lines "a b" (loop edges, both directions), "n_nc" lines
// "id sim3[8]" (NonCorrectedSim3), "n_c" likewise (CorrectedSim3), "n_lc" lines "a b" (LoopConnections), "n_mp" lines "bad ref_id x y z"
int main(int argc, char** argv)
{
    if (argc != 3) { std::fprintf(stderr, "usage: shim_essential4dof_toy walk|fallback case.txt | capacity n\n"); return 2; }
    const std::string mode = argv[1];
    if (mode == "capacity") return capacity(std::atoi(argv[2]));
    std::ifstream in(argv[2]);
    if (!in) return 2;
    int n_kf;
    long loop_id, cur_id;
    in >> n_kf >> loop_id >> cur_id;
    std::deque<Ess4KeyFrame> kfs(n_kf);
    std::map<long, Ess4KeyFrame*> by_id;
    std::vector<long> parent(n_kf), prev(n_kf), next(n_kf);
    Ess4Map map;
    for (int k = 0; k < n_kf; k++) {
        Ess4KeyFrame& kf = kfs[k];
        long id; int bad;
        in >> id >> bad >> parent[k] >> prev[k] >> next[k];
        kf.mnId = (unsigned long)id; kf.mbBad = bad != 0; kf.bImu = true; kf.mpMap = &map;
        kf.mTcw = read_pose(in);
        kf.mImuCalib.mTcb = read_pose(in);
        kf.mImuCalib.mTbc = kf.mImuCalib.mTcb.inverse();
        for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double v; in >> v; kf.mRwb(r, c) = (float)v; }
        for (int r = 0; r < 3; r++) { double v; in >> v; kf.mtwb[r] = (float)v; }
        by_id[id] = &kf;
        map.kfs.push_back(&kf);
    }
    for (int k = 0; k < n_kf; k++) {
        if (parent[k] >= 0) by_id[parent[k]]->mspChildrens.insert(&kfs[k]);
        if (prev[k] >= 0) kfs[k].mPrevKF = by_id[prev[k]];
        if (next[k] >= 0) kfs[k].mNextKF = by_id[next[k]];
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
    std::deque<Ess4MapPoint> mps(n);
    for (int k = 0; k < n; k++) {
        int bad; long ref; float x, y, z;
        in >> bad >> ref >> x >> y >> z;
        mps[k].mbBad = bad != 0; mps[k].mpRefKF = by_id[ref];
        mps[k].mWorldPos = Eigen::Vector3f(x, y, z);
        map.mps.push_back(&mps[k]);
    }
    if (!in) { std::fprintf(stderr, "short case file\n"); return 2; }
    if (mode == "walk") {
        EssentialGraph4DoFFlat g;
        FlattenEssentialGraph4DoF<Ess4KeyFrame, Ess4MapPoint>(&map, by_id[loop_id], by_id[cur_id], non_corrected, corrected, conn, g);
        print(g);
    } else if (mode == "fallback") {
        OptimizeEssentialGraph4DoFHIP<RefOptimizer>(&map, by_id[loop_id], by_id[cur_id], non_corrected, corrected, conn);
        std::printf("reference calls %d pose writes %d map changes %d\n", g_ref_calls, kfs[0].nPoseWrites, map.mnMapChange);
    } else {
        return 2;
    }
    return 0;
}
