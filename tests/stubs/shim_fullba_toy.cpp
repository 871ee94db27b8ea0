// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_fullba.hpp (FullInertialBAHIP: the walk FlattenFullInertialBA, the
// write-back, the early returns and the fallback) on a toy map made of the stand-in types (tests/stubs/standin_*.hpp) against a
// RECORDING FAKE of fiba_solve defined here: it prints the problem it is handed and returns the inputs moved by fixed amounts
// (twb + 0.5, vel + 0.25, biases + 0.125 / + 0.0625 -- with a shared bias the shared values, for every key frame with IMU states --
// points + 1).  No device is needed.
//   shim_fullba_toy <case.txt> its bFixLocal nLoopId stop(-1 none, 0 lowered, 1 raised) bInit priorG priorA
// prints "call ..." lines (the problem), then the state of every key frame and map point and the counters.  Doubles and floats in hex.
// tests/test_shim_fullba.py writes the case and compares with its own restatement of src/Optimizer.cc:392-811.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_fullba.hpp"
#include "orbslam3_shim_fullba.hpp"
#include "record_abi.hpp"

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

static int g_ref_calls = 0, g_solve_calls = 0;
struct RefOptimizer {
    static void FullInertialBA(FbaMap*, int, bool, unsigned long, bool*, bool, float, float) { g_ref_calls++; }
};

// ---- the recording fake (these definitions take the place of the library's) ----
extern "C" int fiba_create(int, fiba_solver** out) { *out = reinterpret_cast<fiba_solver*>(&g_solve_calls); return 0; }
extern "C" int fiba_check(const FibaProblem* p) { return p->n_kf > 1000 ? ORBX_ERR_CAPACITY : 0; }
extern "C" int fiba_solve(fiba_solver*, const FibaProblem* p, const FibaOutputs* o, LbaStats* st)
{
    g_solve_calls++;
    record_abi::dump(*p);           // stderr: the whole struct, for tests/test_shim_abi_golden.py
    std::printf("call n_kf %d n_points %d n_edges %d n_links %d shared %d its %d lambda %a priors %a %a stop %d huber %a %a %a cam %a %a %a %a %a\n", p->n_kf, p->n_points,
                p->n_edges, p->n_links, (int)p->shared_bias, p->max_iters, p->lambda_init, p->prior_g, p->prior_a, p->stop_flag ? (int)*p->stop_flag : -1, p->huber_mono,
                p->huber_stereo, p->huber_inertial, p->fx, p->fy, p->cx, p->cy, p->bf);
    std::printf("call shared_bias %a %a %a %a %a %a\n", p->shared_bg[0], p->shared_bg[1], p->shared_bg[2], p->shared_ba[0], p->shared_ba[1], p->shared_ba[2]);
    for (int i = 0; i < p->n_kf; i++) {
        std::printf("call kf %d %d %d %d", i, (int)p->pose_fixed[i], (int)p->has_imu[i], (int)p->imu_fixed[i]);
        for (int a = 0; a < 9; a++) std::printf(" %a", p->Rwb[9 * i + a]);
        for (int a = 0; a < 3; a++) std::printf(" %a", p->twb[3 * i + a]);
        for (int a = 0; a < 3; a++) std::printf(" %a", p->vel[3 * i + a]);
        for (int a = 0; a < 3; a++) std::printf(" %a", p->bg[3 * i + a]);
        for (int a = 0; a < 3; a++) std::printf(" %a", p->ba[3 * i + a]);
        std::printf("\n");
    }
    for (int l = 0; l < p->n_links; l++) {
        const LibaLink& L = p->links[l];
        std::printf("call link %d %d %d %a", L.kf1, L.kf2, (int)L.robust, (double)L.dT);
        const float* f[] = {L.dR, L.dV, L.dP, L.JRg, L.JVg, L.JVa, L.JPg, L.JPa, L.bias0};
        const int nf[] = {9, 3, 3, 9, 9, 9, 9, 9, 6};
        for (int a = 0; a < 9; a++) for (int k = 0; k < nf[a]; k++) std::printf(" %a", (double)f[a][k]);
        for (int k = 0; k < 81; k++) std::printf(" %a", L.info9[k]);
        for (int k = 0; k < 9; k++) std::printf(" %a", L.info_gyro[k]);
        for (int k = 0; k < 9; k++) std::printf(" %a", L.info_acc[k]);
        std::printf("\n");
    }
    for (int e = 0; e < p->n_edges; e++)
        std::printf("call edge %d %d %a %a %a %a %d\n", p->edge_kf[e], p->edge_point[e], p->edge_obs[3 * e], p->edge_obs[3 * e + 1], p->edge_obs[3 * e + 2], p->edge_inv_sigma2[e],
                    (int)p->edge_stereo[e]);
    for (int i = 0; i < p->n_kf; i++) {
        for (int a = 0; a < 9; a++) o->Rwb[9 * i + a] = p->Rwb[9 * i + a];
        for (int a = 0; a < 3; a++) {
            o->twb[3 * i + a] = p->twb[3 * i + a] + 0.5; o->vel[3 * i + a] = p->vel[3 * i + a] + 0.25;
            const bool sh = p->shared_bias && p->has_imu[i];
            o->bg[3 * i + a] = (sh ? p->shared_bg[a] : p->bg[3 * i + a]) + 0.125; o->ba[3 * i + a] = (sh ? p->shared_ba[a] : p->ba[3 * i + a]) + 0.0625;
        }
    }
    for (int i = 0; i < 3 * p->n_points; i++) o->points[i] = p->points[i] + 1.0;
    std::memset(st, 0, sizeof(*st));
    return 0;
}

template <class M> static void read3x3(std::istream& in, M& m) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double v; in >> v; m(r, c) = (float)v; } }
template <class V> static void read3(std::istream& in, V& v) { for (int r = 0; r < 3; r++) { double x; in >> x; v[r] = (float)x; } }
static IMU::Bias read_bias(std::istream& in) { double b[6]; for (double& x : b) in >> x; return IMU::Bias((float)b[0], (float)b[1], (float)b[2], (float)b[3], (float)b[4], (float)b[5]); }

// case file: "n_kf maxKFid n_mp", per key frame "id bad prev_id(-1) bImu camera2 mnBALocalForKF mnBAFixedForKF has_preintegration
// Rwb[9] twb[3] vel[3] bias[6](ba, bg) n_keys {x y octave uRight}" and, with a pre-integration, "dT dR[9] dV[3] dP[3] JRg[9] JVg[9]
// JVa[9] JPg[9] JPa[9] b[6] C[225]"; per map point "id X[3] n_obs {kf_id leftIndex}"
int main(int argc, char** argv)
{
    if (argc < 9) { std::fprintf(stderr, "usage: shim_fullba_toy case.txt its bFixLocal nLoopId stop bInit priorG priorA\n"); return 2; }
    std::ifstream in(argv[1]);
    if (!in) return 2;
    const int its = std::atoi(argv[2]), stop = std::atoi(argv[5]);
    const bool bFixLocal = std::atoi(argv[3]) != 0, bInit = std::atoi(argv[6]) != 0;
    const unsigned long nLoopId = std::strtoul(argv[4], nullptr, 10);
    const float priorG = (float)std::atof(argv[7]), priorA = (float)std::atof(argv[8]);
    int n_kf, n_mp;
    long max_id;
    in >> n_kf >> max_id >> n_mp;
    std::deque<FbaKeyFrame> kfs(n_kf);
    std::deque<IMU::Preintegrated> pre(n_kf);
    std::deque<MapPoint> mps(n_mp);
    std::map<long, FbaKeyFrame*> by_id;
    std::vector<long> prev(n_kf);
    Pinhole cam2(1.f, 1.f, 0.f, 0.f);
    FbaMap map;
    map.mnMaxKFid = (unsigned long)max_id;
    for (int k = 0; k < n_kf; k++) {
        FbaKeyFrame& kf = kfs[k];
        long id; int bad, imu, c2, has, n_keys; unsigned long bal, baf;
        in >> id >> bad >> prev[k] >> imu >> c2 >> bal >> baf >> has;
        kf.mnId = (unsigned long)id; kf.mbBad = bad != 0; kf.bImu = imu != 0; kf.mpMap = &map; kf.mnBALocalForKF = bal; kf.mnBAFixedForKF = baf;
        if (c2) kf.mpCamera2 = &cam2;
        kf.fx = 400.f; kf.fy = 410.f; kf.cx = 320.f; kf.cy = 240.f; kf.mbf = 40.f;
        kf.mvInvLevelSigma2 = {1.f, 0.5f, 0.25f};
        read3x3(in, kf.mRwb); read3(in, kf.mtwb); read3(in, kf.mVw);
        kf.mImuBias = read_bias(in);
        in >> n_keys;
        for (int j = 0; j < n_keys; j++) { double x, y, ur; int oct; in >> x >> y >> oct >> ur; cv::KeyPoint kp; kp.pt.x = (float)x; kp.pt.y = (float)y; kp.octave = oct; kf.mvKeysUn.push_back(kp); kf.mvuRight.push_back((float)ur); }
        if (has) {
            IMU::Preintegrated& p = pre[k];
            double dT; in >> dT; p.dT = (float)dT;
            read3x3(in, p.dR); read3(in, p.dV); read3(in, p.dP);
            read3x3(in, p.JRg); read3x3(in, p.JVg); read3x3(in, p.JVa); read3x3(in, p.JPg); read3x3(in, p.JPa);
            p.b = read_bias(in);
            for (int r = 0; r < 15; r++) for (int c = 0; c < 15; c++) { double v; in >> v; p.C(r, c) = (float)v; }
            kf.mpImuPreintegrated = &p;
        }
        by_id[id] = &kf;
        map.kfs.push_back(&kf);
    }
    for (int k = 0; k < n_kf; k++) if (prev[k] >= 0) kfs[k].mPrevKF = by_id[prev[k]];
    for (int i = 0; i < n_mp; i++) {
        MapPoint& mp = mps[i];
        long id; int n_obs;
        in >> id; mp.mnId = (unsigned long)id;
        read3(in, mp.mWorldPos);
        in >> n_obs;
        for (int j = 0; j < n_obs; j++) { long kid; int li; in >> kid >> li; mp.mObservations[by_id[kid]] = std::tuple<int, int>(li, -1); }
        map.mvpAllMapPoints.push_back(&mp);
    }
    if (!in) { std::fprintf(stderr, "short case file\n"); return 2; }
    bool flag = stop == 1;
    FullInertialBAHIP<RefOptimizer>(&map, its, bFixLocal, nLoopId, stop < 0 ? nullptr : &flag, bInit, priorG, priorA);
    std::printf("calls solve %d reference %d change %d\n", g_solve_calls, g_ref_calls, map.mnMapChange);
    for (const FbaKeyFrame& k : kfs) {
        std::printf("state %lu %d %d %d %lu", k.mnId, k.nPoseWrites, k.nVelocityWrites, k.nBiasWrites, k.mnBAGlobalForKF);
        const Sophus::SE3f T[2] = {k.mTcw, k.mTcwGBA};
        for (int w = 0; w < 2; w++) {
            const Eigen::Matrix3f R = T[w].rotationMatrix();
            for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) std::printf(" %a", (double)R(r, c));
            for (int r = 0; r < 3; r++) std::printf(" %a", (double)T[w].translation()[r]);
        }
        for (int r = 0; r < 3; r++) std::printf(" %a", (double)k.mVw[r]);
        for (int r = 0; r < 3; r++) std::printf(" %a", (double)k.mVwbGBA[r]);
        const IMU::Bias B[2] = {k.mImuBias, k.mBiasGBA};
        for (int w = 0; w < 2; w++) std::printf(" %a %a %a %a %a %a", (double)B[w].bax, (double)B[w].bay, (double)B[w].baz, (double)B[w].bwx, (double)B[w].bwy, (double)B[w].bwz);
        std::printf("\n");
    }
    for (const IMU::Preintegrated& p : pre) std::printf("bu %a %a %a %a %a %a\n", (double)p.bu.bax, (double)p.bu.bay, (double)p.bu.baz, (double)p.bu.bwx, (double)p.bu.bwy, (double)p.bu.bwz);
    for (const MapPoint& m : mps)
        std::printf("point %lu %d %lu %a %a %a %a %a %a\n", m.mnId, m.nNormalUpdates, m.mnBAGlobalForKF, (double)m.mWorldPos[0], (double)m.mWorldPos[1], (double)m.mWorldPos[2],
                    (double)m.mPosGBA[0], (double)m.mPosGBA[1], (double)m.mPosGBA[2]);
    return 0;
}
