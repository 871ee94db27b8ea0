// TEST INFRASTRUCTURE -- drives the host code of include/orbslam3_shim_imu_init.hpp (the walk FlattenInertialOptimization, the
// write-back imu_init_detail::write_back and the fallback of the three InertialOptimizationHIP overloads) on a toy map made of
// the stand-in types (tests/stubs/standin_*.hpp).
//   walk <case.txt> <overload 1|2|3>       the flattened problem and the bias every pre-integration was given
//   writeback <case.txt>                   write_back with the bias and velocities at the end of the case file
//   fallback <case.txt> <overload 1|2|3>   InertialOptimizationHIP on a case the device refuses
// writeback and fallback print the state of every key frame: velocity, bias, the numbers of velocity / bias writes and of
// re-integrations; fallback also how often the supplied reference class was reached.  Doubles and floats in hex.
// No device is needed: the walk and the write-back are host code, and the refusals come from the argument checks.
// tests/test_shim_imu_init.py writes the case and compares with its own restatement.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_imu_init.hpp"
#include "orbslam3_shim_imu_init.hpp"
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

static int g_ref_calls[3] = {0, 0, 0};
struct RefOptimizer {
    static void InertialOptimization(ImiMap*, Eigen::Matrix3d&, double&, Eigen::Vector3d&, Eigen::Vector3d&, bool, Eigen::MatrixXd&, bool, bool, float, float) { g_ref_calls[0]++; }
    static void InertialOptimization(ImiMap*, Eigen::Vector3d&, Eigen::Vector3d&, float, float) { g_ref_calls[1]++; }
    static void InertialOptimization(ImiMap*, Eigen::Matrix3d&, double&) { g_ref_calls[2]++; }
};

static void print_state(const std::deque<ImiKeyFrame>& kfs)
{
    for (const ImiKeyFrame& k : kfs) {
        std::printf("state %lu %a %a %a", k.mnId, (double)k.mVw[0], (double)k.mVw[1], (double)k.mVw[2]);
        std::printf(" %a %a %a %a %a %a", (double)k.mImuBias.bax, (double)k.mImuBias.bay, (double)k.mImuBias.baz, (double)k.mImuBias.bwx, (double)k.mImuBias.bwy, (double)k.mImuBias.bwz);
        std::printf(" %d %d %d\n", k.nVelocityWrites, k.nBiasWrites, k.mpImuPreintegrated ? k.mpImuPreintegrated->nReintegrated : -1);
    }
}

template <class M> static void read3x3(std::istream& in, M& m) { for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) { double v; in >> v; m(r, c) = (float)v; } }
template <class V> static void read3(std::istream& in, V& v) { for (int r = 0; r < 3; r++) { double x; in >> x; v[r] = (float)x; } }
static IMU::Bias read_bias(std::istream& in) { double b[6]; for (double& x : b) in >> x; return IMU::Bias((float)b[0], (float)b[1], (float)b[2], (float)b[3], (float)b[4], (float)b[5]); }

// case file: "n_kf maxKFid", per key frame "id bad prev_id(-1) has_preintegration  Rwb[9] twb[3] vel[3] bias[6](ba, bg)" and, with a
// pre-integration, "dT dR[9] dV[3] dP[3] JRg[9] JVg[9] JVa[9] JPg[9] JPa[9] b[6] C[81]" (the 9 x 9 block of C); for writeback then
// "bg[3] ba[3]" and n_kf_in_problem x "vel[3]"
int main(int argc, char** argv)
{
    if (argc < 3) { std::fprintf(stderr, "usage: shim_imu_init_toy walk|fallback case.txt overload | writeback case.txt\n"); return 2; }
    const std::string mode = argv[1];
    const int overload = argc > 3 ? std::atoi(argv[3]) : 1;
    std::ifstream in(argv[2]);
    if (!in) return 2;
    int n_kf;
    long max_id;
    in >> n_kf >> max_id;
    std::deque<ImiKeyFrame> kfs(n_kf);
    std::deque<ImiPreintegrated> pre(n_kf);
    std::map<long, ImiKeyFrame*> by_id;
    std::vector<long> prev(n_kf);
    ImiMap map;
    map.mnMaxKFid = (unsigned long)max_id;
    for (int k = 0; k < n_kf; k++) {
        ImiKeyFrame& kf = kfs[k];
        long id; int bad, has;
        in >> id >> bad >> prev[k] >> has;
        kf.mnId = (unsigned long)id; kf.mbBad = bad != 0; kf.bImu = true; kf.mpMap = &map;
        read3x3(in, kf.mRwb); read3(in, kf.mtwb); read3(in, kf.mVw);
        kf.mImuBias = read_bias(in);
        if (has) {
            ImiPreintegrated& p = pre[k];
            double dT; in >> dT; p.dT = (float)dT;
            read3x3(in, p.dR); read3(in, p.dV); read3(in, p.dP);
            read3x3(in, p.JRg); read3x3(in, p.JVg); read3x3(in, p.JVa); read3x3(in, p.JPg); read3x3(in, p.JPa);
            p.b = read_bias(in);
            for (int r = 0; r < 9; r++) for (int c = 0; c < 9; c++) { double v; in >> v; p.C(r, c) = (float)v; }
            for (int r = 9; r < 15; r++) p.C(r, r) = 1.f;
            kf.mpImuPreintegrated = &p;
        }
        by_id[id] = &kf;
        map.kfs.push_back(&kf);
    }
    for (int k = 0; k < n_kf; k++) if (prev[k] >= 0) kfs[k].mPrevKF = by_id[prev[k]];
    if (!in) { std::fprintf(stderr, "short case file\n"); return 2; }
    if (mode == "walk") {
        ImuInitFlat<ImiKeyFrame> g;
        FlattenInertialOptimization(&map, g, overload != 3, overload == 3);
        std::printf("key_frames %zu links %zu refused %d\n", g.kfs.size(), g.links.size(), (int)g.refused);
        {   // stderr: the problem struct made of this walk, for tests/test_shim_abi_golden.py (this toy has no fake of the solve to record it)
            const imu_init_detail::Settings s = {overload != 3, overload == 2, overload != 2, overload == 1, overload == 3, 1e2, 1e6, overload == 3 ? 1.0 : 0.0, 1e3, 200};
            const double Rwg[9] = {0, -1, 0, 1, 0, 0, 0, 0, 1};
            std::vector<double> vel_out;
            ImuInitProblem p;
            ImuInitResult r;
            imu_init_detail::fill(g, s, Rwg, 1.5, vel_out, p, r);
            record_abi::dump(p);
        }
        std::printf("bias %a %a %a %a %a %a\n", g.bg[0], g.bg[1], g.bg[2], g.ba[0], g.ba[1], g.ba[2]);
        for (size_t k = 0; k < g.kfs.size(); k++) {
            std::printf("kf %lu", g.kfs[k]->mnId);
            for (int a = 0; a < 9; a++) std::printf(" %a", g.Rwb[9 * k + a]);
            for (int a = 0; a < 3; a++) std::printf(" %a", g.twb[3 * k + a]);
            for (int a = 0; a < 3; a++) std::printf(" %a", g.vel[3 * k + a]);
            std::printf("\n");
        }
        for (const LibaLink& L : g.links) {
            std::printf("link %lu %lu %d %a", g.kfs[L.kf1]->mnId, g.kfs[L.kf2]->mnId, (int)L.robust, (double)L.dT);
            const float* f[] = {L.dR, L.dV, L.dP, L.JRg, L.JVg, L.JVa, L.JPg, L.JPa, L.bias0};
            const int nf[] = {9, 3, 3, 9, 9, 9, 9, 9, 6};
            for (int a = 0; a < 9; a++) for (int k = 0; k < nf[a]; k++) std::printf(" %a", (double)f[a][k]);
            for (int k = 0; k < 81; k++) std::printf(" %a", L.info9[k]);
            for (int k = 0; k < 9; k++) std::printf(" %a", L.info_gyro[k] + L.info_acc[k]);
            std::printf("\n");
        }
        for (const ImiKeyFrame& k : kfs)
            if (k.mpImuPreintegrated) {
                const IMU::Bias& u = k.mpImuPreintegrated->bu;
                std::printf("bu %lu %a %a %a %a %a %a\n", k.mnId, (double)u.bax, (double)u.bay, (double)u.baz, (double)u.bwx, (double)u.bwy, (double)u.bwz);
            }
    } else if (mode == "writeback") {
        ImuInitFlat<ImiKeyFrame> g;
        FlattenInertialOptimization(&map, g, true, false);
        Eigen::Vector3d bg, ba;
        for (int k = 0; k < 3; k++) in >> bg[k];
        for (int k = 0; k < 3; k++) in >> ba[k];
        std::vector<double> vel(3 * g.kfs.size());
        for (double& v : vel) in >> v;
        if (!in) { std::fprintf(stderr, "short case file\n"); return 2; }
        imu_init_detail::write_back(g, vel.data(), bg, ba);
        print_state(kfs);
    } else if (mode == "fallback") {
        Eigen::Matrix3d Rwg;
        for (int k = 0; k < 3; k++) Rwg(k, k) = 1.0;
        double scale = 1.0;
        Eigen::Vector3d bg, ba;
        Eigen::MatrixXd cov;
        if (overload == 1) InertialOptimizationHIP<RefOptimizer>(&map, Rwg, scale, bg, ba, true, cov, false, false, 1e2f, 1e10f);
        else if (overload == 2) InertialOptimizationHIP<RefOptimizer>(&map, bg, ba, 1e2f, 1e10f);
        else InertialOptimizationHIP<RefOptimizer>(&map, Rwg, scale);
        std::printf("reference calls %d %d %d scale %a\n", g_ref_calls[0], g_ref_calls[1], g_ref_calls[2], scale);
        print_state(kfs);
    } else {
        return 2;
    }
    return 0;
}
