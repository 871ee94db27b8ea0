// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_preint.hpp on the stand-in of standin_imu_preint.hpp for
// tests/test_shim_preint.py.  Numbers leave as hexadecimal floats.
//   roundtrip                 to_state / from_state on an object whose every member is distinct (no device)
//   reintegrate <file>        ReintegrateHIP on the objects of the file, one call
//   frame <file>              PreintegrateIMUHIP on the samples of the file
#define ORBSLAM3_HIP_WITH_REFERENCE
#include <cstdio>
#include <fstream>
#include <string>

#include "standin_imu_preint.hpp"
#include "orbslam3_shim_preint.hpp"

using namespace ORB_SLAM3;
typedef IMU::PiPreintegrated Pre;

static float counter = 0.f;
static float next_value() { counter += 1.f; return counter + 0.25f; }

template <class M>
static void fill(M& m, int n) { for (int i = 0; i < n; i++) m[i] = next_value(); }

static void fill_all(Pre& p)
{
    p.dT = next_value();
    fill(p.C, 225); fill(p.Info, 225); fill(p.Nga.d, 6); fill(p.NgaWalk.d, 6);
    p.b = IMU::Bias(next_value(), next_value(), next_value(), next_value(), next_value(), next_value());
    fill(p.dR, 9); fill(p.dV, 3); fill(p.dP, 3); fill(p.JRg, 9); fill(p.JVg, 9); fill(p.JVa, 9); fill(p.JPg, 9); fill(p.JPa, 9); fill(p.avgA, 3); fill(p.avgW, 3);
    p.bu = IMU::Bias(next_value(), next_value(), next_value(), next_value(), next_value(), next_value());
    fill(p.db, 6);
}

template <class M>
static bool same(const M& a, const M& b, int n) { for (int i = 0; i < n; i++) if (a[i] != b[i]) return false; return true; }
static bool same(const IMU::Bias& a, const IMU::Bias& b) { return a.bax == b.bax && a.bay == b.bay && a.baz == b.baz && a.bwx == b.bwx && a.bwy == b.bwy && a.bwz == b.bwz; }

static int roundtrip()
{
    Pre p, q;
    fill_all(p);
    p.mvMeasurements.resize(5);
    fill_all(q);                                    // other values everywhere
    const auto info0 = q.Info;
    const auto db0 = q.db;
    q.mvMeasurements.resize(2);
    ImuPreintState s;
    preint_detail::to_state(p, s);
    // the layout of the state: row major, the bias order bax bay baz bwx bwy bwz
    bool layout = s.dR[1] == p.dR(0, 1) && s.dR[3] == p.dR(1, 0) && s.C[15 * 2 + 11] == p.C(2, 11) && s.C[15 * 11 + 2] == p.C(11, 2) && s.JPa[7] == p.JPa(2, 1) &&
                  s.b[0] == p.b.bax && s.b[2] == p.b.baz && s.b[3] == p.b.bwx && s.b[5] == p.b.bwz && s.bu[1] == p.bu.bay && s.bu[4] == p.bu.bwy &&
                  s.nga[5] == p.Nga.d[5] && s.nga_walk[0] == p.NgaWalk.d[0] && s.avgW[2] == p.avgW[2] && s.dT == p.dT;
    std::printf("layout %d\nn_meas %d\n", (int)layout, (int)s.n_meas);
    preint_detail::from_state(s, q);
    std::printf("member dT %d\n", (int)(q.dT == p.dT));
    std::printf("member C %d\n", (int)same(q.C, p.C, 225));
    std::printf("member Nga %d\n", (int)same(q.Nga.d, p.Nga.d, 6));
    std::printf("member NgaWalk %d\n", (int)same(q.NgaWalk.d, p.NgaWalk.d, 6));
    std::printf("member b %d\n", (int)same(q.b, p.b));
    std::printf("member bu %d\n", (int)same(q.bu, p.bu));
    std::printf("member dR %d\n", (int)same(q.dR, p.dR, 9));
    std::printf("member dV %d\n", (int)same(q.dV, p.dV, 3));
    std::printf("member dP %d\n", (int)same(q.dP, p.dP, 3));
    std::printf("member JRg %d\n", (int)same(q.JRg, p.JRg, 9));
    std::printf("member JVg %d\n", (int)same(q.JVg, p.JVg, 9));
    std::printf("member JVa %d\n", (int)same(q.JVa, p.JVa, 9));
    std::printf("member JPg %d\n", (int)same(q.JPg, p.JPg, 9));
    std::printf("member JPa %d\n", (int)same(q.JPa, p.JPa, 9));
    std::printf("member avgA %d\n", (int)same(q.avgA, p.avgA, 3));
    std::printf("member avgW %d\n", (int)same(q.avgW, p.avgW, 3));
    // not part of a state: left as they were
    std::printf("kept Info %d\n", (int)same(q.Info, info0, 225));
    std::printf("kept db %d\n", (int)same(q.db, db0, 6));
    std::printf("kept mvMeasurements %d\n", (int)(q.mvMeasurements.size() == 2));
    preint_detail::clear_info_and_db(q);
    bool zero = true;
    for (int i = 0; i < 225; i++) zero = zero && q.Info[i] == 0.f;
    for (int i = 0; i < 6; i++) zero = zero && q.db[i] == 0.f;
    std::printf("cleared %d\n", (int)zero);
    return 0;
}

static void print_object(const char* tag, int i, Pre& p)
{
    ImuPreintState s;
    preint_detail::to_state(p, s);
    std::printf("%s %d", tag, i);
    const float* f = &s.dT;
    for (size_t k = 0; k < offsetof(ImuPreintState, n_meas) / sizeof(float); k++) std::printf(" %a", (double)f[k]);
    float info = 0.f, db = 0.f;
    for (int k = 0; k < 225; k++) info = std::max(info, std::fabs(p.Info[k]));
    for (int k = 0; k < 6; k++) db = std::max(db, std::fabs(p.db[k]));
    std::printf(" %d %a %a\n", (int)s.n_meas, (double)info, (double)db);
    for (const auto& m : p.mvMeasurements) std::printf("meas %s %d %a %a %a %a %a %a %a\n", tag, i, (double)m.a[0], (double)m.a[1], (double)m.a[2], (double)m.w[0], (double)m.w[1], (double)m.w[2], (double)m.t);
}

static void read_calib(std::ifstream& in, Pre& p)
{
    for (int k = 0; k < 6; k++) { double v; in >> v; p.Nga.d[k] = (float)v; }
    for (int k = 0; k < 6; k++) { double v; in >> v; p.NgaWalk.d[k] = (float)v; }
}
static IMU::Bias read_bias(std::ifstream& in)
{
    double v[6];
    for (double& x : v) in >> x;
    return IMU::Bias((float)v[0], (float)v[1], (float)v[2], (float)v[3], (float)v[4], (float)v[5]);
}

static int reintegrate(const char* path)
{
    std::ifstream in(path);
    int n;
    in >> n;
    std::vector<Pre> objs((size_t)n);
    std::vector<Pre*> v;
    for (int i = 0; i < n; i++) {
        Pre& p = objs[(size_t)i];
        fill_all(p);                                // stale values everywhere: Reintegrate() starts from Initialize(bu)
        p.bu = read_bias(in);
        read_calib(in, p);
        int m;
        in >> m;
        for (int k = 0; k < m; k++) {
            double a[7];
            for (double& x : a) in >> x;
            p.mvMeasurements.push_back(Pre::integrable(Eigen::Vector3f((float)a[0], (float)a[1], (float)a[2]), Eigen::Vector3f((float)a[3], (float)a[4], (float)a[5]), (float)a[6]));
        }
        v.push_back(&p);
        if (i == 1) v.push_back(nullptr);           // a key frame without pre-integration
    }
    const bool ok = ReintegrateHIP(v);
    std::printf("accepted %d\n", (int)ok);
    for (int i = 0; i < n; i++) print_object("object", i, objs[(size_t)i]);
    return 0;
}

static void initialize(Pre& p, const IMU::Bias& b)
{
    ImuPreintState s;
    std::memset(&s, 0, sizeof(s));
    s.dR[0] = s.dR[4] = s.dR[8] = 1.f;
    for (int k = 0; k < 6; k++) { s.nga[k] = p.Nga.d[k]; s.nga_walk[k] = p.NgaWalk.d[k]; }
    preint_detail::from_state(s, p);
    preint_detail::clear_info_and_db(p);
    p.b = b; p.bu = b;
}

static int frame(const char* path)
{
    std::ifstream in(path);
    Pre kf, fr;
    fill_all(fr);                                   // (the adapter resets the accumulator of the frame itself)
    const IMU::Bias b_kf = read_bias(in), b_fr = read_bias(in);
    read_calib(in, kf);
    fr.Nga = kf.Nga; fr.NgaWalk = kf.NgaWalk;
    initialize(kf, b_kf);
    fr.b = b_fr;
    fr.mvMeasurements.resize(3);
    double tPrev, tCur;
    int n;
    in >> tPrev >> tCur >> n;
    std::vector<IMU::PiPoint> pts;
    for (int k = 0; k < n; k++) {
        double t, a[6];
        in >> t;
        for (double& x : a) in >> x;
        pts.push_back(IMU::PiPoint(Eigen::Vector3f((float)a[0], (float)a[1], (float)a[2]), Eigen::Vector3f((float)a[3], (float)a[4], (float)a[5]), t));
    }
    const bool ok = PreintegrateIMUHIP(pts, tPrev, tCur, &kf, &fr);
    std::printf("accepted %d\n", (int)ok);
    print_object("kf", 0, kf);
    print_object("frame", 0, fr);
    return 0;
}

int main(int argc, char** argv)
{
    const std::string mode = argc > 1 ? argv[1] : "";
    try {
        if (mode == "roundtrip") return roundtrip();
        if (mode == "reintegrate" && argc > 2) return reintegrate(argv[2]);
        if (mode == "frame" && argc > 2) return frame(argv[2]);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 2;
    }
    std::fprintf(stderr, "usage: shim_preint_toy roundtrip | reintegrate <file> | frame <file>\n");
    return 1;
}
