// TEST INFRASTRUCTURE -- drives include/orbslam3_shim_fisheye.hpp (ComputeStereoFishEyeMatchesHIP) on a toy rig frame made of the
// stand-in types (tests/stubs/standin_fisheye.hpp).
//   shim_fisheye_toy <scenario> <case file> <dump file>     rig | noncontiguous | pinhole_right | no_right
// case file: int32 n_l, mono_l, n_r, mono_r, n_levels; 30 floats of the rig (left fx fy cx cy k0..k3 precision, the same of the
//            right, Rlr row major, tlr); n_levels floats; n_l key points (28 bytes each); n_l x 32 bytes; the same of the right side.
// Built without SHIM_FISHEYE_REAL the C entry point is a RECORDING FAKE defined here: it writes every argument it received to the
// dump file (the same layout as the case file, the rig as the 184 bytes of OrbxFisheyeRig) and returns a pattern; no device is
// needed.  Built with SHIM_FISHEYE_REAL it links the library and runs on the device.  Either way the frame's members are printed;
// tests/test_shim_fisheye.py and tests/test_fisheye_stereo_gpu.py read them.
#define ORBSLAM3_HIP_WITH_REFERENCE
#include "standin_fisheye.hpp"
#include "orbslam3_shim_fisheye.hpp"

#include <cstdio>
#include <cstdlib>
#include <string>

using namespace ORB_SLAM3;

static const char* g_dump = nullptr;

#ifndef SHIM_FISHEYE_REAL
extern "C" const char* orbx_last_error(void) { return "fake"; }
extern "C" int orbm_create(int, orbm_matcher**) { std::fprintf(stderr, "the toy passes its own handle\n"); std::exit(40); }
extern "C" int orbm_stereo_fisheye(orbm_matcher* m, const OrbxKeyPoint* kps_l, const uint8_t* desc_l, int n_l, int mono_l,
                                   const OrbxKeyPoint* kps_r, const uint8_t* desc_r, int n_r, int mono_r, const float* level_sigma2, int n_levels,
                                   const OrbxFisheyeRig* rig, int32_t* left_to_right, int32_t* right_to_left, float* depth, float* p3d,
                                   int32_t* knn_right, int32_t* knn_d0, int32_t* knn_d1)
{
    FILE* f = std::fopen(g_dump, "wb");
    if (!f) std::exit(41);
    const int32_t head[5] = {n_l, mono_l, n_r, mono_r, n_levels};
    std::fwrite(head, 4, 5, f);
    std::fwrite(rig, sizeof(*rig), 1, f);
    std::fwrite(level_sigma2, 4, n_levels, f);
    std::fwrite(kps_l, sizeof(OrbxKeyPoint), n_l, f); std::fwrite(desc_l, 32, n_l, f);
    std::fwrite(kps_r, sizeof(OrbxKeyPoint), n_r, f); std::fwrite(desc_r, 32, n_r, f);
    std::fclose(f);
    std::printf("orbm_stereo_fisheye handle %d diagnostics %d\n", (int)reinterpret_cast<size_t>(m), (knn_right != nullptr) + (knn_d0 != nullptr) + (knn_d1 != nullptr));
    for (int i = 0; i < n_l; i++) { left_to_right[i] = i + 100; depth[i] = 0.5f * i; for (int c = 0; c < 3; c++) p3d[3 * i + c] = i + 0.25f * c; }
    for (int j = 0; j < n_r; j++) right_to_left[j] = j + 200;
    return n_l;
}
#endif

template <class T>
static void get(FILE* f, T* dst, size_t n) { if (n && std::fread(dst, sizeof(T), n, f) != n) std::exit(42); }

int main(int argc, char** argv)
{
    if (argc != 4) return 2;
    const std::string sc = argv[1];
    g_dump = argv[3];
    FILE* f = std::fopen(argv[2], "rb");
    if (!f) return 3;
    int32_t head[5];
    float r[30];
    get(f, head, 5); get(f, r, 30);
    const int n_l = head[0], n_r = head[2], n_levels = head[4];
    RigFrame F;
    F.mvLevelSigma2.resize(n_levels);
    get(f, F.mvLevelSigma2.data(), n_levels);
    F.Nleft = n_l; F.monoLeft = head[1]; F.Nright = n_r; F.monoRight = head[3]; F.N = n_l + n_r;
    static_assert(sizeof(cv::KeyPoint) == 28, "cv::KeyPoint layout");
    F.mvKeys.resize(n_l); F.mvKeysRight.resize(n_r);
    const int pad = sc == "noncontiguous" ? 8 : 0;              // descriptor rows inside a wider matrix: the adapter has to copy them
    cv::Mat wide_l(n_l, 32 + pad, CV_8U), wide_r(n_r, 32 + pad, CV_8U);
    get(f, F.mvKeys.data(), n_l);
    for (int i = 0; i < n_l; i++) get(f, wide_l.ptr<uint8_t>(i) + pad, 32);
    get(f, F.mvKeysRight.data(), n_r);
    for (int i = 0; i < n_r; i++) get(f, wide_r.ptr<uint8_t>(i) + pad, 32);
    std::fclose(f);
    F.mDescriptors = wide_l(cv::Rect(pad, 0, 32, n_l)); F.mDescriptorsRight = wide_r(cv::Rect(pad, 0, 32, n_r));

    KannalaBrandt8Rig left(std::vector<float>(r, r + 8), r[8]), right(std::vector<float>(r + 9, r + 17), r[17]);
    Pinhole pin(458.f, 457.f, 367.f, 248.f);
    F.mpCamera = &left;
    F.mpCamera2 = sc == "pinhole_right" ? static_cast<GeometricCamera*>(&pin) : sc == "no_right" ? nullptr : &right;
    Eigen::Matrix3f R;
    for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) R(i, j) = r[18 + 3 * i + j];
    F.mTlr = Sophus::SE3f(R, Eigen::Vector3f(r[27], r[28], r[29]));
    F.mnCloseMPs = 17; F.mvuRight.assign(3, 5.f);               // stale values the adapter has to replace

#ifdef SHIM_FISHEYE_REAL
    orbm_matcher* m = nullptr;                                  // the calling thread's handle
#else
    orbm_matcher* m = reinterpret_cast<orbm_matcher*>((size_t)7);
#endif
    ComputeStereoFishEyeMatchesHIP<KannalaBrandt8Rig>(F, m);

    std::printf("reference_calls %d close %d sizes %zu %zu %zu %zu %zu\n", F.nReferenceCalls, F.mnCloseMPs, F.mvLeftToRightMatch.size(), F.mvRightToLeftMatch.size(),
                F.mvDepth.size(), F.mvuRight.size(), F.mvStereo3Dpoints.size());
    for (size_t i = 0; i < F.mvLeftToRightMatch.size(); i++)
        std::printf("left %zu %d %a %a %a %a %a\n", i, F.mvLeftToRightMatch[i], (double)F.mvDepth[i], (double)F.mvuRight[i], (double)F.mvStereo3Dpoints[i](0),
                    (double)F.mvStereo3Dpoints[i](1), (double)F.mvStereo3Dpoints[i](2));
    for (size_t j = 0; j < F.mvRightToLeftMatch.size(); j++) std::printf("right %zu %d\n", j, F.mvRightToLeftMatch[j]);
    return 0;
}
