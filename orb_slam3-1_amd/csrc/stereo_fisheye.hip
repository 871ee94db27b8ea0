// stereo_fisheye.hip -- Frame::ComputeStereoFishEyeMatches (reference src/Frame.cc:1246-1286) in two launches:
//
//   k_fisheye_knn       the brute-force 2-nearest-neighbour Hamming search of BFmatcher.knnMatch(left lapping, right lapping, 2) and
//                       Lowe's ratio (:1271).  One lane owns one left descriptor (8 VGPRs), a workgroup owns a tile of kKnnTile
//                       key points of one frame; the frame's right lapping descriptors pass through LDS in chunks of kKnnChunk.
//                       Every lane reads the same LDS address (a broadcast: no bank conflict), two 128-bit reads per candidate,
//                       then 8 XOR + 8 popcount-accumulate and the running (d0, d1, idx0).  It also resets the outputs of its
//                       slice of the frame, so that no separate clearing pass is needed.
//   k_fisheye_geometry  KannalaBrandt8::TriangulateMatches (csrc/kb8_stereo_geometry.h) for the survivors, one lane each, and the
//                       write-back; mvRightToLeftMatch by atomicMax (the reference's loop leaves the highest left index).
//
// Two kernels, not one: the double Jacobi of the null vector needs ~100 VGPRs, and only a few per cent of the lanes survive the
// ratio test; inside the search kernel it would cut the occupancy of the hot loop and leave most of a wave idle behind its survivors.
// The survivor's right index travels between the two in left_to_right itself, so the device entry needs no workspace.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/orbslam3_hip.h"
#include "hip_check.h"
#include "kb8_stereo_geometry.h"
#include "orbm_host.h"

namespace sfe {

constexpr int kKnnTile = 128;                           // left key points per workgroup = threads
constexpr int kKnnChunk = ORBM_FISHEYE_KNN_CHUNK;       // right descriptors per LDS pass: one per thread to stage, 4 KB
static_assert(kKnnChunk == kKnnTile, "each thread stages one right descriptor per pass");
constexpr int kGeoThreads = 64;
constexpr int kNone = 0x7fffffff;
constexpr int kMaxLevels = 32;

struct Args {
    const OrbxKeyPoint* kps_l; const uint8_t* desc_l; const int32_t* n_l; const int32_t* mono_l;
    const OrbxKeyPoint* kps_r; const uint8_t* desc_r; const int32_t* n_r; const int32_t* mono_r;
    int32_t cap_l, cap_r;                               // row strides of the left / right arrays
    int32_t* left_to_right; int32_t* right_to_left; float* depth; float* p3d;       // required
    int32_t* knn_right; int32_t* knn_d0; int32_t* knn_d1;                           // may be NULL
    kb8s::Rig rig;
    float sigma2[kMaxLevels];
    int32_t n_levels;
};

struct Frame { int n_l, mono_l, n_r, mono_r; size_t row_l, row_r; };

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }

__device__ __forceinline__ Frame frame_of(const Args& A, int b)
{
    Frame f;
    f.n_l = clampi(A.n_l[b], 0, A.cap_l); f.mono_l = clampi(A.mono_l[b], 0, f.n_l);
    f.n_r = clampi(A.n_r[b], 0, A.cap_r); f.mono_r = clampi(A.mono_r[b], 0, f.n_r);
    f.row_l = (size_t)b * A.cap_l; f.row_r = (size_t)b * A.cap_r;
    return f;
}

__device__ __forceinline__ int hamming(const uint4& a0, const uint4& a1, const uint4& q0, const uint4& q1)
{
    return __popc(a0.x ^ q0.x) + __popc(a0.y ^ q0.y) + __popc(a0.z ^ q0.z) + __popc(a0.w ^ q0.w) +
           __popc(a1.x ^ q1.x) + __popc(a1.y ^ q1.y) + __popc(a1.z ^ q1.z) + __popc(a1.w ^ q1.w);
}

__global__ __launch_bounds__(kKnnTile) void k_fisheye_knn(Args A)
{
    __shared__ uint4 s_desc[2 * kKnnChunk];
    const int b = blockIdx.y, tid = threadIdx.x, tile0 = blockIdx.x * kKnnTile, i = tile0 + tid;
    const Frame f = frame_of(A, b);
    if (i < f.n_r) A.right_to_left[f.row_r + i] = -1;
    if (i < f.n_l) {
        const size_t o = f.row_l + i;
        A.left_to_right[o] = -1; A.depth[o] = -1.0f;
        A.p3d[3 * o] = 0.f; A.p3d[3 * o + 1] = 0.f; A.p3d[3 * o + 2] = 0.f;
        if (A.knn_right) A.knn_right[o] = -1;
        if (A.knn_d0) A.knn_d0[o] = -1;
        if (A.knn_d1) A.knn_d1[o] = -1;
    }
    if (tile0 + kKnnTile <= f.mono_l || tile0 >= f.n_l) return;        // (uniform over the workgroup) no lapping left key point here
    const bool mine = i >= f.mono_l && i < f.n_l;
    uint4 a0 = make_uint4(0, 0, 0, 0), a1 = a0;
    if (mine) {
        const uint4* p = (const uint4*)(A.desc_l + (f.row_l + i) * 32);
        a0 = p[0]; a1 = p[1];
    }
    int d0 = kNone, d1 = kNone, idx0 = -1;
    for (int c = f.mono_r; c < f.n_r; c += kKnnChunk) {
        const int cnt = min(kKnnChunk, f.n_r - c);
        __syncthreads();                                                // the previous chunk has been read by every wave
        if (tid < cnt) {
            const uint4* p = (const uint4*)(A.desc_r + (f.row_r + c + tid) * 32);
            s_desc[2 * tid] = p[0]; s_desc[2 * tid + 1] = p[1];
        }
        __syncthreads();
#pragma unroll 4
        for (int j = 0; j < cnt; j++) {
            const int d = hamming(a0, a1, s_desc[2 * j], s_desc[2 * j + 1]);
            const bool first = d < d0;                                  // strict: the first of equally good candidates keeps idx0
            d1 = first ? d0 : min(d1, d);
            idx0 = first ? c + j : idx0;
            d0 = first ? d : d0;
        }
    }
    if (!mine) return;
    const size_t o = f.row_l + i;
    if (A.knn_d0 && d0 != kNone) A.knn_d0[o] = d0;
    if (A.knn_d1 && d1 != kNone) A.knn_d1[o] = d1;
    if (f.n_r - f.mono_r >= 2 && kb8s::ratio_ok(d0, d1)) {              // matches[i].size() >= 2 && Lowe's ratio (:1271)
        A.left_to_right[o] = idx0;                                      // the candidate: k_fisheye_geometry confirms or resets it
        if (A.knn_right) A.knn_right[o] = idx0;
    }
}

__global__ __launch_bounds__(kGeoThreads) void k_fisheye_geometry(Args A)
{
    const int b = blockIdx.y, i = blockIdx.x * kGeoThreads + threadIdx.x;
    const Frame f = frame_of(A, b);
    if (i < f.mono_l || i >= f.n_l) return;
    const size_t o = f.row_l + i;
    const int r = A.left_to_right[o];
    if (r < 0) return;
    const OrbxKeyPoint k1 = A.kps_l[o], k2 = A.kps_r[f.row_r + r];
    const float sigma1 = A.sigma2[clampi(k1.octave, 0, A.n_levels - 1)], sigma2 = A.sigma2[clampi(k2.octave, 0, A.n_levels - 1)];
    float p[3] = {0.f, 0.f, 0.f};
    const float z = kb8s::triangulate_matches(A.rig, k1.x, k1.y, k2.x, k2.y, sigma1, sigma2, p);
    if (z > 0.0001f) {                                                  // (:1277)
        A.depth[o] = z;
        A.p3d[3 * o] = p[0]; A.p3d[3 * o + 1] = p[1]; A.p3d[3 * o + 2] = p[2];
        atomicMax(&A.right_to_left[f.row_r + r], i);
    } else {
        A.left_to_right[o] = -1;
    }
}

__global__ __launch_bounds__(256) void k_triangulate_matches(kb8s::Rig rig, const float* __restrict__ pl, const float* __restrict__ pr,
                                                            const float* __restrict__ sl, const float* __restrict__ sr, int n,
                                                            float* __restrict__ code, float* __restrict__ p3d)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float p[3] = {0.f, 0.f, 0.f};
    const float z = kb8s::triangulate_matches(rig, pl[2 * (size_t)i], pl[2 * (size_t)i + 1], pr[2 * (size_t)i], pr[2 * (size_t)i + 1], sl[i], sr[i], p);
    code[i] = z;
    const bool ok = z > 0.f;
    p3d[3 * (size_t)i] = ok ? p[0] : 0.f; p3d[3 * (size_t)i + 1] = ok ? p[1] : 0.f; p3d[3 * (size_t)i + 2] = ok ? p[2] : 0.f;
}

}  // namespace sfe

namespace {

kb8s::Cam cam_of(const OrbxKB8& c, float precision)
{
    kb8s::Cam o;
    o.fx = (float)c.fx; o.fy = (float)c.fy; o.cx = (float)c.cx; o.cy = (float)c.cy;     // floats promoted to double: the casts are exact
    for (int k = 0; k < 4; k++) o.k[k] = (float)c.k[k];
    o.precision = precision;
    return o;
}

kb8s::Rig rig_of(const OrbxFisheyeRig* rig)
{
    kb8s::Rig g;
    g.l = cam_of(rig->left, rig->precision_l); g.r = cam_of(rig->right, rig->precision_r);
    std::memcpy(g.R12, rig->Rlr, sizeof(g.R12)); std::memcpy(g.t12, rig->tlr, sizeof(g.t12));
    return g;
}

int check_rig(const OrbxFisheyeRig* rig)
{
    if (!rig) return fail(ORBX_ERR_ARG, "rig is NULL");
    if (!(rig->left.fx > 0) || !(rig->left.fy > 0) || !(rig->right.fx > 0) || !(rig->right.fy > 0))
        return fail(ORBX_ERR_ARG, "KannalaBrandt8 focal lengths must be positive");
    if (!(rig->precision_l > 0) || !(rig->precision_r > 0)) return fail(ORBX_ERR_ARG, "KannalaBrandt8 precision must be positive");
    return ORBX_OK;
}

int check_side(const OrbxKeyPoint* kps, const uint8_t* desc, int n, int mono, int n_levels, const char* name)
{
    if (n < 0 || mono < 0) return fail(ORBX_ERR_ARG, "%s: negative count", name);
    if (mono > n) return fail(ORBX_ERR_ARG, "%s: mono index %d above the count %d", name, mono, n);
    if (n > 0 && (!kps || !desc)) return fail(ORBX_ERR_ARG, "%s: NULL key points or descriptors", name);
    for (int i = 0; i < n; i++)
        if (kps[i].octave < 0 || kps[i].octave >= n_levels) return fail(ORBX_ERR_ARG, "%s: octave %d of key point %d outside [0, %d)", name, kps[i].octave, i, n_levels);
    return ORBX_OK;
}

// the two launches; ev != NULL brackets them with events
int launch(const sfe::Args& A, int batch, hipStream_t st, hipEvent_t* ev)
{
    const int span = std::max(std::max(A.cap_l, A.cap_r), 1);
    if (ev) ORBX_HIP(hipEventRecord(ev[0], st));
    hipLaunchKernelGGL(sfe::k_fisheye_knn, dim3((span + sfe::kKnnTile - 1) / sfe::kKnnTile, batch), dim3(sfe::kKnnTile), 0, st, A);
    ORBX_HIP(hipGetLastError());
    if (A.cap_l > 0) {
        hipLaunchKernelGGL(sfe::k_fisheye_geometry, dim3((A.cap_l + sfe::kGeoThreads - 1) / sfe::kGeoThreads, batch), dim3(sfe::kGeoThreads), 0, st, A);
        ORBX_HIP(hipGetLastError());
    }
    if (ev) ORBX_HIP(hipEventRecord(ev[1], st));
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbm_stereo_fisheye_check(const OrbxKeyPoint* kps_l, const uint8_t* desc_l, int n_l, int mono_l,
                              const OrbxKeyPoint* kps_r, const uint8_t* desc_r, int n_r, int mono_r,
                              const float* level_sigma2, int n_levels, const OrbxFisheyeRig* rig)
{
    if (n_levels < 1 || n_levels > sfe::kMaxLevels) return fail(ORBX_ERR_ARG, "n_levels %d outside [1, %d]", n_levels, sfe::kMaxLevels);
    if (!level_sigma2) return fail(ORBX_ERR_ARG, "level_sigma2 is NULL");
    if (int r = check_rig(rig)) return r;
    if (int r = check_side(kps_l, desc_l, n_l, mono_l, n_levels, "left")) return r;
    return check_side(kps_r, desc_r, n_r, mono_r, n_levels, "right");
}

int orbm_stereo_fisheye(orbm_matcher* m,
                        const OrbxKeyPoint* kps_l, const uint8_t* desc_l, int n_l, int mono_l,
                        const OrbxKeyPoint* kps_r, const uint8_t* desc_r, int n_r, int mono_r,
                        const float* level_sigma2, int n_levels, const OrbxFisheyeRig* rig,
                        int32_t* left_to_right, int32_t* right_to_left, float* depth, float* p3d,
                        int32_t* knn_right, int32_t* knn_d0, int32_t* knn_d1)
{
    if (int r = orbm_stereo_fisheye_check(kps_l, desc_l, n_l, mono_l, kps_r, desc_r, n_r, mono_r, level_sigma2, n_levels, rig)) return r;
    if (!m) {                                                   // no handle exists without a device: there is no CPU fallback
        const int r = stage::check_device(0);
        return r ? r : fail(ORBX_ERR_ARG, "NULL matcher");
    }
    if (n_l == 0 && n_r == 0) return 0;

    ORBX_HIP(hipSetDevice(m->device));
    Blob blob(m);
    const size_t L = (size_t)n_l, R = (size_t)n_r;
    const int32_t counts[4] = {n_l, mono_l, n_r, mono_r};
    sfe::Args A;
    std::memset(&A, 0, sizeof(A));
    blob.in(A.kps_l, kps_l, L); blob.in(A.desc_l, desc_l, 32 * L);
    blob.in(A.kps_r, kps_r, R); blob.in(A.desc_r, desc_r, 32 * R);
    blob.in(A.n_l, counts, 4);
    const size_t in_bytes = blob.size(), o_out = blob.begin_out();
    blob.out(A.left_to_right, L); blob.out(A.right_to_left, R); blob.out(A.depth, L); blob.out(A.p3d, 3 * L);
    blob.out(A.knn_right, L); blob.out(A.knn_d0, L); blob.out(A.knn_d1, L);
    const size_t all_bytes = blob.size();
    if (int r = m->ensure(all_bytes)) return r;
    blob.bind(m->d_blob);
    uint8_t* b = m->d_blob;
    uint8_t* h = m->h_blob.data();
    A.mono_l = A.n_l + 1; A.n_r = A.n_l + 2; A.mono_r = A.n_l + 3;          // the four counts are one array
    A.cap_l = n_l; A.cap_r = n_r;
    A.rig = rig_of(rig);
    std::memcpy(A.sigma2, level_sigma2, sizeof(float) * n_levels);
    A.n_levels = n_levels;

    if (int r = m->sfe_timer.create()) return r;
    ORBX_HIP(hipMemcpyAsync(b, h, in_bytes, hipMemcpyHostToDevice, m->stream));
    if (int r = launch(A, 1, m->stream, m->sfe_timer.ev)) return r;
    if (all_bytes > o_out) ORBX_HIP(hipMemcpyAsync(h + o_out, b + o_out, all_bytes - o_out, hipMemcpyDeviceToHost, m->stream));
    ORBX_HIP(hipStreamSynchronize(m->stream));
    if (int r = m->sfe_timer.read()) return r;

    const int32_t* h_ltr = blob.host(A.left_to_right);
    int matches = 0;
    for (int i = 0; i < n_l; i++) matches += h_ltr[i] >= 0;
    if (left_to_right) std::memcpy(left_to_right, h_ltr, sizeof(int32_t) * L);
    if (right_to_left) std::memcpy(right_to_left, blob.host(A.right_to_left), sizeof(int32_t) * R);
    if (depth) std::memcpy(depth, blob.host(A.depth), sizeof(float) * L);
    if (p3d) std::memcpy(p3d, blob.host(A.p3d), sizeof(float) * 3 * L);
    if (knn_right) std::memcpy(knn_right, blob.host(A.knn_right), sizeof(int32_t) * L);
    if (knn_d0) std::memcpy(knn_d0, blob.host(A.knn_d0), sizeof(int32_t) * L);
    if (knn_d1) std::memcpy(knn_d1, blob.host(A.knn_d1), sizeof(int32_t) * L);
    return matches;
}

float orbm_stereo_fisheye_last_kernel_ms(const orbm_matcher* m) { return m ? m->sfe_timer.ms : 0.0f; }

int orbm_stereo_fisheye_batch_device(orbm_matcher* m, int batch, int cap,
                                     const OrbxKeyPoint* d_kps_l, const uint8_t* d_desc_l, const int32_t* d_n_l, const int32_t* d_mono_l,
                                     const OrbxKeyPoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_n_r, const int32_t* d_mono_r,
                                     const float* level_sigma2, int n_levels, const OrbxFisheyeRig* rig,
                                     int32_t* d_left_to_right, int32_t* d_right_to_left, float* d_depth, float* d_p3d,
                                     int32_t* d_knn_right, int32_t* d_knn_d0, int32_t* d_knn_d1, void* stream)
{
    if (int r = orbm_stereo_fisheye_check(nullptr, nullptr, 0, 0, nullptr, nullptr, 0, 0, level_sigma2, n_levels, rig)) return r;
    if (batch < 0 || batch > 65535 || cap < 0) return fail(ORBX_ERR_ARG, "batch %d outside [0, 65535] or negative cap %d", batch, cap);
    if (batch > 0 && (!d_n_l || !d_mono_l || !d_n_r || !d_mono_r)) return fail(ORBX_ERR_ARG, "NULL count arrays");
    if (batch > 0 && cap > 0 && (!d_kps_l || !d_desc_l || !d_kps_r || !d_desc_r || !d_left_to_right || !d_right_to_left || !d_depth || !d_p3d))
        return fail(ORBX_ERR_ARG, "NULL device arrays");
    if (((uintptr_t)d_desc_l & 15) || ((uintptr_t)d_desc_r & 15)) return fail(ORBX_ERR_ARG, "descriptor arrays must be 16-byte aligned");
    if (!m) {
        const int r = stage::check_device(0);
        return r ? r : fail(ORBX_ERR_ARG, "NULL matcher");
    }
    if (batch == 0 || cap == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(m->device));
    sfe::Args A;
    std::memset(&A, 0, sizeof(A));
    A.kps_l = d_kps_l; A.desc_l = d_desc_l; A.n_l = d_n_l; A.mono_l = d_mono_l;
    A.kps_r = d_kps_r; A.desc_r = d_desc_r; A.n_r = d_n_r; A.mono_r = d_mono_r;
    A.cap_l = cap; A.cap_r = cap;
    A.left_to_right = d_left_to_right; A.right_to_left = d_right_to_left; A.depth = d_depth; A.p3d = d_p3d;
    A.knn_right = d_knn_right; A.knn_d0 = d_knn_d0; A.knn_d1 = d_knn_d1;
    A.rig = rig_of(rig);
    std::memcpy(A.sigma2, level_sigma2, sizeof(float) * n_levels);
    A.n_levels = n_levels;
    return launch(A, batch, (hipStream_t)stream, nullptr);
}

int orbx_kb8_triangulate_matches(int device, const OrbxFisheyeRig* rig, const float* pts_l, const float* pts_r,
                                 const float* sigma_l, const float* sigma_r, int n, float* code_or_depth, float* p3d)
{
    if (int r = check_rig(rig)) return r;
    if (n < 0 || (n > 0 && (!pts_l || !pts_r || !sigma_l || !sigma_r || !code_or_depth || !p3d))) return fail(ORBX_ERR_ARG, "bad arguments");
    if (int r = stage::check_device(device)) return r;
    if (n == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(device));
    float* d = nullptr;
    const size_t N = (size_t)n;
    ORBX_HIP(hipMalloc((void**)&d, 10 * N * sizeof(float)));            // [pts_l 2n | pts_r 2n | sigma_l n | sigma_r n | code n | p3d 3n]
    hipError_t e = hipMemcpy(d, pts_l, 2 * N * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 2 * N, pts_r, 2 * N * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 4 * N, sigma_l, N * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d + 5 * N, sigma_r, N * sizeof(float), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(sfe::k_triangulate_matches, dim3((n + 255) / 256), dim3(256), 0, 0, rig_of(rig), (const float*)d, (const float*)(d + 2 * N),
                           (const float*)(d + 4 * N), (const float*)(d + 5 * N), n, d + 6 * N, d + 7 * N);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpy(code_or_depth, d + 6 * N, N * sizeof(float), hipMemcpyDeviceToHost);
    if (e == hipSuccess) e = hipMemcpy(p3d, d + 7 * N, 3 * N * sizeof(float), hipMemcpyDeviceToHost);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(ORBX_ERR_HIP, "orbx_kb8_triangulate_matches: %s", hipGetErrorString(e));
    return ORBX_OK;
}

}  // extern "C"
