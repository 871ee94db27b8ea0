// include/orbslam3_hip_track_project.h: the projections between the device-resident tracking searches and pose optimisations.
// The arithmetic is track_project_geometry.h; this file is the lane mapping and the host drivers.  One lane per (frame, row);
// the frame's pose record and the camera are wave-uniform; per-row arrays are structure-of-arrays and coalesced.  The work is
// launch- and latency-bound (about 60 B per row), so the kernels are plain C++ without LDS.
#include "orbm_host.h"
#include "track_project_geometry.h"

namespace tpj {

constexpr int kBlock = 256;

struct FrustumArgs {
    OrbmTrackCamera cam;
    const OrbmFramePose* pose;
    OrbmLocalPoints pts;
    OrbmFrustumOut out;
    float cos_limit;
};

struct LastArgs {
    OrbmTrackCamera cam;
    const OrbmFramePose* pose;
    const float* xyz; const uint8_t* has_point; const int32_t* n; int32_t cap;
    OrbmLastProjOut out;
};

struct HandoverArgs {
    const int32_t* assign; const uint8_t* outlier; const int32_t* n_cur; int32_t cap;
    const int32_t* last_local; int32_t last_cap;
    const uint8_t* bad; const uint8_t* has_obs; int32_t pcap;
    int32_t* assign_local; uint8_t* occupied; uint8_t* skip; int32_t* n_dropped;
};

__global__ void k_frame_pose(const double* __restrict__ pose, int batch, int normalise, OrbmFramePose* __restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double p[7];
    for (int i = 0; i < 7; i++) p[i] = pose[(size_t)b * 7 + i];
    OrbmFramePose F;
    frame_pose(p, normalise, &F);
    out[b] = F;
}

// grid (ceil(pcap / 256), batch).  Every row p < pcap is written; n_to_match[b] was cleared by the launch sequence and takes one
// atomicAdd per wave that saw a point in view.
__global__ __launch_bounds__(kBlock) void k_frustum(const FrustumArgs A)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int pcap = A.pts.pcap;
    const bool in_range = p < pcap;
    const size_t row = (size_t)b * pcap + (in_range ? p : 0);
    Row r = row_none();
    if (in_range && p < A.pts.n[b] && !A.pts.skip[row] && !A.pts.bad[row]) {
        const OrbmFramePose& F = A.pose[b];
        const float P[3] = {A.pts.xyz[row * 3], A.pts.xyz[row * 3 + 1], A.pts.xyz[row * 3 + 2]};
        const float Pn[3] = {A.pts.normal[row * 3], A.pts.normal[row * 3 + 1], A.pts.normal[row * 3 + 2]};
        r = frustum_row(A.cam, F, P, Pn, A.pts.min_distance[row], A.pts.max_distance[row], A.cos_limit);
    }
    if (in_range) {
        A.out.valid[row] = (uint8_t)r.valid;
        A.out.u[row] = r.u; A.out.v[row] = r.v;
        A.out.octave[row] = r.level;
        A.out.view_cos[row] = r.view_cos; A.out.track_depth[row] = r.depth;
        A.out.proj_ur[row] = r.ur;
    }
    const unsigned long long in_view = __ballot(r.valid != 0);
    if (in_view != 0 && (threadIdx.x & 63) == 0) atomicAdd(&A.out.n_to_match[b], __popcll(in_view));
}

__global__ __launch_bounds__(kBlock) void k_project_last(const LastArgs A)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.cap) return;
    const size_t row = (size_t)b * A.cap + i;
    Row r = row_none();
    if (i < A.n[b] && A.has_point[row]) {
        const float x[3] = {A.xyz[row * 3], A.xyz[row * 3 + 1], A.xyz[row * 3 + 2]};
        r = project_last_row(A.cam, A.pose[b], x);
    }
    A.out.valid[row] = (uint8_t)r.valid;
    A.out.u[row] = r.u; A.out.v[row] = r.v;
    A.out.proj_ur[row] = r.ur;
}

// one workgroup per frame: clear skip, barrier, then the features
__global__ __launch_bounds__(kBlock) void k_handover(const HandoverArgs A)
{
    __shared__ int s_dropped;
    const int b = blockIdx.x;
    const size_t f0 = (size_t)b * A.cap, l0 = (size_t)b * A.last_cap, p0 = (size_t)b * A.pcap;
    if (threadIdx.x == 0) s_dropped = 0;
    for (int p = threadIdx.x; p < A.pcap; p += kBlock) A.skip[p0 + p] = 0;
    __syncthreads();                                    // (the skip bytes set below are this workgroup's own earlier stores)
    const int n = min(A.n_cur[b], A.cap);
    int dropped = 0;
    for (int i = threadIdx.x; i < A.cap; i += kBlock) {
        int local = -1;
        uint8_t occ = 0;
        const int a = i < n ? A.assign[f0 + i] : -1;
        if (a >= 0) {                                   // mCurrentFrame.mvpMapPoints[i] != NULL
            const int row = a < A.last_cap ? A.last_local[l0 + a] : -1;
            if (row < 0 || row >= A.pcap) {
                dropped++;
            } else {
                A.skip[p0 + row] = 1;                   // mnLastFrameSeen = mnId: outliers (:3073) and kept points (:3502) alike
                if (!A.outlier[f0 + i] && !A.bad[p0 + row]) {
                    local = row;
                    occ = A.has_obs[p0 + row] ? 1 : 0;
                }
            }
        }
        A.assign_local[f0 + i] = local;
        A.occupied[f0 + i] = occ;
    }
    if (dropped) atomicAdd(&s_dropped, dropped);
    __syncthreads();
    if (threadIdx.x == 0) A.n_dropped[b] = s_dropped;
}

}  // namespace tpj

static int check_camera(const OrbmTrackCamera* cam, int batch)
{
    if (!cam) return fail(ORBX_ERR_ARG, "cam is NULL");
    if (cam->n_levels < 1 || cam->n_levels > ORBM_TRACK_MAX_LEVELS) return fail(ORBX_ERR_ARG, "n_levels %d outside [1, %d]", cam->n_levels, ORBM_TRACK_MAX_LEVELS);
    if (batch < 1) return fail(ORBX_ERR_ARG, "batch %d < 1", batch);
    if (batch > ORBM_TRACK_MAX_BATCH) return fail(ORBX_ERR_CAPACITY, "batch %d above %d", batch, ORBM_TRACK_MAX_BATCH);
    return ORBX_OK;
}

static int check_last(const OrbmTrackCamera* cam, const OrbmFramePose* poses, const float* xyz, const uint8_t* has_point, const int32_t* n, int cap,
                      const OrbmLastProjOut* out, int batch)
{
    if (!poses || !xyz || !has_point || !n || !out) return fail(ORBX_ERR_ARG, "NULL argument");
    if (!out->valid || !out->u || !out->v || !out->proj_ur) return fail(ORBX_ERR_ARG, "NULL output array");
    if (cap <= 0) return fail(ORBX_ERR_ARG, "cap %d <= 0", cap);
    return check_camera(cam, batch);
}

static dim3 row_grid(int rows, int batch) { return dim3((unsigned)((rows + tpj::kBlock - 1) / tpj::kBlock), (unsigned)batch); }

static int launch_frustum(const tpj::FrustumArgs& A, int batch, hipStream_t st)
{
    ORBX_HIP(hipMemsetAsync(A.out.n_to_match, 0, sizeof(int32_t) * (size_t)batch, st));
    hipLaunchKernelGGL(tpj::k_frustum, row_grid(A.pts.pcap, batch), dim3(tpj::kBlock), 0, st, A);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

static int launch_last(const tpj::LastArgs& A, int batch, hipStream_t st)
{
    hipLaunchKernelGGL(tpj::k_project_last, row_grid(A.cap, batch), dim3(tpj::kBlock), 0, st, A);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

// upload [0, out0), run, download [out0, size): the shape of every host-array entry of the handle
template <class Launch>
static int run_staged(orbm_matcher* m, Blob& blob, size_t out0, Launch launch)
{
    hipStream_t st = m->stream;
    if (out0) ORBX_HIP(hipMemcpyAsync(m->d_blob, blob.buf.data(), out0, hipMemcpyHostToDevice, st));
    if (int r = m->tp_timer.start(st)) return r;
    if (int r = launch(st)) return r;
    if (int r = m->tp_timer.stop(st)) return r;
    ORBX_HIP(hipMemcpyAsync(blob.buf.data() + out0, m->d_blob + out0, blob.size() - out0, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    return m->tp_timer.read();
}

extern "C" {

int orbm_track_project_check(const OrbmTrackCamera* cam, const OrbmFramePose* poses, const OrbmLocalPoints* pts, const OrbmFrustumOut* out, int batch)
{
    if (!poses || !pts || !out) return fail(ORBX_ERR_ARG, "NULL argument");
    if (!pts->xyz || !pts->normal || !pts->min_distance || !pts->max_distance || !pts->skip || !pts->bad || !pts->n) return fail(ORBX_ERR_ARG, "NULL local-point array");
    if (!out->valid || !out->u || !out->v || !out->octave || !out->view_cos || !out->track_depth || !out->proj_ur || !out->n_to_match)
        return fail(ORBX_ERR_ARG, "NULL output array");
    if (pts->pcap <= 0) return fail(ORBX_ERR_ARG, "pcap %d <= 0", pts->pcap);
    return check_camera(cam, batch);
}

int orbm_frame_pose_batch_device(orbm_matcher* m, const double* d_pose, int batch, int normalise, OrbmFramePose* d_frame_pose, void* stream)
{
    if (!m || !d_pose || !d_frame_pose) return fail(ORBX_ERR_ARG, "NULL argument");
    if (batch < 1) return fail(ORBX_ERR_ARG, "batch %d < 1", batch);
    if (batch > ORBM_TRACK_MAX_BATCH) return fail(ORBX_ERR_CAPACITY, "batch %d above %d", batch, ORBM_TRACK_MAX_BATCH);
    ORBX_HIP(hipSetDevice(m->device));
    hipLaunchKernelGGL(tpj::k_frame_pose, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, d_pose, batch, normalise ? 1 : 0, d_frame_pose);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int orbm_frustum_batch_device(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* d_frame_pose, const OrbmLocalPoints* pts,
                              float viewing_cos_limit, const OrbmFrustumOut* out, int batch, void* stream)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = orbm_track_project_check(cam, d_frame_pose, pts, out, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    return launch_frustum(tpj::FrustumArgs{*cam, d_frame_pose, *pts, *out, viewing_cos_limit}, batch, (hipStream_t)stream);
}

int orbm_project_last_batch_device(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* d_frame_pose,
                                   const float* d_mp_xyz, const uint8_t* d_has_point, const int32_t* d_n, int cap,
                                   const OrbmLastProjOut* out, int batch, void* stream)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = check_last(cam, d_frame_pose, d_mp_xyz, d_has_point, d_n, cap, out, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    return launch_last(tpj::LastArgs{*cam, d_frame_pose, d_mp_xyz, d_has_point, d_n, cap, *out}, batch, (hipStream_t)stream);
}

int orbm_track_handover_batch_device(orbm_matcher* m, const int32_t* d_assign, const uint8_t* d_outlier, const int32_t* d_n_cur, int cap,
                                     const int32_t* d_last_local, int last_cap, const uint8_t* d_bad, const uint8_t* d_has_obs, int pcap,
                                     int32_t* d_assign_local, uint8_t* d_occupied, uint8_t* d_skip, int32_t* d_n_dropped,
                                     int batch, void* stream)
{
    if (!m || !d_assign || !d_outlier || !d_n_cur || !d_last_local || !d_bad || !d_has_obs || !d_assign_local || !d_occupied || !d_skip || !d_n_dropped)
        return fail(ORBX_ERR_ARG, "NULL argument");
    if (cap <= 0 || last_cap <= 0 || pcap <= 0 || batch < 1) return fail(ORBX_ERR_ARG, "bad batch / capacities");
    if (batch > ORBM_TRACK_MAX_BATCH) return fail(ORBX_ERR_CAPACITY, "batch %d above %d", batch, ORBM_TRACK_MAX_BATCH);
    ORBX_HIP(hipSetDevice(m->device));
    const tpj::HandoverArgs A{d_assign, d_outlier, d_n_cur, cap, d_last_local, last_cap, d_bad, d_has_obs, pcap, d_assign_local, d_occupied, d_skip, d_n_dropped};
    hipLaunchKernelGGL(tpj::k_handover, dim3((unsigned)batch), dim3(tpj::kBlock), 0, (hipStream_t)stream, A);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int orbm_frustum_batch(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* poses, const OrbmLocalPoints* pts,
                       float viewing_cos_limit, const OrbmFrustumOut* out, int batch)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = orbm_track_project_check(cam, poses, pts, out, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    if (int r = m->tp_timer.create()) return r;
    const size_t B = (size_t)batch, rows = B * (size_t)pts->pcap;
    tpj::FrustumArgs A{*cam, nullptr, *pts, *out, viewing_cos_limit};
    Blob blob(m);
    blob.in(A.pose, poses, B);
    blob.in(A.pts.xyz, pts->xyz, rows * 3); blob.in(A.pts.normal, pts->normal, rows * 3);
    blob.in(A.pts.min_distance, pts->min_distance, rows); blob.in(A.pts.max_distance, pts->max_distance, rows);
    blob.in(A.pts.skip, pts->skip, rows); blob.in(A.pts.bad, pts->bad, rows); blob.in(A.pts.n, pts->n, B);
    const size_t out0 = blob.begin_out();
    blob.out(A.out.valid, rows); blob.out(A.out.u, rows); blob.out(A.out.v, rows); blob.out(A.out.octave, rows);
    blob.out(A.out.view_cos, rows); blob.out(A.out.track_depth, rows); blob.out(A.out.proj_ur, rows); blob.out(A.out.n_to_match, B);
    if (int r = m->ensure(blob.size())) return r;
    blob.bind(m->d_blob);
    if (int r = run_staged(m, blob, out0, [&](hipStream_t st) { return launch_frustum(A, batch, st); })) return r;
    std::memcpy(out->valid, blob.host(A.out.valid), rows);
    std::memcpy(out->u, blob.host(A.out.u), rows * 4); std::memcpy(out->v, blob.host(A.out.v), rows * 4);
    std::memcpy(out->octave, blob.host(A.out.octave), rows * 4);
    std::memcpy(out->view_cos, blob.host(A.out.view_cos), rows * 4); std::memcpy(out->track_depth, blob.host(A.out.track_depth), rows * 4);
    std::memcpy(out->proj_ur, blob.host(A.out.proj_ur), rows * 4);
    std::memcpy(out->n_to_match, blob.host(A.out.n_to_match), B * 4);
    return ORBX_OK;
}

int orbm_project_last_batch(orbm_matcher* m, const OrbmTrackCamera* cam, const OrbmFramePose* poses,
                            const float* mp_xyz, const uint8_t* has_point, const int32_t* n, int cap,
                            const OrbmLastProjOut* out, int batch)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = check_last(cam, poses, mp_xyz, has_point, n, cap, out, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    if (int r = m->tp_timer.create()) return r;
    const size_t B = (size_t)batch, rows = B * (size_t)cap;
    tpj::LastArgs A{*cam, nullptr, nullptr, nullptr, nullptr, cap, *out};
    Blob blob(m);
    blob.in(A.pose, poses, B);
    blob.in(A.xyz, mp_xyz, rows * 3); blob.in(A.has_point, has_point, rows); blob.in(A.n, n, B);
    const size_t out0 = blob.begin_out();
    blob.out(A.out.valid, rows); blob.out(A.out.u, rows); blob.out(A.out.v, rows); blob.out(A.out.proj_ur, rows);
    if (int r = m->ensure(blob.size())) return r;
    blob.bind(m->d_blob);
    if (int r = run_staged(m, blob, out0, [&](hipStream_t st) { return launch_last(A, batch, st); })) return r;
    std::memcpy(out->valid, blob.host(A.out.valid), rows);
    std::memcpy(out->u, blob.host(A.out.u), rows * 4); std::memcpy(out->v, blob.host(A.out.v), rows * 4);
    std::memcpy(out->proj_ur, blob.host(A.out.proj_ur), rows * 4);
    return ORBX_OK;
}

float orbm_track_project_last_kernel_ms(const orbm_matcher* m) { return m ? m->tp_timer.ms : 0.f; }

}  // extern "C"
