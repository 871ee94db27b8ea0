// include/orbslam3_hip_track_project_rig.h: the projections in front of the two rig-frame tracking searches, and
// UnprojectStereoFishEye.  The arithmetic is track_project_rig_geometry.h; this file is the lane mapping and the host drivers.
// One lane per (frame, row) evaluates BOTH cameras: the point, its normal and its distances are read once, and n_to_match needs
// both verdicts.  The frame record is indexed by blockIdx.y alone, so it and the camera (a kernel argument) are wave-uniform and
// come through scalar loads, not per lane.  The in/out arrays (the stale MapPoint members) are never read: a side that fails, and
// a row that SearchLocalPoints skips, simply do not store to them.  The f64 atan2 / sin / cos of KannalaBrandt8::project sit
// behind the depth test of their camera, so a lane whose point is behind a camera does not pay for them.
#include "orbm_host.h"
#include "track_project_rig_geometry.h"

namespace tpr {

constexpr int kBlock = 256;

struct FrustumArgs {
    OrbmTrackRigCamera cam;
    const OrbmRigFramePose* pose;
    OrbmLocalPoints pts;
    OrbmRigFrustumOut out;
    float cos_limit;
};

struct LastArgs {
    OrbmTrackRigCamera cam;
    const OrbmRigFramePose* pose;
    const float* xyz; const uint8_t* has_point; const int32_t* n; int32_t cap;
    OrbmRigLastProjOut out;
};

struct UnprojectArgs {
    const OrbmRigFramePose* pose;
    const float* points; const uint8_t* valid; const int32_t* n; int32_t cap;
    float* world;
};

__global__ void k_frame_pose_rig(const OrbmTrackRigCamera cam, const double* __restrict__ pose, int batch, int normalise, OrbmRigFramePose* __restrict__ out)
{
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double p[7];
    for (int i = 0; i < 7; i++) p[i] = pose[(size_t)b * 7 + i];
    OrbmRigFramePose F;
    rig_frame_pose(cam, p, normalise, &F);
    out[b] = F;
}

// grid (ceil(pcap / 256), batch).  n_to_match[b] was cleared by the launch sequence and takes one atomicAdd per wave that saw a
// point in view of either camera.
__global__ __launch_bounds__(kBlock) void k_frustum_rig(const FrustumArgs A)
{
    const int b = blockIdx.y;
    const int p = blockIdx.x * kBlock + threadIdx.x;
    const int pcap = A.pts.pcap;
    const bool in_range = p < pcap;
    const size_t row = (size_t)b * pcap + (in_range ? p : 0);
    const bool live = in_range && p < A.pts.n[b] && !A.pts.skip[row] && !A.pts.bad[row];
    bool seen = false;
    if (live) {
        const OrbmRigFramePose& F = A.pose[b];
        const float P[3] = {A.pts.xyz[row * 3], A.pts.xyz[row * 3 + 1], A.pts.xyz[row * 3 + 2]};
        const float Pn[3] = {A.pts.normal[row * 3], A.pts.normal[row * 3 + 1], A.pts.normal[row * 3 + 2]};
        const float mn = A.pts.min_distance[row], mx = A.pts.max_distance[row];
        const Side l = frustum_left(A.cam, F, P, Pn, mn, mx, A.cos_limit);
        A.out.in_view[row] = (uint8_t)l.valid;
        A.out.pred_level[row] = l.level;
        if (l.valid) {
            A.out.proj_u[row] = l.u; A.out.proj_v[row] = l.v;
            A.out.view_cos[row] = l.view_cos; A.out.track_depth[row] = l.depth;
        }
        const Side r = frustum_right(A.cam, F, P, Pn, mn, mx, A.cos_limit);
        A.out.in_view_r[row] = (uint8_t)r.valid;
        A.out.pred_level_r[row] = r.level;
        if (r.valid) {
            A.out.proj_u_r[row] = r.u; A.out.proj_v_r[row] = r.v;
            A.out.view_cos_r[row] = r.view_cos; A.out.track_depth_r[row] = r.depth;
        }
        seen = l.valid || r.valid;
    } else if (in_range) {                              // the loop of src/Tracking.cc:3490-3507: mbTrackInView(R) = false, nothing else
        A.out.in_view[row] = 0;
        A.out.in_view_r[row] = 0;
    }
    const unsigned long long in_view = __ballot(seen);
    if (in_view != 0 && (threadIdx.x & 63) == 0) atomicAdd(&A.out.n_to_match[b], __popcll(in_view));
}

__global__ __launch_bounds__(kBlock) void k_project_last_rig(const LastArgs A)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.cap) return;
    const size_t row = (size_t)b * A.cap + i;
    LastRow r{0, -1.f, -1.f, -1.f, -1.f};
    if (i < A.n[b] && A.has_point[row]) {
        const float x[3] = {A.xyz[row * 3], A.xyz[row * 3 + 1], A.xyz[row * 3 + 2]};
        r = project_last_rig_row(A.cam, A.pose[b], x);
    }
    A.out.valid[row] = (uint8_t)r.valid;
    A.out.proj_u[row] = r.u; A.out.proj_v[row] = r.v;
    A.out.proj_u_r[row] = r.ur; A.out.proj_v_r[row] = r.vr;
}

__global__ __launch_bounds__(kBlock) void k_unproject_stereo_fisheye(const UnprojectArgs A)
{
    const int b = blockIdx.y;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= A.cap || i >= A.n[b]) return;
    const size_t row = (size_t)b * A.cap + i;
    if (!A.valid[row]) return;
    const float p[3] = {A.points[row * 3], A.points[row * 3 + 1], A.points[row * 3 + 2]};
    float w[3];
    unproject_stereo_fisheye(A.pose[b], p, w);
    A.world[row * 3] = w[0]; A.world[row * 3 + 1] = w[1]; A.world[row * 3 + 2] = w[2];
}

}  // namespace tpr

static int check_batch(int batch)
{
    if (batch < 1) return fail(ORBX_ERR_ARG, "batch %d < 1", batch);
    if (batch > ORBM_TRACK_MAX_BATCH) return fail(ORBX_ERR_CAPACITY, "batch %d above %d", batch, ORBM_TRACK_MAX_BATCH);
    return ORBX_OK;
}

static int check_camera(const OrbmTrackRigCamera* cam, int batch)
{
    if (!cam) return fail(ORBX_ERR_ARG, "cam is NULL");
    if (cam->n_levels < 1 || cam->n_levels > ORBM_TRACK_MAX_LEVELS) return fail(ORBX_ERR_ARG, "n_levels %d outside [1, %d]", cam->n_levels, ORBM_TRACK_MAX_LEVELS);
    return check_batch(batch);
}

static int check_last(const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const float* xyz, const uint8_t* has_point, const int32_t* n, int cap,
                      const OrbmRigLastProjOut* out, int batch)
{
    if (!poses || !xyz || !has_point || !n || !out) return fail(ORBX_ERR_ARG, "NULL argument");
    if (!out->valid || !out->proj_u || !out->proj_v || !out->proj_u_r || !out->proj_v_r) return fail(ORBX_ERR_ARG, "NULL output array");
    if (cap <= 0) return fail(ORBX_ERR_ARG, "cap %d <= 0", cap);
    return check_camera(cam, batch);
}

static int check_unproject(const OrbmRigFramePose* poses, const float* points, const uint8_t* valid, const int32_t* n, int cap, const float* world, int batch)
{
    if (!poses || !points || !valid || !n || !world) return fail(ORBX_ERR_ARG, "NULL argument");
    if (cap <= 0) return fail(ORBX_ERR_ARG, "cap %d <= 0", cap);
    return check_batch(batch);
}

static dim3 row_grid(int rows, int batch) { return dim3((unsigned)((rows + tpr::kBlock - 1) / tpr::kBlock), (unsigned)batch); }

static int launch_frustum(const tpr::FrustumArgs& A, int batch, hipStream_t st)
{
    ORBX_HIP(hipMemsetAsync(A.out.n_to_match, 0, sizeof(int32_t) * (size_t)batch, st));
    hipLaunchKernelGGL(tpr::k_frustum_rig, row_grid(A.pts.pcap, batch), dim3(tpr::kBlock), 0, st, A);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

static int launch_last(const tpr::LastArgs& A, int batch, hipStream_t st)
{
    hipLaunchKernelGGL(tpr::k_project_last_rig, row_grid(A.cap, batch), dim3(tpr::kBlock), 0, st, A);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

static int launch_unproject(const tpr::UnprojectArgs& A, int batch, hipStream_t st)
{
    hipLaunchKernelGGL(tpr::k_unproject_stereo_fisheye, row_grid(A.cap, batch), dim3(tpr::kBlock), 0, st, A);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

// upload the whole blob (inputs, then the in/out and output arrays), run, download [out0, size)
template <class Launch>
static int run_staged(orbm_matcher* m, Blob& blob, size_t out0, Launch launch)
{
    hipStream_t st = m->stream;
    ORBX_HIP(hipMemcpyAsync(m->d_blob, blob.buf.data(), blob.size(), hipMemcpyHostToDevice, st));
    if (int r = m->tpr_timer.start(st)) return r;
    if (int r = launch(st)) return r;
    if (int r = m->tpr_timer.stop(st)) return r;
    ORBX_HIP(hipMemcpyAsync(blob.buf.data() + out0, m->d_blob + out0, blob.size() - out0, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    return m->tpr_timer.read();
}

extern "C" {

int orbm_track_project_rig_check(const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const OrbmLocalPoints* pts, const OrbmRigFrustumOut* out, int batch)
{
    if (!poses || !pts || !out) return fail(ORBX_ERR_ARG, "NULL argument");
    if (!pts->xyz || !pts->normal || !pts->min_distance || !pts->max_distance || !pts->skip || !pts->bad || !pts->n) return fail(ORBX_ERR_ARG, "NULL local-point array");
    if (!out->in_view || !out->pred_level || !out->in_view_r || !out->pred_level_r || !out->n_to_match) return fail(ORBX_ERR_ARG, "NULL output array");
    if (!out->proj_u || !out->proj_v || !out->view_cos || !out->track_depth || !out->proj_u_r || !out->proj_v_r || !out->view_cos_r || !out->track_depth_r)
        return fail(ORBX_ERR_ARG, "NULL in/out array");
    if (pts->pcap <= 0) return fail(ORBX_ERR_ARG, "pcap %d <= 0", pts->pcap);
    return check_camera(cam, batch);
}

int orbm_rig_frame_pose_batch_device(orbm_matcher* m, const OrbmTrackRigCamera* cam, const double* d_pose, int batch, int normalise,
                                     OrbmRigFramePose* d_rig_pose, void* stream)
{
    if (!m || !cam || !d_pose || !d_rig_pose) return fail(ORBX_ERR_ARG, "NULL argument");
    if (int r = check_batch(batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    hipLaunchKernelGGL(tpr::k_frame_pose_rig, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, *cam, d_pose, batch, normalise ? 1 : 0, d_rig_pose);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int orbm_frustum_rig_batch_device(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* d_rig_pose, const OrbmLocalPoints* pts,
                                  float viewing_cos_limit, const OrbmRigFrustumOut* out, int batch, void* stream)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = orbm_track_project_rig_check(cam, d_rig_pose, pts, out, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    return launch_frustum(tpr::FrustumArgs{*cam, d_rig_pose, *pts, *out, viewing_cos_limit}, batch, (hipStream_t)stream);
}

int orbm_project_last_rig_batch_device(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* d_rig_pose,
                                       const float* d_mp_xyz, const uint8_t* d_has_point, const int32_t* d_n, int cap,
                                       const OrbmRigLastProjOut* out, int batch, void* stream)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = check_last(cam, d_rig_pose, d_mp_xyz, d_has_point, d_n, cap, out, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    return launch_last(tpr::LastArgs{*cam, d_rig_pose, d_mp_xyz, d_has_point, d_n, cap, *out}, batch, (hipStream_t)stream);
}

int orbm_unproject_stereo_fisheye_batch_device(orbm_matcher* m, const OrbmRigFramePose* d_rig_pose, const float* d_points, const uint8_t* d_valid,
                                               const int32_t* d_n, int cap, float* d_world, int batch, void* stream)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = check_unproject(d_rig_pose, d_points, d_valid, d_n, cap, d_world, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    return launch_unproject(tpr::UnprojectArgs{d_rig_pose, d_points, d_valid, d_n, cap, d_world}, batch, (hipStream_t)stream);
}

int orbm_frustum_rig_batch(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses, const OrbmLocalPoints* pts,
                           float viewing_cos_limit, const OrbmRigFrustumOut* out, int batch)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = orbm_track_project_rig_check(cam, poses, pts, out, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    if (int r = m->tpr_timer.create()) return r;
    const size_t B = (size_t)batch, rows = B * (size_t)pts->pcap;
    tpr::FrustumArgs A{*cam, nullptr, *pts, *out, viewing_cos_limit};
    Blob blob(m);
    blob.in(A.pose, poses, B);
    blob.in(A.pts.xyz, pts->xyz, rows * 3); blob.in(A.pts.normal, pts->normal, rows * 3);
    blob.in(A.pts.min_distance, pts->min_distance, rows); blob.in(A.pts.max_distance, pts->max_distance, rows);
    blob.in(A.pts.skip, pts->skip, rows); blob.in(A.pts.bad, pts->bad, rows); blob.in(A.pts.n, pts->n, B);
    const size_t out0 = blob.begin_out();
    float* OrbmRigFrustumOut::* const stale[8] = {&OrbmRigFrustumOut::proj_u, &OrbmRigFrustumOut::proj_v, &OrbmRigFrustumOut::view_cos, &OrbmRigFrustumOut::track_depth,
                                                  &OrbmRigFrustumOut::proj_u_r, &OrbmRigFrustumOut::proj_v_r, &OrbmRigFrustumOut::view_cos_r, &OrbmRigFrustumOut::track_depth_r};
    for (auto f : stale) blob.inout(A.out.*f, out->*f, rows);
    // pred_level of a skipped row is kept too: the four verdict arrays go up as the caller holds them
    blob.inout(A.out.in_view, out->in_view, rows); blob.inout(A.out.in_view_r, out->in_view_r, rows);
    blob.inout(A.out.pred_level, out->pred_level, rows); blob.inout(A.out.pred_level_r, out->pred_level_r, rows);
    blob.out(A.out.n_to_match, B);
    if (int r = m->ensure(blob.size())) return r;
    blob.bind(m->d_blob);
    if (int r = run_staged(m, blob, out0, [&](hipStream_t st) { return launch_frustum(A, batch, st); })) return r;
    for (auto f : stale) std::memcpy(out->*f, blob.host(A.out.*f), rows * 4);
    std::memcpy(out->in_view, blob.host(A.out.in_view), rows); std::memcpy(out->in_view_r, blob.host(A.out.in_view_r), rows);
    std::memcpy(out->pred_level, blob.host(A.out.pred_level), rows * 4); std::memcpy(out->pred_level_r, blob.host(A.out.pred_level_r), rows * 4);
    std::memcpy(out->n_to_match, blob.host(A.out.n_to_match), B * 4);
    return ORBX_OK;
}

int orbm_project_last_rig_batch(orbm_matcher* m, const OrbmTrackRigCamera* cam, const OrbmRigFramePose* poses,
                                const float* mp_xyz, const uint8_t* has_point, const int32_t* n, int cap,
                                const OrbmRigLastProjOut* out, int batch)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = check_last(cam, poses, mp_xyz, has_point, n, cap, out, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    if (int r = m->tpr_timer.create()) return r;
    const size_t B = (size_t)batch, rows = B * (size_t)cap;
    tpr::LastArgs A{*cam, nullptr, nullptr, nullptr, nullptr, cap, *out};
    Blob blob(m);
    blob.in(A.pose, poses, B);
    blob.in(A.xyz, mp_xyz, rows * 3); blob.in(A.has_point, has_point, rows); blob.in(A.n, n, B);
    const size_t out0 = blob.begin_out();
    blob.out(A.out.valid, rows); blob.out(A.out.proj_u, rows); blob.out(A.out.proj_v, rows); blob.out(A.out.proj_u_r, rows); blob.out(A.out.proj_v_r, rows);
    if (int r = m->ensure(blob.size())) return r;
    blob.bind(m->d_blob);
    if (int r = run_staged(m, blob, out0, [&](hipStream_t st) { return launch_last(A, batch, st); })) return r;
    std::memcpy(out->valid, blob.host(A.out.valid), rows);
    std::memcpy(out->proj_u, blob.host(A.out.proj_u), rows * 4); std::memcpy(out->proj_v, blob.host(A.out.proj_v), rows * 4);
    std::memcpy(out->proj_u_r, blob.host(A.out.proj_u_r), rows * 4); std::memcpy(out->proj_v_r, blob.host(A.out.proj_v_r), rows * 4);
    return ORBX_OK;
}

int orbm_unproject_stereo_fisheye_batch(orbm_matcher* m, const OrbmRigFramePose* poses, const float* points, const uint8_t* valid,
                                        const int32_t* n, int cap, float* world, int batch)
{
    if (!m) return fail(ORBX_ERR_ARG, "matcher is NULL");
    if (int r = check_unproject(poses, points, valid, n, cap, world, batch)) return r;
    ORBX_HIP(hipSetDevice(m->device));
    if (int r = m->tpr_timer.create()) return r;
    const size_t B = (size_t)batch, rows = B * (size_t)cap;
    tpr::UnprojectArgs A{nullptr, nullptr, nullptr, nullptr, cap, nullptr};
    Blob blob(m);
    blob.in(A.pose, poses, B);
    blob.in(A.points, points, rows * 3); blob.in(A.valid, valid, rows); blob.in(A.n, n, B);
    const size_t out0 = blob.begin_out();
    blob.inout(A.world, world, rows * 3);               // rows without a point keep what the caller holds
    if (int r = m->ensure(blob.size())) return r;
    blob.bind(m->d_blob);
    if (int r = run_staged(m, blob, out0, [&](hipStream_t st) { return launch_unproject(A, batch, st); })) return r;
    std::memcpy(world, blob.host(A.world), rows * 12);
    return ORBX_OK;
}

float orbm_track_project_rig_last_kernel_ms(const orbm_matcher* m) { return m ? m->tpr_timer.ms : 0.f; }

}  // extern "C"
