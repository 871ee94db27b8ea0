// imu_preintegrate.hip -- IMU pre-integration on the device (include/orbslam3_hip_imu_preint.h): the interpolation loop of
// Tracking::PreintegrateIMU, IMU::Preintegrated::Initialize / IntegrateNewMeasurement, the informations of a link and the
// arithmetic of Tracking::PredictStateIMU.  One launch per entry-point call.
//
// Layout: ONE LANE PER JOB ("IMU pre-integration: a lane per job").  A job is a serial recurrence over its
// measurements; its whole state (the 9 x 9 covariance block and 66 further floats) lives in the lane's registers, the 9 x 9 update
// A C A^T + B N B^T is written out in 3 x 3 blocks (A is block lower triangular with identity blocks, B has three non-zero
// blocks), the next measurement is loaded before the current one is used, and no lane ever talks to another: no LDS, no barrier,
// no atomic, and a result cannot depend on what else the launch carries.
// The informations of a link (9 x 9 inverse, cyclic Jacobi) are in double, one lane per link, on private arrays.
#include <cmath>
#include <unordered_set>

#include "batch_stage.h"
#include "imu_preint_math.h"

namespace preint {

constexpr int kThreads = 64;

// ---- one lane per unit of work; the arithmetic is imu_preint_math.h ----
__global__ __launch_bounds__(kThreads) void k_preintegrate(ImuPreintState* __restrict__ states, int n_states, const ImuPreintJob* __restrict__ jobs, int n_jobs,
                                                           const ImuMeasurement* __restrict__ meas, int n_meas, int32_t* __restrict__ status, bool trusted)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n_jobs) preintegrate_job(states, n_states, jobs, n_jobs, meas, n_meas, status, j, trusted);
}

__global__ __launch_bounds__(kThreads) void k_frame_measurements(const OrbeImuSample* __restrict__ samples, const int32_t* __restrict__ n_imu,
                                                                 const int64_t* __restrict__ t_prev_ns, const int64_t* __restrict__ t_cur_ns, int batch, int imu_cap,
                                                                 ImuMeasurement* __restrict__ meas_out, int32_t* __restrict__ count_out)
{
    const int i = blockIdx.x * kThreads + threadIdx.x, bq = blockIdx.y;
    if (bq < batch) frame_measurement(samples, n_imu, t_prev_ns, t_cur_ns, imu_cap, meas_out, count_out, bq, i);
}

__global__ __launch_bounds__(kThreads) void k_links(const ImuPreintState* __restrict__ states, int n_states, const ImuLinkSpec* __restrict__ specs, int n_links,
                                                    LibaLink* __restrict__ links, int32_t* __restrict__ status)
{
    const int l = blockIdx.x * kThreads + threadIdx.x;
    if (l < n_links) build_link(states, n_states, specs, links, status, l);
}

__global__ __launch_bounds__(kThreads) void k_predict(const ImuPreintState* __restrict__ states, int n_states, const ImuPredictJob* __restrict__ jobs, int n_jobs,
                                                      ImuPredictOut* __restrict__ out, int32_t* __restrict__ status)
{
    const int j = blockIdx.x * kThreads + threadIdx.x;
    if (j < n_jobs) predict_job(states, n_states, jobs, out, status, j);
}

inline dim3 grid_for(int n) { return dim3((unsigned)((n + kThreads - 1) / kThreads)); }

}  // namespace preint

struct imu_preint : stage::Batch {};

namespace {

int check_shapes(const void* states, int n_states, const void* items, int n_items, const void* out, const void* status, const char* what)
{
    if (n_states < 0 || n_items < 0) return fail(ORBX_ERR_ARG, "%s: negative size", what);
    if ((n_states > 0 && !states) || (n_items > 0 && (!items || !out || !status))) return fail(ORBX_ERR_ARG, "%s: a pointer is NULL", what);
    return ORBX_OK;
}

int check_preintegrate(const ImuPreintState* states, int n_states, const ImuPreintJob* jobs, int n_jobs, const ImuMeasurement* meas, int n_meas)
{
    if (n_states < 0 || n_jobs < 0 || n_meas < 0) return fail(ORBX_ERR_ARG, "imu_preintegrate: negative size");
    if ((n_states > 0 && !states) || (n_jobs > 0 && !jobs) || (n_meas > 0 && !meas)) return fail(ORBX_ERR_ARG, "imu_preintegrate: a pointer is NULL");
    std::unordered_set<int32_t> written;
    for (int j = 0; j < n_jobs; j++) {
        const ImuPreintJob& q = jobs[j];
        if (q.state < 0 || q.state >= n_states) return fail(ORBX_ERR_ARG, "job %d: state %d out of range", j, q.state);
        if (q.first < 0 || q.count < 0 || q.first > n_meas || q.count > n_meas - q.first)
            return fail(ORBX_ERR_ARG, "job %d: measurements %d + %d out of range", j, q.first, q.count);
        if (!written.insert(q.state).second) return fail(ORBX_ERR_ARG, "job %d: state %d has two writers", j, q.state);
        if (q.reset)
            for (int k = 0; k < 6; k++) if (!std::isfinite(q.bias[k])) return fail(ORBX_ERR_ARG, "job %d: the bias is not finite", j);
        for (int i = 0; i < q.count; i++) {
            const ImuMeasurement& m = meas[q.first + i];
            bool ok = std::isfinite(m.dt);
            for (int k = 0; k < 3; k++) ok = ok && std::isfinite(m.a[k]) && std::isfinite(m.w[k]);
            if (!ok) return fail(ORBX_ERR_ARG, "job %d: measurement %d is not finite", j, q.first + i);
            if (!(m.dt > 0.f)) return fail(ORBX_ERR_ARG, "job %d: measurement %d has dt <= 0", j, q.first + i);
        }
    }
    return ORBX_OK;
}

// a host entry: [in0 | in1 | inout] up, one launch, [inout | status] down.  launch(d_in0, d_in1, d_inout, d_status)
template <class Launch>
int staged(imu_preint* h, const void* in0, size_t b0, const void* in1, size_t b1, void* inout, size_t b2, int32_t* status, size_t n_status, Launch&& launch)
{
    ORBX_HIP(hipSetDevice(h->device));
    stage::Cursor cur;
    const size_t o0 = cur.take(b0), o1 = cur.take(b1), o2 = cur.take(b2);
    const size_t up = cur.pos;
    const size_t os = cur.take(4 * n_status);
    if (int rc = stage::reserve(*h, cur.pos, cur.pos)) return rc;
    if (b0) std::memcpy(h->h_blob + o0, in0, b0);
    if (b1) std::memcpy(h->h_blob + o1, in1, b1);
    if (b2) std::memcpy(h->h_blob + o2, inout, b2);
    uint8_t* const d = h->d_blob;
    if (int rc = stage::run(*h, up, o2, cur.pos, [&] { launch(d + o0, d + o1, d + o2, (int32_t*)(d + os)); })) return rc;
    if (b2) std::memcpy(inout, h->h_blob + o2, b2);
    if (n_status) std::memcpy(status, h->h_blob + os, 4 * n_status);
    return ORBX_OK;
}

hipStream_t as_stream(void* s) { return (hipStream_t)s; }

}  // namespace

extern "C" {

int imu_preint_create(int device, imu_preint** out) { return stage::open(device, out); }

void imu_preint_destroy(imu_preint* h) { stage::close(h); }

double imu_preint_last_device_ms(const imu_preint* h) { return h ? (double)h->last_kernel_ms : 0.0; }

int imu_preint_check(const ImuPreintState* states, int n_states, const ImuPreintJob* jobs, int n_jobs, const ImuMeasurement* meas, int n_meas)
{
    return stage::guarded("imu_preint_check", [&] { return check_preintegrate(states, n_states, jobs, n_jobs, meas, n_meas); });
}

int imu_preintegrate_batch_device(imu_preint* h, ImuPreintState* d_states, int n_states, const ImuPreintJob* d_jobs, int n_jobs,
                                  const ImuMeasurement* d_meas, int n_meas, int32_t* d_status, void* stream)
{
    if (n_states < 0 || n_jobs < 0 || n_meas < 0) return fail(ORBX_ERR_ARG, "imu_preintegrate_batch_device: negative size");
    if ((n_states > 0 && !d_states) || (n_jobs > 0 && (!d_jobs || !d_status)) || (n_meas > 0 && !d_meas))
        return fail(ORBX_ERR_ARG, "imu_preintegrate_batch_device: a pointer is NULL");
    if (!h) return fail(ORBX_ERR_ARG, "the handle is NULL");
    if (n_jobs == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(preint::k_preintegrate, preint::grid_for(n_jobs), dim3(preint::kThreads), 0, as_stream(stream), d_states, n_states, d_jobs, n_jobs, d_meas,
                       n_meas, d_status, false);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int imu_preintegrate_batch(imu_preint* h, ImuPreintState* states, int n_states, const ImuPreintJob* jobs, int n_jobs, const ImuMeasurement* meas,
                           int n_meas, int32_t* status)
{
    return stage::guarded("imu_preintegrate_batch", [&]() -> int {
        if (int rc = check_preintegrate(states, n_states, jobs, n_jobs, meas, n_meas)) return rc;
        if (n_jobs > 0 && !status) return fail(ORBX_ERR_ARG, "imu_preintegrate: status is NULL");
        if (!h) return fail(ORBX_ERR_ARG, "the handle is NULL");
        if (n_jobs == 0) return ORBX_OK;
        return staged(h, jobs, sizeof(ImuPreintJob) * (size_t)n_jobs, meas, sizeof(ImuMeasurement) * (size_t)n_meas, states, sizeof(ImuPreintState) * (size_t)n_states,
                      status, (size_t)n_jobs, [&](uint8_t* dj, uint8_t* dm, uint8_t* ds, int32_t* dst) {
                          hipLaunchKernelGGL(preint::k_preintegrate, preint::grid_for(n_jobs), dim3(preint::kThreads), 0, h->stream, (ImuPreintState*)ds, n_states,
                                             (const ImuPreintJob*)dj, n_jobs, (const ImuMeasurement*)dm, n_meas, dst, true);
                      });
    });
}

int imu_frame_measurements_batch_device(imu_preint* h, const OrbeImuSample* d_samples, const int32_t* d_n_imu, const int64_t* d_t_prev_ns,
                                        const int64_t* d_t_cur_ns, int batch, int imu_cap, ImuMeasurement* d_meas_out, int32_t* d_count_out, void* stream)
{
    if (batch < 0 || imu_cap < 1) return fail(ORBX_ERR_ARG, "imu_frame_measurements_batch_device: batch < 0 or imu_cap < 1");
    if (batch > 65535) return fail(ORBX_ERR_ARG, "imu_frame_measurements_batch_device: more than 65535 streams");
    if (batch > 0 && (!d_samples || !d_n_imu || !d_t_prev_ns || !d_t_cur_ns || !d_meas_out || !d_count_out))
        return fail(ORBX_ERR_ARG, "imu_frame_measurements_batch_device: a pointer is NULL");
    if (!h) return fail(ORBX_ERR_ARG, "the handle is NULL");
    if (batch == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(h->device));
    const dim3 grid((unsigned)((imu_cap + preint::kThreads - 1) / preint::kThreads), (unsigned)batch);
    hipLaunchKernelGGL(preint::k_frame_measurements, grid, dim3(preint::kThreads), 0, as_stream(stream), d_samples, d_n_imu, d_t_prev_ns, d_t_cur_ns, batch, imu_cap,
                       d_meas_out, d_count_out);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int imu_frame_measurements_batch(imu_preint* h, const OrbeImuSample* samples, const int32_t* n_imu, const int64_t* t_prev_ns, const int64_t* t_cur_ns,
                                 int batch, int imu_cap, ImuMeasurement* meas_out, int32_t* count_out)
{
    return stage::guarded("imu_frame_measurements_batch", [&]() -> int {
        if (batch < 0 || imu_cap < 1 || batch > 65535) return fail(ORBX_ERR_ARG, "imu_frame_measurements_batch: batch outside 0 .. 65535 or imu_cap < 1");
        if (batch > 0 && (!samples || !n_imu || !t_prev_ns || !t_cur_ns || !meas_out || !count_out))
            return fail(ORBX_ERR_ARG, "imu_frame_measurements_batch: a pointer is NULL");
        for (int b = 0; b < batch; b++)
            if (n_imu[b] < 0 || n_imu[b] > imu_cap) return fail(ORBX_ERR_ARG, "stream %d: n_imu %d outside 0 .. %d", b, n_imu[b], imu_cap);
        if (!h) return fail(ORBX_ERR_ARG, "the handle is NULL");
        if (batch == 0) return ORBX_OK;
        // [samples | n_imu t_prev t_cur] up, [meas | count] down
        const size_t B = (size_t)batch, nb = sizeof(OrbeImuSample) * B * (size_t)imu_cap;
        std::vector<uint8_t> head(20 * B);
        std::memcpy(head.data(), t_prev_ns, 8 * B); std::memcpy(head.data() + 8 * B, t_cur_ns, 8 * B); std::memcpy(head.data() + 16 * B, n_imu, 4 * B);
        const size_t mb = sizeof(ImuMeasurement) * B * (size_t)imu_cap;
        std::vector<uint8_t> mout(mb, 0);
        const int rc = staged(h, samples, nb, head.data(), head.size(), mout.data(), mb, count_out, B, [&](uint8_t* dsmp, uint8_t* dh, uint8_t* dm, int32_t* dc) {
            const dim3 grid((unsigned)((imu_cap + preint::kThreads - 1) / preint::kThreads), (unsigned)batch);
            hipLaunchKernelGGL(preint::k_frame_measurements, grid, dim3(preint::kThreads), 0, h->stream, (const OrbeImuSample*)dsmp, (const int32_t*)(dh + 16 * B),
                               (const int64_t*)dh, (const int64_t*)(dh + 8 * B), batch, imu_cap, (ImuMeasurement*)dm, dc);
        });
        if (rc) return rc;
        for (size_t b = 0; b < B; b++)
            if (count_out[b] > 0) std::memcpy(meas_out + b * (size_t)imu_cap, mout.data() + sizeof(ImuMeasurement) * b * (size_t)imu_cap, sizeof(ImuMeasurement) * (size_t)count_out[b]);
        return ORBX_OK;
    });
}

int imu_links_batch_device(imu_preint* h, const ImuPreintState* d_states, int n_states, const ImuLinkSpec* d_specs, int n_links, LibaLink* d_links_out,
                           int32_t* d_status, void* stream)
{
    if (int rc = check_shapes(d_states, n_states, d_specs, n_links, d_links_out, d_status, "imu_links_batch_device")) return rc;
    if (!h) return fail(ORBX_ERR_ARG, "the handle is NULL");
    if (n_links == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(preint::k_links, preint::grid_for(n_links), dim3(preint::kThreads), 0, as_stream(stream), d_states, n_states, d_specs, n_links, d_links_out,
                       d_status);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int imu_links_batch(imu_preint* h, const ImuPreintState* states, int n_states, const ImuLinkSpec* specs, int n_links, LibaLink* links_out, int32_t* status)
{
    return stage::guarded("imu_links_batch", [&]() -> int {
        if (int rc = check_shapes(states, n_states, specs, n_links, links_out, status, "imu_links_batch")) return rc;
        for (int l = 0; l < n_links; l++)
            if (specs[l].state < 0 || specs[l].state >= n_states || specs[l].walk_state < -1 || specs[l].walk_state >= n_states)
                return fail(ORBX_ERR_ARG, "link %d: state %d or walk_state %d out of range", l, specs[l].state, specs[l].walk_state);
        if (!h) return fail(ORBX_ERR_ARG, "the handle is NULL");
        if (n_links == 0) return ORBX_OK;
        std::memset(links_out, 0, sizeof(LibaLink) * (size_t)n_links);         // (padding bytes included)
        return staged(h, states, sizeof(ImuPreintState) * (size_t)n_states, specs, sizeof(ImuLinkSpec) * (size_t)n_links, links_out, sizeof(LibaLink) * (size_t)n_links,
                      status, (size_t)n_links, [&](uint8_t* ds, uint8_t* dsp, uint8_t* dl, int32_t* dst) {
                          hipLaunchKernelGGL(preint::k_links, preint::grid_for(n_links), dim3(preint::kThreads), 0, h->stream, (const ImuPreintState*)ds, n_states,
                                             (const ImuLinkSpec*)dsp, n_links, (LibaLink*)dl, dst);
                      });
    });
}

int imu_predict_state_batch_device(imu_preint* h, const ImuPreintState* d_states, int n_states, const ImuPredictJob* d_jobs, int n_jobs, ImuPredictOut* d_out,
                                   int32_t* d_status, void* stream)
{
    if (int rc = check_shapes(d_states, n_states, d_jobs, n_jobs, d_out, d_status, "imu_predict_state_batch_device")) return rc;
    if (!h) return fail(ORBX_ERR_ARG, "the handle is NULL");
    if (n_jobs == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(h->device));
    hipLaunchKernelGGL(preint::k_predict, preint::grid_for(n_jobs), dim3(preint::kThreads), 0, as_stream(stream), d_states, n_states, d_jobs, n_jobs, d_out, d_status);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int imu_predict_state_batch(imu_preint* h, const ImuPreintState* states, int n_states, const ImuPredictJob* jobs, int n_jobs, ImuPredictOut* out, int32_t* status)
{
    return stage::guarded("imu_predict_state_batch", [&]() -> int {
        if (int rc = check_shapes(states, n_states, jobs, n_jobs, out, status, "imu_predict_state_batch")) return rc;
        for (int j = 0; j < n_jobs; j++)
            if (jobs[j].state < 0 || jobs[j].state >= n_states) return fail(ORBX_ERR_ARG, "job %d: state %d out of range", j, jobs[j].state);
        if (!h) return fail(ORBX_ERR_ARG, "the handle is NULL");
        if (n_jobs == 0) return ORBX_OK;
        std::memset(out, 0, sizeof(ImuPredictOut) * (size_t)n_jobs);
        return staged(h, states, sizeof(ImuPreintState) * (size_t)n_states, jobs, sizeof(ImuPredictJob) * (size_t)n_jobs, out, sizeof(ImuPredictOut) * (size_t)n_jobs,
                      status, (size_t)n_jobs, [&](uint8_t* ds, uint8_t* dj, uint8_t* dout, int32_t* dst) {
                          hipLaunchKernelGGL(preint::k_predict, preint::grid_for(n_jobs), dim3(preint::kThreads), 0, h->stream, (const ImuPreintState*)ds, n_states,
                                             (const ImuPredictJob*)dj, n_jobs, (ImuPredictOut*)dout, dst);
                      });
    });
}

}  // extern "C"
