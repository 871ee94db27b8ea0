// The host kit of the solver handles.  For all of them: handle creation and destruction (open / close; the device check,
// stage::check_device, is in hip_check.h, where the handles that use nothing else of this header find it).  For
// the one-workgroup-per-problem solvers (pose_solver.hip, sim3_solver.hip): a batch laid out in ONE pinned buffer with a device
// image, [descriptors | inputs] go up, one launch runs, [outputs] come down (reserve / Cursor / run).  For the host-driven
// Levenberg solvers (lba_solver.hip and its .inc files): the host-mapped scalars a trial's result arrives in (HostScalars), the
// window-setup thread pool (for_each_window) and the pinned result buffer of a batch (PinnedOut).  Host only.
#pragma once
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstring>
#include <exception>
#include <new>
#include <thread>
#include <vector>

#include "hip_check.h"

namespace stage {

struct Batch {                      // (the Levenberg handles built on open / close use the stream and the events only, not the blobs)
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    uint8_t* d_blob = nullptr;      // device image of h_blob (+ device-only scratch behind it)
    uint8_t* h_blob = nullptr;      // pinned staging
    size_t d_cap = 0, h_cap = 0;
    float last_kernel_ms = 0;
};

// deletes a solver S (a Batch, plus whatever ~S releases) with its stream, events and buffers
template <class S>
void close(S* s)
{
    if (!s) return;
    (void)hipSetDevice(s->device);
    if (s->stream) { (void)hipStreamSynchronize(s->stream); (void)hipStreamDestroy(s->stream); }
    if (s->ev0) (void)hipEventDestroy(s->ev0);
    if (s->ev1) (void)hipEventDestroy(s->ev1);
    if (s->d_blob) (void)hipFree(s->d_blob);
    if (s->h_blob) (void)hipHostFree(s->h_blob);
    delete s;
}

// a new solver S on `device` with its stream and the two events around the kernel
template <class S>
int open(int device, S** out)
{
    if (!out) return fail(ORBX_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (int r = check_device(device)) return r;
    ORBX_HIP(hipSetDevice(device));
    S* s = new (std::nothrow) S();
    if (!s) return fail(ORBX_ERR_INTERNAL, "out of host memory");
    s->device = device;
    if (hipStreamCreateWithFlags(&s->stream, hipStreamNonBlocking) != hipSuccess || hipEventCreate(&s->ev0) != hipSuccess ||
        hipEventCreate(&s->ev1) != hipSuccess) {
        close(s);
        return fail(ORBX_ERR_HIP, "stream / event create failed");
    }
    *out = s;
    return ORBX_OK;
}

// room for host_bytes staged and dev_bytes on the device; a buffer that is too small is replaced by one of twice the need (>= 1 MiB)
inline int reserve(Batch& s, size_t host_bytes, size_t dev_bytes)
{
    if (host_bytes > s.h_cap) {
        if (s.h_blob) (void)hipHostFree(s.h_blob);
        s.h_blob = nullptr; s.h_cap = 0;
        const size_t cap = std::max(host_bytes * 2, (size_t)1 << 20);
        ORBX_HIP(hipHostMalloc((void**)&s.h_blob, cap, hipHostMallocDefault));
        s.h_cap = cap;
    }
    if (dev_bytes > s.d_cap) {
        if (s.d_blob) (void)hipFree(s.d_blob);
        s.d_blob = nullptr; s.d_cap = 0;
        const size_t cap = std::max(dev_bytes * 2, (size_t)1 << 20);
        ORBX_HIP(hipMalloc((void**)&s.d_blob, cap));
        s.d_cap = cap;
    }
    return ORBX_OK;
}

// layout of a blob: every array starts on a 16-byte boundary
struct Cursor {
    size_t pos = 0;
    size_t take(size_t bytes)
    {
        const size_t at = pos;
        pos = (pos + bytes + 15) & ~(size_t)15;
        return at;
    }
};

// h_blob[0, up_bytes) up, launch() on s.stream between the two events, [down_off, down_end) down, wait; sets last_kernel_ms
template <class Launch>
int run(Batch& s, size_t up_bytes, size_t down_off, size_t down_end, Launch&& launch)
{
    ORBX_HIP(hipMemcpyAsync(s.d_blob, s.h_blob, up_bytes, hipMemcpyHostToDevice, s.stream));
    ORBX_HIP(hipEventRecord(s.ev0, s.stream));
    launch();
    ORBX_HIP(hipGetLastError());
    ORBX_HIP(hipEventRecord(s.ev1, s.stream));
    ORBX_HIP(hipMemcpyAsync(s.h_blob + down_off, s.d_blob + down_off, down_end - down_off, hipMemcpyDeviceToHost, s.stream));
    ORBX_HIP(hipStreamSynchronize(s.stream));
    (void)hipEventElapsedTime(&s.last_kernel_ms, s.ev0, s.ev1);
    return ORBX_OK;
}

// the C ABI does not let a C++ exception (bad_alloc of a std::vector) through: it becomes ORBX_ERR_INTERNAL
template <class Body>
int guarded(const char* what, Body&& body)
{
    try {
        return body();
    } catch (const std::exception& e) {
        return fail(ORBX_ERR_INTERNAL, "%s: %s", what, e.what());
    } catch (...) {
        return fail(ORBX_ERR_INTERNAL, "%s: unknown exception", what);
    }
}

// ---- the host-driven Levenberg solvers ----
// The reduction kernel that ends a linearisation or a trial writes its scalars into a host-mapped, coherent buffer, h[0..7], and
// then publishes the sequence number of the launch in h[8] (system-scope release): the host polls that word instead of paying
// a device-to-host copy and a stream synchronisation per trial.  A batched handle makes ONE allocation of 16 doubles per window
// and hands out views.
struct HostScalars {
    double* h = nullptr;            // pinned, host-mapped, coherent [16] (the owner: [slots][16])
    double* d = nullptr;            // the same words as the device sees them
    unsigned long long seq = 0;     // sequence number of the last launch that publishes here
    bool owner = false;

    int alloc(int slots = 1)
    {
        if (hipHostMalloc((void**)&h, (size_t)slots * 16 * sizeof(double), hipHostMallocMapped | hipHostMallocCoherent) != hipSuccess) { h = nullptr; return fail(ORBX_ERR_HIP, "hipHostMalloc failed"); }
        owner = true;
        if (hipHostGetDevicePointer((void**)&d, h, 0) != hipSuccess) return fail(ORBX_ERR_HIP, "hipHostGetDevicePointer failed");
        std::memset(h, 0, (size_t)slots * 16 * sizeof(double));
        return ORBX_OK;
    }
    // window `slot` of the allocation; the numbering goes on from what was last published there
    HostScalars view(int slot = 0) const
    {
        HostScalars v;
        v.h = h + 16 * (size_t)slot; v.d = d + 16 * (size_t)slot;
        v.seq = *(const unsigned long long*)(v.h + 8);
        return v;
    }
    void release()
    {
        if (owner && h) (void)hipHostFree(h);
        h = d = nullptr; owner = false;
    }
    // until launch `seq` has published: polling (a trial is a few hundred microseconds of kernels); after 20 ms a stream
    // synchronisation instead, which also surfaces faults
    int wait(hipStream_t stream) const
    {
        const volatile unsigned long long* flag = (const volatile unsigned long long*)(h + 8);
        const auto t0 = std::chrono::steady_clock::now();
        int spins = 0;
        while (*flag != seq) {
            if ((++spins & 1023) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(20)) {
                ORBX_HIP(hipStreamSynchronize(stream));
                if (*flag != seq) return fail(ORBX_ERR_INTERNAL, "reduction results did not arrive");
                break;
            }
        }
        std::atomic_thread_fence(std::memory_order_acquire);
        return ORBX_OK;
    }
};

// setup(i) for the W windows of a batch (structure build + upload: host work, ~0.3 ms a window) on up to 16 threads, each with
// `device` current.  The first window that failed is reported by number.
template <class Setup>
int for_each_window(int W, int device, Setup&& setup)
{
    const int n_thr = std::max(1, std::min({W, (int)std::thread::hardware_concurrency(), 16}));
    std::vector<int> rcs((size_t)W, ORBX_OK);
    std::atomic<int> next(0);
    auto worker = [&]() {
        (void)hipSetDevice(device);
        for (int i = next.fetch_add(1); i < W; i = next.fetch_add(1)) rcs[i] = setup(i);
    };
    std::vector<std::thread> th;
    for (int t = 1; t < n_thr; t++) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
    for (int i = 0; i < W; i++)
        if (rcs[i]) return fail(rcs[i], "window %d could not be set up (code %d; the worker thread holds the detailed message)", i, rcs[i]);
    return ORBX_OK;
}

// The results of the W windows of a batch back to back in one pinned buffer (with_device: and a device image of it), so that a
// call ends with one synchronisation: window i's slice starts at off[i], every array inside it on a 64-byte boundary.
struct PinnedOut {
    uint8_t *h = nullptr, *d = nullptr;
    size_t cap = 0;
    std::vector<size_t> off;
    static size_t al(size_t v) { return (v + 63) & ~(size_t)63; }
    // a window's slice: its states (state_bytes), 3 doubles per point, a double (chi2) and a byte (depth sign) per edge
    static size_t slice_bytes(size_t state_bytes, int n_points, int n_edges) { return al(state_bytes) + al(3 * (size_t)n_points * 8) + al((size_t)n_edges * 8) + al((size_t)n_edges); }
    struct Slice { uint8_t *state, *points, *chi2, *depth; };
    static Slice slice(uint8_t* base, size_t state_bytes, int n_points, int n_edges)
    {
        uint8_t* const points = base + al(state_bytes);
        uint8_t* const chi2 = points + al(3 * (size_t)n_points * 8);
        return Slice{base, points, chi2, chi2 + al((size_t)n_edges * 8)};
    }
    void clear() { off.assign(1, 0); }
    void add(size_t state_bytes, int n_points, int n_edges) { off.push_back(off.back() + slice_bytes(state_bytes, n_points, n_edges)); }
    size_t total() const { return off.back(); }
    // room for total(); a buffer that is too small is replaced by one a quarter larger than the need
    int reserve(bool with_device)
    {
        if (total() <= cap) return ORBX_OK;
        release();
        const size_t want = total() + total() / 4 + 4096;
        if (hipHostMalloc((void**)&h, want) != hipSuccess || (with_device && hipMalloc((void**)&d, want) != hipSuccess))
            return fail(ORBX_ERR_HIP, with_device ? "result buffer allocation failed" : "pinned result buffer allocation failed");
        cap = want;
        return ORBX_OK;
    }
    void release()
    {
        if (h) (void)hipHostFree(h);
        if (d) (void)hipFree(d);
        h = d = nullptr; cap = 0;
    }
};

// poses7 [n][7] (qx qy qz qw tx ty tz) -> pose_q [n][4], pose_t [n][3]; either may be NULL
inline void split_poses7(const double* poses7, int n, double* pose_q, double* pose_t)
{
    for (int i = 0; i < n; i++) {
        if (pose_q) for (int k = 0; k < 4; k++) pose_q[4 * i + k] = poses7[7 * (size_t)i + k];
        if (pose_t) for (int k = 0; k < 3; k++) pose_t[3 * i + k] = poses7[7 * (size_t)i + 4 + k];
    }
}

using Clock = std::chrono::steady_clock;
inline double ms(Clock::time_point a, Clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); }

}  // namespace stage
