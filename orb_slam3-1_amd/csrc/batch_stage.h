// Host side of the one-workgroup-per-problem solvers (pose_solver.hip, sim3_solver.hip): a batch is laid out in ONE pinned
// buffer with a device image, [descriptors | inputs] go up, one launch runs, [outputs] come down.  Host only.
#pragma once
#include <algorithm>
#include <cstdint>
#include <exception>
#include <new>

#include "hip_check.h"

namespace stage {

struct Batch {
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
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return fail(ORBX_ERR_NO_DEVICE, "no HIP device available");
    if (device < 0 || device >= ndev) return fail(ORBX_ERR_ARG, "device %d out of range", device);
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

}  // namespace stage
