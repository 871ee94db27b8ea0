// Host-side state of the orbm_matcher handle and the blob packer its entry points share (orbm_matcher.hip and
// orbm_new_points.hip): every host-buffer entry packs its arrays into one pinned blob and moves them with one copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <vector>

#include "../../include/orbslam3_hip.h"
#include "hip_check.h"

namespace orbm {

constexpr int TH_HIGH = 100, TH_LOW = 50, HISTO_LENGTH = 30;    // src/ORBmatcher.cc:35-37

__device__ __forceinline__ int hamming256(const uint8_t* __restrict__ a, const uint8_t* __restrict__ b)
{
    const unsigned long long* pa = (const unsigned long long*)a;
    const unsigned long long* pb = (const unsigned long long*)b;
    return __popcll(pa[0] ^ pb[0]) + __popcll(pa[1] ^ pb[1]) + __popcll(pa[2] ^ pb[2]) + __popcll(pa[3] ^ pb[3]);
}

}  // namespace orbm

// growable byte buffer in PINNED host memory: every host-buffer entry point packs its arrays here and moves them with one copy;
// from pageable memory that copy runs at a fraction of the link (24 MB for 256 frames of the last-frame search: 2 ms of its 2.5)
struct PinnedBytes {
    uint8_t* p = nullptr;
    size_t n = 0, cap = 0;
    ~PinnedBytes() { if (p) (void)hipHostFree(p); }
    PinnedBytes() = default;
    PinnedBytes(const PinnedBytes&) = delete;
    PinnedBytes& operator=(const PinnedBytes&) = delete;
    size_t size() const { return n; }
    uint8_t* data() { return p; }
    void clear() { n = 0; }
    void resize(size_t bytes)
    {
        if (bytes > cap) {
            const size_t want = std::max(bytes + bytes / 2, (size_t)1 << 16);
            uint8_t* q = nullptr;
            if (hipHostMalloc((void**)&q, want, hipHostMallocDefault) != hipSuccess) throw std::bad_alloc();
            if (p) { std::memcpy(q, p, n); (void)hipHostFree(p); }
            p = q; cap = want;
        }
        if (bytes > n) std::memset(p + n, 0, bytes - n);      // (std::vector semantics: new bytes are zero)
        n = bytes;
    }
};

struct orbm_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    uint8_t* d_blob = nullptr;
    size_t blob_cap = 0;
    PinnedBytes h_blob;
    uint8_t* d_ws = nullptr;            // workspace of the device-resident batch entries (SoA key points, grids, logs, job table)
    size_t ws_cap = 0;
    float* d_scale = nullptr;           // scale factors of the last device-resident call
    float h_scale[32] = {};             // ... staged here: the asynchronous copy must not read the caller's array after the call returned
    hipEvent_t nmp_ev[2] = {nullptr, nullptr};      // orbm_create_new_map_points: events around its one kernel (created on first use)
    float nmp_kernel_ms = 0.f;
    hipEvent_t sfe_ev[2] = {nullptr, nullptr};      // orbm_stereo_fisheye: events around its two kernels (created on first use)
    float sfe_kernel_ms = 0.f;
    hipEvent_t rig_ev[2] = {nullptr, nullptr};      // the rig-frame tracking searches: events around k_grid + k_rig (created on first use)
    float rig_kernel_ms = 0.f;

    int ensure(size_t bytes)
    {
        if (bytes <= blob_cap) return ORBX_OK;
        if (d_blob) (void)hipFree(d_blob);
        d_blob = nullptr; blob_cap = 0;
        const size_t cap = std::max(bytes * 2, (size_t)1 << 20);
        ORBX_HIP(hipMalloc((void**)&d_blob, cap));
        blob_cap = cap;
        return ORBX_OK;
    }
};

struct Blob {                   // host-side packer: every array is appended 16-byte aligned, device address = base + offset
    PinnedBytes& buf;
    explicit Blob(PinnedBytes& b) : buf(b) { buf.clear(); }
    size_t put(const void* src, size_t bytes)
    {
        const size_t off = (buf.size() + 15) & ~(size_t)15;
        buf.resize(off + bytes);
        if (src && bytes) std::memcpy(buf.data() + off, src, bytes);
        return off;
    }
    size_t reserve(size_t bytes) { return put(nullptr, bytes); }
};

inline bool features_unique(const OrbmFeatVec* fv, int n)
{
    std::vector<uint8_t> seen(std::max(n, 1), 0);
    const int total = fv->n_nodes > 0 ? fv->offset[fv->n_nodes] : 0;
    for (int i = 0; i < total; i++) {
        const uint32_t f = fv->feat[i];
        if ((int)f >= n || seen[f]) return false;
        seen[f] = 1;
    }
    return true;
}

inline int check_fv(const OrbmFeatVec* fv, int n, const char* name)
{
    if (!fv) return fail(ORBX_ERR_ARG, "%s is NULL", name);
    if (fv->n_nodes < 0) return fail(ORBX_ERR_ARG, "%s: negative node count", name);
    if (fv->n_nodes == 0) return ORBX_OK;
    if (!fv->node_id || !fv->offset || (!fv->feat && fv->offset[fv->n_nodes] > 0)) return fail(ORBX_ERR_ARG, "%s: NULL arrays", name);
    for (int k = 0; k < fv->n_nodes; k++) {
        if (fv->offset[k + 1] < fv->offset[k]) return fail(ORBX_ERR_ARG, "%s: offsets not monotone", name);
        if (k > 0 && fv->node_id[k] <= fv->node_id[k - 1]) return fail(ORBX_ERR_ARG, "%s: node ids not ascending", name);
    }
    const int total = fv->offset[fv->n_nodes];
    for (int i = 0; i < total; i++)
        if ((int)fv->feat[i] < 0 || (int)fv->feat[i] >= n) return fail(ORBX_ERR_ARG, "%s: feature index %u out of range", name, fv->feat[i]);
    return ORBX_OK;
}
