// Host-side state of the orbm_matcher handle and the blob packer its entry points share (orbm_matcher.hip, orbm_new_points.hip
// and stereo_fisheye.hip): every host-buffer entry packs its arrays into one pinned blob and moves them with one copy.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <new>
#include <type_traits>
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

// two events around the kernels of an entry, created on first use; ms is the kernel time of the entry's last call
struct KernelTimer {
    hipEvent_t ev[2] = {nullptr, nullptr};
    float ms = 0.f;
    ~KernelTimer()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    int create()                        // (before the upload: nothing may fail between the copies and the launch)
    {
        for (hipEvent_t& e : ev)
            if (!e) ORBX_HIP(hipEventCreate(&e));
        return ORBX_OK;
    }
    int start(hipStream_t s) { ORBX_HIP(hipEventRecord(ev[0], s)); return ORBX_OK; }
    int stop(hipStream_t s) { ORBX_HIP(hipEventRecord(ev[1], s)); return ORBX_OK; }
    int read() { ORBX_HIP(hipEventElapsedTime(&ms, ev[0], ev[1])); return ORBX_OK; }      // after the stream was synchronised
};

struct orbm_matcher {
    int device = 0;
    hipStream_t stream = nullptr;
    uint8_t* d_blob = nullptr;
    size_t blob_cap = 0;
    PinnedBytes h_blob;
    std::vector<void*> h_fields;        // Blob's record of the pointer fields it has to bind
    uint8_t* d_ws = nullptr;            // workspace of the device-resident batch entries (SoA key points, grids, logs, job table)
    size_t ws_cap = 0;
    float* d_scale = nullptr;           // scale factors of the last device-resident call
    float h_scale[32] = {};             // ... staged here: the asynchronous copy must not read the caller's array after the call returned
    KernelTimer nmp_timer;              // orbm_create_new_map_points: its one kernel
    KernelTimer sfe_timer;              // orbm_stereo_fisheye: its two kernels
    KernelTimer rig_timer;              // the rig-frame tracking searches: k_grid + k_rig
    KernelTimer rig_bow_timer;          // the rig SearchByBoW / SearchForTriangulation: k_bow_rig, or k_tri_rig + k_tri_rig_finish
    KernelTimer rig_nmp_timer;          // orbm_create_new_map_points_rig: k_new_map_points_rig, once per segment
    float rig_nmp_ms = 0.f;             // ... summed over the segments of the last call
    int rig_nmp_launches = 0;
    KernelTimer tp_timer;               // orbm_frustum_batch / orbm_project_last_batch: their one kernel
    KernelTimer tpr_timer;              // the host-array rig projections (orbm_frustum_rig_batch and its kin): their one kernel

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

// Host-side packer.  Every array is appended 16-byte aligned and its place goes straight into the pointer field of the kernel's
// argument struct: the field first holds the offset, bind(base) -- once, after the device blob is known -- turns every such field
// into base + offset.  Counts are in elements of the field's type.
// RULE: an argument struct lives in storage that does not move between its first in() and bind() -- the stack, or a std::vector
// sized before packing -- because the packer remembers the fields' addresses.  A struct the kernel reads from the blob gets a
// slot<T>() and is copied there with store() after bind().
// Inputs go first, outputs last: begin_out() / size() mark the split, so that upload and download are one copy each.
struct Blob {
    PinnedBytes& buf;
    std::vector<void*>& fields;         // the fields to bind (the caller's vector: reused across calls, no allocation in steady state)
    uint8_t* base = nullptr;
    Blob(PinnedBytes& b, std::vector<void*>& f) : buf(b), fields(f) { buf.clear(); fields.clear(); }
    explicit Blob(orbm_matcher* m) : Blob(m->h_blob, m->h_fields) {}
    size_t size() const { return buf.size(); }
    size_t begin_out() const { return (buf.size() + 15) & ~(size_t)15; }

    // a required array (src == NULL with count > 0: zeros); returns its offset, like out() and inout()
    template <class P> size_t in(P& field, const void* src, size_t count)
    {
        const size_t off = append(src, count * sizeof(*field));
        note(field, off);
        return off;
    }
    // an optional array: absent (src == NULL) it is a NON-NULL pointer to zero bytes, which no kernel reads
    template <class P> void in_opt(P& field, const void* src, size_t count) { in(field, src, src ? count : 0); }
    // fields the kernel does not read in this mode: non-null pointers to zero bytes as well
    template <class... P> void none(P&... field) { (in(field, nullptr, 0), ...); }
    // an optional array whose absence the kernel branches on: absent it is a real nullptr and takes no place
    template <class P> void in_or_null(P& field, const void* src, size_t count) { if (src) in(field, src, count); else field = nullptr; }
    // an array the kernel writes (zeros), and one it reads and writes
    template <class P> size_t out(P& field, size_t count) { return in(field, nullptr, count); }
    template <class P> size_t inout(P& field, const void* src, size_t count) { return in(field, src, count); }
    // a field that shares the array of another, already packed, field
    template <class P, class Q> void alias(P& field, const Q& packed) { note(field, (size_t)reinterpret_cast<uintptr_t>(packed)); }
    // room for n structs T that the kernel reads from the blob
    template <class T> size_t slot(size_t n) { return append(nullptr, sizeof(T) * n); }

    void bind(uint8_t* device_base)
    {
        base = device_base;
        for (void* f : fields) {
            uintptr_t v;
            std::memcpy(&v, f, sizeof(v));
            v += reinterpret_cast<uintptr_t>(base);
            std::memcpy(f, &v, sizeof(v));
        }
        fields.clear();
    }
    template <class T> void store(size_t slot_off, const T* structs, size_t n) { std::memcpy(buf.data() + slot_off, structs, sizeof(T) * n); }
    template <class T> const T* device(size_t slot_off) const { return (const T*)(base + slot_off); }
    template <class T> T* host(const T* bound) { return (T*)(buf.data() + ((const uint8_t*)bound - base)); }   // host copy of a bound field's array

private:
    size_t append(const void* src, size_t bytes)
    {
        const size_t off = (buf.size() + 15) & ~(size_t)15;
        buf.resize(off + bytes);
        if (src && bytes) std::memcpy(buf.data() + off, src, bytes);
        return off;
    }
    template <class P> void note(P& field, size_t off)
    {
        static_assert(std::is_pointer<P>::value && sizeof(P) == sizeof(uintptr_t), "a pointer field");
        field = reinterpret_cast<P>((uintptr_t)off);
        fields.push_back(&field);
    }
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
