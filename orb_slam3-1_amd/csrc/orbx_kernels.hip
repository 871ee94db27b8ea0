// orbx_kernels.hip -- gfx950 kernels of the ORB extractor (reference src/ORBextractor.cc).
//
// Pipeline per batch of B frames (all launches cover the whole batch; blockIdx.y / .z = frame):
//   k_resize        level l-1 -> l, fixed-point bilinear; k_resize_tail: the upper levels in one launch (E1, ComputePyramid :1170-1195)
//   k_fast_strips   FAST-9/16 score + per-cell NMS / threshold fallback / ordered compaction, a workgroup per strip of cells
//                                                                    (E2, ComputeKeyPointsOctTree :787-872)
//   k_octree        quadtree keypoint selection, a workgroup of 1 / 2 / 4 waves per (frame, level): one control wave, a lane per node
//                   within a pass; the helper waves share the key partition of large nodes, the placement of the keys and the final selection
//                                                                    (E3, DistributeOctTree :555-779)
//   k_index         output slot of every keypoint (lapping-area split) (E8, operator() :1140-1167)
//   k_blur          7x7 sigma-2 Gaussian, Q8.8 fixed point             (E6, :1132-1133)
//   k_orient_desc   intensity-centroid angle + steered BRIEF-256, half a wave per keypoint (E5 :76-103, E7 :107-146)
//
// Integer stages are exact by construction; float stages use orbx_math.h (no FMA, no libm).
// HBM layout: one pyramid buffer per frame, levels back to back, row stride rounded up to 64 B so that
// every row starts on a 64-B boundary (coalesced dword loads); blurred pyramid has the same layout.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orbx_device.h"
#include "orbx_introsort.h"
#include "orbx_math.h"

namespace orbx {

__device__ __align__(16) const signed char d_pattern[1024] = {
#include "orb_pattern_31.inc"
};

typedef unsigned short us2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ us2 as_us2(uint32_t v) { return __builtin_bit_cast(us2, v); }
__device__ __forceinline__ uint32_t as_u32(us2 v) { return __builtin_bit_cast(uint32_t, v); }

// ------------------------------------------------------------------------------------------------
// E1: bilinear resize, OpenCV fixed-point scheme (cv::resize INTER_LINEAR 8UC1).  One thread -> 4 horizontally
// adjacent output pixels (one aligned dword store) of a BAND of 16 consecutive output rows; the lanes of a wave are the quads
// of one column strip in F frames of the batch (resize_band), so every lane of a wave is on the same output row.
// Everything that depends on the output column only is a host-built table per QUAD of columns: the first source column
// sx0, and per pixel a v_perm selector that pulls (S[sx], S[sx + 1]) out of the 8 source bytes starting at sx0 as a u16 pair,
// and the coefficient pair (ialpha0, ialpha1) -- so the horizontal pass of a pixel and source row is v_perm + v_dot2.
// The source rows are read straight from L2 / HBM (three dwords per row and thread, no LDS staging, no barrier).
// The source is addressed on its own (base, frame stride, row stride): level 1 is made from the caller's image in place.
// ------------------------------------------------------------------------------------------------
struct SrcImage {
    const uint8_t* base;        // first pixel of frame 0
    size_t frame_stride;        // bytes between frames
    int32_t stride, w, h;       // row stride in bytes (multiple of 4), size
};

// high dword of the 48-bit product of two 24-bit factors (v_mul_hi_u32_u24)
__device__ __forceinline__ uint32_t mul_hi_u24(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)(a & 0xFFFFFFu) * (uint64_t)(b & 0xFFFFFFu)) >> 32); }

struct __attribute__((aligned(4))) Dwords3 { uint32_t x, y, z; };     // 12 bytes at dword alignment: one global_load_dwordx3
typedef uint32_t u32x3 __attribute__((ext_vector_type(3)));
typedef __attribute__((address_space(1))) uint32_t global_u32;
typedef __attribute__((address_space(1))) u32x3 global_u32x3 __attribute__((aligned(4)));     // ... as a vector in global memory: the load stays one instruction
struct __attribute__((aligned(4))) Dwords4 { uint32_t x, y, z, w; };  // 16 bytes at dword alignment: one global_load_dwordx4
// a wave-uniform pointer, opaque to the compiler at this point: what is added to it afterwards is not folded into it
// (returned as a pointer into global memory: a pointer out of a register has no address space the compiler could infer)
typedef __attribute__((address_space(1))) uint8_t global_u8;
__device__ __forceinline__ global_u8* scalar_base(const uint8_t* p) { uint64_t v = (uint64_t)p; asm("" : "+s"(v)); return (global_u8*)v; }

// Four vertical sums t = b0 h0 + b1 h1 + 2 (each term after its shift) -> the four result bytes (t >> 2) of a quad as one dword.
// SAT = false: the host has checked a0 + a1 <= 2048 for every column and b0 + b1 <= 2048 for every row of the level, so each
// product term is at most b * 255 / 512, t at most 1022 and t >> 2 at most 255 -- no clamp: pixels 0 | 2 and 1 | 3 as u16 pairs
// (one v_perm each), one packed 16-bit shift each (nothing crosses the halves), one v_lshl_or: 5 instructions against 11.
template <bool SAT>
__device__ __forceinline__ uint32_t resize_pack(const uint32_t (&t)[4])
{
    if (SAT) return min(t[0] >> 2, 255u) | (min(t[1] >> 2, 255u) << 8) | (min(t[2] >> 2, 255u) << 16) | (min(t[3] >> 2, 255u) << 24);
    const us2 sh2 = {2, 2};
    const uint32_t e = as_u32(as_us2(__builtin_amdgcn_perm(t[2], t[0], 0x05040100u)) >> sh2);
    const uint32_t o = as_u32(as_us2(__builtin_amdgcn_perm(t[3], t[1], 0x05040100u)) >> sh2);
    return e | (o << 8);
}

constexpr int kResizeRows = 64;        // output rows of a workgroup of k_resize: four bands of kResizeBand rows, one per wave
constexpr int kResizeGroup = 4;        // rows of a band whose fresh source rows are loaded together
constexpr int resize_strip_w(int F) { return 256 / F; }      // pixels of a column strip: 64 quads shared by F frames

// One work item of the table-driven resize: the band of kResizeBand output rows from row band * kResizeBand on, of the column
// strip `strip`, in F frames.  Lane (lane / (64 / F), lane % (64 / F)) = (frame of the group, quad of the strip): F = 4 is 16 quads
// (64 pixels) x 4 frames -- the levels are 179..533 pixels wide, a few percent of the lanes idle in the last strip -- and F = 1 is
// 64 quads of one frame (batches below 4 frames).  All frames of a batch share one geometry, so the output row, its ResizeRow
// entry (scalar loads), the source and destination row addresses and both vertical coefficients are wave-uniform; a lane adds its
// frame's and its column's byte offset as ONE 32-bit value (the host checks F x frame stride < 2 GiB for source and destination and
// takes F = 1 otherwise).  `S` / `D`: source image / destination level of the group's first frame, `n_frames` how many of the
// group's frames exist (lanes of frames past the batch do nothing).
// The band is walked top to bottom.  A lane keeps the masked horizontal sums (v_perm + v_dot2 + v_and per pixel) of the previous
// output row's two source rows; where ResizeRow::plan says that the row's top source row is the previous row's bottom one, its
// sums are taken as they are -- a scalar branch, not a select.  Consecutive rows share a source row five times out of six at scale
// 1.2 (1.2 fresh source rows per output row against 2), and a fresh row is one 12-byte load per lane and one horizontal pass.  The
// first row of a band computes both: 1/16 of a row per row.
// The fresh rows of kResizeGroup output rows are loaded together, and those of the next group are issued before the current
// group's stores.  SAT: resize_pack.
template <int F, bool SAT>
__device__ __forceinline__ void resize_band(const uint8_t* S, uint32_t s_frame_stride, int s_stride, uint8_t* D, uint32_t d_frame_stride,
                                            const LevelDesc& dst, const int* __restrict__ q_sx0, const uint4* __restrict__ q_sel,
                                            const uint4* __restrict__ q_alpha, const ResizeRow* __restrict__ rows, int strip, int band,
                                            int n_frames, int lane)
{
    constexpr int QL = 64 / F, G = kResizeGroup;
    static_assert(kResizeBand == 4 * G, "a band is four row groups");
    const int fsel = F == 1 ? 0 : lane / QL, q = strip * QL + (F == 1 ? lane : lane % QL);
    const int y0 = band * kResizeBand, nrows = min(kResizeBand, dst.h - y0);        // (both wave-uniform)
    if (fsel >= n_frames || 4 * q >= dst.w || nrows <= 0) return;
    const int sx0 = q_sx0[q];
    const uint4 sel = q_sel[q], al = q_alpha[q];
    const uint32_t sels[4] = {sel.x, sel.y, sel.z, sel.w}, als[4] = {al.x, al.y, al.z, al.w};
    const uint32_t a = (uint32_t)(sx0 & ~3);
    const uint32_t sh = (uint32_t)(sx0 & 3);
    const uint32_t last = (uint32_t)(s_stride - 4);             // last dword of a row: bytes past the row's pixels only meet coefficient 0
    const bool wide = a + 8 <= last;                            // one 12-byte load per row: the address unit handles 4 lanes per clock whatever the width
    const uint32_t s_off = (uint32_t)fsel * s_frame_stride + a, d_off = (uint32_t)fsel * d_frame_stride + 4u * (uint32_t)q;
    // the last quads of a row: never read past the row's last dword
    const uint32_t s_off0 = s_off + (min(a, last) - a), s_off1 = s_off + (min(a + 4, last) - a), s_off2 = s_off + (min(a + 8, last) - a);
    // (the row address is a scalar pair and stays one -- scalar_base() -- so that a lane's 32-bit offset is the instruction's
    // vector operand: no 64-bit vector addition per load or store)
    auto load_row = [&](uint32_t sy) __attribute__((always_inline)) -> u32x3 {
        const global_u8* row = scalar_base(S + (size_t)sy * (uint32_t)s_stride);
        if (wide) return *(const global_u32x3*)(row + s_off);
        u32x3 t;
        t.x = *(const global_u32*)(row + s_off0); t.y = *(const global_u32*)(row + s_off1); t.z = *(const global_u32*)(row + s_off2);
        return t;
    };
    // masked horizontal sums of the 4 pixels on one source row: S[sx] a0 + S[sx+1] a1 out of the 8 source bytes from column sx0 on
    auto hpass = [&](u32x3 raw, uint32_t (&h)[4]) __attribute__((always_inline)) {
        const uint32_t lo = __builtin_amdgcn_alignbyte(raw.y, raw.x, sh), hi = __builtin_amdgcn_alignbyte(raw.z, raw.y, sh);
#pragma unroll
        for (int k = 0; k < 4; k++)
            h[k] = __builtin_amdgcn_udot2(as_us2(__builtin_amdgcn_perm(hi, lo, sels[k])), as_us2(als[k]), 0u, false) & 0xFFFFF0u;    // (h < 2^24)
    };
    // the table entry (scalar loads; the table is padded to whole 64-row tiles); row i of the band reuses the previous row's bottom
    // row as its top row where the plan says so -- the band's first row has no previous row.  The two rare plans of clamped
    // rows (top = previous top, bottom = top) are not reused: such a row is loaded and filtered again.
    auto reuse_top = [&](const ResizeRow& rw, int i) __attribute__((always_inline)) { return i > 0 && (rw.plan & 3u) == kResizeTopPrevBottom; };
    auto issue = [&](int i, u32x3& top, u32x3& bot) __attribute__((always_inline)) {
        if (i >= nrows) return;
        const ResizeRow rw = rows[y0 + i];
        if (!reuse_top(rw, i)) top = load_row(rw.sy & 0xFFFFu);
        bot = load_row(rw.sy >> 16);
    };
    // The two sets of horizontal sums swap roles with every row: the bottom row's sums of row i are the top row's of row i + 1
    // where they are reused, so the reuse moves nothing.
    uint32_t hx[4], hy[4];
    auto finish = [&](int i, const u32x3& top, const u32x3& bot) __attribute__((always_inline)) {
        if (i >= nrows) return;
        uint32_t (&ht)[4] = (i & 1) ? hx : hy;
        uint32_t (&hb)[4] = (i & 1) ? hy : hx;
        const ResizeRow rw = rows[y0 + i];
        if (!reuse_top(rw, i)) hpass(top, ht);
        hpass(bot, hb);
        // (b * (h >> 4)) >> 16 is the high dword of (b << 12) * (h & ~15): b <= 2048 and h <= 255 * 2048 keep both factors inside
        // 24 bits (v_mul_hi_u32_u24); the table holds b << 12
        uint32_t t[4];
#pragma unroll
        for (int k = 0; k < 4; k++) t[k] = mul_hi_u24(rw.b0, ht[k]) + mul_hi_u24(rw.b1, hb[k]) + 2u;
        // columns past dst.w: coefficients 0 -> 0; the row padding absorbs the tail of the last dword
        *(global_u32*)(scalar_base(D + (size_t)(uint32_t)(y0 + i) * (uint32_t)dst.stride) + d_off) = resize_pack<SAT>(t);
    };
    // (the staged rows are variables of their own: as arrays the compiler keeps them as one wide register tuple and copies it)
    u32x3 ta0, ta1, ta2, ta3, ba0, ba1, ba2, ba3, tb0, tb1, tb2, tb3, bb0, bb1, bb2, bb3;
#define ORBX_RESIZE_GROUP(f, g, t, b) do { f(G * (g), t##0, b##0); f(G * (g) + 1, t##1, b##1); f(G * (g) + 2, t##2, b##2); f(G * (g) + 3, t##3, b##3); } while (0)
    ORBX_RESIZE_GROUP(issue, 0, ta, ba);
    ORBX_RESIZE_GROUP(issue, 1, tb, bb); ORBX_RESIZE_GROUP(finish, 0, ta, ba);
    ORBX_RESIZE_GROUP(issue, 2, ta, ba); ORBX_RESIZE_GROUP(finish, 1, tb, bb);
    ORBX_RESIZE_GROUP(issue, 3, tb, bb); ORBX_RESIZE_GROUP(finish, 2, ta, ba);
    ORBX_RESIZE_GROUP(finish, 3, tb, bb);
#undef ORBX_RESIZE_GROUP
}

template <int F, bool SAT>
__global__ __launch_bounds__(256) void k_resize(SrcImage src, uint8_t* __restrict__ pyr, size_t frame_stride, LevelDesc dst, int n_frames,
                                                const int* __restrict__ q_sx0, const uint4* __restrict__ q_sel, const uint4* __restrict__ q_alpha,
                                                const ResizeRow* __restrict__ rows)
{
    // a workgroup is 64 rows (a band per wave) of one column strip in F frames (blockIdx.y = group of F frames).  These tiles are
    // numbered row-major and handed to the XCDs in contiguous bands (xcd_remap), so the source rows a band of destination rows
    // needs are fetched by one L2 only
    const int strips_x = (dst.w + resize_strip_w(F) - 1) / resize_strip_w(F), tiles_y = (dst.h + kResizeRows - 1) / kResizeRows;
    const int tile = xcd_remap(blockIdx.x, gridDim.x, blockIdx.y);
    if (tile >= strips_x * tiles_y) return;
    const int ty = tile / strips_x, tx = tile - ty * strips_x;
    const int f0 = blockIdx.y * F, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    resize_band<F, SAT>(src.base + (size_t)f0 * src.frame_stride, (uint32_t)src.frame_stride, src.stride, pyr + (size_t)f0 * frame_stride + dst.off,
                        (uint32_t)frame_stride, dst, q_sx0, q_sel, q_alpha, rows, tx, ty * (kResizeRows / kResizeBand) + wave, n_frames - f0,
                        threadIdx.x & 63);
}

// Fallback for levels whose four-column source span exceeds the 8-byte window of the table-driven kernel above (scale factors of
// 2 and more: 3 x scale_x >= 6 source columns between the first and the last pixel of a quad, plus its right neighbour): one thread
// per output pixel straight from the per-column / per-row tables of cv::resize -- the same fixed-point arithmetic, no window.
__global__ __launch_bounds__(256) void k_resize_generic(SrcImage src, uint8_t* __restrict__ pyr, size_t frame_stride, LevelDesc dst,
                                                        const int* __restrict__ xofs, const short* __restrict__ ialpha,
                                                        const int* __restrict__ yofs, const short* __restrict__ ibeta)
{
    const int dx = blockIdx.x * blockDim.x + threadIdx.x, dy = blockIdx.y, frame = blockIdx.z;
    if (dx >= dst.w) return;
    const uint8_t* S = src.base + (size_t)frame * src.frame_stride;
    const int sx = xofs[dx], sy = yofs[dy];
    const uint32_t a0 = (uint16_t)ialpha[2 * dx], a1 = (uint16_t)ialpha[2 * dx + 1];
    const uint32_t b0 = (uint16_t)ibeta[2 * dy], b1 = (uint16_t)ibeta[2 * dy + 1];
    const int sy0 = min(max(sy, 0), src.h - 1), sy1 = min(max(sy + 1, 0), src.h - 1);
    const int sx1 = min(sx + 1, src.w - 1);                     // (its coefficient is 0 where sx is the last column)
    const uint8_t* r0 = S + (size_t)sy0 * src.stride;
    const uint8_t* r1 = S + (size_t)sy1 * src.stride;
    const uint32_t h0 = r0[sx] * a0 + r0[sx1] * a1, h1 = r1[sx] * a0 + r1[sx1] * a1;
    const uint32_t val = ((__umul24(b0, h0 >> 4) >> 16) + (__umul24(b1, h1 >> 4) >> 16) + 2u) >> 2;
    pyr[(size_t)frame * frame_stride + dst.off + (size_t)dy * dst.stride + dx] = (uint8_t)min(val, 255u);
}

// The work split of k_resize_tiles and k_resize_tail (below): one tile of 64 x 64 outputs of level `dst` of ONE frame by 4 waves
// (`wave` 0..3, 16 rows each), the rows across the lanes: a wave covers 16 quads (64 pixels) of FOUR rows at a time, and a
// thread's four rows are dy0 + 4 r, so both source rows of every output row are loaded and filtered (nothing is shared inside a
// thread) -- but a wave is short: one round of loads, four rows.  That is what the latency-bound users need.  The tail is one
// workgroup per frame: with resize_band's four frames per wave it is a quarter of the workgroups with four times the work each
// and took 181 us against 55.
// `S` and `D` are the frame's source image and destination level (wave-uniform: scalar registers); a thread addresses both with
// 32-bit byte offsets (the host refuses frames of 2 GiB and more).  Everything that depends on the output row only is the
// host-built `rows` table (ResizeRow, padded to whole tiles): the two source rows, already clamped, and the two coefficients.
constexpr int kResizeTileW = 64;
template <bool SAT>
__device__ __forceinline__ void resize_tile(const uint8_t* __restrict__ S, int s_stride, uint8_t* __restrict__ D, const LevelDesc& dst,
                                            const int* __restrict__ q_sx0, const uint4* __restrict__ q_sel, const uint4* __restrict__ q_alpha,
                                            const ResizeRow* __restrict__ rows, int tile, int lane, int wave)
{
    const int tiles_x = (dst.w + kResizeTileW - 1) / kResizeTileW;
    const int ty = tile / tiles_x, tx = tile - ty * tiles_x;
    const int q = tx * (kResizeTileW / 4) + (lane & 15), rsel = lane >> 4;
    if (4 * q >= dst.w) return;
    constexpr int NR = kResizeRows / 16;                        // row groups of 4 per wave
    const int dy0 = ty * kResizeRows + wave * (kResizeRows / 4) + rsel;
    ResizeRow rw[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) rw[r] = *(const ResizeRow*)((const uint8_t*)rows + (((uint32_t)dy0 << 4) + 64u * r));
    const int sx0 = q_sx0[q];
    const uint4 sel = q_sel[q], al = q_alpha[q];
    const uint32_t sels[4] = {sel.x, sel.y, sel.z, sel.w}, als[4] = {al.x, al.y, al.z, al.w};
    const uint32_t a = (uint32_t)(sx0 & ~3);
    const uint32_t sh = (uint32_t)(sx0 & 3);
    const uint32_t last = (uint32_t)(s_stride - 4);             // last dword of a row: bytes past the row's pixels only meet coefficient 0
    // all the loads of the wave's rows are issued before the first result is stored (the compiler cannot move a load above a
    // store through pointers it cannot tell apart)
    uint32_t u[NR][3], v[NR][3], r0[NR], r1[NR];
#pragma unroll
    for (int r = 0; r < NR; r++) { r0[r] = __umul24(rw[r].sy & 0xFFFFu, (uint32_t)s_stride) + a; r1[r] = __umul24(rw[r].sy >> 16, (uint32_t)s_stride) + a; }
    if (a + 8 <= last) {            // one 12-byte load per row: the address unit handles 4 lanes per clock whatever the width
#pragma unroll
        for (int r = 0; r < NR; r++) {
            const Dwords3 tu = *(const Dwords3*)(S + r0[r]), tv = *(const Dwords3*)(S + r1[r]);
            u[r][0] = tu.x; u[r][1] = tu.y; u[r][2] = tu.z;
            v[r][0] = tv.x; v[r][1] = tv.y; v[r][2] = tv.z;
        }
    } else {                        // the last quads of a row: never read past the row's last dword
        const uint32_t d1 = min(a + 4, last) - a, d2 = min(a + 8, last) - a;
#pragma unroll
        for (int r = 0; r < NR; r++) {
            u[r][0] = *(const uint32_t*)(S + r0[r]); u[r][1] = *(const uint32_t*)(S + (r0[r] + d1)); u[r][2] = *(const uint32_t*)(S + (r0[r] + d2));
            v[r][0] = *(const uint32_t*)(S + r1[r]); v[r][1] = *(const uint32_t*)(S + (r1[r] + d1)); v[r][2] = *(const uint32_t*)(S + (r1[r] + d2));
        }
    }
    const uint32_t off0 = __umul24((uint32_t)dy0, (uint32_t)dst.stride) + 4u * (uint32_t)q;
#pragma unroll
    for (int r = 0; r < NR; r++) {
        if (dy0 + 4 * r >= dst.h) continue;
        // (b * (h >> 4)) >> 16 is the high dword of (b << 12) * (h & ~15): b <= 2048 and h <= 255 * 2048 keep both factors inside
        // 24 bits (v_mul_hi_u32_u24); the table holds b << 12
        const uint32_t b0 = rw[r].b0, b1 = rw[r].b1;
        // the 8 source bytes from column sx0 on, per row
        const uint32_t ulo = __builtin_amdgcn_alignbyte(u[r][1], u[r][0], sh), uhi = __builtin_amdgcn_alignbyte(u[r][2], u[r][1], sh);
        const uint32_t vlo = __builtin_amdgcn_alignbyte(v[r][1], v[r][0], sh), vhi = __builtin_amdgcn_alignbyte(v[r][2], v[r][1], sh);
        uint32_t out[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const us2 ak = as_us2(als[k]);
            const uint32_t h0 = __builtin_amdgcn_udot2(as_us2(__builtin_amdgcn_perm(uhi, ulo, sels[k])), ak, 0u, false);    // S0[sx] a0 + S0[sx+1] a1
            const uint32_t h1 = __builtin_amdgcn_udot2(as_us2(__builtin_amdgcn_perm(vhi, vlo, sels[k])), ak, 0u, false);
            out[k] = mul_hi_u24(b0, h0 & ~15u) + mul_hi_u24(b1, h1 & ~15u) + 2u;
        }
        // (gfx950's v_ashr_pk_u8_i32 does shift, saturation and packing of two pixels in one instruction, but issues every 8.2
        // cycles against 4.2-4.3 for each of resize_pack's: not used)
        // columns past dst.w: coefficients 0 -> 0; the row padding absorbs the tail of the last dword
        *(uint32_t*)(D + (off0 + (uint32_t)(4 * r) * (uint32_t)dst.stride)) = resize_pack<SAT>(out);
    }
}

// One level of a SMALL batch: a workgroup per 64 x 64 tile and frame (resize_tile).  With few frames the chip is empty and a launch
// lasts as long as its longest wave: four rows per thread behind one round of loads, against resize_band's sixteen rows behind
// four (B = 1 .. 16: 0.112 / 0.120 / 0.152 ms per call with this kernel, 0.139 / 0.145 / 0.175 with k_resize).
template <bool SAT>
__global__ __launch_bounds__(256) void k_resize_tiles(SrcImage src, uint8_t* __restrict__ pyr, size_t frame_stride, LevelDesc dst,
                                                      const int* __restrict__ q_sx0, const uint4* __restrict__ q_sel, const uint4* __restrict__ q_alpha,
                                                      const ResizeRow* __restrict__ rows)
{
    const int tiles_x = (dst.w + kResizeTileW - 1) / kResizeTileW, tiles_y = (dst.h + kResizeRows - 1) / kResizeRows;
    const int tile = xcd_remap(blockIdx.x, gridDim.x, blockIdx.y);
    if (tile >= tiles_x * tiles_y) return;
    resize_tile<SAT>(src.base + (size_t)blockIdx.y * src.frame_stride, src.stride, pyr + (size_t)blockIdx.y * frame_stride + dst.off, dst,
                     q_sx0, q_sel, q_alpha, rows, tile, threadIdx.x & 63, __builtin_amdgcn_readfirstlane(threadIdx.x >> 6));
}

// The upper pyramid levels are small and each depends on the one below: as launches of their own they are a chain of short,
// launch-latency-bound kernels.  Here ONE 1024-thread workgroup per frame walks the levels l_first .. n_levels-1 in turn (four
// tiles at a time -- resize_tile --, a workgroup barrier between levels: the level just written is read back by the same CU).
// SAT: one flag for the whole tail (any of its levels fails the host's coefficient-sum check -> the saturating form).
struct ResizeTables {
    const int* q_sx0[kMaxLevels]; const uint4* q_sel[kMaxLevels]; const uint4* q_alpha[kMaxLevels];
    const ResizeRow* rows[kMaxLevels];
};
template <bool SAT>
__global__ __launch_bounds__(1024) void k_resize_tail(uint8_t* __restrict__ pyr, size_t frame_stride, const LevelDesc* __restrict__ levels,
                                                            ResizeTables T, int l_first, int n_levels)
{
    const int frame = blockIdx.x;
    const int sub = __builtin_amdgcn_readfirstlane(threadIdx.x >> 8), wave = __builtin_amdgcn_readfirstlane((threadIdx.x >> 6) & 3);
    const int lane = threadIdx.x & 63;
    for (int l = l_first; l < n_levels; l++) {
        const LevelDesc D = levels[l], P = levels[l - 1];
        uint8_t* fp = pyr + (size_t)frame * frame_stride;
        const int tiles = ((D.w + kResizeTileW - 1) / kResizeTileW) * ((D.h + kResizeRows - 1) / kResizeRows);
        for (int t = sub; t < tiles; t += 4)
            resize_tile<SAT>(fp + P.off, P.stride, fp + D.off, D, T.q_sx0[l], T.q_sel[l], T.q_alpha[l], T.rows[l], t, lane, wave);
        __syncthreads();            // the level is complete (and visible to this CU) before it becomes the next one's source
    }
}

// ------------------------------------------------------------------------------------------------
// E2: FAST-9/16 on strips of cells -- orbx_fast_strips.inc
// ------------------------------------------------------------------------------------------------
#include "orbx_fast_strips.inc"

// ------------------------------------------------------------------------------------------------
// E3: DistributeOctTree.  One control wave per (frame, level), plus up to three helper waves (see OctJob).  The std::list of nodes is an index-linked list
// in LDS; a node's keys are a contiguous segment of a ping-pong key array (LDS when the level's candidates fit, HBM scratch
// otherwise).  The keys are placed ONCE, ordered by the cell of the level's bucket table they fall into (OctTabDesc, oct_place):
// down to the table's depth a node is a run of cells and divides by arithmetic on the cells' prefix sums (OctTab); only below it
// are keys partitioned, order-preserving, into the other buffer.  A pass of the reference's loops is a batch of up to 64
// DivideNode calls, a lane per node (see k_octree); std::sort is wave-parallel (orbx_introsort.h).
// ------------------------------------------------------------------------------------------------
#ifdef ORBX_OCT_TIMING      // cycle split of the (level 0, frame 0) wave (tools/oct_timing.py); never defined in the product build
__device__ unsigned long long d_oct_prof[11];
#endif
// A workgroup is W = 1, 2 or 4 waves (the host chooses per launch).  Wave 0 is the CONTROL wave: it runs octree_body and owns all the
// sequential state.  The other waves are helpers that run oct_helper_loop and nothing else.  Wave 0 hands them the parts of a pass
// whose items are independent -- the key partition of the nodes the whole wave takes one by one, the initial placement of the keys, the final
// selection -- as JOBS through this LDS record.  Workgroup barriers stand at exactly two points:
//   A  wave 0 has written the job (oct_post_job)    | the helpers wait here between jobs
//   B  every wave, wave 0 included, has done its share of the job
// The record is written by wave 0 only between B and the next A and read by the helpers only between A and B.  Everything else that
// was a barrier when the workgroup was one wave is a fence of the control wave alone (wave_mem_fence).
enum { kOctJobExit = 0, kOctJobPartition = 1, kOctJobPlace = 2, kOctJobSelect = 3 };
constexpr int kOctMaxJobs = 1 << 24;    // the helpers' loop bound; wave 0 stops posting one short of it, so that the EXIT job always fits
struct OctJob {
    int op, n, lds_keys, pad;
    int list[64];           // PARTITION: (batch lane << 16) | node id
    int cnt[4 * 64];        // PARTITION: the four child sizes of the node of batch lane l at cnt[4 l ..]
};
struct OctArgs {
    const LevelDesc* levels; const CellDesc* cells;
    const uint32_t* cand; size_t cand_frame_stride;
    const int* cell_count; int n_cells;
    uint32_t* scratch; size_t scratch_frame_stride;
    int pool, lds_keys_cap;
    uint32_t* sel; int sel_frame_stride;
    int* sel_count; int n_levels; int* status;
    uint8_t* node_scratch; size_t node_stride; int level_first;
    int small_max;          // a node of at most this many keys is partitioned by its lane, a larger one by the whole wave(s)
    const OctTabDesc* tabs; const uint16_t* maps;           // the levels' bucket tables (setup_geometry)
    int* prefix; size_t prefix_frame_stride;                // per frame and level: the prefix sums over the table's cells
};
struct OctLds {
    short* ulx; short* uly; short* brx; short* bry;
    int* beg; int* cnt;
    int* pidx; short* freelist; short* order;       // pidx indexes the push log (6 x pool entries: beyond 16 bits for large pools)
    short* plog;            // push log: the std::list order is the REVERSE of this array without its tombstones (-1)
    uint8_t* flg;           // bit0: bNoMore, bit1: keys live in buffer 1, bits 2-4: depth of a node of the bucket table, kOctDeep below it
};
// A node of depth d <= D (the level's table depth) is a run of 4^(D-d) cells of the bucket table: its `beg` field holds its FIRST CELL,
// its keys are kb[P[cell] .. P[cell + 4^(D-d)]), and its four children are four quarters of that run -- dividing it moves no key.
// A node of depth D is one cell; dividing it partitions its keys as before the table (ping-pong into the other buffer), and its
// children and theirs are DEEP nodes whose `beg` is a key offset.
constexpr int kOctDeep = 7;
struct OctTab {
    int D, n_ini, ncell, w_cell_inv, h_cell_inv;
    float hx;
    int* P;                 // prefix sums over the cells (global, L2-resident): ncell + 1 entries
    int* C;                 // placement only, overlaid on the node pool (which is empty then): counters / cursors per cell ...
    uint16_t* lmap;         // ... and, where they fit too (maps_lds), the level's two maps, staged from gmap
    const uint16_t* gmap;
    int bw, bh;             // entries of the x map and of the y map: the tree's width and height
    bool maps_lds;
    bool fits;              // the overlay fits the pool (the host chose D so; checked by the control wave)
};

// LDS_KEYS: both ping-pong key buffers live in LDS (the host sizes them for the largest level, so the choice is static and
// every key access is a ds_ instruction); otherwise they live in the L2-resident HBM scratch (global_ instructions).
// LDS_NODES: the node pool (boxes, key ranges, push log, the two sort arrays) lives in LDS, which holds about 2500 nodes; levels
// that ask for more features than that (e.g. 12000 features per frame) take the instantiation whose pool lives in an HBM /
// L2-resident scratch of its own -- the same code, global_ instead of ds_ instructions.
//
// One pass of the reference's loops is a BATCH of up to 64 independent DivideNode calls (the nodes of the list that can still
// be divided, resp. the next 64 entries of the sorted to-expand vector), one lane per node: the lanes count their node's keys
// per child (a node with many keys is counted and scattered by the whole wave instead), prefix sums over the lanes give every
// child its node slot, its place in the push log and in the next to-expand vector in exactly the order the sequential loop
// would have produced, and -- in the sorted phase -- the lane at which the running size reaches N (the reference breaks
// there: later lanes do not divide).
struct OctMem {
    OctLds S;
    SortNode* ex_new;       // the to-expand vector being appended to
    SortNode* ex_sorted;    // the sorted previous one (and the sort's scratch)
    uint32_t* kb;           // the two key buffers: kb[0 .. cap) and kb[cap .. 2 cap)
    int cap;
    OctTab T;
};

// carve the node pool and the key buffers of this (frame, level); every wave of the workgroup computes the same pointers
template <bool LDS_KEYS, bool LDS_NODES>
__device__ __forceinline__ OctMem oct_carve(const OctArgs& A, const LevelDesc& L, uint8_t* __restrict__ smem)
{
    const int pool = A.pool;
    OctMem M;
    OctLds& S = M.S;
    uint8_t* p;
    if constexpr (LDS_NODES) p = smem;
    else p = A.node_scratch + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * A.node_stride;
    M.ex_new = (SortNode*)p; p += sizeof(SortNode) * pool;
    M.ex_sorted = (SortNode*)p; p += sizeof(SortNode) * pool;
    S.beg = (int*)p; p += 4 * pool;
    S.cnt = (int*)p; p += 4 * pool;
    S.ulx = (short*)p; p += 2 * pool;  S.uly = (short*)p; p += 2 * pool;
    S.brx = (short*)p; p += 2 * pool;  S.bry = (short*)p; p += 2 * pool;
    S.pidx = (int*)p; p += 4 * pool;
    S.freelist = (short*)p; p += 2 * pool; S.order = (short*)p; p += 2 * pool;
    S.plog = (short*)p; p += 2 * kOctLogFactor * pool;
    S.flg = p; p += (pool + 15) & ~15;
    {
        const OctTabDesc td = A.tabs[A.level_first + blockIdx.x];
        OctTab& T = M.T;
        T.D = td.depth; T.n_ini = td.n_ini; T.ncell = td.n_ini << (2 * td.depth); T.w_cell_inv = td.w_cell_inv; T.h_cell_inv = td.h_cell_inv;
        T.bw = (L.w - kEdge + 3) - (kEdge - 3); T.bh = (L.h - kEdge + 3) - (kEdge - 3);
        T.hx = (float)T.bw / (float)td.n_ini;
        T.P = A.prefix + (size_t)blockIdx.y * A.prefix_frame_stride + td.prefix_off;
        T.C = (int*)M.ex_new;
        T.lmap = (uint16_t*)(T.C + T.ncell + 1);
        T.gmap = A.maps + td.map_off;
        T.maps_lds = td.maps_lds != 0;
        T.fits = td.depth >= 0 && td.depth <= kOctTabMaxDepth && td.n_ini >= 1 && T.bw >= 1 && T.bh >= 1 &&
                 (uint8_t*)(T.lmap + (T.maps_lds ? T.bw + T.bh : 0)) <= p;
    }
    if constexpr (LDS_KEYS) { M.kb = (uint32_t*)p; M.cap = A.lds_keys_cap; }
    else { M.kb = A.scratch + (size_t)blockIdx.y * A.scratch_frame_stride + 2 * (size_t)L.cand_off; M.cap = L.cand_cap; }
    return M;
}

// what DivideNode needs of the node of this lane
struct OctNodeBox { int ulx, uly, brx, bry, beg, cnt, src, midx, midy, in_off, out_off, dep, cell; };
__device__ __forceinline__ OctNodeBox oct_node_box(const OctLds& S, const OctTab& T, int cap, int id)
{
    OctNodeBox b = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, kOctDeep, 0};
    if (id >= 0) {
        b.ulx = S.ulx[id]; b.uly = S.uly[id]; b.brx = S.brx[id]; b.bry = S.bry[id];
        const int f = S.flg[id];
        b.beg = S.beg[id]; b.cnt = S.cnt[id]; b.src = (f >> 1) & 1; b.dep = (f >> 2) & 7;
        if (b.dep <= T.D) { b.cell = b.beg; b.beg = T.P[b.cell]; }         // a node of the table: its keys begin where its first cell does
    }
    const int halfX = (b.brx - b.ulx + 1) >> 1;     // ceil(float(w)/2), w >= 0
    const int halfY = (b.bry - b.uly + 1) >> 1;
    b.midx = b.ulx + halfX; b.midy = b.uly + halfY;
    b.in_off = (b.src ? cap : 0) + b.beg; b.out_off = (b.src ? 0 : cap) + b.beg;
    return b;
}

// The whole wave partitions the nodes of the lanes in `mb` (wave-uniform), one node at a time: ballot + prefix popcount, stable.
// Lane b holds its node's key ranges, key count and mid point; it receives the four child sizes.  The first 64 keys of the NEXT node
// are read before the current one is consumed (two nodes in flight: a node's ranges of the two buffers are its own, so the early
// read cannot meet another node's scatter).
__device__ __forceinline__ void oct_partition_nodes(uint32_t* __restrict__ kb, unsigned long long mb, const int lane, const unsigned long long lt,
                                                    const int in_off, const int out_off, const int cnt, const int midx, const int midy,
                                                    int& c0, int& c1, int& c2, int& c3)
{
    if (mb == 0ull) return;
    int b = __builtin_ctzll(mb);
    int bin = __builtin_amdgcn_readlane(in_off, b), bcnt = __builtin_amdgcn_readlane(cnt, b);
    uint32_t e = (bcnt <= 64 && lane < bcnt) ? kb[bin + lane] : 0u;
    for (;;) {
        const int bout = __builtin_amdgcn_readlane(out_off, b);
        const int bmx = __builtin_amdgcn_readlane(midx, b), bmy = __builtin_amdgcn_readlane(midy, b);
        mb &= mb - 1ull;
        int nb = b, nbin = 0, nbcnt = 0;
        uint32_t e_next = 0;
        if (mb != 0ull) {
            nb = __builtin_ctzll(mb);
            nbin = __builtin_amdgcn_readlane(in_off, nb); nbcnt = __builtin_amdgcn_readlane(cnt, nb);
            if (nbcnt <= 64 && lane < nbcnt) e_next = kb[nbin + lane];
        }
        int s0 = 0, s1 = 0, s2 = 0, s3 = 0;
        if (bcnt <= 64) {
            int cls = -1;
            if (lane < bcnt) cls = ((int)key_x(e) >= bmx ? 1 : 0) + ((int)key_y(e) >= bmy ? 2 : 0);
            const unsigned long long m0 = __ballot(cls == 0), m1 = __ballot(cls == 1), m2 = __ballot(cls == 2), m3 = __ballot(cls == 3);
            s0 = __popcll(m0); s1 = __popcll(m1); s2 = __popcll(m2); s3 = __popcll(m3);
            const unsigned long long mm = (cls == 0) ? m0 : (cls == 1) ? m1 : (cls == 2) ? m2 : m3;
            const int basec = (cls == 0) ? 0 : (cls == 1) ? s0 : (cls == 2) ? s0 + s1 : s0 + s1 + s2;
            if (cls >= 0) kb[bout + basec + __popcll(mm & lt)] = e;
        } else {
            // pass 1: child sizes (four chunks of 64 keys in flight)
            for (int k0 = 0; k0 < bcnt; k0 += 256) {
                uint32_t ev[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { const int k = k0 + 64 * u + lane; ev[u] = (k < bcnt) ? kb[bin + k] : 0u; }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = k0 + 64 * u + lane;
                    const int cls = (k < bcnt) ? ((int)key_x(ev[u]) >= bmx ? 1 : 0) + ((int)key_y(ev[u]) >= bmy ? 2 : 0) : -1;
                    s0 += __popcll(__ballot(cls == 0)); s1 += __popcll(__ballot(cls == 1));
                    s2 += __popcll(__ballot(cls == 2)); s3 += __popcll(__ballot(cls == 3));
                }
            }
            // pass 2: stable scatter into the other buffer
            int w0 = bout, w1 = bout + s0, w2 = w1 + s1, w3 = w2 + s2;
            for (int k0 = 0; k0 < bcnt; k0 += 256) {
                uint32_t ev[4];
#pragma unroll
                for (int u = 0; u < 4; u++) { const int k = k0 + 64 * u + lane; ev[u] = (k < bcnt) ? kb[bin + k] : 0u; }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int k = k0 + 64 * u + lane;
                    const int cls = (k < bcnt) ? ((int)key_x(ev[u]) >= bmx ? 1 : 0) + ((int)key_y(ev[u]) >= bmy ? 2 : 0) : -1;
                    const unsigned long long m0 = __ballot(cls == 0), m1 = __ballot(cls == 1), m2 = __ballot(cls == 2), m3 = __ballot(cls == 3);
                    const unsigned long long mm = (cls == 0) ? m0 : (cls == 1) ? m1 : (cls == 2) ? m2 : m3;
                    const int wc = (cls == 0) ? w0 : (cls == 1) ? w1 : (cls == 2) ? w2 : w3;
                    if (cls >= 0) kb[wc + __popcll(mm & lt)] = ev[u];
                    w0 += __popcll(m0); w1 += __popcll(m1); w2 += __popcll(m2); w3 += __popcll(m3);
                }
            }
        }
        if (lane == b) { c0 = s0; c1 = s1; c2 = s2; c3 = s3; }
        if (mb == 0ull) break;
        b = nb; bin = nbin; bcnt = nbcnt; e = e_next;
    }
}

// ---- a wave's share of a job (wave w of W; wave 0 calls these too)
// PARTITION: list entries w, w + W, ...; lane l loads the box of entry l, exactly as the control wave's lane did
__device__ __forceinline__ void oct_job_partition(const OctMem& M, OctJob* __restrict__ J, const int w, const int W, const int lane, const unsigned long long lt)
{
    const int n = min(__builtin_amdgcn_readfirstlane(J->n), 64);
    int id = -1, bl = 0;
    if (lane < n) { const int v = J->list[lane]; id = v & 0xFFFF; bl = v >> 16; }
    const OctNodeBox nb = oct_node_box(M.S, M.T, M.cap, id);
    const unsigned long long all = (n >= 64) ? ~0ull : (1ull << n) - 1ull;
    const unsigned long long stripe = ((W == 4) ? 0x1111111111111111ull : (W == 2) ? 0x5555555555555555ull : ~0ull) << w;
    const unsigned long long mine = all & stripe;
    int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
    oct_partition_nodes(M.kb, mine, lane, lt, nb.in_off, nb.out_off, nb.cnt, nb.midx, nb.midy, c0, c1, c2, c3);
    if ((mine >> lane) & 1ull) { int* o = J->cnt + 4 * (bl & 63); o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3; }
}

// the cell of the bucket table a key falls into: its root, then the quadrant at every depth, all in the level's two maps
template <class Map>
__device__ __forceinline__ int oct_cell_of(const OctTab& T, const Map xm, const Map ym, const uint32_t e)
{
    return (int)xm[min((int)key_x(e), T.bw - 1)] | (int)ym[min((int)key_y(e), T.bh - 1)];
}

// where a key stands in vToDistributeKeys order (FAST cell row-major, row-major inside a cell): the order that decides between
// keys of equal response
__device__ __forceinline__ unsigned long long oct_cand_rank(const OctTab& T, const uint32_t e)
{
    const uint32_t x = key_x(e), y = key_y(e);
    // FAST cell = (coordinate - 3) / pitch, the division as a multiplication (the host checked it for every coordinate of the level)
    const uint32_t cj = ((x >= 3u ? x - 3u : 0u) * (uint32_t)T.w_cell_inv) >> 20, ci = ((y >= 3u ? y - 3u : 0u) * (uint32_t)T.h_cell_inv) >> 20;
    return ((unsigned long long)((ci << 12) | cj) << 24) | (unsigned long long)((y << 12) | x);
}
// one number to maximise: the response first, then the EARLIER candidate (rank below 2^48)
__device__ __forceinline__ unsigned long long oct_select_score(const OctTab& T, const uint32_t e)
{
    return ((unsigned long long)key_resp(e) << 48) | (0xFFFFFFFFFFFFull - oct_cand_rank(T, e));
}

// PLACE: every candidate of the level goes ONCE to its cell's run of key buffer 0 (counting sort by cell code, not stable), read
// straight from the FAST cells' slots; waves take blocks of 64 FAST cells w, w + W, ..., a lane per FAST cell.  `step` separates
// the phases: a workgroup barrier when the helpers share the job, the control wave's own fence when it works alone.
template <class Step>
__device__ __forceinline__ void oct_place(const OctArgs& A, const LevelDesc& L, const OctMem& M, const int w, const int W, const int lane, Step step)
{
    const OctTab& T = M.T;
    const uint32_t* fc = A.cand + (size_t)blockIdx.y * A.cand_frame_stride;
    const int* cc = A.cell_count + (size_t)blockIdx.y * A.n_cells;
    for (int i = 64 * w + lane; i <= T.ncell; i += 64 * W) T.C[i] = 0;
    if (T.maps_lds) for (int i = 64 * w + lane; i < T.bw + T.bh; i += 64 * W) T.lmap[i] = T.gmap[i];
    step();
    const int nblk = (L.cell_count + 63) >> 6;
    auto pass = [&](const auto xm, const auto ym, const bool scatter) {
        for (int blk = w; blk < nblk; blk += W) {
            const int ci = 64 * blk + lane;
            int n = 0, slot_off = 0;
            if (ci < L.cell_count) { n = cc[L.cell_begin + ci]; slot_off = A.cells[L.cell_begin + ci].slot_off; }
            for (int k = 0; __ballot(k < n) != 0ull; k += 8) {
                uint32_t e[8];
#pragma unroll
                for (int u = 0; u < 8; u++) e[u] = (k + u < n) ? fc[slot_off + k + u] : 0u;
#pragma unroll
                for (int u = 0; u < 8; u++) {
                    if (k + u < n) {
                        const int cell = min(oct_cell_of(T, xm, ym, e[u]), T.ncell - 1);
                        if (!scatter) atomicAdd(&T.C[cell], 1);
                        else { const int pos = atomicAdd(&T.C[cell], 1); if ((unsigned)pos < (unsigned)M.cap) M.kb[pos] = e[u]; }
                    }
                }
            }
        }
    };
    // (one call per home of the maps: each is compiled with its own addressing)
    if (T.maps_lds) pass((const uint16_t*)T.lmap, (const uint16_t*)T.lmap + T.bw, false); else pass(T.gmap, T.gmap + T.bw, false);
    step();
    if (w == 0) {       // exclusive prefix over the cells: P for the divides, C as the scatter's cursors; entry ncell is the total
        int run = 0;
        for (int i0 = 0; i0 <= T.ncell; i0 += 64) {
            const int i = i0 + lane;
            const int v = (i < T.ncell) ? T.C[i] : 0;
            const int incl = wave_incl_scan(v);
            if (i <= T.ncell) { T.P[i] = run + incl - v; T.C[i] = run + incl - v; }
            run += __builtin_amdgcn_readlane(incl, 63);
        }
    }
    step();
    if (T.maps_lds) pass((const uint16_t*)T.lmap, (const uint16_t*)T.lmap + T.bw, true); else pass(T.gmap, T.gmap + T.bw, true);
}

// SELECT: the best-response key of every node (:758-776); blocks of 64 nodes w, w + W, ..., a lane per node.  The reference keeps the
// FIRST key of maximal response in vKeys order; a node's keys no longer stand in that order, so ties go to the key that comes first
// in candidate order (oct_cand_rank).
__device__ __forceinline__ void oct_select_blocks(const OctMem& M, uint32_t* __restrict__ out, const int n_out, const int w, const int W, const int lane)
{
    const OctLds& S = M.S;
    for (int k0 = 64 * w; k0 < n_out; k0 += 64 * W) {
        const int k = k0 + lane;
        int off = 0, cnt = 0;
        if (k < n_out) { const OctNodeBox nb = oct_node_box(S, M.T, M.cap, S.order[k]); off = nb.in_off; cnt = nb.cnt; }
        uint32_t best = 0;
        unsigned long long best_score = 0ull;
        for (int i = 0; __ballot(i < cnt) != 0ull; i += 4) {
            uint32_t e[4];
#pragma unroll
            for (int u = 0; u < 4; u++) e[u] = (i + u < cnt) ? M.kb[off + i + u] : 0u;
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const unsigned long long s = oct_select_score(M.T, e[u]);
                if (i + u < cnt && (i + u == 0 || s > best_score)) { best = e[u]; best_score = s; }
            }
        }
        if (k < n_out) out[k] = best;
    }
}

template <bool LDS_KEYS, bool LDS_NODES>
__device__ __forceinline__ void oct_do_job(const int op, const OctArgs& A, const LevelDesc& L, uint8_t* __restrict__ smem, OctJob* __restrict__ J,
                                           const int w, const int W, const int lane, const unsigned long long lt)
{
    const OctMem M = oct_carve<LDS_KEYS, LDS_NODES>(A, L, smem);
    if (op == kOctJobPartition) oct_job_partition(M, J, w, W, lane, lt);
    else if (op == kOctJobPlace) oct_place(A, L, M, w, W, lane, [] { __syncthreads(); });
    else if (op == kOctJobSelect)
        oct_select_blocks(M, A.sel + (size_t)blockIdx.y * A.sel_frame_stride + L.sel_off, min(__builtin_amdgcn_readfirstlane(J->n), L.sel_cap), w, W, lane);
}

// The helpers' whole life: wait at A, leave on EXIT, do the share, meet at B.  KEYS: 0 scratch, 1 LDS, 2 as the job says (k_octree_dyn:
// the control wave chose the body).  The loop bound is a backstop only: wave 0 posts fewer than kOctMaxJobs jobs, EXIT included.
template <int KEYS, bool LDS_NODES>
__device__ __forceinline__ void oct_helper_loop(const OctArgs& A, uint8_t* __restrict__ smem, OctJob* __restrict__ J, const int w, const int W)
{
    const LevelDesc L = A.levels[A.level_first + blockIdx.x];
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int j = 0; j < kOctMaxJobs; j++) {
        __syncthreads();                                    // A
        const int op = __builtin_amdgcn_readfirstlane(J->op);
        if (op == kOctJobExit) break;
        if constexpr (KEYS == 2) {
            if (__builtin_amdgcn_readfirstlane(J->lds_keys) != 0) oct_do_job<true, true>(op, A, L, smem, J, w, W, lane, lt);
            else oct_do_job<false, true>(op, A, L, smem, J, w, W, lane, lt);
        } else {
            oct_do_job<KEYS == 1, LDS_NODES>(op, A, L, smem, J, w, W, lane, lt);
        }
        __syncthreads();                                    // B
    }
}

// wave 0 posts a job: barrier A.  (Wave 0 calls this in wave-uniform control flow only.)
__device__ __forceinline__ void oct_post_job(OctJob* __restrict__ J, const int op, const int n, const int lds_keys, const int lane, int& jobs)
{
    if (lane == 0) { J->op = op; J->n = n; J->lds_keys = lds_keys; }
    jobs++;
    __syncthreads();                                        // A
}

// The control wave.  Returns on every exit path; the caller posts the EXIT job.
template <bool LDS_KEYS, bool LDS_NODES>
__device__ __forceinline__ void octree_body(const OctArgs& A, uint8_t* __restrict__ smem, int* __restrict__ s_sort_stack, OctJob* __restrict__ J, const int W, int& jobs)
{
    static_assert(LDS_NODES || !LDS_KEYS, "a pool too large for LDS leaves no room for LDS keys");
    const LevelDesc* __restrict__ levels = A.levels;
    const int pool = A.pool, n_levels = A.n_levels;
    int* __restrict__ status = A.status;
    const int level = A.level_first + blockIdx.x, frame = blockIdx.y;     // (a launch covers the levels level_first ..: see enqueue())
    const int lane = threadIdx.x;
    const LevelDesc L = levels[level];
    const int N = L.nfeat;
    const unsigned long long lt = (1ull << lane) - 1ull;
    // this wave's own ordering of what its lanes write and other lanes read: never a workgroup barrier (the helpers are not here)
    auto fence = [] { wave_mem_fence<!(LDS_KEYS && LDS_NODES)>(); };
    auto can_post = [&] { return W > 1 && jobs < kOctMaxJobs - 1; };
#ifdef ORBX_OCT_TIMING
    long long tq[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    const bool timed = level == 0 && frame == 0 && lane == 0;
    long long t_prev = clock64();
    const long long t_kernel0 = t_prev;
    int n_div = 0;
#define ORBX_OTICK(k) if (timed) { const long long t_now = clock64(); tq[k] += t_now - t_prev; t_prev = t_now; }
#else
#define ORBX_OTICK(k)
#endif

    const OctMem M = oct_carve<LDS_KEYS, LDS_NODES>(A, L, smem);
    const OctLds& S = M.S;
    SortNode* const ex_new = M.ex_new;
    SortNode* const ex_sorted = M.ex_sorted;
    uint32_t* const kb = M.kb;
    const int cap = M.cap;

    int* out_count = A.sel_count + (size_t)frame * n_levels + level;
    uint32_t* out = A.sel + (size_t)frame * A.sel_frame_stride + L.sel_off;

    const int width = (L.w - kEdge + 3) - (kEdge - 3), height = (L.h - kEdge + 3) - (kEdge - 3);
    const int nIni = (height > 0) ? (int)roundf((float)width / (float)height) : 0;      // :559
    if (nIni <= 0) {
        if (lane == 0) *out_count = 0;
        return;
    }
    const OctTab& T = M.T;
    if (nIni > pool / 2 || nIni != T.n_ini || !T.fits) {        // (the host builds the table for these very roots, inside the pool's bytes)
        if (lane == 0) { atomicExch(status + frame, ORBX_ERR_INTERNAL); *out_count = 0; }
        return;
    }

    // ---- place the level's candidates: every key goes once to its cell of the bucket table (oct_place); the node pool is still
    // empty and lends the placement its counters
    if (can_post()) {
        oct_post_job(J, kOctJobPlace, 0, LDS_KEYS ? 1 : 0, lane, jobs);
        oct_place(A, L, M, 0, W, lane, [] { __syncthreads(); });
        ORBX_OTICK(0)
        __syncthreads();                                    // B
        ORBX_OTICK(7)
    } else {
        oct_place(A, L, M, 0, 1, lane, fence);
        wave_mem_fence<true>();         // (the prefix sums are in global memory whatever the home of the keys)
    }
    const int total = T.C[T.ncell];
    if (total > cap) {
        if (lane == 0) { atomicExch(status + frame, ORBX_ERR_INTERNAL); *out_count = 0; }
        return;
    }
    ORBX_OTICK(0)
    if (total == 0) {
        if (lane == 0) *out_count = 0;
        return;
    }
    fence();        // (the counters are read: the pool may be written)

    // ---- the list.  std::list<ExtractorNode> with push_front / erase only needs an append-only push log: iterating the
    // list from begin() is walking the log backwards, erase() leaves a tombstone, and nodes pushed while a pass is running
    // sit behind its start index exactly like nodes pushed in front of a running list iterator.
    const int plog_cap = kOctLogFactor * pool;
    int np = 0, size = 0, nfree = pool, n_ex = 0;
    for (int i = lane; i < pool; i += 64) S.freelist[i] = (short)(pool - 1 - i);
    fence();
    bool overflow = false;
    auto compact = [&]() {          // drop tombstones, order preserved (wave-parallel, in place)
        int w = 0;
        for (int i0 = 0; i0 < np; i0 += 64) {
            const int i = i0 + lane;
            const int id = (i < np) ? (int)S.plog[i] : -1;
            const unsigned long long m = __ballot(id >= 0);
            if (id >= 0) { const int pos = w + __popcll(m & lt); S.plog[pos] = (short)id; S.pidx[id] = pos; }
            w += __popcll(m);
        }
        np = w;
        fence();
    };

    // ---- root nodes (:564-586): nIni vertical strips of width hX; root s is the cells [s << 2D, (s + 1) << 2D) of the table
    const float hX = T.hx;
    for (int s = 0; s < nIni; s++) {
        const int cell = s << (2 * T.D);
        const int cnt = __builtin_amdgcn_readfirstlane(T.P[cell + (1 << (2 * T.D))] - T.P[cell]);
        int id = -1;
        if (cnt > 0) {      // empty roots are erased (:595-596)
            id = S.freelist[--nfree];
            if (lane == 0) {
                S.ulx[id] = (short)(int)(hX * (float)s);       S.uly[id] = 0;
                S.brx[id] = (short)(int)(hX * (float)(s + 1)); S.bry[id] = (short)height;
                S.beg[id] = cell; S.cnt[id] = cnt;
                S.flg[id] = (uint8_t)(cnt == 1 ? 1 : 0);        // depth 0, keys in buffer 0
            }
        }
        if (lane == 0) S.order[s] = (short)id;
    }
    fence();
    // the reference push_back()s the roots in strip order; in push-log terms the first strip is pushed last
    for (int s = nIni - 1; s >= 0; s--) {
        const int id = S.order[s];
        if (id >= 0) { if (lane == 0) { S.plog[np] = (short)id; S.pidx[id] = np; } np++; size++; }
    }
    fence();
    ORBX_OTICK(1)

    // One batch of DivideNode calls (:480-536 and the loop bodies :610-676 / :706-750): lane l divides node `id` (or none: -1);
    // lanes are in processing order.  sorted_phase: stop after the lane whose divide brings the list to N nodes; returns
    // whether that happened.
    auto divide_batch = [&](const int id, const bool sorted_phase, int& n_to_expand) -> bool {
        const bool act = id >= 0;
        const OctNodeBox nb = oct_node_box(S, T, cap, id);
        const int ulx = nb.ulx, uly = nb.uly, brx = nb.brx, bry = nb.bry, beg = nb.beg, cnt = nb.cnt, src = nb.src;
        const int midx = nb.midx, midy = nb.midy, in_off = nb.in_off, out_off = nb.out_off;
        // A node above the table's depth divides by lookup: its children are the four quarters of its run of cells, their sizes
        // differences of the prefix sums; no key is read or moved.
        const bool tab = act && nb.dep < T.D;
        const int quarter = tab ? 1 << (2 * (T.D - nb.dep - 1)) : 0;
        int c0 = 0, c1 = 0, c2 = 0, c3 = 0;
        if (tab) {
            const int p1 = T.P[nb.cell + quarter], p2 = T.P[nb.cell + 2 * quarter], p3 = T.P[nb.cell + 3 * quarter], p4 = T.P[nb.cell + 4 * quarter];
            c0 = p1 - beg; c1 = p2 - p1; c2 = p3 - p2; c3 = p4 - p3;
        }
        // The others (a cell of the table, or a node below it) partition their keys.  Scattering a node's keys into the other
        // buffer is harmless when the node ends up not being divided (its range of the other buffer is dead space of its own),
        // so counting and scattering do not wait for the cut.
        const bool part = act && !tab;
        const unsigned long long m_part = __ballot(part);
        const int small_max = (__popcll(m_part) <= 6) ? 0 : A.small_max;      // a handful of nodes: the whole wave takes them one by one
        const bool small = part && cnt <= small_max;
        // the nodes the whole wave takes one by one: with helpers, and more than one such node, they are a PARTITION job
        const unsigned long long m_big = __ballot(part && !small);
        const bool job = __popcll(m_big) > 1 && can_post();
        if (job) {
            if (part && !small) J->list[__popcll(m_big & lt)] = (lane << 16) | id;
            oct_post_job(J, kOctJobPartition, __popcll(m_big), LDS_KEYS ? 1 : 0, lane, jobs);
        }
        if (__ballot(small) != 0ull) {
            // a lane per node: count, then stable scatter
            for (int k = 0; __ballot(small && k < cnt) != 0ull; k += 4) {
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (small && k + u < cnt) {
                        const uint32_t e = kb[in_off + k + u];
                        const int cls = ((int)key_x(e) >= midx ? 1 : 0) + ((int)key_y(e) >= midy ? 2 : 0);
                        c0 += cls == 0; c1 += cls == 1; c2 += cls == 2; c3 += cls == 3;
                    }
                }
            }
            int w0 = out_off, w1 = out_off + c0, w2 = w1 + c1, w3 = w2 + c2;
            for (int k = 0; __ballot(small && k < cnt) != 0ull; k += 4) {
                uint32_t e[4];
#pragma unroll
                for (int u = 0; u < 4; u++) e[u] = (small && k + u < cnt) ? kb[in_off + k + u] : 0u;
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    if (small && k + u < cnt) {
                        const bool r = (int)key_x(e[u]) >= midx, d = (int)key_y(e[u]) >= midy;
                        const int pos = d ? (r ? w3 : w2) : (r ? w1 : w0);
                        kb[pos] = e[u];
                        w0 += (!d && !r); w1 += (!d && r); w2 += (d && !r); w3 += (d && r);
                    }
                }
            }
        }
        if (job) {
            // (the lane-per-node loops above ran beside the helpers' share)
            oct_job_partition(M, J, 0, W, lane, lt);
            ORBX_OTICK(2)
            __syncthreads();                                // B
            ORBX_OTICK(7)
            if (part && !small) { const int* o = J->cnt + 4 * lane; c0 = o[0]; c1 = o[1]; c2 = o[2]; c3 = o[3]; }
        } else {
            oct_partition_nodes(kb, m_big, lane, lt, in_off, out_off, cnt, midx, midy, c0, c1, c2, c3);
        }
        ORBX_OTICK(2)

        // ---- bookkeeping, a lane per node
        bool keep = act, reached = false;
        if (sorted_phase) {
            const int grow = act ? (c0 > 0) + (c1 > 0) + (c2 > 0) + (c3 > 0) - 1 : 0;
            const int incl_g = wave_incl_scan(grow);
            const unsigned long long hit = __ballot(act && size + incl_g >= N);     // `if ((int)lNodes.size() >= N) break;` after this divide
            if (hit != 0ull) { reached = true; keep = act && lane <= __builtin_ctzll(hit); }
        }
        // The children take their node slots before the parents return theirs.  Normally the free list holds enough for the whole
        // batch; when it does not (the pool is only N + 16 nodes, as for the sequential loop), the batch goes in rounds: the longest
        // prefix of the remaining lanes whose children fit.
        for (unsigned long long rem = __ballot(keep); rem != 0ull;) {
            const bool in = (rem >> lane) & 1ull;
            const int ne = in ? (c0 > 0) + (c1 > 0) + (c2 > 0) + (c3 > 0) : 0;
            const int nx = in ? (c0 > 1) + (c1 > 1) + (c2 > 1) + (c3 > 1) : 0;
            const int incl_e = wave_incl_scan(ne), incl_x = wave_incl_scan(nx), incl_a = wave_incl_scan(in ? 1 : 0);
            const bool take = in && incl_e <= nfree;
            const unsigned long long m_take = __ballot(take);
            if (m_take == 0ull) { overflow = true; return true; }
            const int last = 63 - __builtin_clzll(m_take);
            const int tot_e = __builtin_amdgcn_readlane(incl_e, last), tot_x = __builtin_amdgcn_readlane(incl_x, last), tot_a = __builtin_amdgcn_readlane(incl_a, last);
            if (np + tot_e > plog_cap || n_ex + tot_x > pool) { overflow = true; return true; }
            if (take) {
                int slot = np + incl_e - ne, fl = nfree - 1 - (incl_e - ne), xs = n_ex + incl_x - nx, cb = beg;
#pragma unroll
                for (int c = 0; c < 4; c++) {
                    const int cn = (c == 0) ? c0 : (c == 1) ? c1 : (c == 2) ? c2 : c3;
                    if (cn > 0) {
                        const int ch = S.freelist[fl--];
                        const int ux = (c & 1) ? midx : ulx, uy = (c & 2) ? midy : uly;
                        S.ulx[ch] = (short)ux; S.uly[ch] = (short)uy;
                        S.brx[ch] = (short)((c & 1) ? brx : midx); S.bry[ch] = (short)((c & 2) ? bry : midy);
                        // a child by lookup is a quarter of its parent's cells, in the same buffer; a partitioned one is a key range of the other
                        S.beg[ch] = tab ? nb.cell + c * quarter : cb; S.cnt[ch] = cn;
                        S.flg[ch] = (uint8_t)((tab ? ((nb.dep + 1) << 2) | (src << 1) : (kOctDeep << 2) | ((src ^ 1) << 1)) | (cn == 1 ? 1 : 0));
                        S.plog[slot] = (short)ch; S.pidx[ch] = slot; slot++;            // push_front, children n1..n4 in order
                        if (cn > 1) { SortNode sn; sn.count = cn; sn.ulx = ux; sn.node = ch; ex_new[xs++] = sn; }
                        cb += cn;
                    }
                }
                S.plog[S.pidx[id]] = -1;        // erase the parent
            }
            fence();                    // the free-list reads above come before the writes below
            np += tot_e; size += tot_e - tot_a; nfree -= tot_e;
            if (take) S.freelist[nfree + incl_a - 1] = (short)id;
            nfree += tot_a;
            n_to_expand += tot_x; n_ex += tot_x;
#ifdef ORBX_OCT_TIMING
            n_div += tot_a;
#endif
            rem &= ~m_take;
            fence();        // key scatter and node records visible before the next round / batch reads them
        }
        ORBX_OTICK(3)
        return reached;
    };

    bool finish = false;
    int guard = 0;
    while (!finish && !overflow && guard++ < 64) {
        const int prev_size = size;
        int n_to_expand = 0;
        n_ex = 0;
        compact();
        const int np0 = np;                 // children pushed by this pass land behind the pass
        for (int b0 = 0; b0 < np0 && !overflow; b0 += 64) {
            const int idx = np0 - 1 - (b0 + lane);
            int id = -1;
            if (idx >= 0) { const int cur = S.plog[idx]; if (cur >= 0 && !(S.flg[cur] & 1)) id = cur; }
            if (__ballot(id >= 0) != 0ull) divide_batch(id, false, n_to_expand);
        }
        if (size >= N || size == prev_size) {
            finish = true;
        } else if (size + n_to_expand * 3 > N) {
            int guard2 = 0;
            while (!finish && !overflow && guard2++ < 4096) {
                const int prev_size2 = size;
                compact();
                const int n_prev = min(n_ex, pool);
                ORBX_OTICK(4)
                wave_sort_nodes<!LDS_NODES>(ex_new, ex_sorted, n_prev, s_sort_stack, S.order);     // std::sort(..., compareNodes) (:700)
                ORBX_OTICK(5)
                n_ex = 0;
                int dummy = 0;
                for (int b0 = 0; b0 < n_prev && !overflow; b0 += 64) {          // for (j = size - 1; j >= 0; j--)
                    const int j = n_prev - 1 - (b0 + lane);
                    const int id = (j >= 0) ? ex_sorted[j].node : -1;
                    if (divide_batch(id, true, dummy)) break;
                }
                if (size >= N || size == prev_size2) finish = true;
            }
        }
    }
    if (overflow) {
        if (lane == 0) { atomicExch(status + frame, ORBX_ERR_INTERNAL); *out_count = 0; }
        return;
    }
    ORBX_OTICK(4)

    // ---- final list order, then the best-response key of every node, first wins ties (:758-776)
    compact();
    for (int k = lane; k < np && k < pool; k += 64) S.order[k] = S.plog[np - 1 - k];
    fence();
    const int n_out = min(size, L.sel_cap);
    if (n_out > 64 && can_post()) {
        oct_post_job(J, kOctJobSelect, n_out, LDS_KEYS ? 1 : 0, lane, jobs);
        oct_select_blocks(M, out, n_out, 0, W, lane);
        ORBX_OTICK(6)
        __syncthreads();                                    // B
        ORBX_OTICK(7)
    } else {
        oct_select_blocks(M, out, n_out, 0, 1, lane);
    }
    if (lane == 0) {
        *out_count = n_out;
        if (size > L.sel_cap) atomicExch(status + frame, ORBX_ERR_INTERNAL);
    }
    ORBX_OTICK(6)
#ifdef ORBX_OCT_TIMING
    if (timed) {
        for (int i = 0; i < 7; i++) d_oct_prof[i] = (unsigned long long)tq[i];
        d_oct_prof[10] = (unsigned long long)tq[7];         // waiting at the job barriers
        d_oct_prof[7] = (unsigned long long)(clock64() - t_kernel0);
        d_oct_prof[8] = (unsigned long long)total; d_oct_prof[9] = (unsigned long long)n_div;
    }
#endif
}

// Launched with W x 64 threads.  Wave 0 runs the body and then posts EXIT -- at ONE place, whichever way the body returned; the other
// waves run the helpers' loop.  With W = 1 no job is ever posted and no workgroup barrier is executed.
template <bool LDS_KEYS, bool LDS_NODES = true>
__global__ __launch_bounds__(256) void k_octree(const LevelDesc* __restrict__ levels, const CellDesc* __restrict__ cells,
    const uint32_t* __restrict__ cand, size_t cand_frame_stride, const int* __restrict__ cell_count, int n_cells,
    uint32_t* __restrict__ scratch, size_t scratch_frame_stride, int pool, int lds_keys_cap,
    uint32_t* __restrict__ sel, int sel_frame_stride, int* __restrict__ sel_count, int n_levels, int* __restrict__ status,
    uint8_t* __restrict__ node_scratch, size_t node_stride, int level_first, int small_max,
    const OctTabDesc* __restrict__ tabs, const uint16_t* __restrict__ maps, int* __restrict__ prefix, size_t prefix_frame_stride)
{
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ int s_sort_stack[3 * kIntrosortStack];       // the sort's explicit stack (in LDS, not in private scratch)
    __shared__ OctJob s_job;
    const OctArgs A = {levels, cells, cand, cand_frame_stride, cell_count, n_cells, scratch, scratch_frame_stride, pool, lds_keys_cap,
                       sel, sel_frame_stride, sel_count, n_levels, status, node_scratch, node_stride, level_first, small_max,
                       tabs, maps, prefix, prefix_frame_stride};
    const int W = (int)(blockDim.x >> 6);                                   // 1, 2 or 4 waves (the host's choice per launch)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave != 0) { oct_helper_loop<LDS_KEYS ? 1 : 0, LDS_NODES>(A, smem, &s_job, wave, W); return; }
    int jobs = 0;
    octree_body<LDS_KEYS, LDS_NODES>(A, smem, s_sort_stack, &s_job, W, jobs);
    if (W > 1) oct_post_job(&s_job, kOctJobExit, 0, 0, (int)threadIdx.x, jobs);
}

// Small batches (a single frame: the reference's own use) are bound by the latency of the level-0 wave, and a level's key buffers are
// SIZED for the 3x3-NMS worst case (a quarter of the pixels: 614 KB for two buffers at 640 x 480) while a real level holds a few
// thousand candidates.  This kernel counts the level's candidates first and takes the keys-in-LDS body when they fit the LDS it was
// given (no L2 round trip per key-partition step: 0.079 -> 0.062 ms for the octree of one 320 x 200 frame), the scratch body otherwise;
// both bodies are compiled in, each with its own static addressing (no flat accesses).  The control wave alone counts and chooses;
// every job tells the helpers which key home it is about.
__global__ __launch_bounds__(256) void k_octree_dyn(const LevelDesc* __restrict__ levels, const CellDesc* __restrict__ cells,
    const uint32_t* __restrict__ cand, size_t cand_frame_stride, const int* __restrict__ cell_count, int n_cells,
    uint32_t* __restrict__ scratch, size_t scratch_frame_stride, int pool, int lds_keys_cap,
    uint32_t* __restrict__ sel, int sel_frame_stride, int* __restrict__ sel_count, int n_levels, int* __restrict__ status,
    uint8_t* __restrict__ node_scratch, size_t node_stride, int level_first, int small_max,
    const OctTabDesc* __restrict__ tabs, const uint16_t* __restrict__ maps, int* __restrict__ prefix, size_t prefix_frame_stride)
{
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ int s_sort_stack[3 * kIntrosortStack];
    __shared__ OctJob s_job;
    const OctArgs A = {levels, cells, cand, cand_frame_stride, cell_count, n_cells, scratch, scratch_frame_stride, pool, lds_keys_cap,
                       sel, sel_frame_stride, sel_count, n_levels, status, node_scratch, node_stride, level_first, small_max,
                       tabs, maps, prefix, prefix_frame_stride};
    const int W = (int)(blockDim.x >> 6);                                   // 1, 2 or 4 waves (the host's choice per launch)
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (wave != 0) { oct_helper_loop<2, true>(A, smem, &s_job, wave, W); return; }
    const LevelDesc L = levels[level_first + blockIdx.x];
    const int* cc = cell_count + (size_t)blockIdx.y * n_cells + L.cell_begin;
    int total = 0;
    for (int ci = threadIdx.x; ci < L.cell_count; ci += 64) total += cc[ci];
    for (int o = 32; o > 0; o >>= 1) total += __shfl_xor(total, o);
    total = __builtin_amdgcn_readfirstlane(total);
    int jobs = 0;
    if (total <= lds_keys_cap) octree_body<true, true>(A, smem, s_sort_stack, &s_job, W, jobs);
    else octree_body<false, true>(A, smem, s_sort_stack, &s_job, W, jobs);
    if (W > 1) oct_post_job(&s_job, kOctJobExit, 0, 0, (int)threadIdx.x, jobs);
}

// test hook: wave_sort_nodes on one array (orbx_debug_wave_sort)
__global__ __launch_bounds__(64) void k_debug_wave_sort(SortNode* __restrict__ data, int n)
{
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ int s_stack[3 * kIntrosortStack];
    SortNode* const v = (SortNode*)smem;
    SortNode* const out = v + n;
    short* const rank_tmp = (short*)(out + n);
    for (int i = threadIdx.x; i < n; i += 64) v[i] = data[i];
    __syncthreads();
    wave_sort_nodes(v, out, n, s_stack, rank_tmp);
    for (int i = threadIdx.x; i < n; i += 64) data[i] = out[i];
}

// test hook: fast_m_tree alone (orbx_debug_fast_scores).  One lane per 7 x 7 patch; the patches of a workgroup lie in LDS as the strips'
// tiles do, at row pitch `pitch`: per_band = pitch / 8 of them side by side, eight columns apart, in bands of seven rows.
__global__ __launch_bounds__(64) void k_debug_fast_scores(const uint8_t* __restrict__ patches, int n, int pitch, int per_band, int* __restrict__ out)
{
    extern __shared__ __align__(16) uint8_t smem[];
    const int i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    const int band = (int)threadIdx.x / per_band, col = 8 * ((int)threadIdx.x - band * per_band);
    uint8_t* const p = smem + band * 7 * pitch + col;           // rows 0..6, columns col .. col + 6 <= 8 * per_band - 2 < pitch
    for (int r = 0; r < 7; r++)
        for (int c = 0; c < 7; c++) p[r * pitch + c] = patches[(size_t)i * 49 + r * 7 + c];
    wave_lds_fence();                                           // a lane reads what it wrote itself
    out[i] = fast_m_tree(p + 3 * pitch + 3, pitch);
}

// ------------------------------------------------------------------------------------------------
// E8 (index part): slot of every selected keypoint in the output arrays.  Level-major order; keypoints
// whose scaled x lies in [lap0, lap1] are written from the back (stereoIndex--), the rest from the front.
// One wave per frame.  meta[k] = (level << 24 | rank within level), dst[k] = output row.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_index(const LevelDesc* __restrict__ levels, int n_levels,
                                              const uint32_t* __restrict__ sel, int sel_frame_stride,
                                              const int* __restrict__ sel_count, int lap0, int lap1, int cap,
                                              int* __restrict__ kp_dst, int kp_frame_stride,
                                              int* __restrict__ n_out, int* __restrict__ mono_out, int* __restrict__ status)
{
    const int frame = blockIdx.x, lane = threadIdx.x;
    const int* sc = sel_count + (size_t)frame * n_levels;
    int total = 0;
    for (int l = 0; l < n_levels; l++) total += sc[l];
    int* dst = kp_dst + (size_t)frame * kp_frame_stride;
    int mono = 0, stereo = total - 1;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int l = 0; l < n_levels; l++) {
        const LevelDesc L = levels[l];
        const uint32_t* s = sel + (size_t)frame * sel_frame_stride + L.sel_off;
        const int n = sc[l];
        for (int k0 = 0; k0 < n; k0 += 64) {
            const int k = k0 + lane;
            bool valid = k < n, lap = false;
            if (valid) {
                float x = (float)(key_x(s[k]) + 16);
                if (l != 0) x = x * L.scale;
                lap = (x >= (float)lap0) && (x <= (float)lap1);
            }
            const unsigned long long ml = __ballot(valid && lap), mm = __ballot(valid && !lap);
            if (valid) dst[L.sel_off + k] = lap ? stereo - __popcll(ml & lt) : mono + __popcll(mm & lt);
            stereo -= __popcll(ml);
            mono += __popcll(mm);
        }
    }
    if (lane == 0) {
        n_out[frame] = total;
        mono_out[frame] = mono;
        if (total > cap) atomicExch(status + frame, ORBX_ERR_CAPACITY);
    }
}

// ------------------------------------------------------------------------------------------------
// E6: GaussianBlur 7x7, sigma 2, BORDER_REFLECT_101 -- OpenCV 4.x fixed-point path:
// horizontal u8 x Q8.8 taps -> Q8.8 (u16), vertical Q8.8 x Q8.8 -> Q16.16, (v + 0x8000) >> 16.
// 256 threads per 64x58 output tile; the (64+6) x (58+6) source window is staged in LDS (k_blur).
// ------------------------------------------------------------------------------------------------
__device__ __forceinline__ int reflect101(int p, int len)
{
    if (len == 1) return 0;
    while (p < 0 || p >= len) p = (p < 0) ? -p : 2 * len - 2 - p;
    return p;
}

constexpr int kBlurTW = 64, kBlurTH = 58;        // outputs per tile; 58 + 6 = 64 staged rows = 32 row pairs
constexpr int kBlurSP = 96;                      // LDS row pitch: source column x0 - 4 is byte 12, so the 16-byte chunks of the tile start at byte 16

// one horizontal work item: rows 2p, 2p+1 of the staged window x columns 4q .. 4q+3 -> four (row 2p | row 2p+1 << 16) Q8.8 pairs.
// Output column 4q+k of a row uses source bytes k+1 .. k+7 of the 12 bytes w0 w1 w2 (taps (t0 t1 t2 t3) on k+1..k+4, (t2 t1 t0 0)
// on k+5..k+8).  The taps sum to 256, so a sum never exceeds 255 * 256 = 65280: it fits 16 bits.
__device__ __forceinline__ void blur_h_item(const uint8_t* __restrict__ src /* row 2p, byte 12 + 4q */, uint32_t* __restrict__ hp, uint32_t tapA, uint32_t tapB)
{
    uint32_t o[2][4];
#pragma unroll
    for (int rr = 0; rr < 2; rr++) {
        const uint32_t* w = (const uint32_t*)(src + rr * kBlurSP);
        const uint32_t w0 = w[0], w1 = w[1], w2 = w[2];
        o[rr][0] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 1), tapA, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 1), tapB, 0u, false), false);
        o[rr][1] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 2), tapA, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 2), tapB, 0u, false), false);
        o[rr][2] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, 3), tapA, __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, 3), tapB, 0u, false), false);
        o[rr][3] = __builtin_amdgcn_udot4(w1, tapA, __builtin_amdgcn_udot4(w2, tapB, 0u, false), false);
    }
    // (row 2p | row 2p+1 << 16): the low halves of two sums in one v_perm
    *(uint4*)hp = make_uint4(__builtin_amdgcn_perm(o[1][0], o[0][0], 0x05040100u), __builtin_amdgcn_perm(o[1][1], o[0][1], 0x05040100u),
                             __builtin_amdgcn_perm(o[1][2], o[0][2], 0x05040100u), __builtin_amdgcn_perm(o[1][3], o[0][3], 0x05040100u));
}

struct BlurTaps { us2 e0, e1, e2, e3, o0, o1, o2, o3; };

// one vertical work item: output rows 2m, 2m+1 x columns 4q .. 4q+3 from the row pairs m .. m+3 (`hp`: pair m, column 4q).
// The 7 taps of an output are 4 x v_dot2_u32_u16 on those pairs (even row: (t0 t1)(t2 t3)(t2 t1)(t0 0), odd: (0 t0)(t1 t2)(t3 t2)(t1 t0)),
// rounding folded into the first accumulator, the four result bytes gathered with v_perm.
__device__ __forceinline__ void blur_v_item(const uint32_t* __restrict__ hp, const BlurTaps& c, uint8_t* __restrict__ dst, uint32_t off, uint32_t stride, bool odd_row)
{
    const uint4 P0 = *(const uint4*)hp, P1 = *(const uint4*)(hp + kBlurTW), P2 = *(const uint4*)(hp + 2 * kBlurTW), P3 = *(const uint4*)(hp + 3 * kBlurTW);
    const uint32_t a0[4] = {P0.x, P0.y, P0.z, P0.w}, a1[4] = {P1.x, P1.y, P1.z, P1.w}, a2[4] = {P2.x, P2.y, P2.z, P2.w}, a3[4] = {P3.x, P3.y, P3.z, P3.w};
    uint32_t e[4], o[4];
#pragma unroll
    for (int k = 0; k < 4; k++) {       // Q16.16 sums + 0x8000: the result byte is bits 16..23 (at most 255 * 65536 + 32768)
        e[k] = __builtin_amdgcn_udot2(as_us2(a3[k]), c.e3, __builtin_amdgcn_udot2(as_us2(a2[k]), c.e2, __builtin_amdgcn_udot2(as_us2(a1[k]), c.e1,
               __builtin_amdgcn_udot2(as_us2(a0[k]), c.e0, 0x8000u, false), false), false), false);
        o[k] = __builtin_amdgcn_udot2(as_us2(a3[k]), c.o3, __builtin_amdgcn_udot2(as_us2(a2[k]), c.o2, __builtin_amdgcn_udot2(as_us2(a1[k]), c.o1,
               __builtin_amdgcn_udot2(as_us2(a0[k]), c.o0, 0x8000u, false), false), false), false);
    }
    // bytes 2 of four accumulators -> one dword
    const uint32_t pe = __builtin_amdgcn_perm(__builtin_amdgcn_perm(e[3], e[2], 0x0C0C0602u), __builtin_amdgcn_perm(e[1], e[0], 0x0C0C0602u), 0x05040100u);
    const uint32_t po = __builtin_amdgcn_perm(__builtin_amdgcn_perm(o[3], o[2], 0x0C0C0602u), __builtin_amdgcn_perm(o[1], o[0], 0x0C0C0602u), 0x05040100u);
    *(uint32_t*)(dst + off) = pe;                       // the row padding absorbs the tail of the last dword
    if (odd_row) *(uint32_t*)(dst + (off + stride)) = po;
}

// 256 threads per 64 x 58 output tile at a multiple of 64 columns.  The (64 + 6) x (58 + 6) source window is staged in LDS as the
// four aligned 16-byte chunks of the tile's columns plus the dword on either side (columns x0-4 .. x0+67): thread (row, chunk) =
// (tid >> 2, tid & 3) loads one chunk, the threads of chunks 0 and 3 the side dwords as well, all before one wait.  Loaded bytes past
// the last column are row padding; they only reach outputs that are not stored.  The three columns left of column 0 and right of
// column w - 1 (BORDER_REFLECT_101) are byte copies inside LDS, in the tiles that the host marks as touching that edge (TileDesc::edge).
//   horizontal  512 work items of 2 rows x 4 columns, two per thread (blur_h_item)
//   vertical    464 work items of 2 rows x 4 columns, two per thread (blur_v_item)
// Work items outside the image (quads at or beyond w, rows that no stored output reads) are skipped in all three phases.
// raw_out != nullptr (level 0 taken from the caller's image): the tile's own pixels are also copied into the pyramid, which
// is what later readers of level 0 (descriptors, stereo matching, the mvImagePyramid getter) use.
__global__ __launch_bounds__(256) void k_blur(SrcImage lvl0, const uint8_t* __restrict__ pyr, uint8_t* __restrict__ raw_out, uint8_t* __restrict__ blur,
                                              size_t frame_stride, const LevelDesc* __restrict__ levels, const TileDesc* __restrict__ tiles, int n_tiles,
                                              int t0, int t1, int t2, int t3)
{
    constexpr int SP = kBlurSP, SR = kBlurTH + 6;
    __shared__ __align__(16) uint8_t s_src[SR * SP];
    __shared__ __align__(16) uint32_t s_hp[(SR / 2) * kBlurTW];
    const int tile_idx = xcd_remap(blockIdx.x, gridDim.x, blockIdx.y);     // contiguous tile range per XCD (see k_fast_strips)
    if (tile_idx >= n_tiles) return;
    const TileDesc T = tiles[tile_idx];
    const LevelDesc L = levels[T.level];
    const bool ext = T.level == 0 && lvl0.base != nullptr;
    // per-frame bases are wave-uniform (scalar registers); everything per thread is a 32-bit offset inside the frame's level
    const uint8_t* img = ext ? lvl0.base + (size_t)blockIdx.y * lvl0.frame_stride : pyr + (size_t)blockIdx.y * frame_stride + L.off;
    const uint32_t istride = (uint32_t)(ext ? lvl0.stride : L.stride), ostride = (uint32_t)L.stride;
    uint8_t* dst = blur + (size_t)blockIdx.y * frame_stride + L.off;
    const int tid = threadIdx.x;
    const int x0 = T.x0, y0 = T.y0, w = L.w, h = L.h;
    const int rows_in = min(h - y0, kBlurTH);           // output rows of this tile; staged rows 0 .. rows_in + 5 feed them
    {
        const int r = tid >> 2, c = tid & 3;
        const int cx = x0 + 16 * c, y = y0 + r - 3;
        uint4 v = make_uint4(0u, 0u, 0u, 0u);
        uint32_t left = 0u, right = 0u;
        if (r < rows_in + 6) {
            const uint32_t ro = __umul24((uint32_t)reflect101(y, h), istride);
            if (cx < w) v = *(const uint4*)(img + (ro + (uint32_t)cx));
            if (c == 0 && x0 > 0) left = *(const uint32_t*)(img + (ro + (uint32_t)(x0 - 4)));
            if (c == 3 && x0 + kBlurTW < w) right = *(const uint32_t*)(img + (ro + (uint32_t)(x0 + kBlurTW)));
            *(uint4*)(s_src + r * SP + 16 + 16 * c) = v;
            if (c == 0) *(uint32_t*)(s_src + r * SP + 12) = left;
            if (c == 3) *(uint32_t*)(s_src + r * SP + 16 + kBlurTW) = right;
            // level 0 of the pyramid = the caller's image (what k_copy_level0 would have written): the tile's own rows, dword by dword
            // up to the last pixel's
            if (ext && raw_out != nullptr && r >= 3 && r < rows_in + 3 && cx < w) {
                uint8_t* rp = raw_out + (size_t)blockIdx.y * frame_stride + L.off + (__umul24((uint32_t)y, ostride) + (uint32_t)cx);
                if (cx + 12 < w) *(uint4*)rp = v;
                else {
                    *(uint32_t*)rp = v.x;
                    if (cx + 4 < w) *(uint32_t*)(rp + 4) = v.y;
                    if (cx + 8 < w) *(uint32_t*)(rp + 8) = v.z;
                }
            }
        }
    }
    __syncthreads();
    if (T.edge) {       // (uniform) columns -3 .. -1 and w .. w+2 of every staged row: wave j copies column -1-j and / or w+j
        const int r = tid & 63, j = __builtin_amdgcn_readfirstlane(tid >> 6);
        if (j < 3) {
            uint8_t* row = s_src + r * SP + 16 - x0;        // byte of column 0
            if (T.edge & 1) row[-1 - j] = row[reflect101(-1 - j, w)];
            if ((T.edge & 2) && w + j < x0 + kBlurTW + 4) row[w + j] = row[reflect101(w + j, w)];
        }
        __syncthreads();
    }
    const uint32_t tapA = (uint32_t)t0 | ((uint32_t)t1 << 8) | ((uint32_t)t2 << 16) | ((uint32_t)t3 << 24);
    const uint32_t tapB = (uint32_t)t2 | ((uint32_t)t1 << 8) | ((uint32_t)t0 << 16);
    const int q = tid & 15, pm = tid >> 4;              // this thread's quad of columns; its row pairs are pm and pm + 16 in both passes
    const bool q_in = x0 + 4 * q < w;
    // ---- horizontal: row pair p holds staged rows 2p, 2p+1; the last pair a stored output reads is (rows_in + 5) >> 1 ----
    {
        const uint8_t* sp = s_src + 2 * pm * SP + 12 + 4 * q;
        uint32_t* hp = s_hp + pm * kBlurTW + 4 * q;
        if (q_in && 2 * pm < rows_in + 6) blur_h_item(sp, hp, tapA, tapB);
        if (q_in && 2 * pm + 32 < rows_in + 6) blur_h_item(sp + 32 * SP, hp + 16 * kBlurTW, tapA, tapB);
    }
    __syncthreads();
    // ---- vertical ----
    {
        BlurTaps c;
        c.e0 = as_us2((uint32_t)t0 | ((uint32_t)t1 << 16)); c.e1 = as_us2((uint32_t)t2 | ((uint32_t)t3 << 16));
        c.e2 = as_us2((uint32_t)t2 | ((uint32_t)t1 << 16)); c.e3 = as_us2((uint32_t)t0);
        c.o0 = as_us2((uint32_t)t0 << 16); c.o1 = as_us2((uint32_t)t1 | ((uint32_t)t2 << 16));
        c.o2 = as_us2((uint32_t)t3 | ((uint32_t)t2 << 16)); c.o3 = as_us2((uint32_t)t1 | ((uint32_t)t0 << 16));
        const uint32_t* hp = s_hp + pm * kBlurTW + 4 * q;
        const uint32_t off = __umul24((uint32_t)(y0 + 2 * pm), ostride) + (uint32_t)(x0 + 4 * q);
        if (q_in && 2 * pm < rows_in) blur_v_item(hp, c, dst, off, ostride, 2 * pm + 1 < rows_in);
        if (q_in && 2 * pm + 32 < rows_in) blur_v_item(hp + 16 * kBlurTW, c, dst, off + 32u * ostride, ostride, 2 * pm + 33 < rows_in);
    }
}

// ------------------------------------------------------------------------------------------------
// E5 + E7 + E8: half a wave per keypoint.  IC_Angle on the unblurred level, steered BRIEF on the blurred
// level, then the cv::KeyPoint record and the 32-byte descriptor are written to their output row.
// ------------------------------------------------------------------------------------------------
// mask of the radius-15 disc (umax, :453-468) per patch row, as byte masks of the 8 dwords that hold columns u = -15 .. 16
struct IcMask { uint32_t m[32][8]; };
constexpr IcMask make_ic_mask()
{
    IcMask t{};
    const int um[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};
    for (int r = 0; r < 31; r++) {
        const int v = r - 15, av = v < 0 ? -v : v;
        for (int j = 0; j < 8; j++)
            for (int k = 0; k < 4; k++) {
                const int u = -15 + 4 * j + k, au = u < 0 ? -u : u;
                if (u <= 15 && au <= um[av]) t.m[r][j] |= 0xFFu << (8 * k);
            }
    }
    return t;
}
__device__ const IcMask d_ic_mask = make_ic_mask();

__global__ __launch_bounds__(256) void k_orient_desc(const uint8_t* __restrict__ pyr, const uint8_t* __restrict__ blur, size_t frame_stride,
                                                     const LevelDesc* __restrict__ levels, int n_levels,
                                                     const uint32_t* __restrict__ sel, int sel_frame_stride,
                                                     const int* __restrict__ sel_count,
                                                     const int* __restrict__ kp_dst, int kp_frame_stride,
                                                     OrbxKeyPoint* __restrict__ kps, uint8_t* __restrict__ desc, int cap,
                                                     OrbxKeyPoint* __restrict__ lvl_kps /* optional: per-level keypoints, level coords */,
                                                     int quads_per_frame, int batch)
{
    // TWO keypoints per wave, one per half: the intensity-centroid rows (31 lanes each), the angle, its sine and cosine and
    // the bookkeeping are the same instructions for both halves, and a lane steers 8 of its keypoint's 256 pairs instead of 4 --
    // a third fewer wave instructions per keypoint than one keypoint per wave.
    // Everything a keypoint needs -- the 31x31 disc of the unblurred level (IC_Angle) and the 37x37 window of the blurred level
    // that the rotated pattern can reach (|coordinate| <= 18 < EDGE_THRESHOLD) -- is fetched up front with wide loads (the address
    // unit takes 16 clocks per wave-wide load whatever its width), so a wave sees two dependent memory round trips (selection
    // record, patches).
    constexpr int kBR = 18, kBP = 64, kPR = 15;                 // blur: 37 rows x 4 chunks
    constexpr int kBBytes = (2 * kBR + 1) * kBP;
    __shared__ __align__(16) uint8_t s_patch[8][kBBytes];
    // 1-D grid of octets_per_frame * batch workgroups (8 keypoints each).  Workgroup w runs on XCD w % 8: giving XCD k the
    // contiguous range [k * total / 8, (k + 1) * total / 8) of (frame, octet) pairs keeps all the patches of a frame in ONE L2
    // (2.4 MB of pyramid + blur per frame against 4 MB of L2) instead of fetching every frame into all eight.
    const int total_wg = gridDim.x, per_xcd = total_wg >> 3;            // the host pads the grid to a multiple of 8
    const int v_id = (int)(blockIdx.x & 7) * per_xcd + (int)(blockIdx.x >> 3);
    const int frame = v_id / quads_per_frame, quad = v_id - frame * quads_per_frame;
    if (frame >= batch) return;                                         // grid padding (uniform for the workgroup)
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int half = lane >> 5, hl = lane & 31;
    // the selection slots of all levels are one flat range [0, sel_frame_stride): a half-wave takes slot s and finds its level
    // from the level offsets, so no workgroup is launched for slots a level does not have
    // (the levels' slot ranges start at even offsets, so both halves of a wave are in the same level: scalar table loads)
    const int s_pair = quad * 8 + wave * 2, s_flat = s_pair + half;
    int level = 0;
    for (int l = 1; l < n_levels; l++) level = (s_pair >= levels[l].sel_off) ? l : level;
    const LevelDesc L = levels[level];
    const int k = s_flat - L.sel_off;
    const bool live = s_flat < sel_frame_stride && k < L.sel_cap && k < sel_count[(size_t)frame * n_levels + level];
    const int slot = L.sel_off + (live ? k : 0);
    const uint32_t e = live ? sel[(size_t)frame * sel_frame_stride + slot] : 0u;
    const int row = live ? kp_dst[(size_t)frame * kp_frame_stride + slot] : -1;
    uint32_t pw[8];
#pragma unroll
    for (int q = 0; q < 8; q++) pw[q] = ((const uint32_t*)d_pattern)[hl + 32 * q];       // one dword = (x0, y0, x1, y1) as int8
    const int px = (int)key_x(e) + 16, py = (int)key_y(e) + 16;     // level coordinates (:885-886)
    uint8_t* sb = s_patch[wave * 2 + half];
    const int xb = (px - kBR) & ~15;                                // 16-byte aligned window start (rows are 64-B aligned)
    // The time of this kernel is the number of keypoints a CU holds in flight over their two memory round trips (measured: it
    // scales with the LDS a workgroup is given), so LDS only holds what is addressed at random -- the blurred window.  The
    // intensity-centroid rows go straight into the registers of the lanes that own them: row r of the 31 x 31 patch = the 9 dwords
    // from the dword that holds column u = -15 on (dword-aligned wide loads).
    uint32_t icw[9];
#pragma unroll
    for (int j = 0; j < 9; j++) icw[j] = 0u;
    if (live) {
        const uint8_t* bbase = blur + (size_t)frame * frame_stride + L.off + (size_t)(py - kBR) * L.stride + xb;
        for (int i = hl; i < (2 * kBR + 1) * 4; i += 32) {
            const int r = i >> 2, c = i & 3;
            *(uint4*)(sb + r * kBP + 16 * c) = *(const uint4*)(bbase + (size_t)r * L.stride + 16 * c);
        }
        if (hl < 2 * kPR + 1) {
            const uint8_t* rp = pyr + (size_t)frame * frame_stride + L.off + (size_t)(py - kPR + hl) * L.stride + ((px - kPR) & ~3);
            const Dwords4 q0 = *(const Dwords4*)rp, q1 = *(const Dwords4*)(rp + 16);
            icw[0] = q0.x; icw[1] = q0.y; icw[2] = q0.z; icw[3] = q0.w; icw[4] = q1.x; icw[5] = q1.y; icw[6] = q1.z; icw[7] = q1.w;
            icw[8] = *(const uint32_t*)(rp + 32);
        }
    }
    // the LDS window is private to the (half-)wave: its own writes are ordered before its own reads by the LDS queue; only the
    // compiler has to be kept from reordering them -- no workgroup barrier, so a wave never waits for its three neighbours
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    if (__ballot(live) == 0ull) return;

    // ---- IC_Angle (:76-103): lane r < 31 of a half owns patch row v = r - 15: its 31 bytes as 8 byte-aligned dwords, masked to
    // the disc; the row sums  a = sum I  and  b = sum (u + 15) I  are byte dot products, m10 += b - 15 a, m01 += v a ----
    int m10 = 0, m01 = 0;
    if (live && hl < 2 * kPR + 1) {
        const uint32_t sh = (uint32_t)((px - kPR) & 3);
        const uint4 ma = *(const uint4*)&d_ic_mask.m[hl][0], mb = *(const uint4*)&d_ic_mask.m[hl][4];
        const uint32_t mk[8] = {ma.x, ma.y, ma.z, ma.w, mb.x, mb.y, mb.z, mb.w};
        uint32_t a = 0u, b = 0u;
#pragma unroll
        for (int j = 0; j < 8; j++) {
            const uint32_t d = __builtin_amdgcn_alignbyte(icw[j + 1], icw[j], sh) & mk[j];
            a = __builtin_amdgcn_udot4(d, 0x01010101u, a, false);
            b = __builtin_amdgcn_udot4(d, 0x03020100u + 0x04040404u * (uint32_t)j, b, false);
        }
        m10 = (int)b - 15 * (int)a;
        m01 = (hl - kPR) * (int)a;
    }
    for (int o = 16; o > 0; o >>= 1) { m10 += __shfl_xor(m10, o); m01 += __shfl_xor(m01, o); }     // (inside the half)
    const float angle = fast_atan2_deg((float)m01, (float)m10);

    // ---- steered BRIEF: a lane handles the pairs hl, hl + 32, ..., hl + 224 of its keypoint; ballot q = the descriptor's 32-bit
    // word q of the lower-half keypoint in its low half, of the upper-half keypoint in its high half
    const float factorPI = (float)(3.141592653589793238462643383279502884 / 180.f);
    float a, b;
    sincos_f32(angle * factorPI, &a, &b);
    const uint8_t* bimg = sb + kBR * kBP + (px - xb);
    unsigned long long w[8];
#pragma unroll
    for (int q = 0; q < 8; q++) {
        const float x0 = (float)(signed char)(pw[q] & 0xFF), y0 = (float)(signed char)((pw[q] >> 8) & 0xFF);
        const float x1 = (float)(signed char)((pw[q] >> 16) & 0xFF), y1 = (float)(signed char)(pw[q] >> 24);
        int t0 = 0, t1 = 0;
        if (live) {
            t0 = bimg[cv_round_f(x0 * b + y0 * a) * kBP + cv_round_f(x0 * a - y0 * b)];
            t1 = bimg[cv_round_f(x1 * b + y1 * a) * kBP + cv_round_f(x1 * a - y1 * b)];
        }
        w[q] = __ballot(t0 < t1);
    }
    if (!live) return;
    if (hl == 0) {
        OrbxKeyPoint kp;
        kp.x = (float)px; kp.y = (float)py;
        kp.size = (float)L.patch_size; kp.angle = angle; kp.response = (float)key_resp(e);
        kp.octave = level; kp.class_id = -1;
        if (lvl_kps) lvl_kps[(size_t)frame * sel_frame_stride + slot] = kp;
        if (level != 0) { kp.x = kp.x * L.scale; kp.y = kp.y * L.scale; }      // :1149-1151
        if (row >= 0 && row < cap) kps[(size_t)frame * cap + row] = kp;
    }
    if (hl < 8 && row >= 0 && row < cap) {
        unsigned long long mine = w[0];
#pragma unroll
        for (int q = 1; q < 8; q++) mine = (hl == q) ? w[q] : mine;
        ((uint32_t*)(desc + ((size_t)frame * cap + row) * 32))[hl] = (uint32_t)(mine >> (32 * half));
    }
}

// ------------------------------------------------------------------------------------------------
// Frame::ComputeStereoMatches (reference src/Frame.cc:931-1101), SURVEY 8(f) rank 4.  One wave per left key point:
// the row table of the reference (vRowIndices) becomes a lane-strided scan of the right key points with the same band
// test; first minimum through a (distance, index) key; then the 11 x 11 SAD sliding window over 11 shifts on the left
// key point's pyramid level, parabola fit and the disparity gates, in the reference's float expressions.
// ------------------------------------------------------------------------------------------------
struct StereoTables { float scale[16], inv_scale[16]; };

__global__ __launch_bounds__(256) void k_stereo_match(const uint8_t* __restrict__ pyrL, const uint8_t* __restrict__ pyrR, size_t frame_stride,
                                                     const LevelDesc* __restrict__ levels, StereoTables T,
                                                     const OrbxKeyPoint* __restrict__ kpsL, const uint8_t* __restrict__ descL, const int32_t* __restrict__ nL,
                                                     const OrbxKeyPoint* __restrict__ kpsR, const uint8_t* __restrict__ descR, const int32_t* __restrict__ nR,
                                                     int cap, float mb, float mbf, int n_levels,
                                                     float* __restrict__ u_right, float* __restrict__ depth, int32_t* __restrict__ sad_out)
{
    __shared__ uint8_t s_l[4][11 * 12], s_r[4][11 * 24];
    __shared__ int s_part[4][11 * 11];
    const int frame = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int iL = blockIdx.x * 4 + wave;
    const int n_l = min(nL[frame], cap), n_r = min(nR[frame], cap);
    const bool live = iL < n_l;
    const size_t fo = (size_t)frame * cap;
    // ---- best right key point by descriptor distance (:973-1008) ----
    float uL = 0, vL = 0;
    int levelL = 0;
    unsigned key = 0xFFFFFFFFu;
    if (live) {
        const OrbxKeyPoint kl = kpsL[fo + iL];
        uL = kl.x; vL = kl.y; levelL = kl.octave;
        const int v_row = (int)vL;                                           // vRowIndices[vL]
        const float minZ = mb, minD = 0, maxD = mbf / minZ;
        const float minU = uL - maxD, maxU = uL - minD;
        const unsigned long long* dl = (const unsigned long long*)(descL + (fo + iL) * 32);
        const unsigned long long d0 = dl[0], d1 = dl[1], d2 = dl[2], d3 = dl[3];
        for (int iR = lane; iR < n_r; iR += 64) {
            const OrbxKeyPoint kr = kpsR[fo + iR];
            const float r = 2.0f * T.scale[kr.octave & 15];
            const int maxr = (int)ceilf(kr.y + r), minr = (int)floorf(kr.y - r);
            if (v_row < minr || v_row > maxr) continue;                      // the row table of :941-960
            if (kr.octave < levelL - 1 || kr.octave > levelL + 1) continue;
            if (!(kr.x >= minU && kr.x <= maxU)) continue;
            const unsigned long long* dr = (const unsigned long long*)(descR + (fo + iR) * 32);
            const int dist = __popcll(d0 ^ dr[0]) + __popcll(d1 ^ dr[1]) + __popcll(d2 ^ dr[2]) + __popcll(d3 ^ dr[3]);
            if (dist < 100) key = min(key, ((unsigned)dist << 20) | (unsigned)iR);     // bestDist starts at TH_HIGH; first minimum
        }
    }
    for (int o = 32; o > 0; o >>= 1) key = min(key, (unsigned)__shfl_xor((int)key, o));
    const int thOrbDist = (100 + 50) / 2;
    bool ok = live && key != 0xFFFFFFFFu && (int)(key >> 20) < thOrbDist;
    if (levelL < 0 || levelL >= n_levels) ok = false;          // key points that do not come from this extractor: no table lookups out of range
    // ---- sub-pixel match by correlation (:1011-1083) ----
    float scaleduR0 = 0;
    int y0 = 0, xl0 = 0, xr_start = 0;
    size_t loff = 0;
    int lstride = 0;
    if (ok) {
        const float uR0 = kpsR[fo + (key & 0xFFFFFu)].x;
        const float scaleFactor = T.inv_scale[levelL & 15];
        const float scaleduL = roundf(uL * scaleFactor), scaledvL = roundf(vL * scaleFactor);
        scaleduR0 = roundf(uR0 * scaleFactor);
        const LevelDesc L = levels[levelL];
        loff = (size_t)L.off; lstride = L.stride;
        const int w = 5, Ls = 5;
        const float iniu = scaleduR0 + Ls - w, endu = scaleduR0 + Ls + w + 1;
        if (iniu < 0 || endu >= (float)L.w) ok = false;
        y0 = (int)(scaledvL - w); xl0 = (int)(scaleduL - w); xr_start = (int)(scaleduR0 - Ls - w);
        // cv::Mat::rowRange / colRange would assert outside the level image; key points of the extractor never get here
        if (y0 < 0 || y0 + 11 > L.h || xl0 < 0 || xl0 + 11 > L.w || xr_start < 0 || xr_start + 21 > L.w) ok = false;
    }
    if (ok) {
        const uint8_t* il = pyrL + (size_t)frame * frame_stride + loff;
        const uint8_t* ir = pyrR + (size_t)frame * frame_stride + loff;
        for (int i = lane; i < 121; i += 64) { const int r = i / 11, c = i - r * 11; s_l[wave][r * 12 + c] = il[(size_t)(y0 + r) * lstride + xl0 + c]; }
        for (int i = lane; i < 231; i += 64) { const int r = i / 21, c = i - r * 21; s_r[wave][r * 24 + c] = ir[(size_t)(y0 + r) * lstride + xr_start + c]; }
    }
    __syncthreads();
    if (ok) {
        for (int i = lane; i < 121; i += 64) {
            const int sft = i / 11, r = i - sft * 11;
            int acc = 0;
#pragma unroll
            for (int c = 0; c < 11; c++) acc += abs((int)s_l[wave][r * 12 + c] - (int)s_r[wave][r * 24 + sft + c]);
            s_part[wave][sft * 11 + r] = acc;
        }
    }
    __syncthreads();
    if (ok && lane == 0) {
        const int Ls = 5;
        float vDists[11];
        int bestDist = 0x7FFFFFFF, bestincR = 0;
        for (int sft = 0; sft < 11; sft++) {
            int sad = 0;
            for (int r = 0; r < 11; r++) sad += s_part[wave][sft * 11 + r];
            const float dist = (float)sad;                                   // cv::norm(IL, IR, NORM_L1)
            if (dist < (float)bestDist) { bestDist = (int)dist; bestincR = sft - Ls; }
            vDists[sft] = dist;
        }
        float ur_out = -1.0f, depth_out = -1.0f;
        int sad_best = -1;
        if (!(bestincR == -Ls || bestincR == Ls)) {
            const float dist1 = vDists[Ls + bestincR - 1], dist2 = vDists[Ls + bestincR], dist3 = vDists[Ls + bestincR + 1];
            const float deltaR = (dist1 - dist3) / (2.0f * (dist1 + dist3 - 2.0f * dist2));
            if (!(deltaR < -1 || deltaR > 1)) {
                float bestuR = T.scale[levelL & 15] * ((float)scaleduR0 + (float)bestincR + deltaR);
                float disparity = (uL - bestuR);
                const float minD = 0, maxD = mbf / mb;
                if (disparity >= minD && disparity < maxD) {
                    if (disparity <= 0) { disparity = 0.01; bestuR = uL - 0.01; }      // double literals, as in :1073-1074
                    depth_out = mbf / disparity;
                    ur_out = bestuR;
                    sad_best = bestDist;
                }
            }
        }
        u_right[fo + iL] = ur_out; depth[fo + iL] = depth_out; sad_out[fo + iL] = sad_best;
    } else if (live && lane == 0) {
        u_right[fo + iL] = -1.0f; depth[fo + iL] = -1.0f; sad_out[fo + iL] = -1;
    }
}

// median cut of :1086-1100: matches whose SAD is >= 1.5 * 1.4 * median are dropped.  One workgroup per frame.
__global__ __launch_bounds__(256) void k_stereo_median(const int32_t* __restrict__ nL, int cap, int n_pow2_max,
                                                      float* __restrict__ u_right, float* __restrict__ depth, const int32_t* __restrict__ sad)
{
    extern __shared__ int s_sad[];       // n_pow2_max
    __shared__ int s_cnt;
    const int frame = blockIdx.x, tid = threadIdx.x;
    const int n = min(nL[frame], cap);
    int n_pow2 = 2;                      // this frame's own sort size (the launch's LDS is sized for the arrays' capacity)
    while (n_pow2 < n) n_pow2 <<= 1;
    n_pow2 = min(n_pow2, n_pow2_max);
    const size_t fo = (size_t)frame * cap;
    if (tid == 0) s_cnt = 0;
    __syncthreads();
    int local = 0;
    for (int i = tid; i < n_pow2; i += 256) {
        const int v = (i < n) ? sad[fo + i] : -1;
        s_sad[i] = v >= 0 ? v : 0x7FFFFFFF;
        local += v >= 0;
    }
    if (local) atomicAdd(&s_cnt, local);
    __syncthreads();
    // bitonic sort by the 4 waves: wave w owns chunk w (n_pow2 / 4 values); exchanges with a stride below the chunk size stay inside it
    // (the wave's own program order), only the three passes across chunks take a workgroup barrier
    {
        const int lane = tid & 63, wave = tid >> 6;
        const int chunk = n_pow2 >> 2, pairs = n_pow2 >> 3;
        bool need_block = false;             // (the barrier above made the values visible)
        for (int k = 2; k <= n_pow2; k <<= 1)
            for (int j = k >> 1; j > 0; j >>= 1) {
                const bool cross = j >= chunk || n_pow2 < 8;
                if (cross || need_block) __syncthreads();
                else { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); }
                need_block = cross;
                const int t0 = n_pow2 >= 8 ? wave * pairs + lane : tid, t1 = n_pow2 >= 8 ? (wave + 1) * pairs : (n_pow2 >> 1), ts = n_pow2 >= 8 ? 64 : 256;
                for (int t = t0; t < t1; t += ts) {
                    const int lo = 2 * t - (t & (j - 1)), hi = lo + j;
                    const bool up = (lo & k) == 0;
                    const int a = s_sad[lo], b = s_sad[hi];
                    if ((a > b) == up) { s_sad[lo] = b; s_sad[hi] = a; }
                }
            }
        __syncthreads();
    }
    const int m = s_cnt;
    if (m == 0) return;
    const float median = (float)s_sad[m / 2];
    const float thDist = 1.5f * 1.4f * median;
    for (int i = tid; i < n; i += 256) {
        const int v = sad[fo + i];
        if (v >= 0 && !((float)v < thDist)) { u_right[fo + i] = -1; depth[fo + i] = -1; }
    }
}

}  // namespace orbx
