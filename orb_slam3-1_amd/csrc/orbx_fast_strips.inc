// orbx_fast_strips.inc -- E2: FAST-9/16 for the cells of ComputeKeyPointsOctTree (reference src/ORBextractor.cc:787-872),
// one 256-thread workgroup per STRIP = a run of horizontally adjacent cells of one cell row.  (Included by orbx_kernels.hip.)
//
// The cell interiors of a level tile its detection area exactly (SURVEY E2), so a strip is processed as ONE image region and
// the cell structure only enters where the reference's semantics need it: the 3x3 non-maximum suppression treats everything
// outside a pixel's own cell interior as 0, the iniThFAST -> minThFAST fallback is per cell, and the output order is
// cell-major / row-major.  At iniThFAST, over the whole strip, every WAVE owns the rows y = wave, wave + 4, ... of the strip and
// keeps its lists to itself (counters in SGPRs, no LDS atomics, no workgroup barrier until the score map is needed by the
// neighbours):
//
//   stage 1  dense, 4 pixels per lane in packed u16 pairs: the COMPASS quick test -- a 9-arc of the ring contains ring pixel
//            0 or 8 and ring pixel 4 or 12, so a corner at t has, with one polarity, one pixel of each of these two opposite
//            pairs beyond the threshold.  5 aligned LDS dword reads and 34 vector instructions per 4 pixels; a quad with a
//            survivor becomes ONE 16-bit entry of the wave's list (ballot + mbcnt).  On the synthetic frames 5.7 % of the
//            pixels survive at t = 20 (the exact 8-pair test: 3.8 %, at 3.4x the instructions).
//   expand   128 entries at a time -> list of surviving pixels (DPP prefix sum of the popcounts)
//   stage 2  one lane per surviving pixel: M = max over the 16 arcs of min(+-(v - ring)), both polarities in one packed-f16
//            min3 / max3 tree (fast_m_tree); OpenCV's corner test at t is M > t and its response M - 1 (SURVEY App. A.1).  M goes
//            into a byte map with a zero halo; pixels with M > t join the wave's corner list.
//   -------- workgroup barrier --------
//   nms      one lane per corner: strict 3x3 maximum over the neighbours that are corners at t AND lie in the same cell
//            interior; winners set a bit in their cell's row-major bitmask.
//   -------- workgroup barrier --------
//   rank     per cell (one wave each): exclusive prefix of the mask's word popcounts -> cell count (0 => fallback phase)
//   emit     one lane per corner whose bit is set: rank = prefix[word] + popcount(lower bits) -> the cell's slots in HBM.
//
// Then minThFAST for each cell of the strip that found nothing (:843-846; 9 % of the cells of the synthetic frames, a handful of
// corners each).  The quick test is the wide part and is shared out as before: every wave lists the entries of its rows, cell
// by cell.  After ONE workgroup barrier the k-th such cell of the strip is the work of wave k & 3 alone, which expands the
// cell's segment of all four entry lists and runs stage 2, nms, rank and emit of that cell, ordered by its own LDS queue
// (wave_lds_fence).  No further barrier is needed because a cell is self-contained: the suppression masks everything outside
// the cell interior, and the cell's mask words, prefix words, total and map bytes have no other writer -- a quad that
// straddles two cells is scored by both owners, which store the same score in the same byte.  The cells of a strip run side
// by side, and a strip without such a cell (three in four) pays nothing.
//
// Set-up.  Everything a workgroup needs before the first pixel, except the pixels, is known when the geometry is set up, so the host
// builds one record per strip (StripRec): where the tile lies in the pyramid, its size in 16-byte chunks with an exact reciprocal for
// chunk -> (row, chunk of the row), and the cells' columns, slots and the finished column -> cell row exactly as they lie in LDS.  The
// record is addressed by the strip index alone: 32 bytes through the scalar unit, the table as one 16-byte load per lane of wave 0.
// Two dependent global round trips remain (record, tile).  A thread has its chunks of the tile in flight together, three at a time, and
// zeroes the score map and the bitmasks with 16-byte LDS stores while they travel; then one wait, the LDS stores, ONE barrier.
//
// A corner list that overflows (more than corner_cap corners of a wave: pathological images, or the debug knob of the tests)
// sends its wave through the same nms / emit code over ALL the pixels it scored instead (its rows of the strip; in the
// minThFAST pass, the rows and quads of its cell).  Everything is integer; the result is the reference's vToDistributeKeys order and
// content bit for bit.

struct StripDesc {               // (host: the strip geometry, from which the layout of the LDS and the records below are made)
    int16_t level;
    int16_t cell0, ncell;       // cells [cell0, cell0 + ncell) of the cell table, left to right
    int16_t x0, x1;             // columns [x0, x1) spanned by the cells' sub-images (first cell's x0 .. last cell's x1)
    int16_t y0, y1;             // rows [y0, y1) of the sub-images (the same for every cell of a cell row)
    int16_t pad;
};

constexpr int kStripMaxCells = 8;
constexpr int kStripMapPitchMax = 4 * 64 + 8;         // map columns of the widest strip the host accepts (64 quads)

// What a workgroup keeps about its cells in LDS, exactly as the host lays it out in the strip's record: one 16-byte copy per lane.
struct __attribute__((aligned(16))) StripTab {
    int32_t cx0[kStripMaxCells];        // first map column of the cell's interior
    int32_t iw[kStripMaxCells];         // interior width
    int32_t slot_off[kStripMaxCells], slot_cap[kStripMaxCells];     // the cell's slots in the per-frame candidate buffer
    uint8_t colcell[(kStripMapPitchMax + 15) & ~15];                // u8 per map column: cell of the strip that owns it, 0xFF = none
};

// One record per strip, built when the geometry is set up: everything the kernel's set-up needs, addressed by the strip index alone
// (no load depends on another).  The first 32 bytes are read with scalar loads, the table with one 16-byte load per lane.
struct __attribute__((aligned(16))) StripRec {
    // (pairs of 16-bit values, all non-negative: low half | high half << 16 -- the scalar unit loads whole dwords)
    uint32_t src_off;           // pyramid byte of tile row 0, tile column 0 inside the frame (level offset + y0 * stride + xa)
    uint32_t stride;            // row stride of the level in the pyramid
    uint32_t y0_xa;             // first row of the sub-images | image column of tile column 0 (16-B aligned: dwordx4 loads)
    uint32_t th_nch;            // tile rows | 16-B chunks per tile row (up to the dword after the last quad)
    uint32_t g0_qoff;           // first image dword that holds a detection column | tile byte of quad 0's own dword (4 .. 16)
    uint32_t ncell_cell0;       // cells of the strip | the first one's index in the cell table
    uint32_t level;
    uint32_t inv_nch;           // (i * inv_nch) >> 16 == i / nch for every i < th * nch (proved by the host for every strip)
    StripTab tab;
};
static_assert(sizeof(StripTab) % 16 == 0 && sizeof(StripRec) == 32 + sizeof(StripTab), "StripRec: 32 header bytes, then the table");
constexpr int kStripTabChunks = (int)(sizeof(StripTab) / 16);

struct FastLds {                // byte offsets into the dynamic LDS block (host-computed from the largest strip)
    int32_t tile_pitch;         // bytes per tile row (multiple of 16)
    int32_t map_off, map_pitch; // M map: (ih + 2) rows, 4 bytes of margin left of the first quad; padded to whole 16-byte stores
    int32_t ent_off, ent_cap;   // u16 entries of stage 1, ent_cap per wave (worst case: every quad of the wave's rows, cell by cell)
    int32_t px_off;             // u16 surviving pixels of one batch, kPxCap per wave
    int32_t corner_off, corner_cap;   // u16 corners, corner_cap per wave
    int32_t bits_off, pre_off, wpc;   // u32 bitmasks and their word prefix sums, wpc words per cell
    int32_t total;
};

constexpr int kStripWidth = 160;      // target strip width in pixels: four 36-px cells
constexpr int kEntBatch = 128;        // entries expanded at a time ...
constexpr int kPxCap = 4 * kEntBatch; // ... into at most this many pixels
constexpr int kCornerCap = 256;       // corners a wave lists before it falls back to scanning the pixels it scored

// The score tree in packed f16, both polarities at once.  A byte b read as f16 is the subnormal b * 2^-24; differences, minima and maxima of
// such values are exact, and the raw 16 bits of a non-negative result are the integer itself.  This needs the kernel's f16 denormal mode
// "preserve" (hipcc's default, .amdhsa_float_denorm_mode_16_64 3) and opcodes that do not flush; tests/test_fast_score_tree_gpu.py runs
// this function alone (orbx_debug_fast_scores) over every difference.
typedef _Float16 fast_h2 __attribute__((ext_vector_type(2)));
// v_pk_minimum3_f16 / v_pk_maximum3_f16 (gfx950)
__device__ __forceinline__ fast_h2 fast_pk_min3(fast_h2 a, fast_h2 b, fast_h2 c) { return __builtin_elementwise_minimum(__builtin_elementwise_minimum(a, b), c); }
__device__ __forceinline__ fast_h2 fast_pk_max3(fast_h2 a, fast_h2 b, fast_h2 c) { return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), c); }
// (v - r, r - v) from two zero-extended bytes: low half v.lo + -r.lo, high half -v.lo + r.lo.  Round to nearest: x - x is +0 in both halves.
__device__ __forceinline__ fast_h2 fast_pk_diff(uint32_t v, uint32_t r)
{
    uint32_t d;
    asm("v_pk_add_f16 %0, %1, %2 op_sel_hi:[0,0] neg_lo:[0,1] neg_hi:[1,0]" : "=v"(d) : "v"(v), "v"(r));
    return __builtin_bit_cast(fast_h2, d);
}

// M = max(0, max over the 16 arcs of min(d), max over the arcs of min(-d)), d = centre - ring pixel: OpenCV's corner score + 1
__device__ __forceinline__ int fast_m_tree(const uint8_t* __restrict__ t, int pitch)
{
    const uint32_t v = t[0];
    fast_h2 d[16];                // (d, -d)
    d[0] = fast_pk_diff(v, t[3 * pitch]);       d[1] = fast_pk_diff(v, t[3 * pitch + 1]);   d[2] = fast_pk_diff(v, t[2 * pitch + 2]);   d[3] = fast_pk_diff(v, t[pitch + 3]);
    d[4] = fast_pk_diff(v, t[3]);               d[5] = fast_pk_diff(v, t[-pitch + 3]);      d[6] = fast_pk_diff(v, t[-2 * pitch + 2]);  d[7] = fast_pk_diff(v, t[-3 * pitch + 1]);
    d[8] = fast_pk_diff(v, t[-3 * pitch]);      d[9] = fast_pk_diff(v, t[-3 * pitch - 1]);  d[10] = fast_pk_diff(v, t[-2 * pitch - 2]); d[11] = fast_pk_diff(v, t[-pitch - 3]);
    d[12] = fast_pk_diff(v, t[-3]);             d[13] = fast_pk_diff(v, t[pitch - 3]);      d[14] = fast_pk_diff(v, t[2 * pitch - 2]);  d[15] = fast_pk_diff(v, t[3 * pitch - 1]);
    // minimum of every run of 3, then of every run of 9 as three runs of 3: (min of d[k .. k+8], min of -d[k .. k+8])
    fast_h2 lo3[16], lo9[16];
#pragma unroll
    for (int k = 0; k < 16; k++) lo3[k] = fast_pk_min3(d[k], d[(k + 1) & 15], d[(k + 2) & 15]);
#pragma unroll
    for (int k = 0; k < 16; k++) lo9[k] = fast_pk_min3(lo3[k], lo3[(k + 3) & 15], lo3[(k + 6) & 15]);
    // maximum over the arcs, 16 -> 6 -> 2, the last one together with +0: (best_dark, -best_bright), both clamped at 0.  The +0 also
    // keeps a -0 from the bit-level read-out below (none can arise: every d is +0 or non-zero, and minimum / maximum order -0 below +0).
    const fast_h2 a0 = fast_pk_max3(lo9[0], lo9[1], lo9[2]), a1 = fast_pk_max3(lo9[3], lo9[4], lo9[5]), a2 = fast_pk_max3(lo9[6], lo9[7], lo9[8]);
    const fast_h2 a3 = fast_pk_max3(lo9[9], lo9[10], lo9[11]), a4 = fast_pk_max3(lo9[12], lo9[13], lo9[14]);
    const fast_h2 b0 = fast_pk_max3(a0, a1, a2), b1 = fast_pk_max3(a3, a4, lo9[15]);
    const fast_h2 zero = {(_Float16)0.0f, (_Float16)0.0f};
    const fast_h2 m = fast_pk_max3(b0, b1, zero);
    // low half against high half; the raw bits of the non-negative subnormal are M
    uint32_t r;
    asm("v_pk_max_f16 %0, %1, %1 op_sel:[0,1]" : "=v"(r) : "v"(__builtin_bit_cast(uint32_t, m)));
    return (int)(r & 0xFFFFu);
}

// inclusive prefix sum over the 64 lanes without LDS traffic (row_shr 1 / 2 / 4 / 8, row_bcast 15 / 31)
__device__ __forceinline__ int wave_incl_scan(int v)
{
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xF, 0xF, false);
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xA, 0xF, false);     // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xC, 0xF, false);     // row_bcast:31 into rows 2 and 3
    return v;
}

// the LDS lists of a wave are written and read by the same wave: its LDS operations execute in order, only the compiler has
// to be kept from moving the reads above the writes
__device__ __forceinline__ void wave_lds_fence()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

#ifdef ORBX_FAST_TIMING     // cycle split over all workgroups' thread 0 (tools/fast_timing.py); never defined in the product build
__device__ unsigned long long d_fast_prof[16];
#define ORBX_FTICK(k) if (threadIdx.x == 0) { const long long t_now = clock64(); atomicAdd(&d_fast_prof[(k) + fallback_slot], (unsigned long long)(t_now - t_prev)); t_prev = t_now; }
#else
#define ORBX_FTICK(k)
#endif
__global__ __launch_bounds__(256) void k_fast_strips(SrcImage lvl0, const uint8_t* __restrict__ pyr, size_t frame_stride,
                                                     const StripRec* __restrict__ recs, int n_strips, int n_cells,
                                                     int ini_th, int min_th, FastLds Z,
                                                     uint32_t* __restrict__ cand, size_t cand_frame_stride, int* __restrict__ cell_count,
                                                     int* __restrict__ status_clear)
{
    extern __shared__ __align__(16) uint8_t smem[];
    __shared__ StripTab s_tab;
    __shared__ int s_total[kStripMaxCells];
    __shared__ int s_seg[4][kStripMaxCells + 1];        // minThFAST: where the segment of the k-th fallback cell starts in a wave's entry list
#ifdef ORBX_FAST_TIMING
    long long t_prev = clock64();
    int fallback_slot = 0;
#endif

    // the first launch of a batch clears the frames' status words (enqueue(): every writer of a non-zero status is ordered behind
    // this launch); one thread per frame, in a workgroup that every grid has
    if (status_clear != nullptr && blockIdx.x == 0 && threadIdx.x == 0) status_clear[blockIdx.y] = 0;
    const int strip_idx = xcd_remap(blockIdx.x, gridDim.x, blockIdx.y);
    if (strip_idx >= n_strips) return;
    const StripRec* S = recs + strip_idx;
    const int frame = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // the strip's record: 32 bytes through the scalar unit, the table by wave 0, one 16-byte chunk per lane; both addresses need
    // nothing but the strip index
    const uint4 h0 = ((const uint4*)S)[0], h1 = ((const uint4*)S)[1];
    uint4 tab_chunk = make_uint4(0u, 0u, 0u, 0u);
    if (wave == 0) tab_chunk = ((const uint4*)&S->tab)[min(lane, kStripTabChunks - 1)];
    const int sy0 = (int)(h0.z & 0xFFFFu), xa = (int)(h0.z >> 16);
    const int th = (int)(h0.w & 0xFFFFu), nch = (int)(h0.w >> 16), ih = th - 6;
    const int g0 = (int)(h1.x & 0xFFFFu), qoff = (int)(h1.x >> 16);
    const int ncell = (int)(h1.y & 0xFFFFu), cell0 = (int)(h1.y >> 16);
    const uint32_t inv_nch = h1.w;
#if defined(ORBX_FAST_CUT)      // a cut variant emits nothing: the stages downstream see empty cells, not whatever the buffer held
    if ((int)threadIdx.x < ncell) cell_count[(size_t)frame * n_cells + cell0 + threadIdx.x] = 0;
#endif
    const bool ext = h1.z == 0u && lvl0.base != nullptr;         // level 0 read from the caller's image in place
    // tile row 0, tile column 0 of this frame: a scalar base, the threads add 32-bit offsets
    const uint8_t* img = (ext ? lvl0.base : pyr) + (size_t)frame * (ext ? lvl0.frame_stride : frame_stride) +
                         (ext ? (size_t)sy0 * (size_t)lvl0.stride + (size_t)xa : (size_t)h0.x);
    const uint32_t istride = ext ? (uint32_t)lvl0.stride : h0.y;

    const int TP = Z.tile_pitch, MP = Z.map_pitch;
    uint8_t* tile = smem;
    uint8_t* mmap = smem + Z.map_off;                            // map column = 4 * gx + k + 4, map row = y + 1
    uint16_t* ent = (uint16_t*)(smem + Z.ent_off) + wave * Z.ent_cap;
    uint16_t* pxl = (uint16_t*)(smem + Z.px_off) + wave * kPxCap;
    uint16_t* corners = (uint16_t*)(smem + Z.corner_off) + wave * Z.corner_cap;
    uint32_t* bits = (uint32_t*)(smem + Z.bits_off);
    uint32_t* pre = (uint32_t*)(smem + Z.pre_off);
    const int WPC = Z.wpc;

    // ---- tile load (16-B chunks; the pyramid rows are 64-B aligned): chunk i = tid + 256 * k is chunk i % nch of tile row i / nch.
    // A thread issues the loads of a group of three chunks back to back (a chunk past the end is the last one again, so no load sits
    // behind a branch) and stores what it owns after ONE wait.  Under the first group's loads: the clears.  (Strips of 640 x 480
    // frames are one group; ten chunks per thread is the most the host accepts: 133 rows of 18.) ----
    const int n_chunk = th * nch;
    uint4 c0, c1, c2;
    uint32_t d0, d1, d2;
    auto issue = [&](const int k, uint32_t& dst) {
        const uint32_t i = (uint32_t)min(tid + 256 * k, n_chunk - 1);
        // (24-bit multiplies: i < 4096, inv_nch <= 65536, r < 256, the pitches below 2^23)
        const uint32_t r = __umul24(i, inv_nch) >> 16, q = i - __umul24(r, (uint32_t)nch);
        dst = __umul24(r, (uint32_t)TP) + 16u * q;
        return *(const uint4*)(img + (__umul24(r, istride) + 16u * q));
    };
    auto land = [&](const int k, const uint32_t dst, const uint4& c) { if (tid + 256 * k < n_chunk) *(uint4*)(tile + dst) = c; };
    c0 = issue(0, d0); c1 = issue(1, d1); c2 = issue(2, d2);
    {   // (the host pads both regions to whole 16-byte stores)
        const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
        for (int i = tid; i < ((ih + 2) * MP + 15) >> 4; i += 256) ((uint4*)mmap)[i] = zero;
        for (int i = tid; i < (ncell * WPC + 3) >> 2; i += 256) ((uint4*)bits)[i] = zero;
    }
    if (wave == 0 && lane < kStripTabChunks) ((uint4*)&s_tab)[lane] = tab_chunk;
    land(0, d0, c0); land(1, d1, c1); land(2, d2, c2);
    for (int k = 3; 256 * k < n_chunk; k += 3) {
        c0 = issue(k, d0); c1 = issue(k + 1, d1); c2 = issue(k + 2, d2);
        land(k, d0, c0); land(k + 1, d1, c1); land(k + 2, d2, c2);
    }
    __syncthreads();

    ORBX_FTICK(0)
#if defined(ORBX_FAST_CUT) && ORBX_FAST_CUT == 0
    return;
#endif
    // nms + bit of one pixel (map column mc, row y): the reference's cv::FAST non-maximum suppression inside the cell sub-image
    auto nms_pixel = [&](const int y, const int mc, const int t, const int cA, const int cB) {
        const uint8_t* p = mmap + (y + 1) * MP + mc;
        const int m = p[0];
        const int j = s_tab.colcell[mc];
        if (m > t && j >= cA && j < cB) {
            const int xl = mc - s_tab.cx0[j], iw = s_tab.iw[j];
            // neighbours outside the cell interior count as 0, and so do those that are no corners at t: the pixel survives when its
            // score beats the largest of the eight (branch-free: a short-circuit chain costs a branch per neighbour in SIMD)
            const bool hl = xl > 0, hr = xl < iw - 1, hu = y > 0, hd = y < ih - 1;
            // (the map has a halo row above and below and margin columns: all eight reads are in bounds, then masked)
            const int r0 = p[-MP - 1], r1 = p[-MP], r2 = p[-MP + 1], r3 = p[-1], r4 = p[1], r5 = p[MP - 1], r6 = p[MP], r7 = p[MP + 1];
            const int n0 = (hu && hl) ? r0 : 0, n1 = hu ? r1 : 0, n2 = (hu && hr) ? r2 : 0;
            const int n3 = hl ? r3 : 0, n4 = hr ? r4 : 0;
            const int n5 = (hd && hl) ? r5 : 0, n6 = hd ? r6 : 0, n7 = (hd && hr) ? r7 : 0;
            const int nmax = max(max(max(n0, n1), max(n2, n3)), max(max(n4, n5), max(n6, n7)));
            // a neighbour n counts with its response n - 1 when n > t, else 0:  s = m - 1 > (nmax > t ? nmax - 1 : 0)
            const bool keep = (m - 1) > ((nmax > t) ? nmax - 1 : 0);
            if (keep) { const int q = y * iw + xl; atomicOr(&bits[j * WPC + (q >> 5)], 1u << (q & 31)); }
        }
    };
    // emission of one pixel if its bit is set
    auto emit_pixel = [&](const int y, const int mc, const int cA, const int cB) {
        const int j = s_tab.colcell[mc];
        if (j >= cA && j < cB) {
            const int iw = s_tab.iw[j], q = y * iw + (mc - s_tab.cx0[j]);
            const uint32_t wd = bits[j * WPC + (q >> 5)];
            if ((wd >> (q & 31)) & 1u) {
                const int rk = (int)pre[j * WPC + (q >> 5)] + __popc(wd & ((1u << (q & 31)) - 1u));
                const int m = mmap[(y + 1) * MP + mc];
                // coordinates relative to minBorder (= level coordinates - 16), as vToDistributeKeys holds them (:865-866)
                // k_octree depends on this order: its tie-break between keys of equal response (oct_cand_rank, orbx_kernels.hip)
                // recomputes a key's place in it from the coordinates alone -- cells in table order (row-major, pitch wCell x hCell,
                // interiors from 3 px inside the cell), rank rk row-major inside the cell's interior.  Change one, change the other.
                if (rk < s_tab.slot_cap[j])
                    cand[(size_t)frame * cand_frame_stride + s_tab.slot_off[j] + rk] =
                        pack_key((uint32_t)(4 * g0 + mc - 4 - 16), (uint32_t)(sy0 + 3 + y - 16), (uint32_t)(m - 1));
            }
        }
    };

    int ncorner = 0;                // wave-uniform: corners this wave found in the current phase (> corner_cap: overflow)
    int gA = 0, ng = 1;             // active quads of the current phase

    // the quads that hold the columns of the cells [cA, cB)
    auto set_cols = [&](const int cA, const int cB) {
        const int mA = s_tab.cx0[cA], mB = s_tab.cx0[cB - 1] + s_tab.iw[cB - 1] - 1;       // first / last active map column
        gA = (mA - 4) >> 2;
        ng = ((mB - 4) >> 2) - gA + 1;
    };
    const int nrow_w = (ih - wave + 3) >> 2;              // the wave's rows: wave, wave + 4, ...
    // stage 1 of cv::FAST(cell, t, true) over the active quads of the wave's rows: the entries join the wave's list behind the nent
    // it holds; returns the new length
    auto stage1 = [&](const int t, int nent) {
        const int n_items = nrow_w * ng;
        {
            const uint32_t T2 = (uint32_t)t | ((uint32_t)t << 16);
            const int q64 = 64 / ng, r64 = 64 - q64 * ng;     // 64 items further on: q64 rows down, r64 quads right
            int ry = (int)(((float)lane + 0.5f) * (1.0f / (float)ng)), gx = lane - ry * ng;
            for (int base = 0; base < n_items; base += 64) {
                uint32_t entry = 0;
                if (base + lane < n_items) {
                    const int y = 4 * ry + wave;
                    const uint32_t* row = (const uint32_t*)(tile + (y + 3) * TP + qoff) + gA + gx;       // the quad's own dword
                    const int pd = TP >> 2;
                    const uint32_t cur = row[0], prv = row[-1], nxt = row[1], up3 = row[-3 * pd], dn3 = row[3 * pd];
                    // pixels (0, 2) and (1, 3) of the quad as 2 x u16 each
                    const us2 ce = as_us2(__builtin_amdgcn_perm(0u, cur, 0x0C020C00u)), co = as_us2(__builtin_amdgcn_perm(0u, cur, 0x0C030C01u));
                    const us2 r0e = as_us2(__builtin_amdgcn_perm(0u, dn3, 0x0C020C00u)), r0o = as_us2(__builtin_amdgcn_perm(0u, dn3, 0x0C030C01u));
                    const us2 r8e = as_us2(__builtin_amdgcn_perm(0u, up3, 0x0C020C00u)), r8o = as_us2(__builtin_amdgcn_perm(0u, up3, 0x0C030C01u));
                    // ring 4 = columns +3: pixels 0, 2 -> bytes cur[3], nxt[1]; pixels 1, 3 -> nxt[0], nxt[2]   (perm: bytes 0-3 = 2nd operand)
                    const us2 r4e = as_us2(__builtin_amdgcn_perm(nxt, cur, 0x0C050C03u)), r4o = as_us2(__builtin_amdgcn_perm(nxt, cur, 0x0C060C04u));
                    // ring 12 = columns -3: pixels 0, 2 -> prv[1], prv[3]; pixels 1, 3 -> prv[2], cur[0]
                    const us2 r12e = as_us2(__builtin_amdgcn_perm(cur, prv, 0x0C030C01u)), r12o = as_us2(__builtin_amdgcn_perm(cur, prv, 0x0C040C02u));
                    const us2 T2v = as_us2(T2);
                    const us2 lo_e = __builtin_elementwise_sub_sat(ce, T2v), lo_o = __builtin_elementwise_sub_sat(co, T2v);     // max(v - t, 0)
                    const us2 hi_e = ce + T2v, hi_o = co + T2v;
                    const us2 dk_e = __builtin_elementwise_max(__builtin_elementwise_min(r0e, r8e), __builtin_elementwise_min(r4e, r12e));
                    const us2 dk_o = __builtin_elementwise_max(__builtin_elementwise_min(r0o, r8o), __builtin_elementwise_min(r4o, r12o));
                    const us2 br_e = __builtin_elementwise_min(__builtin_elementwise_max(r0e, r8e), __builtin_elementwise_max(r4e, r12e));
                    const us2 br_o = __builtin_elementwise_min(__builtin_elementwise_max(r0o, r8o), __builtin_elementwise_max(r4o, r12o));
                    // non-zero half = candidate:  sat(lo - dk) != 0 <=> dk < v - t;  sat(br - hi) != 0 <=> br > v + t
                    const uint32_t c_e = as_u32(__builtin_elementwise_sub_sat(lo_e, dk_e)) | as_u32(__builtin_elementwise_sub_sat(br_e, hi_e));
                    const uint32_t c_o = as_u32(__builtin_elementwise_sub_sat(lo_o, dk_o)) | as_u32(__builtin_elementwise_sub_sat(br_o, hi_o));
                    uint32_t m_e, m_o;           // min(c, 1) per half (the compiler would expand a C-level min into compares and selects)
                    asm("v_pk_min_u16 %0, %1, %2" : "=v"(m_e) : "v"(c_e), "v"(0x00010001u));
                    asm("v_pk_min_u16 %0, %1, %2" : "=v"(m_o) : "v"(c_o), "v"(0x00010001u));
                    const uint32_t mw = m_e | (m_o << 1);                 // bit 0: pixel 0, bit 1: pixel 1, bit 16: pixel 2, bit 17: pixel 3
                    // 16-bit entry: pixels 0..3 -> bits 0..3, row index of the wave -> bits 4..8 (< 32), quad -> bits 9..14 (< 64)
                    if (mw) entry = (mw & 3u) | ((mw >> 14) & 0xCu) | ((uint32_t)ry << 4) | ((uint32_t)gx << 9) | 0x8000u;
                }
                const unsigned long long bal = __ballot(entry != 0u);
                if (entry) ent[nent + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u))] = (uint16_t)entry;
                nent += __popcll(bal);
                gx += r64; ry += q64;
                if (gx >= ng) { gx -= ng; ry++; }
            }
        }
        wave_lds_fence();
        return nent;
    };
    // expand + stage 2 over nent entries, which may come from all four waves' lists: entry i is entry i + (d & 0xFFFF) of the lists'
    // block and was listed by wave d >> 16, d = d0 below c1, d1 below c2, d2 below c3, d3 from there; the corners join the wave's list
    const uint16_t* ent_all = (const uint16_t*)(smem + Z.ent_off);
    auto stage2 = [&](const int t, const int nent, const int c1, const int c2, const int c3, const int d0, const int d1, const int d2, const int d3) {
        for (int e0 = 0; e0 < nent; e0 += kEntBatch) {
            const int e1 = min(e0 + kEntBatch, nent);
            int npx = 0;
            for (int base = e0; base < e1; base += 64) {
                const int i = base + lane;
                int d = d0;
                d = i >= c1 ? d1 : d; d = i >= c2 ? d2 : d; d = i >= c3 ? d3 : d;
                const uint32_t en = (i < e1) ? (uint32_t)ent_all[i + (d & 0xFFFF)] | ((uint32_t)d & 0x30000u) : 0u;
                const int cnt = __popc(en & 0xFu);
                const int incl = wave_incl_scan(cnt);
                if (cnt) {
                    const uint32_t id = ((((en >> 4) & 31u) * 4u + (en >> 16)) << 8) | (((en >> 9) & 63u) << 2);     // (y << 8) | (4 * gx)
                    int p = npx + incl - cnt;
                    if (en & 1u) pxl[p++] = (uint16_t)(id | 0u);
                    if (en & 2u) pxl[p++] = (uint16_t)(id | 1u);
                    if (en & 4u) pxl[p++] = (uint16_t)(id | 2u);
                    if (en & 8u) pxl[p++] = (uint16_t)(id | 3u);
                }
                npx += __builtin_amdgcn_readlane(incl, 63);
            }
            wave_lds_fence();
            for (int base = 0; base < npx; base += 64) {
                const int i = base + lane;
                bool corner = false;
                int id = 0;
                if (i < npx) {
                    id = pxl[i];
                    const int y = id >> 8, xq = (id & 0xFF) + 4 * gA;             // xq = 4 * (gA + gx) + k
                    id = (y << 8) | xq;
                    const int m = fast_m_tree(tile + (y + 3) * TP + qoff + xq, TP);
                    mmap[(y + 1) * MP + xq + 4] = (uint8_t)m;
                    corner = m > t;
                }
                const unsigned long long bal = __ballot(corner);
                const int at = ncorner + (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(bal >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)bal, 0u));
                if (corner && at < Z.corner_cap) corners[at] = (uint16_t)id;
                ncorner += __popcll(bal);
            }
            wave_lds_fence();
        }
    };
    // nms or emission over the wave's corners -- or, after an overflow, over every pixel of the active quads of the nrows rows
    // y0, y0 + ystep, ... that the list was made from
    auto for_corners = [&](const int y0, const int ystep, const int nrows, auto&& fn) {
        if (ncorner <= Z.corner_cap) {
            for (int base = 0; base < ncorner; base += 64) {
                const int i = base + lane;
                if (i < ncorner) { const int id = corners[i]; fn(id >> 8, (id & 0xFF) + 4); }
            }
        } else {
            const int wpx = 4 * ng, n = nrows * wpx;
            const float inv = 1.0f / (float)wpx;
            for (int i = lane; i < n; i += 64) {
                const int ry = (int)(((float)i + 0.5f) * inv), xq = 4 * gA + i - ry * wpx;
                fn(ystep * ry + y0, xq + 4);
            }
        }
    };
    // exclusive prefix of the word popcounts of cell j's mask, by one wave
    auto rank_cell = [&](const int j) {
        const int nwords = (s_tab.iw[j] * ih + 31) >> 5;
        int run = 0;
        for (int w0 = 0; w0 < nwords; w0 += 64) {
            const int i = w0 + lane;
            const int my = (i < nwords) ? __popc(bits[j * WPC + i]) : 0;
            const int incl = wave_incl_scan(my);
            if (i < nwords) pre[j * WPC + i] = (uint32_t)(run + incl - my);
            run += __builtin_amdgcn_readlane(incl, 63);
        }
        if (lane == 0) s_total[j] = run;
    };
    // ---- iniThFAST over the whole strip ----
    uint32_t fb_cells = 0u;         // workgroup-uniform: bit j = cell j found nothing at iniThFAST
    set_cols(0, ncell);
    {
        const int nent = stage1(ini_th, 0);
        ORBX_FTICK(1)
#if !defined(ORBX_FAST_CUT) || ORBX_FAST_CUT >= 2
        const int d = (wave * Z.ent_cap) | (wave << 16);         // the wave's own list
        stage2(ini_th, nent, nent, nent, nent, d, d, d, d);
#endif
    }
    ORBX_FTICK(2)
#if !defined(ORBX_FAST_CUT) || ORBX_FAST_CUT >= 3
    __syncthreads();                                              // every wave's scores are in the map
    ORBX_FTICK(3)
    for_corners(wave, 4, nrow_w, [&](int y, int mc) { nms_pixel(y, mc, ini_th, 0, ncell); });
    __syncthreads();                                              // every winner's bit is set
    ORBX_FTICK(4)
    for (int j = wave; j < ncell; j += 4) rank_cell(j);
    __syncthreads();
    ORBX_FTICK(5)
    // (read here, between two barriers: the owner of a fallback cell writes s_total[j] again after the next one)
    fb_cells = (uint32_t)__ballot(lane < ncell && s_total[min(lane, kStripMaxCells - 1)] == 0);
    for_corners(wave, 4, nrow_w, [&](int y, int mc) { emit_pixel(y, mc, 0, ncell); });
    ORBX_FTICK(6)
#endif
#if defined(ORBX_FAST_CUT)      // instruction-budget experiments (tools/fast_cuts.sh): the kernel ends after a prefix of its stages
    if (ini_th >= 0) return;
#endif
#ifdef ORBX_FAST_TIMING
    fallback_slot = 8;
#endif
    // ---- per cell without a single keypoint, minThFAST (:843-846).  The quick test, which is wide, is shared out like the first
    // one: every wave lists the entries of its rows, one segment per fallback cell (its entry list is its own and free by now).
    // Everything behind it is small (a handful of corners per cell), so after ONE barrier the k-th fallback cell is the work of wave
    // k & 3 alone: it expands the cell's segment of all four lists, scores, suppresses, ranks and emits, ordered by its own LDS queue.
    // That is safe because a cell is self-contained: the suppression masks everything outside its interior, and its mask words, prefix
    // words, total and the map bytes of its columns are written by its owner only (a quad shared with the neighbour cell gets the
    // same scores from both owners, in bytes of their own). ----
    if (fb_cells) {
        int k = 0, nent = 0;
        if (lane == 0) s_seg[wave][0] = 0;
        for (uint32_t rest = fb_cells; rest; rest &= rest - 1u, k++) {
            const int j = __builtin_ctz(rest);
            set_cols(j, j + 1);
            nent = stage1(min_th, nent);
            if (lane == 0) s_seg[wave][k + 1] = nent;
        }
        ORBX_FTICK(1)
        // every wave's entries and segment ends are in LDS -- and no wave is still emitting from the iniThFAST pass (its overflow
        // scan reads every cell's mask, which the owners are about to write)
        __syncthreads();
        ORBX_FTICK(3)
        k = 0;
        for (uint32_t rest = fb_cells; rest; rest &= rest - 1u, k++) {
            if ((k & 3) != wave) continue;
            const int j = __builtin_ctz(rest);
#ifdef ORBX_FAST_TIMING
            if (threadIdx.x == 0) atomicAdd(&d_fast_prof[15], 1ull);
#endif
            set_cols(j, j + 1);
            // entry i of the cell = entry i + d[w] of wave w's list, w = the number of c[] that i has reached
            auto seg = [&](int w, int kk) { return __builtin_amdgcn_readfirstlane(s_seg[w][kk]); };          // (uniform: into SGPRs)
            const int b0 = seg(0, k), b1 = seg(1, k), b2 = seg(2, k), b3 = seg(3, k);
            const int c1 = seg(0, k + 1) - b0, c2 = c1 + seg(1, k + 1) - b1, c3 = c2 + seg(2, k + 1) - b2, n = c3 + seg(3, k + 1) - b3;
            const int d0 = b0, d1 = (Z.ent_cap + b1 - c1) | (1 << 16), d2 = (2 * Z.ent_cap + b2 - c2) | (2 << 16), d3 = (3 * Z.ent_cap + b3 - c3) | (3 << 16);
            ncorner = 0;
            stage2(min_th, n, c1, c2, c3, d0, d1, d2, d3);
            ORBX_FTICK(2)
            for_corners(0, 1, ih, [&](int y, int mc) { nms_pixel(y, mc, min_th, j, j + 1); });
            wave_lds_fence();
            ORBX_FTICK(4)
            rank_cell(j);
            wave_lds_fence();
            ORBX_FTICK(5)
            for_corners(0, 1, ih, [&](int y, int mc) { emit_pixel(y, mc, j, j + 1); });
            ORBX_FTICK(6)
        }
    }
    __syncthreads();
    if (tid < ncell) cell_count[(size_t)frame * n_cells + cell0 + tid] = min(s_total[tid], s_tab.slot_cap[tid]);
}
