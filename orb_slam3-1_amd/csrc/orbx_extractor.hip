// orbx_extractor.hip -- host driver + C ABI of the gfx950 ORB extractor.
//
// Mirrors ORB_SLAM3::ORBextractor (reference include/ORBextractor.h:44-109, src/ORBextractor.cc):
// constructor tables on the host (E0), then one fixed sequence of kernel launches per batch of
// frames (orbx_kernels.hip).  No CPU compute path exists: without a HIP device every entry point fails.
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "hip_check.h"
#include "orbx_kernels.hip"

namespace orbx {

thread_local std::string g_last_error;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

static inline int cv_round_host(double v) { return (int)std::nearbyint(v); }
static inline int cv_floor_host(double v) { int i = (int)v; return i - (i > v); }
static inline int round_up(int v, int a) { return (v + a - 1) / a * a; }
constexpr int kResizeFrames = 4;       // frames across the lanes of a wave of the table-driven resize (resize_band's F)
// a lane reaches its frame of the group with a 32-bit byte offset
static inline bool resize_frames_fit(size_t frame_stride) { return (uint64_t)kResizeFrames * frame_stride < ((uint64_t)1 << 31); }
static inline short sat_short(float v) { int iv = (int)std::nearbyintf(v); return (short)std::min(std::max(iv, -32768), 32767); }

// The per-row tables of cv::resize INTER_LINEAR 8UC1 from src_h to dst_h rows: yofs / ib as OpenCV builds
// them, and `rows`, what the table-driven kernels read -- the source rows clamped to the image, the coefficients as the kernels
// multiply them (b << 12) and the reuse plan of resize_band (ResizeRow::plan, on the clamped rows), padded to whole tiles of
// kResizeRows rows with copies of the last row.  *sums_ok: b0 + b1 <= 2048 in every row (the unclamped form is exact).
static int build_resize_rows(int src_h, int dst_h, std::vector<int>& yofs, std::vector<short>& ib, std::vector<ResizeRow>& rows, bool* sums_ok)
{
    const double scale_y = 1. / ((double)dst_h / src_h);
    yofs.assign(dst_h, 0); ib.assign((size_t)dst_h * 2, 0);
    for (int dy = 0; dy < dst_h; dy++) {
        float fy = (float)((dy + 0.5) * scale_y - 0.5);
        int sy = cv_floor_host(fy);
        fy -= sy;
        yofs[dy] = sy;
        ib[2 * dy] = sat_short((1.f - fy) * 2048);
        ib[2 * dy + 1] = sat_short(fy * 2048);
    }
    rows.assign((size_t)round_up(dst_h, kResizeRows), ResizeRow());
    *sums_ok = true;
    int p0 = -1, p1 = -1;               // the previous row's clamped source rows
    for (size_t dy = 0; dy < rows.size(); dy++) {
        const int y = std::min((int)dy, dst_h - 1);
        const int sy0 = std::min(std::max(yofs[y], 0), src_h - 1), sy1 = std::min(std::max(yofs[y] + 1, 0), src_h - 1);
        if (ib[2 * y] < 0 || ib[2 * y] > 2048 || ib[2 * y + 1] < 0 || ib[2 * y + 1] > 2048)
            return fail(ORBX_ERR_INTERNAL, "resize table: row coefficients %d %d", ib[2 * y], ib[2 * y + 1]);
        if (ib[2 * y] + ib[2 * y + 1] > 2048) *sums_ok = false;
        rows[dy].sy = (uint32_t)sy0 | ((uint32_t)sy1 << 16);
        rows[dy].b0 = (uint32_t)ib[2 * y] << 12; rows[dy].b1 = (uint32_t)ib[2 * y + 1] << 12;
        rows[dy].plan = (sy0 == p1 ? kResizeTopPrevBottom : (sy0 == p0 ? kResizeTopPrevTop : kResizeTopFresh)) | (sy1 == sy0 ? kResizeBottomIsTop : 0u);
        p0 = sy0; p1 = sy1;
    }
    return ORBX_OK;
}

// getGaussianKernelFixedPoint_ED (OpenCV 4.x): Q8.8 taps, error diffusion, centre = 256 - 2*sum(others)
static void gauss_taps_q8(int n, double sigma, int* taps)
{
    std::vector<double> k(n);
    const double scale2x = -0.5 / (sigma * sigma);
    double sum = 0;
    for (int i = 0; i < n; i++) { const double x = i - (n - 1) * 0.5; k[i] = std::exp(scale2x * x * x); sum += k[i]; }
    sum = 1. / sum;
    double err = 0;
    long long acc = 0;
    for (int i = 0; i < n / 2; i++) {
        const double adj = k[i] * sum * 256.0 + err;
        const long long v0 = cv_round_host(adj);
        err = adj - (double)v0;
        taps[i] = taps[n - 1 - i] = (int)v0;
        acc += v0;
    }
    taps[n / 2] = (int)(256 - 2 * acc);
}

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t n = 0;
    int ensure(size_t count)
    {
        if (count <= n) return ORBX_OK;
        if (p) { (void)hipFree(p); p = nullptr; n = 0; }
        ORBX_HIP(hipMalloc((void**)&p, count * sizeof(T)));
        n = count;
        return ORBX_OK;
    }
    int upload(const std::vector<T>& v)
    {
        int r = ensure(v.size() ? v.size() : 1);
        if (r) return r;
        if (!v.empty()) ORBX_HIP(hipMemcpy(p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice));
        return ORBX_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; n = 0; }
};

// the blur's tiles of a w x h level, appended in row-major order (k_blur: kBlurTW x kBlurTH outputs per workgroup)
static void append_blur_tiles(int level, int w, int h, std::vector<TileDesc>& tiles)
{
    for (int y0 = 0; y0 < h; y0 += kBlurTH)
        for (int x0 = 0; x0 < w; x0 += kBlurTW) {
            TileDesc t; t.level = (int16_t)level; t.x0 = (int16_t)x0; t.y0 = (int16_t)y0;
            // (the 7 taps of the tile's last column, x0 + 63, reach column x0 + 66)
            t.edge = (int16_t)((x0 == 0 ? 1 : 0) | (w <= x0 + kBlurTW + 2 ? 2 : 0));
            tiles.push_back(t);
        }
}

// Two blur launches by level range: tiles[0, *split) must be exactly the tiles of the levels below `level` and tiles[*split, n) exactly
// those from `level` on.  False when the list is not in level order (no such cut exists).
static bool blur_tile_split(const std::vector<TileDesc>& tiles, int level, int* split)
{
    size_t t = 0;
    while (t < tiles.size() && tiles[t].level < level) t++;
    *split = (int)t;
    for (; t < tiles.size(); t++) if (tiles[t].level < level) return false;
    return true;
}

}  // namespace orbx

using namespace orbx;

struct orbx_extractor {
    int device = 0;
    int nfeatures = 0, nlevels = 0, ini_th = 0, min_th = 0;
    float scale_factor_f = 0;
    double scale_factor_d = 0;           // the reference member is a double (include/ORBextractor.h:92)
    std::vector<float> scale, inv_scale, sigma2, inv_sigma2;
    std::vector<int> nfeat;
    int taps[7];
    int max_kp = 0;

    // geometry for the current image size
    int geo_w = 0, geo_h = 0;
    std::vector<LevelDesc> levels;
    std::vector<CellDesc> cells;
    std::vector<TileDesc> tiles;
    size_t pyr_frame_bytes = 0;
    int cand_frame_entries = 0, sel_frame_entries = 0;
    std::vector<StripDesc> strips;       // FAST work items: runs of adjacent cells of one cell row
    std::vector<StripRec> strip_recs;    // ... and what the kernel reads of each: one record per strip, in the same order
    FastLds fast_layout;
    int fast_corner_cap = 0;             // 0 = kCornerCap; tests shrink it to drive the overflow path (orbx_debug_set_fast_corner_cap)
    size_t fast_lds = 0, oct_lds = 0;
    int oct_pool = 0, oct_lds_keys = 0, oct_small_keys = 0;
    bool oct_nodes_hbm = false;          // the octree's node pool does not fit LDS: it lives in d_oct_nodes
    size_t oct_node_stride = 0;
    size_t oct_small_lds = 0;
    int oct_dyn_keys = 0;                // k_octree_dyn (batches up to oct_dyn_max_batch frames whose levels' worst-case key buffers do not fit LDS): keys that do
    size_t oct_dyn_lds = 0;
    bool oct_keys_forced = false;

    DevBuf<LevelDesc> d_levels;
    DevBuf<CellDesc> d_cells;
    DevBuf<TileDesc> d_tiles;
    DevBuf<StripRec> d_strips;
    // the octree's bucket tables (OctTabDesc): per level the depth, and the boundaries of its cells
    std::vector<OctTabDesc> oct_tabs;
    std::vector<int16_t> oct_bounds;
    std::vector<uint16_t> oct_maps;
    DevBuf<OctTabDesc> d_oct_tabs;
    DevBuf<int16_t> d_oct_bounds;        // (the kernel reads the maps; the boundaries they are made from are kept for orbx_debug_octree_table)
    DevBuf<uint16_t> d_oct_maps;
    size_t oct_prefix_frame = 0;         // prefix sums per frame, all levels
    int oct_tab_depth_max = kOctTabMaxDepth;     // ORBX_OCT_TAB_DEPTH (tests: a shallow table sends the divides below it through the partition code)
    // resize tables per destination level: per quad of columns the first source column, 4 v_perm selectors, 4 coefficient pairs
    // and per destination row the two source rows and the two coefficients (ResizeRow)
    std::vector<DevBuf<int> > d_qsx0;
    std::vector<DevBuf<uint4> > d_qsel, d_qalpha;
    std::vector<DevBuf<ResizeRow> > d_rows;
    std::vector<DevBuf<int> > d_xofs, d_yofs;    // per-column / per-row tables of the levels that take k_resize_generic (resize_generic[l])
    std::vector<DevBuf<short> > d_ialpha, d_ibeta;
    std::vector<uint8_t> resize_generic;
    std::vector<uint8_t> resize_sat;     // levels whose coefficient sums do not prove the clamp to 255 dead: the saturating kernels

    // per-batch scratch
    int batch_cap = 0, last_batch = 0;
    DevBuf<uint8_t> d_pyr, d_blur;
    DevBuf<uint32_t> d_cand, d_scratch, d_sel;
    DevBuf<uint8_t> d_oct_nodes;
    DevBuf<int> d_oct_prefix;
    DevBuf<int> d_cell_count, d_sel_count, d_kp_dst;
    DevBuf<OrbxKeyPoint> d_lvl_kps;
    // staging for the host-pointer API
    DevBuf<OrbxKeyPoint> d_kps;
    DevBuf<uint8_t> d_desc;
    DevBuf<int> d_n, d_mono, d_status;
    DevBuf<int> d_sad;                   // ComputeStereoMatches: SAD of the accepted matches
    DevBuf<uint8_t> d_stereo_io;         // host-buffer variant of the stereo matcher
    int out_cap = 0;
    hipStream_t stream = nullptr;
    // per-stage HIP-event profiling (off by default)
    static constexpr int kProfEvents = 8;
    bool profile = false;
    hipEvent_t prof_ev[kProfEvents] = {};
    int prof_marks = 0;
    hipStream_t prof_stream = nullptr;
    // side stream for the blur (runs beside the latency-bound octree)
    hipStream_t side_stream = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // second stream for the octree of the upper pyramid levels (their node pools are small: own launch, own LDS size)
    hipStream_t oct_stream = nullptr;
    hipEvent_t ev_oct_join = nullptr, ev_fast0 = nullptr, ev_resize = nullptr;
    hipEvent_t ev_tail = nullptr;        // the resize tail's levels are written (a blur of every level on the launch stream reads them: ORBX_BLUR_SPLIT=0)
    int dbg_tail_delay_us = 0;           // tests: a spin kernel in front of the resize tail (orbx_debug_set_tail_delay)
    int last_octree_variant = 0;         // which k_octree instantiation / schedule the last enqueue used (orbx_debug_last_schedule)
    int oct_split = 0, oct_pool_hi = 0;  // levels [oct_split, nlevels) go to the second launch with a pool of oct_pool_hi nodes (0: one launch)
    size_t oct_lds_hi = 0;
    // streams for the ranges a large batch is cut into (enqueue)
    int split_parts = 1;                 // ORBX_SPLIT (measurement knob, see enqueue)
    bool serial_schedule = false;        // ORBX_SERIAL=1: every kernel of a batch on the launch stream, one launch per stage (per-kernel profiles)
    bool last_resize_bands = false;      // the last enqueue resized a level with k_resize (orbx_debug_resize_bands)
    int resize_band_min = 64;            // batches from this size on take k_resize (bands of rows, frames across the lanes), smaller ones k_resize_tiles (ORBX_RESIZE_BAND_MIN)
    int resize_tail_first = 4;           // first pyramid level of the fused resize tail (ORBX_RESIZE_TAIL; 0: a launch per level)
    bool oct_dyn_off = false;            // ORBX_OCT_DYN=0: small batches keep the scratch instantiation (measurement / tests)
    int oct_dyn_max_batch = 64;          // largest batch that takes k_octree_dyn (ORBX_OCT_DYN_MAXB; measured: one frame 0.163 -> 0.136 ms,
                                         // 64 frames 0.412 -> 0.352 ms per call, 256 frames 0.99 -> 1.12 ms: the LDS is the blur's there; LDS keys for the early level-0 launch alone: 0.993 -> 1.008)
    // Waves per octree workgroup (k_octree: one control wave, W - 1 helpers): ORBX_OCT_WAVES = 1 | 2 | 4 forces every launch; otherwise
    // a launch that runs on a mostly empty chip (up to 64 frames) takes 4 and the launches beside FAST / the blur take oct_waves_beside.
    // Measured at B = 256 (ms per step, medians of three; W of the three launches): 1/1/1 0.897, 2/2/2 0.868, 4/4/4 0.912, 4/1/1 0.892,
    // 4/2/2 0.871, 2/1/2 0.900, 2/2/1 0.878, 1/2/2 0.875, 2/2/4 0.925: helpers that wait at a barrier still hold the wave slots that the
    // blur's workgroups need, and two waves per workgroup is where that stops paying.  B = 64: 1 wave 0.315 ms per call, 2 0.299, 4 0.290.
    int oct_waves_env = 0;
    int oct_waves_beside[3] = {2, 2, 2};  // level 0 started early, the lower levels, the upper levels
    // k_octree's lane-per-node threshold for launches of more than one wave (ORBX_OCT_SMALL_MAX; one wave: 32).  Re-measured with
    // helpers: 16 / 8 / 0 leave the B = 256 step where it is (0.868 / 0.868 / 0.868 against 0.868) and take a single frame from 0.115 to
    // 0.107 / 0.105 / 0.103 ms, but the serial octree stage of 64 frames went from 0.23 to 0.67 ms with each of them; not understood, so 32 stays.
    int oct_small_max_waves = 32;
    int last_oct_waves[3] = {0, 0, 0};    // W of the last enqueue's launches, same order; 0: no such launch (orbx_debug_octree_waves)
    int oct_dyn_keys_beside = 6144;      // LDS keys per workgroup when the blur runs beside the octree (batches of 32 frames and more)
    bool resize_beside = true;           // the whole resize chain on the side stream beside FAST on level 0 (ORBX_RESIZE_BESIDE=0: in front of it)
    // Hand-offs of the large-batch schedule (run_range with a blur stream; see the comment there).  Each has a switch, 0 restores
    // the schedule without it:
    bool blur_split = true;              // ORBX_BLUR_SPLIT: the blur in two launches by level range, the tail's levels on the tail's queue
                                         // behind FAST on them; no wait for the resize tail on the launch stream
    bool bind_records = true;            // ORBX_BIND_RECORDS: an event that follows a launch is that launch's stop event, not a marker of its own
    bool status_in_fast = true;          // ORBX_STATUS_IN_FAST: the first FAST launch clears the status words, no fill kernel in front of it
    int blur_split_tile = 0;             // first blur tile of level resize_tail_first (setup_geometry; tiles are in level order)
    int last_handoffs = 0;               // which of them the last enqueue used (orbx_debug_last_handoffs)
    std::vector<hipStream_t> aux_streams;
    hipEvent_t ev_parts_fork = nullptr;
    std::vector<hipEvent_t> ev_parts_join;

    int setup_geometry(int w, int h);
    int ensure_batch(int batch);
    int enqueue(const uint8_t* d_imgs, bool level0_ready, int batch, int row_stride, size_t frame_stride,
                int lap0, int lap1, OrbxKeyPoint* o_kps, uint8_t* o_desc, int cap, int* o_n, int* o_mono, int* o_status,
                hipStream_t st);
    int launch_orient_desc(int f0, int n_frames, hipStream_t s, OrbxKeyPoint* o_kps, uint8_t* o_desc, int cap);
};

// E0: constructor tables (reference src/ORBextractor.cc:409-445)
static void build_tables(orbx_extractor* e)
{
    const int nl = e->nlevels;
    e->scale.assign(nl, 1.0f); e->sigma2.assign(nl, 1.0f); e->inv_scale.resize(nl); e->inv_sigma2.resize(nl);
    for (int i = 1; i < nl; i++) {
        e->scale[i] = (float)(e->scale[i - 1] * e->scale_factor_d);
        e->sigma2[i] = e->scale[i] * e->scale[i];
    }
    for (int i = 0; i < nl; i++) {
        e->inv_scale[i] = 1.0f / e->scale[i];
        e->inv_sigma2[i] = 1.0f / e->sigma2[i];
    }
    e->nfeat.resize(nl);
    const float factor = (float)(1.0f / e->scale_factor_d);
    float per_scale = e->nfeatures * (1 - factor) / (1 - (float)std::pow((double)factor, (double)nl));
    int sum = 0;
    for (int l = 0; l < nl - 1; l++) {
        e->nfeat[l] = (int)std::nearbyintf(per_scale);
        sum += e->nfeat[l];
        per_scale *= factor;
    }
    e->nfeat[nl - 1] = std::max(e->nfeatures - sum, 0);
    e->max_kp = 0;
    // per level the octree returns at most N + 3 nodes -- except that its FIRST pass divides every root without looking at N
    // (src/ORBextractor.cc:606-672: the size test follows the pass), so a level with a tiny budget still returns up to 4 nodes per root
    // (nIni = round(width / height) roots; 8 roots = images up to 8.5 : 1 are covered by this bound, wider ones report ORBX_ERR_CAPACITY)
    for (int l = 0; l < nl; l++) e->max_kp += std::max(e->nfeat[l] + 3, 32);
    gauss_taps_q8(7, 2.0, e->taps);
}

// The boundaries of the 2^depth cells that DivideNode's ceil-halving (src/ORBextractor.cc:480-486; oct_node_box on the device) cuts
// [lo, hi) into when it is applied `depth` times: out[0 .. 2^depth].  A box narrower than 2^depth repeats boundaries (empty cells).
static void oct_cell_bounds(int lo, int hi, int depth, int16_t* out)
{
    out[0] = (int16_t)lo; out[1 << depth] = (int16_t)hi;
    for (int step = 1 << depth; step > 1; step >>= 1)
        for (int i = 0; i < (1 << depth); i += step) {
            const int a = out[i], b = out[i + step];
            out[i + step / 2] = (int16_t)(a + ((b - a + 1) >> 1));
        }
}

int orbx_extractor::setup_geometry(int w, int h)
{
    if (w == geo_w && h == geo_h) return ORBX_OK;
    geo_w = geo_h = 0;          // (a failure below leaves no geometry: the tables are rebuilt by the next call, whatever its size)
    levels.assign(nlevels, LevelDesc());
    oct_tabs.assign(nlevels, OctTabDesc());
    oct_bounds.clear();
    oct_maps.clear();
    cells.clear();
    tiles.clear();
    strips.clear();
    strip_recs.clear();
    size_t off = 0;
    int cand_off = 0, sel_off = 0, max_tw = 0, max_th = 0, max_nfeat = 0;
    std::vector<int> node_need(nlevels, 0);
    d_qsx0.resize(nlevels); d_yofs.resize(nlevels); d_qsel.resize(nlevels); d_qalpha.resize(nlevels); d_ibeta.resize(nlevels); d_rows.resize(nlevels);
    d_xofs.resize(nlevels); d_ialpha.resize(nlevels); resize_generic.assign(nlevels, 0); resize_sat.assign(nlevels, 0);
    for (int l = 0; l < nlevels; l++) {
        LevelDesc& L = levels[l];
        L.w = (int)std::nearbyintf((float)w * inv_scale[l]);      // ComputePyramid :1175
        L.h = (int)std::nearbyintf((float)h * inv_scale[l]);
        if (L.w < 1 || L.h < 1) return fail(ORBX_ERR_ARG, "pyramid level %d of a %dx%d image is empty", l, w, h);
        if (L.w > 4096 + 32 || L.h > 4096 + 32) return fail(ORBX_ERR_ARG, "image %dx%d too large (keys are 12-bit)", w, h);
        L.stride = round_up(L.w, 64);
        L.off = (int64_t)off;
        off += (size_t)L.stride * L.h;
        off = (off + 255) & ~(size_t)255;
        L.nfeat = nfeat[l];
        L.scale = scale[l];
        L.patch_size = (int)(kPatch * scale[l]);
        {   // (see build_tables: N + 3, or what the first pass makes of the roots when the level's budget is tiny)
            const int bw = (L.w - kEdge + 3) - (kEdge - 3), bh = (L.h - kEdge + 3) - (kEdge - 3);
            const int n_ini = bh > 0 ? (int)std::roundf((float)bw / (float)bh) : 0;
            L.sel_off = sel_off; L.sel_cap = std::max({nfeat[l] + 3, 32, 4 * std::max(n_ini, 0)});
            node_need[l] = std::max(nfeat[l], 4 * std::max(n_ini, 0));         // nodes the level's list can hold at once (+ 16 below)
        }
        sel_off += (L.sel_cap + 1) & ~1;        // even: the two key points of a wave of k_orient_desc share a level
        max_nfeat = std::max(max_nfeat, node_need[l]);
        // FAST cells (ComputeKeyPointsOctTree :787-822)
        L.cell_begin = (int)cells.size();
        L.cand_off = cand_off;
        const int minBX = kEdge - 3, minBY = minBX, maxBX = L.w - kEdge + 3, maxBY = L.h - kEdge + 3;
        const float width = (float)(maxBX - minBX), height = (float)(maxBY - minBY);
        const int nCols = (int)(width / 35.f), nRows = (int)(height / 35.f);
        int cell_pitch_x = 4096, cell_pitch_y = 4096;           // (a level without FAST cells has no key to rank)
        if (nCols > 0 && nRows > 0) {
            const int wCell = (int)std::ceil(width / nCols), hCell = (int)std::ceil(height / nRows);
            cell_pitch_x = std::max(wCell, 2); cell_pitch_y = std::max(hCell, 2);
            for (int i = 0; i < nRows; i++) {
                const float iniY = (float)(minBY + i * hCell);
                float maxY = iniY + hCell + 6;
                if (iniY >= maxBY - 3) continue;
                if (maxY > maxBY) maxY = (float)maxBY;
                for (int j = 0; j < nCols; j++) {
                    const float iniX = (float)(minBX + j * wCell);
                    float maxX = iniX + wCell + 6;
                    if (iniX >= maxBX - 6) continue;
                    if (maxX > maxBX) maxX = (float)maxBX;
                    CellDesc c;
                    c.level = (int16_t)l;
                    c.x0 = (int16_t)iniX; c.x1 = (int16_t)maxX; c.y0 = (int16_t)iniY; c.y1 = (int16_t)maxY;
                    const int iw = c.x1 - c.x0 - 6, ih = c.y1 - c.y0 - 6;
                    if (iw <= 0 || ih <= 0) continue;       // cv::FAST finds nothing in a sub-image thinner than 7 px
                    c.slot_off = cand_off;
                    c.slot_cap = ((iw + 1) / 2) * ((ih + 1) / 2);     // 3x3 NMS: no two 8-adjacent survivors
                    cand_off += c.slot_cap;
                    max_tw = std::max(max_tw, c.x1 - c.x0);
                    max_th = std::max(max_th, c.y1 - c.y0);
                    cells.push_back(c);
                }
            }
        }
        L.cell_count = (int)cells.size() - L.cell_begin;
        L.cand_cap = cand_off - L.cand_off;
        {   // the pitch's reciprocal for oct_cand_rank, exact for every coordinate of the level.  ceil(2^20 / pitch) is exact for
            // v * (pitch - 1) < 2^20, i.e. up to about 15 000 px at pitches of 35-70; levels are at most 4 128 px (keys are 12-bit,
            // checked above), so the loop below is a guard that cannot trip today.
            auto inv = [](int pitch) { return (int)(((1u << 20) + (uint32_t)pitch - 1u) / (uint32_t)pitch); };
            oct_tabs[l].w_cell_inv = inv(cell_pitch_x); oct_tabs[l].h_cell_inv = inv(cell_pitch_y);
            for (int v = 0; v < std::max(L.w, L.h); v++)
                if ((int)(((uint32_t)v * (uint32_t)oct_tabs[l].w_cell_inv) >> 20) != v / cell_pitch_x || (int)(((uint32_t)v * (uint32_t)oct_tabs[l].h_cell_inv) >> 20) != v / cell_pitch_y)
                    return fail(ORBX_ERR_INTERNAL, "level %d: FAST cell of coordinate %d is not exact as a multiplication", l, v);
        }
        // strips: the cells of a cell row are adjacent (interiors tile the row); cut every row into runs of at most
        // kStripMaxCells cells and about kStripWidth columns, evenly
        for (int c0 = L.cell_begin; c0 < (int)cells.size();) {
            int c1 = c0 + 1;
            while (c1 < (int)cells.size() && cells[c1].y0 == cells[c0].y0) c1++;
            const int n_row = c1 - c0;
            const int w_cell = std::max(cells[c0].x1 - cells[c0].x0 - 6, 1);
            static const int strip_width = getenv("ORBX_STRIP_WIDTH") ? std::max(48, std::min(atoi(getenv("ORBX_STRIP_WIDTH")), 250)) : kStripWidth;
            const int per = std::max(1, std::min(kStripMaxCells, (strip_width - 6) / w_cell));
            const int n_strips_row = (n_row + per - 1) / per;
            for (int k = 0; k < n_strips_row; k++) {
                const int a = c0 + (int)((long long)n_row * k / n_strips_row), b = c0 + (int)((long long)n_row * (k + 1) / n_strips_row);
                StripDesc sd;
                sd.level = (int16_t)l; sd.cell0 = (int16_t)a; sd.ncell = (int16_t)(b - a);
                sd.x0 = cells[a].x0; sd.x1 = cells[b - 1].x1; sd.y0 = cells[a].y0; sd.y1 = cells[a].y1; sd.pad = 0;
                strips.push_back(sd);
            }
            c0 = c1;
        }
        // blur tiles
        append_blur_tiles(l, L.w, L.h, tiles);
        // resize tables (cv::resize INTER_LINEAR 8UC1); level l is made from level l-1
        if (l > 0) {
            const LevelDesc& P = levels[l - 1];
            const double scale_x = 1. / ((double)L.w / P.w);
            const int wpad = round_up(L.w, 4);          // k_resize reads 4 entries per 16-B load
            std::vector<int> xofs(wpad, 0), yofs;
            std::vector<short> ia((size_t)wpad * 2, 0), ib;
            auto sat = sat_short;
            bool sums_ok = true;                        // a0 + a1 <= 2048 in every column and b0 + b1 <= 2048 in every row
            for (int dx = 0; dx < L.w; dx++) {
                float fx = (float)((dx + 0.5) * scale_x - 0.5);
                int sx = cv_floor_host(fx);
                fx -= sx;
                if (sx < 0) { fx = 0; sx = 0; }
                if (sx >= P.w - 1) { fx = 0; sx = P.w - 1; }
                xofs[dx] = sx;
                ia[2 * dx] = sat((1.f - fx) * 2048);
                ia[2 * dx + 1] = sat(fx * 2048);
                if (ia[2 * dx] < 0 || ia[2 * dx + 1] < 0 || ia[2 * dx] + ia[2 * dx + 1] > 2048) sums_ok = false;
            }
            // per quad of destination columns (k_resize): sx0, selectors of (S[sx], S[sx+1]) inside the 8 bytes from sx0 on,
            // coefficient pairs; columns past the level's width get coefficient 0 (they land in the row padding as 0)
            const int nq = wpad / 4;
            std::vector<int> qsx0(nq);
            std::vector<uint4> qsel(nq), qal(nq);
            for (int q = 0; q < nq; q++) {
                qsx0[q] = xofs[4 * q];
                uint32_t se[4], al[4];
                for (int k = 0; k < 4; k++) {
                    const int dx = 4 * q + k;
                    if (dx < L.w) {
                        const int o = xofs[dx] - qsx0[q];
                        if (o < 0) return fail(ORBX_ERR_INTERNAL, "resize table: source offset %d", o);
                        if (o > 6) { resize_generic[l] = 1; se[k] = 0x0C0C0C0Cu; al[k] = 0u; continue; }     // scale factors >= 2: the level takes k_resize_generic
                        se[k] = (uint32_t)o | 0x0C000C00u | ((uint32_t)(o + 1) << 16);
                        al[k] = (uint32_t)(uint16_t)ia[2 * dx] | ((uint32_t)(uint16_t)ia[2 * dx + 1] << 16);
                    } else { se[k] = 0x0C0C0C0Cu; al[k] = 0u; }
                }
                qsel[q] = make_uint4(se[0], se[1], se[2], se[3]);
                qal[q] = make_uint4(al[0], al[1], al[2], al[3]);
            }
            // per destination row: the clamped source rows, the shifted coefficients and the reuse plan (build_resize_rows)
            std::vector<ResizeRow> rows;
            bool rows_ok = true;
            if (int rr = build_resize_rows(P.h, L.h, yofs, ib, rows, &rows_ok)) return rr;
            // the kernels drop the clamp to 255 where both coefficient sums prove it dead; a level that fails keeps the saturating form
            resize_sat[l] = !(sums_ok && rows_ok);
            int r;
            if (resize_generic[l] && ((r = d_xofs[l].upload(xofs)) || (r = d_ialpha[l].upload(ia)) || (r = d_yofs[l].upload(yofs)) || (r = d_ibeta[l].upload(ib)))) return r;
            if ((r = d_qsx0[l].upload(qsx0)) || (r = d_qsel[l].upload(qsel)) || (r = d_qalpha[l].upload(qal)) || (r = d_rows[l].upload(rows))) return r;
        }
    }
    pyr_frame_bytes = off;
    // (k_resize and k_blur address the levels of one frame with 32-bit byte offsets)
    if (off >= ((size_t)1 << 31)) return fail(ORBX_ERR_ARG, "the pyramid of a %dx%d image exceeds 2 GiB per frame", w, h);
    cand_frame_entries = std::max(cand_off, 1);
    sel_frame_entries = sel_off;
    // FAST kernel LDS: sized for the largest strip (orbx_fast_strips.inc)
    {
        if (cells.size() > 32767) return fail(ORBX_ERR_ARG, "%zu FAST cells exceed the strip table's 16-bit cell index", cells.size());
        int max_nch = 1, max_ngx = 1, max_sth = 7, max_ent = 1, max_ncell = 1, max_int = 1;
        for (const StripDesc& sd : strips) {
            const int g0 = (sd.x0 + 3) >> 2, g1 = (sd.x1 - 4) >> 2, ngx = g1 - g0 + 1, sth = sd.y1 - sd.y0, ih = sth - 6;
            if (ngx > 64 || ih > 127) return fail(ORBX_ERR_ARG, "FAST strip of %dx%d px exceeds the 64-quad x 127-row work item index", sd.x1 - sd.x0, sth);
            const int xa = (4 * (g0 - 1)) & ~15, qoff = 4 * g0 - xa;
            max_nch = std::max(max_nch, (qoff + 4 * ngx + 4 + 15) >> 4);
            for (int j = 0; j < sd.ncell; j++) { const CellDesc& c = cells[sd.cell0 + j]; max_int = std::max(max_int, (c.x1 - c.x0 - 6) * ih); }
            max_ngx = std::max(max_ngx, ngx); max_sth = std::max(max_sth, sth);
            // (the minThFAST pass lists the wave's rows cell by cell: a quad that straddles two cells is listed with both)
            max_ent = std::max(max_ent, ((ih + 3) / 4) * (ngx + sd.ncell - 1));
            max_ncell = std::max(max_ncell, (int)sd.ncell);
        }
        if (max_int > 8191) return fail(ORBX_ERR_ARG, "FAST cell interior of %d px exceeds the 8191-px bitmask", max_int);
        FastLds& Z = fast_layout;
        auto al16 = [](size_t v) { return (v + 15) & ~(size_t)15; };
        size_t o = 0;
        Z.tile_pitch = 16 * max_nch;
        o = al16((size_t)max_sth * Z.tile_pitch);
        Z.map_off = (int)o; Z.map_pitch = 4 * max_ngx + 8;
        o = al16(o + (size_t)(max_sth - 6 + 2) * Z.map_pitch);
        Z.ent_cap = (max_ent + 7) & ~7;
        Z.ent_off = (int)o; o = al16(o + 2 * 4 * (size_t)Z.ent_cap);
        Z.px_off = (int)o; o = al16(o + 2 * 4 * (size_t)kPxCap);
        Z.corner_cap = fast_corner_cap > 0 ? fast_corner_cap : kCornerCap;
        Z.corner_off = (int)o; o = al16(o + 2 * 4 * (size_t)Z.corner_cap);
        Z.wpc = (max_int + 31) / 32;
        Z.pre_off = (int)o; o = al16(o + 4 * (size_t)max_ncell * Z.wpc);
        Z.bits_off = (int)o; o = al16(o + 4 * (size_t)max_ncell * Z.wpc);
        Z.total = (int)o;
        fast_lds = o;
        if (fast_lds > 150 * 1024) return fail(ORBX_ERR_ARG, "FAST strip of %d quads x %d rows does not fit LDS", max_ngx, max_sth);
        // the strips' records (orbx_fast_strips.inc: StripRec): what the kernel's set-up would otherwise compute or fetch per workgroup
        strip_recs.assign(strips.size(), StripRec());
        for (size_t si = 0; si < strips.size(); si++) {
            const StripDesc& sd = strips[si];
            const LevelDesc& L = levels[sd.level];
            StripRec& R = strip_recs[si];
            const int g0 = (sd.x0 + 3) >> 2, g1 = (sd.x1 - 4) >> 2, ngx = g1 - g0 + 1;       // first / last image dword that holds a detection column
            const int xa = (4 * (g0 - 1)) & ~15, qoff = 4 * g0 - xa, nch = (qoff + 4 * ngx + 4 + 15) >> 4, sth = sd.y1 - sd.y0;
            R.src_off = (uint32_t)((size_t)L.off + (size_t)sd.y0 * L.stride + xa);          // (the frame is below 2 GiB)
            R.stride = (uint32_t)L.stride;
            auto pair = [](int lo, int hi) { return (uint32_t)lo | ((uint32_t)hi << 16); };
            if (sd.y0 < 0 || xa < 0 || sd.cell0 < 0) return fail(ORBX_ERR_INTERNAL, "FAST strip at row %d, column %d, cell %d", sd.y0, xa, sd.cell0);
            R.y0_xa = pair(sd.y0, xa); R.th_nch = pair(sth, nch); R.g0_qoff = pair(g0, qoff); R.ncell_cell0 = pair(sd.ncell, sd.cell0);
            R.level = (uint32_t)sd.level;
            // chunk i of the tile is chunk i % nch of row i / nch: the division as a multiplication, exact for every chunk of the strip
            R.inv_nch = (65536u + (uint32_t)nch - 1u) / (uint32_t)nch;
            for (uint32_t i = 0; i < (uint32_t)(sth * nch); i++)
                if (((i * R.inv_nch) >> 16) != i / (uint32_t)nch)
                    return fail(ORBX_ERR_INTERNAL, "FAST strip of %d rows x %d chunks: the row of chunk %u is not exact", sth, nch, i);
            std::memset(R.tab.colcell, 0xFF, sizeof(R.tab.colcell));
            for (int j = 0; j < sd.ncell; j++) {
                const CellDesc& c = cells[sd.cell0 + j];
                R.tab.cx0[j] = c.x0 + 3 - 4 * g0 + 4; R.tab.iw[j] = c.x1 - c.x0 - 6;
                R.tab.slot_off[j] = c.slot_off; R.tab.slot_cap[j] = c.slot_cap;
                if (R.tab.cx0[j] < 0 || R.tab.cx0[j] + R.tab.iw[j] > Z.map_pitch)
                    return fail(ORBX_ERR_INTERNAL, "FAST cell columns %d + %d outside the strip's %d map columns", R.tab.cx0[j], R.tab.iw[j], Z.map_pitch);
                for (int i = 0; i < R.tab.iw[j]; i++) R.tab.colcell[R.tab.cx0[j] + i] = (uint8_t)j;
            }
        }
    }
    // octree kernel LDS
    oct_pool = max_nfeat + 16;
    if (oct_pool > 32000) return fail(ORBX_ERR_ARG, "nfeatures per level %d too large for the device octree (16-bit node ids)", max_nfeat);
    const char* env = getenv("ORBX_OCT_LDS_KEYS");
    oct_lds_keys = env ? atoi(env) : 0;      // measured on MI355X: L2-resident HBM scratch + more resident waves beats LDS keys
    oct_keys_forced = env != nullptr;        // ... for large batches; small batches are latency-bound and take LDS keys (enqueue())
    auto pool_bytes = [](int pool) { return (size_t)pool * (2 * sizeof(SortNode) + 8 + 16 + 2 * kOctLogFactor) + (size_t)((pool + 15) & ~15); };
    const size_t node_bytes = pool_bytes(oct_pool);
    // Large batches run the octree beside the blur, and a workgroup's LDS is sized by its launch: with one launch every level
    // would hold the node pool of the largest one (8 levels x 14 KB per frame and CU leave the blur no LDS to run in).  The upper
    // levels -- fewer features each -- therefore get a launch of their own with a pool of their size; the split that minimises
    // the LDS per frame is taken.
    oct_split = 0; oct_pool_hi = 0; oct_lds_hi = 0;
    {
        size_t best = (size_t)nlevels * node_bytes;
        for (int sp = 1; sp < nlevels; sp++) {
            int hi = 0;
            for (int l = sp; l < nlevels; l++) hi = std::max(hi, node_need[l]);
            const size_t cost = (size_t)sp * node_bytes + (size_t)(nlevels - sp) * pool_bytes(hi + 16);
            if (cost < best) { best = cost; oct_split = sp; oct_pool_hi = hi + 16; oct_lds_hi = pool_bytes(hi + 16) + 16; }
        }
    }
    // the node pool of a level lives in LDS (about 2500 nodes); a level with more features takes the instantiation whose pool
    // lives in an HBM scratch (ensure_batch allocates it)
    // the bucket tables: the deepest table that the level's feature budget can use (about four cells per feature: the list ends at N
    // nodes) and whose counters and boundaries fit the level's own node pool, which lends them its bytes while the keys are placed
    oct_prefix_frame = 0;
    for (int l = 0; l < nlevels; l++) {
        const LevelDesc& L = levels[l];
        OctTabDesc& T = oct_tabs[l];
        const int bw = (L.w - kEdge + 3) - (kEdge - 3), bh = (L.h - kEdge + 3) - (kEdge - 3);
        T.n_ini = bh > 0 ? std::max((int)std::roundf((float)bw / (float)bh), 0) : 0;
        T.depth = 0; T.bounds_off = (int)oct_bounds.size(); T.prefix_off = (int)oct_prefix_frame;
        if (T.n_ini < 1) continue;                      // (the kernel returns no key point for such a level)
        if (bw < 1) return fail(ORBX_ERR_INTERNAL, "level %d: %d roots in a tree %d wide", l, T.n_ini, bw);
        const size_t pool_b = pool_bytes(node_need[l] + 16), map_bytes = 2 * (size_t)(bw + bh);
        auto counter_bytes = [&](int d) { return 4 * (((size_t)T.n_ini << (2 * d)) + 1); };
        while (T.depth < oct_tab_depth_max && ((long long)T.n_ini << (2 * T.depth)) < 4LL * L.nfeat &&
               ((size_t)T.n_ini << (2 * (T.depth + 1))) <= 65536 && counter_bytes(T.depth + 1) <= pool_b) T.depth++;
        if (counter_bytes(T.depth) > pool_b) return fail(ORBX_ERR_ARG, "level %d: %d roots do not fit the octree's node pool", l, T.n_ini);
        T.maps_lds = counter_bytes(T.depth) + map_bytes <= pool_b;      // (not with a tiny budget on a large image: the maps stay in global memory)
        const int nb = (1 << T.depth) + 1;
        const float hX = (float)bw / (float)T.n_ini;
        oct_bounds.resize(oct_bounds.size() + (size_t)(T.n_ini + 1) * nb);
        int16_t* xb = oct_bounds.data() + T.bounds_off;
        for (int s = 0; s <= T.n_ini; s++, xb += nb)       // roots (:564-577), then the rows
            if (s < T.n_ini) oct_cell_bounds((int)(hX * (float)s), (int)(hX * (float)(s + 1)), T.depth, xb);
            else oct_cell_bounds(0, bh, T.depth, xb);
        oct_prefix_frame += ((size_t)T.n_ini << (2 * T.depth)) + 1;
        // the maps: a key's root is (int)(x / hX) (:585); inside the root, the quadrant at every depth (x >= midx, y >= midy)
        auto spread = [](int v) { int s = 0; for (int b = 0; b < kOctTabMaxDepth; b++) s |= ((v >> b) & 1) << (2 * b); return s; };
        auto cell_index = [&](const int16_t* b, int v) { int i = 0; for (int d = T.depth - 1; d >= 0; d--) i = 2 * i + (v >= b[(2 * i + 1) << d] ? 1 : 0); return i; };
        T.map_off = (int)oct_maps.size();
        const int16_t* b0 = oct_bounds.data() + T.bounds_off;
        for (int x = 0; x < bw; x++) {
            const int root = std::min(std::max((int)((float)x / hX), 0), T.n_ini - 1);
            oct_maps.push_back((uint16_t)((root << (2 * T.depth)) | spread(cell_index(b0 + root * nb, x))));
        }
        for (int y = 0; y < bh; y++) oct_maps.push_back((uint16_t)(2 * spread(cell_index(b0 + T.n_ini * nb, y))));
    }
    oct_prefix_frame = std::max<size_t>(oct_prefix_frame, 1);
    oct_nodes_hbm = node_bytes > 150 * 1024;
    oct_node_stride = (node_bytes + 255) & ~(size_t)255;
    if (oct_nodes_hbm) oct_lds_keys = 0;
    if (!oct_nodes_hbm && node_bytes + 8 * (size_t)oct_lds_keys > 150 * 1024) oct_lds_keys = (int)((150 * 1024 - node_bytes) / 8);
    if (oct_lds_keys < 0) oct_lds_keys = 0;
    oct_lds = node_bytes + 8 * (size_t)oct_lds_keys + 16;
    // second configuration for small batches: both key buffers of a level (up to 4096 candidates) live in LDS
    int max_cand_cap = 0;
    for (const LevelDesc& lv : levels) max_cand_cap = std::max(max_cand_cap, lv.cand_cap);
    oct_small_keys = max_cand_cap;
    if (oct_nodes_hbm || node_bytes + 8 * (size_t)oct_small_keys > 150 * 1024) oct_small_keys = 0;      // does not fit: small batches use the scratch path too
    oct_small_lds = node_bytes + 8 * (size_t)oct_small_keys + 16;
    if (oct_lds_keys > 0 && oct_lds_keys < max_cand_cap) oct_lds_keys = 0;              // the LDS instantiation needs room for a whole level
    // third configuration, for the smallest batches when a level's worst case does NOT fit: as many keys as LDS holds beside the
    // node pool; the kernel takes the LDS body for every (level, frame) whose actual candidates fit (k_octree_dyn)
    oct_dyn_keys = 0; oct_dyn_lds = 0;
    if (!oct_nodes_hbm && oct_small_keys == 0 && node_bytes + 8 * 2048 <= 150 * 1024) {
        oct_dyn_keys = (int)std::min<size_t>((size_t)max_cand_cap, (150 * 1024 - node_bytes) / 8);
        if (const char* envd = getenv("ORBX_OCT_DYN_KEYS")) oct_dyn_keys = std::max(64, std::min(oct_dyn_keys, atoi(envd)));     // (tests: force the fallback body)
        oct_dyn_lds = node_bytes + 8 * (size_t)oct_dyn_keys + 16;
    }
    if (!oct_nodes_hbm) {
        ORBX_HIP(hipFuncSetAttribute((const void*)k_octree<false>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)node_bytes + 64));
        ORBX_HIP(hipFuncSetAttribute((const void*)k_octree<true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max(oct_lds, oct_small_lds)));
        if (oct_dyn_keys > 0) ORBX_HIP(hipFuncSetAttribute((const void*)k_octree_dyn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)oct_dyn_lds));
    } else {
        oct_lds = 64; oct_small_lds = 64;
    }
    ORBX_HIP(hipFuncSetAttribute((const void*)k_fast_strips, hipFuncAttributeMaxDynamicSharedMemorySize, (int)fast_lds));
    int r;
    if ((r = d_oct_tabs.upload(oct_tabs)) || (r = d_oct_bounds.upload(oct_bounds)) || (r = d_oct_maps.upload(oct_maps))) return r;
    if ((r = d_levels.upload(levels)) || (r = d_cells.upload(cells)) || (r = d_tiles.upload(tiles)) || (r = d_strips.upload(strip_recs))) return r;
    // the blur by level range (enqueue): the tiles of the levels before the resize tail and those of the tail's levels
    blur_split_tile = (int)tiles.size();
    if (resize_tail_first >= 2 && resize_tail_first < nlevels && !blur_tile_split(tiles, resize_tail_first, &blur_split_tile))
        return fail(ORBX_ERR_INTERNAL, "the blur tiles of levels %d.. are not one range of the tile list", resize_tail_first);
    geo_w = w; geo_h = h;
    batch_cap = 0;      // scratch must be re-sized for the new geometry
    return ORBX_OK;
}

int orbx_extractor::ensure_batch(int batch)
{
    if (batch <= batch_cap) return ORBX_OK;
    int r;
    const size_t B = (size_t)batch;
    // + 64: the 16-byte patch chunks of k_orient_desc may start up to 45 bytes right of a key point's last patch column
    if ((r = d_pyr.ensure(B * pyr_frame_bytes + 64)) || (r = d_blur.ensure(B * pyr_frame_bytes + 64)) ||
        (r = d_cand.ensure(B * cand_frame_entries)) || (r = d_scratch.ensure(B * 2 * cand_frame_entries)) ||
        (r = d_sel.ensure(B * sel_frame_entries)) || (r = d_cell_count.ensure(B * std::max<size_t>(cells.size(), 1))) ||
        (r = d_sel_count.ensure(B * nlevels)) || (r = d_kp_dst.ensure(B * sel_frame_entries)) ||
        (r = d_lvl_kps.ensure(B * sel_frame_entries)) || (r = d_n.ensure(B)) || (r = d_mono.ensure(B)) || (r = d_status.ensure(B)))
        return r;
    if (oct_nodes_hbm && (r = d_oct_nodes.ensure(B * nlevels * oct_node_stride))) return r;
    if ((r = d_oct_prefix.ensure(B * oct_prefix_frame))) return r;
    // the pyramid row padding is read by dword loads at row ends; keep it defined
    ORBX_HIP(hipMemset(d_pyr.p, 0, B * pyr_frame_bytes + 64));
    ORBX_HIP(hipMemset(d_blur.p, 0, B * pyr_frame_bytes + 64));
    batch_cap = batch;
    return ORBX_OK;
}

namespace orbx {
// test aid: keeps a stream busy for `ticks` of the 100 MHz wall clock (orbx_debug_set_tail_delay)
__global__ void k_debug_spin(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}
// copies B frames of arbitrary row stride into pyramid level 0 (dword stores, byte loads)
__global__ __launch_bounds__(256) void k_copy_level0(const uint8_t* __restrict__ src, int row_stride, size_t src_frame_stride,
                                                     uint8_t* __restrict__ pyr, size_t frame_stride, LevelDesc L)
{
    const int x4 = (blockIdx.x * blockDim.x + threadIdx.x) * 4;
    const int y = blockIdx.y;
    if (x4 >= L.w) return;
    const uint8_t* s = src + (size_t)blockIdx.z * src_frame_stride + (size_t)y * row_stride + x4;
    uint32_t v = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) if (x4 + k < L.w) v |= (uint32_t)s[k] << (8 * k);
    *(uint32_t*)(pyr + (size_t)blockIdx.z * frame_stride + L.off + (size_t)y * L.stride + x4) = v;
}
}  // namespace orbx

// The one launch of k_orient_desc, for frames [f0, f0 + n_frames) of the batch scratch: the pipeline (enqueue) and the test entry
// orbx_debug_orient_desc both come through here, so the grid expression and the argument list cannot drift apart.  o_kps / o_desc
// are the [batch][cap] outputs of the whole batch.
int orbx_extractor::launch_orient_desc(int f0, int n_frames, hipStream_t s, OrbxKeyPoint* o_kps, uint8_t* o_desc, int cap)
{
    const int quads = (sel_frame_entries + 7) / 8;       // workgroups per frame: 8 key points each (two per wave)
    hipLaunchKernelGGL(k_orient_desc, dim3((unsigned)(((long long)quads * n_frames + 7) / 8 * 8)), dim3(256), 0, s,
                       d_pyr.p + (size_t)f0 * pyr_frame_bytes, d_blur.p + (size_t)f0 * pyr_frame_bytes, pyr_frame_bytes,
                       d_levels.p, nlevels, d_sel.p + (size_t)f0 * sel_frame_entries, sel_frame_entries, d_sel_count.p + (size_t)f0 * nlevels,
                       d_kp_dst.p + (size_t)f0 * sel_frame_entries, sel_frame_entries,
                       o_kps + (size_t)f0 * cap, o_desc + (size_t)f0 * cap * 32, cap, d_lvl_kps.p + (size_t)f0 * sel_frame_entries, quads, n_frames);
    const hipError_t le = hipGetLastError();
    if (le != hipSuccess) return fail(ORBX_ERR_HIP, "launch of k_orient_desc: %s", hipGetErrorString(le));
    return ORBX_OK;
}

int orbx_extractor::enqueue(const uint8_t* d_imgs, bool level0_ready, int batch, int row_stride, size_t frame_stride,
                            int lap0, int lap1, OrbxKeyPoint* o_kps, uint8_t* o_desc, int cap, int* o_n, int* o_mono, int* o_status,
                            hipStream_t st)
{
    const int B = batch;
    // optional per-stage timing with HIP events on the launch stream (bench.py roofline leg)
    int mark_i = 0;
    auto mark = [&]() { if (profile && mark_i < kProfEvents) (void)hipEventRecord(prof_ev[mark_i++], st); };
#define ORBX_LAUNCHED(name) do { const hipError_t le_ = hipGetLastError(); if (le_ != hipSuccess) return fail(ORBX_ERR_HIP, "launch of %s: %s", name, hipGetErrorString(le_)); } while (0)
    // Level 0 is the caller's image.  When its rows can be read with aligned 16-byte loads it is used in place: the resize to
    // level 1, FAST and the blur read it where it lies, and the blur -- which touches every pixel anyway -- leaves the copy in
    // the pyramid that the later readers of level 0 (descriptors, stereo matching, orbx_pyramid_level) use.  Otherwise it is
    // copied first (k_copy_level0), as it is when the host-pointer entry points have uploaded it into the pyramid themselves.
    // (... and when a tile's rows are within 32-bit offsets of its first one, as k_fast_strips addresses them)
    const bool in_place = !level0_ready && ((uintptr_t)d_imgs % 16 == 0) && (row_stride % 16 == 0) && (frame_stride % 16 == 0) && row_stride < (1 << 23);
    const int n_cells = (int)cells.size();
    // Optionally (ORBX_SPLIT=2..4) a large batch is cut into ranges, each on a stream of its own, so that one range's latency-bound
    // stages (octree, the dependent resize launches) could hide behind the others' FAST / blur / descriptors.  Measured on MI355X
    // (B = 256, round 2): 1 range 1.344 ms per step, 2 ranges 1.348, 3 ranges 1.637, 4 ranges 1.649 -- the blur beside the octree
    // already fills the idle chip and whole-chip kernels of different streams do not co-run, so the default stays ONE range.
    int parts = 1;
    if (!profile && split_parts > 1 && B >= 32 * split_parts) parts = std::min(split_parts, 1 + (int)aux_streams.size());
    // (small batches: the blur is a few microseconds, less than the fork / join across streams costs)
    hipStream_t side_q = (parts == 1 && !profile && !serial_schedule && side_stream && B >= 32) ? side_stream : nullptr;
    // first level of the fused resize tail for a range of nB frames (nlevels: none), and the first FAST strip of its levels
    // (resize_tail_first: the levels from there on are one launch, a workgroup per frame -- k_resize_tail)
    // (only with many frames: a single workgroup walks a small batch's levels slower than one wide launch per level does)
    auto tail_plan = [&](int nB, int& l_tail, int& tail_strip) {
        l_tail = (nB >= 64 && resize_tail_first >= 2 && resize_tail_first < nlevels) ? resize_tail_first : nlevels;
        for (int l = l_tail; l < nlevels; l++) if (resize_generic[l]) l_tail = nlevels;      // (the fused tail only knows the table-driven kernel)
        tail_strip = (int)strips.size();        // (the strips are in level order)
        for (int si = (int)strips.size() - 1; si >= 0 && strips[si].level >= l_tail; si--) tail_strip = si;
    };
    // The status words are cleared by the first kernel of the launch stream where that is FAST on the lowest levels: the large-batch
    // schedule with the resize tail beside it (run_range below), level 0 in place.  Every writer of a non-zero status (k_octree,
    // k_index) runs behind an event recorded after that launch or after a later one of the launch stream.  Elsewhere: a fill.
    bool status_by_fast = false;
    if (status_in_fast && side_q && oct_stream && n_cells > 0 && (level0_ready || in_place)) {
        int lt, ts;
        tail_plan(B, lt, ts);
        status_by_fast = lt < nlevels && ts > 0;
    }
    if (!status_by_fast) ORBX_HIP(hipMemsetAsync(o_status, 0, sizeof(int) * B, st));
    int handoffs = status_by_fast ? 4 : 0;

    // One range of frames [f0, f0 + nB) through the whole pipeline on stream `s`; the blur either on `blur_s` beside the octree
    // (a single range: the octree is one wave per frame and level and leaves most of the chip idle) or on `s` itself.
    auto run_range = [&](int f0, int nB, hipStream_t s, hipStream_t blur_s, bool marks) -> int {
        uint8_t* pyr = d_pyr.p + (size_t)f0 * pyr_frame_bytes;
        uint8_t* blr = d_blur.p + (size_t)f0 * pyr_frame_bytes;
        SrcImage lvl0;
        lvl0.base = nullptr; lvl0.frame_stride = 0; lvl0.stride = 0; lvl0.w = levels[0].w; lvl0.h = levels[0].h;
        if (in_place) { lvl0.base = d_imgs + (size_t)f0 * frame_stride; lvl0.frame_stride = frame_stride; lvl0.stride = row_stride; }
        if (marks) mark();
        if (!level0_ready && !in_place) {
            const LevelDesc& L0 = levels[0];
            dim3 g((L0.w / 4 + 255) / 256, L0.h, nB);
            hipLaunchKernelGGL(k_copy_level0, g, dim3(256), 0, s, d_imgs + (size_t)f0 * frame_stride, row_stride, frame_stride, pyr, pyr_frame_bytes, L0);
            ORBX_LAUNCHED("k_copy_level0");
        }
        if (marks) mark();
        int l_tail, tail_strip;
        tail_plan(nB, l_tail, tail_strip);
        // Launches `kern` on queue `q` and, with `ev`, records `ev` behind it.  Such a record publishes nothing but "this kernel has
        // finished", so the event is made the launch's own stop event (hipExtLaunchKernelGGL) and no marker packet is enqueued.
        // (Measured, DESIGN.md 5i: the next kernel of the queue starts 5.5 us behind a kernel that carries an event instead of 7 us
        // behind the marker -- most of the hand-off is the completion signal, not the packet -- and the step gains 7 us over its
        // six records, the largest share of the three hand-off changes.)
        auto launch_ev = [&](hipEvent_t ev, auto kern, dim3 grid, dim3 block, size_t lds, hipStream_t q, auto... args) -> hipError_t {
            if (ev && bind_records) {
                hipExtLaunchKernelGGL(kern, grid, block, (uint32_t)lds, q, nullptr, ev, 0, args...);
                handoffs |= 2;
                return hipSuccess;
            }
            hipLaunchKernelGGL(kern, grid, block, lds, q, args...);
            return ev ? hipEventRecord(ev, q) : hipSuccess;
        };
        // FAST on level 0 needs no resized level, so the whole resize chain (levels 1 .. and the tail) runs on the side stream beside
        // it; `s` waits for the levels before the tail (ev_resize) in front of FAST on levels 1 ..  (1.005 -> 0.991 ms per 256-frame
        // step.  Measured and dropped in the same session: the blur on a stream of its own right behind the resize chain, beside
        // FAST -- two issue-bound whole-chip kernels side by side: 1.10 ms.)
        const bool chain_beside = resize_beside && blur_s && oct_stream && n_cells > 0 && l_tail < nlevels && l_tail > 1 &&
                                  !strips.empty() && strips[0].level == 0;
        hipStream_t rs = chain_beside ? oct_stream : s;
        if (chain_beside) { ORBX_HIP(hipEventRecord(ev_fork, s)); ORBX_HIP(hipStreamWaitEvent(rs, ev_fork, 0)); }
        bool resize_bands = false;          // a level went through k_resize (orbx_debug_resize_bands)
        for (int l = 1; l < l_tail; l++) {
            const LevelDesc& D = levels[l];
            const LevelDesc& P = levels[l - 1];
            SrcImage src;
            src.base = pyr + P.off; src.frame_stride = pyr_frame_bytes; src.stride = P.stride; src.w = P.w; src.h = P.h;
            if (l == 1 && in_place) src = lvl0;
            const hipEvent_t ev = (chain_beside && l == l_tail - 1) ? ev_resize : nullptr;      // the chain's last launch: the levels before the tail are written
            if (resize_generic[l]) {
                ORBX_HIP(launch_ev(ev, k_resize_generic, dim3((D.w + 255) / 256, D.h, nB), dim3(256), 0, rs, src, pyr, pyr_frame_bytes, D,
                                   d_xofs[l].p, d_ialpha[l].p, d_yofs[l].p, d_ibeta[l].p));
                ORBX_LAUNCHED("k_resize_generic");
                continue;
            }
            if (nB < resize_band_min) {          // few frames: short waves, a workgroup per tile and frame
                dim3 g(xcd_grid(((D.w + kResizeTileW - 1) / kResizeTileW) * ((D.h + kResizeRows - 1) / kResizeRows)), nB);
                ORBX_HIP(launch_ev(ev, resize_sat[l] ? k_resize_tiles<true> : k_resize_tiles<false>, g, dim3(256), 0, rs, src, pyr, pyr_frame_bytes, D,
                                   d_qsx0[l].p, d_qsel[l].p, d_qalpha[l].p, d_rows[l].p));
                ORBX_LAUNCHED("k_resize_tiles");
                continue;
            }
            // four frames across the lanes of a wave where a lane reaches all four with a 32-bit offset, in the source (level 1 read
            // in place: the caller's frame stride) and in the pyramid; batches below four frames and larger frames: one frame per wave
            const int F = (nB >= 4 && resize_frames_fit(src.frame_stride) && resize_frames_fit(pyr_frame_bytes)) ? kResizeFrames : 1;
            dim3 g(xcd_grid(((D.w + resize_strip_w(F) - 1) / resize_strip_w(F)) * ((D.h + kResizeRows - 1) / kResizeRows)), (nB + F - 1) / F);
            auto kern = F == 1 ? (resize_sat[l] ? k_resize<1, true> : k_resize<1, false>) : (resize_sat[l] ? k_resize<kResizeFrames, true> : k_resize<kResizeFrames, false>);
            ORBX_HIP(launch_ev(ev, kern, g, dim3(256), 0, rs, src, pyr, pyr_frame_bytes, D, nB, d_qsx0[l].p, d_qsel[l].p, d_qalpha[l].p, d_rows[l].p));
            resize_bands = true;
            ORBX_LAUNCHED("k_resize");
        }
        // The octree is one wave per (level, frame).  With few frames the chip is empty anyway and a wave's latency is the
        // whole stage: keep the ping-pong key buffers in LDS (no L2 round trip per DivideNode).  With many frames the larger
        // LDS footprint would halve the resident waves, and the L2-resident scratch wins.
        const bool small_batch = !oct_keys_forced && oct_small_keys > 0 && (long long)B * nlevels <= 512;
        // (one wave per level and frame: below 32 frames every workgroup has a CU of its own, LDS is free)
        const bool dyn_keys = !oct_keys_forced && !small_batch && oct_dyn_keys > 0 && B <= oct_dyn_max_batch && !oct_dyn_off;
        // (with the blur beside the octree -- 32 frames and more -- a workgroup takes a smaller share of its CU's LDS)
        const int dyn_k = (blur_s && B >= 32) ? std::min(oct_dyn_keys, oct_dyn_keys_beside) : oct_dyn_keys;
        const size_t o_lds = small_batch ? oct_small_lds : (dyn_keys ? oct_dyn_lds - 8 * (size_t)(oct_dyn_keys - dyn_k) : oct_lds);
        const int o_keys = small_batch ? oct_small_keys : (dyn_keys ? dyn_k : oct_lds_keys);
        uint32_t* sel = d_sel.p + (size_t)f0 * sel_frame_entries;
        int* sel_cnt = d_sel_count.p + (size_t)f0 * nlevels;
        int* kp_dst = d_kp_dst.p + (size_t)f0 * sel_frame_entries;
        auto oct_kernel = oct_nodes_hbm ? k_octree<false, false> : (dyn_keys ? k_octree_dyn : (o_keys > 0 ? k_octree<true, true> : k_octree<false, true>));
        // (keys in LDS: one launch, the buffers are sized for the largest level anyway)
        const bool two_launches = !oct_nodes_hbm && (o_keys == 0 || dyn_keys) && oct_split > 0 && oct_stream && blur_s;
        const int lv_lo = two_launches ? oct_split : nlevels;
        // `which`: 0 level 0 started early, 1 the lower levels (or all of them), 2 the upper levels
        const bool oct_beside = B > 64;                  // the launch shares a full chip: with FAST / the blur, or with its own 2 000 workgroups
        last_oct_waves[0] = last_oct_waves[1] = last_oct_waves[2] = 0;
        // (the launches below take an event to record behind them, see launch_ev; a launch of nothing still records it)
        auto launch_octree = [&](hipStream_t qs, int lv0, int lv1, size_t lds, int pool, int keys, int which, hipEvent_t ev) -> hipError_t {
            const int W = oct_waves_env ? oct_waves_env : (oct_beside ? oct_waves_beside[which] : 4);
            if (lv1 <= lv0) return ev ? hipEventRecord(ev, qs) : hipSuccess;
            last_oct_waves[which] = W;
            return launch_ev(ev, oct_kernel, dim3(lv1 - lv0, nB), dim3(64 * W), lds, qs, d_levels.p, d_cells.p, d_cand.p + (size_t)f0 * cand_frame_entries, (size_t)cand_frame_entries,
                             d_cell_count.p + (size_t)f0 * std::max<size_t>(cells.size(), 1), n_cells, d_scratch.p + (size_t)f0 * 2 * cand_frame_entries, (size_t)2 * cand_frame_entries, pool, keys,
                             sel, sel_frame_entries, sel_cnt, nlevels, o_status + f0,
                             d_oct_nodes.p ? d_oct_nodes.p + (size_t)f0 * nlevels * oct_node_stride : nullptr, oct_node_stride, lv0, W > 1 ? oct_small_max_waves : 32,
                             d_oct_tabs.p, d_oct_maps.p, d_oct_prefix.p + (size_t)f0 * oct_prefix_frame, oct_prefix_frame);
        };
        // the blur of tiles [t0, t1): a range of levels (the tiles are in level order).  The launch that blurs level 0 also leaves its
        // in-place copy in the pyramid.
        auto launch_blur = [&](hipStream_t bs, int t0, int t1, hipEvent_t ev) -> hipError_t {
            if (t1 <= t0) return ev ? hipEventRecord(ev, bs) : hipSuccess;
            return launch_ev(ev, k_blur, dim3(xcd_grid(t1 - t0), nB), dim3(256), 0, bs, lvl0, pyr, (in_place && t0 == 0) ? pyr : nullptr, blr, pyr_frame_bytes,
                             d_levels.p, d_tiles.p + t0, t1 - t0, taps[0], taps[1], taps[2], taps[3]);
        };
        const int n_tiles = (int)tiles.size();
        bool oct0_early = false;            // level 0's octree already runs beside FAST on the levels above it (below)
        bool tail_beside = false;           // the resize tail ran on oct_stream: its levels are ordered before their blur (below)
        uint32_t* cand = d_cand.p + (size_t)f0 * cand_frame_entries;
        int* cell_cnt = d_cell_count.p + (size_t)f0 * std::max<size_t>(cells.size(), 1);
        bool clear_pending = status_by_fast;        // the first FAST launch of the launch stream clears the status words
        auto launch_fast = [&](hipStream_t fs, int s0, int s1, hipEvent_t ev) -> hipError_t {
            if (s1 <= s0) return ev ? hipEventRecord(ev, fs) : hipSuccess;
            int* clear = (clear_pending && fs == s) ? o_status + f0 : nullptr;
            if (clear) clear_pending = false;
            return launch_ev(ev, k_fast_strips, dim3(xcd_grid(s1 - s0), nB), dim3(256), fast_lds, fs, lvl0, pyr, pyr_frame_bytes,
                             d_strips.p + s0, s1 - s0, n_cells, ini_th, min_th, fast_layout, cand, (size_t)cand_frame_entries, cell_cnt, clear);
        };
        // With side streams the resize tail -- one latency-bound workgroup per frame -- and FAST on its levels run BESIDE FAST on the
        // lower levels (which only need the levels before the tail) instead of in front of it.
        const bool beside = l_tail < nlevels && blur_s && oct_stream && n_cells > 0 && tail_strip > 0;
        // The blur in two launches by level range (ORBX_BLUR_SPLIT): the levels before the tail on the launch stream directly behind
        // FAST -- which has waited for them (ev_resize) --, the tail's levels on the tail's own queue behind FAST on them, where queue
        // order puts them behind k_resize_tail: that queue idles there while FAST on the lower levels finishes.  The launch stream
        // then never waits for the tail.  k_orient_desc is ordered behind the second launch by the join that FAST on the tail's levels
        // already has: blur (oct_stream) -> the first ev_oct_join -> blur_s waits for it in front of its octree and of k_index ->
        // k_index -> ev_join -> s waits for it in front of k_orient_desc.
        // (Measured and dropped: the second launch behind the upper levels' octree, the phase in which the one blur runs -- k_index then
        // starts behind it and ends after the launch stream's blur, the join moves back; slower than one blur)
        const bool blur_ranges = blur_split && beside && l_tail == resize_tail_first && blur_split_tile > 0 && blur_split_tile < n_tiles;
        bool fork_recorded = false;         // ev_fork already follows the launch stream's last FAST launch
        if (l_tail < nlevels) {
            ResizeTables T;
            std::memset(&T, 0, sizeof(T));
            for (int l = l_tail; l < nlevels; l++) { T.q_sx0[l] = d_qsx0[l].p; T.q_sel[l] = d_qsel[l].p; T.q_alpha[l] = d_qalpha[l].p; T.rows[l] = d_rows[l].p; }
            hipStream_t ts = beside ? oct_stream : s;
            if (beside && !chain_beside) { ORBX_HIP(hipEventRecord(ev_fork, s)); ORBX_HIP(hipStreamWaitEvent(ts, ev_fork, 0)); }
            if (dbg_tail_delay_us > 0) hipLaunchKernelGGL(k_debug_spin, dim3(1), dim3(64), 0, ts, (long long)dbg_tail_delay_us * 100);
            bool tail_sat = false;
            for (int l = l_tail; l < nlevels; l++) tail_sat = tail_sat || resize_sat[l];
            // one blur on `s` reads EVERY level: it has to wait for the tail's levels (ev_tail; FAST on them may still run).  With the
            // blur by level range nobody outside this queue reads them before the join.
            ORBX_HIP(launch_ev((beside && !blur_ranges) ? ev_tail : nullptr, tail_sat ? k_resize_tail<true> : k_resize_tail<false>, dim3(nB), dim3(1024), 0, ts,
                               pyr, pyr_frame_bytes, d_levels.p, T, l_tail, nlevels));
            ORBX_LAUNCHED("k_resize_tail");
            if (beside) {
                tail_beside = true;
                ORBX_HIP(launch_fast(ts, tail_strip, (int)strips.size(), blur_ranges ? nullptr : ev_oct_join));
                if (blur_ranges) ORBX_HIP(launch_blur(ts, blur_split_tile, n_tiles, ev_oct_join));
                // FAST on level 0 first; its octree -- the longest chain of the stage -- then runs beside FAST on levels 1..
                // (a launch per level with every level's octree started early was measured too: the extra launch tails cost
                // FAST 40 us, more than the octrees gain)
                // The launch stream's last FAST launch carries ev_fork, which starts the octrees.
                int l1_strip = tail_strip;
                for (int si = tail_strip - 1; si >= 0 && strips[si].level >= 1; si--) l1_strip = si;
                if (two_launches && oct_split > 1 && l1_strip > 0 && l1_strip < tail_strip) {
                    ORBX_HIP(launch_fast(s, 0, l1_strip, ev_fast0));
                    ORBX_HIP(hipStreamWaitEvent(blur_s, ev_fast0, 0));
                    ORBX_HIP(launch_octree(blur_s, 0, 1, o_lds, oct_pool, o_keys, 0, nullptr));
                    oct0_early = true;
                    if (chain_beside) ORBX_HIP(hipStreamWaitEvent(s, ev_resize, 0));
                    ORBX_HIP(launch_fast(s, l1_strip, tail_strip, ev_fork));
                } else if (chain_beside && l1_strip > 0 && l1_strip < tail_strip) {
                    ORBX_HIP(launch_fast(s, 0, l1_strip, nullptr));
                    ORBX_HIP(hipStreamWaitEvent(s, ev_resize, 0));
                    ORBX_HIP(launch_fast(s, l1_strip, tail_strip, ev_fork));
                } else {
                    if (chain_beside) ORBX_HIP(hipStreamWaitEvent(s, ev_resize, 0));
                    ORBX_HIP(launch_fast(s, 0, tail_strip, ev_fork));
                }
                fork_recorded = true;
                ORBX_HIP(hipStreamWaitEvent(blur_s, ev_oct_join, 0));
            } else {
                if (marks) mark();
                if (n_cells > 0) ORBX_HIP(launch_fast(s, 0, (int)strips.size(), nullptr));
            }
        } else {
            if (marks) mark();
            if (n_cells > 0) ORBX_HIP(launch_fast(s, 0, (int)strips.size(), nullptr));
        }
        ORBX_LAUNCHED("k_fast_strips");
        if (clear_pending) return fail(ORBX_ERR_INTERNAL, "no FAST launch on the launch stream took the status clear");
        if (marks) mark();
        // With a side stream the throughput-bound blur stays on the launch stream (it starts the moment FAST ends) and the
        // latency-bound octree + index go beside it: octree of the lower levels and the index on `blur_s`, the upper levels'
        // octree on `oct_stream`.  Without one (profiling) everything is serial on `s`.
        // The queues of the large-batch schedule, and what orders them (a hand-off between queues costs the waiting queue 5 - 13 us
        // also when the event completed long ago, so the launch stream -- the queue the caller waits on -- takes as few as it can):
        //   s           [status fill, unless FAST clears it] ev_fork | FAST level 0 +ev_fast0 | wait ev_resize | FAST levels 1 .. tail
        //               +ev_fork | blur of the levels before the tail | wait ev_join | k_orient_desc
        //   oct_stream  wait ev_fork | k_resize x (tail - 1) +ev_resize | k_resize_tail | FAST on the tail's levels | blur of the tail's
        //               levels +ev_oct_join | wait ev_fork | octree of the upper levels +ev_oct_join
        //   blur_s      wait ev_fast0 | octree of level 0 | wait ev_oct_join (FAST and blur of the tail's levels) | wait ev_fork |
        //               octree of the lower levels | wait ev_oct_join | k_index +ev_join
        // "+ev": the event is the stop event of that launch (launch_ev).
        hipStream_t os = blur_s ? blur_s : s;
        if (blur_s) {
            if (!fork_recorded) ORBX_HIP(hipEventRecord(ev_fork, s));
            ORBX_HIP(hipStreamWaitEvent(blur_s, ev_fork, 0));
        }
        if (two_launches) {
            ORBX_HIP(hipStreamWaitEvent(oct_stream, ev_fork, 0));
            {   // (dynamic LDS keys: the upper levels hold fewer candidates -- half the allotment)
                const int k_hi = dyn_keys ? std::max(64, o_keys / 2) : 0;
                ORBX_HIP(launch_octree(oct_stream, oct_split, nlevels, oct_lds_hi + 8 * (size_t)k_hi, oct_pool_hi, k_hi, 2, ev_oct_join));
            }
        }
        ORBX_HIP(launch_octree(os, oct0_early ? 1 : 0, lv_lo, o_lds, oct_pool, o_keys, 1, nullptr));
        if (blur_s) {
            if (blur_ranges) ORBX_HIP(launch_blur(s, 0, blur_split_tile, nullptr));
            else {
                if (tail_beside) ORBX_HIP(hipStreamWaitEvent(s, ev_tail, 0));
                ORBX_HIP(launch_blur(s, 0, n_tiles, nullptr));
            }
        }
        if (blur_ranges) handoffs |= 1;
        last_octree_variant = (oct_nodes_hbm ? 0 : (dyn_keys ? 3 : (o_keys > 0 ? 1 : 2))) | (two_launches ? 4 : 0) | (oct0_early ? 8 : 0) | (in_place ? 16 : 0) | (tail_beside ? 32 : 0) | (chain_beside ? 64 : 0);
        last_resize_bands = resize_bands;
        if (two_launches) ORBX_HIP(hipStreamWaitEvent(os, ev_oct_join, 0));
        ORBX_LAUNCHED("k_octree / k_blur");
        if (marks) mark();
        ORBX_HIP(launch_ev(blur_s ? ev_join : nullptr, k_index, dim3(nB), dim3(64), 0, os, d_levels.p, nlevels, sel, sel_frame_entries, sel_cnt,
                           lap0, lap1, cap, kp_dst, sel_frame_entries, o_n + f0, o_mono + f0, o_status + f0));
        ORBX_LAUNCHED("k_index");
        if (marks) mark();
        if (blur_s) ORBX_HIP(hipStreamWaitEvent(s, ev_join, 0));
        else ORBX_HIP(launch_blur(s, 0, n_tiles, nullptr));
        if (marks) mark();
        if (const int lr = launch_orient_desc(f0, nB, s, o_kps, o_desc, cap)) return lr;
        if (marks) mark();
        return ORBX_OK;
    };

    int r;
    if (parts == 1) {
        if ((r = run_range(0, B, st, side_q, true))) return r;
    } else {
        ORBX_HIP(hipEventRecord(ev_parts_fork, st));
        for (int p = 0; p < parts; p++) {
            const int f0 = (int)((long long)B * p / parts), f1 = (int)((long long)B * (p + 1) / parts);
            hipStream_t s = p == 0 ? st : aux_streams[p - 1];
            if (p > 0) ORBX_HIP(hipStreamWaitEvent(s, ev_parts_fork, 0));
            if ((r = run_range(f0, f1 - f0, s, nullptr, false))) return r;
            if (p > 0) { ORBX_HIP(hipEventRecord(ev_parts_join[p - 1], s)); ORBX_HIP(hipStreamWaitEvent(st, ev_parts_join[p - 1], 0)); }
        }
    }
    prof_marks = mark_i;
    prof_stream = st;
    ORBX_HIP(hipGetLastError());
    last_batch = B;
    last_handoffs = handoffs;
    return ORBX_OK;
}

extern "C" {

// Per-stage device time of the LAST enqueue, measured with HIP events recorded on the launch stream.
// stages: 0 level-0 copy, 1 pyramid resize (all levels), 2 FAST cells, 3 octree, 4 index, 5 blur, 6 orient+descriptor.
int orbx_profile_enable(orbx_extractor* e, int on)
{
    if (!e) return fail(ORBX_ERR_ARG, "NULL handle");
    ORBX_HIP(hipSetDevice(e->device));
    if (on && !e->prof_ev[0])
        for (int i = 0; i < orbx_extractor::kProfEvents; i++) ORBX_HIP(hipEventCreate(&e->prof_ev[i]));
    e->profile = on != 0;
    e->prof_marks = 0;
    return ORBX_OK;
}

int orbx_profile_read(orbx_extractor* e, float* stage_ms, int n_stages)
{
    if (!e || !stage_ms) return fail(ORBX_ERR_ARG, "NULL argument");
    if (!e->profile || e->prof_marks < 2) return fail(ORBX_ERR_ARG, "profiling was not enabled for the last call");
    ORBX_HIP(hipSetDevice(e->device));
    ORBX_HIP(hipStreamSynchronize(e->prof_stream));
    for (int i = 0; i < n_stages; i++) {
        stage_ms[i] = 0.f;
        if (i + 1 < e->prof_marks) ORBX_HIP(hipEventElapsedTime(&stage_ms[i], e->prof_ev[i], e->prof_ev[i + 1]));
    }
    return ORBX_OK;
}

const char* orbx_last_error(void) { return g_last_error.c_str(); }

int orbx_device_count(void)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int orbx_create(int nfeatures, float scale_factor, int nlevels, int ini_th_fast, int min_th_fast, int device, orbx_extractor** out)
{
    if (!out) return fail(ORBX_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (nlevels < 1 || nlevels > kMaxLevels || nfeatures < 1 || !(scale_factor > 1.0f))
        return fail(ORBX_ERR_ARG, "bad extractor parameters (nfeatures=%d scale=%f nlevels=%d)", nfeatures, scale_factor, nlevels);
    if (int r = stage::check_device(device)) return r;
    ORBX_HIP(hipSetDevice(device));
    orbx_extractor* e = new orbx_extractor();
    e->device = device;
    e->nfeatures = nfeatures; e->nlevels = nlevels; e->ini_th = ini_th_fast; e->min_th = min_th_fast;
    e->scale_factor_f = scale_factor; e->scale_factor_d = (double)scale_factor;
    build_tables(e);
    if (hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking) != hipSuccess) { delete e; return fail(ORBX_ERR_HIP, "stream create failed"); }
    if (hipStreamCreateWithFlags(&e->side_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_parts_fork, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&e->oct_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_oct_join, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_tail, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_resize, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&e->ev_fast0, hipEventDisableTiming) != hipSuccess) { orbx_destroy(e); return fail(ORBX_ERR_HIP, "side stream create failed"); }
    if (const char* env = getenv("ORBX_SERIAL")) e->serial_schedule = atoi(env) != 0;
    if (const char* env = getenv("ORBX_SPLIT")) e->split_parts = std::max(1, std::min(atoi(env), 4));
    if (const char* env = getenv("ORBX_RESIZE_TAIL")) e->resize_tail_first = atoi(env);
    if (const char* env = getenv("ORBX_RESIZE_BAND_MIN")) e->resize_band_min = std::max(atoi(env), 1);
    if (const char* env = getenv("ORBX_RESIZE_BESIDE")) e->resize_beside = atoi(env) != 0;
    if (const char* env = getenv("ORBX_BLUR_SPLIT")) e->blur_split = atoi(env) != 0;
    if (const char* env = getenv("ORBX_BIND_RECORDS")) e->bind_records = atoi(env) != 0;
    if (const char* env = getenv("ORBX_STATUS_IN_FAST")) e->status_in_fast = atoi(env) != 0;
    if (const char* env = getenv("ORBX_OCT_DYN")) e->oct_dyn_off = atoi(env) == 0;
    if (const char* env = getenv("ORBX_OCT_DYN_MAXB")) e->oct_dyn_max_batch = atoi(env);
    if (const char* env = getenv("ORBX_OCT_WAVES")) { const int wv = atoi(env); if (wv == 1 || wv == 2 || wv == 4) e->oct_waves_env = wv; }
    if (const char* env = getenv("ORBX_OCT_TAB_DEPTH")) e->oct_tab_depth_max = std::max(0, std::min(kOctTabMaxDepth, atoi(env)));
    if (const char* env = getenv("ORBX_OCT_SMALL_MAX")) e->oct_small_max_waves = std::max(0, std::min(64, atoi(env)));
    if (const char* env = getenv("ORBX_OCT_WAVES_BESIDE")) {       // A/B runs: three digits, e.g. 412 (early level 0, lower, upper levels)
        for (int i = 0; i < 3 && env[i]; i++) { const int wv = env[i] - '0'; if (wv == 1 || wv == 2 || wv == 4) e->oct_waves_beside[i] = wv; }
    }
    if (const char* env = getenv("ORBX_OCT_DYN_KEYS_BESIDE")) e->oct_dyn_keys_beside = std::max(64, atoi(env));
    for (int i = 0; i + 1 < e->split_parts; i++) {
        hipStream_t s = nullptr; hipEvent_t ev = nullptr;
        if (hipStreamCreateWithFlags(&s, hipStreamNonBlocking) != hipSuccess || hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) {
            if (s) (void)hipStreamDestroy(s);
            break;      // fewer ranges then
        }
        e->aux_streams.push_back(s); e->ev_parts_join.push_back(ev);
    }
    *out = e;
    return ORBX_OK;
}

void orbx_destroy(orbx_extractor* e)
{
    if (!e) return;
    (void)hipSetDevice(e->device);
    if (e->stream) { (void)hipStreamSynchronize(e->stream); (void)hipStreamDestroy(e->stream); }
    if (e->side_stream) { (void)hipStreamSynchronize(e->side_stream); (void)hipStreamDestroy(e->side_stream); }
    if (e->oct_stream) { (void)hipStreamSynchronize(e->oct_stream); (void)hipStreamDestroy(e->oct_stream); }
    if (e->ev_oct_join) (void)hipEventDestroy(e->ev_oct_join);
    if (e->ev_fast0) (void)hipEventDestroy(e->ev_fast0);
    if (e->ev_resize) (void)hipEventDestroy(e->ev_resize);
    if (e->ev_tail) (void)hipEventDestroy(e->ev_tail);
    if (e->ev_fork) (void)hipEventDestroy(e->ev_fork);
    if (e->ev_join) (void)hipEventDestroy(e->ev_join);
    for (hipStream_t s : e->aux_streams) { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); }
    for (hipEvent_t ev : e->ev_parts_join) (void)hipEventDestroy(ev);
    if (e->ev_parts_fork) (void)hipEventDestroy(e->ev_parts_fork);
    e->d_levels.release(); e->d_cells.release(); e->d_tiles.release(); e->d_strips.release();
    for (auto& b : e->d_qsx0) b.release();
    for (auto& b : e->d_yofs) b.release();
    for (auto& b : e->d_qsel) b.release();
    for (auto& b : e->d_qalpha) b.release();
    for (auto& b : e->d_ibeta) b.release();
    for (auto& b : e->d_rows) b.release();
    for (auto& b : e->d_xofs) b.release();
    for (auto& b : e->d_ialpha) b.release();
    e->d_pyr.release(); e->d_blur.release(); e->d_cand.release(); e->d_scratch.release(); e->d_sel.release(); e->d_oct_nodes.release(); e->d_oct_prefix.release(); e->d_oct_tabs.release(); e->d_oct_bounds.release(); e->d_oct_maps.release();
    e->d_cell_count.release(); e->d_sel_count.release(); e->d_kp_dst.release(); e->d_lvl_kps.release();
    e->d_kps.release(); e->d_desc.release(); e->d_n.release(); e->d_mono.release(); e->d_status.release();
    e->d_sad.release(); e->d_stereo_io.release();
    delete e;
}

int orbx_max_keypoints(const orbx_extractor* e) { return e ? e->max_kp : 0; }

// the same bound for ONE image geometry: per level max(N + 3, 32, 4 x nIni) with the level's own nIni (the bordered area of the upper
// levels of a wide image is relatively wider still: the 2 x 16-px border does not shrink with the level)
int orbx_max_keypoints_for(const orbx_extractor* e, int width, int height)
{
    if (!e || width < 1 || height < 1) return 0;
    int total = 0;
    for (int l = 0; l < e->nlevels; l++) {
        const int lw = (int)std::nearbyintf((float)width * e->inv_scale[l]), lh = (int)std::nearbyintf((float)height * e->inv_scale[l]);
        const int bw = (lw - kEdge + 3) - (kEdge - 3), bh = (lh - kEdge + 3) - (kEdge - 3);
        const int n_ini = bh > 0 ? (int)std::roundf((float)bw / (float)bh) : 0;
        total += std::max({e->nfeat[l] + 3, 32, 4 * std::max(n_ini, 0)});
    }
    return total;
}
int orbx_levels(const orbx_extractor* e) { return e ? e->nlevels : 0; }
float orbx_scale_factor(const orbx_extractor* e) { return e ? e->scale_factor_f : 0.f; }

int orbx_scale_tables(const orbx_extractor* e, float* scale, float* inv_scale, float* sigma2, float* inv_sigma2)
{
    if (!e) return fail(ORBX_ERR_ARG, "NULL handle");
    for (int i = 0; i < e->nlevels; i++) {
        if (scale) scale[i] = e->scale[i];
        if (inv_scale) inv_scale[i] = e->inv_scale[i];
        if (sigma2) sigma2[i] = e->sigma2[i];
        if (inv_sigma2) inv_sigma2[i] = e->inv_sigma2[i];
    }
    return ORBX_OK;
}

int orbx_features_per_level(const orbx_extractor* e, int* n_per_level)
{
    if (!e || !n_per_level) return fail(ORBX_ERR_ARG, "NULL argument");
    for (int i = 0; i < e->nlevels; i++) n_per_level[i] = e->nfeat[i];
    return ORBX_OK;
}

int orbx_extract_batch_device(orbx_extractor* e, const uint8_t* d_imgs, int batch, int width, int height,
                              int row_stride, size_t frame_stride, int lap0, int lap1,
                              OrbxKeyPoint* d_kps, uint8_t* d_desc, int cap, int32_t* d_n, int32_t* d_mono,
                              int32_t* d_status, void* stream)
{
    if (!e || !d_imgs || !d_kps || !d_desc || !d_n || !d_mono || !d_status) return fail(ORBX_ERR_ARG, "NULL argument");
    if (batch < 1 || width < 1 || height < 1 || row_stride < width || cap < 1) return fail(ORBX_ERR_ARG, "bad batch/geometry");
    // (k_resize and k_blur address the pixels of one frame with 32-bit byte offsets, row x stride as a 24-bit product)
    if (row_stride >= (1 << 24) || (uint64_t)row_stride * (uint64_t)height >= (1ull << 31))
        return fail(ORBX_ERR_ARG, "a frame of %d rows of %d bytes exceeds 2 GiB (or a row 16 MiB)", height, row_stride);
    ORBX_HIP(hipSetDevice(e->device));
    int r;
    if ((r = e->setup_geometry(width, height)) || (r = e->ensure_batch(batch))) return r;
    return e->enqueue(d_imgs, false, batch, row_stride, frame_stride, lap0, lap1, d_kps, d_desc, cap, d_n, d_mono, d_status,
                      (hipStream_t)stream);
}

int orbx_extract_batch(orbx_extractor* e, const uint8_t* const* imgs, int batch, int width, int height, int stride,
                       int lap0, int lap1, OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n, int* mono_index)
{
    if (!e || !imgs || !kps || !desc || !n || !mono_index) return fail(ORBX_ERR_ARG, "NULL argument");
    if (batch < 1 || cap < 1) return fail(ORBX_ERR_ARG, "bad batch/capacity");
    if (width < 1 || height < 1) { for (int b = 0; b < batch; b++) { n[b] = 0; mono_index[b] = -1; } return ORBX_ERR_EMPTY; }
    if (stride < width) return fail(ORBX_ERR_ARG, "stride < width");
    ORBX_HIP(hipSetDevice(e->device));
    int r;
    if ((r = e->setup_geometry(width, height)) || (r = e->ensure_batch(batch))) return r;
    const size_t B = (size_t)batch;
    if ((r = e->d_kps.ensure(B * cap)) || (r = e->d_desc.ensure(B * cap * 32))) return r;
    const LevelDesc& L0 = e->levels[0];
    for (int b = 0; b < batch; b++) {
        if (!imgs[b]) return fail(ORBX_ERR_ARG, "imgs[%d] is NULL", b);
        ORBX_HIP(hipMemcpy2DAsync(e->d_pyr.p + b * e->pyr_frame_bytes + L0.off, L0.stride, imgs[b], stride, width, height,
                                  hipMemcpyHostToDevice, e->stream));
    }
    if ((r = e->enqueue(nullptr, true, batch, 0, 0, lap0, lap1, e->d_kps.p, e->d_desc.p, cap, e->d_n.p, e->d_mono.p, e->d_status.p, e->stream)))
        return r;
    std::vector<int> st(batch);
    ORBX_HIP(hipMemcpyAsync(n, e->d_n.p, sizeof(int) * B, hipMemcpyDeviceToHost, e->stream));
    ORBX_HIP(hipMemcpyAsync(mono_index, e->d_mono.p, sizeof(int) * B, hipMemcpyDeviceToHost, e->stream));
    ORBX_HIP(hipMemcpyAsync(st.data(), e->d_status.p, sizeof(int) * B, hipMemcpyDeviceToHost, e->stream));
    ORBX_HIP(hipMemcpyAsync(kps, e->d_kps.p, sizeof(OrbxKeyPoint) * B * cap, hipMemcpyDeviceToHost, e->stream));
    ORBX_HIP(hipMemcpyAsync(desc, e->d_desc.p, B * cap * 32, hipMemcpyDeviceToHost, e->stream));
    ORBX_HIP(hipStreamSynchronize(e->stream));
    for (int b = 0; b < batch; b++)
        if (st[b] != ORBX_OK) return fail(st[b], "frame %d: device status %d (n=%d, cap=%d)", b, st[b], n[b], cap);
    return ORBX_OK;
}

int orbx_extract(orbx_extractor* e, const uint8_t* img, int width, int height, int stride,
                 int lap0, int lap1, OrbxKeyPoint* kps, uint8_t* desc, int cap, int* n, int* mono_index)
{
    if (!img || width < 1 || height < 1) {      // _image.empty() (:1090-1091)
        if (n) *n = 0;
        if (mono_index) *mono_index = -1;
        return ORBX_ERR_EMPTY;
    }
    const uint8_t* imgs[1] = {img};
    return orbx_extract_batch(e, imgs, 1, width, height, stride, lap0, lap1, kps, desc, cap, n, mono_index);
}

int orbx_pyramid_level_size(const orbx_extractor* e, int level, int* width, int* height)
{
    if (!e || level < 0 || level >= e->nlevels || e->geo_w == 0) return fail(ORBX_ERR_ARG, "no pyramid (level %d)", level);
    if (width) *width = e->levels[level].w;
    if (height) *height = e->levels[level].h;
    return ORBX_OK;
}

static int download_level(orbx_extractor* e, const uint8_t* base, int frame, int level, int border, uint8_t* dst, int dst_stride)
{
    if (!e || !dst || level < 0 || level >= e->nlevels || frame < 0 || frame >= e->last_batch || border < 0)
        return fail(ORBX_ERR_ARG, "bad frame/level");
    const LevelDesc& L = e->levels[level];
    if (dst_stride < L.w + 2 * border) return fail(ORBX_ERR_ARG, "dst_stride too small");
    ORBX_HIP(hipSetDevice(e->device));
    ORBX_HIP(hipStreamSynchronize(e->stream));
    ORBX_HIP(hipMemcpy2D(dst + (size_t)border * dst_stride + border, dst_stride, base + (size_t)frame * e->pyr_frame_bytes + L.off,
                         L.stride, L.w, L.h, hipMemcpyDeviceToHost));
    if (border > 0) {       // copyMakeBorder(..., BORDER_REFLECT_101) (:1185,:1190)
        auto refl = [](int p, int len) { if (len == 1) return 0; while (p < 0 || p >= len) p = p < 0 ? -p : 2 * len - 2 - p; return p; };
        for (int y = 0; y < L.h + 2 * border; y++) {
            const int sy = refl(y - border, L.h) + border;
            uint8_t* row = dst + (size_t)y * dst_stride;
            const uint8_t* srow = dst + (size_t)sy * dst_stride;
            if (sy != y) std::memcpy(row + border, srow + border, L.w);
            for (int x = 0; x < border; x++) {
                row[x] = row[border + refl(x - border, L.w)];
                row[border + L.w + x] = row[border + refl(L.w + x, L.w)];
            }
        }
    }
    return ORBX_OK;
}

int orbx_pyramid_level(orbx_extractor* e, int frame, int level, int border, uint8_t* dst, int dst_stride)
{
    return download_level(e, e ? e->d_pyr.p : nullptr, frame, level, border, dst, dst_stride);
}

int orbx_debug_blurred_level(orbx_extractor* e, int frame, int level, uint8_t* dst, int dst_stride)
{
    return download_level(e, e ? e->d_blur.p : nullptr, frame, level, 0, dst, dst_stride);
}

int orbx_debug_candidates(orbx_extractor* e, int frame, int level, OrbxKeyPoint* out, int cap, int* n)
{
    if (!e || !out || !n || level < 0 || level >= e->nlevels || frame < 0 || frame >= e->last_batch) return fail(ORBX_ERR_ARG, "bad frame/level");
    ORBX_HIP(hipSetDevice(e->device));
    ORBX_HIP(hipStreamSynchronize(e->stream));
    const LevelDesc& L = e->levels[level];
    std::vector<int> cnt(std::max(L.cell_count, 1));
    std::vector<uint32_t> ent(std::max(L.cand_cap, 1));
    if (L.cell_count > 0) {
        ORBX_HIP(hipMemcpy(cnt.data(), e->d_cell_count.p + (size_t)frame * e->cells.size() + L.cell_begin, sizeof(int) * L.cell_count, hipMemcpyDeviceToHost));
        ORBX_HIP(hipMemcpy(ent.data(), e->d_cand.p + (size_t)frame * e->cand_frame_entries + L.cand_off, sizeof(uint32_t) * L.cand_cap, hipMemcpyDeviceToHost));
    }
    int k = 0;
    for (int c = 0; c < L.cell_count; c++) {
        const CellDesc& cd = e->cells[L.cell_begin + c];
        for (int i = 0; i < cnt[c]; i++, k++) {
            if (k >= cap) continue;
            const uint32_t en = ent[cd.slot_off - L.cand_off + i];
            OrbxKeyPoint kp;
            kp.x = (float)key_x(en); kp.y = (float)key_y(en); kp.size = 7.f; kp.angle = -1.f; kp.response = (float)key_resp(en);
            kp.octave = 0; kp.class_id = -1;
            out[k] = kp;
        }
    }
    *n = k;
    return ORBX_OK;
}

int orbx_debug_level_keypoints(orbx_extractor* e, int frame, int level, OrbxKeyPoint* out, int cap, int* n)
{
    if (!e || !out || !n || level < 0 || level >= e->nlevels || frame < 0 || frame >= e->last_batch) return fail(ORBX_ERR_ARG, "bad frame/level");
    ORBX_HIP(hipSetDevice(e->device));
    ORBX_HIP(hipStreamSynchronize(e->stream));
    const LevelDesc& L = e->levels[level];
    int cnt = 0;
    ORBX_HIP(hipMemcpy(&cnt, e->d_sel_count.p + (size_t)frame * e->nlevels + level, sizeof(int), hipMemcpyDeviceToHost));
    *n = cnt;
    const int m = std::min(cnt, cap);
    if (m > 0)
        ORBX_HIP(hipMemcpy(out, e->d_lvl_kps.p + (size_t)frame * e->sel_frame_entries + L.sel_off, sizeof(OrbxKeyPoint) * m, hipMemcpyDeviceToHost));
    return ORBX_OK;
}

// Test hook: shrinks the per-wave corner list of the FAST kernel so that ordinary images take its overflow path (every pixel of
// the wave's rows goes through nms / emission).  cap <= 0 restores the default.  Takes effect at the next geometry setup.
int orbx_debug_set_tail_delay(orbx_extractor* e, int microseconds)
{
    if (!e || microseconds < 0 || microseconds > 20000) return fail(ORBX_ERR_ARG, "bad tail delay");
    e->dbg_tail_delay_us = microseconds;
    return ORBX_OK;
}

int orbx_debug_resize_bands(orbx_extractor* e)
{
    if (!e) return fail(ORBX_ERR_ARG, "NULL handle");
    return e->last_resize_bands ? 1 : 0;
}

int orbx_debug_resize_rows(int src_h, int dst_h, uint32_t* rows, int* band_rows)
{
    if (src_h < 1 || dst_h < 1 || !rows || !band_rows) return fail(ORBX_ERR_ARG, "bad row table request");
    std::vector<int> yofs;
    std::vector<short> ib;
    std::vector<ResizeRow> t;
    bool sums_ok = true;
    if (int r = build_resize_rows(src_h, dst_h, yofs, ib, t, &sums_ok)) return r;
    for (int y = 0; y < dst_h; y++) { rows[4 * y] = t[y].sy; rows[4 * y + 1] = t[y].b0; rows[4 * y + 2] = t[y].b1; rows[4 * y + 3] = t[y].plan; }
    *band_rows = kResizeBand;
    return sums_ok ? 1 : 0;
}

int orbx_debug_octree_waves(orbx_extractor* e, int launch)
{
    if (!e || launch < 0 || launch > 2) return fail(ORBX_ERR_ARG, "NULL handle or launch outside 0..2");
    return e->last_oct_waves[launch];
}

int orbx_debug_octree_table(orbx_extractor* e, int level, int* depth, int* n_ini, int16_t* bounds, int cap)
{
    if (!e || !depth || !n_ini || !bounds || level < 0 || level >= (int)e->oct_tabs.size()) return fail(ORBX_ERR_ARG, "NULL argument, no geometry yet or level outside the pyramid");
    ORBX_HIP(hipSetDevice(e->device));
    OctTabDesc t;
    ORBX_HIP(hipMemcpy(&t, e->d_oct_tabs.p + level, sizeof(t), hipMemcpyDeviceToHost));
    const int n = t.n_ini > 0 ? (t.n_ini + 1) * ((1 << t.depth) + 1) : 0;
    if (n > cap) return fail(ORBX_ERR_CAPACITY, "%d boundaries, room for %d", n, cap);
    if (n > 0) ORBX_HIP(hipMemcpy(bounds, e->d_oct_bounds.p + t.bounds_off, sizeof(int16_t) * n, hipMemcpyDeviceToHost));
    *depth = t.depth; *n_ini = t.n_ini;
    return n;
}

int orbx_debug_last_schedule(orbx_extractor* e)
{
    if (!e) return fail(ORBX_ERR_ARG, "NULL handle");
    return e->last_octree_variant;
}

int orbx_debug_last_handoffs(orbx_extractor* e)
{
    if (!e) return fail(ORBX_ERR_ARG, "NULL handle");
    return e->last_handoffs;
}

// host only: the blur's tile list of a width x height image and its cut in front of `level`, as setup_geometry makes them
int orbx_debug_blur_tile_split(float scale_factor, int nlevels, int width, int height, int level, int16_t* tile_levels, int cap, int* split)
{
    if (!tile_levels || !split || nlevels < 1 || nlevels > kMaxLevels || !(scale_factor > 1.0f) || width < 1 || height < 1)
        return fail(ORBX_ERR_ARG, "bad tile split request");
    orbx_extractor e;
    e.nfeatures = 1; e.nlevels = nlevels; e.scale_factor_f = scale_factor; e.scale_factor_d = (double)scale_factor;
    build_tables(&e);
    std::vector<TileDesc> tiles;
    for (int l = 0; l < nlevels; l++)
        append_blur_tiles(l, (int)std::nearbyintf((float)width * e.inv_scale[l]), (int)std::nearbyintf((float)height * e.inv_scale[l]), tiles);
    if ((int)tiles.size() > cap) return fail(ORBX_ERR_CAPACITY, "%d tiles, room for %d", (int)tiles.size(), cap);
    for (size_t t = 0; t < tiles.size(); t++) tile_levels[t] = tiles[t].level;
    if (!blur_tile_split(tiles, level, split)) return fail(ORBX_ERR_INTERNAL, "the blur tiles of levels %d.. are not one range of the tile list", level);
    return (int)tiles.size();
}

int orbx_debug_set_fast_corner_cap(orbx_extractor* e, int cap)
{
    if (!e) return fail(ORBX_ERR_ARG, "NULL handle");
    e->fast_corner_cap = cap > 0 ? std::min(cap, 4096) : 0;
    e->geo_w = e->geo_h = 0;            // force setup_geometry to rebuild the LDS layout
    return ORBX_OK;
}

// host-side run of the device introsort restatement (pins it against std::sort in the CPU tests)
int orbx_debug_introsort(int32_t* count, int32_t* ulx, int32_t* node, int n)
{
    if (n < 0) return ORBX_ERR_ARG;
    std::vector<SortNode> v(n);
    for (int i = 0; i < n; i++) { v[i].count = count[i]; v[i].ulx = ulx[i]; v[i].node = node[i]; }
    std::vector<int> stack(3 * kIntrosortStack);
    introsort_nodes(v.data(), n, stack.data());
    for (int i = 0; i < n; i++) { count[i] = v[i].count; ulx[i] = v[i].ulx; node[i] = v[i].node; }
    return ORBX_OK;
}

// the octree's wave-parallel std::sort on the device (one wave, arrays staged in LDS exactly as k_octree holds them): pinned
// against std::sort itself by tests/test_extractor_gpu.py
int orbx_debug_wave_sort(int32_t* count, int32_t* ulx, int32_t* node, int n)
{
    if (n < 0 || n > 4000) return fail(ORBX_ERR_ARG, "n %d outside 0..4000", n);
    if (n == 0) return ORBX_OK;
    std::vector<SortNode> v(n);
    for (int i = 0; i < n; i++) { v[i].count = count[i]; v[i].ulx = ulx[i]; v[i].node = node[i]; }
    SortNode* d = nullptr;
    ORBX_HIP(hipMalloc(&d, sizeof(SortNode) * n));
    int r = ORBX_OK;
    const size_t lds = 2 * sizeof(SortNode) * (size_t)n + 2 * (size_t)n + 16;
    if (hipMemcpy(d, v.data(), sizeof(SortNode) * n, hipMemcpyHostToDevice) != hipSuccess) r = ORBX_ERR_HIP;
    if (!r && hipFuncSetAttribute((const void*)k_debug_wave_sort, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) r = ORBX_ERR_HIP;
    if (!r) {
        hipLaunchKernelGGL(k_debug_wave_sort, dim3(1), dim3(64), lds, 0, d, n);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) r = ORBX_ERR_HIP;
    }
    if (!r && hipMemcpy(v.data(), d, sizeof(SortNode) * n, hipMemcpyDeviceToHost) != hipSuccess) r = ORBX_ERR_HIP;
    (void)hipFree(d);
    if (r) return fail(r, "device sort failed");
    for (int i = 0; i < n; i++) { count[i] = v[i].count; ulx[i] = v[i].ulx; node[i] = v[i].node; }
    return ORBX_OK;
}

// the FAST score tree of k_fast_strips alone, on n row-major 7 x 7 patches in host memory: M (OpenCV's corner score + 1, 0 where no
// arc of nine is all brighter or all darker) per patch.  Pinned against the definition by tests/test_fast_score_tree_gpu.py.
int orbx_debug_fast_scores(const uint8_t* patches, int n, int pitch, int* out)
{
    if (n < 0 || n > (1 << 22)) return fail(ORBX_ERR_ARG, "n %d outside 0..2^22", n);
    if (pitch < 8 || pitch > 1024) return fail(ORBX_ERR_ARG, "pitch %d outside 8..1024", pitch);
    if (n == 0) return ORBX_OK;
    if (!patches || !out) return fail(ORBX_ERR_ARG, "NULL argument");
    const int per_band = std::min(pitch / 8, 64), bands = (64 + per_band - 1) / per_band;
    const size_t lds = (size_t)bands * 7 * pitch;               // a few KB: 64 bands at pitch 8 .. 15, one at pitch >= 512
    uint8_t* d_in = nullptr;
    int* d_out = nullptr;
    ORBX_HIP(hipMalloc(&d_in, (size_t)n * 49));
    int r = ORBX_OK;
    if (hipMalloc(&d_out, sizeof(int) * (size_t)n) != hipSuccess) r = ORBX_ERR_HIP;
    if (!r && hipMemcpy(d_in, patches, (size_t)n * 49, hipMemcpyHostToDevice) != hipSuccess) r = ORBX_ERR_HIP;
    if (!r) {
        hipLaunchKernelGGL(k_debug_fast_scores, dim3((n + 63) / 64), dim3(64), lds, 0, d_in, n, pitch, per_band, d_out);
        if (hipGetLastError() != hipSuccess || hipDeviceSynchronize() != hipSuccess) r = ORBX_ERR_HIP;
    }
    if (!r && hipMemcpy(out, d_out, sizeof(int) * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess) r = ORBX_ERR_HIP;
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    if (r) return fail(r, "device score tree failed");
    return ORBX_OK;
}

// k_orient_desc alone, through the pipeline's own launch (launch_orient_desc), on hand-built stage outputs: level images, blurred
// levels, selection records, counts and output rows are written where the pipeline stages would have left them.  See the header.
int orbx_debug_orient_desc(orbx_extractor* e, int width, int height, int batch, const uint8_t* raw, const uint8_t* blurred, int pad_byte,
                           const int32_t* counts, const int32_t* keys, int cap, int guard_rows,
                           OrbxKeyPoint* kps, uint8_t* desc, OrbxKeyPoint* lvl_kps, int lvl_cap, int32_t* sel_caps)
{
    if (!e || !raw || !blurred || !counts || !kps || !desc || !lvl_kps) return fail(ORBX_ERR_ARG, "NULL argument");
    if (width < 1 || height < 1 || batch < 1 || batch > 64 || cap < 1 || cap > (1 << 20) || guard_rows < 0 || guard_rows > (1 << 20) || pad_byte < 0 || pad_byte > 255)
        return fail(ORBX_ERR_ARG, "bad batch/geometry/capacity");
    ORBX_HIP(hipSetDevice(e->device));
    int r;
    if ((r = e->setup_geometry(width, height)) || (r = e->ensure_batch(batch))) return r;
    const int nl = e->nlevels, B = batch, S = e->sel_frame_entries;
    // every key inside the area FAST can report (EDGE_THRESHOLD = 19: the kernel's loads then stay inside the level), every count
    // within the level's slots -- checked before anything is uploaded
    size_t n_keys = 0, level_bytes = 0;
    for (int l = 0; l < nl; l++) level_bytes += (size_t)e->levels[l].w * e->levels[l].h;
    for (int b = 0; b < B; b++)
        for (int l = 0; l < nl; l++) {
            const LevelDesc& L = e->levels[l];
            const int c = counts[(size_t)b * nl + l];
            if (c < 0 || c > L.sel_cap || c > lvl_cap) return fail(ORBX_ERR_ARG, "frame %d level %d: %d keys, the level has %d slots (lvl_cap %d)", b, l, c, L.sel_cap, lvl_cap);
            if (c > 0 && !keys) return fail(ORBX_ERR_ARG, "keys is NULL");
            for (int k = 0; k < c; k++, n_keys++) {
                const int32_t* q = keys + 4 * n_keys;
                if (q[0] < kEdge || q[0] > L.w - kEdge - 1 || q[1] < kEdge || q[1] > L.h - kEdge - 1 || q[2] < 0 || q[2] > 255)
                    return fail(ORBX_ERR_ARG, "frame %d level %d key %d: (%d, %d, %d) outside [%d, %d] x [%d, %d] x [0, 255]", b, l, k, q[0], q[1], q[2],
                                kEdge, L.w - kEdge - 1, kEdge, L.h - kEdge - 1);
            }
        }
    for (int l = 0; l < nl; l++) {
        if (e->levels[l].sel_cap > lvl_cap) return fail(ORBX_ERR_ARG, "lvl_cap %d below the %d slots of level %d", lvl_cap, e->levels[l].sel_cap, l);
        if (sel_caps) sel_caps[l] = e->levels[l].sel_cap;
    }
    // slots beyond a level's count hold a key the kernel could read safely: a lane that took one for live would show in lvl_kps
    // (cleared to 0xFF below, written by every live lane whatever its row), not as a fault
    std::vector<uint32_t> sel((size_t)B * S, pack_key((uint32_t)(kEdge - 16), (uint32_t)(kEdge - 16), 0xEEu));
    std::vector<int> dst((size_t)B * S, -1), cnt((size_t)B * nl);
    n_keys = 0;
    for (int b = 0; b < B; b++)
        for (int l = 0; l < nl; l++) {
            const LevelDesc& L = e->levels[l];
            cnt[(size_t)b * nl + l] = counts[(size_t)b * nl + l];
            for (int k = 0; k < counts[(size_t)b * nl + l]; k++, n_keys++) {
                const int32_t* q = keys + 4 * n_keys;
                sel[(size_t)b * S + L.sel_off + k] = pack_key((uint32_t)(q[0] - 16), (uint32_t)(q[1] - 16), (uint32_t)q[2]);
                dst[(size_t)b * S + L.sel_off + k] = q[3];
            }
        }
    const size_t out_rows = (size_t)B * cap + 2 * (size_t)guard_rows;
    if ((r = e->d_kps.ensure(out_rows)) || (r = e->d_desc.ensure(out_rows * 32))) return r;
    hipStream_t st = e->stream;
    ORBX_HIP(hipMemsetAsync(e->d_pyr.p, pad_byte, (size_t)B * e->pyr_frame_bytes + 64, st));
    ORBX_HIP(hipMemsetAsync(e->d_blur.p, pad_byte, (size_t)B * e->pyr_frame_bytes + 64, st));
    e->batch_cap = 0;           // the next extract call clears the padding again (ensure_batch)
    for (int b = 0; b < B; b++) {
        size_t o = (size_t)b * level_bytes;
        for (int l = 0; l < nl; l++) {
            const LevelDesc& L = e->levels[l];
            ORBX_HIP(hipMemcpy2DAsync(e->d_pyr.p + (size_t)b * e->pyr_frame_bytes + L.off, L.stride, raw + o, L.w, L.w, L.h, hipMemcpyHostToDevice, st));
            ORBX_HIP(hipMemcpy2DAsync(e->d_blur.p + (size_t)b * e->pyr_frame_bytes + L.off, L.stride, blurred + o, L.w, L.w, L.h, hipMemcpyHostToDevice, st));
            o += (size_t)L.w * L.h;
        }
    }
    ORBX_HIP(hipMemcpyAsync(e->d_sel.p, sel.data(), sizeof(uint32_t) * sel.size(), hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync(e->d_kp_dst.p, dst.data(), sizeof(int) * dst.size(), hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync(e->d_sel_count.p, cnt.data(), sizeof(int) * cnt.size(), hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemsetAsync(e->d_lvl_kps.p, 0xFF, sizeof(OrbxKeyPoint) * (size_t)B * S, st));
    ORBX_HIP(hipMemcpyAsync(e->d_kps.p, kps, sizeof(OrbxKeyPoint) * out_rows, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync(e->d_desc.p, desc, 32 * out_rows, hipMemcpyHostToDevice, st));
    if ((r = e->launch_orient_desc(0, B, st, e->d_kps.p + guard_rows, e->d_desc.p + (size_t)guard_rows * 32, cap))) return r;
    e->last_batch = B;
    ORBX_HIP(hipMemcpyAsync(kps, e->d_kps.p, sizeof(OrbxKeyPoint) * out_rows, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipMemcpyAsync(desc, e->d_desc.p, 32 * out_rows, hipMemcpyDeviceToHost, st));
    for (int b = 0; b < B; b++)
        for (int l = 0; l < nl; l++)
            ORBX_HIP(hipMemcpyAsync(lvl_kps + ((size_t)b * nl + l) * lvl_cap, e->d_lvl_kps.p + (size_t)b * S + e->levels[l].sel_off,
                                    sizeof(OrbxKeyPoint) * e->levels[l].sel_cap, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    return ORBX_OK;
}

// Frame::ComputeStereoMatches (src/Frame.cc:931-1101) on the pyramids both extractors hold from their LAST extract call.
static int stereo_enqueue(orbx_extractor* l, orbx_extractor* r, int frame0, int batch,
                          const OrbxKeyPoint* d_kps_l, const uint8_t* d_desc_l, const int32_t* d_n_l,
                          const OrbxKeyPoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_n_r, int cap,
                          float mb, float mbf, float* d_u_right, float* d_depth, hipStream_t st)
{
    if (l->geo_w == 0 || l->geo_w != r->geo_w || l->geo_h != r->geo_h || l->nlevels != r->nlevels || l->scale_factor_f != r->scale_factor_f)
        return fail(ORBX_ERR_ARG, "the two extractors do not hold pyramids of the same geometry");
    if (l->device != r->device) return fail(ORBX_ERR_ARG, "the two extractors live on different devices");
    if (frame0 < 0 || batch < 1 || frame0 + batch > l->last_batch || frame0 + batch > r->last_batch) return fail(ORBX_ERR_ARG, "frames outside the last extract call");
    if (l->nlevels > 16) return fail(ORBX_ERR_ARG, "more than 16 pyramid levels");
    if (cap < 1 || cap > 8192) return fail(ORBX_ERR_ARG, "cap %d outside 1..8192", cap);
    if (!(mb > 0.f) || !(mbf > 0.f)) return fail(ORBX_ERR_ARG, "mb and mbf must be positive");
    int rr = l->d_sad.ensure((size_t)batch * cap);
    if (rr) return rr;
    StereoTables T;
    for (int i = 0; i < 16; i++) { T.scale[i] = l->scale[std::min(i, l->nlevels - 1)]; T.inv_scale[i] = l->inv_scale[std::min(i, l->nlevels - 1)]; }
    const uint8_t* pl = l->d_pyr.p + (size_t)frame0 * l->pyr_frame_bytes;
    const uint8_t* pr = r->d_pyr.p + (size_t)frame0 * r->pyr_frame_bytes;
    hipLaunchKernelGGL(k_stereo_match, dim3((cap + 3) / 4, batch), dim3(256), 0, st, pl, pr, l->pyr_frame_bytes, l->d_levels.p, T,
                       d_kps_l, d_desc_l, d_n_l, d_kps_r, d_desc_r, d_n_r, cap, mb, mbf, l->nlevels, d_u_right, d_depth, l->d_sad.p);
    int n_pow2 = 2;
    while (n_pow2 < cap) n_pow2 <<= 1;
    hipLaunchKernelGGL(k_stereo_median, dim3(batch), dim3(256), (size_t)n_pow2 * sizeof(int), st, d_n_l, cap, n_pow2, d_u_right, d_depth, l->d_sad.p);
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}

int orbx_stereo_matches_device(orbx_extractor* left, orbx_extractor* right, int batch,
                               const OrbxKeyPoint* d_kps_l, const uint8_t* d_desc_l, const int32_t* d_n_l,
                               const OrbxKeyPoint* d_kps_r, const uint8_t* d_desc_r, const int32_t* d_n_r, int cap,
                               float mb, float mbf, float* d_u_right, float* d_depth, void* stream)
{
    if (!left || !right || !d_kps_l || !d_desc_l || !d_n_l || !d_kps_r || !d_desc_r || !d_n_r || !d_u_right || !d_depth) return fail(ORBX_ERR_ARG, "NULL argument");
    ORBX_HIP(hipSetDevice(left->device));
    return stereo_enqueue(left, right, 0, batch, d_kps_l, d_desc_l, d_n_l, d_kps_r, d_desc_r, d_n_r, cap, mb, mbf, d_u_right, d_depth, (hipStream_t)stream);
}

int orbx_stereo_matches(orbx_extractor* left, orbx_extractor* right, int frame,
                        const OrbxKeyPoint* kps_l, const uint8_t* desc_l, int n_l,
                        const OrbxKeyPoint* kps_r, const uint8_t* desc_r, int n_r, float mb, float mbf, float* u_right, float* depth)
{
    if (!left || !right || n_l < 0 || n_r < 0 || (n_l > 0 && (!kps_l || !desc_l || !u_right || !depth)) || (n_r > 0 && (!kps_r || !desc_r)))
        return fail(ORBX_ERR_ARG, "NULL argument");
    if (n_l == 0) return ORBX_OK;
    ORBX_HIP(hipSetDevice(left->device));
    const int cap = std::max(std::max(n_l, n_r), 1);
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    const size_t o_kl = 0, o_dl = al(o_kl + sizeof(OrbxKeyPoint) * (size_t)cap), o_kr = al(o_dl + 32 * (size_t)cap), o_dr = al(o_kr + sizeof(OrbxKeyPoint) * (size_t)cap),
                 o_n = al(o_dr + 32 * (size_t)cap), o_u = al(o_n + 8), o_d = al(o_u + 4 * (size_t)cap), total = al(o_d + 4 * (size_t)cap);
    int r = left->d_stereo_io.ensure(total);
    if (r) return r;
    uint8_t* b = left->d_stereo_io.p;
    hipStream_t st = left->stream;
    const int32_t nn[2] = {n_l, n_r};
    ORBX_HIP(hipMemcpyAsync(b + o_kl, kps_l, sizeof(OrbxKeyPoint) * (size_t)n_l, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipMemcpyAsync(b + o_dl, desc_l, 32 * (size_t)n_l, hipMemcpyHostToDevice, st));
    if (n_r > 0) {
        ORBX_HIP(hipMemcpyAsync(b + o_kr, kps_r, sizeof(OrbxKeyPoint) * (size_t)n_r, hipMemcpyHostToDevice, st));
        ORBX_HIP(hipMemcpyAsync(b + o_dr, desc_r, 32 * (size_t)n_r, hipMemcpyHostToDevice, st));
    }
    ORBX_HIP(hipMemcpyAsync(b + o_n, nn, 8, hipMemcpyHostToDevice, st));
    ORBX_HIP(hipStreamSynchronize(right->stream));      // the right pyramid was written on the other handle's stream
    r = stereo_enqueue(left, right, frame, 1, (const OrbxKeyPoint*)(b + o_kl), b + o_dl, (const int32_t*)(b + o_n),
                       (const OrbxKeyPoint*)(b + o_kr), b + o_dr, (const int32_t*)(b + o_n) + 1, cap, mb, mbf, (float*)(b + o_u), (float*)(b + o_d), st);
    if (r) return r;
    ORBX_HIP(hipMemcpyAsync(u_right, b + o_u, 4 * (size_t)n_l, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipMemcpyAsync(depth, b + o_d, 4 * (size_t)n_l, hipMemcpyDeviceToHost, st));
    ORBX_HIP(hipStreamSynchronize(st));
    return ORBX_OK;
}

// host-side evaluation of the shared float helpers (pins them against the oracle in the CPU tests)
float orbx_debug_fast_atan2(float y, float x) { return fast_atan2_deg(y, x); }
void orbx_debug_sincos(float a, float* c, float* s) { sincos_f32(a, c, s); }

#ifdef ORBX_FAST_TIMING
int orbx_debug_fast_prof(unsigned long long* out16)
{
    unsigned long long z[16] = {0};
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(d_fast_prof), sizeof(z)) != hipSuccess) return ORBX_ERR_HIP;
    if (hipMemcpyToSymbol(HIP_SYMBOL(d_fast_prof), z, sizeof(z)) != hipSuccess) return ORBX_ERR_HIP;
    return ORBX_OK;
}
#endif
#ifdef ORBX_OCT_TIMING
int orbx_debug_oct_prof(unsigned long long* out11)
{
    if (hipMemcpyFromSymbol(out11, HIP_SYMBOL(d_oct_prof), 11 * sizeof(unsigned long long)) != hipSuccess) return ORBX_ERR_HIP;
    return ORBX_OK;
}
#endif


}  // extern "C"
