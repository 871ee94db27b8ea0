// orbm_rig_search.inc -- the two tracking searches for a two-camera fisheye rig frame (F.Nleft != -1): kernel, host driver and
// the C ABI of include/orbslam3_hip_rig_match.h, and the device-resident entries of include/orbslam3_hip_rig_track_device.h (k_rig_dev_setup
// in front of the same k_grid and k_rig).  Included by orbm_matcher.hip (once, after its host helpers), whose
// search_window, key helpers, rot_bin, three_maxima, ProjFrameDev, k_grid, check_frame, stage_frame and launch helpers it uses as they are.
// Reference: src/ORBmatcher.cc:43-213 (Frame x map points) and :1676-1887 (last frame).  DESIGN.md 4k.
namespace orbm {

struct RigArgs {
    ProjFrameDev L, R;                      // mvKeys + mGrid, mvKeysRight + mGridRight (u_right == nullptr on both)
    const int32_t* l2r; const int32_t* r2l; // mvLeftToRightMatch, mvRightToLeftMatch
    int32_t n_pts;
    const uint8_t* valid; const float* u; const float* v; const int32_t* level; const float* view_cos;             // left camera (map points) / the entry (last frame)
    const uint8_t* valid_r; const float* u_r; const float* v_r; const int32_t* level_r; const float* view_cos_r;   // right camera; the last-frame search reads u_r, v_r only
    const float* depth; const uint8_t* bad;         // map points only
    const float* angle;                             // last frame only
    const uint8_t* desc; const uint8_t* has_obs;
    float th, th_far, nnratio;
    int32_t far_points, check_ori, level_window;
    int32_t last_mode;                      // 0: Frame x map points (:43), 1: last frame (:1676)
    int32_t* assign; uint8_t* occupied;     // [L.n + R.n], left slots first
    int32_t* log_slot; int32_t* log_bin;    // last frame: rotation log, 2 * n_pts entries (wave w owns [w * n_pts, (w + 1) * n_pts))
    int32_t* n_matches;
};

constexpr int kRigThreads = 128;            // two waves: one per side

// LDS bytes of one staged side: descriptors, x, y, octave, CSR entries (48 B per feature) + the cell table
__host__ __device__ inline size_t rig_side_bytes(int n, int ncell) { return (size_t)n * 48 + ((((size_t)ncell + 1) * 4 + 15) & ~(size_t)15); }

__device__ __forceinline__ uint8_t* rig_stage_side(ProjFrameDev& F, uint8_t* p, int tid)
{
    const int n = F.n, ncell = F.cols * F.rows;
    uint8_t* s_desc = p; p += (size_t)n * 32;
    float* s_x = (float*)p; p += (size_t)n * 4;
    float* s_y = (float*)p; p += (size_t)n * 4;
    int32_t* s_oct = (int32_t*)p; p += (size_t)n * 4;
    int32_t* s_cfeat = (int32_t*)p; p += (size_t)n * 4;
    int32_t* s_coff = (int32_t*)p; p += (((size_t)ncell + 1) * 4 + 15) & ~(size_t)15;
    for (int i = tid; i < n * 8; i += kRigThreads) ((uint32_t*)s_desc)[i] = ((const uint32_t*)F.desc)[i];
    for (int i = tid; i < n; i += kRigThreads) { s_x[i] = F.x[i]; s_y[i] = F.y[i]; s_oct[i] = F.octave[i]; }
    const int nfeat_cells = min(F.cell_off[ncell], n);
    for (int i = tid; i < nfeat_cells; i += kRigThreads) s_cfeat[i] = F.cell_feat[i];
    for (int i = tid; i <= ncell; i += kRigThreads) s_coff[i] = F.cell_off[i];
    F.desc = s_desc; F.x = s_x; F.y = s_y; F.octave = s_oct; F.cell_feat = s_cfeat; F.cell_off = s_coff;
    return p;
}

// `!vIndices2.empty()` of :1735 for the calling wave: does Frame::GetFeaturesInArea return anything?  Cells, level filter and
// the |dx|, |dy| < r test only -- occupancy plays no part and no descriptor is read.  Stops at the first 64 cells that hold a hit.
__device__ __forceinline__ bool rig_window_nonempty(const ProjFrameDev& F, float x, float y, float r, int minLevel, int maxLevel, int lane)
{
    const int nMinCellX = max(0, (int)floorf((x - F.min_x - r) * F.winv));
    if (nMinCellX >= F.cols) return false;
    const int nMaxCellX = min(F.cols - 1, (int)ceilf((x - F.min_x + r) * F.winv));
    if (nMaxCellX < 0) return false;
    const int nMinCellY = max(0, (int)floorf((y - F.min_y - r) * F.hinv));
    if (nMinCellY >= F.rows) return false;
    const int nMaxCellY = min(F.rows - 1, (int)ceilf((y - F.min_y + r) * F.hinv));
    if (nMaxCellY < 0) return false;
    const bool bCheckLevels = (minLevel > 0) || (maxLevel >= 0);
    const int ny = nMaxCellY - nMinCellY + 1, nx = nMaxCellX - nMinCellX + 1;
    const int ncell = nx * ny;
    for (int c0 = 0; c0 < ncell; c0 += 64) {
        const int c = c0 + lane;
        bool hit = false;
        if (c < ncell) {
            const int cq = c / ny;
            const int cell = (nMinCellX + cq) * F.rows + nMinCellY + (c - cq * ny);
            const int e1 = F.cell_off[cell + 1];
            for (int e = F.cell_off[cell]; e < e1 && !hit; e++) {
                const int idx = F.cell_feat[e];
                if (bCheckLevels) {
                    const int oc = F.octave[idx];
                    if (oc < minLevel) continue;
                    if (maxLevel >= 0 && oc > maxLevel) continue;
                }
                hit = fabsf(F.x[idx] - x) < r && fabsf(F.y[idx] - y) < r;
            }
        }
        if (__ballot(hit) != 0ull) return true;
    }
    return false;
}

__device__ __forceinline__ void rig_load_desc(const uint8_t* desc, int i, unsigned long long d[4])
{
    const unsigned long long* dp = (const unsigned long long*)(desc + (size_t)i * 32);
    d[0] = dp[0]; d[1] = dp[1]; d[2] = dp[2]; d[3] = dp[3];
}

// One workgroup of two waves per rig frame; the points go in the reference's order.
//  last frame: the two passes of an entry touch disjoint slots (left [0, L.n), right [L.n, ..)) and the right pass's gate --
//   entry valid, LEFT projection inside the image, LEFT window not empty -- is geometry only.  So wave 0 runs the whole left
//   loop and wave 1 the whole right loop (evaluating the gate itself with rig_window_nonempty), each against its own half of
//   the occupancy table and with its own log; they meet at the one histogram (LDS atomics), one three_maxima, and each
//   filters its own log.  The filter is a set operation and nmatches a count, so the order of log entries does not matter.
//  map points: the sides are coupled through l2r / r2l, so the points stay strictly in order, but the two windows of ONE point
//   are walked at once, both against the occupancy as it stands before the point.  The left outcome is final.  The right one
//   is final unless (a) the left pass took the `continue` of :125-126 -- then it is discarded --, or (b) the left pass's
//   partner write CHANGED the occupancy of right slot L.n + l2r in a way the right window can see: the slot became free
//   (has_obs = 0 over an occupied slot: it may now be a candidate), or it became occupied and is the right wave's best or
//   second candidate (any other candidate is irrelevant to the outcome: the dirty rule of k_proj_par within a point).  Then
//   the right window is searched again against the exact occupancy.  Wave 1's first lane commits everything in the
//   reference's order (left slot, its partner, r2l partner, right slot), so a later write to the same slot wins.
template <bool STAGE>
__global__ __launch_bounds__(kRigThreads) void k_rig(const RigArgs* __restrict__ jobs)
{
    const RigArgs A = jobs[blockIdx.x];
    extern __shared__ __align__(16) uint8_t s_dyn[];
    __shared__ int s_hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    __shared__ int s_nm[2];
    __shared__ float s_scale[32];
    __shared__ int s_col[2][32];
    __shared__ unsigned long long s_res[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    ProjFrameDev L = A.L, R = A.R;
    const int nl = L.n, nr = R.n;
    uint8_t* s_occ = s_dyn;
    if (STAGE) {
        uint8_t* p = s_dyn + (((size_t)nl + nr + 15) & ~(size_t)15);
        p = rig_stage_side(L, p, tid);
        p = rig_stage_side(R, p, tid);
    }
    if (tid < L.n_levels && tid < 32) s_scale[tid] = L.scale_factors[tid];      // one table per frame (checked on the host)
    L.scale_factors = s_scale; R.scale_factors = s_scale;
    for (int i = tid; i < nl + nr; i += kRigThreads) s_occ[i] = A.occupied[i];
    if (tid < HISTO_LENGTH) s_hist[tid] = 0;
    __syncthreads();

    if (A.last_mode) {
        uint8_t* occ = s_occ + (wave ? nl : 0);
        const int slot0 = wave ? nl : 0;
        const float* side_angle = wave ? R.angle : L.angle;
        int32_t* log_slot = A.log_slot + (size_t)wave * A.n_pts;
        int32_t* log_bin = A.log_bin + (size_t)wave * A.n_pts;
        int nm = 0, nlog = 0;
        for (int i = 0; i < A.n_pts; i++) {
            if (!A.valid[i]) continue;
            const float x = A.u[i], y = A.v[i];
            if (x < L.min_x || x > L.max_x) continue;                  // :1715-1718: the LEFT projection gates both passes
            if (y < L.min_y || y > L.max_y) continue;
            const int oct = A.level[i];
            const float r = A.th * s_scale[oct];                       // :1724, :1802
            int minLevel, maxLevel;
            if (A.level_window == ORBM_LEVELS_FORWARD) { minLevel = oct; maxLevel = -1; }          // :1729, :1807
            else if (A.level_window == ORBM_LEVELS_BACKWARD) { minLevel = 0; maxLevel = oct; }     // :1731, :1809
            else { minLevel = oct - 1; maxLevel = oct + 1; }                                        // :1733, :1811
            unsigned long long d[4], kb, ks;
            rig_load_desc(A.desc, i, d);
            if (wave == 0) {
                search_window<true>(L, occ, x, y, r, minLevel, maxLevel, 0.f, d, lane, s_col[0], kb, ks);     // (an empty window has no best: :1735 needs no test of its own here)
            } else {
                if (!rig_window_nonempty(L, x, y, r, minLevel, maxLevel, lane)) continue;                      // :1735
                search_window<true>(R, occ, A.u_r[i], A.v_r[i], r, minLevel, maxLevel, 0.f, d, lane, s_col[1], kb, ks);   // no bounds test on the right projection
            }
            if (kb == kNoKey) continue;
            const int bestIdx = key_idx(kb);
            if (key_dist(kb) > TH_HIGH) continue;                      // :1770, :1836
            if (lane == 0) {
                A.assign[slot0 + bestIdx] = i;
                occ[bestIdx] = A.has_obs[i];
                if (A.check_ori) {
                    const int bin = rot_bin(A.angle[i], side_angle[bestIdx]);
                    log_slot[nlog] = slot0 + bestIdx; log_bin[nlog] = bin;
                    atomicAdd(&s_hist[bin], 1);
                }
            }
            nlog++; nm++;
            wave_lds_sync();        // this wave's next window must see the occupancy update (the other wave never reads this half)
        }
        __syncthreads();
        if (A.check_ori) {          // ONE histogram over both sides (:1865-1884)
            if (tid == 0) {
                int i1, i2, i3;
                three_maxima(s_hist, HISTO_LENGTH, i1, i2, i3);
                s_keep[0] = i1; s_keep[1] = i2; s_keep[2] = i3;
            }
            __syncthreads();
            const int i1 = s_keep[0], i2 = s_keep[1], i3 = s_keep[2];
            for (int k0 = 0; k0 < nlog; k0 += 64) {
                const int k = k0 + lane;
                bool drop = false;
                if (k < nlog) {
                    const int b = log_bin[k];
                    drop = b != i1 && b != i2 && b != i3;
                    if (drop) { const int s = log_slot[k]; A.assign[s] = -1; s_occ[s] = 0; }        // mvpMapPoints[...] = NULL (:1879)
                }
                nm -= __popcll(__ballot(drop));
            }
        }
        if (lane == 0) s_nm[wave] = nm;
        __syncthreads();
        if (tid == 0) *A.n_matches = s_nm[0] + s_nm[1];
    } else {
        const bool bFactor = A.th != 1.0f;
        uint8_t* occ_r = s_occ + nl;
        int nm = 0;
        for (int i = 0; i < A.n_pts; i++) {
            const int inL = A.valid[i], inR = A.valid_r[i];
            if (!inL && !inR) continue;                                // :52
            if (A.far_points && A.depth[i] > A.th_far) continue;       // :55
            if (A.bad[i]) continue;                                    // :58
            const int lvlR = A.level_r[i];
            const bool doR = inR && lvlR != -1;                        // :144-146
            unsigned long long d[4], kb = kNoKey, ks = kNoKey;
            rig_load_desc(A.desc, i, d);
            float xr = 0.f, yr = 0.f, rr = 0.f;
            if (wave == 0) {
                if (inL) {
                    const int lvl = A.level[i];
                    float r = ((double)A.view_cos[i] > 0.998) ? 2.5f : 4.0f;       // RadiusByViewingCos (:215-221)
                    if (bFactor) r *= A.th;
                    r = r * s_scale[lvl];
                    search_window<true>(L, s_occ, A.u[i], A.v[i], r, lvl - 1, lvl, 0.f, d, lane, s_col[0], kb, ks);
                }
                if (lane == 0) { s_res[0] = kb; s_res[1] = ks; }
            } else if (doR) {
                rr = ((double)A.view_cos_r[i] > 0.998) ? 2.5f : 4.0f;              // :147: th is not applied
                rr = rr * s_scale[lvlR];
                xr = A.u_r[i]; yr = A.v_r[i];
                search_window<true>(R, occ_r, xr, yr, rr, lvlR - 1, lvlR, 0.f, d, lane, s_col[1], kb, ks);
            }
            __syncthreads();
            if (wave == 1) {
                const unsigned long long lb = s_res[0], ls = s_res[1];
                const uint8_t ho = A.has_obs[i];
                bool cancel = false, dirty = false;
                if (lb != kNoKey && key_dist(lb) <= TH_HIGH) {         // :123
                    const int bi = key_idx(lb);
                    const int bd2 = (ls == kNoKey) ? 256 : key_dist(ls);
                    const int lev = L.octave[bi], lev2 = (ls == kNoKey) ? -1 : L.octave[key_idx(ls)];
                    if (lev == lev2 && (float)key_dist(lb) > A.nnratio * (float)bd2) cancel = true;     // :125-126: `continue` takes the right pass with it
                    else {
                        const int p = A.l2r[bi];
                        const bool was = (p != -1) ? occ_r[p] != 0 : ho != 0;
                        if (lane == 0) {
                            A.assign[bi] = i; s_occ[bi] = ho;                          // :129
                            if (p != -1) { A.assign[nl + p] = i; occ_r[p] = ho; }      // :131-135, unconditional
                        }
                        nm += (p != -1) ? 2 : 1;
                        if (doR && p != -1 && was != (ho != 0))
                            dirty = !ho || (kb != kNoKey && key_idx(kb) == p) || (ks != kNoKey && key_idx(ks) == p);
                    }
                }
                if (!cancel && doR) {
                    if (dirty) {
                        wave_lds_sync();
                        search_window<true>(R, occ_r, xr, yr, rr, lvlR - 1, lvlR, 0.f, d, lane, s_col[1], kb, ks);
                    }
                    if (kb != kNoKey && key_dist(kb) <= TH_HIGH) {     // :193
                        const int bi = key_idx(kb);
                        const int bd2 = (ks == kNoKey) ? 256 : key_dist(ks);
                        const int lev = R.octave[bi], lev2 = (ks == kNoKey) ? -1 : R.octave[key_idx(ks)];
                        if (!(lev == lev2 && (float)key_dist(kb) > A.nnratio * (float)bd2)) {          // :195
                            const int q = A.r2l[bi];
                            if (lane == 0) {
                                if (q != -1) { A.assign[q] = i; s_occ[q] = ho; }       // :198-202
                                A.assign[nl + bi] = i; occ_r[bi] = ho;                 // :205
                            }
                            nm += (q != -1) ? 2 : 1;
                        }
                    }
                }
            }
            __syncthreads();        // the occupancy updates must be seen by the next point's two windows
        }
        if (tid == 64) *A.n_matches = nm;
    }
    __syncthreads();
    for (int i = tid; i < nl + nr; i += kRigThreads) A.occupied[i] = s_occ[i];
}

// ---- device-resident batch of the two rig searches (include/orbslam3_hip_rig_track_device.h, DESIGN.md 4p) -----------------------
// The rig twin of k_proj_dev_setup: the frames are what the two extractors and the rig's stereo step left in HBM.  One workgroup per
// frame turns both sides' OrbxKeyPoint records into the SoA arrays and writes the frame's RigArgs and the two ProjArgs k_grid reads
// ON THE DEVICE.  What the host entries refuse, this kernel clamps (the counts never visit the host): counts into [0, cap], partner
// entries outside [-1, n_other) to -1, levels to the table (-1 stays on the right: no right pass).
struct RigDevSide { const OrbxKeyPoint* kps; const uint8_t* desc; const int32_t* n; const int32_t* partner; int32_t cap;
                    float* x; float* y; int32_t* oct; float* ang; int32_t* cell_off; int32_t* cell_feat; int32_t* partner_out; };
struct RigDevSetup {
    RigDevSide side[2];
    // the points: fields of RigArgs, [batch][p_cap]
    const uint8_t* p_valid; const float* p_u; const float* p_v; const int32_t* p_level; const float* p_vcos;
    const uint8_t* p_valid_r; const float* p_u_r; const float* p_v_r; const int32_t* p_level_r; const float* p_vcos_r;
    const float* p_depth; const uint8_t* p_bad; const float* p_angle; const uint8_t* p_desc; const uint8_t* p_obs; const int32_t* p_n; int32_t p_cap;
    const int32_t* level_window;                        // [batch] or nullptr
    int32_t* level; int32_t* level_r; uint8_t* obs_ones; int32_t* log_slot; int32_t* log_bin;      // scratch: [batch][p_cap], the logs [batch][2 * p_cap]
    const float* scale; int32_t n_levels, cols, rows;
    float min_x, min_y, max_x, max_y, th, th_far, nnratio;
    int32_t far_points, check_ori, last_mode, slot_cap;
    int32_t* assign; uint8_t* occupied; int32_t* n_matches; int32_t* n_slots;
    RigArgs* jobs; ProjArgs* grids;                     // [batch], [2 * batch]: left side of frame b at 2b
};
__global__ __launch_bounds__(256) void k_rig_dev_setup(RigDevSetup P)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    int n[2];
    for (int s = 0; s < 2; s++) n[s] = min(max(P.side[s].n[b], 0), P.side[s].cap);
    const int n_pts = min(max(P.p_n[b], 0), P.p_cap);
    const size_t cells = (size_t)P.cols * P.rows, prow = (size_t)b * P.p_cap;
    for (int s = 0; s < 2; s++) {
        const RigDevSide& S = P.side[s];
        const size_t row = (size_t)b * S.cap;
        const int n_other = n[s ^ 1];
        for (int i = tid; i < n[s]; i += 256) {
            const OrbxKeyPoint k = S.kps[row + i];
            S.x[row + i] = k.x; S.y[row + i] = k.y; S.oct[row + i] = k.octave; S.ang[row + i] = k.angle;
            const int p = S.partner[row + i];
            S.partner_out[row + i] = (p < -1 || p >= n_other) ? -1 : p;
        }
    }
    for (int i = tid; i < n_pts; i += 256) {
        P.level[prow + i] = min(max(P.p_level[prow + i], 0), P.n_levels - 1);
        if (P.level_r) { const int l = P.p_level_r[prow + i]; P.level_r[prow + i] = l == -1 ? -1 : min(max(l, 0), P.n_levels - 1); }
        if (P.obs_ones) P.obs_ones[prow + i] = 1;
    }
    if (tid == 0) {
        RigArgs A;
        for (int s = 0; s < 2; s++) {
            const RigDevSide& S = P.side[s];
            const size_t row = (size_t)b * S.cap;
            ProjFrameDev& F = s ? A.R : A.L;
            F.x = S.x + row; F.y = S.y + row; F.octave = S.oct + row; F.angle = S.ang + row; F.desc = S.desc + row * 32;
            F.cell_off = S.cell_off + (size_t)b * (cells + 1); F.cell_feat = S.cell_feat + row;
            F.scale_factors = P.scale;
            F.min_x = P.min_x; F.min_y = P.min_y; F.max_x = P.max_x; F.max_y = P.max_y;
            F.winv = (float)P.cols / (P.max_x - P.min_x); F.hinv = (float)P.rows / (P.max_y - P.min_y);        // mfGridElementWidthInv / HeightInv
            F.n = n[s]; F.cols = P.cols; F.rows = P.rows; F.n_levels = P.n_levels; F.u_right = nullptr;
            ProjArgs G = ProjArgs{};
            G.F = F;
            P.grids[2 * (size_t)b + s] = G;
        }
        A.l2r = P.side[0].partner_out + (size_t)b * P.side[0].cap; A.r2l = P.side[1].partner_out + (size_t)b * P.side[1].cap;
        A.n_pts = n_pts;
        A.valid = P.p_valid + prow; A.u = P.p_u + prow; A.v = P.p_v + prow; A.level = P.level + prow;
        A.u_r = P.p_u_r + prow; A.v_r = P.p_v_r + prow;
        A.view_cos = P.p_vcos ? P.p_vcos + prow : nullptr; A.valid_r = P.p_valid_r ? P.p_valid_r + prow : nullptr;
        A.level_r = P.level_r ? P.level_r + prow : nullptr; A.view_cos_r = P.p_vcos_r ? P.p_vcos_r + prow : nullptr;
        A.depth = P.p_depth ? P.p_depth + prow : nullptr; A.bad = P.p_bad ? P.p_bad + prow : nullptr;
        A.angle = P.p_angle ? P.p_angle + prow : nullptr;
        A.desc = P.p_desc + prow * 32; A.has_obs = P.p_obs ? P.p_obs + prow : P.obs_ones + prow;
        A.th = P.th; A.th_far = P.th_far; A.nnratio = P.nnratio; A.far_points = P.far_points; A.check_ori = P.check_ori;
        A.level_window = P.level_window ? P.level_window[b] : ORBM_LEVELS_AROUND;      // (k_rig takes anything else as _AROUND too)
        A.last_mode = P.last_mode;
        A.assign = P.assign + (size_t)b * P.slot_cap; A.occupied = P.occupied + (size_t)b * P.slot_cap;
        A.log_slot = P.log_slot ? P.log_slot + 2 * prow : nullptr; A.log_bin = P.log_bin ? P.log_bin + 2 * prow : nullptr;
        A.n_matches = P.n_matches + b;
        P.jobs[b] = A;
        if (P.n_slots) P.n_slots[b] = n[0] + n[1];
    }
}

}  // namespace orbm

// one rig search problem; host pointers
struct RigJob {
    const OrbmRigFrame* rig;
    const OrbmRigMapPoints* mp;         // exactly one of mp / last
    const OrbmRigLastPoints* last;
    int level_window;
    int32_t* assign; uint8_t* occupied;
    int n_matches;                      // out
};

static const char* const kRigSide[2] = {"rig left: ", "rig right: "};      // check_frame's and stage_frame's `who`

static int rig_check(const OrbmRigFrame* rig, const OrbmRigMapPoints* mp, const OrbmRigLastPoints* last, const int32_t* assign, const uint8_t* occupied)
{
    if (!rig) return fail(ORBX_ERR_ARG, "NULL rig frame");
    if ((mp != nullptr) == (last != nullptr)) return fail(ORBX_ERR_ARG, "exactly one of the map points and the last-frame points is given");
    if (!assign || !occupied) return fail(ORBX_ERR_ARG, "NULL assign/occupied");
    const OrbmFrame& l = rig->left; const OrbmFrame& r = rig->right;
    if (int e = check_frame(&l, kRigSide[0], 32)) return e;           // (k_rig keeps the one scale table in 32 floats of LDS)
    if (int e = check_frame(&r, kRigSide[1], 32)) return e;
    if (l.u_right) return fail(ORBX_ERR_ARG, "a rig frame has no u_right (left.u_right must be NULL)");
    if (!(l.min_x == r.min_x && l.min_y == r.min_y && l.max_x == r.max_x && l.max_y == r.max_y)) return fail(ORBX_ERR_ARG, "the two sides disagree in the image bounds");
    if (l.grid_cols != r.grid_cols || l.grid_rows != r.grid_rows) return fail(ORBX_ERR_ARG, "the two sides disagree in the grid");
    if (l.n_levels != r.n_levels) return fail(ORBX_ERR_ARG, "the two sides disagree in n_levels");
    for (int k = 0; k < l.n_levels; k++)
        if (!(l.scale_factors[k] == r.scale_factors[k])) return fail(ORBX_ERR_ARG, "the two sides disagree in scale factor %d", k);
    if ((l.n > 0 && !rig->left_to_right) || (r.n > 0 && !rig->right_to_left)) return fail(ORBX_ERR_ARG, "NULL left_to_right / right_to_left");
    for (int i = 0; i < l.n; i++)
        if (rig->left_to_right[i] < -1 || rig->left_to_right[i] >= r.n) return fail(ORBX_ERR_ARG, "left_to_right[%d] = %d outside [-1, %d)", i, rig->left_to_right[i], r.n);
    for (int i = 0; i < r.n; i++)
        if (rig->right_to_left[i] < -1 || rig->right_to_left[i] >= l.n) return fail(ORBX_ERR_ARG, "right_to_left[%d] = %d outside [-1, %d)", i, rig->right_to_left[i], l.n);
    const int nlv = l.n_levels;
    if (mp) {
        if (mp->n < 0) return fail(ORBX_ERR_ARG, "negative point count");
        if (mp->n > 0 && (!mp->in_view || !mp->proj_u || !mp->proj_v || !mp->pred_level || !mp->view_cos || !mp->in_view_r || !mp->proj_u_r || !mp->proj_v_r ||
                          !mp->pred_level_r || !mp->view_cos_r || !mp->track_depth || !mp->bad || !mp->has_obs || !mp->desc))
            return fail(ORBX_ERR_ARG, "NULL map point arrays");
        for (int i = 0; i < mp->n; i++) {
            if (mp->in_view[i] && (mp->pred_level[i] < 0 || mp->pred_level[i] >= nlv)) return fail(ORBX_ERR_ARG, "point %d: level %d out of range", i, mp->pred_level[i]);
            if (mp->in_view_r[i] && (mp->pred_level_r[i] < -1 || mp->pred_level_r[i] >= nlv)) return fail(ORBX_ERR_ARG, "point %d: right level %d out of range", i, mp->pred_level_r[i]);
        }
    } else {
        if (last->n < 0) return fail(ORBX_ERR_ARG, "negative point count");
        if (last->n > 0 && (!last->valid || !last->proj_u || !last->proj_v || !last->proj_u_r || !last->proj_v_r || !last->octave || !last->has_obs || !last->desc))
            return fail(ORBX_ERR_ARG, "NULL last-frame point arrays");
        for (int i = 0; i < last->n; i++)
            if (last->valid[i] && (last->octave[i] < 0 || last->octave[i] >= nlv)) return fail(ORBX_ERR_ARG, "entry %d: octave %d out of range", i, last->octave[i]);
    }
    return ORBX_OK;
}
// Packs all jobs into one blob; ONE k_grid launch over the 2 x n_jobs sides, ONE k_rig launch with a workgroup per rig frame;
// one copy brings assign / occupied / counts back.
static int run_rig_jobs(orbm_matcher* m, RigJob* jobs, int n_jobs, int last_mode, float th, int far_points, float th_far, float nnratio, int check_ori)
{
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    if (!jobs || n_jobs < 1) return fail(ORBX_ERR_ARG, "no jobs");
    for (int j = 0; j < n_jobs; j++) {
        const RigJob& q = jobs[j];
        if (int e = rig_check(q.rig, last_mode ? nullptr : q.mp, last_mode ? q.last : nullptr, q.assign, q.occupied)) return e;
        if (last_mode) {
            if (q.level_window < ORBM_LEVELS_AROUND || q.level_window > ORBM_LEVELS_BACKWARD) return fail(ORBX_ERR_ARG, "job %d: bad level_window %d", j, q.level_window);
            if (check_ori && q.last->n > 0 && (!q.last->angle || (q.rig->left.n > 0 && !q.rig->left.angle) || (q.rig->right.n > 0 && !q.rig->right.angle)))
                return fail(ORBX_ERR_ARG, "job %d: NULL angle arrays", j);
        }
    }
    ORBX_HIP(hipSetDevice(m->device));
    (void)hipGetLastError();
    const size_t lds_budget = dynamic_lds_budget<orbm::k_rig<true>, orbm::k_rig<false>>();
    Blob blob(m);
    std::vector<orbm::RigArgs> args(n_jobs);
    const size_t oargs = blob.slot<orbm::RigArgs>(n_jobs);
    const size_t ogrid = blob.slot<orbm::ProjArgs>((size_t)n_jobs * 2);        // k_grid's jobs: the sides as frames
    size_t max_n = 0, lds_full = 0, lds_occ = 64;
    bool device_grid = true;            // Frame::AssignFeaturesToGrid of both sides on the device (k_grid) when every side fits its LDS sort
    for (int j = 0; j < n_jobs; j++) device_grid = device_grid && jobs[j].rig->left.n <= 8192 && jobs[j].rig->right.n <= 8192;
    for (int j = 0; j < n_jobs; j++) {
        const RigJob& q = jobs[j];
        orbm::RigArgs& A = args[j];
        const OrbmFrame* side[2] = {&q.rig->left, &q.rig->right};
        for (int s = 0; s < 2; s++)     // (the one scale table of the frame follows the sides)
            if (int e = stage_frame(blob, side[s], device_grid, s ? A.R : A.L, true, false, kRigSide[s], 32)) return e;
        const int nl = side[0]->n, nr = side[1]->n, ncell = side[0]->grid_cols * side[0]->grid_rows;
        const size_t slots = (size_t)nl + nr;
        max_n = std::max(max_n, (size_t)std::max(nl, nr));
        if (slots + 256 > lds_budget) return fail(ORBX_ERR_ARG, "rig frame with %d + %d features exceeds the LDS occupancy table", nl, nr);
        lds_occ = std::max(lds_occ, (slots + 63) & ~(size_t)63);
        lds_full = std::max(lds_full, ((slots + 15) & ~(size_t)15) + orbm::rig_side_bytes(nl, ncell) + orbm::rig_side_bytes(nr, ncell));
        blob.in(A.L.scale_factors, side[0]->scale_factors, side[0]->n_levels); blob.alias(A.R.scale_factors, A.L.scale_factors);
        A.L.n_levels = A.R.n_levels = side[0]->n_levels;
        blob.in(A.l2r, q.rig->left_to_right, nl); blob.in(A.r2l, q.rig->right_to_left, nr);
        if (!last_mode) {
            const OrbmRigMapPoints* p = q.mp;
            const size_t n = p->n;
            A.n_pts = p->n;
            blob.in(A.valid, p->in_view, n); blob.in(A.u, p->proj_u, n); blob.in(A.v, p->proj_v, n);
            blob.in(A.level, p->pred_level, n); blob.in(A.view_cos, p->view_cos, n);
            blob.in(A.valid_r, p->in_view_r, n); blob.in(A.u_r, p->proj_u_r, n); blob.in(A.v_r, p->proj_v_r, n);
            blob.in(A.level_r, p->pred_level_r, n); blob.in(A.view_cos_r, p->view_cos_r, n);
            blob.in(A.depth, p->track_depth, n); blob.in(A.bad, p->bad, n);
            blob.in(A.desc, p->desc, 32 * n); blob.in(A.has_obs, p->has_obs, n);
            blob.none(A.angle, A.log_slot, A.log_bin);
        } else {
            const OrbmRigLastPoints* p = q.last;
            const size_t n = p->n;
            A.n_pts = p->n;
            blob.in(A.valid, p->valid, n); blob.in(A.u, p->proj_u, n); blob.in(A.v, p->proj_v, n);
            blob.in(A.u_r, p->proj_u_r, n); blob.in(A.v_r, p->proj_v_r, n);
            blob.in(A.level, p->octave, n); blob.in_opt(A.angle, p->angle, n);
            blob.in(A.desc, p->desc, 32 * n); blob.in(A.has_obs, p->has_obs, n);
            blob.out(A.log_slot, 2 * std::max(n, (size_t)1)); blob.out(A.log_bin, 2 * std::max(n, (size_t)1));
            blob.none(A.view_cos, A.valid_r, A.level_r, A.view_cos_r, A.depth, A.bad);
        }
        A.th = th; A.th_far = th_far; A.nnratio = nnratio; A.far_points = far_points; A.check_ori = check_ori;
        A.level_window = q.level_window; A.last_mode = last_mode;
    }
    // in/out and output arrays of all jobs sit together at the end: one copy brings every result back
    const size_t out_begin = blob.begin_out();
    for (int j = 0; j < n_jobs; j++) {
        const size_t slots = (size_t)jobs[j].rig->left.n + jobs[j].rig->right.n;
        blob.inout(args[j].assign, jobs[j].assign, slots); blob.inout(args[j].occupied, jobs[j].occupied, slots);
        blob.out(args[j].n_matches, 1);
    }
    if (int e = m->ensure(blob.size())) return e;
    blob.bind(m->d_blob);
    blob.store(oargs, args.data(), n_jobs);
    orbm::ProjArgs* grids = (orbm::ProjArgs*)(m->h_blob.data() + ogrid);
    for (int j = 0; j < n_jobs; j++) {
        grids[2 * j] = orbm::ProjArgs{}; grids[2 * j].F = args[j].L;
        grids[2 * j + 1] = orbm::ProjArgs{}; grids[2 * j + 1].F = args[j].R;
    }
    const bool stage = lds_full <= lds_budget;      // selected per launch: every frame of the batch fits, or none is staged
    const size_t lds = stage ? lds_full : lds_occ;
    uint8_t* base = m->d_blob;
    if (int e = m->rig_timer.create()) return e;
    ORBX_HIP(hipMemcpyAsync(base, m->h_blob.data(), blob.size(), hipMemcpyHostToDevice, m->stream));
    if (int e = m->rig_timer.start(m->stream)) return e;
    if (device_grid)
        if (int e = launch_grid(m->stream, blob.device<orbm::ProjArgs>(ogrid), 2 * n_jobs, max_n)) return e;
    if (int e = launch_staged(orbm::k_rig<true>, orbm::k_rig<false>, stage, n_jobs, orbm::kRigThreads, lds, m->stream, blob.device<orbm::RigArgs>(oargs))) return e;
    ORBX_HIP(hipGetLastError());
    if (int e = m->rig_timer.stop(m->stream)) return e;
    ORBX_HIP(hipMemcpyAsync(m->h_blob.data() + out_begin, base + out_begin, blob.size() - out_begin, hipMemcpyDeviceToHost, m->stream));
    ORBX_HIP(hipStreamSynchronize(m->stream));
    if (int e = m->rig_timer.read()) return e;
    for (int j = 0; j < n_jobs; j++) {
        const size_t slots = (size_t)jobs[j].rig->left.n + jobs[j].rig->right.n;
        if (slots > 0) {
            std::memcpy(jobs[j].assign, blob.host(args[j].assign), sizeof(int32_t) * slots);
            std::memcpy(jobs[j].occupied, blob.host(args[j].occupied), slots);
        }
        std::memcpy(&jobs[j].n_matches, blob.host(args[j].n_matches), sizeof(int32_t));
    }
    return ORBX_OK;
}

// ---- the device-resident entries: checks on the host, then setup + grid + search enqueued on the caller's stream ----
static int rig_dev_check(const OrbmDeviceRigFrames* f, const OrbmDeviceRigLastPoints* last, const OrbmDeviceRigMapPoints* mp, int batch)
{
    if (!f) return fail(ORBX_ERR_ARG, "NULL rig frames");
    if ((mp != nullptr) == (last != nullptr)) return fail(ORBX_ERR_ARG, "exactly one of the map points and the last-frame points is given");
    if (batch < 1) return fail(ORBX_ERR_ARG, "batch %d", batch);
    if (!f->d_kps_l || !f->d_desc_l || !f->d_n_l || !f->d_kps_r || !f->d_desc_r || !f->d_n_r || !f->d_left_to_right || !f->d_right_to_left || !f->scale_factors)
        return fail(ORBX_ERR_ARG, "NULL rig frame arrays");
    if (f->cap_l < 1 || f->cap_r < 1) return fail(ORBX_ERR_ARG, "capacities %d + %d", f->cap_l, f->cap_r);
    if ((int64_t)f->slot_cap < (int64_t)f->cap_l + f->cap_r) return fail(ORBX_ERR_ARG, "slot_cap %d below cap_l + cap_r = %d + %d", f->slot_cap, f->cap_l, f->cap_r);
    if (f->n_levels < 1 || f->n_levels > 32) return fail(ORBX_ERR_ARG, "n_levels %d outside [1, 32]", f->n_levels);
    if (f->grid_cols < 1 || f->grid_rows < 1 || f->grid_cols * (int64_t)f->grid_rows > (1 << 20) || !(f->max_x > f->min_x) || !(f->max_y > f->min_y)) return fail(ORBX_ERR_ARG, "bad frame grid");
    if (last) {
        if (!last->d_valid || !last->d_u || !last->d_v || !last->d_u_r || !last->d_v_r || !last->d_octave || !last->d_desc || !last->d_n) return fail(ORBX_ERR_ARG, "NULL last-frame point arrays");
        if (last->cap < 1) return fail(ORBX_ERR_ARG, "point capacity %d", last->cap);
    } else {
        if (!mp->d_in_view || !mp->d_u || !mp->d_v || !mp->d_pred_level || !mp->d_view_cos || !mp->d_in_view_r || !mp->d_u_r || !mp->d_v_r || !mp->d_pred_level_r ||
            !mp->d_view_cos_r || !mp->d_track_depth || !mp->d_bad || !mp->d_has_obs || !mp->d_desc || !mp->d_n) return fail(ORBX_ERR_ARG, "NULL map point arrays");
        if (mp->cap < 1) return fail(ORBX_ERR_ARG, "point capacity %d", mp->cap);
    }
    if (f->cap_l > 8192 || f->cap_r > 8192) return fail(ORBX_ERR_CAPACITY, "at most 8192 features per side (the grid is sorted in LDS)");
    if ((size_t)f->cap_l + f->cap_r + 256 > dynamic_lds_budget<orbm::k_rig<true>, orbm::k_rig<false>>())
        return fail(ORBX_ERR_CAPACITY, "rig frames of %d + %d features exceed the LDS occupancy table", f->cap_l, f->cap_r);
    return ORBX_OK;
}

static int rig_search_batch_device(orbm_matcher* m, const OrbmDeviceRigFrames* f, const OrbmDeviceRigLastPoints* last, const OrbmDeviceRigMapPoints* mp, int batch,
                                   float th, int check_ori, int32_t* d_assign, uint8_t* d_occupied, int32_t* d_n_matches, int32_t* d_n_slots, void* stream)
{
    if (int e = rig_dev_check(f, last, mp, batch)) return e;
    if (!d_assign || !d_occupied || !d_n_matches) return fail(ORBX_ERR_ARG, "NULL assign / occupied / n_matches");
    if (last && check_ori && !last->d_angle) return fail(ORBX_ERR_ARG, "check_orientation needs d_angle");
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    ORBX_HIP(hipSetDevice(m->device));
    hipStream_t st = (hipStream_t)stream;
    const size_t B = (size_t)batch, cap[2] = {(size_t)f->cap_l, (size_t)f->cap_r}, pcap = (size_t)(last ? last->cap : mp->cap);
    const int ncell = f->grid_cols * f->grid_rows;
    const bool ones = last && !last->d_has_obs;
    auto al = [](size_t v) { return (v + 255) & ~(size_t)255; };
    size_t off = 0;
    auto take = [&](size_t bytes) { const size_t o = off; off += al(bytes); return o; };
    size_t o_x[2], o_y[2], o_oct[2], o_ang[2], o_coff[2], o_cfeat[2], o_partner[2];
    for (int s = 0; s < 2; s++) {
        o_x[s] = take(B * cap[s] * 4); o_y[s] = take(B * cap[s] * 4); o_oct[s] = take(B * cap[s] * 4); o_ang[s] = take(B * cap[s] * 4);
        o_coff[s] = take(B * ((size_t)ncell + 1) * 4); o_cfeat[s] = take(B * cap[s] * 4); o_partner[s] = take(B * cap[s] * 4);
    }
    const size_t o_level = take(B * pcap * 4), o_level_r = take(mp ? B * pcap * 4 : 0), o_ones = take(ones ? B * pcap : 0);
    const size_t o_ls = take(last ? 2 * B * pcap * 4 : 0), o_lb = take(last ? 2 * B * pcap * 4 : 0);
    const size_t o_jobs = take(B * sizeof(orbm::RigArgs)), o_grids = take(2 * B * sizeof(orbm::ProjArgs));
    if (int e = reserve_workspace(m, off)) return e;
    if (int e = scale_factors_to_device(m, f->scale_factors, f->n_levels, st)) return e;
    uint8_t* w = m->d_ws;
    orbm::RigDevSetup P;
    std::memset(&P, 0, sizeof(P));
    const OrbxKeyPoint* kps[2] = {f->d_kps_l, f->d_kps_r}; const uint8_t* desc[2] = {f->d_desc_l, f->d_desc_r};
    const int32_t* n[2] = {f->d_n_l, f->d_n_r}; const int32_t* partner[2] = {f->d_left_to_right, f->d_right_to_left};
    for (int s = 0; s < 2; s++)
        P.side[s] = orbm::RigDevSide{kps[s], desc[s], n[s], partner[s], (int32_t)cap[s], (float*)(w + o_x[s]), (float*)(w + o_y[s]), (int32_t*)(w + o_oct[s]),
                                     (float*)(w + o_ang[s]), (int32_t*)(w + o_coff[s]), (int32_t*)(w + o_cfeat[s]), (int32_t*)(w + o_partner[s])};
    if (last) {
        P.p_valid = last->d_valid; P.p_u = last->d_u; P.p_v = last->d_v; P.p_u_r = last->d_u_r; P.p_v_r = last->d_v_r; P.p_level = last->d_octave;
        P.p_angle = last->d_angle; P.p_desc = last->d_desc; P.p_obs = last->d_has_obs; P.p_n = last->d_n; P.level_window = last->d_level_window;
        P.log_slot = (int32_t*)(w + o_ls); P.log_bin = (int32_t*)(w + o_lb);
        if (ones) P.obs_ones = w + o_ones;
    } else {
        P.p_valid = mp->d_in_view; P.p_u = mp->d_u; P.p_v = mp->d_v; P.p_level = mp->d_pred_level; P.p_vcos = mp->d_view_cos;
        P.p_valid_r = mp->d_in_view_r; P.p_u_r = mp->d_u_r; P.p_v_r = mp->d_v_r; P.p_level_r = mp->d_pred_level_r; P.p_vcos_r = mp->d_view_cos_r;
        P.p_depth = mp->d_track_depth; P.p_bad = mp->d_bad; P.p_desc = mp->d_desc; P.p_obs = mp->d_has_obs; P.p_n = mp->d_n;
        P.level_r = (int32_t*)(w + o_level_r);
        P.th_far = mp->th_far; P.nnratio = mp->nnratio; P.far_points = mp->far_points;
    }
    P.p_cap = (int32_t)pcap; P.level = (int32_t*)(w + o_level);
    P.scale = m->d_scale; P.n_levels = f->n_levels; P.cols = f->grid_cols; P.rows = f->grid_rows;
    P.min_x = f->min_x; P.min_y = f->min_y; P.max_x = f->max_x; P.max_y = f->max_y; P.th = th;
    P.check_ori = last && check_ori ? 1 : 0; P.last_mode = last ? 1 : 0; P.slot_cap = f->slot_cap;
    P.assign = d_assign; P.occupied = d_occupied; P.n_matches = d_n_matches; P.n_slots = d_n_slots;
    P.jobs = (orbm::RigArgs*)(w + o_jobs); P.grids = (orbm::ProjArgs*)(w + o_grids);
    // staged or not by the capacities, with run_rig_jobs' arithmetic over the counts: every frame of the batch fits, or none is staged
    const size_t slots = cap[0] + cap[1];
    const size_t lds_occ = std::max((size_t)64, (slots + 63) & ~(size_t)63);
    const size_t lds_full = ((slots + 15) & ~(size_t)15) + orbm::rig_side_bytes((int)cap[0], ncell) + orbm::rig_side_bytes((int)cap[1], ncell);
    const bool stage = lds_full <= dynamic_lds_budget<orbm::k_rig<true>, orbm::k_rig<false>>();
    hipLaunchKernelGGL(orbm::k_rig_dev_setup, dim3(batch), dim3(256), 0, st, P);
    if (int e = launch_grid(st, P.grids, 2 * batch, std::max(cap[0], cap[1]))) return e;
    if (int e = launch_staged(orbm::k_rig<true>, orbm::k_rig<false>, stage, batch, orbm::kRigThreads, stage ? lds_full : lds_occ, st, (const orbm::RigArgs*)P.jobs)) return e;
    ORBX_HIP(hipGetLastError());
    return ORBX_OK;
}


extern "C" {

int orbm_rig_search_device_check(const OrbmDeviceRigFrames* frames, const OrbmDeviceRigLastPoints* last, const OrbmDeviceRigMapPoints* mp, int batch)
{
    return rig_dev_check(frames, last, mp, batch);
}

int orbm_search_by_projection_last_rig_batch_device(orbm_matcher* m, const OrbmDeviceRigFrames* frames, const OrbmDeviceRigLastPoints* last, int batch,
        float th, int check_orientation, int32_t* d_assign, uint8_t* d_occupied, int32_t* d_n_matches, int32_t* d_n_slots, void* stream)
{
    return rig_search_batch_device(m, frames, last, nullptr, batch, th, check_orientation, d_assign, d_occupied, d_n_matches, d_n_slots, stream);
}

int orbm_search_by_projection_rig_batch_device(orbm_matcher* m, const OrbmDeviceRigFrames* frames, const OrbmDeviceRigMapPoints* points, int batch,
        float th, int32_t* d_assign, uint8_t* d_occupied, int32_t* d_n_matches, int32_t* d_n_slots, void* stream)
{
    return rig_search_batch_device(m, frames, nullptr, points, batch, th, 0, d_assign, d_occupied, d_n_matches, d_n_slots, stream);
}

int orbm_rig_search_check(const OrbmRigFrame* rig, const OrbmRigMapPoints* mp, const OrbmRigLastPoints* last, const int32_t* assign, const uint8_t* occupied)
{
    return rig_check(rig, mp, last, assign, occupied);
}

int orbm_search_by_projection_rig(orbm_matcher* m, const OrbmRigFrame* rig, const OrbmRigMapPoints* pts, float th, int far_points, float th_far, float nnratio,
                                  int32_t* assign, uint8_t* occupied)
{
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    if (!pts) return fail(ORBX_ERR_ARG, "NULL map points");
    RigJob q{rig, pts, nullptr, 0, assign, occupied, 0};
    const int r = run_rig_jobs(m, &q, 1, 0, th, far_points, th_far, nnratio, 0);
    return r ? r : q.n_matches;
}

int orbm_search_by_projection_last_rig(orbm_matcher* m, const OrbmRigFrame* rig, const OrbmRigLastPoints* pts, float th, int level_window, int check_orientation,
                                       int32_t* assign, uint8_t* occupied)
{
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    if (!pts) return fail(ORBX_ERR_ARG, "NULL last-frame points");
    RigJob q{rig, nullptr, pts, level_window, assign, occupied, 0};
    const int r = run_rig_jobs(m, &q, 1, 1, th, 0, 0.f, 0.f, check_orientation ? 1 : 0);
    return r ? r : q.n_matches;
}

int orbm_search_by_projection_rig_batch(orbm_matcher* m, OrbmRigMapQuery* queries, int n_frames, float th, int far_points, float th_far, float nnratio)
{
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    if (!queries || n_frames < 1) return fail(ORBX_ERR_ARG, "no queries");
    std::vector<RigJob> jobs(n_frames);
    for (int j = 0; j < n_frames; j++) {
        if (!queries[j].pts) return fail(ORBX_ERR_ARG, "query %d: NULL map points", j);
        jobs[j] = RigJob{queries[j].rig, queries[j].pts, nullptr, 0, queries[j].assign, queries[j].occupied, 0};
    }
    if (int r = run_rig_jobs(m, jobs.data(), n_frames, 0, th, far_points, th_far, nnratio, 0)) return r;
    for (int j = 0; j < n_frames; j++) queries[j].n_matches = jobs[j].n_matches;
    return ORBX_OK;
}

int orbm_search_by_projection_last_rig_batch(orbm_matcher* m, OrbmRigLastQuery* queries, int n_frames, float th, int check_orientation)
{
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    if (!queries || n_frames < 1) return fail(ORBX_ERR_ARG, "no queries");
    std::vector<RigJob> jobs(n_frames);
    for (int j = 0; j < n_frames; j++) {
        if (!queries[j].pts) return fail(ORBX_ERR_ARG, "query %d: NULL last-frame points", j);
        jobs[j] = RigJob{queries[j].rig, nullptr, queries[j].pts, queries[j].level_window, queries[j].assign, queries[j].occupied, 0};
    }
    if (int r = run_rig_jobs(m, jobs.data(), n_frames, 1, th, 0, 0.f, 0.f, check_orientation ? 1 : 0)) return r;
    for (int j = 0; j < n_frames; j++) queries[j].n_matches = jobs[j].n_matches;
    return ORBX_OK;
}

float orbm_rig_search_last_kernel_ms(const orbm_matcher* m) { return m ? m->rig_timer.ms : 0.f; }

}  // extern "C"
