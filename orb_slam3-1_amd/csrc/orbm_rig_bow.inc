// SearchByBoW(KeyFrame*, Frame&) and SearchForTriangulation for two-camera fisheye rigs (include/orbslam3_hip_rig_bow.h, which
// restates the reference's branches).  Included by orbm_matcher.hip after its kernels and host helpers.
#include "kb8_stereo_geometry.h"

namespace orbm {

// ---- SearchByBoW, F.Nleft != -1 (src/ORBmatcher.cc:296-323, :357-386) -------------------------------------------------------------
struct RigBowPairDev {
    // side 1 = KeyFrame, side 2 = Frame; feature indices of side 2 below n_left are the left camera's
    const uint8_t* d1; const uint8_t* v1; const float* a1; const uint32_t* node1; const int32_t* off1; const uint32_t* feat1;
    const uint8_t* d2; const float* a2; const uint32_t* node2; const int32_t* off2; const uint32_t* feat2;
    int32_t n1, n2, n_left, nn1, nn2, serial;
    int32_t* match;         // [n2] Frame slot -> KF feature
    int32_t* n_matches;
};

constexpr unsigned kBowNoKey = 0xFFFFFFFFu;

// The reference's loops for one node, by one lane: a node of more than 512 Frame features, and every node of a pair whose feature
// vectors put a feature into two nodes (nodes then interact through the slots and run in order).
__device__ void bow_rig_node(const RigBowPairDev& P, int k, int f, float nnratio)
{
    for (int i1 = P.off1[k]; i1 < P.off1[k + 1]; i1++) {
        const int idx1 = (int)P.feat1[i1];
        if (!P.v1[idx1]) continue;                              // !pMP || pMP->isBad()
        const uint8_t* da = P.d1 + (size_t)idx1 * 32;
        int best1 = 256, bestIdx = -1, best2 = 256, best1R = 256, bestIdxR = -1;       // (bestDist2R is computed and never read: `|| true`)
        for (int i2 = P.off2[f]; i2 < P.off2[f + 1]; i2++) {
            const int idx2 = (int)P.feat2[i2];
            if (P.match[idx2] >= 0) continue;
            const int dist = hamming256(da, P.d2 + (size_t)idx2 * 32);
            if (idx2 < P.n_left) {
                if (dist < best1) { best2 = best1; best1 = dist; bestIdx = idx2; }
                else if (dist < best2) best2 = dist;
            } else if (dist < best1R) { best1R = dist; bestIdxR = idx2; }
        }
        if (best1 > TH_LOW) continue;                           // :327 -- the right side is looked at under the LEFT best only
        if ((float)best1 < nnratio * (float)best2) P.match[bestIdx] = idx1;
        if (best1R <= TH_LOW) P.match[bestIdxR] = idx1;
    }
}

// the smallest key of a 16-lane group in every lane of it (the ladder of bow_group_top2 without the second key)
template <int CTRL>
__device__ __forceinline__ void bow_min_step(unsigned& k) { k = min(k, (unsigned)__builtin_amdgcn_update_dpp(-1, (int)k, CTRL, 0xF, 0xF, false)); }
__device__ __forceinline__ unsigned bow_group_min(unsigned k)
{
    bow_min_step<0xB1>(k); bow_min_step<0x4E>(k); bow_min_step<0x141>(k); bow_min_step<0x140>(k);
    return k;
}
// whether any lane of this lane's 16-lane group holds `pred` (one wave ballot; the group's lanes are converged)
__device__ __forceinline__ bool bow_group_any(bool pred) { return ((__ballot(pred) >> (threadIdx.x & 48)) & 0xFFFFull) != 0; }

// What a key-frame feature does with the group's reduced keys: the decision table of :327-386.  kl1 / kl2: the two smallest left
// keys of the group, kr1: the smallest right key (kBowNoKey: none); a key is (distance << 16) | position in the node.  Returns
// the positions to consume (-1: none).
__device__ __forceinline__ void bow_rig_decide(unsigned kl1, unsigned kl2, unsigned kr1, float nnratio, int& take_l, int& take_r)
{
    take_l = take_r = -1;
    const int best1 = (int)(kl1 >> 16), best2 = (kl2 == kBowNoKey) ? 256 : (int)(kl2 >> 16);
    if ((float)best1 < nnratio * (float)best2) take_l = (int)(kl1 & 0xFFFFu);
    if (kr1 != kBowNoKey && (int)(kr1 >> 16) <= TH_LOW) take_r = (int)(kr1 & 0xFFFFu);
}

// One node by a 16-lane group (a DPP row), as bow_node_group: the key-frame features in order, the Frame features of the node spread
// over the lanes, which keep the consumed state of their candidates (positions sub, sub + 16, ...) in a register bitmask.  Two
// reductions per key-frame feature: (best, second) over the left candidates, the minimum over the right ones (the reference's second-best right
// distance is never read); a candidate enters the reduction of its own side only.  Shortcuts that follow from :327: no live left
// candidate in the group (one ballot) -- nothing can be written, both reductions are skipped; left best above TH_LOW -- the right reduction is skipped; a node without right
// candidates never runs it.
__device__ void bow_rig_node_group(const RigBowPairDev& P, int k, int f, float nnratio, int sub)
{
    const int b2 = P.off2[f], n2 = P.off2[f + 1] - b2;
    unsigned right = 0;                                         // bit j: candidate sub + 16*j is the right camera's
    for (int c = sub, j = 0; c < n2; c += kBowGroup, j++) if ((int)P.feat2[b2 + c] >= P.n_left) right |= 1u << j;
    const bool any_right = bow_group_any(right != 0);
    unsigned taken = 0;                                         // bit j: candidate sub + 16*j is consumed
    for (int i1 = P.off1[k]; i1 < P.off1[k + 1]; i1++) {
        const int idx1 = (int)P.feat1[i1];
        if (!P.v1[idx1]) continue;                              // (uniform over the group)
        const unsigned long long* da = (const unsigned long long*)(P.d1 + (size_t)idx1 * 32);
        const unsigned long long a0 = da[0], a1 = da[1], a2 = da[2], a3 = da[3];
        unsigned kl1 = kBowNoKey, kl2 = kBowNoKey, kr1 = kBowNoKey;
        for (int c = sub, j = 0; c < n2; c += kBowGroup, j++) {
            if ((taken >> j) & 1u) continue;
            const unsigned long long* db = (const unsigned long long*)(P.d2 + (size_t)P.feat2[b2 + c] * 32);
            const unsigned key = ((unsigned)(__popcll(a0 ^ db[0]) + __popcll(a1 ^ db[1]) + __popcll(a2 ^ db[2]) + __popcll(a3 ^ db[3])) << 16) | (unsigned)c;
            if ((right >> j) & 1u) kr1 = min(kr1, key);
            else if (key < kl1) { kl2 = kl1; kl1 = key; } else if (key < kl2) kl2 = key;
        }
        if (!bow_group_any(kl1 != kBowNoKey)) continue;
        bow_group_top2(kl1, kl2);
        if ((int)(kl1 >> 16) > TH_LOW) continue;
        if (any_right) kr1 = bow_group_min(kr1);
        int tl, tr;
        bow_rig_decide(kl1, kl2, kr1, nnratio, tl, tr);
        if (tl >= 0 && (tl & (kBowGroup - 1)) == sub) { taken |= 1u << (tl / kBowGroup); P.match[P.feat2[b2 + tl]] = idx1; }
        if (tr >= 0 && (tr & (kBowGroup - 1)) == sub) { taken |= 1u << (tr / kBowGroup); P.match[P.feat2[b2 + tr]] = idx1; }
    }
}

// The common case, as bow_node_group_regs: a node of at most 16 J Frame features whose descriptors and indices the lanes hold in
// registers; the key-frame features are loaded 16 at a time and handed round by 16-lane shuffles, so the loop over them has no
// memory access but the stores of the matches.
template <int J>
__device__ void bow_rig_node_group_regs(const RigBowPairDev& P, int k, int f, float nnratio, int sub)
{
    const int b2 = P.off2[f], n2 = P.off2[f + 1] - b2;         // n2 <= 16 J
    int idx2[J];
    unsigned long long db[J][4];
    unsigned left = 0, right = 0;                               // bit j: this lane's candidate j exists and is the left / right camera's
#pragma unroll
    for (int j = 0; j < J; j++) { const int c = sub + kBowGroup * j; idx2[j] = 0; if (c < n2) { idx2[j] = (int)P.feat2[b2 + c]; if (idx2[j] < P.n_left) left |= 1u << j; else right |= 1u << j; } }
#pragma unroll
    for (int j = 0; j < J; j++) {
#pragma unroll
        for (int q = 0; q < 4; q++) db[j][q] = 0ull;
        if ((left | right) >> j & 1u) {
            const unsigned long long* dp = (const unsigned long long*)(P.d2 + (size_t)idx2[j] * 32);
#pragma unroll
            for (int q = 0; q < 4; q++) db[j][q] = dp[q];
        }
    }
    const bool any_right = bow_group_any(right != 0);
    bool live = bow_group_any(left != 0);                       // a left candidate is left: without one nothing more can be written (:327)
    const int b1 = P.off1[k], n1 = P.off1[k + 1] - b1;
    for (int i0 = 0; i0 < n1 && live; i0 += kBowGroup) {
        const int ii = i0 + sub;
        int idx1m = 0, valid = 0;
        unsigned long long A[4] = {0ull, 0ull, 0ull, 0ull};
        if (ii < n1) {
            idx1m = (int)P.feat1[b1 + ii];
            valid = P.v1[idx1m] ? 1 : 0;                        // !pMP || pMP->isBad()
            const unsigned long long* da = (const unsigned long long*)(P.d1 + (size_t)idx1m * 32);
#pragma unroll
            for (int q = 0; q < 4; q++) A[q] = da[q];
        }
        const unsigned vmask = (unsigned)((__ballot(valid != 0) >> (threadIdx.x & 48)) & 0xFFFFull);
        const int cnt = min(kBowGroup, n1 - i0);
        for (int i = 0; i < cnt; i++) {
            if (!((vmask >> i) & 1u)) continue;                 // uniform over the group
            if (!live) break;
            const unsigned long long a0 = shfl16_u64(A[0], i), a1 = shfl16_u64(A[1], i), a2 = shfl16_u64(A[2], i), a3 = shfl16_u64(A[3], i);
            const int idx1 = __shfl(idx1m, i, kBowGroup);
            unsigned kl1 = kBowNoKey, kl2 = kBowNoKey, kr1 = kBowNoKey;
#pragma unroll
            for (int j = 0; j < J; j++) {
                if (!(((left | right) >> j) & 1u)) continue;
                const unsigned key = ((unsigned)(__popcll(a0 ^ db[j][0]) + __popcll(a1 ^ db[j][1]) + __popcll(a2 ^ db[j][2]) + __popcll(a3 ^ db[j][3])) << 16) | (unsigned)(sub + kBowGroup * j);
                if ((right >> j) & 1u) kr1 = min(kr1, key);
                else if (key < kl1) { kl2 = kl1; kl1 = key; } else if (key < kl2) kl2 = key;
            }
            bow_group_top2(kl1, kl2);
            if ((int)(kl1 >> 16) > TH_LOW) continue;
            if (any_right) kr1 = bow_group_min(kr1);
            int tl, tr;
            bow_rig_decide(kl1, kl2, kr1, nnratio, tl, tr);
            // the lane that owns a winner consumes it (its bit leaves left / right) and records the match
            if (tl >= 0 && (tl & (kBowGroup - 1)) == sub) {
                const int jb = tl / kBowGroup;
                left &= ~(1u << jb);
                int bestIdx = idx2[0];
#pragma unroll
                for (int j = 1; j < J; j++) if (jb == j) bestIdx = idx2[j];
                P.match[bestIdx] = idx1;
            }
            if (tl >= 0) live = bow_group_any(left != 0);       // (tl is uniform over the group)
            if (tr >= 0 && (tr & (kBowGroup - 1)) == sub) {
                const int jb = tr / kBowGroup;
                right &= ~(1u << jb);
                int bestIdx = idx2[0];
#pragma unroll
                for (int j = 1; j < J; j++) if (jb == j) bestIdx = idx2[j];
                P.match[bestIdx] = idx1;
            }
        }
    }
}

// A workgroup per pair, a 16-lane group per common node.  The rotation histogram is a set function of the final slot array -- every
// slot is written at most once, a written slot is invisible afterwards -- so it is built from match after the nodes, in LDS.
__global__ __launch_bounds__(kBowThreads) void k_bow_rig(const RigBowPairDev* __restrict__ pairs, float nnratio, int check_ori)
{
    __shared__ int s_hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    __shared__ int s_count;
    const RigBowPairDev P = pairs[blockIdx.x];
    const int tid = threadIdx.x;
    for (int i = tid; i < P.n2; i += kBowThreads) P.match[i] = -1;
    if (tid < HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) s_count = 0;
    __threadfence_block();
    __syncthreads();
    if (P.serial) {
        if (tid == 0) {
            int k = 0, f = 0;                                   // merge-join of the two ascending node lists (:248-401)
            while (k < P.nn1 && f < P.nn2) {
                if (P.node1[k] == P.node2[f]) { bow_rig_node(P, k, f, nnratio); k++; f++; }
                else if (P.node1[k] < P.node2[f]) k++;
                else f++;
            }
        }
    } else {
        const int sub = tid & (kBowGroup - 1);
        for (int k = tid / kBowGroup; k < P.nn1; k += kBowThreads / kBowGroup) {
            const uint32_t key = P.node1[k];
            int lo = 0, hi = P.nn2;
            while (lo < hi) { const int mid = (lo + hi) >> 1; if (P.node2[mid] < key) lo = mid + 1; else hi = mid; }
            if (lo < P.nn2 && P.node2[lo] == key) {
                const int n2 = P.off2[lo + 1] - P.off2[lo];
                if (n2 > 32 * kBowGroup) { if (sub == 0) bow_rig_node(P, k, lo, nnratio); }     // beyond the per-lane bitmask: one lane walks it
                else if (n2 <= 2 * kBowGroup) bow_rig_node_group_regs<2>(P, k, lo, nnratio, sub);
                else if (n2 <= 4 * kBowGroup) bow_rig_node_group_regs<4>(P, k, lo, nnratio, sub);
                else if (n2 <= 6 * kBowGroup) bow_rig_node_group_regs<6>(P, k, lo, nnratio, sub);
                else bow_rig_node_group(P, k, lo, nnratio, sub);
            }
        }
    }
    __threadfence_block();
    __syncthreads();
    if (check_ori) {
        for (int i = tid; i < P.n2; i += kBowThreads) {
            const int m = P.match[i];
            if (m >= 0) atomicAdd(&s_hist[rot_bin(P.a1[m], P.a2[i])], 1);
        }
        __syncthreads();
        if (tid == 0) { int a, b, c; three_maxima(s_hist, HISTO_LENGTH, a, b, c); s_keep[0] = a; s_keep[1] = b; s_keep[2] = c; }
        __syncthreads();
    }
    int local = 0;
    for (int i = tid; i < P.n2; i += kBowThreads) {
        const int m = P.match[i];
        if (m < 0) continue;
        if (check_ori) {
            const int bin = rot_bin(P.a1[m], P.a2[i]);
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) { P.match[i] = -1; continue; }
        }
        local++;
    }
    if (local) atomicAdd(&s_count, local);
    __syncthreads();
    if (tid == 0) *P.n_matches = s_count;
}

// ---- SearchForTriangulation, both key frames rigs (src/ORBmatcher.cc:907-1146) -----------------------------------------------------
// The reference never writes vbMatched2, so the key-frame-1 features do not interact, and its candidate loop is an order-free set
// function: a candidate replaces the holder when dist <= bestDist and the gate passes, a failing candidate changes nothing, so the
// winner among {no map point, dist <= TH_LOW, gate passes} has the smallest dist and, among equal distances, is the LAST in node
// order -- the minimum of (dist << 16) | (0xFFFF - position).  One wave per entry of key frame 1's feature vector; its lanes take the
// key-frame-2 features of the node, and every lane whose candidate survives the Hamming test evaluates the gate
// (kb8s::triangulate_matches: two Newton unprojections, a 4x4 null vector in double, two projections) under the record of its
// (bRight1, bRight2).  A second launch, a workgroup per pair, builds the histogram, filters and counts.
constexpr int kTriRigWaves = 4;
struct RigTriPairDev {
    const uint8_t* d1; const uint8_t* mp1; const float* x1; const float* y1; const int32_t* oct1; const float* a1;
    const uint32_t* node1; const int32_t* off1; const uint32_t* feat1;
    const uint8_t* d2; const uint8_t* mp2; const float* x2; const float* y2; const int32_t* oct2; const float* a2;
    const uint32_t* node2; const int32_t* off2; const uint32_t* feat2;
    const float* sigma1; const float* sigma2;
    const kb8s::Rig* rigs;              // [4] ll, lr, rl, rr
    int32_t n1, nl1, nl2, nn1, nn2, first_block;      // first_block: where the pair's blocks start in the grid
    int32_t* match12; int32_t* n_matches;
};

__global__ __launch_bounds__(64 * kTriRigWaves) void k_tri_rig(const RigTriPairDev* __restrict__ pairs, int n_pairs, int coarse)
{
    __shared__ kb8s::Rig s_rig[4];
    int lo = 0, hi = n_pairs;                                   // the pair of this block: the last one with first_block <= blockIdx.x
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (pairs[mid].first_block <= (int)blockIdx.x) lo = mid; else hi = mid; }
    const RigTriPairDev& A = pairs[lo];
    if (!coarse) {
        const float* src = (const float*)A.rigs;
        float* dst = (float*)s_rig;
        for (int i = threadIdx.x; i < (int)(4 * sizeof(kb8s::Rig) / sizeof(float)); i += 64 * kTriRigWaves) dst[i] = src[i];
    }
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int total1 = A.nn1 > 0 ? A.off1[A.nn1] : 0;
    const int e1 = ((int)blockIdx.x - A.first_block) * kTriRigWaves + (int)(threadIdx.x >> 6);     // wave-uniform
    if (e1 >= total1) return;
    const int idx1 = (int)A.feat1[e1];
    if (A.mp1[idx1]) return;                                    // already a MapPoint (:974); match12 was -1 on upload
    int l1 = 0, h1 = A.nn1;                                     // node of entry e1: last k with off1[k] <= e1
    while (h1 - l1 > 1) { const int mid = (l1 + h1) >> 1; if (A.off1[mid] <= e1) l1 = mid; else h1 = mid; }
    const uint32_t node = A.node1[l1];
    int l2 = 0, h2 = A.nn2;
    while (l2 < h2) { const int mid = (l2 + h2) >> 1; if (A.node2[mid] < node) l2 = mid + 1; else h2 = mid; }
    if (l2 >= A.nn2 || A.node2[l2] != node) return;
    const unsigned long long* da = (const unsigned long long*)(A.d1 + (size_t)idx1 * 32);
    const unsigned long long a0 = da[0], a1 = da[1], a2 = da[2], a3 = da[3];
    const int right1 = idx1 >= A.nl1 ? 1 : 0;
    float u1 = 0.f, v1 = 0.f, sg1 = 0.f;
    if (!coarse) { u1 = A.x1[idx1]; v1 = A.y1[idx1]; sg1 = A.sigma1[A.oct1[idx1]]; }
    const int b2 = A.off2[l2], n2 = A.off2[l2 + 1] - b2;       // n2 <= 65535 (orbm_rig_bow_check)
    unsigned best = kBowNoKey;
    for (int c = lane; c < n2; c += 64) {
        const int idx2 = (int)A.feat2[b2 + c];
        if (A.mp2[idx2]) continue;
        const unsigned long long* db = (const unsigned long long*)(A.d2 + (size_t)idx2 * 32);
        const int dist = __popcll(a0 ^ db[0]) + __popcll(a1 ^ db[1]) + __popcll(a2 ^ db[2]) + __popcll(a3 ^ db[3]);
        if (dist > TH_LOW) continue;
        const unsigned key = ((unsigned)dist << 16) | (unsigned)(0xFFFF - c);
        if (key > best) continue;                               // (a lane's own earlier candidate already beats it)
        if (!coarse) {
            float p3d[3];
            const kb8s::Rig& g = s_rig[2 * right1 + (idx2 >= A.nl2 ? 1 : 0)];
            if (!(kb8s::triangulate_matches(g, u1, v1, A.x2[idx2], A.y2[idx2], sg1, A.sigma2[A.oct2[idx2]], p3d) > 0.0001f)) continue;
        }
        best = key;
    }
    best = wave_min_u32(best);                                  // (all 64 lanes are here: every exit above is wave-uniform)
    if (lane == 0 && best != kBowNoKey) A.match12[idx1] = (int)A.feat2[b2 + (0xFFFF - (int)(best & 0xFFFFu))];
}

__global__ __launch_bounds__(256) void k_tri_rig_finish(const RigTriPairDev* __restrict__ pairs, int check_ori)
{
    __shared__ int s_hist[HISTO_LENGTH];
    __shared__ int s_keep[3];
    __shared__ int s_count;
    const RigTriPairDev& A = pairs[blockIdx.x];
    const int tid = threadIdx.x;
    if (tid < HISTO_LENGTH) s_hist[tid] = 0;
    if (tid == 0) s_count = 0;
    __syncthreads();
    if (check_ori) {
        for (int i = tid; i < A.n1; i += 256) {
            const int m = A.match12[i];
            if (m >= 0) atomicAdd(&s_hist[rot_bin(A.a1[i], A.a2[m])], 1);
        }
        __syncthreads();
        if (tid == 0) { int a, b, c; three_maxima(s_hist, HISTO_LENGTH, a, b, c); s_keep[0] = a; s_keep[1] = b; s_keep[2] = c; }
        __syncthreads();
    }
    int local = 0;
    for (int i = tid; i < A.n1; i += 256) {
        const int m = A.match12[i];
        if (m < 0) continue;
        if (check_ori) {
            const int bin = rot_bin(A.a1[i], A.a2[m]);
            if (bin != s_keep[0] && bin != s_keep[1] && bin != s_keep[2]) { A.match12[i] = -1; continue; }
        }
        local++;
    }
    if (local) atomicAdd(&s_count, local);
    __syncthreads();
    if (tid == 0) *A.n_matches = s_count;
}

}  // namespace orbm

// ---- host side ----

// check_fv and what the kernels of this file need beyond it: offsets that start at 0 and a node that fits the 16-bit position field
static int rig_bow_check_fv(const OrbmFeatVec* fv, int n, const char* name)
{
    if (int e = check_fv(fv, n, name)) return e;
    if (fv->n_nodes == 0) return ORBX_OK;
    if (fv->offset[0] != 0) return fail(ORBX_ERR_ARG, "%s: offsets do not start at 0", name);
    for (int k = 0; k < fv->n_nodes; k++)
        if (fv->offset[k + 1] - fv->offset[k] > 65535) return fail(ORBX_ERR_ARG, "%s: node %d holds more than 65535 features", name, k);
    return ORBX_OK;
}

static int rig_bow_check_pair(const OrbmBowRigPair* p, int check_ori)
{
    if (p->n_kf < 0 || p->n_f < 0) return fail(ORBX_ERR_ARG, "negative feature count");
    if (p->n_left_f < 0 || p->n_left_f > p->n_f) return fail(ORBX_ERR_ARG, "n_left_f = %d outside [0, %d]", p->n_left_f, p->n_f);
    if ((p->n_kf > 0 && (!p->desc_kf || !p->valid_kf)) || (p->n_f > 0 && !p->desc_f)) return fail(ORBX_ERR_ARG, "NULL descriptor/valid array");
    if (p->n_f > 0 && !p->match_f2kf) return fail(ORBX_ERR_ARG, "NULL match_f2kf");
    if (check_ori && ((p->n_kf > 0 && !p->angle_kf) || (p->n_f > 0 && !p->angle_f))) return fail(ORBX_ERR_ARG, "NULL angle array");
    if (int e = rig_bow_check_fv(&p->fv_kf, p->n_kf, "fv_kf")) return e;
    return rig_bow_check_fv(&p->fv_f, p->n_f, "fv_f");
}

static int rig_tri_check_pair(const OrbmRigTriPair* p, int check_ori)
{
    if (!p->kf1 || !p->kf2 || !p->geom || !p->level_sigma2_1 || !p->level_sigma2_2) return fail(ORBX_ERR_ARG, "NULL key frame, geometry or level sigmas");
    if (p->n_levels < 1 || p->n_levels > 32) return fail(ORBX_ERR_ARG, "n_levels = %d outside [1, 32]", p->n_levels);
    const OrbmTriSide* side[2] = {p->kf1, p->kf2};
    const int n_left[2] = {p->n_left_1, p->n_left_2};
    for (int q = 0; q < 2; q++) {
        const OrbmTriSide* k = side[q];
        if (k->n < 0) return fail(ORBX_ERR_ARG, "negative feature count");
        if (n_left[q] < 0 || n_left[q] > k->n) return fail(ORBX_ERR_ARG, "n_left_%d = %d outside [0, %d]", q + 1, n_left[q], k->n);
        if (k->n > 0 && (!k->desc || !k->has_mp || !k->x || !k->y || !k->octave)) return fail(ORBX_ERR_ARG, "NULL key-frame arrays");
        if (check_ori && k->n > 0 && !k->angle) return fail(ORBX_ERR_ARG, "NULL angles");
        for (int i = 0; i < k->n; i++)
            if (k->octave[i] < 0 || k->octave[i] >= p->n_levels) return fail(ORBX_ERR_ARG, "key frame %d: octave %d of feature %d out of range", q + 1, k->octave[i], i);
        if (int e = rig_bow_check_fv(&k->fv, k->n, q ? "fv2" : "fv1")) return e;
        // key frame 1 only: a wave per entry owns match12[feature].  Key frame 2's vector is only read, a repeated feature there is a candidate twice
        if (q == 0 && !features_unique(&k->fv, k->n)) return fail(ORBX_ERR_ARG, "a feature of key frame 1 appears in two vocabulary nodes");
    }
    if (p->kf1->n > 0 && !p->match12) return fail(ORBX_ERR_ARG, "NULL match12");
    return ORBX_OK;
}

static int rig_bow_check(const OrbmBowRigPair* bow, const OrbmRigTriPair* tri, int check_ori)
{
    if ((bow != nullptr) == (tri != nullptr)) return fail(ORBX_ERR_ARG, "exactly one of the SearchByBoW pair and the SearchForTriangulation pair is given");
    return bow ? rig_bow_check_pair(bow, check_ori) : rig_tri_check_pair(tri, check_ori);
}

// all pairs in one blob, ONE k_bow_rig launch with a workgroup per pair, one copy back
static int run_bow_rig(orbm_matcher* m, OrbmBowRigPair* pairs, int n_pairs, float nnratio, int check_ori)
{
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    if (!pairs || n_pairs < 1) return fail(ORBX_ERR_ARG, "no pairs");
    for (int p = 0; p < n_pairs; p++)
        if (int e = rig_bow_check(&pairs[p], nullptr, check_ori)) return e;
    ORBX_HIP(hipSetDevice(m->device));
    Blob blob(m);
    std::vector<orbm::RigBowPairDev> descs(n_pairs);
    const size_t desc_off = blob.slot<orbm::RigBowPairDev>(n_pairs);
    static const int32_t zero_off[1] = {0};
    for (int p = 0; p < n_pairs; p++) {
        const OrbmBowRigPair& q = pairs[p];
        orbm::RigBowPairDev& D = descs[p];
        const int nn1 = q.fv_kf.n_nodes, nn2 = q.fv_f.n_nodes;
        D.n1 = q.n_kf; D.n2 = q.n_f; D.n_left = q.n_left_f; D.nn1 = nn1; D.nn2 = nn2;
        blob.in(D.d1, q.desc_kf, (size_t)q.n_kf * 32); blob.in(D.v1, q.valid_kf, q.n_kf); blob.in_opt(D.a1, q.angle_kf, q.n_kf);
        blob.in(D.node1, q.fv_kf.node_id, nn1); blob.in(D.off1, nn1 ? q.fv_kf.offset : zero_off, nn1 + 1); blob.in(D.feat1, q.fv_kf.feat, nn1 ? q.fv_kf.offset[nn1] : 0);
        blob.in(D.d2, q.desc_f, (size_t)q.n_f * 32); blob.in_opt(D.a2, q.angle_f, q.n_f);
        blob.in(D.node2, q.fv_f.node_id, nn2); blob.in(D.off2, nn2 ? q.fv_f.offset : zero_off, nn2 + 1); blob.in(D.feat2, q.fv_f.feat, nn2 ? q.fv_f.offset[nn2] : 0);
        D.serial = !features_unique(&q.fv_f, q.n_f);
    }
    const size_t out_begin = blob.begin_out();
    for (int p = 0; p < n_pairs; p++) { blob.out(descs[p].match, std::max(pairs[p].n_f, 1)); blob.out(descs[p].n_matches, 1); }
    if (int e = m->ensure(blob.size())) return e;
    blob.bind(m->d_blob);
    blob.store(desc_off, descs.data(), n_pairs);
    if (int e = m->rig_bow_timer.create()) return e;
    ORBX_HIP(hipMemcpyAsync(m->d_blob, m->h_blob.data(), out_begin, hipMemcpyHostToDevice, m->stream));
    if (int e = m->rig_bow_timer.start(m->stream)) return e;
    hipLaunchKernelGGL(orbm::k_bow_rig, dim3(n_pairs), dim3(orbm::kBowThreads), 0, m->stream, blob.device<orbm::RigBowPairDev>(desc_off), nnratio, check_ori);
    ORBX_HIP(hipGetLastError());
    if (int e = m->rig_bow_timer.stop(m->stream)) return e;
    ORBX_HIP(hipMemcpyAsync(m->h_blob.data() + out_begin, m->d_blob + out_begin, blob.size() - out_begin, hipMemcpyDeviceToHost, m->stream));
    ORBX_HIP(hipStreamSynchronize(m->stream));
    if (int e = m->rig_bow_timer.read()) return e;
    for (int p = 0; p < n_pairs; p++) {
        if (pairs[p].n_f > 0) std::memcpy(pairs[p].match_f2kf, blob.host(descs[p].match), sizeof(int32_t) * pairs[p].n_f);
        std::memcpy(&pairs[p].n_matches, blob.host(descs[p].n_matches), sizeof(int32_t));
    }
    return ORBX_OK;
}

// all pairs in one blob; ONE k_tri_rig launch over the feature-vector entries of every pair, ONE k_tri_rig_finish launch
static int run_tri_rig(orbm_matcher* m, OrbmRigTriPair* pairs, int n_pairs, int only_stereo, int coarse, int check_ori)
{
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    if (!pairs || n_pairs < 1) return fail(ORBX_ERR_ARG, "no pairs");
    for (int p = 0; p < n_pairs; p++)
        if (int e = rig_bow_check(nullptr, &pairs[p], check_ori)) return e;
    if (only_stereo) {              // bStereo1 is false for every feature of a rig key frame (:979-983)
        for (int p = 0; p < n_pairs; p++) { std::fill(pairs[p].match12, pairs[p].match12 + pairs[p].kf1->n, -1); pairs[p].n_matches = 0; }
        m->rig_bow_timer.ms = 0.f;
        return ORBX_OK;
    }
    ORBX_HIP(hipSetDevice(m->device));
    Blob blob(m);
    std::vector<orbm::RigTriPairDev> descs(n_pairs);
    const size_t desc_off = blob.slot<orbm::RigTriPairDev>(n_pairs);
    static const int32_t zero_off[1] = {0};
    long long n_blocks = 0;
    for (int p = 0; p < n_pairs; p++) {
        const OrbmRigTriPair& q = pairs[p];
        orbm::RigTriPairDev& A = descs[p];
        auto pack_side = [&](const OrbmTriSide* k, const uint8_t*& d, const uint8_t*& mp, const float*& x, const float*& y, const int32_t*& oct, const float*& a,
                             const uint32_t*& node, const int32_t*& off, const uint32_t*& feat) {
            const int n = k->n, nn = k->fv.n_nodes;
            blob.in(d, k->desc, (size_t)n * 32); blob.in(mp, k->has_mp, n); blob.in(x, k->x, n); blob.in(y, k->y, n); blob.in(oct, k->octave, n); blob.in_opt(a, k->angle, n);
            blob.in(node, k->fv.node_id, nn); blob.in(off, nn ? k->fv.offset : zero_off, nn + 1); blob.in(feat, k->fv.feat, nn > 0 ? k->fv.offset[nn] : 0);
        };
        pack_side(q.kf1, A.d1, A.mp1, A.x1, A.y1, A.oct1, A.a1, A.node1, A.off1, A.feat1);
        pack_side(q.kf2, A.d2, A.mp2, A.x2, A.y2, A.oct2, A.a2, A.node2, A.off2, A.feat2);
        blob.in(A.sigma1, q.level_sigma2_1, q.n_levels); blob.in(A.sigma2, q.level_sigma2_2, q.n_levels);
        kb8s::Rig rigs[4];          // ll, lr, rl, rr: camera 1 is key frame 1's (bRight1), camera 2 key frame 2's (bRight2)
        for (int c = 0; c < 4; c++) {
            const float* cam[2] = {q.geom->cam[c >> 1], q.geom->cam[2 + (c & 1)]};
            kb8s::Cam* dst[2] = {&rigs[c].l, &rigs[c].r};
            for (int s = 0; s < 2; s++) {
                dst[s]->fx = cam[s][0]; dst[s]->fy = cam[s][1]; dst[s]->cx = cam[s][2]; dst[s]->cy = cam[s][3];
                for (int k = 0; k < 4; k++) dst[s]->k[k] = cam[s][4 + k];
                dst[s]->precision = cam[s][8];
            }
            for (int k = 0; k < 9; k++) rigs[c].R12[k] = q.geom->R12[c][k];
            for (int k = 0; k < 3; k++) rigs[c].t12[k] = q.geom->t12[c][k];
        }
        blob.in(A.rigs, rigs, 4);
        A.n1 = q.kf1->n; A.nl1 = q.n_left_1; A.nl2 = q.n_left_2; A.nn1 = q.kf1->fv.n_nodes; A.nn2 = q.kf2->fv.n_nodes;
        const int total1 = A.nn1 > 0 ? q.kf1->fv.offset[A.nn1] : 0;
        A.first_block = (int32_t)n_blocks;
        n_blocks += (total1 + orbm::kTriRigWaves - 1) / orbm::kTriRigWaves;
        if (n_blocks > 0x7FFFFFFFll) return fail(ORBX_ERR_ARG, "too many feature-vector entries in one batch");
    }
    const size_t out_begin = blob.begin_out();
    std::vector<size_t> match_off(n_pairs);
    for (int p = 0; p < n_pairs; p++) { match_off[p] = blob.out(descs[p].match12, std::max(pairs[p].kf1->n, 1)); blob.out(descs[p].n_matches, 1); }
    for (int p = 0; p < n_pairs; p++) std::memset(m->h_blob.data() + match_off[p], 0xFF, sizeof(int32_t) * std::max(pairs[p].kf1->n, 1));      // match12 = -1
    if (int e = m->ensure(blob.size())) return e;
    blob.bind(m->d_blob);
    blob.store(desc_off, descs.data(), n_pairs);
    if (int e = m->rig_bow_timer.create()) return e;
    ORBX_HIP(hipMemcpyAsync(m->d_blob, m->h_blob.data(), blob.size(), hipMemcpyHostToDevice, m->stream));
    if (int e = m->rig_bow_timer.start(m->stream)) return e;
    const orbm::RigTriPairDev* d_pairs = blob.device<orbm::RigTriPairDev>(desc_off);
    if (n_blocks > 0) hipLaunchKernelGGL(orbm::k_tri_rig, dim3((unsigned)n_blocks), dim3(64 * orbm::kTriRigWaves), 0, m->stream, d_pairs, n_pairs, coarse ? 1 : 0);
    hipLaunchKernelGGL(orbm::k_tri_rig_finish, dim3(n_pairs), dim3(256), 0, m->stream, d_pairs, check_ori);
    ORBX_HIP(hipGetLastError());
    if (int e = m->rig_bow_timer.stop(m->stream)) return e;
    ORBX_HIP(hipMemcpyAsync(m->h_blob.data() + out_begin, m->d_blob + out_begin, blob.size() - out_begin, hipMemcpyDeviceToHost, m->stream));
    ORBX_HIP(hipStreamSynchronize(m->stream));
    if (int e = m->rig_bow_timer.read()) return e;
    for (int p = 0; p < n_pairs; p++) {
        if (pairs[p].kf1->n > 0) std::memcpy(pairs[p].match12, blob.host(descs[p].match12), sizeof(int32_t) * pairs[p].kf1->n);
        std::memcpy(&pairs[p].n_matches, blob.host(descs[p].n_matches), sizeof(int32_t));
    }
    return ORBX_OK;
}

extern "C" {

int orbm_rig_bow_check(const OrbmBowRigPair* bow, const OrbmRigTriPair* tri, int check_orientation) { return rig_bow_check(bow, tri, check_orientation); }

int orbm_search_by_bow_rig(orbm_matcher* m, const uint8_t* desc_kf, int n_kf, const uint8_t* valid_kf, const float* angle_kf, const OrbmFeatVec* fv_kf,
                           const uint8_t* desc_f, int n_f, int n_left_f, const float* angle_f, const OrbmFeatVec* fv_f,
                           float nnratio, int check_orientation, int32_t* match_f2kf)
{
    if (!m) return fail(ORBX_ERR_ARG, "NULL matcher");
    if (!fv_kf || !fv_f) return fail(ORBX_ERR_ARG, "NULL feature vector");
    OrbmBowRigPair p{desc_kf, n_kf, valid_kf, angle_kf, *fv_kf, desc_f, n_f, n_left_f, angle_f, *fv_f, match_f2kf, 0};
    const int r = run_bow_rig(m, &p, 1, nnratio, check_orientation ? 1 : 0);
    return r ? r : p.n_matches;
}

int orbm_search_by_bow_rig_batch(orbm_matcher* m, OrbmBowRigPair* pairs, int n_pairs, float nnratio, int check_orientation)
{
    return run_bow_rig(m, pairs, n_pairs, nnratio, check_orientation ? 1 : 0);
}

int orbm_search_for_triangulation_rig(orbm_matcher* m, const OrbmTriSide* kf1, int n_left_1, const OrbmTriSide* kf2, int n_left_2,
                                      const OrbmRigTriGeometry* geom, const float* level_sigma2_1, const float* level_sigma2_2, int n_levels,
                                      int only_stereo, int coarse, int check_orientation, int32_t* match12)
{
    OrbmRigTriPair p{kf1, n_left_1, kf2, n_left_2, geom, level_sigma2_1, level_sigma2_2, n_levels, match12, 0};
    const int r = run_tri_rig(m, &p, 1, only_stereo, coarse, check_orientation ? 1 : 0);
    return r ? r : p.n_matches;
}

int orbm_search_for_triangulation_rig_batch(orbm_matcher* m, OrbmRigTriPair* pairs, int n_pairs, int only_stereo, int coarse, int check_orientation)
{
    return run_tri_rig(m, pairs, n_pairs, only_stereo, coarse, check_orientation ? 1 : 0);
}

float orbm_rig_bow_last_kernel_ms(const orbm_matcher* m) { return m ? m->rig_bow_timer.ms : 0.f; }

}  // extern "C"
