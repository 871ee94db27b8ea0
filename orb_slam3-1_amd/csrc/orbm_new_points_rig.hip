// orbm_new_points_rig.hip -- LocalMapping::CreateNewMapPoints for two-camera fisheye rigs (reference src/LocalMapping.cc:392-716
// with mpCamera2 set; include/orbslam3_hip_rig_newpoints.h restates the branches): the candidate gate of k_tri_rig fused with
// the neighbour chain and per-match geometry of k_new_map_points.
//
// A key-frame-1 feature interacts with nothing but its own chain, GIVEN which neighbours the baseline test skips: it walks the
// neighbours in order until the first one where it matches and passes every gate.  The skip decisions are the one coupling
// between features (the reference's Ow1 is overwritten per match and read by the next neighbour's baseline test), so they are an
// input of the kernel -- a 64-bit mask -- and the host driver cuts the call where a decision depends on the matches before it.
// A wave serves an entry of key frame 1's feature vector: the lanes spread over the neighbour's features of the same vocabulary
// node, every lane whose candidate survives the Hamming test evaluates the KannalaBrandt8 gate under the record of its
// (bRight1, bRight2), the wave minimum of (dist << 16) | (0xFFFF - position) is the winner of the reference's sequential loop,
// and lane 0 runs the geometry (orbm_new_points_rig_geometry.h).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "../../include/orbslam3_hip.h"
#include "hip_check.h"
#include "orbm_host.h"
#include "orbm_new_points_rig_geometry.h"

namespace orbm {

// Lanes per entry: 64, a whole wave, as k_tri_rig.  The alternative -- 16 lanes, four entries per wave, as k_new_map_points -- puts
// the gates and geometry chains of four entries into one divergent branch, but ties four neighbour chains together: a wave then
// runs until its longest chain ends, and entries that sit at different neighbours serialise.  Measured on 1000 + 1000 key points
// (profiles/rig_newpoints_group_width.txt): 0.34 - 0.39 ms against 0.52 ms at 10 neighbours, 0.78 - 0.90 ms against 0.92 ms at 30.  The device
// has room for the 2000 waves of a key frame; the chain length, not the lane use, bounds the kernel.  Any power of two up to 64
// compiles: every exit below is uniform over the group.
constexpr int kRnpGroup = 64;
constexpr int kRnpThreads = 256;
constexpr unsigned kRnpNoKey = 0xFFFFFFFFu;

struct RnpKeyFrameDev {
    const uint8_t* desc; const uint8_t* has_mp;
    const float* x; const float* y; const int32_t* octave;
    const int32_t* off; const uint32_t* feat;       // mFeatVec, flattened
    const float* sigma2; const float* scale;
    const int32_t* node_of;                         // [nodes of key frame 1] -> the same vocabulary node in this key frame's mFeatVec or -1 (neighbours only)
    nmp_rig::Side side[2];                          // left, right
    kb8s::Rig rigs[4];                              // ll, lr, rl, rr of the pair (key frame 1, this neighbour)
    int32_t n_left, coarse;
};

struct RnpArgs {
    const RnpKeyFrameDev* kf;                       // [1 + n_nb], key frame 1 first
    const int32_t* entry_node;                      // [total1]: node (index into key frame 1's mFeatVec) of each flattened entry
    int32_t total1, n1, j0, j1;                     // this launch walks the neighbours [j0, j1)
    unsigned long long skip;                        // bit j: the baseline test skips neighbour j
    nmp::Rule rule;
    float last_scale;                               // kf1->mvScaleFactors[nLevels - 1]
    int32_t* neighbour; int32_t* idx2; float* x3d;  // [n1], neighbour pre-set to -1 and kept between the launches of a call
    float* normal; float* max_dist; float* min_dist;
    int32_t* n_matched; int32_t* n_created; int32_t* max_matched_idx1;      // [n_nb], pre-set to 0, 0, -1
    int32_t* match12;                               // [n_nb][n1] pre-set to -1, or NULL
};

__device__ __forceinline__ nmp_rig::Obs rnp_obs(const RnpKeyFrameDev& K, int i)
{
    nmp_rig::Obs o;
    o.x = K.x[i]; o.y = K.y[i];
    const int oct = K.octave[i];
    o.sigma2 = K.sigma2[oct]; o.scale = K.scale[oct];
    return o;
}

__global__ __launch_bounds__(kRnpThreads) void k_new_map_points_rig(RnpArgs A)
{
    const int e1 = (blockIdx.x * kRnpThreads + threadIdx.x) / kRnpGroup;        // the lanes of a group share e1 and every branch below
    const int sub = threadIdx.x & (kRnpGroup - 1);
    if (e1 >= A.total1) return;
    const RnpKeyFrameDev& K1 = A.kf[0];
    const int idx1 = (int)K1.feat[e1];
    if (K1.has_mp[idx1] || A.neighbour[idx1] >= 0) return;      // already a MapPoint (src/ORBmatcher.cc:974), or made one in an earlier launch
    const int node1 = A.entry_node[e1];
    const unsigned long long* da = (const unsigned long long*)(K1.desc + (size_t)idx1 * 32);
    const unsigned long long a0 = da[0], a1 = da[1], a2 = da[2], a3 = da[3];
    const int right1 = idx1 >= K1.n_left ? 1 : 0;
    const float u1 = K1.x[idx1], v1 = K1.y[idx1];
    const float sg1 = K1.sigma2[K1.octave[idx1]];

    for (int j = A.j0; j < A.j1; j++) {                         // (bounded: j1 <= ORBM_MAX_NEIGHBOURS)
        if ((A.skip >> j) & 1ull) continue;
        const RnpKeyFrameDev& K2 = A.kf[1 + j];
        const int l2 = K2.node_of[node1];
        if (l2 < 0) continue;
        const int b2 = K2.off[l2], n2 = K2.off[l2 + 1] - b2;    // n2 <= 65535 (orbm_create_new_map_points_rig_check)
        unsigned best = kRnpNoKey;
        for (int c = sub; c < n2; c += kRnpGroup) {
            const int idx2 = (int)K2.feat[b2 + c];
            if (K2.has_mp[idx2]) continue;
            const unsigned long long* db = (const unsigned long long*)(K2.desc + (size_t)idx2 * 32);
            const int dist = __popcll(a0 ^ db[0]) + __popcll(a1 ^ db[1]) + __popcll(a2 ^ db[2]) + __popcll(a3 ^ db[3]);
            if (dist > TH_LOW) continue;
            const unsigned key = ((unsigned)dist << 16) | (unsigned)(0xFFFF - c);
            if (key > best) continue;                           // (a lane's own earlier candidate already beats it)
            if (!K2.coarse) {
                float p3d[3];
                const kb8s::Rig& g = K2.rigs[2 * right1 + (idx2 >= K2.n_left ? 1 : 0)];
                if (!(kb8s::triangulate_matches(g, u1, v1, K2.x[idx2], K2.y[idx2], sg1, K2.sigma2[K2.octave[idx2]], p3d) > 0.0001f)) continue;
            }
            best = key;
        }
        for (int o = kRnpGroup / 2; o > 0; o >>= 1) best = min(best, (unsigned)__shfl_xor((int)best, o, kRnpGroup));
        if (best == kRnpNoKey) continue;
        const int idx2 = (int)K2.feat[b2 + (0xFFFF - (int)(best & 0xFFFFu))];
        int created = 0;
        if (sub == 0) {
            atomicAdd(&A.n_matched[j], 1);
            atomicMax(&A.max_matched_idx1[j], idx1);
            if (A.match12) A.match12[(size_t)j * A.n1 + idx1] = idx2;
            const int right2 = idx2 >= K2.n_left ? 1 : 0;
            const nmp_rig::Side& S1 = K1.side[right1];
            const nmp_rig::Side& S2 = K2.side[right2];
            float x3D[3];
            created = nmp_rig::new_point(S1, rnp_obs(K1, idx1), S2, rnp_obs(K2, idx2), A.rule, x3D) ? 1 : 0;
            if (created) {
                A.neighbour[idx1] = j; A.idx2[idx1] = idx2;
                A.x3d[3 * idx1] = x3D[0]; A.x3d[3 * idx1 + 1] = x3D[1]; A.x3d[3 * idx1 + 2] = x3D[2];
                nmp_rig::normal_and_depth(x3D, S1.pose.Ow, S2.pose.Ow, K1.side[0].pose.Ow, K1.scale[K1.octave[idx1]], A.last_scale,
                                          A.normal + 3 * idx1, A.max_dist + idx1, A.min_dist + idx1);
                atomicAdd(&A.n_created[j], 1);
            }
        }
        if (__shfl(created, 0, kRnpGroup)) break;               // the feature holds a map point from here on
    }
}

}  // namespace orbm

namespace {

int rnp_check_key_frame(const OrbmRigMapKeyFrame* k, const char* name, bool unique)
{
    const OrbmTriSide& s = k->side;
    if (s.n < 0) return fail(ORBX_ERR_ARG, "%s: negative feature count", name);
    if (k->n_left < 0 || k->n_left > s.n) return fail(ORBX_ERR_ARG, "%s: n_left = %d outside [0, %d]", name, k->n_left, s.n);
    if (s.n > 0 && (!s.desc || !s.has_mp || !s.x || !s.y || !s.octave)) return fail(ORBX_ERR_ARG, "%s: NULL key-frame arrays", name);
    if (k->n_levels < 1 || k->n_levels > 32) return fail(ORBX_ERR_ARG, "%s: n_levels = %d outside [1, 32]", name, k->n_levels);
    if (!k->level_sigma2 || !k->scale_factors) return fail(ORBX_ERR_ARG, "%s: NULL scale tables", name);
    if (std::isnan(k->mb) || k->mb < 0) return fail(ORBX_ERR_ARG, "%s: mb is NaN or negative", name);
    if (int e = check_fv(&s.fv, s.n, name)) return e;
    if (s.fv.n_nodes > 0) {
        if (s.fv.offset[0] != 0) return fail(ORBX_ERR_ARG, "%s: feature-vector offsets must start at 0", name);
        for (int q = 0; q < s.fv.n_nodes; q++)
            if (s.fv.offset[q + 1] - s.fv.offset[q] > 65535) return fail(ORBX_ERR_ARG, "%s: node %d holds more than 65535 features", name, q);
    }
    // key frame 1 only: a lane group per entry owns the outputs of its feature.  A neighbour's vector is only read
    if (unique && !features_unique(&s.fv, s.n)) return fail(ORBX_ERR_ARG, "%s: a feature appears in two vocabulary nodes", name);
    for (int i = 0; i < s.n; i++)
        if (s.octave[i] < 0 || s.octave[i] >= k->n_levels) return fail(ORBX_ERR_ARG, "%s: octave %d of feature %d out of range", name, s.octave[i], i);
    return ORBX_OK;
}

int rnp_check(const OrbmRigMapKeyFrame* kf1, const OrbmRigMapKeyFrame* neighbours, int n_neighbours, const OrbmRigMapPair* pairs,
              const OrbmMapParams* params, const OrbmNewPoints* out)
{
    if (!kf1 || !params || !out) return fail(ORBX_ERR_ARG, "NULL argument");
    if (n_neighbours < 0 || n_neighbours > ORBM_MAX_NEIGHBOURS) return fail(ORBX_ERR_ARG, "n_neighbours %d outside [0, %d]", n_neighbours, ORBM_MAX_NEIGHBOURS);
    if (n_neighbours > 0 && (!neighbours || !pairs || !out->n_matched || !out->n_created)) return fail(ORBX_ERR_ARG, "NULL neighbour arrays");
    if (int e = rnp_check_key_frame(kf1, "kf1", true)) return e;
    for (int j = 0; j < n_neighbours; j++) {
        if (int e = rnp_check_key_frame(&neighbours[j], "neighbour", false)) return e;
        if (!pairs[j].geom) return fail(ORBX_ERR_ARG, "pair %d: NULL geometry", j);
    }
    const int n1 = kf1->side.n;
    if (n1 > 0 && (!out->neighbour || !out->idx2 || !out->x3d || !out->point_stereo)) return fail(ORBX_ERR_ARG, "NULL output arrays");
    const bool want_normal = out->normal || out->max_dist || out->min_dist;
    if (want_normal && n1 > 0 && (!out->normal || !out->max_dist || !out->min_dist)) return fail(ORBX_ERR_ARG, "normal, max_dist and min_dist go together");
    return ORBX_OK;
}

void rnp_cam(kb8s::Cam& c, const float* p)
{
    c.fx = p[0]; c.fy = p[1]; c.cx = p[2]; c.cy = p[3];
    for (int k = 0; k < 4; k++) c.k[k] = p[4 + k];
    c.precision = p[8];
}

}  // namespace

extern "C" {

int orbm_create_new_map_points_rig_check(const OrbmRigMapKeyFrame* kf1, const OrbmRigMapKeyFrame* neighbours, int n_neighbours,
                                         const OrbmRigMapPair* pairs, const OrbmMapParams* params, const OrbmNewPoints* out)
{
    return rnp_check(kf1, neighbours, n_neighbours, pairs, params, out);
}

int orbm_create_new_map_points_rig(orbm_matcher* m, const OrbmRigMapKeyFrame* kf1, const OrbmRigMapKeyFrame* neighbours, int n_neighbours,
                                   const OrbmRigMapPair* pairs, const OrbmMapParams* params, OrbmNewPoints* out, uint8_t* skipped)
{
    int r = rnp_check(kf1, neighbours, n_neighbours, pairs, params, out);
    if (r) return r;
    const int n1 = kf1->side.n;
    const OrbmFeatVec& fv1 = kf1->side.fv;
    const int nn1 = fv1.n_nodes, total1 = nn1 > 0 ? fv1.offset[nn1] : 0;
    const bool nothing = n1 == 0 || n_neighbours == 0 || total1 == 0;      // no search can match: no launch, and no device needed
    if (!m && !nothing) {                                       // no handle exists without a device: there is no CPU fallback
        const int r = stage::check_device(0);
        return r ? r : fail(ORBX_ERR_ARG, "NULL matcher");
    }
    const bool want_normal = out->normal != nullptr;
    for (int i = 0; i < n1; i++) {
        out->neighbour[i] = -1; out->idx2[i] = -1; out->point_stereo[i] = 0;
        out->x3d[3 * i] = out->x3d[3 * i + 1] = out->x3d[3 * i + 2] = 0.f;
        if (want_normal) { out->normal[3 * i] = out->normal[3 * i + 1] = out->normal[3 * i + 2] = 0.f; out->max_dist[i] = out->min_dist[i] = 0.f; }
    }
    for (int j = 0; j < n_neighbours; j++) out->n_matched[j] = out->n_created[j] = 0;
    if (out->match12)
        for (size_t i = 0; i < (size_t)n1 * n_neighbours; i++) out->match12[i] = -1;
    if (m) { m->rig_nmp_ms = 0.f; m->rig_nmp_launches = 0; }

    // the baseline test (:447-455) with either centre of key frame 1, in the reference's float expression
    uint8_t skipL[ORBM_MAX_NEIGHBOURS], skipR[ORBM_MAX_NEIGHBOURS], skip[ORBM_MAX_NEIGHBOURS];
    for (int j = 0; j < n_neighbours; j++) {
        skipL[j] = nmp_rig::baseline_too_short(kf1->Ow[0], neighbours[j].Ow[0], neighbours[j].mb) ? 1 : 0;
        skipR[j] = nmp_rig::baseline_too_short(kf1->Ow[1], neighbours[j].Ow[0], neighbours[j].mb) ? 1 : 0;
        skip[j] = skipL[j];
    }
    if (nothing) {                                              // no match can happen: Ow1 stays the left centre
        if (skipped) std::memcpy(skipped, skipL, n_neighbours);
        return 0;
    }

    ORBX_HIP(hipSetDevice(m->device));
    Blob blob(m);
    const int nkf = 1 + n_neighbours;
    std::vector<orbm::RnpKeyFrameDev> kfs(nkf);
    std::memset((void*)kfs.data(), 0, sizeof(orbm::RnpKeyFrameDev) * nkf);
    std::vector<int32_t> node_of(nn1);
    static const int32_t zero_off[1] = {0};
    for (int q = 0; q < nkf; q++) {
        const OrbmRigMapKeyFrame* k = q ? &neighbours[q - 1] : kf1;
        const OrbmTriSide& s = k->side;
        const int n = s.n, nn = s.fv.n_nodes, tot = nn > 0 ? s.fv.offset[nn] : 0;
        orbm::RnpKeyFrameDev& d = kfs[q];
        blob.in(d.desc, s.desc, (size_t)n * 32); blob.in(d.has_mp, s.has_mp, n);
        blob.in(d.x, s.x, n); blob.in(d.y, s.y, n); blob.in(d.octave, s.octave, n);
        blob.in(d.off, nn > 0 ? s.fv.offset : zero_off, nn + 1); blob.in(d.feat, s.fv.feat, tot);
        blob.in(d.sigma2, k->level_sigma2, k->n_levels); blob.in(d.scale, k->scale_factors, k->n_levels);
        if (q) {                                                // both node lists ascend (check_fv): one merge pass per neighbour
            int b = 0;
            for (int a = 0; a < nn1; a++) {
                while (b < nn && s.fv.node_id[b] < fv1.node_id[a]) b++;
                node_of[a] = (b < nn && s.fv.node_id[b] == fv1.node_id[a]) ? b : -1;
            }
            blob.in(d.node_of, node_of.data(), nn1);
        } else blob.none(d.node_of);
        for (int c = 0; c < 2; c++) {
            std::memcpy(d.side[c].pose.Rcw, k->Rcw[c], sizeof(float) * 9); std::memcpy(d.side[c].pose.tcw, k->tcw[c], sizeof(float) * 3);
            std::memcpy(d.side[c].pose.Ow, k->Ow[c], sizeof(float) * 3);
            rnp_cam(d.side[c].cam, k->cam[c]);
        }
        d.n_left = k->n_left;
        if (q) {
            const OrbmRigMapPair& p = pairs[q - 1];
            for (int c = 0; c < 4; c++) {       // ll, lr, rl, rr: camera 1 is key frame 1's (bRight1), camera 2 the neighbour's (bRight2)
                rnp_cam(d.rigs[c].l, p.geom->cam[c >> 1]); rnp_cam(d.rigs[c].r, p.geom->cam[2 + (c & 1)]);
                std::memcpy(d.rigs[c].R12, p.geom->R12[c], sizeof(float) * 9); std::memcpy(d.rigs[c].t12, p.geom->t12[c], sizeof(float) * 3);
            }
            d.coarse = p.coarse ? 1 : 0;
        }
    }
    std::vector<int32_t> entry_node(total1);
    for (int a = 0; a < nn1; a++)
        for (int e = fv1.offset[a]; e < fv1.offset[a + 1]; e++) entry_node[e] = a;
    orbm::RnpArgs A;
    blob.in(A.entry_node, entry_node.data(), total1);
    const size_t o_kf = blob.slot<orbm::RnpKeyFrameDev>(nkf);
    // outputs: `neighbour` (-1) and the three counters (0, 0, -1) travel with the inputs, the rest is written where neighbour >= 0
    const size_t o_out = blob.begin_out();
    const size_t o_cnt = blob.out(A.n_matched, n_neighbours);
    blob.out(A.n_created, n_neighbours); blob.out(A.max_matched_idx1, n_neighbours);
    const size_t cnt_end = blob.size();
    blob.out(A.neighbour, n1);
    const size_t in_bytes = blob.size();
    blob.out(A.idx2, n1); blob.out(A.x3d, (size_t)3 * n1);
    blob.out(A.normal, (size_t)3 * n1); blob.out(A.max_dist, n1); blob.out(A.min_dist, n1);
    if (out->match12) blob.out(A.match12, (size_t)n1 * n_neighbours); else A.match12 = nullptr;
    const size_t all_bytes = blob.size();
    r = m->ensure(all_bytes);
    if (r) return r;
    blob.bind(m->d_blob);
    blob.store(o_kf, kfs.data(), nkf);
    uint8_t* b = m->d_blob;
    uint8_t* h = m->h_blob.data();
    std::memset(blob.host(A.neighbour), 0xFF, sizeof(int32_t) * n1);
    std::memset(blob.host(A.max_matched_idx1), 0xFF, sizeof(int32_t) * n_neighbours);
    A.kf = blob.device<orbm::RnpKeyFrameDev>(o_kf);
    A.total1 = total1; A.n1 = n1;
    A.rule.inertial = params->inertial; A.rule.far_points = params->far_points; A.rule.th_far = params->th_far;
    A.rule.ratio_factor = 1.5f * params->scale_factor_1;
    A.last_scale = kf1->scale_factors[kf1->n_levels - 1];
    if ((r = m->rig_nmp_timer.create())) return r;
    ORBX_HIP(hipMemcpyAsync(b, h, in_bytes, hipMemcpyHostToDevice, m->stream));
    if (out->match12) ORBX_HIP(hipMemsetAsync(A.match12, 0xFF, sizeof(int32_t) * n1 * n_neighbours, m->stream));
    const int groups_per_block = orbm::kRnpThreads / orbm::kRnpGroup;
    const dim3 grid((total1 + groups_per_block - 1) / groups_per_block);
    const int32_t* h_matched = blob.host(A.n_matched);
    const int32_t* h_max = blob.host(A.max_matched_idx1);

    // Segments.  The state is which centre of key frame 1 the reference's Ow1 holds: 0 = left.  A neighbour whose test comes out
    // the same for both centres needs no state; before one where it differs the launches so far are finished and their counters
    // read back.  Neighbour 0 is never ambiguous: the state is "left".
    int state = 0, j0 = 0;
    unsigned long long mask = 0ull;
    while (j0 < n_neighbours) {
        int j1 = j0 + 1;
        while (j1 < n_neighbours && skipL[j1] == skipR[j1]) j1++;
        for (int j = j0; j < j1; j++)
            if (skip[j]) mask |= 1ull << j;
        A.j0 = j0; A.j1 = j1; A.skip = mask;
        if ((r = m->rig_nmp_timer.start(m->stream))) return r;
        hipLaunchKernelGGL(orbm::k_new_map_points_rig, grid, dim3(orbm::kRnpThreads), 0, m->stream, A);
        ORBX_HIP(hipGetLastError());
        if ((r = m->rig_nmp_timer.stop(m->stream))) return r;
        m->rig_nmp_launches++;
        if (j1 < n_neighbours)                                  // an ambiguous neighbour follows: the counters of this segment alone
            ORBX_HIP(hipMemcpyAsync(h + o_cnt, b + o_cnt, cnt_end - o_cnt, hipMemcpyDeviceToHost, m->stream));
        else
            ORBX_HIP(hipMemcpyAsync(h + o_out, b + o_out, all_bytes - o_out, hipMemcpyDeviceToHost, m->stream));
        ORBX_HIP(hipStreamSynchronize(m->stream));
        if ((r = m->rig_nmp_timer.read())) return r;
        m->rig_nmp_ms += m->rig_nmp_timer.ms;
        if (j1 < n_neighbours) {
            for (int j = j1 - 1; j >= j0; j--)
                if (!skip[j] && h_matched[j] > 0) { state = h_max[j] >= kf1->n_left ? 1 : 0; break; }
            skip[j1] = state ? skipR[j1] : skipL[j1];
        }
        j0 = j1;
    }

    const int32_t* h_nb = blob.host(A.neighbour); const int32_t* h_idx2 = blob.host(A.idx2);
    const float* h_x3d = blob.host(A.x3d); const float* h_nrm = blob.host(A.normal);
    const float* h_mx = blob.host(A.max_dist); const float* h_mn = blob.host(A.min_dist);
    int created = 0;
    for (int i = 0; i < n1; i++) {
        if (h_nb[i] < 0) continue;
        created++;
        out->neighbour[i] = h_nb[i]; out->idx2[i] = h_idx2[i];
        for (int c = 0; c < 3; c++) out->x3d[3 * i + c] = h_x3d[3 * i + c];
        if (want_normal) {
            for (int c = 0; c < 3; c++) out->normal[3 * i + c] = h_nrm[3 * i + c];
            out->max_dist[i] = h_mx[i]; out->min_dist[i] = h_mn[i];
        }
    }
    if (out->match12) std::memcpy(out->match12, blob.host(A.match12), sizeof(int32_t) * n1 * n_neighbours);
    std::memcpy(out->n_matched, h_matched, sizeof(int32_t) * n_neighbours);
    std::memcpy(out->n_created, blob.host(A.n_created), sizeof(int32_t) * n_neighbours);
    if (skipped) std::memcpy(skipped, skip, n_neighbours);
    return created;
}

float orbm_create_new_map_points_rig_last_kernel_ms(const orbm_matcher* m) { return m ? m->rig_nmp_ms : 0.0f; }
int orbm_create_new_map_points_rig_last_launches(const orbm_matcher* m) { return m ? m->rig_nmp_launches : 0; }

}  // extern "C"
