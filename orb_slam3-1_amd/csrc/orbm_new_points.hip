// orbm_new_points.hip -- LocalMapping::CreateNewMapPoints (reference src/LocalMapping.cc:392-716) as one launch:
// SearchForTriangulation against every neighbour plus the per-match geometry (orbm_new_points_geometry.h).
//
// The reference's call site builds ORBmatcher(0.6, false) (no rotation histogram), never writes vbMatched2 and visits every
// neighbour once, so a key-frame-1 feature interacts with nothing but its own chain: it walks the neighbours in order until
// the first one where it matches and passes every gate.  The kernel gives each entry of key frame 1's feature vector a
// group of 16 lanes: the lanes spread over the neighbour's features of the same vocabulary node, a (distance, position)
// key reduction picks what k_triangulation's sequential `dist > bestDist -> continue` rule picks (the LAST of the equally
// good candidates that pass the epipolar test), and lane 0 of the group runs the geometry.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "../../include/orbslam3_hip.h"
#include "hip_check.h"
#include "orbm_host.h"
#include "orbm_new_points_geometry.h"

namespace orbm {

constexpr int kNmpGroup = 16;           // lanes per key-frame-1 feature: a vocabulary node holds 10-20 features of a 1000-2000 feature key frame
constexpr int kNmpThreads = 256;

struct NmpKeyFrameDev {
    const uint8_t* desc; const uint8_t* has_mp; const uint8_t* stereo;
    const float* x; const float* y; const int32_t* octave;
    const float* u_right; const float* depth; const float* key_x; const float* key_y;
    const int32_t* off; const uint32_t* feat;       // mFeatVec, flattened
    const float* sigma2; const float* scale;
    const int32_t* node_of;                         // [nodes of key frame 1] -> the same vocabulary node in this key frame's mFeatVec or -1 (neighbours only)
    nmp::Camera cam;
    float F12[9]; float ep_x, ep_y;                 // of the pair (key frame 1, this neighbour)
    int32_t coarse;
};

struct NmpArgs {
    const NmpKeyFrameDev* kf;                       // [1 + n_nb], key frame 1 first
    const int32_t* entry_node;                      // [total1]: node (index into key frame 1's mFeatVec) of each flattened entry
    int32_t total1, n_nb, n1;
    nmp::Rule rule;
    float last_scale;                               // kf1->mvScaleFactors[nLevels - 1]
    int32_t* neighbour; int32_t* idx2; float* x3d; uint8_t* point_stereo;       // [n1], neighbour pre-set to -1
    float* normal; float* max_dist; float* min_dist;
    int32_t* n_matched; int32_t* n_created;         // [n_nb], pre-set to 0
    int32_t* match12;                               // [n_nb][n1] pre-set to -1, or NULL
};

__device__ __forceinline__ nmp::Obs nmp_obs(const NmpKeyFrameDev& K, int i)
{
    nmp::Obs o;
    o.x = K.x[i]; o.y = K.y[i]; o.ur = K.u_right[i]; o.depth = K.depth[i];
    o.kx = K.key_x[i]; o.ky = K.key_y[i];
    const int oct = K.octave[i];
    o.sigma2 = K.sigma2[oct]; o.scale = K.scale[oct];
    return o;
}

__global__ __launch_bounds__(kNmpThreads) void k_new_map_points(NmpArgs A)
{
    const int e1 = (blockIdx.x * kNmpThreads + threadIdx.x) / kNmpGroup;        // the 16 lanes of a group share e1 and every branch below
    const int sub = threadIdx.x & (kNmpGroup - 1);
    if (e1 >= A.total1) return;
    const NmpKeyFrameDev& K1 = A.kf[0];
    const int idx1 = (int)K1.feat[e1];
    if (K1.has_mp[idx1]) return;                                // already a MapPoint (src/ORBmatcher.cc:968)
    const int node1 = A.entry_node[e1];
    const bool bStereo1 = K1.stereo[idx1] != 0;
    const uint8_t* dd1 = K1.desc + (size_t)idx1 * 32;
    const float x1 = K1.x[idx1], y1 = K1.y[idx1];

    for (int j = 0; j < A.n_nb; j++) {
        const NmpKeyFrameDev& K2 = A.kf[1 + j];
        const int l2 = K2.node_of[node1];
        if (l2 < 0) continue;
        const float la = x1 * K2.F12[0] + y1 * K2.F12[3] + K2.F12[6];           // Pinhole::epipolarConstrain, as k_triangulation
        const float lb = x1 * K2.F12[1] + y1 * K2.F12[4] + K2.F12[7];
        const float lc = x1 * K2.F12[2] + y1 * K2.F12[5] + K2.F12[8];
        const float den = la * la + lb * lb;
        const int b2 = K2.off[l2], n2 = K2.off[l2 + 1] - b2;
        // min over (dist, ~position): the smallest distance among the candidates that pass every test, the last of them on ties
        unsigned long long key = ~0ull;
        for (int p = sub; p < n2; p += kNmpGroup) {
            const int idx2 = (int)K2.feat[b2 + p];
            if (K2.has_mp[idx2]) continue;
            const int dist = hamming256(dd1, K2.desc + (size_t)idx2 * 32);
            if (dist > TH_LOW) continue;
            const float kx = K2.x[idx2], ky = K2.y[idx2];
            const int o2 = K2.octave[idx2];
            if (!bStereo1 && !K2.stereo[idx2]) {
                const float distex = K2.ep_x - kx, distey = K2.ep_y - ky;
                if (distex * distex + distey * distey < 100 * K2.scale[o2]) continue;       // too close to the epipole (:1011)
            }
            bool ok = K2.coarse != 0;
            if (!ok && den != 0) {
                const float num = la * kx + lb * ky + lc;
                const float dsqr = num * num / den;
                ok = (double)dsqr < 3.84 * (double)K2.sigma2[o2];
            }
            if (ok) {
                const unsigned long long k = ((unsigned long long)dist << 32) | (unsigned)(0x7FFFFFFF - p);
                key = k < key ? k : key;
            }
        }
        for (int o = kNmpGroup / 2; o > 0; o >>= 1) {
            const unsigned long long other = __shfl_xor(key, o, kNmpGroup);
            key = other < key ? other : key;
        }
        if (key == ~0ull) continue;
        const int idx2 = (int)K2.feat[b2 + (0x7FFFFFFF - (int)(key & 0xFFFFFFFFu))];
        int created = 0;
        if (sub == 0) {
            atomicAdd(&A.n_matched[j], 1);
            if (A.match12) A.match12[(size_t)j * A.n1 + idx1] = idx2;
            float x3D[3];
            int pstereo = 0;
            created = nmp::new_point(K1.cam, nmp_obs(K1, idx1), K2.cam, nmp_obs(K2, idx2), A.rule, x3D, &pstereo) ? 1 : 0;
            if (created) {
                A.neighbour[idx1] = j; A.idx2[idx1] = idx2; A.point_stereo[idx1] = (uint8_t)pstereo;
                A.x3d[3 * idx1] = x3D[0]; A.x3d[3 * idx1 + 1] = x3D[1]; A.x3d[3 * idx1 + 2] = x3D[2];
                nmp::normal_and_depth(x3D, K1.cam.Ow, K2.cam.Ow, K1.scale[K1.octave[idx1]], A.last_scale,
                                      A.normal + 3 * idx1, A.max_dist + idx1, A.min_dist + idx1);
                atomicAdd(&A.n_created[j], 1);
            }
        }
        if (__shfl(created, 0, kNmpGroup)) break;               // the feature holds a map point from here on
    }
}

}  // namespace orbm

namespace {

int check_key_frame(const OrbmMapKeyFrame* k, const char* name)
{
    const OrbmTriSide& s = k->side;
    if (s.n < 0) return fail(ORBX_ERR_ARG, "%s: negative feature count", name);
    if (s.n > 0 && (!s.desc || !s.has_mp || !s.stereo || !s.x || !s.y || !s.octave || !k->u_right || !k->depth))
        return fail(ORBX_ERR_ARG, "%s: NULL key-frame arrays", name);
    if ((k->key_x == nullptr) != (k->key_y == nullptr)) return fail(ORBX_ERR_ARG, "%s: key_x and key_y go together", name);
    if (k->n_levels < 1 || !k->level_sigma2 || !k->scale_factors) return fail(ORBX_ERR_ARG, "%s: NULL scale tables", name);
    const int r = check_fv(&s.fv, s.n, name);
    if (r) return r;
    if (s.fv.n_nodes > 0 && s.fv.offset[0] != 0) return fail(ORBX_ERR_ARG, "%s: feature-vector offsets must start at 0", name);
    if (!features_unique(&s.fv, s.n)) return fail(ORBX_ERR_ARG, "%s: a feature appears in two vocabulary nodes", name);
    for (int i = 0; i < s.n; i++)
        if (s.octave[i] < 0 || s.octave[i] >= k->n_levels) return fail(ORBX_ERR_ARG, "%s: octave out of range", name);
    return ORBX_OK;
}

}  // namespace

extern "C" {

int orbm_create_new_map_points(orbm_matcher* m, const OrbmMapKeyFrame* kf1, const OrbmMapKeyFrame* neighbours, int n_neighbours,
                               const OrbmMapPair* pairs, const OrbmMapParams* params, OrbmNewPoints* out)
{
    if (!kf1 || !params || !out) return fail(ORBX_ERR_ARG, "NULL argument");
    if (n_neighbours < 0 || n_neighbours > ORBM_MAX_NEIGHBOURS) return fail(ORBX_ERR_ARG, "n_neighbours %d outside [0, %d]", n_neighbours, ORBM_MAX_NEIGHBOURS);
    if (n_neighbours > 0 && (!neighbours || !pairs || !out->n_matched || !out->n_created)) return fail(ORBX_ERR_ARG, "NULL neighbour arrays");
    int r = check_key_frame(kf1, "kf1");
    if (r) return r;
    for (int j = 0; j < n_neighbours; j++)
        if ((r = check_key_frame(&neighbours[j], "neighbour")) != ORBX_OK) return r;
    const int n1 = kf1->side.n;
    if (n1 > 0 && (!out->neighbour || !out->idx2 || !out->x3d || !out->point_stereo)) return fail(ORBX_ERR_ARG, "NULL output arrays");
    const bool want_normal = out->normal || out->max_dist || out->min_dist;
    if (want_normal && n1 > 0 && (!out->normal || !out->max_dist || !out->min_dist)) return fail(ORBX_ERR_ARG, "normal, max_dist and min_dist go together");
    if (!m) {                                                   // no handle exists without a device: there is no CPU fallback
        const int r = stage::check_device(0);
        return r ? r : fail(ORBX_ERR_ARG, "NULL matcher");
    }
    for (int i = 0; i < n1; i++) {
        out->neighbour[i] = -1; out->idx2[i] = -1; out->point_stereo[i] = 0;
        out->x3d[3 * i] = out->x3d[3 * i + 1] = out->x3d[3 * i + 2] = 0.f;
        if (want_normal) { out->normal[3 * i] = out->normal[3 * i + 1] = out->normal[3 * i + 2] = 0.f; out->max_dist[i] = out->min_dist[i] = 0.f; }
    }
    for (int j = 0; j < n_neighbours; j++) out->n_matched[j] = out->n_created[j] = 0;
    if (out->match12)
        for (size_t i = 0; i < (size_t)n1 * n_neighbours; i++) out->match12[i] = -1;
    const OrbmFeatVec& fv1 = kf1->side.fv;
    const int nn1 = fv1.n_nodes, total1 = nn1 > 0 ? fv1.offset[nn1] : 0;
    if (n1 == 0 || n_neighbours == 0 || total1 == 0) return 0;

    ORBX_HIP(hipSetDevice(m->device));
    Blob blob(m);
    const int nkf = 1 + n_neighbours;
    std::vector<orbm::NmpKeyFrameDev> kfs(nkf);
    std::memset((void*)kfs.data(), 0, sizeof(orbm::NmpKeyFrameDev) * nkf);
    std::vector<int32_t> node_of(nn1);
    for (int q = 0; q < nkf; q++) {
        const OrbmMapKeyFrame* k = q ? &neighbours[q - 1] : kf1;
        const OrbmTriSide& s = k->side;
        const int n = s.n, nn = s.fv.n_nodes, tot = nn > 0 ? s.fv.offset[nn] : 0;
        orbm::NmpKeyFrameDev& d = kfs[q];
        blob.in(d.desc, s.desc, (size_t)n * 32); blob.in(d.has_mp, s.has_mp, n); blob.in(d.stereo, s.stereo, n);
        blob.in(d.x, s.x, n); blob.in(d.y, s.y, n); blob.in(d.octave, s.octave, n);
        blob.in(d.u_right, k->u_right, n); blob.in(d.depth, k->depth, n);
        if (k->key_x) { blob.in(d.key_x, k->key_x, n); blob.in(d.key_y, k->key_y, n); }
        else { blob.alias(d.key_x, d.x); blob.alias(d.key_y, d.y); }
        blob.in(d.off, s.fv.offset, nn > 0 ? nn + 1 : 0); blob.in(d.feat, s.fv.feat, tot);
        blob.in(d.sigma2, k->level_sigma2, k->n_levels); blob.in(d.scale, k->scale_factors, k->n_levels);
        if (q) {                                                // both node lists ascend (check_fv): one merge pass per neighbour
            int b = 0;
            for (int a = 0; a < nn1; a++) {
                while (b < nn && s.fv.node_id[b] < fv1.node_id[a]) b++;
                node_of[a] = (b < nn && s.fv.node_id[b] == fv1.node_id[a]) ? b : -1;
            }
            blob.in(d.node_of, node_of.data(), nn1);
        } else blob.none(d.node_of);
        std::memcpy(d.cam.Rcw, k->Rcw, sizeof(d.cam.Rcw)); std::memcpy(d.cam.tcw, k->tcw, sizeof(d.cam.tcw)); std::memcpy(d.cam.Ow, k->Ow, sizeof(d.cam.Ow));
        d.cam.fx = k->fx; d.cam.fy = k->fy; d.cam.cx = k->cx; d.cam.cy = k->cy; d.cam.invfx = k->invfx; d.cam.invfy = k->invfy;
        d.cam.mb = k->mb; d.cam.mbf = k->mbf;
        if (q) {
            const OrbmMapPair& p = pairs[q - 1];
            std::memcpy(d.F12, p.F12, sizeof(d.F12)); d.ep_x = p.ep_x; d.ep_y = p.ep_y; d.coarse = p.coarse;
        }
    }
    std::vector<int32_t> entry_node(total1);
    for (int a = 0; a < nn1; a++)
        for (int e = fv1.offset[a]; e < fv1.offset[a + 1]; e++) entry_node[e] = a;
    orbm::NmpArgs A;
    blob.in(A.entry_node, entry_node.data(), total1);
    const size_t o_kf = blob.slot<orbm::NmpKeyFrameDev>(nkf);
    // outputs: `neighbour` (-1) and the two counters (0) travel with the inputs, the rest is written where neighbour >= 0
    const size_t o_out = blob.begin_out();
    blob.out(A.neighbour, n1); blob.out(A.n_matched, n_neighbours); blob.out(A.n_created, n_neighbours);
    const size_t in_bytes = blob.size();
    blob.out(A.idx2, n1); blob.out(A.x3d, (size_t)3 * n1); blob.out(A.point_stereo, n1);
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
    A.kf = blob.device<orbm::NmpKeyFrameDev>(o_kf);
    A.total1 = total1; A.n_nb = n_neighbours; A.n1 = n1;
    A.rule.inertial = params->inertial; A.rule.far_points = params->far_points; A.rule.th_far = params->th_far;
    A.rule.ratio_factor = 1.5f * params->scale_factor_1;
    A.last_scale = kf1->scale_factors[kf1->n_levels - 1];
    if ((r = m->nmp_timer.create())) return r;
    ORBX_HIP(hipMemcpyAsync(b, h, in_bytes, hipMemcpyHostToDevice, m->stream));
    if (out->match12) ORBX_HIP(hipMemsetAsync(A.match12, 0xFF, sizeof(int32_t) * n1 * n_neighbours, m->stream));
    const int groups_per_block = orbm::kNmpThreads / orbm::kNmpGroup;
    if ((r = m->nmp_timer.start(m->stream))) return r;
    hipLaunchKernelGGL(orbm::k_new_map_points, dim3((total1 + groups_per_block - 1) / groups_per_block), dim3(orbm::kNmpThreads), 0, m->stream, A);
    ORBX_HIP(hipGetLastError());
    if ((r = m->nmp_timer.stop(m->stream))) return r;
    ORBX_HIP(hipMemcpyAsync(h + o_out, b + o_out, all_bytes - o_out, hipMemcpyDeviceToHost, m->stream));
    ORBX_HIP(hipStreamSynchronize(m->stream));
    if ((r = m->nmp_timer.read())) return r;

    const int32_t* h_nb = blob.host(A.neighbour); const int32_t* h_idx2 = blob.host(A.idx2);
    const float* h_x3d = blob.host(A.x3d); const float* h_nrm = blob.host(A.normal);
    const float* h_mx = blob.host(A.max_dist); const float* h_mn = blob.host(A.min_dist);
    const uint8_t* h_ps = blob.host(A.point_stereo);
    int created = 0;
    for (int i = 0; i < n1; i++) {
        if (h_nb[i] < 0) continue;
        created++;
        out->neighbour[i] = h_nb[i]; out->idx2[i] = h_idx2[i]; out->point_stereo[i] = h_ps[i];
        for (int c = 0; c < 3; c++) out->x3d[3 * i + c] = h_x3d[3 * i + c];
        if (want_normal) {
            for (int c = 0; c < 3; c++) out->normal[3 * i + c] = h_nrm[3 * i + c];
            out->max_dist[i] = h_mx[i]; out->min_dist[i] = h_mn[i];
        }
    }
    if (out->match12) std::memcpy(out->match12, blob.host(A.match12), sizeof(int32_t) * n1 * n_neighbours);
    std::memcpy(out->n_matched, blob.host(A.n_matched), sizeof(int32_t) * n_neighbours);
    std::memcpy(out->n_created, blob.host(A.n_created), sizeof(int32_t) * n_neighbours);
    return created;
}

float orbm_create_new_map_points_last_kernel_ms(const orbm_matcher* m) { return m ? m->nmp_timer.ms : 0.0f; }

}  // extern "C"
