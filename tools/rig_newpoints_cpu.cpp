// One-core host half of the sequence orbm_create_new_map_points_rig replaces, for tools/rig_newpoints_timing.py: after every
// per-neighbour search on the device the matches are triangulated on the host with csrc/orbm_new_points_rig_geometry.h -- the
// very functions k_new_map_points_rig runs --, has_mp of key frame 1 is updated for the next search, and the Ow1 state of
// LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:423, :512-542) is carried.  Built as a shared library and called in
// process: g++ -O3 -ffp-contract=off -shared -fPIC -I include.
#include <cstdint>
#include <cstring>

#include "orbslam3_hip.h"
#include "../orb_slam3-1_amd/csrc/orbm_new_points_rig_geometry.h"

static nmp_rig::Side side_of(const OrbmRigMapKeyFrame* k, int right)
{
    nmp_rig::Side s;
    std::memset(&s, 0, sizeof(s));
    std::memcpy(s.pose.Rcw, k->Rcw[right], sizeof(s.pose.Rcw)); std::memcpy(s.pose.tcw, k->tcw[right], sizeof(s.pose.tcw));
    std::memcpy(s.pose.Ow, k->Ow[right], sizeof(s.pose.Ow));
    const float* p = k->cam[right];
    s.cam.fx = p[0]; s.cam.fy = p[1]; s.cam.cx = p[2]; s.cam.cy = p[3];
    for (int q = 0; q < 4; q++) s.cam.k[q] = p[4 + q];
    s.cam.precision = p[8];
    return s;
}

static nmp_rig::Obs obs_of(const OrbmRigMapKeyFrame* k, int i)
{
    nmp_rig::Obs o;
    o.x = k->side.x[i]; o.y = k->side.y[i];
    o.sigma2 = k->level_sigma2[k->side.octave[i]]; o.scale = k->scale_factors[k->side.octave[i]];
    return o;
}

extern "C" {

// the baseline test of :447-455 with the centre the state names (0: left, 1: right)
int rnp_cpu_skip(const OrbmRigMapKeyFrame* kf1, const OrbmRigMapKeyFrame* kf2, int state)
{
    return nmp_rig::baseline_too_short(kf1->Ow[state ? 1 : 0], kf2->Ow[0], kf2->mb) ? 1 : 0;
}

// the matches of neighbour j in ascending idx1: geometry, outputs and has_mp1 for the accepted ones, *state for every match.
// Returns the number of points created.
int rnp_cpu_neighbour(const OrbmRigMapKeyFrame* kf1, const OrbmRigMapKeyFrame* kf2, const int32_t* match12, const OrbmMapParams* params, int j, uint8_t* has_mp1,
                      int32_t* neighbour, int32_t* idx2_out, float* x3d, float* normal, float* max_dist, float* min_dist, int32_t* state)
{
    nmp::Rule rule;
    rule.inertial = params->inertial; rule.far_points = params->far_points; rule.th_far = params->th_far; rule.ratio_factor = 1.5f * params->scale_factor_1;
    const nmp_rig::Side S1[2] = {side_of(kf1, 0), side_of(kf1, 1)}, S2[2] = {side_of(kf2, 0), side_of(kf2, 1)};
    const float last_scale = kf1->scale_factors[kf1->n_levels - 1];
    int created = 0;
    for (int i1 = 0; i1 < kf1->side.n; i1++) {
        const int i2 = match12[i1];
        if (i2 < 0) continue;
        const int r1 = i1 >= kf1->n_left ? 1 : 0, r2 = i2 >= kf2->n_left ? 1 : 0;
        *state = r1;
        float X[3];
        if (!nmp_rig::new_point(S1[r1], obs_of(kf1, i1), S2[r2], obs_of(kf2, i2), rule, X)) continue;
        has_mp1[i1] = 1;
        neighbour[i1] = j; idx2_out[i1] = i2;
        x3d[3 * i1] = X[0]; x3d[3 * i1 + 1] = X[1]; x3d[3 * i1 + 2] = X[2];
        nmp_rig::normal_and_depth(X, S1[r1].pose.Ow, S2[r2].pose.Ow, S1[0].pose.Ow, kf1->scale_factors[kf1->side.octave[i1]], last_scale, normal + 3 * i1,
                                  max_dist + i1, min_dist + i1);
        created++;
    }
    return created;
}

}  // extern "C"
