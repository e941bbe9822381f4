// aw_rays.h -- ray queries (aw_cast_rays, k_rays): mj_ray / the rangefinder sensor for a table of
// rays attached to bodies, every env (or a chosen subset) in one launch.  Along pnt + x vec: the
// first render entry crossed and the x >= 0 of that crossing.
//
// One workgroup per output row: wave 0 runs stage_pose (the env's params, its geom_size / geom_pos
// overrides, the kinematics at its current qpos), all threads stage the world poses of the primitive
// render entries into LDS (ray_geoms), then thread r owns ray r: it composes the ray into the world
// from its body's frame and walks the entries.  The walk is the wave's: its bound is the OR of the
// wave's keep masks (a readlane-style reduction), so every round works on one entry -- one primitive
// type, one LDS address read by all lanes (a broadcast, no bank conflicts) -- and the own mask bit,
// the bounding-sphere reject and ray_prim are per-lane predicates.  Nothing of DState is written.
//
// The crossing is mju_rayGeom's rule (ray_prim / ray_geom: the smallest root t >= 0, so a ray that
// starts inside a geom reports where it leaves it), evaluated on the unit direction from an origin
// moved along the ray to two bounding radii in front of the entry's centre (entry_near's remedy for
// the cancellation of the quadratic with the origin metres away; an origin inside that distance is
// used as it is), and divided by |vec| at the end.  Nearest wins, an exact tie goes to the lower entry.
//
// Two deviations from mj_ray:
//   * mesh geoms are absent (the meshes are not available offline); the hand's primitive collision
//     geoms are in the table, as in every render kernel;
//   * planes are hit from both sides and are finite where their size is positive, as the depth
//     renderer draws them (ray_prim); mj_ray hits an infinite plane's front face only.
// Sites are never hit.
#pragma once
#include "aw_common.h"
#include "aw_render.h"

namespace aw {

// aw_ray_rec (include/adroit_wave.h), field for field: the handle's device table holds these
struct RayRec {
  float pnt[3], vec[3];
  float xmax;
  int body;
  unsigned long long keep;
};
static_assert(sizeof(RayRec) == 40, "RayRec is aw_ray_rec");

// world poses of the primitive render entries of one env: what render_geoms computes, without the
// pixel boxes (no camera here), and with the bounding radius taken from the env's own size
struct RayGeoms {
  float pos[MAXRG][3], mat[MAXRG][9], size[MAXRG][3], rb[MAXRG];
  int type[MAXRG];
};

// A sibling of render_geoms, not a factor of it: the render kernels' frames are pinned bit for bit
// and keep the function they were compiled from.  The pose statements are the same ones.  rb: the
// model's rbound belongs to the model's size, and a per-env geom_size may be larger (hammer
// variation "size"), so the radius is MuJoCo's formula on the staged size; planes: 0 (no sphere).
AW_DEV void ray_geoms(const DModel& m, const Env& s, RayGeoms& r, int tid, int nthreads) {
  for (int g = tid; g < m.nrgeom; g += nthreads) {
    const int b = MD(rg_body, g), cg = MD(rg_cgeom, g);
    float lp[3], lq[4], bq[4], v[3], q[4], sz[3];
    for (int k = 0; k < 3; k++) lp[k] = MD(rg_pos, 3 * g + k);
    for (int k = 0; k < 4; k++) { lq[k] = MD(rg_quat, 4 * g + k); bq[k] = s.xquat[b][k]; }
    if (cg >= 0 && MD(geom_ovr, cg)) apply_ovr<3>(m, s, 4, cg, lp);
    rotvq(v, lp, bq);
    add3(r.pos[g], v, s.xpos[b]);
    mulq(q, bq, lq);
    q2m(r.mat[g], q);
    for (int k = 0; k < 3; k++) r.size[g][k] = sz[k] = cg >= 0 ? s.gsize[cg][k] : MD(rg_size, 3 * g + k);
    const int type = MD(rg_type, g);
    float rb = 0.f;
    if (type == GEOM_SPHERE) rb = sz[0];
    else if (type == GEOM_CAPSULE) rb = sz[0] + sz[1];
    else if (type == GEOM_CYLINDER) rb = sqrtf(sz[0] * sz[0] + sz[1] * sz[1]);
    else if (type == GEOM_BOX) rb = sqrtf(dot3(sz, sz));
    r.rb[g] = rb;
    r.type[g] = type;
  }
}

// OR of a 64-bit mask over the wave, the same value in every lane
AW_DEV unsigned long long wave_or64(unsigned long long v) {
  unsigned lo = (unsigned)v, hi = (unsigned)(v >> 32);
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    lo |= (unsigned)__shfl_xor((int)lo, d, 64);
    hi |= (unsigned)__shfl_xor((int)hi, d, 64);
  }
  return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)lo) |
         (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)hi) << 32;
}

// The nearest crossing t (metres along the unit direction d from o) of the ray with the entries of
// `keep`, and its entry; -1 / -1 when nothing is crossed.  tlim: crossings beyond it are not wanted
// (a cull only; the caller decides at xmax).  The reject is conservative -- the sphere is padded by
// more than the fp32 error of the test, |oc| 2^-22 at most in the perpendicular -- so the result is
// the exhaustive loop's.  Every lane of the wave must call this (the reduction and the loop are the
// wave's); a lane without a ray passes keep 0.
AW_DEV float ray_nearest(const RayGeoms& r, int ng, unsigned long long keep, const float* o, const float* d,
                         float tlim, int& hit) {
  const unsigned long long all = ng < 64 ? (1ull << ng) - 1ull : ~0ull;
  keep &= all;
  float best = 3.0e38f;
  hit = -1;
  for (unsigned long long mk = wave_or64(keep); mk; mk &= mk - 1ull) {
    const int g = __builtin_ctzll(mk);   // uniform: a scalar, and r.*[g] one address for the wave
    if (!((keep >> g) & 1ull)) continue;
    const float rb = r.rb[g];
    float s0 = 0.f;
    if (rb > 0.f) {
      float oc[3], perp[3];
      sub3(oc, r.pos[g], o);
      const float tc = dot3(oc, d);
      for (int k = 0; k < 3; k++) perp[k] = oc[k] - tc * d[k];
      const float rr = 1.001f * rb + 1.0e-5f + 4.0e-7f * (fabsf(oc[0]) + fabsf(oc[1]) + fabsf(oc[2]));
      if (dot3(perp, perp) > rr * rr || tc + rr < 0.f || tc - rr > fminf(best, tlim)) continue;
      s0 = fmaxf(tc - 2.f * rr, 0.f);
    }
    float o2[3];
    for (int k = 0; k < 3; k++) o2[k] = o[k] + s0 * d[k];
    const float t = ray_prim(r.pos[g], r.mat[g], r.size[g], r.type[g], o2, d);
    if (t >= 0.f && s0 + t < best) { best = s0 + t; hit = g; }
  }
  return hit >= 0 ? best : -1.f;
}

}  // namespace aw
