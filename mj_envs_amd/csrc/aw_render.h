// aw_render.h -- depth, colour and segmentation ray casting against primitive geoms and sites (fp32).
//
// Replaces the reference's OpenGL frame (hand_manipulation_suite/headless_observer.py:34-52)
// with metric z-depth and a Phong-shaded colour frame; see mj_envs_amd/render.py for the camera
// construction and the shading model.  numpy restatements for the tests: oracle/depth.py
// (geometry), tests/rgb_checker.py (colour), tests/label_checker.py (segmentation).
#pragma once
#include "aw_common.h"
#include "aw_dynamics.h"
#include "aw_solver.h"

namespace aw {

// first crossing t >= 0 of the ray o + t v (v unit, world frame) with a primitive geom, or -1;
// planes are finite where their size is positive (as MuJoCo draws them)
AW_DEV float ray_prim(const float* pos, const float* mat, const float* size, int type, const float* o,
                      const float* v) {
  if (type == GEOM_PLANE) {
    float dif[3], lp[3], lv[3];
    sub3(dif, o, pos);
    mulmtv3(lp, mat, dif);
    mulmtv3(lv, mat, v);
    if (fabsf(lv[2]) < MINVAL) return -1.f;
    const float t = -lp[2] / lv[2];
    if (t < 0.f) return -1.f;
    const float x = lp[0] + t * lv[0], y = lp[1] + t * lv[1];
    if ((size[0] > 0.f && fabsf(x) > size[0]) || (size[1] > 0.f && fabsf(y) > size[1])) return -1.f;
    return t;
  }
  return ray_geom(pos, mat, size, o, v, type);
}

// world poses of the rendered entries of one env (s.xpos / s.xquat from stage_kinematics):
// the primitive geoms, then (colour renderer only) the visible sites
struct RGeoms {
  float pos[MAXRG][3], mat[MAXRG][9], size[MAXRG][3], rb[MAXRG];
  float box[MAXRG][4];   // conservative pixel box of the bounding sphere: col min / max, row min / max
  int type[MAXRG];
};

// image-space box of entry g's bounding sphere: x / z over the sphere's camera-frame bounding box
// is extremal at its corners (conservative); behind / straddling the camera or unbounded
// (planes: rbound 0) -> the whole image
AW_DEV void pixel_box(RGeoms& r, int g, const float* cam) {
  const float rb = r.rb[g];
  float c[3], x = 0.f, y = 0.f, z = 0.f;
  sub3(c, r.pos[g], cam);
  x = dot3(c, cam + 9); y = dot3(c, cam + 6); z = dot3(c, cam + 3);
  float b0 = -1e30f, b1 = 1e30f, b2 = -1e30f, b3 = 1e30f;
  if (rb > 0.f && z - rb > 1e-3f) {
    const float z0 = z - rb, z1 = z + rb;
    const float umin = fminf((x - rb) / z0, (x - rb) / z1), umax = fmaxf((x + rb) / z0, (x + rb) / z1);
    const float vmin = fminf((y - rb) / z0, (y - rb) / z1), vmax = fmaxf((y + rb) / z0, (y + rb) / z1);
    b0 = (umin - cam[12]) / cam[13] - 1.f;   // column range (one pixel of slack)
    b1 = (umax - cam[12]) / cam[13] + 1.f;
    b2 = (cam[14] - vmax) / cam[15] - 1.f;   // row range
    b3 = (cam[14] - vmin) / cam[15] + 1.f;
  }
  r.box[g][0] = b0; r.box[g][1] = b1; r.box[g][2] = b2; r.box[g][3] = b3;
}

AW_DEV void render_geoms(const DModel& m, const Env& s, RGeoms& r, const float* cam, int tid, int nthreads) {
  for (int g = tid; g < m.nrgeom; g += nthreads) {
    const int b = MD(rg_body, g), cg = MD(rg_cgeom, g);
    float lp[3], lq[4], bq[4], v[3], q[4];
    for (int k = 0; k < 3; k++) lp[k] = MD(rg_pos, 3 * g + k);
    for (int k = 0; k < 4; k++) { lq[k] = MD(rg_quat, 4 * g + k); bq[k] = s.xquat[b][k]; }
    if (cg >= 0 && MD(geom_ovr, cg)) apply_ovr<3>(m, s, 4, cg, lp);
    rotvq(v, lp, bq);
    add3(r.pos[g], v, s.xpos[b]);
    mulq(q, bq, lq);
    q2m(r.mat[g], q);
    for (int k = 0; k < 3; k++) r.size[g][k] = cg >= 0 ? s.gsize[cg][k] : MD(rg_size, 3 * g + k);
    r.rb[g] = MD(rg_rbound, g);
    r.type[g] = MD(rg_type, g);
    pixel_box(r, g, cam);
  }
}

// entries [nrgeom, nrgeom + nrsite): the visible sites, at the site positions of stage_kinematics
// (per-env site_pos overrides applied there)
AW_DEV void render_sites(const DModel& m, const Env& s, RGeoms& r, const float* cam, int tid, int nthreads) {
  for (int g = m.nrgeom + tid; g < m.nrgeom + m.nrsite; g += nthreads) {
    const int b = MD(rg_body, g);
    float lq[4], bq[4], q[4];
    for (int k = 0; k < 4; k++) { lq[k] = MD(rg_quat, 4 * g + k); bq[k] = s.xquat[b][k]; }
    copy3(r.pos[g], s.sxpos[MD(rg_site, g)]);
    mulq(q, bq, lq);
    q2m(r.mat[g], q);
    for (int k = 0; k < 3; k++) r.size[g][k] = MD(rg_size, 3 * g + k);
    r.rb[g] = MD(rg_rbound, g);
    r.type[g] = MD(rg_type, g);
    pixel_box(r, g, cam);
  }
}

// the entries among [0, ne) whose pixel box meets the rows of the 64-pixel span at p0: found once
// per wave (lane g tests entry g, ballot)
AW_DEV unsigned long long span_entries(const RGeoms& r, int ne, int W, int H, int p0, int lane) {
  const int rlo = p0 / W, rhi = min(p0 + 63, W * H - 1) / W;
  const bool on = lane < ne && r.box[lane][2] <= (float)rhi && r.box[lane][3] >= (float)rlo;
  return __ballot(on);
}

// unit direction of the ray through image position (col, row) (fractional: supersampling)
AW_DEV void pixel_ray(const float* cam, float col, float row, float* d) {
  const float u = cam[12] + cam[13] * col, w = cam[14] - cam[15] * row;
  for (int k = 0; k < 3; k++) d[k] = cam[3 + k] + u * cam[9 + k] + w * cam[6 + k];
  normalize3(d);
}

// entry g against the ray of pixel (fc, fr): column / row box, bounding-sphere cull against the
// nearest crossing so far, exact ray-primitive test; the crossing t or -1
AW_DEV float entry_hit(const RGeoms& r, int g, const float* cam, const float* d, float fc, float fr, float best) {
  if (fc < r.box[g][0] || fc > r.box[g][1] || fr < r.box[g][2] || fr > r.box[g][3]) return -1.f;
  const float rb = r.rb[g];
  if (rb > 0.f) {
    float oc[3];
    sub3(oc, r.pos[g], cam);
    const float tc = dot3(oc, d);
    const float d2 = dot3(oc, oc) - tc * tc;
    if (d2 > rb * rb || tc + rb < 0.f || tc - rb > best) return -1.f;
  }
  return ray_prim(r.pos[g], r.mat[g], r.size[g], r.type[g], cam, d);
}

// nearest crossing of the ray with the entries of mask (3e38 if none) and its entry
AW_DEV float nearest_hit(const RGeoms& r, unsigned long long mask, const float* cam, const float* d, float fc,
                         float fr, int& hit) {
  float best = 3.0e38f;
  hit = -1;
  while (mask) {
    const int g = __builtin_ctzll(mask);
    mask &= mask - 1ull;
    const float t = entry_hit(r, g, cam, d, fc, fr, best);
    if (t >= 0.f && t < best) { best = t; hit = g; }
  }
  return best;
}

// z-depth of the 64 pixels [p0, p0 + 64) handled by one wave
AW_DEV void render_span(const RGeoms& r, int ng, const float* cam, int W, int H, int p0, int lane, float* out) {
  const int np = W * H;
  const int p = p0 + lane;
  const unsigned long long mask = span_entries(r, ng, W, H, p0, lane);
  const int row = p / W, col = p - row * W;
  float d[3];
  pixel_ray(cam, (float)col, (float)row, d);
  int hit;
  const float best = nearest_hit(r, mask, cam, d, (float)col, (float)row, hit);
  if (p < np) out[p] = best < 1.0e38f ? best * dot3(d, cam + 3) : cam[16];
}

// Segmentation.  nearest_hit's crossings carry the cancellation of ray_geom's quadratic, b^2 - a c
// with the ray origin metres from a round geom a few millimetres thick: about 1e-4 m for a finger
// link 4.5 m from the free camera.  Depth takes that (2e-3 m is its gate), a label does not: where
// two links overlap at a joint, crossings 3e-4 m apart change their order and the pixel names a
// link that no ray near it sees.  So labels order the entries that cross within LABEL_TIE of the
// nearest by entry_near: the crossing from an origin moved along the ray to two bounding radii in
// front of the entry's centre, where the same fp32 arithmetic is good to about 1e-6 m.
// Crossings that entry_near cannot tell apart (LABEL_EPS of the distance: coplanar faces, such as a
// cylinder's cap flush with a box) go to the lower entry, as an exact tie does.
constexpr float LABEL_TIE = 2.0e-3f;   // the depth gate: what nearest_hit's order is trusted to
constexpr float LABEL_EPS = 4.0e-6f;   // of t: a few times entry_near's error (ulp(t) for the moved origin and the sum)

// entry_hit's culls against lim, then the crossing t of entry g along cam + t d evaluated from the
// origin cam + s d, s = max(0, (centre - cam) . d - 2 rbound) (outside the bounding sphere, in front
// of it; planes, rbound 0: from cam itself, no quadratic), or -1
AW_DEV float entry_near(const RGeoms& r, int g, const float* cam, const float* d, float fc, float fr, float lim) {
  if (fc < r.box[g][0] || fc > r.box[g][1] || fr < r.box[g][2] || fr > r.box[g][3]) return -1.f;
  const float rb = r.rb[g];
  float s = 0.f;
  if (rb > 0.f) {
    float oc[3];
    sub3(oc, r.pos[g], cam);
    const float tc = dot3(oc, d);
    const float d2 = dot3(oc, oc) - tc * tc;
    if (d2 > rb * rb || tc + rb < 0.f || tc - rb > lim) return -1.f;
    s = fmaxf(tc - 2.f * rb, 0.f);
  }
  float o[3];
  for (int k = 0; k < 3; k++) o[k] = cam[k] + s * d[k];
  const float t = ray_prim(r.pos[g], r.mat[g], r.size[g], r.type[g], o, d);
  return t >= 0.f ? s + t : -1.f;
}

// what pixel p0 + lane of the 64 pixels [p0, p0 + 64) handled by one wave shows: its render entry
// (-1: nothing), the unit ray d, the crossing `front` the search ends on, the crossing `near` of
// nearest_hit's loop (what depth is written from; 3e38: no geom) and optionally the z-depth.
// Geoms: render_span's search (nearest_hit's loop) says whether the ray hits anything and how deep -- depth
// is written from it, so it is render_span's depth bit for bit, and a pixel is background exactly
// where that depth is zfar; among the geoms crossing within LABEL_TIE of it the nearest by
// entry_near is the label (within LABEL_EPS the lower entry).  Sites (ns > 0): the nearest
// visible-site crossing in front of that geom replaces it (a geom wins a tie; among sites the
// nearest, then the lower entry -- "in front of the opaque crossing" as render_span_rgb blends, drawn
// solid), by entry_near as well.
AW_DEV int span_hit(const RGeoms& r, int ng, int ns, const float* cam, int W, int H, int p0, int lane, float* depth,
                    float* d, float& front, float& near) {
  const int np = W * H;
  const int p = p0 + lane;
  const unsigned long long all = span_entries(r, ng + ns, W, H, p0, lane);
  const unsigned long long gmask = ng < 64 ? all & ((1ull << ng) - 1ull) : all, smask = ng < 64 ? all >> ng : 0ull;
  const int row = p / W, col = p - row * W;
  const float fc = (float)col, fr = (float)row;
  pixel_ray(cam, fc, fr, d);
  // nearest_hit's loop, statement for statement (the same entry_hit calls in the same order, so the
  // same best), which also keeps the entries that crossed within LABEL_TIE of the nearest so far;
  // a crossing more than LABEL_TIE in front of all before it (each >= best) drops them.  What is
  // left holds every entry within LABEL_TIE of the final best: mostly the hit alone
  float best = 3.0e38f;
  int hit = -1;
  unsigned long long cand = 0ull;
  for (unsigned long long mk = gmask; mk; mk &= mk - 1ull) {
    const int g = __builtin_ctzll(mk);
    const float t = entry_hit(r, g, cam, d, fc, fr, best);
    if (t >= 0.f && t < best + LABEL_TIE) cand = (t + LABEL_TIE < best ? 0ull : cand) | 1ull << g;
    if (t >= 0.f && t < best) { best = t; hit = g; }
  }
  if (depth && p < np) depth[p] = best < 1.0e38f ? best * dot3(d, cam + 3) : cam[16];
  front = near = best;
  if (hit >= 0 && ((cand & (cand - 1ull)) || ns > 0)) {   // sites are compared with entry_near's crossing
    const int coarse = hit;
    hit = -1;
    front = 3.0e38f;
    unsigned long long mk = cand;
    while (mk) {
      const int g = __builtin_ctzll(mk);
      mk &= mk - 1ull;
      const float t = entry_near(r, g, cam, d, fc, fr, g == coarse ? 3.0e38f : best + LABEL_TIE);
      if (t >= 0.f && t < front - LABEL_EPS * front) { front = t; hit = g; }
    }
    if (hit < 0) { hit = coarse; front = best; }   // grazing: the moved origin misses what the camera's just hit
  }
  unsigned long long mk = smask;
  while (mk) {
    const int g = ng + __builtin_ctzll(mk);
    mk &= mk - 1ull;
    const float t = entry_near(r, g, cam, d, fc, fr, front);
    if (t >= 0.f && t < front - LABEL_EPS * front) { front = t; hit = g; }
  }
  return hit;
}
// segmentation label (and optionally z-depth) of the span: one dword per lane, lut[entry] of
// span_hit, or background
AW_DEV void render_span_labels(const RGeoms& r, int ng, int ns, const float* cam, const int* lut, int background,
                               int W, int H, int p0, int lane, int* out, float* depth) {
  float d[3], front, near;
  const int hit = span_hit(r, ng, ns, cam, W, H, p0, lane, depth, d, front, near);
  if (p0 + lane < W * H) out[p0 + lane] = hit >= 0 ? lut[hit] : background;
}

// Point cloud (aw_render_cloud): whether pixel p0 + lane is a candidate -- span_hit finds an entry, the
// entry's bit of `keep` is set and the world point pt = cam + t d lies inside the closed box (lo xyz,
// hi xyz; nullptr: no crop).  t: for a geom the crossing the depth frame is written from (`near`), so
// the cloud is that frame unprojected, the same t a few roundings apart -- `front` is the same
// crossing wherever one geom is hit alone, and where several cross within LABEL_TIE it is entry_near's
// re-evaluation, up to nearest_hit's cancellation error (1e-4 m at 4.5 m) away; for a site, which
// writes no depth, its own crossing `front`.  pt is written either way.
AW_DEV bool render_span_cloud(const RGeoms& r, int ng, int ns, const float* cam, unsigned long long keep,
                              const float* box, int W, int H, int p0, int lane, float* pt) {
  float d[3], front, near;
  const int hit = span_hit(r, ng, ns, cam, W, H, p0, lane, nullptr, d, front, near);
  const float t = hit >= ng ? front : near;
  for (int k = 0; k < 3; k++) pt[k] = cam[k] + t * d[k];
  bool in = p0 + lane < W * H && hit >= 0 && ((keep >> (hit & 63)) & 1ull) != 0ull;
  if (box)
    for (int k = 0; k < 3; k++) in = in && pt[k] >= box[k] && pt[k] <= box[3 + k];
  return in;
}

// ---------------------------------------------------------------------------------------
// colour: Phong shading of the nearest opaque geom, visible sites blended over it
constexpr int MAXSITEHIT = 4;       // translucent crossings kept per ray (the nearest)

struct RColors {
  float col[MAXRG][COL_W];
  float light[MAXLIGHT + 1][LIGHT_W];
  int nlight;
  unsigned bytes[4][48];             // one wave's 64 rgb pixels, repacked into dwords
};

// the part of the per-env colour table that no camera enters: entry colours (tint rows: a colour
// channel read from the env's params) and the model's lights, behind the headlight's slot
// (look: background rgb, headlight ambient / diffuse / specular, headlight on)
// col / light (aw_set_appearance): this env's own records, [ne][COL_W] / [nlight][LIGHT_W] in device
// memory, in place of the model's; nullptr: the model's.  The tint rows apply on top of either.
AW_DEV void render_colors_env(const DModel& m, const Env& s, RColors& c, const float* look, int tid, int nthreads,
                              const float* col = nullptr, const float* light = nullptr) {
  const int ne = m.nrgeom + m.nrsite;
  for (int i = tid; i < ne * COL_W; i += nthreads) {
    const int e = i / COL_W, k = i - e * COL_W;
    float v = col ? col[i] : MD(rg_col, i);
    for (int t = 0; t < m.ntint; t++)
      if (MD(tint_entry, t) == e && MD(tint_chan, t) == k) v = s.prm[MD(tint_slot, t)] * MD(tint_scale, t);
    c.col[e][k] = v;
  }
  const int head = look[6] != 0.f ? 1 : 0;
  for (int i = tid; i < m.nlight * LIGHT_W; i += nthreads)
    c.light[head + i / LIGHT_W][i % LIGHT_W] = light ? light[i] : MD(light, i);
  if (tid == 0) c.nlight = head + m.nlight;
}

// castshadow of the model's own lights (behind the headlight's slot): slot 21 = 1, MuJoCo's default --
// no Adroit XML sets the attribute, and the model table, whose bytes are pinned, does not carry it.
// Only the kernels that cast shadows read the slot; a per-env light record brings its own.
AW_DEV void render_castshadow(const DModel& m, RColors& c, const float* look, int tid) {
  if (tid < m.nlight) c.light[(look[6] != 0.f ? 1 : 0) + tid][21] = 1.f;
}

// the headlight (light 0 when look switches it on): a point light at the camera, no cone, no
// attenuation
AW_DEV void render_headlight(RColors& c, const float* cam, const float* look, int tid) {
  if (look[6] != 0.f && tid == 0) {
    float* q = c.light[0];
    for (int k = 0; k < LIGHT_W; k++) q[k] = 0.f;
    for (int k = 0; k < 3; k++) { q[k] = cam[k]; q[6 + k] = look[3]; q[9 + k] = look[4]; q[12 + k] = look[5]; }
    q[15] = 1.f;
    q[18] = -2.f;
  }
}

// per-env colour table and light list of one camera
AW_DEV void render_colors(const DModel& m, const Env& s, RColors& c, const float* cam, const float* look, int tid,
                          int nthreads) {
  render_colors_env(m, s, c, look, tid, nthreads);
  render_headlight(c, cam, look, tid);
}

// world camera record of a view given in the frame of a body (s.xpos / s.xquat from
// stage_kinematics): position xpos[b] + rot(xquat[b], pos), the three axes rotated by xquat[b],
// the pixel map and zfar copied; body 0 (the world): the record as it is, no arithmetic
AW_DEV void compose_view(const Env& s, const float* rec, int body, float* cam, int tid) {
  if (tid < 4) {   // position, forward, up, right
    float v[3], r[3];
    copy3(v, rec + 3 * tid);
    copy3(r, v);
    if (body > 0) {
      rotvq(r, v, s.xquat[body]);
      if (tid == 0) add3(r, r, s.xpos[body]);
    }
    copy3(cam + 3 * tid, r);
  } else if (tid < 9) {   // u0, du, v0, dv, zfar
    cam[8 + tid] = rec[8 + tid];
  }
}

// outward normal at the point lp of a primitive's surface (entry frame)
AW_DEV void prim_normal(int type, const float* size, const float* lp, float* n) {
  n[0] = 0.f; n[1] = 0.f; n[2] = 1.f;                                  // plane
  if (type == GEOM_SPHERE) copy3(n, lp);
  else if (type == GEOM_CAPSULE) {                                     // radial from the nearest axis point
    n[0] = lp[0]; n[1] = lp[1]; n[2] = lp[2] - fminf(fmaxf(lp[2], -size[1]), size[1]);
  } else if (type == GEOM_CYLINDER) {                                  // the surface the point lies on: side or cap
    const float side = fabsf(sqrtf(lp[0] * lp[0] + lp[1] * lp[1]) - size[0]), cap = fabsf(fabsf(lp[2]) - size[1]);
    if (side <= cap) { n[0] = lp[0]; n[1] = lp[1]; n[2] = 0.f; }
    else n[2] = lp[2];
  } else if (type == GEOM_BOX) {                                       // the slab the point lies on
    float e[3];
    for (int k = 0; k < 3; k++) e[k] = fabsf(fabsf(lp[k]) - size[k]);
    const int ax = e[0] <= e[1] && e[0] <= e[2] ? 0 : (e[1] <= e[2] ? 1 : 2);
    for (int k = 0; k < 3; k++) n[k] = k == ax ? lp[k] : 0.f;
  }
  normalize3(n);
}

// x^e for shading exponents: 0 for x <= 0
AW_DEV float shade_pow(float x, float e) { return x > 0.f ? exp2f(e * log2f(x)) : 0.f; }

// Cast shadows (aw_set_appearance, shadows 1): whether a primitive geom of `mask` -- entries [0, ng),
// sites never occlude -- crosses the ray o + t l (l unit) at 0 < t < tmax.  Any hit ends the search.
// Per occluder a conservative bounding-sphere test against the segment (the radius padded against
// the rounding of the test itself; planes, rbound 0: none) comes before the exact crossing, so the
// answer is the exhaustive loop's as long as mask holds every true occluder (RShadow below; all
// ones: exhaustive).
constexpr float SHADOW_EPS = 1.0e-4f;   // the origin's lift off the surface, and the segment's end before the light
AW_DEV float shadow_rb(float rb) { return 1.001f * rb + 1.0e-6f; }
AW_DEV bool occluded(const RGeoms& r, unsigned long long mask, const float* o, const float* l, float tmax) {
  // The lanes' masks differ, but the loop is the wave's: each round takes the lowest candidate of
  // the first lane that has one left (ballot + readlane: uniform among the lanes that are here,
  // whatever branch they came through), and the lanes that hold it test it.  So every round works
  // on one entry -- one primitive type, one broadcast LDS address -- instead of 64 different ones.
  bool hit = false;
  for (;;) {
    const unsigned long long live = __ballot(mask != 0ull);
    if (!live) break;
    const int src = __builtin_ctzll(live);
    const unsigned long long m = (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)mask, src) |
                                 (unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)(unsigned)(mask >> 32), src) << 32;
    const int g = __builtin_ctzll(m);
    const bool mine = ((mask >> g) & 1ull) != 0ull;
    mask &= ~(1ull << g);
    if (!mine) continue;
    const float rb = r.rb[g];
    if (rb > 0.f) {
      float oc[3];
      sub3(oc, r.pos[g], o);
      const float tc = dot3(oc, l), rr = shadow_rb(rb);
      if (dot3(oc, oc) - tc * tc > rr * rr || tc + rr < 0.f || tc - rr > tmax) continue;
    }
    const float t = ray_prim(r.pos[g], r.mat[g], r.size[g], r.type[g], o, l);
    if (t > 0.f && t < tmax) { hit = true; mask = 0ull; }   // any hit ends this lane's search
  }
  return hit;
}

// The occluders that can lie between a point and a positional light, looked up instead of searched:
// per casting light a SHADOW_GRID x SHADOW_GRID grid over the light's view of the scene (gnomonic
// coordinates x = u.e1 / u.m0, y = u.e2 / u.m0 of a direction u from the light, |x|, |y| < T, about
// the axis m0 towards the centroid of the occluders' centres), each cell holding the mask of the
// occluders whose cone of directions from the light (axis: centre - light, half angle asin(rbound /
// distance), the radius padded as in `occluded`) meets the cell's bounding cone.  A point's shadow
// ray runs along the direction light -> point, so every geom it can cross is in the mask of that
// direction's cell: a superset of the true occluders, and `occluded` makes the exact decision.
// `always` holds what has no cone -- planes (rbound 0) and geoms that reach the light's own plane or
// lie too far off the axis for the grid (tan > SHADOW_TMAX) -- and is part of every cell; a
// direction off the grid can meet nothing else.  T is fitted to the gridded cones, so the cells are
// as fine as the scene allows: a cell is about 15 cm across at the Adroit table.  Lights that do
// not cast, directional lights and degenerate frames have on == 0: the exhaustive mask.
// The poses are the env's and no camera enters, but the grid is rebuilt per view with the pixel
// boxes (render_geoms fills the poses there); it costs a few microseconds per launch.
constexpr int SHADOW_GRID = 16;
constexpr float SHADOW_TMAX = 2.0f;
struct RShadow {
  unsigned long long cell[MAXLIGHT + 1][SHADOW_GRID * SHADOW_GRID];
  unsigned long long always[MAXLIGHT + 1];
  float fr[MAXLIGHT + 1][16];   // light pos, m0, e1, e2, T, cells per unit, on
};

// thread L < nlight: the frame and the extent of light L's grid
AW_DEV void shadow_frames(const RGeoms& r, const RColors& c, RShadow& sh, int ng, int tid) {
  if (tid >= c.nlight) return;
  const float* q = c.light[tid];
  float* f = sh.fr[tid];
  f[14] = 0.f;
  sh.always[tid] = ~0ull;
  if (q[21] == 0.f || q[20] != 0.f) return;
  float mean[3] = {0.f, 0.f, 0.f}, cnt = 0.f;
  for (int g = 0; g < ng; g++)
    if (r.rb[g] > 0.f) { add3(mean, mean, r.pos[g]); cnt += 1.f; }
  if (cnt == 0.f) return;
  float m0[3], e1[3], e2[3];
  for (int k = 0; k < 3; k++) m0[k] = mean[k] / cnt - q[k];
  if (!(normalize3(m0) > 1.0e-6f)) return;
  const float ax[3] = {fabsf(m0[0]) < 0.6f ? 1.f : 0.f, fabsf(m0[0]) < 0.6f ? 0.f : 1.f, 0.f};
  cross3(e1, m0, ax);
  normalize3(e1);
  cross3(e2, m0, e1);
  unsigned long long always = 0ull;
  float T = 0.f;
  for (int g = 0; g < ng; g++) {
    const float rr = shadow_rb(r.rb[g]);
    float a[3];
    sub3(a, r.pos[g], q);
    const float z = dot3(a, m0), D = norm3(a);
    float tn = 3.0e38f;                                   // tan(angle off the axis + the cone's half angle)
    if (r.rb[g] > 0.f && z > rr) {
      const float ca = z / D, sn = rr / D;
      const float ta = sqrtf(fmaxf(1.f - ca * ca, 0.f)) / ca, tt = sn / sqrtf(fmaxf(1.f - sn * sn, 1.0e-12f));
      if (1.f - ta * tt > 0.05f) tn = (ta + tt) / (1.f - ta * tt);
    }
    if (tn < SHADOW_TMAX) T = fmaxf(T, tn);
    else always |= 1ull << g;
  }
  T = 1.001f * T + 1.0e-4f;
  for (int k = 0; k < 3; k++) { f[k] = q[k]; f[3 + k] = m0[k]; f[6 + k] = e1[k]; f[9 + k] = e2[k]; }
  f[12] = T;
  f[13] = (float)SHADOW_GRID / (2.f * T);
  sh.always[tid] = always;
  f[14] = T < SHADOW_TMAX + 1.f ? 1.f : 0.f;              // (a NaN record: off)
}

// one thread per cell: the cell's mask for every light whose grid is on
AW_DEV void shadow_cells(const RGeoms& r, const RColors& c, RShadow& sh, int ng, int tid0, int nthreads) {
  for (int tid = tid0; tid < SHADOW_GRID * SHADOW_GRID; tid += nthreads)
  for (int L = 0; L < c.nlight; L++) {
    const float* f = sh.fr[L];
    if (f[14] == 0.f) continue;
    const float T = f[12], w = 2.f * T / (float)SHADOW_GRID;
    const float x0 = -T + w * (float)(tid % SHADOW_GRID), y0 = -T + w * (float)(tid / SHADOW_GRID);
    float cd[3], cphi = 1.f;
    for (int k = 0; k < 3; k++) cd[k] = f[3 + k] + (x0 + 0.5f * w) * f[6 + k] + (y0 + 0.5f * w) * f[9 + k];
    normalize3(cd);
    for (int q = 0; q < 4; q++) {
      float v[3];
      for (int k = 0; k < 3; k++) v[k] = f[3 + k] + (x0 + (q & 1 ? w : 0.f)) * f[6 + k] + (y0 + (q & 2 ? w : 0.f)) * f[9 + k];
      normalize3(v);
      cphi = fminf(cphi, dot3(v, cd));
    }
    const float sphi = sqrtf(fmaxf(1.f - cphi * cphi, 0.f));
    const unsigned long long always = sh.always[L];
    unsigned long long mask = always;
    for (int g = 0; g < ng; g++) {
      if ((always >> g) & 1ull) continue;
      float a[3];
      sub3(a, r.pos[g], f);
      const float D = norm3(a), sn = shadow_rb(r.rb[g]) / D;   // < 1: z > rr in shadow_frames
      const float cs = sqrtf(fmaxf(1.f - sn * sn, 0.f));
      if (dot3(a, cd) / D >= cs * cphi - sn * sphi - 1.0e-4f) mask |= 1ull << g;
    }
    sh.cell[L][tid] = mask;
  }
}

// the candidate occluders of light L for a shadow ray that starts at o
AW_DEV unsigned long long shadow_mask(const RShadow& sh, int L, const float* o) {
  const float* f = sh.fr[L];
  if (f[14] == 0.f) return ~0ull;
  float u[3];
  sub3(u, o, f);
  const float z = dot3(u, f + 3), T = f[12];
  if (z > 0.f) {
    const float x = dot3(u, f + 6) / z, y = dot3(u, f + 9) / z;
    if (fabsf(x) < T && fabsf(y) < T) {
      const int ix = min(max((int)((x + T) * f[13]), 0), SHADOW_GRID - 1);
      const int iy = min(max((int)((y + T) * f[13]), 0), SHADOW_GRID - 1);
      return sh.cell[L][iy * SHADOW_GRID + ix];
    }
  }
  return sh.always[L];
}

// the point where the ray cam + t d crosses entry g, evaluated as entry_near does: from an origin
// moved along the ray to two bounding radii in front of the entry's centre, where the quadratic's
// cancellation is about 1e-6 m instead of the 1e-4 m it has from a camera metres away -- which is
// SHADOW_EPS, so a shadow ray started from the coarse point could begin inside the entry it leaves.
// Falls back to the coarse point where the moved origin grazes past.
AW_DEV void shadow_point(const RGeoms& r, int g, const float* cam, const float* d, float t, float* P) {
  const float rb = r.rb[g];
  float s = 0.f, tt = t;
  if (rb > 0.f) {
    float oc[3], o[3];
    sub3(oc, r.pos[g], cam);
    s = fmaxf(dot3(oc, d) - 2.f * rb, 0.f);
    for (int k = 0; k < 3; k++) o[k] = cam[k] + s * d[k];
    const float t2 = ray_prim(r.pos[g], r.mat[g], r.size[g], r.type[g], o, d);
    if (t2 >= 0.f && fabsf(s + t2 - t) < 1.0e-3f) tt = t2; else s = 0.f;
  }
  for (int k = 0; k < 3; k++) P[k] = (cam[k] + s * d[k]) + tt * d[k];
}

// linear rgb of entry g where the ray cam + t d crosses it.  SHADOW: a light with castshadow set
// (slot 21; the headlight's is 0) that faces the surface (n.l > 0) with f > 0 is hidden -- f = 0, its
// ambient term stays -- where `occluded` finds a primitive geom (entries [0, ng)) between the point
// lifted SHADOW_EPS along the facing normal and the light: a positional light up to SHADOW_EPS
// before it, a directional one without end.  sh: the light's grid of candidate occluders.
template <bool SHADOW = false>
AW_DEV void shade(const RGeoms& r, const RColors& c, int g, const float* cam, const float* d, float t, float* rgb,
                  int ng = 0, const RShadow* sh = nullptr) {
  float P[3], dif[3], lp[3], nl[3], n[3];
  for (int k = 0; k < 3; k++) P[k] = cam[k] + t * d[k];
  sub3(dif, P, r.pos[g]);
  mulmtv3(lp, r.mat[g], dif);
  prim_normal(r.type[g], r.size[g], lp, nl);
  mulmv3(n, r.mat[g], nl);
  if (dot3(n, d) > 0.f) scl3(n, n, -1.f);              // face the ray origin
  const float* a = c.col[g];
  const float spec = a[4], shin = a[5];
  for (int k = 0; k < 3; k++) rgb[k] = a[6] * a[k];
  for (int L = 0; L < c.nlight; L++) {
    const float* q = c.light[L];
    float l[3], f = 1.f;
    float tmax = 3.0e38f;
    if (q[20] != 0.f) scl3(l, q + 3, -1.f);
    else {
      sub3(l, q, P);
      const float dist = normalize3(l);
      tmax = dist - SHADOW_EPS;
      f = 1.f / (q[15] + dist * (q[16] + dist * q[17]));
      if (q[18] > -1.5f) {
        const float cs = -dot3(l, q + 3);
        f = cs >= q[18] ? f * shade_pow(cs, q[19]) : 0.f;
      }
    }
    const float ndl = dot3(n, l);
    if constexpr (SHADOW) {
      if (q[21] != 0.f && ndl > 0.f && f > 0.f) {
        float Ps[3];
        shadow_point(r, g, cam, d, t, Ps);
        for (int k = 0; k < 3; k++) Ps[k] += SHADOW_EPS * n[k];
        const unsigned long long geoms = ng < 64 ? (1ull << ng) - 1ull : ~0ull;
        if (occluded(r, shadow_mask(*sh, L, Ps) & geoms, Ps, l, tmax)) f = 0.f;
      }
    }
    float sp = 0.f;
    if (ndl > 0.f) {
      float rv = 0.f;
      for (int k = 0; k < 3; k++) rv -= (2.f * ndl * n[k] - l[k]) * d[k];
      sp = spec * shade_pow(rv, shin);
    }
    const float df = fmaxf(ndl, 0.f);
    for (int k = 0; k < 3; k++) rgb[k] += q[6 + k] * a[k] + f * (q[9 + k] * a[k] * df + q[12 + k] * sp);
  }
}

// colour (and optionally z-depth) of the 64 pixels [p0, p0 + 64) handled by wave `wave`: per
// sample ray the nearest opaque geom (render_span's search), shaded; the MAXSITEHIT nearest
// site crossings in front of it blended over it back to front; ss x ss samples averaged
template <bool SHADOW = false>
AW_DEV void render_span_rgb(const RGeoms& r, RColors& c, int ng, int ns, const float* cam, const float* look, int W,
                            int H, int ss, int p0, int lane, int wave, unsigned char* out, bool dwords,
                            float* depth, const RShadow* sh = nullptr) {
  const int np = W * H;
  const int p = p0 + lane;
  const unsigned long long all = span_entries(r, ng + ns, W, H, p0, lane);
  const unsigned long long gmask = ng < 64 ? all & ((1ull << ng) - 1ull) : all, smask = ng < 64 ? all >> ng : 0ull;
  const int row = p / W, col = p - row * W;
  const float fc = (float)col, fr = (float)row;
  float acc[3] = {0.f, 0.f, 0.f};
  for (int sy = 0; sy < ss; sy++)
    for (int sx = 0; sx < ss; sx++) {
      // sample at the centre of sub-cell (sx, sy) of the pixel (ss 1: the pixel centre itself)
      const float ox = ((float)sx + 0.5f) / (float)ss - 0.5f, oy = ((float)sy + 0.5f) / (float)ss - 0.5f;
      float d[3], rgb[3];
      pixel_ray(cam, fc + ox, fr + oy, d);
      int hit;
      const float best = nearest_hit(r, gmask, cam, d, fc, fr, hit);
      if (depth && p < np) depth[p] = best < 1.0e38f ? best * dot3(d, cam + 3) : cam[16];
      if (hit >= 0) shade<SHADOW>(r, c, hit, cam, d, best, rgb, ng, sh);
      else copy3(rgb, look);
      // the nearest site crossings in front of the opaque one, sorted by t (registers)
      float st[MAXSITEHIT];
      int sg[MAXSITEHIT];
#pragma unroll
      for (int k = 0; k < MAXSITEHIT; k++) { st[k] = 3.0e38f; sg[k] = -1; }
      unsigned long long mk = smask;
      while (mk) {
        const int g = ng + __builtin_ctzll(mk);
        mk &= mk - 1ull;
        float t = entry_hit(r, g, cam, d, fc, fr, best);
        if (t < 0.f || t >= best) continue;
        int e = g;
#pragma unroll
        for (int k = 0; k < MAXSITEHIT; k++)
          if (t < st[k]) { const float tt = st[k]; const int gg = sg[k]; st[k] = t; sg[k] = e; t = tt; e = gg; }
      }
#pragma unroll
      for (int k = MAXSITEHIT - 1; k >= 0; k--)
        if (sg[k] >= 0) {
          float sc[3];
          shade<SHADOW>(r, c, sg[k], cam, d, st[k], sc, ng, sh);
          const float al = c.col[sg[k]][3];
          for (int q = 0; q < 3; q++) rgb[q] = al * sc[q] + (1.f - al) * rgb[q];
        }
      for (int q = 0; q < 3; q++) acc[q] += rgb[q];
    }
  unsigned char px[3];
  const float inv = 1.f / (float)(ss * ss);
  for (int q = 0; q < 3; q++) px[q] = (unsigned char)floorf(255.f * fminf(fmaxf(acc[q] * inv, 0.f), 1.f) + 0.5f);
  if (!dwords) {
    if (p < np)
      for (int q = 0; q < 3; q++) out[(size_t)p * 3 + q] = px[q];
    return;
  }
  // 64 pixels = 192 contiguous bytes: through LDS, then whole dwords from the low lanes (the frame
  // size and base are multiples of 4 bytes, and so is every span's start, 192 p0 / 64)
  unsigned char* stage = reinterpret_cast<unsigned char*>(c.bytes[wave]);
  for (int q = 0; q < 3; q++) stage[3 * lane + q] = px[q];
  wsync();
  const int nd = 3 * min(64, np - p0) / 4;
  if (lane < nd) reinterpret_cast<unsigned*>(out + (size_t)p0 * 3)[lane] = c.bytes[wave][lane];
  wsync();
}

}  // namespace aw
