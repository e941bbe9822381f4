// aw_api.hip -- the C-ABI of the MI355X batched Adroit simulator (include/adroit_wave.h): the
// handle, the host side of every aw_* entry point, and the task-independent kernels.  It
// instantiates no per-task kernel: those come from the task units (aw_kernels.hip), reached through
// the launcher tables task_ops<TASK> / wide_ops<TASK> (aw_handle.h) across the link.
// The model table -> device tables builder is host-only code of its own: aw_model_host.h.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include <memory>
#include <string>
#include <vector>

#include "../../include/adroit_wave.h"
#include "../../include/aw_blob.h"
#include "aw_collide.h"
#include "aw_common.h"
#include "aw_handle.h"
#include "aw_model_host.h"
#include "aw_policy.h"
#include "aw_task.h"

using namespace aw;

// ---------------------------------------------------------------------------------------
// the task-independent kernels
__global__ void __launch_bounds__(64) k_task_eval(DModel m, int n, const float* qpos, const float* qvel,
                                                  const float* xpos, const float* xquat, const float* sxpos,
                                                  const float* touch, float* obs, float* reward, uint8_t* done,
                                                  uint8_t* goal) {
  __shared__ Env s;
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  if (lane < m.nq) { s.qpos[lane] = qpos[(size_t)i * m.nq + lane]; s.qlo[lane] = 0.f; }
  if (lane < m.nv) s.qvel[lane] = qvel[(size_t)i * m.nv + lane];
  for (int k = lane; k < m.nbody * 3; k += 64) (&s.xpos[0][0])[k] = xpos[(size_t)i * m.nbody * 3 + k];
  for (int k = lane; k < m.nbody * 4; k += 64) (&s.xquat[0][0])[k] = xquat[(size_t)i * m.nbody * 4 + k];
  for (int k = lane; k < m.nsite * 3; k += 64) (&s.sxpos[0][0])[k] = sxpos[(size_t)i * m.nsite * 3 + k];
  if (lane == 0) s.touch[0] = touch ? touch[i] : 0.f;
  wsync();
  write_obs(m, s, lane, obs + (size_t)i * m.obs_dim);
  if (lane == 0) {
    float r;
    int dn, gl;
    task_reward(m, s, &r, &dn, &gl);
    reward[i] = r; done[i] = (uint8_t)dn; goal[i] = (uint8_t)gl;
  }
}

// Test hook (aw_collide_test): the narrowphase of one primitive pair per workgroup, given world
// poses -- exact-geometry collider tests against the oracle's colliders.
// Lanes 0..15 call it with the same pair (gl = lane): capsule-box runs on the 16-lane row and MPR
// on lanes 0 and 1 as in the narrowphase, every other collider on lane 0.
AW_DEV void collide_gv(const DModel& m, const GV& a, const GV& b, float margin, Emit& e, int gl) {
  const int lo = a.type, hi = b.type;   // a.type <= b.type
  if (hi == GEOM_BOX && lo == GEOM_CAPSULE) {
    c_capsule_box(a, b, margin, e, gl);
    return;
  }
  if (lo != GEOM_PLANE && (lo == GEOM_CYLINDER || hi == GEOM_CYLINDER)) {   // MPR on lanes 0 and 1
    if (gl > 1) return;
    const GV& g = gl ? b : a;
    mpr::GVdT<double> own;
    for (int k = 0; k < 3; k++) { own.pos[k] = g.pos[k]; own.size[k] = g.size[k]; }
    for (int k = 0; k < 9; k++) own.mat[k] = g.mat[k];
    own.type = g.type;
    c_convex64(m, own, gl, (double)margin, e);
    return;
  }
  if (gl != 0) return;
  if (lo == GEOM_PLANE) {
    if (hi == GEOM_SPHERE) c_plane_sphere(a.pos, a.mat, b.pos, b.size[0], margin, e);
    else if (hi == GEOM_CAPSULE) c_plane_capsule(a, b, margin, e);
    else if (hi == GEOM_CYLINDER) c_plane_cylinder(a, b, margin, e);
    else if (hi == GEOM_BOX) c_plane_box(a, b, margin, e);
  } else if (hi == GEOM_BOX && lo == GEOM_BOX) {
    c_box_box(a, b, margin, e);
  } else if (hi == GEOM_BOX) {
    c_sphere_box_pt(a.pos, a.size[0], b, margin, e);
  } else if (lo == GEOM_SPHERE && hi == GEOM_SPHERE) {
    c_sphere_sphere(a.pos, a.size[0], b.pos, b.size[0], margin, e);
  } else if (lo == GEOM_SPHERE) {
    c_sphere_capsule(a, b, margin, e);
  } else {
    c_capsule_capsule(a, b, margin, e);
  }
}

__global__ void __launch_bounds__(64) k_collide_test(DModel m, int n, const int* types, const float* pos,
                                                     const float* mat, const float* size, const float* margin,
                                                     float* out, int* count, double* out64) {
  __shared__ Env s;
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n) return;
  if (lane == 0) { s.ncon = 0; s.status = 0u; }
  wsync();
  if (lane < 16) {
    GV g[2];
    for (int q = 0; q < 2; q++) {
      g[q].type = types[2 * i + q];
      for (int k = 0; k < 3; k++) { g[q].pos[k] = pos[6 * i + 3 * q + k]; g[q].size[k] = size[6 * i + 3 * q + k]; }
      for (int k = 0; k < 9; k++) g[q].mat[k] = mat[18 * i + 9 * q + k];
    }
    const int f = g[0].type <= g[1].type ? 0 : 1;
    Emit e{&s, 0, 0, out64 ? out64 + (size_t)i * MAXPAIRCON * 7 : nullptr};
    collide_gv(m, g[f], g[1 - f], margin[i], e, lane);
  }
  wsync();
  const int nc = s.ncon < MAXPAIRCON ? s.ncon : MAXPAIRCON;
  if (lane == 0) count[i] = nc;
  if (lane < nc) {
    float* o = out + ((size_t)i * MAXPAIRCON + s.con_key[lane]) * 7;   // emission order
    o[0] = s.con_dist[lane];
    for (int k = 0; k < 3; k++) { o[1 + k] = s.con_pos[lane][k]; o[4 + k] = s.con_nrm[lane][k]; }
  }
}

// Test hook (aw_midphase_test): the conservative midphase cull of one model pair per workgroup, on
// given world poses and sizes of its two geoms.  Lane 0 stages them where the narrowphase reads
// them (gxpos, gxquat, gsize of the pair's geoms in a shared Env) and calls the *_may_touch of
// the pair's class as it stands; classes 0 and 1 have no cull (keep = 1).  info: keep, g1, g2,
// class, type of g1, type of g2 (keep = -1, nothing else written: pair id out of range).
__global__ void __launch_bounds__(64) k_midphase_test(DModel m, int n, const int* pair, const float* pos,
                                                      const float* quat, const float* size, int* info,
                                                      float* margin) {
  __shared__ Env s;
  const int i = blockIdx.x, lane = threadIdx.x;
  if (i >= n || lane != 0) return;
  const int p = pair[i];
  if ((unsigned)p >= (unsigned)m.npairall) { info[6 * i] = -1; return; }
  const int g[2] = {MD(cp_g1, p), MD(cp_g2, p)};
  for (int q = 0; q < 2; q++) {
    for (int k = 0; k < 3; k++) { s.gxpos[g[q]][k] = pos[6 * i + 3 * q + k]; s.gsize[g[q]][k] = size[6 * i + 3 * q + k]; }
    for (int k = 0; k < 4; k++) s.gxquat[g[q]][k] = quat[8 * i + 4 * q + k];
  }
  const int cls = MD(cp_class, p);
  bool keep = true;
  if (cls == 2) keep = capbox_may_touch(m, s, p);
  else if (cls == 3) keep = boxbox_may_touch(m, s, p);
  else if (cls == 4) keep = mpr_may_touch(m, s, p);
  int* o = info + 6 * i;
  o[0] = keep ? 1 : 0; o[1] = g[0]; o[2] = g[1]; o[3] = cls;
  o[4] = MD(geom_type, g[0]); o[5] = MD(geom_type, g[1]);
  margin[i] = MD(cp_margin, p);
}

__global__ void k_random_actions(int n, int nu, uint64_t seed, uint64_t step, uint64_t env_offset, float* out) {
  int env = blockIdx.x * blockDim.x + threadIdx.x;
  if (env >= n) return;
  const uint32_t genv = (uint32_t)(env_offset + (uint64_t)env);   // global env id (shard offset)
  for (int blk = 0; blk * 4 < nu; blk++) {
    uint32_t c[4] = {genv, (uint32_t)step, (uint32_t)(step >> 32), (uint32_t)blk};
    philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
    for (int k = 0; k < 4 && blk * 4 + k < nu; k++) out[(size_t)env * nu + blk * 4 + k] = 2.f * u01(c[k]) - 1.f;
  }
}

// Appearance sampler (aw_appearance_sample): one thread per float of one env's record vector
// [col | light | look] (F = nc + nl + AW_LOOK_FLOATS floats; row0 + blockIdx.y: the row).  Float i is
// lo[i] + (hi[i] - lo[i]) u01(x), x = word i & 3 of philox({genv, draw, 0xA99E, i >> 2}, seed).  The
// flag slots (light 18, 20, 21; look 6) are lo's.  A light's dir is renormalised: the thread of
// a dir slot draws all three components and divides its own by their length, in fp64 (correctly
// rounded whatever the fp32 divide / sqrt flags are, so the host restates it bit for bit); a zero
// vector stays.  env_ids (nullptr: row r is env r): an id outside [0, n) is skipped; a null output
// is not written.  Every store index is the env's own row.
AW_DEV float appearance_draw(const float* lo, const float* hi, int i, uint32_t genv, uint64_t seed, uint64_t draw) {
  uint32_t c[4] = {genv, (uint32_t)draw, 0xA99Eu, (uint32_t)(i >> 2)};
  philox(c, (uint32_t)seed, (uint32_t)(seed >> 32));
  return lo[i] + (hi[i] - lo[i]) * u01(c[i & 3]);
}
__global__ void __launch_bounds__(256) k_appearance(int n, int nc, int nl, const float* __restrict__ lo,
                                                    const float* __restrict__ hi, const int* __restrict__ env_ids,
                                                    int row0, uint64_t env_offset, uint64_t seed, uint64_t draw, float* col,
                                                    float* light, float* look) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x, F = nc + nl + AW_LOOK_FLOATS;
  const int row = row0 + (int)blockIdx.y;
  const int env = env_ids ? env_ids[row] : row;
  if (i >= F || (unsigned)env >= (unsigned)n) return;
  const uint32_t genv = (uint32_t)(env_offset + (uint64_t)env);
  float v = appearance_draw(lo, hi, i, genv, seed, draw);
  if (i < nc) {
    if (col) col[(size_t)env * nc + i] = v;
  } else if (i < nc + nl) {
    const int k = (i - nc) % LIGHT_W;
    if (k == 18 || k == 20 || k == 21) v = lo[i];
    if (k >= 3 && k < 6) {
      const int i0 = i - (k - 3);
      double d[3], nn = 0.0;
      for (int q = 0; q < 3; q++) { d[q] = (double)appearance_draw(lo, hi, i0 + q, genv, seed, draw); nn += d[q] * d[q]; }
      if (nn > 0.0) v = (float)(d[k - 3] / sqrt(nn));
    }
    if (light) light[(size_t)env * nl + (i - nc)] = v;
  } else {
    if (i - nc - nl == 6) v = lo[i];
    if (look) look[(size_t)env * AW_LOOK_FLOATS + (i - nc - nl)] = v;
  }
}

// The state rows of selected envs (aw_get_state_ids; aw_clone_envs' read pass): one wave per output
// row, four per workgroup; row k receives env env_ids[k], an id outside [0, n) leaves it untouched.
// The id is wave-uniform (readfirstlane), so the row bases are scalar.  Any output may be null; the
// episode outputs are aw_clone_envs' (the running episode's counters).
__global__ void __launch_bounds__(256) k_get_state_ids(DState st, int n, int nq, int nv, int nparam,
                                                       const int* __restrict__ env_ids, int n_sel, float* qpos,
                                                       float* qvel, float* warm, float* params, int* ep_len,
                                                       float* ep_ret, int* ep_goal) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (k >= n_sel) return;
  const int env = __builtin_amdgcn_readfirstlane(env_ids[k]);
  if ((unsigned)env >= (unsigned)n) return;
  for (int i = lane; i < nq; i += 64)
    if (qpos) qpos[(size_t)k * nq + i] = st.qpos[(size_t)env * nq + i];
  for (int i = lane; i < nv; i += 64) {
    if (qvel) qvel[(size_t)k * nv + i] = st.qvel[(size_t)env * nv + i];
    if (warm) warm[(size_t)k * nv + i] = st.warm[(size_t)env * nv + i];
  }
  for (int i = lane; i < nparam; i += 64)
    if (params) params[(size_t)k * nparam + i] = st.params[(size_t)env * nparam + i];
  if (lane == 0) {
    if (ep_len) ep_len[k] = st.ep_len[env];
    if (ep_ret) ep_ret[k] = st.ep_ret[env];
    if (ep_goal) ep_goal[k] = st.ep_goal[env];
  }
}

// Farthest-point sampling (aw_cloud_fps): one workgroup of T threads per row, instantiated per
// capacity class CAP >= cap so that a small cloud does not claim a large cloud's LDS.  The row's
// c = min(count, cap) candidates are staged in LDS once (the selected point of every iteration is
// read from there by all threads, one broadcast address); thread t owns the kc = ceil(c / T) <= K =
// CAP / T consecutive candidates [t kc, (t + 1) kc) -- the work follows the row's count, not its
// capacity -- and keeps their coordinates and minimum squared distances in registers.  Owning
// consecutive candidates makes the lowest index of a tie the lowest j within a thread, then the
// lowest lane, then the lowest wave, so the argmax carries no index through the reductions: per
// iteration every thread folds the last selection into its kc minima and takes their maximum
// (strict >: the lowest j), wave_max (DPP) gives the wave's maximum, the lowest lane of the ballot
// that holds it the wave's index; lane 0 leaves both in LDS, and behind the iteration's one barrier
// every wave repeats the same step over the NW wave results (lane w reads wave w's pair, the index
// comes back through readlane: one LDS round trip).  The wave results are double buffered by
// iteration parity, as k_cloud's counts are.  Slots past c (minimum -1, below every distance)
// never win while c >= 1.  The distance is (dx dx + dy dy) + dz dz in individually rounded fp32
// operations, so the choice is reproducible on the host bit for bit (the library flushes fp32
// denormals: squared distances below 1.2e-38 count as 0).  T is small where several rows fit a
// CU's LDS (their latency chains overlap) and 1024 where one row fills it.
template <int CAP, int T>
__global__ void __launch_bounds__(T) k_fps(int cap, int P, const float* __restrict__ xyz, const int* __restrict__ count,
                                           float* __restrict__ out_xyz, int* __restrict__ out_idx) {
  constexpr int K = CAP / T, NW = T / 64;
  static_assert(CAP % T == 0 && T % 64 == 0 && NW <= 64, "k_fps: whole waves, whole candidates per thread");
  __shared__ float pts[CAP * 3];
  __shared__ int sel[AW_FPS_MAXPOINTS];
  __shared__ float wv[2][NW];
  __shared__ int wi[2][NW];
  const int row = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int c = min(max(count[row], 0), cap);   // uniform over the block, and so is every barrier below
  const float* src = xyz + (size_t)row * cap * 3;
  for (int i = tid; i < 3 * c; i += T) pts[i] = src[i];
  if (tid == 0) sel[0] = 0;
  __syncthreads();
  const int kc = (c + T - 1) / T;   // <= K, as c <= cap <= CAP
  float px[K], py[K], pz[K], md[K];
#pragma unroll
  for (int j = 0; j < K; j++) {
    const int i = tid * kc + j;
    const bool own = j < kc && i < c;
    px[j] = own ? pts[3 * i] : 0.f;
    py[j] = own ? pts[3 * i + 1] : 0.f;
    pz[j] = own ? pts[3 * i + 2] : 0.f;
    md[j] = own ? __builtin_inff() : -1.f;
  }
  const int m = min(P, c);
  int cur = 0;
  for (int k = 1; k < m; k++) {
    const float sx = pts[3 * cur], sy = pts[3 * cur + 1], sz = pts[3 * cur + 2];
    float bv = -2.f;
    int bi = 0;
#pragma unroll
    for (int j = 0; j < K; j++) {
      if (j < kc) {   // uniform over the block
        const float dx = __fsub_rn(px[j], sx), dy = __fsub_rn(py[j], sy), dz = __fsub_rn(pz[j], sz);
        const float d = __fadd_rn(__fadd_rn(__fmul_rn(dx, dx), __fmul_rn(dy, dy)), __fmul_rn(dz, dz));
        md[j] = fminf(md[j], d);
        if (md[j] > bv) { bv = md[j]; bi = tid * kc + j; }
      }
    }
    const float wm = wave_max(bv);
    const unsigned long long eq = __ballot(bv == wm);
    const int widx = rlane_i(bi, eq ? __builtin_ctzll(eq) : 0);
    const int b = k & 1;
    if (lane == 0) { wv[b][wave] = wm; wi[b][wave] = widx; }
    __syncthreads();
    const float cv = lane < NW ? wv[b][lane] : -2.f;
    const int ci = lane < NW ? wi[b][lane] : 0;
    const float cm = wave_max(cv);
    const unsigned long long ceq = __ballot(lane < NW && cv == cm);
    cur = rlane_i(ci, ceq ? __builtin_ctzll(ceq) : 0);
    if (tid == 0) sel[k] = cur;
  }
  __syncthreads();
  // selections past c repeat cyclically; an empty row is zeros and index -1
  for (int j = tid; j < P; j += T) {
    const int i = c > 0 ? sel[j % c] : -1;
    if (out_idx) out_idx[(size_t)row * P + j] = i;
    for (int q = 0; q < 3; q++) out_xyz[((size_t)row * P + j) * 3 + q] = i >= 0 ? pts[3 * i + q] : 0.f;
  }
}

// ---------------------------------------------------------------------------------------
// host side
namespace {
thread_local std::string g_err;
int fail(int code, const std::string& msg) { g_err = msg; return code; }
#define HIPCHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) return fail(AW_EHIP, std::string(#x) + ": " + hipGetErrorString(e_)); } while (0)

}  // namespace

static int upload_header(aw_handle* h) {
  HIPCHK(hipMemcpy(h->dmhdr, &h->m, sizeof(DModel), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((DModel*)h->dmhdr + 1, &h->st, sizeof(DState), hipMemcpyHostToDevice));
  DModel mw = h->m;
  mw.jspill = h->jspill_wide;
  mw.mfac = h->mfac_wide;
  HIPCHK(hipMemcpy(h->dmhdr_wide, &mw, sizeof(DModel), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy((DModel*)h->dmhdr_wide + 1, &h->st, sizeof(DState), hipMemcpyHostToDevice));
  return AW_OK;
}

// The launcher tables of a task kind (kernels are instantiated per task: the dof tree of aw_trees.h
// is a template argument); nullptr: not a task, or (-DAW_ONLY_TASK: a library that holds one task,
// tools/stage_profile.py) not in this build
static const TaskOps* task_ops_of(int kind) {
  switch (kind) {
#ifdef AW_ONLY_TASK
    case AW_ONLY_TASK: return task_ops<AW_ONLY_TASK>();
#else
    case 0: return task_ops<0>();
    case 1: return task_ops<1>();
    case 2: return task_ops<2>();
    case 3: return task_ops<3>();
#endif
    default: return nullptr;
  }
}
static const WideOps* wide_ops_of(int kind) {
  switch (kind) {
#ifdef AW_ONLY_TASK
    case AW_ONLY_TASK: return wide_ops<AW_ONLY_TASK>();
#else
    case 0: return wide_ops<0>();
    case 1: return wide_ops<1>();
    case 2: return wide_ops<2>();
    case 3: return wide_ops<3>();
#endif
    default: return nullptr;
  }
}

// persistent grid of the k_step instantiation the handle currently selects
static void update_slots(aw_handle* h) {
  h->slots = h->grid_env > 0 ? h->grid_env : h->grid_env == 0 ? (1 << 30) : h->ops->slots(h->device);
}

// device-to-device copies of per-env arrays on one stream, in list order; a field whose caller-side
// end is null is skipped (the getters and setters of the state, episode and status arrays)
struct CopyField {
  void* dst;
  const void* src;
  size_t bytes;
};
static int copy_fields(std::initializer_list<CopyField> fields, void* stream) {
  for (const CopyField& f : fields)
    if (f.dst && f.src) HIPCHK(hipMemcpyAsync(f.dst, f.src, f.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return AW_OK;
}

// The views of one render launch (fn: the entry point, for the message): every body must be a body
// of the model; the records are host arrays and travel as a kernel argument.
static int fill_views(const aw_handle* h, const char* fn, const aw_view* views, int nviews, ViewsRec& r) {
  r = {};
  for (int v = 0; v < nviews; v++) {
    if (views[v].body < 0 || views[v].body >= h->m.nbody)
      return fail(AW_EINVAL, std::string(fn) + ": a view's body is not a body of the model");
    memcpy(r.c[v], views[v].rec, sizeof(r.c[v]));
    r.body[v] = views[v].body;
  }
  return AW_OK;
}
// the caller's look record, or the default one
static LookRec look_rec(const float* look) {
  LookRec l = {{0.f, 0.f, 0.f, 0.1f, 0.4f, 0.5f, 1.f}};
  if (look) memcpy(l.c, look, sizeof(l.c));
  return l;
}

extern "C" {

const char* aw_last_error(void) { return g_err.c_str(); }

static void free_handle(aw_handle* h) {
  if (!h) return;
  if (h->dmodel) (void)hipFree(h->dmodel);
  if (h->dmhdr) (void)hipFree(h->dmhdr);
  if (h->dstate) (void)hipFree(h->dstate);
  if (h->m.jspill) (void)hipFree(h->m.jspill);
  if (h->m.mfac) (void)hipFree(h->m.mfac);
  if (h->next_env) (void)hipFree(h->next_env);
  if (h->dmhdr_wide) (void)hipFree(h->dmhdr_wide);
  if (h->jspill_wide) (void)hipFree(h->jspill_wide);
  if (h->mfac_wide) (void)hipFree(h->mfac_wide);
  if (h->dsens) (void)hipFree(h->dsens);
  if (h->ddata) (void)hipFree(h->ddata);
  if (h->sensordata) (void)hipFree(h->sensordata);
  if (h->clone_scratch) (void)hipFree(h->clone_scratch);
  if (h->rays) (void)hipFree(h->rays);
  if (h->app_bounds) (void)hipFree(h->app_bounds);
  delete h;
}

// carve the per-env state arrays out of one allocation (each 256-byte aligned)
static size_t layout_state(aw_handle* h, char* base) {
  size_t N = (size_t)h->nenv, nq = h->m.nq, nv = h->m.nv, np = std::max(h->m.nparam, 1);
  uintptr_t p = (uintptr_t)base;   // base == nullptr: dry run, only the size is used
  auto take = [&](size_t b) { uintptr_t r = p; p += (b + 255) & ~size_t(255); return (char*)r; };
  DState& st = h->st;
  st.qpos = (float*)take(N * nq * 4); st.qvel = (float*)take(N * nv * 4); st.warm = (float*)take(N * nv * 4);
  st.params = (float*)take(N * np * 4); st.ep_len = (int*)take(N * 4); st.ep_ret = (float*)take(N * 4);
  st.ep_goal = (int*)take(N * 4); st.episode = (int*)take(N * 4); st.status = (unsigned*)take(N * 4);
  st.last_ret = (float*)take(N * 4); st.last_goal = (int*)take(N * 4); st.last_len = (int*)take(N * 4);
  st.status_acc = (unsigned*)take(N * 4); st.sum_ret = (float*)take(N * 4); st.n_success = (int*)take(N * 4);
  return (size_t)(p - (uintptr_t)base);
}

int aw_create(const void* blob, size_t nbytes, int n_envs, int device, aw_handle** out) {
  if (!blob || !out || n_envs <= 0) return fail(AW_EINVAL, "aw_create: bad arguments");
  *out = nullptr;
  Blob B{blob, nbytes};
  std::unique_ptr<aw_handle, void (*)(aw_handle*)> h(new aw_handle(), free_handle);
  h->device = device;
  h->nenv = n_envs;
  std::unique_ptr<MData> md(new MData());   // value-initialised: zero
  SensTab sens = {};
  DataTab data = {};
  std::string err;
  if (int rc = build_model(B, h->m, *md, sens, data, err)) return fail(rc, err);
  h->NV = h->m.nv;
  h->nsensor = sens.n;
  if (int rc = check_tree(B, h->m.task_kind, *md, err)) return fail(rc, err);
  std::vector<float> def;   // default params of every env
  if (int rc = param_defaults(B, h->m.nparam, def, err)) return fail(rc, err);
  h->ops = task_ops_of(h->m.task_kind);
  h->wide = wide_ops_of(h->m.task_kind);
  if (!h->ops || !h->wide) return fail(AW_EUNSUPPORTED, "task not instantiated in this build");
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipMalloc(&h->dmodel, sizeof(MData)));
  HIPCHK(hipMemcpy(h->dmodel, md.get(), sizeof(MData), hipMemcpyHostToDevice));
  h->m.d = (const MData*)h->dmodel;
  // fast tier: one spill block per workgroup of k_reset / k_set_state (one per env)
  HIPCHK(hipMalloc((void**)&h->m.jspill, (size_t)n_envs * JSPILL_FAST * sizeof(float)));
  HIPCHK(hipMalloc((void**)&h->m.mfac, (size_t)n_envs * MFAC * sizeof(float)));
  HIPCHK(hipMalloc(&h->dmhdr, sizeof(DModel) + sizeof(DState)));
  const size_t nq = 10 + 3 * (size_t)n_envs;   // + per-env costs and the claim permutation (k_order)
  HIPCHK(hipMalloc((void**)&h->next_env, nq * sizeof(int)));
  HIPCHK(hipMemset(h->next_env, 0, nq * sizeof(int)));
  // wide tier: its persistent grid and one spill block per wide workgroup
  h->wide_grid = std::min(n_envs, h->wide->slots(device));
  HIPCHK(hipMalloc((void**)&h->jspill_wide, (size_t)h->wide_grid * JSPILL_WIDE * sizeof(float)));
  HIPCHK(hipMalloc((void**)&h->mfac_wide, (size_t)h->wide_grid * MFAC * sizeof(float)));
  HIPCHK(hipMalloc(&h->dmhdr_wide, sizeof(DModel) + sizeof(DState)));
  const size_t bytes = layout_state(h.get(), nullptr);   // dry run: sizes only
  HIPCHK(hipMalloc(&h->dstate, bytes));
  HIPCHK(hipMemset(h->dstate, 0, bytes));
  layout_state(h.get(), (char*)h->dstate);
  size_t N = (size_t)n_envs, np = std::max(h->m.nparam, 1);
  std::vector<float> prm(N * np, 0.f);
  for (size_t e = 0; e < N; e++)
    for (int k = 0; k < h->m.nparam; k++) prm[e * np + k] = def[k];
  HIPCHK(hipMemcpy(h->st.params, prm.data(), prm.size() * 4, hipMemcpyHostToDevice));
  if (int rc2 = upload_header(h.get())) return rc2;
  // the sensor block last, so that every block above sits where it sat without it
  HIPCHK(hipMalloc(&h->dsens, sizeof(SensTab)));
  HIPCHK(hipMemcpy(h->dsens, &sens, sizeof(SensTab), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(((MData*)h->dmodel)->sens, &h->dsens, sizeof(void*), hipMemcpyHostToDevice));
  HIPCHK(hipMalloc(&h->ddata, sizeof(DataTab)));   // and the mjData output block after it (aw_set_data)
  HIPCHK(hipMemcpy(h->ddata, &data, sizeof(DataTab), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(((MData*)h->dmodel)->data, &h->ddata, sizeof(void*), hipMemcpyHostToDevice));
  if (const char* e = getenv("AW_STEP_GRID")) h->grid_env = std::max(atoi(e), 0);
  update_slots(h.get());
  *out = h.release();
  return AW_OK;
}

int aw_destroy(aw_handle* h) {
  if (!h) return AW_OK;
  (void)hipSetDevice(h->device);
  free_handle(h);
  return AW_OK;
}

int aw_dims(const aw_handle* h, int* d) {
  if (!h || !d) return fail(AW_EINVAL, "aw_dims: null");
  const DModel& m = h->m;
  int v[AW_NDIMS] = {m.nq, m.nv, m.nu, m.obs_dim, m.nparam, m.frame_skip, m.horizon, m.task_kind, h->nenv,
                     m.nbody, m.nsite, m.ngeom, m.npairall, NCONMAX, NJMAX, WIDE_MAXDENSE, std::min(h->slots, h->nenv),
                     FAST_MAXCON, 64 * FAST_NRL, fast_maxdense_of(m.task_kind), h->wide_grid};
  memcpy(d, v, sizeof(v));
  return AW_OK;
}

int aw_set_option(aw_handle* h, int disableflags, int iterations, int noslip_iterations) {
  if (!h) return fail(AW_EINVAL, "aw_set_option: null");
  if (disableflags >= 0 && (disableflags & ~0xFFFF))
    return fail(AW_EUNSUPPORTED, "aw_set_option: only MuJoCo's disable bits 0..15 (the MPR collider always runs in fp64)");
  if (disableflags >= 0) h->m.disableflags = disableflags;
  if (iterations >= 0) h->m.iterations = iterations;
  if (noslip_iterations >= 0) h->m.noslip_iterations = noslip_iterations;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());   // steps already queued on any stream read the old header
  return upload_header(h);
}

int aw_set_tier(aw_handle* h, int mode) {
  if (!h || mode < 0 || mode > 1) return fail(AW_EINVAL, "aw_set_tier: mode must be 0 (automatic) or 1 (wide only)");
  h->m.force_wide = mode;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());   // queued launches read the old header
  return upload_header(h);
}

int aw_set_sensors(aw_handle* h, int enable) {
  if (!h || enable < 0 || enable > 1) return fail(AW_EINVAL, "aw_set_sensors: enable must be 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());   // queued launches read the old table
  const size_t bytes = (size_t)h->nenv * std::max(h->nsensor, 1) * sizeof(float);
  if (enable && !h->sensordata) HIPCHK(hipMalloc((void**)&h->sensordata, bytes));
  if (enable && !h->sensors) HIPCHK(hipMemset(h->sensordata, 0, bytes));   // zero until an env's next forward
  float* out = enable ? h->sensordata : nullptr;
  HIPCHK(hipMemcpy(&((SensTab*)h->dsens)->out, &out, sizeof(out), hipMemcpyHostToDevice));
  h->sensors = enable != 0;
  return AW_OK;
}

static_assert(AW_DATA_MAX_CONTACTS == WIDE_MAXCON, "aw_set_data's contact cap is the wide tier's contact storage");
static_assert(AW_CONTACT_DWORDS * 4 == 4 * sizeof(MRec), "a contact record is four 16-byte stores");
int aw_set_data(aw_handle* h, int groups, int max_contacts, const aw_data_bufs* bufs) {
  if (!h) return fail(AW_EINVAL, "aw_set_data: null");
  if (groups & ~(AW_DATA_KIN | AW_DATA_DYN | AW_DATA_CONTACT)) return fail(AW_EINVAL, "aw_set_data: unknown group bits");
  // the table's head (groups, capacity, buffers); geom_id behind it stays as aw_create wrote it
  DataTab t;
  memset(&t, 0, sizeof(t));
  if (groups) {
    if (!bufs) return fail(AW_EINVAL, "aw_set_data: no buffers");
    if (max_contacts < 1 || max_contacts > AW_DATA_MAX_CONTACTS)
      return fail(AW_EINVAL, "aw_set_data: max_contacts must be 1..128 (the wide tier's contact storage)");
    if ((groups & AW_DATA_KIN) && !(bufs->xpos && bufs->xquat && bufs->site_xpos))
      return fail(AW_EINVAL, "aw_set_data: AW_DATA_KIN needs xpos, xquat and site_xpos");
    if ((groups & AW_DATA_DYN) && !(bufs->qacc && bufs->qfrc_constraint && bufs->counts))
      return fail(AW_EINVAL, "aw_set_data: AW_DATA_DYN needs qacc, qfrc_constraint and counts");
    if ((groups & AW_DATA_CONTACT) && !bufs->contact) return fail(AW_EINVAL, "aw_set_data: AW_DATA_CONTACT needs contact");
    if ((groups & AW_DATA_CONTACT) && ((uintptr_t)bufs->contact & 15))
      return fail(AW_EINVAL, "aw_set_data: contact must be 16-byte aligned");
    t.groups = groups;
    t.max_contacts = max_contacts;
    // only the requested groups' pointers reach the device: the others are never dereferenced
    if (groups & AW_DATA_KIN) { t.xpos = bufs->xpos; t.xquat = bufs->xquat; t.site_xpos = bufs->site_xpos; }
    if (groups & AW_DATA_DYN) { t.qacc = bufs->qacc; t.qfrc_constraint = bufs->qfrc_constraint; t.counts = bufs->counts; }
    if (groups & AW_DATA_CONTACT) t.contact = (MRec*)bufs->contact;
  }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());   // queued launches read the old table
  HIPCHK(hipMemcpy(h->ddata, &t, offsetof(DataTab, geom_id), hipMemcpyHostToDevice));
  h->data_groups = groups;
  return AW_OK;
}

int aw_sensor_count(const aw_handle* h) {
  if (!h) return fail(AW_EINVAL, "aw_sensor_count: null");
  return h->nsensor;
}

int aw_sensordata(aw_handle* h, float* out, void* stream) {
  if (!h || !out) return fail(AW_EINVAL, "aw_sensordata: null");
  if (!h->sensors) return fail(AW_EINVAL, "aw_sensordata: sensors are disabled (aw_set_sensors)");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemcpyAsync(out, h->sensordata, (size_t)h->nenv * h->nsensor * sizeof(float), hipMemcpyDeviceToDevice,
                        (hipStream_t)stream));
  return AW_OK;
}

int aw_set_fault(aw_handle* h, int kind, int arg) {
  if (!h || kind < 0 || kind > 2) return fail(AW_EINVAL, "aw_set_fault: kind must be 0 (none), 1 (margin) or 2 (stick row)");
  if (kind == 2 && (arg < 0 || arg >= h->m.nfl)) return fail(AW_EINVAL, "aw_set_fault: no such frictionloss row");
  if (kind == 1 && (arg < -1000 || arg > 1000)) return fail(AW_EINVAL, "aw_set_fault: margin shift beyond 1 mm");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());   // queued launches read the old table / header
  MData* dm = (MData*)h->dmodel;
  const int np = h->m.npairall;
  if (h->fault_cls.empty()) {      // the table as built, saved once
    h->fault_margin0.resize(np); h->fault_rb0.resize(np); h->fault_margin64_0.resize(np); h->fault_cls.resize(np);
    HIPCHK(hipMemcpy(h->fault_margin0.data(), dm->cp_margin, np * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h->fault_rb0.data(), dm->cp_rb, np * sizeof(float), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h->fault_margin64_0.data(), dm->cp_margin64, np * sizeof(double), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(h->fault_cls.data(), dm->cp_class, np * sizeof(int), hipMemcpyDeviceToHost));
  }
  std::vector<float> mg = h->fault_margin0, rb = h->fault_rb0;
  std::vector<double> mg64 = h->fault_margin64_0;
  if (kind == 1) {
    // every sphere / capsule pair (collider class 1): activation, the fp64 decision, the rows'
    // includemargin and the broadphase radius all see the shifted margin
    const double dl = 1e-6 * arg;
    for (int p = 0; p < np; p++)
      if (h->fault_cls[p] == 1) {
        mg64[p] += dl;
        mg[p] = (float)mg64[p];
        rb[p] = (float)((double)rb[p] + dl);
      }
  }
  HIPCHK(hipMemcpy(dm->cp_margin, mg.data(), np * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dm->cp_rb, rb.data(), np * sizeof(float), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(dm->cp_margin64, mg64.data(), np * sizeof(double), hipMemcpyHostToDevice));
  h->m.fault_flrow = kind == 2 ? arg : -1;
  return upload_header(h);
}

int aw_reset(aw_handle* h, const uint8_t* mask, const float* params, uint64_t seed, float* obs, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_reset: null");
  HIPCHK(hipSetDevice(h->device));
  h->ops->reset(h, mask, params, seed, obs, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_step(aw_handle* h, const float* actions, float* obs, float* reward, uint8_t* done, uint8_t* goal,
            float* terminal_obs, int autoreset, uint64_t seed, void* stream) {
  if (!h || !actions || !obs || !reward || !done || !goal) return fail(AW_EINVAL, "aw_step: null buffer");
  HIPCHK(hipSetDevice(h->device));
  h->ops->step(h, actions, obs, reward, done, goal, terminal_obs, autoreset, seed, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_random_actions(aw_handle* h, uint64_t seed, uint64_t step, float* actions, void* stream) {
  if (!h || !actions) return fail(AW_EINVAL, "aw_random_actions: null");
  HIPCHK(hipSetDevice(h->device));
  int bs = 256, nb = (h->nenv + bs - 1) / bs;
  hipLaunchKernelGGL(k_random_actions, dim3(nb), dim3(bs), 0, (hipStream_t)stream, h->nenv, h->m.nu, seed, step,
                     (uint64_t)h->m.env_offset, actions);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_get_state(aw_handle* h, float* qpos, float* qvel, float* warm, float* params, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_get_state: null");
  HIPCHK(hipSetDevice(h->device));
  const size_t N = h->nenv;
  const DState& s = h->st;
  return copy_fields({{qpos, s.qpos, N * h->m.nq * 4}, {qvel, s.qvel, N * h->m.nv * 4}, {warm, s.warm, N * h->m.nv * 4},
                      {h->m.nparam ? params : nullptr, s.params, N * h->m.nparam * 4}}, stream);
}

int aw_set_state(aw_handle* h, const float* qpos, const float* qvel, const float* warm, const float* params,
                 float* obs, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_set_state: null");
  HIPCHK(hipSetDevice(h->device));
  h->ops->set(h, qpos, qvel, warm, params, obs, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

static void launch_get_ids(aw_handle* h, const int32_t* env_ids, int n_sel, float* qpos, float* qvel, float* warm,
                           float* params, int* ep_len, float* ep_ret, int* ep_goal, hipStream_t st) {
  hipLaunchKernelGGL(k_get_state_ids, dim3((n_sel + 3) / 4), dim3(256), 0, st, h->st, h->nenv, h->m.nq, h->m.nv,
                     h->m.nparam, env_ids, n_sel, qpos, qvel, warm, h->m.nparam ? params : nullptr, ep_len, ep_ret,
                     ep_goal);
}

int aw_set_state_ids(aw_handle* h, const int32_t* env_ids, int n_sel, const int32_t* rows, int n_rows,
                     const float* qpos, const float* qvel, const float* warm, const float* params, int reset_episode,
                     float* obs, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_set_state_ids: null");
  if (!env_ids || n_sel < 1 || n_rows < 1)
    return fail(AW_EINVAL, "aw_set_state_ids: env_ids must be given, n_sel >= 1 and n_rows >= 1");
  HIPCHK(hipSetDevice(h->device));
  const SetIds a = {env_ids, rows, nullptr, n_sel, n_rows, qpos, qvel, warm, h->m.nparam ? params : nullptr,
                    nullptr, nullptr, nullptr, reset_episode != 0};
  h->ops->set_ids(h, a, obs, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_get_state_ids(aw_handle* h, const int32_t* env_ids, int n_sel, float* qpos, float* qvel, float* warm,
                     float* params, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_get_state_ids: null");
  if (!env_ids || n_sel < 1) return fail(AW_EINVAL, "aw_get_state_ids: env_ids must be given and n_sel >= 1");
  HIPCHK(hipSetDevice(h->device));
  launch_get_ids(h, env_ids, n_sel, qpos, qvel, warm, params, nullptr, nullptr, nullptr, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_clone_envs(aw_handle* h, const int32_t* src_ids, const int32_t* dst_ids, int n, int episode, float* obs,
                  void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_clone_envs: null");
  if (!src_ids || !dst_ids || n < 1 || n > h->nenv)
    return fail(AW_EINVAL, "aw_clone_envs: src_ids and dst_ids must be given and n in 1..n_envs");
  HIPCHK(hipSetDevice(h->device));
  // the scratch block: nenv rows of qpos, qvel, warmstart, params and the three episode counters
  const size_t N = (size_t)h->nenv, nq = h->m.nq, nv = h->m.nv, np = h->m.nparam;
  if (!h->clone_scratch) HIPCHK(hipMalloc(&h->clone_scratch, N * (nq + 2 * nv + np + 3) * sizeof(float)));
  float* q = (float*)h->clone_scratch;
  float *v = q + N * nq, *w = v + N * nv, *p = w + N * nv, *er = p + N * np;
  int32_t *el = (int32_t*)(er + N), *eg = el + N;
  // every read before any write: the gather ends before the set kernel starts (one stream)
  launch_get_ids(h, src_ids, n, q, v, w, p, episode ? el : nullptr, episode ? er : nullptr, episode ? eg : nullptr,
                 (hipStream_t)stream);
  const SetIds a = {dst_ids, nullptr, src_ids, n, n, q, v, w, np ? p : nullptr,
                    episode ? el : nullptr, episode ? er : nullptr, episode ? eg : nullptr, 0};
  h->ops->set_ids(h, a, obs, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_status(aw_handle* h, uint32_t* last, uint32_t* sticky, void* stream) {
  if (!h || (!last && !sticky)) return fail(AW_EINVAL, "aw_status: null");
  HIPCHK(hipSetDevice(h->device));
  const size_t b = (size_t)h->nenv * 4;
  return copy_fields({{last, h->st.status, b}, {sticky, h->st.status_acc, b}}, stream);
}

int aw_clear_status(aw_handle* h, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_clear_status: null");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipMemsetAsync(h->st.status_acc, 0, (size_t)h->nenv * 4, (hipStream_t)stream));
  return AW_OK;
}

int aw_set_env_offset(aw_handle* h, uint64_t env_offset) {
  if (!h) return fail(AW_EINVAL, "aw_set_env_offset: null");
  h->m.env_offset = env_offset;
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());   // steps already queued read the old header
  return upload_header(h);
}

int aw_get_episode(aw_handle* h, int32_t* ep_len, float* ep_ret, int32_t* ep_goal, int32_t* episodes,
                   void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_get_episode: null");
  HIPCHK(hipSetDevice(h->device));
  const size_t b = (size_t)h->nenv * 4;
  const DState& s = h->st;
  return copy_fields({{ep_len, s.ep_len, b}, {ep_ret, s.ep_ret, b}, {ep_goal, s.ep_goal, b}, {episodes, s.episode, b}},
                     stream);
}

int aw_set_episode(aw_handle* h, const int32_t* ep_len, const float* ep_ret, const int32_t* ep_goal,
                   const int32_t* episodes, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_set_episode: null");
  HIPCHK(hipSetDevice(h->device));
  const size_t b = (size_t)h->nenv * 4;
  const DState& s = h->st;
  return copy_fields({{s.ep_len, ep_len, b}, {s.ep_ret, ep_ret, b}, {s.ep_goal, ep_goal, b}, {s.episode, episodes, b}},
                     stream);
}

int aw_episode_totals(aw_handle* h, int32_t* episodes, float* sum_return, int32_t* successes, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_episode_totals: null");
  HIPCHK(hipSetDevice(h->device));
  const size_t b = (size_t)h->nenv * 4;
  const DState& s = h->st;
  return copy_fields({{episodes, s.episode, b}, {sum_return, s.sum_ret, b}, {successes, s.n_success, b}}, stream);
}

int aw_set_episode_totals(aw_handle* h, const int32_t* episodes, const float* sum_return, const int32_t* successes,
                          void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_set_episode_totals: null");
  HIPCHK(hipSetDevice(h->device));
  const size_t b = (size_t)h->nenv * 4;
  const DState& s = h->st;
  return copy_fields({{s.episode, episodes, b}, {s.sum_ret, sum_return, b}, {s.n_success, successes, b}}, stream);
}

int aw_episode_stats(aw_handle* h, float* last_return, int32_t* last_goal, int32_t* last_len, int32_t* episodes,
                     void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_episode_stats: null");
  HIPCHK(hipSetDevice(h->device));
  const size_t b = (size_t)h->nenv * 4;
  const DState& s = h->st;
  return copy_fields({{last_return, s.last_ret, b}, {last_goal, s.last_goal, b}, {last_len, s.last_len, b},
                      {episodes, s.episode, b}}, stream);
}

int aw_task_eval(aw_handle* h, int n, const float* qpos, const float* qvel, const float* xpos, const float* xquat,
                 const float* sxpos, const float* touch, float* obs, float* reward, uint8_t* done, uint8_t* goal,
                 void* stream) {
  if (!h || n <= 0) return fail(AW_EINVAL, "aw_task_eval: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_task_eval, dim3(n), dim3(64), 0, (hipStream_t)stream, h->m, n, qpos, qvel, xpos, xquat,
                     sxpos, touch, obs, reward, done, goal);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_forward_dump(aw_handle* h, int env, const float* ctrl, float* out, void* stream) {
  if (!h || !out || env < 0 || env >= h->nenv) return fail(AW_EINVAL, "aw_forward_dump: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  h->ops->dump(h, env, ctrl, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_forward_dump_wide(aw_handle* h, int env, const float* ctrl, float* out, void* stream) {
  if (!h || !out || env < 0 || env >= h->nenv) return fail(AW_EINVAL, "aw_forward_dump_wide: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  h->wide->dump(h, env, ctrl, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_dynamics(aw_handle* h, const int32_t* env_ids, int n_sel, const aw_dyn_point* points, int npoints,
                const float* qpos, const float* qvel, const float* ctrl, const aw_dyn_out* out, void* stream) {
  if (!h || !out) return fail(AW_EINVAL, "aw_dynamics: null handle or out");
  const bool pt_out = out->point_pos || out->point_vel || out->jacp || out->jacr;
  if (!pt_out && !out->qM && !out->qMinv && !out->qfrc_bias && !out->qfrc_passive && !out->qfrc_actuator && !out->xvel)
    return fail(AW_EINVAL, "aw_dynamics: no output requested");
  if (npoints < 0 || npoints > AW_DYN_MAXPOINTS || (npoints > 0 && !points))
    return fail(AW_EINVAL, "aw_dynamics: npoints must be 0..AW_DYN_MAXPOINTS, with points given");
  if (pt_out && npoints == 0) return fail(AW_EINVAL, "aw_dynamics: a point output needs npoints >= 1");
  if (env_ids && n_sel < 1) return fail(AW_EINVAL, "aw_dynamics: n_sel must be >= 1 with env_ids");
  DynPts pts = {};   // a kernel argument, as the views of the render calls are
  for (int p = 0; p < npoints; p++) {
    const int kind = points[p].kind, id = points[p].id;
    if (kind != AW_PT_BODY && kind != AW_PT_BODYCOM && kind != AW_PT_SITE)
      return fail(AW_EINVAL, "aw_dynamics: a point's kind is none of AW_PT_BODY, AW_PT_BODYCOM, AW_PT_SITE");
    if (id < 0 || id >= (kind == AW_PT_SITE ? h->m.nsite : h->m.nbody))
      return fail(AW_EINVAL, "aw_dynamics: a point's id is not a body / site of the model");
    pts.kind[p] = kind;
    pts.id[p] = id;
  }
  HIPCHK(hipSetDevice(h->device));
  h->ops->dyn(h, env_ids, env_ids ? n_sel : h->nenv, pts, npoints, qpos, qvel, ctrl, *out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_solve_ik(aw_handle* h, const int32_t* env_ids, int n_sel, const aw_ik_target* targets, int ntargets,
                uint64_t dof_mask, const float* goal, const float* qpos0, const aw_ik_opt* opt, const aw_ik_out* out,
                void* stream) {
  if (!h || !targets || !goal || !opt || !out || !out->qpos)
    return fail(AW_EINVAL, "aw_solve_ik: null handle, targets, goal, opt, out or out->qpos");
  if (ntargets < 1 || ntargets > AW_IK_MAXTARGETS) return fail(AW_EINVAL, "aw_solve_ik: ntargets must be 1..AW_IK_MAXTARGETS");
  if (env_ids && n_sel < 1) return fail(AW_EINVAL, "aw_solve_ik: n_sel must be >= 1 with env_ids");
  IkTgt tg = {};   // a kernel argument, as the points of aw_dynamics are
  int rows = 0;
  for (int p = 0; p < ntargets; p++) {
    const aw_ik_target& t = targets[p];
    if (t.kind != AW_PT_BODY && t.kind != AW_PT_BODYCOM && t.kind != AW_PT_SITE)
      return fail(AW_EINVAL, "aw_solve_ik: a target's kind is none of AW_PT_BODY, AW_PT_BODYCOM, AW_PT_SITE");
    if (t.id < 0 || t.id >= (t.kind == AW_PT_SITE ? h->m.nsite : h->m.nbody))
      return fail(AW_EINVAL, "aw_solve_ik: a target's id is not a body / site of the model");
    if (!std::isfinite(t.wpos) || !std::isfinite(t.wrot) || t.wpos < 0.f || t.wrot < 0.f)
      return fail(AW_EINVAL, "aw_solve_ik: a target's weights must be finite and >= 0");
    if (t.wpos == 0.f && t.wrot == 0.f) return fail(AW_EINVAL, "aw_solve_ik: a target with both weights 0");
    tg.kind[p] = t.kind;
    tg.id[p] = t.id;
    tg.row[p] = rows;
    tg.wpos[p] = t.wpos;
    tg.wrot[p] = t.wrot;
    rows += (t.wpos > 0.f ? 3 : 0) + (t.wrot > 0.f ? 3 : 0);
  }
  if (rows > AW_IK_MAXROWS) return fail(AW_EINVAL, "aw_solve_ik: more than AW_IK_MAXROWS residual rows");
  const uint64_t below_nv = h->m.nv < 64 ? (1ull << h->m.nv) - 1ull : ~0ull;
  if (!(dof_mask & below_nv)) return fail(AW_EINVAL, "aw_solve_ik: dof_mask selects no dof of the model");
  if (opt->max_iter < 0 || opt->max_iter > AW_IK_MAXITER) return fail(AW_EINVAL, "aw_solve_ik: max_iter must be 0..AW_IK_MAXITER");
  if (!(opt->damping > 0.f) || !std::isfinite(opt->damping)) return fail(AW_EINVAL, "aw_solve_ik: damping must be finite and > 0");
  if (!(opt->tol >= 0.f)) return fail(AW_EINVAL, "aw_solve_ik: tol must be >= 0");
  if (!std::isfinite(opt->max_step)) return fail(AW_EINVAL, "aw_solve_ik: max_step must be finite");
  if (opt->clamp_range != 0 && opt->clamp_range != 1) return fail(AW_EINVAL, "aw_solve_ik: clamp_range must be 0 or 1");
  HIPCHK(hipSetDevice(h->device));
  h->ops->ik(h, env_ids, env_ids ? n_sel : h->nenv, tg, ntargets, rows, dof_mask & below_nv, goal, qpos0, *opt, *out,
             (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

static_assert(sizeof(aw_ray_rec) == 40 && offsetof(aw_ray_rec, keep) == 32, "aw_ray_rec is 40 bytes");
int aw_set_rays(aw_handle* h, const aw_ray_rec* rays, int nrays) {
  if (!h) return fail(AW_EINVAL, "aw_set_rays: null");
  if (nrays < 0 || nrays > AW_MAX_RAYS || (nrays > 0 && !rays))
    return fail(AW_EINVAL, "aw_set_rays: nrays must be 0..AW_MAX_RAYS, with rays given");
  // validated here, so that every index the kernel forms from the table is trusted
  const unsigned long long all = h->m.nrgeom < 64 ? (1ull << h->m.nrgeom) - 1ull : ~0ull;
  std::vector<aw_ray_rec> tab(rays, rays + nrays);
  for (aw_ray_rec& r : tab) {
    if (r.body < 0 || r.body >= h->m.nbody) return fail(AW_EINVAL, "aw_set_rays: a ray's body is not a body of the model");
    bool fin = std::isfinite(r.xmax), zero = true;
    for (int k = 0; k < 3; k++) {
      fin = fin && std::isfinite(r.pnt[k]) && std::isfinite(r.vec[k]);
      zero = zero && r.vec[k] == 0.f;
    }
    if (!fin || zero) return fail(AW_EINVAL, "aw_set_rays: pnt, vec and xmax must be finite and vec not zero");
    r.keep &= all;
  }
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());   // casts already queued on any stream read the old table
  if (nrays == 0) {
    if (h->rays) HIPCHK(hipFree(h->rays));
    h->rays = nullptr;
    h->nrays = 0;
    return AW_OK;
  }
  h->nrays = 0;   // no table while the upload can still fail
  if (!h->rays) HIPCHK(hipMalloc(&h->rays, AW_MAX_RAYS * sizeof(aw_ray_rec)));
  HIPCHK(hipMemcpy(h->rays, tab.data(), (size_t)nrays * sizeof(aw_ray_rec), hipMemcpyHostToDevice));
  h->nrays = nrays;
  return AW_OK;
}

int aw_cast_rays(aw_handle* h, const int32_t* env_ids, int n_sel, const float* env_rays, float* dist, int32_t* entry,
                 void* stream) {
  if (!h || !dist) return fail(AW_EINVAL, "aw_cast_rays: null handle or dist");
  if (!h->rays || h->nrays < 1) return fail(AW_EINVAL, "aw_cast_rays: no ray table set (aw_set_rays)");
  if (env_ids && n_sel < 1) return fail(AW_EINVAL, "aw_cast_rays: n_sel must be >= 1 with env_ids");
  HIPCHK(hipSetDevice(h->device));
  h->ops->rays(h, env_ids, env_ids ? n_sel : h->nenv, env_rays, dist, entry, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_render_depth(aw_handle* h, const float* cam, int width, int height, float* out, void* stream) {
  if (!h || !cam || !out || width <= 0 || height <= 0 || width > 4096 || height > 4096)
    return fail(AW_EINVAL, "aw_render_depth: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  CamRec c;
  memcpy(c.c, cam, sizeof(c.c));   // host array: the camera record travels as a kernel argument
  h->ops->depth(h, c, width, height, out, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_render_rgb(aw_handle* h, const float* cam, const float* look, int width, int height, int ss, uint8_t* rgb,
                  float* depth, void* stream) {
  if (!h || !cam || !rgb || width <= 0 || height <= 0 || width > 1024 || height > 1024 || (ss != 1 && ss != 2) ||
      (depth && ss != 1))
    return fail(AW_EINVAL, "aw_render_rgb: bad arguments");
  if (!h->m.appearance) return fail(AW_EUNSUPPORTED, "aw_render_rgb: the model table carries no appearance arrays");
  HIPCHK(hipSetDevice(h->device));
  CamRec c;
  memcpy(c.c, cam, sizeof(c.c));
  if (has_appearance(h)) {   // one world-frame view: the same frames
    ViewsRec r = {};
    memcpy(r.c[0], cam, sizeof(r.c[0]));
    h->ops->views(h, r, 1, nullptr, look_rec(look), width, height, ss, rgb, depth, (hipStream_t)stream);
  } else {
    h->ops->rgb(h, c, look_rec(look), width, height, ss, rgb, depth, (hipStream_t)stream);
  }
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_render_views(aw_handle* h, const aw_view* views, int nviews, const float* env_cam, const float* look, int width,
                    int height, int ss, uint8_t* rgb, float* depth, void* stream) {
  if (!h || !views || nviews < 1 || nviews > AW_MAX_VIEWS || (!rgb && !depth) || width <= 0 || height <= 0 ||
      width > 1024 || height > 1024 || (ss != 1 && ss != 2) || (ss != 1 && (depth || !rgb)))
    return fail(AW_EINVAL, "aw_render_views: bad arguments");
  ViewsRec r;
  if (int rc = fill_views(h, "aw_render_views", views, nviews, r)) return rc;
  if (rgb && !h->m.appearance)
    return fail(AW_EUNSUPPORTED, "aw_render_views: the model table carries no appearance arrays");
  HIPCHK(hipSetDevice(h->device));
  h->ops->views(h, r, nviews, env_cam, look_rec(look), width, height, ss, rgb, depth, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_set_appearance(aw_handle* h, const aw_appearance* app, int shadows) {
  if (!h || (shadows != 0 && shadows != 1)) return fail(AW_EINVAL, "aw_set_appearance: shadows must be 0 or 1");
  if (!h->m.appearance)
    return fail(AW_EUNSUPPORTED, "aw_set_appearance: the model table carries no appearance arrays");
  HIPCHK(hipSetDevice(h->device));
  HIPCHK(hipDeviceSynchronize());   // frames already queued are shaded from the tables they were launched with
  h->app = app ? AppRec{app->col, app->light, app->look} : AppRec{nullptr, nullptr, nullptr};
  h->shadows = shadows;
  return AW_OK;
}

int aw_appearance_defaults(const aw_handle* h, float* col, float* light, int* nlight) {
  if (!h) return fail(AW_EINVAL, "aw_appearance_defaults: null");
  if (!h->m.appearance)
    return fail(AW_EUNSUPPORTED, "aw_appearance_defaults: the model table carries no appearance arrays");
  HIPCHK(hipSetDevice(h->device));
  const MData* d = (const MData*)h->dmodel;
  const size_t ne = (size_t)(h->m.nrgeom + h->m.nrsite);
  if (col) HIPCHK(hipMemcpy(col, d->rg_col, ne * COL_W * sizeof(float), hipMemcpyDeviceToHost));
  if (light && h->m.nlight) {
    HIPCHK(hipMemcpy(light, d->light, (size_t)h->m.nlight * LIGHT_W * sizeof(float), hipMemcpyDeviceToHost));
    for (int l = 0; l < h->m.nlight; l++) light[l * LIGHT_W + 21] = 1.f;   // castshadow: MuJoCo's default
  }
  if (nlight) *nlight = h->m.nlight;
  return AW_OK;
}

int aw_appearance_sample(aw_handle* h, const float* lo, const float* hi, const int32_t* env_ids, int n_sel,
                         uint64_t seed, uint64_t draw, float* col, float* light, float* look, void* stream) {
  if (!h) return fail(AW_EINVAL, "aw_appearance_sample: null");
  if (!h->m.appearance)
    return fail(AW_EUNSUPPORTED, "aw_appearance_sample: the model table carries no appearance arrays");
  if (!lo || !hi || (!col && !light && !look) || (env_ids && n_sel < 1))
    return fail(AW_EINVAL, "aw_appearance_sample: lo and hi, an output, and n_sel >= 1 with env_ids must be given");
  const int nc = (h->m.nrgeom + h->m.nrsite) * COL_W, nl = h->m.nlight * LIGHT_W, F = nc + nl + AW_LOOK_FLOATS;
  for (int i = 0; i < F; i++)
    if (!(lo[i] <= hi[i])) return fail(AW_EINVAL, "aw_appearance_sample: the bounds need lo <= hi in every slot");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  // the bounds travel through a device block of the handle (too long for kernel arguments), uploaded
  // only when they differ from the last call's: then the stream is drained first (a sampler launch
  // still queued reads the old bounds) and the copy is complete before the host arrays are let go
  const size_t cap = (size_t)(MAXRG * COL_W + MAXLIGHT * LIGHT_W + AW_LOOK_FLOATS);
  if (!h->app_bounds) HIPCHK(hipMalloc((void**)&h->app_bounds, 2 * cap * sizeof(float)));
  std::vector<float> b(lo, lo + F);
  b.insert(b.end(), hi, hi + F);
  if (b.size() != h->app_bounds_host.size() || memcmp(b.data(), h->app_bounds_host.data(), b.size() * sizeof(float))) {
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(h->app_bounds, lo, F * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(h->app_bounds + cap, hi, F * sizeof(float), hipMemcpyHostToDevice));
    h->app_bounds_host.swap(b);
  }
  const int rows = env_ids ? n_sel : h->nenv;
  for (int r0 = 0; r0 < rows; r0 += 65535)   // the grid's y limit
    hipLaunchKernelGGL(k_appearance, dim3((F + 255) / 256, std::min(rows - r0, 65535)), dim3(256), 0, st, h->nenv, nc, nl,
                       h->app_bounds, h->app_bounds + cap, env_ids, r0, (uint64_t)h->m.env_offset, seed, draw, col,
                       light, look);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_render_entries(const aw_handle* h, int* ngeom, int* nsite) {
  if (!h || !ngeom || !nsite) return fail(AW_EINVAL, "aw_render_entries: null");
  *ngeom = h->m.nrgeom;
  *nsite = h->m.nrsite;
  return AW_OK;
}

int aw_render_labels(aw_handle* h, const aw_view* views, int nviews, const float* env_cam, const int32_t* env_ids,
                     int n_sel, const int32_t* lut, int32_t background, int sites, int width, int height,
                     int32_t* labels, float* depth, void* stream) {
  if (!h || !views || nviews < 1 || nviews > AW_MAX_VIEWS || !labels || width <= 0 || height <= 0 || width > 1024 ||
      height > 1024 || (env_ids && n_sel < 1) || (sites != 0 && sites != 1))
    return fail(AW_EINVAL, "aw_render_labels: bad arguments");
  ViewsRec r;
  if (int rc = fill_views(h, "aw_render_labels", views, nviews, r)) return rc;
  if (sites && !h->m.appearance)
    return fail(AW_EUNSUPPORTED, "aw_render_labels: the model table carries no appearance arrays (no visible sites)");
  HIPCHK(hipSetDevice(h->device));
  const int ne = h->m.nrgeom + h->m.nrsite;
  LutRec l;
  for (int e = 0; e < MAXRG; e++) l.v[e] = e < ne && lut ? lut[e] : e;   // a kernel argument, as the views are
  h->ops->labels(h, r, nviews, env_cam, env_ids, env_ids ? n_sel : h->nenv, l, background, sites, width, height, labels,
                 depth, (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_render_cloud(aw_handle* h, const aw_view* views, int nviews, const float* env_cam, const int32_t* env_ids,
                    int n_sel, const uint8_t* keep, const float* box, int frame_body, int sites, int width, int height,
                    int cap, float* xyz, int32_t* pix, int32_t* count, void* stream) {
  if (!h || !views || nviews < 1 || nviews > AW_MAX_VIEWS || !xyz || !count || width <= 0 || height <= 0 ||
      width > 1024 || height > 1024 || (env_ids && n_sel < 1) || (sites != 0 && sites != 1) || cap < 1 ||
      cap > AW_CLOUD_MAXCAND)
    return fail(AW_EINVAL, "aw_render_cloud: bad arguments");
  ViewsRec r;
  if (int rc = fill_views(h, "aw_render_cloud", views, nviews, r)) return rc;
  if (frame_body < 0 || frame_body >= h->m.nbody)
    return fail(AW_EINVAL, "aw_render_cloud: frame_body is not a body of the model");
  for (int k = 0; box && k < 3; k++)
    if (!(box[k] <= box[3 + k])) return fail(AW_EINVAL, "aw_render_cloud: the box needs lo <= hi on every axis");
  if (sites && !h->m.appearance)
    return fail(AW_EUNSUPPORTED, "aw_render_cloud: the model table carries no appearance arrays (no visible sites)");
  HIPCHK(hipSetDevice(h->device));
  CloudRec c = {};
  const int ne = h->m.nrgeom + h->m.nrsite;
  for (int e = 0; e < ne; e++)
    if (!keep || keep[e]) c.keep |= 1ull << e;   // kernel arguments too: the keep table and the box
  if (box) memcpy(c.box, box, sizeof(c.box));
  c.crop = box ? 1 : 0;
  c.frame_body = frame_body;
  c.cap = cap;
  h->ops->cloud(h, r, nviews, env_cam, env_ids, env_ids ? n_sel : h->nenv, c, sites, width, height, xyz, pix, count,
                (hipStream_t)stream);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_cloud_fps(int n, int cap, const float* xyz, const int32_t* count, int npoints, float* out_xyz, int32_t* out_idx,
                 void* stream) {
  if (n <= 0 || cap < 1 || cap > AW_CLOUD_MAXCAND || !xyz || !count || npoints < 1 || npoints > AW_FPS_MAXPOINTS ||
      !out_xyz)
    return fail(AW_EINVAL, "aw_cloud_fps: bad arguments");
  hipStream_t st = (hipStream_t)stream;
  // the capacity classes: LDS per workgroup 16 / 28 / 52 / 100 KiB
  if (cap <= 1024)
    hipLaunchKernelGGL((k_fps<1024, 256>), dim3(n), dim3(256), 0, st, cap, npoints, xyz, count, out_xyz, out_idx);
  else if (cap <= 2048)
    hipLaunchKernelGGL((k_fps<2048, 256>), dim3(n), dim3(256), 0, st, cap, npoints, xyz, count, out_xyz, out_idx);
  else if (cap <= 4096)
    hipLaunchKernelGGL((k_fps<4096, 512>), dim3(n), dim3(512), 0, st, cap, npoints, xyz, count, out_xyz, out_idx);
  else
    hipLaunchKernelGGL((k_fps<8192, 1024>), dim3(n), dim3(1024), 0, st, cap, npoints, xyz, count, out_xyz, out_idx);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_policy_mlp(int n, int in_dim, int hidden, int out_dim, const float* params, const float* obs, float* act,
                  int sample, uint64_t seed, uint64_t step, uint64_t env_offset, void* stream) {
  if (n <= 0 || !params || !obs || !act || in_dim <= 0 || in_dim > MLP_IMAX || out_dim <= 0 || out_dim > MLP_OMAX)
    return fail(AW_EINVAL, "aw_policy_mlp: bad arguments");
  const int bs = 256, nb = (n + bs - 1) / bs;
  hipStream_t st = (hipStream_t)stream;
  switch (hidden) {
    case 32: hipLaunchKernelGGL(k_mlp<32>, dim3(nb), dim3(bs), 0, st, n, in_dim, out_dim, params, obs, act, sample, seed, step, env_offset); break;
    case 64: hipLaunchKernelGGL(k_mlp<64>, dim3(nb), dim3(bs), 0, st, n, in_dim, out_dim, params, obs, act, sample, seed, step, env_offset); break;
    default: return fail(AW_EUNSUPPORTED, "aw_policy_mlp: hidden width must be 32 or 64 (two hidden layers)");
  }
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_collide_test(aw_handle* h, int n, const int32_t* types, const float* pos, const float* mat, const float* size,
                    const float* margin, float* out, int32_t* count, double* out64, void* stream) {
  if (!h || n <= 0 || !types || !pos || !mat || !size || !margin || !out || !count)
    return fail(AW_EINVAL, "aw_collide_test: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_collide_test, dim3(n), dim3(64), 0, st, h->m, n, types, pos, mat, size, margin, out, count, out64);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_midphase_test(aw_handle* h, int n, const int32_t* pair, const float* pos, const float* quat, const float* size,
                     int32_t* info, float* margin, void* stream) {
  if (!h || n <= 0 || !pair || !pos || !quat || !size || !info || !margin)
    return fail(AW_EINVAL, "aw_midphase_test: bad arguments");
  HIPCHK(hipSetDevice(h->device));
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(k_midphase_test, dim3(n), dim3(64), 0, st, h->m, n, pair, pos, quat, size, info, margin);
  HIPCHK(hipGetLastError());
  return AW_OK;
}

int aw_stage_profile(unsigned long long* out, int reset) {
#ifdef AW_STAGE_PROF
  HIPCHK(stage_prof_read(out, reset));
  return AW_OK;
#else
  (void)out; (void)reset;
  return fail(AW_EUNSUPPORTED, "library built without -DAW_STAGE_PROF");
#endif
}

}  // extern "C"
