// aw_kernels.hip -- the kernels of ONE task and the launcher table that hands them to the API unit
// (aw_api.hip).  The library holds this file eight times (__graft_entry__.py): per task once with
// -DAW_TASK_TU=<task> (the fast tier: k_step, k_reset, k_set_state, k_set_state_ids, k_dump, k_depth, k_rgb, k_views,
// k_views_app, k_labels, k_cloud, k_dyn (aw_dyn.h), k_rays (aw_rays.h), k_ik (aw_ik.h), k_order and task_ops<task>) and once with -DAW_TASK_TU=<task> -DAW_WIDE (the wide
// tier: k_step_wide, k_dump_wide and wide_ops<task>).  AW_WIDE is the tier switch of aw_common.h's capacities; the
// env-step both tiers run is aw_step.h.  Written once: finish_forward (the tail of k_reset and the set-state kernels),
// set_state_body (both set-state kernels), stage_pose / view_cam (the render kernels' prologue and per-view camera).
#ifndef AW_TASK_TU
#error "aw_kernels.hip is one task's unit: compile it with -DAW_TASK_TU=<task kind>"
#endif
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "aw_common.h"
#include "aw_handle.h"
#include "aw_render.h"
#include "aw_step.h"
#ifndef AW_WIDE
#include "aw_dyn.h"   // k_dyn: the fast-tier unit only
#include "aw_rays.h"  // k_rays: likewise
#include "aw_ik.h"    // k_ik: likewise
#endif

using namespace aw;

// introspection: one forward of one env, both tiers (aw_forward_dump / aw_forward_dump_wide)
// dump layout (floats): see mj_envs_amd/_native.py dump_layout (same offsets from the tier's capacities)
constexpr int DUMP_SCAL = 1760, DUMP_CON = 1768, DUMP_EFC = DUMP_CON + 14 * MAXCON;
static_assert(DUMP_EFC + 5 * MAXEFC == (WIDE ? AW_DUMP_SIZE_WIDE : AW_DUMP_SIZE), "AW_DUMP_SIZE(_WIDE) out of date");
// distinct kernel names per tier: the fast and wide units both instantiate it
#ifdef AW_WIDE
#define AW_K_DUMP k_dump_wide
#else
#define AW_K_DUMP k_dump
#endif
template <int TASK>
__global__ void __launch_bounds__(64) AW_K_DUMP(DModel m, DState st, int env, const float* ctrl, float* out) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  const int lane = threadIdx.x;
  load_env<NV>(m, s, st, env, lane);
  if (lane < m.nu) s.ctrl[lane] = ctrl ? ctrl[lane] : 0.f;
  stage_model(m, s, st.params + (size_t)env * m.nparam, lane);
  float Mrow[NV];
  Dof d;
  for (int r = lane; r < MAXEFC; r += 64) out[DUMP_EFC + 4 * MAXEFC + r] = -1.f;
  forward<TASK, true>(m, s, lane, Mrow, d, out + DUMP_EFC + 4 * MAXEFC);   // + the Newton row states
  for (int i = lane; i < MAXB * 3; i += 64) out[i] = i < m.nbody * 3 ? (&s.xpos[0][0])[i] : 0.f;
  for (int i = lane; i < MAXB * 4; i += 64) out[96 + i] = i < m.nbody * 4 ? (&s.xquat[0][0])[i] : 0.f;
  for (int i = lane; i < MAXS * 3; i += 64) out[224 + i] = i < m.nsite * 3 ? (&s.sxpos[0][0])[i] : 0.f;
  if (lane < MAXV) {
    bool v = lane < NV;
    out[320 + lane] = v ? d.qacc_smooth : 0.f;
    out[356 + lane] = v ? d.qfrc_smooth : 0.f;
    out[392 + lane] = v ? d.qacc : 0.f;
    out[428 + lane] = v ? d.qfrc_con : 0.f;
  }
  for (int k = 0; k < NV; k++)
    if (lane < NV) out[464 + lane * NV + k] = Mrow[k];
  if (lane == 0) {
    out[DUMP_SCAL] = (float)s.ncon; out[DUMP_SCAL + 1] = (float)s.nefc; out[DUMP_SCAL + 2] = (float)s.nsparse;
    out[DUMP_SCAL + 3] = (float)s.ndense; out[DUMP_SCAL + 4] = s.touch[0]; out[DUMP_SCAL + 5] = (float)s.status;
    out[DUMP_SCAL + 6] = (float)s.it_newton; out[DUMP_SCAL + 7] = (float)s.it_noslip;
  }
  for (int c = lane; c < MAXCON; c += 64) {
    bool v = c < s.ncon;
    out[DUMP_CON + c] = v ? s.con_dist[c] : 0.f;
    for (int k = 0; k < 3; k++) out[DUMP_CON + MAXCON + 3 * c + k] = v ? s.con_pos[c][k] : 0.f;
    float fr[9];
    for (int k = 0; k < 3; k++) { fr[k] = v ? s.con_nrm[c][k] : 1.f; fr[3 + k] = 0.f; }
    make_frame(fr);
    for (int k = 0; k < 9; k++) out[DUMP_CON + 4 * MAXCON + 9 * c + k] = v ? fr[k] : 0.f;
    out[DUMP_CON + 13 * MAXCON + c] = v ? (float)s.con_pair[c] : -1.f;
  }
  for (int r = lane; r < MAXEFC; r += 64) {
    bool v = r < s.nefc;
    out[DUMP_EFC + r] = v ? s.efc_force[r] : 0.f;
    out[DUMP_EFC + MAXEFC + r] = v ? s.efc_aref[r] : 0.f;
    out[DUMP_EFC + 2 * MAXEFC + r] = v ? s.efc_D[r] : 0.f;
    out[DUMP_EFC + 3 * MAXEFC + r] = v ? (float)s.efc_type[r] : -1.f;
  }
}

#ifdef AW_WIDE
// The wide tier: persistent workgroups drain the queue the fast launch before it filled (q[0]
// entries; an empty queue ends every workgroup at its first claim).  Same env-step code with
// MuJoCo's capacities; mptr is the wide header (its jspill: one JSPILL_WIDE block per workgroup).
// The claim loop is bounded by the handle's env count (the queue holds at most one entry per env and
// launch), so every wave reaches its exit whatever the queue words hold; an entry that is not a valid
// (env < n, kind DK_STEP / DK_FORWARD) pair is skipped -- -DAW_DEVICE_ASSERT traps instead.
template <int TASK, bool SENS, bool DATA>
__global__ void __launch_bounds__(64) k_step_wide(const DModel* __restrict__ mptr, const float* __restrict__ actions,
                                                  float* obs, float* reward, uint8_t* done, uint8_t* goal,
                                                  float* terminal_obs, int autoreset, uint64_t seed,
                                                  int* __restrict__ q, int n) {
  const DModel& m = *mptr;
  const DState& st = *reinterpret_cast<const DState*>(mptr + 1);
  __shared__ Env s;
  __shared__ StepIO io;
  const int lane = threadIdx.x;
  park_io(io, lane, actions, obs, reward, done, goal, terminal_obs, autoreset, seed, nullptr);
  for (int claims = 0; claims <= n; claims++) {
    int k = 0;
    if (lane == 0) k = atomicAdd(q + 1, 1);
    k = __builtin_amdgcn_readfirstlane(k);
    const int nq = q[0];
#ifdef AW_DEVICE_ASSERT
    if ((unsigned)nq > (unsigned)n) __builtin_trap();
#endif
    if (k >= nq || k >= n) break;
    const int ent = q[2 + k];
    const int env = ent & 0x3fffffff, kind = ent >> 30;
    if ((unsigned)env >= (unsigned)n || kind > DK_FORWARD) {
#ifdef AW_DEVICE_ASSERT
      __builtin_trap();
#endif
      continue;
    }
    env_step<TASK, SENS, DATA>(m, s, st, env, lane, io, kind);
  }
}

template <int TASK>
static void launch_wide(aw_handle* h, const float* a, float* obs, float* rew, uint8_t* done, uint8_t* goal,
                        float* tobs, int autoreset, uint64_t seed, hipStream_t st) {
  with_sens_data(h, [&](auto S, auto D) {
    hipLaunchKernelGGL((k_step_wide<TASK, decltype(S)::value, decltype(D)::value>), dim3(h->wide_grid), dim3(64), 0, st,
                       (const DModel*)h->dmhdr_wide, a, obs, rew, done, goal, tobs, autoreset, seed, h->next_env + 8, h->nenv);
  });
}
template <int TASK>
static void launch_dump_wide(aw_handle* h, int env, const float* ctrl, float* out, hipStream_t st) {
  DModel mw = h->m;
  mw.jspill = h->jspill_wide;   // the dense rows past JL in the wide tier's spill block (slot 0)
  mw.mfac = h->mfac_wide;
  hipLaunchKernelGGL((k_dump_wide<TASK>), dim3(1), dim3(64), 0, st, mw, h->st, env, ctrl, out);
}
template <int TASK> const WideOps* wide_ops() {
  static const WideOps ops = {[](int device) { return resident_slots(k_step_wide<TASK, false, false>, device); },
                              launch_wide<TASK>, launch_dump_wide<TASK>};
  return &ops;
}
template const WideOps* wide_ops<AW_TASK_TU>();

#else  // the fast tier

#ifdef AW_STAGE_PROF
// the stage profiler's counters, next to the kernels that write them, and their way out
__device__ unsigned long long g_stage_prof[AW_NPROF];
hipError_t stage_prof_read(unsigned long long* out, int reset) {
  hipError_t e = hipSuccess;
  if (out) e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_stage_prof), sizeof(unsigned long long) * AW_NPROF);
  if (reset && e == hipSuccess) {
    unsigned long long z[AW_NPROF] = {};
    e = hipMemcpyToSymbol(HIP_SYMBOL(g_stage_prof), z, sizeof(z));
  }
  return e;
}
#endif

// The next env for a persistent k_step workgroup, XCD-aware.  Workgroups b and b + 8 share an XCD
// (round-robin dispatch, MI355X_MICROARCH.md -- for speed only, correctness never depends on it),
// so workgroup class c = b % 8 owns envs [n c / 8, n (c + 1) / 8): its first round takes the class's
// first gridDim.x / 8 envs, the rest are claimed from the class's own counter.  Neighbouring envs,
// whose rows share 32-byte sectors (state and obs rows, the 1- and 4-byte per-env scalars), are then
// written through ONE L2, where the partial sectors merge before write-back: k_step's HBM traffic
// 1.81 -> 1.30 KB per env-step (r04p, raw counters).  A class whose range is exhausted claims from
// the next classes, so the tail stays balanced.  Returns n when every class is exhausted.
AW_DEV int claim_env(int* next_env, int n, int lane) {
  const int c0 = blockIdx.x & 7, share = gridDim.x >> 3;
  for (int t = 0; t < 8; t++) {
    const int c = (c0 + t) & 7;
    const int lo = (int)((long long)n * c / 8), hi = (int)((long long)n * (c + 1) / 8);
    if (lo + share >= hi) continue;   // the class's first round covered it
    int k = 0;
    if (lane == 0) k = atomicAdd(next_env + c, 1);
    // readfirstlane: env stays a scalar (SGPR addresses, no per-lane pointer spills)
    const int e = lo + share + __builtin_amdgcn_readfirstlane(k);
    if (e < hi) return e;
  }
  return n;
}

// One launch = one env-step of every env (fast tier).  next_env[0..7]: the per-XCD claim
// counters, next_env[8..]: the wide-tier queue (defer_env).  One kernel per (task, sensors, data).
template <int TASK, bool SENS, bool DATA>
__global__ void __launch_bounds__(64) AW_KSTEP_ATTR k_step(DModel mval, const DModel* __restrict__ mptr, DState stval,
                                             int n, const float* __restrict__ actions,
                                             float* obs, float* reward, uint8_t* done, uint8_t* goal,
                                             float* terminal_obs, int autoreset, uint64_t seed,
                                             int* __restrict__ next_env) {
  // model scalars read from the device copy on demand (scalar loads behind the loop's memory
  // clobber) instead of ~50 kernel-argument SGPRs held live across the whole launch
  const DModel& m = *mptr;
  (void)mval;
  // the state pointers read from the device header where they are used (the loop's memory
  // clobber forces the reload) instead of ~30 SGPRs of kernel arguments live across the launch
  const DState& st = *reinterpret_cast<const DState*>(mptr + 1);   // DState follows DModel in the header
  (void)stval;
  __shared__ Env s;
  __shared__ StepIO io;
  const int lane = threadIdx.x;
  park_io(io, lane, actions, obs, reward, done, goal, terminal_obs, autoreset, seed, next_env + 8);
  const bool xmap = (int)gridDim.x < n && (gridDim.x & 7) == 0;
  // claim positions map to envs through k_order's permutation (same XCD class, costliest first:
  // the launch's last claims are its cheapest envs, r05 A/B -0.3 % random, -2.9 % DAPG)
  if (lane == 0) {
    io.cost = xmap ? reinterpret_cast<unsigned*>(next_env + 10 + n) : nullptr;
    io.perm = xmap ? next_env + 10 + 2 * n : nullptr;
  }
  wsync();
  auto env_of = [&](int pos) {
    if (!io.perm) return pos;
    const int e = io.perm[pos];
    return (unsigned)e < (unsigned)n ? e : pos;
  };
  // Persistent workgroups: the grid is one workgroup per resident slot (launch_step); each takes
  // a first env, then the next unclaimed ones from the launch's counters, so the per-slot spill
  // block (s.slot) is rewritten in the XCD's L2 instead of streaming a per-env block to memory.
  // Envs go out in XCD-contiguous ranges (claim_env above); grids that are not a multiple of 8
  // workgroups (AW_STEP_GRID) take env blockIdx.x first and then claim from one counter.  Every
  // workgroup exits once the counters pass n.
  int env = xmap ? (int)((long long)n * (blockIdx.x & 7) / 8) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  if (xmap && env >= (int)((long long)n * ((blockIdx.x & 7) + 1) / 8)) env = claim_env(next_env, n, lane);
  while (env < n) {
    env_step<TASK, SENS, DATA>(m, s, st, env_of(env), lane, io);
    if ((int)gridDim.x >= n) break;            // one env per workgroup: no counter
    int claim = 0;
    if (xmap) {
      env = claim_env(next_env, n, lane);
      continue;
    }
    if (lane == 0) claim = atomicAdd(next_env, 1);
    // readfirstlane, not a shuffle: env stays a scalar, so the addresses formed from it are
    // SGPR values instead of per-lane 64-bit VGPR pairs spilled to scratch once per env
    env = (int)gridDim.x + __builtin_amdgcn_readfirstlane(claim);
  }
}

// The tail of every kernel that leaves an env in a new state (k_reset, k_set_state, k_set_state_ids):
// the forward, the state stored, an env that overflows the fast capacities handed to the wide tier
// (which finishes it), else the sensors, the mjData views, the obs row and the status.
template <int TASK>
AW_DEV void finish_forward(const DModel& m, Env& s, const DState& st, int env, int lane, float* obs, int* defer) {
  constexpr int NV = Tree<TASK>::NV;
  float Mrow[NV];
  Dof d;
  forward<TASK>(m, s, lane, Mrow, d);
  store_env<NV>(m, s, st, env, lane);
  if (fast_overflow(m, s)) {
    if (lane == 0) { st.status[env] = s.status & ~ST_OVF; st.status_acc[env] |= s.status & ~ST_OVF; }
    defer_env(defer, env, DK_FORWARD, lane);
    return;
  }
  if (SENSTAB()->out) stage_sensors(m, s, lane, env);
  if (DATATAB()->groups) stage_data(m, s, lane, env, d.qacc, d.qfrc_con);
  if (obs) write_obs(m, s, lane, obs + (size_t)env * m.obs_dim);
  if (lane == 0) { st.status[env] = s.status; st.status_acc[env] |= s.status; }
}

template <int TASK>
__global__ void __launch_bounds__(64) k_reset(DModel m, DState st, int n, const uint8_t* mask,
                                              const float* params, uint64_t seed, float* obs, int* defer) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= n) return;
  if (mask && !mask[env]) return;
  if (lane == 0) { s.status = 0u; s.slot = blockIdx.x; }
  reset_prepare<NV>(m, s, st, env, lane, params, seed);
  finish_forward<TASK>(m, s, st, env, lane, obs, defer);
}

// Env `env` takes row `row` of the non-null inputs and runs the forward (k_set_state: env = row =
// blockIdx.x; k_set_state_ids: a selected pair).  Both kernels run these statements in this order,
// so a selected env ends bit for bit where k_set_state would leave it.  ep_len_in / ep_ret_in /
// ep_goal_in (aw_clone_envs with episode != 0) replace the env's running-episode counters by row
// `row` of those arrays; else reset_episode zeroes them as reset_prepare does.  The finished-episode
// count, the last-episode stats and the totals are never written.
template <int TASK>
AW_DEV void set_state_body(const DModel& m, Env& s, const DState& st, int env, int row, int lane, const float* qpos,
                           const float* qvel, const float* warm, const float* params, const int* ep_len_in,
                           const float* ep_ret_in, const int* ep_goal_in, int reset_episode, float* obs, int* defer) {
  constexpr int NV = Tree<TASK>::NV;
  load_env<NV>(m, s, st, env, lane);
  if (lane < NV) {
    if (qpos) s.qpos[lane] = qpos[(size_t)row * m.nq + lane];
    if (qvel) s.qvel[lane] = qvel[(size_t)row * m.nv + lane];
    if (warm) s.warm[lane] = warm[(size_t)row * m.nv + lane];
  }
  if (params && lane < m.nparam) st.params[(size_t)env * m.nparam + lane] = params[(size_t)row * m.nparam + lane];
  if (lane == 0) {
    if (ep_len_in) { st.ep_len[env] = ep_len_in[row]; st.ep_ret[env] = ep_ret_in[row]; st.ep_goal[env] = ep_goal_in[row]; }
    else if (reset_episode) { st.ep_len[env] = 0; st.ep_ret[env] = 0.f; st.ep_goal[env] = 0; }
  }
  __threadfence_block();
  wsync();
  if (lane < m.nu) s.ctrl[lane] = 0.f;
  stage_model(m, s, st.params + (size_t)env * m.nparam, lane);
  finish_forward<TASK>(m, s, st, env, lane, obs, defer);
}

// every env from its own row; reads no id array and leaves the episode counters alone
template <int TASK>
__global__ void __launch_bounds__(64) k_set_state(DModel m, DState st, int n, const float* qpos, const float* qvel,
                                                  const float* warm, const float* params, float* obs, int* defer) {
  __shared__ Env s;
  const int env = blockIdx.x, lane = threadIdx.x;
  if (env >= n) return;
  set_state_body<TASK>(m, s, st, env, env, lane, qpos, qvel, warm, params, nullptr, nullptr, nullptr, 0, obs, defer);
}

// a subset (aw_set_state_ids, aw_clone_envs): workgroup k sets env env_ids[k] from row rows[k] (rows ==
// nullptr: row row0 + k).  env and row are wave-uniform scalars (readfirstlane, as claim_env's
// result is): the addresses formed from them stay in SGPRs.  A pair whose env is outside [0, n),
// whose row is outside [0, n_rows) or (also_ids != nullptr: aw_clone_envs' source ids) whose
// also_ids[k] is outside [0, n) returns before it has written anything.  The grid is at most n
// workgroups (launch_set_ids): s.slot = blockIdx.x stays inside the per-env spill blocks and the
// deferred envs inside the wide queue.
template <int TASK>
__global__ void __launch_bounds__(64) k_set_state_ids(DModel m, DState st, int n, const int* __restrict__ env_ids,
                                                      const int* __restrict__ rows, const int* __restrict__ also_ids,
                                                      int row0, int n_rows, const float* qpos, const float* qvel,
                                                      const float* warm, const float* params, const int* ep_len_in,
                                                      const float* ep_ret_in, const int* ep_goal_in, int reset_episode,
                                                      float* obs, int* defer) {
  __shared__ Env s;
  const int lane = threadIdx.x;
  const int env = __builtin_amdgcn_readfirstlane(env_ids[blockIdx.x]);
  const int row = rows ? __builtin_amdgcn_readfirstlane(rows[blockIdx.x]) : row0 + (int)blockIdx.x;
  if ((unsigned)env >= (unsigned)n || (unsigned)row >= (unsigned)n_rows) return;
  if (also_ids && (unsigned)__builtin_amdgcn_readfirstlane(also_ids[blockIdx.x]) >= (unsigned)n) return;
  set_state_body<TASK>(m, s, st, env, row, lane, qpos, qvel, warm, params, ep_len_in, ep_ret_in, ep_goal_in,
                       reset_episode, obs, defer);
}

// What the render kernels share.  stage_pose: wave 0 brings env's pose into LDS (qpos, the model rows
// of its params, the kinematics) before the block's first barrier.  view_cam: a view's world record
// composed into LDS and, behind one barrier, held in scalar registers (it is uniform over the block, as
// k_rgb's kernel argument is).  Every barrier of a view loop is uniform: nviews is a kernel argument
// and an early return takes the whole block.
template <int NV>
AW_DEV void stage_pose(const DModel& m, Env& s, const DState& st, int env, int lane) {
  if (lane < NV) { s.qpos[lane] = st.qpos[(size_t)env * m.nq + lane]; s.qlo[lane] = 0.f; }
  wsync();
  stage_model(m, s, st.params + (size_t)env * m.nparam, lane);
  stage_kinematics(m, s, lane);
}
AW_DEV void view_cam(const Env& s, const float* rec, int body, float* lcam, int tid, float (&cam)[AW_CAM_FLOATS]) {
  compose_view(s, rec, body, lcam, tid);
  __syncthreads();
  for (int k = 0; k < AW_CAM_FLOATS; k++)
    cam[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, lcam[k])));
}

// depth frame of every env's current state: wave 0 runs the kinematics, then all four waves
// cast the pixels (one workgroup per env; render geom poses staged in LDS)
template <int TASK>
__global__ void __launch_bounds__(256) k_depth(DModel m, DState st, int n, CamRec cam, int W, int H, float* out) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  __shared__ RGeoms rg;
  const int env = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (env >= n) return;
  if (tid < 64) stage_pose<NV>(m, s, st, env, lane);
  __syncthreads();
  render_geoms(m, s, rg, cam.c, tid, 256);
  __syncthreads();
  float* o = out + (size_t)env * W * H;
  for (int p0 = (tid >> 6) * 64; p0 < W * H; p0 += 256) render_span(rg, m.nrgeom, cam.c, W, H, p0, lane, o);
}

// colour frame (and optionally the aligned depth frame) of every env's current state: k_depth's
// structure, with the visible sites, the env's colour table and the lights staged next to the
// geom poses; each wave shades 64-pixel spans (aw_render.h render_span_rgb)
template <int TASK>
__global__ void __launch_bounds__(256) k_rgb(DModel m, DState st, int n, CamRec cam, LookRec look, int W, int H, int ss,
                                             unsigned char* out, int dwords, float* depth) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  __shared__ RGeoms rg;
  __shared__ RColors rc;
  const int env = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (env >= n) return;
  if (tid < 64) stage_pose<NV>(m, s, st, env, lane);
  __syncthreads();
  render_geoms(m, s, rg, cam.c, tid, 256);
  render_sites(m, s, rg, cam.c, tid, 256);
  render_colors(m, s, rc, cam.c, look.c, tid, 256);
  __syncthreads();
  unsigned char* o = out + (size_t)env * W * H * 3;
  float* z = depth ? depth + (size_t)env * W * H : nullptr;
  for (int p0 = (tid >> 6) * 64; p0 < W * H; p0 += 256)
    render_span_rgb(rg, rc, m.nrgeom, m.nrsite, cam.c, look.c, W, H, ss, p0, lane, tid >> 6, o, dwords != 0, z);
}

// several cameras per launch, each in the frame of a body, optionally one record per env and view
// (aw_render_views): k_rgb's (RGB) or k_depth's structure with the staging and the kinematics done
// once per env, then per view the camera (view_cam), the pixel boxes and the headlight rebuilt
// against it and the spans cast.  The aw_render.h functions are the ones k_depth / k_rgb call, so a
// world-frame view writes their frames bit for bit.  dwords: rgb_dwords.
struct NoLds {};   // the LDS block an instantiation does not have
template <int TASK, bool RGB>
__global__ void __launch_bounds__(256) k_views(DModel m, DState st, int n, ViewsRec views, int nviews,
                                               const float* __restrict__ env_cam, LookRec look, int W, int H, int ss,
                                               unsigned char* out, int dwords, float* depth) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  __shared__ RGeoms rg;
  __shared__ std::conditional_t<RGB, RColors, NoLds> rc;
  __shared__ float lcam[AW_CAM_FLOATS];
  const int env = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (env >= n) return;
  if (tid < 64) stage_pose<NV>(m, s, st, env, lane);
  __syncthreads();
  if constexpr (RGB) render_colors_env(m, s, rc, look.c, tid, 256);
  const size_t np = (size_t)W * H;
  for (int v = 0; v < nviews; v++) {
    const size_t frame = (size_t)env * nviews + v;
    float cam[AW_CAM_FLOATS];
    view_cam(s, env_cam ? env_cam + frame * AW_CAM_FLOATS : views.c[v], views.body[v], lcam, tid, cam);
    render_geoms(m, s, rg, cam, tid, 256);
    if constexpr (RGB) {
      render_sites(m, s, rg, cam, tid, 256);
      render_headlight(rc, cam, look.c, tid);
    }
    __syncthreads();
    float* z = depth ? depth + frame * np : nullptr;
    for (int p0 = (tid >> 6) * 64; p0 < W * H; p0 += 256) {
      if constexpr (RGB)
        render_span_rgb(rg, rc, m.nrgeom, m.nrsite, cam, look.c, W, H, ss, p0, lane, tid >> 6, out + frame * np * 3,
                        dwords != 0, z);
      else
        render_span(rg, m.nrgeom, cam, W, H, p0, lane, z);
    }
    __syncthreads();   // the next view overwrites cam, the boxes and the headlight
  }
}

// k_views<TASK, true> with the handle's appearance state (aw_set_appearance).  A kernel of its own,
// not a second wrapper over one body: with the view loop in a shared inlined body the depth and the
// shadow frames measured 1-2 % slower than from these two copies.  What differs from
// k_views: APP: env e's colour and light records come from app.col + e ne COL_W / app.light + e
// nlight LIGHT_W and its look from app.look + e AW_LOOK_FLOATS, each where the pointer is given
// (nullptr: the model's records / the launch's host look).  The look row goes through LDS into scalar
// registers once per block, as the camera record does.  SHADOW: shade casts the shadow rays
// (aw_render.h occluded) against the candidates of the lights' occluder grids (RShadow: 10 KiB of
// LDS, built per view behind two more uniform barriers).  waves_per_eu(4): left alone the shadow
// instantiations take 142 VGPRs, three waves per SIMD; capped at 128 (48 bytes of scratch) they run
// four, which is what 39.7 KiB of LDS allows anyway -- 2.68 -> 2.20 ms per 64x64 frame of 8 192
// hammer envs.  The instantiations without shadows take 91 and are not affected.  Whatever the per-env
// records hold, every output index is blockIdx.x, the view and the lane: a workgroup writes only its
// own env's frames.
template <int TASK, bool APP, bool SHADOW>
__global__ void __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(4)))
k_views_app(DModel m, DState st, int n, ViewsRec views, int nviews, const float* __restrict__ env_cam, LookRec look,
            AppRec app, int W, int H, int ss, unsigned char* out, int dwords, float* depth) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  __shared__ RGeoms rg;
  __shared__ RColors rc;
  __shared__ float lcam[AW_CAM_FLOATS];
  __shared__ float llook[AW_LOOK_FLOATS];
  __shared__ std::conditional_t<SHADOW, RShadow, NoLds> sh;
  const int env = blockIdx.x, tid = threadIdx.x, lane = tid & 63;
  if (env >= n) return;
  if (tid < 64) {
    stage_pose<NV>(m, s, st, env, lane);
  } else if (tid < 64 + AW_LOOK_FLOATS) {
    const int k = tid - 64;
    llook[k] = APP && app.look ? app.look[(size_t)env * AW_LOOK_FLOATS + k] : look.c[k];
  }
  __syncthreads();
  float lk[AW_LOOK_FLOATS];
  for (int k = 0; k < AW_LOOK_FLOATS; k++)
    lk[k] = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, llook[k])));
  const int ne = m.nrgeom + m.nrsite;
  render_colors_env(m, s, rc, lk, tid, 256, APP && app.col ? app.col + (size_t)env * ne * COL_W : nullptr,
                    APP && app.light ? app.light + (size_t)env * m.nlight * LIGHT_W : nullptr);
  const size_t np = (size_t)W * H;
  for (int v = 0; v < nviews; v++) {
    const size_t frame = (size_t)env * nviews + v;
    float cam[AW_CAM_FLOATS];
    view_cam(s, env_cam ? env_cam + frame * AW_CAM_FLOATS : views.c[v], views.body[v], lcam, tid, cam);
    render_geoms(m, s, rg, cam, tid, 256);
    render_sites(m, s, rg, cam, tid, 256);
    render_headlight(rc, cam, lk, tid);
    if (SHADOW && !(APP && app.light)) render_castshadow(m, rc, lk, tid);   // (behind view_cam's barrier: staged)
    __syncthreads();
    const RShadow* shp = nullptr;
    if constexpr (SHADOW) {   // the lights' occluder grids over the poses render_geoms just wrote
      shadow_frames(rg, rc, sh, m.nrgeom, tid);
      __syncthreads();
      shadow_cells(rg, rc, sh, m.nrgeom, tid, 256);
      __syncthreads();
      shp = &sh;
    }
    float* z = depth ? depth + frame * np : nullptr;
    for (int p0 = (tid >> 6) * 64; p0 < W * H; p0 += 256)
      render_span_rgb<SHADOW>(rg, rc, m.nrgeom, m.nrsite, cam, lk, W, H, ss, p0, lane, tid >> 6, out + frame * np * 3,
                              dwords != 0, z, shp);
    __syncthreads();   // the next view overwrites cam, the boxes and the headlight
  }
}

// segmentation frames (aw_render_labels): k_views<TASK, false>'s structure, writing one int32 label
// per pixel (aw_render.h render_span_labels) and optionally the depth frame.
// SITES: the visible sites join the entries.  The workgroup renders env env_ids[blockIdx.x] (NULL:
// blockIdx.x) into output row blockIdx.x; an id outside [0, n) is uniform over the block, which
// leaves before its first barrier with its row untouched.  The env id selects what is read (the
// state, the params, env_cam's records); every output index is blockIdx.x, the view and the lane.
// The look-up table travels as a kernel argument and is staged into LDS once.
template <int TASK, bool SITES>
__global__ void __launch_bounds__(256) k_labels(DModel m, DState st, int n, ViewsRec views, int nviews,
                                                const float* __restrict__ env_cam, const int* __restrict__ env_ids,
                                                LutRec lut, int background, int W, int H, int* labels, float* depth) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  __shared__ RGeoms rg;
  __shared__ float lcam[AW_CAM_FLOATS];
  __shared__ int slut[MAXRG];
  const int tid = threadIdx.x, lane = tid & 63;
  const int env = env_ids ? env_ids[blockIdx.x] : (int)blockIdx.x;
  if (env < 0 || env >= n) return;
  if (tid < 64) stage_pose<NV>(m, s, st, env, lane);
  else if (tid < 64 + MAXRG) slut[tid - 64] = lut.v[tid - 64];
  __syncthreads();
  const int ns = SITES ? m.nrsite : 0;
  const size_t np = (size_t)W * H;
  for (int v = 0; v < nviews; v++) {
    const size_t frame = (size_t)blockIdx.x * nviews + v;
    float cam[AW_CAM_FLOATS];
    view_cam(s, env_cam ? env_cam + ((size_t)env * nviews + v) * AW_CAM_FLOATS : views.c[v], views.body[v], lcam, tid,
             cam);
    render_geoms(m, s, rg, cam, tid, 256);
    if constexpr (SITES) render_sites(m, s, rg, cam, tid, 256);
    __syncthreads();
    float* z = depth ? depth + frame * np : nullptr;
    for (int p0 = (tid >> 6) * 64; p0 < W * H; p0 += 256)
      render_span_labels(rg, m.nrgeom, ns, cam, slut, background, W, H, p0, lane, labels + frame * np, z);
    __syncthreads();   // the next view overwrites cam and the boxes
  }
}

// point-cloud candidates (aw_render_cloud): k_labels' structure, keeping, of every pixel that passes
// render_span_cloud (a hit on a kept entry inside the crop box), the world point and the flat pixel
// index v H W + p, compacted in ascending pixel order into the first cap slots of output row
// blockIdx.x.  No atomics: the four waves cast one round of 256 consecutive pixels,
// each ballots its candidates and leaves the popcount in LDS; behind one barrier a candidate's slot
// is the running base (the candidates of all earlier rounds and views, carried identically by every
// thread) + the counts of the lower waves + the candidates on lower lanes.  The counts are double
// buffered by round parity: a wave writes a buffer again two rounds later, past the barrier that
// every wave reaches only after it has read it.  The round loop and all its barriers are uniform
// (a wave whose span starts past the frame contributes 0).  count receives the row's total, which
// may exceed cap; slots past min(total, cap) are not written.  Env selection and the early return of
// an id outside [0, n) are k_labels'.
template <int TASK, bool SITES>
__global__ void __launch_bounds__(256) k_cloud(DModel m, DState st, int n, ViewsRec views, int nviews,
                                               const float* __restrict__ env_cam, const int* __restrict__ env_ids,
                                               CloudRec c, int W, int H, float* xyz, int* pix, int* count) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  __shared__ RGeoms rg;
  __shared__ float lcam[AW_CAM_FLOATS];
  __shared__ int wcnt[2][4];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int env = env_ids ? env_ids[blockIdx.x] : (int)blockIdx.x;
  if (env < 0 || env >= n) return;
  if (tid < 64) stage_pose<NV>(m, s, st, env, lane);
  __syncthreads();
  const int ns = SITES ? m.nrsite : 0;
  const int np = W * H;
  const unsigned long long below = (1ull << lane) - 1ull;
  float* orow = xyz + (size_t)blockIdx.x * c.cap * 3;
  int* prow = pix ? pix + (size_t)blockIdx.x * c.cap : nullptr;
  int base = 0, round = 0;
  for (int v = 0; v < nviews; v++) {
    float cam[AW_CAM_FLOATS];
    view_cam(s, env_cam ? env_cam + ((size_t)env * nviews + v) * AW_CAM_FLOATS : views.c[v], views.body[v], lcam, tid,
             cam);
    render_geoms(m, s, rg, cam, tid, 256);
    if constexpr (SITES) render_sites(m, s, rg, cam, tid, 256);
    __syncthreads();
    for (int r0 = 0; r0 < np; r0 += 256, round++) {
      const int p0 = r0 + wave * 64;
      float pt[3] = {0.f, 0.f, 0.f};
      bool in = false;
      if (p0 < np) in = render_span_cloud(rg, m.nrgeom, ns, cam, c.keep, c.crop ? c.box : nullptr, W, H, p0, lane, pt);
      const unsigned long long mk = __ballot(in);
      if (lane == 0) wcnt[round & 1][wave] = __popcll(mk);
      __syncthreads();
      int slot = base + __popcll(mk & below);
      for (int w = 0; w < 4; w++) {
        const int cw = wcnt[round & 1][w];
        if (w < wave) slot += cw;
        base += cw;
      }
      if (in && slot < c.cap) {
        if (c.frame_body > 0) {   // rot(xquat[b])^T (pt - xpos[b]): the rotation by the conjugate
          const float* q = s.xquat[c.frame_body];
          const float qc[4] = {q[0], -q[1], -q[2], -q[3]};
          float dif[3];
          sub3(dif, pt, s.xpos[c.frame_body]);
          rotvq(pt, dif, qc);
        }
        for (int k = 0; k < 3; k++) orow[(size_t)slot * 3 + k] = pt[k];
        if (prow) prow[slot] = v * np + p0 + lane;
      }
    }
    __syncthreads();   // the next view overwrites cam and the boxes
  }
  if (tid == 0) count[blockIdx.x] = base;
}

// ray queries (aw_cast_rays; aw_rays.h): output row blockIdx.x casts the handle's ray table at env
// env_ids[blockIdx.x] (nullptr: env blockIdx.x); an id outside [0, n) is uniform over the block, which
// leaves before its first barrier with its row untouched.  The block is 64 ceil(R / 64) threads and
// thread r owns ray r: record r of the table (body, xmax and keep always; pnt and vec unless env_rays
// gives the env's own six floats, indexed by ENV id), composed into the world from the body's frame
// (body 0: as given).  A zero or non-finite vec, or a non-finite pnt, is a miss: nothing but floats
// comes from env_rays, and the table's body was checked on the host, so every index is trusted.  The
// direction is normalised after a scaling by its largest component (no under- or overflow of the
// square), the crossing found in metres and divided by |vec|: dist is the x of pnt + x vec.
// Stores: lane r writes dist[row][r] and entry[row][r], contiguous runs per wave, its own row only.
template <int TASK>
__global__ void __launch_bounds__(256) k_rays(DModel m, DState st, int n, const int* __restrict__ env_ids,
                                              const RayRec* __restrict__ rays, int R,
                                              const float* __restrict__ env_rays, float* dist, int* entry) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  __shared__ RayGeoms rg;
  const int tid = threadIdx.x, lane = tid & 63;
  const int env = env_ids ? __builtin_amdgcn_readfirstlane(env_ids[blockIdx.x]) : (int)blockIdx.x;
  if ((unsigned)env >= (unsigned)n) return;
  if (tid < 64) stage_pose<NV>(m, s, st, env, lane);
  __syncthreads();
  ray_geoms(m, s, rg, tid, (int)blockDim.x);
  __syncthreads();
  const bool live = tid < R;
  const RayRec& rec = rays[live ? tid : R - 1];
  const int body = rec.body;
  const float xmax = rec.xmax;
  float pv[6];
  if (env_rays) {
    const float* er = env_rays + ((size_t)env * R + (live ? tid : R - 1)) * 6;
    for (int k = 0; k < 6; k++) pv[k] = er[k];
  } else {
    for (int k = 0; k < 3; k++) { pv[k] = rec.pnt[k]; pv[3 + k] = rec.vec[k]; }
  }
  float o[3], v[3];
  copy3(o, pv);
  copy3(v, pv + 3);
  if (body > 0) {
    rotvq(o, pv, s.xquat[body]);
    add3(o, o, s.xpos[body]);
    rotvq(v, pv + 3, s.xquat[body]);
  }
  const float big = fmaxf(fmaxf(fabsf(v[0]), fabsf(v[1])), fabsf(v[2]));
  const float osum = fabsf(o[0]) + fabsf(o[1]) + fabsf(o[2]);
  const bool ok = live && big > 0.f && big < 3.0e38f && osum < 3.0e38f;   // (a NaN fails every comparison)
  float d[3] = {0.f, 0.f, 1.f}, len = 1.f;
  if (ok) {
    for (int k = 0; k < 3; k++) d[k] = v[k] / big;
    const float nd = sqrtf(dot3(d, d));   // in [1, sqrt 3]
    for (int k = 0; k < 3; k++) d[k] /= nd;
    len = big * nd;
  } else {
    for (int k = 0; k < 3; k++) o[k] = 0.f;
  }
  const float tlim = xmax > 0.f ? 1.001f * (xmax * len) + 1.0e-6f : 3.0e38f;
  int hit;
  const float t = ray_nearest(rg, m.nrgeom, ok ? rec.keep : 0ull, o, d, tlim, hit);
  float x = hit >= 0 ? t / len : -1.f;
  if (!(x >= 0.f) || (xmax > 0.f && x > xmax)) { x = -1.f; hit = -1; }
  if (live) {
    const size_t i = (size_t)blockIdx.x * R + tid;
    dist[i] = x;
    if (entry) entry[i] = hit;
  }
}

// Claim order for the next k_step launch (longest processing time first): per XCD class c (k_step's
// env range [n c / 8, n (c + 1) / 8)) the envs are bucketed by their last env-step's shader cycles
// on a quarter-octave scale and written costliest bucket first into perm (positions of the same
// range), so the launch's last claims are its cheapest envs.  One workgroup per class.
static __device__ int cost_bucket(unsigned c) {
  if (c < (1u << 16)) return 0;
  const int e = 31 - __clz(c);                       // floor(log2 c) >= 16
  const int key = 4 * e + (int)((c >> (e - 2)) & 3);  // quarter octaves
  const int b = key - 4 * 16;
  return b > 63 ? 63 : b;
}
static __global__ void __launch_bounds__(1024) k_order(const unsigned* __restrict__ cost, int* __restrict__ perm, int n) {
  const int c = blockIdx.x;
  const int lo = (int)((long long)n * c / 8), hi = (int)((long long)n * (c + 1) / 8);
  __shared__ int hist[64];
  if (threadIdx.x < 64) hist[threadIdx.x] = 0;
  __syncthreads();
  for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) atomicAdd(&hist[cost_bucket(cost[i])], 1);
  __syncthreads();
  if (threadIdx.x == 0) {
    int acc = 0;
    for (int b = 63; b >= 0; b--) { const int h = hist[b]; hist[b] = acc; acc += h; }
  }
  __syncthreads();
  for (int i = lo + (int)threadIdx.x; i < hi; i += blockDim.x) {
    const int k = atomicAdd(&hist[cost_bucket(cost[i])], 1);
    perm[lo + k] = i;
  }
}

// every launch that runs a fast-tier forward clears the wide queue first and drains it after
static void clear_queue(aw_handle* h, bool counters, hipStream_t st) {
  if (counters) (void)hipMemsetAsync(h->next_env, 0, 10 * sizeof(int), st);   // XCD counters + queue heads
  else (void)hipMemsetAsync(h->next_env + 8, 0, 2 * sizeof(int), st);
}
template <int TASK>
static void launch_step(aw_handle* h, const float* a, float* obs, float* rew, uint8_t* done, uint8_t* goal,
                        float* tobs, int autoreset, uint64_t seed, hipStream_t st) {
  // grid = the handle's persistent slot count (aw_create / aw_set_option), capped at nenv
  const int grid = std::min(h->nenv, h->slots);
  clear_queue(h, grid < h->nenv, st);
  if (grid < h->nenv && (grid & 7) == 0)   // the XCD-class claim path (k_step xmap)
    hipLaunchKernelGGL(k_order, dim3(8), dim3(1024), 0, st, reinterpret_cast<const unsigned*>(h->next_env + 10 + h->nenv),
                       h->next_env + 10 + 2 * h->nenv, h->nenv);
  with_sens_data(h, [&](auto S, auto D) {
    hipLaunchKernelGGL((k_step<TASK, decltype(S)::value, decltype(D)::value>), dim3(grid), dim3(64), 0, st, h->m,
                       (const DModel*)h->dmhdr, h->st, h->nenv, a, obs, rew, done, goal, tobs, autoreset, seed, h->next_env);
  });
  wide_ops<TASK>()->run(h, a, obs, rew, done, goal, tobs, autoreset, seed, st);
}
template <int TASK>
static void launch_reset(aw_handle* h, const uint8_t* mask, const float* params, uint64_t seed, float* obs,
                         hipStream_t st) {
  clear_queue(h, false, st);
  hipLaunchKernelGGL((k_reset<TASK>), dim3(h->nenv), dim3(64), 0, st, h->m, h->st, h->nenv, mask, params, seed, obs,
                     h->next_env + 8);
  wide_ops<TASK>()->run(h, nullptr, obs, nullptr, nullptr, nullptr, nullptr, 0, seed, st);
}
template <int TASK>
static void launch_set(aw_handle* h, const float* q, const float* v, const float* w, const float* p, float* obs,
                       hipStream_t st) {
  clear_queue(h, false, st);
  hipLaunchKernelGGL((k_set_state<TASK>), dim3(h->nenv), dim3(64), 0, st, h->m, h->st, h->nenv, q, v, w, p, obs,
                     h->next_env + 8);
  wide_ops<TASK>()->run(h, nullptr, obs, nullptr, nullptr, nullptr, nullptr, 0, 0, st);
}
// one workgroup per selected pair, at most nenv per launch: a longer list (ids that repeat or lie
// out of range) goes out in pieces, each with its own queue clear and wide-tier drain, so that
// blockIdx.x indexes the per-env spill blocks and the queue never holds more than nenv entries
template <int TASK>
static void launch_set_ids(aw_handle* h, const SetIds& a, float* obs, hipStream_t st) {
  for (int k0 = 0; k0 < a.n_sel; k0 += h->nenv) {
    const int grid = std::min(h->nenv, a.n_sel - k0);
    clear_queue(h, false, st);
    hipLaunchKernelGGL((k_set_state_ids<TASK>), dim3(grid), dim3(64), 0, st, h->m, h->st, h->nenv, a.env_ids + k0,
                       a.rows ? a.rows + k0 : nullptr, a.also_ids ? a.also_ids + k0 : nullptr, k0, a.n_rows, a.qpos,
                       a.qvel, a.warm, a.params, a.ep_len, a.ep_ret, a.ep_goal, a.reset_episode, obs, h->next_env + 8);
    wide_ops<TASK>()->run(h, nullptr, obs, nullptr, nullptr, nullptr, nullptr, 0, 0, st);
  }
}
template <int TASK>
static void launch_dump(aw_handle* h, int env, const float* ctrl, float* out, hipStream_t st) {
  hipLaunchKernelGGL((k_dump<TASK>), dim3(1), dim3(64), 0, st, h->m, h->st, env, ctrl, out);
}

template <int TASK>
static void launch_depth(aw_handle* h, const CamRec& cam, int W, int H, float* out, hipStream_t st) {
  hipLaunchKernelGGL((k_depth<TASK>), dim3(h->nenv), dim3(256), 0, st, h->m, h->st, h->nenv, cam, W, H, out);
}
// whole-dword stores of RGB frames: frame f starts at byte f * 3 W H of rgb, so the frame size and
// the output base both have to be multiples of 4 bytes
static int rgb_dwords(const uint8_t* rgb, int W, int H) {
  return rgb && (3 * (size_t)W * H) % 4 == 0 && (uintptr_t)rgb % 4 == 0;
}
template <int TASK>
static void launch_rgb(aw_handle* h, const CamRec& cam, const LookRec& look, int W, int H, int ss, uint8_t* rgb,
                       float* depth, hipStream_t st) {
  hipLaunchKernelGGL((k_rgb<TASK>), dim3(h->nenv), dim3(256), 0, st, h->m, h->st, h->nenv, cam, look, W, H, ss, rgb,
                     rgb_dwords(rgb, W, H), depth);
}
// depth only: k_views<TASK, false>; RGB: k_views<TASK, true>, or while the handle holds per-env
// tables and / or casts shadows (has_appearance) the k_views_app instantiation of that state
template <int TASK>
static void launch_views(aw_handle* h, const ViewsRec& views, int nviews, const float* env_cam, const LookRec& look,
                         int W, int H, int ss, uint8_t* rgb, float* depth, hipStream_t st) {
  auto go = [&](auto kernel, auto... app) {
    hipLaunchKernelGGL(kernel, dim3(h->nenv), dim3(256), 0, st, h->m, h->st, h->nenv, views, nviews, env_cam, look,
                       app..., W, H, ss, rgb, rgb_dwords(rgb, W, H), depth);
  };
  if (!rgb) go(k_views<TASK, false>);
  else if (!has_appearance(h)) go(k_views<TASK, true>);
  else if (!h->shadows) go(k_views_app<TASK, true, false>, h->app);
  else if (h->app.any()) go(k_views_app<TASK, true, true>, h->app);
  else go(k_views_app<TASK, false, true>, h->app);
}
// grid: the output rows (the selected envs, or all of them)
template <int TASK>
static void launch_labels(aw_handle* h, const ViewsRec& views, int nviews, const float* env_cam, const int32_t* env_ids,
                          int grid, const LutRec& lut, int32_t background, int sites, int W, int H, int32_t* labels,
                          float* depth, hipStream_t st) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, h->m, h->st, h->nenv, views, nviews, env_cam, env_ids, lut,
                       background, W, H, labels, depth);
  };
  sites ? go(k_labels<TASK, true>) : go(k_labels<TASK, false>);
}
template <int TASK>
static void launch_cloud(aw_handle* h, const ViewsRec& views, int nviews, const float* env_cam, const int32_t* env_ids,
                         int grid, const CloudRec& c, int sites, int W, int H, float* xyz, int32_t* pix, int32_t* count,
                         hipStream_t st) {
  auto go = [&](auto kernel) {
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(256), 0, st, h->m, h->st, h->nenv, views, nviews, env_cam, env_ids, c, W,
                       H, xyz, pix, count);
  };
  sites ? go(k_cloud<TASK, true>) : go(k_cloud<TASK, false>);
}
// grid: the output rows (the selected envs, or all of them)
template <int TASK>
static void launch_dyn(aw_handle* h, const int32_t* env_ids, int grid, const DynPts& pts, int npoints, const float* qpos,
                       const float* qvel, const float* ctrl, const aw_dyn_out& out, hipStream_t st) {
  hipLaunchKernelGGL((k_dyn<TASK>), dim3(grid), dim3(64), 0, st, h->m, h->st, h->nenv, env_ids, pts, npoints, qpos, qvel,
                     ctrl, out);
}
// grid: the output rows (the selected envs, or all of them); block: one thread per ray, whole waves
template <int TASK>
static void launch_rays(aw_handle* h, const int32_t* env_ids, int grid, const float* env_rays, float* dist,
                        int32_t* entry, hipStream_t st) {
  hipLaunchKernelGGL((k_rays<TASK>), dim3(grid), dim3(64 * ((h->nrays + 63) / 64)), 0, st, h->m, h->st, h->nenv, env_ids,
                     (const RayRec*)h->rays, h->nrays, env_rays, dist, entry);
}
// grid: the output rows (the selected envs, or all of them)
template <int TASK>
static void launch_ik(aw_handle* h, const int32_t* env_ids, int grid, const IkTgt& tg, int ntargets, int mrows,
                      uint64_t dof_mask, const float* goal, const float* qpos0, const aw_ik_opt& opt, const aw_ik_out& out,
                      hipStream_t st) {
  hipLaunchKernelGGL((k_ik<TASK>), dim3(grid), dim3(64), 0, st, h->m, h->st, h->nenv, env_ids, tg, ntargets, mrows,
                     (unsigned long long)dof_mask, goal, qpos0, opt, out);
}
template <int TASK> const TaskOps* task_ops() {
  static const TaskOps ops = {[](int device) { return resident_slots(k_step<TASK, false, false>, device); },  // the persistent grid
                              launch_step<TASK>, launch_reset<TASK>, launch_set<TASK>, launch_set_ids<TASK>,
                              launch_dump<TASK>, launch_depth<TASK>, launch_rgb<TASK>, launch_views<TASK>,
                              launch_labels<TASK>, launch_cloud<TASK>, launch_dyn<TASK>, launch_rays<TASK>, launch_ik<TASK>};
  return &ops;
}
template const TaskOps* task_ops<AW_TASK_TU>();
#endif  // AW_WIDE
