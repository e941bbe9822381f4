// aw_step.h -- the env-step on the wave, device code only: collision, mj_forward, mj_Euler, the
// state checks, the reset and env_step, which the kernels of aw_kernels.hip run (both capacity
// tiers: the same code, shaped by aw_common.h's capacities).
//
// One workgroup = one 64-lane wave = one env.  A step launch runs frame_skip x mj_step
// (forward + Euler) and the task layer for every env; the per-env working set stays in LDS /
// VGPRs for the whole launch, so HBM traffic is the compulsory state + action + obs bytes.
#pragma once
#include "aw_collide.h"
#include "aw_common.h"
#include "aw_dynamics.h"
#include "aw_handle.h"   // DState
#include "aw_solver.h"
#include "aw_task.h"
#include "aw_tree.h"

// k_step is allocated for two waves per SIMD (<= 256 VGPRs): its LDS footprint (< 20 KiB)
// already admits 8 envs per CU, and the register allocator left alone would take 350+
#ifndef AW_KSTEP_ATTR
#define AW_KSTEP_ATTR __attribute__((amdgpu_waves_per_eu(2, 2)))
#endif

#ifndef AW_ENV_LANE
// opaque env-level lane ids: per-lane state / obs addresses are formed where they are used, not
// once per env and spilled.  With the env index scalar (readfirstlane claim) this takes k_step's
// scratch 280 -> 92 B/lane and its HBM traffic 7.9 -> 1.7 KB per env-step, +1.7 % (DAPG +2.1 %,
// A/B r03za); -DAW_ENV_LANE= (plain lane ids) restores the old form.
#define AW_ENV_LANE(x) opaque(x)
#endif

// ---------------------------------------------------------------------------------------
// contacts -> (pair, emission) key order: rank of each key among the n keys (keys are unique),
// then a scatter to that slot; normals are normalised on the way
AW_DEV void sort_contacts(Env& s, int lane) {
  int n = s.ncon;
  if (n > MAXCON) n = MAXCON;
  // lane = contact, in chunks of 64 (the wide tier's 100 contacts take two)
  int key[NCH], rank[NCH], pair[NCH];
  float dist[NCH], pos[NCH][3], nrm[NCH][3];
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int c = lane + 64 * h;
    key[h] = c < n ? s.con_key[c] : 0x7fffffff;
    rank[h] = 0;
  }
  if constexpr (NCH == 1) {
    for (int j = 0; j < n; j++) rank[0] += rlane_i(key[0], j) < key[0] ? 1 : 0;
  } else {
    for (int j = 0; j < n; j++) {
      const int kj = s.con_key[j];
#pragma unroll
      for (int h = 0; h < NCH; h++) rank[h] += kj < key[h] ? 1 : 0;
    }
  }
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    const int c = lane + 64 * h;
    dist[h] = 0.f;
    pair[h] = 0;
    for (int k = 0; k < 3; k++) pos[h][k] = nrm[h][k] = 0.f;
    if (c < n) {
      dist[h] = s.con_dist[c];
      pair[h] = s.con_pair[c];
      for (int k = 0; k < 3; k++) { pos[h][k] = s.con_pos[c][k]; nrm[h][k] = s.con_nrm[c][k]; }
    }
  }
  wsync();
#pragma unroll
  for (int h = 0; h < NCH; h++) {
    if (lane + 64 * h < n) {
      const int r = rank[h];
      s.con_key[r] = key[h];
      s.con_dist[r] = dist[h];
      s.con_pair[r] = pair[h];
      copy3(s.con_pos[r], pos[h]);
      normalize3(nrm[h]);         // mju_makeFrame's first step; tangents are rebuilt where used
      copy3(s.con_nrm[r], nrm[h]);
    }
  }
  if (lane == 0) {
    s.ncon = n - (int)s.kin64_mask;   // fp64-dropped candidates sorted last (stage_collision)
    // the wide tier's nconmax applies to the decided contacts, in pair order (mj_collision)
    if (s.ncon > CON_CAP) { s.ncon = CON_CAP; s.status |= ST_CON_OVERFLOW; }
  }
  wsync();
}

// Midphase of collider class C (2, 3, 4), lane per pair: a pair whose geoms provably stay farther
// apart than margin + 1e-4 (aw_collide.h *_may_touch: exact lower bounds on the distance) emits
// nothing in its collider either and is dropped; the survivors are compacted in place at the
// front of the class's slice of the list.  Returns their count.
template <int C>
AW_DEV int midphase(const DModel& m, Env& s, short* list, int cnt, int lane) {
  int nsurv = 0;
  const unsigned long long below = (1ull << lane) - 1ull;
  for (int base = 0; base < cnt; base += 64) {
    const int i = base + lane;
    const int pair = i < cnt ? list[i] : 0;
    bool keep = false;
    if (i < cnt) {
      if constexpr (C == 2) keep = capbox_may_touch(m, s, pair);
      else if constexpr (C == 3) keep = boxbox_may_touch(m, s, pair);
      else keep = mpr_may_touch(m, s, pair);
    }
    const unsigned long long mask = __ballot(keep);
    wsync();
    if (keep) list[nsurv + __popcll(mask & below)] = (short)pair;
    nsurv += __popcll(mask);
    wsync();
  }
  return nsurv;
}

// narrowphase over the broadphase survivors of one collider class
template <int C>
AW_DEV void narrow_class(const DModel& m, Env& s, const short* plist, int cnt, int lane) {
  const int st = m.cls_start[C];
  if constexpr (C == 2) {
    // sphere / capsule - box: midphase, then one survivor per 16-lane DPP row, four per round
    // (capsule-box's 43-candidate minimiser search is spread over the row, capbox_tstar_row)
    short* list = const_cast<short*>(plist) + st;
    const int nsurv = midphase<C>(m, s, list, cnt, lane);
    for (int i0 = 0; i0 < nsurv; i0 += 4) {
      const int i = i0 + (lane >> 4);
      if (i < nsurv) collide_pair<C>(m, s, list[i], lane & 15);
    }
  } else if constexpr (C == 3) {
    short* list = const_cast<short*>(plist) + st;
    const int nsurv = midphase<C>(m, s, list, cnt, lane);
    for (int i = lane; i < nsurv; i += 64) collide_pair<C>(m, s, list[i]);
  } else if constexpr (C == 4) {
    // MPR: two lanes per pair (aw_collide.h swap_pair), 32 pairs per round
    for (int i0 = 0; i0 < cnt; i0 += 32) {
      const int i = i0 + (lane >> 1);
      if (i < cnt) collide_pair<C>(m, s, plist[st + i], lane & 1);
    }
  } else {
    for (int i = lane; i < cnt; i += 64) collide_pair<C>(m, s, plist[st + i]);
  }
}

// mj_collision: bounding-sphere broadphase over the static candidate list (one pair per lane,
// 64 per round), survivors compacted class-major into an LDS list (ballot + mbcnt), then ONE
// narrowphase loop over the list: lanes of a round mostly share a collider, instead of every
// round executing every collider branch its lanes happen to need.  MPR pairs (class 4) run on
// fp64 geometry: stage_kin64 computes their bodies' frames once the broadphase has kept one.
AW_DEV void stage_collision(const DModel& m, Env& s, int lane) {
  if (lane == 0) s.ncon = 0;
  wsync();
  if (!(m.disableflags & (DSBL_CONSTRAINT | DSBL_CONTACT))) {
    short* plist = reinterpret_cast<short*>(&s.J[0][0]);   // dense J rows are dead until stage_constraints
    int cnt[NCLASS];
#pragma unroll
    for (int c = 0; c < NCLASS; c++) cnt[c] = 0;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int base = 0; base < m.npairall; base += 64) {   // rounds of 64 pairs
      const int p = base + lane;
      bool pass = false;
      int cls = -1;
      if (p < m.npairall) {
        const int pk = MD(cp_pack, p);
        const float rb = MD(cp_rb, p);
        cls = pk & 0xff;
        const int g1 = (pk >> 8) & 0xff, g2 = pk >> 16;
        float dif[3];
        sub3(dif, s.gxpos[g2], s.gxpos[g1]);
        if (rb < 0.f) {
          // plane (g1) pair: the other geom's bounding sphere against the plane through the plane
          // geom's centre, normal = its z axis (every plane collider emits only within the margin)
          const float* q = s.gxquat[g1];
          const float n[3] = {2.f * (q[1] * q[3] + q[0] * q[2]), 2.f * (q[2] * q[3] - q[0] * q[1]),
                              1.f - 2.f * (q[1] * q[1] + q[2] * q[2])};
          pass = !(dot3(n, dif) > -rb - 1.f + 1e-4f);
        } else {
          pass = !(dot3(dif, dif) > rb * rb);
        }
      }
#pragma unroll
      for (int c = 0; c < NCLASS; c++) {
        const bool mine = pass && cls == c;
        const unsigned long long mask = __ballot(mine);
        if (mine) plist[m.cls_start[c] + cnt[c] + __popcll(mask & below)] = (short)p;
        cnt[c] += __popcll(mask);
      }
    }
    AW_PROF(s, PR_CO_BROAD);
    wsync();
    narrow_class<0>(m, s, plist, cnt[0], lane);
    AW_PROF(s, PR_CO_C0);
    narrow_class<1>(m, s, plist, cnt[1], lane);
    AW_PROF(s, PR_CO_C1);
    narrow_class<2>(m, s, plist, cnt[2], lane);
    AW_PROF(s, PR_CO_C2);
    narrow_class<3>(m, s, plist, cnt[3], lane);
    AW_PROF(s, PR_CO_C3);
    // contacts of the sphere / capsule classes within DEC_EPS of their margin (aw_collide.h): their
    // activation is decided in fp64 below, so their bodies' fp64 frames are staged with the MPR ones
    wsync();
    const int nc0 = s.ncon < MAXCON ? s.ncon : MAXCON;
    unsigned long long km = 0ull;
    bool und[NCH];
#pragma unroll
    for (int h = 0; h < NCH; h++) {
      const int c = lane + 64 * h;
      und[h] = false;
#if AW_TAIL_HEADS
      // pair 0 for the lanes past the contacts: the three reads are one clause behind con_pair
      const bool cv = c < nc0;
      const int pr0 = s.con_pair[cv ? c : 0];
      const int pr = cv ? pr0 : 0;
      const int cls = MD(cp_pack, pr) & 0xff;
      const float mg = MD(cp_margin, pr);
      const unsigned long long k64 = MD(cp_kin64, pr);
      if (cv) {
        und[h] = (cls == 1 || cls == 2) && fabsf(s.con_dist[c] - mg) <= DEC_EPS;
        if (und[h]) km |= k64;
      }
#else
      if (c < nc0) {
        const int pr = s.con_pair[c];
        const int cls = MD(cp_pack, pr) & 0xff;
        und[h] = (cls == 1 || cls == 2) && fabsf(s.con_dist[c] - MD(cp_margin, pr)) <= DEC_EPS;
        if (und[h]) km |= MD(cp_kin64, pr);
      }
#endif
    }
    // MPR (cylinder) pairs: the midphase first (fp32 frames, exact distance lower bounds), so
    // that only pairs that can touch request fp64 frames and run fp64 MPR (hammer: the upright
    // wall's bounding sphere covers the scene, 5 of its 6 broadphase survivors never touch)
    if (cnt[4] > 0) cnt[4] = midphase<4>(m, s, plist + m.cls_start[4], cnt[4], lane);
    // the surviving MPR pairs' body closures: only those frames are computed in fp64
    for (int i = lane; i < cnt[4]; i += 64) km |= MD(cp_kin64, plist[m.cls_start[4] + i]);
    if (__ballot(km != 0ull)) {
      if (lane == 0) s.kin64_mask = 0ull;
      wsync();
      if (km) atomicOr(&s.kin64_mask, km);
      wsync();
      stage_kin64(m, s, lane);
      AW_PROF(s, PR_CO_KIN64);
#ifdef AW_STAGE_PROF
      const int nc_before = s.ncon;
      AW_PROF_ADD(s, PR_MPR_PAIRS, cnt[4]);
#endif
      if (cnt[4] > 0) narrow_class<4>(m, s, plist, cnt[4], lane);
#ifdef AW_STAGE_PROF
      wsync();
      AW_PROF_ADD(s, PR_MPR_CONTACTS, s.ncon - nc_before);
#endif
      // fp64 activation: drop a candidate beyond its margin (its key moves past every valid key, so
      // the sort puts it last and cuts it), keep the others with their fp64 distance
      int ndrop = 0;
#pragma unroll
      for (int h = 0; h < NCH; h++) {
        const int c = lane + 64 * h;
        bool drop = false;
        if (und[h]) {
          const double d64 = contact_dist64(m, s, c);
          drop = d64 > MD(cp_margin64, s.con_pair[c]);
          if (drop) s.con_key[c] = 0x7fff0000 + c;
          else s.con_dist[c] = (float)d64;
        }
        ndrop += __popcll(__ballot(drop));
      }
      if (lane == 0) s.kin64_mask = (unsigned long long)ndrop;   // handed to the sort (frames are dead)
    } else if (lane == 0) {
      s.kin64_mask = 0ull;
    }
  } else if (lane == 0) {
    s.kin64_mask = 0ull;
  }
  wsync();
  AW_PROF(s, PR_CO_NARROW);
  sort_contacts(s, lane);
}

// lane-local dof vectors of a forward pass (VGPRs; lane = dof)
struct Dof {
  float qacc, qacc_smooth, qfrc_smooth, qfrc_con;
};

// mj_forward: everything up to qacc / forces / sensors; Mrow is left in registers.  Stage order
// follows the LDS overlays (aw_common.h Env): the constraint rows are assembled while the
// phase-K arrays (cdof, subcom) are alive, then the solver phase reuses that storage.
// ROWST (aw_forward_dump only): the Newton solve's final row states (S_*) go to rowst[r]
// touch: evaluate the touch sensors (AW_TOUCH_LAST: only the forwards whose s.touch is read -- the
// env-step's last substep, the reset / DK_FORWARD forward, the dump and test kernels)
#ifndef AW_TOUCH_LAST
#define AW_TOUCH_LAST 1
#endif
template <int TASK, bool ROWST = false>
AW_DEV void forward(const DModel& m, Env& s, int lane, float (&Mrow)[Tree<TASK>::NV], Dof& d, float* rowst = nullptr,
                    bool touch = true) {
  constexpr int NV = Tree<TASK>::NV;
  stage_kinematics(m, s, lane, touch);   // AW_SITES_LAST: sxpos / txmat have the readers s.touch has
  AW_PROF(s, PR_KIN);
  stage_collision(m, s, lane);
  AW_PROF(s, PR_COLL);
  stage_com(m, s, lane);
  AW_PROF(s, PR_COM);
  d.qfrc_smooth = stage_velocity(m, s, lane);
  AW_PROF(s, PR_RNE);
  stage_crb<TASK>(m, s, lane, Mrow);
  AW_PROF(s, PR_CRB);
  if (lane == 0) { s.it_newton = 1000 * NT_EXIT_NOROWS; s.it_noslip = 0; }
  stage_constraints<NV>(m, s, lane);
  AW_PROF(s, PR_CONSTR);
  // qacc_smooth = M \ qfrc_smooth: mj_factorM + mj_solveM over the dof tree (aw_tree.h)
  {
    float row[NV];
#pragma unroll
    for (int k = 0; k < NV; k++) row[k] = Mrow[k];
    float invd;
    tree_factor<TASK>(row, invd, lane);
    // noslip inverts the same M: it reloads this factor instead of factoring again (AW_MFAC_HANDOFF)
    if (AW_MFAC_HANDOFF && s.nefc != 0 && noslip_on(m)) mfac_store<NV>(m, s, lane, row, invd);
    d.qacc_smooth = tree_solve<TASK>(row, invd, d.qfrc_smooth, lane);
  }
  AW_PROF(s, PR_SMOOTH);
  if (s.nefc == 0) {
    d.qacc = d.qacc_smooth;
    d.qfrc_con = 0.f;
  } else {
    float a = 0.f;
    solve_newton<NV, ROWST>(m, s, lane, Mrow, a, d.qfrc_smooth, d.qacc_smooth, rowst);
    AW_PROF(s, PR_NEWTON);
    if (noslip_on(m)) solve_noslip<TASK>(m, s, lane, Mrow, a);
    AW_PROF(s, PR_NOSLIP);
    for (int r = lane; r < s.nefc; r += 64) s.rowbuf[r] = s.efc_force[r];
    wsync();
    float qc = jt_mul<NV>(m, s, lane);
    d.qacc = lane < NV ? a : 0.f;
    d.qfrc_con = lane < NV ? qc : 0.f;
  }
  if (!AW_TOUCH_LAST || touch) stage_touch(m, s, lane);
  AW_PROF(s, PR_JT_TOUCH);
}

// mj_Euler: implicit joint damping (M + h D factored over the dof tree, aw_tree.h),
// semi-implicit positions, warmstart <- qacc
template <int TASK>
AW_DEV void euler(const DModel& m, Env& s, int lane, const float (&Mrow)[Tree<TASK>::NV], const Dof& d) {
  constexpr int NV = Tree<TASK>::NV;
  const float h = m.timestep;
  const bool dmp = !(m.disableflags & (DSBL_EULERDAMP | DSBL_PASSIVE));
  float acc;
  if (dmp) {
    float row[NV];
    const float dd = lane < NV ? h * MD(dof_damping, lane) : 0.f;
#pragma unroll
    for (int k = 0; k < NV; k++) row[k] = Mrow[k] + (k == lane ? dd : 0.f);
    float invd;
    tree_factor<TASK>(row, invd, lane);
    acc = tree_solve<TASK>(row, invd, d.qfrc_smooth + d.qfrc_con, lane);
  } else {
    acc = d.qacc;
  }
  if (lane < NV) {
    float v = s.qvel[lane] + h * acc;
    s.qvel[lane] = v;
#if AW_QPOS_COMP
    // qpos += h v as MuJoCo's fp64 sum: qpos + qlo carries the position to ~2^-48 relative across the
    // env-step's substeps (TwoProduct of h v, TwoSum into qpos, renormalised), so the fp64 consumers
    // (qpos64) see the reference's positions at substeps 2.. instead of a rounding per substep
    const float q = s.qpos[lane], p = h * v, pe = fmaf(h, v, -p);
    const float sm = q + p, bb = sm - q, e = (q - (sm - bb)) + (p - bb);
    const float lo = s.qlo[lane] + (pe + e), hi = sm + lo;
    s.qpos[lane] = hi;
    s.qlo[lane] = lo - (hi - sm);
#else
    s.qpos[lane] += h * v;
#endif
    s.warm[lane] = d.qacc;
  }
  wsync();
}

// mj_resetData on the state: qpos0 (= 0 for these models), qvel, warmstart and ctrl zeroed --
// after a bad-state reset inside an env-step, the remaining substeps run with ctrl = 0, as the
// reference's do_simulation writes ctrl once before its frame_skip mj_step calls
template <int NV>
AW_DEV void reset_state(Env& s, int lane) {
  if (lane < NV) { s.qpos[lane] = 0.f; s.qlo[lane] = 0.f; s.qvel[lane] = 0.f; s.warm[lane] = 0.f; s.ctrl[lane] = 0.f; }
  wsync();
}

AW_DEV bool bad_value(float x) { return !(fabsf(x) <= 1e10f); }

// mj_checkPos / mj_checkVel: bad state -> flag + reset to qpos0 / 0
template <int NV>
AW_DEV void check_state(Env& s, int lane) {
  bool bp = lane < NV && bad_value(s.qpos[lane]);
  bool bv = lane < NV && bad_value(s.qvel[lane]);
  unsigned long long bpm = __ballot(bp), bvm = __ballot(bv);
  if (bpm | bvm) {
    if (lane == 0) s.status |= (bpm ? ST_BADQPOS : 0u) | (bvm ? ST_BADQVEL : 0u);
    reset_state<NV>(s, lane);
  }
}
// mj_checkAcc: bad qacc -> flag + reset; the caller re-runs forward
template <int NV>
AW_DEV bool check_acc(Env& s, int lane, const Dof& d) {
  if (__ballot(lane < NV && bad_value(d.qacc))) {
    if (lane == 0) s.status |= ST_BADQACC;
    reset_state<NV>(s, lane);
    return true;
  }
  return false;
}

// ---------------------------------------------------------------------------------------
template <int NV>
AW_DEV void load_env(const DModel& m, Env& s, const DState& st, int env, int lane) {
  if (lane < NV) {
    s.qpos[lane] = GIN(st.qpos)[(size_t)env * m.nq + lane];
    s.qlo[lane] = 0.f;   // the stored state is fp32: the env-step starts from it exactly
    s.qvel[lane] = GIN(st.qvel)[(size_t)env * m.nv + lane];
    s.warm[lane] = GIN(st.warm)[(size_t)env * m.nv + lane];
  }
  if (lane == 0) { s.status = 0u; s.slot = blockIdx.x; }
}
template <int NV>
AW_DEV void store_env(const DModel& m, Env& s, const DState& st, int env, int lane) {
  if (lane < NV) {
    GOUT(st.qpos)[(size_t)env * m.nq + lane] = s.qpos[lane];
    GOUT(st.qvel)[(size_t)env * m.nv + lane] = s.qvel[lane];
    GOUT(st.warm)[(size_t)env * m.nv + lane] = s.warm[lane];
  }
}

// reset bookkeeping + parameters (given or sampled) + qpos0; forward runs in the caller
template <int NV>
AW_DEV void reset_prepare(const DModel& m, Env& s, const DState& st, int env, int lane,
                          const float* params_in, uint64_t seed) {
  float* prm = st.params + (size_t)env * m.nparam;
  if (lane == 0) {
    if (params_in) {
      for (int p = 0; p < m.nparam; p++) prm[p] = params_in[(size_t)env * m.nparam + p];
    } else {
      float tmp[MAXP];
#pragma unroll
      for (int p = 0; p < MAXP; p++) tmp[p] = p < m.nparam ? prm[p] : 0.f;
      sample_params(m, seed, (uint32_t)(m.env_offset + (unsigned long long)env), (uint32_t)st.episode[env], tmp);
#pragma unroll
      for (int p = 0; p < MAXP; p++)
        if (p < m.nparam) prm[p] = tmp[p];
    }
    st.ep_len[env] = 0;
    st.ep_ret[env] = 0.f;
    st.ep_goal[env] = 0;
  }
  __threadfence_block();
  wsync();
  if (lane < m.nu) s.ctrl[lane] = 0.f;
  reset_state<NV>(s, lane);
  stage_model(m, s, prm, lane);
}

// reset one env in LDS: params (given or sampled), qpos0/0/0, forward, obs
template <int TASK>
AW_DEV void reset_env(const DModel& m, Env& s, const DState& st, int env, int lane,
                      const float* params_in, uint64_t seed, float* obs) {
  constexpr int NV = Tree<TASK>::NV;
  reset_prepare<NV>(m, s, st, env, lane, params_in, seed);
  float Mrow[NV];
  Dof d;
  forward<TASK>(m, s, lane, Mrow, d);
  if (obs) write_obs(m, s, lane, obs + (size_t)env * m.obs_dim);
}

// ---------------------------------------------------------------------------------------
// The wide-tier queue (aw_common.h, two capacity tiers): q[0] = entries, q[1] = the wide kernel's
// claim counter, q[2 + k] = env | kind << 30.  DK_STEP: the whole env-step is re-run from the
// unchanged pre-step state (the fast tier wrote nothing for it); DK_FORWARD: the state, params and
// bookkeeping are written, only mj_forward + obs are re-run (a reset / set_state forward, ctrl 0).
enum { DK_STEP = 0, DK_FORWARD = 1 };
constexpr unsigned ST_OVF = ST_CON_OVERFLOW | ST_EFC_OVERFLOW;
AW_DEV void defer_env(int* q, int env, int kind, int lane) {
  if (lane == 0) {
    const int k = atomicAdd(q, 1);
    q[2 + k] = env | (kind << 30);
  }
}
// fast tier: did the forward just run drop a contact or a row (uniform LDS read)?  (aw_set_tier's
// test mode sends every forward to the wide tier)
AW_DEV bool fast_overflow(const DModel& m, const Env& s) { return !WIDE && ((s.status & ST_OVF) != 0u || m.force_wide); }

// The per-launch I/O of an env-step, parked in LDS by the launching kernel: env_step reads each
// pointer where it is used (the substep loop's memory clobber keeps the reads there), instead of
// ~16 SGPRs of kernel arguments -- and the per-env addresses formed from them -- held live across
// the whole env-step, which the register allocator spilled to scratch once per env (r05h: +2 KB of
// HBM writes per env-step).
struct StepIO {
  const float* actions;
  float *obs, *reward, *terminal_obs;
  uint8_t *done, *goal;
  int* defer;        // fast tier: the wide-tier queue; nullptr in the wide tier
  uint64_t seed;
  int autoreset;
  unsigned* cost;    // per env: shader cycles of its last env-step (k_order's sort key); nullptr: off
  const int* perm;   // claim position -> env (k_order: each XCD class's envs, most expensive first)
  unsigned long long t0;   // this workgroup's current env-step start (s_memtime)
};
// LDS budgets (one wave per workgroup): the fast tier's Env + StepIO inside the 20 480-byte granule
// that gives eight envs per CU (two waves per SIMD); the wide tier's inside 40 KiB (four per CU, one
// wave per SIMD).  A layout change that breaks either is a compile error, not an occupancy surprise.
static_assert(WIDE || sizeof(Env) + sizeof(StepIO) <= 20480, "fast-tier LDS past the two-waves-per-SIMD budget");
static_assert(!WIDE || sizeof(Env) + sizeof(StepIO) <= 40960, "wide-tier LDS past the one-wave-per-SIMD budget");
static_assert(sizeof(((Env*)nullptr)->rowbuf) / sizeof(float) >= 64 * FAST_NRL, "row buffer holds the observation");

AW_DEV void park_io(StepIO& io, int lane, const float* actions, float* obs, float* reward, uint8_t* done,
                    uint8_t* goal, float* terminal_obs, int autoreset, uint64_t seed, int* defer) {
  if (lane == 0) {
    io.actions = actions; io.obs = obs; io.reward = reward; io.terminal_obs = terminal_obs;
    io.done = done; io.goal = goal; io.defer = defer; io.seed = seed; io.autoreset = autoreset;
    io.cost = nullptr; io.perm = nullptr; io.t0 = 0;
  }
  wsync();
}

// One env-step of env `env`: frame_skip x (forward + Euler), task layer, and the auto-reset.
// forward<NV> has exactly ONE inlined call site (the loop below drives substeps, the mj_checkAcc
// retry and the reset forward through it), which keeps the code object small enough for the
// instruction cache.  Fast tier (defer != nullptr): a forward that overflows the fast capacities
// abandons the env-step before anything is written and queues it for the wide tier (or, in the
// reset forward, queues that forward alone).  kind DK_FORWARD (wide tier): only mj_forward + obs of
// the stored state with ctrl 0 -- the reset forward's path through the same loop.
// SENS (aw_set_sensors): a separate instantiation of the step kernels that also evaluates the
// model's sensors (stage_sensors) after the forwards whose s.touch is read; with SENS false the
// env-step is the code it was without them.  DATA (aw_set_data): likewise for the batched mjData
// views (stage_data), at the same places.
template <int TASK, bool SENS, bool DATA>
AW_DEV void env_step(const DModel& m, Env& s, const DState& st, int env, int lane, StepIO& io,
                     int kind = DK_STEP) {
  constexpr int NV = Tree<TASK>::NV;
  wsync();
  AW_PROF_START(s);
  if (lane == 0 && io.cost) io.t0 = __builtin_amdgcn_s_memtime();
  {
    // an opaque lane id here and in the env-step tail below: per-lane state / obs addresses
    // are formed where they are used instead of once per env and spilled to scratch
    const int el = AW_ENV_LANE(lane);
    load_env<NV>(m, s, st, env, el);
    if (WIDE && el == 0) s.status = ST_WIDE;
    if (el < m.nu) {
      float c = 0.f;
      if (kind == DK_STEP) c = MD(act_mid, el) + clampf(GIN(io.actions)[(size_t)env * m.nu + el], -1.f, 1.f) * MD(act_rng, el);
      s.ctrl[el] = c;
    }
    stage_model(m, s, st.params + (size_t)env * m.nparam, el);
  }
  float Mrow[NV];
  Dof d;
  int sub = 0;
  bool resetting = kind == DK_FORWARD, retry = false;
  AW_PROF(s, PR_PRE);
#pragma nounroll
  while (true) {
    // memory clobber: keeps LICM from hoisting the (loop-invariant) model loads of a whole
    // substep out of this loop, which would pin them in registers across every stage
    asm volatile("" ::: "memory");
    // and no lane-dependent value is hoisted out of the loop either (the lane id is re-derived
    // per substep): loop-invariant masks and offsets would otherwise occupy SGPRs / VGPRs across
    // every stage of the substep
    const int sl = opaque(lane);
    if (!resetting && !retry) check_state<NV>(s, sl);
    AW_PROF(s, PR_CHECK);
    // s.touch is read by the observation only: after the last substep (its mj_checkAcc retry
    // included) and after the reset forward
    forward<TASK>(m, s, sl, Mrow, d, nullptr, resetting || sub + 1 >= m.frame_skip);
    if (fast_overflow(m, s)) {
      if (!resetting) {            // nothing of this env-step is written: the wide tier re-runs it
        defer_env(io.defer, env, DK_STEP, sl);
        return;
      }
      break;                       // the reset forward alone goes to the wide tier (below)
    }
    if (resetting) break;
    if (!retry && check_acc<NV>(s, sl, d)) { retry = true; continue; }
    retry = false;
    if constexpr (SENS) {
      // sim.data.sensordata after step(): the last substep's forward (its mj_checkAcc retry included)
      if (sub + 1 >= m.frame_skip) stage_sensors(m, s, sl, env);
    }
    if constexpr (DATA) {
      if (sub + 1 >= m.frame_skip) stage_data(m, s, sl, env, d.qacc, d.qfrc_con);
    }
    euler<TASK>(m, s, sl, Mrow, d);
    AW_PROF(s, PR_EULER);
    AW_PROF_COUNT(s, PR_SUBSTEPS);
    if (++sub < m.frame_skip) continue;
    // env-step complete: observation, reward, episode bookkeeping
    const int tl = AW_ENV_LANE(lane);
    write_obs(m, s, tl, io.obs + (size_t)env * m.obs_dim);
    int term = 0, trunc = 0;
    if (tl == 0) {
      float r;
      int dn, gl;
      task_reward(m, s, &r, &dn, &gl);
      GOUT(io.reward)[env] = r;
      GOUT(io.goal)[env] = (uint8_t)gl;
      int t = GIN(st.ep_len)[env] + 1;
      term = dn;
      trunc = (m.horizon > 0 && t >= m.horizon) ? 1 : 0;
      GOUT(io.done)[env] = (uint8_t)(term | (trunc << 1));
      float ret = GIN(st.ep_ret)[env] + r;
      int gcount = GIN(st.ep_goal)[env] + gl;
      GOUT(st.ep_len)[env] = t;
      GOUT(st.ep_ret)[env] = ret;
      GOUT(st.ep_goal)[env] = gcount;
      GOUT(st.status)[env] = s.status;
      GOUT(st.status_acc)[env] |= s.status;
      if (term || trunc) {
        st.last_ret[env] = ret;
        st.last_goal[env] = gcount;
        st.last_len[env] = t;
        st.episode[env] += 1;
        st.sum_ret[env] += ret;
        st.n_success[env] += gcount > m.success_steps ? 1 : 0;
      }
    }
    store_env<NV>(m, s, st, env, tl);
    AW_PROF(s, PR_TASK);
    const int ended = __builtin_amdgcn_readfirstlane(term | trunc);
    if (!(io.autoreset && ended)) break;
    __threadfence_block();
    if (float* tob = io.terminal_obs)
      for (int o = tl; o < m.obs_dim; o += 64) GOUT(tob)[(size_t)env * m.obs_dim + o] = s.rowbuf[o];
    wsync();
    reset_prepare<NV>(m, s, st, env, tl, nullptr, io.seed);
    if (WIDE && tl == 0) s.status |= ST_WIDE;
    AW_PROF(s, PR_RESET);
    resetting = true;
  }
  if (resetting) {
    const int rl = AW_ENV_LANE(lane);
    store_env<NV>(m, s, st, env, rl);
    if (fast_overflow(m, s)) {
      if (rl == 0) st.status_acc[env] |= s.status & ~ST_OVF;
      defer_env(io.defer, env, DK_FORWARD, rl);
    } else {
      // the reset / set_state forward's sensors replace the ended episode's, aligned with obs
      if constexpr (SENS) stage_sensors(m, s, rl, env);
      if constexpr (DATA) stage_data(m, s, rl, env, d.qacc, d.qfrc_con);
      if (float* ob = io.obs) write_obs(m, s, rl, ob + (size_t)env * m.obs_dim);
      if (rl == 0) {
        st.status_acc[env] |= s.status;
        if (kind == DK_FORWARD) st.status[env] |= s.status;
      }
    }
  }
  // this env-step's cost for the next launch's claim order (k_order)
  if (lane == 0 && io.cost) {
    const unsigned long long dt = __builtin_amdgcn_s_memtime() - io.t0;
    io.cost[env] = dt > 0xffffffffull ? 0xffffffffu : (unsigned)dt;
  }
#ifdef AW_STAGE_PROF
  AW_PROF(s, PR_TASK);
  AW_PROF_COUNT(s, PR_CALLS);
  if (lane == 0)
    for (int i = 0; i < AW_NPROF; i++)
      if (!prof_global(i)) atomicAdd(&g_stage_prof[i], (unsigned long long)s.prof_acc[prof_slot(i)]);
#endif
}
