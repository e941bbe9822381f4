// aw_dyn.h -- dynamics queries (aw_dynamics, k_dyn): Jacobians, velocities, M, inv(M) and the three
// terms of qfrc_smooth for a chosen subset of envs, on demand.  One wave per output row composes the
// forward's own stage functions (aw_dynamics.h stage_model / stage_kinematics / stage_com /
// stage_crb, aw_tree.h tree_factor / tree_inverse) and stores the derived outputs; the step, reset,
// set-state and render kernels call nothing of this file.
//
// Stage order: load_env, the optional qpos / qvel rows, stage_model, stage_kinematics, stage_com, the
// point records, the Jacobians, dyn_comvel (cvel), the velocities, dyn_forces (RNE, passive,
// actuation), stage_crb (after RNE: it overwrites cinert), tree_factor + tree_inverse.  What no
// requested output needs is skipped on wave-uniform tests of the kernel arguments: the velocity stage
// without a velocity or force output, its RNE half without a force output, the M stages without qM /
// qMinv, the factor and the inverse without qMinv.
//
// The velocity stage is stage_velocity's text split at the point where cvel is complete: that
// function returns only passive - bias + actuator and overwrites cvel with the subtree forces, and
// it keeps the signature the step kernels compile against.  The expressions are the same ones on
// the same values, so the three terms sum to its result.
#pragma once
#include "aw_common.h"
#include "aw_dynamics.h"
#include "aw_handle.h"
#include "aw_step.h"
#include "aw_tree.h"

namespace aw {

// (the point table of one launch, DynPts, is a kernel argument as ViewsRec is: aw_handle.h)
// The row's points in LDS: the world position and the body each moves with.  Lane p writes record p
// once; the Jacobian loop then reads record p as a broadcast (every lane the same address), and the
// ancestry test is one bit of body_dofmask[body] -- the dofs of the body and of its ancestors, which
// the model table already holds -- so no parent walk and no per-lane copy of the table.  The records
// live in two constraint-row arrays of Env, which k_dyn never fills (it builds no rows): a __shared__
// block of their own (320 bytes) would lift the kernel from Env's 20 256 bytes past the 20 480-byte
// granule at which eight workgroups share a CU.
static_assert(4 * AW_DYN_MAXPOINTS <= MAXEFC, "point records do not fit the constraint-row arrays");
AW_DEV float* dyn_pos(Env& s, int p) { return s.efc_aref + 4 * p; }
AW_DEV int& dyn_body(Env& s, int p) { return reinterpret_cast<int*>(s.efc_force)[p]; }

// tree prefix sum of per-body 6-vectors by pointer jumping (stage_velocity's tree_prefix): v is lane
// b's local term on entry and arr[b] the sum over b and its ancestors on return; targets in rowbuf
AW_DEV void dyn_tree_prefix(const DModel& m, Env& s, int lane, float (*arr)[6], float (&v)[6]) {
  const bool own = lane > 0 && lane < m.nbody;
  const int b = own ? lane : 0;
  int* tgt = reinterpret_cast<int*>(s.rowbuf);
  int t = own ? MD(body_parentid, b) : -1;
  if (own)
    for (int k = 0; k < 6; k++) arr[b][k] = v[k];
  if (lane < m.nbody) tgt[lane] = t;
  wsync();
  while (__ballot(t >= 0)) {   // at most log2(tree depth) + 1 rounds
    float u[6];
    int tt = -1;
    if (t >= 0) {
      for (int k = 0; k < 6; k++) u[k] = arr[t][k];
      tt = tgt[t];
    }
    wsync();
    if (t >= 0) {
      for (int k = 0; k < 6; k++) { v[k] += u[k]; arr[b][k] = v[k]; }
      tgt[b] = tt;
      t = tt;
    }
    wsync();
  }
}

// mj_comVel: s.cvel[b] for every body (and cacc[0] = -gravity, which dyn_forces starts from)
AW_DEV void dyn_comvel(const DModel& m, Env& s, int lane) {
  if (lane == 0) {
    for (int k = 0; k < 6; k++) { s.cvel[0][k] = 0; s.cacc[0][k] = 0; }
    if (!(m.disableflags & DSBL_GRAVITY)) { s.cacc[0][3] = -m.gravity[0]; s.cacc[0][4] = -m.gravity[1]; s.cacc[0][5] = -m.gravity[2]; }
  }
  wsync();
  const bool own = lane > 0 && lane < m.nbody;
  const int b = own ? lane : 0;
  const int da = MD(body_dofadr, b), dn = own ? MD(body_dofnum, b) : 0;
  float lv[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int k = 0; k < MAXJB; k++)
    if (k < dn) {
      const int j = da + k;
      const float qv = s.qvel[j];
      for (int c = 0; c < 6; c++) lv[c] = fmaf(s.cdof[j][c], qv, lv[c]);
    }
  dyn_tree_prefix(m, s, lane, s.cvel, lv);
}

// mj_rne (flg_acc = 0), mj_passive, mj_fwdActuation after dyn_comvel: the three terms of
// qfrc_smooth = pas - bias + act, lane = dof (lanes >= nv: zeros).  Overwrites cvel and cacc.
struct DynFrc {
  float bias, pas, act;
};
AW_DEV DynFrc dyn_forces(const DModel& m, Env& s, int lane) {
  float (*cvel)[6] = s.cvel;
  float (*cacc)[6] = s.cacc;
  {
    const bool own = lane > 0 && lane < m.nbody;
    const int b = own ? lane : 0;
    const int p = own ? MD(body_parentid, b) : 0, da = MD(body_dofadr, b), dn = own ? MD(body_dofnum, b) : 0;
    float w[6], la[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    for (int c = 0; c < 6; c++) w[c] = cvel[p][c];
#pragma unroll
    for (int k = 0; k < MAXJB; k++)
      if (k < dn) {
        const int j = da + k;
        float cd[6], cdd[6];
        const float qv = s.qvel[j];
        for (int c = 0; c < 6; c++) cd[c] = s.cdof[j][c];
        cross_motion(cdd, w, cd);
        for (int c = 0; c < 6; c++) { la[c] = fmaf(cdd[c], qv, la[c]); w[c] = fmaf(cd[c], qv, w[c]); }
      }
    dyn_tree_prefix(m, s, lane, cacc, la);
  }
  // local body force: cinert*cacc + cvel x* (cinert*cvel), written over cacc
  for (int b = 1 + lane; b < m.nbody; b += 64) {
    float f[6], t1[6], t2[6];
    mul_inert_vec(f, s.cinert[b], cacc[b]);
    mul_inert_vec(t1, s.cinert[b], cvel[b]);
    cross_force(t2, cvel[b], t1);
    for (int k = 0; k < 6; k++) f[k] += t2[k];
    for (int k = 0; k < 6; k++) cacc[b][k] = f[k];
  }
  wsync();
  // subtree sum (DFS range) -> cvel storage
  float sub[6];
  const int bb = lane < m.nbody ? lane : 0;
  for (int k = 0; k < 6; k++) sub[k] = 0;
  if (lane < m.nbody && lane > 0)
#pragma unroll AW_SUB_UNROLL
    for (int d = bb; d < MD(body_subtree_end, bb); d++)
      for (int k = 0; k < 6; k++) sub[k] += cacc[d][k];
  wsync();
  if (lane < m.nbody)
    for (int k = 0; k < 6; k++) cvel[bb][k] = sub[k];
  wsync();
  DynFrc r = {0.f, 0.f, 0.f};
  if (lane < m.nv) {
    const int j = lane;
    r.bias = dot6(s.cdof[j], cvel[MD(dof_bodyid, j)]);
    r.pas = (m.disableflags & DSBL_PASSIVE) ? 0.f : -MD(dof_damping, j) * s.qvel[j];
    const int u = MD(dof_act, j);
    if (u >= 0 && !(m.disableflags & DSBL_ACTUATION)) {
      float ctrl = s.ctrl[u];
      if (MD(act_ctrllimited, u) && !(m.disableflags & DSBL_CLAMPCTRL))
        ctrl = clampf(ctrl, MD(act_ctrlrange, 2 * u), MD(act_ctrlrange, 2 * u + 1));
      float gear = MD(act_gear, u);
      float len = gear * s.qpos[j], vel = gear * s.qvel[j];
      const auto bp = MDP(act_bias, 3 * u);
      float f = MD(act_gain, u) * ctrl + bp[0] + bp[1] * len + bp[2] * vel;
      if (MD(act_forcelimited, u)) f = clampf(f, MD(act_forcerange, 2 * u), MD(act_forcerange, 2 * u + 1));
      r.act = gear * f;
    }
  }
  wsync();
  return r;
}

// mj_objectVelocity (flg_local 0) of a point p moving with body b: (omega, v at p) from cvel[b],
// which is taken at subtree_com[body_rootid[b]]
AW_DEV void dyn_point_vel(const DModel& m, const Env& s, int b, const float* p, float* out6) {
  float r[3], c[3];
  sub3(r, p, s.subcom[MD(body_rootid, b)]);
  cross3(c, s.cvel[b], r);
  for (int k = 0; k < 3; k++) { out6[k] = s.cvel[b][k]; out6[3 + k] = s.cvel[b][3 + k] + c[k]; }
}

}  // namespace aw

// Output row blockIdx.x evaluates env env_ids[blockIdx.x] (nullptr: env blockIdx.x); an id outside
// [0, n) is uniform over the wave, which leaves before it has written anything.  The env id selects
// what is READ (the stored state, the params); every input row (qpos, qvel, ctrl) and every output
// index is formed from blockIdx.x, a point index < npoints <= AW_DYN_MAXPOINTS, a body < nbody and a
// dof lane < NV, so a wave writes only its own row.  Nothing of DState is written.  Stores: lane =
// dof writes the rows of jacp / jacr as contiguous nv-float runs; M and inv(M) are symmetric, so lane
// i stores its register row as COLUMN i (out[k nv + i] = row[k]): one coalesced run per k.
template <int TASK>
__global__ void __launch_bounds__(64) k_dyn(DModel m, DState st, int n, const int* __restrict__ env_ids, DynPts pts,
                                            int npoints, const float* __restrict__ qpos,
                                            const float* __restrict__ qvel, const float* __restrict__ ctrl,
                                            aw_dyn_out o) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  const int lane = threadIdx.x;
  const size_t row = blockIdx.x;
  const int env = env_ids ? __builtin_amdgcn_readfirstlane(env_ids[row]) : (int)blockIdx.x;
  if ((unsigned)env >= (unsigned)n) return;
  load_env<NV>(m, s, st, env, lane);
  if (lane < NV) {
    if (qpos) s.qpos[lane] = qpos[row * m.nq + lane];
    if (qvel) s.qvel[lane] = qvel[row * m.nv + lane];
  }
  if (lane < m.nu) s.ctrl[lane] = ctrl ? ctrl[row * m.nu + lane] : 0.f;
  stage_model(m, s, st.params + (size_t)env * m.nparam, lane);
  stage_kinematics(m, s, lane);
  stage_com(m, s, lane);

  if (lane < npoints) {
    const int kind = pts.kind[lane], id = pts.id[lane];
    float p[3];
    int b = id;
    if (kind == AW_PT_SITE) { copy3(p, s.sxpos[id]); b = MD(site_bodyid, id); }
    else if (kind == AW_PT_BODYCOM) copy3(p, s.xipos[id]);
    else copy3(p, s.xpos[id]);
    for (int k = 0; k < 3; k++) dyn_pos(s, lane)[k] = p[k];
    dyn_body(s, lane) = b;
    if (o.point_pos)
      for (int k = 0; k < 3; k++) o.point_pos[(row * npoints + lane) * 3 + k] = p[k];
  }
  wsync();

  if (o.jacp || o.jacr) {
    const int li = lane < NV ? lane : NV - 1;
    float cd[6];
    for (int k = 0; k < 6; k++) cd[k] = s.cdof[li][k];
    for (int p = 0; p < npoints; p++) {
      const int b = dyn_body(s, p);
      const bool on = (MD(body_dofmask, b) >> li) & 1ull;
      float r[3], jp[3];
      sub3(r, dyn_pos(s, p), s.subcom[MD(body_rootid, b)]);
      cross3(jp, cd, r);
      if (lane < NV) {
        const size_t base = (row * npoints + p) * 3 * NV + lane;
        for (int k = 0; k < 3; k++) {
          if (o.jacp) o.jacp[base + (size_t)k * NV] = on ? cd[3 + k] + jp[k] : 0.f;
          if (o.jacr) o.jacr[base + (size_t)k * NV] = on ? cd[k] : 0.f;
        }
      }
    }
  }

  const bool want_frc = o.qfrc_bias || o.qfrc_passive || o.qfrc_actuator;
  if (want_frc || o.xvel || o.point_vel) {
    dyn_comvel(m, s, lane);
    if (o.xvel && lane < m.nbody) {
      float v[6];
      dyn_point_vel(m, s, lane, s.xpos[lane], v);
      for (int k = 0; k < 6; k++) o.xvel[(row * m.nbody + lane) * 6 + k] = v[k];
    }
    if (o.point_vel && lane < npoints) {
      float v[6];
      dyn_point_vel(m, s, dyn_body(s, lane), dyn_pos(s, lane), v);
      for (int k = 0; k < 6; k++) o.point_vel[(row * npoints + lane) * 6 + k] = v[k];
    }
    wsync();   // dyn_forces overwrites cvel
    if (want_frc) {
      const DynFrc f = dyn_forces(m, s, lane);
      if (lane < NV) {
        if (o.qfrc_bias) o.qfrc_bias[row * NV + lane] = f.bias;
        if (o.qfrc_passive) o.qfrc_passive[row * NV + lane] = f.pas;
        if (o.qfrc_actuator) o.qfrc_actuator[row * NV + lane] = f.act;
      }
    }
  }

  if (o.qM || o.qMinv) {
    float Mrow[NV];
    stage_crb<TASK>(m, s, lane, Mrow);
    const size_t base = row * NV * NV + lane;
    if (o.qM && lane < NV)
#pragma unroll
      for (int k = 0; k < NV; k++) o.qM[base + (size_t)k * NV] = Mrow[k];
    if (o.qMinv) {
      float invd, X[NV];
      tree_factor<TASK>(Mrow, invd, lane);
      tree_inverse<TASK>(Mrow, invd, lane, X);
      if (lane < NV)
#pragma unroll
        for (int k = 0; k < NV; k++) o.qMinv[base + (size_t)k * NV] = X[k];
    }
  }
}
