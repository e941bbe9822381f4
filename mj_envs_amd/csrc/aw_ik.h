// aw_ik.h -- inverse kinematics (aw_solve_ik, k_ik): batched damped least squares, one launch.  One
// wave per output row runs the whole iteration of include/adroit_wave.h in LDS: the forward's own
// stage_kinematics / stage_com at the trial q, the weighted residual e and Jacobian J of the targets,
// A = J J' + damping I on the matrix cores, its Cholesky factor, dq = J' A^-1 e, the step limit and the
// range clamp -- and leaves on a wave-uniform test of its own residual.  The step, reset, set-state
// and render kernels call nothing of this file.
//
// LDS placement (no second __shared__ block: Env's 20 256 bytes sit under the 20 480-byte granule at
// which eight workgroups share a CU).  k_ik builds no contacts and no constraint rows, so it owns
//   s.J rows [0, m)            J, row stride VS, lane = dof writes column `lane`.  stage_kinematics
//                              stages its joint records in the same rows at the top of every
//                              iteration; J is rebuilt after it, so the two never overlap in time
//   efc_v0 .. efc_D            A, then its lower Cholesky factor in place: m x m, row stride IK_AS
//   efc_aref                   the target records: 16 floats per target (IkRec below)
//   efc_force                  e [0, 24) and y = A^-1 e [32, 56)
// Lane maps: target records lane = target; Jacobian lane = dof (column); J J' the 16x16x4 MFMA tiling
// of stage_crb (lane & 15 = tile row / column, lane >> 4 = k within the K-step); Cholesky and the two
// triangular solves lane = row.  Every reduction has one order, fixed by the lane map alone
// (wave_sum / wave_max butterflies, the MFMA's K order, j ascending in the factor), so a row's result
// does not depend on the grid or on env_ids.
#pragma once
#include "aw_common.h"
#include "aw_dynamics.h"
#include "aw_handle.h"
#include "aw_step.h"

// 1 (default): J J' with v_mfma_f32_16x16x4_f32; 0: one entry per lane and pass, dot products from LDS
#ifndef AW_IK_MFMA
#define AW_IK_MFMA 1
#endif

namespace aw {

constexpr int IK_AS = 25;   // row stride of A: odd, so the lanes of a column step hit distinct banks
constexpr int IK_REC = 16;  // floats per target record
constexpr int IK_E = 0, IK_Y = 32;   // e and y inside efc_force
static_assert(IK_REC * AW_IK_MAXTARGETS <= MAXEFC, "target records do not fit efc_aref");
static_assert(IK_Y + AW_IK_MAXROWS <= MAXEFC && IK_E + AW_IK_MAXROWS <= IK_Y, "e and y do not fit efc_force");
static_assert(AW_IK_MAXROWS <= JL && AW_IK_MAXROWS <= 32 && MAXV <= VS, "J does not fit the dense-J rows");
static_assert(4 * ((MAXV + 3) / 4) <= VS, "the last MFMA K-step reads inside a J row");
static_assert(offsetof(Env, efc_D) == offsetof(Env, efc_v0) + 3 * sizeof(float) * MAXEFC &&
                  IK_AS * AW_IK_MAXROWS <= 4 * MAXEFC,
              "A does not fit efc_v0 .. efc_D");
static_assert(3 * AW_IK_MAXTARGETS <= AW_IK_MAXROWS, "eight position targets fit the row capacity");

// target record p: {pos[3], body} {quat[4]} {goal pos[3], -} {goal quat[4]}
AW_DEV float* ik_rec(Env& s, int p) { return s.efc_aref + IK_REC * p; }
AW_DEV int& ik_body(Env& s, int p) { return reinterpret_cast<int*>(s.efc_aref)[IK_REC * p + 3]; }
AW_DEV float* ik_A(Env& s) { return s.efc_v0; }

// world-frame rotation vector of d = qg * conj(qc), the shorter way round (include/adroit_wave.h)
AW_DEV void ik_rotvec(float* r, const float* qg, const float* qc) {
  const float cj[4] = {qc[0], -qc[1], -qc[2], -qc[3]};
  float d[4];
  mulq(d, qg, cj);
  if (d[0] < 0.f)
    for (int k = 0; k < 4; k++) d[k] = -d[k];
  const float n = sqrtf(d[1] * d[1] + d[2] * d[2] + d[3] * d[3]);
  const float f = n > 0.f ? 2.f * atan2f(n, d[0]) / n : 0.f;
  for (int k = 0; k < 3; k++) r[k] = n > 0.f ? f * d[1 + k] : 0.f;
}

}  // namespace aw

// Output row blockIdx.x solves for env env_ids[blockIdx.x] (nullptr: env blockIdx.x); an id outside
// [0, n) is uniform over the wave, which leaves before it has written anything.  The env id selects
// what is READ (the stored state, the params); goal, qpos0 and every output index are formed from
// blockIdx.x, a target < ntargets <= AW_IK_MAXTARGETS and a dof lane < NV, so a wave writes only its
// own row.  Nothing of DState is written.  tg.row[p]: first row of target p; mrows: the row count m.
template <int TASK>
__global__ void __launch_bounds__(64) k_ik(DModel m, DState st, int n, const int* __restrict__ env_ids, IkTgt tg,
                                           int ntargets, int mrows, unsigned long long dof_mask,
                                           const float* __restrict__ goal, const float* __restrict__ qpos0,
                                           aw_ik_opt opt, aw_ik_out o) {
  constexpr int NV = Tree<TASK>::NV;
  __shared__ Env s;
  const int lane = threadIdx.x;
  const size_t row = blockIdx.x;
  const int env = env_ids ? __builtin_amdgcn_readfirstlane(env_ids[row]) : (int)blockIdx.x;
  if ((unsigned)env >= (unsigned)n) return;
  load_env<NV>(m, s, st, env, lane);
  if (qpos0 && lane < NV) s.qpos[lane] = qpos0[row * m.nq + lane];
  stage_model(m, s, st.params + (size_t)env * m.nparam, lane);

  const int li = lane < NV ? lane : NV - 1;
  const bool free_dof = lane < NV && ((dof_mask >> li) & 1ull);
  const bool is_tgt = lane < ntargets;
  const int tp = is_tgt ? lane : 0;
  const int kind = tg.kind[tp], id = tg.id[tp], row0 = tg.row[tp];
  const float wpos = tg.wpos[tp], wrot = tg.wrot[tp];
  if (is_tgt) {
    float* R = ik_rec(s, lane);
    const float* g = goal + (row * ntargets + lane) * 7;
    float gq[4] = {g[3], g[4], g[5], g[6]};
    normq(gq);
    for (int k = 0; k < 3; k++) R[8 + k] = g[k];
    for (int k = 0; k < 4; k++) R[12 + k] = gq[k];
  }
  float* es = s.efc_force + IK_E;
  float* ys = s.efc_force + IK_Y;
  float* As = ik_A(s);

  int it = 0;
  float err;
  for (;;) {
    // 1. forward kinematics at q; the targets' poses and the residual
    stage_kinematics(m, s, lane);
    stage_com(m, s, lane);
    if (is_tgt) {
      float p[3], q[4];
      int b = id;
      if (kind == AW_PT_SITE) {
        b = MD(site_bodyid, id);
        float sq[4];
        for (int c = 0; c < 4; c++) sq[c] = MD(site_quat, 4 * id + c);
        copy3(p, s.sxpos[id]);
        mulq(q, s.xquat[b], sq);
      } else {
        copy3(p, kind == AW_PT_BODYCOM ? s.xipos[id] : s.xpos[id]);
        for (int c = 0; c < 4; c++) q[c] = s.xquat[id][c];
      }
      float* R = ik_rec(s, lane);
      for (int k = 0; k < 3; k++) R[k] = p[k];
      ik_body(s, lane) = b;
      for (int k = 0; k < 4; k++) R[4 + k] = q[k];
      int r = row0;
      if (wpos > 0.f) {
        for (int k = 0; k < 3; k++) es[r + k] = wpos * (R[8 + k] - p[k]);
        r += 3;
      }
      if (wrot > 0.f) {
        float rv[3];
        ik_rotvec(rv, R + 12, q);
        for (int k = 0; k < 3; k++) es[r + k] = wrot * rv[k];
      }
    }
    wsync();
    const float ev = lane < mrows ? es[lane] : 0.f;
    err = sqrtf(wave_sum(ev * ev));
    // 3. (wave-uniform: err comes out of a readlane)
    if (!(err <= 3.402823466e38f) || err <= opt.tol || it >= opt.max_iter) break;

    // 4. J: lane = dof
    {
      float cd[6];
      for (int k = 0; k < 6; k++) cd[k] = s.cdof[li][k];
      for (int p = 0; p < ntargets; p++) {
        const int b = ik_body(s, p);
        const bool on = free_dof && ((MD(body_dofmask, b) >> li) & 1ull);
        const float wp = tg.wpos[p], wr = tg.wrot[p];
        float r[3], jp[3];
        sub3(r, ik_rec(s, p), s.subcom[MD(body_rootid, b)]);
        cross3(jp, cd, r);
        int rr = tg.row[p];
        if (lane < NV) {
          if (wp > 0.f) {
            for (int k = 0; k < 3; k++) s.J[rr + k][lane] = on ? wp * (cd[3 + k] + jp[k]) : 0.f;
            rr += 3;
          }
          if (wr > 0.f)
            for (int k = 0; k < 3; k++) s.J[rr + k][lane] = on ? wr * cd[k] : 0.f;
        }
      }
    }
    wsync();

    // 5. A = J J' + damping I (lower triangle computed, stored to both halves)
#if AW_IK_MFMA
    {
      typedef float f4 __attribute__((ext_vector_type(4)));
      constexpr int KS = (NV + 3) / 4;
      const int sub = lane >> 4, col = lane & 15;
      const bool two = mrows > 16;   // uniform: the second tile row exists
      f4 a00 = {0.f, 0.f, 0.f, 0.f}, a10 = a00, a11 = a00;
#pragma unroll
      for (int ks = 0; ks < KS; ks++) {
        const int c = 4 * ks + sub;   // < VS: inside the row
        const float v0 = s.J[col][c], v1 = s.J[16 + col][c];   // rows < 32 = JL: load, then select
        const float x0 = (col < mrows && c < NV) ? v0 : 0.f;
        const float x1 = (16 + col < mrows && c < NV) ? v1 : 0.f;
        a00 = __builtin_amdgcn_mfma_f32_16x16x4f32(x0, x0, a00, 0, 0, 0);
        if (two) {
          a10 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, x0, a10, 0, 0, 0);
          a11 = __builtin_amdgcn_mfma_f32_16x16x4f32(x1, x1, a11, 0, 0, 0);
        }
      }
#pragma unroll
      for (int r = 0; r < 4; r++) {
        const int i0 = 4 * sub + r, i1 = 16 + i0, k0 = col, k1 = 16 + col;
        if (i0 < mrows && k0 <= i0) {
          const float v = a00[r] + (i0 == k0 ? opt.damping : 0.f);
          As[i0 * IK_AS + k0] = v;
          As[k0 * IK_AS + i0] = v;
        }
        if (i1 < mrows) {   // (i1 < mrows implies two)
          As[i1 * IK_AS + k0] = a10[r];
          As[k0 * IK_AS + i1] = a10[r];
          if (k1 <= i1) {
            const float v = a11[r] + (i1 == k1 ? opt.damping : 0.f);
            As[i1 * IK_AS + k1] = v;
            As[k1 * IK_AS + i1] = v;
          }
        }
      }
    }
#else
    for (int idx = lane; idx < mrows * mrows; idx += 64) {
      const int i = idx / mrows, k = idx - i * mrows;
      float acc = 0.f;
      for (int c = 0; c < NV; c++) acc = fmaf(s.J[i][c], s.J[k][c], acc);
      As[i * IK_AS + k] = acc + (i == k ? opt.damping : 0.f);
    }
#endif
    wsync();

    // 6. Cholesky, one column step at a time, lanes on rows (left-looking: column k of L from the
    // columns before it); lane i keeps 1 / L[i][i].  A pivot that is not > 0 ends the row's loop.
    const int ri = lane < mrows ? lane : mrows - 1;
    float invd = 0.f;
    bool ok = true;
    for (int k = 0; k < mrows; k++) {
      float v = As[ri * IK_AS + k];
      for (int j = 0; j < k; j++) v = fmaf(-As[ri * IK_AS + j], As[k * IK_AS + j], v);
      const float piv = rlane(v, k);
      if (!(piv > 0.f)) { ok = false; break; }
      const float lkk = sqrtf(piv), inv = 1.0f / lkk;
      if (lane == k) { As[k * IK_AS + k] = lkk; invd = inv; }
      else if (lane > k && lane < mrows) As[lane * IK_AS + k] = v * inv;
      wsync();
    }
    if (!ok) break;
    // L z = e, then L' y = z: lane i holds entry i
    float rhs = ev;
    for (int k = 0; k < mrows; k++) {
      const float zk = rlane(rhs, k) * rlane(invd, k);
      if (lane == k) rhs = zk;
      else if (lane > k && lane < mrows) rhs = fmaf(-As[lane * IK_AS + k], zk, rhs);
    }
    for (int k = mrows - 1; k >= 0; k--) {
      const float yk = rlane(rhs, k) * rlane(invd, k);
      if (lane == k) rhs = yk;
      else if (lane < k) rhs = fmaf(-As[k * IK_AS + lane], yk, rhs);
    }
    if (lane < mrows) ys[lane] = rhs;
    wsync();

    // dq = J' y (lane = dof; a column outside dof_mask is zero), 7. the step limit, 8. 9. the update
    float dq = 0.f;
    if (free_dof)
      for (int r = 0; r < mrows; r++) dq = fmaf(s.J[r][lane], ys[r], dq);
    if (opt.max_step > 0.f) {
      const float mx = wave_max(fabsf(dq));
      if (mx > opt.max_step) dq = clampf(dq * (opt.max_step / mx), -opt.max_step, opt.max_step);
    }
    if (free_dof) {
      float q = s.qpos[lane] + dq;
      if (opt.clamp_range && MD(jnt_limited, li)) q = clampf(q, MD(jnt_range, 2 * li), MD(jnt_range, 2 * li + 1));
      s.qpos[lane] = q;
    }
    it++;
    wsync();
  }

  // the outputs belong to the q the loop left: its last pass evaluated the poses and e at that q
  if (lane < NV) o.qpos[row * m.nq + lane] = s.qpos[lane];
  if (lane == 0) {
    if (o.err) o.err[row] = err;
    if (o.iters) o.iters[row] = it;
  }
  if (is_tgt) {
    const float* R = ik_rec(s, lane);
    if (o.point_pos)
      for (int k = 0; k < 3; k++) o.point_pos[(row * ntargets + lane) * 3 + k] = R[k];
    if (o.point_quat)
      for (int k = 0; k < 4; k++) o.point_quat[(row * ntargets + lane) * 4 + k] = R[4 + k];
  }
}
