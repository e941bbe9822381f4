/* adroit_wave.h -- C-ABI of the MI355X batched Adroit simulator (libadroit_hip.so).
 *
 * Drop-in boundary for the reference hot path.  The reference binds the physics through
 * mujoco-py (Cython) -> MuJoCo 2.1.0 C API, driven by mjrl's MujocoEnv and the task classes:
 *
 *   aw_create   replaces mujoco_py.load_model_from_path + MjSim(...)        (via mjrl
 *               MujocoEnv.__init__, hand_manipulation_suite/hammer_v0.py:20)
 *   aw_reset    replaces MujocoEnv.reset -> sim.reset() + reset_model()     (hammer_v0.py:106-132,
 *               door_v0.py:103-119, pen_v0.py:115-132, relocate_v0.py:85-103)
 *   aw_step     replaces *EnvV0.step: clip/scale action (hammer_v0.py:55-59), do_simulation
 *               (:60, mj_step x frame_skip), get_obs (:92-104), reward/done/goal (:62-90)
 *   aw_get_state / aw_set_state  replace get_env_state / set_env_state     (hammer_v0.py:134-153)
 *   aw_task_eval  the task layer alone on caller-provided kinematics (golden-vector parity)
 *
 * Conventions
 *   - All array arguments are DEVICE pointers (HIP / torch.cuda memory), fp32 unless noted,
 *     env-major: obs[N][obs_dim], actions[N][nu], qpos[N][nq], params[N][nparam].
 *   - The library owns the simulator state (qpos, qvel, qacc_warmstart, per-env model params,
 *     episode counters); the caller owns every I/O buffer it passes in.
 *   - Every call enqueues on `stream` (a hipStream_t, NULL = default stream) and returns
 *     without synchronising.  One handle per host thread / stream.
 *   - Return 0 on success, a negative AW_E* code on error (message: aw_last_error()).
 *     Per-env faults (NaN state, contact / constraint overflow) never abort a batch: they are
 *     reported as AW_ST_* flags by aw_status, and a NaN state is reset as MuJoCo does.
 */
#ifndef ADROIT_WAVE_H
#define ADROIT_WAVE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct aw_handle aw_handle;

enum {
  AW_OK = 0,
  AW_EINVAL = -1,    /* bad argument */
  AW_EBLOB = -2,     /* malformed or unsupported model table */
  AW_EHIP = -3,      /* HIP runtime error */
  AW_ENOMEM = -4,
  AW_EUNSUPPORTED = -5
};

/* per-env status flags (aw_status) */
enum {
  AW_ST_BADQPOS = 1,
  AW_ST_BADQVEL = 2,
  AW_ST_BADQACC = 4,
  AW_ST_CON_OVERFLOW = 8,   /* a contact past nconmax (100) was dropped, as MuJoCo drops it */
  AW_ST_EFC_OVERFLOW = 16,  /* a constraint row past njmax (500) was dropped, as MuJoCo drops it */
  AW_ST_WIDE = 32           /* informational: the step ran in the wide-capacity tier (below) */
};

/* aw_dims() output order.  MAXCON / MAXEFC / MAXDENSE: the per-env capacities for contacts,
 * constraint rows and dense (contact) rows -- the reference model's own, nconmax 100 / njmax 500
 * (DAPG_assets.xml:4); a step that needs more drops what MuJoCo drops and raises
 * AW_ST_*_OVERFLOW.  Two tiers hold them: every env-step runs in the fast tier (FAST_* capacities,
 * per task -- FAST_MAXDENSE is 192 for relocate-v0, 128 for the others -- two waves per SIMD); one
 * that needs more is abandoned there before anything is written and
 * re-run in the same aw_step / aw_reset / aw_set_state call by the wide tier (MuJoCo's
 * capacities, WIDE_GRID persistent workgroups), which marks it AW_ST_WIDE.
 * GRID: workgroups of one aw_step launch (one per resident slot on the device, capped at
 * n_envs); below n_envs the persistent workgroups claim the remaining envs from per-XCD
 * counters (contiguous env ranges per XCD, stealing once a range is exhausted), each range in
 * descending order of its envs' last env-step cost (longest processing time first). */
enum {
  AW_DIM_NQ, AW_DIM_NV, AW_DIM_NU, AW_DIM_OBS, AW_DIM_NPARAM, AW_DIM_FRAME_SKIP,
  AW_DIM_HORIZON, AW_DIM_TASK, AW_DIM_NENV, AW_DIM_NBODY, AW_DIM_NSITE, AW_DIM_NGEOM,
  AW_DIM_NPAIR, AW_DIM_MAXCON, AW_DIM_MAXEFC, AW_DIM_MAXDENSE, AW_DIM_GRID,
  AW_DIM_FAST_MAXCON, AW_DIM_FAST_MAXEFC, AW_DIM_FAST_MAXDENSE, AW_DIM_WIDE_GRID, AW_NDIMS
};

/* model table = Model.to_blob() of mj_envs_amd/mjcf.py with the task block attached
 * (mj_envs_amd/tasks.py attach_task).  Allocates state for n_envs envs on `device`.
 * The table is not trusted (mj_envs_amd/csrc/aw_model_host.h): an entry that is missing or whose
 * length does not follow from the table's dims, or an object id out of range, is AW_EBLOB; a
 * well-formed model beyond the kernels' capacities or features is AW_EUNSUPPORTED. */
int aw_create(const void* blob, size_t nbytes, int n_envs, int device, aw_handle** out);
int aw_destroy(aw_handle* h);
int aw_dims(const aw_handle* h, int* dims /* [AW_NDIMS] */);

/* MuJoCo-style disable flags (mjtDisableBit values, bits 0..15; bit 14 = noslip, bit 15 =
 * explicit damping; higher bits: AW_EUNSUPPORTED -- the MPR (cylinder) collider always runs in
 * fp64 on fp64 geometry) and solver iteration counts; negative values keep the current setting.
 * Waits for the device (queued steps finish with the old options), then re-uploads the model
 * header that k_step reads. */
int aw_set_option(aw_handle* h, int disableflags, int iterations, int noslip_iterations);

/* Capacity tier (test / diagnostic hook): mode 0 = automatic (the fast tier, and the wide tier
 * for a step that needs more than the fast capacities), mode 1 = every env-step, reset and
 * set_state forward re-run by the wide tier (the fast tier's results discarded), so a test can
 * compare the two tiers on the same inputs.  Waits for the device. */
int aw_set_tier(aw_handle* h, int mode);

/* Fault injection (test hook: the parity classifier's negative tests, tests/test_gpu_classifier.py;
 * never set by the product).  kind 0: none (the model table as built); kind 1: the margin of every
 * sphere / capsule pair (collider class 1) shifted by arg x 1e-6 m -- contact activation, the fp64
 * near-margin decision, the rows' includemargin and the broadphase radius; kind 2: frictionloss row
 * `arg` (dof order) held in the stick state (its frictionloss limit raised to 1e6, so mj_solNewton's
 * row never enters a linear zone and noslip never lets it slide).  Waits for the device. */
int aw_set_fault(aw_handle* h, int kind, int arg);

/* MuJoCo's sensordata (sim.data.sensordata of the reference after step() / reset() /
 * set_env_state()): every sensor of the model in its declared order -- the Adroit models carry
 * actuatorfrc, touch and jointpos sensors (DAPG_assets.xml:269-342), one scalar each, 65 in all
 * (hammer 66 with S_nail).  Off by default: aw_set_sensors(h, 1) allocates the [N][nsensordata]
 * buffer (zero until an env's next step, reset or set_state) and selects the instantiation of the
 * step kernels that also evaluates the sensors; with sensors off the step is the kernel it was.
 * Values are those of the last mj_forward before the last integration of the env-step (the lag the
 * observation has): jointpos = qpos there, actuatorfrc = the actuator's scalar force after the
 * forcerange clamp, touch = mj_sensorAcc's sum of the positive contact normal forces on the site's
 * body whose normal ray meets the site's volume.  An env that auto-reset in a step holds its reset
 * forward's values, aligned with obs.  mjDSBL_SENSOR zeroes every entry.  aw_set_sensors waits for
 * the device; aw_sensordata copies the buffer to out (device [N][nsensordata], fp32) and is
 * AW_EINVAL while sensors are disabled. */
int aw_set_sensors(aw_handle* h, int enable);
int aw_sensor_count(const aw_handle* h);
int aw_sensordata(aw_handle* h, float* out, void* stream);

/* Batched mjData views (sim.data of the reference after step() / reset() / set_env_state()): body
 * and site frames, qacc, the constraint force, the solver's counts, and the contact list with
 * mj_contactForce's forces, for every env, written by the step / reset / set_state kernels straight
 * into the CALLER's device buffers -- there is no copy call.  Off by default.  aw_set_data(h, groups,
 * max_contacts, bufs) selects the groups (an OR of AW_DATA_*; 0 disables and ignores the rest) and
 * the instantiation of the step kernels that also writes them; with data off the step is the kernel
 * it was.  Every buffer of a requested group must be device memory that stays valid until data is
 * disabled or the handle destroyed; buffers of groups not requested are ignored (may be NULL) and
 * never written.  Values are those of the last mj_forward before the last integration of the
 * env-step (the lag obs has); an env that auto-reset in a step holds its reset forward's values,
 * aligned with obs.  A buffer row keeps its content until the env's next step, reset or set_state.
 *   AW_DATA_KIN      xpos [N][nbody][3], xquat [N][nbody][4], site_xpos [N][nsite][3]   (fp32)
 *   AW_DATA_DYN      qacc [N][nv], qfrc_constraint [N][nv] (fp32), counts int32 [N][4] = ncon, nefc,
 *                    Newton iterations, noslip iterations; ncon is the forward's count even when it
 *                    exceeds max_contacts
 *   AW_DATA_CONTACT  contact [N][max_contacts] records of AW_CONTACT_DWORDS 32-bit words (64 bytes:
 *                    64 max_contacts bytes per env, 134 MB at 65 536 envs with max_contacts 32; DAPG
 *                    grasps reach 12 contacts).  Only records < min(ncon, max_contacts) of an env
 *                    are written, in mj_collision's order; memory past them is left as it was.
 * Contact record: float dist, pos[3], normal[3] (unit, geom1 -> geom2), force[3] (contact frame:
 * normal, then the two tangents of mju_makeFrame(normal); mj_contactForce from efc_force after
 * noslip), torsion (condim 4's third component), mu (sliding friction); int32 geom1, geom2 (model
 * geom ids), dim, efc_address (-1 and zero force: a contact without constraint rows).
 * AW_EINVAL: unknown group bits, a NULL buffer of a requested group, max_contacts < 1 or above the
 * wide tier's contact storage (AW_DATA_MAX_CONTACTS).  Waits for the device.  Sensors and data may be
 * on together. */
enum { AW_DATA_KIN = 1, AW_DATA_DYN = 2, AW_DATA_CONTACT = 4 };
#define AW_CONTACT_DWORDS 16
#define AW_DATA_MAX_CONTACTS 128
typedef struct {
  float *xpos, *xquat, *site_xpos, *qacc, *qfrc_constraint;
  int32_t* counts;
  void* contact;
} aw_data_bufs;
int aw_set_data(aw_handle* h, int groups, int max_contacts, const aw_data_bufs* bufs);

/* Reset envs (mask[e] != 0, or all if mask == NULL): qpos = qpos0, qvel = 0, warmstart = 0,
 * per-env model params from `params` [N][nparam] or, if NULL, sampled on device (Philox,
 * keyed by seed, global env id and episode count) from the reference reset distribution;
 * then mj_forward.  obs (may be NULL) receives the reset observation. */
int aw_reset(aw_handle* h, const uint8_t* mask, const float* params, uint64_t seed, float* obs,
             void* stream);

/* One env step for all envs: a = clip(actions, -1, 1); ctrl = act_mid + a * act_rng;
 * frame_skip x mj_step; obs / reward / goal.  done[e]: bit0 = terminated (pen drop),
 * bit1 = truncated (horizon reached).  With autoreset != 0 an env whose episode ended is
 * reset in the same launch (new params sampled with `seed`) and obs holds its first
 * observation; terminal_obs (may be NULL) receives the last obs of the ended episode. */
int aw_step(aw_handle* h, const float* actions, float* obs, float* reward, uint8_t* done,
            uint8_t* goal, float* terminal_obs, int autoreset, uint64_t seed, void* stream);

/* i.i.d. U(-1, 1) actions from Philox (key = seed, counter = (global env id, step)) */
int aw_random_actions(aw_handle* h, uint64_t seed, uint64_t step, float* actions, void* stream);

/* Global id of this handle's env 0 (default 0).  A shard of a larger batch (one handle per
 * GPU, envs [offset, offset + n_envs) of the global batch) sets it so every Philox stream --
 * reset draws (aw_reset / auto-reset), aw_random_actions, aw_policy_mlp noise -- is keyed by the
 * GLOBAL env id: N shards reproduce one unsharded run bit for bit.  Waits for the device. */
int aw_set_env_offset(aw_handle* h, uint64_t env_offset);

/* state round trip: qpos [N][nq], qvel [N][nv], warmstart [N][nv], params [N][nparam];
 * any pointer may be NULL.  set_state runs mj_forward (obs may be NULL). */
int aw_get_state(aw_handle* h, float* qpos, float* qvel, float* warmstart, float* params,
                 void* stream);
int aw_set_state(aw_handle* h, const float* qpos, const float* qvel, const float* warmstart,
                 const float* params, float* obs, void* stream);

/* Indexed state access: set, read and clone a subset of the envs on the device (demonstration-state
 * resets, restarts from a replay buffer, branching one state into the K rollouts of a sampling
 * planner, broadcasting B root states into a B x K planner batch on another handle).  Every id and
 * row array is a DEVICE int32 array, as aw_render_labels' env_ids is.
 *   aw_set_state_ids: env env_ids[k] (k < n_sel) takes row rows[k] (rows == NULL: row k) of every
 * non-NULL input array -- qpos [n_rows][nq], qvel / warmstart [n_rows][nv], params [n_rows][nparam];
 * a NULL array keeps that env's current values, and all four NULL re-runs the forward of the
 * selected envs.  Then mj_forward with ctrl 0 for the selected envs only (n_sel workgroups).  obs:
 * NULL, or the caller's [N][obs_dim] buffer indexed by ENV id, of which only the selected envs' rows
 * are written (as aw_reset with a mask writes it).  For a selected env every result -- the stored
 * state, the obs row, its status (last and sticky), its sensordata row, its mjData-view rows -- is bit
 * for bit what aw_set_state gives for the same values, the hand-off of a forward beyond the fast
 * capacities to the wide tier included (aw_set_tier(h, 1) forces it); an env that is not selected is
 * untouched in every buffer.  reset_episode != 0 zeroes the selected envs' running-episode counters
 * (steps, return, goal steps: what aw_get_episode's first three report), as aw_reset does; the
 * finished-episode count (the Philox episode key), the last-episode stats and the totals are never
 * touched.  A pair whose env_ids[k] is outside [0, N) or whose rows[k] (or k, with rows NULL) is
 * outside [0, n_rows) is skipped: nothing is written for it.  env_ids must be distinct: the library
 * does not check it, and an env listed more than once ends in the state of one of its rows,
 * unspecified which (nothing outside that env is written).  rows may repeat (a broadcast).
 * AW_EINVAL: NULL handle or env_ids, n_sel < 1, n_rows < 1.
 *   aw_get_state_ids: output row k (qpos [n_sel][nq], ...) receives env env_ids[k]; an id outside
 * [0, N) leaves row k untouched; any output may be NULL; ids may repeat.  A plain gather, no forward.
 * AW_EINVAL: NULL handle or env_ids, n_sel < 1.
 *   aw_clone_envs: env dst_ids[k] becomes a copy of env src_ids[k] (k < n): qpos, qvel, warmstart,
 * params and, with episode != 0, the running-episode counters (never the finished-episode count, the
 * last-episode stats or the totals); then the forward of the dst envs as in aw_set_state_ids (obs as
 * there).  Every read happens before any write: the n source rows are gathered into a scratch block of
 * the handle, then set from there on the same stream -- src {0,1}, dst {1,0} swaps two envs, src
 * {0,0,0}, dst {1,2,3} broadcasts one.  The FIRST call allocates the scratch block (N rows; a
 * hipMalloc, so not inside a graph capture); aw_destroy frees it.  dst_ids must be distinct (the rule
 * of env_ids above); src_ids may repeat.  A pair with either id outside [0, N) is skipped whole.
 * AW_EINVAL: NULL handle, src_ids or dst_ids, n outside 1..N. */
int aw_set_state_ids(aw_handle* h, const int32_t* env_ids, int n_sel, const int32_t* rows, int n_rows,
                     const float* qpos, const float* qvel, const float* warmstart, const float* params,
                     int reset_episode, float* obs, void* stream);
int aw_get_state_ids(aw_handle* h, const int32_t* env_ids, int n_sel, float* qpos, float* qvel,
                     float* warmstart, float* params, void* stream);
int aw_clone_envs(aw_handle* h, const int32_t* src_ids, const int32_t* dst_ids, int n, int episode,
                  float* obs, void* stream);

/* per-env status flags (AW_ST_*), uint32 [N]: `last` = flags raised by the last step / reset /
 * set_state of each env, `sticky` = OR of every flag raised since aw_create or the last
 * aw_clear_status (MuJoCo's warning counters play this role); either pointer may be NULL */
int aw_status(aw_handle* h, uint32_t* last, uint32_t* sticky, void* stream);
int aw_clear_status(aw_handle* h, void* stream);

/* completed-episode statistics: return, goal-step count, length of each env's last finished
 * episode, and the number of finished episodes; any pointer may be NULL */
int aw_episode_stats(aw_handle* h, float* last_return, int32_t* last_goal_steps,
                     int32_t* last_len, int32_t* episodes, void* stream);

/* running totals over every finished episode of each env: count, sum of returns, and count of
 * successful episodes (> task success_steps goal steps: hammer_v0.py:167-175, pen_v0.py:180-188) */
int aw_episode_totals(aw_handle* h, int32_t* episodes, float* sum_return, int32_t* successes,
                      void* stream);

/* Restore the running totals (checkpoint / resume): finished-episode count, summed return,
 * successes.  The finished-episode count is also the Philox episode key of the reset draws, so a
 * checkpoint restores it once, here or through aw_set_episode, with the same value.  A complete
 * checkpoint is aw_get_state (qpos, qvel, warmstart, params) + aw_get_episode (ep_len, ep_ret,
 * ep_goal) + aw_episode_totals (episodes, sum_return, successes), restored with aw_set_state,
 * aw_set_episode and aw_set_episode_totals. */
int aw_set_episode_totals(aw_handle* h, const int32_t* episodes, const float* sum_return,
                          const int32_t* successes, void* stream);

/* episode bookkeeping of the running episode (checkpoint / resume, staggered starts): steps
 * taken, return so far, goal steps so far, finished-episode count; any pointer may be NULL */
int aw_get_episode(aw_handle* h, int32_t* ep_len, float* ep_ret, int32_t* ep_goal, int32_t* episodes,
                   void* stream);
int aw_set_episode(aw_handle* h, const int32_t* ep_len, const float* ep_ret, const int32_t* ep_goal,
                   const int32_t* episodes, void* stream);

/* Task layer only, on caller-provided kinematics for n samples (device pointers, fp32):
 * qpos [n][nq], qvel [n][nv], xpos [n][nbody][3], xquat [n][nbody][4],
 * site_xpos [n][nsite][3], touch [n] (the task's touch sensor value) ->
 * obs [n][obs_dim], reward [n], done [n], goal [n]. */
int aw_task_eval(aw_handle* h, int n, const float* qpos, const float* qvel, const float* xpos,
                 const float* xquat, const float* site_xpos, const float* touch, float* obs,
                 float* reward, uint8_t* done, uint8_t* goal, void* stream);

/* Introspection for parity tests: run mj_forward (no integration) on env `env` of the
 * current state with raw control `ctrl` [nu] (NULL = 0) and copy internals into out (fp32,
 * AW_DUMP_SIZE floats; layout: mj_envs_amd/_native.py DUMP_LAYOUT). */
#define AW_DUMP_SIZE 3400
int aw_forward_dump(aw_handle* h, int env, const float* ctrl, float* out, void* stream);
/* The same forward through the wide-capacity tier (MuJoCo's nconmax 100 / njmax 500: contacts and
 * rows past the fast tier's capacities are kept), AW_DUMP_SIZE_WIDE floats, the layout of
 * dump_layout(128, 512). */
#define AW_DUMP_SIZE_WIDE 6120
int aw_forward_dump_wide(aw_handle* h, int env, const float* ctrl, float* out, void* stream);

/* Dynamics queries (k_dyn): the model-based half of sim.data for a chosen subset of envs, on demand --
 * point and body Jacobians (mujoco-py get_site_jacp / jacr, get_body_jacp / jacr), linear and angular
 * velocities (get_body_xvelp / xvelr, get_site_xvelp / xvelr), the joint-space inertia and its inverse,
 * and the three terms of qfrc_smooth.  One wave per output row composes the forward's own position
 * and velocity stages (kinematics, mj_comPos, mj_comVel, mj_rne, mj_passive, mj_fwdActuation, mj_crb,
 * the tree-sparse LDL') and stores what was asked for; no collision, no constraint solve.
 *   VALUES are those of mj_forward's position and velocity stages AT THE GIVEN STATE -- what mujoco-py
 * shows after sim.forward() -- not the pre-integration values of the last substep that the AW_DATA_*
 * views hold after a step.
 *   env_ids / n_sel: as in aw_render_labels.  NULL: every env, n = n_envs; else a DEVICE int32 array of
 * n = n_sel ids and output row k is env env_ids[k]; an id outside [0, n_envs) leaves row k of every
 * output untouched; ids may repeat.
 *   points: a HOST array of npoints (0..AW_DYN_MAXPOINTS) records, handed to the kernel by value:
 * kind AW_PT_BODY (the body frame's origin xpos[id]), AW_PT_BODYCOM (the body's centre of mass
 * xipos[id]) or AW_PT_SITE (site_xpos[id]); the point moves with body id (the site's body).
 *   qpos [n][nq], qvel [n][nv]: NULL (the env's own stored state) or DEVICE arrays indexed by OUTPUT
 * ROW that replace the env's values for this evaluation only; nothing of the simulation is written.
 * The model parameters are always the env's own (mass, position and size variations, reset draws).
 *   ctrl [n][nu]: NULL (zero) or DEVICE raw controls indexed by output row, as aw_forward_dump takes
 * them; only qfrc_actuator reads them.
 *   out: DEVICE fp32 buffers, any may be NULL (then not computed; whole stages are skipped when no
 * requested output needs them):
 *     qM, qMinv [n][nv][nv]   dense symmetric: mj_fullM's matrix (armature on the diagonal) and its
 *                             inverse from the tree factorisation (mj_factorM / mj_solveM)
 *     qfrc_bias, qfrc_passive, qfrc_actuator [n][nv]   mj_rne with flg_acc = 0, -damping qvel, the
 *                             actuator forces mapped to the dofs; passive - bias + actuator = qfrc_smooth
 *     xvel [n][nbody][6]      (angular, linear at xpos[b]) in world axes: mj_objectVelocity, flg_local 0
 *     point_pos [n][npoints][3], point_vel [n][npoints][6]   the points and their (angular, linear) velocity
 *     jacp, jacr [n][npoints][3][nv]   mj_jac: column i is zero unless dof i moves the point's body b,
 *                             else jacr = cdof_i[0:3], jacp = cdof_i[3:6] + cdof_i[0:3] x (p -
 *                             subtree_com[body_rootid[b]]); body 0 has zero Jacobians
 * The handle's aw_set_option disable flags (gravity, passive, actuation, clampctrl) act as in the forward.
 * Enqueues on `stream`, allocates nothing, does not wait.
 * AW_EINVAL (every other call still works afterwards): NULL h or out, every output NULL, npoints
 * outside 0..AW_DYN_MAXPOINTS or NULL points with npoints > 0, a point output (point_pos, point_vel,
 * jacp, jacr) with npoints == 0, an unknown kind, an id outside its range, n_sel < 1 with env_ids. */
enum { AW_PT_BODY = 0, AW_PT_BODYCOM = 1, AW_PT_SITE = 2 };
#define AW_DYN_MAXPOINTS 16
typedef struct { int32_t kind, id; } aw_dyn_point;
typedef struct {
  float *qM, *qMinv;
  float *qfrc_bias, *qfrc_passive, *qfrc_actuator;
  float *xvel;
  float *point_pos, *point_vel;
  float *jacp, *jacr;
} aw_dyn_out;
int aw_dynamics(aw_handle* h, const int32_t* env_ids, int n_sel, const aw_dyn_point* points, int npoints,
                const float* qpos, const float* qvel, const float* ctrl, const aw_dyn_out* out, void* stream);

/* Inverse kinematics (k_ik): batched damped least squares, the whole iteration in one launch.  Given
 * where up to AW_IK_MAXTARGETS points (and their frames) should be, find joint positions: one wave per
 * output row runs the forward's kinematics, the residual, the Jacobian, the m x m solve and the update
 * in LDS until the row's own residual is small, and stores the result.  No collision, no constraint
 * solve, no posture or null-space term.  All Adroit joints are hinge or slide, so nq == nv.
 *   env_ids / n_sel: as in aw_dynamics.  NULL: every env, n = n_envs; else a DEVICE int32 array of
 * n = n_sel ids and output row k is env env_ids[k]; an id outside [0, n_envs) leaves row k of every
 * output untouched; ids may repeat.
 *   targets: a HOST array of ntargets (1..AW_IK_MAXTARGETS) records, handed to the kernel by value:
 * kind / id as aw_dyn_point; wpos > 0 adds three position rows, wrot > 0 three orientation rows; m, the
 * total row count, is 1..AW_IK_MAXROWS.  The orientation of a point: AW_PT_BODY and AW_PT_BODYCOM
 * xquat[id]; AW_PT_SITE xquat[site_bodyid] * site_quat[id] (site_xmat).
 *   goal: DEVICE [n][ntargets][7] indexed by OUTPUT ROW: position xyz, then quaternion wxyz, which the
 * kernel normalises; a half that is not weighted is ignored; not validated.
 *   dof_mask: bit i lets dof i move; bits at or above nv are ignored.
 *   qpos0: NULL (the env's stored qpos is the start) or DEVICE [n][nq] indexed by output row.  The
 * model parameters are always the env's own (body_pos, body_quat, site_pos, geom_* overrides, reset draws).
 *   Orientation residual: the world-frame rotation vector r of d = q_goal * conj(q_cur), d negated if
 * d.w < 0: r = 2 atan2(|d.xyz|, d.w) d.xyz / |d.xyz|, zero when |d.xyz| underflows.  It pairs with jacr.
 *   Iteration of one row, from k = 0 while k < max_iter:
 *     1. forward kinematics at q
 *     2. the residual e: position rows wpos (goal - p), orientation rows wrot r
 *     3. e non-finite: stop; |e|_2 <= tol: stop
 *     4. J: rows wpos * jacp and wrot * jacr (aw_dynamics' definition), columns outside dof_mask zeroed
 *     5. A = J J^T + damping I_m
 *     6. y = A^-1 e by Cholesky (a pivot that is not > 0 -- non-finite input only -- stops the row), dq = J^T y
 *     7. max_step > 0 and max_i |dq_i| > max_step: dq is scaled by max_step / max_i |dq_i|
 *     8. q += dq
 *     9. clamp_range: each masked dof with jnt_limited is clamped to jnt_range
 *    10. k += 1
 *   out: DEVICE buffers; err, point_pos and point_quat always belong to the returned q (after a loop
 * that ended on max_iter the kinematics and the residual are evaluated once more):
 *     qpos [n][nq]                 required
 *     err [n]                      |e|_2, or NULL
 *     iters int32 [n]              the number of updates applied, or NULL
 *     point_pos [n][ntargets][3], point_quat [n][ntargets][4]   the targets' poses at qpos, or NULL
 * Nothing of the simulation is written; a wave writes only its own row.  Enqueues one launch on
 * `stream`, allocates nothing and does not wait, so it can sit inside a captured graph.
 * AW_EINVAL (every other call still works afterwards): NULL h, targets, goal, opt, out or out->qpos;
 * ntargets outside 1..AW_IK_MAXTARGETS; an unknown kind, an id outside its range; a negative or
 * non-finite weight; a target with both weights 0; more than AW_IK_MAXROWS rows; dof_mask with no bit
 * below nv; max_iter outside 0..AW_IK_MAXITER; damping not > 0 or not finite; tol < 0 or NaN; a
 * non-finite max_step; clamp_range not 0 or 1; n_sel < 1 with env_ids. */
#define AW_IK_MAXTARGETS 8
#define AW_IK_MAXROWS 24
#define AW_IK_MAXITER 64
typedef struct { int32_t kind, id; float wpos, wrot; } aw_ik_target;
typedef struct { int32_t max_iter; float damping, tol, max_step; int32_t clamp_range; } aw_ik_opt;
typedef struct { float* qpos; float* err; int32_t* iters; float* point_pos; float* point_quat; } aw_ik_out;
int aw_solve_ik(aw_handle* h, const int32_t* env_ids, int n_sel, const aw_ik_target* targets, int ntargets,
                uint64_t dof_mask, const float* goal, const float* qpos0, const aw_ik_opt* opt, const aw_ik_out* out,
                void* stream);

/* Depth camera observation (the reference renders RGB through OpenGL:
 * headless_observer.py:20-52 -- free camera azimuth 90, distance 4.5, elevation from the
 * object / last-camera direction, 640x480 frame centre-cropped to 128x128 and resized to
 * 64x64).  Ray-casts every primitive geom of every env's current state (forward kinematics
 * of qpos) into out [N][height][width]: z-depth in metres along the camera axis, cam[AW_CAM_ZFAR]
 * where nothing is hit.  cam: a HOST array of AW_CAM_FLOATS floats (mj_envs_amd/render.py)
 * (position, forward, up, right, then the pixel -> image-plane map u = u0 + du*col,
 * v = v0 - dv*row, then zfar).  Meshes (absent offline) are not rendered. */
#define AW_CAM_FLOATS 17
#define AW_CAM_ZFAR 16
int aw_render_depth(aw_handle* h, const float* cam, int width, int height, float* out, void* stream);

/* RGB camera observation (the frame headless_observer.py:34-52 returns and
 * CustomPixelObservationWrapper(obs_key="pixels") feeds to PlaNet / the CNN PPO path), from the
 * same camera record as aw_render_depth.  One launch ray-casts every env's current state into
 * rgb [N][height][width][3] uint8 and, with depth != NULL (ss must be 1), the aligned depth frame
 * depth [N][height][width], bit for bit what aw_render_depth writes.
 *   Opaque pass: the nearest primitive geom (the depth renderer's search), Phong-shaded in linear
 * [0,1] fp32: c = emission*a + sum over lights [ amb*a + f*(dif*a*max(n.l,0) + [n.l>0]*spe*spec*
 * max(r.v,0)^(128*shin)) ], a = the geom's rgb (explicit rgba, else its material's; geoms are
 * opaque), f = attenuation * spot (positional lights with cutoff < 180: (-l.dir)^exponent inside
 * the cone, 0 outside).  Lights: the camera headlight (a point light at the camera, no cone, no
 * attenuation), then the model's <light>s (up to 4).  No reflections, fog, skybox or textures (a
 * textured material is drawn with its rgba).
 *   Shadows: off unless aw_set_appearance switches them on.  Then they are hard shadows from an
 * any-hit ray.  For a sample whose ray crosses entry g (a geom or a site) at P with facing normal n, a
 * shadow ray is cast for each light that is not the headlight, has castshadow != 0 (slot 21 of its
 * record), n.l > 0 and f > 0: origin P + 1e-4 n, direction l, tested over 0 < t < dist - 1e-4 for a
 * positional light and over every t > 0 for a directional one.  Occluders are the primitive geoms
 * only (finite planes and g itself included); sites never occlude but are shaded with shadows.  If
 * any occluder is crossed, f = 0 for that light: its diffuse and specular terms vanish, its ambient
 * term stays.  No penumbra, no shadow map.  A bounding-sphere test against the segment comes before
 * each exact test; the result is the exhaustive loop's.
 *   Appearance: with per-env tables on the handle (aw_set_appearance) env e is shaded from its own
 * colour and light records and its own look row in place of the model's records and the host look.
 * With shadows or tables on, aw_render_rgb renders through aw_render_views' path with one
 * world-frame view (the same frames, as stated there).
 *   Stand-in rule: the hand's visual geoms are meshes (absent offline); the primitive collision
 * proxy of a group hidden by default (>= 3) is drawn with the colour and material of the first
 * mesh geom of its body, if there is one.
 *   Sites: the visible ones (group 0-2, alpha > 0: hammer nail_goal / S_target, relocate target --
 * the goal markers) are blended over the opaque colour back to front, c = alpha*shade + (1-alpha)*c,
 * the 4 nearest crossings in front of the opaque one; they never write depth.  Per-env site_pos
 * params move them.  Tint rows of the task block (hammer variation "mass": head red = mass / 2.5,
 * hammer_v0.py:118) replace a colour channel by a scaled per-env param.
 *   ss in {1, 2}: ss x ss rays at the centres of the pixel's sub-cells, averaged before
 * floor(255*clamp(c)+0.5).  64x64 with ss = 2 is the box-filtered 128x128 crop (enable_resize).
 *   look: HOST array of AW_LOOK_FLOATS floats -- background rgb, headlight ambient / diffuse /
 * specular, headlight active -- or NULL = 0 0 0, 0.1 0.4 0.5, 1.
 *   Parity: unpinned against the reference (OpenGL, meshes, PNG textures); the kernel is pinned to
 * the fp64 restatement of this model in tests/rgb_checker.py.
 * AW_EINVAL: ss not 1 or 2, depth with ss 2, sizes <= 0 or > 1024, NULL rgb.  AW_EUNSUPPORTED: the
 * model table lacks the appearance arrays (an older file; every other call still works). */
#define AW_LOOK_FLOATS 7
int aw_render_rgb(aw_handle* h, const float* cam, const float* look, int width, int height, int ss,
                  uint8_t* rgb, float* depth, void* stream);

/* Cameras in the frame of a body, one per env, several per launch.  One launch renders every view
 * of every env's current state: the model is staged and the kinematics run once per env, then each
 * view's world record is composed and its frame ray-cast as aw_render_rgb / aw_render_depth do.
 *   views: HOST array of nviews (1..AW_MAX_VIEWS) records, each the AW_CAM_FLOATS layout of
 * aw_render_depth expressed in the frame of body `body` (0 = the world): the models' own <camera>s,
 * a camera mounted on a moving body such as the palm, or the free camera
 * (mj_envs_amd/render.py model_camera / mounted_camera / free_camera).  A record of body 0 is used
 * as it is.  For body b > 0 the kernel composes the world record in fp32 from the env's body frames:
 * position xpos[b] + rot(xquat[b], pos), the three axes rotated by xquat[b], the five scalars copied.
 *   env_cam: NULL, or DEVICE [N][nviews][AW_CAM_FLOATS]: env e renders view v from env_cam[e][v]
 * in place of views[v].rec (camera randomisation; the body is still views[v].body).  A per-env
 * record is not validated: whatever it holds, the kernel writes only that env's own frames.
 *   rgb: DEVICE [N][nviews][height][width][3] uint8 or NULL; depth: DEVICE [N][nviews][height][width]
 * or NULL.  Shading, sites, tints, look and ss are aw_render_rgb's, with the headlight at the
 * composed camera position.  With rgb == NULL the call is depth-only (ss must be 1) and needs no
 * appearance arrays.  One view of body 0 without env_cam writes bit for bit the frames of
 * aw_render_rgb (rgb != NULL) / aw_render_depth (rgb == NULL).
 * AW_EINVAL: nviews outside 1..AW_MAX_VIEWS, a body outside [0, nbody), both outputs NULL, ss not 1
 * or 2, depth or a NULL rgb with ss 2, sizes <= 0 or > 1024.  AW_EUNSUPPORTED: rgb != NULL on a
 * model table without the appearance arrays. */
#define AW_MAX_VIEWS 4
typedef struct { float rec[AW_CAM_FLOATS]; int32_t body; } aw_view;
int aw_render_views(aw_handle* h, const aw_view* views, int nviews, const float* env_cam, const float* look,
                    int width, int height, int ss, uint8_t* rgb, float* depth, void* stream);

/* Per-env appearance and cast shadows of the colour frames (visual domain randomisation).  Off by
 * default; while off, every render call launches the kernels and writes the frames it did before.
 * The state lives on the handle: aw_render_rgb and aw_render_views (rgb != NULL) pick it up;
 * aw_render_labels, aw_render_cloud, aw_render_depth and depth-only aw_render_views ignore it.
 *   app: NULL = tables off, else three DEVICE arrays, each of which may be NULL on its own.  Entry
 * order is aw_render_entries': primitive geoms, then visible sites (ne = ngeom + nsite).  The caller
 * owns the buffers; they must stay valid until appearance is switched off or the handle destroyed.
 * The render kernels read them at launch: a write between two renders shows in the next frame.
 * Tint rows apply on top of the per-env colour record as they do on top of the model's (hammer
 * variation "mass" keeps its red channel).  look[e][0..2] is env e's background, 3..5 its headlight's
 * ambient / diffuse / specular, 6 switches its headlight on.  Per-env records are not validated:
 * whatever they hold, a workgroup writes only its own env's frames.
 *   Light slot 21, castshadow: 1 in every model light record that aw_appearance_defaults returns and
 * that the kernels stage from the model when no light table is given (MuJoCo's default; the Adroit
 * models do not set the attribute, and the model table itself does not carry it), 0 in the
 * headlight's; read only when shadows are on.
 *   shadows: 1 casts the shadow rays defined at aw_render_rgb.  aw_set_appearance waits for the device.
 *   aw_appearance_defaults copies the model's records to HOST arrays col [ne][8] and light
 * [nlight][24] (either may be NULL) and the light count to nlight (may be NULL).
 *   aw_appearance_sample draws records on the device, one thread per float of the env's record vector
 * [col | light | look], F = ne*8 + nlight*24 + 7 floats, between the HOST bounds lo and hi [F]: float
 * i of env e is lo[i] + (hi[i] - lo[i]) * u01(x), x = word i & 3 of philox({env_offset + e,
 * (uint32)draw, 0xA99E, i >> 2}, seed) -- shards reproduce an unsharded run.  Flag slots are copied
 * from lo: light 18 (cos cutoff), 20 (directional), 21 (castshadow) and look 6; a light's dir is
 * renormalised after the draw.  env_ids: NULL = every env, else a DEVICE int32 array of n_sel ids --
 * only those rows are written, an id outside [0, N) is skipped.  col / light / look: DEVICE outputs
 * of the shapes above; a NULL one is not written.
 * AW_EUNSUPPORTED: the model table has no appearance arrays.  AW_EINVAL: shadows not 0 or 1; in
 * aw_appearance_sample a NULL lo or hi, all three outputs NULL, n_sel < 1 with env_ids given, or
 * lo > hi (or a NaN) in any slot.  After either error every other call still works. */
#define AW_COL_FLOATS   8    /* rgb, alpha, specular, 128*shininess, emission, pad */
#define AW_LIGHT_FLOATS 24   /* pos dir ambient diffuse specular attenuation, cos(cutoff) or -2, exponent,
                                directional, castshadow (slot 21), pad */
typedef struct {
  const float* col;    /* DEVICE [N][ngeom+nsite][AW_COL_FLOATS]  or NULL = the model's */
  const float* light;  /* DEVICE [N][nlight][AW_LIGHT_FLOATS]     or NULL = the model's */
  const float* look;   /* DEVICE [N][AW_LOOK_FLOATS]              or NULL = the call's host look */
} aw_appearance;
int aw_set_appearance(aw_handle* h, const aw_appearance* app, int shadows);
int aw_appearance_defaults(const aw_handle* h, float* col, float* light, int* nlight);
int aw_appearance_sample(aw_handle* h, const float* lo, const float* hi, const int32_t* env_ids, int n_sel,
                         uint64_t seed, uint64_t draw, float* col, float* light, float* look, void* stream);

/* Segmentation frames: what each pixel of a camera shows (mujoco-py's sim.render(...,
 * segmentation=True)).  The ray caster's render entries are the primitive (non-mesh) geoms in model
 * order, then the visible sites (group 0-2, alpha > 0) in site order; aw_render_entries returns the
 * two counts (nsite is 0 on a table without the appearance arrays).
 *   aw_render_labels renders the views of aw_render_views (views, nviews, env_cam as there; env_cam
 * is always [N][nviews][AW_CAM_FLOATS], indexed by env id) into labels [n][nviews][height][width]
 * int32: per pixel lut[entry] of the nearest geom crossing (the depth renderer's search), or
 * background where the ray hits nothing.  Geoms that cross within 2e-3 m of the nearest (links
 * that overlap at a joint, coplanar faces) are ordered by a crossing re-evaluated from an origin
 * next to the geom, good to about 1e-6 m; what that cannot tell apart goes to the lower entry.
 * sites 1: the nearest visible site crossing strictly in
 * front of that geom replaces it (a geom wins a tie; among sites the nearest, then the lower entry):
 * sites are drawn solid, as MuJoCo's segmentation draws them.  sites 0 needs no appearance arrays.
 *   lut: HOST array of ngeom + nsite labels or NULL (the entry index itself); mj_envs_amd/labels.py
 * builds tables of model geom ids, body ids, body classes and mujoco-py's objtype << 16 | objid.
 *   env_ids: NULL (every env, n = N, n_sel ignored) or DEVICE array of n_sel env ids: output row k
 * is env env_ids[k] (n = n_sel).  An id outside [0, N) leaves its row untouched.
 *   depth: NULL or DEVICE [n][nviews][height][width], bit for bit the depth frames of
 * aw_render_views depth-only (sites never write depth).
 * AW_EINVAL: nviews outside 1..AW_MAX_VIEWS, a body outside [0, nbody), NULL labels, sizes <= 0 or
 * > 1024, n_sel < 1 with env_ids given, sites not 0 or 1.  AW_EUNSUPPORTED: sites 1 on a model
 * table without the appearance arrays. */
int aw_render_entries(const aw_handle* h, int* ngeom, int* nsite);
int aw_render_labels(aw_handle* h, const aw_view* views, int nviews, const float* env_cam,
                     const int32_t* env_ids, int n_sel, const int32_t* lut, int32_t background,
                     int sites, int width, int height, int32_t* labels, float* depth, void* stream);

/* Point-cloud observations: a fixed-size 3D cloud per env from the depth cameras -- every pixel
 * unprojected into the world, cropped to a box, filtered by what it shows, the views merged
 * (aw_render_cloud), then farthest-point-sampled down to npoints (aw_cloud_fps).
 *   aw_render_cloud takes views, nviews, env_cam, env_ids / n_sel, sites, width and height as
 * aw_render_labels does and writes the candidate points of output row k (env env_ids[k], or env k).
 * A pixel is a candidate when (1) its ray hits a render entry -- aw_render_labels' search and tie
 * rules, so the hit mask and the entry are bit for bit those of aw_render_labels with lut NULL --
 * (2) keep[entry] != 0 and (3) the fp32 world point cam_pos + t*d (d the pixel's unit ray; t for a
 * geom the crossing the depth frame of aw_render_labels is written from, so depth = (p - cam_pos) .
 * forward to a few fp32 roundings: the cloud is that depth frame unprojected; for a site, which
 * writes no depth, the site's own crossing) lies inside the closed box.  Candidates are stored in ascending flat
 * pixel index v*height*width + row*width + col, whatever the schedule (no atomics).
 *   keep: HOST array of ngeom + nsite bytes (aw_render_entries), or NULL = every entry is kept;
 * mj_envs_amd/labels.py keep_table builds one from body names.  box: HOST array of 6 floats, lo xyz
 * then hi xyz, world frame, or NULL = no crop.  frame_body: 0 = the stored points are world
 * coordinates; a body id b = they are rot(xquat[b])^T (p - xpos[b]), the env's own body frame of
 * this render (the crop is still tested on the world point).  cap: 1..AW_CLOUD_MAXCAND slots per row.
 *   xyz: DEVICE [n][cap][3] fp32.  pix: DEVICE [n][cap] int32 or NULL, the candidate's flat pixel
 * index: colours and labels of a cloud are a gather from aw_render_views / aw_render_labels frames
 * of the same views.  count: DEVICE [n] int32, the row's number of candidates, which may exceed cap;
 * only the first min(count, cap) are stored and the slots past them are left untouched.  An env id
 * outside [0, N) leaves its row untouched, count included.
 * AW_EINVAL: as aw_render_labels (NULL xyz or count in place of NULL labels), cap outside
 * 1..AW_CLOUD_MAXCAND, frame_body outside [0, nbody), a box with lo > hi (or a NaN) on an axis.
 * AW_EUNSUPPORTED: sites 1 on a model table without the appearance arrays.
 *   aw_cloud_fps is stateless (no handle): rows xyz [n][cap][3] with count [n] candidates each ->
 * out_xyz [n][npoints][3] and out_idx [n][npoints] int32 (or NULL), all DEVICE.  With c = min(count,
 * cap) (a negative count is 0): selection 0 is candidate 0; selection k < min(npoints, c) is the
 * candidate with the largest minimum squared distance to selections 0..k-1, the lowest index on a
 * tie; slots k >= c repeat selection k mod c; with c == 0 the row is zeros and out_idx -1.  The
 * squared distance is (dx*dx + dy*dy) + dz*dz with every difference, product and sum an individually
 * rounded fp32 operation (no fused multiply-add; denormals flushed), so an fp32 restatement on the
 * host reproduces the choice bit for bit (tests/cloud_checker.py).  out_xyz is a bitwise copy of the
 * chosen candidates.  Coordinates are expected finite.
 * AW_EINVAL: n < 1, cap outside 1..AW_CLOUD_MAXCAND, npoints outside 1..AW_FPS_MAXPOINTS, NULL xyz,
 * count or out_xyz. */
#define AW_CLOUD_MAXCAND 8192
#define AW_FPS_MAXPOINTS 1024
int aw_render_cloud(aw_handle* h, const aw_view* views, int nviews, const float* env_cam,
                    const int32_t* env_ids, int n_sel, const uint8_t* keep, const float* box,
                    int frame_body, int sites, int width, int height, int cap, float* xyz, int32_t* pix,
                    int32_t* count, void* stream);
int aw_cloud_fps(int n, int cap, const float* xyz, const int32_t* count, int npoints, float* out_xyz,
                 int32_t* out_idx, void* stream);

/* Ray queries: mj_ray and the rangefinder sensor on the device.  A table of up to AW_MAX_RAYS rays,
 * each attached to a body, is cast at every env's (or a subset's) current state in one launch: per ray
 * the first render entry crossed and how far along the ray.
 *   aw_set_rays: rays is a HOST array of nrays records; the call validates it, waits for the device
 * (as aw_set_option does) and uploads it to a device table owned by the handle.  nrays == 0 drops the
 * table.  pnt, vec: origin and direction in the frame of body `body` (0 = the world, used as given);
 * the kernel composes pnt_w = xpos[b] + rot(xquat[b], pnt), vec_w = rot(xquat[b], vec) in fp32.  vec
 * need not be unit.  xmax <= 0: no limit.  keep: bit e keeps render entry e (the primitive geoms, in
 * aw_render_entries' order; bits at or above ngeom are ignored); mj_envs_amd/rays.py keep_mask
 * builds it with mj_ray's elimination rules (geomgroup, flg_static, bodyexclude, alpha 0).
 *   aw_cast_rays enqueues one launch on `stream`; it allocates nothing and does not wait.  env_ids /
 * n_sel: as in aw_dynamics -- NULL (every env, n = N, n_sel ignored) or a DEVICE array of n_sel env
 * ids, output row k is env env_ids[k]; an id outside [0, N) leaves its row untouched in both outputs.
 * env_rays: NULL, or DEVICE [N][R][6] fp32 indexed by ENV id (R = the table's nrays): env e casts ray
 * r from pnt, vec = env_rays[e][r][0..2], [3..5], expressed in the frame of rays[r].body; xmax, body
 * and keep still come from record r.  The floats are not validated: a NaN or zero vec (or a
 * non-finite pnt) is a miss, and a workgroup writes only its own row.
 *   dist: DEVICE [n][R] fp32, the x >= 0 for which pnt_w + x vec_w is the first crossing with a kept
 * entry (with a unit vec: metres) -- the smallest non-negative root (mju_rayGeom's rule), so a ray
 * that starts inside a geom reports where it leaves it; the nearest entry wins, an exact tie goes to
 * the lower entry.  -1 when nothing kept is crossed or x > xmax (xmax > 0).  entry: DEVICE [n][R]
 * int32 or NULL, the render entry crossed, -1 on a miss.  Sites are never hit.  Nothing of the
 * simulation state is written, and no appearance arrays are needed.
 *   Two deviations from mj_ray: mesh geoms are absent (not available offline; the hand's primitive
 * collision geoms are in the table), and planes are hit from both sides and are finite where their
 * size is positive, as the depth renderer draws them (mj_ray: the front face of an infinite plane).
 * AW_EINVAL, aw_set_rays: nrays outside 0..AW_MAX_RAYS, NULL rays with nrays > 0, a body outside
 * [0, nbody), a zero or non-finite vec, a non-finite pnt or xmax.  aw_cast_rays: NULL h or dist, no
 * ray table set, n_sel < 1 with env_ids given.  After either error every other call still works. */
#define AW_MAX_RAYS 256
typedef struct { float pnt[3], vec[3]; float xmax; int32_t body; uint64_t keep; } aw_ray_rec;  /* 40 bytes */
int aw_set_rays(aw_handle* h, const aw_ray_rec* rays, int nrays);
int aw_cast_rays(aw_handle* h, const int32_t* env_ids, int n_sel, const float* env_rays, float* dist,
                 int32_t* entry, void* stream);

/* On-device Gaussian MLP policy: mjrl gaussian_mlp.MLP as used by the
 * reference's DAPG baseline (algos/baselines.py:67-86, hidden_sizes=(32, 32)) -- two tanh
 * hidden layers of width `hidden` (32 or 64), in/out affine transforms, and with sample != 0
 * the Gaussian exploration noise exp(log_std) * N(0, 1) (Philox, key = seed, counter =
 * (env_offset + env, step)); sample == 0 returns the mean (get_action(...)[1]['evaluation']).
 * params: device fp32 block, layout in mj_envs_amd/csrc/aw_policy.h; obs [n][in_dim] ->
 * act [n][out_dim], in_dim <= 64, out_dim <= 32.  Stateless: no handle. */
int aw_policy_mlp(int n, int in_dim, int hidden, int out_dim, const float* params, const float* obs,
                  float* act, int sample, uint64_t seed, uint64_t step, uint64_t env_offset, void* stream);

/* Test hook: the narrowphase collider of n primitive pairs given world poses (device arrays):
 * types [n][2] (MuJoCo mjtGeom: plane 0, sphere 2, capsule 3, cylinder 5, box 6), pos [n][2][3],
 * mat [n][2][9] (row-major rotations), size [n][2][3], margin [n] -> count [n] and out
 * [n][AW_MAXPAIRCON][7] = (dist, pos[3], normal[3]) in emission order, the normal pointing from
 * the lower-type geom to the other (MuJoCo's geom1 -> geom2).  The MPR collider runs at the
 * handle's precision.  out64 (may be NULL): [n][AW_MAXPAIRCON][7] fp64, the MPR (cylinder) pairs'
 * contacts before rounding to fp32.  Used by the exact-geometry collider tests against the oracle. */
#define AW_MAXPAIRCON 8
int aw_collide_test(aw_handle* h, int n, const int32_t* types, const float* pos, const float* mat,
                    const float* size, const float* margin, float* out, int32_t* count, double* out64,
                    void* stream);

/* Test hook: the conservative midphase cull (the narrowphase's *_may_touch) of n cases (device
 * arrays): pair [n] (index into the model's pair list: explicit pairs, then candidates), and for the
 * pair's two geoms in the pair's own order pos [n][2][3], quat [n][2][4] (w x y z) and size
 * [n][2][3] -> info [n][6] = (keep, g1, g2, collider class, type of g1, type of g2) and margin [n]
 * (the pair's margin, which the cull reads from the model).  Classes 0 (plane pairs) and 1 (sphere /
 * capsule pairs) have no cull: keep = 1.  A pair index out of range: keep = -1, the rest unwritten.
 * Used by the cull soundness test: keep = 0 only where the collider emits nothing. */
int aw_midphase_test(aw_handle* h, int n, const int32_t* pair, const float* pos, const float* quat,
                     const float* size, int32_t* info, float* margin, void* stream);

/* Diagnostic: per-stage shader-clock cycles of k_step summed over all waves since the last
 * reset (40 counters, see aw_common.h PR_*).  Only libraries built with -DAW_STAGE_PROF
 * collect them; the product build returns AW_EUNSUPPORTED. */
int aw_stage_profile(unsigned long long* out, int reset);

const char* aw_last_error(void);

#ifdef __cplusplus
}
#endif

#endif /* ADROIT_WAVE_H */
