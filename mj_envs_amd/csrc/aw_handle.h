// aw_handle.h -- what the task units (aw_kernels.hip) and the API unit (aw_api.hip) share: the
// device-side state, the handle behind the C-ABI (include/adroit_wave.h), and the launcher tables
// through which the API unit reaches the kernels of a task across the link.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <type_traits>
#include <vector>

#include "../../include/adroit_wave.h"
#include "aw_common.h"

using namespace aw;

// ---------------------------------------------------------------------------------------
// device-side state owned by the handle
struct DState {
  float* qpos; float* qvel; float* warm; float* params;
  int* ep_len; float* ep_ret; int* ep_goal; int* episode; unsigned* status;
  float* last_ret; int* last_goal; int* last_len;
  unsigned* status_acc;   // OR of every step's flags since create / aw_clear_status (sticky)
  float* sum_ret;         // sum of the returns of every finished episode
  int* n_success;         // finished episodes with > success_steps goal steps (evaluate_success)
};

// the camera and look records of the render kernels (k_depth, k_rgb, k_views, k_labels): host arrays that travel as
// kernel arguments
struct CamRec {
  float c[AW_CAM_FLOATS];
};
struct LookRec {
  float c[AW_LOOK_FLOATS];
};
// the views of one aw_render_views launch (k_views): each record in the frame of its body
struct ViewsRec {
  float c[AW_MAX_VIEWS][AW_CAM_FLOATS];
  int body[AW_MAX_VIEWS];
};
// the look-up table of one aw_render_labels launch (k_labels): render entry -> label
struct LutRec {
  int v[MAXRG];
};
// the filters of one aw_render_cloud launch (k_cloud): bit e of keep is set where render entry e is
// kept (MAXRG entries: one mask), the world-frame crop box (lo xyz, hi xyz; crop 0: none), the body
// whose frame the stored points are expressed in (0: the world) and the row capacity
struct CloudRec {
  unsigned long long keep;
  float box[6];
  int crop, frame_body, cap;
};
// the point table of one aw_dynamics launch (k_dyn, aw_dyn.h): kind (AW_PT_*) and object id per point
struct DynPts {
  int kind[AW_DYN_MAXPOINTS], id[AW_DYN_MAXPOINTS];
};
// the target table of one aw_solve_ik launch (k_ik, aw_ik.h): kind (AW_PT_*), object id, the two weights
// and the first residual row of each target
struct IkTgt {
  int kind[AW_IK_MAXTARGETS], id[AW_IK_MAXTARGETS], row[AW_IK_MAXTARGETS];
  float wpos[AW_IK_MAXTARGETS], wrot[AW_IK_MAXTARGETS];
};
// the per-env appearance tables of aw_set_appearance (k_views_app): the caller's device buffers,
// [N][ne][COL_W], [N][nlight][LIGHT_W], [N][AW_LOOK_FLOATS]; nullptr: the model's / the launch's look
struct AppRec {
  const float *col, *light, *look;
  bool any() const { return col || light || look; }
};
static_assert(AW_COL_FLOATS == COL_W && AW_LIGHT_FLOATS == LIGHT_W, "the appearance records are the kernels' own");
static_assert(MAXRG <= 64, "CloudRec::keep holds one bit per render entry");

// the selection and the inputs of one k_set_state_ids launch (aw_set_state_ids, aw_clone_envs): device
// arrays; env env_ids[k] takes row rows[k] (nullptr: row k) of the non-null state and episode arrays;
// also_ids (nullptr, or aw_clone_envs' source ids): a pair is skipped when also_ids[k] is no env
struct SetIds {
  const int32_t *env_ids, *rows, *also_ids;
  int n_sel, n_rows;
  const float *qpos, *qvel, *warm, *params;
  const int32_t* ep_len;
  const float* ep_ret;
  const int32_t* ep_goal;
  int reset_episode;
};

struct TaskOps;
struct WideOps;
struct aw_handle {
  int device, nenv, NV;
  const TaskOps* ops = nullptr;   // the launchers of the model's task, fast and wide tier (aw_create)
  const WideOps* wide = nullptr;
  DModel m;
  DState st;
  void* dmodel = nullptr;
  void* dmhdr = nullptr;   // device copy of m (k_step reads its scalars from here)
  void* dstate = nullptr;
  int* next_env = nullptr;   // [0, 8): k_step's per-XCD claim counters; [8, 10 + nenv): the wide-tier
                             // queue (count, claim counter, entries; aw_step.h defer_env);
                             // [10 + nenv, 10 + 2 nenv): per-env env-step cycles, [10 + 2 nenv,
                             // 10 + 3 nenv): the claim permutation (k_order)
  int slots = 0;             // persistent k_step grid: resident workgroups of the selected instantiation,
                             // or AW_STEP_GRID (read at aw_create; 0 = one workgroup per env)
  int grid_env = -1;         // AW_STEP_GRID at create (-1: unset)
  void* dmhdr_wide = nullptr;   // the wide tier's header: m with jspill -> jspill_wide, then st
  float* jspill_wide = nullptr; // one JSPILL_WIDE block per wide workgroup
  float* mfac_wide = nullptr;   // one MFAC block per wide workgroup
  int wide_grid = 0;            // persistent k_step_wide workgroups (resident slots, capped at nenv)
  // aw_set_fault: the model table's pair margins / broadphase radii as built (restored by kind 0)
  std::vector<float> fault_margin0, fault_rb0;
  std::vector<double> fault_margin64_0;
  std::vector<int> fault_cls;
  int nsensor = 0;               // the model's sensor count = its sensordata length
  void* dsens = nullptr;         // the device SensTab (the model table's `sens`)
  float* sensordata = nullptr;   // aw_set_sensors: [nenv][nsensor], allocated on the first enable
  bool sensors = false;          // on: the SensTab's `out` points at sensordata and the step launches take the
                                 // kernels that evaluate the sensors
  void* ddata = nullptr;         // the device DataTab (the model table's `data`)
  int data_groups = 0;           // aw_set_data: the AW_DATA_* groups the kernels write (0: off) into the caller's
                                 // buffers; nonzero selects the step kernels with stage_data
  AppRec app = {nullptr, nullptr, nullptr};   // aw_set_appearance: per-env colour / light / look tables (all
  int shadows = 0;                            // nullptr: off) and cast shadows (has_appearance below)
  float* app_bounds = nullptr;          // aw_appearance_sample: the device copy of lo | hi, and what it holds
  std::vector<float> app_bounds_host;
  void* rays = nullptr;          // aw_set_rays: the device ray table (AW_MAX_RAYS records of aw_ray_rec, allocated on
  int nrays = 0;                 // the first call) and the number of rays it holds (0: no table; aw_cast_rays)
  void* clone_scratch = nullptr; // aw_clone_envs: the gathered source rows (state and episode counters of nenv
                                 // rows), allocated on the first call
};

// the handle holds appearance tables or casts shadows: its RGB frames come from k_views_app
static inline bool has_appearance(const aw_handle* h) { return h->app.any() || h->shadows; }

// resident workgroups of a one-wave kernel on the device (occupancy x CUs): a persistent grid
template <class K>
static int resident_slots(K kernel, int device) {
  int per_cu = 0, cus = 0;
  (void)hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, 64, 0);
  (void)hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device);
  return std::max(per_cu, 1) * std::max(cus, 1);
}
// launch(SENS, DATA) with the handle's switches as compile-time booleans: the step kernels'
// instantiation that also evaluates the sensors (aw_set_sensors) / writes the mjData views (aw_set_data)
template <class F>
static void with_sens_data(const aw_handle* h, F launch) {
  using T = std::true_type;
  using N = std::false_type;
  switch ((h->sensors ? 1 : 0) | (h->data_groups ? 2 : 0)) {
    case 3: launch(T{}, T{}); break;
    case 2: launch(N{}, T{}); break;
    case 1: launch(T{}, N{}); break;
    default: launch(N{}, N{}); break;
  }
}

// The launchers of one task, behind one table: task_ops<TASK> is defined (and with it every
// fast-tier kernel of TASK instantiated) only in the -DAW_TASK_TU=TASK unit of aw_kernels.hip; the
// API unit sees the declaration and calls it across the link.
struct TaskOps {
  int (*slots)(int device);
  void (*step)(aw_handle*, const float*, float*, float*, uint8_t*, uint8_t*, float*, int, uint64_t, hipStream_t);
  void (*reset)(aw_handle*, const uint8_t*, const float*, uint64_t, float*, hipStream_t);
  void (*set)(aw_handle*, const float*, const float*, const float*, const float*, float*, hipStream_t);
  void (*set_ids)(aw_handle*, const SetIds&, float*, hipStream_t);
  void (*dump)(aw_handle*, int, const float*, float*, hipStream_t);
  void (*depth)(aw_handle*, const CamRec&, int, int, float*, hipStream_t);
  void (*rgb)(aw_handle*, const CamRec&, const LookRec&, int, int, int, uint8_t*, float*, hipStream_t);
  void (*views)(aw_handle*, const ViewsRec&, int, const float*, const LookRec&, int, int, int, uint8_t*, float*,
                hipStream_t);
  void (*labels)(aw_handle*, const ViewsRec&, int, const float*, const int32_t*, int, const LutRec&, int32_t, int, int,
                 int, int32_t*, float*, hipStream_t);
  void (*cloud)(aw_handle*, const ViewsRec&, int, const float*, const int32_t*, int, const CloudRec&, int, int, int,
                float*, int32_t*, int32_t*, hipStream_t);
  void (*dyn)(aw_handle*, const int32_t*, int, const DynPts&, int, const float*, const float*, const float*,
              const aw_dyn_out&, hipStream_t);
  void (*rays)(aw_handle*, const int32_t*, int, const float*, float*, int32_t*, hipStream_t);
  void (*ik)(aw_handle*, const int32_t*, int, const IkTgt&, int, int, uint64_t, const float*, const float*,
             const aw_ik_opt&, const aw_ik_out&, hipStream_t);
};
template <int TASK> const TaskOps* task_ops();

// The wide tier's launcher table, defined in the -DAW_WIDE -DAW_TASK_TU=TASK unit of aw_kernels.hip
// (k_step_wide<TASK>): `run` drains the queue that the fast launch before it filled.
struct WideOps {
  int (*slots)(int device);
  void (*run)(aw_handle*, const float*, float*, float*, uint8_t*, uint8_t*, float*, int, uint64_t, hipStream_t);
  void (*dump)(aw_handle*, int, const float*, float*, hipStream_t);   // aw_forward_dump_wide
};
template <int TASK> const WideOps* wide_ops();

#ifdef AW_STAGE_PROF
// The stage profiler's counters (g_stage_prof) live in the fast task unit, whose kernels write them;
// that unit copies them out (out != nullptr) and zeroes them (reset) for aw_stage_profile.
hipError_t stage_prof_read(unsigned long long* out, int reset);
#endif
