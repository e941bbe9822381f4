"""ctypes binding of the C-ABI in include/adroit_wave.h (libadroit_hip.so).

The product path: every compute call goes to the HIP library.  There is no CPU fallback:
if the library is missing or cannot be loaded, ``load()`` raises.  Device memory is managed
with torch (``torch.cuda`` tensors are HIP allocations on ROCm); pointers and the current
stream are passed through as plain integers.

The boundary is stated once: ``ABI`` holds the return and argument types of every exported
function, ``_dev`` is the one check of a device tensor before its address crosses it.
"""
from __future__ import annotations

import ctypes
import os
from typing import Optional

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
# AW_LIB selects a diagnostic build (e.g. libadroit_hip_prof.so with the stage profiler)
LIB_PATH = os.environ.get("AW_LIB") or os.path.join(HERE, "libadroit_hip.so")

AW_NDIMS = 21
# the fast tier's capacities (aw_common.h FAST_*; the aw_forward_dump layout uses them); the
# effective ones are the reference model's nconmax / njmax, held by the wide tier (aw_dims)
MAXCON, MAXEFC, MAXDENSE = 48, 192, 128
NCONMAX, NJMAX = 100, 500
ST_BADQPOS, ST_BADQVEL, ST_BADQACC, ST_CON_OVERFLOW, ST_EFC_OVERFLOW, ST_WIDE = 1, 2, 4, 8, 16, 32
ST_OVERFLOW = ST_CON_OVERFLOW | ST_EFC_OVERFLOW   # constraints dropped at MuJoCo's own caps


def dump_layout(maxcon=MAXCON, maxefc=MAXEFC):
    """float offsets inside the aw_forward_dump output (aw_kernels.hip k_dump, DUMP_*)"""
    c, e = 1768, 1768 + 14 * maxcon
    return dict(xpos=(0, 96), xquat=(96, 128), site_xpos=(224, 96), qacc_smooth=(320, 36),
                qfrc_smooth=(356, 36), qacc=(392, 36), qfrc_constraint=(428, 36), qM=(464, 1296),
                scalars=(1760, 8), con_dist=(c, maxcon), con_pos=(c + maxcon, 3 * maxcon),
                con_frame=(c + 4 * maxcon, 9 * maxcon), con_pair=(c + 13 * maxcon, maxcon),
                efc_force=(e, maxefc), efc_aref=(e + maxefc, maxefc), efc_D=(e + 2 * maxefc, maxefc),
                efc_type=(e + 3 * maxefc, maxefc), efc_state=(e + 4 * maxefc, maxefc))


DUMP_LAYOUT = dump_layout()
WIDE_MAXCON_STORE, WIDE_MAXEFC = 128, 512       # the wide tier's contact storage and row slots
DUMP_LAYOUT_WIDE = dump_layout(WIDE_MAXCON_STORE, WIDE_MAXEFC)
AW_DUMP_SIZE_WIDE = 1768 + 14 * WIDE_MAXCON_STORE + 5 * WIDE_MAXEFC
# why the Newton solve stopped (aw_solver.h NT_EXIT_*)
NT_EXIT = ("max_iterations", "no_descent", "fp32_noise_floor", "improvement", "gradient", "no_constraints")
AW_DUMP_SIZE = 1768 + 14 * MAXCON + 5 * MAXEFC

# batched mjData views (include/adroit_wave.h aw_set_data): group bits, the contact record's size in
# 32-bit words and its fields as (first word, words, is_int), the largest max_contacts
AW_DATA_KIN, AW_DATA_DYN, AW_DATA_CONTACT = 1, 2, 4
AW_DATA_ALL = AW_DATA_KIN | AW_DATA_DYN | AW_DATA_CONTACT
DATA_GROUPS = {"kin": AW_DATA_KIN, "dyn": AW_DATA_DYN, "contact": AW_DATA_CONTACT}
AW_CONTACT_DWORDS = 16
AW_DATA_MAX_CONTACTS = 128
CONTACT_FIELDS = dict(dist=(0, 1, False), pos=(1, 3, False), normal=(4, 3, False), force=(7, 3, False),
                      torsion=(10, 1, False), mu=(11, 1, False), geom1=(12, 1, True), geom2=(13, 1, True),
                      dim=(14, 1, True), efc_address=(15, 1, True))
# the buffers of each group, in aw_data_bufs' order
DATA_BUFFERS = {AW_DATA_KIN: ("xpos", "xquat", "site_xpos"), AW_DATA_DYN: ("qacc", "qfrc_constraint", "counts"),
                AW_DATA_CONTACT: ("contact",)}

_lib = None
_i, _u64, _sz, _vp, _P = ctypes.c_int, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER


class DataBufs(ctypes.Structure):
    """aw_data_bufs: the caller's device buffers of aw_set_data"""
    _fields_ = [(k, _vp) for k in ("xpos", "xquat", "site_xpos", "qacc", "qfrc_constraint", "counts", "contact")]


AW_MAX_VIEWS = 4
AW_CAM_FLOATS = 17           # floats of a host camera record (mj_envs_amd/render.py)
AW_CLOUD_MAXCAND = 8192      # candidate slots per row (aw_render_cloud, aw_cloud_fps)
AW_FPS_MAXPOINTS = 1024      # sampled points per row (aw_cloud_fps)


class View(ctypes.Structure):
    """aw_view: a camera record in the frame of a body (0: the world)"""
    _fields_ = [("rec", ctypes.c_float * AW_CAM_FLOATS), ("body", ctypes.c_int32)]


class AppearanceBufs(ctypes.Structure):
    """aw_appearance (include/adroit_wave.h): the per-env colour, light and look tables, device pointers"""
    _fields_ = [("col", _vp), ("light", _vp), ("look", _vp)]


AW_COL_FLOATS, AW_LIGHT_FLOATS, AW_LOOK_FLOATS = 8, 24, 7

# dynamics queries (include/adroit_wave.h aw_dynamics): point kinds, the point capacity, the outputs in
# aw_dyn_out's order with their row shapes as functions of (nv, nbody, npoints), and which need points
AW_PT_BODY, AW_PT_BODYCOM, AW_PT_SITE = 0, 1, 2
AW_DYN_MAXPOINTS = 16
DYN_OUTPUTS = ("qM", "qMinv", "qfrc_bias", "qfrc_passive", "qfrc_actuator", "xvel", "point_pos", "point_vel",
               "jacp", "jacr")
DYN_POINT_OUTPUTS = ("point_pos", "point_vel", "jacp", "jacr")


def dyn_shape(name: str, nv: int, nbody: int, npoints: int) -> tuple:
    """row shape of one aw_dynamics output"""
    return dict(qM=(nv, nv), qMinv=(nv, nv), qfrc_bias=(nv,), qfrc_passive=(nv,), qfrc_actuator=(nv,),
                xvel=(nbody, 6), point_pos=(npoints, 3), point_vel=(npoints, 6), jacp=(npoints, 3, nv),
                jacr=(npoints, 3, nv))[name]


class DynPoint(ctypes.Structure):
    """aw_dyn_point: a point of aw_dynamics (kind AW_PT_*, body or site id)"""
    _fields_ = [("kind", ctypes.c_int32), ("id", ctypes.c_int32)]


class DynOut(ctypes.Structure):
    """aw_dyn_out: the device fp32 output buffers of aw_dynamics, NULL where not requested"""
    _fields_ = [(k, _vp) for k in DYN_OUTPUTS]


# inverse kinematics (include/adroit_wave.h aw_solve_ik): the capacities and the three records
AW_IK_MAXTARGETS, AW_IK_MAXROWS, AW_IK_MAXITER = 8, 24, 64
IK_MAXTARGETS, IK_MAXROWS, IK_MAXITER = AW_IK_MAXTARGETS, AW_IK_MAXROWS, AW_IK_MAXITER
IK_OUTPUTS = ("qpos", "err", "iters", "point_pos", "point_quat")


class IKTarget(ctypes.Structure):
    """aw_ik_target: a point of aw_solve_ik (kind AW_PT_*, body or site id) and its two weights"""
    _fields_ = [("kind", ctypes.c_int32), ("id", ctypes.c_int32), ("wpos", ctypes.c_float), ("wrot", ctypes.c_float)]


class IKOpt(ctypes.Structure):
    """aw_ik_opt: the iteration's options"""
    _fields_ = [("max_iter", ctypes.c_int32), ("damping", ctypes.c_float), ("tol", ctypes.c_float),
                ("max_step", ctypes.c_float), ("clamp_range", ctypes.c_int32)]


class IKOut(ctypes.Structure):
    """aw_ik_out: the device output buffers of aw_solve_ik, NULL where not requested (qpos is required)"""
    _fields_ = [(k, _vp) for k in IK_OUTPUTS]


def ik_shape(name: str, nq: int, ntargets: int) -> tuple:
    """row shape of one aw_solve_ik output"""
    return dict(qpos=(nq,), err=(), iters=(), point_pos=(ntargets, 3), point_quat=(ntargets, 4))[name]


def check_ik_targets(targets, nbody: int, nsite: int) -> int:
    """aw_solve_ik's rules for the target table alone: ``targets`` a list of (kind, id, wpos, wrot);
    returns the residual row count m.  ValueError names the rule: the target count, an unknown kind, an
    id out of range, a negative or non-finite weight, a target with both weights 0, more than
    ``IK_MAXROWS`` rows.  Pure: needs no GPU."""
    tg = list(targets)
    if not 1 <= len(tg) <= IK_MAXTARGETS:
        raise ValueError(f"solve_ik: {len(tg)} targets, 1..{IK_MAXTARGETS} per call")
    rows = 0
    for kind, idx, wpos, wrot in tg:
        if kind not in (AW_PT_BODY, AW_PT_BODYCOM, AW_PT_SITE):
            raise ValueError(f"solve_ik: unknown target kind {kind}")
        lim = nsite if kind == AW_PT_SITE else nbody
        if not 0 <= int(idx) < lim:
            raise ValueError(f"solve_ik: target id {idx} outside [0, {lim})")
        for w in (wpos, wrot):
            if not np.isfinite(w) or w < 0:
                raise ValueError(f"solve_ik: a weight must be finite and >= 0, not {w}")
        if wpos == 0 and wrot == 0:
            raise ValueError("solve_ik: a target with both weights 0")
        rows += (3 if wpos > 0 else 0) + (3 if wrot > 0 else 0)
    if rows > IK_MAXROWS:
        raise ValueError(f"solve_ik: {rows} residual rows, at most {IK_MAXROWS}")
    return rows


def check_ik_args(targets, dof_mask: int, nv: int, nbody: int, nsite: int, max_iter: int = 20, damping: float = 1e-4,
                  tol: float = 1e-4, max_step: float = 0.0, clamp_range=True, n_sel=None) -> int:
    """aw_solve_ik's argument rules on host values alone (nothing touches the GPU): the target table
    (``check_ik_targets``), then a ``dof_mask`` with no bit below nv, ``max_iter`` outside
    0..``IK_MAXITER``, ``damping`` not finite and > 0, ``tol`` < 0 or NaN, a non-finite ``max_step``,
    ``clamp_range`` not 0 / 1, ``n_sel`` < 1; ValueError names the rule.  Returns the row count m."""
    rows = check_ik_targets(targets, nbody, nsite)
    if isinstance(dof_mask, (bool, np.bool_)) or not isinstance(dof_mask, (int, np.integer)) or \
            not 0 <= int(dof_mask) < 1 << 64:
        raise ValueError("solve_ik: dof_mask is an unsigned 64-bit integer")
    if not int(dof_mask) & ((1 << nv) - 1):
        raise ValueError(f"solve_ik: dof_mask {int(dof_mask):#x} selects no dof below nv = {nv}")
    if isinstance(max_iter, (bool, np.bool_)) or not isinstance(max_iter, (int, np.integer)) or \
            not 0 <= max_iter <= IK_MAXITER:
        raise ValueError(f"solve_ik: max_iter must be an integer in 0..{IK_MAXITER}, not {max_iter}")
    if not (np.isfinite(damping) and damping > 0):
        raise ValueError(f"solve_ik: damping must be finite and > 0, not {damping}")
    if not tol >= 0:
        raise ValueError(f"solve_ik: tol must be >= 0, not {tol}")
    if not np.isfinite(max_step):
        raise ValueError(f"solve_ik: max_step must be finite, not {max_step}")
    if clamp_range not in (0, 1, False, True):
        raise ValueError(f"solve_ik: clamp_range must be 0 or 1, not {clamp_range}")
    if n_sel is not None and n_sel < 1:
        raise ValueError(f"solve_ik: n_sel must be >= 1, not {n_sel}")
    return rows


# ray queries (include/adroit_wave.h aw_set_rays / aw_cast_rays): the table's capacity and aw_ray_rec as a
# numpy structured type (40 bytes: pnt, vec, xmax, body, keep)
AW_MAX_RAYS = 256
RAY_DTYPE = np.dtype([("pnt", "<f4", (3,)), ("vec", "<f4", (3,)), ("xmax", "<f4"), ("body", "<i4"), ("keep", "<u8")])
assert RAY_DTYPE.itemsize == 40

# slots of a record vector [col | light | look] that aw_appearance_sample copies from ``lo``
LIGHT_FLAG_SLOTS = (18, 20, 21)
LOOK_FLAG_SLOT = 6

# Every exported function of include/adroit_wave.h, in the header's order: name -> (restype, argtypes).
# The only statement of the binding's types (tests/test_native_abi.py holds it to the header's
# prototypes): a new entry point is one line here and one method below.
ABI = {
    "aw_create": (_i, [_vp, _sz, _i, _i, _P(_vp)]),
    "aw_destroy": (_i, [_vp]),
    "aw_dims": (_i, [_vp, _P(_i)]),
    "aw_set_option": (_i, [_vp, _i, _i, _i]),
    "aw_set_tier": (_i, [_vp, _i]),
    "aw_set_fault": (_i, [_vp, _i, _i]),
    "aw_set_sensors": (_i, [_vp, _i]),
    "aw_sensor_count": (_i, [_vp]),
    "aw_sensordata": (_i, [_vp, _vp, _vp]),
    "aw_set_data": (_i, [_vp, _i, _i, _P(DataBufs)]),
    "aw_reset": (_i, [_vp, _vp, _vp, _u64, _vp, _vp]),
    "aw_step": (_i, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _i, _u64, _vp]),
    "aw_random_actions": (_i, [_vp, _u64, _u64, _vp, _vp]),
    "aw_set_env_offset": (_i, [_vp, _u64]),
    "aw_get_state": (_i, [_vp] * 6),
    "aw_set_state": (_i, [_vp] * 7),
    "aw_set_state_ids": (_i, [_vp, _vp, _i, _vp, _i, _vp, _vp, _vp, _vp, _i, _vp, _vp]),
    "aw_get_state_ids": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp, _vp]),
    "aw_clone_envs": (_i, [_vp, _vp, _vp, _i, _i, _vp, _vp]),
    "aw_status": (_i, [_vp] * 4),
    "aw_clear_status": (_i, [_vp, _vp]),
    "aw_episode_stats": (_i, [_vp] * 6),
    "aw_episode_totals": (_i, [_vp] * 5),
    "aw_set_episode_totals": (_i, [_vp] * 5),
    "aw_get_episode": (_i, [_vp] * 6),
    "aw_set_episode": (_i, [_vp] * 6),
    "aw_task_eval": (_i, [_vp, _i] + [_vp] * 11),
    "aw_forward_dump": (_i, [_vp, _i, _vp, _vp, _vp]),
    "aw_forward_dump_wide": (_i, [_vp, _i, _vp, _vp, _vp]),
    "aw_dynamics": (_i, [_vp, _vp, _i, _P(DynPoint), _i, _vp, _vp, _vp, _P(DynOut), _vp]),
    "aw_solve_ik": (_i, [_vp, _vp, _i, _P(IKTarget), _i, _u64, _vp, _vp, _P(IKOpt), _P(IKOut), _vp]),
    "aw_render_depth": (_i, [_vp, _vp, _i, _i, _vp, _vp]),
    "aw_render_rgb": (_i, [_vp, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "aw_render_views": (_i, [_vp, _P(View), _i, _vp, _vp, _i, _i, _i, _vp, _vp, _vp]),
    "aw_set_appearance": (_i, [_vp, _P(AppearanceBufs), _i]),
    "aw_appearance_defaults": (_i, [_vp, _vp, _vp, _P(_i)]),
    "aw_appearance_sample": (_i, [_vp, _vp, _vp, _vp, _i, _u64, _u64, _vp, _vp, _vp, _vp]),
    "aw_render_entries": (_i, [_vp, _P(_i), _P(_i)]),
    "aw_render_labels": (_i, [_vp, _P(View), _i, _vp, _vp, _i, _vp, _i, _i, _i, _i, _vp, _vp, _vp]),
    "aw_render_cloud": (_i, [_vp, _P(View), _i, _vp, _vp, _i, _vp, _vp] + [_i] * 5 + [_vp] * 4),
    "aw_cloud_fps": (_i, [_i, _i, _vp, _vp, _i, _vp, _vp, _vp]),
    "aw_set_rays": (_i, [_vp, _vp, _i]),
    "aw_cast_rays": (_i, [_vp, _vp, _i, _vp, _vp, _vp, _vp]),
    "aw_policy_mlp": (_i, [_i] * 4 + [_vp, _vp, _vp, _i, _u64, _u64, _u64, _vp]),
    "aw_collide_test": (_i, [_vp, _i] + [_vp] * 9),
    "aw_midphase_test": (_i, [_vp, _i] + [_vp] * 7),
    "aw_stage_profile": (_i, [_vp, _i]),
    "aw_last_error": (ctypes.c_char_p, []),
}
EXPORTS = tuple(ABI)


def data_groups(data) -> int:
    """AW_DATA_* mask of ``data``: False / None -> 0, True -> every group, a group name or an
    iterable of them ("kin", "dyn", "contact"), or the mask itself"""
    if data is None or data is False:
        return 0
    if data is True:
        return AW_DATA_ALL
    if isinstance(data, int):
        if data & ~AW_DATA_ALL or data < 0:
            raise ValueError(f"data: unknown group bits in {data}")
        return data
    names = (data,) if isinstance(data, str) else tuple(data)
    g = 0
    for k in names:
        if k not in DATA_GROUPS:
            raise ValueError(f"data: unknown group {k!r} (one of {sorted(DATA_GROUPS)})")
        g |= DATA_GROUPS[k]
    return g


class NativeError(RuntimeError):
    pass


def load():
    """Load libadroit_hip.so (raises if absent: the HIP path is the only path) and give every
    function of ``ABI`` its types.  A symbol the library lacks: with AW_LIB set (a diagnostic
    build, possibly of an older revision) it is skipped, and calling it raises AttributeError;
    without AW_LIB (the product library) ``load()`` raises NativeError naming every missing one."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NativeError(f"{LIB_PATH} not built; run `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(LIB_PATH)
    fns = {name: getattr(L, name, None) for name in ABI}
    missing = [name for name, fn in fns.items() if fn is None]
    if missing and not os.environ.get("AW_LIB"):
        raise NativeError(f"{LIB_PATH} lacks {', '.join(missing)}; rebuild it")
    for name, fn in fns.items():
        if fn is not None:
            fn.restype, fn.argtypes = ABI[name]
    _lib = L
    return L


STAGES = ("pre", "kinematics", "collision", "com_crb", "rne_smooth_solve", "constraints", "newton",
          "noslip", "jt_touch", "euler", "task_obs", "reset", "checks")
SUBSTAGES = ("nt_init", "nt_hess", "nt_chol", "nt_solve", "nt_ls", "nt_upd", "ns_minv", "ns_setup", "ns_iter",
             "co_broad", "co_narrow", "com", "rne", "co_plane", "co_round", "co_roundbox", "co_boxbox",
             "nt_hsparse", "nt_hoffd")
# timed intervals recorded in slots past the counters (stage_profile: v[39..41])
EXTRA_STAGES = ("co_kin64", "cs_sparse", "cs_j")


def stage_profile(reset: bool = True) -> dict:
    """Per-stage shader-clock cycles of k_step (diagnostic build only, see aw_stage_profile)."""
    buf = (ctypes.c_ulonglong * 44)()
    _check(load().aw_stage_profile(buf, int(reset)))
    v = list(buf)
    out = {name: v[i] for i, name in enumerate(STAGES)}
    out["waves"], out["substeps"] = v[13], v[14]
    out["newton_iters"], out["noslip_iters"], out["nefc"], out["ncon"] = v[15], v[16], v[17], v[18]
    for i, name in enumerate(SUBSTAGES):
        out[name] = v[19 + i]
    out["offd_rows"] = v[38]
    out["co_kin64"] = v[39]
    out["cs_sparse"], out["cs_j"] = v[40], v[41]
    out["mpr_pairs"], out["mpr_contacts"] = v[42], v[43]
    return out


def kernel_build_id() -> str:
    """Short hash of the HIP sources, the C-ABI header and the compile flags the product library
    is built from: ties a committed rocprof summary to the kernel revision it measured."""
    import hashlib
    import sys
    root = os.path.dirname(HERE)
    h = hashlib.sha256()
    for d in (os.path.join(HERE, "csrc"), os.path.join(root, "include")):
        for f in sorted(os.listdir(d)):
            with open(os.path.join(d, f), "rb") as fh:
                h.update(f.encode() + b"\0" + fh.read())
    if root not in sys.path:
        sys.path.insert(0, root)
    import __graft_entry__
    h.update(" ".join(__graft_entry__.HIPCC_FLAGS).encode())
    if os.environ.get("AW_LIB"):
        h.update(os.path.basename(os.environ["AW_LIB"]).encode())
    return h.hexdigest()[:12]


def _check(rc: int):
    if rc != 0:
        raise NativeError(f"adroit_wave error {rc}: {load().aw_last_error().decode()}")


def _ptr(t) -> Optional[int]:
    if t is None:
        return None
    return t.data_ptr()


def _stream():
    import torch
    return torch.cuda.current_stream().cuda_stream


def check_ids(ids, n: int, name: str = "env_ids", distinct: bool = True) -> np.ndarray:
    """Env ids (or rows) given on the host -- a list or a numpy array -- as a checked int32 vector:
    integers, each in [0, n) and (``distinct``) no id twice; ValueError otherwise.  Pure: needs no
    GPU.  (Ids given as a device int32 tensor are not checked anywhere: reading them would wait
    for the device; the library skips what is out of range, include/adroit_wave.h aw_set_state_ids.)"""
    a = np.asarray(ids)
    if a.ndim != 1 or a.size < 1:
        raise ValueError(f"{name}: a non-empty one-dimensional list of ids, not shape {a.shape}")
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError(f"{name}: integer ids, not {a.dtype}")
    if int(a.min()) < 0 or int(a.max()) >= int(n):
        bad = a[(a < 0) | (a >= int(n))]
        raise ValueError(f"{name}: id {int(bad[0])} outside [0, {int(n)})")
    if distinct and np.unique(a).size != a.size:
        u, c = np.unique(a, return_counts=True)
        raise ValueError(f"{name}: id {int(u[c > 1][0])} listed more than once")
    return np.ascontiguousarray(a, np.int32)


def _require(ok, msg: str):
    """an argument check that ``python -O`` does not remove"""
    if not ok:
        raise AssertionError(msg)


def _dev(t, what: str, dtype, shape, optional: bool = True):
    """The check of a tensor whose address goes to the library: ``t`` must be on the device,
    contiguous, of ``dtype`` and exactly of ``shape`` (a None in it leaves that dimension free;
    ``shape`` None: any shape); None passes only where ``optional``.  Returns ``t``; AssertionError
    ``"<call>: <name> must be a device <dtype> <shape>"`` otherwise (``what``: ``"<call>: <name>"``)."""
    if t is None and optional:
        return None
    ok = t is not None and getattr(t, "is_cuda", False) and t.dtype == dtype and t.is_contiguous()
    if ok and shape is not None:
        ok = t.dim() == len(shape) and all(w is None or int(d) == int(w) for d, w in zip(t.shape, shape))
    if not ok:
        dims = "" if shape is None else " [" + ", ".join("*" if w is None else str(int(w)) for w in shape) + "]"
        raise AssertionError(f"{what} must be a device {dtype}{dims}")
    return t


def _record(x, n: int, what: str):
    """a host fp32 record of exactly ``n`` floats (a camera, look or box record) as a flat array
    whose address goes to the library; None stays None"""
    if x is None:
        return None
    a = np.ascontiguousarray(x, np.float32).ravel()
    _require(a.size == n, f"{what} has {n} floats")
    return a


def _host_ptr(a):
    return None if a is None else a.ctypes.data


def _views_arg(views, call: str):
    """(aw_view array, nviews) of a list of (camera record, body) pairs"""
    arr = (View * max(len(views), 1))()
    for k, (rec, body) in enumerate(views):
        arr[k].rec[:] = _record(rec, AW_CAM_FLOATS, f"{call}: a camera record").tolist()
        arr[k].body = int(body)
    return arr, len(views)


def cloud_fps(xyz, count, out_xyz, out_idx=None, cap: Optional[int] = None, npoints: Optional[int] = None):
    """Farthest-point sampling of every row (include/adroit_wave.h aw_cloud_fps; stateless): xyz
    [n, cap, 3] (device, fp32) with count [n] (device, int32) candidates per row -> out_xyz
    [n, P, 3] (device, fp32) and optionally out_idx [n, P] (device, int32).  Selection 0 is
    candidate 0, each further one the candidate farthest from those chosen (lowest index on a tie);
    rows shorter than P repeat cyclically, an empty row is zeros / -1.  cap, npoints: handed to the
    library in place of the tensors' dimensions."""
    import torch
    _dev(xyz, "cloud_fps: xyz", torch.float32, (None, None, 3))
    _dev(out_xyz, "cloud_fps: out_xyz", torch.float32, (None, None, 3))
    _dev(count, "cloud_fps: count", torch.int32, (None,))
    n = int(count.shape[0]) if count is not None else int(xyz.shape[0])
    if cap is None:
        cap = int(xyz.shape[1])
    if npoints is None:
        npoints = int(out_xyz.shape[1])
    # a count the library refuses may be handed through; one it accepts is the row stride it works with
    if xyz is not None:
        _require(xyz.shape[0] == n and (cap == xyz.shape[1] or not 1 <= cap <= AW_CLOUD_MAXCAND),
                 "cloud_fps: cap is xyz's second dimension")
    if out_xyz is not None:
        _require(out_xyz.shape[0] == n and (npoints == out_xyz.shape[1] or not 1 <= npoints <= AW_FPS_MAXPOINTS),
                 "cloud_fps: npoints is out_xyz's second dimension")
    if out_idx is not None:
        _require(out_xyz is not None, "cloud_fps: out_idx needs out_xyz")
        _dev(out_idx, "cloud_fps: out_idx", torch.int32, tuple(out_xyz.shape[:2]))
    _check(load().aw_cloud_fps(n, int(cap), _ptr(xyz), _ptr(count), int(npoints), _ptr(out_xyz), _ptr(out_idx),
                               _stream()))


class Sim:
    """One batch of ``n_envs`` envs of one task on one GPU (owns the device state)."""

    def __init__(self, blob: bytes, n_envs: int, device: int = 0, env_offset: int = 0):
        import torch
        L = load()
        self.device = device
        self.torch_device = torch.device("cuda", device)
        self._blob = ctypes.create_string_buffer(blob, len(blob))
        h = _vp()
        with torch.cuda.device(device):
            _check(L.aw_create(self._blob, len(blob), n_envs, device, ctypes.byref(h)))
        self.h = h
        d = (ctypes.c_int * AW_NDIMS)()
        _check(L.aw_dims(self.h, d))
        (self.nq, self.nv, self.nu, self.obs_dim, self.nparam, self.frame_skip, self.horizon,
         self.task_kind, self.n_envs, self.nbody, self.nsite, self.ngeom, self.npair,
         self.maxcon, self.maxefc, self.maxdense, self.grid, self.fast_maxcon, self.fast_maxefc,
         self.fast_maxdense, self.wide_grid) = list(d)
        # the model's sensordata length (65 / 66); 0 with an older diagnostic library (AW_LIB)
        self.nsensordata = int(L.aw_sensor_count(self.h)) if hasattr(L, "aw_sensor_count") else 0
        self.env_offset = 0
        if env_offset:
            self.set_env_offset(env_offset)

    def set_env_offset(self, env_offset: int):
        """global id of env 0 (shards): Philox streams are keyed by the global env id"""
        _check(load().aw_set_env_offset(self.h, int(env_offset)))
        self.env_offset = int(env_offset)

    def close(self):
        if getattr(self, "h", None):
            load().aw_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # --- buffers ---------------------------------------------------------------------------
    def empty(self, *shape, dtype=None):
        import torch
        return torch.empty(*shape, dtype=dtype or torch.float32, device=self.torch_device)

    def set_option(self, disableflags: int = -1, iterations: int = -1, noslip_iterations: int = -1):
        _check(load().aw_set_option(self.h, disableflags, iterations, noslip_iterations))

    def set_tier(self, mode: int):
        """0: automatic (fast tier, wide tier for overflowing env-steps); 1: wide tier only (tests)"""
        _check(load().aw_set_tier(self.h, int(mode)))

    def set_sensors(self, enable: bool):
        """MuJoCo's sensordata on or off (off at create): on, every step / reset / set_state also
        evaluates the model's sensors into a device buffer [n_envs, nsensordata], read with
        ``sensordata`` (include/adroit_wave.h aw_set_sensors); off, the step is the kernel it was"""
        _check(load().aw_set_sensors(self.h, int(bool(enable))))

    def sensordata(self, out):
        """copy the sensor buffer into out [n_envs, nsensordata] (device, fp32); raises while
        sensors are off"""
        import torch
        _dev(out, "sensordata: out", torch.float32, (self.n_envs, self.nsensordata), optional=False)
        _check(load().aw_sensordata(self.h, _ptr(out), _stream()))
        return out

    def set_data(self, groups, max_contacts: int = 32, bufs: Optional[dict] = None):
        """Batched mjData views on or off (include/adroit_wave.h aw_set_data).  ``groups``: an
        AW_DATA_* mask, True, or group names ("kin", "dyn", "contact"); 0 / False disables.  Allocates
        the requested groups' device tensors (zero until an env's next step, reset or set_state),
        keeps them alive for as long as the kernels write them, and returns them by name: xpos
        [N, nbody, 3], xquat [N, nbody, 4], site_xpos [N, nsite, 3], qacc / qfrc_constraint [N, nv]
        (fp32), counts [N, 4] (int32: ncon, nefc, Newton iterations, noslip iterations), contact
        [N, max_contacts, AW_CONTACT_DWORDS] (fp32 words; CONTACT_FIELDS; the integer fields are
        read with ``.view(torch.int32)``).  ``bufs`` supplies tensors of the caller's instead
        (contiguous, at least those sizes): the kernels write them in place."""
        import torch
        g = data_groups(groups)
        n, K = self.n_envs, int(max_contacts)
        shapes = dict(xpos=(n, self.nbody, 3), xquat=(n, self.nbody, 4), site_xpos=(n, self.nsite, 3),
                      qacc=(n, self.nv), qfrc_constraint=(n, self.nv), counts=(n, 4),
                      contact=(n, max(K, 0), AW_CONTACT_DWORDS))
        out, c = {}, DataBufs()
        if g and 1 <= K <= AW_DATA_MAX_CONTACTS:      # (the library reports a bad max_contacts)
            for bit, names in DATA_BUFFERS.items():
                if not g & bit:
                    continue
                for k in names:
                    dt = torch.int32 if k == "counts" else torch.float32
                    t = bufs[k] if bufs and k in bufs else torch.zeros(shapes[k], dtype=dt, device=self.torch_device)
                    need = int(np.prod(shapes[k]))
                    _dev(t, f"set_data: {k}", dt, None, optional=False)
                    _require(t.numel() >= need, f"set_data: {k} must hold >= {need} elements")
                    out[k] = t
                    setattr(c, k, t.data_ptr())
        _check(load().aw_set_data(self.h, g, K, ctypes.byref(c)))
        self._data_bufs = out                         # the kernels write these until the next set_data
        self.data_groups, self.max_contacts = g, K
        return out

    def set_fault(self, kind: int, arg: int = 0):
        """test hook (include/adroit_wave.h aw_set_fault): 0 none, 1 class-1 margins + arg um,
        2 frictionloss row `arg` held in the stick state"""
        _check(load().aw_set_fault(self.h, int(kind), int(arg)))

    def reset(self, obs, params=None, mask=None, seed: int = 1):
        _check(load().aw_reset(self.h, _ptr(mask), _ptr(params), seed, _ptr(obs), _stream()))

    def step(self, actions, obs, reward, done, goal, terminal_obs=None, autoreset: bool = False,
             seed: int = 1):
        _check(load().aw_step(self.h, _ptr(actions), _ptr(obs), _ptr(reward), _ptr(done), _ptr(goal),
                              _ptr(terminal_obs), int(autoreset), seed, _stream()))

    def random_actions(self, out, seed: int, step: int):
        _check(load().aw_random_actions(self.h, seed, step, _ptr(out), _stream()))

    def get_state(self, qpos=None, qvel=None, warm=None, params=None):
        _check(load().aw_get_state(self.h, _ptr(qpos), _ptr(qvel), _ptr(warm), _ptr(params), _stream()))

    def set_state(self, qpos=None, qvel=None, warm=None, params=None, obs=None):
        _check(load().aw_set_state(self.h, _ptr(qpos), _ptr(qvel), _ptr(warm), _ptr(params), _ptr(obs),
                                   _stream()))

    def _rows(self, call: str, n: int, **arrays):
        """the per-row arrays of a call: device fp32 [n, nq | nv | nv | nparam | nu] or None"""
        import torch
        width = dict(qpos=self.nq, qvel=self.nv, warm=self.nv, params=self.nparam, ctrl=self.nu)
        for k, t in arrays.items():
            _dev(t, f"{call}: {k}", torch.float32, (n, width[k]))

    def _n_sel(self, call: str, env_ids) -> int:
        """rows of a call that selects envs with ``env_ids`` (a device int32 vector; None: every env)"""
        import torch
        if _dev(env_ids, f"{call}: env_ids", torch.int32, (None,)) is None:
            return self.n_envs
        return int(env_ids.shape[0])

    def set_state_ids(self, env_ids, rows=None, n_rows: Optional[int] = None, qpos=None, qvel=None, warm=None,
                      params=None, reset_episode: bool = False, obs=None):
        """Set env env_ids[k] from row rows[k] (None: row k) of the given [n_rows, ...] arrays and run
        its forward (include/adroit_wave.h aw_set_state_ids).  env_ids, rows: device int32 vectors, not
        validated (the library skips ids and rows out of range; env_ids must be distinct).  obs:
        [n_envs, obs_dim], indexed by env id; only the selected envs' rows are written."""
        import torch
        given = [t for t in (qpos, qvel, warm, params) if t is not None]
        _dev(env_ids, "set_state_ids: env_ids", torch.int32, (None,), optional=False)
        n_sel = int(env_ids.shape[0])
        _dev(rows, "set_state_ids: rows", torch.int32, (n_sel,))
        if n_rows is None:
            n_rows = int(given[0].shape[0]) if given else n_sel
        self._rows("set_state_ids", n_rows, qpos=qpos, qvel=qvel, warm=warm, params=params)
        _dev(obs, "set_state_ids: obs", torch.float32, (self.n_envs, self.obs_dim))
        _check(load().aw_set_state_ids(self.h, _ptr(env_ids), n_sel, _ptr(rows), int(n_rows), _ptr(qpos), _ptr(qvel),
                                       _ptr(warm), _ptr(params), int(bool(reset_episode)), _ptr(obs), _stream()))

    def get_state_ids(self, env_ids, qpos=None, qvel=None, warm=None, params=None):
        """row k of the given [n_sel, ...] arrays receives env env_ids[k] (device int32; an id out of
        range leaves its row as it was): include/adroit_wave.h aw_get_state_ids"""
        import torch
        _dev(env_ids, "get_state_ids: env_ids", torch.int32, (None,), optional=False)
        n_sel = int(env_ids.shape[0])
        self._rows("get_state_ids", n_sel, qpos=qpos, qvel=qvel, warm=warm, params=params)
        _check(load().aw_get_state_ids(self.h, _ptr(env_ids), n_sel, _ptr(qpos), _ptr(qvel), _ptr(warm), _ptr(params),
                                       _stream()))

    def clone_envs(self, src_ids, dst_ids, episode: bool = True, obs=None):
        """env dst_ids[k] becomes a copy of env src_ids[k] (device int32 vectors; every read before any
        write; dst_ids distinct), then the forward of the dst envs: include/adroit_wave.h aw_clone_envs.
        The first call allocates the handle's scratch block."""
        import torch
        _dev(src_ids, "clone_envs: src_ids", torch.int32, (None,), optional=False)
        n = int(src_ids.shape[0])
        _dev(dst_ids, "clone_envs: dst_ids", torch.int32, (n,), optional=False)
        _dev(obs, "clone_envs: obs", torch.float32, (self.n_envs, self.obs_dim))
        _check(load().aw_clone_envs(self.h, _ptr(src_ids), _ptr(dst_ids), n, int(bool(episode)), _ptr(obs),
                                    _stream()))

    def status(self, last=None, sticky=None):
        """per-env flags (ST_*): of the last step (last) / OR since create or clear_status (sticky)"""
        _check(load().aw_status(self.h, _ptr(last), _ptr(sticky), _stream()))

    def clear_status(self):
        _check(load().aw_clear_status(self.h, _stream()))

    def episode_totals(self, episodes=None, sum_return=None, successes=None):
        _check(load().aw_episode_totals(self.h, _ptr(episodes), _ptr(sum_return), _ptr(successes), _stream()))

    def set_episode_totals(self, episodes=None, sum_return=None, successes=None):
        """restore the running totals (checkpoint); see include/adroit_wave.h aw_set_episode_totals"""
        _check(load().aw_set_episode_totals(self.h, _ptr(episodes), _ptr(sum_return), _ptr(successes), _stream()))

    def get_episode(self, ep_len=None, ep_ret=None, ep_goal=None, episodes=None):
        _check(load().aw_get_episode(self.h, _ptr(ep_len), _ptr(ep_ret), _ptr(ep_goal), _ptr(episodes),
                                     _stream()))

    def set_episode(self, ep_len=None, ep_ret=None, ep_goal=None, episodes=None):
        _check(load().aw_set_episode(self.h, _ptr(ep_len), _ptr(ep_ret), _ptr(ep_goal), _ptr(episodes),
                                     _stream()))

    def episode_stats(self, last_return=None, last_goal=None, last_len=None, episodes=None):
        _check(load().aw_episode_stats(self.h, _ptr(last_return), _ptr(last_goal), _ptr(last_len),
                                       _ptr(episodes), _stream()))

    def task_eval(self, n, qpos, qvel, xpos, xquat, site_xpos, touch, obs, reward, done, goal):
        _check(load().aw_task_eval(self.h, n, _ptr(qpos), _ptr(qvel), _ptr(xpos), _ptr(xquat),
                                   _ptr(site_xpos), _ptr(touch), _ptr(obs), _ptr(reward), _ptr(done),
                                   _ptr(goal), _stream()))

    def render_depth(self, out, cam: np.ndarray):
        """Depth frames of every env's current state into out [N, H, W] (device, fp32);
        cam: the host camera record of mj_envs_amd.render.free_camera."""
        import torch
        _dev(out, "render_depth: out", torch.float32, (self.n_envs, None, None), optional=False)
        _, h, w = out.shape
        c = _record(cam, AW_CAM_FLOATS, "render_depth: camera record")
        _check(load().aw_render_depth(self.h, _host_ptr(c), w, h, _ptr(out), _stream()))

    def render_rgb(self, out, cam: np.ndarray, look: Optional[np.ndarray] = None, ss: int = 1, depth=None):
        """Colour frames of every env's current state into out [N, H, W, 3] (device, uint8) and,
        with depth [N, H, W] (device, fp32; ss must be 1), the aligned depth frames of the same
        launch.  cam: the host camera record of mj_envs_amd.render.free_camera; look: 7 host floats
        (background rgb, headlight ambient / diffuse / specular, headlight on) or None for the
        defaults (include/adroit_wave.h aw_render_rgb)."""
        import torch
        _dev(out, "render_rgb: out", torch.uint8, (self.n_envs, None, None, 3), optional=False)
        n, h, w, _ = out.shape
        _dev(depth, "render_rgb: depth", torch.float32, (n, h, w))
        c = _record(cam, AW_CAM_FLOATS, "render_rgb: camera record")
        lk = _record(look, AW_LOOK_FLOATS, "render_rgb: look record")
        _check(load().aw_render_rgb(self.h, _host_ptr(c), _host_ptr(lk), w, h, int(ss), _ptr(out), _ptr(depth),
                                    _stream()))

    def render_views(self, views, width: int, height: int, rgb=None, depth=None, env_cam=None,
                     look: Optional[np.ndarray] = None, ss: int = 1):
        """Every view of every env's current state in one launch (include/adroit_wave.h
        aw_render_views).  views: a list of (record, body) pairs -- a 17-float host camera record in
        the frame of body ``body`` (0: the world; mj_envs_amd.render model_camera / mounted_camera,
        or (free_camera(...), 0)); rgb [N, V, H, W, 3] (device, uint8) and / or depth [N, V, H, W]
        (device, fp32; ss must be 1); env_cam [N, V, 17] (device, fp32): per-env records used in
        place of the views' own; look as in render_rgb."""
        import torch
        arr, nv = _views_arg(views, "render_views")
        n, w, h = self.n_envs, int(width), int(height)
        _dev(rgb, "render_views: rgb", torch.uint8, (n, nv, h, w, 3))
        _dev(depth, "render_views: depth", torch.float32, (n, nv, h, w))
        _dev(env_cam, "render_views: env_cam", torch.float32, (n, nv, AW_CAM_FLOATS))
        lk = _record(look, AW_LOOK_FLOATS, "render_views: look record")
        _check(load().aw_render_views(self.h, arr, nv, _ptr(env_cam), _host_ptr(lk), w, h, int(ss), _ptr(rgb),
                                      _ptr(depth), _stream()))

    def set_appearance(self, colors=None, lights=None, look=None, shadows: bool = False):
        """Per-env appearance tables and cast shadows of the colour frames (include/adroit_wave.h
        aw_set_appearance).  colors [n_envs, ne, 8], lights [n_envs, nlight, 24], look [n_envs, 7]:
        contiguous fp32 device tensors or None (the model's records / the call's host look); the
        handle keeps references, so they stay alive until they are replaced.  All None and
        ``shadows`` False: everything off.  Waits for the device."""
        import torch
        ne, nl = sum(self.render_entries()), self.appearance_defaults()[1].shape[0]
        _dev(colors, "set_appearance: colors", torch.float32, (self.n_envs, ne, AW_COL_FLOATS))
        _dev(lights, "set_appearance: lights", torch.float32, (self.n_envs, nl, AW_LIGHT_FLOATS))
        _dev(look, "set_appearance: look", torch.float32, (self.n_envs, AW_LOOK_FLOATS))
        bufs = None
        if colors is not None or lights is not None or look is not None:
            bufs = AppearanceBufs(_ptr(colors), _ptr(lights), _ptr(look))
        _check(load().aw_set_appearance(self.h, None if bufs is None else ctypes.byref(bufs), int(shadows)))
        self._appearance = (colors, lights, look)

    def appearance_defaults(self):
        """(colors [ne, 8], lights [nlight, 24]): the model's own records as host fp32 arrays
        (include/adroit_wave.h aw_appearance_defaults)"""
        nl = ctypes.c_int()
        _check(load().aw_appearance_defaults(self.h, None, None, ctypes.byref(nl)))
        col = np.zeros((sum(self.render_entries()), AW_COL_FLOATS), np.float32)
        light = np.zeros((nl.value, AW_LIGHT_FLOATS), np.float32)
        _check(load().aw_appearance_defaults(self.h, col.ctypes.data, light.ctypes.data, None))
        return col, light

    def appearance_sample(self, lo, hi, colors=None, lights=None, look=None, env_ids=None, seed: int = 0,
                          draw: int = 0, n_sel: Optional[int] = None):
        """Draw per-env appearance records on the device between the host bounds ``lo`` / ``hi``
        (record vectors [col | light | look]; include/adroit_wave.h aw_appearance_sample) into the
        given device tensors (None: not written).  env_ids: a device int32 vector, only those rows
        are written (None: every env)."""
        import torch
        n = 0
        if _dev(env_ids, "appearance_sample: env_ids", torch.int32, (None,)) is not None:
            n = env_ids.numel() if n_sel is None else int(n_sel)
        for k, t in (("colors", colors), ("lights", lights), ("look", look)):     # (the first dimension only)
            _dev(t, f"appearance_sample: {k}", torch.float32,
                 None if t is None else (self.n_envs,) + (None,) * (len(t.shape) - 1))
        ng, ns = self.render_entries()
        nf = (ng + ns) * AW_COL_FLOATS + AW_LOOK_FLOATS
        nf += AW_LIGHT_FLOATS * (lights.shape[1] if lights is not None else self.appearance_defaults()[1].shape[0])
        lo = _record(lo, nf, "appearance_sample: lo")
        hi = _record(hi, nf, "appearance_sample: hi")
        _check(load().aw_appearance_sample(self.h, lo.ctypes.data, hi.ctypes.data, _ptr(env_ids), n, int(seed), int(draw),
                                           _ptr(colors), _ptr(lights), _ptr(look), _stream()))

    def render_entries(self):
        """(ngeom, nsite) of the ray caster's render entries: the primitive geoms in model order, then
        the visible sites in site order (include/adroit_wave.h aw_render_entries)"""
        ng, ns = ctypes.c_int(0), ctypes.c_int(0)
        _check(load().aw_render_entries(self.h, ctypes.byref(ng), ctypes.byref(ns)))
        return ng.value, ns.value

    def render_labels(self, views, width: int, height: int, labels, depth=None, env_cam=None, env_ids=None,
                      lut=None, background: int = -1, sites=0, n_sel: Optional[int] = None):
        """Segmentation frames of every view in one launch (include/adroit_wave.h aw_render_labels).
        views, env_cam: as in render_views (env_cam is [n_envs, V, 17] whatever env_ids selects);
        env_ids [n] (device, int32): output row k shows env env_ids[k] (None: every env, n = n_envs);
        labels [n, V, H, W] (device, int32) and optionally depth [n, V, H, W] (device, fp32);
        lut: host ints, one label per render entry (None: the entry index); background: the label
        of a pixel that shows nothing; sites 1: the visible sites are drawn too.  n_sel: the count
        handed to the library with env_ids (default: their number)."""
        import torch
        arr, nv = _views_arg(views, "render_labels")
        w, h = int(width), int(height)
        n = self._n_sel("render_labels", env_ids)
        _dev(labels, "render_labels: labels", torch.int32, (n, nv, h, w))
        _dev(depth, "render_labels: depth", torch.float32, (n, nv, h, w))
        _dev(env_cam, "render_labels: env_cam", torch.float32, (self.n_envs, nv, AW_CAM_FLOATS))
        lt = None
        if lut is not None:
            lt = np.ascontiguousarray(lut, np.int32)
            _require(lt.ndim == 1 and lt.size == sum(self.render_entries()),
                     "render_labels: lut has one label per render entry")
        _check(load().aw_render_labels(self.h, arr, nv, _ptr(env_cam), _ptr(env_ids), n if n_sel is None else int(n_sel),
                                       _host_ptr(lt), int(background), int(sites), w, h, _ptr(labels), _ptr(depth),
                                       _stream()))

    def render_cloud(self, views, width: int, height: int, xyz, count, pix=None, keep=None, box=None,
                     frame_body: int = 0, sites=0, env_cam=None, env_ids=None, cap: Optional[int] = None,
                     n_sel: Optional[int] = None):
        """Point-cloud candidates of every view in one launch (include/adroit_wave.h aw_render_cloud):
        the pixels that hit a kept render entry inside the crop box, unprojected, in ascending flat
        pixel order.  views, env_cam, env_ids, sites, n_sel: as in render_labels.  xyz [n, cap, 3]
        (device, fp32), count [n] (device, int32: the row's candidates, possibly more than cap) and
        optionally pix [n, cap] (device, int32: flat pixel index v * H * W + row * W + col).
        keep: host bytes, one per render entry (None: all kept); box: 6 host floats, lo xyz then hi
        xyz in the world frame (None: no crop); frame_body: the body whose frame the stored points
        are expressed in (0: the world).  cap: the capacity handed to the library (default, and the
        only one it accepts: xyz's second dimension)."""
        import torch
        arr, nv = _views_arg(views, "render_cloud")
        w, h = int(width), int(height)
        n = self._n_sel("render_cloud", env_ids)
        if _dev(xyz, "render_cloud: xyz", torch.float32, (n, None, 3)) is not None:
            if cap is None:
                cap = int(xyz.shape[1])
            # a cap the library refuses may be handed through; one it accepts is the row stride it writes with
            _require(cap == xyz.shape[1] or not 1 <= cap <= AW_CLOUD_MAXCAND,
                     "render_cloud: cap is xyz's second dimension")
        _dev(count, "render_cloud: count", torch.int32, (n,))
        if pix is not None:
            _require(xyz is not None, "render_cloud: pix needs xyz")
            _dev(pix, "render_cloud: pix", torch.int32, tuple(xyz.shape[:2]))
        _dev(env_cam, "render_cloud: env_cam", torch.float32, (self.n_envs, nv, AW_CAM_FLOATS))
        kp = None
        if keep is not None:
            kp = np.ascontiguousarray(np.asarray(keep) != 0, np.uint8)
            _require(kp.ndim == 1 and kp.size == sum(self.render_entries()),
                     "render_cloud: keep has one byte per render entry")
        bx = _record(box, 6, "render_cloud: box (lo xyz, hi xyz)")
        _check(load().aw_render_cloud(self.h, arr, nv, _ptr(env_cam), _ptr(env_ids), n if n_sel is None else int(n_sel),
                                      _host_ptr(kp), _host_ptr(bx), int(frame_body), int(sites), w, h,
                                      0 if cap is None else int(cap), _ptr(xyz), _ptr(pix), _ptr(count), _stream()))

    def collide_test(self, types, pos, mat, size, margin, fp64: bool = False):
        """narrowphase of n primitive pairs (test hook): list of arrays [(dist, pos[3], normal[3]), ...]
        (fp64: the MPR pairs' fp64 results instead of the fp32 contacts)"""
        import torch
        n = len(types)
        dev = self.torch_device
        t = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device=dev).contiguous()
        out = torch.zeros(n, 8, 7, device=dev)
        cnt = torch.zeros(n, dtype=torch.int32, device=dev)
        out64 = torch.zeros(n, 8, 7, dtype=torch.float64, device=dev) if fp64 else None
        args = [t(types, torch.int32), t(pos), t(mat), t(size), t(margin)]   # alive until the kernel ran
        _check(load().aw_collide_test(self.h, n, *[_ptr(a) for a in args], _ptr(out), _ptr(cnt), _ptr(out64),
                                      _stream()))
        o = (out64 if fp64 else out).cpu().numpy().astype(np.float64)
        c = cnt.cpu().numpy()
        return [o[i, :c[i]] for i in range(n)]

    def midphase_test(self, pair, pos, quat, size):
        """midphase cull of n cases (test hook): pair [n] model pair ids, pos [n, 2, 3], quat [n, 2, 4],
        size [n, 2, 3] of the pair's geoms in its own order -> dict of numpy arrays keep, g1, g2, cls,
        type1, type2 (int32 [n]) and margin (fp32 [n], the pair's)"""
        import torch
        n = len(pair)
        dev = self.torch_device
        t = lambda a, dt=torch.float32: torch.tensor(np.asarray(a), dtype=dt, device=dev).contiguous()
        args = [t(pair, torch.int32), t(pos), t(quat), t(size)]   # alive until the kernel ran
        _require(args[1].numel() == 6 * n and args[2].numel() == 8 * n and args[3].numel() == 6 * n,
                 "midphase_test: pos [n, 2, 3], quat [n, 2, 4], size [n, 2, 3]")
        info = torch.zeros(n, 6, dtype=torch.int32, device=dev)
        mg = torch.zeros(n, device=dev)
        _check(load().aw_midphase_test(self.h, n, *[_ptr(a) for a in args], _ptr(info), _ptr(mg), _stream()))
        i = info.cpu().numpy()
        return dict(keep=i[:, 0], g1=i[:, 1], g2=i[:, 2], cls=i[:, 3], type1=i[:, 4], type2=i[:, 5],
                    margin=mg.cpu().numpy())

    def dynamics(self, out: dict, points=(), env_ids=None, qpos=None, qvel=None, ctrl=None,
                 n_sel: Optional[int] = None, npoints: Optional[int] = None):
        """Dynamics queries of the selected envs in one launch (include/adroit_wave.h aw_dynamics).
        out: name -> device fp32 tensor for the outputs wanted (DYN_OUTPUTS; [n, ...] with the row
        shapes of ``dyn_shape``), written in place.  points: host (kind, id) pairs (AW_PT_*).  env_ids
        [n] (device, int32): output row k is env env_ids[k] (None: every env, n = n_envs).  qpos
        [n, nq], qvel [n, nv] (device, fp32): replace the env's own state for this evaluation only;
        ctrl [n, nu]: raw controls for qfrc_actuator (None: zero).  n_sel, npoints: the counts handed
        to the library in place of the arguments' own lengths."""
        import torch
        pts = list(points)
        arr = (DynPoint * max(len(pts), 1))()
        for k, (kind, idx) in enumerate(pts):
            arr[k].kind, arr[k].id = int(kind), int(idx)
        n, npt = self._n_sel("dynamics", env_ids), len(pts)
        unknown = set(out) - set(DYN_OUTPUTS)
        _require(not unknown, f"dynamics: unknown outputs {sorted(unknown)}")
        c = DynOut()
        for k, t in out.items():
            if _dev(t, f"dynamics: {k}", torch.float32, (n,) + dyn_shape(k, self.nv, self.nbody, npt)) is not None:
                setattr(c, k, t.data_ptr())
        self._rows("dynamics", n, qpos=qpos, qvel=qvel, ctrl=ctrl)
        _check(load().aw_dynamics(self.h, _ptr(env_ids), n if n_sel is None else int(n_sel), arr,
                                  npt if npoints is None else int(npoints), _ptr(qpos), _ptr(qvel), _ptr(ctrl),
                                  ctypes.byref(c), _stream()))

    def solve_ik(self, out: dict, targets, goal, dof_mask: int, env_ids=None, qpos0=None, max_iter: int = 20,
                 damping: float = 1e-4, tol: float = 1e-4, max_step: float = 0.0, clamp_range=True,
                 n_sel: Optional[int] = None):
        """Damped-least-squares inverse kinematics of the selected envs in one launch
        (include/adroit_wave.h aw_solve_ik).  out: name -> device tensor, written in place: qpos
        [n, nq] (required), err [n] (fp32), iters [n] (int32), point_pos [n, T, 3], point_quat [n, T, 4].
        targets: host (kind, id, wpos, wrot) records (AW_PT_*).  goal [n, T, 7] (device, fp32): position
        xyz and quaternion wxyz per target, by output row.  dof_mask: bit i lets dof i move.  env_ids [n]
        (device, int32): output row k is env env_ids[k] (None: every env).  qpos0 [n, nq] (device, fp32):
        the start, by output row (None: the env's stored qpos).  The host values are checked with
        ``check_ik_args`` (ValueError) before anything reaches the library."""
        import torch
        tg = [(int(k), int(i), float(wp), float(wr)) for k, i, wp, wr in targets]
        n = self._n_sel("solve_ik", env_ids)
        check_ik_args(tg, dof_mask, self.nv, self.nbody, self.nsite, max_iter, damping, tol, max_step, clamp_range,
                      n_sel if env_ids is not None else None)
        unknown = set(out) - set(IK_OUTPUTS)
        _require(not unknown, f"solve_ik: unknown outputs {sorted(unknown)}")
        arr = (IKTarget * len(tg))(*[IKTarget(*t) for t in tg])
        c = IKOut()
        for k in IK_OUTPUTS:
            t = _dev(out.get(k), f"solve_ik: {k}", torch.int32 if k == "iters" else torch.float32,
                     (n,) + ik_shape(k, self.nq, len(tg)), optional=k != "qpos")
            if t is not None:
                setattr(c, k, t.data_ptr())
        _dev(goal, "solve_ik: goal", torch.float32, (n, len(tg), 7), optional=False)
        self._rows("solve_ik", n, qpos=qpos0)
        opt = IKOpt(int(max_iter), float(damping), float(tol), float(max_step), int(clamp_range))
        _check(load().aw_solve_ik(self.h, _ptr(env_ids), n if n_sel is None else int(n_sel), arr, len(tg),
                                  int(dof_mask), _ptr(goal), _ptr(qpos0), ctypes.byref(opt), ctypes.byref(c), _stream()))

    def set_rays(self, records, nrays: Optional[int] = None):
        """Upload the handle's ray table (include/adroit_wave.h aw_set_rays): ``records`` a host array
        of ``RAY_DTYPE`` (mj_envs_amd/rays.py builds them), or None / empty to drop the table.  The
        library validates the records (NativeError on a bad one) and waits for the device.  nrays:
        the count handed to the library in place of the array's length."""
        rec = None if records is None else np.ascontiguousarray(records, RAY_DTYPE).ravel()
        n = (0 if rec is None else int(rec.size)) if nrays is None else int(nrays)
        # a count the library refuses may be handed through; one it accepts must lie inside the array it reads
        _require(rec is None or n <= rec.size or n > AW_MAX_RAYS, "set_rays: nrays exceeds the records given")
        _check(load().aw_set_rays(self.h, None if rec is None or rec.size == 0 else rec.ctypes.data, n))
        self.nrays = n

    def cast_rays(self, dist, entry=None, env_ids=None, env_rays=None, n_sel: Optional[int] = None):
        """Cast the ray table at the selected envs' current state in one launch (include/adroit_wave.h
        aw_cast_rays).  dist [n, R] (device, fp32): the x of the first crossing along pnt + x vec, -1
        on a miss; entry [n, R] (device, int32) or None: the render entry crossed, -1 on a miss.
        env_ids [n] (device, int32): output row k is env env_ids[k] (None: every env, n = n_envs).
        env_rays [n_envs, R, 6] (device, fp32, indexed by env id): per-env pnt and vec in place of
        the records' own.  n_sel: the count handed to the library with env_ids."""
        import torch
        n, R = self._n_sel("cast_rays", env_ids), getattr(self, "nrays", 0)
        _dev(dist, "cast_rays: dist", torch.float32, (n, R))
        _dev(entry, "cast_rays: entry", torch.int32, (n, R))
        _dev(env_rays, "cast_rays: env_rays", torch.float32, (self.n_envs, R, 6))
        _check(load().aw_cast_rays(self.h, _ptr(env_ids), n if n_sel is None else int(n_sel), _ptr(env_rays),
                                   _ptr(dist), _ptr(entry), _stream()))

    def forward_dump(self, env: int, ctrl=None, wide: bool = False) -> dict:
        """one forward of env `env` (ctrl: raw controls or None = 0) and its internals; wide=True runs it
        through the wide-capacity tier (aw_forward_dump_wide: MuJoCo's nconmax / njmax)"""
        out = self.empty(AW_DUMP_SIZE_WIDE if wide else AW_DUMP_SIZE)
        fn = load().aw_forward_dump_wide if wide else load().aw_forward_dump
        _check(fn(self.h, env, _ptr(ctrl), _ptr(out), _stream()))
        o = out.cpu().numpy().astype(np.float64)
        res = {k: o[a:a + n] for k, (a, n) in (DUMP_LAYOUT_WIDE if wide else DUMP_LAYOUT).items()}
        nv, nb, ns = self.nv, self.nbody, self.nsite
        res["xpos"] = res["xpos"][:3 * nb].reshape(nb, 3)
        res["xquat"] = res["xquat"][:4 * nb].reshape(nb, 4)
        res["site_xpos"] = res["site_xpos"][:3 * ns].reshape(ns, 3)
        for k in ("qacc_smooth", "qfrc_smooth", "qacc", "qfrc_constraint"):
            res[k] = res[k][:nv]
        res["qM"] = res["qM"][:nv * nv].reshape(nv, nv)
        sc = res["scalars"]
        ncon, nefc = int(sc[0]), int(sc[1])
        res.update(ncon=ncon, nefc=nefc, nsparse=int(sc[2]), ndense=int(sc[3]), touch=sc[4], status=int(sc[5]),
                   solver_iter=int(sc[6]) % 1000, solver_exit=NT_EXIT[int(sc[6]) // 1000], noslip_iter=int(sc[7]))
        res["con_dist"] = res["con_dist"][:ncon]
        res["con_pos"] = res["con_pos"][:3 * ncon].reshape(ncon, 3)
        res["con_frame"] = res["con_frame"][:9 * ncon].reshape(ncon, 9)
        res["con_pair"] = res["con_pair"][:ncon].astype(int)
        for k in ("efc_force", "efc_aref", "efc_D", "efc_type", "efc_state"):
            res[k] = res[k][:nefc]
        return res
