"""Inverse kinematics on the device (``aw_solve_ik`` / ``k_ik``, ``AdroitVecEnv.solve_ik``).

Batched damped least squares, the whole iteration in one launch: given where sites and bodies (the
palm, the fingertips) should be, find joint positions -- for every env or a subset, from the env's own
qpos or from ``qpos0`` rows, without touching the simulation.  The iteration is the one stated in
include/adroit_wave.h: ``dq = J^T (J J^T + damping I)^-1 e`` with the weighted position / orientation
residual ``e``, an optional step limit and clamping to the joint ranges, until ``|e| <= tol``.

    tg = targets(env.model, sites=["S_grasp"])
    res = env.solve_ik(tg, goal_pos=goal, dofs=dof_mask(env.model, chain="S_grasp"))
    env.set_state(qpos=res.qpos)               # or step(qpos_to_actions(env.model, res.qpos))
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from ._native import AW_PT_BODY, AW_PT_BODYCOM, AW_PT_SITE
from .dynamics import PointTable, _resolve


class TargetTable(PointTable):
    """The targets of one ``solve_ik`` call: ``records`` -- host (kind, id) pairs in the order sites,
    bodies, body coms -- with ``wpos`` / ``wrot`` per target and ``names``; ``index(name)`` finds a
    target, ``rows`` is the residual row count m."""

    def __init__(self, records, names, wpos, wrot):
        super().__init__(records, names)
        self.wpos, self.wrot = [float(w) for w in wpos], [float(w) for w in wrot]

    @property
    def ik_records(self):
        """(kind, id, wpos, wrot) per target, as ``Sim.solve_ik`` takes them"""
        return [(k, i, wp, wr) for (k, i), wp, wr in zip(self.records, self.wpos, self.wrot)]

    @property
    def rows(self) -> int:
        return sum((3 if wp > 0 else 0) + (3 if wr > 0 else 0) for wp, wr in zip(self.wpos, self.wrot))


def targets(model, sites=(), bodies=(), body_coms=(), wpos=1.0, wrot=0.0) -> TargetTable:
    """The target table of ``sites``, ``bodies`` (the body frames) and ``body_coms``, each item a name
    or id as in ``dynamics.points``, or ``(name, wpos, wrot)`` to override the call's weights for that
    target.  ``wpos`` > 0: three position rows; ``wrot`` > 0: three orientation rows.  At most
    ``IK_MAXTARGETS`` targets and ``IK_MAXROWS`` rows.  Pure: needs no GPU."""
    recs, names, wp, wr = [], [], [], []
    for kind, code, items, suffix in (("site", AW_PT_SITE, sites, ""), ("body", AW_PT_BODY, bodies, ""),
                                      ("body", AW_PT_BODYCOM, body_coms, ":com")):
        for x in items:
            a, b = wpos, wrot
            if isinstance(x, (tuple, list)):
                if len(x) != 3:
                    raise ValueError(f"targets: an override is (name, wpos, wrot), not {x!r}")
                x, a, b = x
            i = _resolve(model, kind, x)
            recs.append((code, i))
            names.append(model.names[kind][i] + suffix)
            wp.append(float(a))
            wr.append(float(b))
    if len(set(names)) != len(names):
        dup = sorted({n for n in names if names.count(n) > 1})
        raise ValueError(f"targets: {dup[0]!r} listed more than once")
    t = TargetTable(recs, names, wp, wr)
    _native.check_ik_targets(t.ik_records, len(model.names["body"]), len(model.names["site"]))
    return t


def body_dofmask(model, body: int) -> int:
    """bit i set where dof i moves ``body``: the dofs of the body and of its ancestors (the device
    model's body_dofmask)"""
    parent = np.asarray(model.arrays["body_parentid"]).astype(int)
    dof_body = np.asarray(model.arrays["dof_bodyid"]).astype(int)
    chain = set()
    b = int(body)
    while b > 0:
        chain.add(b)
        b = int(parent[b])
    return sum(1 << i for i, d in enumerate(dof_body.tolist()) if d in chain)


def dof_mask(model, joints=None, chain=None, actuated: bool = False) -> int:
    """The ``dof_mask`` of ``solve_ik``: the union of ``joints`` (names or ids; Adroit's joints are
    hinge or slide, so joint i is dof i), of the dofs that move ``chain`` (a site or body name: the
    dofs of its body and of that body's ancestors) and, with ``actuated``, of every dof an actuator
    drives.  Pure: needs no GPU."""
    mask = 0
    for j in (joints or ()):
        mask |= 1 << _resolve(model, "joint", j)
    if chain is not None:
        if isinstance(chain, str) and chain in model.names["site"]:
            body = int(np.asarray(model.arrays["site_bodyid"])[model.names["site"].index(chain)])
        else:
            body = _resolve(model, "body", chain)
        mask |= body_dofmask(model, body)
    if actuated:
        for j in np.asarray(model.arrays["actuator_trnid"]).astype(int).ravel().tolist():
            mask |= 1 << j
    if not mask:
        raise ValueError("dof_mask: no dof selected (give joints, chain or actuated=True)")
    return mask


def qpos_to_actions(model, qpos):
    """Normalised actions whose position set-points are ``qpos``: the inverse of the step's control
    map ``ctrl = act_mid + clip(a, -1, 1) act_rng`` for the joint each actuator drives,
    ``clip((q[joint of actuator u] - act_mid[u]) / act_rng[u], -1, 1)``.  ``qpos`` [..., nq], numpy
    or torch -> [..., nu] of the same kind.  Adroit's arm actuators are affine position servos
    (force = kp (ctrl - q) with a bias, against gravity and contact), so this is the
    set-point the servo is given, not a guarantee of where the joint settles."""
    trn = np.asarray(model.arrays["actuator_trnid"]).astype(np.int64).ravel()
    mid = np.asarray(model.arrays["task_act_mid"])
    rng = np.asarray(model.arrays["task_act_rng"])
    if isinstance(qpos, np.ndarray) or not hasattr(qpos, "device"):
        q = np.asarray(qpos)
        return np.clip((q[..., trn] - mid.astype(q.dtype)) / rng.astype(q.dtype), -1, 1)
    import torch
    t = lambda a: torch.as_tensor(a, dtype=qpos.dtype, device=qpos.device)
    idx = torch.as_tensor(trn, device=qpos.device)
    return ((qpos.index_select(-1, idx) - t(mid)) / t(rng)).clamp(-1.0, 1.0)


class IKResult:
    """The result of one ``solve_ik`` call, device tensors: ``qpos`` [n, nq], ``err`` [n] (the
    weighted residual norm at qpos), ``iters`` [n] (int32, updates applied), ``point_pos`` [n, T, 3],
    ``point_quat`` [n, T, 4] (the targets' poses at qpos); ``converged`` [n] (bool: err <= tol) and
    the lookups ``pos(name)`` [n, 3] / ``quat(name)`` [n, 4]."""

    def __init__(self, table: TargetTable, tensors: dict, tol: float):
        self.targets, self.tensors, self.tol = table, dict(tensors), float(tol)

    def __getattr__(self, name):            # only reached for names that are no attribute
        t = self.__dict__.get("tensors", {})
        if name in t:
            return t[name]
        raise AttributeError(name)

    @property
    def converged(self):
        return self.tensors["err"] <= self.tol

    def pos(self, name):
        return self.tensors["point_pos"][:, self.targets.index(name)]

    def quat(self, name):
        return self.tensors["point_quat"][:, self.targets.index(name)]


def check_solve_args(table, n: int, nq: int, goal_pos_shape=None, goal_quat_shape=None, qpos0_shape=None):
    """``AdroitVecEnv.solve_ik``'s checks on shapes alone (nothing touches the GPU): a position goal
    for every table with a position weight, a quaternion goal for every one with an orientation weight"""
    T = len(table)
    need_pos, need_rot = any(w > 0 for w in table.wpos), any(w > 0 for w in table.wrot)
    if need_pos and goal_pos_shape is None:
        raise ValueError("solve_ik: goal_pos is needed (a target has wpos > 0)")
    if need_rot and goal_quat_shape is None:
        raise ValueError("solve_ik: goal_quat is needed (a target has wrot > 0)")
    for shp, w, k in ((goal_pos_shape, (n, T, 3), "goal_pos"), (goal_quat_shape, (n, T, 4), "goal_quat"),
                      (qpos0_shape, (n, nq), "qpos0")):
        if shp is not None and tuple(int(x) for x in shp) != w:
            raise ValueError(f"solve_ik: {k} must be {list(w)}, not {list(shp)}")


def solve(env, table: TargetTable, goal_pos, goal_quat, dofs, env_ids, qpos0, out: Optional[IKResult], opt: dict):
    """``AdroitVecEnv.solve_ik``: checks, buffers, the goal record and the launch"""
    import torch
    s = env.sim
    ids = None if env_ids is None else env._ids(env_ids, env.num_envs, "env_ids", distinct=False)
    n = env.num_envs if ids is None else int(ids.shape[0])
    T = len(table)
    shp = lambda t: None if t is None else tuple(t.shape)
    check_solve_args(table, n, env.nq, shp(goal_pos), shp(goal_quat), shp(qpos0))
    unknown = set(opt) - {"max_iter", "damping", "tol", "max_step", "clamp_range"}
    if unknown:
        raise TypeError(f"solve_ik: unknown options {sorted(unknown)}")
    mask = dof_mask(env.model, actuated=True) if dofs is None else int(dofs)
    goal = torch.zeros(n, T, 7, device=s.torch_device)
    goal[..., 3] = 1.0
    if goal_pos is not None:
        goal[..., :3] = goal_pos.to(torch.float32)
    if goal_quat is not None:
        goal[..., 3:] = goal_quat.to(torch.float32)
    tensors = {}
    for k in _native.IK_OUTPUTS:
        shape = (n,) + _native.ik_shape(k, env.nq, T)
        dt = torch.int32 if k == "iters" else torch.float32
        t = out.tensors.get(k) if out is not None else None
        if t is None or tuple(t.shape) != shape or t.dtype != dt:
            t = torch.zeros(shape, dtype=dt, device=s.torch_device)
        tensors[k] = t
    s.solve_ik(tensors, table.ik_records, goal, mask, env_ids=ids,
               qpos0=None if qpos0 is None else qpos0.to(torch.float32).contiguous(), **opt)
    return IKResult(table, tensors, opt.get("tol", 1e-4))
