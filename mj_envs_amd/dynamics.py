"""Dynamics queries on the device (``aw_dynamics`` / ``k_dyn``, ``AdroitVecEnv.dynamics``).

The model-based half of ``sim.data``: point and body Jacobians (mujoco-py ``get_site_jacp`` /
``get_body_jacr``), linear and angular velocities (``get_body_xvelp`` / ``get_site_xvelr``), the
joint-space inertia ``qM`` and its inverse, and ``qfrc_bias`` / ``qfrc_passive`` / ``qfrc_actuator``
-- for every env or a subset, at the env's own state or at trial ``qpos`` / ``qvel`` rows that leave
the simulation untouched (an IK loop, a computed-torque law).  The values are those of
``mj_forward``'s position and velocity stages at that state: what mujoco-py shows after
``sim.forward()``, not the pre-integration values the ``data=`` views hold after a step.

    pts = points(env.model, sites=["S_grasp"], bodies=["Object"])
    d = env.dynamics(pts, want=("jacp", "point_pos", "qM", "qfrc_bias"))
    J = d.jacp("S_grasp")                      # [N, 3, nv]
"""
from __future__ import annotations

from typing import Optional

import numpy as np

from . import _native
from ._native import AW_DYN_MAXPOINTS, AW_PT_BODY, AW_PT_BODYCOM, AW_PT_SITE, DYN_OUTPUTS, DYN_POINT_OUTPUTS

DEFAULT_WANT = ("point_pos", "point_vel", "jacp", "jacr")


class PointTable:
    """The points of one ``dynamics`` call: ``records`` -- host (kind, id) pairs in the order sites,
    bodies, body coms -- and ``names``; ``index(name)`` finds a point.  A body that is listed both as
    a body and as a com is looked up as ``"<name>"`` and ``"<name>:com"``."""

    def __init__(self, records, names):
        self.records = [(int(k), int(i)) for k, i in records]
        self.names = list(names)

    def __len__(self):
        return len(self.records)

    def index(self, name) -> int:
        if isinstance(name, (int, np.integer)):
            if not 0 <= int(name) < len(self.records):
                raise KeyError(f"point {int(name)} of {len(self.records)}")
            return int(name)
        if name not in self.names:
            raise KeyError(f"no point named {name!r} (one of {self.names})")
        return self.names.index(name)


def _resolve(model, kind: str, x) -> int:
    names = model.names[kind]
    if isinstance(x, str):
        if x not in names:
            raise KeyError(f"no {kind} named {x!r}")
        return names.index(x)
    if isinstance(x, (bool, np.bool_)) or not isinstance(x, (int, np.integer)):
        raise TypeError(f"a {kind} is given by name or by id, not {type(x).__name__}")
    if not 0 <= int(x) < len(names):
        raise KeyError(f"{kind} id {int(x)} outside [0, {len(names)})")
    return int(x)


def points(model, sites=(), bodies=(), body_coms=()) -> PointTable:
    """The point table of ``sites`` (``site_xpos``), ``bodies`` (the body frames' origins ``xpos``)
    and ``body_coms`` (the centres of mass ``xipos``), each given by name or id; at most
    ``AW_DYN_MAXPOINTS`` points.  Pure: needs no GPU."""
    recs, names = [], []
    for kind, code, items, suffix in (("site", AW_PT_SITE, sites, ""), ("body", AW_PT_BODY, bodies, ""),
                                      ("body", AW_PT_BODYCOM, body_coms, ":com")):
        for x in items:
            i = _resolve(model, kind, x)
            recs.append((code, i))
            names.append(model.names[kind][i] + suffix)
    if len(recs) > AW_DYN_MAXPOINTS:
        raise ValueError(f"points: {len(recs)} points, at most {AW_DYN_MAXPOINTS} per call")
    if len(set(names)) != len(names):
        dup = sorted({n for n in names if names.count(n) > 1})
        raise ValueError(f"points: {dup[0]!r} listed more than once")
    return PointTable(recs, names)


def check_dynamics_args(want, npoints: int, n: int, nq: int, nv: int, nu: int, qpos_shape=None, qvel_shape=None,
                        actions_shape=None, ctrl_shape=None) -> tuple:
    """``AdroitVecEnv.dynamics``'s argument checks on shapes alone (nothing touches the GPU); returns
    the outputs wanted in ``aw_dyn_out``'s order.  n: the output rows (the selected envs, or all)."""
    names = (want,) if isinstance(want, str) else tuple(want)
    if not names:
        raise ValueError("dynamics: no output wanted")
    for k in names:
        if k not in DYN_OUTPUTS:
            raise ValueError(f"dynamics: unknown output {k!r} (one of {list(DYN_OUTPUTS)})")
    if not 0 <= int(npoints) <= AW_DYN_MAXPOINTS:
        raise ValueError(f"dynamics: {npoints} points, at most {AW_DYN_MAXPOINTS} per call")
    if npoints == 0 and any(k in DYN_POINT_OUTPUTS for k in names):
        raise ValueError(f"dynamics: {[k for k in names if k in DYN_POINT_OUTPUTS]} need points")
    if actions_shape is not None and ctrl_shape is not None:
        raise ValueError("dynamics: actions (normalised) and ctrl (raw) are two forms of one input; give one")
    for shp, w, k in ((qpos_shape, nq, "qpos"), (qvel_shape, nv, "qvel"), (actions_shape, nu, "actions"),
                      (ctrl_shape, nu, "ctrl")):
        if shp is not None and tuple(int(x) for x in shp) != (n, w):
            raise ValueError(f"dynamics: {k} must be [{n}, {w}], not {list(shp)}")
    return tuple(k for k in DYN_OUTPUTS if k in names)


class Dynamics:
    """The result of one ``dynamics`` call: the requested outputs as device fp32 tensors by name
    (``qM``, ``qMinv`` [n, nv, nv]; ``qfrc_bias``, ``qfrc_passive``, ``qfrc_actuator`` [n, nv]; ``xvel``
    [n, nbody, 6]; ``point_pos`` [n, P, 3]; ``point_vel`` [n, P, 6]; ``jacp_all`` / ``jacr_all``
    [n, P, 3, nv]) and lookups by point name: ``jacp(name)``, ``jacr(name)`` [n, 3, nv], ``pos(name)``
    [n, 3], ``vel(name)`` [n, 6] (angular, linear).  An output that was not wanted raises
    AttributeError."""

    def __init__(self, table: PointTable, tensors: dict, model=None):
        self.points, self.tensors, self.model = table, dict(tensors), model

    def __getattr__(self, name):            # only reached for names that are no attribute
        t = self.__dict__.get("tensors", {})
        key = {"jacp_all": "jacp", "jacr_all": "jacr"}.get(name, name)
        if key in t:
            return t[key]
        if key in DYN_OUTPUTS:
            raise AttributeError(f"dynamics: {key} was not wanted in this call")
        raise AttributeError(name)

    def _of(self, key, name):
        if key not in self.tensors:
            raise AttributeError(f"dynamics: {key} was not wanted in this call")
        return self.tensors[key][:, self.points.index(name)]

    def jacp(self, name):
        return self._of("jacp", name)

    def jacr(self, name):
        return self._of("jacr", name)

    def pos(self, name):
        return self._of("point_pos", name)

    def vel(self, name):
        return self._of("point_vel", name)

    def body_vel(self, body):
        """[n, 6] (angular, linear at the body frame's origin) of a body by name or id (needs ``xvel``)"""
        if "xvel" not in self.tensors:
            raise AttributeError("dynamics: xvel was not wanted in this call")
        b = _resolve(self.model, "body", body) if self.model is not None else int(body)
        return self.tensors["xvel"][:, b]


def opspace_inertia(J, Minv):
    """The operational-space inertia ``(J M^-1 J^T)^-1`` of a task Jacobian, batched: J [n, k, nv],
    Minv [n, nv, nv] -> [n, k, k] (torch)."""
    import torch
    return torch.linalg.inv(J @ Minv @ J.transpose(-1, -2))


def evaluate(env, table: Optional[PointTable], env_ids, want, qpos, qvel, actions, ctrl, out: Optional[Dynamics]):
    """``AdroitVecEnv.dynamics``: checks, buffers, the control map and the launch"""
    import torch
    s = env.sim
    table = table if table is not None else PointTable([], [])
    ids = None if env_ids is None else env._ids(env_ids, env.num_envs, "env_ids", distinct=False)
    n = env.num_envs if ids is None else int(ids.shape[0])
    shp = lambda t: None if t is None else tuple(t.shape)
    names = check_dynamics_args(want, len(table), n, env.nq, env.nv, env.nu, shp(qpos), shp(qvel), shp(actions),
                                shp(ctrl))
    if actions is not None:                  # the step's own map: clip to [-1, 1], then act_mid + a act_rng
        mid = torch.as_tensor(env.act_mid, device=s.torch_device)
        rng = torch.as_tensor(env.act_rng, device=s.torch_device)
        ctrl = mid + actions.to(torch.float32).clamp(-1.0, 1.0) * rng
    c = lambda t: None if t is None else t.to(torch.float32).contiguous()
    tensors = {}
    for k in names:
        shape = (n,) + _native.dyn_shape(k, env.nv, s.nbody, len(table))
        t = out.tensors.get(k) if out is not None else None
        if t is None or tuple(t.shape) != shape:
            t = torch.zeros(shape, device=s.torch_device)
        tensors[k] = t
    s.dynamics(tensors, table.records, env_ids=ids, qpos=c(qpos), qvel=c(qvel), ctrl=c(ctrl))
    return Dynamics(table, tensors, env.model)


class EnvDynamics:
    """mujoco-py's names over one env (the single-env facades' ``env.data``): each call evaluates
    the env's current state -- with ``ctrl`` the facade's last raw control -- and returns float64
    numpy arrays in mujoco-py's shapes: the Jacobians flat [3 nv], velocities [3], forces [nv]."""

    def __init__(self, vec, ctrl=None):
        self._vec, self._ctrl = vec, ctrl

    def _one(self, want, **pts):
        table = points(self._vec.model, **pts) if pts else None
        return self._vec.dynamics(table, want=want, ctrl=self._ctrl)

    @staticmethod
    def _np(t):
        return t[0].cpu().numpy().astype(np.float64)

    def get_site_jacp(self, name):
        return self._np(self._one(("jacp",), sites=[name]).jacp(0)).ravel()

    def get_site_jacr(self, name):
        return self._np(self._one(("jacr",), sites=[name]).jacr(0)).ravel()

    def get_body_jacp(self, name):
        return self._np(self._one(("jacp",), bodies=[name]).jacp(0)).ravel()

    def get_body_jacr(self, name):
        return self._np(self._one(("jacr",), bodies=[name]).jacr(0)).ravel()

    def get_site_xvelp(self, name):
        return self._np(self._one(("point_vel",), sites=[name]).vel(0))[3:]

    def get_site_xvelr(self, name):
        return self._np(self._one(("point_vel",), sites=[name]).vel(0))[:3]

    def get_body_xvelp(self, name):
        return self._np(self._one(("point_vel",), bodies=[name]).vel(0))[3:]

    def get_body_xvelr(self, name):
        return self._np(self._one(("point_vel",), bodies=[name]).vel(0))[:3]

    @property
    def qfrc_bias(self):
        return self._np(self._one(("qfrc_bias",)).qfrc_bias)

    @property
    def qfrc_passive(self):
        return self._np(self._one(("qfrc_passive",)).qfrc_passive)

    @property
    def qfrc_actuator(self):
        return self._np(self._one(("qfrc_actuator",)).qfrc_actuator)

    @property
    def qM_full(self):
        """the dense [nv, nv] inertia (mujoco-py's ``qM`` is the packed form: another name)"""
        return self._np(self._one(("qM",)).qM)
