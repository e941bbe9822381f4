"""Batched ``sim.data`` views over the device buffers the step kernels write (aw_set_data).

``AdroitVecEnv(data=...)`` exposes ``env.data`` (``DataViews``): the arrays the reference's task
files read -- ``body_xpos``, ``body_xquat``, ``site_xpos``, ``qacc``, ``qfrc_constraint``, the
contact list with ``mj_contactForce``'s forces -- as torch views of device memory, one leading env
axis, no copies.  The values are those of the last ``mj_forward`` before the last integration of the
env-step (or of the reset / set_state forward): what ``sim.data`` holds after ``step()``.

The single-env facades expose the same names as float64 numpy arrays of their one env
(``EnvData``), the contact arrays cut to ``ncon``.
"""
from __future__ import annotations

import numpy as np

from . import _native

_KIN = ("body_xpos", "body_xquat", "site_xpos")
_DYN = ("qacc", "qfrc_constraint", "ncon", "nefc", "solver_iter", "noslip_iter")
GROUP_OF = {**{k: "kin" for k in _KIN}, **{k: "dyn" for k in _DYN}, "contact": "contact"}


def make_frame_np(normal):
    """mju_makeFrame for unit normals [..., 3] -> frames [..., 3, 3] (rows: normal, tangent 1, 2)"""
    n = np.asarray(normal, np.float64)
    t = np.where((np.abs(n[..., 1:2]) < 0.5), np.array([0.0, 1.0, 0.0]), np.array([0.0, 0.0, 1.0]))
    t = t - (n * t).sum(-1, keepdims=True) * n
    t = t / np.linalg.norm(t, axis=-1, keepdims=True)
    return np.stack([n, t, np.cross(n, t)], axis=-2)


def contact_force_np(dim, efc_address, mu, efc_force):
    """mj_contactForce with pyramidal cones for one contact: (force[3] in the contact frame, torsion).
    ``mu``: the contact's friction[0:3]; condim 1: the row's force; else normal = the sum of the
    2 (dim - 1) edge forces and component i = (f[2i-2] - f[2i-1]) mu[i-1]; no rows: zero."""
    f, tors = np.zeros(3), 0.0
    if efc_address < 0:
        return f, tors
    a = int(efc_address)
    if dim == 1:
        f[0] = efc_force[a]
        return f, tors
    p = np.asarray(efc_force[a:a + 2 * (dim - 1)], np.float64)
    f[0] = p.sum()
    comp = [(p[2 * i] - p[2 * i + 1]) * mu[i] for i in range(dim - 1)]
    f[1] = comp[0]
    if dim > 2:
        f[2] = comp[1]
    if dim > 3:
        tors = comp[2]
    return f, tors


class ContactViews:
    """``data.contact``: [N, K] views of the contact records (K = max_contacts).  ``mask[e, c]`` tells
    which records are the env's current contacts (c < min(ncon[e], K)); the others hold whatever
    they held before."""

    def __init__(self, owner, rec, counts):
        import torch
        self._o, self._rec, self._counts = owner, rec, counts
        self._irec = rec.view(torch.int32)
        self.max_contacts = rec.shape[1]

    def __getattr__(self, name):
        f = _native.CONTACT_FIELDS.get(name)
        if f is None:
            raise AttributeError(name)
        w0, nw, is_int = f
        src = self._irec if is_int else self._rec
        return src[:, :, w0] if nw == 1 else src[:, :, w0:w0 + nw]

    @property
    def mask(self):
        import torch
        if self._counts is None:
            raise AttributeError("contact.mask needs ncon: enable the 'dyn' group too")
        k = torch.arange(self.max_contacts, device=self._rec.device)
        return k[None, :] < self._counts[:, 0:1].clamp(max=self.max_contacts)

    def normal_force_between(self, a, b):
        """[N]: the summed normal force of the current contacts between ``a`` and ``b`` -- each a body
        or geom name or id (``("geom", id)`` / ``("body", id)`` for ids; a bare int is a body id)"""
        ga, gb = self._o._geoms_of(a), self._o._geoms_of(b)
        import torch
        hi = self._o._ngeom - 1            # records outside the mask may hold anything
        g1, g2 = self.geom1.long().clamp(0, hi), self.geom2.long().clamp(0, hi)
        hit = ((ga[g1] & gb[g2]) | (gb[g1] & ga[g2])) & self.mask
        fn = self.force[:, :, 0]
        return torch.where(hit, fn, torch.zeros_like(fn)).sum(dim=1)

    def force_world(self):
        """[N, K, 3]: each contact's force (normal + tangential) in the world frame, on geom2's body
        (mj_contactForce rotated by the contact frame); zero outside ``mask``"""
        import torch
        n = self.normal
        ey = torch.tensor([0.0, 1.0, 0.0], device=n.device)
        ez = torch.tensor([0.0, 0.0, 1.0], device=n.device)
        t = torch.where(n[..., 1:2].abs() < 0.5, ey, ez)
        t = t - (n * t).sum(-1, keepdim=True) * n
        t = t / t.norm(dim=-1, keepdim=True).clamp_min(1e-15)
        t2 = torch.cross(n, t, dim=-1)
        f = self.force
        w = f[..., 0:1] * n + f[..., 1:2] * t + f[..., 2:3] * t2
        return torch.where(self.mask[..., None], w, torch.zeros_like(w))


class DataViews:
    """``AdroitVecEnv.data``: torch views of the buffers the kernels write; a name of a group that
    was not enabled raises AttributeError."""

    def __init__(self, model, sim, groups, max_contacts=32):
        import torch
        self.model, self.groups = model, _native.data_groups(groups)
        self._b = b = sim.set_data(self.groups, max_contacts)
        self.max_contacts = int(max_contacts)
        dev = sim.torch_device
        if "xpos" in b:
            self.body_xpos, self.body_xquat, self.site_xpos = b["xpos"], b["xquat"], b["site_xpos"]
        counts = b.get("counts")
        if counts is not None:
            self.qacc, self.qfrc_constraint = b["qacc"], b["qfrc_constraint"]
            self.ncon, self.nefc, self.solver_iter, self.noslip_iter = (counts[:, k] for k in range(4))
        if "contact" in b:
            self.contact = ContactViews(self, b["contact"], counts)
        self._geom_body = torch.as_tensor(np.asarray(model.arrays["geom_bodyid"], np.int64), device=dev)
        self._ngeom = int(self._geom_body.numel())

    def __getattr__(self, name):     # only reached for names not set above
        if name in GROUP_OF:
            raise AttributeError(f"data.{name}: the {GROUP_OF[name]!r} group is not enabled (AdroitVecEnv(data=...))")
        raise AttributeError(name)

    def _geoms_of(self, x):
        """bool [ngeom] device mask of the geoms ``x`` names: a geom, or every geom of a body"""
        import torch
        names = self.model.names
        kind, idx = None, None
        if isinstance(x, tuple):
            kind, idx = x[0], int(x[1])
        elif isinstance(x, str):
            if x in names["geom"]:
                kind, idx = "geom", names["geom"].index(x)
            elif x in names["body"]:
                kind, idx = "body", names["body"].index(x)
            else:
                raise KeyError(f"no geom or body named {x!r}")
        else:
            kind, idx = "body", int(x)
        if kind == "geom":
            m = torch.zeros(self._ngeom, dtype=torch.bool, device=self._geom_body.device)
            m[idx] = True
            return m
        if kind != "body":
            raise ValueError(f"kind must be 'geom' or 'body', not {kind!r}")
        return self._geom_body == idx


class EnvData:
    """``env.data`` of a single-env facade: float64 numpy copies of env 0, the contact arrays cut to
    ncon (at most max_contacts).  ``views`` None: the env was created with data=False and holds
    none of them.  ``dynamics`` (``mj_envs_amd.dynamics.EnvDynamics``): mujoco-py's model-based
    queries -- get_site_jacp, get_body_xvelp, qfrc_bias, qM_full ... -- evaluated on demand."""

    class _Contacts:
        pass

    def __init__(self, views: DataViews, dynamics=None):
        self._dynamics = dynamics
        if views is None:
            return
        v = views
        for k in _KIN + ("qacc", "qfrc_constraint"):
            if k in v.__dict__:
                setattr(self, k, getattr(v, k)[0].cpu().numpy().astype(np.float64))
        if "ncon" in v.__dict__:
            for k in ("ncon", "nefc", "solver_iter", "noslip_iter"):
                setattr(self, k, int(getattr(v, k)[0]))
        if "contact" in v.__dict__:
            c = v.contact
            n = min(self.ncon, c.max_contacts) if hasattr(self, "ncon") else c.max_contacts
            self.contact = EnvData._Contacts()
            for k, (_, _, is_int) in _native.CONTACT_FIELDS.items():
                a = getattr(c, k)[0, :n].cpu().numpy()
                setattr(self.contact, k, a.astype(np.int32 if is_int else np.float64))
            frames = make_frame_np(self.contact.normal) if n else np.zeros((0, 3, 3))
            self.contact.force_world = np.einsum("ck,ckj->cj", self.contact.force, frames) if n else np.zeros((0, 3))

    def __getattr__(self, name):     # only reached for names not set above
        dyn = self.__dict__.get("_dynamics")
        if dyn is not None and not name.startswith("_") and hasattr(type(dyn), name):
            return getattr(dyn, name)
        if name in GROUP_OF:
            raise AttributeError(f"data.{name}: the {GROUP_OF[name]!r} group is not enabled (data=...)")
        raise AttributeError(name)
