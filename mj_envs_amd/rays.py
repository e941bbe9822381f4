"""Ray queries (``aw_set_rays`` / ``aw_cast_rays``, ``AdroitVecEnv.raycast``): MuJoCo's ``mj_ray`` and
its ``rangefinder`` sensor for a batch -- along a ray attached to a body, what is the first thing hit
and how far is it?  Fingertip proximity, "is the object occluded from the palm", height above the
table, a sparse lidar fan on the wrist.

A ``Rays`` set is a table of at most 256 records (``_native.RAY_DTYPE``, the C-ABI's ``aw_ray_rec``):
origin ``pnt`` and direction ``vec`` in the frame of ``body`` (0: the world), a range limit ``xmax``
(<= 0: none) and a 64-bit ``keep`` mask over the render entries (``labels.render_entries``: the
primitive geoms in model order).  One launch casts the whole table at every env's current state;
the answer per ray is ``dist``, the x >= 0 of the first crossing ``pnt + x vec`` (metres for a unit
``vec``; -1 on a miss), and the entry crossed.  The builders below make the common tables;
``keep_mask`` applies ``mj_ray``'s elimination rules (geomgroup, flg_static, bodyexclude, invisible
geoms) on the compiled model's arrays.

Two deviations from ``mj_ray`` (include/adroit_wave.h): mesh geoms are absent (they are not available
offline; the hand's primitive collision geoms are in the table), and planes are hit from both sides
and are finite where their size is positive, as the depth renderer draws them.  A ray that starts
inside a geom reports where it leaves it (``mju_rayGeom``'s rule).  Sites are never hit.
"""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence, Union

import numpy as np

from ._native import AW_MAX_RAYS, RAY_DTYPE
from .labels import entry_bodies, keep_table, label_table, render_entries
from .mjcf import quat2mat

NGROUP = 6            # mjNGROUP: the length of mj_ray's geomgroup
FILTER_KEYS = ("geomgroup", "flg_static", "bodyexclude", "bodies")


def _body_id(model, b: Union[int, str], what: str = "body") -> int:
    if isinstance(b, str):
        if b not in model.names["body"]:
            raise ValueError(f"{what}: the model has no body {b!r}")
        return model.name2id("body", b)
    b = int(b)
    if not 0 <= b < int(model.nbody):
        raise ValueError(f"{what}: body {b} outside [0, {int(model.nbody)})")
    return b


def keep_mask(model, geomgroup=None, flg_static=True, bodyexclude=-1, bodies=None) -> int:
    """The ``keep`` mask of a ray (bit e: render entry e may be hit) under ``mj_ray``'s elimination
    rules: ``geomgroup`` (6 flags or None) drops the geoms whose ``geom_group`` (clamped to 0..5) has
    a zero flag; ``flg_static`` False drops the geoms of bodies welded to the world
    (``body_weldid == 0``); ``bodyexclude`` (a body id or name; -1: none) drops that body's geoms;
    a geom without a material whose rgba alpha is 0, or whose material's alpha is 0, is always
    dropped (a model table without the appearance arrays has no such information: nothing is
    dropped for it, and ``geomgroup`` raises).  ``bodies`` (names or ids): only the geoms of those
    bodies' subtrees stay (``labels.keep_table``)."""
    geoms, _ = render_entries(model)
    if len(geoms) > 64:
        raise ValueError("keep_mask: more than 64 render entries")
    ex = -1 if isinstance(bodyexclude, (int, np.integer)) and int(bodyexclude) < 0 else _body_id(model, bodyexclude,
                                                                                              "bodyexclude")
    has = lambda k: k in model.arrays
    if geomgroup is not None:
        geomgroup = [bool(f) for f in np.asarray(geomgroup).ravel()]
        if len(geomgroup) != NGROUP:
            raise ValueError(f"geomgroup: {NGROUP} flags, not {len(geomgroup)}")
        if not has("geom_group"):
            raise ValueError("geomgroup: the model table carries no geom_group")
    sub = None if bodies is None else keep_table(model, [_body_id(model, b, "bodies") for b in bodies])
    mask = 0
    for e, g in enumerate(geoms):
        b = int(model.geom_bodyid[g])
        if b == ex:
            continue
        if has("geom_matid") and has("geom_rgba") and has("mat_rgba"):
            mat = int(model.geom_matid[g])
            if (mat < 0 and model.geom_rgba[g, 3] == 0) or (mat >= 0 and model.mat_rgba[mat, 3] == 0):
                continue
        if not flg_static and int(model.body_weldid[b]) == 0:
            continue
        if geomgroup is not None and not geomgroup[min(max(int(model.geom_group[g]), 0), NGROUP - 1)]:
            continue
        if sub is not None and not sub[e]:
            continue
        mask |= 1 << e
    return mask


def check_records(model, rec: np.ndarray, what: str = "rays") -> np.ndarray:
    """``rec`` as a contiguous ``RAY_DTYPE`` vector, or ValueError on what ``aw_set_rays`` rejects:
    more than 256 records, a body outside [0, nbody), a zero or non-finite ``vec``, a non-finite
    ``pnt`` or ``xmax``"""
    rec = np.ascontiguousarray(rec, RAY_DTYPE).ravel()
    if rec.size > AW_MAX_RAYS:
        raise ValueError(f"{what}: {rec.size} rays, at most {AW_MAX_RAYS} per table")
    if rec.size:
        bad = (rec["body"] < 0) | (rec["body"] >= int(model.nbody))
        if bad.any():
            raise ValueError(f"{what}: ray {int(np.flatnonzero(bad)[0])}: body {int(rec['body'][bad][0])} outside "
                             f"[0, {int(model.nbody)})")
        fin = np.isfinite(rec["pnt"]).all(1) & np.isfinite(rec["vec"]).all(1) & np.isfinite(rec["xmax"])
        if not fin.all():
            raise ValueError(f"{what}: ray {int(np.flatnonzero(~fin)[0])}: pnt, vec and xmax must be finite")
        zero = (rec["vec"] == 0).all(1)
        if zero.any():
            raise ValueError(f"{what}: ray {int(np.flatnonzero(zero)[0])}: vec is zero")
    return rec


class Rays:
    """A ray table: ``records`` (``RAY_DTYPE`` [R]), one label per ray and, after ``concat``, the
    slice of each named part (``parts``)."""

    def __init__(self, model, records, labels: Optional[Sequence[str]] = None, parts: Optional[Dict[str, slice]] = None):
        self.model = model
        self.records = check_records(model, records)
        n = int(self.records.size)
        self.labels: List[str] = [f"ray{k}" for k in range(n)] if labels is None else [str(s) for s in labels]
        if len(self.labels) != n:
            raise ValueError(f"Rays: {len(self.labels)} labels for {n} rays")
        self.parts: Dict[str, slice] = dict(parts or {})

    def __len__(self) -> int:
        return int(self.records.size)

    def part(self, name: str) -> slice:
        """the slice of the rays that ``concat`` joined under ``name``"""
        if name not in self.parts:
            raise KeyError(f"Rays: no part {name!r} (parts: {sorted(self.parts)})")
        return self.parts[name]

    def key(self) -> bytes:
        """the table's bytes: what decides whether a handle already holds it"""
        return self.records.tobytes()


def concat(*sets: Rays, **named: Rays) -> Rays:
    """Join ray sets into one table (at most 256 rays): positional sets keep their own parts, a
    keyword set becomes the part of that name -- ``concat(tips=fan_a, wrist=fan_b)`` --, and
    ``RayHits.named("tips")`` / ``result.part("tips")`` address its rays."""
    items = [(None, s) for s in sets] + list(named.items())
    if not items:
        raise ValueError("concat: no ray sets")
    recs, labels, parts, at = [], [], {}, 0
    for name, s in items:
        if not isinstance(s, Rays):
            raise ValueError("concat: every item is a Rays")
        for k, sl in s.parts.items():
            key = k if name is None else f"{name}.{k}"
            if key in parts:
                raise ValueError(f"concat: part {key!r} twice")
            parts[key] = slice(at + sl.start, at + sl.stop)
        if name is not None:
            if name in parts:
                raise ValueError(f"concat: part {name!r} twice")
            parts[name] = slice(at, at + len(s))
        recs.append(s.records)
        labels += s.labels if name is None else [f"{name}:{l}" for l in s.labels]
        at += len(s)
    if at > AW_MAX_RAYS:
        raise ValueError(f"concat: {at} rays, at most {AW_MAX_RAYS} per table")
    return Rays(items[0][1].model, np.concatenate(recs), labels, parts)


def _records(body, pnt, vec, xmax, keep) -> np.ndarray:
    pnt, vec = np.atleast_2d(np.asarray(pnt, np.float64)), np.atleast_2d(np.asarray(vec, np.float64))
    if pnt.shape[-1] != 3 or vec.shape[-1] != 3 or pnt.ndim != 2 or vec.ndim != 2:
        raise ValueError("rays: pnt and vec are [K, 3] (or [3])")
    k = max(len(pnt), len(vec))
    rec = np.zeros(k, RAY_DTYPE)
    with np.errstate(over="ignore"):
        rec["pnt"], rec["vec"] = np.broadcast_to(pnt, (k, 3)), np.broadcast_to(vec, (k, 3))
        rec["xmax"] = np.broadcast_to(np.asarray(xmax, np.float64), (k,))
    rec["body"] = np.broadcast_to(np.asarray(body), (k,))
    rec["keep"] = np.broadcast_to(np.asarray(keep, np.uint64), (k,))
    return rec


def body_rays(model, body, pnt, vec, xmax=0.0, labels=None, **filter) -> Rays:
    """K rays riding on ``body`` (a name or an id; 0 / "world": static rays): ``pnt`` and ``vec`` [K, 3]
    (or one [3]) in the body's frame, ``xmax`` one limit or K (<= 0: none), ``filter``: the keywords
    of ``keep_mask``"""
    b = _body_id(model, body)
    rec = _records(b, pnt, vec, xmax, keep_mask(model, **filter))
    name = model.names["body"][b]
    return Rays(model, rec, labels or [f"{name}[{k}]" for k in range(rec.size)])


def rangefinder(model, sites: Sequence[Union[int, str]], cutoff: float = 0.0) -> Rays:
    """MuJoCo's rangefinder sensor on each of ``sites`` (names or ids): the ray from the site's
    position along the site's +z axis, expressed in the frame of the site's body (``site_pos``, the z
    column of ``site_quat``'s matrix), with the site's own body excluded; ``cutoff`` > 0 limits the
    range (a farther hit reads -1)."""
    if isinstance(sites, (str, int, np.integer)):
        sites = [sites]
    recs, labels = [], []
    for s in sites:
        if isinstance(s, str) and s not in model.names["site"]:
            raise ValueError(f"rangefinder: the model has no site {s!r}")
        i = model.name2id("site", s) if isinstance(s, str) else int(s)
        if not 0 <= i < int(model.nsite):
            raise ValueError(f"rangefinder: site {i} outside [0, {int(model.nsite)})")
        b = int(model.site_bodyid[i])
        z = quat2mat(np.asarray(model.site_quat[i], np.float64))[:, 2]
        recs.append(_records(b, model.site_pos[i], z, cutoff, keep_mask(model, bodyexclude=b)))
        labels.append(model.names["site"][i])
    if not recs:
        raise ValueError("rangefinder: no sites")
    return Rays(model, np.concatenate(recs), labels)


def cone(axis, half_angle_deg: float, count: int) -> np.ndarray:
    """``count`` distinct unit vectors [count, 3] inside the cone of ``half_angle_deg`` about ``axis``,
    deterministic: ray 0 is the axis, ray k lies at polar angle acos(1 - (1 - cos half) k / count) and
    azimuth k times the golden angle (an equal-area spiral over the cap)"""
    a = np.asarray(axis, np.float64).ravel()
    if a.shape != (3,) or not np.isfinite(a).all() or not np.linalg.norm(a) > 0:
        raise ValueError("fan: axis is a finite non-zero 3-vector")
    if not (isinstance(count, (int, np.integer)) and count >= 1):
        raise ValueError("fan: count >= 1")
    if not 0.0 <= float(half_angle_deg) <= 180.0:
        raise ValueError("fan: half_angle_deg in [0, 180]")
    a = a / np.linalg.norm(a)
    e1 = np.cross(a, [1.0, 0.0, 0.0] if abs(a[0]) < 0.6 else [0.0, 1.0, 0.0])
    e1 /= np.linalg.norm(e1)
    e2 = np.cross(a, e1)
    k = np.arange(count)
    ct = 1.0 - (1.0 - math.cos(math.radians(float(half_angle_deg)))) * k / count
    st = np.sqrt(np.maximum(1.0 - ct * ct, 0.0))
    phi = k * (math.pi * (3.0 - math.sqrt(5.0)))
    v = ct[:, None] * a + st[:, None] * (np.cos(phi)[:, None] * e1 + np.sin(phi)[:, None] * e2)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def fan(model, site_or_body: str, axis, half_angle_deg: float, count: int, xmax: float = 0.0, **filter) -> Rays:
    """A deterministic cone of ``count`` unit rays (``cone``) from a site (its position, ``axis`` in the
    site's frame) or from a body's origin (``axis`` in the body's frame), riding on that body.
    ``filter``: the keywords of ``keep_mask`` -- a fan on a fingertip site usually wants
    ``bodyexclude=`` the fingertip's body."""
    v = cone(axis, half_angle_deg, count)
    if site_or_body in model.names["site"]:
        i = model.name2id("site", site_or_body)
        b = int(model.site_bodyid[i])
        R = quat2mat(np.asarray(model.site_quat[i], np.float64))
        pnt, v = np.asarray(model.site_pos[i], np.float64), v @ R.T
    elif site_or_body in model.names["body"]:
        b, pnt = model.name2id("body", site_or_body), np.zeros(3)
    else:
        raise ValueError(f"fan: the model has no site or body {site_or_body!r}")
    rec = _records(b, pnt, v, xmax, keep_mask(model, **filter))
    return Rays(model, rec, [f"{site_or_body}[{k}]" for k in range(count)])


def segments(model, count: int, **filter) -> Rays:
    """``count`` world-frame rays with ``xmax`` 1, to be filled per env through ``env_rays`` with
    ``(a, b - a)``: the segment from a to b is crossed where 0 <= x <= 1 (line of sight).  The
    records' own pnt / vec (the origin, +z) are placeholders."""
    if not (isinstance(count, (int, np.integer)) and 1 <= count <= AW_MAX_RAYS):
        raise ValueError(f"segments: count in 1..{AW_MAX_RAYS}")
    rec = _records(0, np.zeros(3), np.tile([0.0, 0.0, 1.0], (count, 1)), 1.0, keep_mask(model, **filter))
    return Rays(model, rec, [f"segment{k}" for k in range(count)])


class RayHits:
    """The result of one cast (device tensors, row k = the k-th selected env): ``dist`` [n, R] fp32,
    ``hit`` (``dist >= 0``), ``entry`` [n, R] int32 (None when not asked for), and from it ``geom_id`` /
    ``body_id`` (the model's ids, -1 on a miss)."""

    def __init__(self, rays: Rays, dist, entry=None):
        self.rays, self.dist, self.entry = rays, dist, entry

    @property
    def hit(self):
        return self.dist >= 0

    def _lut(self, table):
        import torch
        if self.entry is None:
            raise AttributeError("RayHits: cast with entry=True for geom_id / body_id")
        ng = len(render_entries(self.rays.model)[0])
        lut = torch.as_tensor(np.asarray(table[:ng], np.int64), device=self.entry.device)
        e = self.entry.long()
        return torch.where(e >= 0, lut[e.clamp(min=0)], torch.full_like(e, -1))

    @property
    def geom_id(self):
        return self._lut(label_table(self.rays.model, "geom"))

    @property
    def body_id(self):
        return self._lut(entry_bodies(self.rays.model))

    def points(self, pnt_w, vec_w):
        """the crossing points ``pnt_w + dist * vec_w`` [n, R, 3] of rays given in the world frame
        (tensors broadcastable to [n, R, 3]); NaN where the ray missed"""
        import torch
        x = torch.where(self.dist >= 0, self.dist, torch.full_like(self.dist, float("nan")))
        return pnt_w + x.unsqueeze(-1) * vec_w

    def named(self, name: str) -> "RayHits":
        """the hits of the rays ``concat`` joined under ``name``"""
        sl = self.rays.part(name)
        sub = Rays(self.rays.model, self.rays.records[sl], self.rays.labels[sl])
        return RayHits(sub, self.dist[:, sl], None if self.entry is None else self.entry[:, sl])
