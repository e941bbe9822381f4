"""Label tables of the segmentation renderer (``aw_render_labels``, ``AdroitVecEnv.render_segmentation``).

The ray caster knows, per pixel, which *render entry* it hit: the primitive (non-mesh) geoms in
model order, then the visible sites (group 0-2, alpha > 0) in site order -- the table
``csrc/aw_model_host.h`` builds and ``aw_render_entries`` counts.  A label frame is that entry
passed through an int32 look-up table; this module builds the tables from a compiled model:

* ``"entry"``   the entry index itself;
* ``"geom"``    the model's geom id (sites: -1);
* ``"body"``    the model's body id of the geom / site;
* ``"mujoco"``  mujoco-py's segmentation pair packed into one int, ``objtype << 16 | objid`` with
  mjtObj geom 5 / site 6 (``unpack_mujoco`` splits it again);
* ``body_classes(model, roots)``  class k + 1 for what hangs below ``roots[k]`` in the body tree,
  0 elsewhere: hand / object / table masks;
* ``keep_table(model, roots)``  the byte table of the point-cloud renderer: which entries' pixels
  become points.
"""
from __future__ import annotations

from typing import List, Sequence, Tuple, Union

import numpy as np

MESH = 7
MJOBJ_GEOM, MJOBJ_SITE = 5, 6          # mjtObj
KINDS = ("entry", "geom", "body", "mujoco")
APPEARANCE = ("geom_rgba", "geom_group", "geom_matid", "site_rgba", "site_group", "site_matid", "site_type",
              "site_size", "mat_rgba", "light_pos")


def render_entries(model) -> Tuple[List[int], List[int]]:
    """(geom ids, site ids) in render-entry order: entry k < len(geoms) is geom ``geoms[k]``, entry
    len(geoms) + j is site ``sites[j]``.  A model without the appearance arrays has no site entries."""
    geoms = [g for g in range(int(model.ngeom)) if int(model.geom_type[g]) != MESH]
    sites: List[int] = []
    if all(k in model.arrays for k in APPEARANCE):
        sites = [i for i in range(int(model.nsite)) if model.site_group[i] <= 2 and model.site_rgba[i, 3] > 0]
    return geoms, sites


def entry_bodies(model) -> np.ndarray:
    """int32 [n entries]: the body each render entry belongs to"""
    geoms, sites = render_entries(model)
    return np.array([model.geom_bodyid[g] for g in geoms] + [model.site_bodyid[i] for i in sites], np.int32)


def label_table(model, kind: str = "geom") -> np.ndarray:
    """int32 look-up table [n entries] of ``kind`` (one of KINDS)"""
    geoms, sites = render_entries(model)
    if kind == "entry":
        return np.arange(len(geoms) + len(sites), dtype=np.int32)
    if kind == "geom":
        return np.array(geoms + [-1] * len(sites), np.int32)
    if kind == "body":
        return entry_bodies(model)
    if kind == "mujoco":
        return np.array([MJOBJ_GEOM << 16 | g for g in geoms] + [MJOBJ_SITE << 16 | i for i in sites], np.int32)
    raise ValueError(f"label_table: kind must be one of {KINDS}, not {kind!r}")


def unpack_mujoco(labels, background: int = -1):
    """(objtype, objid) of ``"mujoco"`` labels (numpy or torch); ``background`` pixels give -1, -1"""
    bg = labels == background
    typ, oid = labels >> 16, labels & 0xFFFF
    typ[bg] = -1
    oid[bg] = -1
    return typ, oid


def _body_id(model, b: Union[int, str]) -> int:
    return model.name2id("body", b) if isinstance(b, str) else int(b)


def body_classes(model, roots: Sequence[Union[int, str]]) -> np.ndarray:
    """int32 look-up table [n entries]: class k + 1 for an entry whose body lies in the subtree of
    ``roots[k]`` (body ids or names), 0 elsewhere.  With nested roots the deepest one wins: the
    first root met walking from the entry's body up to the world."""
    ids = [_body_id(model, r) for r in roots]
    assert len(set(ids)) == len(ids), "body_classes: a body is listed twice"
    cls = {b: k + 1 for k, b in enumerate(ids)}
    parent = np.asarray(model.body_parentid)
    out = []
    for b in entry_bodies(model):
        b = int(b)
        while b not in cls and b != 0:
            b = int(parent[b])
        out.append(cls.get(b, 0))
    return np.array(out, np.int32)


def keep_table(model, roots: Sequence[Union[int, str]], drop: bool = False) -> np.ndarray:
    """uint8 keep table [n entries] of the point-cloud renderer (``aw_render_cloud``,
    ``AdroitVecEnv.render_pointcloud(keep=...)``): 1 for an entry whose body lies in the subtree of
    one of ``roots`` (body ids or names), 0 elsewhere -- ``["forearm", "Object"]`` keeps the hand and
    the object and drops the table, the floor and the wall.  ``drop``: the complement, e.g.
    ``keep_table(m, ["table"], drop=True)`` keeps everything but the table."""
    inside = body_classes(model, roots) > 0
    return (~inside if drop else inside).astype(np.uint8)


def names(model, kind: str = "geom") -> dict:
    """{label: name} of a ``label_table(model, kind)`` frame: geom / site names for "entry", "geom"
    and "mujoco" ("site:<name>" for a site entry), body names for "body".  The background label is
    the caller's and is not in the dict."""
    geoms, sites = render_entries(model)
    gn = [model.names["geom"][g] for g in geoms]
    sn = ["site:" + model.names["site"][i] for i in sites]
    lut = label_table(model, kind)
    if kind == "body":
        return {int(b): model.names["body"][int(b)] for b in lut}
    if kind == "geom":
        return {int(l): n for l, n in zip(lut, gn)}
    return {int(l): n for l, n in zip(lut, gn + sn)}
