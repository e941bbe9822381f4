"""Point-cloud checker -- TEST INFRASTRUCTURE ONLY (checker of aw_render_cloud / aw_cloud_fps).

Two independent restatements of include/adroit_wave.h:

* farthest-point sampling: ``fps`` is the rule in numpy fp32, every difference, product and sum
  one rounded fp32 operation in the header's order, so its choice is the kernel's bit for bit;
  ``fps_definition`` is the rule as a sentence in fp64 (per candidate the minimum over ALL
  selections so far, recomputed from scratch), which pins ``fps`` itself;
* unprojection: per pixel the render entry (the label rule of tests/label_checker.py) and the
  world point ``cam + t d`` in fp64 on the oracle's poses, from ``rgb_checker._cross``; membership
  of the cloud is then the keep table and the closed crop box.
"""
import numpy as np

import rgb_checker
from oracle.depth import INF


# ---------------------------------------------------------------------------------------
# farthest-point sampling
def fps(xyz, count, npoints):
    """int32 [npoints] of one row: xyz [cap, 3], ``count`` candidates (clamped to cap)"""
    xyz = np.asarray(xyz, np.float32)
    c = int(min(max(int(count), 0), len(xyz)))
    if c == 0:
        return np.full(npoints, -1, np.int32)
    p = xyz[:c]
    mind = np.full(c, np.inf, np.float32)
    sel = [0]
    for _ in range(1, min(npoints, c)):
        d = p - p[sel[-1]]                                           # fp32 - fp32 -> fp32
        sq = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert sq.dtype == np.float32
        mind = np.minimum(mind, sq)
        sel.append(int(np.argmax(mind)))                             # the first maximum: the lowest index
    return np.array([sel[k % c] for k in range(npoints)], np.int32)


def fps_rows(xyz, count, npoints):
    """int32 [n, npoints] of xyz [n, cap, 3], count [n]"""
    return np.stack([fps(x, c, npoints) for x, c in zip(xyz, count)])


def fps_definition(points, npoints, highest=False):
    """the selection rule in fp64, from the definition: list of min(npoints, c) indices.
    ``highest``: the rule with ties going to the highest index instead (to show that there are ties)"""
    p = np.asarray(points, np.float64)
    sel = [0]
    while len(sel) < min(npoints, len(p)):
        best, arg = -1.0, -1
        for i in range(len(p)):
            m = min(float(((p[i] - p[s]) ** 2).sum()) for s in sel)
            if m > best or (highest and m == best):                  # strict: the lowest index keeps a tie
                best, arg = m, i
        sel.append(arg)
    return sel


# ---------------------------------------------------------------------------------------
# unprojection
def unproject(cam, width, height, geoms, sites=(), with_sites=False):
    """(entry [H*W] int, -1: nothing; xyz [H*W, 3] fp64, NaN where nothing; t [H*W]) of a world
    camera record over checker entries (rgb_checker.oracle_scene): the nearest geom crossing, or
    with ``with_sites`` the nearest visible-site crossing strictly in front of it"""
    cam = np.asarray(cam, np.float64)
    o, fwd, up, right = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    u = cam[12] + cam[13] * np.arange(width)
    w = cam[14] - cam[15] * np.arange(height)
    d = fwd[None, None] + u[None, :, None] * right[None, None] + w[:, None, None] * up[None, None]
    d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
    ng = len(geoms)
    tg = rgb_checker._cross(geoms, o, d)
    t = tg.min(0)
    entry = np.where(np.isfinite(t), tg.argmin(0), -1)
    if with_sites and len(sites):
        ts = rgb_checker._cross(list(sites), o, d)
        ts = np.where(ts < t[None], ts, INF)
        front = ts.min(0)
        entry = np.where(np.isfinite(front), ng + ts.argmin(0), entry)
        t = np.where(np.isfinite(front), front, t)
    with np.errstate(invalid="ignore"):
        xyz = np.where((entry >= 0)[:, None], o[None] + np.where(np.isfinite(t), t, 0.0)[:, None] * d, np.nan)
    return entry, xyz, t


def members(entry, xyz, keep=None, box=None):
    """bool [H*W]: the pixels whose point belongs to the cloud"""
    ok = entry >= 0
    if keep is not None:
        ok &= np.asarray(keep)[np.maximum(entry, 0)] != 0
    if box is not None:
        box = np.asarray(box, np.float64)
        with np.errstate(invalid="ignore"):
            ok &= ((xyz >= box[None, :3]) & (xyz <= box[None, 3:])).all(-1)
    return ok


def to_body_frame(xyz, xpos, xquat):
    """rot(xquat)^T (xyz - xpos) in fp64"""
    from mj_envs_amd.mjcf import quat2mat
    return (np.asarray(xyz, np.float64) - np.asarray(xpos, np.float64)) @ quat2mat(np.asarray(xquat, np.float64))
