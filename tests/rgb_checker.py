"""numpy colour ray caster -- TEST INFRASTRUCTURE ONLY (checker of aw_render_rgb).

fp64 restatement of the shading model of include/adroit_wave.h (aw_render_rgb) over the fp64
oracle's poses.  Ray / primitive crossings come from the depth checker (oracle/depth.py
``ray_local``); this file adds what colour needs:

* the render table: every primitive geom in model order, then the visible sites (group 0-2,
  alpha > 0), each with rgb, alpha, specular, 128*shininess, emission -- rgb is the explicit rgba
  or else the material's; a geom of a group hidden by default (>= 3) stands in for its body's
  absent mesh and takes the first mesh geom's colour and material; geoms are opaque; tint rows
  replace a channel by a scaled per-env param;
* normals (plane +z, sphere radial, capsule radial from the nearest axis point, cylinder side or
  cap, box the slab of entry), flipped to face the ray origin;
* c = emission*a + sum_L [ amb*a + f*(dif*a*max(n.l,0) + [n.l>0]*spe*spec*max(r.v,0)^(128 shin)) ],
  f = attenuation*spot, the headlight (a point light at the camera) before the model's lights;
* the 4 nearest site crossings in front of the opaque one blended back to front;
* ss x ss samples per pixel, averaged, floor(255*clamp(c)+0.5).

The reference renders through OpenGL with meshes and textures that are not available offline,
so like depth this pins the HIP kernel to the model above, not to the reference.
"""
import numpy as np

from oracle.depth import INF, oracle_geoms, ray_local

DEFAULT_LOOK = np.array([0, 0, 0, 0.1, 0.4, 0.5, 1.0])
MESH = 7


# ---------------------------------------------------------------------------------------
# render table from a compiled model
def visible_sites(model):
    return [i for i in range(model.nsite) if model.site_group[i] <= 2 and model.site_rgba[i, 3] > 0]


def _record(model, rgba, matid, alpha):
    default = np.array_equal(rgba, [0.5, 0.5, 0.5, 1.0])
    rgb = model.mat_rgba[matid, :3] if (matid >= 0 and default) else rgba[:3]
    spec, shin, emis = (model.mat_specular[matid], model.mat_shininess[matid], model.mat_emission[matid]) \
        if matid >= 0 else (0.5, 0.5, 0.0)
    return [rgb[0], rgb[1], rgb[2], alpha, spec, 128.0 * shin, emis]


def entry_colors(model, params=None):
    """[n entries, 7] rgb, alpha, specular, 128*shininess, emission of the render table of an
    attached model (tasks.attach_task), with its tint rows applied from ``params``"""
    out = []
    for g in range(model.ngeom):
        if model.geom_type[g] == MESH:
            continue
        src = g
        if model.geom_group[g] >= 3:
            mesh = [q for q in range(model.ngeom)
                    if model.geom_type[q] == MESH and model.geom_bodyid[q] == model.geom_bodyid[g]]
            src = mesh[0] if mesh else g
        out.append(_record(model, model.geom_rgba[src], int(model.geom_matid[src]), 1.0))
    for i in visible_sites(model):
        out.append(_record(model, model.site_rgba[i], int(model.site_matid[i]), model.site_rgba[i, 3]))
    out = np.array(out, np.float64)
    tint = model.arrays.get("task_tint", np.zeros((0, 3), np.int32))
    for (entry, chan, slot), scale in zip(tint, model.arrays.get("task_tint_scale", [])):
        out[entry, chan] = params[slot] * scale
    return out


def model_lights(model):
    """light records: dict(pos, dir, amb, dif, spe, att, cosc (None: no cone), exponent, directional)"""
    out = []
    for l in range(model.nlight):
        directional = bool(model.light_directional[l])
        cone = (not directional) and model.light_cutoff[l] < 180.0
        out.append(dict(pos=model.light_pos[l], dir=model.light_dir[l], amb=model.light_ambient[l],
                        dif=model.light_diffuse[l], spe=model.light_specular[l], att=model.light_attenuation[l],
                        cosc=np.cos(np.radians(model.light_cutoff[l])) if cone else None,
                        exponent=model.light_exponent[l], directional=directional))
    return out


def oracle_sites(orc, model):
    """(type, size, pos, mat) of the visible sites from an Oracle after forward1"""
    sx = orc.get("site_xpos").reshape(-1, 3)
    sm = orc.get("site_xmat").reshape(-1, 9)
    return [(int(model.site_type[i]), model.site_size[i], sx[i], sm[i]) for i in visible_sites(model)]


def oracle_scene(orc, model, params=None):
    """geoms, sites, colours, lights of an Oracle state (after forward1 with ``params``)"""
    return oracle_geoms(orc, model), oracle_sites(orc, model), entry_colors(model, params), model_lights(model)


# ---------------------------------------------------------------------------------------
def _normal(typ, size, lp, pl, vl):
    """outward normal (entry frame) at the surface points lp [n, 3] of rays pl + t vl"""
    n = np.zeros_like(lp)
    if typ == 0:
        n[:, 2] = 1.0
    elif typ == 2:
        n = lp.copy()
    elif typ == 3:
        n = lp.copy()
        n[:, 2] = lp[:, 2] - np.clip(lp[:, 2], -size[1], size[1])
    elif typ == 5:
        side = np.abs(np.hypot(lp[:, 0], lp[:, 1]) - size[0]) <= np.abs(np.abs(lp[:, 2]) - size[1])
        n[:, 0] = np.where(side, lp[:, 0], 0.0)
        n[:, 1] = np.where(side, lp[:, 1], 0.0)
        n[:, 2] = np.where(side, 0.0, lp[:, 2])
    elif typ == 6:
        # the slab whose near crossing is the last one (the face of entry)
        with np.errstate(divide="ignore", invalid="ignore"):
            t1 = (-np.asarray(size) - pl) / vl
            t2 = (np.asarray(size) - pl) / vl
        tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
        tn = np.where(np.isnan(tn), -INF, tn)
        tf = np.where(np.isnan(tf), INF, tf)
        inside = tn.max(-1) < 0                      # origin inside: the exit face
        ax = np.where(inside, tf.argmin(-1), tn.argmax(-1))
        n[np.arange(len(lp)), ax] = lp[np.arange(len(lp)), ax]
    return n / np.linalg.norm(n, axis=-1, keepdims=True)


def _pow(x, e):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(x > 0, np.power(np.maximum(x, 1e-300), e), 0.0)


def shade(entry, color, o, d, t, lights):
    """linear rgb [n, 3] where the rays o + t d [n] cross the entry (type, size, pos, mat)"""
    typ, size, pos, mat = entry
    mat = np.asarray(mat, np.float64).reshape(3, 3)
    size = np.asarray(size, np.float64)
    P = o + t[:, None] * d
    lp = (P - pos) @ mat
    nl = _normal(int(typ), size, lp, np.broadcast_to((o - pos) @ mat, lp.shape), d @ mat)
    n = nl @ mat.T
    n = np.where(((n * d).sum(-1) > 0)[:, None], -n, n)
    a, spec, shin, emis = color[:3], color[4], color[5], color[6]
    rgb = np.tile(emis * a, (len(t), 1))
    for L in lights:
        if L["directional"]:
            l = np.tile(-np.asarray(L["dir"]), (len(t), 1))
            f = np.ones(len(t))
        else:
            l = np.asarray(L["pos"]) - P
            dist = np.linalg.norm(l, axis=-1)
            l = l / dist[:, None]
            f = 1.0 / (L["att"][0] + dist * (L["att"][1] + dist * L["att"][2]))
            if L["cosc"] is not None:
                cs = -(l @ np.asarray(L["dir"]))
                f = np.where(cs >= L["cosc"], f * _pow(cs, L["exponent"]), 0.0)
        ndl = (n * l).sum(-1)
        r = 2.0 * ndl[:, None] * n - l
        sp = np.where(ndl > 0, spec * _pow(-(r * d).sum(-1), shin), 0.0)
        df = np.maximum(ndl, 0.0)
        rgb = rgb + np.asarray(L["amb"])[None] * a[None] + f[:, None] * (
            np.asarray(L["dif"])[None] * a[None] * df[:, None] + np.asarray(L["spe"])[None] * sp[:, None])
    return rgb


def _cross(entries, o, d):
    """t [n entries, n rays] (inf: miss)"""
    out = np.full((len(entries), len(d)), INF)
    for k, (typ, size, pos, mat) in enumerate(entries):
        mat = np.asarray(mat, np.float64).reshape(3, 3)
        vl = d @ mat
        out[k] = ray_local(np.broadcast_to((o - pos) @ mat, vl.shape), vl, int(typ), np.asarray(size, np.float64))
    return out


def headlight(cam, look):
    return dict(pos=np.asarray(cam[:3], np.float64), dir=np.zeros(3), amb=np.full(3, look[3]),
                dif=np.full(3, look[4]), spe=np.full(3, look[5]), att=np.array([1.0, 0, 0]), cosc=None,
                exponent=0.0, directional=False)


def render_rgb(cam, width, height, geoms, sites, colors, lights, look=None, ss=1, quantise=True):
    """-> dict(rgb [H, W, 3] uint8 (float linear colour if not quantise), depth [H, W],
    geom [H, W] (render entry of the opaque crossing, -1: none), site [H, W] (nearest site entry in
    front of it, -1: none)); geom / site / depth are those of the first sample"""
    cam = np.asarray(cam, np.float64)
    look = DEFAULT_LOOK if look is None else np.asarray(look, np.float64)
    o, fwd, up, right = cam[0:3], cam[3:6], cam[6:9], cam[9:12]
    all_lights = ([headlight(cam, look)] if look[6] != 0 else []) + list(lights)
    ng = len(geoms)
    acc = np.zeros((height * width, 3))
    first = None
    for sy in range(ss):
        for sx in range(ss):
            ox, oy = (sx + 0.5) / ss - 0.5, (sy + 0.5) / ss - 0.5
            u = cam[12] + cam[13] * (np.arange(width) + ox)
            w = cam[14] - cam[15] * (np.arange(height) + oy)
            d = fwd[None, None] + u[None, :, None] * right[None, None] + w[:, None, None] * up[None, None]
            d = (d / np.linalg.norm(d, axis=-1, keepdims=True)).reshape(-1, 3)
            tg = _cross(geoms, o, d) if ng else np.full((0, len(d)), INF)
            gid = tg.argmin(0) if ng else np.zeros(len(d), int)
            best = tg.min(0) if ng else np.full(len(d), INF)
            gid = np.where(np.isfinite(best), gid, -1)
            rgb = np.tile(look[:3], (len(d), 1))
            for g in np.unique(gid[gid >= 0]):
                mk = gid == g
                rgb[mk] = shade(geoms[g], colors[g], o, d[mk], best[mk], all_lights)
            sid = np.full(len(d), -1)
            if sites:
                ts = _cross(sites, o, d)
                ts = np.where(ts < best[None], ts, INF)
                order = np.argsort(ts, axis=0, kind="stable")[:4]          # the 4 nearest
                sid = np.where(np.isfinite(ts.min(0)), ng + order[0], -1)
                for rank in range(len(order) - 1, -1, -1):                  # back to front
                    k = order[rank]
                    tk = np.take_along_axis(ts, k[None], 0)[0]
                    for s in np.unique(k[np.isfinite(tk)]):
                        mk = (k == s) & np.isfinite(tk)
                        al = colors[ng + s][3]
                        rgb[mk] = al * shade(sites[s], colors[ng + s], o, d[mk], tk[mk], all_lights) + (1 - al) * rgb[mk]
            acc += rgb
            if first is None:
                depth = np.where(np.isfinite(best), best * (d @ fwd), cam[16])
                first = dict(depth=depth.reshape(height, width), geom=gid.reshape(height, width),
                             site=sid.reshape(height, width))
    c = (acc / (ss * ss)).reshape(height, width, 3)
    first["rgb"] = np.floor(255.0 * np.clip(c, 0, 1) + 0.5).astype(np.uint8) if quantise else c
    return first


def project(cam, point):
    """fractional (col, row) of a world point in the image of a camera record"""
    cam = np.asarray(cam, np.float64)
    v = np.asarray(point, np.float64) - cam[:3]
    z = v @ cam[3:6]
    return ((v @ cam[9:12]) / z - cam[12]) / cam[13], (cam[14] - (v @ cam[6:9]) / z) / cam[15]
