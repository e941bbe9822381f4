"""numpy checker of per-env appearance and cast shadows -- TEST INFRASTRUCTURE ONLY.

Adds to tests/rgb_checker.py (which is not edited) what include/adroit_wave.h states for
aw_set_appearance / aw_appearance_sample:

* the shadow ray, by wrapping ``rgb_checker.shade``: for a sample whose ray crosses an entry at P
  with facing normal n, each light with castshadow set is hidden (its diffuse and specular terms
  vanish, its ambient term stays) where a primitive geom crosses the ray from P + 1e-4 n towards
  the light at 0 < t < dist - 1e-4 (a directional light: any t > 0).  Sites never occlude; the
  headlight never casts.  The loop is exhaustive: no culling here.
* colour and light records (the 8- and 24-float layouts) turned into the checker's tables;
* Philox4x32-10 and the sampler: float i of env e is lo[i] + (hi[i] - lo[i]) u01(x), x = word i & 3
  of philox({genv, draw, 0xA99E, i >> 2}, seed); flag slots copied from lo; dir renormalised.
"""
import contextlib

import numpy as np

import rgb_checker
from oracle.depth import ray_local

EPS = 1e-4
COL_W, LIGHT_W, LOOK_W = 8, 24, 7
LIGHT_FLAGS = (18, 20, 21)


# ---------------------------------------------------------------------------------------
# records -> the checker's tables
def lights_from_records(rec):
    """light dicts of rgb_checker (plus ``castshadow``) from records [nlight, 24]"""
    out = []
    for q in np.asarray(rec, np.float64).reshape(-1, LIGHT_W):
        out.append(dict(pos=q[0:3], dir=q[3:6], amb=q[6:9], dif=q[9:12], spe=q[12:15], att=q[15:18],
                        cosc=q[18] if q[18] > -1.5 else None, exponent=q[19], directional=q[20] != 0,
                        castshadow=q[21] != 0))
    return out


def model_lights(model):
    """rgb_checker.model_lights with MuJoCo's default castshadow = on"""
    return [dict(L, castshadow=True) for L in rgb_checker.model_lights(model)]


def colors_from_records(rec, model=None, params=None):
    """[ne, 7] colour table of rgb_checker from records [ne, 8]; with ``model``: its tint rows
    applied on top from ``params``"""
    out = np.asarray(rec, np.float64).reshape(-1, COL_W)[:, :7].copy()
    if model is not None:
        tint = model.arrays.get("task_tint", np.zeros((0, 3), np.int32))
        for (entry, chan, slot), scale in zip(tint, model.arrays.get("task_tint_scale", [])):
            out[entry, chan] = params[slot] * scale
    return out


# ---------------------------------------------------------------------------------------
# the shadow ray
def occluded(geoms, entry, o, d, t, L):
    """bool [n]: whether a geom hides light L from the points where the rays o + t d cross ``entry``"""
    typ, size, pos, mat = entry
    mat = np.asarray(mat, np.float64).reshape(3, 3)
    size = np.asarray(size, np.float64)
    P = o + t[:, None] * d
    lp = (P - pos) @ mat
    nl = rgb_checker._normal(int(typ), size, lp, np.broadcast_to((o - pos) @ mat, lp.shape), d @ mat)
    n = nl @ mat.T
    n = np.where(((n * d).sum(-1) > 0)[:, None], -n, n)
    if L["directional"]:
        l = np.tile(-np.asarray(L["dir"], np.float64), (len(t), 1))
        tmax = np.full(len(t), np.inf)
    else:
        l = np.asarray(L["pos"], np.float64) - P
        dist = np.linalg.norm(l, axis=-1)
        l = l / dist[:, None]
        tmax = dist - EPS
    Ps = P + EPS * n
    hit = np.zeros(len(t), bool)
    for gt, gs, gp, gm in geoms:
        gm = np.asarray(gm, np.float64).reshape(3, 3)
        tt = ray_local((Ps - gp) @ gm, l @ gm, int(gt), np.asarray(gs, np.float64))
        hit |= (tt > 0) & (tt < tmax)
    # the ray is cast only where the light reaches the surface at all; elsewhere f (df) is 0 anyway
    return hit & ((n * l).sum(-1) > 0)


@contextlib.contextmanager
def shadow_shade(geoms):
    """rgb_checker.shade wrapped with the shadow ray against ``geoms`` for the time of the block"""
    plain = rgb_checker.shade

    def shade(entry, color, o, d, t, lights):
        base = plain(entry, color, o, d, t, [])          # emission
        rgb = base.copy()
        for L in lights:
            term = plain(entry, color, o, d, t, [L]) - base
            if L.get("castshadow", False):
                dark = dict(L, dif=np.zeros(3), spe=np.zeros(3))
                occ = occluded(geoms, entry, o, d, t, L)
                term = np.where(occ[:, None], plain(entry, color, o, d, t, [dark]) - base, term)
            rgb = rgb + term
        return rgb

    rgb_checker.shade = shade
    try:
        yield
    finally:
        rgb_checker.shade = plain


def render_rgb(cam, width, height, geoms, sites, colors, lights, look=None, ss=1, quantise=True, shadows=False):
    """rgb_checker.render_rgb, with cast shadows when ``shadows`` (the headlight it builds from
    ``look`` carries no castshadow key and never casts)"""
    if not shadows:
        return rgb_checker.render_rgb(cam, width, height, geoms, sites, colors, lights, look=look, ss=ss, quantise=quantise)
    with shadow_shade(geoms):
        return rgb_checker.render_rgb(cam, width, height, geoms, sites, colors, lights, look=look, ss=ss, quantise=quantise)


# ---------------------------------------------------------------------------------------
# the sampler
def philox(c, k0, k1):
    """Philox4x32-10: counters c [..., 4] uint32, key (k0, k1) -> [..., 4] uint32"""
    c = [np.asarray(c[..., i], np.uint64) for i in range(4)]
    k0, k1 = np.uint64(k0 & 0xFFFFFFFF), np.uint64(k1 & 0xFFFFFFFF)
    M = np.uint64(0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c[0], np.uint64(0xCD9E8D57) * c[2]
        hi0, lo0, hi1, lo1 = p0 >> np.uint64(32), p0 & M, p1 >> np.uint64(32), p1 & M
        c = [hi1 ^ c[1] ^ k0, lo1, hi0 ^ c[3] ^ k1, lo0]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & M, (k1 + np.uint64(0xBB67AE85)) & M
    return np.stack(c, -1).astype(np.uint32)


def u01(x):
    return (np.asarray(x, np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(1.0 / 16777216.0)


def sample(lo, hi, ne, nlight, envs, seed, draw, env_offset=0, fma=False):
    """float32 [len(envs), F] record vectors the device sampler writes for ``envs``.  ``fma``: the
    interpolation with one rounding (the contraction the kernel's compiler may choose)."""
    lo, hi = np.asarray(lo, np.float32), np.asarray(hi, np.float32)
    nf = ne * COL_W + nlight * LIGHT_W + LOOK_W
    assert lo.shape == (nf,) and hi.shape == (nf,)
    envs = np.asarray(envs, np.int64)
    i = np.arange(nf)
    c = np.zeros((len(envs), nf, 4), np.uint32)
    c[..., 0] = ((envs + env_offset) & 0xFFFFFFFF)[:, None]
    c[..., 1] = draw & 0xFFFFFFFF
    c[..., 2] = 0xA99E
    c[..., 3] = (i >> 2)[None]
    x = philox(c, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
    u = u01(np.take_along_axis(x, np.broadcast_to((i & 3)[None, :, None], (len(envs), nf, 1)), -1)[..., 0])
    if fma:
        out = (lo.astype(np.float64) + (hi - lo).astype(np.float64) * u.astype(np.float64)).astype(np.float32)
    else:
        out = (lo + ((hi - lo) * u).astype(np.float32)).astype(np.float32)
    a = ne * COL_W
    for l in range(nlight):
        b = a + l * LIGHT_W
        for k in LIGHT_FLAGS:
            out[:, b + k] = lo[b + k]
        dv = out[:, b + 3:b + 6].astype(np.float64)
        nn = dv[:, 0] * dv[:, 0] + dv[:, 1] * dv[:, 1] + dv[:, 2] * dv[:, 2]
        ok = nn > 0
        out[ok, b + 3:b + 6] = (dv[ok] / np.sqrt(nn[ok])[:, None]).astype(np.float32)
    out[:, nf - 1] = lo[nf - 1]
    return out
