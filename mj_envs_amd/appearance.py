"""Per-env appearance of the colour renderer (``aw_set_appearance``, ``aw_appearance_sample``):
visual domain randomisation -- every env of a batch with its own object and hand colours, its own
lights and its own background -- and cast shadows.

An env's appearance is one record vector ``[col | light | look]``:

* ``col``   ``[ne, 8]``  per render entry (primitive geoms in model order, then the visible sites;
  ``labels.render_entries``): rgb, alpha, specular, 128*shininess, emission, pad;
* ``light`` ``[nlight, 24]``  per model light: pos 0..2, dir 3..5, ambient 6..8, diffuse 9..11,
  specular 12..14, attenuation 15..17, cos(cutoff) or -2 at 18, exponent 19, directional 20,
  castshadow 21, pad;
* ``look``  ``[7]``  background rgb, headlight ambient / diffuse / specular, headlight on.

``model_records`` builds the model's own records on the host (what ``csrc/aw_model_host.h`` puts
into the device tables and ``aw_appearance_defaults`` returns); ``ranges`` turns readable
arguments into the ``lo`` / ``hi`` vectors the on-device sampler interpolates between;
``Appearance`` holds the three device tensors of a batch.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence, Tuple

import numpy as np

from . import labels
from ._native import AW_COL_FLOATS, AW_LIGHT_FLOATS, AW_LOOK_FLOATS

MESH = 7
DEFAULT_LOOK = np.array([0.0, 0.0, 0.0, 0.1, 0.4, 0.5, 1.0], np.float32)
L_POS, L_DIR, L_AMB, L_DIF, L_SPE, L_ATT, L_COSC, L_EXP, L_DIRECTIONAL, L_CASTSHADOW = 0, 3, 6, 9, 12, 15, 18, 19, 20, 21


def _record(model, rgba, matid: int, alpha: float):
    default = np.array_equal(rgba, [0.5, 0.5, 0.5, 1.0])
    rgb = model.mat_rgba[matid, :3] if (matid >= 0 and default) else rgba[:3]
    spec, shin, emis = (model.mat_specular[matid], model.mat_shininess[matid], model.mat_emission[matid]) \
        if matid >= 0 else (0.5, 0.5, 0.0)
    return [rgb[0], rgb[1], rgb[2], alpha, spec, 128.0 * shin, emis, 0.0]


def model_records(model) -> Tuple[np.ndarray, np.ndarray]:
    """(col [ne, 8], light [nlight, 24]) float32: the model's own colour and light records, as the
    device tables hold them.  A geom of a group hidden by default (>= 3) stands in for its body's
    absent mesh and takes the first mesh geom's colour and material; geoms are opaque; tint rows are
    applied by the kernel per env and are not part of the record."""
    if not all(k in model.arrays for k in labels.APPEARANCE):
        raise ValueError("model_records: the model carries no appearance arrays")
    geoms, sites = labels.render_entries(model)
    col = []
    for g in geoms:
        src = g
        if model.geom_group[g] >= 3:
            mesh = [q for q in range(int(model.ngeom))
                    if model.geom_type[q] == MESH and model.geom_bodyid[q] == model.geom_bodyid[g]]
            src = mesh[0] if mesh else g
        col.append(_record(model, model.geom_rgba[src], int(model.geom_matid[src]), 1.0))
    for i in sites:
        col.append(_record(model, model.site_rgba[i], int(model.site_matid[i]), model.site_rgba[i, 3]))
    nl = len(model.light_cutoff)
    light = np.zeros((nl, AW_LIGHT_FLOATS), np.float64)
    for l in range(nl):
        directional = bool(model.light_directional[l])
        for at, key in ((L_POS, "light_pos"), (L_DIR, "light_dir"), (L_AMB, "light_ambient"), (L_DIF, "light_diffuse"),
                        (L_SPE, "light_specular"), (L_ATT, "light_attenuation")):
            light[l, at:at + 3] = model.arrays[key][l]
        cone = (not directional) and model.light_cutoff[l] < 180.0
        light[l, L_COSC] = np.cos(model.light_cutoff[l] * np.pi / 180.0) if cone else -2.0
        light[l, L_EXP] = model.light_exponent[l]
        light[l, L_DIRECTIONAL] = 1.0 if directional else 0.0
        light[l, L_CASTSHADOW] = 1.0
    return np.array(col, np.float64).reshape(-1, AW_COL_FLOATS).astype(np.float32), light.astype(np.float32)


def sizes(model) -> Tuple[int, int, int]:
    """(ne, nlight, F): render entries, lights and the length of an env's record vector"""
    geoms, sites = labels.render_entries(model)
    ne, nl = len(geoms) + len(sites), len(model.light_cutoff)
    return ne, nl, ne * AW_COL_FLOATS + nl * AW_LIGHT_FLOATS + AW_LOOK_FLOATS


def split(model, vec):
    """views (col [..., ne, 8], light [..., nlight, 24], look [..., 7]) of record vectors [..., F]"""
    ne, nl, nf = sizes(model)
    vec = np.asarray(vec)
    assert vec.shape[-1] == nf, f"a record vector of this model holds {nf} floats"
    a, b = ne * AW_COL_FLOATS, ne * AW_COL_FLOATS + nl * AW_LIGHT_FLOATS
    lead = vec.shape[:-1]
    return (vec[..., :a].reshape(*lead, ne, AW_COL_FLOATS), vec[..., a:b].reshape(*lead, nl, AW_LIGHT_FLOATS),
            vec[..., b:])


def _pair(v, what: str):
    """(lo, hi) rgb triples of a colour range: ((r,g,b),(r,g,b)), or one (r,g,b) for both"""
    a = np.asarray(v, np.float64)
    if a.shape == (3,):
        a = np.stack([a, a])
    if a.shape != (2, 3) or not (a[0] <= a[1]).all():
        raise ValueError(f"ranges: {what} must be ((r, g, b), (r, g, b)) with lo <= hi, not {v!r}")
    return a[0], a[1]


def ranges(model, rgb_jitter: float = 0.0, bodies: Optional[Dict[str, Sequence]] = None, light_pos: float = 0.0,
           light_diffuse: Optional[Tuple[float, float]] = None, background=None, headlight=None,
           look: Optional[Sequence[float]] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(lo, hi) float32 [F] for ``AdroitVecEnv.randomize_appearance`` / ``aw_appearance_sample``.
    With no argument lo == hi == the model's records and ``look`` (default: the renderer's default
    look), so nothing varies.

    * ``rgb_jitter``     every entry's rgb within +- this of the model's, clipped to [0, 1];
    * ``bodies``         {body name: ((r,g,b),(r,g,b))}: the rgb range of every entry on that body or
      below it in the body tree (``labels.body_classes``), replacing the jitter; an unknown name raises;
    * ``light_pos``      every light's position within +- this many metres per axis;
    * ``light_diffuse``  (lo, hi): every light's diffuse intensity (grey) in that range;
    * ``background``     ((r,g,b),(r,g,b)): the background colour range;
    * ``headlight``      (lo, hi): the headlight's diffuse intensity in that range.
    """
    col, light = model_records(model)
    base = np.concatenate([col.ravel(), light.ravel(),
                           DEFAULT_LOOK if look is None else np.asarray(look, np.float32).reshape(AW_LOOK_FLOATS)])
    lo, hi = base.astype(np.float32), base.astype(np.float32)
    clo, llo, klo = split(model, lo)
    chi, lhi, khi = split(model, hi)
    if rgb_jitter:
        clo[:, :3] = np.clip(col[:, :3] - np.float32(rgb_jitter), 0.0, 1.0)
        chi[:, :3] = np.clip(col[:, :3] + np.float32(rgb_jitter), 0.0, 1.0)
    for name, rng in (bodies or {}).items():
        if name not in model.names["body"]:
            raise KeyError(f"ranges: the model has no body named {name!r}")
        a, b = _pair(rng, f"bodies[{name!r}]")
        on = labels.body_classes(model, [name]) > 0
        clo[on, :3], chi[on, :3] = a, b
    if light_pos:
        llo[:, L_POS:L_POS + 3] = light[:, L_POS:L_POS + 3] - np.float32(light_pos)
        lhi[:, L_POS:L_POS + 3] = light[:, L_POS:L_POS + 3] + np.float32(light_pos)
    if light_diffuse is not None:
        a, b = float(light_diffuse[0]), float(light_diffuse[1])
        if not a <= b:
            raise ValueError("ranges: light_diffuse must be (lo, hi) with lo <= hi")
        llo[:, L_DIF:L_DIF + 3], lhi[:, L_DIF:L_DIF + 3] = a, b
    if background is not None:
        klo[:3], khi[:3] = _pair(background, "background")
    if headlight is not None:
        a, b = float(headlight[0]), float(headlight[1])
        if not a <= b:
            raise ValueError("ranges: headlight must be (lo, hi) with lo <= hi")
        klo[4], khi[4] = a, b
    return lo, hi


class Appearance:
    """The per-env appearance tables of one ``AdroitVecEnv``: ``colors [N, ne, 8]``, ``lights
    [N, nlight, 24]``, ``look [N, 7]`` -- device fp32 tensors, initialised to the model's records
    (``aw_appearance_defaults``) and the default look.  The render kernels read them at launch once
    ``env.set_appearance(app)`` has handed them over, so a write shows in the next frame."""

    def __init__(self, env, look: Optional[Sequence[float]] = None):
        import torch
        sim = getattr(env, "sim", env)
        col, light = sim.appearance_defaults()
        dev, n = sim.torch_device, sim.n_envs
        lk = DEFAULT_LOOK if look is None else np.asarray(look, np.float32).reshape(AW_LOOK_FLOATS)
        self.colors = torch.from_numpy(col).to(dev).unsqueeze(0).repeat(n, 1, 1).contiguous()
        self.lights = torch.from_numpy(light).to(dev).unsqueeze(0).repeat(n, 1, 1).contiguous()
        self.look = torch.from_numpy(lk.copy()).to(dev).unsqueeze(0).repeat(n, 1).contiguous()

    @property
    def num_floats(self) -> int:
        return self.colors[0].numel() + self.lights[0].numel() + AW_LOOK_FLOATS
