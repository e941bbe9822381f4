"""Camera observations: depth and colour (BASELINE config 5).

The reference renders RGB through OpenGL from mujoco-py's offscreen free camera
(``hand_manipulation_suite/headless_observer.py:20-52``):

* ``mj_viewer_headless_setup`` (``:20-31``): free camera, ``azimuth = 90``, ``distance = 4.5``,
  then ``set_view('default')`` (``:59-66``): ``elevation = -45 + deg(arccos(v_x / v_z)) / 2`` with
  ``v = body_xpos[obj_bid] - cam_xpos[-1]`` (the model's last camera);
* the camera's look-at point is mujoco-py's free-camera default: the per-axis median of
  ``geom_xpos`` when the render context is created;
* ``render`` (``:34-52``): a 640x480 frame, flipped upright, centre-cropped to 128x128 ("mimic
  zoom") and, with ``enable_resize``, resized to 64x64.

The build replaces the GL rasteriser with a HIP ray caster (``aw_render_depth``): one
workgroup per env, forward kinematics of the env's qpos on one wave, then each geom's pixel
box (its projected bounding sphere); each wave takes 64 pixels, ballots the geoms whose box
meets those rows and casts its rays against only those.  The output is metric z-depth on the
64x64 grid whose pixels are the 2x2 blocks of that 128x128 crop.  Depth has no reference
counterpart (the reference returns RGB), so this path is parity-unpinned against the
reference; it is checked against an independent numpy ray caster on the fp64 oracle's
kinematics (``oracle/depth.py``, ``tests/test_render.py``).

Colour (``aw_render_rgb``, ``k_rgb``) comes from the same camera record, unchanged: per sample
ray the depth renderer's nearest opaque geom, shaded in linear [0, 1] fp32 with

    c = emission a + sum_L [ amb_L a + f_L ( dif_L a max(n.l, 0) + [n.l > 0] spe_L spec max(r.v, 0)^(128 shin) ) ]

(a: the geom's rgb -- an explicit rgba, else its material's; n: the surface normal facing the ray;
l: towards the light, r = reflect(-l, n), v = -ray; f_L = attenuation x spot cone), under the
camera headlight (a point light at the camera: ambient 0.1, diffuse 0.4, specular 0.5) followed
by the model's lights; then the visible sites (group 0-2, alpha > 0: the goal markers -- hammer's
``nail_goal`` / ``S_target``, relocate's per-env ``target``) blended over it back to front,
``c = alpha shade + (1 - alpha) c``.  With ``ss = 2`` four rays through the centres of the pixel's
sub-cells are averaged, so the 64x64 frame is the box-filtered 128x128 crop (the reference's
``enable_resize`` frame); the result is quantised ``floor(255 clamp(c) + 0.5)`` to uint8
``[N, H, W, 3]``, optionally with the aligned depth frame of the same launch (RGB-D).
Stand-in rule: a collision proxy in a group hidden by default (>= 3) is drawn in the colour and
material of the first mesh geom of its body (the hand: ``MatViz``); geoms are opaque.  Tint rows
of the task block show a per-env param as a colour: hammer's ``variation_type="mass"`` sets the
head's red channel to ``mass / 2.5`` as the reference does (``hammer_v0.py:118``).  No textures
(a textured material is drawn with its rgba), reflections, fog or skybox; hard cast shadows from
the model's lights and per-env colours, lights and backgrounds are off unless
``AdroitVecEnv.set_appearance`` / ``randomize_appearance`` switch them on
(``mj_envs_amd/appearance.py``, ``tests/appearance_checker.py``).  Like depth
this is parity-unpinned against the reference's OpenGL frame; it is checked against an fp64 numpy
restatement of the model above (``tests/rgb_checker.py``, ``tests/test_render_rgb.py``).

Other cameras (``aw_render_views``, ``k_views``): a record may be given in the frame of a body
(0: the world) and the kernel composes the world record from that body's pose, so the models'
own ``<camera>``s (``model_camera``: ``fixed``, ``vil_camera``, pen's ``view_1..5``), a camera
riding on a body (``mounted_camera``: an eye-in-hand view on the palm) and one record per env
(``jitter_cameras``: pose and field-of-view randomisation) render through the same ray caster, up
to four views of every env per launch.  ``free_camera`` and the two single-camera entry points
are unchanged.

Point clouds (``aw_render_cloud`` / ``k_cloud``, ``aw_cloud_fps`` / ``k_fps``;
``AdroitVecEnv.render_pointcloud``): the depth pixels of up to four of those cameras unprojected into
the world (``cam + t d`` with the depth frame's own crossing ``t``), cropped to a box
(``workspace_box``: a default per task, over the table top), filtered by render entry
(``labels.keep_table``: drop the table and the background), merged in pixel order and
farthest-point-sampled on the device to a fixed number of points per env, optionally in the frame of
a body such as the palm.

Reference quirks kept: hammer sets up its observer once, in ``__init__``, while ``obj_bid`` is
still the placeholder ``-1`` (``hammer_v0.py:15,35-38``), so the elevation uses the LAST body.
door and relocate construct their observer with placeholder body 0 (``door_v0.py:16,41``,
``relocate_v0.py:14,32``) and call its setup on EVERY reset (``door_v0.py:114``,
``relocate_v0.py:98``): body 0 is the world, so the camera is the same each time.  pen overrides
``mj_viewer_headless_setup`` (its second definition, ``pen_v0.py:163-177``, wins) and calls it on
every reset (``:127``) with ``target_obj_bid``, the 'target' body, whose position reset never
moves (only its orientation is drawn).  Meshes (the hand's visual geoms) are not available
offline; the primitive collision proxies are rendered in their place.
"""
from __future__ import annotations

import math

import numpy as np

from .mjcf import _kinematics0, quat2mat

CAM_FLOATS = 17
ZFAR = 10.0
FULL_W, FULL_H, CROP = 640, 480, 128
FOVY_DEG = 45.0                    # MuJoCo default visual/global/fovy
OBS_BID = {"hammer-v0": -1, "door-v0": 0, "pen-v0": "target", "relocate-v0": 0}   # body id or name


def _geom_world0(model):
    xpos, xquat, xmat = _kinematics0(model)
    gb = model.geom_bodyid
    gpos = np.array([xpos[b] + xmat[b] @ model.geom_pos[g] for g, b in enumerate(gb)])
    return xpos, gpos


def free_camera(model, env_id: str, width: int = 64, height: int = 64, zfar: float = ZFAR,
                aerial: bool = False) -> np.ndarray:
    """The reference's headless camera as the ``AW_CAM_FLOATS`` record of ``aw_render_depth``
    (``aerial``: ``set_view('aerial')``, elevation -45 - deg(...)/2, ``headless_observer.py:62-63``).

    Layout: position[3], forward[3], up[3], right[3], u0, du, v0, dv, zfar.  A ray through output
    pixel (row i, col j) has direction forward + (u0 + du*j) * right + (v0 - dv*i) * up.
    """
    xpos, gpos = _geom_world0(model)
    lookat = np.median(gpos, axis=0)                        # mujoco-py free-camera default
    cam = model.cam_pos[-1] if len(model.cam_pos) else np.zeros(3)
    cam_b = int(model.cam_bodyid[-1]) if len(model.cam_bodyid) else 0
    xq = _kinematics0(model)[1][cam_b]
    cam_world = xpos[cam_b] + quat2mat(xq) @ cam
    bid = OBS_BID.get(env_id, 0)
    if isinstance(bid, str):
        bid = model.name2id("body", bid)
    v = xpos[bid] - cam_world
    ratio = float(np.clip(v[0] / v[2], -1.0, 1.0)) if v[2] != 0 else 0.0
    elevation = -45.0 + (-1.0 if aerial else 1.0) * math.degrees(math.acos(ratio)) / 2.0
    azimuth, distance = 90.0, 4.5
    az, el = math.radians(azimuth), math.radians(elevation)
    fwd = np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
    up = np.array([-math.sin(el) * math.cos(az), -math.sin(el) * math.sin(az), math.cos(el)])
    right = np.cross(fwd, up)
    pos = lookat - distance * fwd
    # full-frame image plane at unit distance: x in [-tx, tx], y in [-ty, ty]
    ty = math.tan(math.radians(FOVY_DEG) / 2.0)
    tx = ty * FULL_W / FULL_H
    # output pixel (i, j) = centre of a (CROP/width) x (CROP/height) block of the centred crop
    bx, by = CROP / width, CROP / height
    x0, y0 = (FULL_W - CROP) / 2.0, (FULL_H - CROP) / 2.0
    u0 = (2.0 * (x0 + 0.5 * bx) / FULL_W - 1.0) * tx
    du = 2.0 * bx / FULL_W * tx
    v0 = (1.0 - 2.0 * (y0 + 0.5 * by) / FULL_H) * ty
    dv = 2.0 * by / FULL_H * ty
    rec = np.concatenate([pos, fwd, up, right, [u0, du, v0, dv, zfar]]).astype(np.float32)
    assert rec.size == CAM_FLOATS
    return rec


def pixel_rays(cam: np.ndarray, width: int, height: int) -> np.ndarray:
    """Unit ray directions [height, width, 3] of a camera record (host-side helper)."""
    cam = np.asarray(cam, np.float64)
    fwd, up, right = cam[3:6], cam[6:9], cam[9:12]
    u = cam[12] + cam[13] * np.arange(width)
    v = cam[14] - cam[15] * np.arange(height)
    d = fwd[None, None] + u[None, :, None] * right[None, None] + v[:, None, None] * up[None, None]
    return d / np.linalg.norm(d, axis=-1, keepdims=True)


# ---------------------------------------------------------------------------------------
# cameras in the frame of a body (aw_render_views): a record keeps the layout above, expressed in
# the frame of a body (0: the world); the kernel composes the world record from the body's pose
def pinhole_record(pos, R, width: int, height: int, fovy: float, zfar: float = ZFAR) -> np.ndarray:
    """The record of a MuJoCo fixed camera at ``pos`` with frame ``R`` (3x3, columns x / y / z):
    it looks along -z, up is +y, right is +x; vertical field of view ``fovy`` degrees over the
    full ``width`` x ``height`` frame (no crop), rays through the pixel centres."""
    R = np.asarray(R, np.float64).reshape(3, 3)
    ty = math.tan(math.radians(float(fovy)) / 2.0)
    tx = ty * width / height
    rec = np.concatenate([np.asarray(pos, np.float64), -R[:, 2], R[:, 1], R[:, 0],
                          [-tx + tx / width, 2.0 * tx / width, ty - ty / height, 2.0 * ty / height, zfar]])
    assert rec.size == CAM_FLOATS
    return rec.astype(np.float32)


def model_camera(model, name: str, width: int = 64, height: int = 64, zfar: float = ZFAR):
    """``(record, body)`` of the model's own camera ``name`` (``fixed``, ``vil_camera``, pen's
    ``view_1`` ...) from the camera table of ``tasks.load_model``; ``KeyError`` if the model was
    loaded without it or declares no such camera."""
    i = model.camera_id(name)
    c = model.cameras
    return (pinhole_record(c["cam_pos"][i], quat2mat(c["cam_quat"][i]), width, height, c["cam_fovy"][i], zfar),
            int(c["cam_bodyid"][i]))


def mounted_camera(model, body, pos, forward, up, width: int = 64, height: int = 64, fovy: float = FOVY_DEG,
                   zfar: float = ZFAR):
    """``(record, body id)`` of a user camera riding on ``body`` (a name or an id; 0 / "world": a
    static camera): ``pos``, ``forward`` and ``up`` in the body's frame, ``up`` orthogonalised
    against ``forward``.  An eye-in-hand view is a camera on ``palm``."""
    bid = model.name2id("body", body) if isinstance(body, str) else int(body)
    if not 0 <= bid < model.nbody:
        raise ValueError(f"mounted_camera: body {body!r} is not a body of the model")
    f = np.asarray(forward, np.float64)
    f = f / np.linalg.norm(f)
    u = np.asarray(up, np.float64)
    u = u - f * (f @ u)
    if np.linalg.norm(u) < 1e-9:
        raise ValueError("mounted_camera: up is parallel to forward")
    u = u / np.linalg.norm(u)
    return pinhole_record(pos, np.stack([np.cross(f, u), u, -f], axis=1), width, height, fovy, zfar), bid


def jitter_cameras(record, n: int, rng: np.random.Generator, pos_sigma: float = 0.0, rot_sigma_deg: float = 0.0,
                   fovy_scale_range=(1.0, 1.0)) -> np.ndarray:
    """``[n, 17]`` float32 per-env records around ``record`` (camera randomisation; the ``env_cam``
    rows of one view): per env a rotation by N(0, ``rot_sigma_deg``) degrees about a uniformly
    random axis applied to forward / up / right (Rodrigues, then re-orthonormalised: forward kept,
    up made orthogonal to it, right = forward x up), a N(0, ``pos_sigma``) offset of the position on
    each axis, and one factor drawn uniformly from ``fovy_scale_range`` on ``u0, du, v0, dv`` (the
    tangent of the half field of view).  Zero sigmas and a unit range return ``record`` n times."""
    rec = np.asarray(record, np.float64).reshape(CAM_FLOATS)
    out = np.tile(rec, (n, 1))
    lo, hi = fovy_scale_range
    for e in range(n):
        axis = rng.normal(size=3)
        ang = math.radians(rot_sigma_deg) * rng.normal()
        dp = pos_sigma * rng.normal(size=3)
        sc = rng.uniform(lo, hi)
        if pos_sigma != 0.0:
            out[e, 0:3] = rec[0:3] + dp
        if rot_sigma_deg != 0.0:
            k = axis / np.linalg.norm(axis)
            rot = lambda v: v * math.cos(ang) + np.cross(k, v) * math.sin(ang) + k * (k @ v) * (1.0 - math.cos(ang))
            f = rot(rec[3:6])
            f = f / np.linalg.norm(f)
            u = rot(rec[6:9])
            u = u - f * (f @ u)
            u = u / np.linalg.norm(u)
            out[e, 3:6], out[e, 6:9], out[e, 9:12] = f, u, np.cross(f, u)
        if (lo, hi) != (1.0, 1.0):
            out[e, 12:16] = rec[12:16] * sc
    return out.astype(np.float32)


# point clouds (aw_render_cloud / aw_cloud_fps, AdroitVecEnv.render_pointcloud): how far above the
# table top the default crop of a task reaches -- door's frame and handle stand 0.70 m tall, the
# other tasks play out within reach of the raised hand
WORKSPACE_HEIGHT = {"hammer-v0": 0.6, "door-v0": 0.8, "pen-v0": 0.6, "relocate-v0": 0.6}
WORKSPACE_CLEARANCE = 0.005        # the box starts this far above the table top: the top itself is cut away


def workspace_box(env_id: str, model=None) -> np.ndarray:
    """Default crop of a task's point cloud: float32 ``[lo xyz, hi xyz]`` in the world frame.  x / y:
    the extent of the table top (the box geom of body ``table``, 0.9 m square, over which the
    object's and the target's reset ranges lie); z: from ``WORKSPACE_CLEARANCE`` above the table
    top, so the top's own pixels fall outside, to ``WORKSPACE_HEIGHT[env_id]`` above it.  The forearm
    enters through the y-lo face and is cut there.  A convenience: pass any box as ``crop``."""
    if model is None:
        from .tasks import load_model
        model = load_model(env_id)
    xpos, _, xmat = _kinematics0(model)
    table = model.name2id("body", "table")
    tops = [g for g in range(int(model.ngeom)) if int(model.geom_bodyid[g]) == table and int(model.geom_type[g]) == 6]
    if not tops:
        raise ValueError(f"workspace_box: {env_id} has no table top (a box geom on body 'table')")
    g = tops[0]
    c = xpos[table] + xmat[table] @ model.geom_pos[g]
    half = np.asarray(model.geom_size[g], np.float64)
    top = c[2] + half[2]
    lo = [c[0] - half[0], c[1] - half[1], top + WORKSPACE_CLEARANCE]
    hi = [c[0] + half[0], c[1] + half[1], top + WORKSPACE_HEIGHT.get(env_id, 0.6)]
    return np.array(lo + hi, np.float32)


def compose_record(record, xpos, xquat) -> np.ndarray:
    """The world record (fp64) of ``record`` given in the frame of a body at ``xpos`` / ``xquat``:
    what the kernel computes in fp32 (host-side helper for checks)."""
    rec = np.asarray(record, np.float64).copy()
    R = quat2mat(np.asarray(xquat, np.float64))
    rec[0:3] = np.asarray(xpos, np.float64) + R @ rec[0:3]
    for k in (3, 6, 9):
        rec[k:k + 3] = R @ rec[k:k + 3]
    return rec
