"""Batched counterparts of the reference's env plumbing.

* ``PixelObservationVecEnv`` -- ``utils/wrappers.py:32-76`` ``CustomPixelObservationWrapper``
  over N envs: ``obs_key`` selects ``"pixels"`` or ``"state"`` (``wrappers.py:9-10``), both kept
  (``pixels_only=False``, ``:35``) and readable with ``get_pixels`` / ``get_state``
  (``:72-76``); torch tensors out (``:55,70``); 5-tuple ``(obs, reward, terminated, truncated,
  info)`` (gym 0.26 ``StepAPICompatibility``, ``:34``); an ``action_repeat`` loop with the
  wrapper's ``timer`` and ``max_episode_length`` 200 (``:38-40,57-68``).
  Pixels: the reference renders a 64x64 RGB frame through OpenGL every step; here a pixel
  observation comes from the HIP ray caster, from the same camera (``mj_envs_amd/render.py``),
  rendered only when pixels are asked for: by default the 64x64 metric depth frame
  ``[N, 1, H, W]``; with ``render_kwargs={"mode": "rgb", "ss": 2}`` the colour frame
  ``[N, H, W, 3]`` float32 in 0..255 (Phong-shaded primitives, the hand's collision proxies in
  its mesh material's colour, the goal-marker sites blended in; parity-unpinned against the
  reference's OpenGL frame); with ``render_kwargs={"mode": "segmentation", "kind": "body"}`` the
  label frame ``[N, 1, H, W]`` float32 (``AdroitVecEnv.render_segmentation``); with
  ``render_kwargs={"mode": "pointcloud", "num_points": 512, "crop": "workspace"}`` the
  farthest-point-sampled cloud ``[N, num_points, 3]`` of the depth pixels
  (``AdroitVecEnv.render_pointcloud``).
* ``SB3VecEnv`` -- the stable-baselines3 ``VecEnv`` method surface (``reset``, ``step_async`` /
  ``step_wait``, ``step``, ``get_attr`` / ``set_attr`` / ``env_method``, ``env_is_wrapped``,
  ``seed``, ``close``, ``num_envs``, spaces) without importing SB3; numpy out as SB3 expects
  (the reference's PPO baseline, ``algos/baselines.py:106-183``, wraps its one env in SB3's).
* ``make_env`` / ``step`` / ``reset`` -- ``utils/helpers.py:41-78``: ``state_type``
  ``"observation"`` -> pixels, ``"vector"`` -> state; ``step`` returns ``(obs, reward, done,
  success)`` with ``success = info['goal_achieved']``.

Documented differences from the reference wrapper:
  * ``action_repeat > 1`` raises TypeError in the reference (``items[1] += ...`` on a tuple,
    ``wrappers.py:68``).  Here it runs the intended loop per env: an extra repeat's reward is
    added unless the episode ended in the first step or in that repeat, or the timer passed
    ``max_episode_length`` (``:64``), after which the env's later repeats count for nothing.
    The batch keeps stepping, so an env that ended mid-loop was auto-reset by the kernel: its
    terminated / truncated flag is reported (the reference returns the first step's flags).
"""
from __future__ import annotations

from typing import Any, List, Optional, Sequence

import numpy as np

from .envs import AdroitVecEnv, Box

PIXELS_KEY = "pixels"
STATE_KEY = "state"


class PixelObservationVecEnv:
    """``CustomPixelObservationWrapper`` over an ``AdroitVecEnv`` (device tensors), or over a
    single-env facade (``HammerEnvV0`` ...; its batch of one is wrapped).  ``host_tensors=True``
    returns CPU float tensors and takes numpy / CPU actions, as the reference wrapper does
    (``wrappers.py:55,70-76``), so the reference's drivers -- ``record_policy``
    (``utils/visualize_env.py:108-128``): ``gym_env.env.mj_viewer_headless_setup()``,
    ``reset``, ``get_pixels().numpy()``, ``step(gym_env, a)`` -- run unchanged."""

    def __init__(self, env: AdroitVecEnv, obs_key: str = PIXELS_KEY, render_kwargs: Optional[dict] = None,
                 action_repeat: int = 1, host_tensors: bool = False):
        if obs_key not in (PIXELS_KEY, STATE_KEY):
            raise KeyError(obs_key)
        self._facade = None
        if not isinstance(env, AdroitVecEnv) and isinstance(getattr(env, "vec", None), AdroitVecEnv):
            self._facade = env                # its flags (pen's use_aerial_view) stay reachable
            env = env.vec                     # a single-env facade: wrap its batch of one
        self.host_tensors = bool(host_tensors)
        rk = render_kwargs or {}
        self.env = env
        self.num_envs = env.num_envs
        self.obs_key = obs_key
        self.width, self.height = int(rk.get("width", 64)), int(rk.get("height", 64))
        self.mode, self.ss = rk.get("mode", "depth"), int(rk.get("ss", 1))
        if self.mode not in ("depth", "rgb", "segmentation", "pointcloud"):
            raise ValueError("render_kwargs['mode'] must be 'depth', 'rgb', 'segmentation' or 'pointcloud', "
                             f"not {self.mode!r}")
        # mode "pointcloud": render_kwargs["num_points"] / ["crop"] / ["keep"] / ["sites"] / ["frame"] /
        # ["max_candidates"] as AdroitVecEnv.render_pointcloud takes them; the pixels are the sampled
        # points [N, num_points, 3], width / height the size of the depth frames they come from
        self.cloud_kwargs = dict(num_points=int(rk.get("num_points", 512)), crop=rk.get("crop"), keep=rk.get("keep"),
                                 sites=bool(rk.get("sites", False)), frame=rk.get("frame"),
                                 max_candidates=int(rk.get("max_candidates", 4096)))
        # mode "segmentation": render_kwargs["kind"] / ["lut"] / ["background"] / ["sites"] as
        # AdroitVecEnv.render_segmentation takes them; the labels as float32, shaped like depth
        self.seg_kwargs = dict(kind=rk.get("kind", "geom"), lut=rk.get("lut"), background=int(rk.get("background", -1)),
                               sites=bool(rk.get("sites", False)))
        # render_kwargs["camera"]: a model camera's name, a (record, body) pair or "free" -- or a list
        # of those, rendered in one launch as [N, V, ...]; render_kwargs["env_cams"]: per-env records
        # [N, V, 17] (AdroitVecEnv.render_views).  Without the key: the reference's free camera.
        cam = rk.get("camera")
        self.cameras = None if cam is None else (list(cam) if isinstance(cam, list) else [cam])
        self.multi_view = isinstance(cam, list)
        self.env_cams = rk.get("env_cams")
        if self.env_cams is not None and self.cameras is None:
            raise ValueError("render_kwargs['env_cams'] needs render_kwargs['camera']")
        # mode "rgb": render_kwargs["appearance"] = (lo, hi) of appearance.ranges -- every env draws its own
        # colours, lights and background at reset() and again whenever its episode ends;
        # render_kwargs["shadows"]: cast shadows (AdroitVecEnv.set_appearance)
        self.appearance, self.shadows = rk.get("appearance"), bool(rk.get("shadows", False))
        if (self.appearance is not None or self.shadows) and self.mode != "rgb":
            raise ValueError("render_kwargs['appearance'] / ['shadows'] need mode 'rgb'")
        self.appearance_seed = int(rk.get("appearance_seed", 0))
        self.steps = 0          # step() calls so far: the draw index of the appearance sampler
        if self.appearance is not None or self.shadows:
            env.set_appearance(env.appearance() if self.appearance is not None else None, shadows=self.shadows)
        self.action_repeat = int(action_repeat)
        self.max_episode_length = 200          # wrappers.py:39 (hard-coded there too)
        import torch
        self.timer = torch.zeros(env.num_envs, dtype=torch.int32, device=env.sim.torch_device)
        self._pixels = None
        self._pixels_fresh = False
        self.action_space = env.action_space
        self.state_space = env.observation_space
        lo = -np.inf if self.mode == "segmentation" else 0.0      # labels: whatever the table holds
        self.pixel_space = Box(0.0, 255.0, (self.height, self.width, 3)) if self.mode == "rgb" \
            else Box(lo, np.inf, (1, self.height, self.width))
        if self.multi_view:
            nv = len(self.cameras)
            self.pixel_space = Box(0.0, 255.0, (nv, self.height, self.width, 3)) if self.mode == "rgb" \
                else Box(lo, np.inf, (nv, self.height, self.width))
        if self.mode == "pointcloud":
            self.pixel_space = Box(-np.inf, np.inf, (self.cloud_kwargs["num_points"], 3))
        self.observation_space = self.pixel_space if obs_key == PIXELS_KEY else self.state_space

    # --- observations --------------------------------------------------------------------
    def _out(self, t):
        return t.cpu().clone() if self.host_tensors else t

    def get_state(self):
        return self._out(self.env.obs)

    def get_pixels(self):
        if not self._pixels_fresh:
            n, h, w = self.num_envs, self.height, self.width
            if self.mode == "pointcloud":
                cams = None if self.cameras is None else (self.cameras if self.multi_view else self.cameras[0])
                self._pixels, self.cloud_count = self.env.render_pointcloud(cams, w, h, env_cams=self.env_cams,
                                                                            **self.cloud_kwargs)
            elif self.mode == "segmentation":
                nv = 1 if self.cameras is None else len(self.cameras)
                if self._pixels is None:
                    import torch
                    self._seg32 = self.env.sim.empty(n, nv, h, w, dtype=torch.int32)   # what the kernel writes
                    self._pixels = self.env.sim.empty(n, nv, h, w)
                self.env.render_segmentation(["free"] if self.cameras is None else self.cameras, w, h,
                                             env_cams=self.env_cams, out=self._seg32, **self.seg_kwargs)
                self._pixels.copy_(self._seg32)                                      # float32 labels
            elif self.cameras is not None:
                self._render_cameras(n, h, w)
            elif self.mode == "rgb":
                if self._pixels is None:
                    import torch
                    self._rgb8 = self.env.sim.empty(n, h, w, 3, dtype=torch.uint8)   # what the kernel writes
                    self._pixels = self.env.sim.empty(n, h, w, 3)
                self.env.render_rgb(w, h, ss=self.ss, out=self._rgb8)
                self._pixels.copy_(self._rgb8)                                       # float32 0..255
            else:
                if self._pixels is None:
                    self._pixels = self.env.sim.empty(n, 1, h, w)
                self.env.render_depth(w, h, out=self._pixels.view(n, h, w))
            self._pixels_fresh = True
        return self._out(self._pixels)

    def _render_cameras(self, n, h, w):
        """the pixels of render_kwargs["camera"]: one launch for all its views; a single camera
        keeps the shapes of the free camera's observation"""
        nv = len(self.cameras)
        if self.mode == "rgb":
            if self._pixels is None:
                import torch
                self._rgb8 = self.env.sim.empty(n, nv, h, w, 3, dtype=torch.uint8)
                self._pixels = self.env.sim.empty(n, nv, h, w, 3) if self.multi_view else self.env.sim.empty(n, h, w, 3)
            self.env.render_views(self.cameras, w, h, ss=self.ss, env_cams=self.env_cams, out=self._rgb8)
            self._pixels.view(n, nv, h, w, 3).copy_(self._rgb8)                      # float32 0..255
        else:
            if self._pixels is None:
                self._pixels = self.env.sim.empty(n, nv, h, w)     # one camera: [N, 1, H, W] as before
            self.env.render_views(self.cameras, w, h, rgb=False, depth=True, env_cams=self.env_cams,
                                  depth_out=self._pixels)

    def _obs(self):
        return self.get_pixels() if self.obs_key == PIXELS_KEY else self.get_state()

    def mj_viewer_headless_setup(self):
        """forwarded to the env, as gym's wrapper attribute lookup does for the reference; a wrapped
        single-env facade keeps its own flags (pen_v0.py:174-177 reads use_aerial_view)"""
        return self.env.mj_viewer_headless_setup(self.width, self.height)

    def _actions(self, actions):
        import torch
        if isinstance(actions, torch.Tensor) and actions.device == self.env.sim.torch_device:
            return actions
        a = torch.as_tensor(np.asarray(actions, np.float32) if not isinstance(actions, torch.Tensor)
                            else actions.float())
        return a.reshape(self.num_envs, -1).to(self.env.sim.torch_device)

    # --- episode control -----------------------------------------------------------------
    def reset(self, **kw):
        self.timer.zero_()
        self.env.reset(**kw)
        if self.appearance is not None:      # every env looks new
            self.env.randomize_appearance(self.appearance, seed=self.appearance_seed, draw=self.steps)
        self._pixels_fresh = False
        return self._obs(), {}

    def step(self, actions):
        actions = self._actions(actions)
        obs, rew, term, trunc, info = self.env.step(actions)
        self._pixels_fresh = False
        reward = rew.clone()
        term, trunc = term.clone(), trunc.clone()
        info = dict(info)
        self.timer += 1
        if self.action_repeat > 1:
            # wrappers.py:62-68 per env: after each extra step, stop counting once the first
            # step or this one terminated or the timer passed max_episode_length
            live = ~(term | trunc)
            for _ in range(self.action_repeat - 1):
                _, r2, t2, u2, _ = self.env.step(actions)
                ended_now = (t2 | u2) & live     # the kernel auto-reset it: report the end
                term |= t2 & live
                trunc |= u2 & live
                live &= ~t2 & ~u2 & (self.timer <= self.max_episode_length)
                reward += r2 * live
                self.timer += live.int()
                live &= ~ended_now
            info["goal_achieved"] = self.env.goal.bool()
        ended = term | trunc
        self.timer.masked_fill_(ended, 0)       # the kernel auto-reset these envs
        self.steps += 1
        if self.appearance is not None:
            # the envs whose episode ended start the next one with a new look; the others keep theirs
            ids = ended.nonzero().flatten().int()
            if ids.numel():
                self.env.randomize_appearance(self.appearance, env_ids=ids, seed=self.appearance_seed, draw=self.steps)
        if self.host_tensors:
            reward, term, trunc = reward.cpu(), term.cpu(), trunc.cpu()
            info = {k: (v.cpu() if hasattr(v, "cpu") else v) for k, v in info.items()}
        return self._obs(), reward, term, trunc, info

    def close(self):
        self.env.close()


class SB3VecEnv:
    """stable-baselines3 ``VecEnv`` surface over an ``AdroitVecEnv`` (numpy in / out)."""

    def __init__(self, env: AdroitVecEnv):
        self.env = env
        self.num_envs = env.num_envs
        self.observation_space = env.observation_space
        self.action_space = env.action_space
        self._actions = None
        import torch
        self._act = torch.zeros(env.num_envs, env.nu, device=env.sim.torch_device)

    def reset(self):
        return self.env.reset().cpu().numpy().copy()

    def step_async(self, actions):
        self._actions = np.asarray(actions, np.float32).reshape(self.num_envs, -1)

    def step_wait(self):
        import torch
        self._act.copy_(torch.from_numpy(self._actions))
        obs, rew, term, trunc, info = self.env.step(self._act)
        o = obs.cpu().numpy().copy()
        r = rew.cpu().numpy().copy()
        t, u = term.cpu().numpy(), trunc.cpu().numpy()
        g = info["goal_achieved"].cpu().numpy()
        ended = t | u
        tobs = info["terminal_obs"].cpu().numpy() if ended.any() else None
        infos: List[dict] = []
        for e in range(self.num_envs):
            d = {"goal_achieved": bool(g[e])}
            if ended[e]:
                d["terminal_observation"] = tobs[e].copy()
                d["TimeLimit.truncated"] = bool(u[e] and not t[e])
            infos.append(d)
        return o, r, ended, infos

    def step(self, actions):
        self.step_async(actions)
        return self.step_wait()

    def _idx(self, indices) -> Sequence[int]:
        if indices is None:
            return range(self.num_envs)
        if isinstance(indices, int):
            return [indices]
        return list(indices)

    def get_attr(self, attr_name: str, indices=None) -> List[Any]:
        v = getattr(self.env, attr_name)
        return [v for _ in self._idx(indices)]

    def set_attr(self, attr_name: str, value: Any, indices=None) -> None:
        setattr(self.env, attr_name, value)

    def env_method(self, method_name: str, *args, indices=None, **kwargs) -> List[Any]:
        fn = getattr(self.env, method_name)
        return [fn(*args, **kwargs) for _ in self._idx(indices)]

    def env_is_wrapped(self, wrapper_class, indices=None) -> List[bool]:
        return [False for _ in self._idx(indices)]

    def seed(self, seed: Optional[int] = None) -> List[Optional[int]]:
        if seed is not None:
            self.env.seed = int(seed)
        return [seed for _ in range(self.num_envs)]

    def close(self):
        self.env.close()


# ---------------------------------------------------------------------------------------
def make_env(config, num_envs: int = 1, device: int = 0):
    """``utils/helpers.py:56-78`` make_env for the Adroit suite, batched: ``config.env_name``,
    ``config.variation_type``, ``config.state_type`` ('observation' -> pixels, 'vector' ->
    state), ``config.nogui`` (False: the GUI wrapper, state tensors, no pixels); optional
    ``config.pixel_mode``: ``"depth"`` (default), ``"rgb"`` (colour pixels, 2x2 rays per pixel:
    the reference's resized frame) or ``"segmentation"`` (label pixels shaped like depth; optional
    ``config.segmentation_kind`` -- "geom", "body", "entry", "mujoco" -- and
    ``config.segmentation_sites``) or ``"pointcloud"`` (the sampled cloud ``[N, config.num_points, 3]``,
    default 512 points; optional ``config.pointcloud_crop`` -- a box or "workspace" -- and
    ``config.pointcloud_keep``, as ``AdroitVecEnv.render_pointcloud`` takes them); optional ``config.camera``: the pixels' camera -- a model
    camera's name, a ``(record, body)`` pair or a list of those (``render_kwargs["camera"]``;
    default: the reference's free camera); optional ``config.sensors``: MuJoCo's sensordata in
    ``info["sensordata"]`` of every step (``AdroitVecEnv(sensors=True)``); optional ``config.data``
    (True or group names) and ``config.max_contacts``: the batched ``sim.data`` views in ``env.data``
    (``AdroitVecEnv(data=...)``)."""
    env = AdroitVecEnv(config.env_name, num_envs, device=device,
                       variation_type=getattr(config, "variation_type", None),
                       seed=int(getattr(config, "seed", 1) or 1),
                       sensors=bool(getattr(config, "sensors", False)),
                       data=getattr(config, "data", False) or False,
                       max_contacts=int(getattr(config, "max_contacts", 32) or 32))
    rk = dict(width=64, height=64)
    mode = getattr(config, "pixel_mode", "depth") or "depth"
    if mode == "rgb":
        rk.update(mode="rgb", ss=2)
    elif mode == "segmentation":
        rk.update(mode="segmentation", kind=getattr(config, "segmentation_kind", "geom") or "geom",
                  sites=bool(getattr(config, "segmentation_sites", False)))
    elif mode == "pointcloud":
        rk.update(mode="pointcloud", num_points=int(getattr(config, "num_points", 512) or 512),
                  crop=getattr(config, "pointcloud_crop", None), keep=getattr(config, "pointcloud_keep", None))
    elif mode != "depth":
        raise Exception(f"Unsupported pixel mode '{mode}'")
    if getattr(config, "camera", None) is not None:
        rk.update(camera=config.camera)
    if not getattr(config, "nogui", True):
        return PixelObservationVecEnv(env, obs_key=STATE_KEY, render_kwargs=rk)
    st = getattr(config, "state_type", "vector")
    if st == "observation":
        return PixelObservationVecEnv(env, obs_key=PIXELS_KEY, render_kwargs=rk)
    if st == "vector":
        return PixelObservationVecEnv(env, obs_key=STATE_KEY, render_kwargs=rk)
    raise Exception(f"Unsupported state type '{st}'")


def reset(env):
    return env.reset()


def step(env, action):
    """``utils/helpers.py:44-54``: ``(obs, reward, done, success)``, success = goal_achieved."""
    obs, reward, term, trunc, info = env.step(action)
    return obs, reward, term, info["goal_achieved"]
