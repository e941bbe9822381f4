"""Per-env appearance and cast shadows on the CPU: the shadow ray of tests/appearance_checker.py on
an analytic scene, what fp32 poses cost it on the task scenes (and that those scenes have shadows
in view), the sampler's restatement, appearance.ranges and the pixel wrapper's draw schedule.
The kernels are held to these restatements in tests/test_gpu_appearance.py."""
import numpy as np
import pytest

from conftest import ENVS, load_task_model, make_oracle

TOL = 2            # per channel, of 255: the colour renderer's criterion (tests/test_render_rgb.py)
EYE = np.eye(3)
GREY = [0.6, 0.5, 0.4, 1.0, 0.0, 64.0, 0.0]           # no highlight: ambient + diffuse only
OFF = [0, 0, 0, 0, 0, 0, 0]                           # black background, headlight off


def _sun(castshadow=True):
    return dict(pos=np.zeros(3), dir=np.array([0, 0, -1.0]), amb=np.full(3, 0.2), dif=np.full(3, 0.7),
                spe=np.zeros(3), att=np.array([1.0, 0, 0]), cosc=None, exponent=0.0, directional=True,
                castshadow=castshadow)


# ---------------------------------------------------------------------------------------
def test_analytic_shadow():
    """a unit sphere at z = 2 over an infinite plane, a directional light straight down, the camera
    looking down from the side"""
    import appearance_checker as ac
    import rgb_checker
    W = H = 41
    fwd = np.array([0.0, 3.0, -4.0]) / 5.0
    right = np.array([1.0, 0, 0])
    up = np.cross(right, fwd)
    span = 0.3
    cam = np.concatenate([[0, -6.0, 8.0], fwd, up, right, [-span, 2 * span / (W - 1), span, 2 * span / (H - 1), 50.0]])
    geoms = [(0, [0, 0, 0], np.zeros(3), EYE), (2, [1.0, 0, 0], np.array([0, 0, 2.0]), EYE)]
    colors = np.array([GREY, GREY])
    lit = ac.render_rgb(cam, W, H, geoms, [], colors, [_sun()], look=OFF, quantise=False)
    sh = ac.render_rgb(cam, W, H, geoms, [], colors, [_sun()], look=OFF, quantise=False, shadows=True)
    a = np.array(GREY[:3])
    # where each pixel's ray meets the plane
    o = cam[:3]
    u = cam[12] + cam[13] * np.arange(W)
    w = cam[14] - cam[15] * np.arange(H)
    d = fwd[None, None] + u[None, :, None] * right[None, None] + w[:, None, None] * up[None, None]
    d /= np.linalg.norm(d, axis=-1, keepdims=True)
    P = o + (-o[2] / d[..., 2])[..., None] * d
    r = np.hypot(P[..., 0], P[..., 1])
    plane, sphere = sh["geom"] == 0, sh["geom"] == 1
    assert (lit["geom"] == sh["geom"]).all() and plane.sum() > 500 and sphere.sum() > 100
    inside, outside = plane & (r < 0.98), plane & (r > 1.02)
    assert inside.sum() > 30 and outside.sum() > 300
    assert np.allclose(sh["rgb"][inside], 0.2 * a)                      # ambient only
    assert np.allclose(sh["rgb"][outside], (0.2 + 0.7) * a)             # fully lit
    assert np.allclose(lit["rgb"][plane], (0.2 + 0.7) * a)              # without shadows: lit everywhere
    # the sphere's own lit hemisphere is unshadowed (the ray leaves the surface it starts on)
    assert np.allclose(sh["rgb"][sphere], lit["rgb"][sphere])
    assert (sh["rgb"][sphere].sum(-1) > 0.2 * a.sum() + 1e-3).mean() > 0.5
    # the headlight casts nothing: with it as the only light, shadows change no pixel
    head = [0, 0, 0, 0.1, 0.4, 0.5, 1.0]
    h0 = ac.render_rgb(cam, W, H, geoms, [], colors, [], look=head, quantise=False)
    h1 = ac.render_rgb(cam, W, H, geoms, [], colors, [], look=head, quantise=False, shadows=True)
    assert np.array_equal(h0["rgb"], h1["rgb"])
    # nor does a light whose castshadow is off
    n1 = ac.render_rgb(cam, W, H, geoms, [], colors, [_sun(False)], look=OFF, quantise=False, shadows=True)
    assert np.array_equal(n1["rgb"], lit["rgb"])
    # a site between light and plane casts nothing, and is itself shaded with shadows
    plane_only = geoms[:1]
    site = [(2, [1.0, 0, 0], np.array([0, 0, 2.0]), EYE)]
    col2 = np.array([GREY, [0.1, 0.9, 0.1, 0.5, 0.0, 64.0, 0.0]])
    s1 = ac.render_rgb(cam, W, H, plane_only, site, col2, [_sun()], look=OFF, quantise=False, shadows=True)
    s0 = ac.render_rgb(cam, W, H, plane_only, site, col2, [_sun()], look=OFF, quantise=False)
    assert np.allclose(s1["rgb"], s0["rgb"]) and (s1["site"] == 1).sum() > 100
    under = (s1["site"] < 0) & (s1["geom"] == 0) & (r < 0.98)
    assert under.sum() > 30 and np.allclose(s1["rgb"][under], (0.2 + 0.7) * a)
    # a site under the sphere is in its shadow
    low = [(2, [0.5, 0, 0], np.array([0, 0, 0.5]), EYE)]
    s2 = ac.render_rgb(cam, W, H, geoms, low, np.array([GREY, GREY, [0.1, 0.9, 0.1, 1.0, 0.0, 64.0, 0.0]]), [_sun()],
                       look=OFF, quantise=False, shadows=True)
    on = s2["site"] == 2
    assert on.sum() > 10 and np.allclose(s2["rgb"][on], 0.2 * np.array([0.1, 0.9, 0.1]))
    # a positional light: nothing beyond it occludes (the sphere is above the light)
    lamp = dict(_sun(), directional=False, pos=np.array([0, 0, 0.9]))
    p1 = ac.render_rgb(cam, W, H, geoms, [], colors, [lamp], look=OFF, quantise=False, shadows=True)
    p0 = ac.render_rgb(cam, W, H, geoms, [], colors, [lamp], look=OFF, quantise=False)
    assert np.allclose(p1["rgb"][plane], p0["rgb"][plane])
    assert rgb_checker.shade.__module__ == "rgb_checker"                # the wrapper is gone again


def _within(a, b):
    return np.abs(a.astype(int) - b.astype(int)).max(-1) <= TOL


def test_shadow_cap_calibration(oracle_lib):
    """test_cap_calibration (tests/test_render_rgb.py) with the shadow ray: the checker on the
    oracle's fp64 poses against the checker on the same poses rounded to fp32 with the camera moved
    1e-6 m -- pixels further apart than 2/255 stay below 0.5 % -- and, on each of those scenes,
    shadows change more than 2 % of the pixels: the GPU tests made like this have shadows in view."""
    import appearance_checker as ac
    import rgb_checker
    from mj_envs_amd.render import free_camera
    from mj_envs_amd.tasks import sample_params
    W = H = 64
    for env_id in ENVS:
        m, orc = make_oracle(env_id)
        rng = np.random.default_rng(5)
        n = 2
        st, _ = orc.reset(sample_params(env_id, m, rng, n))
        for _ in range(6):
            orc.step(st, rng.uniform(-1, 1, (n, orc.nu)))
        cam = free_camera(m, env_id, W, H).astype(np.float64)
        cam32 = cam.copy()
        cam32[:3] += 1e-6
        lights = ac.model_lights(m)
        for e in range(n):
            orc.forward1(st["params"][e], st["qpos"][e], st["qvel"][e])
            geoms, sites, colors, _ = rgb_checker.oracle_scene(orc, m, st["params"][e])
            a = ac.render_rgb(cam, W, H, geoms, sites, colors, lights, shadows=True)["rgb"]
            f32 = lambda es: [(t, s, np.float32(p).astype(np.float64), np.float32(x).astype(np.float64))
                              for t, s, p, x in es]
            b = ac.render_rgb(cam32, W, H, f32(geoms), f32(sites), colors, lights, shadows=True)["rgb"]
            plain = ac.render_rgb(cam, W, H, geoms, sites, colors, lights)["rgb"]
            bad = 1.0 - _within(a, b).mean()
            changed = (a != plain).any(-1).mean()
            print(f"shadow cap calibration {env_id} env {e}: {bad:.5f} of pixels differ by more than {TOL}/255; "
                  f"shadows change {changed:.4f} of the pixels")
            assert bad < 0.005, (env_id, e, bad)
            assert changed > 0.02, (env_id, e, changed)
            assert (a.astype(int) <= plain.astype(int)).all()            # a shadow only darkens


# ---------------------------------------------------------------------------------------
def test_philox_known_answer():
    """Philox4x32-10 test vectors of the Random123 distribution (kat_vectors)"""
    import appearance_checker as ac
    z = ac.philox(np.zeros((1, 4), np.uint32), 0, 0)[0]
    assert [int(v) for v in z] == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    f = ac.philox(np.full((1, 4), 0xFFFFFFFF, np.uint32), 0xFFFFFFFF, 0xFFFFFFFF)[0]
    assert [int(v) for v in f] == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]


def test_sampler_restatement():
    import appearance_checker as ac
    from mj_envs_amd import appearance
    m = load_task_model("relocate-v0")
    ne, nl, nf = appearance.sizes(m)
    lo, hi = appearance.ranges(m, rgb_jitter=0.1, light_pos=0.5, light_diffuse=(0.4, 1.0),
                               background=((0, 0, 0), (1, 1, 1)), headlight=(0.2, 0.6))
    # widen dir too, so that the renormalisation has something to do
    _, llo, _ = appearance.split(m, lo)
    _, lhi, _ = appearance.split(m, hi)
    llo[:, 3:6] -= 0.3
    lhi[:, 3:6] += 0.3
    assert (lo <= hi).all() and (lo < hi).sum() > 3 * ne
    for fma in (False, True):
        v = ac.sample(lo, hi, ne, nl, np.arange(5), seed=11, draw=3, fma=fma)
        assert v.shape == (5, nf) and v.dtype == np.float32
        col, light, look = appearance.split(m, v)
        _, dlo, _ = appearance.split(m, lo)
        _, dhi, _ = appearance.split(m, hi)
        free = np.ones(nf, bool)
        free.reshape(-1)[ne * 8:ne * 8 + nl * 24].reshape(nl, 24)[:, 3:6] = False      # dir: renormalised
        assert ((v >= lo) & (v <= hi))[:, free].all()
        assert np.array_equal(v[:, lo == hi], np.broadcast_to(lo[lo == hi], (5, (lo == hi).sum())))
        for k in ac.LIGHT_FLAGS:
            assert (light[..., k] == dlo[:, k]).all()
        assert (look[:, 6] == lo[-1]).all()
        assert np.allclose(np.linalg.norm(light[..., 3:6].astype(np.float64), axis=-1), 1.0, atol=2e-7)
        assert len({tuple(r) for r in v}) == 5                                        # every env its own
    # lo == hi everywhere: lo bit for bit, for any seed
    base = appearance.ranges(m)[0]
    v = ac.sample(base, base, ne, nl, [0, 7], seed=99, draw=5)
    assert np.array_equal(v.view(np.uint32), np.stack([base, base]).view(np.uint32))
    # a shard reproduces the unsharded rows; seed and draw matter
    a = ac.sample(lo, hi, ne, nl, [2, 3], seed=11, draw=3)
    b = ac.sample(lo, hi, ne, nl, [0, 1], seed=11, draw=3, env_offset=2)
    assert np.array_equal(a, b)
    assert not np.array_equal(a, ac.sample(lo, hi, ne, nl, [2, 3], seed=12, draw=3))
    assert not np.array_equal(a, ac.sample(lo, hi, ne, nl, [2, 3], seed=11, draw=4))


def test_model_records_match_checker():
    """appearance.model_records restates the device tables: rgb_checker's colours and lights"""
    import appearance_checker as ac
    import rgb_checker
    from mj_envs_amd import appearance
    for env_id in ENVS:
        m = load_task_model(env_id)
        col, light = appearance.model_records(m)
        assert col.dtype == np.float32 and col.shape == (appearance.sizes(m)[0], 8) and light.shape == (m.nlight, 24)
        assert np.allclose(ac.colors_from_records(col), rgb_checker.entry_colors(m), rtol=1e-7)
        assert (col[:, 7] == 0).all() and (light[:, 21] == 1).all() and (light[:, 22:] == 0).all()
        for L, R in zip(ac.lights_from_records(light), ac.model_lights(m)):
            for k in ("pos", "dir", "amb", "dif", "spe", "att", "exponent"):
                assert np.allclose(L[k], R[k], rtol=1e-7), (env_id, k)
            assert L["directional"] == R["directional"] and L["castshadow"]
            assert (L["cosc"] is None) == (R["cosc"] is None) and (L["cosc"] is None or abs(L["cosc"] - R["cosc"]) < 1e-7)


def test_ranges():
    from mj_envs_amd import appearance, labels
    from mj_envs_amd.tasks import render_entry
    m = load_task_model("relocate-v0")
    ne, nl, nf = appearance.sizes(m)
    col, light = appearance.model_records(m)
    lo, hi = appearance.ranges(m)
    assert lo.dtype == np.float32 and lo.shape == (nf,) and np.array_equal(lo, hi)
    c, l, k = appearance.split(m, lo)
    assert np.array_equal(c, col) and np.array_equal(l, light) and np.array_equal(k, appearance.DEFAULT_LOOK)
    red = ((0.8, 0.0, 0.0), (1.0, 0.2, 0.2))
    lo, hi = appearance.ranges(m, bodies={"Object": red})
    clo, chi = appearance.split(m, lo)[0], appearance.split(m, hi)[0]
    ball = render_entry(m, m.name2id("geom", "sphere"))
    changed = np.flatnonzero((clo != chi).any(1))
    assert list(changed) == [ball]                                       # the ball's entry only
    assert np.allclose(clo[ball, :3], red[0]) and np.allclose(chi[ball, :3], red[1])
    assert np.array_equal(clo[:, 3:], col[:, 3:]) and np.array_equal(chi[:, 3:], col[:, 3:])
    # a body with a subtree: the palm's entries and everything below it (the fingers)
    lo, hi = appearance.ranges(m, bodies={"palm": ((0, 0, 0), (1, 1, 1))})
    on = (appearance.split(m, lo)[0] != appearance.split(m, hi)[0]).any(1)
    assert np.array_equal(on, labels.body_classes(m, ["palm"]) > 0) and 5 < on.sum() < ne
    with pytest.raises(KeyError):
        appearance.ranges(m, bodies={"no_such_body": red})
    with pytest.raises(ValueError):
        appearance.ranges(m, bodies={"Object": ((1, 1, 1), (0, 0, 0))})
    with pytest.raises(ValueError):
        appearance.ranges(m, light_diffuse=(1.0, 0.4))
    # the other arguments touch their own slots only
    lo, hi = appearance.ranges(m, rgb_jitter=0.1, light_pos=0.5, light_diffuse=(0.4, 1.0),
                               background=((0, 0, 0), (1, 1, 1)), headlight=(0.2, 0.6))
    (clo, llo, klo), (chi, lhi, khi) = appearance.split(m, lo), appearance.split(m, hi)
    assert (clo[:, :3] >= 0).all() and (chi[:, :3] <= 1).all() and (chi[:, :3] - clo[:, :3] <= 0.2 + 1e-6).all()
    assert np.array_equal(clo[:, 3:], chi[:, 3:])
    assert np.allclose(lhi[:, :3] - llo[:, :3], 1.0) and (llo[:, 9:12] == np.float32(0.4)).all() and (lhi[:, 9:12] == 1).all()
    rest = [i for i in range(24) if i not in (0, 1, 2, 9, 10, 11)]
    assert np.array_equal(llo[:, rest], lhi[:, rest])
    assert list(klo) == [0, 0, 0, np.float32(0.1), np.float32(0.2), np.float32(0.5), 1]
    assert list(khi) == [1, 1, 1, np.float32(0.1), np.float32(0.6), np.float32(0.5), 1]
    # hammer: no light in the hand's subtree means nothing, but the model has its one light
    assert appearance.sizes(load_task_model("hammer-v0"))[1] == 1


# ---------------------------------------------------------------------------------------
class _FakeSim:
    torch_device = "cpu"


class _FakeEnv:
    """what PixelObservationVecEnv needs of an AdroitVecEnv, recording the appearance calls"""

    def __init__(self, n):
        import torch
        from mj_envs_amd.envs import Box
        self.num_envs, self.sim, self.calls = n, _FakeSim(), []
        self.action_space, self.observation_space = Box(-1.0, 1.0, (2,)), Box(-np.inf, np.inf, (3,))
        self.obs, self.goal = torch.zeros(n, 3), torch.zeros(n, dtype=torch.uint8)
        self.next_done = torch.zeros(n, dtype=torch.bool)

    def appearance(self):
        return "tables"

    def set_appearance(self, app, shadows=False):
        self.calls.append(("set", app, shadows))

    def randomize_appearance(self, ranges, env_ids=None, seed=0, draw=0):
        self.calls.append(("draw", ranges, None if env_ids is None else [int(i) for i in env_ids], seed, draw))

    def reset(self, **kw):
        self.calls.append(("reset",))
        return self.obs

    def step(self, actions):
        import torch
        self.calls.append(("step",))
        term = self.next_done.clone()
        return self.obs, torch.zeros(self.num_envs), term, torch.zeros_like(term), {"goal_achieved": self.goal.bool()}


def test_wrapper_draw_schedule():
    """draws happen at reset for all envs and after a step only for the envs that ended"""
    import torch
    from mj_envs_amd.wrappers import PixelObservationVecEnv
    n = 4
    env = _FakeEnv(n)
    rng = ("lo", "hi")
    w = PixelObservationVecEnv(env, obs_key="state", render_kwargs={"mode": "rgb", "appearance": rng, "shadows": True,
                                                                    "appearance_seed": 9})
    assert env.calls == [("set", "tables", True)]
    w.reset()
    assert env.calls[1:] == [("reset",), ("draw", rng, None, 9, 0)]
    act = np.zeros((n, 2), np.float32)
    w.step(act)                                            # nobody ended: no draw inside the step
    assert env.calls[3:] == [("step",)]
    env.next_done = torch.tensor([False, True, False, True])
    w.step(act)
    assert env.calls[4:] == [("step",), ("draw", rng, [1, 3], 9, 2)]
    env.next_done = torch.zeros(n, dtype=torch.bool)
    w.step(act)
    assert env.calls[6:] == [("step",)]
    # shadows alone: switched on once, never a draw
    env2 = _FakeEnv(n)
    w2 = PixelObservationVecEnv(env2, obs_key="state", render_kwargs={"mode": "rgb", "shadows": True})
    w2.reset()
    env2.next_done = torch.ones(n, dtype=torch.bool)
    w2.step(act)
    assert env2.calls == [("set", None, True), ("reset",), ("step",)]
    # without either key the env's appearance is never touched
    env3 = _FakeEnv(n)
    w3 = PixelObservationVecEnv(env3, obs_key="state", render_kwargs={"mode": "rgb"})
    w3.reset()
    w3.step(act)
    assert env3.calls == [("reset",), ("step",)]
    with pytest.raises(ValueError):
        PixelObservationVecEnv(_FakeEnv(n), render_kwargs={"mode": "depth", "shadows": True})
