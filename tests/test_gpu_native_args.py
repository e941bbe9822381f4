"""The binding's argument checks on the device (mj_envs_amd/_native.py ``_dev``): every tensor
argument of every checked ``Sim`` method (and of ``cloud_fps``) is refused as a host tensor, with a
wrong dtype, with a wrong shape and non-contiguous -- by an AssertionError raised BEFORE the library
is called -- and the same call then succeeds with the right arguments.

During the refused calls the library is fenced: only the queries that take no caller tensor are
let through, so a check that is missing fails this test instead of handing the kernels a bad pointer.
hammer-v0, 2 envs, 8x8 frames, one view, 4 rays, cap 64: these calls have no size at which they are harder."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, W, H, R, CAP, P = 2, 8, 8, 4, 64, 16


class Fence:
    """the library while bad arguments are handed in"""
    OPEN = ("aw_render_entries", "aw_appearance_defaults", "aw_last_error")

    def __init__(self, lib):
        self._lib = lib

    def __getattr__(self, name):
        if name not in self.OPEN:
            raise RuntimeError(f"{name} was reached with a bad argument")
        return getattr(self._lib, name)


def bad_variants(t):
    """t as a host tensor, with another dtype, with another shape and non-contiguous"""
    import torch
    other = torch.float32 if t.dtype != torch.float32 else torch.int32
    wide = torch.zeros(tuple(t.shape[:-1]) + (2 * t.shape[-1],), dtype=t.dtype, device=t.device)
    out = dict(host=t.cpu(), dtype=t.to(other), shape=t.unsqueeze(0).contiguous(), strided=wide[..., ::2])
    assert out["strided"].shape == t.shape and not out["strided"].is_contiguous()
    return out


@pytest.fixture(scope="module")
def ctx():
    import torch
    from mj_envs_amd import rays
    from mj_envs_amd.envs import AdroitVecEnv
    from mj_envs_amd.render import free_camera
    env = AdroitVecEnv("hammer-v0", N)
    env.reset()
    s = env.sim
    s.set_sensors(True)
    s.set_rays(rays.body_rays(env.model, 0, np.array([0.0, 0.0, 1.0]), np.array([[0, 0, -1.0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])).records)
    assert s.nrays == R
    i32 = lambda *shape: torch.zeros(*shape, dtype=torch.int32, device=s.torch_device)
    ids = lambda: torch.tensor([1, 0], dtype=torch.int32, device=s.torch_device)
    col, light = s.appearance_defaults()
    ne, nl = col.shape[0], light.shape[0]
    rec = np.concatenate([col.ravel(), light.ravel(), [0, 0, 0, 0.1, 0.4, 0.5, 1]]).astype(np.float32)
    views = [(free_camera(env.model, "hammer-v0", W, H), 0)]
    cam = views[0][0]
    data_shapes = dict(xpos=(N, s.nbody, 3), xquat=(N, s.nbody, 4), site_xpos=(N, s.nsite, 3), qacc=(N, s.nv),
                       qfrc_constraint=(N, s.nv), counts=(N, 4), contact=(N, 4, 16))
    f = s.empty
    # call name -> (function of the keyword arguments, the right tensor arguments, the other arguments)
    calls = {
        "sensordata": (s.sensordata, dict(out=f(N, s.nsensordata)), {}),
        "set_data": (lambda **b: s.set_data(True, 4, bufs=b),
                     {k: (i32(*sh) if k == "counts" else f(*sh).zero_()) for k, sh in data_shapes.items()}, {}),
        "set_state_ids": (s.set_state_ids, dict(env_ids=ids(), rows=ids(), qpos=f(N, s.nq).zero_(), qvel=f(N, s.nv).zero_(),
                                                warm=f(N, s.nv).zero_(), params=None, obs=f(N, s.obs_dim)), {}),
        "get_state_ids": (s.get_state_ids, dict(env_ids=ids(), qpos=f(N, s.nq), qvel=f(N, s.nv), warm=f(N, s.nv),
                                                params=f(N, s.nparam)), {}),
        "clone_envs": (s.clone_envs, dict(src_ids=ids(), dst_ids=ids(), obs=f(N, s.obs_dim)), {}),
        "render_depth": (s.render_depth, dict(out=f(N, H, W)), dict(cam=cam)),
        "render_rgb": (s.render_rgb, dict(out=f(N, H, W, 3, dtype=torch.uint8), depth=f(N, H, W)), dict(cam=cam)),
        "render_views": (s.render_views, dict(rgb=f(N, 1, H, W, 3, dtype=torch.uint8), depth=f(N, 1, H, W),
                                              env_cam=torch.as_tensor(np.tile(cam, (N, 1, 1)), device=s.torch_device)),
                         dict(views=views, width=W, height=H)),
        "set_appearance": (s.set_appearance, dict(colors=f(N, ne, 8).zero_(), lights=f(N, nl, 24).zero_(),
                                                  look=f(N, 7).zero_()), {}),
        "appearance_sample": (s.appearance_sample, dict(colors=f(N, ne, 8), lights=f(N, nl, 24), look=f(N, 7), env_ids=ids()),
                              dict(lo=rec, hi=rec)),
        "render_labels": (s.render_labels, dict(labels=i32(N, 1, H, W), depth=f(N, 1, H, W), env_ids=ids(),
                                                env_cam=torch.as_tensor(np.tile(cam, (N, 1, 1)), device=s.torch_device)),
                          dict(views=views, width=W, height=H)),
        "render_cloud": (s.render_cloud, dict(xyz=f(N, CAP, 3), count=i32(N), pix=i32(N, CAP), env_ids=ids(),
                                              env_cam=torch.as_tensor(np.tile(cam, (N, 1, 1)), device=s.torch_device)),
                         dict(views=views, width=W, height=H)),
        "cloud_fps": (None, dict(xyz=f(N, CAP, 3).zero_(), count=i32(N), out_xyz=f(N, P, 3), out_idx=i32(N, P)), {}),
        "dynamics": (lambda qM, jacp, **kw: s.dynamics(dict(qM=qM, jacp=jacp), points=[(0, 1)], **kw),
                     dict(qM=f(N, s.nv, s.nv), jacp=f(N, 1, 3, s.nv), env_ids=ids(), qpos=f(N, s.nq).zero_(),
                          qvel=f(N, s.nv).zero_(), ctrl=f(N, s.nu).zero_()), {}),
        "cast_rays": (s.cast_rays, dict(dist=f(N, R), entry=i32(N, R), env_ids=ids(), env_rays=f(N, R, 6).fill_(1.0)), {}),
    }
    yield dict(env=env, sim=s, calls=calls)
    s.set_appearance()
    s.set_data(0)
    s.set_sensors(False)


def _state(s):
    q, v = s.empty(N, s.nq), s.empty(N, s.nv)
    s.get_state(qpos=q, qvel=v)
    return q.cpu().numpy().view(np.uint32), v.cpu().numpy().view(np.uint32)


CALLS = ("sensordata", "set_data", "set_state_ids", "get_state_ids", "clone_envs", "render_depth", "render_rgb",
         "render_views", "set_appearance", "appearance_sample", "render_labels", "render_cloud", "cloud_fps", "dynamics",
         "cast_rays")


def test_every_checked_call_is_covered(ctx):
    assert set(ctx["calls"]) == set(CALLS)


@pytest.mark.parametrize("call", CALLS)
def test_bad_tensors_never_reach_the_library(ctx, call, monkeypatch):
    from mj_envs_amd import _native
    s = ctx["sim"]
    fn, tensors, rest = ctx["calls"][call]
    fn = fn or _native.cloud_fps
    lib = _native.load()
    # leave a known message in aw_last_error (a NULL handle: nothing is launched)
    assert lib.aw_get_state_ids(None, None, 1, None, None, None, None, None) == -1
    err = lib.aw_last_error()
    assert b"aw_get_state_ids" in err
    q0, v0 = _state(s)
    refused = 0
    with monkeypatch.context() as mp:
        mp.setattr(_native, "load", lambda: Fence(lib))
        for name, t in tensors.items():
            if t is None:
                continue
            for kind, bad in bad_variants(t).items():
                if call == "set_data" and kind == "shape":
                    bad = t.ravel()[:-1].clone()            # (any shape is taken; too few elements is not)
                with pytest.raises(AssertionError, match=f"{call}: {name}"):
                    fn(**{**tensors, name: bad}, **rest)
                assert lib.aw_last_error() == err, (name, kind)
                refused += 1
    assert refused == 4 * sum(t is not None for t in tensors.values())
    q1, v1 = _state(s)
    assert np.array_equal(q0, q1) and np.array_equal(v0, v1)
    fn(**tensors, **rest)                                   # the same call with the right arguments
    assert lib.aw_last_error() == err
