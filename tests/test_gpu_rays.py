"""Ray queries on the device (aw_set_rays / aw_cast_rays, k_rays) against the fp64 checker
(tests/ray_checker.py over the oracle's kinematics), against the depth and label frames, and their
selection / shape / error / Python surface.  16 envs per handle.

The gate is the project's depth gate: on every ray the checker does not mark ``graze`` the hit flag
agrees and |x_gpu - x_ref| <= 2e-3 m; on every ray marked neither ``graze`` nor ``tie`` the entry
agrees (ray_checker.compare).

Measured on an MI355X (test_site_axes, the state six random steps after reset(seed=3), 16 envs per
task, 168-192 rays each): on average 114-126 rays of an env hit, at 0.0003-7.9 m; 9-34 of 2 688-3 072 rays are ties,
none grazes; the largest |x_gpu - x_ref| is 8.9e-6 m over all hits and over the hits nearer than
0.3 m (hammer 4.8e-6, door 3.3e-6, pen 1.8e-6 / 7.5e-7, relocate 8.9e-6): 1/200 of the gate.  The 4 096
pixel rays agree with the depth frame within 2e-3 m and with the label frame's entry on every pixel.
"""
import numpy as np
import pytest

import ray_checker
from conftest import ENVS, make_oracle

pytestmark = pytest.mark.gpu

N = 16
DIST_FILL, ENTRY_FILL = 123.0, 0x5A5A5A5A
AW_EINVAL = -1


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _rollout(sim, steps=6):
    """test_render's regime: reset(seed=3), then random steps away from the rest pose"""
    torch = _torch()
    n = sim.n_envs
    obs = sim.empty(n, sim.obs_dim)
    sim.reset(obs, seed=3)
    act = sim.empty(n, sim.nu)
    rew, done, goal = sim.empty(n), sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
    for k in range(steps):
        sim.random_actions(act, 7, k)
        sim.step(act, obs, rew, done, goal)
    return obs, rew, done, goal


def _state(sim):
    """(qpos, qvel, params) of every env as fp64 numpy"""
    torch = _torch()
    n = sim.n_envs
    qpos, qvel, params = sim.empty(n, sim.nq), sim.empty(n, sim.nv), sim.empty(n, max(sim.nparam, 1))
    sim.get_state(qpos, qvel, None, params if sim.nparam else None)
    torch.cuda.synchronize()
    f = lambda t: t.cpu().numpy().astype(np.float64)
    return f(qpos), f(qvel), f(params)[:, : sim.nparam]


_CTX = {}


def _ctx(env_id, variation=None):
    """one handle per (task, variation) for the whole module, at the state of test 1; no test that
    uses it changes its state (a cast writes nothing but its outputs)"""
    _torch()
    key = (env_id, variation)
    if key not in _CTX:
        from mj_envs_amd import _native
        from mj_envs_amd.tasks import param_layout
        m, orc = make_oracle(env_id, variation)
        sim = _native.Sim(m.to_blob(), N)
        _rollout(sim)
        Q, V, P = _state(sim)
        _CTX[key] = dict(env_id=env_id, m=m, orc=orc, sim=sim, Q=Q, V=V, P=P,
                         layout=param_layout(env_id, m, variation))
    return _CTX[key]


def _cast(sim, rays, env_ids=None, env_rays=None, entry=True, upload=True):
    """(dist [n, R], entry [n, R] or None) as numpy"""
    torch = _torch()
    if upload:
        sim.set_rays(rays.records)
    n = sim.n_envs if env_ids is None else int(env_ids.shape[0])
    dist = torch.full((n, len(rays)), DIST_FILL, device=sim.torch_device)
    ent = torch.full((n, len(rays)), ENTRY_FILL, dtype=torch.int32, device=sim.torch_device) if entry else None
    sim.cast_rays(dist, ent, env_ids=env_ids, env_rays=env_rays)
    torch.cuda.synchronize()
    return dist.cpu().numpy(), None if ent is None else ent.cpu().numpy()


def _ref(c, rec, envs=None, env_rays=None):
    """the checker's dict, every field stacked over the envs: [n, R]"""
    envs = range(N) if envs is None else envs
    out = [ray_checker.check_env(c["orc"], c["m"], rec, c["P"][e], c["Q"][e], c["V"][e],
                                 None if env_rays is None else env_rays[e], c["layout"]) for e in envs]
    return {k: np.stack([o[k] for o in out]) for k in out[0]}


def _site_axis_rays(m):
    """for every site +-x, +-y, +-z of the site frame from the site's position, its body excluded"""
    from mj_envs_amd import rays
    from mj_envs_amd.mjcf import quat2mat
    sets = []
    for i in range(int(m.nsite)):
        b = int(m.site_bodyid[i])
        R = quat2mat(np.asarray(m.site_quat[i], np.float64))
        sets.append(rays.body_rays(m, b, m.site_pos[i], np.concatenate([R.T, -R.T]), bodyexclude=b))
    return rays.concat(*sets)


def _site_axis_result(c):
    """test 1's table and its GPU result on the shared handle (computed once)"""
    if "axes" not in c:
        r = _site_axis_rays(c["m"])
        c["axes"] = (r,) + _cast(c["sim"], r)
    return c["axes"]


# ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ENVS)
def test_site_axes(env_id):
    """1: 168-192 body-mounted rays, one launch, all 16 envs, every task"""
    c = _ctx(env_id)
    r, dist, ent = _site_axis_result(c)
    assert 168 <= len(r) <= 192
    ref = _ref(c, r.records)
    ray_checker.compare(f"site axes {env_id}", dist, ent, ref, graze_max=0.02, tie_max=0.05)
    assert 100 <= (ref["x"] >= 0).sum(1).min() and ((ent >= 0) == (dist >= 0)).all()
    assert (dist[dist < 0] == -1).all() and ent.max() < len(ray_checker.scene(c["orc"], c["m"]))


def test_pixel_rays_vs_frames():
    """2: the free camera's 4 096 pixel rays through env_rays, 256 per env of 16 clones of env 0,
    against aw_render_depth's frame, aw_render_labels' entries and the checker"""
    torch = _torch()
    from mj_envs_amd import _native, rays
    from mj_envs_amd.render import free_camera, pixel_rays
    env_id, W, H = "hammer-v0", 64, 64
    m, orc = make_oracle(env_id)
    sim = _native.Sim(m.to_blob(), N)
    _rollout(sim)
    dev = sim.torch_device
    sim.clone_envs(torch.zeros(N - 1, dtype=torch.int32, device=dev),
                   torch.arange(1, N, dtype=torch.int32, device=dev))
    cam = free_camera(m, env_id, W, H)
    d = pixel_rays(cam, W, H).reshape(N, 256, 3)
    er = np.concatenate([np.broadcast_to(cam[:3].astype(np.float64), d.shape), d], -1).astype(np.float32)
    table = rays.body_rays(m, 0, np.zeros(3), np.tile([0.0, 0.0, 1.0], (256, 1)))
    dist, ent = _cast(sim, table, env_rays=torch.as_tensor(er, device=dev))
    depth = sim.empty(N, H, W)
    sim.render_depth(depth, cam)
    labels = sim.empty(N, 1, H, W, dtype=torch.int32)
    sim.render_labels([(cam, 0)], W, H, labels, lut=None, background=-1, sites=0)
    torch.cuda.synchronize()
    D, L = depth[0].cpu().numpy().reshape(-1), labels[0, 0].cpu().numpy().reshape(-1)
    x, e = dist.reshape(-1).astype(np.float64), ent.reshape(-1)
    z = np.where(x >= 0, x * (er[..., 3:].reshape(-1, 3).astype(np.float64) @ cam[3:6].astype(np.float64)), cam[16])
    zok = (np.abs(z - D) <= 2e-3) & ((x >= 0) == (D < cam[16]))
    lok = e == L
    print(f"pixel rays: {zok.mean():.5f} of pixels within 2e-3 m of the depth frame, {lok.mean():.5f} carry the label "
          f"frame's entry, {(x >= 0).mean():.3f} hit")
    assert zok.mean() >= 0.995 and lok.mean() >= 0.995 and (x >= 0).mean() > 0.5
    Q, V, P = _state(sim)
    c = dict(m=m, orc=orc, Q=Q, V=V, P=P, layout=None)
    ref = _ref(c, table.records, env_rays=er.astype(np.float64))
    ray_checker.compare("pixel rays vs checker", dist, ent, ref, graze_max=0.02)


FILTERS = dict(exclude=dict(bodyexclude="palm"), moving=dict(flg_static=False, bodyexclude="palm"),
               group=dict(geomgroup=[0, 0, 0, 0, 1, 0], bodyexclude="palm"), obj=dict(bodies=["Object"]))


def test_mounted_fan_and_filters():
    """3: a palm-frame fan on 16 envs in different states under each filter, and keep = 0"""
    from mj_envs_amd import rays
    c = _ctx("hammer-v0")
    m = c["m"]
    parts = {k: rays.fan(m, "palm", [0.0, -1.0, 0.3], 120.0, 40, **f) for k, f in FILTERS.items()}
    none = rays.fan(m, "palm", [0.0, -1.0, 0.3], 120.0, 8)
    none.records["keep"] = 0
    table = rays.concat(none=rays.Rays(m, none.records), **parts)
    dist, ent = _cast(c["sim"], table)
    ref = _ref(c, table.records)
    ray_checker.compare("palm fan, four filters", dist, ent, ref)
    hits = rays.RayHits(table, dist, ent)
    assert (hits.named("none").dist == -1).all() and (hits.named("none").entry == -1).all()
    geoms = [g for g in range(int(m.ngeom)) if m.geom_type[g] != 7]
    body = np.array([m.geom_bodyid[g] for g in geoms])
    for k in FILTERS:
        h = hits.named(k)
        assert (h.dist >= 0).any(), k                                           # the filter leaves something to hit
        assert ((table.records["keep"][table.part(k)][None] >> np.maximum(h.entry, 0).astype(np.uint64)) & np.uint64(1))[h.entry >= 0].all()
    eo = hits.named("obj").entry
    assert (body[eo[eo >= 0]] == m.name2id("body", "Object")).all()
    em = hits.named("moving").entry
    assert (m.body_weldid[body[em[em >= 0]]] != 0).all()
    assert not np.array_equal(hits.named("exclude").dist, hits.named("moving").dist)   # the table and floor were hit
    assert np.unique(dist[:, table.part("exclude")], axis=0).shape[0] == N              # 16 different states


def test_xmax_and_segments():
    """4: a hit at x0 is a miss under xmax = 0.9 x0 and a hit under 1.1 x0; line_of_sight"""
    torch = _torch()
    from mj_envs_amd import rays
    from mj_envs_amd.envs import AdroitVecEnv
    c = _ctx("hammer-v0")
    r, dist, ent = _site_axis_result(c)
    ids = torch.zeros(1, dtype=torch.int32, device=c["sim"].torch_device)
    x0 = dist[0].astype(np.float64)
    assert (x0 >= 0).sum() > 100
    for scale, hit in ((0.9, False), (1.1, True)):
        rec = r.records.copy()
        rec["xmax"] = np.where(x0 >= 0, scale * x0, 0.0)
        d, e = _cast(c["sim"], rays.Rays(c["m"], rec), env_ids=ids)
        assert ((d[0] >= 0) == ((x0 >= 0) & hit)).all(), scale
        if hit:
            assert np.array_equal(d[0], dist[0]) and np.array_equal(e[0], ent[0])
        else:
            assert (d[0] == -1).all() and (e[0] == -1).all()
    # segments from S_grasp to the object body's position, every env: the state of the shared handle
    env = AdroitVecEnv("hammer-v0", N)
    m, orc = c["m"], c["orc"]
    f32 = lambda a: torch.as_tensor(a.astype(np.float32), device=env.sim.torch_device)
    env.set_state(qpos=f32(c["Q"]), qvel=f32(c["V"]), params=f32(c["P"]))
    a, b = np.zeros((N, 1, 3)), np.zeros((N, 1, 3))
    for e_ in range(N):
        orc.forward1(c["P"][e_], c["Q"][e_], c["V"][e_])
        a[e_, 0] = orc.get("site_xpos").reshape(-1, 3)[m.name2id("site", "S_grasp")]
        b[e_, 0] = orc.get("xpos").reshape(-1, 3)[m.name2id("body", "Object")]
    for name, filt in (("all", {}), ("hand only", dict(bodyexclude="Object", flg_static=False))):
        occ, entry = env.line_of_sight(f32(a), f32(b), **filt)
        seg = rays.segments(m, 1, **filt)
        er = np.concatenate([a, b - a], -1).astype(np.float32).astype(np.float64)
        ref = _ref(c, seg.records, env_rays=er)
        want = (ref["x"] >= 0) & (ref["x"] < 1)
        use = ~ref["graze"] & (np.abs(ref["x"] - 1) * np.linalg.norm(er[..., 3:], axis=-1) > ray_checker.TOL)
        occ, entry = occ.cpu().numpy(), entry.cpu().numpy()
        print(f"line of sight ({name}): {int(want.sum())} of {N} occluded, {int((~use).sum())} marginal")
        assert (occ == want)[use].all() and (entry[use & ~ref["tie"]] == np.where(want, ref["entry"], -1)[use & ~ref["tie"]]).all()
        assert tuple(occ.shape) == (N, 1) and ((entry >= 0) == occ).all()
    env.close()


def test_start_inside():
    """5: from the centre of a finger capsule and of the hammer's handle, nothing excluded: the exit
    crossing of that very geom"""
    from mj_envs_amd import rays
    from mj_envs_amd.mjcf import quat2mat
    c = _ctx("hammer-v0")
    m = c["m"]
    geoms = [g for g in range(int(m.ngeom)) if m.geom_type[g] != 7]
    sets, want = [], []
    for name in ("C_ffdistal", "handle"):
        g = m.name2id("geom", name)
        R = quat2mat(np.asarray(m.geom_quat[g], np.float64))
        sets.append(rays.body_rays(m, int(m.geom_bodyid[g]), m.geom_pos[g], R[:, 0]))    # radially out of the capsule
        want.append((geoms.index(g), float(m.geom_size[g, 0])))
    table = rays.concat(*sets)
    dist, ent = _cast(c["sim"], table)
    ref = _ref(c, table.records)
    ray_checker.compare("start inside", dist, ent, ref)
    for k, (e, radius) in enumerate(want):
        assert (ref["entry"][:, k] == e).all() and np.allclose(ref["x"][:, k], radius, atol=1e-9)
        assert (ent[:, k] == e).all() and np.abs(dist[:, k] - radius).max() <= 1e-5


@pytest.mark.parametrize("variation", ["size", "pos"])
def test_per_env_model_params(variation):
    """6: envs with their own geom_size / geom_pos get their own geometry"""
    from mj_envs_amd import rays
    c = _ctx("hammer-v0", variation)
    m = c["m"]
    assert np.unique(c["P"][:, 3:], axis=0).shape[0] == N                       # 16 different heads
    head = m.name2id("geom", "head")
    inside = rays.body_rays(m, "Object", m.geom_pos[head], rays.cone([0, 0, 1], 180.0, 24))   # from the model's head centre
    table = rays.concat(_site_axis_rays(m), head=inside)
    dist, ent = _cast(c["sim"], table)
    ref = _ref(c, table.records)
    ray_checker.compare(f"hammer variation {variation}", dist, ent, ref, graze_max=0.02, tie_max=0.05)
    h = dist[:, table.part("head")]
    assert np.unique(h.round(4), axis=0).shape[0] == N                          # each env sees its own head
    if variation == "size":                                                     # ... and leaves it where its own size ends:
        model_only = np.stack([ray_checker.check_env(c["orc"], m, inside.records, c["P"][e], c["Q"][e], c["V"][e])["x"]
                               for e in range(N)])                              # not where the model's size would
        assert (h >= 0).all() and np.abs(model_only - h).max() > 5e-3


def test_selection_and_shapes():
    """7: R = 1, 64, 65, 256; env_ids as a subset with a repeat and ids out of range; no write past [n][R]"""
    torch = _torch()
    from mj_envs_amd import rays
    c = _ctx("hammer-v0")
    sim, m = c["sim"], c["m"]
    axes = _site_axis_rays(m)
    full = rays.concat(axes, rays.fan(m, "palm", [0.0, -1.0, 0.3], 150.0, 256 - len(axes), bodyexclude="palm"))
    assert len(full) == 256
    dist, ent = _cast(sim, full)
    ray_checker.compare("256 rays", dist, ent, _ref(c, full.records))
    dev = sim.torch_device
    for R in (1, 64, 65):
        sub = rays.Rays(m, full.records[:R])
        sim.set_rays(sub.records)
        buf = torch.full((N * R + 64,), DIST_FILL, device=dev)
        ebuf = torch.full((N * R + 64,), ENTRY_FILL, dtype=torch.int32, device=dev)
        sim.cast_rays(buf[: N * R].view(N, R), ebuf[: N * R].view(N, R))
        torch.cuda.synchronize()
        assert np.array_equal(buf[: N * R].view(N, R).cpu().numpy(), dist[:, :R]), R      # bit for bit the same rays
        assert np.array_equal(ebuf[: N * R].view(N, R).cpu().numpy(), ent[:, :R]), R
        assert (buf[N * R:] == DIST_FILL).all() and (ebuf[N * R:] == ENTRY_FILL).all(), R
    # a subset, a repeated id, ids outside [0, N): the rows of the full cast, the sentinel elsewhere
    sel = [3, 3, 99, 0, -1, 15, N]
    ids = torch.tensor(sel, dtype=torch.int32, device=dev)
    R = 256
    buf = torch.full((len(sel) * R + 64,), DIST_FILL, device=dev)
    ebuf = torch.full((len(sel) * R + 64,), ENTRY_FILL, dtype=torch.int32, device=dev)
    sim.set_rays(full.records)
    sim.cast_rays(buf[: len(sel) * R].view(-1, R), ebuf[: len(sel) * R].view(-1, R), env_ids=ids)
    torch.cuda.synchronize()
    d2, e2 = buf[: len(sel) * R].view(-1, R).cpu().numpy(), ebuf[: len(sel) * R].view(-1, R).cpu().numpy()
    for k, e in enumerate(sel):
        if 0 <= e < N:
            assert np.array_equal(d2[k], dist[e]) and np.array_equal(e2[k], ent[e]), k
        else:
            assert (d2[k] == DIST_FILL).all() and (e2[k] == ENTRY_FILL).all(), k
    assert (buf[len(sel) * R:] == DIST_FILL).all() and (ebuf[len(sel) * R:] == ENTRY_FILL).all()
    # entry = NULL; NULL env_ids = arange(N)
    d3, e3 = _cast(sim, full, entry=False, upload=False)
    assert e3 is None and np.array_equal(d3, dist)
    d4, e4 = _cast(sim, full, env_ids=torch.arange(N, dtype=torch.int32, device=dev), upload=False)
    assert np.array_equal(d4, dist) and np.array_equal(e4, ent)


def test_no_side_effects():
    """8: casting between steps changes nothing of the simulation or of a depth frame"""
    torch = _torch()
    from mj_envs_amd import _native
    from mj_envs_amd.render import free_camera
    m, _ = make_oracle("hammer-v0")
    table = _site_axis_rays(m)
    cam = free_camera(m, "hammer-v0", 64, 64)
    out = []
    for cast in (False, True):
        sim = _native.Sim(m.to_blob(), N)
        obs = sim.empty(N, sim.obs_dim)
        sim.reset(obs, seed=3)
        act, rew = sim.empty(N, sim.nu), sim.empty(N)
        done, goal = sim.empty(N, dtype=torch.uint8), sim.empty(N, dtype=torch.uint8)
        status = sim.empty(N, dtype=torch.int32)
        rec = []
        if cast:
            sim.set_rays(table.records)
            d, e = sim.empty(N, len(table)), sim.empty(N, len(table), dtype=torch.int32)
        for k in range(5):
            sim.random_actions(act, 7, k)
            sim.step(act, obs, rew, done, goal)
            sim.status(last=status)
            rec += [obs.clone(), rew.clone(), done.clone(), status.clone()]
            if cast:
                sim.cast_rays(d, e)
        depth0, depth1 = sim.empty(N, 64, 64), sim.empty(N, 64, 64)
        sim.render_depth(depth0, cam)
        if cast:
            sim.cast_rays(d, e)
        sim.render_depth(depth1, cam)
        qpos, qvel, warm, params = sim.empty(N, sim.nq), sim.empty(N, sim.nv), sim.empty(N, sim.nv), sim.empty(N, sim.nparam)
        sim.get_state(qpos, qvel, warm, params)
        torch.cuda.synchronize()
        assert torch.equal(depth0, depth1)
        out.append([t.cpu() for t in rec + [qpos, qvel, warm, params, depth1]])
    for a, b in zip(*out):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def test_argument_checks():
    """9: every AW_EINVAL of both calls is decided on the host, and a valid cast afterwards still
    gives test 1's numbers; NaN / zero vec rows of env_rays are misses that leave their neighbours alone"""
    torch = _torch()
    from mj_envs_amd import _native
    c = _ctx("hammer-v0")
    sim, m = c["sim"], c["m"]
    r, dist, ent = _site_axis_result(c)
    L = _native.load()
    R, dev = len(r), sim.torch_device

    def still_fine(upload):
        d, e = _cast(sim, r, upload=upload)
        assert np.array_equal(d, dist) and np.array_equal(e, ent)

    sim.set_rays(r.records)
    good = r.records[:4].copy()

    def broken(field, idx, value):
        rec = good.copy()
        if idx is None:
            rec[field][1] = value
        else:
            rec[field][1, idx] = value
        return rec

    bad_tables = [(good, -1), (good, 257), (None, 3),
                  (broken("body", None, int(m.nbody)), None), (broken("body", None, -1), None),
                  (broken("vec", slice(None), 0.0), None), (broken("vec", 1, np.nan), None),
                  (broken("vec", 2, np.inf), None), (broken("pnt", 0, -np.inf), None), (broken("pnt", 2, np.nan), None),
                  (broken("xmax", None, np.nan), None), (broken("xmax", None, np.inf), None)]
    for k, (rec, nrays) in enumerate(bad_tables):
        with pytest.raises(_native.NativeError, match="aw_set_rays"):
            sim.set_rays(rec, nrays=nrays)
        still_fine(upload=False)                           # a refused table leaves the old one in place
    assert L.aw_set_rays(None, good.ctypes.data, 4) == AW_EINVAL
    d = torch.full((N, R), DIST_FILL, device=dev)
    ids = torch.arange(N, dtype=torch.int32, device=dev)
    assert L.aw_cast_rays(None, None, 0, None, d.data_ptr(), None, None) == AW_EINVAL
    assert L.aw_cast_rays(sim.h, None, 0, None, None, None, None) == AW_EINVAL                       # NULL dist
    for n_sel in (0, -3):
        assert L.aw_cast_rays(sim.h, ids.data_ptr(), n_sel, None, d.data_ptr(), None, None) == AW_EINVAL
    assert b"aw_cast_rays" in L.aw_last_error()
    still_fine(upload=False)
    sim.set_rays(None)                                     # nrays 0 drops the table
    assert L.aw_cast_rays(sim.h, None, 0, None, d.data_ptr(), None, None) == AW_EINVAL
    assert b"no ray table" in L.aw_last_error()
    torch.cuda.synchronize()
    assert (d == DIST_FILL).all()                          # no refused call wrote anything
    obs = sim.empty(N, sim.obs_dim)                        # every other call still works
    sim.set_state(obs=obs)
    assert torch.isfinite(obs).all()
    still_fine(upload=True)
    # env_rays: the table's own pnt / vec for every ray, with a NaN vec, a zero vec, an inf pnt planted
    er = np.zeros((N, R, 6), np.float32)
    er[..., :3], er[..., 3:] = r.records["pnt"], r.records["vec"]
    d0, e0 = _cast(sim, r, env_rays=torch.as_tensor(er, device=dev), upload=False)
    assert np.array_equal(d0, dist) and np.array_equal(e0, ent)
    hits = np.flatnonzero(dist[5] >= 0)[:3]
    poisoned = er.copy()
    poisoned[5, hits[0], 3:] = np.nan
    poisoned[5, hits[1], 3:] = 0.0
    poisoned[5, hits[2], 0] = np.inf
    poisoned[7, R - 1, 4] = np.nan
    d1, e1 = _cast(sim, r, env_rays=torch.as_tensor(poisoned, device=dev), upload=False)
    bad = np.zeros((N, R), bool)
    bad[5, hits], bad[7, R - 1] = True, True
    assert (d1[bad] == -1).all() and (e1[bad] == -1).all()
    assert np.array_equal(d1[~bad], dist[~bad]) and np.array_equal(e1[~bad], ent[~bad])


def test_env_surface():
    """10: AdroitVecEnv(rays=...) fills ray_dist / info["ray_dist"] after step, reset and an auto-reset
    with what an explicit raycast gives at the same state; the single-env env.ray"""
    torch = _torch()
    from mj_envs_amd import rays
    from mj_envs_amd.envs import AdroitVecEnv, HammerEnvV0
    from mj_envs_amd.tasks import attach_task, load_model
    m = attach_task(load_model("hammer-v0"), "hammer-v0")
    tips = [s for s in m.names["site"] if s.startswith("S_") and s.endswith("tip")]
    table = rays.concat(range=rays.rangefinder(m, tips, cutoff=0.5),
                        fan=rays.fan(m, "palm", [0.0, -1.0, 0.3], 60.0, 20, bodyexclude="palm"))
    env = AdroitVecEnv("hammer-v0", N, rays=table)
    other = rays.segments(m, 3)

    def same_as_explicit(what):
        hits = env.raycast(table)
        assert torch.equal(hits.dist, env.ray_dist), what
        assert tuple(env.ray_dist.shape) == (N, len(table)) and (env.ray_dist >= 0).any()
        g, b = hits.geom_id.cpu().numpy(), hits.body_id.cpu().numpy()
        e = hits.entry.cpu().numpy()
        assert ((g >= 0) == (e >= 0)).all() and (b[e >= 0] == m.geom_bodyid[g[e >= 0]]).all() and (b[e < 0] == -1).all()
        assert tuple(hits.named("fan").dist.shape) == (N, 20) and torch.equal(hits.hit, hits.dist >= 0)

    env.reset()
    same_as_explicit("reset")
    act = env.sim.empty(N, env.nu)
    for k in range(3):
        env.random_actions(act, k, seed=7)
        _, _, _, _, info = env.step(act)
        assert info["ray_dist"] is env.ray_dist
        same_as_explicit(f"step {k}")
    env.raycast(other)                                     # another table in between: the attached one comes back
    env.sim.set_episode(ep_len=torch.full((N,), env.horizon - 2, dtype=torch.int32, device=env.sim.torch_device))
    before = env.ray_dist.clone()
    truncated = torch.zeros(N, dtype=torch.bool, device=env.sim.torch_device)
    for k in range(3):
        env.random_actions(act, 10 + k, seed=7)
        _, _, _, trunc, info = env.step(act)
        truncated |= trunc
        same_as_explicit(f"auto-reset step {k}")
    assert truncated.all() and not torch.equal(before, env.ray_dist)
    st = env.get_state()
    env.set_state(qpos=st["qpos"].flip(0).contiguous(), qvel=st["qvel"].flip(0).contiguous())
    same_as_explicit("set_state")
    pts = env.raycast(table).points(torch.zeros(3, device=env.sim.torch_device),
                                    torch.ones(3, device=env.sim.torch_device))
    assert tuple(pts.shape) == (N, len(table), 3) and (torch.isnan(pts[..., 0]) == (env.ray_dist < 0)).all()
    env.close()
    off = AdroitVecEnv("hammer-v0", 2)                     # off by default: no attribute, no info key
    off.reset()
    info = off.step(off.sim.empty(2, off.nu).zero_())[4]
    assert "ray_dist" not in info and not hasattr(off, "ray_dist")
    off.close()
    # the single-env facade: mj_ray's arguments, (dist, geomid), -1 / -1 on a miss
    one = HammerEnvV0(seed=5)
    m1, orc = make_oracle("hammer-v0")
    qp, qv = one._qpos_qvel()
    for pnt, vec, kw in (([0.0, 0.0, 1.0], [0.0, 0.0, -1.0], {}), ([0.0, -0.3, 1.0], [0.0, 0.1, -1.0], dict(flg_static=0)),
                         ([0.0, 0.0, 1.0], [0.0, 0.0, -2.0], dict(geomgroup=[1, 0, 0, 0, 0, 0])),
                         ([0.0, 0.0, 3.0], [0.0, 0.0, 1.0], {}), ([0.0, 0.0, 1.0], [0.0, 0.0, -1.0], dict(bodyexclude=0))):
        dist, geomid = one.ray(pnt, vec, **kw)
        assert isinstance(dist, float) and isinstance(geomid, int)
        rec = rays.body_rays(m1, 0, pnt, vec, geomgroup=kw.get("geomgroup"), flg_static=bool(kw.get("flg_static", 1)),
                             bodyexclude=kw.get("bodyexclude", -1)).records
        ref = ray_checker.check_env(orc, m1, rec, one._params(), qp, qv)
        geoms = [g for g in range(int(m1.ngeom)) if m1.geom_type[g] != 7]
        assert not ref["graze"][0] and not ref["tie"][0]
        if ref["x"][0] < 0:
            assert (dist, geomid) == (-1.0, -1)
        else:
            assert abs(dist - ref["x"][0]) * np.linalg.norm(vec) <= ray_checker.TOL and geomid == geoms[ref["entry"][0]]
    assert one.ray([0.0, 0.0, 3.0], [0.0, 0.0, 1.0]) == (-1.0, -1)
    one.close()
