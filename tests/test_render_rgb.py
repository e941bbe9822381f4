"""RGB camera observations: appearance tables of the compiled models, the fp64 colour checker on
analytic scenes (CPU), and the HIP colour ray caster (aw_render_rgb) against the checker on the
fp64 oracle's kinematics (GPU).

Parity is unpinned against the reference (OpenGL, meshes and PNG textures, not available
offline); the kernel is held to the shading model of include/adroit_wave.h as restated in
tests/rgb_checker.py: >= 99 % of pixels within 2/255 in every channel (the rest: silhouette
pixels whose ray grazes an edge and flips between two surfaces in fp32, and the rounding of the
highlight's power).  test_cap_calibration bounds what fp32 poses alone cost of that 1 %.
"""
import numpy as np
import pytest

from conftest import ENVS, load_task_model, make_oracle

TOL = 2            # per channel, of 255
APPEARANCE = ("geom_rgba", "geom_group", "geom_matid", "site_rgba", "site_group", "site_matid", "mat_rgba",
              "mat_specular", "mat_shininess", "mat_emission", "light_pos", "light_dir", "light_directional",
              "light_ambient", "light_diffuse", "light_specular", "light_attenuation", "light_cutoff",
              "light_exponent")
VISIBLE = {"hammer-v0": ["nail_goal", "S_target"], "door-v0": [], "pen-v0": [], "relocate-v0": ["target"]}


# ---------------------------------------------------------------------------------------
# CPU: model tables
def test_model_tables():
    import rgb_checker
    from mj_envs_amd.tasks import load_model
    for env_id in ENVS:
        m = load_model(env_id)
        ng, ns, nm, nl = m.ngeom, m.nsite, m.nmat, m.nlight
        shapes = dict(geom_rgba=(ng, 4), geom_group=(ng,), geom_matid=(ng,), site_rgba=(ns, 4), site_group=(ns,),
                      site_matid=(ns,), mat_rgba=(nm, 4), mat_specular=(nm,), mat_shininess=(nm,),
                      mat_emission=(nm,), light_pos=(nl, 3), light_dir=(nl, 3), light_directional=(nl,),
                      light_ambient=(nl, 3), light_diffuse=(nl, 3), light_specular=(nl, 3),
                      light_attenuation=(nl, 3), light_cutoff=(nl,), light_exponent=(nl,))
        assert set(shapes) == set(APPEARANCE)
        for k, shp in shapes.items():
            assert getattr(m, k).shape == shp, (env_id, k)
        for ids in (m.geom_matid, m.site_matid):
            assert ids.min() >= -1 and ids.max() < nm
        assert nl == 1 and np.allclose(np.linalg.norm(m.light_dir, axis=1), 1.0)
        # MuJoCo's defaults where the XML is silent
        assert np.allclose(m.light_ambient, 0) and m.light_cutoff[0] == 45 and m.light_exponent[0] == 10
        assert np.allclose(m.light_attenuation, [[1, 0, 0]])
        viz = m.name2id("material", "MatViz")
        assert np.allclose(m.mat_rgba[viz], [0.9, 0.7, 0.5, 1]) and m.mat_specular[viz] == 0.75
        assert m.mat_shininess[m.name2id("material", "tablecube")] == 0.5      # default
        assert [m.names["site"][i] for i in rgb_checker.visible_sites(m)] == VISIBLE[env_id]
    m = load_model("hammer-v0")
    assert np.allclose(m.geom_rgba[m.name2id("geom", "head")], [0.4, 0.4, 0.4, 1])
    assert np.allclose(m.geom_rgba[m.name2id("geom", "handle")], [0.5, 0.5, 0.5, 1])     # default, MatWood
    assert np.allclose(m.site_rgba[m.name2id("site", "S_target")], [0, 1, 0, 0.2])
    # stand-in rule: the hand's collision proxies take MatViz from their body's mesh geom
    col = rgb_checker.entry_colors(load_task_model("hammer-v0"))
    from mj_envs_amd.tasks import render_entry
    palm = col[render_entry(m, m.name2id("geom", "C_palm0"))]
    assert np.allclose(palm, [0.9, 0.7, 0.5, 1, 0.75, 12.8, 0])
    assert col.shape == (int((m.geom_type != 7).sum()) + 2, 7)


def test_tint_rows():
    from mj_envs_amd.tasks import render_entry
    for env_id in ENVS:
        for var in ([None, "mass", "pos", "size"] if env_id == "hammer-v0" else [None]):
            m = load_task_model(env_id, var)
            rows = m.arrays["task_tint"]
            if env_id == "hammer-v0" and var == "mass":
                assert rows.shape == (1, 3)
                assert list(rows[0]) == [render_entry(m, m.name2id("geom", "head")), 0, 3]
                assert np.allclose(m.arrays["task_tint_scale"], [1 / 2.5])
            else:
                assert rows.shape == (0, 3) and len(m.arrays["task_tint_scale"]) == 0


# ---------------------------------------------------------------------------------------
# CPU: checker on analytic scenes
CAM = np.array([0, -5, 0, 0, 1, 0, 0, 0, 1, 1, 0, 0, -0.1, 0.2 / 10, 0.1, 0.2 / 10, 10.0])   # 11x11, centre (5, 5)
EYE = np.eye(3)
GREY = np.array([[0.6, 0.5, 0.4, 1.0, 0.5, 64.0, 0.0]])


def test_checker_sphere_headlight():
    from rgb_checker import render_rgb
    sph = [(2, [0.5, 0, 0], np.zeros(3), EYE)]
    r = render_rgb(CAM, 11, 11, sph, [], GREY, [], quantise=False)["rgb"]
    # centre pixel: n = l = v -> (amb + dif) a + spe spec
    assert np.allclose(r[5, 5], (0.1 + 0.4) * GREY[0, :3] + 0.5 * 0.5, atol=1 / 255)
    # brightness falls towards the limb
    lum = r.sum(-1)
    hit = render_rgb(CAM, 11, 11, sph, [], GREY, [])["geom"][5] == 0
    cols = np.nonzero(hit)[0]
    assert len(cols) >= 5 and np.all(np.diff(lum[5, 5:cols[-1] + 1]) < 0) and np.all(np.diff(lum[5, cols[0]:6]) > 0)
    q = render_rgb(CAM, 11, 11, sph, [], GREY, [])
    assert q["rgb"].dtype == np.uint8 and np.all(q["rgb"][0, 0] == 0) and q["geom"][0, 0] == -1
    assert np.array_equal(q["rgb"][5, 5], np.floor(255 * r[5, 5] + 0.5).astype(np.uint8))


def test_checker_box_face_uniform():
    """a face seen square-on from far away under a directional light has one colour"""
    from rgb_checker import render_rgb
    light = dict(pos=np.zeros(3), dir=np.array([0, 1.0, 0]), amb=np.full(3, 0.1), dif=np.full(3, 0.7),
                 spe=np.zeros(3), att=np.array([1.0, 0, 0]), cosc=None, exponent=0.0, directional=True)
    box = [(6, [0.3, 0.3, 0.3], np.zeros(3), EYE)]
    r = render_rgb(CAM, 11, 11, box, [], GREY, [light], look=[0, 0, 0, 0, 0, 0, 0], quantise=False)
    hit = r["geom"] == 0
    assert hit.sum() > 9 and np.allclose(r["rgb"][hit], (0.1 + 0.7) * GREY[0, :3])
    assert np.allclose(r["depth"][hit], 4.7)


def test_checker_spot_cone():
    """a point outside a light's cone gets that light's ambient term only"""
    from rgb_checker import render_rgb
    look = [0, 0, 0, 0, 0, 0, 0]                       # headlight off
    plane = [(0, [0, 0, 0], np.zeros(3), EYE)]
    cam = np.array([0, 0, 5, 0, 0, -1, 0, 1, 0, 1, 0, 0, -0.4, 0.8 / 10, 0.4, 0.8 / 10, 10.0])
    light = dict(pos=np.array([0, 0, 1.0]), dir=np.array([0, 0, -1.0]), amb=np.full(3, 0.2), dif=np.full(3, 0.7),
                 spe=np.full(3, 0.3), att=np.array([1.0, 0, 0]), cosc=np.cos(np.radians(45)), exponent=10.0,
                 directional=False)
    r = render_rgb(cam, 11, 11, plane, [], GREY, [light], look=look, quantise=False)["rgb"]
    # pixel (5, 10): the point (2, 0, 0), 63 degrees off the light's axis -> ambient only
    assert np.allclose(r[5, 10], 0.2 * GREY[0, :3])
    # the point under the light: ambient + diffuse + specular (r.v = 1, spot = 1, no attenuation)
    assert np.allclose(r[5, 5], (0.2 + 0.7) * GREY[0, :3] + 0.3 * 0.5)


def test_checker_site_blend():
    from rgb_checker import render_rgb
    box = (6, [0.3, 0.3, 0.3], np.zeros(3), EYE)
    col = np.array([GREY[0], [0, 1, 0, 0.25, 0.0, 64.0, 1.0]])     # the site: emissive green, no highlight
    look = [0, 0, 0, 0, 0, 0, 0]                                   # no light at all: emission only
    base = render_rgb(CAM, 11, 11, [box], [], col[:1], [], look=look, quantise=False)
    front = render_rgb(CAM, 11, 11, [box], [(2, [0.2, 0, 0], np.array([0, -1.0, 0]), EYE)], col, [], look=look,
                       quantise=False)
    assert front["site"][5, 5] == 1 and front["geom"][5, 5] == 0
    assert np.allclose(front["rgb"][5, 5], 0.25 * np.array([0, 1.0, 0]) + 0.75 * base["rgb"][5, 5])
    assert np.array_equal(front["depth"], base["depth"])           # sites never write depth
    behind = render_rgb(CAM, 11, 11, [box], [(2, [0.2, 0, 0], np.array([0, 1.0, 0]), EYE)], col, [], look=look,
                        quantise=False)
    assert np.array_equal(behind["rgb"], base["rgb"]) and (behind["site"] == -1).all()
    # with lights: the same blend of the two shaded colours
    lit = render_rgb(CAM, 11, 11, [box], [(2, [0.2, 0, 0], np.array([0, -1.0, 0]), EYE)], col, [], quantise=False)
    lit0 = render_rgb(CAM, 11, 11, [box], [], col[:1], [], quantise=False)
    site = (0.1 + 0.4) * np.array([0, 1.0, 0]) + np.array([0, 1.0, 0])   # headlight on the site + emission
    assert np.allclose(lit["rgb"][5, 5], 0.25 * site + 0.75 * lit0["rgb"][5, 5])


def test_checker_supersample_half_covered():
    from rgb_checker import render_rgb
    look = [0.2, 0.4, 0.6, 0, 0, 0, 0]
    col = np.array([[1.0, 0, 0, 1, 0, 64.0, 1.0]])                 # emissive red
    # a plane patch x in [0, 1] seen from above: its edge x = 0 runs through the centre column
    cam = np.array([0, 0, 5, 0, 0, -1, 0, 1, 0, 1, 0, 0, -0.1, 0.2 / 10, 0.1, 0.2 / 10, 10.0])
    patch = [(0, [0.5, 0.5, 0], np.array([0.5, 0, 0]), EYE)]
    r1 = render_rgb(cam, 11, 11, patch, [], col, [], look=look, ss=1, quantise=False)["rgb"]
    r2 = render_rgb(cam, 11, 11, patch, [], col, [], look=look, ss=2, quantise=False)["rgb"]
    assert np.allclose(r2[5, 5], 0.5 * np.array([1.0, 0, 0]) + 0.5 * np.array(look[:3]))
    assert np.allclose(r2[5, 7], [1, 0, 0]) and np.allclose(r2[5, 3], look[:3]) and np.allclose(r1[5, 7], [1, 0, 0])


# ---------------------------------------------------------------------------------------
# scenes on the oracle
def _reference(m, orc, cam, W, H, q, v, p, ss=1, look=None):
    import rgb_checker
    orc.forward1(p if len(p) else None, q, v)
    geoms, sites, colors, lights = rgb_checker.oracle_scene(orc, m, p)
    return rgb_checker.render_rgb(cam, W, H, geoms, sites, colors, lights, look=look, ss=ss)


def _within(a, b):
    return np.abs(a.astype(int) - b.astype(int)).max(-1) <= TOL


def test_cap_calibration(oracle_lib):
    """What fp32 poses alone cost: the checker on the oracle's fp64 poses against the checker on
    the same poses rounded to fp32 with the camera origin moved 1e-6 m; pixels further apart than
    2/255 stay below 0.5 % (half of what the GPU tests allow), on scenes made like theirs -- every
    task, 6 random steps from a sampled reset."""
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
        for e in range(n):
            orc.forward1(st["params"][e], st["qpos"][e], st["qvel"][e])
            geoms, sites, colors, lights = rgb_checker.oracle_scene(orc, m, st["params"][e])
            a = rgb_checker.render_rgb(cam, W, H, geoms, sites, colors, lights)["rgb"]
            f32 = lambda es: [(t, s, np.float32(p).astype(np.float64), np.float32(x).astype(np.float64))
                              for t, s, p, x in es]
            b = rgb_checker.render_rgb(cam32, W, H, f32(geoms), f32(sites), colors, lights)["rgb"]
            bad = 1.0 - _within(a, b).mean()
            print(f"cap calibration {env_id} env {e}: {bad:.5f} of pixels differ by more than {TOL}/255")
            assert bad < 0.005, (env_id, e, bad)
            assert a.std() > 0 and (a.reshape(-1, 3) != 0).any()


# ---------------------------------------------------------------------------------------
# GPU
def _gpu():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _make_sim(env_id, n, variation=None, params=None, steps=6):
    """(model, oracle, sim) after a reset (explicit params or seed 3) and `steps` random steps"""
    torch = _gpu()
    from mj_envs_amd import _native
    m, orc = make_oracle(env_id, variation)
    sim = _native.Sim(m.to_blob(), n)
    obs = sim.empty(n, sim.obs_dim)
    if params is None:
        sim.reset(obs, seed=3)
    else:
        sim.reset(obs, params=torch.tensor(np.asarray(params), dtype=torch.float32, device=sim.torch_device))
    act = sim.empty(n, sim.nu)
    rew, done, goal = sim.empty(n), sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
    for k in range(steps):
        sim.random_actions(act, 7, k)
        sim.step(act, obs, rew, done, goal)
    return m, orc, sim


def _state(sim):
    torch = _gpu()
    qpos, qvel = sim.empty(sim.n_envs, sim.nq), sim.empty(sim.n_envs, sim.nv)
    params = sim.empty(sim.n_envs, max(sim.nparam, 1))
    sim.get_state(qpos, qvel, None, params if sim.nparam else None)
    torch.cuda.synchronize()
    return tuple(x.cpu().numpy().astype(np.float64) for x in (qpos, qvel, params[:, :sim.nparam]))


def _frames(sim, cam, W, H, ss=1, look=None, depth=False):
    torch = _gpu()
    out = sim.empty(sim.n_envs, H, W, 3, dtype=torch.uint8)
    out.fill_(77)
    z = sim.empty(sim.n_envs, H, W) if depth else None
    sim.render_rgb(out, cam, look=look, ss=ss, depth=z)
    torch.cuda.synchronize()
    return (out.cpu().numpy(), z.cpu().numpy()) if depth else out.cpu().numpy()


def _compare(m, orc, sim, cam, W, H, frames, envs, ss=1, look=None, what=""):
    Q, V, P = _state(sim)
    refs = {}
    for e in envs:
        ref = _reference(m, orc, cam, W, H, Q[e], V[e], P[e], ss=ss, look=look)
        ok = _within(frames[e], ref["rgb"])
        print(f"{what} env {e}: {ok.mean():.5f} of pixels within {TOL}/255, max diff "
              f"{np.abs(frames[e].astype(int) - ref['rgb'].astype(int)).max()}")
        assert ok.mean() >= 0.99, (what, e, ok.mean())
        refs[e] = ref
    return refs


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", ENVS)
def test_gpu_rgb_vs_checker(env_id):
    from mj_envs_amd.render import free_camera
    n, W, H = 4, 64, 64
    m, orc, sim = _make_sim(env_id, n)
    cam = free_camera(m, env_id, W, H)
    F = _frames(sim, cam, W, H)
    _compare(m, orc, sim, cam, W, H, F, range(n), what=env_id)
    for e in range(n):
        assert F[e].std() > 0 and (F[e].reshape(-1, 3) != 0).any(1).mean() > 0.5   # not constant, not all background


@pytest.mark.gpu
def test_gpu_rgbd():
    """one launch gives the colour frame and the depth frame aw_render_depth writes, bit for bit;
    where nothing opaque is hit and no site lies, the pixel is the background"""
    from mj_envs_amd.render import free_camera
    torch = _gpu()
    n, W, H = 4, 64, 64
    m, orc, sim = _make_sim("hammer-v0", n)
    look = np.array([0.2, 0.4, 0.6, 0.1, 0.4, 0.5, 1.0], np.float32)
    bg = np.floor(255 * look[:3].astype(np.float64) + 0.5).astype(np.uint8)
    for wide in (1.0, 8.0):        # the task's camera, and one 8x as wide that sees past the walls
        cam = free_camera(m, "hammer-v0", W, H)
        c, r = (W - 1) / 2.0, (H - 1) / 2.0
        cam[12], cam[14] = cam[12] + cam[13] * c * (1 - wide), cam[14] - cam[15] * r * (1 - wide)
        cam[13], cam[15] = cam[13] * wide, cam[15] * wide
        F, Z = _frames(sim, cam, W, H, look=look, depth=True)
        D = sim.empty(n, H, W)
        sim.render_depth(D, cam)
        torch.cuda.synchronize()
        assert np.array_equal(Z.view(np.uint32), D.cpu().numpy().view(np.uint32))
        refs = _compare(m, orc, sim, cam, W, H, F, range(n), look=look, what=f"rgbd x{wide:g}")
        for e in range(n):
            empty = (Z[e] == cam[16]) & (refs[e]["site"] < 0)
            assert (F[e][empty] == bg).all()
            if wide > 1:
                assert empty.mean() > 0.05


@pytest.mark.gpu
def test_gpu_relocate_goal_marker():
    """the target site (green, alpha 0.125) is where the env's params put it"""
    import rgb_checker
    from mj_envs_amd.render import free_camera
    W = H = 64
    m0 = load_task_model("relocate-v0")
    obj = m0.arrays["task_param_default"][:3]
    targets = np.array([[0.15, -0.1, 0.3], [-0.18, 0.15, 0.22]])
    params = np.concatenate([np.tile(obj, (2, 1)), targets], 1)
    m, orc, sim = _make_sim("relocate-v0", 2, params=params, steps=0)
    cam = free_camera(m, "relocate-v0", W, H)
    F = _frames(sim, cam, W, H)
    refs = _compare(m, orc, sim, cam, W, H, F, range(2), what="relocate goal")
    ng = int((m.geom_type != 7).sum())
    for e in range(2):
        f = F[e].astype(int)
        green = (f[..., 1] > f[..., 0] + 8) & (f[..., 1] > f[..., 2] + 8)
        rows, cols = np.nonzero(green)
        assert len(rows) > 20
        orc.forward1(params[e], *(_state(sim)[k][e] for k in (0, 1)))
        centre = orc.get("site_xpos").reshape(-1, 3)[m.name2id("site", "target")]
        pc, pr = rgb_checker.project(cam, centre)
        print(f"goal marker env {e}: blob centroid ({cols.mean():.2f}, {rows.mean():.2f}), projected ({pc:.2f}, {pr:.2f})")
        assert abs(cols.mean() - pc) <= 1.0 and abs(rows.mean() - pr) <= 1.0
    cover = (refs[0]["site"] == ng) | (refs[1]["site"] == ng)
    differ = (F[0] != F[1]).any(-1)
    assert differ[cover].mean() > 0.9 and not differ[~cover].any()


@pytest.mark.gpu
def test_gpu_hammer_mass_tint():
    """variation 'mass': the head's red channel is mass / 2.5 (hammer_v0.py:118)"""
    from mj_envs_amd.render import free_camera
    from mj_envs_amd.tasks import render_entry
    W = H = 64
    m0 = load_task_model("hammer-v0", "mass")
    params = np.tile(m0.arrays["task_param_default"], (2, 1))
    params[:, 3] = [0.25, 2.5]
    m, orc, sim = _make_sim("hammer-v0", 2, variation="mass", params=params, steps=0)
    cam = free_camera(m, "hammer-v0", W, H)
    F = _frames(sim, cam, W, H)
    refs = _compare(m, orc, sim, cam, W, H, F, range(2), what="hammer mass")
    head = render_entry(m, m.name2id("geom", "head"))
    mk = (refs[0]["geom"] == head) & (refs[1]["geom"] == head)
    assert mk.sum() >= 4
    for e in range(2):
        assert _within(F[e][mk], refs[e]["rgb"][mk]).mean() >= 0.99
    got = F[1][mk][:, 0].mean() - F[0][mk][:, 0].mean()
    want = refs[1]["rgb"][mk][:, 0].astype(float).mean() - refs[0]["rgb"][mk][:, 0].astype(float).mean()
    print(f"hammer mass tint: head pixels {mk.sum()}, red difference {got:.2f} (checker {want:.2f})")
    assert want > 0 and got >= 0.5 * want


@pytest.mark.gpu
@pytest.mark.parametrize("n,W,H,envs", [(3, 7, 5, (0, 1, 2)), (3, 40, 25, (0, 1, 2)), (130, 64, 64, (0, 64, 129))])
def test_gpu_rgb_shapes(n, W, H, envs):
    """7x5: byte stores, one partial span; 40x25: dword stores, partial last span; 130 envs"""
    from mj_envs_amd.render import free_camera
    m, orc, sim = _make_sim("hammer-v0", n)
    cam = free_camera(m, "hammer-v0", W, H)
    F = _frames(sim, cam, W, H)
    _compare(m, orc, sim, cam, W, H, F, envs, what=f"shape {n}x{H}x{W}")


@pytest.mark.gpu
def test_gpu_rgb_supersampling():
    from mj_envs_amd.render import free_camera
    m, orc, sim = _make_sim("hammer-v0", 2)
    F2 = _frames(sim, free_camera(m, "hammer-v0", 64, 64), 64, 64, ss=2).astype(np.float64)
    F1 = _frames(sim, free_camera(m, "hammer-v0", 128, 128), 128, 128).astype(np.float64)
    mean = F1.reshape(2, 64, 2, 64, 2, 3).mean((2, 4))
    print(f"supersampling: max |ss2 - block mean| = {np.abs(F2 - mean).max():.3f}")
    assert np.abs(F2 - mean).max() <= 1.0


@pytest.mark.gpu
def test_gpu_rgb_api():
    torch = _gpu()
    from mj_envs_amd import _native
    from mj_envs_amd.envs import AdroitVecEnv, Box, HammerEnvV0
    from mj_envs_amd.render import free_camera
    from mj_envs_amd.wrappers import PixelObservationVecEnv
    n = 3
    env = AdroitVecEnv("hammer-v0", n)
    w = PixelObservationVecEnv(env, render_kwargs={"mode": "rgb", "ss": 2})
    assert isinstance(w.pixel_space, Box) and w.pixel_space.shape == (64, 64, 3) and w.pixel_space.high.max() == 255
    px, _ = w.reset()
    assert tuple(px.shape) == (n, 64, 64, 3) and px.dtype == torch.float32
    assert float(px.min()) >= 0 and float(px.max()) <= 255 and float(px.std()) > 0
    state0 = w.get_state().clone()
    assert tuple(state0.shape) == (n, env.obs_dim) and torch.equal(state0, env.obs)
    before = px.clone()
    act = torch.ones(n, env.nu, device=env.sim.torch_device)
    for _ in range(3):
        px2 = w.step(act)[0]
    assert not torch.equal(px2, before)
    # the default wrapper is unchanged: depth pixels
    wd = PixelObservationVecEnv(AdroitVecEnv("hammer-v0", 2))
    assert tuple(wd.reset()[0].shape) == (2, 1, 64, 64) and wd.pixel_space.shape == (1, 64, 64)
    # facade
    fac = HammerEnvV0()
    assert fac.render().shape == (64, 64)
    f = fac.render(mode="rgb", enable_resize=False)
    assert f.shape == (128, 128, 3) and f.dtype == np.float64 and 0 <= f.min() and f.max() <= 255
    assert fac.render(mode="rgb").shape == (64, 64, 3)
    # C-ABI argument checks
    sim = env.sim
    cam = free_camera(env.model, "hammer-v0")
    out = sim.empty(n, 64, 64, 3, dtype=torch.uint8)
    with pytest.raises(_native.NativeError, match="error -1"):
        sim.render_rgb(out, cam, ss=3)
    with pytest.raises(_native.NativeError, match="error -1"):
        sim.render_rgb(out, cam, ss=2, depth=sim.empty(n, 64, 64))
    # a model table without the appearance arrays (an older file): everything but colour works
    m = load_task_model("hammer-v0")
    for k in APPEARANCE:
        del m.arrays[k]
    old = _native.Sim(m.to_blob(), 2)
    obs = old.empty(2, old.obs_dim)
    old.reset(obs, seed=1)
    a = old.empty(2, old.nu).zero_()
    old.step(a, obs, old.empty(2), old.empty(2, dtype=torch.uint8), old.empty(2, dtype=torch.uint8))
    d = old.empty(2, 64, 64)
    old.render_depth(d, cam)
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all() and torch.isfinite(d).all()
    with pytest.raises(_native.NativeError, match="error -5"):
        old.render_rgb(old.empty(2, 64, 64, 3, dtype=torch.uint8), cam)
