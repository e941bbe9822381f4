"""Cameras: the models' own <camera>s, cameras mounted on a body, per-env records and several views
per launch (aw_render_views, k_views).

CPU: the camera table of the compiled models, the record constructors of mj_envs_amd/render.py,
and what fp32 poses and an fp32-composed camera alone cost against the fp64 checker (the
calibration of the GPU caps, as test_render_rgb.test_cap_calibration does for the free camera).
GPU: aw_render_views bit for bit against aw_render_rgb / aw_render_depth where they overlap, view
against view, and against the fp64 checker (tests/rgb_checker.py) on the oracle's kinematics with
the project's caps: colour >= 99 % of pixels within 2/255 per channel, depth >= 99.5 % within 2e-3 m.
"""
import numpy as np
import pytest

from conftest import ENVS, load_task_model, make_oracle
from test_render_rgb import APPEARANCE, TOL, _gpu, _make_sim, _state, _within

DEPTH_TOL = 2e-3
# the eye-in-hand mount used throughout: on the palm, 15 cm behind it, looking along the fingers
WRIST = dict(body="palm", pos=(0.0, -0.15, 0.0), forward=(0.0, 0.6, 0.8), up=(0.0, -0.8, 0.6), fovy=90.0)
GUARD = 4096


def _wrist(m, W, H):
    from mj_envs_amd.render import mounted_camera
    return mounted_camera(m, WRIST["body"], WRIST["pos"], WRIST["forward"], WRIST["up"], W, H, WRIST["fovy"])


def _axes(rec):
    return np.asarray(rec, np.float64)[3:12].reshape(3, 3)      # forward, up, right


def _orthonormal(rec, tol=1e-6):
    a = _axes(rec)
    return np.allclose(a @ a.T, np.eye(3), atol=tol) and np.allclose(np.cross(a[0], a[1]), a[2], atol=tol)


# ---------------------------------------------------------------------------------------
# CPU: the camera table
def test_camera_table():
    from mj_envs_amd.mjcf import euler2quat_mj
    from mj_envs_amd.tasks import load_model
    q45 = np.array([0.92388, 0.382683, 0, 0])
    q45 = q45 / np.linalg.norm(q45)
    for env_id in ENVS:
        m = load_model(env_id)
        c = m.cameras
        want = ["fixed", "vil_camera"] + ([f"view_{k}" for k in range(1, 6)] if env_id == "pen-v0" else [])
        assert c["names"] == want, env_id
        n = len(want)
        assert c["cam_pos"].shape == (n, 3) and c["cam_quat"].shape == (n, 4) and c["cam_fovy"].shape == (n,)
        assert np.allclose(c["cam_pos"][0], [0, -0.7, 0.7]) and np.allclose(c["cam_pos"][1], [0, -1.2, 1.2])
        for k in (0, 1):
            assert np.allclose(c["cam_quat"][k], q45, atol=1e-12) and c["cam_fovy"][k] == 45.0
        assert np.allclose(np.linalg.norm(c["cam_quat"], axis=1), 1.0)
        # the table is host side only; the arrays the blob carries are what they were
        assert not any(k in m.arrays for k in ("cam_quat", "cam_fovy", "cam_names", "cameras"))
        assert np.array_equal(m.cam_pos, c["cam_pos"]) and np.array_equal(m.cam_bodyid, c["cam_bodyid"])
        assert (m.cam_bodyid == 0).all() and m.cam_pos.shape == (n, 3)
        # the task model (a copy) keeps the table
        assert load_task_model(env_id).cameras["names"] == want
    # pen's view_1: euler under the model's compiler settings (radians, eulerseq xyz)
    pen = load_model("pen-v0")
    i = pen.camera_id("view_1")
    assert np.allclose(pen.cameras["cam_pos"][i], [-0.8, -0.8, 0.8])
    assert np.allclose(pen.cameras["cam_quat"][i], euler2quat_mj([0.785, -0.785, -0.785], "xyz"), atol=1e-12)
    with pytest.raises(KeyError, match="view_9"):
        pen.camera_id("view_9")


def test_camera_table_absent():
    """a model loaded without its camera file: named lookups say so, everything else works"""
    from mj_envs_amd.mjcf import Model
    from mj_envs_amd.render import free_camera, model_camera, mounted_camera
    from mj_envs_amd.tasks import MODEL_DIR, TASKS, load_model
    import os
    m = Model.load_npz(os.path.join(MODEL_DIR, TASKS["hammer-v0"].xml.replace(".xml", ".npz")))
    assert m.cameras is None
    with pytest.raises(KeyError, match="camera table"):
        model_camera(m, "fixed", 64, 64)
    assert np.array_equal(free_camera(m, "hammer-v0"), free_camera(load_model("hammer-v0"), "hammer-v0"))
    assert mounted_camera(m, "palm", (0, 0, 0), (0, 1, 0), (0, 0, 1))[1] == m.name2id("body", "palm")
    assert m.to_blob() == Model.load_npz(os.path.join(MODEL_DIR, "DAPG_hammer.npz")).to_blob()


def test_orientation_forms(tmp_path):
    """<camera> orientation goes through the compiler's _orient: quat, euler, axisangle, xyaxes, zaxis;
    fovy defaults to 45; a mode other than fixed is refused"""
    from mj_envs_amd.mjcf import _Compiler, quat2mat
    xml = """<mujoco><compiler angle="radian"/><worldbody>
      <camera name="a" pos="1 2 3" xyaxes="0 1 0 -1 0.5 0"/>
      <camera name="b" zaxis="0 1 1" fovy="60"/>
      <camera name="c" axisangle="0 0 1 1.5707963267948966"/>
      <camera name="d"/>
      <body name="arm" pos="0 0 1"><camera name="e" quat="0 0 0 2" mode="fixed"/></body>
    </worldbody></mujoco>"""
    p = tmp_path / "cams.xml"
    p.write_text(xml)
    c = _Compiler(str(p))
    cams = c.bodies[0]["cameras"] + c.bodies[1]["cameras"]
    assert [k["name"] for k in cams] == list("abcde")
    R = quat2mat(cams[0]["quat"])
    assert np.allclose(R[:, 0], [0, 1, 0]) and np.allclose(R[:, 1], [-1, 0, 0]) and np.allclose(R[:, 2], [0, 0, 1])
    assert np.allclose(quat2mat(cams[1]["quat"])[:, 2], np.array([0, 1, 1]) / np.sqrt(2)) and cams[1]["fovy"] == 60.0
    assert np.allclose(quat2mat(cams[2]["quat"])[:, 0], [0, 1, 0])
    assert np.allclose(cams[3]["quat"], [1, 0, 0, 0]) and cams[3]["fovy"] == 45.0 and np.allclose(cams[0]["pos"], [1, 2, 3])
    assert np.allclose(cams[4]["quat"], [0, 0, 0, 1])
    p.write_text(xml.replace('mode="fixed"', 'mode="trackcom"'))
    with pytest.raises(NotImplementedError, match="trackcom"):
        _Compiler(str(p))


# ---------------------------------------------------------------------------------------
# CPU: records
def _ray(rec, col, row):
    rec = np.asarray(rec, np.float64)
    d = rec[3:6] + (rec[12] + rec[13] * col) * rec[9:12] + (rec[14] - rec[15] * row) * rec[6:9]
    return d / np.linalg.norm(d)


def test_pinhole_record():
    from mj_envs_amd.mjcf import quat2mat
    from mj_envs_amd.render import ZFAR, model_camera, pinhole_record
    from mj_envs_amd.tasks import load_model
    rng = np.random.default_rng(0)
    for W, H, fovy in ((64, 64, 45.0), (40, 25, 90.0), (7, 5, 30.0)):
        q = rng.normal(size=4)
        R = quat2mat(q / np.linalg.norm(q))
        pos = rng.normal(size=3)
        rec = pinhole_record(pos, R, W, H, fovy)
        assert rec.dtype == np.float32 and rec.shape == (17,) and rec[16] == ZFAR
        assert np.allclose(rec[:3], pos, atol=1e-6) and _orthonormal(rec)
        # MuJoCo's fixed camera: looks along -z, up +y, right +x
        assert np.allclose(_axes(rec), [-R[:, 2], R[:, 1], R[:, 0]], atol=1e-6)
        # the frame centre (between pixel centres: col (W-1)/2, row (H-1)/2) is the optical axis
        assert np.allclose(_ray(rec, (W - 1) / 2, (H - 1) / 2), rec[3:6], atol=1e-6)
        # frame edges (half a pixel outside the outer pixel centres): fovy top to bottom, W/H across
        top, bot = _ray(rec, (W - 1) / 2, -0.5), _ray(rec, (W - 1) / 2, H - 0.5)
        assert np.isclose(np.degrees(np.arccos(np.clip(top @ bot, -1, 1))), fovy, atol=1e-4)
        lft, rgt = _ray(rec, -0.5, (H - 1) / 2), _ray(rec, W - 0.5, (H - 1) / 2)
        tx = np.tan(np.arccos(np.clip(lft @ rgt, -1, 1)) / 2)
        assert np.isclose(tx / np.tan(np.radians(fovy) / 2), W / H, rtol=1e-5)
        assert top @ rec[6:9] > 0 and rgt @ rec[9:12] > 0      # row 0 is the top, col 0 the left
    m = load_model("hammer-v0")
    rec, body = model_camera(m, "fixed", 64, 64)
    assert body == 0 and np.allclose(rec[:3], [0, -0.7, 0.7])
    assert np.allclose(rec[3:6], [0, np.sin(np.pi / 4), -np.cos(np.pi / 4)], atol=1e-5)
    assert np.allclose(rec[9:12], [1, 0, 0], atol=1e-6)
    assert model_camera(m, "vil_camera", 32, 32)[0][13] == pytest.approx(2 * np.tan(np.radians(22.5)) / 32)


def test_mounted_and_jitter():
    from mj_envs_amd.render import compose_record, jitter_cameras, model_camera, mounted_camera
    from mj_envs_amd.tasks import load_model
    m = load_model("hammer-v0")
    rec, body = _wrist(m, 64, 64)
    assert body == m.name2id("body", "palm") and _orthonormal(rec)
    assert np.allclose(rec[:3], WRIST["pos"]) and np.allclose(rec[3:6], WRIST["forward"], atol=1e-6)
    assert np.allclose(rec[6:9], WRIST["up"], atol=1e-6) and rec[13] == pytest.approx(2.0 / 64)
    # up is orthogonalised against forward
    skew, _ = mounted_camera(m, 0, (0, 0, 1), (1, 0, 0), (0.3, 0, 1), 32, 32, 60.0)
    assert _orthonormal(skew) and np.allclose(skew[6:9], [0, 0, 1], atol=1e-6)
    with pytest.raises(ValueError):
        mounted_camera(m, 0, (0, 0, 1), (1, 0, 0), (2, 0, 0))
    # composing keeps the frame orthonormal and the pixel map
    q = np.array([0.5, -0.5, 0.5, 0.5])
    w = compose_record(rec, [0.1, 0.2, 0.3], q)
    assert _orthonormal(w) and np.array_equal(w[12:], rec[12:].astype(np.float64))
    base = model_camera(m, "vil_camera", 64, 64)[0]
    same = jitter_cameras(base, 5, np.random.default_rng(1), 0.0, 0.0, (1.0, 1.0))
    assert same.dtype == np.float32 and same.shape == (5, 17) and (same == base[None]).all()
    J = jitter_cameras(base, 16, np.random.default_rng(1), 0.02, 3.0, (0.9, 1.1))
    assert J.shape == (16, 17) and J.dtype == np.float32
    ratios = []
    for r in J:
        assert _orthonormal(r, 1e-5)
        s = r[12:16].astype(np.float64) / base[12:16]
        assert np.allclose(s, s[0], rtol=1e-6) and 0.9 - 1e-6 <= s[0] <= 1.1 + 1e-6 and r[16] == base[16]
        ratios.append(s[0])
        assert np.degrees(np.arccos(np.clip(r[3:6] @ base[3:6], -1, 1))) < 5 * 3.0
    assert np.std(ratios) > 0 and 0 < np.abs(J[:, :3] - base[:3]).max() < 5 * 0.02
    assert len({tuple(r) for r in J}) == 16


# ---------------------------------------------------------------------------------------
# scenes on the oracle
def _world_record(orc, m, view):
    """fp64 world record of a (record, body) view from the oracle's body frames (after forward1)"""
    from mj_envs_amd.render import compose_record
    rec, body = view
    if body == 0:
        return np.asarray(rec, np.float64)
    return compose_record(rec, orc.get("xpos").reshape(-1, 3)[body], orc.get("xquat").reshape(-1, 4)[body])


def _compose32(rec, xpos, xquat):
    """the kernel's composition (aw_render.h compose_view) in fp32 from fp32-rounded body frames"""
    f = np.float32
    rec, p, q = np.asarray(rec, f), np.asarray(xpos).astype(f), np.asarray(xquat).astype(f)
    out = rec.copy()
    u = q[1:]
    for k in range(4):
        v = rec[3 * k:3 * k + 3]
        t = (np.cross(u, v).astype(f) * f(2)).astype(f)
        r = (v + q[0] * t).astype(f) + np.cross(u, t).astype(f)
        out[3 * k:3 * k + 3] = (r + p).astype(f) if k == 0 else r
    return out.astype(np.float64)


def _check_frame(rgb, depth, ref, what):
    """the project's caps against a checker frame; prints each figure before it asserts"""
    ok = _within(rgb, ref["rgb"]).mean()
    zok = (np.abs(depth.astype(np.float64) - ref["depth"]) <= DEPTH_TOL).mean()
    print(f"{what}: colour {ok:.5f} within {TOL}/255, depth {zok:.5f} within {DEPTH_TOL} m")
    assert ok >= 0.99, (what, ok)
    assert zok >= 0.995, (what, zok)


def test_view_calibration(oracle_lib):
    """What fp32 alone costs on the new cameras: the checker on the oracle's fp64 poses with an
    fp64-composed camera against the checker on the poses rounded to fp32 with the camera composed
    in fp32 from the fp32-rounded body frames.  Colour pixels further apart than 2/255 stay below
    0.5 %, depth pixels further apart than 2e-3 m below 0.25 % -- half of what the GPU tests allow.
    The wrist mount sits outside every geom and sees a scene: >= 20 distinct geoms, >= 58 % of the
    pixels hit something."""
    import rgb_checker
    from mj_envs_amd.render import model_camera
    from mj_envs_amd.tasks import sample_params
    W = H = 64
    f32 = lambda es: [(t, s, np.float32(p).astype(np.float64), np.float32(x).astype(np.float64)) for t, s, p, x in es]
    for env_id in ENVS:
        m, orc = make_oracle(env_id)
        rng = np.random.default_rng(5)
        n = 2
        st, _ = orc.reset(sample_params(env_id, m, rng, n))
        for _ in range(6):
            orc.step(st, rng.uniform(-1, 1, (n, orc.nu)))
        views = {"fixed": model_camera(m, "fixed", W, H), "wrist": _wrist(m, W, H)}
        if env_id == "pen-v0":
            views["view_1"] = model_camera(m, "view_1", W, H)
        for e in range(n):
            orc.forward1(st["params"][e], st["qpos"][e], st["qvel"][e])
            geoms, sites, colors, lights = rgb_checker.oracle_scene(orc, m, st["params"][e])
            xpos, xquat = orc.get("xpos").reshape(-1, 3), orc.get("xquat").reshape(-1, 4)
            for name, (rec, body) in views.items():
                cam = _world_record(orc, m, (rec, body))
                cam32 = _compose32(rec, xpos[body], xquat[body]) if body else np.asarray(rec, np.float64)
                a = rgb_checker.render_rgb(cam, W, H, geoms, sites, colors, lights)
                b = rgb_checker.render_rgb(cam32, W, H, f32(geoms), f32(sites), colors, lights)
                bad = 1.0 - _within(a["rgb"], b["rgb"]).mean()
                zbad = (np.abs(a["depth"] - b["depth"]) > DEPTH_TOL).mean()
                print(f"view calibration {env_id} env {e} {name}: colour {bad:.5f}, depth {zbad:.5f} of pixels apart")
                assert bad < 0.005, (env_id, e, name, bad)
                assert zbad < 0.0025, (env_id, e, name, zbad)
                assert a["rgb"].std() > 0
                if name == "wrist":
                    seen = np.unique(a["geom"][a["geom"] >= 0])
                    near = a["depth"][a["geom"] >= 0].min()
                    print(f"  wrist: {len(seen)} geoms, {(a['geom'] >= 0).mean():.3f} of pixels hit, nearest {near:.3f} m")
                    assert len(seen) >= 20 and (a["geom"] >= 0).mean() >= 0.58 and near > 0.05


# ---------------------------------------------------------------------------------------
# GPU
def _guarded(torch, sim, shape, dtype, fill):
    """a tensor of `shape` inside one allocation with GUARD bytes before and after it, all filled
    with a sentinel -> (view, whole allocation as bytes)"""
    item = torch.empty(0, dtype=dtype).element_size()
    nbytes = int(np.prod(shape)) * item
    raw = torch.full((GUARD + nbytes + GUARD,), fill, dtype=torch.uint8, device=sim.torch_device)
    return raw[GUARD:GUARD + nbytes].view(dtype).view(*shape), raw


def _guards_ok(raw, fill):
    return bool((raw[:GUARD] == fill).all()) and bool((raw[-GUARD:] == fill).all())


def _views(sim, views, W, H, rgb=True, depth=True, env_cam=None, ss=1, look=None):
    """one aw_render_views launch into sentinel-filled, guarded outputs -> (rgb, depth) numpy"""
    torch = _gpu()
    n, nv = sim.n_envs, len(views)
    F = Z = fraw = zraw = None
    if rgb:
        F, fraw = _guarded(torch, sim, (n, nv, H, W, 3), torch.uint8, 77)
    if depth:
        Z, zraw = _guarded(torch, sim, (n, nv, H, W), torch.float32, 0xA5)
    ec = None if env_cam is None else torch.tensor(np.asarray(env_cam, np.float32), device=sim.torch_device).contiguous()
    sim.render_views(views, W, H, rgb=F, depth=Z, env_cam=ec, look=look, ss=ss)
    torch.cuda.synchronize()
    assert fraw is None or _guards_ok(fraw, 77), "bytes written outside the rgb frames"
    assert zraw is None or _guards_ok(zraw, 0xA5), "bytes written outside the depth frames"
    return (None if F is None else F.cpu().numpy()), (None if Z is None else Z.cpu().numpy())


def _bits(z):
    return np.ascontiguousarray(z).view(np.uint32)


def _references(m, orc, sim, views, W, H, envs, env_cam=None):
    """{(env, view): checker frame} on the oracle's fp64 kinematics of the sim's state, every view's
    world record composed in fp64"""
    import rgb_checker
    Q, V, P = _state(sim)
    out = {}
    for e in envs:
        orc.forward1(P[e] if len(P[e]) else None, Q[e], V[e])
        geoms, sites, colors, lights = rgb_checker.oracle_scene(orc, m, P[e])
        for v, (rec, body) in enumerate(views):
            r = rec if env_cam is None else env_cam[e][v]
            out[e, v] = rgb_checker.render_rgb(_world_record(orc, m, (r, body)), W, H, geoms, sites, colors, lights)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(64, 64), (7, 5)])
def test_gpu_views_bitwise_existing(W, H):
    """one world-frame view is aw_render_rgb's / aw_render_depth's frame, bit for bit"""
    from mj_envs_amd.render import free_camera
    torch = _gpu()
    n = 3
    m, orc, sim = _make_sim("hammer-v0", n)
    cam = free_camera(m, "hammer-v0", W, H)
    rgb0 = sim.empty(n, H, W, 3, dtype=torch.uint8).fill_(1)
    z0, d0 = sim.empty(n, H, W).fill_(-1), sim.empty(n, H, W).fill_(-1)
    sim.render_rgb(rgb0, cam, depth=z0)
    sim.render_depth(d0, cam)
    rgb2 = sim.empty(n, H, W, 3, dtype=torch.uint8).fill_(1)
    sim.render_rgb(rgb2, cam, ss=2)
    torch.cuda.synchronize()
    F, Z = _views(sim, [(cam, 0)], W, H)
    assert np.array_equal(F[:, 0], rgb0.cpu().numpy()) and np.array_equal(_bits(Z[:, 0]), _bits(z0.cpu().numpy()))
    _, D = _views(sim, [(cam, 0)], W, H, rgb=False)
    assert np.array_equal(_bits(D[:, 0]), _bits(d0.cpu().numpy()))
    F2, _ = _views(sim, [(cam, 0)], W, H, depth=False, ss=2)
    assert np.array_equal(F2[:, 0], rgb2.cpu().numpy())
    assert F.std() > 0 and (W < 64 or (F2 != F).any())


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", ["hammer-v0", "pen-v0"])
def test_gpu_views_independent(env_id):
    """each view of a three-view launch is the single-view launch of its camera, bit for bit"""
    from mj_envs_amd.render import free_camera, model_camera
    W = H = 64
    m, orc, sim = _make_sim(env_id, 3)
    views = [(free_camera(m, env_id, W, H), 0), model_camera(m, "vil_camera", W, H), _wrist(m, W, H)]
    F, Z = _views(sim, views, W, H)
    _, D = _views(sim, views, W, H, rgb=False)
    assert np.array_equal(_bits(D), _bits(Z))
    for v, view in enumerate(views):
        f, z = _views(sim, [view], W, H)
        assert np.array_equal(F[:, v], f[:, 0]) and np.array_equal(_bits(Z[:, v]), _bits(z[:, 0])), v
        assert F[:, v].std() > 0
    assert (F[:, 0] != F[:, 1]).any() and (F[:, 1] != F[:, 2]).any()


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", ENVS)
def test_gpu_views_vs_checker(env_id):
    """a model camera and the eye-in-hand mount against the fp64 checker, the wrist record composed
    in fp64 from the oracle's palm frame"""
    from mj_envs_amd.render import model_camera
    n, W, H = 4, 64, 64
    m, orc, sim = _make_sim(env_id, n)
    views = [model_camera(m, "fixed", W, H), _wrist(m, W, H)]
    F, Z = _views(sim, views, W, H)
    refs = _references(m, orc, sim, views, W, H, range(n))
    for e in range(n):
        for v, name in enumerate(("fixed", "wrist")):
            _check_frame(F[e, v], Z[e, v], refs[e, v], f"{env_id} env {e} {name}")
            assert F[e, v].std() > 0 and (Z[e, v] < 10.0).any()        # not constant
    Q = _state(sim)[0]
    assert not np.array_equal(Q[0], Q[1]) and (F[0, 1] != F[1, 1]).any()      # the wrist view follows the hand


@pytest.mark.gpu
@pytest.mark.parametrize("mount", ["vil_camera", "palm"])
def test_gpu_views_per_env(mount):
    """env e renders from env_cam[e]: its frame is env e's frame of a launch whose shared record is
    record e, bit for bit; one env also against the checker"""
    from mj_envs_amd.render import jitter_cameras, model_camera
    n, W, H = 4, 64, 64
    m, orc, sim = _make_sim("hammer-v0", n)
    rec, body = model_camera(m, "vil_camera", W, H) if mount == "vil_camera" else _wrist(m, W, H)
    J = jitter_cameras(rec, n, np.random.default_rng(11), 0.02, 3.0, (0.9, 1.1))
    assert len({tuple(r) for r in J}) == n
    F, Z = _views(sim, [(rec, body)], W, H, env_cam=J[:, None])
    for e in range(n):
        f, z = _views(sim, [(J[e], body)], W, H)
        assert np.array_equal(F[e, 0], f[e, 0]) and np.array_equal(_bits(Z[e, 0]), _bits(z[e, 0])), e
    f, _ = _views(sim, [(rec, body)], W, H)
    assert (F != f).any()
    ref = _references(m, orc, sim, [(rec, body)], W, H, [2], env_cam=J[:, None])
    _check_frame(F[2, 0], Z[2, 0], ref[2, 0], f"per-env {mount} env 2")


@pytest.mark.gpu
def test_gpu_views_unvalidated_records():
    """a per-env record is not validated: no address in the kernel depends on it (pixel indices come
    from the lane), so NaN, infinite or huge records cost only their own env's frames -- every pixel
    of those is still written, the other envs' frames are what they are without them, and nothing
    lands outside the outputs (the guards of _views)"""
    from mj_envs_amd.render import model_camera
    n, W, H = 4, 40, 25
    m, orc, sim = _make_sim("hammer-v0", n)
    views = [model_camera(m, "vil_camera", W, H), _wrist(m, W, H)]
    ec = np.stack([np.stack([r for r, _ in views])] * n).astype(np.float32)
    ec[1] = np.nan
    ec[2, 0, :3], ec[2, 0, 12:16] = np.inf, 1e30
    ec[2, 1, 3:12], ec[2, 1, 16] = -1e30, np.nan
    F, Z = _views(sim, views, W, H, env_cam=ec)
    f, z = _views(sim, views, W, H)
    for e in (0, 3):
        assert np.array_equal(F[e], f[e]) and np.array_equal(_bits(Z[e]), _bits(z[e]))
    assert (_bits(Z) != 0xA5A5A5A5).all()        # the sentinel is gone from every depth pixel


@pytest.mark.gpu
@pytest.mark.parametrize("n,V,W,H,envs", [(3, 2, 7, 5, ()), (3, 3, 40, 25, (0, 1, 2)), (130, 2, 64, 64, (0, 64, 129))])
def test_gpu_views_shapes(n, V, W, H, envs):
    """7x5 x 2 views: byte stores, view 1 of env 0 starts at byte 105; 40x25 x 3: dword stores with a
    partial last span; 130 envs.  Every view equals its single-view launch (another frame offset)
    bit for bit; against the checker where a frame has enough pixels for the 99 % cap to allow one
    (a 7x5 frame has 35)."""
    from mj_envs_amd.render import free_camera, model_camera
    m, orc, sim = _make_sim("hammer-v0", n)
    views = [model_camera(m, "fixed", W, H), _wrist(m, W, H), (free_camera(m, "hammer-v0", W, H), 0)][:V]
    F, Z = _views(sim, views, W, H)
    assert F.shape == (n, V, H, W, 3) and Z.shape == (n, V, H, W)
    for v, view in enumerate(views):
        f, z = _views(sim, [view], W, H)
        assert np.array_equal(F[:, v], f[:, 0]) and np.array_equal(_bits(Z[:, v]), _bits(z[:, 0])), v
        assert F[:, v].std() > 0
    refs = _references(m, orc, sim, views, W, H, envs)
    for (e, v), ref in refs.items():
        _check_frame(F[e, v], Z[e, v], ref, f"shape {n}x{V}x{H}x{W} env {e} view {v}")


@pytest.mark.gpu
def test_gpu_views_errors():
    from mj_envs_amd import _native
    from mj_envs_amd.render import free_camera
    torch = _gpu()
    n, W, H = 2, 16, 16
    m, orc, sim = _make_sim("hammer-v0", n, steps=0)
    cam = free_camera(m, "hammer-v0", W, H)
    rgb = lambda v=1, w=W, h=H: sim.empty(n, v, h, w, 3, dtype=torch.uint8)
    dep = lambda v=1, w=W, h=H: sim.empty(n, v, h, w)
    einval = lambda: pytest.raises(_native.NativeError, match="error -1")
    with einval():
        sim.render_views([], W, H, rgb=rgb(0))                                   # nviews 0
    with einval():
        sim.render_views([(cam, 0)] * 5, W, H, rgb=rgb(5))                        # nviews > AW_MAX_VIEWS
    for body in (-1, sim.nbody):
        with einval():
            sim.render_views([(cam, body)], W, H, rgb=rgb())
    with einval():
        sim.render_views([(cam, 0)], W, H)                                       # both outputs NULL
    for ss in (0, 3):
        with einval():
            sim.render_views([(cam, 0)], W, H, rgb=rgb(), ss=ss)
    with einval():
        sim.render_views([(cam, 0)], W, H, rgb=rgb(), depth=dep(), ss=2)          # depth with ss 2
    with einval():
        sim.render_views([(cam, 0)], W, H, depth=dep(), ss=2)                     # no rgb with ss 2
    for w, h in ((1025, 1), (1, 1025), (0, 4), (4, 0)):
        with einval():
            sim.render_views([(cam, 0)], w, h, rgb=rgb(1, max(w, 1), max(h, 1))[:, :, :h, :w].contiguous())
    sim.render_views([(cam, 0)] * 4, W, H, rgb=rgb(4), depth=dep(4))             # the limits themselves pass
    sim.render_views([(cam, sim.nbody - 1)], W, H, depth=dep())
    # a model table without the appearance arrays: depth-only works, colour is unsupported
    m0 = load_task_model("hammer-v0")
    for k in APPEARANCE:
        del m0.arrays[k]
    old = _native.Sim(m0.to_blob(), n)
    old.reset(old.empty(n, old.obs_dim), seed=3)
    view = _wrist(m, W, H)
    d, want = old.empty(n, 1, H, W).fill_(-1), dep().fill_(-2)
    old.render_views([view], W, H, depth=d)
    sim.reset(sim.empty(n, sim.obs_dim), seed=3)
    sim.render_views([view], W, H, depth=want)
    torch.cuda.synchronize()
    assert torch.equal(d, want) and float(d.min()) > 0
    with pytest.raises(_native.NativeError, match="error -5"):
        old.render_views([view], W, H, rgb=old.empty(n, 1, H, W, 3, dtype=torch.uint8))


@pytest.mark.gpu
def test_gpu_views_python_surface():
    torch = _gpu()
    from mj_envs_amd.envs import AdroitVecEnv, HammerEnvV0
    from mj_envs_amd.render import jitter_cameras, model_camera
    from mj_envs_amd.wrappers import PixelObservationVecEnv, make_env
    n = 3
    env = AdroitVecEnv("hammer-v0", n)
    env.reset()
    wrist = _wrist(env.model, 64, 64)
    F = env.render_views(["free", "vil_camera", wrist])
    assert tuple(F.shape) == (n, 3, 64, 64, 3) and F.dtype == torch.uint8
    F2, Z2 = env.render_views(["fixed", wrist], 32, 24, depth=True)
    assert tuple(F2.shape) == (n, 2, 24, 32, 3) and tuple(Z2.shape) == (n, 2, 24, 32) and Z2.dtype == torch.float32
    Z = env.render_views(["fixed"], rgb=False, depth=True)
    assert tuple(Z.shape) == (n, 1, 64, 64) and Z.dtype == torch.float32
    # render_rgb / render_depth: without `camera` today's entry points, today's frames
    direct = env.sim.empty(n, 64, 64, 3, dtype=torch.uint8)
    env.sim.render_rgb(direct, env.mj_viewer_headless_setup(64, 64))
    assert torch.equal(env.render_rgb(), direct) and torch.equal(F[:, 0], direct)
    assert torch.equal(env.render_rgb(camera="vil_camera"), F[:, 1]) and torch.equal(env.render_rgb(camera=wrist), F[:, 2])
    assert torch.equal(env.render_depth(camera="fixed"), Z[:, 0])
    ec = torch.tensor(jitter_cameras(model_camera(env.model, "vil_camera")[0], n, np.random.default_rng(0), 0.02, 3.0,
                                     (0.9, 1.1))[:, None], device=env.sim.torch_device)
    assert not torch.equal(env.render_views(["vil_camera"], env_cams=ec)[:, 0], F[:, 1])
    with pytest.raises(KeyError, match="nope"):
        env.render_views(["nope"])
    # the wrapper: one camera keeps the shapes, a list adds the view axis
    act = torch.ones(n, env.nu, device=env.sim.torch_device)
    w1 = PixelObservationVecEnv(env, render_kwargs={"mode": "rgb", "camera": "vil_camera"})
    assert w1.pixel_space.shape == (64, 64, 3)
    px = w1.reset()[0]
    assert tuple(px.shape) == (n, 64, 64, 3) and px.dtype == torch.float32
    assert torch.equal(px, env.render_rgb(camera="vil_camera").float())
    assert tuple(w1.step(act)[0].shape) == (n, 64, 64, 3)
    wd = PixelObservationVecEnv(env, render_kwargs={"camera": wrist})
    assert wd.pixel_space.shape == (1, 64, 64) and tuple(wd.reset()[0].shape) == (n, 1, 64, 64)
    w2 = PixelObservationVecEnv(env, render_kwargs={"mode": "rgb", "camera": ["vil_camera", wrist]})
    assert w2.pixel_space.shape == (2, 64, 64, 3)
    px2 = w2.reset()[0]
    assert tuple(px2.shape) == (n, 2, 64, 64, 3) and float(px2.std()) > 0 and float(px2.max()) <= 255
    nxt = w2.step(act)[0]
    assert tuple(nxt.shape) == (n, 2, 64, 64, 3)
    wz = PixelObservationVecEnv(env, render_kwargs={"camera": ["fixed", wrist], "env_cams": ec.repeat(1, 2, 1)})
    assert wz.pixel_space.shape == (2, 64, 64) and tuple(wz.reset()[0].shape) == (n, 2, 64, 64)
    # without the key nothing changes: the free camera through aw_render_rgb / aw_render_depth
    w0 = PixelObservationVecEnv(env, render_kwargs={"mode": "rgb"})
    px0 = w0.reset()[0]
    env.sim.render_rgb(direct, env.mj_viewer_headless_setup(64, 64))
    assert tuple(px0.shape) == (n, 64, 64, 3) and torch.equal(px0, direct.float())
    assert tuple(PixelObservationVecEnv(env).reset()[0].shape) == (n, 1, 64, 64)

    class Cfg:
        env_name, state_type, pixel_mode, camera = "hammer-v0", "observation", "rgb", ["fixed", "vil_camera"]
    assert tuple(make_env(Cfg(), num_envs=2).reset()[0].shape) == (2, 2, 64, 64, 3)
    fac = HammerEnvV0()
    assert fac.render(camera="fixed").shape == (64, 64) and fac.render(mode="rgb", camera="vil_camera").shape == (64, 64, 3)
    assert fac.render().shape == (64, 64)
