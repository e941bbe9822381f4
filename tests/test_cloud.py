"""Point-cloud observations (aw_render_cloud, aw_cloud_fps): the numpy farthest-point-sampling checker
against the rule's fp64 definition, what fp32 poses cost the checker's cloud membership, the keep
tables and the default crops (CPU); the HIP kernels k_fps against that checker bit for bit and
k_cloud against the label and depth frames of aw_render_labels, against the fp64 checker
(tests/cloud_checker.py), in a body's frame, its errors and its Python surface (GPU).

Membership of a cloud is a per-pixel yes / no, compared like a label: >= 99.5 % of a frame's pixels
agree with the checker (label_checker.AGREE, the project's depth gate), and where both sides see the
same entry the points agree to 2e-3 m, the depth gate.
"""
import functools

import numpy as np
import pytest

import cloud_checker
import label_checker
from conftest import ENVS, load_task_model, make_oracle
from test_cameras import DEPTH_TOL, _bits, _compose32, _guarded, _guards_ok, _world_record, _wrist
from test_labels import _labels
from test_render_rgb import APPEARANCE, _gpu, _make_sim, _state

# the crop of every scene below: it cuts through the hand, the object and (door) the door, with no
# face on a large flat surface -- the table top is at z = 0, the slab's underside at z = -0.05
BOX = np.array([-0.30, -0.35, -0.10, 0.25, 0.30, 0.32], np.float32)
XYZ_FILL, PIX_FILL, CNT_FILL = 0xA5, 0x5A, 0x5A
UNTOUCHED = 0x5A5A5A5A


def _keep(m):
    """the keep table of the tests: everything but the table (its top and legs)"""
    from mj_envs_amd import labels
    return labels.keep_table(m, ["table"], drop=True)


# ---------------------------------------------------------------------------------------
# CPU
def test_fps_checker_vs_definition():
    rng = np.random.default_rng(0)
    for c, P in ((40, 16), (61, 61), (23, 40), (1, 4)):
        p = rng.normal(size=(c, 3)).astype(np.float32)
        want = cloud_checker.fps_definition(p, P)
        got = cloud_checker.fps(np.concatenate([p, rng.normal(size=(7, 3)).astype(np.float32)]), c, P)
        assert got.dtype == np.int32 and got.shape == (P,)
        assert list(got[:min(P, c)]) == want, (c, P)
        assert len(set(want)) == len(want)                                    # no near-ties: all distinct
        assert list(got) == [want[k % c] for k in range(P)]                   # cyclic padding
    # the count is clamped to the rows there are; an empty row
    p = rng.normal(size=(9, 3)).astype(np.float32)
    assert list(cloud_checker.fps(p, 500, 9)) == cloud_checker.fps_definition(p, 9)
    assert list(cloud_checker.fps(p, 0, 3)) == [-1, -1, -1] and list(cloud_checker.fps(p, -4, 2)) == [-1, -1]
    assert cloud_checker.fps_rows(np.stack([p, p]), [9, 4], 5).shape == (2, 5)


def test_fps_checker_lattice_ties():
    """integer lattice points, some twice: every squared distance is an exact integer in fp32 and in
    fp64, so the two agree on every tie, which goes to the lowest index; ties there are (the highest
    index would select differently)"""
    rng = np.random.default_rng(1)
    p = rng.integers(0, 3, size=(48, 3)).astype(np.float32)
    assert len({tuple(r) for r in p}) < len(p)                                # duplicates
    want = cloud_checker.fps_definition(p, 48)
    assert list(cloud_checker.fps(p, 48, 48)) == want
    assert cloud_checker.fps_definition(p, 48, highest=True) != want
    # once every distinct point is taken the minimum distance is 0 everywhere: index 0 again
    nd = len({tuple(r) for r in p})
    assert want[nd] == 0 and len(set(want[:nd])) == nd


def _cal_views(m, env_id):
    from mj_envs_amd.render import free_camera, model_camera
    return [(64, 64, {"free": (free_camera(m, env_id, 64, 64), 0), "vil_camera": model_camera(m, "vil_camera", 64, 64)}),
            (40, 25, {"vil_camera": model_camera(m, "vil_camera", 40, 25)})]


def test_cloud_calibration(oracle_lib):
    """What fp32 alone costs the checker's cloud: membership (hit, kept, inside BOX) of the checker on
    the oracle's fp64 poses against the checker on the poses rounded to fp32 with the camera moved
    1e-6 m, on scenes made like the GPU tests', at their sizes, views, keep table and box.  At most
    1 - AGREE of a frame's pixels disagree (measured: none); BOX cuts every scene
    (some hits inside, some outside) and the two clouds' points stay within the depth gate."""
    import rgb_checker
    from mj_envs_amd.tasks import sample_params
    f32 = lambda es: [(t, s, np.float32(p).astype(np.float64), np.float32(x).astype(np.float64)) for t, s, p, x in es]
    for env_id in ENVS:
        m, orc = make_oracle(env_id)
        keep = _keep(m)
        rng = np.random.default_rng(5)
        n = 2
        st, _ = orc.reset(sample_params(env_id, m, rng, n))
        for _ in range(6):
            orc.step(st, rng.uniform(-1, 1, (n, orc.nu)))
        for e in range(n):
            orc.forward1(st["params"][e], st["qpos"][e], st["qvel"][e])
            geoms, sites, _, _ = rgb_checker.oracle_scene(orc, m, st["params"][e])
            for W, H, views in _cal_views(m, env_id):
                for name, view in views.items():
                    cam = _world_record(orc, m, view)
                    moved = cam.copy()
                    moved[:3] += 1e-6
                    for with_sites in (0, 1):
                        ea, pa, _ = cloud_checker.unproject(cam, W, H, geoms, sites, with_sites)
                        eb, pb, _ = cloud_checker.unproject(moved, W, H, f32(geoms), f32(sites), with_sites)
                        for kp in (None, keep):
                            ma, mb = cloud_checker.members(ea, pa, kp, BOX), cloud_checker.members(eb, pb, kp, BOX)
                            flips = (ma != mb).mean()
                            both = ma & mb & (ea == eb)
                            far = np.linalg.norm(pa[both] - pb[both], axis=-1).max() if both.any() else 0.0
                            hits = ea >= 0
                            print(f"cloud calibration {env_id} env {e} {name} {W}x{H} sites {with_sites} "
                                  f"keep {kp is not None}: {flips:.5f} of pixels flip, {ma.sum()} of {hits.sum()} hits "
                                  f"inside, points {far:.2e} m apart")
                            assert flips <= 1.0 - label_checker.AGREE, (env_id, e, name, W, H, flips)
                            assert far <= DEPTH_TOL
                            if kp is None:
                                assert 0 < ma.sum() < hits.sum(), (env_id, e, name, W, H)   # the box cuts the scene


def test_keep_table_and_workspace_box():
    from mj_envs_amd import labels
    from mj_envs_amd.render import WORKSPACE_CLEARANCE, workspace_box
    for env_id in ENVS:
        m = load_task_model(env_id)
        body = labels.label_table(m, "body")
        names = [m.names["body"][int(b)] for b in body]
        obj = "frame" if env_id == "door-v0" else "Object"                       # the door hangs in its frame
        k = labels.keep_table(m, ["forearm", obj])
        assert k.dtype == np.uint8 and k.shape == body.shape and set(k.tolist()) == {0, 1}
        assert np.array_equal(k, (labels.body_classes(m, ["forearm", obj]) > 0).astype(np.uint8))
        assert all(k[i] == 0 for i, nm in enumerate(names) if nm in ("world", "table"))
        assert all(k[i] == 1 for i, nm in enumerate(names) if nm in ("palm", "Object", "latch") or nm[:2] == "ff")
        assert {"palm", obj, "table", "world"} <= set(names)
        d = labels.keep_table(m, ["table"], drop=True)
        assert all(d[i] == 0 for i, nm in enumerate(names) if nm == "table") and 0 < d.sum() < len(d)
        assert all(d[i] == 1 for i, nm in enumerate(names) if nm in ("world", "palm", obj))
        assert np.array_equal(labels.keep_table(m, ["table"]) + d, np.ones_like(d))
        assert labels.keep_table(m, []).sum() == 0
        # the default crop: over the table top, starting just above it
        b = workspace_box(env_id)
        assert b.dtype == np.float32 and b.shape == (6,) and (b[:3] < b[3:]).all()
        assert np.array_equal(b, workspace_box(env_id, m))
        assert np.allclose(b[[0, 1, 3, 4]], [-0.45, -0.45, 0.45, 0.45]) and b[2] == pytest.approx(WORKSPACE_CLEARANCE)
        assert 0.5 <= b[5] <= 1.0
    assert workspace_box("door-v0")[5] > workspace_box("hammer-v0")[5]        # the door stands taller


# ---------------------------------------------------------------------------------------
# GPU: farthest-point sampling
@functools.lru_cache(maxsize=None)
def _fps_case(cap, P):
    """(xyz [n, cap, 3], count [n], checker's idx [n, P]) of one shape, computed once"""
    rng = np.random.default_rng(cap)
    if cap == 300:
        count = np.array([300, 37, 0, 500], np.int32)             # the last exceeds cap: 300 are used
        xyz = rng.normal(size=(4, cap, 3)).astype(np.float32)
        xyz[3] = rng.integers(0, 6, size=(cap, 3))                # lattice points, some twice: exact ties
        assert len({tuple(r) for r in xyz[3]}) < cap
    else:
        count = np.array([cap, cap - cap // 3 - 1], np.int32)
        xyz = rng.normal(size=(2, cap, 3)).astype(np.float32)
    xyz.setflags(write=False)
    idx = cloud_checker.fps_rows(xyz, count, P)
    idx.setflags(write=False)
    return xyz, count, idx


@pytest.mark.gpu
@pytest.mark.parametrize("cap,P", [(300, 16), (300, 64), (1500, 8), (3000, 8), (8192, 8)])
def test_gpu_fps_exact(cap, P):
    """k_fps against the numpy fp32 checker, index for index: cap 300 (the 1024-candidate
    instantiation; rows of 300, 37 -- padded cyclically at P = 64 --, 0 and 500 > cap candidates, the
    last a lattice with duplicates), cap 1500 and 3000 (the 2048 and 4096 ones) and cap 8192 (the
    largest LDS); the rows' counts give one to eight candidates per thread, full and partial"""
    torch = _gpu()
    from mj_envs_amd import _native

    class Dev:
        torch_device = torch.device("cuda:0")
    xyz, count, want = _fps_case(cap, P)
    n = len(count)
    X = torch.tensor(xyz, device=Dev.torch_device)
    C = torch.tensor(count, device=Dev.torch_device)
    O, oraw = _guarded(torch, Dev, (n, P, 3), torch.float32, XYZ_FILL)
    I, iraw = _guarded(torch, Dev, (n, P), torch.int32, PIX_FILL)
    _native.cloud_fps(X, C, O, I)
    torch.cuda.synchronize()
    assert _guards_ok(oraw, XYZ_FILL) and _guards_ok(iraw, PIX_FILL), "bytes written outside the outputs"
    idx, out = I.cpu().numpy(), O.cpu().numpy()
    for r in range(n):
        differ = np.flatnonzero(idx[r] != want[r])
        print(f"fps cap {cap} P {P} row {r} (count {count[r]}): {len(differ)} of {P} selections differ"
              + (f", first at {differ[0]}: {idx[r][differ[0]]} for {want[r][differ[0]]}" if len(differ) else ""))
    assert np.array_equal(idx, want)
    ref = np.where((want >= 0)[..., None], xyz[np.arange(n)[:, None], np.maximum(want, 0)], np.float32(0))
    assert np.array_equal(_bits(out), _bits(ref.astype(np.float32)))
    if cap == 300:
        assert (idx[2] == -1).all() and (out[2] == 0).all()
        assert idx[3].max() < 300 and (P == 16 or np.array_equal(idx[1][37:], idx[1][:P - 37]))
    # without out_idx the points are the same
    O2, o2raw = _guarded(torch, Dev, (n, P, 3), torch.float32, XYZ_FILL)
    _native.cloud_fps(X, C, O2)
    torch.cuda.synchronize()
    assert _guards_ok(o2raw, XYZ_FILL) and torch.equal(O2, O)


# ---------------------------------------------------------------------------------------
# GPU: the candidates
def _cloud(sim, views, W, H, cap, keep=None, box=None, frame_body=0, sites=0, env_cam=None, env_ids=None, pix=True):
    """one aw_render_cloud launch into sentinel-filled, guarded outputs -> (xyz, pix, count) numpy"""
    torch = _gpu()
    n = sim.n_envs if env_ids is None else len(env_ids)
    X, xraw = _guarded(torch, sim, (n, cap, 3), torch.float32, XYZ_FILL)
    C, craw = _guarded(torch, sim, (n,), torch.int32, CNT_FILL)
    P = praw = None
    if pix:
        P, praw = _guarded(torch, sim, (n, cap), torch.int32, PIX_FILL)
    ec = None if env_cam is None else torch.tensor(np.asarray(env_cam, np.float32), device=sim.torch_device).contiguous()
    ids = None if env_ids is None else torch.tensor(np.asarray(env_ids, np.int32), device=sim.torch_device)
    sim.render_cloud(views, W, H, X, C, pix=P, keep=keep, box=box, frame_body=frame_body, sites=sites, env_cam=ec,
                     env_ids=ids)
    torch.cuda.synchronize()
    assert _guards_ok(xraw, XYZ_FILL), "bytes written outside xyz"
    assert _guards_ok(craw, CNT_FILL), "bytes written outside count"
    assert praw is None or _guards_ok(praw, PIX_FILL), "bytes written outside pix"
    return X.cpu().numpy(), (None if P is None else P.cpu().numpy()), C.cpu().numpy()


def _untouched_past(xyz, pix, count, cap):
    """the slots past min(count, cap) still hold the sentinels"""
    for r, c in enumerate(np.minimum(count, cap)):
        if not (_bits(xyz[r, c:]) == 0xA5A5A5A5).all() or (pix is not None and not (pix[r, c:] == UNTOUCHED).all()):
            return False
    return True


def _inside(p, box):
    return ((p >= box[:3]) & (p <= box[3:])).all(-1)              # fp32 comparisons, as the kernel's


@pytest.mark.gpu
@pytest.mark.parametrize("W,H", [(7, 5), (40, 25)])
def test_gpu_cloud_matches_labels(W, H):
    """the free camera and the palm-mounted camera in one launch, the table dropped, BOX cutting the
    scene: pix and count are, exactly and in order, the pixels whose aw_render_labels entry (lut NULL,
    the same views) is kept and whose returned point passes the box test; the points reproduce that
    call's depth frame; a smaller cap, the sites, per-env records and a subset with ids out of range"""
    from mj_envs_amd.render import free_camera, jitter_cameras
    n, V = 3, 2
    m, orc, sim = _make_sim("hammer-v0", n)
    views = [(free_camera(m, "hammer-v0", W, H), 0), _wrist(m, W, H)]
    keep, np_ = _keep(m), W * H
    cap = V * np_
    ng = sim.render_entries()[0]
    palm = views[1][1]
    J = np.stack([jitter_cameras(r, n, np.random.default_rng(3 + k), 0.02, 3.0, (0.9, 1.1))
                  for k, (r, _) in enumerate(views)], axis=1)
    for sites, ec in ((0, None), (1, None), (0, J)):
        E, Z = _labels(sim, views, W, H, sites=sites, env_cam=ec)
        E, Z = E.reshape(n, cap), Z.reshape(n, cap)
        allx, allp, allc = _cloud(sim, views, W, H, cap, keep=keep, sites=sites, env_cam=ec)      # no crop
        xyz, pix, count = _cloud(sim, views, W, H, cap, keep=keep, box=BOX, sites=sites, env_cam=ec)
        assert _untouched_past(allx, allp, allc, cap) and _untouched_past(xyz, pix, count, cap)
        for e in range(n):
            kept = np.flatnonzero((E[e] >= 0) & (keep[np.maximum(E[e], 0)] != 0))
            assert allc[e] == len(kept) and np.array_equal(allp[e, :allc[e]], kept), (sites, e)
            want = _inside(allx[e, :allc[e]], BOX)
            print(f"cloud {W}x{H} sites {sites} per-env {ec is not None} env {e}: {(E[e] >= 0).sum()} hits, "
                  f"{len(kept)} kept, {want.sum()} inside the box")
            assert count[e] == want.sum() and np.array_equal(pix[e, :count[e]], kept[want]), (sites, e)
            assert np.array_equal(_bits(xyz[e, :count[e]]), _bits(allx[e, :allc[e]][want]))
            assert count[e] <= allc[e] <= (E[e] >= 0).sum()
            if W == 40:
                assert 0 < count[e] < allc[e] < (E[e] >= 0).sum()              # the box and the table both cut
            # the points against the depth frames of the labels call: depth = (xyz - cam) . forward
            d = sim.forward_dump(e)
            for v, (rec, body) in enumerate(views):
                r = rec if ec is None else ec[e][v]
                cam = _compose32(r, d["xpos"][body], d["xquat"][body]) if body else np.asarray(r, np.float64)
                mine = (allp[e, :allc[e]] >= v * np_) & (allp[e, :allc[e]] < (v + 1) * np_)
                z = (allx[e, :allc[e]][mine].astype(np.float64) - cam[:3]) @ cam[3:6]
                zref = Z[e][allp[e, :allc[e]][mine]].astype(np.float64)
                rel = np.abs(z - zref) / zref
                site = E[e][allp[e, :allc[e]][mine]] >= ng
                print(f"  view {v}: {mine.sum()} points ({site.sum()} on sites), depth within "
                      f"{rel[~site].max() if (~site).any() else 0:.2e} relative")
                assert mine.any() or W < 40, (sites, e, v)
                # a geom's point and the depth come from the same crossing, a few fp32 roundings apart; a site's
                # point lies in front of the depth frame, which sites never write
                assert (rel[~site] <= 1e-5).all() and (z[site] < zref[site]).all(), (sites, e, v)
                assert sites or not site.any()
        if ec is None and sites == 0:
            full, fullc = (xyz, pix), count
    xyz, pix = full
    # a smaller cap: the first cap candidates and the true count
    small = max(1, int(fullc.max()) // 2)
    sx, sp, sc = _cloud(sim, views, W, H, small, keep=keep, box=BOX)
    assert np.array_equal(sc, fullc) and np.array_equal(sp, pix[:, :small])
    assert np.array_equal(_bits(sx), _bits(xyz[:, :small]))
    # without pix; without a keep table every hit is a candidate
    nx, npix, nc = _cloud(sim, views, W, H, cap, keep=keep, box=BOX, pix=False)
    assert npix is None and np.array_equal(nc, fullc) and np.array_equal(_bits(nx), _bits(xyz))
    E, _ = _labels(sim, views, W, H, depth=False)
    _, hp, hc = _cloud(sim, views, W, H, cap)
    for e in range(n):
        assert np.array_equal(hp[e, :hc[e]], np.flatnonzero(E[e].reshape(-1) >= 0))
    # a subset: rows in the order of env_ids; an id outside [0, N) leaves its row untouched, count included
    ox, op, oc = _cloud(sim, views, W, H, cap, keep=keep, box=BOX, env_ids=[-1, 2, n, 2, 0])
    assert (_bits(ox[[0, 2]]) == 0xA5A5A5A5).all() and (op[[0, 2]] == UNTOUCHED).all() and (oc[[0, 2]] == UNTOUCHED).all()
    for row, e in ((1, 2), (3, 2), (4, 0)):
        assert oc[row] == fullc[e] and np.array_equal(op[row], pix[e]) and np.array_equal(_bits(ox[row]), _bits(xyz[e]))
    assert palm > 0 and (fullc[0] != fullc[1] or (pix[0] != pix[1]).any())     # the envs differ


@pytest.mark.gpu
@pytest.mark.parametrize("env_id", ENVS)
def test_gpu_cloud_vs_checker(env_id):
    """the scenes and sizes of test_gpu_labels_vs_checker: membership of the cloud (hit, table dropped,
    inside BOX) against the fp64 checker on the oracle's kinematics on >= AGREE of a frame's pixels,
    and the points of the pixels where both see the same entry within the depth gate"""
    import rgb_checker
    from mj_envs_amd.render import free_camera, model_camera
    n = 2
    m, orc, sim = _make_sim(env_id, n)
    keep = _keep(m)
    Q, Vel, P = _state(sim)
    for W, H, views, names in ((64, 64, [(free_camera(m, env_id, 64, 64), 0), model_camera(m, "vil_camera", 64, 64)],
                                ("free", "vil_camera")),
                               (40, 25, [model_camera(m, "vil_camera", 40, 25)], ("vil_camera",))):
        np_ = W * H
        cap = len(views) * np_
        refs = {}
        for e in range(n):
            orc.forward1(P[e] if len(P[e]) else None, Q[e], Vel[e])
            geoms, sites, _, _ = rgb_checker.oracle_scene(orc, m, P[e])
            for v, view in enumerate(views):
                cam = _world_record(orc, m, view)
                refs[e, v] = [cloud_checker.unproject(cam, W, H, geoms, sites, s)[:2] for s in (0, 1)]
        for with_sites in (0, 1):
            xyz, pix, count = _cloud(sim, views, W, H, cap, keep=keep, box=BOX, sites=with_sites)
            E, _ = _labels(sim, views, W, H, sites=with_sites, depth=False)
            assert (count <= cap).all() and (count > 0).all()
            for e in range(n):
                got = np.zeros(cap, bool)
                got[pix[e, :count[e]]] = True
                pts = np.full((cap, 3), np.nan)
                pts[pix[e, :count[e]]] = xyz[e, :count[e]]
                assert (np.diff(pix[e, :count[e]]) > 0).all()
                for v, name in enumerate(names):
                    entry, ref = refs[e, v][with_sites]
                    want = cloud_checker.members(entry, ref, keep, BOX)
                    mine = got[v * np_:(v + 1) * np_]
                    agree = (mine == want).mean()
                    both = mine & want & (E[e, v].reshape(-1) == entry)
                    far = np.linalg.norm(pts[v * np_:(v + 1) * np_][both] - ref[both], axis=-1)
                    print(f"cloud {env_id} env {e} {name} {W}x{H} sites {with_sites}: {agree:.5f} of pixels agree, "
                          f"{mine.sum()} / {want.sum()} members, {both.sum()} shared points within "
                          f"{far.max() if both.any() else 0:.2e} m")
                    assert agree >= label_checker.AGREE, (env_id, e, name, W, H, agree)
                    assert both.any() and far.max() <= DEPTH_TOL, (env_id, e, name, W, H)


@pytest.mark.gpu
def test_gpu_cloud_frame_body():
    """frame_body = palm: the same candidates, each the world-frame point of the same call carried into
    the palm's frame with the oracle's palm pose at the env's qpos, to the 1e-5 m the GPU's body frames
    agree with the oracle's; the crop is still the world's"""
    from mj_envs_amd.render import free_camera
    n, W, H = 3, 40, 25
    m, orc, sim = _make_sim("hammer-v0", n)
    views = [(free_camera(m, "hammer-v0", W, H), 0), _wrist(m, W, H)]
    keep, cap = _keep(m), 2 * W * H
    palm = m.name2id("body", "palm")
    wx, wp, wc = _cloud(sim, views, W, H, cap, keep=keep, box=BOX)
    bx, bp, bc = _cloud(sim, views, W, H, cap, keep=keep, box=BOX, frame_body=palm)
    assert np.array_equal(wc, bc) and np.array_equal(wp, bp) and (wc > 0).all()
    Q, Vel, P = _state(sim)
    for e in range(n):
        orc.forward1(P[e] if len(P[e]) else None, Q[e], Vel[e])
        xpos, xquat = orc.get("xpos").reshape(-1, 3)[palm], orc.get("xquat").reshape(-1, 4)[palm]
        want = cloud_checker.to_body_frame(wx[e, :wc[e]], xpos, xquat)
        err = np.abs(bx[e, :wc[e]] - want).max()
        print(f"frame_body env {e}: {wc[e]} points, palm-frame points within {err:.2e} m")
        assert err <= 1e-5, (e, err)
        assert np.abs(bx[e, :wc[e]] - wx[e, :wc[e]]).max() > 0.05            # another frame altogether
    # frame 0 through the argument is the default
    zx, zp, zc = _cloud(sim, views, W, H, cap, keep=keep, box=BOX, frame_body=0)
    assert np.array_equal(_bits(zx), _bits(wx)) and np.array_equal(zp, wp)


@pytest.mark.gpu
def test_gpu_cloud_errors():
    from mj_envs_amd import _native
    from mj_envs_amd.render import free_camera
    torch = _gpu()
    n, W, H, cap = 2, 16, 16, 64
    m, orc, sim = _make_sim("hammer-v0", n, steps=0)
    cam = free_camera(m, "hammer-v0", W, H)
    xyz, cnt = sim.empty(n, cap, 3), sim.empty(n, dtype=torch.int32)
    ids = torch.tensor([1, 0], dtype=torch.int32, device=sim.torch_device)
    einval = lambda: pytest.raises(_native.NativeError, match="error -1")
    call = lambda views=((cam, 0),), w=W, h=H, x=xyz, c=cnt, **kw: sim.render_cloud(list(views), w, h, x, c, **kw)
    with einval():
        call(views=())                                                            # nviews 0
    with einval():
        call(views=[(cam, 0)] * 5)                                                # nviews > AW_MAX_VIEWS
    for body in (-1, sim.nbody):
        with einval():
            call(views=[(cam, body)])
    with einval():
        call(x=None, cap=cap)                                                     # NULL xyz
    with einval():
        call(c=None)                                                              # NULL count
    for w, h in ((1025, 1), (1, 1025), (0, 4), (4, 0)):
        with einval():
            call(w=w, h=h)
    for k in (0, -3):
        with einval():
            call(env_ids=ids, n_sel=k)                                            # n_sel < 1 with env_ids
    for s in (2, -1):
        with einval():
            call(sites=s)
    for c in (0, -1, _native.AW_CLOUD_MAXCAND + 1):
        with einval():
            call(cap=c)                                                           # cap out of range
    for b in (-1, sim.nbody):
        with einval():
            call(frame_body=b)
    for axis in range(3):
        bad = BOX.copy()
        bad[axis], bad[3 + axis] = BOX[3 + axis], BOX[axis]                       # lo > hi
        with einval():
            call(box=bad)
    with einval():
        call(box=np.array([0, 0, np.nan, 1, 1, 1], np.float32))
    # aw_cloud_fps
    out, idx = sim.empty(n, 8, 3), sim.empty(n, 8, dtype=torch.int32)
    for kw in (dict(cap=0), dict(cap=_native.AW_CLOUD_MAXCAND + 1), dict(npoints=0),
               dict(npoints=_native.AW_FPS_MAXPOINTS + 1)):
        with einval():
            _native.cloud_fps(xyz, cnt, out, idx, **kw)
    with einval():
        _native.cloud_fps(None, cnt, out, idx, cap=cap)
    with einval():
        _native.cloud_fps(xyz, cnt, None, None, npoints=8)
    # the limits themselves pass, and a valid call still works after the failures
    big = sim.empty(n, _native.AW_CLOUD_MAXCAND, 3)
    sim.render_cloud([(cam, 0)] * 4, W, H, big, cnt, sites=1, frame_body=sim.nbody - 1,
                     box=np.array([0, 0, 0, 0, 0, 0], np.float32))             # lo == hi is a box
    sim.render_cloud([(cam, sim.nbody - 1)], W, H, xyz[:1].contiguous(), cnt[:1].contiguous(), env_ids=ids[:1], n_sel=1)
    one = sim.empty(n, 1, 3)
    sim.render_cloud([(cam, 0)], W, H, one, cnt)
    _native.cloud_fps(one, cnt, sim.empty(n, _native.AW_FPS_MAXPOINTS, 3))
    torch.cuda.synchronize()
    assert int(cnt.min()) > 1                                                     # the count is not capped
    # a model table without the appearance arrays: geoms work, sites are unsupported
    m0 = load_task_model("hammer-v0")
    for k in APPEARANCE:
        del m0.arrays[k]
    old = _native.Sim(m0.to_blob(), n)
    old.reset(old.empty(n, old.obs_dim), seed=3)
    with pytest.raises(_native.NativeError, match="error -5"):
        old.render_cloud([(cam, 0)], W, H, xyz, cnt, sites=1)
    old.render_cloud([(cam, 0)], W, H, xyz, cnt)
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_gpu_cloud_python_surface():
    torch = _gpu()
    from mj_envs_amd import labels
    from mj_envs_amd.envs import AdroitVecEnv, HammerEnvV0
    from mj_envs_amd.render import workspace_box
    from mj_envs_amd.wrappers import PixelObservationVecEnv, make_env
    n = 3
    env = AdroitVecEnv("hammer-v0", n)
    env.reset()
    wrist = _wrist(env.model, 64, 64)
    pts, count = env.render_pointcloud()
    assert tuple(pts.shape) == (n, 512, 3) and pts.dtype == torch.float32 and pts.is_cuda
    assert tuple(count.shape) == (n,) and count.dtype == torch.int32 and int(count.min()) > 512
    assert int(count.max()) <= 4096                                               # the clamped count
    again, count2 = env.render_pointcloud()
    assert torch.equal(pts, again) and torch.equal(count, count2)                 # deterministic, bit for bit
    box = workspace_box("hammer-v0")
    p2, c2, i2 = env.render_pointcloud(["free", wrist], 32, 24, num_points=64, crop="workspace",
                                       keep=["forearm", "Object", "nail_board"], frame="palm", return_index=True)
    assert tuple(p2.shape) == (n, 64, 3) and tuple(i2.shape) == (n, 64) and i2.dtype == torch.int32
    assert int(c2.min()) > 0 and int(i2.min()) >= 0 and int(i2.max()) < 2 * 32 * 24
    a2, b2, j2 = env.render_pointcloud(["free", wrist], 32, 24, num_points=64, crop=box,
                                       keep=labels.keep_table(env.model, ["forearm", "Object", "nail_board"]),
                                       frame=env.model.name2id("body", "palm"), return_index=True)
    assert torch.equal(p2, a2) and torch.equal(c2, b2) and torch.equal(i2, j2)
    # the index gathers what the sampled pixels show: kept bodies only
    seg = env.render_segmentation(["free", wrist], 32, 24, lut=labels.keep_table(env.model, ["forearm", "Object",
                                  "nail_board"]).astype(np.int32), background=0)
    assert bool((torch.gather(seg.reshape(n, -1), 1, i2.long()) == 1).all())
    # world-frame points of a cropped cloud lie inside the crop; selection 0 is the first candidate
    pw, cw, iw = env.render_pointcloud("vil_camera", crop=box, return_index=True)
    lo, hi = torch.tensor(box[:3], device=pw.device), torch.tensor(box[3:], device=pw.device)
    assert bool(((pw >= lo) & (pw <= hi)).all()) and bool((iw[:, 0] == iw.min(dim=1).values).all())
    sub, csub = env.render_pointcloud("vil_camera", crop=box, env_ids=[2, 0])
    assert tuple(sub.shape) == (2, 512, 3) and torch.equal(sub, pw[[2, 0]]) and torch.equal(csub, cw[[2, 0]])
    few, cfew = env.render_pointcloud("vil_camera", crop=box, max_candidates=100, num_points=128)
    assert tuple(few.shape) == (n, 128, 3) and bool((cfew == 100).all()) and torch.equal(few[:, 100:], few[:, :28])
    none, cnone = env.render_pointcloud(crop=[5, 5, 5, 6, 6, 6])                  # an empty cloud: zeros
    assert bool((cnone == 0).all()) and bool((none == 0).all())
    with pytest.raises(ValueError):
        env.render_pointcloud(crop="nope")
    # the facade
    fac = HammerEnvV0()
    cloud = fac.render(mode="pointcloud")
    assert cloud.shape == (512, 3) and cloud.dtype == np.float64 and np.isfinite(cloud).all() and cloud.std() > 0
    assert fac.render(mode="pointcloud", camera="vil_camera", num_points=32, crop="workspace").shape == (32, 3)
    assert fac.render().shape == (64, 64)                                         # the other modes are what they were
    # the wrapper
    w1 = PixelObservationVecEnv(env, render_kwargs={"mode": "pointcloud", "num_points": 256, "crop": "workspace",
                                                    "camera": ["vil_camera", wrist], "keep": ["forearm", "Object"]})
    assert w1.pixel_space.shape == (256, 3) and w1.observation_space.shape == (256, 3)
    px = w1.reset()[0]
    assert tuple(px.shape) == (n, 256, 3) and px.dtype == torch.float32
    want, wc = env.render_pointcloud(["vil_camera", wrist], num_points=256, crop="workspace", keep=["forearm", "Object"])
    assert torch.equal(px, want) and torch.equal(w1.cloud_count, wc)
    act = torch.ones(n, env.nu, device=env.sim.torch_device)
    nxt = w1.step(act)[0]
    assert tuple(nxt.shape) == (n, 256, 3) and not torch.equal(nxt, want)
    w0 = PixelObservationVecEnv(env, render_kwargs={"mode": "pointcloud"})
    assert w0.pixel_space.shape == (512, 3) and tuple(w0.reset()[0].shape) == (n, 512, 3)
    assert tuple(PixelObservationVecEnv(env).reset()[0].shape) == (n, 1, 64, 64)  # depth, as before

    class Cfg:
        env_name, state_type, pixel_mode, num_points, camera = "hammer-v0", "observation", "pointcloud", 128, "vil_camera"
    assert tuple(make_env(Cfg(), num_envs=2).reset()[0].shape) == (2, 128, 3)
    Cfg.camera, Cfg.num_points = None, None
    assert tuple(make_env(Cfg(), num_envs=2).reset()[0].shape) == (2, 512, 3)
