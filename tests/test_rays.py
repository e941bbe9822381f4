"""Ray queries (aw_set_rays / aw_cast_rays), CPU side: the fp64 checker (tests/ray_checker.py) on
analytic scenes, and mj_envs_amd/rays.py -- keep_mask against hand-built expectations on the hammer
model, the builders' records, concat, every ValueError -- and the library's exports.  The HIP kernel
is held to the checker in tests/test_gpu_rays.py."""
import numpy as np
import pytest

import abi_header
import ray_checker
from conftest import load_task_model

EYE = np.eye(3)
ALL = np.uint64(0xFFFFFFFFFFFFFFFF)


def _one(geoms, p, v, keep=ALL, xmax=0.0):
    r = ray_checker.check(geoms, np.array([p], np.float64), np.array([v], np.float64), np.array([keep], np.uint64),
                          np.array([xmax]))
    return float(r["x"][0]), int(r["entry"][0]), bool(r["tie"][0]), bool(r["graze"][0])


def test_checker_analytic():
    sphere = (2, [0.5, 0, 0], np.zeros(3), EYE)
    assert _one([sphere], [0, -5, 0], [0, 1, 0])[:2] == (4.5, 0)
    assert _one([sphere], [0, -5, 0], [0, -1, 0])[:2] == (-1.0, -1)            # behind the origin: t >= 0 only
    # start inside: the exit crossing
    assert _one([sphere], [0, 0, 0], [0, 0, 1])[:2] == (0.5, 0)
    assert np.isclose(_one([sphere], [0.1, 0, 0], [1, 0, 0])[0], 0.4)
    # a non-unit vec: x is in units of vec
    assert np.isclose(_one([sphere], [0, -5, 0], [0, 2, 0])[0], 2.25)
    assert np.isclose(_one([sphere], [0, -5, 0], [0, 0.5, 0])[0], 9.0)
    # xmax, in units of x; <= 0: none
    assert _one([sphere], [0, -5, 0], [0, 1, 0], xmax=4.4)[:2] == (-1.0, -1)
    assert _one([sphere], [0, -5, 0], [0, 1, 0], xmax=4.6)[:2] == (4.5, 0)
    assert _one([sphere], [0, -5, 0], [0, 2, 0], xmax=2.2)[:2] == (-1.0, -1)
    box = (6, [0.3, 0.2, 0.1], np.zeros(3), EYE)
    assert np.isclose(_one([box], [0.01, -5, 0.02], [0, 1, 0])[0], 4.8)
    assert np.isclose(_one([box], [0.01, 0, 0.02], [0, 0, 1])[0], 0.08)        # inside a box
    cap = (3, [0.2, 0.5, 0], np.zeros(3), EYE)
    assert np.isclose(_one([cap], [0, -5, 0.1], [0, 1, 0])[0], 4.8)            # the lateral surface
    assert np.isclose(_one([cap], [0, 0, 5], [0, 0, -1])[0], 4.3)              # the end sphere
    cyl = (5, [0.3, 0.4, 0], np.zeros(3), EYE)
    assert np.isclose(_one([cyl], [0.1, 0.05, 5], [0, 0, -1])[0], 4.6)         # the cap
    assert _one([cyl], [0.31, 0, 5], [0, 0, -1])[:2] == (-1.0, -1)
    plane = (0, [0.05, 0.05, 0], np.zeros(3), EYE)
    assert np.isclose(_one([plane], [0.01, 0.02, 5], [0, 0, -1])[0], 5.0)
    assert np.isclose(_one([plane], [0.01, 0.02, -5], [0, 0, 1])[0], 5.0)      # from below too
    assert _one([plane], [0.06, 0, 5], [0, 0, -1])[:2] == (-1.0, -1)           # finite
    # rotated and moved: a capsule along world x at (1, 2, 3)
    R = np.array([[0, 0, 1], [0, 1, 0], [-1, 0, 0]], np.float64)
    assert np.isclose(_one([(3, [0.1, 0.4, 0], np.array([1.0, 2.0, 3.0]), R)], [1.2, 2, 5], [0, 0, -1])[0], 1.9)
    # nearest wins, keep masks out, an exact tie goes to the lower entry and is marked
    two = [box, (2, [0.1, 0, 0], np.array([0, -1.0, 0]), EYE)]
    x, e, tie, _ = _one(two, [0, -5, 0], [0, 1, 0])
    assert np.isclose(x, 3.9) and e == 1 and not tie
    assert np.isclose(_one(two, [0, -5, 0], [0, 1, 0], keep=np.uint64(1))[0], 4.8)
    assert _one(two, [0, -5, 0], [0, 1, 0], keep=np.uint64(0))[:2] == (-1.0, -1)
    x, e, tie, _ = _one([box, box], [0, -5, 0], [0, 1, 0])
    assert e == 0 and tie
    # graze: a ray 1e-6 inside a sphere's silhouette
    assert _one([sphere], [0.5 - 1e-6, -5, 0], [0, 1, 0])[3]
    assert not _one([sphere], [0.3, -5, 0], [0, 1, 0])[3]
    # zero and NaN vecs are misses
    assert _one([sphere], [0, -5, 0], [0, 0, 0])[:2] == (-1.0, -1)
    assert _one([sphere], [0, -5, 0], [0, np.nan, 0])[:2] == (-1.0, -1)


def test_keep_mask():
    from mj_envs_amd import labels, rays
    m = load_task_model("hammer-v0")
    geoms, _ = labels.render_entries(m)
    ng = len(geoms)
    bits = lambda mask: [geoms[e] for e in range(64) if mask >> e & 1]
    assert bits(rays.keep_mask(m)) == geoms and rays.keep_mask(m) < 1 << ng
    palm = m.name2id("body", "palm")
    want = [g for g in geoms if m.geom_bodyid[g] != palm]
    assert len(want) == ng - 2                                        # C_palm0, C_palm1
    assert bits(rays.keep_mask(m, bodyexclude=palm)) == want == bits(rays.keep_mask(m, bodyexclude="palm"))
    # flg_static False: the world's, the table's, the tracker's and the nail board's geoms go
    static = {"world", "table", "vive_tracker", "nail_board"}
    want = [g for g in geoms if m.names["body"][m.geom_bodyid[g]] not in static]
    assert bits(rays.keep_mask(m, flg_static=False)) == want and len(want) == ng - 9
    # one group: the hand's collision geoms are group 4
    want = [g for g in geoms if m.geom_group[g] == 4]
    assert bits(rays.keep_mask(m, geomgroup=[0, 0, 0, 0, 1, 0])) == want and len(want) == 20
    assert m.names["geom"][want[0]] == "C_forearm1"
    assert bits(rays.keep_mask(m, geomgroup=[1, 0, 0, 0, 0, 0])) == [g for g in geoms if m.geom_group[g] == 0]
    # an alpha-0 geom without a material, and a material with alpha 0
    head, handle = m.name2id("geom", "head"), m.name2id("geom", "handle")
    m.arrays["geom_rgba"] = m.geom_rgba.copy()
    m.arrays["geom_rgba"][head, 3] = 0.0
    m.arrays["geom_rgba"][handle, 3] = 0.0                            # has a material: its own alpha does not count
    assert bits(rays.keep_mask(m)) == [g for g in geoms if g != head]
    m.arrays["mat_rgba"] = m.mat_rgba.copy()
    m.arrays["mat_rgba"][m.geom_matid[handle], 3] = 0.0
    gone = {g for g in geoms if m.geom_matid[g] == m.geom_matid[handle]} | {head}
    assert handle in gone and bits(rays.keep_mask(m)) == [g for g in geoms if g not in gone]
    # bodies: subtrees through labels.keep_table; the rules combine
    m = load_task_model("hammer-v0")
    obj = [g for g in geoms if m.names["body"][m.geom_bodyid[g]] == "Object"]
    assert bits(rays.keep_mask(m, bodies=["Object"])) == obj and len(obj) == 3
    assert rays.keep_mask(m, bodies=["Object"], bodyexclude="Object") == 0
    assert rays.keep_mask(m, bodies=["Object"], flg_static=False) == rays.keep_mask(m, bodies=["Object"])


def test_builders():
    from mj_envs_amd import rays
    from mj_envs_amd._native import RAY_DTYPE
    from mj_envs_amd.mjcf import quat2mat
    m = load_task_model("hammer-v0")
    assert RAY_DTYPE.itemsize == 40 and [RAY_DTYPE.fields[k][1] for k in ("pnt", "vec", "xmax", "body", "keep")] == \
        [0, 12, 24, 28, 32]
    sites = ["S_fftip", "S_grasp", "tool"]
    rf = rays.rangefinder(m, sites, cutoff=0.5)
    assert len(rf) == 3 and rf.labels == sites and rf.records.dtype == RAY_DTYPE
    for k, s in enumerate(sites):
        i = m.name2id("site", s)
        r = rf.records[k]
        assert r["body"] == m.site_bodyid[i] and r["xmax"] == np.float32(0.5)
        assert np.array_equal(r["pnt"], m.site_pos[i].astype(np.float32))
        assert np.array_equal(r["vec"], quat2mat(m.site_quat[i])[:, 2].astype(np.float32))
        assert r["keep"] == rays.keep_mask(m, bodyexclude=int(m.site_bodyid[i]))
    assert len(rays.rangefinder(m, "S_grasp")) == 1 and rays.rangefinder(m, "S_grasp").records["xmax"][0] == 0
    # fan: unit, inside the cone, distinct, deterministic; ray 0 is the axis
    ax = np.array([0.0, 1.0, 1.0]) / np.sqrt(2)
    f = rays.fan(m, "palm", ax, 25.0, 12, xmax=0.3, bodyexclude="palm")
    v = f.records["vec"].astype(np.float64)
    assert len(f) == 12 and np.allclose(np.linalg.norm(v, axis=1), 1, atol=1e-6) and np.allclose(v[0], ax, atol=1e-7)
    assert (v @ ax >= np.cos(np.radians(25.0)) - 1e-6).all() and (v @ ax).min() < np.cos(np.radians(20.0))
    assert all(np.linalg.norm(v[i] - v[j]) > 1e-2 for i in range(12) for j in range(i))
    assert (f.records["body"] == m.name2id("body", "palm")).all() and (f.records["pnt"] == 0).all()
    assert (f.records["xmax"] == np.float32(0.3)).all() and f.records["keep"][0] == rays.keep_mask(m, bodyexclude="palm")
    assert np.array_equal(rays.fan(m, "palm", ax, 25.0, 12, xmax=0.3, bodyexclude="palm").records, f.records)
    i = m.name2id("site", "S_fftip")                                   # on a site: its position, axis in its frame
    fs = rays.fan(m, "S_fftip", [0, 0, 1], 30.0, 5)
    assert (fs.records["body"] == m.site_bodyid[i]).all() and np.array_equal(fs.records["pnt"][3], m.site_pos[i].astype(np.float32))
    assert np.allclose(fs.records["vec"][0], quat2mat(m.site_quat[i])[:, 2], atol=1e-6)
    sg = rays.segments(m, 7, bodyexclude="palm")
    assert len(sg) == 7 and (sg.records["xmax"] == 1).all() and (sg.records["body"] == 0).all()
    br = rays.body_rays(m, "ffdistal", [[0, 0, 0], [0, 0, 0.01]], [0, 0, 2.0], xmax=[0.1, 0.0])
    assert len(br) == 2 and br.records["xmax"].tolist() == [np.float32(0.1), 0.0] and br.records["vec"][1, 2] == 2.0
    assert br.labels == ["ffdistal[0]", "ffdistal[1]"]


def test_concat():
    from mj_envs_amd import rays
    m = load_task_model("hammer-v0")
    a, b = rays.fan(m, "palm", [0, 0, 1], 10.0, 5), rays.rangefinder(m, ["S_fftip", "S_mftip"])
    c = rays.concat(tips=b, wrist=a)
    assert len(c) == 7 and c.part("tips") == slice(0, 2) and c.part("wrist") == slice(2, 7)
    assert np.array_equal(c.records[c.part("wrist")], a.records) and c.labels[0] == "tips:S_fftip"
    d = rays.concat(c, extra=a)                                        # positional sets keep their parts
    assert d.part("tips") == slice(0, 2) and d.part("extra") == slice(7, 12) and len(d) == 12
    e = rays.concat(left=c, right=c)
    assert e.part("right.wrist") == slice(9, 14) and e.part("left") == slice(0, 7)
    with pytest.raises(KeyError):
        c.part("nope")
    full = rays.segments(m, 256)
    assert len(rays.concat(full)) == 256
    with pytest.raises(ValueError):
        rays.concat(full, one=rays.segments(m, 1))
    with pytest.raises(ValueError):
        rays.concat()
    with pytest.raises(ValueError):
        rays.concat(c, tips=a)                                         # a part named twice
    hits = rays.RayHits(c, np.arange(14.0).reshape(2, 7), np.arange(14).reshape(2, 7))
    sub = hits.named("wrist")
    assert sub.dist.tolist() == [[2, 3, 4, 5, 6], [9, 10, 11, 12, 13]] and len(sub.rays) == 5


def test_value_errors():
    """everything aw_set_rays would reject raises on the host, before a table exists"""
    from mj_envs_amd import rays
    m = load_task_model("hammer-v0")
    nb = int(m.nbody)
    bad = [lambda: rays.body_rays(m, nb, [0, 0, 0], [0, 0, 1]),
           lambda: rays.body_rays(m, -1, [0, 0, 0], [0, 0, 1]),
           lambda: rays.body_rays(m, "nobody", [0, 0, 0], [0, 0, 1]),
           lambda: rays.body_rays(m, 0, [0, 0, 0], [0, 0, 0]),
           lambda: rays.body_rays(m, 0, [0, 0, 0], [0, np.nan, 1]),
           lambda: rays.body_rays(m, 0, [0, 0, 0], [0, np.inf, 1]),
           lambda: rays.body_rays(m, 0, [np.inf, 0, 0], [0, 0, 1]),
           lambda: rays.body_rays(m, 0, [0, 0, 0], [0, 0, 1], xmax=np.nan),
           lambda: rays.body_rays(m, 0, [0, 0, 0], [0, 0, 1e39]),          # not finite as fp32
           lambda: rays.body_rays(m, 0, np.zeros((257, 3)), [0, 0, 1]),
           lambda: rays.body_rays(m, 0, [0, 0], [0, 0, 1]),
           lambda: rays.body_rays(m, 0, [0, 0, 0], [0, 0, 1], bodyexclude=nb),
           lambda: rays.body_rays(m, 0, [0, 0, 0], [0, 0, 1], geomgroup=[1, 1]),
           lambda: rays.body_rays(m, 0, [0, 0, 0], [0, 0, 1], bodies=["nobody"]),
           lambda: rays.rangefinder(m, ["no_site"]),
           lambda: rays.rangefinder(m, [int(m.nsite)]),
           lambda: rays.rangefinder(m, []),
           lambda: rays.rangefinder(m, ["S_grasp"], cutoff=np.inf),
           lambda: rays.fan(m, "nothing", [0, 0, 1], 10.0, 4),
           lambda: rays.fan(m, "palm", [0, 0, 0], 10.0, 4),
           lambda: rays.fan(m, "palm", [0, 0, 1], 10.0, 0),
           lambda: rays.fan(m, "palm", [0, 0, 1], 10.0, 257),
           lambda: rays.fan(m, "palm", [0, 0, 1], 200.0, 4),
           lambda: rays.segments(m, 0),
           lambda: rays.segments(m, 257)]
    for k, f in enumerate(bad):
        with pytest.raises(ValueError):
            f()
            pytest.fail(f"case {k} did not raise")
    rec = rays.segments(m, 2).records.copy()
    rec["body"][1] = nb
    with pytest.raises(ValueError):
        rays.Rays(m, rec)
    with pytest.raises(ValueError):
        rays.Rays(m, rays.segments(m, 2).records, labels=["one"])


def test_library_exports_rays():
    import ctypes
    from mj_envs_amd import _native
    lib = _native.load()
    for s in ("aw_set_rays", "aw_cast_rays"):
        assert s in _native.EXPORTS and isinstance(getattr(lib, s), ctypes._CFuncPtr)
    assert abi_header.defines()["AW_MAX_RAYS"] == 256 and _native.AW_MAX_RAYS == 256
    assert abi_header.struct_body("aw_ray_rec") == "float pnt[3], vec[3]; float xmax; int32_t body; uint64_t keep;"
    # RAY_DTYPE is that record: the same fields in the same order, packed as the C struct is
    ctype = {"float": "<f4", "int32_t": "<i4", "uint64_t": "<u8"}
    want = []
    for t, name in abi_header.struct_fields("aw_ray_rec"):
        name, _, ext = name.partition("[")
        want.append((name, ctype[t], (int(ext[:-1]),)) if ext else (name, ctype[t]))
    assert _native.RAY_DTYPE == np.dtype(want) and _native.RAY_DTYPE.itemsize == 40
    assert hasattr(_native.Sim, "set_rays") and hasattr(_native.Sim, "cast_rays")
