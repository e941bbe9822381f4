"""Inverse kinematics, the parts that need no GPU: check_ik_args' rejections, ik.targets / ik.dof_mask /
qpos_to_actions on the models, the shape checks of AdroitVecEnv.solve_ik, and the condition the GPU
tests (tests/test_gpu_ik.py) rely on: the fp64 checker (tests/ik_checker.py) alone reaches tol within
the cap on every convergence case."""
import numpy as np
import pytest

import ik_checker as ic
from conftest import load_task_model
from mj_envs_amd import _native, ik

SITE, BODY, COM = _native.AW_PT_SITE, _native.AW_PT_BODY, _native.AW_PT_BODYCOM
GOOD = dict(targets=[(SITE, 1, 1.0, 0.0)], dof_mask=0x3F, nv=36, nbody=30, nsite=20)


def check(**kw):
    a = {**GOOD, **kw}
    return _native.check_ik_args(a.pop("targets"), a.pop("dof_mask"), a.pop("nv"), a.pop("nbody"), a.pop("nsite"), **a)


def test_check_ik_args_accepts_and_counts_rows():
    assert check() == 3
    assert check(targets=[(SITE, 1, 1.0, 0.1), (BODY, 9, 0.0, 2.0), (COM, 29, 0.5, 0.0)]) == 12
    assert check(targets=[(BODY, k, 1.0, 0.0) for k in range(8)]) == 24          # the capacities themselves
    assert check(targets=[(BODY, k, 1.0, 1.0) for k in range(4)], max_iter=64, tol=0.0, max_step=0.05,
                 clamp_range=0, n_sel=1) == 24
    assert check(dof_mask=(1 << 63) | 1) == 3                                    # bits at or above nv are ignored
    assert check(max_iter=0, tol=float("inf"), max_step=-1.0) == 3


@pytest.mark.parametrize("name,kw,match", [
    ("no_targets", dict(targets=[]), "targets"),
    ("nine_targets", dict(targets=[(BODY, k, 1.0, 0.0) for k in range(9)]), "targets"),
    ("unknown_kind", dict(targets=[(3, 0, 1.0, 0.0)]), "kind"),
    ("negative_kind", dict(targets=[(-1, 0, 1.0, 0.0)]), "kind"),
    ("body_id_past_end", dict(targets=[(BODY, 30, 1.0, 0.0)]), "id"),
    ("com_id_negative", dict(targets=[(COM, -1, 1.0, 0.0)]), "id"),
    ("site_id_past_end", dict(targets=[(SITE, 20, 1.0, 0.0)]), "id"),
    ("negative_wpos", dict(targets=[(SITE, 1, -1.0, 0.0)]), "weight"),
    ("nan_wrot", dict(targets=[(SITE, 1, 1.0, float("nan"))]), "weight"),
    ("inf_wpos", dict(targets=[(SITE, 1, float("inf"), 0.0)]), "weight"),
    ("both_weights_zero", dict(targets=[(SITE, 1, 0.0, 0.0)]), "both weights 0"),
    ("27_rows", dict(targets=[(BODY, k, 1.0, 1.0) for k in range(4)] + [(SITE, 1, 1.0, 0.0)]), "rows"),
    ("mask_zero", dict(dof_mask=0), "dof_mask"),
    ("mask_above_nv", dict(dof_mask=1 << 36), "dof_mask"),
    ("mask_negative", dict(dof_mask=-1), "dof_mask"),
    ("max_iter_negative", dict(max_iter=-1), "max_iter"),
    ("max_iter_65", dict(max_iter=65), "max_iter"),
    ("damping_zero", dict(damping=0.0), "damping"),
    ("damping_negative", dict(damping=-1e-4), "damping"),
    ("damping_inf", dict(damping=float("inf")), "damping"),
    ("damping_nan", dict(damping=float("nan")), "damping"),
    ("tol_negative", dict(tol=-1e-9), "tol"),
    ("tol_nan", dict(tol=float("nan")), "tol"),
    ("max_step_inf", dict(max_step=float("inf")), "max_step"),
    ("max_step_nan", dict(max_step=float("nan")), "max_step"),
    ("clamp_range_2", dict(clamp_range=2), "clamp_range"),
    ("n_sel_zero", dict(n_sel=0), "n_sel"),
])
def test_check_ik_args_rejects(name, kw, match):
    with pytest.raises(ValueError, match=match):
        check(**kw)


def test_targets_on_relocate_and_pen():
    m = load_task_model("relocate-v0")
    t = ik.targets(m, sites=["S_grasp"])
    assert t.ik_records == [(SITE, 1, 1.0, 0.0)] and t.names == ["S_grasp"] and t.rows == 3 and len(t) == 1
    t = ik.targets(m, sites=[("S_grasp", 1.0, 0.1)], bodies=["ffdistal", 5], body_coms=["Object"], wpos=2.0)
    obj = m.name2id("body", "Object")
    assert t.ik_records == [(SITE, 1, 1.0, 0.1), (BODY, 9, 2.0, 0.0), (BODY, 5, 2.0, 0.0), (COM, obj, 2.0, 0.0)]
    assert t.names == ["S_grasp", "ffdistal", "palm", "Object:com"] and t.rows == 15
    assert t.index("palm") == 2 and t.index(3) == 3
    with pytest.raises(KeyError):
        t.index("thdistal")
    p = load_task_model("pen-v0")
    t = ik.targets(p, bodies=list(ic.TIPS), wpos=0.0, wrot=1.0)
    assert [r[:2] for r in t.ik_records] == [(BODY, p.name2id("body", b)) for b in ic.TIPS] and t.rows == 15
    assert all(r[2:] == (0.0, 1.0) for r in t.ik_records)
    with pytest.raises(KeyError):
        ik.targets(m, sites=["no_such_site"])
    with pytest.raises(ValueError, match="more than once"):
        ik.targets(m, bodies=["palm", 5])
    with pytest.raises(ValueError, match="both weights 0"):
        ik.targets(m, bodies=[("palm", 0.0, 0.0)])
    with pytest.raises(ValueError, match="rows"):
        ik.targets(m, bodies=list(ic.TIPS), wrot=1.0)                          # 30 rows
    with pytest.raises(ValueError, match="targets"):
        ik.targets(m, bodies=list(range(1, 10)))


def test_dof_mask_on_relocate_and_pen():
    m = load_task_model("relocate-v0")       # ARTx ARTy ARTz ARRx ARRy ARRz WRJ1 WRJ0 FFJ3..0 ... OBJ*
    assert ik.dof_mask(m, joints=["ARTx", "ARRz", 7]) == 0b10100001
    assert ik.dof_mask(m, chain="S_grasp") == 0xFF                              # the palm: arm and wrist
    assert ik.dof_mask(m, chain="ffdistal") == 0xFFF
    assert ik.dof_mask(m, chain="Object") == 0x3F << 30
    assert ik.dof_mask(m, actuated=True) == (1 << 30) - 1
    assert ik.dof_mask(m, joints=["OBJTx"], chain="palm") == 0xFF | 1 << 30
    p = load_task_model("pen-v0")            # WRJ1 WRJ0 FFJ3..0 MFJ3..0 RFJ3..0 LFJ4..0 THJ4..0 OBJ*
    assert ik.dof_mask(p, chain="S_grasp") == 0x3
    assert ik.dof_mask(p, chain="ffdistal") == 0x3F
    assert ik.dof_mask(p, chain="thdistal") == 0x3 | 0x1F << 19
    assert ik.dof_mask(p, actuated=True) == (1 << 24) - 1
    assert ic.case_spec("fingers", p)[1] == ((1 << 24) - 1) & ~0x3
    with pytest.raises(ValueError, match="no dof"):
        ik.dof_mask(m)
    with pytest.raises(KeyError):
        ik.dof_mask(m, joints=["no_such_joint"])
    # the chain is the device model's body_dofmask: the dofs dyn_checker's parent walk finds
    import dyn_checker as dc
    for b in (0, 5, 9, m.name2id("body", "Object")):
        assert ik.body_dofmask(m, b) == sum(1 << i for i, on in enumerate(dc.body_dofs(m, b)) if on)


@pytest.mark.parametrize("env_id", ["relocate-v0", "pen-v0"])
def test_qpos_to_actions_round_trip(env_id):
    """through the step's control map ctrl = act_mid + clip(a) act_rng: set-points inside the control
    range come back exactly as the joint positions, ones outside saturate at +-1"""
    import torch
    m = load_task_model(env_id)
    nq, nu = m.dims["nq"], m.dims["nu"]
    mid, rng_ = m.arrays["task_act_mid"], m.arrays["task_act_rng"]
    trn = np.asarray(m.arrays["actuator_trnid"]).astype(int).ravel()
    r = np.random.default_rng(0)
    a = r.uniform(-0.95, 0.95, (5, nu))
    q = r.normal(size=(5, nq))
    q[:, trn] = mid + a * rng_
    got = ik.qpos_to_actions(m, q)
    assert got.shape == (5, nu)
    np.testing.assert_allclose(got, a, atol=1e-12)
    np.testing.assert_allclose(mid + np.clip(got, -1, 1) * rng_, q[:, trn], atol=1e-12)
    far = q.copy()
    far[:, trn[0]] = mid[0] + 3 * rng_[0]
    far[:, trn[1]] = mid[1] - 3 * rng_[1]
    sat = ik.qpos_to_actions(m, far)
    assert (sat[:, 0] == 1).all() and (sat[:, 1] == -1).all()
    t = ik.qpos_to_actions(m, torch.as_tensor(q, dtype=torch.float32))
    assert t.dtype == torch.float32 and tuple(t.shape) == (5, nu)
    np.testing.assert_allclose(t.numpy(), a, atol=1e-5)


def test_solve_shape_checks():
    m = load_task_model("relocate-v0")
    t = ik.targets(m, sites=[("S_grasp", 1.0, 0.1)], bodies=["ffdistal"])
    ik.check_solve_args(t, 4, 36, (4, 2, 3), (4, 2, 4), (4, 36))
    with pytest.raises(ValueError, match="goal_pos is needed"):
        ik.check_solve_args(t, 4, 36, None, (4, 2, 4))
    with pytest.raises(ValueError, match="goal_quat is needed"):
        ik.check_solve_args(t, 4, 36, (4, 2, 3), None)
    with pytest.raises(ValueError, match="goal_pos must be"):
        ik.check_solve_args(t, 4, 36, (4, 1, 3), (4, 2, 4))
    with pytest.raises(ValueError, match="qpos0 must be"):
        ik.check_solve_args(t, 4, 36, (4, 2, 3), (4, 2, 4), (3, 36))
    ik.check_solve_args(ik.targets(m, sites=["S_grasp"]), 2, 36, (2, 1, 3))    # no orientation weight: no quaternion


def test_checker_pieces():
    """the checker's own algebra: mat2quat inverts the quaternion's matrix, rotvec is the rotation vector"""
    r = np.random.default_rng(1)
    for _ in range(20):
        q = r.normal(size=4)
        q /= np.linalg.norm(q)
        w, x, y, z = q
        R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                      [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                      [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]])
        p = ic.mat2quat(R)
        assert min(np.abs(p - q).max(), np.abs(p + q).max()) < 1e-12
    ax = np.array([1.0, 2.0, -2.0]) / 3
    for ang in (1e-9, 0.3, 3.0):
        d = np.concatenate([[np.cos(ang / 2)], np.sin(ang / 2) * ax])
        q0 = np.array([0.5, 0.5, -0.5, 0.5])
        np.testing.assert_allclose(ic.rotvec(ic.mulq(d, q0), q0), ang * ax, atol=1e-12)
        np.testing.assert_allclose(ic.rotvec(-ic.mulq(d, q0), q0), ang * ax, atol=1e-12)   # the sign of q is free
    assert not ic.rotvec(np.array([1.0, 0, 0, 0]), np.array([1.0, 0, 0, 0])).any()


@pytest.mark.parametrize("name", ic.CONVERGENCE)
def test_checker_converges_on_every_gpu_case(name):
    """the condition of test_gpu_ik.py's convergence test: on each of its cases the fp64 checker reaches
    tol within the cap in every env, takes more than one update to get there, and ends at the goals"""
    c = ic.case(name)
    r = ic.solve_batch(c["o"], c["m"], c["P"], c["q0"], c["targets"], c["goal"], c["mask"], max_iter=ic.CAP, tol=ic.TOL)
    print(name, "rows", ic.rows_of(c["targets"]), "iters", r["iters"].tolist(), "err", r["err"].tolist())
    assert (r["err"] <= ic.TOL).all() and (r["iters"] <= ic.CAP).all()
    assert (r["iters"] >= 2).all()                       # (the Jacobian is re-evaluated on the way)
    for t, (_, _, wp, wr) in enumerate(c["targets"]):
        if wp > 0:
            assert np.abs(r["point_pos"][:, t] - c["goal"][:, t, :3]).max() <= ic.TOL / wp
        if wr > 0:
            assert max(ic.quat_angle(c["goal"][e, t, 3:], r["point_quat"][e, t]) for e in range(4)) <= ic.TOL / wr
    free = np.array([(c["mask"] >> i) & 1 for i in range(c["o"].nv)], bool)
    np.testing.assert_array_equal(r["qpos"][:, ~free], c["q0"][:, ~free])


def test_one_update_floor_is_measurable():
    """the fp32 floor of one update (ik_checker.one_update_floor) on every one-update case: it holds its
    rounding-only part, lies below 1e-2 of the update -- the systems are conditioned well enough for an
    fp32 solve to mean something -- and on the door the envs differ by far more than the GPU test's bound"""
    for name in ic.CASES:
        d64, floor, rounding = ic.one_update_floor(name)
        print(f"{name}: max |dq| {np.abs(d64).max():.3f}, fp32 floor {floor:.2e}, rounding alone {rounding:.2e}")
        assert np.abs(d64).max() > 1e-2 and 0 < rounding <= floor < 1e-2
    d64, floor, _ = ic.one_update_floor("door-latch")     # the door frames differ, so the updates do
    assert np.abs(d64[0] - d64[1]).max() > 1000 * 4 * floor * np.abs(d64).max()


def test_kinematics_precision_term():
    """quantise: every entry within half a grid step of rel * max|a|, the array's own dtype kept"""
    a = np.random.default_rng(2).normal(size=(5, 3)).astype(np.float32)
    q = ic.quantise(a, ic.KIN_FP32)
    assert q.dtype == a.dtype and 0 < np.abs(q - a).max() <= 0.5 * ic.KIN_FP32 * np.abs(a).max() * (1 + 1e-3)
    assert ic.quantise(np.zeros(3), 1e-6).tolist() == [0, 0, 0]
