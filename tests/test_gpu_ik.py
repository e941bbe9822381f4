"""Inverse kinematics on the GPU (aw_solve_ik / k_ik): one update and whole solves against the fp64
checker (tests/ik_checker.py) on DAPG grasp states of all four tasks, max_iter = 0 against aw_dynamics,
the mask / limit / step options, env selection, the absence of side effects on the simulation, the
ABI's errors and the Python facades."""
import ctypes

import numpy as np
import pytest
import torch

import ik_checker as ic
import sensor_states as ss
from conftest import load_task_model
from mj_envs_amd import _native, ik

pytestmark = pytest.mark.gpu
POS_FIGURE = 1e-5          # what test_gpu_dynamics.py holds point_pos to (relative)
SENTINEL = -7              # iters of a row that was not written


def _t(a, dt=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dt, device="cuda").contiguous()


def sim_at(env_id, k=1, q=None):
    """a 4-env handle at DAPG step k (the params are the states' own), optionally with another qpos"""
    d = ss.dapg_states(env_id)
    sim = _native.Sim(load_task_model(env_id).to_blob(), 4)
    sim.set_state(_t(ss.f32(d["qpos"][k]) if q is None else q), _t(ss.f32(d["qvel"][k])), _t(ss.f32(d["warm"][k])),
                  _t(ss.f32(d["P"])))
    return sim


def run(sim, targets, goal, mask, env_ids=None, qpos0=None, want=_native.IK_OUTPUTS, **opt):
    """one aw_solve_ik launch into sentinel-filled buffers of every output -> name -> numpy (fp32 / int32)"""
    ids = None if env_ids is None else _t(env_ids, torch.int32)
    n = sim.n_envs if ids is None else int(ids.shape[0])
    bufs = {k: (torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda") if k == "iters" else
                torch.full((n,) + _native.ik_shape(k, sim.nq, len(targets)), float("nan"), device="cuda"))
            for k in _native.IK_OUTPUTS}
    sim.solve_ik({k: bufs[k] for k in want}, targets, _t(goal), mask, env_ids=ids,
                 qpos0=None if qpos0 is None else _t(qpos0), **opt)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in bufs.items()}


def run_case(c, sim=None, **opt):
    own = sim is None
    sim = sim_at(c["env_id"]) if own else sim
    r = run(sim, c["targets"], c["goal"], c["mask"], qpos0=c["q0"], **opt)
    if own:
        sim.close()
    return r


def at_returned_q(c, qpos):
    """the checker's poses and residual norm at the GPU's returned qpos (fp64 oracle forward)"""
    pos, quat, err = [], [], []
    for e in range(len(qpos)):
        p, q, _, _ = ic.evaluate(c["o"], c["m"], c["P"][e], qpos[e].astype(np.float64), c["targets"])
        pos.append(p)
        quat.append(q)
        err.append(np.linalg.norm(ic.residual(c["targets"], c["goal"][e], p, q, np.float64)))
    return np.stack(pos), np.stack(quat), np.array(err)


def check_outputs_at(c, r):
    """err, point_pos and point_quat belong to the returned qpos: point_pos to 1e-5 relative, the
    quaternion to the same figure up to sign; err inherits the rows' errors -- position rows wpos times
    the position error, orientation rows 2 wrot times the quaternion error, sqrt(m) rows"""
    pos, quat, err = at_returned_q(c, r["qpos"])
    fig_p = np.abs(r["point_pos"] - pos).max() / np.abs(pos).max()
    dq = np.minimum(np.abs(r["point_quat"] - quat).max(axis=-1), np.abs(r["point_quat"] + quat).max(axis=-1)).max()
    wp = max(t[2] for t in c["targets"])
    wr = max(t[3] for t in c["targets"])
    tol_err = POS_FIGURE * np.sqrt(ic.rows_of(c["targets"])) * max(wp * np.abs(pos).max(), 2 * wr)
    fig_e = np.abs(r["err"] - err).max()
    print(f"  at the returned q: point_pos rel {fig_p:.2e}, point_quat {dq:.2e} (figure {POS_FIGURE:.0e}), "
          f"|err - checker| {fig_e:.2e} (bound {tol_err:.2e})")
    assert fig_p < POS_FIGURE and dq < POS_FIGURE and fig_e < tol_err


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ic.CASES))
def test_one_update_matches_the_checker(name):
    """max_iter = 1, no step limit, no clamp: qpos - qpos0 against the fp64 checker, each case held to 4 x
    ITS OWN fp32 floor (ik_checker.one_update_floor: the checker in float32 from kinematics of fp32
    precision, KIN_FP32 = 1.9e-6 relative, against the checker in float64; the part that is rounding of
    the solve alone is printed next to it).  Floors (CPU) -> bounds, and the GPU's figures (MI355X):
    relocate-arm 1.2e-6 -> 4.9e-6, relocate-hand21 7.7e-4 -> 3.1e-3, pen-fingers 6.0e-5 -> 2.4e-4,
    hammer-palm 9.6e-6 -> 3.8e-5, door-latch 1.5e-5 -> 6.0e-5; GPU 1.0e-6, 4.7e-4, 7.7e-6, 5.6e-6, 1.5e-5."""
    c = ic.case(name)
    d64, floor, rounding = ic.one_update_floor(name)
    r = run_case(c, **ic.ONE_UPDATE)
    got = r["qpos"].astype(np.float64) - c["q0"]
    fig = ic.update_error(got, d64)
    print(f"{name}: rows {ic.rows_of(c['targets'])}, max |dq| {np.abs(d64).max():.3f}, GPU figure {fig:.2e}, "
          f"floor {floor:.2e} (rounding alone {rounding:.2e}), bound {4 * floor:.2e}")
    assert (r["iters"] == 1).all() and np.isfinite(r["qpos"]).all()
    assert fig <= 4 * floor
    free = np.array([(c["mask"] >> i) & 1 for i in range(r["qpos"].shape[1])], bool)
    np.testing.assert_array_equal(r["qpos"][:, ~free], c["q0"][:, ~free].astype(np.float32))
    check_outputs_at(c, r)
    if name == "door-latch":     # two envs, the same start and goal, different door frames: different updates
        # (by far more than the bound lets either differ from the checker run with its own params)
        assert np.abs(got[0] - got[1]).max() > 100 * 4 * floor * np.abs(d64).max()
        assert np.abs(c["P"][0] - c["P"][1]).max() > 1e-3


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ic.CONVERGENCE)
def test_convergence(name):
    c = ic.case(name)
    ref = ic.solve_batch(c["o"], c["m"], c["P"], c["q0"], c["targets"], c["goal"], c["mask"], max_iter=ic.CAP, tol=ic.TOL)
    r = run_case(c, max_iter=ic.CAP, tol=ic.TOL)
    print(f"{name}: checker iterations {ref['iters'].tolist()}, GPU {r['iters'].tolist()}, GPU err {r['err'].tolist()}")
    assert (r["err"] <= ic.TOL).all()
    assert (r["iters"] <= ref["iters"] + 2).all()
    # independently: the oracle's forward at the GPU's qpos puts every weighted point at its goal
    pos, quat, _ = at_returned_q(c, r["qpos"])
    for t, (_, _, wp, wr) in enumerate(c["targets"]):
        for e in range(4):
            g = c["goal"][e, t]
            if wp > 0:
                assert np.linalg.norm(pos[e, t] - g[:3]) <= ic.TOL + 1e-5 * max(1.0, np.linalg.norm(g[:3])), (t, e)
            if wr > 0:
                assert ic.quat_angle(g[3:] / np.linalg.norm(g[3:]), quat[e, t]) <= ic.TOL / wr + 1e-5, (t, e)
    check_outputs_at(c, r)
    free = np.array([(c["mask"] >> i) & 1 for i in range(r["qpos"].shape[1])], bool)
    np.testing.assert_array_equal(r["qpos"][:, ~free], c["q0"][:, ~free].astype(np.float32))   # 4: the mask


# 3 ------------------------------------------------------------------------------------------------
def test_max_iter_zero():
    c = ic.case("relocate-hand21")
    sim = sim_at(c["env_id"])
    stored = sim.empty(4, sim.nq)
    sim.get_state(qpos=stored)
    pts = [(k, i) for k, i, _, _ in c["targets"]]
    for q0 in (c["q0"][::-1].copy(), None):
        r = run(sim, c["targets"], c["goal"], c["mask"], qpos0=q0, max_iter=0)
        start = stored.cpu().numpy() if q0 is None else q0.astype(np.float32)
        np.testing.assert_array_equal(r["qpos"], start)
        assert (r["iters"] == 0).all() and np.isfinite(r["err"]).all() and (r["err"] > ic.TOL).all()
        pp = torch.full((4, len(pts), 3), float("nan"), device="cuda")
        sim.dynamics(dict(point_pos=pp), pts, qpos=None if q0 is None else _t(q0))
        torch.cuda.synchronize()
        np.testing.assert_array_equal(r["point_pos"], pp.cpu().numpy())
    sim.close()


# 4 ------------------------------------------------------------------------------------------------
def test_limits_steps_and_a_nan_goal():
    c = ic.case("relocate-arm")
    sim = sim_at(c["env_id"])
    m = c["m"]
    free = np.array([(c["mask"] >> i) & 1 for i in range(sim.nq)], bool)
    far = c["goal"].copy()
    far[:, :, 0] += 2.0                                   # 2 m away: out of reach
    r = run(sim, c["targets"], far, c["mask"], qpos0=c["q0"], max_iter=10, clamp_range=True)
    assert (r["iters"] == 10).all() and (r["err"] > ic.TOL).all()
    assert all(np.isfinite(r[k]).all() for k in ("qpos", "err", "point_pos", "point_quat"))
    rng = np.asarray(m.arrays["jnt_range"]).reshape(-1, 2).astype(np.float32)
    sel = free & np.asarray(m.arrays["jnt_limited"]).astype(bool)
    assert sel.any() and (r["qpos"][:, sel] >= rng[sel, 0]).all() and (r["qpos"][:, sel] <= rng[sel, 1]).all()
    assert ((r["qpos"][:, sel] == rng[sel, 0]) | (r["qpos"][:, sel] == rng[sel, 1])).any()    # (the clamp acted)
    np.testing.assert_array_equal(r["qpos"][:, ~free], c["q0"][:, ~free].astype(np.float32))
    s = run(sim, c["targets"], far, c["mask"], qpos0=c["q0"], max_iter=10, max_step=0.05, clamp_range=False)
    moved = np.abs(s["qpos"].astype(np.float64) - c["q0"])
    assert (s["iters"] == 10).all() and (moved <= 10 * 0.05 * (1 + 1e-6)).all() and moved.max() > 0.05
    # a NaN goal in one row: that row stops at once, the others are bitwise what they are without it
    base = run(sim, c["targets"], c["goal"], c["mask"], qpos0=c["q0"], max_iter=ic.CAP)
    bad = c["goal"].copy()
    bad[1, 0, 1] = np.nan
    r = run(sim, c["targets"], bad, c["mask"], qpos0=c["q0"], max_iter=ic.CAP)
    assert r["iters"][1] == 0 and np.isnan(r["err"][1])
    np.testing.assert_array_equal(r["qpos"][1], c["q0"][1].astype(np.float32))
    for k in _native.IK_OUTPUTS:
        np.testing.assert_array_equal(r[k][[0, 2, 3]], base[k][[0, 2, 3]], err_msg=k)
    sim.close()


# 5 ------------------------------------------------------------------------------------------------
def test_selection():
    c = ic.case("relocate-hand21")
    sim = sim_at(c["env_id"])
    opt = dict(max_iter=5, tol=0.0)
    full = run(sim, c["targets"], c["goal"], c["mask"], qpos0=c["q0"], **opt)
    rows = [2, 0, 2, 0]                                   # qpos0 and goal by OUTPUT ROW; row 3's id is no env
    sel = run(sim, c["targets"], c["goal"][rows], c["mask"], env_ids=[2, 0, 2, 99], qpos0=c["q0"][rows], **opt)
    for k in _native.IK_OUTPUTS:
        np.testing.assert_array_equal(sel[k][:3], full[k][[2, 0, 2]], err_msg=k)
        assert (sel[k][3] == SENTINEL) if k == "iters" else np.isnan(sel[k][3]).all(), k
    assert not np.array_equal(full["qpos"][0], full["qpos"][2])                   # (the rows do differ)
    part = run(sim, c["targets"], c["goal"], c["mask"], qpos0=c["q0"], want=("qpos", "iters"), **opt)
    np.testing.assert_array_equal(part["qpos"], full["qpos"])                     # the optional outputs are optional
    np.testing.assert_array_equal(part["iters"], full["iters"])
    assert np.isnan(part["err"]).all() and np.isnan(part["point_pos"]).all() and np.isnan(part["point_quat"]).all()
    sim.close()


# 6 ------------------------------------------------------------------------------------------------
def test_no_side_effects_on_the_simulation():
    """two handles at the same state; one solves (start override, every output) before a step: its
    state is bitwise unchanged by the call, and the step's obs, reward and final state equal the twin's"""
    c = ic.case("relocate-hand21")
    d = ss.dapg_states(c["env_id"])
    act = _t(np.clip(d["act"][1], -1, 1))
    res = []
    for call in (False, True):
        sim = sim_at(c["env_id"])

        def state():
            bufs = [sim.empty(4, sim.nq), sim.empty(4, sim.nv), sim.empty(4, sim.nv), sim.empty(4, sim.nparam)]
            sim.get_state(*bufs)
            torch.cuda.synchronize()
            return [b.cpu().numpy() for b in bufs]

        before = state()
        if call:
            r = run(sim, c["targets"], c["goal"], c["mask"], qpos0=c["q0"][::-1].copy(), max_iter=8)
            assert np.isfinite(r["qpos"]).all() and (r["iters"] > 0).all()
            for a, b in zip(before, state()):
                np.testing.assert_array_equal(a, b)
        obs, rew = sim.empty(4, sim.obs_dim), sim.empty(4)
        done, goal = sim.empty(4, dtype=torch.uint8), sim.empty(4, dtype=torch.uint8)
        sim.step(act, obs, rew, done, goal)
        torch.cuda.synchronize()
        res.append([obs.cpu().numpy(), rew.cpu().numpy()] + state())
        sim.close()
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


# 7 ------------------------------------------------------------------------------------------------
def test_abi_errors_then_a_valid_call():
    m = load_task_model("door-v0")
    sim = _native.Sim(m.to_blob(), 3)
    obs = sim.empty(3, sim.obs_dim)
    sim.reset(obs, seed=3)
    L = _native.load()
    qp = torch.full((3, sim.nq), float("nan"), device="cuda")
    goal = torch.zeros(3, 9, 7, device="cuda")
    goal[..., 3] = 1
    ids = _t([0, 1, 2], torch.int32)
    S, B = _native.AW_PT_SITE, _native.AW_PT_BODY
    nan, inf = float("nan"), float("inf")

    def call(h=sim.h, env_ids=None, n_sel=0, tg=((S, 0, 1.0, 0.0),), ntargets=None, mask=0x3F, opt=(20, 1e-4, 1e-4, 0.0, 1),
             null=()):
        arr = (_native.IKTarget * max(len(tg), 1))(*[_native.IKTarget(*t) for t in tg])
        o = _native.IKOut()
        if "qpos" not in null:
            o.qpos = qp.data_ptr()
        op = _native.IKOpt(*opt)
        return L.aw_solve_ik(h, env_ids, n_sel, None if "targets" in null else arr, len(tg) if ntargets is None else ntargets,
                             mask, None if "goal" in null else goal.data_ptr(), None,
                             None if "opt" in null else ctypes.byref(op), None if "out" in null else ctypes.byref(o), None)

    bad = dict(null_handle=dict(h=None), null_targets=dict(null=("targets",)), null_goal=dict(null=("goal",)),
               null_opt=dict(null=("opt",)), null_out=dict(null=("out",)), null_qpos=dict(null=("qpos",)),
               ntargets_zero=dict(ntargets=0), ntargets_negative=dict(ntargets=-1), ntargets_9=dict(tg=((B, 1, 1.0, 0.0),) * 9),
               unknown_kind=dict(tg=((3, 0, 1.0, 0.0),)), negative_kind=dict(tg=((-1, 0, 1.0, 0.0),)),
               body_id_past_end=dict(tg=((B, sim.nbody, 1.0, 0.0),)), site_id_negative=dict(tg=((S, -1, 1.0, 0.0),)),
               site_id_past_end=dict(tg=((S, sim.nsite, 1.0, 0.0),)),
               negative_weight=dict(tg=((S, 0, -1.0, 0.0),)), nan_weight=dict(tg=((S, 0, 1.0, nan),)),
               inf_weight=dict(tg=((S, 0, inf, 0.0),)), both_weights_zero=dict(tg=((S, 0, 0.0, 0.0),)),
               rows_27=dict(tg=((B, 1, 1.0, 1.0),) * 4 + ((S, 0, 1.0, 0.0),)),
               mask_zero=dict(mask=0), mask_above_nv=dict(mask=1 << sim.nv),
               max_iter_negative=dict(opt=(-1, 1e-4, 1e-4, 0.0, 1)), max_iter_65=dict(opt=(65, 1e-4, 1e-4, 0.0, 1)),
               damping_zero=dict(opt=(20, 0.0, 1e-4, 0.0, 1)), damping_negative=dict(opt=(20, -1.0, 1e-4, 0.0, 1)),
               damping_nan=dict(opt=(20, nan, 1e-4, 0.0, 1)), damping_inf=dict(opt=(20, inf, 1e-4, 0.0, 1)),
               tol_negative=dict(opt=(20, 1e-4, -1e-6, 0.0, 1)), tol_nan=dict(opt=(20, 1e-4, nan, 0.0, 1)),
               max_step_nan=dict(opt=(20, 1e-4, 1e-4, nan, 1)), max_step_inf=dict(opt=(20, 1e-4, 1e-4, inf, 1)),
               clamp_range_2=dict(opt=(20, 1e-4, 1e-4, 0.0, 2)), clamp_range_negative=dict(opt=(20, 1e-4, 1e-4, 0.0, -1)),
               n_sel_zero=dict(env_ids=ids.data_ptr(), n_sel=0), n_sel_negative=dict(env_ids=ids.data_ptr(), n_sel=-2))
    for name, kw in bad.items():
        assert call(**kw) == -1, name                    # AW_EINVAL
        assert b"aw_solve_ik" in L.aw_last_error(), name
    torch.cuda.synchronize()
    assert torch.isnan(qp).all()
    assert call() == 0                                   # every other call still works
    assert call(env_ids=ids.data_ptr(), n_sel=3, tg=((B, 1, 1.0, 1.0),) * 4, mask=(1 << 63) | 1, opt=(64, 1e-4, 0.0, 0.05, 0)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(qp).all()
    with pytest.raises(ValueError, match="max_iter"):    # the binding refuses on the host what the library would
        sim.solve_ik(dict(qpos=qp), [(S, 0, 1.0, 0.0)], goal[:, :1].contiguous(), 0x3F, max_iter=65)
    rew, done, gl = sim.empty(3), sim.empty(3, dtype=torch.uint8), sim.empty(3, dtype=torch.uint8)
    sim.step(torch.zeros(3, sim.nu, device="cuda"), obs, rew, done, gl)
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all()
    sim.close()


# 8 ------------------------------------------------------------------------------------------------
def test_facades():
    from mj_envs_amd.dynamics import points
    from mj_envs_amd.envs import AdroitVecEnv, RelocateEnvV0
    c = ic.case("relocate-hand21")
    d = ss.dapg_states(c["env_id"])
    env = AdroitVecEnv(c["env_id"], 4, autoreset=False)
    env.set_state(_t(c["q0"]), _t(ss.f32(d["qvel"][1])), _t(ss.f32(d["warm"][1])), _t(c["P"]))
    tg = ik.targets(env.model, sites=[("S_grasp", 1.0, 0.1)], bodies=list(ic.TIPS))
    assert tg.ik_records == list(c["targets"])
    gp, gq = _t(c["goal"][:, :, :3]), _t(c["goal"][:, :, 3:])
    res = env.solve_ik(tg, goal_pos=gp, goal_quat=gq, max_iter=ic.CAP, tol=ic.TOL)     # dofs None: every actuated dof
    torch.cuda.synchronize()
    raw = run(env.sim, c["targets"], c["goal"], c["mask"], max_iter=ic.CAP, tol=ic.TOL)
    for k in _native.IK_OUTPUTS:
        np.testing.assert_array_equal(res.tensors[k].cpu().numpy(), raw[k], err_msg=k)
    assert res.converged.all() and res.converged.dtype == torch.bool
    np.testing.assert_array_equal(res.pos("ffdistal").cpu().numpy(), raw["point_pos"][:, 1])
    np.testing.assert_array_equal(res.quat("S_grasp").cpu().numpy(), raw["point_quat"][:, 0])
    res2 = env.solve_ik(tg, goal_pos=gp[[3, 1]], goal_quat=gq[[3, 1]], dofs=ik.dof_mask(env.model, actuated=True),
                        env_ids=[3, 1], qpos0=_t(c["q0"][[3, 1]]), out=res, max_iter=ic.CAP)
    assert res2.tensors["qpos"].data_ptr() != res.tensors["qpos"].data_ptr()           # [2, nq]: another shape
    np.testing.assert_array_equal(res2.qpos.cpu().numpy(), raw["qpos"][[3, 1]])
    with pytest.raises(ValueError, match="goal_pos must be"):
        env.solve_ik(tg, goal_pos=gp, goal_quat=gq, env_ids=[3, 1])
    res3 = env.solve_ik(tg, goal_pos=gp, goal_quat=gq, out=res, max_iter=ic.CAP, tol=ic.TOL)
    assert all(res3.tensors[k].data_ptr() == res.tensors[k].data_ptr() for k in _native.IK_OUTPUTS)   # reused
    with pytest.raises(TypeError, match="unknown options"):
        env.solve_ik(tg, goal_pos=gp, goal_quat=gq, iterations=3)
    # the solution, made the state of two envs: aw_dynamics shows the points at the goals
    env.set_state(qpos=res3.qpos[[1, 2]].contiguous(), env_ids=[1, 2])
    dyn = env.dynamics(points(env.model, sites=["S_grasp"], bodies=list(ic.TIPS)), want=("point_pos",))
    torch.cuda.synchronize()
    pp = dyn.point_pos.cpu().numpy().astype(np.float64)
    for e in (1, 2):
        for t in range(len(tg)):
            g = c["goal"][e, t, :3]
            assert np.linalg.norm(pp[e, t] - g) <= ic.TOL + POS_FIGURE * max(1.0, np.linalg.norm(g)), (e, t)
    a = ik.qpos_to_actions(env.model, res3.qpos)
    assert tuple(a.shape) == (4, env.nu) and a.is_cuda and float(a.abs().max()) <= 1.0
    env.close()
    one = RelocateEnvV0()
    one.reset(seed=2)
    t1 = ik.targets(one.model, sites=["S_grasp"])
    st = one.vec.get_state()
    base = one.vec.dynamics(points(one.model, sites=["S_grasp"]), want=("point_pos",)).point_pos[0, 0].cpu().numpy()
    out = one.solve_ik(t1, goal_pos=(base + np.array([0.03, 0.02, 0.04]))[None], dofs=0x3F)
    assert out["qpos"].shape == (one.vec.nq,) and out["qpos"].dtype == np.float64 and out["converged"]
    assert out["err"] <= 1e-4 and 1 <= out["iters"] <= 20 and out["point_pos"].shape == (1, 3)
    for k, v in one.vec.get_state().items():
        np.testing.assert_array_equal(v.cpu().numpy(), st[k].cpu().numpy())
    one.close()
