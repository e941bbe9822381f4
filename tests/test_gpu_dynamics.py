"""Dynamics queries on the GPU (aw_dynamics / k_dyn): against the fp64 checker (tests/dyn_checker.py)
on DAPG grasp states of all four tasks, against the existing forward hook, env selection, the state
override, the absence of side effects on the simulation, the ABI's errors, and a closed IK loop."""
import ctypes

import numpy as np
import pytest
import torch

import dyn_checker as dc
import sensor_states as ss
from conftest import load_task_model, make_oracle
from data_states import rel
from mj_envs_amd import _native

pytestmark = pytest.mark.gpu
ALL = _native.DYN_OUTPUTS
# the figures test_forward_internals_match_oracle holds each kind of quantity to
FIGURE = dict(point_pos=1e-5, jacp=1e-5, jacr=1e-5, qM=1e-4, xvel=1e-3, point_vel=1e-3, qfrc_bias=1e-3,
              qfrc_passive=1e-3, qfrc_actuator=1e-3, qMinv=1e-3)


def _t(a, dt=torch.float32):
    return torch.tensor(np.asarray(a), dtype=dt, device="cuda").contiguous()


def _sim(env_id, n, variation_type=None):
    m = load_task_model(env_id, variation_type)
    return m, _native.Sim(m.to_blob(), n)


def task_points(m, env_id):
    """a palm site, a fingertip body, the task's object body and its com, body 0"""
    obj = m.name2id("body", "latch" if env_id == "door-v0" else "Object")
    return [(dc.PT_SITE, m.name2id("site", "S_grasp")), (dc.PT_BODY, m.name2id("body", "ffdistal")),
            (dc.PT_BODY, obj), (dc.PT_BODYCOM, obj), (dc.PT_BODY, 0)]


def run(sim, pts, want=ALL, env_ids=None, qpos=None, qvel=None, ctrl=None, **kw):
    """one aw_dynamics launch into NaN-filled buffers of EVERY output (only ``want`` is handed to the
    library) -> name -> float64 numpy (exact copies of the fp32 values)"""
    ids = None if env_ids is None else _t(env_ids, torch.int32)
    n = sim.n_envs if ids is None else int(ids.shape[0])
    bufs = {k: torch.full((n,) + _native.dyn_shape(k, sim.nv, sim.nbody, len(pts)), float("nan"), device="cuda")
            for k in ALL}
    c = lambda a: None if a is None else _t(a)
    sim.dynamics({k: bufs[k] for k in want}, pts, env_ids=ids, qpos=c(qpos), qvel=c(qvel), ctrl=c(ctrl), **kw)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().astype(np.float64) for k, v in bufs.items()}


def set_states(sim, q, v, w, P):
    sim.set_state(_t(q), _t(v), _t(w), _t(P))


def get_state(sim):
    q, v = sim.empty(sim.n_envs, sim.nq), sim.empty(sim.n_envs, sim.nv)
    w, p = sim.empty(sim.n_envs, sim.nv), sim.empty(sim.n_envs, sim.nparam)
    sim.get_state(q, v, w, p)
    torch.cuda.synchronize()
    return [x.cpu().numpy() for x in (q, v, w, p)]


def dapg_case(env_id, k=1, mass=None):
    """(model, oracle, P, qpos, qvel, warm, act) of DAPG step k, 4 envs, rounded to fp32; mass: the
    hammer's per-env masses under variation_type="mass" """
    d = ss.dapg_states(env_id)
    m, o, P = d["m"], d["o"], d["P"]
    if mass is not None:
        m, o = make_oracle(env_id, "mass")
        P = np.concatenate([P, np.asarray(mass, float)[:, None]], axis=1)
    return m, o, ss.f32(P), ss.f32(d["qpos"][k]), ss.f32(d["qvel"][k]), ss.f32(d["warm"][k]), d["act"][k]


def ctrl_f32(m, act):
    """the step's control map in fp32, as the Python layer evaluates it"""
    a = np.clip(np.asarray(act, np.float32), -1, 1)
    return (m.task_act_mid.astype(np.float32) + a * m.task_act_rng.astype(np.float32)).astype(np.float64)


def check_against(got, o, m, P, q, v, ctrl, pts, tag):
    """every output within its figure (measured: qMinv 1.6e-4 at hammer's lightest mass, every other
    output below 1e-6 -- no output needs an fp32 floor)"""
    ref = dc.evaluate_batch(o, m, P, q, v, ctrl, pts)
    bad = []
    for k in ALL:
        r = rel(got[k], ref[k])
        print(f"{tag} {k}: rel {r:.2e} figure {FIGURE[k]:.0e}")
        assert np.isfinite(got[k]).all(), k
        if not r < FIGURE[k]:
            bad.append((k, r))
    assert not bad, bad


# 1 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id,mass,how", [("hammer-v0", None, None), ("hammer-v0", (0.3, 1.0, 1.7, 2.4), "ctrl"),
                                             ("door-v0", None, "ctrl"), ("pen-v0", None, "actions"),
                                             ("relocate-v0", None, "ctrl")])
def test_outputs_match_the_checker(env_id, mass, how):
    m, o, P, q, v, w, act = dapg_case(env_id, mass=mass)
    pts = task_points(m, env_id)
    if how == "actions":                       # through AdroitVecEnv: names, the control map, the result object
        from mj_envs_amd.dynamics import points
        from mj_envs_amd.envs import AdroitVecEnv
        env = AdroitVecEnv(env_id, 4, autoreset=False)
        env.set_state(_t(q), _t(v), _t(w), _t(P))
        obj = "Object"
        d = env.dynamics(points(env.model, sites=["S_grasp"], bodies=["ffdistal", obj, 0], body_coms=[obj]), want=ALL,
                         actions=_t(act))
        pts = d.points.records
        torch.cuda.synchronize()
        got = {k: d.tensors[k].cpu().numpy().astype(np.float64) for k in ALL}
        np.testing.assert_array_equal(d.jacp("Object:com").cpu().numpy(), got["jacp"][:, d.points.index("Object:com")])
        np.testing.assert_array_equal(d.vel("ffdistal").cpu().numpy(), got["point_vel"][:, 1])
        np.testing.assert_array_equal(d.body_vel("ffdistal").cpu().numpy(),
                                      got["xvel"][:, m.name2id("body", "ffdistal")])
        with pytest.raises(ValueError, match="give one"):
            env.dynamics(None, want=("qfrc_actuator",), actions=_t(act), ctrl=_t(act))
        d2 = env.dynamics(d.points, want=("jacp", "qM"), out=d)          # the buffers are reused
        assert d2.tensors["jacp"].data_ptr() == d.tensors["jacp"].data_ptr()
        ctrl = ctrl_f32(m, act)
        env.close()
    else:
        _, sim = _sim(env_id, 4, "mass" if mass is not None else None)
        set_states(sim, q, v, w, P)
        ctrl = ss.f32(ss.ctrl_of(m, act)) if how == "ctrl" else None
        got = run(sim, pts, ctrl=ctrl)
        if mass is not None:                   # the per-env params reach M
            assert rel(got["qM"][0], got["qM"][3]) > 1e-3
        sim.close()
    check_against(got, o, m, P, q, v, ctrl, pts, f"{env_id}{' mass' if mass is not None else ''}")
    world = list(pts).index((dc.PT_BODY, 0))               # body 0: zero Jacobians, zero velocity
    assert np.abs(got["point_vel"]).max() > 1e-3 and np.abs(got["jacp"]).max() > 0.1
    assert not got["jacp"][:, world].any() and not got["jacr"][:, world].any() and not got["point_vel"][:, world].any()
    np.testing.assert_array_equal(got["qM"], got["qM"].transpose(0, 2, 1))


@pytest.mark.parametrize("flags", [(1 << 6) | (1 << 5), (1 << 10), (1 << 7)])
def test_disable_flags_act_as_in_the_forward(flags):
    """aw_set_option's gravity | passive, actuation and clampctrl disable bits against the oracle with
    the same bits; the controls lie outside the ctrlrange so that the clamp matters"""
    env_id = "hammer-v0"
    m, _, P, q, v, w, act = dapg_case(env_id)
    _, o = make_oracle(env_id)                 # (an oracle of its own: the shared one keeps its options)
    o.set_option(disableflags=flags)
    _, sim = _sim(env_id, 4)
    sim.set_option(disableflags=flags)
    set_states(sim, q, v, w, P)
    ctrl = ss.f32(m.task_act_mid + 1.5 * np.sign(act + 1e-9) * m.task_act_rng)
    want = ("qfrc_bias", "qfrc_passive", "qfrc_actuator")
    got = run(sim, [], want=want, ctrl=ctrl)
    ref = dc.evaluate_batch(o, m, P, q, v, ctrl, [])
    for k in want:
        if np.abs(ref[k]).max() == 0:
            assert not got[k].any(), k
        else:
            assert rel(got[k], ref[k]) < FIGURE[k], (k, rel(got[k], ref[k]))
    zero = {(1 << 6) | (1 << 5): "qfrc_passive", 1 << 10: "qfrc_actuator"}.get(flags)
    assert zero is None or not got[zero].any()
    if flags == 1 << 7:                        # (the clamp matters: with it the actuator forces differ)
        sim.set_option(disableflags=0)
        assert rel(run(sim, [], want=want, ctrl=ctrl)["qfrc_actuator"], got["qfrc_actuator"]) > 1e-2
    sim.close()


# 2 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ["hammer-v0", "relocate-v0"])
def test_matches_the_forward_hook(env_id):
    """qM at the env's own state is aw_forward_dump's bit for bit; passive - bias + actuator is its
    qfrc_smooth to rel < 1e-6 (the same stage functions on the same values)"""
    m, o, P, q, v, w, act = dapg_case(env_id)
    _, sim = _sim(env_id, 4)
    set_states(sim, q, v, w, P)
    ctrl = ss.f32(ss.ctrl_of(m, act))
    got = run(sim, [], want=("qM", "qfrc_bias", "qfrc_passive", "qfrc_actuator"), ctrl=ctrl)
    for e in range(4):
        d = sim.forward_dump(e, ctrl=_t(ctrl[e]))
        np.testing.assert_array_equal(got["qM"][e], d["qM"])
        s = got["qfrc_passive"][e] - got["qfrc_bias"][e] + got["qfrc_actuator"][e]
        r = rel(s, d["qfrc_smooth"])
        print(f"{env_id} env {e}: rel(passive - bias + actuator, dump qfrc_smooth) = {r:.2e}")
        assert r < 1e-6
    sim.close()


# 3 ------------------------------------------------------------------------------------------------
def test_selection_sentinels_and_point_counts():
    env_id = "hammer-v0"
    m, o, P, q, v, w, act = dapg_case(env_id)
    _, _, P2, q2, v2, w2, _ = dapg_case(env_id, k=2)
    cat = lambda a, b: np.concatenate([a, b[:2]])
    _, sim = _sim(env_id, 6)
    set_states(sim, cat(q, q2), cat(v, v2), cat(w, w2), cat(P, P2))
    base = task_points(m, env_id)
    pts = [base[k % 5] for k in range(16)]              # the capacity, with repeated entries
    ctrl = np.tile(ss.f32(ss.ctrl_of(m, act)), (2, 1))[:6]
    full = run(sim, pts, ctrl=ctrl)
    for k in ALL:
        assert np.isfinite(full[k]).all(), k
    for k in _native.DYN_POINT_OUTPUTS:                 # equal blocks
        for p in range(5, 16):
            np.testing.assert_array_equal(full[k][:, p], full[k][:, p % 5])
    ids = [4, 1, 99, 1]
    sel = run(sim, pts, env_ids=ids, ctrl=ctrl[[4, 1, 0, 1]])
    for k in ALL:
        for row, e in ((0, 4), (1, 1), (3, 1)):
            np.testing.assert_array_equal(sel[k][row], full[k][e], err_msg=k)
        assert np.isnan(sel[k][2]).all(), k              # an id outside [0, N): the row is untouched
    assert rel(full["qM"][4], full["qM"][1]) > 1e-6      # (the rows do differ)
    part = run(sim, pts, want=("jacp", "qfrc_bias"), env_ids=ids)
    for k in ALL:
        if k in ("jacp", "qfrc_bias"):
            np.testing.assert_array_equal(part[k][[0, 1, 3]], full[k][[4, 1, 1]])
        else:
            assert np.isnan(part[k]).all(), k            # not requested: the sentinel everywhere
    only_m = run(sim, [], want=("qM",))                  # no points
    np.testing.assert_array_equal(only_m["qM"], full["qM"])
    assert np.isnan(only_m["qMinv"]).all()
    sim.close()


# 4 ------------------------------------------------------------------------------------------------
def test_state_override_reproduces_the_other_env():
    env_id = "relocate-v0"
    m, o, P, q, v, w, act = dapg_case(env_id)
    P = np.tile(P[0], (4, 1))                            # equal params
    _, sim = _sim(env_id, 4)
    set_states(sim, q, v, w, P)
    pts = task_points(m, env_id)
    ctrl = ss.f32(ss.ctrl_of(m, act))
    own = run(sim, pts, ctrl=ctrl)
    before = get_state(sim)
    perm = [1, 2, 3, 0]
    over = run(sim, pts, qpos=q[perm], qvel=v[perm], ctrl=ctrl[perm])
    for k in ALL:
        np.testing.assert_array_equal(over[k], own[k][perm], err_msg=k)
    half = run(sim, pts, qpos=q[perm])                   # qpos alone: the env's own qvel
    np.testing.assert_array_equal(half["point_pos"], own["point_pos"][perm])
    np.testing.assert_array_equal(half["qM"], own["qM"][perm])
    assert not np.array_equal(half["point_vel"], own["point_vel"][perm])
    for a, b in zip(before, get_state(sim)):
        np.testing.assert_array_equal(a, b)
    sim.close()


# 5 ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", [False, True])
def test_no_side_effects_on_the_simulation(extras):
    """two handles, the same state; one calls aw_dynamics (override, ctrl, every output) between two
    steps: obs, reward, flags, status, final state (and sensordata / data views) are bit-equal"""
    env_id = "hammer-v0"
    m, o, P, q, v, w, act = dapg_case(env_id)
    pts = task_points(m, env_id)
    res = []
    for call in (False, True):
        _, sim = _sim(env_id, 4)
        bufs = {}
        if extras:
            sim.set_sensors(True)
            bufs = sim.set_data(True, 16)
        set_states(sim, q, v, w, P)
        obs, rew = sim.empty(4, sim.obs_dim), sim.empty(4)
        done, goal = sim.empty(4, dtype=torch.uint8), sim.empty(4, dtype=torch.uint8)
        st = sim.empty(4, dtype=torch.int32)
        out = []
        for k in range(2):
            sim.step(_t(np.clip(act * (1 - 0.5 * k), -1, 1)), obs, rew, done, goal)
            sim.status(last=st)
            torch.cuda.synchronize()
            out += [x.cpu().numpy().copy() for x in (obs, rew, done, goal, st)]
            if extras:
                sd = sim.empty(4, sim.nsensordata)
                sim.sensordata(sd)
                out += [sd.cpu().numpy()] + [b.cpu().numpy().copy() for _, b in sorted(bufs.items())]
            if call and k == 0:
                r = run(sim, pts, qpos=q[::-1].copy(), qvel=v[::-1].copy(), ctrl=ss.f32(ss.ctrl_of(m, act)))
                assert all(np.isfinite(r[n]).all() for n in ALL)
        out += get_state(sim)
        res.append(out)
        sim.close()
    assert len(res[0]) == len(res[1])
    for a, b in zip(*res):
        np.testing.assert_array_equal(a, b)


# 6 ------------------------------------------------------------------------------------------------
def test_abi_errors_then_a_valid_call():
    env_id = "door-v0"
    m, sim = _sim(env_id, 3)
    obs = sim.empty(3, sim.obs_dim)
    sim.reset(obs, seed=3)
    L = _native.load()
    qM = torch.full((3, sim.nv, sim.nv), float("nan"), device="cuda")
    jp = torch.full((3, 1, 3, sim.nv), float("nan"), device="cuda")
    ids = _t([0, 1, 2], torch.int32)

    def call(h=sim.h, env_ids=None, n_sel=0, pts=((0, 1),), npoints=None, outs=None, null_out=False, null_pts=False):
        arr = (_native.DynPoint * max(len(pts), 1))()
        for k, (kind, idx) in enumerate(pts):
            arr[k].kind, arr[k].id = kind, idx
        c = _native.DynOut()
        for k, t in (dict(qM=qM, jacp=jp) if outs is None else outs).items():
            setattr(c, k, t.data_ptr())
        return L.aw_dynamics(h, env_ids, n_sel, None if null_pts else arr, len(pts) if npoints is None else npoints,
                             None, None, None, None if null_out else ctypes.byref(c), None)

    bad = dict(null_handle=dict(h=None), null_out=dict(null_out=True), no_output=dict(outs={}),
               npoints_negative=dict(npoints=-1), npoints_17=dict(pts=((0, 1),) * 17),
               null_points=dict(null_pts=True), point_output_without_points=dict(pts=(), outs=dict(jacp=jp)),
               unknown_kind=dict(pts=((3, 0),)), negative_kind=dict(pts=((-1, 0),)),
               body_id_past_end=dict(pts=((_native.AW_PT_BODY, sim.nbody),)),
               com_id_negative=dict(pts=((_native.AW_PT_BODYCOM, -1),)),
               site_id_past_end=dict(pts=((_native.AW_PT_SITE, sim.nsite),)),
               n_sel_zero=dict(env_ids=ids.data_ptr(), n_sel=0), n_sel_negative=dict(env_ids=ids.data_ptr(), n_sel=-2))
    for name, kw in bad.items():
        assert call(**kw) == -1, name                    # AW_EINVAL
        assert b"aw_dynamics" in L.aw_last_error(), name
    torch.cuda.synchronize()
    assert torch.isnan(qM).all() and torch.isnan(jp).all()
    assert call(env_ids=ids.data_ptr(), n_sel=3) == 0    # every other call still works
    assert call(pts=(), outs=dict(qM=qM)) == 0
    assert call(pts=((_native.AW_PT_SITE, sim.nsite - 1),)) == 0
    torch.cuda.synchronize()
    assert torch.isfinite(qM).all() and torch.isfinite(jp).all()
    with pytest.raises(_native.NativeError, match="npoints"):
        sim.dynamics(dict(qM=qM), [], npoints=17)
    rew, done, goal = sim.empty(3), sim.empty(3, dtype=torch.uint8), sim.empty(3, dtype=torch.uint8)
    sim.step(torch.zeros(3, sim.nu, device="cuda"), obs, rew, done, goal)
    torch.cuda.synchronize()
    assert torch.isfinite(obs).all()
    sim.close()


# 7 ------------------------------------------------------------------------------------------------
def dls_step(J, e, lam=1e-4):
    """dq = J^T (J J^T + lam I)^-1 e"""
    return J.T @ np.linalg.solve(J @ J.T + lam * np.eye(3), e)


def test_closed_loop_reach_with_the_qpos_override():
    """damped-least-squares IK on relocate's six arm dofs toward the palm site's position at a second,
    known configuration (reachable by construction), iterating on trial qpos rows only: the GPU loop
    reaches 1e-4 m within the CPU checker loop's iteration count + 2, and leaves the simulation alone"""
    env_id = "relocate-v0"
    m, o, P, q, v, w, act = dapg_case(env_id)
    arm = np.arange(6)
    pts = [(dc.PT_SITE, m.name2id("site", "S_grasp"))]
    q0 = q[0].copy()
    q1 = q0.copy()
    q1[arm] += np.array([0.10, 0.08, 0.12, 0.45, -0.40, 0.40])
    target = dc.evaluate(o, m, P[0], q1, v[0], None, pts)["point_pos"][0]
    TOL, CAP = 1e-4, 40

    def loop(query):
        qk = q0.copy()
        for it in range(CAP + 1):
            pos, J = query(qk)
            e = target - pos
            if np.linalg.norm(e) < TOL:
                return it, np.linalg.norm(e)
            qk[arm] += dls_step(J[:, arm], e)
        return CAP + 1, np.linalg.norm(e)

    def cpu(qk):
        r = dc.evaluate(o, m, P[0], qk, v[0], None, pts)
        return r["point_pos"][0], r["jacp"][0]

    k_ref, e_ref = loop(cpu)
    assert 2 <= k_ref <= CAP, (k_ref, e_ref)           # (several steps: the Jacobian is re-evaluated on the way)

    _, sim = _sim(env_id, 4)
    set_states(sim, q, v, w, P)
    before = get_state(sim)

    def gpu(qk):
        r = run(sim, pts, want=("point_pos", "jacp"), env_ids=[0], qpos=ss.f32(qk)[None])
        return r["point_pos"][0, 0], r["jacp"][0, 0]

    k_gpu, e_gpu = loop(gpu)
    print(f"IK: checker loop {k_ref} iterations (|e| {e_ref:.2e}), GPU loop {k_gpu} (|e| {e_gpu:.2e})")
    assert k_gpu <= k_ref + 2, (k_gpu, k_ref, e_gpu)
    for a, b in zip(before, get_state(sim)):
        np.testing.assert_array_equal(a, b)
    sim.close()


def test_facade_names():
    """mujoco-py's names on the single-env facade's env.data, in mujoco-py's shapes, equal to the
    batched call on the same state"""
    from mj_envs_amd.envs import RelocateEnvV0
    env = RelocateEnvV0()
    env.reset(seed=2)
    a = np.linspace(-0.5, 0.5, env.vec.nu)
    env.step(a)
    d = env.data
    nv = env.vec.nv
    jp, jr = d.get_site_jacp("S_grasp"), d.get_body_jacr("Object")
    assert jp.shape == (3 * nv,) and jr.shape == (3 * nv,) and jp.dtype == np.float64
    assert d.get_body_xvelp("palm").shape == (3,) and d.get_site_xvelr("S_grasp").shape == (3,)
    assert d.qfrc_bias.shape == (nv,) and d.qfrc_passive.shape == (nv,) and d.qM_full.shape == (nv, nv)
    from mj_envs_amd.dynamics import points
    ctrl = _t(ctrl_f32(env.model, a)[None])
    r = env.vec.dynamics(points(env.model, sites=["S_grasp"], bodies=["palm", "Object"]), want=ALL, ctrl=ctrl)
    c = lambda t: t[0].cpu().numpy().astype(np.float64)
    np.testing.assert_array_equal(jp, c(r.jacp("S_grasp")).ravel())
    np.testing.assert_array_equal(d.get_site_jacr("S_grasp"), c(r.jacr("S_grasp")).ravel())
    np.testing.assert_array_equal(d.get_body_jacp("Object"), c(r.jacp("Object")).ravel())
    np.testing.assert_array_equal(jr, c(r.jacr("Object")).ravel())
    np.testing.assert_array_equal(d.get_body_xvelp("palm"), c(r.vel("palm"))[3:])
    np.testing.assert_array_equal(d.get_body_xvelr("palm"), c(r.vel("palm"))[:3])
    np.testing.assert_array_equal(d.get_site_xvelp("S_grasp"), c(r.vel("S_grasp"))[3:])
    np.testing.assert_array_equal(d.qfrc_actuator, c(r.qfrc_actuator))
    np.testing.assert_array_equal(d.qM_full, c(r.qM))
    assert np.abs(d.qfrc_actuator).max() > 0
    env.reset(seed=3)                                    # zero controls again, as sim.reset() leaves data.ctrl
    r0 = env.vec.dynamics(None, want=("qfrc_actuator",))
    np.testing.assert_array_equal(env.data.qfrc_actuator, c(r0.qfrc_actuator))
    env.close()
