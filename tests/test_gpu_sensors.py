"""MuJoCo sensordata on device (aw_set_sensors / aw_sensordata) against the fp64 oracle, on the
DAPG-driven states of tests/sensor_states.py (4 tasks x 3 env-steps x 4 envs; the CPU test
tests/test_sensors.py asserts that those inputs are well conditioned in the reference itself).

Tolerances, from identical fp32 inputs:
  * jointpos: |err| <= 2e-5 + 1e-5 |q| -- what the suite holds the step's obs, and so qpos, to
    (tests/test_gpu_parity.py test_reset_obs_matches_oracle_all_tasks).
  * actuatorfrc: |err| <= 2e-5 max(1, |biasprm[1]|) + 1e-4 |f|: the qpos tolerance through the
    actuator's position gain (the arm actuators are 500 ctrl - 200 q).
  * touch: |err| <= 2e-3 + 2e-3 |f| N, the tolerance the suite holds constraint quantities to
    (test_gpu_parity.py: efc_aref); a pad is a miss outside that, or when it is on in one and off in
    the other while the oracle reads more than 2e-3 N; misses <= 5 % of a task's firing cases.
"""
import functools

import numpy as np
import pytest

from conftest import ENVS
import sensor_states as ss

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TOUCH_RTOL, TOUCH_ATOL = 2e-3, 2e-3


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _t(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype or torch.float32, device="cuda")


def _sim(d, n, sensors=True):
    from mj_envs_amd import _native
    sim = _native.Sim(d["m"].to_blob(), n)
    if sensors:
        sim.set_sensors(True)
    return sim


def _bufs(sim, n):
    return (sim.empty(n, sim.obs_dim), sim.empty(n), sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8))


def _sens(sim):
    out = sim.sensordata(sim.empty(sim.n_envs, sim.nsensordata))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _set(sim, d, k, rows=slice(None)):
    sim.set_state(_t(d["qpos"][k][rows]), _t(d["qvel"][k][rows]), _t(d["warm"][k][rows]), _t(d["P"][rows]))


@functools.lru_cache(maxsize=None)
def gpu_results(env_id, tier=0):
    """per chosen env-step: sensordata after set_state alone (fwd) and after one more aw_step (step)"""
    d = ss.dapg_states(env_id)
    n = ss.N_ENVS
    sim = _sim(d, n)
    sim.set_tier(tier)
    obs, rew, done, goal = _bufs(sim, n)
    fwd, step, status = [], [], []
    for k in range(len(d["steps"])):
        _set(sim, d, k)
        fwd.append(_sens(sim))
        sim.step(_t(d["act"][k]), obs, rew, done, goal)
        step.append(_sens(sim))
        st = sim.empty(n, dtype=torch.int32)
        sim.status(last=st)
        status.append(st.cpu().numpy())
    sim.close()
    return dict(fwd=fwd, step=step, status=status)


def _columns(m):
    types, objs = ss.sensor_layout(m)
    return {t: np.flatnonzero(types == t) for t in (ss.SENS_TOUCH, ss.SENS_JOINTPOS, ss.SENS_ACTUATORFRC)}, objs


def _check_smooth(m, got, ref, what):
    cols, objs = _columns(m)
    jc, ac = cols[ss.SENS_JOINTPOS], cols[ss.SENS_ACTUATORFRC]
    ej = np.abs(got[..., jc] - ref[..., jc])
    print(f"{what}: jointpos max |err| {ej.max():.2e}")
    assert (ej <= 2e-5 + 1e-5 * np.abs(ref[..., jc])).all(), what
    gain = np.abs(m.arrays["actuator_biasprm"].reshape(-1, 3)[objs[ac], 1])
    ea = np.abs(got[..., ac] - ref[..., ac])
    bound = 2e-5 * np.maximum(1.0, gain) + 1e-4 * np.abs(ref[..., ac])
    print(f"{what}: actuatorfrc max |err| / bound {(ea / bound).max():.3f}")
    assert (ea <= bound).all(), what


def _touch_misses(m, got, ref):
    tc = _columns(m)[0][ss.SENS_TOUCH]
    g, r = got[..., tc], ref[..., tc]
    out = np.abs(g - r) > TOUCH_ATOL + TOUCH_RTOL * np.abs(r)
    flip = ((g > 0) != (r > 0)) & (r > TOUCH_ATOL)
    firing = r > 0
    relerr = np.abs(g - r)[firing] / r[firing] if firing.any() else np.zeros(1)
    return int((out | flip).sum()), int(firing.sum()), relerr


@pytest.mark.parametrize("env_id", ENVS)
def test_step_sensordata_vs_oracle(env_id):
    """teacher-forced: aw_set_state with the oracle's state, one aw_step with the same action"""
    d = ss.dapg_states(env_id)
    got, ref = np.stack(gpu_results(env_id)["step"]), np.stack(d["sens_f32"])
    assert got.shape == ref.shape == (3, ss.N_ENVS, d["m"].nsensor)
    _check_smooth(d["m"], got, ref, f"step {env_id}")
    miss, firing, relerr = _touch_misses(d["m"], got, ref)
    print(f"step {env_id}: touch misses {miss} of {firing} firing cases; relative error of the firing pads: "
          f"median {np.median(relerr):.2e} p90 {np.quantile(relerr, 0.9):.2e} max {relerr.max():.2e}")
    assert firing >= 20
    assert miss <= 0.05 * firing


@pytest.mark.parametrize("env_id", ENVS)
def test_set_state_forward_sensordata_vs_oracle(env_id):
    d = ss.dapg_states(env_id)
    got, ref = np.stack(gpu_results(env_id)["fwd"]), np.stack(d["fwd_f32"])
    _check_smooth(d["m"], got, ref, f"set_state {env_id}")
    miss, firing, relerr = _touch_misses(d["m"], got, ref)
    print(f"set_state {env_id}: touch misses {miss} of {firing} firing cases, max relative error {relerr.max():.2e}")
    assert miss <= 0.05 * firing


@pytest.mark.parametrize("env_id", ENVS)
def test_reset_sensordata(env_id):
    """aw_reset with explicit params: jointpos is qpos0 exactly, touch the oracle's reset forward"""
    d = ss.dapg_states(env_id)
    m, o, n = d["m"], d["o"], ss.N_ENVS
    sim = _sim(d, n)
    assert not _sens(sim).any()                # zero until the first step / reset / set_state
    P = ss.f32(d["P"])
    sim.reset(None, params=_t(P))
    got = _sens(sim)
    cols, _ = _columns(m)
    qpos0 = m.arrays["qpos0"]
    jnt = ss.sensor_layout(m)[1][cols[ss.SENS_JOINTPOS]]
    np.testing.assert_array_equal(got[:, cols[ss.SENS_JOINTPOS]], np.tile(qpos0[jnt].astype(np.float32), (n, 1)))
    st, _ = o.reset(P)
    ref = np.stack([ss.oracle_forward_sensors(o, P[e], st["qpos"][e], st["qvel"][e], st["warm"][e]) for e in range(n)])
    _check_smooth(m, got, ref, f"reset {env_id}")
    tc = cols[ss.SENS_TOUCH]
    np.testing.assert_allclose(got[:, tc], ref[:, tc], rtol=TOUCH_RTOL, atol=TOUCH_ATOL)
    sim.close()


def test_hammer_nail_sensor_is_the_observation_input():
    """sensordata[S_nail] clipped to [-1, 1] is the obs entry, bit for bit, where the nail is struck"""
    found = ss.first_nail_state()
    assert found is not None
    m, P, q, v, w, act, t, e, adr = found
    n = ss.N_ENVS
    from mj_envs_amd import _native
    sim = _native.Sim(m.to_blob(), n)
    sim.set_sensors(True)
    obs, rew, done, goal = _bufs(sim, n)
    sim.set_state(_t(q), _t(v), _t(w), _t(P))
    sim.step(_t(act), obs, rew, done, goal)
    sd = _sens(sim)
    o = obs.cpu().numpy()
    print(f"S_nail after env-step {t}: sensordata {sd[:, adr]}, obs {o[:, m.nq + 12]}")
    np.testing.assert_array_equal(np.clip(sd[:, adr], np.float32(-1), np.float32(1)), o[:, m.nq + 12])
    sim.close()


@pytest.mark.parametrize("env_id", ENVS)
def test_sensors_have_no_side_effects(env_id):
    """sensors on against off, 3 steps from the same state: everything else bitwise equal"""
    d = ss.dapg_states(env_id)
    n = ss.N_ENVS
    outs = []
    for on in (False, True):
        sim = _sim(d, n, sensors=on)
        obs, rew, done, goal = _bufs(sim, n)
        _set(sim, d, 0)
        rec = []
        for k in range(3):
            sim.step(_t(d["act"][k]), obs, rew, done, goal)
            q, v, w = sim.empty(n, sim.nq), sim.empty(n, sim.nv), sim.empty(n, sim.nv)
            sim.get_state(q, v, w)
            torch.cuda.synchronize()
            rec.append([x.cpu().numpy().copy() for x in (obs, rew, done, goal, q, v, w)])
        outs.append(rec)
        sim.close()
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))


@pytest.mark.parametrize("env_id", ENVS)
def test_wide_tier_sensordata_bitwise(env_id):
    """every forward re-run by the wide tier (aw_set_tier 1) writes the automatic tier's bits"""
    a, w = gpu_results(env_id, 0), gpu_results(env_id, 1)
    from mj_envs_amd import _native
    assert all((s & _native.ST_WIDE).all() for s in w["status"]) and not any((s & _native.ST_WIDE).any() for s in a["status"])
    for key in ("fwd", "step"):
        for x, y in zip(a[key], w[key]):
            np.testing.assert_array_equal(x.view(np.uint32), y.view(np.uint32))


def test_autoreset_row_holds_the_reset_forward():
    env_id, n = "relocate-v0", 3
    d = ss.dapg_states(env_id)
    rows = slice(0, n)
    sim = _sim(d, n)
    obs, rew, done, goal = _bufs(sim, n)
    _set(sim, d, 0, rows)
    sim.set_episode(ep_len=_t([0, sim.horizon - 1, 0], torch.int32))
    sim.step(_t(d["act"][0][rows]), obs, rew, done, goal, autoreset=True, seed=11)
    got = _sens(sim)
    assert done.cpu().numpy().tolist() == [0, 2, 0]
    ref = gpu_results(env_id)["step"][0]
    for e in (0, 2):                                         # untouched by their neighbour's reset
        np.testing.assert_array_equal(got[e].view(np.uint32), ref[e].view(np.uint32))
    cols, _ = _columns(d["m"])
    assert not got[1, cols[ss.SENS_JOINTPOS]].any()          # qpos0 = 0
    q, v, w, p = sim.empty(n, sim.nq), sim.empty(n, sim.nv), sim.empty(n, sim.nv), sim.empty(n, sim.nparam)
    sim.get_state(q, v, w, p)
    torch.cuda.synchronize()
    assert not q[1].any() and not v[1].any()
    sim.set_state(q, v, w, p)
    again = _sens(sim)
    np.testing.assert_array_equal(got[1].view(np.uint32), again[1].view(np.uint32))
    sim.close()


def test_claimed_envs_write_their_own_rows():
    """2 100 envs: more than one launch's resident workgroups, so rows are written by workgroups
    that claimed their env; envs 0 and 2 099 carry a grasp state, the others rest at reset"""
    env_id, n = "hammer-v0", 2100
    d = ss.dapg_states(env_id)
    m = d["m"]
    sim = _sim(d, n)
    assert sim.grid < n
    src = 1                                                  # env 1 of env-step 0 of the 4-env states
    q, v, w = (np.zeros((n, m.nq), np.float32) for _ in range(3))
    P = np.tile(d["P"][src], (n, 1))
    act = np.zeros((n, sim.nu), np.float32)
    for e in (0, n - 1):
        q[e], v[e], w[e], act[e] = d["qpos"][0][src], d["qvel"][0][src], d["warm"][0][src], d["act"][0][src]
    sim.set_state(_t(q), _t(v), _t(w), _t(P))
    obs, rew, done, goal = _bufs(sim, n)
    sim.step(_t(act), obs, rew, done, goal)
    got = _sens(sim)
    ref = gpu_results(env_id)["step"][0][src]
    for e in (0, n - 1):
        np.testing.assert_array_equal(got[e].view(np.uint32), ref.view(np.uint32))
    np.testing.assert_array_equal(got[1].view(np.uint32), got[n - 2].view(np.uint32))
    sim.close()


def test_disable_sensor_flag_zeroes_every_entry():
    d = ss.dapg_states("door-v0")
    n = ss.N_ENVS
    sim = _sim(d, n)
    obs, rew, done, goal = _bufs(sim, n)
    _set(sim, d, 0)
    assert _sens(sim).any()
    sim.set_option(disableflags=1 << 12)                     # mjDSBL_SENSOR
    sim.step(_t(d["act"][0]), obs, rew, done, goal)
    assert not _sens(sim).any()
    sim.close()


def test_python_surface():
    from mj_envs_amd import _native
    from mj_envs_amd.envs import AdroitVecEnv, RelocateEnvV0
    from mj_envs_amd.mjcf import SENS_TOUCH
    n = 3
    env = AdroitVecEnv("relocate-v0", n, sensors=True)
    ns = env.model.nsensor
    env.reset()
    assert env.sensordata.shape == (n, ns) and env.sensordata.is_cuda and env.sensordata.dtype == torch.float32
    assert len(env.sensor_names) == ns == len(env.sensor_types) == 65
    order = np.argsort(env.model.arrays["sensor_adr"])
    assert env.sensor_names == [env.model.names["sensor"][i] for i in order]
    tcols = np.flatnonzero(env.sensor_types == SENS_TOUCH)
    assert len(tcols) == 21 and all(env.sensor_names[c].startswith("ST_") for c in tcols)
    act = torch.zeros(n, env.nu, device="cuda")
    _, _, _, _, info = env.step(act)
    assert info["sensordata"] is env.sensordata
    assert torch.equal(env.touch, env.sensordata[:, torch.as_tensor(tcols, device="cuda")])
    assert env.sensordata.abs().sum() > 0                    # the actuator forces of a held pose
    env.close()

    off = AdroitVecEnv("relocate-v0", n)
    off.reset()
    _, _, _, _, info = off.step(act)
    assert "sensordata" not in info
    for name in ("sensordata", "touch"):
        with pytest.raises(AttributeError):
            getattr(off, name)
    with pytest.raises(_native.NativeError, match="disabled"):
        off.sim.sensordata(off.sim.empty(n, ns))
    assert off.sim.nsensordata == ns
    off.close()

    one = RelocateEnvV0(sensors=True)
    one.step(np.zeros(one.vec.nu))
    sd = one.sensordata
    assert sd.dtype == np.float64 and sd.shape == (ns,)
    np.testing.assert_array_equal(sd, one.vec.sensordata[0].cpu().numpy().astype(np.float64))
    one.close()
