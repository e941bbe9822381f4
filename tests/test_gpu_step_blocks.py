"""The site passes of the env-step's kinematics (aw_dynamics.h AW_SITES_LAST) and stage_crb's compiled
tree masks (AW_CRB_TREE), through aw_step with auto-reset, for every task.

Per task two handles, of 3 envs (not a multiple of 8; sensors and the mjData views on: the SENS / DATA
instantiations, whose site_xpos row is the last substep's) and of 70 envs (more than 64), the same
global env ids, set to the same contact states (tests/test_gpu_parity.py contact_states, 20 oracle
env-steps of random actions) with aw_set_state; 8 env-steps under Philox actions with autoreset;
aw_set_episode puts every env's horizon end at env-step 3, so that step's reset forward and the steps
after it are in the run.

(a) the 3 shared envs give the same bits in both handles at every step;
(b) teacher-forced against the fp64 oracle, with the tolerances of tests/test_gpu_parity.py: post-step
    state within its one-step tolerance (_state_err) in >= ONE_STEP_MIN of the (env, step) cases of
    the 70-env handle, rewards (_rewards_close) in >= REWARD_MIN; the observation of the cases within
    the state tolerance to rtol 1e-3 / atol 2e-3 (its test_hammer_variations_one_step, which has no
    name for it) -- hammer's nail-impact entry included, also held to the suite's force tolerance
    (tests/data_states.py force_ok); the reset forward's observation to rtol 1e-5 / atol 2e-5 (its
    test_reset_obs_matches_oracle_all_tasks); site_xpos of the 3-env handle after every step and
    after the reset within the position tolerance of _state_err;
(c) hammer under the committed DAPG policy, 8 envs, 40 env-steps: the nail-impact entry of the
    observation (the touch sensor's reading, built from sxpos / txmat) is nonzero somewhere.
"""
import functools
import os

import numpy as np
import pytest

from conftest import ENVS, GOLDEN, load_task_model
import data_states as ds
import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

N_SMALL, N_BIG, STEPS, END_STEP = 3, 70, 8, 3
ACT_SEED, RESET_SEED = 7, 11


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _t(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype or torch.float32, device="cuda")


def _np(t):
    return t.cpu().numpy().copy()


def _rollout(sim, st0, P, data=None):
    """STEPS env-steps of one handle from the given states; per step the pre-step state, the action
    and everything the step returned"""
    n = sim.n_envs
    sim.set_state(_t(st0["qpos"][:n]), _t(st0["qvel"][:n]), _t(st0["warm"][:n]), _t(P[:n]))
    sim.set_episode(ep_len=_t(np.full(n, sim.horizon - END_STEP), torch.int32))
    obs, tobs, rew = sim.empty(n, sim.obs_dim), sim.empty(n, sim.obs_dim), sim.empty(n)
    done, goal = sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
    act = sim.empty(n, sim.nu)
    q, v, w, p = sim.empty(n, sim.nq), sim.empty(n, sim.nv), sim.empty(n, sim.nv), sim.empty(n, sim.nparam)
    rec = []
    for k in range(STEPS):
        sim.get_state(q, v, w, p)
        r = dict(pre=dict(qpos=_np(q), qvel=_np(v), warm=_np(w), params=_np(p)))
        sim.random_actions(act, ACT_SEED, k)
        tobs.zero_()
        sim.step(act, obs, rew, done, goal, terminal_obs=tobs, autoreset=True, seed=RESET_SEED)
        sim.get_state(q, v, w, p)
        torch.cuda.synchronize()
        r.update(act=_np(act), obs=_np(obs), tobs=_np(tobs), rew=_np(rew), done=_np(done), goal=_np(goal),
                 qpos=_np(q), qvel=_np(v), params=_np(p))
        if data is not None:
            r["site_xpos"] = _np(data["site_xpos"])
        rec.append(r)
    return rec


@functools.lru_cache(maxsize=None)
def runs(env_id):
    """(model, oracle, rollout of the 3-env handle, rollout of the 70-env handle), computed once"""
    from mj_envs_amd import _native
    m, o, P, st0 = tp.contact_states(env_id, N_BIG, 20, seed=3)
    blob = m.to_blob()
    small = _native.Sim(blob, N_SMALL)
    small.set_sensors(True)
    data = small.set_data(True)
    big = _native.Sim(blob, N_BIG)
    out = (m, o, _rollout(small, st0, P, data), _rollout(big, st0, P))
    small.close()
    big.close()
    return out


@pytest.mark.parametrize("env_id", ENVS)
def test_shared_envs_are_bitwise_equal_in_both_handles(env_id):
    _, _, small, big = runs(env_id)
    ended = 0
    for k, (a, b) in enumerate(zip(small, big)):
        for key in ("act", "obs", "tobs", "rew", "done", "goal", "qpos", "qvel", "params"):
            x, y = np.ascontiguousarray(a[key]), np.ascontiguousarray(b[key][:N_SMALL])
            np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8), err_msg=f"{env_id} step {k} {key}")
        ended += int((b["done"] != 0).sum())
        if k == END_STEP - 1:      # the horizon end: every env truncated (or done) and was reset
            assert (b["done"] != 0).all() and not b["qpos"].any() and not b["qvel"].any()
    assert ended >= N_BIG


def _f64(a):
    return np.asarray(a, np.float64)


@pytest.mark.parametrize("env_id", ENVS)
def test_steps_and_reset_forward_match_oracle(env_id):
    m, o, small, big = runs(env_id)
    touch_at = m.nq + 12 if env_id == "hammer-v0" else None
    oks, roks, n_obs = [], [], 0
    for k, r in enumerate(big):
        st = {key: _f64(val) for key, val in r["pre"].items()}
        o_ref, r_ref, _, _, _ = o.step(st, _f64(r["act"]), nthreads=8)
        ended = r["done"] != 0
        # the state of an env that ended is the next episode's: its last step is held by terminal_obs
        eq, ev, ok = tp._state_err(np.where(ended[:, None], st["qpos"], r["qpos"]),
                                   np.where(ended[:, None], st["qvel"], r["qvel"]), st["qpos"], st["qvel"])
        obs_last = np.where(ended[:, None], r["tobs"], r["obs"])
        oks.append(ok)
        roks.append(tp._rewards_close(r["rew"], r_ref, check=False))
        sel = ok
        print(f"{env_id} step {k}: state ok {ok.mean():.4f}, max |dqpos| {eq.max():.2e}, |dqvel|/(1+|v|) {ev.max():.2e}, "
              f"max |dobs| {np.abs(obs_last - o_ref)[sel].max():.2e}, ended {int(ended.sum())}")
        np.testing.assert_allclose(obs_last[sel], o_ref[sel], rtol=1e-3, atol=2e-3, err_msg=f"{env_id} step {k}")
        n_obs += int(sel.sum())
        if touch_at is not None:
            assert ds.force_ok(obs_last[sel, touch_at], o_ref[sel, touch_at]).all(), (k, obs_last[:, touch_at], o_ref[:, touch_at])
        if ended.any():
            # the returned observation is the reset forward's, of the parameters the reset sampled
            _, reset_ref = o.reset(_f64(r["params"][ended]))
            np.testing.assert_allclose(r["obs"][ended], reset_ref, rtol=1e-5, atol=2e-5, err_msg=f"{env_id} reset at step {k}")
    ok, rok = np.concatenate(oks), np.concatenate(roks)
    print(f"{env_id}: {ok.mean():.4f} of {ok.size} (env, step) cases within the state tolerance, rewards {rok.mean():.4f}, "
          f"{n_obs} observations compared")
    assert ok.mean() >= tp.ONE_STEP_MIN and rok.mean() >= tp.REWARD_MIN, (ok.mean(), rok.mean())

    # site_xpos of the 3-env handle (the DATA instantiation), one env at a time in the oracle
    bad, worst = [], 0.0
    zero = np.zeros((1, 1))
    for k, r in enumerate(small):
        for e in range(N_SMALL):
            pre = {key: _f64(val[e]) for key, val in r["pre"].items()}
            if r["done"][e]:
                ref = ds.oracle_forward_data(o, _f64(r["params"][e]), _f64(r["qpos"][e]), _f64(r["qvel"][e]), np.zeros(m.nv))
            else:
                ref = ds.oracle_step_data(o, m, pre["params"], pre["qpos"], pre["qvel"], pre["warm"], _f64(r["act"][e]), True)
            got, want = _f64(r["site_xpos"][e]).reshape(1, -1), ref["site_xpos"].reshape(1, -1)
            err, _, good = tp._state_err(got, zero, want, zero)
            worst = max(worst, float(err[0]))
            if not good[0] and big[k]["done"][e] == r["done"][e] and oks[k][e]:
                bad.append((k, e, float(err[0])))
    print(f"{env_id}: site_xpos max |err| {worst:.2e} over {STEPS * N_SMALL} (env, step) cases")
    assert not bad, bad


def test_hammer_nail_impact_reaches_the_observation():
    from mj_envs_amd import _native
    from mj_envs_amd.policy import GaussianMLP
    from mj_envs_amd.tasks import sample_params
    env_id, n = "hammer-v0", 8
    m = load_task_model(env_id)
    sim = _native.Sim(m.to_blob(), n)
    pol = GaussianMLP.from_npz(os.path.join(GOLDEN, "dapg_hammer.npz"))
    obs, rew = sim.empty(n, sim.obs_dim), sim.empty(n)
    done, goal = sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
    sim.reset(obs, params=_t(tp.f32(sample_params(env_id, m, np.random.default_rng(5), n))))
    touch = []
    for _ in range(40):
        sim.step(_t(pol.mean_np(obs.cpu().numpy())), obs, rew, done, goal)
        touch.append(obs[:, m.nq + 12].cpu().numpy().copy())
    sim.close()
    touch = np.array(touch)
    print(f"hammer DAPG: nail-impact entry nonzero in {int((touch != 0).sum())} of {touch.size} (step, env) cases, max {touch.max():.3f}")
    assert np.isfinite(touch).all() and (touch != 0).any()
