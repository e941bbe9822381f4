"""The merged load heads of the env-step (AW_CS_HEAD in aw_solver.h; AW_TAIL_HEADS in
aw_dynamics.h / aw_step.h) move model reads, never arithmetic: the product library must give the bits
of a library built with every one of them at 0 (tools/build_variant.py's build, made once here when
it is missing or older than the sources).

Both libraries are loaded into this process, one after the other behind `_native.load()`.  Per task,
in the fast and in the wide tier, from the same states (aw_set_state):

(a) aw_forward_dump of every env: qacc, the constraint rows, the contact list, the counts;
(b) qpos / qvel / warmstart / obs / reward / done after each of 3 env-steps under Philox actions;
(c) both again with frictionloss and limit rows disabled (no lane of the frictionloss, joint-limit and
    tendon-limit arms is active: every index of their load heads is the clamped one).

The states are the ones at which a merged head can go wrong, and the test asserts that they occur:
oracle rollouts of random actions (contacts, a few limit rows), the zero pose (no contact; many
joint-limit rows, no tendon-limit row: both sides of every limited tendon inactive), the zero pose
with the free object lifted (no contact in any task), and for hammer eight DAPG mid-episode states
with the most rows (nefc > 64: the impedance loop's second trip).  An env without an active limit
row occurs among the rollout states.  All four tasks have tendons and frictionloss dofs, so an empty
tendon or frictionloss table is reached only through (c).
"""
import contextlib
import ctypes
import functools
import os

import numpy as np
import pytest

from conftest import ENVS, GOLDEN, REPO
import test_gpu_parity as tp

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ZERO_FLAGS = ("-DAW_CS_HEAD=0", "-DAW_TAIL_HEADS=0")
ZERO_LIB = os.path.join(REPO, "mj_envs_amd", "libadroit_hip_heads0.so")
N_ROLL, STEPS, ACT_SEED = 6, 3, 13
DSBL_FRICTIONLOSS, DSBL_LIMIT = 1 << 2, 1 << 3
C_LIM_JNT, C_LIM_TEN = 2, 3
DUMP_KEYS = ("qacc", "qacc_smooth", "qfrc_constraint", "scalars", "con_dist", "con_pos", "con_frame", "con_pair",
             "efc_force", "efc_aref", "efc_D", "efc_type", "efc_state")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _t(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype or torch.float32, device="cuda")


def _np(t):
    return t.cpu().numpy().copy()


@functools.lru_cache(maxsize=None)
def zero_lib():
    """the library with every load-head macro at 0, built when absent or older than its sources"""
    import __graft_entry__ as g
    csrc = os.path.join(REPO, "mj_envs_amd", "csrc")
    deps = [os.path.join(csrc, f) for f in os.listdir(csrc)] + [os.path.join(REPO, "__graft_entry__.py")]
    if g._stale(ZERO_LIB, deps):
        g.build_hip(ZERO_LIB, ZERO_FLAGS)
    return ZERO_LIB


@contextlib.contextmanager
def library(path):
    """`_native.load()` answers with the library at `path` (None: the product library) inside the block;
    every handle made inside is closed inside"""
    from mj_envs_amd import _native
    product = _native.load()
    if path is None:
        yield
        return
    L = ctypes.CDLL(path)
    for name, sig in _native.ABI.items():
        fn = getattr(L, name)          # the same revision's ABI: nothing may be missing
        fn.restype, fn.argtypes = sig
    _native._lib = L
    try:
        yield
    finally:
        _native._lib = product


@functools.lru_cache(maxsize=None)
def states(env_id):
    """(model, params, qpos, qvel, warm) fp32 rows: N_ROLL oracle rollout states, the zero pose, the zero pose
    with the object lifted; hammer: + the 8 DAPG mid-episode states with the most rows (product library)"""
    m, o, P, st = tp.contact_states(env_id, N_ROLL, 20, seed=3)
    nv = o.nv
    q = np.vstack([st["qpos"], np.zeros((2, nv))])
    q[-1, nv - 4] = 0.4            # the free object's z translation: clear of the table and the hand
    v = np.vstack([st["qvel"], np.zeros((2, nv))])
    w = np.vstack([st["warm"], np.zeros((2, nv))])
    P = np.vstack([P, P[:2]])
    if env_id == "hammer-v0":
        from mj_envs_amd import _native
        from mj_envs_amd.policy import GaussianMLP
        n = 64
        sim = _native.Sim(m.to_blob(), n)
        pol = GaussianMLP.from_npz(os.path.join(GOLDEN, "dapg_hammer.npz"))
        obs, rew = sim.empty(n, sim.obs_dim), sim.empty(n)
        done, goal = sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
        sim.reset(obs, seed=21)
        for _ in range(120):
            sim.step(_t(pol.mean_np(obs.cpu().numpy())), obs, rew, done, goal)
        gq, gv, gw, gp = sim.empty(n, sim.nq), sim.empty(n, sim.nv), sim.empty(n, sim.nv), sim.empty(n, sim.nparam)
        sim.get_state(gq, gv, gw, gp)
        torch.cuda.synchronize()
        top = np.argsort([-sim.forward_dump(e)["nefc"] for e in range(n)])[:8]
        sim.close()
        q, v, w, P = (np.vstack([a, _np(b)[top]]) for a, b in ((q, gq), (v, gv), (w, gw), (P, gp)))
    return m, tp.f32(P), tp.f32(q), tp.f32(v), tp.f32(w)


def _run(env_id, lib, wide, flags):
    """the dumps of every env at the set states and STEPS env-steps from them, with one library"""
    from mj_envs_amd import _native
    m, P, q, v, w = states(env_id)
    n = len(q)
    with library(lib):
        sim = _native.Sim(m.to_blob(), n)
        if flags:
            sim.set_option(disableflags=flags)
        sim.set_tier(1 if wide else 0)
        sim.set_state(_t(q), _t(v), _t(w), _t(P))
        dumps = [sim.forward_dump(e, wide=wide) for e in range(n)]
        obs, rew = sim.empty(n, sim.obs_dim), sim.empty(n)
        done, goal = sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
        act = sim.empty(n, sim.nu)
        gq, gv, gw = sim.empty(n, sim.nq), sim.empty(n, sim.nv), sim.empty(n, sim.nv)
        steps = []
        for k in range(STEPS):
            sim.random_actions(act, ACT_SEED, k)
            sim.step(act, obs, rew, done, goal)
            sim.get_state(gq, gv, gw)
            torch.cuda.synchronize()
            steps.append(dict(qpos=_np(gq), qvel=_np(gv), warm=_np(gw), obs=_np(obs), rew=_np(rew), done=_np(done)))
        sim.close()
    return dumps, steps


@functools.lru_cache(maxsize=None)
def product_run(env_id, wide, flags):
    return _run(env_id, None, wide, flags)


def _same_bits(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    np.testing.assert_array_equal(a.view(np.uint8), b.view(np.uint8), err_msg=what)


@pytest.mark.parametrize("flags", [0, DSBL_FRICTIONLOSS | DSBL_LIMIT], ids=["rows", "no_fl_no_limit"])
@pytest.mark.parametrize("wide", [False, True], ids=["fast", "wide"])
@pytest.mark.parametrize("env_id", ENVS)
def test_heads_on_is_bitwise_heads_off(env_id, wide, flags):
    dumps, steps = product_run(env_id, wide, flags)
    dumps0, steps0 = _run(env_id, zero_lib(), wide, flags)
    for e, (a, b) in enumerate(zip(dumps, dumps0)):
        for key in DUMP_KEYS:
            _same_bits(a[key], b[key], f"{env_id} env {e} dump {key}")
    for k, (a, b) in enumerate(zip(steps, steps0)):
        for key in a:
            _same_bits(a[key], b[key], f"{env_id} step {k} {key}")
    assert all(np.isfinite(s["qpos"]).all() and np.isfinite(s["obs"]).all() for s in steps)
    if flags:
        # no frictionloss and no limit row anywhere: the three sparse arms ran with no active lane
        assert all(d["nsparse"] == 0 for d in dumps)


def _limit_rows(d):
    t = d["efc_type"].astype(int)
    return int((t == C_LIM_JNT).sum()), int((t == C_LIM_TEN).sum())


def test_states_reach_the_clamped_paths():
    """the conditions the docstring names occur in the states the comparison runs on (fast tier dumps)"""
    from mj_envs_amd.tasks import load_model
    no_contact, no_limit_row, ten_inactive, jnt_rows = {}, {}, {}, {}
    for env_id in ENVS:
        mm = load_model(env_id)
        assert mm.ntendon > 0 and int(np.count_nonzero(mm.tendon_limited)) > 0, env_id   # no task without tendons
        dumps, _ = product_run(env_id, False, 0)
        lim = [_limit_rows(d) for d in dumps]
        no_contact[env_id] = sum(d["ncon"] == 0 for d in dumps)
        no_limit_row[env_id] = sum(j + t == 0 for j, t in lim)
        ten_inactive[env_id] = sum(t == 0 for _, t in lim)
        jnt_rows[env_id] = max(j for j, _ in lim)
        print(f"{env_id}: {len(dumps)} states, ncon {[d['ncon'] for d in dumps]}, nefc {[d['nefc'] for d in dumps]}, "
              f"(joint, tendon) limit rows {lim}")
        assert no_contact[env_id] >= 1, f"{env_id}: no state without contacts"
        assert ten_inactive[env_id] >= 1, f"{env_id}: no state with every tendon limit inactive"
        assert jnt_rows[env_id] >= 1 and any(d["ncon"] > 0 for d in dumps), env_id
    assert sum(no_limit_row.values()) >= 1, "no state without an active limit row"
    hammer, _ = product_run("hammer-v0", False, 0)
    assert max(d["nefc"] for d in hammer) > 64, "hammer: no state whose impedance loop takes a second trip"
