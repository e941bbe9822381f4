"""Batched mjData views on device (aw_set_data) against the fp64 oracle and against what the kernels
already emit, on the DAPG grasp states of tests/sensor_states.py (4 tasks x 3 env-steps x 4 envs;
tests/test_data.py asserts on the oracle alone that those inputs are well conditioned).

Tolerances, from identical fp32 inputs:
  * xpos, site_xpos: |err| <= 2e-5 + 1e-5 |x|, what the suite holds obs (and so positions) to;
    xquat the same up to the quaternion's sign.
  * qacc: rel < 2e-3 (tests/test_gpu_parity.py test_forward_internals_match_oracle, its `rel`).
  * qfrc_constraint and every contact force component (normal, two tangents, torsion):
    |err| <= 2e-3 + 2e-3 |ref|, what the suite holds constraint quantities to (touch, efc_aref).
  * contacts are matched by (geom1, geom2, index within the pair); matched contacts: dist atol 2e-5,
    pos atol 2e-4 (test_gpu_parity.py), normal atol 2e-4 (the pos figure).
  * per task at most 5 % of the oracle's pressing contacts (normal force > 2e-3 N) may be unmatched
    or out of tolerance; GPU-only contacts pressing harder than 2e-3 N count as misses against the
    same total; at least 40 pressing contacts are compared per task after aw_step (the forward of
    the same states with ctrl 0, after aw_set_state, presses a little less: pen 39 -- floor 35).
"""
import ctypes
import functools

import numpy as np
import pytest

from conftest import ENVS
import data_states as ds
import sensor_states as ss

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ALL = 7
KEYS = ("xpos", "xquat", "site_xpos", "qacc", "qfrc_constraint", "counts", "contact")
GEO_ATOL = (2e-5, 2e-4, 2e-4)            # dist, pos, normal


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _t(a, dtype=None):
    return torch.tensor(np.asarray(a), dtype=dtype or torch.float32, device="cuda")


def _sim(d, n, groups=ALL, K=32, sensors=False, bufs=None):
    from mj_envs_amd import _native
    sim = _native.Sim(d["m"].to_blob(), n)
    if sensors:
        sim.set_sensors(True)
    b = sim.set_data(groups, K, bufs) if groups else {}
    return sim, b


def _bufs(sim, n):
    return (sim.empty(n, sim.obs_dim), sim.empty(n), sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8))


def _snap(b):
    torch.cuda.synchronize()
    return {k: v.cpu().numpy().copy() for k, v in b.items()}


def _set(sim, d, k, rows=slice(None)):
    sim.set_state(_t(d["qpos"][k][rows]), _t(d["qvel"][k][rows]), _t(d["warm"][k][rows]), _t(d["P"][rows]))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _contacts(snap, e):
    """env e's current contacts of a snapshot as the arrays of data_states.decode_contacts"""
    from mj_envs_amd import _native
    rec = snap["contact"][e]
    n = min(int(snap["counts"][e, 0]), rec.shape[0])
    out = {}
    for k, (w0, nw, is_int) in _native.CONTACT_FIELDS.items():
        a = rec[:n].view(np.int32) if is_int else rec[:n]
        out[k] = (a[:, w0] if nw == 1 else a[:, w0:w0 + nw]).astype(int if is_int else np.float64)
    return out


@functools.lru_cache(maxsize=None)
def gpu_results(env_id, tier=0):
    """per chosen env-step: every buffer after set_state alone (fwd) and after one more aw_step (step),
    the step's obs and status; computed once and shared"""
    d = ss.dapg_states(env_id)
    n = ss.N_ENVS
    sim, b = _sim(d, n)
    sim.set_tier(tier)
    obs, rew, done, goal = _bufs(sim, n)
    out = dict(fwd=[], step=[], obs=[], fwd_obs=[], status=[])
    for k in range(len(d["steps"])):
        sim.set_state(_t(d["qpos"][k]), _t(d["qvel"][k]), _t(d["warm"][k]), _t(d["P"]), obs=obs)
        out["fwd"].append(_snap(b))
        out["fwd_obs"].append(obs.cpu().numpy().copy())
        sim.step(_t(d["act"][k]), obs, rew, done, goal)
        out["step"].append(_snap(b))
        out["obs"].append(obs.cpu().numpy().copy())
        st = sim.empty(n, dtype=torch.int32)
        sim.status(last=st)
        out["status"].append(st.cpu().numpy())
    sim.close()
    return out


def _q(x, qs=(0.5, 0.9, 1.0)):
    x = np.asarray(x, float)
    return " ".join(f"{np.quantile(x, q):.2e}" for q in qs) if x.size else "-"


def _check_vs_oracle(env_id, got_k, ref_k, what, floor):
    pressing = misses = 0
    e_pos, e_quat, e_qacc, e_qfrc, e_force, e_geo = [], [], [], [], [], []
    bad = []
    for k, (snap, refs) in enumerate(zip(got_k, ref_k)):
        for e, ref in enumerate(refs):
            tag = (what, env_id, k, e)
            for key in ("xpos", "site_xpos"):
                err = np.abs(snap[key][e] - ref[key])
                e_pos.append(err.max())
                if not (err <= 2e-5 + 1e-5 * np.abs(ref[key])).all():
                    bad.append(tag + (key,))
            q, qr = snap["xquat"][e].astype(np.float64), ref["xquat"]
            sign = np.where((q * qr).sum(axis=1, keepdims=True) < 0, -1.0, 1.0)
            err = np.abs(sign * q - qr)
            e_quat.append(err.max())
            if not (err <= 2e-5 + 1e-5 * np.abs(qr)).all():
                bad.append(tag + ("xquat",))
            r = ds.rel(snap["qacc"][e], ref["qacc"])
            e_qacc.append(r)
            if not r < 2e-3:
                bad.append(tag + ("qacc", r))
            err = np.abs(snap["qfrc_constraint"][e] - ref["qfrc_constraint"])
            e_qfrc.append(err.max())
            if not ds.force_ok(snap["qfrc_constraint"][e], ref["qfrc_constraint"]).all():
                bad.append(tag + ("qfrc_constraint", err.max()))
            got = _contacts(snap, e)
            p, miss, same, errs = ds.compare_contacts(got, ref["contact"], GEO_ATOL)
            pressing += p
            misses += miss
            e_force.extend(errs)
            if same:
                if not (snap["counts"][e, :2] == ref["counts"][:2]).all():
                    bad.append(tag + ("counts", snap["counts"][e].tolist(), ref["counts"].tolist()))
                c = ref["contact"]
                e_geo.append(max(np.abs(got["dist"] - c["dist"]).max(), 0.1 * np.abs(got["pos"] - c["pos"]).max(),
                                 0.1 * np.abs(got["normal"] - c["normal"]).max()))
                if not ((got["dim"] == c["dim"]).all() and (got["efc_address"] == c["efc_address"]).all()
                        and np.abs(got["mu"] - c["mu"]).max() < 1e-6):
                    bad.append(tag + ("dim / efc_address / mu",))
            else:
                print(f"{what} {env_id} step {k} env {e}: contact sets differ, GPU {ds.contact_keys(got['geom1'], got['geom2'])} "
                      f"oracle {ds.contact_keys(ref['contact']['geom1'], ref['contact']['geom2'])}")
    print(f"{what} {env_id}: |err| quantiles (median p90 max): pos {_q(e_pos)}  quat {_q(e_quat)}  qacc rel {_q(e_qacc)}  "
          f"qfrc_constraint {_q(e_qfrc)}  contact force components {_q(e_force)}  "
          f"geometry (dist, pos / 10, normal / 10) {_q(e_geo)}")
    print(f"{what} {env_id}: {misses} misses of {pressing} pressing contacts")
    assert not bad, bad
    assert pressing >= floor
    assert misses <= 0.05 * pressing


# --- 1. against the oracle ---------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ENVS)
def test_step_data_vs_oracle(env_id):
    """teacher-forced: aw_set_state with the oracle's state, one aw_step with the same action"""
    _check_vs_oracle(env_id, gpu_results(env_id)["step"], ds.data_refs(env_id)["step_f32"], "step", 40)


@pytest.mark.parametrize("env_id", ENVS)
def test_set_state_forward_data_vs_oracle(env_id):
    _check_vs_oracle(env_id, gpu_results(env_id)["fwd"], ds.data_refs(env_id)["fwd_f32"], "set_state", 35)


# --- 2. consistency with what the kernel already emits -------------------------------------------
def _obs_slices(env_id, m, snap, e):
    """[(obs slice, the fp32 value the kernel's task_obs forms from the frames)] (aw_task.h task_obs)"""
    id_, nq = m.arrays["task_idx"].astype(int), m.nq
    X, S = snap["xpos"][e], snap["site_xpos"][e]
    if env_id == "hammer-v0":      # S_grasp, Object, S_target
        return [(slice(nq, nq + 3), S[id_[0]]), (slice(nq + 3, nq + 6), X[id_[1]]), (slice(nq + 9, nq + 12), S[id_[3]])]
    if env_id == "door-v0":        # palm, handle, palm - handle
        o = nq - 3
        return [(slice(o + 2, o + 5), S[id_[0]]), (slice(o + 5, o + 8), S[id_[1]]), (slice(o + 8, o + 11), S[id_[0]] - S[id_[1]])]
    if env_id == "pen-v0":         # object position, object - target position
        o = nq - 6
        return [(slice(o, o + 3), X[id_[1]]), (slice(o + 15, o + 18), X[id_[1]] - S[id_[2]])]
    o = nq - 6                     # relocate: palm - object, palm - target, object - target
    p, ob, t = S[id_[0]], X[id_[1]], S[id_[2]]
    return [(slice(o, o + 3), p - ob), (slice(o + 3, o + 6), p - t), (slice(o + 6, o + 9), ob - t)]


def _assert_obs_consistent(env_id, m, snap, obs, envs):
    for e in envs:
        for sl, val in _obs_slices(env_id, m, snap, e):
            assert val.dtype == np.float32
            np.testing.assert_array_equal(_bits(obs[e, sl]), _bits(val), err_msg=f"{env_id} env {e} obs[{sl}]")


@pytest.mark.parametrize("env_id", ENVS)
def test_frames_are_the_observation_inputs(env_id):
    """hammer: site_xpos[S_grasp], body_xpos[Object], site_xpos[S_target] are obs[33:36], [36:39],
    [42:45] bit for bit; the analogous slices of the other tasks -- after a step and after set_state"""
    m, g = ss.dapg_states(env_id)["m"], gpu_results(env_id)
    if env_id == "hammer-v0":
        assert [(s.start, s.stop) for s, _ in _obs_slices(env_id, m, g["step"][0], 0)] == [(33, 36), (36, 39), (42, 45)]
    for k in range(3):
        _assert_obs_consistent(env_id, m, g["step"][k], g["obs"][k], range(ss.N_ENVS))
        _assert_obs_consistent(env_id, m, g["fwd"][k], g["fwd_obs"][k], range(ss.N_ENVS))


def test_sensordata_unchanged_with_data_on():
    """sensors and data on together: sensordata is what it is with data off, and the pads are the
    contact records' normal forces (hammer, grasp states)"""
    env_id, n = "hammer-v0", ss.N_ENVS
    d = ss.dapg_states(env_id)
    out = []
    for groups in (0, ALL):
        sim, b = _sim(d, n, groups=groups, sensors=True)
        obs, rew, done, goal = _bufs(sim, n)
        _set(sim, d, 0)
        sim.step(_t(d["act"][0]), obs, rew, done, goal)
        sd = sim.sensordata(sim.empty(n, sim.nsensordata))
        torch.cuda.synchronize()
        out.append((sd.cpu().numpy().copy(), _snap(b)))
        sim.close()
    np.testing.assert_array_equal(_bits(out[0][0]), _bits(out[1][0]))
    assert out[0][0].any()
    for key in KEYS:                                   # and the data is what it is without sensors
        np.testing.assert_array_equal(_bits(out[1][1][key]), _bits(gpu_results(env_id)["step"][0][key]))


# --- 3. no side effects -----------------------------------------------------------------------
@pytest.mark.parametrize("sensors", (False, True))
@pytest.mark.parametrize("env_id", ("hammer-v0", "relocate-v0"))
def test_data_has_no_side_effects(env_id, sensors):
    """data on against off, 5 env-steps from the same state: obs, reward, done, goal, the get_state
    tensors and status bitwise equal"""
    d = ss.dapg_states(env_id)
    n = ss.N_ENVS
    outs = []
    for groups in (0, ALL):
        sim, _ = _sim(d, n, groups=groups, sensors=sensors)
        obs, rew, done, goal = _bufs(sim, n)
        _set(sim, d, 0)
        rec = []
        for k in range(5):
            sim.step(_t(d["act"][k % 3]), obs, rew, done, goal)
            q, v, w, p = sim.empty(n, sim.nq), sim.empty(n, sim.nv), sim.empty(n, sim.nv), sim.empty(n, sim.nparam)
            sim.get_state(q, v, w, p)
            st = sim.empty(n, dtype=torch.int32)
            sim.status(last=st)
            torch.cuda.synchronize()
            rec.append([x.cpu().numpy().copy() for x in (obs, rew, done, goal, q, v, w, p, st)])
        outs.append(rec)
        sim.close()
    for a, b in zip(*outs):
        for x, y in zip(a, b):
            np.testing.assert_array_equal(_bits(x), _bits(y))


# --- 4. tier equality -------------------------------------------------------------------------
@pytest.mark.parametrize("env_id", ("hammer-v0", "relocate-v0"))
def test_wide_tier_data_bitwise(env_id):
    """every forward re-run by the wide tier (aw_set_tier 1) writes the automatic tier's bits"""
    from mj_envs_amd import _native
    a, w = gpu_results(env_id, 0), gpu_results(env_id, 1)
    assert all((s & _native.ST_WIDE).all() for s in w["status"]) and not any((s & _native.ST_WIDE).any() for s in a["status"])
    for key in ("fwd", "step"):
        for x, y in zip(a[key], w[key]):
            for name in KEYS:
                np.testing.assert_array_equal(_bits(x[name]), _bits(y[name]), err_msg=f"{key} {name}")


# --- 5. truncation ----------------------------------------------------------------------------
def test_truncated_contact_list():
    """max_contacts 4 on states with ncon >= 5: counts hold the true ncon, records 0..3 are those of
    the untruncated run, and nothing past them -- records of envs with fewer contacts, the memory
    after the last env's row -- is written"""
    env_id, n, K = "door-v0", ss.N_ENVS, 4
    d = ss.dapg_states(env_id)
    full = gpu_results(env_id)["step"][0]
    assert (full["counts"][:, 0] >= 5).all()
    SENT = 12345.0
    big = torch.full((n + 1, K, 16), SENT, device="cuda")
    from mj_envs_amd import _native
    sim, b = _sim(d, n, groups=_native.AW_DATA_DYN | _native.AW_DATA_CONTACT, K=K, bufs=dict(contact=big))
    assert b["contact"] is big
    obs, rew, done, goal = _bufs(sim, n)
    _set(sim, d, 0)
    sim.step(_t(d["act"][0]), obs, rew, done, goal)
    got = _snap(b)
    np.testing.assert_array_equal(got["counts"], full["counts"])
    np.testing.assert_array_equal(_bits(got["contact"][:n]), _bits(full["contact"][:, :K]))
    assert (got["contact"][n] == SENT).all()           # past the last env's row
    # an env with fewer contacts than K keeps the records past its own: reset, 0 contacts at rest
    big.fill_(SENT)
    sim.reset(None, params=_t(ss.f32(d["P"])))
    rest = _snap(b)
    nc = rest["counts"][:, 0]
    assert (nc < K).any()
    for e in range(n):
        assert (rest["contact"][e, min(nc[e], K):] == SENT).all()
        assert not (rest["contact"][e, :min(nc[e], K)] == SENT).any()
    assert (rest["contact"][n] == SENT).all()
    sim.close()


# --- 6. auto-reset alignment -------------------------------------------------------------------
def test_autoreset_row_holds_the_reset_forward():
    env_id, n = "relocate-v0", 3
    d = ss.dapg_states(env_id)
    m, rows = d["m"], slice(0, n)
    sim, b = _sim(d, n)
    obs, rew, done, goal = _bufs(sim, n)
    _set(sim, d, 0, rows)
    sim.set_episode(ep_len=_t([0, sim.horizon - 1, 0], torch.int32))
    sim.step(_t(d["act"][0][rows]), obs, rew, done, goal, autoreset=True, seed=11)
    got = _snap(b)
    o = obs.cpu().numpy()
    assert done.cpu().numpy().tolist() == [0, 2, 0]
    ref = gpu_results(env_id)["step"][0]
    for e in (0, 2):                                         # untouched by their neighbour's reset
        for key in KEYS:
            np.testing.assert_array_equal(_bits(got[key][e]), _bits(ref[key][e]), err_msg=key)
    _assert_obs_consistent(env_id, m, got, o, range(n))      # env 1: the returned first obs of the new episode
    # ncon and qacc are a reset forward's: set_state of the stored (reset) state reproduces the row
    q, v, w, p = sim.empty(n, sim.nq), sim.empty(n, sim.nv), sim.empty(n, sim.nv), sim.empty(n, sim.nparam)
    sim.get_state(q, v, w, p)
    torch.cuda.synchronize()
    assert not q[1].any() and not v[1].any()
    sim.set_state(q, v, w, p)
    again = _snap(b)
    for key in KEYS:
        np.testing.assert_array_equal(_bits(got[key][1]), _bits(again[key][1]), err_msg=key)
    assert got["counts"][1, 0] != ref["counts"][1, 0] or not np.array_equal(got["qacc"][1], ref["qacc"][1])
    sim.close()


# --- 7. claim loop ----------------------------------------------------------------------------
def test_claimed_envs_write_their_own_rows():
    """4 096 envs, more than one launch's resident workgroups: rows are written by workgroups that
    claimed their env.  Buffers pre-filled with NaN; after one random-action step every env's KIN
    and DYN rows are finite and 0 <= ncon <= 100"""
    env_id, n = "hammer-v0", 4096
    d = ss.dapg_states(env_id)
    sim, b = _sim(d, n)
    assert sim.grid < n
    obs, rew, done, goal = _bufs(sim, n)
    sim.reset(obs, seed=3)
    for key, t in b.items():
        if key != "counts":
            t.fill_(float("nan"))
    b["counts"].fill_(-1)
    act = sim.empty(n, sim.nu)
    sim.random_actions(act, seed=7, step=0)
    sim.step(act, obs, rew, done, goal)
    torch.cuda.synchronize()
    for key in ("xpos", "xquat", "site_xpos", "qacc", "qfrc_constraint"):
        assert bool(torch.isfinite(b[key]).all()), key
    nc = b["counts"][:, 0]
    assert int(nc.min()) >= 0 and int(nc.max()) <= 100
    assert int(b["counts"][:, 1:].min()) >= 0
    # the current records are written, the others are not
    K = b["contact"].shape[1]
    cur = torch.arange(K, device="cuda")[None, :] < nc.clamp(max=K)[:, None]
    fin = torch.isfinite(b["contact"][:, :, :12]).all(dim=2)
    assert bool((fin == cur).all())
    sim.close()


# --- 8. ABI -----------------------------------------------------------------------------------
def test_abi_argument_checks_and_groups():
    from mj_envs_amd import _native
    L = _native.load()
    env_id, n = "pen-v0", ss.N_ENVS
    d = ss.dapg_states(env_id)
    sim, _ = _sim(d, n, groups=0)
    full = {k: torch.zeros_like(_t(v), dtype=torch.int32 if k == "counts" else torch.float32)
            for k, v in gpu_results(env_id)["step"][0].items()}

    def call(groups, K, **drop):
        c = _native.DataBufs()
        for k, t in full.items():
            setattr(c, k, None if k in drop else t.data_ptr())
        return L.aw_set_data(sim.h, groups, K, ctypes.byref(c))

    EINVAL = -1
    assert call(8, 32) == EINVAL and call(15, 32) == EINVAL and call(-1, 32) == EINVAL      # unknown group bits
    assert b"group" in L.aw_last_error()
    assert call(ALL, 0) == EINVAL and call(ALL, -3) == EINVAL and call(ALL, 129) == EINVAL  # max_contacts
    assert b"max_contacts" in L.aw_last_error()
    for k, bit in (("xpos", 1), ("xquat", 1), ("site_xpos", 1), ("qacc", 2), ("qfrc_constraint", 2), ("counts", 2),
                   ("contact", 4)):
        assert call(bit, 32, **{k: 1}) == EINVAL, k                                         # NULL buffer of a requested group
        assert call(ALL & ~bit, 32, **{k: 1}) == 0, k                                       # not requested: ignored
    assert L.aw_set_data(sim.h, ALL, 32, None) == EINVAL
    assert call(0, 0) == 0 and L.aw_set_data(sim.h, 0, 0, None) == 0                        # disable ignores the rest
    assert call(ALL, 128) == 0 and call(ALL, 1) == 0 and call(0, 32) == 0

    # groups individually: a group not requested leaves its buffer untouched; enable -> disable -> enable
    obs, rew, done, goal = _bufs(sim, n)
    ref = gpu_results(env_id)["step"][0]
    for groups in (1, 2, 4, 0, ALL):
        assert call(groups, 32) == 0
        _set(sim, d, 0)
        for t in full.values():                               # (after set_state's own forward wrote its rows)
            t.fill_(-7)
        sim.step(_t(d["act"][0]), obs, rew, done, goal)
        got = _snap(full)
        for bit, names in _native.DATA_BUFFERS.items():
            for k in names:
                if groups & bit and k != "contact":
                    np.testing.assert_array_equal(_bits(got[k]), _bits(ref[k]), err_msg=f"groups {groups} {k}")
                elif groups & bit:
                    nc = ref["counts"][:, 0]
                    for e in range(n):
                        np.testing.assert_array_equal(_bits(got[k][e, :nc[e]]), _bits(ref[k][e, :nc[e]]))
                        assert (got[k][e, nc[e]:] == -7).all()
                else:
                    assert (got[k] == -7).all(), f"groups {groups}: {k} was written"
    sim.close()


# --- 9. Python surface ------------------------------------------------------------------------
def test_python_surface_against_oracle():
    """AdroitVecEnv(data=True) on relocate grasp states: normal_force_between(Object, finger / hand
    geoms) against the oracle's contacts, force_world against numpy"""
    from mj_envs_amd.data import make_frame_np
    from mj_envs_amd.envs import AdroitVecEnv
    env_id, n, k = "relocate-v0", ss.N_ENVS, 1
    d = ss.dapg_states(env_id)
    m = d["m"]
    env = AdroitVecEnv(env_id, n, data=True, autoreset=False)
    env.set_state(_t(d["qpos"][k]), _t(d["qvel"][k]), _t(d["warm"][k]), _t(d["P"]))
    env.step(_t(d["act"][k]))
    torch.cuda.synchronize()
    D = env.data
    refs = ds.data_refs(env_id)["step_f32"][k]
    assert D.body_xpos.shape == (n, m.nbody, 3) and D.body_xquat.shape == (n, m.nbody, 4)
    assert D.site_xpos.shape == (n, m.nsite, 3) and D.qacc.shape == D.qfrc_constraint.shape == (n, m.nv)
    assert D.ncon.dtype == torch.int32 and D.contact.geom1.dtype == torch.int32 and D.contact.pos.shape == (n, 32, 3)
    assert all(x.is_cuda for x in (D.body_xpos, D.qacc, D.ncon, D.contact.force))
    g = gpu_results(env_id)["step"][k]
    np.testing.assert_array_equal(_bits(D.body_xpos.cpu().numpy()), _bits(g["xpos"]))       # views of the kernel's buffers
    np.testing.assert_array_equal(D.ncon.cpu().numpy(), g["counts"][:, 0])
    np.testing.assert_array_equal(D.contact.mask.cpu().numpy(), np.arange(32)[None, :] < g["counts"][:, :1])

    obj = m.name2id("body", "Object")
    gb = np.asarray(m.arrays["geom_bodyid"])
    palm = m.name2id("body", "ffdistal")            # a finger that holds the ball in every case
    # the object against the whole hand: every body but the world and the object, one geom at a time
    tot_hand = np.zeros(n)
    for e, ref in enumerate(refs):
        c = ref["contact"]
        b1, b2 = gb[c["geom1"]], gb[c["geom2"]]
        on_obj = (b1 == obj) | (b2 == obj)
        tot_hand[e] = c["force"][on_obj & (b1 != 0) & (b2 != 0), 0].sum()
    assert (tot_hand > 0.1).any()                            # the grasp presses
    got = torch.zeros(n, device="cuda")
    for b in range(1, m.nbody):
        if b != obj:
            got += D.contact.normal_force_between("Object", ("body", b))
    got = got.cpu().numpy()
    print(f"normal_force_between(Object, hand): GPU {got}, oracle {tot_hand}")
    # a sum of at most 12 contacts, each within the force tolerance
    assert (np.abs(got - tot_hand) <= 12 * ds.F_ATOL + ds.F_RTOL * np.abs(tot_hand)).all()
    # by name, by id and symmetric; geom names address one geom
    pn = D.contact.normal_force_between("Object", "ffdistal")
    assert torch.equal(pn, D.contact.normal_force_between(palm, obj))
    ref_palm = np.array([r["contact"]["force"][((gb[r["contact"]["geom1"]] == palm) & (gb[r["contact"]["geom2"]] == obj)) |
                                               ((gb[r["contact"]["geom2"]] == palm) & (gb[r["contact"]["geom1"]] == obj)), 0].sum()
                         for r in refs])
    assert (np.abs(pn.cpu().numpy() - ref_palm) <= 12 * ds.F_ATOL + ds.F_RTOL * np.abs(ref_palm)).all()
    per_geom = sum(D.contact.normal_force_between(("geom", int(gi)), "Object") for gi in np.flatnonzero(gb == palm))
    np.testing.assert_allclose(per_geom.cpu().numpy(), pn.cpu().numpy(), rtol=1e-6, atol=1e-6)
    with pytest.raises(KeyError):
        D.contact.normal_force_between("Object", "no_such_thing")

    # force_world against numpy from the same records
    fw = D.contact.force_world().cpu().numpy()
    assert fw.shape == (n, 32, 3)
    for e in range(n):
        c = _contacts(g, e)
        want = np.einsum("ck,ckj->cj", c["force"], make_frame_np(c["normal"]))
        np.testing.assert_allclose(fw[e, :len(want)], want, rtol=1e-5, atol=1e-5)
        assert not fw[e, len(want):].any()
    env.close()


def test_python_surface_groups_and_facade():
    from mj_envs_amd.envs import AdroitVecEnv, HammerEnvV0
    from mj_envs_amd.wrappers import make_env
    import types
    off = AdroitVecEnv("hammer-v0", 2)
    with pytest.raises(AttributeError, match="data=False"):
        off.data
    off.close()
    kin = AdroitVecEnv("hammer-v0", 2, data=("kin",))
    kin.reset()
    assert kin.data.body_xpos.abs().sum() > 0
    for name in ("qacc", "ncon", "contact"):
        with pytest.raises(AttributeError, match="not enabled"):
            getattr(kin.data, name)
    kin.close()
    env = make_env(types.SimpleNamespace(env_name="door-v0", state_type="vector", nogui=True, data=True, max_contacts=8), 2)
    base = env
    while not isinstance(base, AdroitVecEnv):
        base = base.env
    assert base.data.contact.max_contacts == 8
    base.close()

    one = HammerEnvV0(data=True)
    m = one.model

    def check(D):
        v = one.vec.data
        assert D.body_xpos.dtype == np.float64 and D.body_xpos.shape == (m.nbody, 3) and D.site_xpos.shape == (m.nsite, 3)
        assert D.body_xquat.shape == (m.nbody, 4) and D.qacc.shape == D.qfrc_constraint.shape == (m.nv,)
        np.testing.assert_array_equal(D.body_xpos, v.body_xpos[0].cpu().numpy().astype(np.float64))
        np.testing.assert_array_equal(D.qacc, v.qacc[0].cpu().numpy().astype(np.float64))
        assert D.ncon == int(v.ncon[0]) and D.nefc == int(v.nefc[0]) and isinstance(D.solver_iter, int)
        assert D.contact.dist.shape == (D.ncon,) and D.contact.pos.shape == (D.ncon, 3) and D.contact.force.shape == (D.ncon, 3)
        assert D.contact.geom1.dtype == np.int32 and D.contact.mu.shape == (D.ncon,)
        assert D.contact.force_world.shape == (D.ncon, 3)
        # hammer: the frames are the observation's (S_grasp, Object, S_target), after step, reset and set_env_state
        id_ = m.arrays["task_idx"].astype(int)
        ob = one.get_obs()
        np.testing.assert_array_equal(ob[33:36], D.site_xpos[id_[0]].astype(np.float32))
        np.testing.assert_array_equal(ob[36:39], D.body_xpos[id_[1]].astype(np.float32))
        np.testing.assert_array_equal(ob[42:45], D.site_xpos[id_[3]].astype(np.float32))
        return D

    a = check(one.data).body_xpos                                    # after reset (the constructor's)
    state = one.get_env_state()
    rng = np.random.default_rng(0)
    for _ in range(3):
        one.step(rng.uniform(-1, 1, one.vec.nu))
    b = check(one.data)
    assert not np.array_equal(a, b.body_xpos) and np.abs(b.qacc).sum() > 0
    one.set_env_state(state)
    np.testing.assert_array_equal(check(one.data).body_xpos, a)
    one.reset()
    check(one.data)
    one.close()
