"""Rollout fingerprints for the bitwise pin of the env-step (GPU box):

    AW_LIB=mj_envs_amd/libadroit_hip_parent.so python tools/rollout_bits.py COMMIT OUT.json

Per task, 128 envs: 20 env-steps under random actions and 60 in the DAPG closed loop, each from a
seeded reset with auto-reset; the SHA-256 of every step's obs and of the final qpos and qvel.
tests/golden/rollout_bits.json is this file's output for the library of the commit BEFORE a kernel
change (COMMIT, recorded in the file) -- never for the code under test;
tests/test_gpu_rollout_bits.py compares the product library with it.  A kernel change that is meant
to move the arithmetic re-records the file from its own parent and says so."""
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if REPO not in sys.path:
    sys.path.insert(0, REPO)

ENVS = ("hammer-v0", "door-v0", "pen-v0", "relocate-v0")
N_ENVS, STEPS = 128, {"random": 20, "dapg": 60}


def sha(a) -> str:
    return hashlib.sha256(np.ascontiguousarray(a, dtype=np.float32).tobytes()).hexdigest()


def rollout(env_id, pol):
    """(every step's obs [steps, n, obs_dim], final qpos, final qvel) of one seeded rollout"""
    import torch
    from mj_envs_amd import _native
    from mj_envs_amd.policy import GaussianMLP
    from mj_envs_amd.tasks import attach_task, load_model
    n = N_ENVS
    sim = _native.Sim(attach_task(load_model(env_id), env_id).to_blob(), n)
    obs, act = sim.empty(n, sim.obs_dim), sim.empty(n, sim.nu)
    rew, done, goal = sim.empty(n), sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
    sim.reset(obs, seed=5)
    p = GaussianMLP.from_npz(os.path.join(REPO, "tests", "golden", f"dapg_{env_id.split('-')[0]}.npz"),
                             device=0) if pol == "dapg" else None
    obs_all = []
    for k in range(STEPS[pol]):
        if p is not None:
            p.act(obs, out=act)
        else:
            sim.random_actions(act, 9, k)
        sim.step(act, obs, rew, done, goal, autoreset=True, seed=5)
        obs_all.append(obs.cpu().numpy().copy())
    q, v = sim.empty(n, sim.nq), sim.empty(n, sim.nv)
    sim.get_state(q, v)
    torch.cuda.synchronize()
    out = np.stack(obs_all), q.cpu().numpy(), v.cpu().numpy()
    sim.close()
    return out


def fingerprint(env_id):
    """{policy: {obs: [sha per step], qpos: sha, qvel: sha}} and the DAPG rollout's obs"""
    fp, dapg_obs = {}, None
    for pol in ("random", "dapg"):
        obs, q, v = rollout(env_id, pol)
        fp[pol] = dict(obs=[sha(o) for o in obs], qpos=sha(q), qvel=sha(v))
        if pol == "dapg":
            dapg_obs = obs
    return fp, dapg_obs


def nail_impact(dapg_obs):
    """hammer-v0's nail-impact entry of every hashed DAPG obs: the clamped touch sensor, the obs's
    last entry (aw_task.h task_obs, out[nq + 12] of nq + 13)"""
    return dapg_obs[:, :, -1]


if __name__ == "__main__":
    commit, path = sys.argv[1], sys.argv[2]
    rec = dict(commit=commit, envs=N_ENVS, steps=STEPS, tasks={})
    for env_id in ENVS:
        rec["tasks"][env_id], dobs = fingerprint(env_id)
        if env_id == "hammer-v0":
            t = nail_impact(dobs)
            print("hammer-v0 DAPG nail-impact entries: nonzero", int((t != 0).sum()), "of", t.size, "max", float(t.max()))
    with open(path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("saved", path)
