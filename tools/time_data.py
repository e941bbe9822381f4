"""Cost of the mjData output stage: k_step per env-step with data off against each group and all
groups, hammer-v0, 4 096 envs under the reference's pretrained DAPG policy (mean actions from the
on-device MLP, the regime where the hand grasps and the contact list is long).

Five handles of the same batch (same seeds, staggered episode phases, in-kernel auto-reset): data
off, AW_DATA_KIN, AW_DATA_DYN, AW_DATA_CONTACT, all three.  The stage has no side effects, so all run
the same trajectories.  After an untimed pre-roll they are stepped alternately, in an order that
rotates every step, HIP events around each aw_step launch (k_step and the wide tier's drain), so
that a drift of the machine hits all alike; per variant the median and the min / max of the
per-step times are printed, then one JSON line.

    python tools/time_data.py [--envs 4096] [--steps 100] [--preroll 100] [--env hammer-v0] [--max-contacts 32]
"""
import argparse
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--preroll", type=int, default=100)
    ap.add_argument("--env", default="hammer-v0")
    ap.add_argument("--max-contacts", type=int, default=32)
    args = ap.parse_args()

    import numpy as np
    import torch
    from mj_envs_amd import _native
    from mj_envs_amd.policy import GaussianMLP
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_data.py: no GPU (a kernel time is only measured on one)")

    n = args.envs
    m = attach_task(load_model(args.env), args.env)
    pol = GaussianMLP.from_npz(os.path.join(REPO, "tests", "golden", f"dapg_{args.env.split('-')[0]}.npz"))

    class Run:
        def __init__(self, groups):
            self.sim = sim = _native.Sim(m.to_blob(), n)
            self.bufs = sim.set_data(groups, args.max_contacts)
            self.obs, self.act, self.rew = sim.empty(n, sim.obs_dim), sim.empty(n, sim.nu), sim.empty(n)
            self.done, self.goal = sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
            sim.reset(self.obs, seed=11)
            sim.set_episode(ep_len=torch.from_numpy((np.arange(n) * 7919 % sim.horizon).astype(np.int32)).cuda())
            self.ms = []

        def step(self, k, timed=False):
            pol.act(self.obs, out=self.act, step=k)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            self.sim.step(self.act, self.obs, self.rew, self.done, self.goal, autoreset=True, seed=11)
            b.record()
            return (a, b) if timed else None

    runs = {"data_off": Run(0), "kin": Run(_native.AW_DATA_KIN), "dyn": Run(_native.AW_DATA_DYN),
            "contact": Run(_native.AW_DATA_CONTACT), "all": Run(_native.AW_DATA_ALL)}
    order = list(runs.values())
    for k in range(args.preroll):
        for r in order:
            r.step(k)
    torch.cuda.synchronize()
    for k in range(args.preroll, args.preroll + args.steps):
        rot = order[k % len(order):] + order[:k % len(order)]
        evs = [(r, r.step(k, timed=True)) for r in rot]
        torch.cuda.synchronize()
        for r, (a, b) in evs:
            r.ms.append(a.elapsed_time(b))
    for k, r in runs.items():
        assert torch.equal(runs["data_off"].obs, r.obs), f"data group {k} changed the trajectories"
    counts = runs["all"].bufs["counts"]
    ncon = counts[:, 0].float()
    med = {k: float(np.median(r.ms)) for k, r in runs.items()}
    for k, r in runs.items():
        print(f"{k:9s} median {med[k]:.4f} ms  min {min(r.ms):.4f}  max {max(r.ms):.4f}  "
              f"{100 * (med[k] / med['data_off'] - 1):+.2f} %  ({len(r.ms)} env-steps)")
    nb, ns, nv = runs["all"].sim.nbody, runs["all"].sim.nsite, runs["all"].sim.nv
    print(json.dumps(dict(env=args.env, envs=n, policy="dapg", steps=args.steps, preroll=args.preroll,
                          max_contacts=args.max_contacts,
                          ms_per_env_step={k: round(v, 4) for k, v in med.items()},
                          over_off={k: round(v / med["data_off"], 4) for k, v in med.items() if k != "data_off"},
                          mean_ncon=round(float(ncon.mean()), 2), max_ncon=int(ncon.max()),
                          bytes_per_env_step=dict(kin=4 * (7 * nb + 3 * ns), dyn=4 * (2 * nv + 4),
                                                  contact_mean=round(64 * float(ncon.clamp(max=args.max_contacts).mean()), 1)),
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
