"""Cost of the sensor stage: k_step per env-step with sensors on against off, hammer-v0, 4 096 envs
under the reference's pretrained DAPG policy (mean actions from the on-device MLP, the regime
where the touch pads fire).

Two handles of the same batch (same seeds, staggered episode phases, in-kernel auto-reset), one
with aw_set_sensors(1); the sensors have no side effects, so both run the same trajectories.  After
an untimed pre-roll the two are stepped alternately, HIP events around each aw_step launch (k_step
and the wide tier's drain), so that a drift of the machine hits both alike; per variant the
median and the min / max of the per-step times are printed, then one JSON line.

    python tools/time_sensors.py [--envs 4096] [--steps 100] [--preroll 100] [--env hammer-v0]
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
    args = ap.parse_args()

    import numpy as np
    import torch
    from mj_envs_amd import _native
    from mj_envs_amd.policy import GaussianMLP
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_sensors.py: no GPU (a kernel time is only measured on one)")

    n = args.envs
    m = attach_task(load_model(args.env), args.env)
    pol = GaussianMLP.from_npz(os.path.join(REPO, "tests", "golden", f"dapg_{args.env.split('-')[0]}.npz"))

    class Run:
        def __init__(self, sensors):
            self.sim = sim = _native.Sim(m.to_blob(), n)
            sim.set_sensors(sensors)
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

    runs = {"sensors_off": Run(False), "sensors_on": Run(True)}
    for k in range(args.preroll):
        for r in runs.values():
            r.step(k)
    torch.cuda.synchronize()
    for k in range(args.preroll, args.preroll + args.steps):
        evs = [(r, r.step(k, timed=True)) for r in runs.values()]
        torch.cuda.synchronize()
        for r, (a, b) in evs:
            r.ms.append(a.elapsed_time(b))
    assert torch.equal(runs["sensors_off"].obs, runs["sensors_on"].obs), "the sensors changed the trajectories"
    sd = runs["sensors_on"].sim.sensordata(runs["sensors_on"].sim.empty(n, runs["sensors_on"].sim.nsensordata))
    types = m.arrays["sensor_type"][np.argsort(m.arrays["sensor_adr"])]
    firing = float((sd[:, torch.as_tensor(np.flatnonzero(types == 0)).cuda()] > 0).sum(dim=1).float().mean())
    med = {k: float(np.median(r.ms)) for k, r in runs.items()}
    for k, r in runs.items():
        print(f"{k:12s} median {med[k]:.4f} ms  min {min(r.ms):.4f}  max {max(r.ms):.4f}  ({len(r.ms)} env-steps)")
    print(json.dumps(dict(env=args.env, envs=n, policy="dapg", steps=args.steps, preroll=args.preroll,
                          ms_per_env_step={k: round(v, 4) for k, v in med.items()},
                          on_over_off=round(med["sensors_on"] / med["sensors_off"], 4),
                          firing_pads_per_env=round(firing, 2), kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
