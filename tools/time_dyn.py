"""Kernel times of the dynamics queries (aw_dynamics, k_dyn) next to one k_step launch of the same
handle: hammer-v0, 4 096 envs.

HIP events around each variant, after a warm-up of every variant, on the state after a short random
rollout from staggered episode phases (tools/time_labels.py's regime).  Variants:
  all_4pts    every output, 4 points (palm site, fingertip body, the object body and its com), ctrl given
  jac_only    jacp and jacr of those points: kinematics and mj_comPos only
  m_only      qM: no points, no velocity stage
  step        one aw_step with random actions (autoreset), the same handle
The variants are timed in alternating rounds so that a drift of the machine hits all of them alike;
the step comes last in a round, so every dynamics launch of a round sees the same state.  Per variant
the median and the min / max are printed, then one JSON line with the medians and their ratios to the
step.  No gate rides on these numbers.

    python tools/time_dyn.py [--envs 4096] [--launches 50] [--rollout 30] [--env hammer-v0]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rollout", type=int, default=30)
    ap.add_argument("--env", default="hammer-v0")
    args = ap.parse_args()

    import numpy as np
    import torch
    from mj_envs_amd import _native
    from mj_envs_amd.dynamics import points
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_dyn.py: no GPU (a kernel time is only measured on one)")

    n = args.envs
    m = attach_task(load_model(args.env), args.env)
    sim = _native.Sim(m.to_blob(), n)
    obs = sim.empty(n, sim.obs_dim)
    sim.reset(obs, seed=11)
    sim.set_episode(ep_len=torch.from_numpy((np.arange(n) * 7919 % sim.horizon).astype(np.int32)).cuda())
    act = sim.empty(n, sim.nu)
    rew, done, goal = sim.empty(n), sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
    step_no = [0]

    def step():
        sim.random_actions(act, 13, step_no[0])
        step_no[0] += 1
        sim.step(act, obs, rew, done, goal, autoreset=True, seed=11)

    for _ in range(args.rollout):
        step()
    obj = "latch" if args.env == "door-v0" else "Object"
    pts = points(m, sites=["S_grasp"], bodies=["ffdistal", obj], body_coms=[obj]).records
    bufs = {k: sim.empty(n, *_native.dyn_shape(k, sim.nv, sim.nbody, len(pts))) for k in _native.DYN_OUTPUTS}
    qM = sim.empty(n, sim.nv, sim.nv)
    ctrl = torch.zeros(n, sim.nu, device=sim.torch_device)
    variants = {
        "all_4pts": lambda: sim.dynamics(bufs, pts, ctrl=ctrl),
        "jac_only": lambda: sim.dynamics({k: bufs[k] for k in ("jacp", "jacr")}, pts),
        "m_only": lambda: sim.dynamics(dict(qM=qM), []),
    }
    for fn in list(variants.values()) + [step]:
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    times = {k: [] for k in list(variants) + ["step"]}
    for _ in range(args.launches):
        evs = [(name, *timed(fn)) for name, fn in variants.items()]
        sim.random_actions(act, 13, step_no[0])          # (outside the step's events)
        step_no[0] += 1
        evs.append(("step", *timed(lambda: sim.step(act, obs, rew, done, goal, autoreset=True, seed=11))))
        torch.cuda.synchronize()
        for name, a, b in evs:
            times[name].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:10s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} rounds)")
    print(json.dumps(dict(env=args.env, envs=n, points=len(pts), rounds=args.launches,
                          ms={k: round(v, 4) for k, v in med.items()},
                          over_step={k: round(med[k] / med["step"], 3) for k in variants},
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
