"""Kernel times of the ray queries (aw_cast_rays, k_rays) next to the nearest existing way to cast a
few rays per env -- a depth-only aw_render_views of 8x8 pixels, 64 rays -- and to one k_step launch of
the same handle: hammer-v0, 4 096 envs.

HIP events around each variant, after a warm-up of every variant, on the state after a short random
rollout from staggered episode phases (tools/time_labels.py's regime).  Variants:
  fingers_60  a 12-ray fan of 30 degrees on each of the five S_*tip sites (the tip's own body excluded)
  full_256    those 60 and a 196-ray fan on the palm: the table's capacity
  subset      full_256 for N / 8 envs through env_ids
  per_env     full_256 with env_rays given (every env its own pnt / vec)
  depth_8x8   aw_render_views, depth only, one 8x8 view of the free camera
  step        one aw_step with random actions (autoreset), the same handle
The handle holds one table, so a round uploads each table before the variants that use it, outside
the events (aw_set_rays waits for the device).  The variants are timed in alternating rounds so that a
drift of the machine hits all of them alike; the step comes last in a round, so every cast of a round
sees the same state.  Per variant the median and the min / max are printed, then one JSON line with
the medians and their ratios to depth_8x8 and to the step.  No gate rides on these numbers.

    python tools/time_rays.py [--envs 4096] [--launches 50] [--rollout 30] [--env hammer-v0]
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
    from mj_envs_amd import _native, rays
    from mj_envs_amd.render import free_camera
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_rays.py: no GPU (a kernel time is only measured on one)")

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
    tips = [s for s in m.names["site"] if s.startswith("S_") and s.endswith("tip")]
    fingers = rays.concat(*[rays.fan(m, s, [0, 0, 1], 30.0, 12, bodyexclude=int(m.site_bodyid[m.name2id("site", s)]))
                            for s in tips])
    full = rays.concat(fingers, rays.fan(m, "palm", [0.0, -1.0, 0.3], 120.0, _native.AW_MAX_RAYS - len(fingers),
                                         bodyexclude="palm"))
    nsub = max(n // 8, 1)
    ids = torch.from_numpy((np.arange(nsub) * (n // nsub)).astype(np.int32)).cuda()
    er = np.zeros((n, len(full), 6), np.float32)
    er[..., :3], er[..., 3:] = full.records["pnt"], full.records["vec"]
    env_rays = torch.as_tensor(er, device=sim.torch_device)
    d60, e60 = sim.empty(n, len(fingers)), sim.empty(n, len(fingers), dtype=torch.int32)
    d256, e256 = sim.empty(n, len(full)), sim.empty(n, len(full), dtype=torch.int32)
    dsub, esub = sim.empty(nsub, len(full)), sim.empty(nsub, len(full), dtype=torch.int32)
    view = [(free_camera(m, args.env, 8, 8), 0)]
    depth = sim.empty(n, 1, 8, 8)
    # (table to upload first or None, variant)
    plan = [(fingers, "fingers_60", lambda: sim.cast_rays(d60, e60)),
            (full, "full_256", lambda: sim.cast_rays(d256, e256)),
            (None, "subset", lambda: sim.cast_rays(dsub, esub, env_ids=ids)),
            (None, "per_env", lambda: sim.cast_rays(d256, e256, env_rays=env_rays)),
            (None, "depth_8x8", lambda: sim.render_views(view, 8, 8, depth=depth))]
    for table, _, fn in plan:
        if table is not None:
            sim.set_rays(table.records)
        for _ in range(args.warmup):
            fn()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    names = [name for _, name, _ in plan]
    times = {k: [] for k in names + ["step"]}
    for _ in range(args.launches):
        evs = []
        for table, name, fn in plan:
            if table is not None:
                sim.set_rays(table.records)              # (outside the events; waits for the device)
            evs.append((name, *timed(fn)))
        sim.random_actions(act, 13, step_no[0])          # (outside the step's events)
        step_no[0] += 1
        evs.append(("step", *timed(lambda: sim.step(act, obs, rew, done, goal, autoreset=True, seed=11))))
        torch.cuda.synchronize()
        for name, a, b in evs:
            times[name].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:10s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} rounds)")
    print(json.dumps(dict(env=args.env, envs=n, subset=nsub, rays=dict(fingers_60=len(fingers), full_256=len(full)),
                          rounds=args.launches, ms={k: round(v, 4) for k, v in med.items()},
                          over_depth_8x8={k: round(med[k] / med["depth_8x8"], 3) for k in names if k != "depth_8x8"},
                          over_step={k: round(med[k] / med["step"], 3) for k in names},
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
