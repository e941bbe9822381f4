"""Kernel times of the camera renderers: hammer-v0, 8 192 envs, 64x64 (BASELINE config 5's size).

HIP events around 50 launches each of k_depth, k_rgb ss=1, k_rgb ss=1 + depth and k_rgb ss=2,
after a warm-up of every variant, on the state after a short random rollout from staggered
episode phases (the bench's regime).  The variants are timed in alternating rounds so that a
drift of the machine hits all of them alike; per variant the median and the min / max of the
per-launch times are printed, then one JSON line with the medians and their ratio to k_depth.

    python tools/time_render.py [--envs 8192] [--launches 50] [--rollout 30]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rollout", type=int, default=30)
    ap.add_argument("--env", default="hammer-v0")
    args = ap.parse_args()

    import numpy as np
    import torch
    from mj_envs_amd import _native
    from mj_envs_amd.render import free_camera
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_render.py: no GPU (a kernel time is only measured on one)")

    n, W, H = args.envs, 64, 64
    m = attach_task(load_model(args.env), args.env)
    sim = _native.Sim(m.to_blob(), n)
    obs = sim.empty(n, sim.obs_dim)
    sim.reset(obs, seed=11)
    sim.set_episode(ep_len=torch.from_numpy((np.arange(n) * 7919 % sim.horizon).astype(np.int32)).cuda())
    act = sim.empty(n, sim.nu)
    rew, done, goal = sim.empty(n), sim.empty(n, dtype=torch.uint8), sim.empty(n, dtype=torch.uint8)
    for k in range(args.rollout):
        sim.random_actions(act, 13, k)
        sim.step(act, obs, rew, done, goal, autoreset=True, seed=11)
    cam = free_camera(m, args.env, W, H)
    depth = sim.empty(n, H, W)
    rgb = sim.empty(n, H, W, 3, dtype=torch.uint8)
    variants = {
        "k_depth": lambda: sim.render_depth(depth, cam),
        "k_rgb_ss1": lambda: sim.render_rgb(rgb, cam, ss=1),
        "k_rgb_ss1_depth": lambda: sim.render_rgb(rgb, cam, ss=1, depth=depth),
        "k_rgb_ss2": lambda: sim.render_rgb(rgb, cam, ss=2),
    }
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.launches):
        evs = []
        for name, fn in variants.items():
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            evs.append((name, a, b))
        torch.cuda.synchronize()
        for name, a, b in evs:
            times[name].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:16s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} launches)")
    print(json.dumps(dict(env=args.env, envs=n, width=W, height=H, launches=args.launches,
                          ms={k: round(v, 4) for k, v in med.items()},
                          ratio_to_k_depth={k: round(v / med["k_depth"], 3) for k, v in med.items()},
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
