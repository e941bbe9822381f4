"""Kernel times of the multi-view renderer against the single-camera entry points: hammer-v0,
8 192 envs, 64x64.

HIP events around each variant, after a warm-up of every variant, on the state after a short
random rollout from staggered episode phases (tools/time_render.py's regime).  Colour and depth
each in these variants:
  (a) aw_render_rgb ss 1 / aw_render_depth            one launch, the free camera
  (b) aw_render_views, one free-camera view            the same frame through k_views
  (c) aw_render_views, three views                     free camera, vil_camera, fixed
  (d) three aw_render_rgb / aw_render_depth launches   the same three frames, one launch each
  (w) aw_render_views, three views                     free camera, vil_camera, the palm mount (a
      body-mounted view has no single-launch counterpart: for information)
The variants are timed in alternating rounds so that a drift of the machine hits all of them
alike; per variant the median and the min / max of the per-round times are printed, then one JSON
line with the medians and the ratios (b)/(a) and (c)/(d).

    python tools/time_views.py [--envs 8192] [--launches 50] [--rollout 30]
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
    from mj_envs_amd.render import free_camera, model_camera, mounted_camera
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_views.py: no GPU (a kernel time is only measured on one)")

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
    free = free_camera(m, args.env, W, H)
    views = [(free, 0), model_camera(m, "vil_camera", W, H), model_camera(m, "fixed", W, H)]
    wrist = views[:2] + [mounted_camera(m, "palm", (0.0, -0.15, 0.0), (0.0, 0.6, 0.8), (0.0, -0.8, 0.6), W, H, 90.0)]
    depth, rgb = sim.empty(n, H, W), sim.empty(n, H, W, 3, dtype=torch.uint8)
    depth1, rgb1 = sim.empty(n, 1, H, W), sim.empty(n, 1, H, W, 3, dtype=torch.uint8)
    depth3, rgb3 = sim.empty(n, 3, H, W), sim.empty(n, 3, H, W, 3, dtype=torch.uint8)

    def three(fn):
        for rec, _ in views:
            fn(rec)

    variants = {
        "rgb_a_render_rgb": lambda: sim.render_rgb(rgb, free, ss=1),
        "rgb_b_views_1": lambda: sim.render_views(views[:1], W, H, rgb=rgb1),
        "rgb_c_views_3": lambda: sim.render_views(views, W, H, rgb=rgb3),
        "rgb_d_render_rgb_x3": lambda: three(lambda rec: sim.render_rgb(rgb, rec, ss=1)),
        "rgb_w_views_3_wrist": lambda: sim.render_views(wrist, W, H, rgb=rgb3),
        "depth_a_render_depth": lambda: sim.render_depth(depth, free),
        "depth_b_views_1": lambda: sim.render_views(views[:1], W, H, depth=depth1),
        "depth_c_views_3": lambda: sim.render_views(views, W, H, depth=depth3),
        "depth_d_render_depth_x3": lambda: three(lambda rec: sim.render_depth(depth, rec)),
        "depth_w_views_3_wrist": lambda: sim.render_views(wrist, W, H, depth=depth3),
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
        print(f"{k:24s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} rounds)")
    ratios = {f"{p}_b_over_a": round(med[f"{p}_b_views_1"] / med[a], 3)
              for p, a in (("rgb", "rgb_a_render_rgb"), ("depth", "depth_a_render_depth"))}
    ratios.update({f"{p}_c_over_d": round(med[f"{p}_c_views_3"] / med[d], 3)
                   for p, d in (("rgb", "rgb_d_render_rgb_x3"), ("depth", "depth_d_render_depth_x3"))})
    print(json.dumps(dict(env=args.env, envs=n, width=W, height=H, rounds=args.launches,
                          ms={k: round(v, 4) for k, v in med.items()}, ratios=ratios,
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
