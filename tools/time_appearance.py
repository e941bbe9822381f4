"""Kernel times of the colour renderer with per-env appearance tables and cast shadows: hammer-v0,
8 192 envs, 64x64, one view and three views per launch (aw_render_views, rgb only, ss 1).

HIP events around each variant, after a warm-up of every variant, on the state after a short
random rollout from staggered episode phases (tools/time_views.py's regime).  Per view count:
  (off)      nothing set: k_views<TASK, true>, the kernel of the commit before appearance existed
  (tables)   per-env colour, light and look tables drawn by aw_appearance_sample, shadows off
  (shadows)  the model's records, shadows on
  (both)     per-env tables and shadows
The variants are timed in alternating rounds so that a drift of the machine hits all of them
alike (aw_set_appearance, which waits for the device, sits outside the timed interval); per
variant the median and the min / max of the per-round times are printed, then one JSON line with
the medians and the ratios against (off).  The sampler's own launch is timed too.

With AW_LIB pointing at a library of a commit without aw_set_appearance only (off) is timed: the
figure the others are compared with, from the same tool.

    python tools/time_appearance.py [--envs 8192] [--launches 50] [--rollout 30]
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
    from mj_envs_amd import _native, appearance
    from mj_envs_amd.render import free_camera, model_camera
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_appearance.py: no GPU (a kernel time is only measured on one)")

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
    rgb1, rgb3 = sim.empty(n, 1, H, W, 3, dtype=torch.uint8), sim.empty(n, 3, H, W, 3, dtype=torch.uint8)

    has_app = hasattr(_native.load(), "aw_set_appearance")
    modes = {"off": (False, False)}
    app = None
    if has_app:
        modes.update(tables=(True, False), shadows=(False, True), both=(True, True))
        app = appearance.Appearance(sim)
        lo, hi = appearance.ranges(m, rgb_jitter=0.1, light_pos=0.5, light_diffuse=(0.4, 1.0),
                                   background=((0, 0, 0), (1, 1, 1)), headlight=(0.2, 0.6))
        sim.appearance_sample(lo, hi, app.colors, app.lights, app.look, seed=11, draw=0)

    def select(mode):
        if has_app:
            tables, shadows = modes[mode]
            if tables:
                sim.set_appearance(app.colors, app.lights, app.look, shadows=shadows)
            else:
                sim.set_appearance(shadows=shadows)

    variants = {}
    for mode in modes:
        variants[f"{mode}_views_1"] = (mode, lambda: sim.render_views(views[:1], W, H, rgb=rgb1))
        variants[f"{mode}_views_3"] = (mode, lambda: sim.render_views(views, W, H, rgb=rgb3))
    if has_app:
        variants["sampler"] = ("off", lambda: sim.appearance_sample(lo, hi, app.colors, app.lights, app.look,
                                                                    seed=11, draw=1))
    for mode, fn in variants.values():
        select(mode)
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    times = {k: [] for k in variants}
    for _ in range(args.launches):
        for name, (mode, fn) in variants.items():
            select(mode)                                   # waits for the device: outside the interval
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            times[name].append(a.elapsed_time(b))
    select("off")
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:18s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} rounds)")
    ratios = {f"{mode}_over_off_{nv}": round(med[f"{mode}_views_{nv}"] / med[f"off_views_{nv}"], 3)
              for mode in modes if mode != "off" for nv in (1, 3)}
    print(json.dumps(dict(env=args.env, envs=n, width=W, height=H, rounds=args.launches,
                          ms={k: round(v, 4) for k, v in med.items()}, ratios=ratios,
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
