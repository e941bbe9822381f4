"""Kernel times of the segmentation renderer against the depth-only views: hammer-v0, 8 192 envs,
64x64.

HIP events around each variant, after a warm-up of every variant, on the state after a short
random rollout from staggered episode phases (tools/time_views.py's regime).  Variants:
  depth_views_1 / _3    aw_render_views depth-only, one view (the free camera) / three views (free
                        camera, vil_camera, fixed): existing code, the baseline
  labels_1 / _3         aw_render_labels, the same views, geoms only
  labels_depth_1 / _3   the same with the depth frames written too
  labels_sites_1 / _3   the same views with the visible sites drawn
  labels_subset64_3     three views of a 64-env subset (env_ids)
The variants are timed in alternating rounds so that a drift of the machine hits all of them
alike; per variant the median and the min / max of the per-round times are printed, then one JSON
line with the medians and the ratios labels / depth-only views.

    python tools/time_labels.py [--envs 8192] [--launches 50] [--rollout 30]
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
    from mj_envs_amd.render import free_camera, model_camera
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_labels.py: no GPU (a kernel time is only measured on one)")

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
    views = [(free_camera(m, args.env, W, H), 0), model_camera(m, "vil_camera", W, H), model_camera(m, "fixed", W, H)]
    nsub = min(64, n)
    ids = torch.from_numpy((np.arange(nsub) * (n // nsub)).astype(np.int32)).cuda()
    depth = {v: sim.empty(n, v, H, W) for v in (1, 3)}
    lab = {v: sim.empty(n, v, H, W, dtype=torch.int32) for v in (1, 3)}
    lab_sub = sim.empty(nsub, 3, H, W, dtype=torch.int32)

    variants = {}
    for v in (1, 3):
        vs = views[:v]
        variants[f"depth_views_{v}"] = lambda vs=vs, v=v: sim.render_views(vs, W, H, depth=depth[v])
        variants[f"labels_{v}"] = lambda vs=vs, v=v: sim.render_labels(vs, W, H, lab[v])
        variants[f"labels_depth_{v}"] = lambda vs=vs, v=v: sim.render_labels(vs, W, H, lab[v], depth=depth[v])
        variants[f"labels_sites_{v}"] = lambda vs=vs, v=v: sim.render_labels(vs, W, H, lab[v], sites=1)
    variants["labels_subset64_3"] = lambda: sim.render_labels(views, W, H, lab_sub, env_ids=ids)
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
        print(f"{k:20s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} rounds)")
    ratios = {f"{k}_{v}_over_depth_views": round(med[f"{k}_{v}"] / med[f"depth_views_{v}"], 3)
              for k in ("labels", "labels_depth", "labels_sites") for v in (1, 3)}
    print(json.dumps(dict(env=args.env, envs=n, subset=nsub, width=W, height=H, rounds=args.launches,
                          ms={k: round(v, 4) for k, v in med.items()}, ratios=ratios,
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
