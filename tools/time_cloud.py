"""Kernel times of the point-cloud observation against the segmentation renderer and against
farthest-point sampling written in torch: hammer-v0, 8 192 envs, 64x64, 512 points.

HIP events around each variant, after a warm-up of every variant, on the state after a short
random rollout from staggered episode phases (tools/time_labels.py's regime).  Variants, with one
view (the free camera) and with three (free camera, vil_camera, fixed):
  labels_depth_1 / _3   aw_render_labels with the depth frames: existing code, the baseline of k_cloud
  cloud_1 / _3          aw_render_cloud (k_cloud): the hand, the object and the nail board kept, cropped
                        to render.workspace_box, --cap slots per env
  fps_1 / _3            aw_cloud_fps (k_fps) on those candidates, 512 points
  torch_fps_1 / _3      the same sampling as the batched torch loop a user would write: per selection
                        one distance pass over [envs, cap], a running minimum and an argmax -- about
                        six launches per selected point
The HIP variants are timed in alternating rounds so that a drift of the machine hits all of them
alike; the torch loop (thousands of launches per call) is timed --torch-rounds times after them.
Per variant the median and the min / max are printed, the candidate counts, how many of the torch
loop's selections k_fps shares, then one JSON line with the medians and the ratios.

    python tools/time_cloud.py [--envs 8192] [--launches 50] [--rollout 30] [--cap 2048] [--points 512]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_fps(xyz, count, npoints):
    """farthest-point sampling of xyz [n, cap, 3] with count [n] valid rows each -> int64 [n, npoints]
    (selection 0 is candidate 0; rows shorter than npoints repeat their last maxima)"""
    import torch
    n, cap, _ = xyz.shape
    rows = torch.arange(n, device=xyz.device)
    valid = torch.arange(cap, device=xyz.device)[None] < count.clamp(max=cap)[:, None]
    mind = torch.where(valid, torch.full_like(xyz[..., 0], float("inf")), torch.full_like(xyz[..., 0], -1.0))
    last = torch.zeros(n, dtype=torch.long, device=xyz.device)
    sel = torch.zeros(n, npoints, dtype=torch.long, device=xyz.device)
    for k in range(1, npoints):
        d = xyz - xyz[rows, last][:, None]
        sq = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
        mind = torch.where(valid, torch.minimum(mind, sq), mind)
        last = mind.argmax(1)
        sel[:, k] = last
    return sel


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--launches", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--rollout", type=int, default=30)
    ap.add_argument("--cap", type=int, default=2048)
    ap.add_argument("--points", type=int, default=512)
    ap.add_argument("--torch-rounds", type=int, default=3)
    ap.add_argument("--env", default="hammer-v0")
    args = ap.parse_args()

    import numpy as np
    import torch
    from mj_envs_amd import _native, labels
    from mj_envs_amd.render import free_camera, model_camera, workspace_box
    from mj_envs_amd.tasks import attach_task, load_model
    if not torch.cuda.is_available():
        raise SystemExit("time_cloud.py: no GPU (a kernel time is only measured on one)")

    n, W, H, cap, P = args.envs, 64, 64, args.cap, args.points
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
    roots = [b for b in ("forearm", "Object", "nail_board", "frame") if b in m.names["body"]]
    keep, box = labels.keep_table(m, roots), workspace_box(args.env, m)
    depth = {v: sim.empty(n, v, H, W) for v in (1, 3)}
    lab = {v: sim.empty(n, v, H, W, dtype=torch.int32) for v in (1, 3)}
    xyz = {v: sim.empty(n, cap, 3) for v in (1, 3)}
    cnt = {v: torch.zeros(n, dtype=torch.int32, device=sim.torch_device) for v in (1, 3)}
    out = sim.empty(n, P, 3)
    idx = sim.empty(n, P, dtype=torch.int32)

    variants = {}
    for v in (1, 3):
        vs = views[:v]
        variants[f"labels_depth_{v}"] = lambda vs=vs, v=v: sim.render_labels(vs, W, H, lab[v], depth=depth[v])
        variants[f"cloud_{v}"] = lambda vs=vs, v=v: sim.render_cloud(vs, W, H, xyz[v], cnt[v], keep=keep, box=box)
        variants[f"fps_{v}"] = lambda v=v: _native.cloud_fps(xyz[v], cnt[v], out, idx)
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        return a, b, r

    times = {k: [] for k in variants}
    for _ in range(args.launches):
        evs = [(name, *timed(fn)[:2]) for name, fn in variants.items()]
        torch.cuda.synchronize()
        for name, a, b in evs:
            times[name].append(a.elapsed_time(b))
    shared = {}
    for v in (1, 3):
        c = cnt[v].clamp(max=cap)
        print(f"candidates_{v}: mean {float(cnt[v].float().mean()):.1f}  min {int(cnt[v].min())}  max {int(cnt[v].max())}"
              f"  (cap {cap}; {int((cnt[v] > cap).sum())} envs truncated, {int((c < P).sum())} with fewer than {P})")
        _native.cloud_fps(xyz[v], cnt[v], out, idx)
        torch_fps(xyz[v], cnt[v], P)                               # warm-up
        torch.cuda.synchronize()
        times[f"torch_fps_{v}"] = []
        for _ in range(args.torch_rounds):
            a, b, sel = timed(lambda: torch_fps(xyz[v], cnt[v], P))
            torch.cuda.synchronize()
            times[f"torch_fps_{v}"].append(a.elapsed_time(b))
        full = c >= P
        shared[v] = float((sel[full] == idx[full].long()).float().mean()) if bool(full.any()) else float("nan")
        print(f"selections_{v}: k_fps and the torch loop agree on {shared[v]:.5f} of the selections of the "
              f"{int(full.sum())} envs with >= {P} candidates")
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:20s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} rounds)")
    ratios = {}
    for v in (1, 3):
        ratios[f"cloud_{v}_over_labels_depth"] = round(med[f"cloud_{v}"] / med[f"labels_depth_{v}"], 3)
        ratios[f"torch_fps_{v}_over_fps"] = round(med[f"torch_fps_{v}"] / med[f"fps_{v}"], 1)
    print(json.dumps(dict(env=args.env, envs=n, width=W, height=H, cap=cap, points=P, rounds=args.launches,
                          torch_rounds=args.torch_rounds, ms={k: round(v, 4) for k, v in med.items()}, ratios=ratios,
                          selections_shared={str(v): round(s, 5) for v, s in shared.items()},
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
