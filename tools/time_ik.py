"""Kernel time of the one-launch inverse kinematics (aw_solve_ik, k_ik) next to the torch loop over
aw_dynamics that it replaces: relocate-v0, 4 096 envs, 8 fixed iterations from the envs' own qpos.  Fixed:
tol = 0, and goals 0.3 m from the current poses with max_step = 0.02, so that no row can arrive (and
leave on a residual of exactly 0) within 8 steps; the tool checks that every row of both cases applied
all 8 updates before it prints a ratio.

  arm3     S_grasp's position on the six arm dofs (3 rows)
  hand21   five fingertip positions plus the palm site's pose on every actuated dof (21 rows)
Per case two variants:
  k_ik     one aw_solve_ik launch, max_iter 8
  loop     README.md's loop, 8 times: env.dynamics(point_pos, jacp[, jacr], qpos=q), J J' + damping I,
           torch.linalg.solve, the same step limit, the update.  aw_dynamics returns no orientations,
           so hand21's three orientation rows carry jacr with a zero residual: the launches, the HBM
           traffic and the linear algebra of 21 rows, not a converging orientation.
HIP events around each variant after a warm-up of every variant, in alternating rounds so that a drift
of the machine hits both alike; per variant the median and the min / max, then one JSON line with the
medians and loop / k_ik.  No gate rides on these numbers.

    python tools/time_ik.py [--envs 4096] [--launches 30] [--iters 8]
"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=4096)
    ap.add_argument("--launches", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--iters", type=int, default=8)
    args = ap.parse_args()

    import numpy as np
    import torch
    from mj_envs_amd import _native, ik
    from mj_envs_amd.dynamics import points
    from mj_envs_amd.envs import AdroitVecEnv
    if not torch.cuda.is_available():
        raise SystemExit("time_ik.py: no GPU (a kernel time is only measured on one)")

    n, K, lam, max_step = args.envs, args.iters, 1e-4, 0.02
    env = AdroitVecEnv("relocate-v0", n, autoreset=True)
    env.reset(seed=11)
    dev = env.sim.torch_device
    q0 = env.get_state()["qpos"].clone()
    tips = ["ffdistal", "mfdistal", "rfdistal", "lfdistal", "thdistal"]
    gen = torch.Generator(device=dev).manual_seed(5)
    cases = {}
    for name, tg, pts, mask in (
            ("arm3", ik.targets(env.model, sites=["S_grasp"]), points(env.model, sites=["S_grasp"]), 0x3F),
            ("hand21", ik.targets(env.model, sites=[("S_grasp", 1.0, 0.1)], bodies=tips),
             points(env.model, sites=["S_grasp"], bodies=tips), ik.dof_mask(env.model, actuated=True))):
        here = env.dynamics(pts, want=("point_pos",)).point_pos
        goal = torch.zeros(n, len(tg), 7, device=dev)
        off = 2 * torch.rand(here.shape, generator=gen, device=dev) - 1
        goal[..., :3] = here + 0.3 * off / off.norm(dim=-1, keepdim=True)
        goal[..., 3] = 1.0
        cols = torch.tensor([i for i in range(env.nv) if (mask >> i) & 1], device=dev)
        out = {k: torch.zeros((n,) + _native.ik_shape(k, env.nq, len(tg)), device=dev,
                              dtype=torch.int32 if k == "iters" else torch.float32) for k in _native.IK_OUTPUTS}
        cases[name] = dict(tg=tg, pts=pts, mask=mask, goal=goal, cols=cols, out=out, rot=tg.rows > 3 * len(tg))

    def k_ik(c):
        env.sim.solve_ik(c["out"], c["tg"].ik_records, c["goal"], c["mask"], max_iter=K, damping=lam, tol=0.0,
                         max_step=max_step)

    def loop(c):
        q, d = q0.clone(), c.get("dyn")
        eye = lam * torch.eye(c["tg"].rows, device=dev)
        for _ in range(K):
            d = env.dynamics(c["pts"], want=("point_pos", "jacp", "jacr") if c["rot"] else ("point_pos", "jacp"),
                             qpos=q, out=d)
            J = d.jacp_all[..., c["cols"]].reshape(n, -1, len(c["cols"]))
            e = (c["goal"][..., :3] - d.point_pos).reshape(n, -1)
            if c["rot"]:
                J = torch.cat([J, 0.1 * d.jacr(0)[..., c["cols"]]], dim=1)
                e = torch.cat([e, torch.zeros(n, 3, device=dev)], dim=1)
            dq = (J.mT @ torch.linalg.solve(J @ J.mT + eye, e[..., None]))[..., 0]
            q[:, c["cols"]] += dq * (max_step / dq.abs().amax(dim=1, keepdim=True)).clamp(max=1.0)
        c["dyn"] = d
        return q

    variants = {f"{name}_{v.__name__}": (lambda c=c, v=v: v(c)) for name, c in cases.items() for v in (k_ik, loop)}
    for fn in variants.values():
        for _ in range(args.warmup):
            fn()
    torch.cuda.synchronize()
    for name, c in cases.items():
        print(f"{name}: rows {c['tg'].rows}, dofs {len(c['cols'])}, k_ik iters {int(c['out']['iters'].min())}.."
              f"{int(c['out']['iters'].max())}, median err {float(c['out']['err'].median()):.2e}")
        if int(c["out"]["iters"].min()) != K:
            raise SystemExit(f"time_ik.py: {name}: a row left before {K} updates; the two variants would compare unequal work")

    def timed(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        return a, b

    times = {k: [] for k in variants}
    for _ in range(args.launches):
        evs = [(name, *timed(fn)) for name, fn in variants.items()]
        torch.cuda.synchronize()
        for name, a, b in evs:
            times[name].append(a.elapsed_time(b))
    med = {k: float(np.median(v)) for k, v in times.items()}
    for k, v in times.items():
        print(f"{k:14s} median {med[k]:.4f} ms  min {min(v):.4f}  max {max(v):.4f}  ({len(v)} rounds)")
    print(json.dumps(dict(env="relocate-v0", envs=n, iters=K, rounds=args.launches,
                          ms={k: round(v, 4) for k, v in med.items()},
                          loop_over_k_ik={name: round(med[f"{name}_loop"] / med[f"{name}_k_ik"], 2) for name in cases},
                          kernel_build=_native.kernel_build_id())))


if __name__ == "__main__":
    main()
