"""Sampling-based planning on the simulator itself: branch B root states into B x K rollouts.

``Shooter`` owns a planner batch of ``roots * samples`` envs.  ``evaluate`` sets env ``b * K + k``
from root ``b`` in one ``aw_set_state_ids`` call (``rows = branch_rows(B, K)``: the B x K states
are never materialised), steps the batch under the given action sequences and returns each
sequence's return -- the inner loop of random shooting, MPPI and CEM.  The root states may come
from another handle's ``get_state`` (the envs being controlled).  No kernels of its own.
"""
from __future__ import annotations

from typing import Optional

import numpy as np

STATE_KEYS = ("qpos", "qvel", "qacc_warmstart", "params")


def branch_rows(B: int, K: int) -> np.ndarray:
    """row of the root that planner env i branches from: ``arange(B * K) // K`` (int32)"""
    return (np.arange(int(B) * int(K)) // int(K)).astype(np.int32)


def check_evaluate_args(actions_shape, roots: int, samples: int, nu: int, horizon: int, state_shapes=None,
                        widths=None) -> int:
    """``Shooter.evaluate``'s argument checks on shapes alone (nothing touches the GPU); returns H.
    actions_shape: [H, roots, samples, nu] with 1 <= H < horizon (an episode that ran into the
    horizon would be truncated inside the rollout).  state_shapes / widths: the root state's shapes
    by key and the planner's row widths by key (a params width that differs is another variation
    type's state)."""
    shp = tuple(int(x) for x in actions_shape)
    if len(shp) != 4:
        raise ValueError(f"evaluate: actions must be [H, {roots}, {samples}, {nu}], not rank {len(shp)}")
    if shp[1:] != (roots, samples, nu):
        raise ValueError(f"evaluate: actions must be [H, {roots}, {samples}, {nu}], not {list(shp)}")
    H = shp[0]
    if H < 1:
        raise ValueError("evaluate: actions hold no step")
    if horizon > 0 and H >= horizon:
        raise ValueError(f"evaluate: {H} steps reach the task's horizon ({horizon})")
    for k, s in (state_shapes or {}).items():
        if k not in (widths or {}):
            raise ValueError(f"evaluate: root_state has no field {k!r} (one of {list(STATE_KEYS)})")
        if tuple(s) != (roots, widths[k]):
            raise ValueError(f"evaluate: root_state[{k!r}] must be [{roots}, {widths[k]}], not {list(s)}")
    return H


class Shooter:
    """``roots`` x ``samples`` planner envs of ``env_id`` on GPU ``device`` (autoreset off)."""

    def __init__(self, env_id: str, roots: int, samples: int, device: int = 0, variation_type: Optional[str] = None):
        import torch
        from .envs import AdroitVecEnv
        self.roots, self.samples = int(roots), int(samples)
        if self.roots < 1 or self.samples < 1:
            raise ValueError("Shooter: roots and samples must be >= 1")
        n = self.roots * self.samples
        self.env = AdroitVecEnv(env_id, n, device=device, variation_type=variation_type, autoreset=False)
        dev = self.env.sim.torch_device
        self._ids = torch.arange(n, dtype=torch.int32, device=dev)
        self._rows = torch.as_tensor(branch_rows(self.roots, self.samples), device=dev)
        e = self.env
        self._widths = dict(qpos=e.nq, qvel=e.nv, qacc_warmstart=e.nv, params=e.nparam)
        e.reset()

    def check_args(self, root_state, actions) -> int:
        e = self.env
        return check_evaluate_args(actions.shape, self.roots, self.samples, e.nu, e.horizon,
                                   {k: v.shape for k, v in root_state.items() if v is not None}, self._widths)

    def evaluate(self, root_state, actions):
        """root_state: dict of [B, ...] device tensors as ``AdroitVecEnv.get_state`` returns them (a
        field left out or None keeps the planner envs' own values); actions [H, B, K, nu] (device,
        fp32).  Sets planner env b K + k from root b with its episode counters at zero, steps H times
        and returns ``(returns [B, K] fp32, goal_steps [B, K] int32, terminated [B, K] bool)``:
        the step rewards added in step order from zero, the steps with the goal achieved, and whether
        any step terminated."""
        import torch
        H = self.check_args(root_state, actions)
        e, B, K = self.env, self.roots, self.samples
        st = {k: v for k, v in root_state.items() if v is not None}
        e.set_state(**st, env_ids=self._ids, rows=self._rows, reset_episode=True)
        dev = e.sim.torch_device
        act = actions.to(device=dev, dtype=torch.float32).contiguous().view(H, B * K, e.nu)
        ret = torch.zeros(B * K, device=dev)
        goal_steps = torch.zeros(B * K, dtype=torch.int32, device=dev)
        term = torch.zeros(B * K, dtype=torch.bool, device=dev)
        for h in range(H):
            _, r, t, _, info = e.step(act[h])
            ret = ret + r
            goal_steps = goal_steps + info["goal_achieved"].to(torch.int32)
            term = term | t
        return ret.view(B, K), goal_steps.view(B, K), term.view(B, K)

    def close(self):
        self.env.close()
