"""Bitwise pin of the env-step (GPU box): per task, 128 envs run 20 env-steps under random actions
and 60 in the DAPG closed loop with auto-reset (tools/rollout_bits.py), and the SHA-256 of every
step's obs and of the final qpos / qvel must equal tests/golden/rollout_bits.json -- recorded from
the library of the commit named in that file, the parent of the last kernel change, never from the
code under test.  A kernel change that keeps the arithmetic (the same IEEE operations on the same
values in the same order) passes unchanged.

hammer-v0's DAPG rollout must also show a nonzero nail-impact entry among the hashed obs: a touch
sensor stuck at zero in the reference recording and in the code under test alike cannot pass."""
import importlib.util
import json
import os

import numpy as np
import pytest

from conftest import ENVS, GOLDEN, REPO

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def bits():
    spec = importlib.util.spec_from_file_location("rollout_bits", os.path.join(REPO, "tools", "rollout_bits.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def recorded():
    with open(os.path.join(GOLDEN, "rollout_bits.json")) as f:
        return json.load(f)


@pytest.mark.parametrize("env_id", ENVS)
def test_rollout_bits(env_id, bits, recorded):
    assert recorded["envs"] == bits.N_ENVS and recorded["steps"] == bits.STEPS
    assert len(recorded["commit"]) >= 7          # the commit whose library was recorded
    fp, dapg_obs = bits.fingerprint(env_id)
    ref = recorded["tasks"][env_id]
    for pol in ("random", "dapg"):
        assert len(fp[pol]["obs"]) == bits.STEPS[pol]
        first = next((k for k, (a, b) in enumerate(zip(fp[pol]["obs"], ref[pol]["obs"])) if a != b), None)
        assert first is None, f"{env_id} {pol}: obs differ from commit {recorded['commit']} at step {first}"
        assert fp[pol]["qpos"] == ref[pol]["qpos"], f"{env_id} {pol}: final qpos differs"
        assert fp[pol]["qvel"] == ref[pol]["qvel"], f"{env_id} {pol}: final qvel differs"
    if env_id == "hammer-v0":
        t = bits.nail_impact(dapg_obs)
        print("hammer-v0 DAPG nail-impact entries: nonzero", int((t != 0).sum()), "of", t.size)
        assert np.isfinite(t).all() and (t != 0).any(), "no nail impact in the hashed hammer DAPG obs"
