"""Model compiler checks: dims vs SURVEY §2 / DAPG policy shapes, ctrl ranges, regeneration."""
import os

import numpy as np
import pytest

from conftest import ENVS, GOLDEN

# (nq, nu, obs_dim, frame_skip, horizon, nbody) -- SURVEY §2 per-task table; obs/act dims are
# also pinned by the DAPG pickles' param_shapes (46/26, 39/28, 45/24, 39/30)
EXPECTED = {
    "hammer-v0": (33, 26, 46, 5, 200, 31),
    "door-v0": (30, 28, 39, 1, 200, 31),
    "pen-v0": (30, 24, 45, 5, 100, 30),
    "relocate-v0": (36, 30, 39, 5, 200, 29),
}
# broadphase-independent candidate pairs (hammer/pen/relocate match SURVEY §2 exactly; door has
# 6 more: door/latch geoms vs the world-welded frame are not parent-filtered in MuJoCo)
CANDIDATES = {"hammer-v0": 238, "door-v0": 288, "pen-v0": 127, "relocate-v0": 107}


@pytest.mark.parametrize("env_id", ENVS)
def test_dims(env_id):
    from mj_envs_amd.tasks import TASKS, load_model
    m = load_model(env_id)
    nq, nu, obs, fs, hz, nb = EXPECTED[env_id]
    assert (m.nq, m.nv, m.nu, m.nbody) == (nq, nq, nu, nb)
    spec = TASKS[env_id]
    assert (spec.obs_dim, spec.frame_skip, spec.horizon, spec.nu) == (obs, fs, hz, nu)
    assert m.ncand == CANDIDATES[env_id]
    assert m.npair == 19                      # DAPG_assets.xml:71-91 (one pair listed twice)
    assert m.ntendon == 44


@pytest.mark.parametrize("env_id", ENVS)
def test_model_constants(env_id):
    from mj_envs_amd.tasks import load_model
    m = load_model(env_id)
    assert m.opt["timestep"] == 0.002 and m.opt["iterations"] == 20 and m.opt["noslip_iterations"] == 20
    # joint defaults (DAPG_assets.xml:12)
    hand = [i for i, n in enumerate(m.names["joint"]) if n.endswith(("J0", "J1", "J2", "J3", "J4"))]
    assert np.allclose(m.dof_armature[hand][2:], 0.001)
    assert np.all(m.dof_frictionloss > 0)
    assert np.all(m.dof_invweight0 > 0) and np.all(m.tendon_invweight0 > 0)
    # arm actuators are affine 500 ctrl - 200 q, hand 1 / -1, wrist 10 / -10
    wr = m.names["actuator"].index("A_WRJ1")
    assert m.actuator_gainprm[wr, 0] == 10 and m.actuator_biasprm[wr, 1] == -10
    ff = m.names["actuator"].index("A_FFJ3")
    assert m.actuator_gainprm[ff, 0] == 1 and m.actuator_biasprm[ff, 1] == -1
    assert np.all(m.actuator_ctrllimited == 1)
    assert np.all(m.body_mass[m.body_weldid > 0] > 0)


def test_pen_inertia_from_geoms():
    """pen Object has no <inertial>: mass = 1500 kg/m3 cylinder + 1000 kg/m3 cap/clip geoms."""
    from mj_envs_amd.tasks import load_model
    m = load_model("pen-v0")
    b = m.name2id("body", "Object")
    pen = 1500 * np.pi * 0.015 ** 2 * 0.13
    top = 1000 * np.pi * 0.017 ** 2 * 0.04
    bot = 1000 * np.pi * 0.013 ** 2 * 0.004
    cli = 1000 * 8 * 0.004 * 0.006 * 0.03
    assert m.body_mass[b] == pytest.approx(pen + top + bot + cli, rel=1e-12)


@pytest.mark.parametrize("env_id", ENVS)
def test_committed_model_matches_fresh_compile(env_id):
    """the committed model tables against a fresh compile of the reference's MJCF scenes
    (tests/golden/mjcf: the task files and the two files they include, stored as fixtures)"""
    from mj_envs_amd.mjcf import compile_mjcf
    from mj_envs_amd.tasks import TASKS, load_model
    fresh = compile_mjcf(os.path.join(GOLDEN, "mjcf", TASKS[env_id].xml))
    m = load_model(env_id)
    assert fresh.dims == m.dims
    for k, v in fresh.arrays.items():
        np.testing.assert_array_equal(v, m.arrays[k], err_msg=k)


def test_blob_roundtrip():
    from mj_envs_amd.tasks import attach_task, load_model
    m = attach_task(load_model("hammer-v0"), "hammer-v0")
    blob = m.to_blob()
    assert blob[:4] == b"AWMB"
    assert len(blob) < 200_000
