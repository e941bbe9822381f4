"""Batched mjData views (aw_set_data): what needs no GPU.

The GPU tests (tests/test_gpu_data.py) compare contact forces, qacc and qfrc_constraint against the
fp64 oracle on the DAPG grasp states of tests/sensor_states.py.  test_inputs_are_well_conditioned
asserts on the oracle alone that those states are not ones where the reference itself moves when
its input is rounded to fp32, so a GPU miss there is the GPU's.
"""
import types

import numpy as np
import pytest

import abi_header
from conftest import ENVS
import data_states as ds


@pytest.mark.parametrize("env_id", ENVS)
def test_inputs_are_well_conditioned(env_id):
    """fp64 inputs against the same inputs rounded to fp32, all 12 cases of the task: identical
    contact sets, ncon 1..12, no force component out of the GPU tests' tolerance, qacc and
    qfrc_constraint within 6e-5 relative; 41..117 row-carrying contacts per task"""
    r = ds.data_refs(env_id)
    rows = pressing = 0
    dims = set()
    worst_q = worst_f = 0.0
    for ex_k, rd_k in zip(r["step_exact"], r["step_f32"]):
        for ex, rd in zip(ex_k, rd_k):
            ce, cr = ex["contact"], rd["contact"]
            assert 1 <= ex["counts"][0] <= 12
            np.testing.assert_array_equal(ex["counts"][:2], rd["counts"][:2])
            p, miss, same, errs = ds.compare_contacts(cr, ce)
            assert same and miss == 0
            assert ds.force_ok(cr["force"], ce["force"]).all() and ds.force_ok(cr["torsion"], ce["torsion"]).all()
            rows += int((ce["efc_address"] >= 0).sum())
            pressing += p
            dims |= set(ce["dim"].tolist())
            worst_q = max(worst_q, ds.rel(rd["qacc"], ex["qacc"]), ds.rel(rd["qfrc_constraint"], ex["qfrc_constraint"]))
            worst_f = max([worst_f] + errs)
    print(f"{env_id}: {rows} row-carrying contacts, {pressing} pressing, condims {sorted(dims)}, qacc / qfrc_constraint "
          f"move {worst_q:.2e} relative, force components {worst_f:.2e} N under fp32 rounding")
    assert 41 <= rows <= 117
    assert pressing >= 40                       # the GPU test's floor holds on the reference itself
    assert worst_q <= 6e-5


def test_every_condim_occurs():
    """condim 1, 3 and 4 contacts all occur in the GPU tests' references"""
    dims = set()
    for env_id in ENVS:
        for k in ds.data_refs(env_id)["step_f32"]:
            for rec in k:
                dims.update(rec["contact"]["dim"].tolist())
    assert dims == {1, 3, 4}


def test_contact_force_decoder():
    """the numpy mj_contactForce on hand-made contacts"""
    from mj_envs_amd.data import contact_force_np, make_frame_np
    ef = np.array([9.0, 5.0, 1.0, 2.0, 4.0, 0.5, 1.5, 3.0, 1.0, 7.0, 2.0])
    mu = np.array([1.0, 0.5, 0.01])
    f, t = contact_force_np(1, 0, mu, ef)                     # condim 1: the row's force
    np.testing.assert_array_equal(f, [9.0, 0, 0]); assert t == 0.0
    f, t = contact_force_np(3, 1, mu, ef)                     # rows 1..4
    np.testing.assert_allclose(f, [5 + 1 + 2 + 4, (5 - 1) * 1.0, (2 - 4) * 0.5]); assert t == 0.0
    f, t = contact_force_np(4, 5, mu, ef)                     # rows 5..10
    np.testing.assert_allclose(f, [0.5 + 1.5 + 3 + 1 + 7 + 2, (0.5 - 1.5) * 1.0, (3 - 1) * 0.5])
    assert t == pytest.approx((7 - 2) * 0.01)
    f, t = contact_force_np(3, -1, mu, ef)                    # no rows
    assert not f.any() and t == 0.0
    # mju_makeFrame: orthonormal, right-handed, first row the normal; the y / z branch
    n = np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [0.6, 0.48, 0.64]])
    fr = make_frame_np(n)
    np.testing.assert_allclose(fr @ fr.transpose(0, 2, 1), np.tile(np.eye(3), (3, 1, 1)), atol=1e-12)
    np.testing.assert_allclose(np.linalg.det(fr), 1.0)
    np.testing.assert_array_equal(fr[:, 0], n)
    np.testing.assert_allclose(fr[0, 1], [0, 1, 0]); np.testing.assert_allclose(fr[1, 1], [0, 0, 1])


def test_decoder_reproduces_the_oracle_frames():
    """make_frame_np(normal) is the frame the oracle's contacts carry"""
    from mj_envs_amd.data import make_frame_np
    for rec in ds.data_refs("relocate-v0")["step_f32"][1]:
        c = rec["contact"]
        np.testing.assert_allclose(make_frame_np(c["normal"]), c["frame"], atol=1e-12)


def test_record_layout_matches_the_header():
    from mj_envs_amd import _native
    assert abi_header.prototypes()["aw_set_data"][0] == "int"
    assert "aw_set_data" in _native.EXPORTS and hasattr(_native.load(), "aw_set_data")
    enums, defines = abi_header.enums(), abi_header.defines()
    assert (enums["AW_DATA_KIN"], enums["AW_DATA_DYN"], enums["AW_DATA_CONTACT"]) == \
        (_native.AW_DATA_KIN, _native.AW_DATA_DYN, _native.AW_DATA_CONTACT) == (1, 2, 4)
    assert defines["AW_CONTACT_DWORDS"] == _native.AW_CONTACT_DWORDS == 16
    assert defines["AW_DATA_MAX_CONTACTS"] == _native.AW_DATA_MAX_CONTACTS == 128
    # the struct's members in order are the binding's fields, every one a pointer
    fields = abi_header.struct_fields("aw_data_bufs")
    assert all(t.endswith("*") for t, _ in fields)
    assert [k for _, k in fields] == [f[0] for f in _native.DataBufs._fields_]
    # the record: 12 floats then 4 int32, contiguous, in the header's order
    want = [("dist", 1, False), ("pos", 3, False), ("normal", 3, False), ("force", 3, False), ("torsion", 1, False),
            ("mu", 1, False), ("geom1", 1, True), ("geom2", 1, True), ("dim", 1, True), ("efc_address", 1, True)]
    at = 0
    for (name, n, is_int), (k, f) in zip(want, _native.CONTACT_FIELDS.items()):
        assert (k, f) == (name, (at, n, is_int))
        at += n
    assert at == _native.AW_CONTACT_DWORDS
    assert _native.AW_NDIMS == 21                      # existing entry points are as they were


def test_data_argument_handling():
    from mj_envs_amd import _native
    from mj_envs_amd.envs import AdroitVecEnv
    g = _native.data_groups
    assert g(False) == g(None) == g(0) == g(()) == 0
    assert g(True) == 7 and g(("kin", "dyn", "contact")) == 7
    assert g("kin") == 1 and g(["dyn"]) == 2 and g(("contact", "kin")) == 5 and g(6) == 6
    for bad in ("kinematics", ("kin", "forces"), 8, -1):
        with pytest.raises(ValueError):
            g(bad)
    # rejected before the model is loaded or the GPU touched
    with pytest.raises(ValueError, match="unknown group"):
        AdroitVecEnv("hammer-v0", 2, data=("kin", "contacts"))
    for k in (0, 129):
        with pytest.raises(ValueError, match="max_contacts"):
            AdroitVecEnv("hammer-v0", 2, data=True, max_contacts=k)


def test_make_env_forwards_config_data(monkeypatch):
    from mj_envs_amd import wrappers
    seen = {}

    class Stop(Exception):
        pass

    def fake(env_id, num_envs, **kw):
        seen.update(kw)
        raise Stop

    monkeypatch.setattr(wrappers, "AdroitVecEnv", fake)
    cfg = types.SimpleNamespace(env_name="door-v0", data=("kin", "contact"), max_contacts=8)
    with pytest.raises(Stop):
        wrappers.make_env(cfg, 2)
    assert seen["data"] == ("kin", "contact") and seen["max_contacts"] == 8 and seen["sensors"] is False
    seen.clear()
    with pytest.raises(Stop):
        wrappers.make_env(types.SimpleNamespace(env_name="door-v0"), 2)
    assert seen["data"] is False and seen["max_contacts"] == 32
