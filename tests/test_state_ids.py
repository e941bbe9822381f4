"""Indexed state access (aw_set_state_ids / aw_get_state_ids / aw_clone_envs) and the planning
helpers, as far as they go without a GPU: the symbols, the NULL-handle errors, the host-side id
checks and the Shooter's argument checks."""
import numpy as np
import pytest

import abi_header

CALLS = ("aw_set_state_ids", "aw_get_state_ids", "aw_clone_envs")
AW_EINVAL = -1


def test_symbols_declared_exported_listed():
    from mj_envs_amd import _native
    declared = abi_header.prototypes()
    lib = _native.load()
    for s in CALLS:
        assert s in declared and declared[s][0] == "int", s
        assert hasattr(lib, s), s
        assert s in _native.EXPORTS, s


def test_null_handle_is_einval():
    from mj_envs_amd import _native
    lib = _native.load()
    assert lib.aw_set_state_ids(None, None, 1, None, 1, None, None, None, None, 0, None, None) == AW_EINVAL
    assert b"aw_set_state_ids" in lib.aw_last_error()
    assert lib.aw_get_state_ids(None, None, 1, None, None, None, None, None) == AW_EINVAL
    assert b"aw_get_state_ids" in lib.aw_last_error()
    assert lib.aw_clone_envs(None, None, None, 1, 1, None, None) == AW_EINVAL
    assert b"aw_clone_envs" in lib.aw_last_error()


def test_check_ids_accepts_valid():
    from mj_envs_amd._native import check_ids
    out = check_ids([3, 0, 9, 15], 16, "env_ids")
    assert out.dtype == np.int32 and out.tolist() == [3, 0, 9, 15]
    assert check_ids(np.array([5, 5, 5]), 16, "rows", distinct=False).tolist() == [5, 5, 5]


@pytest.mark.parametrize("ids", [[1, 2, 1], [-1, 2], [0, 16], np.array([0.0, 1.0])],
                         ids=["duplicate", "negative", "n", "float"])
def test_check_ids_raises(ids):
    from mj_envs_amd._native import check_ids
    with pytest.raises(ValueError):
        check_ids(ids, 16, "env_ids")


def test_branch_rows():
    from mj_envs_amd.planning import branch_rows
    assert branch_rows(3, 4).tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2]


def test_shooter_argument_checks():
    from mj_envs_amd.planning import check_evaluate_args
    B, K, nu, horizon = 2, 4, 30, 200
    assert check_evaluate_args((3, B, K, nu), B, K, nu, horizon) == 3
    for bad in ((3, B * K, nu), (3, B + 1, K, nu), (3, B, K + 1, nu), (3, B, K, nu - 1), (horizon, B, K, nu),
                (horizon + 5, B, K, nu)):
        with pytest.raises(ValueError):
            check_evaluate_args(bad, B, K, nu, horizon)
    widths = dict(qpos=36, qvel=36, qacc_warmstart=36, params=6)
    ok = dict(qpos=(B, 36), params=(B, 6))
    assert check_evaluate_args((3, B, K, nu), B, K, nu, horizon, ok, widths) == 3
    with pytest.raises(ValueError):      # another variation type's params
        check_evaluate_args((3, B, K, nu), B, K, nu, horizon, dict(params=(B, 3)), widths)
    with pytest.raises(ValueError):
        check_evaluate_args((3, B, K, nu), B, K, nu, horizon, dict(qpos=(B + 1, 36)), widths)
