"""stage_crb takes the structure of M from the task's compiled dof tree (aw_trees.h), the solver stages
from the model table's dof_ancmask: aw_create must refuse a model whose table and compiled tree
disagree (aw_model_host.h check_tree).  The check compiled into a stand-alone host program
(tests/tree_check.cc) with the project's compiler and run on the CPU, as tests/test_model_build.py
drives the builder: the four shipped models pass; one flipped dof_ancmask bit or one changed
dof_parentid is an error with a message."""
import os
import subprocess

import pytest

from conftest import ENVS, load_task_model
from test_model_build import _set, edited

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def tree_check(tmp_path_factory):
    """run(table bytes, flip=None | (row, bit)) -> dict of the printed fields"""
    from __graft_entry__ import hipcc_path
    d = tmp_path_factory.mktemp("tree_check")
    exe = str(d / "tree_check")
    subprocess.run([hipcc_path(), "-x", "hip", "--offload-host-only", "-std=c++17", "-O1", "-o", exe,
                    os.path.join(HERE, "tree_check.cc")], check=True)

    def run(table: bytes, flip=None):
        path = str(d / "table.awmb")
        with open(path, "wb") as f:
            f.write(table)
        r = subprocess.run([exe, path, *([str(flip[0]), str(flip[1])] if flip else [])], capture_output=True, text=True)
        assert r.returncode == 0, f"exit {r.returncode}: {r.stderr[-2000:]}"
        head, msg = r.stdout.rstrip("\n").split(" msg=", 1)
        out = {k: int(v) for k, v in (kv.split("=") for kv in head.split())}
        out["msg"] = msg
        return out

    return run


@pytest.fixture(scope="module")
def tables():
    return {e: load_task_model(e).to_blob() for e in ENVS}


@pytest.mark.parametrize("env_id", ENVS)
def test_shipped_models_agree_with_their_compiled_tree(tree_check, tables, env_id):
    got = tree_check(tables[env_id])
    assert (got["build"], got["tree"], got["msg"]) == (0, 0, ""), got


def _nv(env_id):
    return int(load_task_model(env_id).nv)


# (row, bit) of the built dof_ancmask: an ancestor bit cleared (every task: dof 1 descends from dof
# 0), an unrelated bit set (the last dof is the object's or the door's, not under dof 2), a dof made
# its own ancestor, and a bit in the first unused row
FLIPS = {"ancestor cleared": lambda nv: (1, 0), "unrelated set": lambda nv: (nv - 1, 2),
         "self": lambda nv: (4, 4), "row past nv": lambda nv: (nv, 0) if nv < 36 else (3, 40)}


@pytest.mark.parametrize("flip", list(FLIPS))
@pytest.mark.parametrize("env_id", ENVS)
def test_one_flipped_ancmask_bit_is_rejected(tree_check, tables, env_id, flip):
    got = tree_check(tables[env_id], FLIPS[flip](_nv(env_id)))
    assert got["build"] == 0 and got["tree"] != 0, got
    assert "dof_ancmask" in got["msg"], got


@pytest.mark.parametrize("env_id", ENVS)
def test_one_changed_dof_parentid_is_rejected(tree_check, tables, env_id):
    """dof 2, then the last dof, hung under dof 0: still parents-first, so the builder accepts the
    table and builds consistent masks for it -- of another tree than the compiled one"""
    nv = _nv(env_id)
    for j, p in ((2, 0), (nv - 1, 0)):
        bad = edited(tables[env_id], _set("dof_parentid", j, p))
        assert bad != tables[env_id]
        got = tree_check(bad)
        assert got["build"] == 0 and got["tree"] != 0, got
        assert "tree" in got["msg"], got
