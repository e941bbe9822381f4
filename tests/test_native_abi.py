"""The C-ABI library loads and exports every entry point include/adroit_wave.h declares, and the
binding (mj_envs_amd/_native.py: ``ABI``, the constants, ``load()``, the argument checks) says what
the header says (no compute calls: this runs on the CPU-only build container)."""
import ctypes
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import abi_header
from conftest import REPO

# C scalar types of the header -> the ctypes type the binding must declare
SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}
RESTYPES = {"int": ctypes.c_int, "const char*": ctypes.c_char_p}
# header names of the per-env status flags -> the names the binding gives them
ST_NAMES = {"AW_ST_BADQPOS": "ST_BADQPOS", "AW_ST_BADQVEL": "ST_BADQVEL", "AW_ST_BADQACC": "ST_BADQACC",
            "AW_ST_CON_OVERFLOW": "ST_CON_OVERFLOW", "AW_ST_EFC_OVERFLOW": "ST_EFC_OVERFLOW", "AW_ST_WIDE": "ST_WIDE"}
REQUIRED = ("AW_NDIMS", "AW_DUMP_SIZE", "AW_DUMP_SIZE_WIDE", "AW_CAM_FLOATS", "AW_LOOK_FLOATS", "AW_MAX_VIEWS",
            "AW_COL_FLOATS", "AW_LIGHT_FLOATS", "AW_CLOUD_MAXCAND", "AW_FPS_MAXPOINTS", "AW_MAX_RAYS", "AW_DYN_MAXPOINTS",
            "AW_CONTACT_DWORDS", "AW_DATA_MAX_CONTACTS", "AW_DATA_KIN", "AW_DATA_DYN", "AW_DATA_CONTACT", "AW_PT_BODY",
            "AW_PT_BODYCOM", "AW_PT_SITE")


def declared_symbols():
    return sorted(abi_header.prototypes())


def mirrors():
    from mj_envs_amd import _native
    return {"aw_view": _native.View, "aw_dyn_point": _native.DynPoint, "aw_dyn_out": _native.DynOut,
            "aw_data_bufs": _native.DataBufs, "aw_appearance": _native.AppearanceBufs}


def test_header_declares_boundary():
    syms = declared_symbols()
    for s in ("aw_create", "aw_reset", "aw_step", "aw_get_state", "aw_set_state", "aw_status",
              "aw_destroy", "aw_last_error", "aw_task_eval", "aw_random_actions"):
        assert s in syms


def test_library_exports_all_symbols():
    from mj_envs_amd import _native
    lib = _native.load()
    for s in declared_symbols():
        assert hasattr(lib, s), s
        assert isinstance(getattr(lib, s), ctypes._CFuncPtr)
    assert set(declared_symbols()) == set(_native.EXPORTS)


def test_no_cpu_fallback_in_product():
    """The product package must not import the oracle (test infrastructure)."""
    pkg = os.path.join(REPO, "mj_envs_amd")
    for root, _, files in os.walk(pkg):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(root, f)).read()
                assert "pyoracle" not in txt and "from oracle" not in txt, f


def check_binding(abi):
    """every assertion of the binding-against-header test on a table ``abi`` (so that the test of
    the test below can hand in a spoiled one)"""
    protos = abi_header.prototypes()
    assert list(abi) == list(protos)                 # one entry per prototype, in the header's order
    for name, (ret, params) in protos.items():
        restype, argtypes = abi[name]
        assert restype is RESTYPES[ret], name
        assert len(argtypes) == len(params), name
        for got, decl in zip(argtypes, params):
            ctype = decl.rsplit(None, 1)[0] if " " in decl else decl     # the declaration without the name
            ctype = ctype[len("const "):] if ctype.startswith("const ") else ctype
            if ctype.endswith("*"):
                base = ctype.rstrip("*").strip()
                if base in mirrors():
                    assert ctype.count("*") == 1 and got is ctypes.POINTER(mirrors()[base]), (name, decl)
                else:
                    assert got is ctypes.c_void_p or issubclass(got, ctypes._Pointer), (name, decl)
            else:
                assert got is SCALARS[ctype], (name, decl)


def test_binding_matches_header():
    """ABI against the header's prototypes: the same functions, parameter counts, exact scalar types,
    pointers as c_void_p or POINTER(...), struct pointers as the POINTER of the mirror, the restype;
    and after load() every function object of the library carries exactly the table's types"""
    from mj_envs_amd import _native
    check_binding(_native.ABI)
    assert _native.EXPORTS == tuple(_native.ABI)
    lib = _native.load()
    for name, (restype, argtypes) in _native.ABI.items():
        fn = getattr(lib, name)
        assert fn.restype is restype and list(fn.argtypes) == list(argtypes), name
    # a mirror has the header's fields in the header's order
    for cname, mirror in mirrors().items():
        assert [k.partition("[")[0] for _, k in abi_header.struct_fields(cname)] == [f[0] for f in mirror._fields_], cname
    assert ctypes.sizeof(_native.View) == 4 * abi_header.defines()["AW_CAM_FLOATS"] + 4


def test_binding_check_notices_a_wrong_table():
    """the check above fails on a truncated uint64_t, a missing entry and a struct pointer left untyped"""
    from mj_envs_amd import _native
    abi = dict(_native.ABI)
    args = list(abi["aw_reset"][1])
    args[3] = ctypes.c_int
    with pytest.raises(AssertionError):
        check_binding({**abi, "aw_reset": (ctypes.c_int, args)})
    with pytest.raises(AssertionError):
        check_binding({k: v for k, v in abi.items() if k != "aw_cast_rays"})
    args = list(abi["aw_render_views"][1])
    args[1] = ctypes.c_void_p
    with pytest.raises(AssertionError):
        check_binding({**abi, "aw_render_views": (ctypes.c_int, args)})


def test_constants_match_header():
    """every integer #define AW_* and every enumerator that _native defines under the same name (the
    AW_ST_* flags as ST_*) has the header's value, and the ones the binding relies on are there"""
    from mj_envs_amd import _native
    values = {**abi_header.defines(), **abi_header.enums()}
    for name in REQUIRED + tuple(ST_NAMES):
        assert name in values, name
    for name in REQUIRED:
        assert hasattr(_native, name), name
    checked = 0
    for name, v in values.items():
        ours = ST_NAMES.get(name, name)
        if hasattr(_native, ours):
            assert getattr(_native, ours) == v, name
            checked += 1
        else:
            assert name not in ST_NAMES, name
    assert checked >= len(REQUIRED) + len(ST_NAMES)


class StandIn:
    """a library object with every function of the table but ``lacking``"""

    def __init__(self, names, lacking):
        for k in names:
            if k not in lacking:
                setattr(self, k, types.SimpleNamespace())


def test_missing_symbol_rule(monkeypatch):
    """a symbol the library lacks: skipped with AW_LIB set (a diagnostic build), NativeError naming
    every one without (the product library)"""
    from mj_envs_amd import _native
    lacking = ("aw_set_rays", "aw_midphase_test")
    lib = StandIn(_native.ABI, lacking)
    monkeypatch.setattr(ctypes, "CDLL", lambda path: lib)
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.setenv("AW_LIB", _native.LIB_PATH)
    assert _native.load() is lib
    for name, (restype, argtypes) in _native.ABI.items():
        if name in lacking:
            assert not hasattr(lib, name)
        else:
            fn = getattr(lib, name)
            assert fn.restype is restype and fn.argtypes == argtypes, name
    monkeypatch.setattr(_native, "_lib", None)
    monkeypatch.delenv("AW_LIB")
    with pytest.raises(_native.NativeError) as e:
        _native.load()
    assert all(name in str(e.value) for name in lacking)
    assert _native._lib is None


def test_dev_refuses_host_tensors_and_none():
    """_dev on the CPU: a host tensor fails the device test whatever else holds; None passes only
    where optional"""
    import torch
    from mj_envs_amd import _native
    t = torch.zeros(2, 3)
    with pytest.raises(AssertionError, match=r"render_depth: out must be a device torch.float32 \[2, \*\]"):
        _native._dev(t, "render_depth: out", torch.float32, (2, None))
    with pytest.raises(AssertionError, match="set_data: xpos must be a device torch.float32$"):
        _native._dev(t, "set_data: xpos", torch.float32, None, optional=False)
    with pytest.raises(AssertionError):
        _native._dev(np.zeros((2, 3), np.float32), "call: x", torch.float32, (2, 3))
    with pytest.raises(AssertionError, match="sensordata: out must be"):
        _native._dev(None, "sensordata: out", torch.float32, (2, 3), optional=False)
    assert _native._dev(None, "cast_rays: entry", torch.int32, (2, 3)) is None
    # the calls without a handle go through it too
    with pytest.raises(AssertionError, match="cloud_fps: xyz"):
        _native.cloud_fps(torch.zeros(1, 4, 3), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 2, 3))


def test_views_and_records():
    from mj_envs_amd import _native
    cam = np.arange(_native.AW_CAM_FLOATS, dtype=np.float64)
    arr, nv = _native._views_arg([(cam, 0), (cam[::-1].reshape(1, -1), 5)], "render_views")
    assert nv == 2 and len(arr) == 2 and isinstance(arr[0], _native.View)
    assert list(arr[0].rec) == cam.tolist() and arr[0].body == 0
    assert list(arr[1].rec) == cam[::-1].tolist() and arr[1].body == 5
    arr, nv = _native._views_arg([], "render_views")          # (the library refuses nviews 0; the array is never empty)
    assert nv == 0 and len(arr) == 1
    with pytest.raises(AssertionError, match="render_cloud: a camera record has 17 floats"):
        _native._views_arg([(cam[:-1], 0)], "render_cloud")
    look = _native._record([0, 0, 0, 0.1, 0.4, 0.5, 1], _native.AW_LOOK_FLOATS, "render_rgb: look record")
    assert look.dtype == np.float32 and look.shape == (7,) and look.flags.c_contiguous
    assert _native._record(None, 6, "render_cloud: box") is None
    assert _native._record(np.zeros((2, 3)), 6, "render_cloud: box").shape == (6,)
    for bad in (np.zeros(5), np.zeros(7), np.zeros((2, 6))):
        with pytest.raises(AssertionError, match="render_cloud: box has 6 floats"):
            _native._record(bad, 6, "render_cloud: box")


def test_checks_survive_python_O():
    """the checks are raised, not asserted: an interpreter started with -O still refuses"""
    code = ("import numpy as np, torch\n"
            "from mj_envs_amd import _native\n"
            "print('debug', __debug__)\n"
            "for f in (lambda: _native._dev(torch.zeros(2), 'call: x', torch.float32, (2,)),\n"
            "          lambda: _native._record(np.zeros(5), 6, 'call: box'),\n"
            "          lambda: _native._views_arg([(np.zeros(3), 0)], 'call')):\n"
            "    try:\n"
            "        f()\n"
            "        print('passed')\n"
            "    except AssertionError as e:\n"
            "        print('raised', e)\n")
    r = subprocess.run([sys.executable, "-O", "-c", code], cwd=REPO, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().splitlines()
    assert lines[0] == "debug False"
    assert len(lines) == 4 and all(ln.startswith("raised call") for ln in lines[1:]), lines
