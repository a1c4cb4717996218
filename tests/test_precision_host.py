"""CPU-only tests of the matmul precision tier's interface (include/mintime_hip.h: mt_gemm_set_precision / mt_gemm_get_precision;
lib.set_matmul_precision / get_matmul_precision, mintime_amd.matmul_precision).  No compute call is made: the setting is host state."""
import os
import subprocess
import sys

import pytest

import mintime_amd
from mintime_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module", autouse=True)
def _library():
    if not os.path.exists(lib.LIB_PATH):
        lib.build()
    yield
    lib.set_matmul_precision("highest")


def test_abi_version_agrees_in_header_binding_and_library():
    assert lib.ABI_VERSION == lib.header_version() == 123
    assert lib.get().mt_version() == 123
    assert "mt_gemm_set_precision" in lib.PROTOTYPES and "mt_gemm_get_precision" in lib.PROTOTYPES


def test_setter_returns_the_previous_level_and_round_trips():
    h = lib.get()
    try:
        h.mt_gemm_set_precision(0)
        assert h.mt_gemm_set_precision(1) == 0 and h.mt_gemm_get_precision() == 1
        assert h.mt_gemm_set_precision(1) == 1
        assert h.mt_gemm_set_precision(0) == 1 and h.mt_gemm_get_precision() == 0
        assert lib.set_matmul_precision("high") == "highest" and lib.get_matmul_precision() == "high"
        assert lib.set_matmul_precision("highest") == "high" and lib.get_matmul_precision() == "highest"
        assert mintime_amd.set_matmul_precision is lib.set_matmul_precision
        assert mintime_amd.get_matmul_precision is lib.get_matmul_precision
    finally:
        lib.set_matmul_precision("highest")


@pytest.mark.parametrize("level", [2, -1, 7])
def test_unknown_level_is_refused_and_changes_nothing(level):
    h = lib.get()
    try:
        for cur in (0, 1):
            h.mt_gemm_set_precision(cur)
            rc = h.mt_gemm_set_precision(level)
            assert rc < 0, rc
            assert b"mt_gemm_set_precision" in h.mt_last_error()
            assert h.mt_gemm_get_precision() == cur
        for name in ("medium", "HIGH", ""):                   # no one-product tier, no aliases
            with pytest.raises(lib.MintimeHipError):
                lib.set_matmul_precision(name)
            with pytest.raises(lib.MintimeHipError):
                mintime_amd.matmul_precision(name)
        assert h.mt_gemm_get_precision() == 1
    finally:
        lib.set_matmul_precision("highest")


def test_context_manager_restores_the_previous_tier_also_on_an_exception():
    try:
        lib.set_matmul_precision("highest")
        with mintime_amd.matmul_precision("high"):
            assert lib.get_matmul_precision() == "high"
            with mintime_amd.matmul_precision("highest"):
                assert lib.get_matmul_precision() == "highest"
            assert lib.get_matmul_precision() == "high"
        assert lib.get_matmul_precision() == "highest"
        with pytest.raises(ZeroDivisionError):
            with mintime_amd.matmul_precision("high"):
                assert lib.get_matmul_precision() == "high"
                1 / 0
        assert lib.get_matmul_precision() == "highest"
        lib.set_matmul_precision("high")
        with pytest.raises(KeyError):
            with mintime_amd.matmul_precision("highest"):
                raise KeyError("x")
        assert lib.get_matmul_precision() == "high"
    finally:
        lib.set_matmul_precision("highest")


_CHILD = """
import sys
sys.path.insert(0, {root!r})
import mintime_amd
from mintime_amd import lib
h = lib.get()
level = h.mt_gemm_get_precision()
err = h.mt_last_error() or b""
print("RESULT", level, lib.get_matmul_precision(), err.decode())
"""


def _child(value):
    """The initial tier of a FRESH interpreter (the environment variable is read once per process)."""
    env = dict(os.environ)
    env.pop("MT_MATMUL_PRECISION", None)
    if value is not None:
        env["MT_MATMUL_PRECISION"] = value
    r = subprocess.run([sys.executable, "-c", _CHILD.format(root=ROOT)], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT")][-1]
    _, level, name, *msg = line.split(" ", 3)
    return int(level), name, (msg[0] if msg else "")


def test_environment_variable_sets_the_initial_tier():
    assert _child("high")[:2] == (1, "high")
    assert _child("highest")[:2] == (0, "highest")
    level, name, msg = _child(None)
    assert (level, name) == (0, "highest") and "MT_MATMUL_PRECISION" not in msg
    # anything else keeps highest and says so through mt_last_error() on the first get
    level, name, msg = _child("medium")
    assert (level, name) == (0, "highest")
    assert "MT_MATMUL_PRECISION=medium" in msg, msg


def test_no_recording_thunk_is_generated_for_the_precision_entry_points():
    """Neither function takes a stream: csrc/gen_plan.py must leave them alone (a launch plan records launches, and the tier is read
    when a recorded call is dispatched at replay)."""
    import importlib.util
    spec = importlib.util.spec_from_file_location("gen_plan", os.path.join(lib.CSRC, "gen_plan.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    hdr = open(os.path.join(ROOT, "include", "mintime_hip.h")).read()
    launching = [name for ret, name, ps in gp.prototypes(hdr) if ps and ps[-1] == ("void*", "stream")]
    assert "mt_gemm_planes" in launching
    assert "mt_gemm_set_precision" not in launching and "mt_gemm_get_precision" not in launching
    import ctypes
    handle = ctypes.CDLL(lib.LIB_PATH)
    assert not hasattr(handle, "mti_gemm_set_precision") and not hasattr(handle, "mti_gemm_get_precision")
