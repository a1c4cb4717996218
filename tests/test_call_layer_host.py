"""The checked call layer of lib.py (`lib.mt.<entry point>`) and the two binding tables behind it, on a machine without a device:
the tables against include/mintime_hip.h type by type, argument counts, pointer slots, return codes.  Every call passes None as the
stream and fails before any kernel is launched."""
import ctypes as C
import importlib.util
import os
import re

import pytest
import torch

from mintime_amd import lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCALARS = {"int": C.c_int, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double, "unsigned": C.c_uint, "mt_rowmap": lib.RowMap}


def _gen_plan():
    spec = importlib.util.spec_from_file_location("gen_plan", os.path.join(lib.CSRC, "gen_plan.py"))
    gp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gp)
    return gp


def _header():
    return open(os.path.join(ROOT, "include", "mintime_hip.h")).read()


def _is_pointer(a):
    return a is C.c_void_p or hasattr(a, "contents")          # void* or POINTER(T), never the fp32 marker


def _mismatches(launches, queries, restypes):
    """Every disagreement between the two tables and the header, as strings."""
    bad = []
    both = {**queries, **launches}
    protos = _gen_plan().prototypes(_header())
    assert len(protos) >= 100
    for ret, name, ps in protos:
        table = both.get(name)
        if table is None or len(table) != len(ps):
            bad.append(f"{name}: {len(ps)} parameters in the header")
            continue
        if restypes.get(name, C.c_int) is not SCALARS[ret]:
            bad.append(f"{name}: returns {ret}")
        for i, ((ctype, pname), a) in enumerate(zip(ps, table)):
            ctype = ctype.replace(" ", "")
            if ctype in ("float*", "constfloat*"):
                ok = a is lib.f32p
            elif ctype.endswith("*"):
                ok = _is_pointer(a)
            else:
                ok = a is SCALARS[ctype]
            if not ok:
                bad.append(f"{name}: argument {i} ({pname}) is {ctype} in the header, {a.__name__} in the table")
    # the declarations gen_plan.prototypes leaves out: no parameters, or a string result
    for ret, name in re.findall(r"^(int|int64_t|const char\*)\s+(mt_\w+)\s*\(\s*(?:void)?\s*\)\s*;", _header(), flags=re.M):
        want = C.c_char_p if ret == "const char*" else SCALARS[ret]
        if both.get(name) != [] or restypes.get(name, C.c_int) is not want:
            bad.append(f"{name}: no parameters, returns {ret}")
    return bad


def test_tables_agree_with_the_header_type_by_type():
    assert not set(lib.LAUNCHES) & set(lib.QUERIES)
    assert lib.PROTOTYPES == {**lib.QUERIES, **lib.LAUNCHES}
    assert _mismatches(lib.LAUNCHES, lib.QUERIES, lib._RESTYPES) == []
    # the comparison sees one int of the wrong width, and a float* slot declared as a plain pointer
    wrong = dict(lib.LAUNCHES)
    i = wrong["mt_sf_bn_relu_fwd"].index(C.c_int)
    wrong["mt_sf_bn_relu_fwd"] = [C.c_int64 if j == i else a for j, a in enumerate(wrong["mt_sf_bn_relu_fwd"])]
    bad = _mismatches(wrong, lib.QUERIES, lib._RESTYPES)
    assert len(bad) == 1 and bad[0].startswith(f"mt_sf_bn_relu_fwd: argument {i} ")
    wrong = dict(lib.LAUNCHES, mt_mul_add=[C.c_void_p] + lib.LAUNCHES["mt_mul_add"][1:])
    assert len(_mismatches(wrong, lib.QUERIES, lib._RESTYPES)) == 1
    assert len(_mismatches(lib.LAUNCHES, lib.QUERIES, dict(lib._RESTYPES, mt_planes_elems=C.c_int))) == 1


def test_launching_table_is_what_gen_plan_wraps():
    gp = _gen_plan()
    wrapped = {name for ret, name, ps in gp.prototypes(_header())
               if ps[-1] == ("void*", "stream") and ret == "int" and name not in gp.SKIP}
    assert wrapped == set(lib.LAUNCHES) and len(wrapped) >= 50
    lib.get()
    assert {"mt_" + k for k in vars(lib.mt)} == wrapped


def test_wrong_argument_count_raises_before_the_library_is_entered():
    for args in ((None, 0, 16, None, None), (None, 0)):            # one too many (with the stream); one too few (without it)
        with pytest.raises(lib.MintimeHipError, match=r"mt_memset_async takes 3 arguments .* got %d" % len(args)):
            lib.mt.memset_async(*args)


def test_pointer_slot_refuses_cpu_tensors_and_wrong_dtypes():
    with pytest.raises(lib.MintimeHipError, match=r"mt_memset_async: argument 0 is a CPU tensor"):
        lib.mt.memset_async(torch.zeros(16, dtype=torch.uint8), 0, 16, None)
    # a float* slot: the dtype is looked at first, so both refusals show on a machine without a device
    with pytest.raises(lib.MintimeHipError, match=r"mt_mul_add: argument 1 is a float\* slot .* got torch.int32"):
        lib.mt.mul_add(None, torch.zeros(4, dtype=torch.int32), None, None, 4, None)
    with pytest.raises(lib.MintimeHipError, match=r"mt_mul_add: argument 1 is a CPU tensor"):
        lib.mt.mul_add(None, torch.zeros(4), None, None, 4, None)
    with pytest.raises(lib.MintimeHipError, match=r"float\* slot"):
        lib._slot("mt_x", 3, torch.zeros(4, dtype=torch.int32), True, None)
    with pytest.raises(lib.MintimeHipError, match=r"mt_x: argument 3 is a CPU tensor"):
        lib._slot("mt_x", 3, torch.zeros(4, dtype=torch.int32), False, None)


def test_nonzero_return_code_raises_with_the_librarys_message():
    with pytest.raises(lib.MintimeHipError, match=r"mt_memset_async failed \(-?\d+\): .*null pointer"):
        lib.mt.memset_async(None, 0, 16, None)
    with pytest.raises(AttributeError):
        lib.mt.se_pool_parts                                       # a query: its int is a value, not an error code
