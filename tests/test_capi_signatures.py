"""CPU-only tests of the binding's own plumbing, with no library loaded: the signature table of cafexp_amd/capi.py against
every prototype of include/cafe_mi355x.h (kind and width of the result and of each argument), the out-struct filler and the
rate frame of the per-family and gain calls."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

from cafexp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPAQUE = {"cafe_ctx", "cafe_sharded"}                       # handles: the binding never looks inside
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint64_t": C.c_uint64, "size_t": C.c_size_t,
           "unsigned long long": C.c_ulonglong, "double": C.c_double, "float": C.c_float}


def _prototypes():
    """[(name, result, [parameter, ...])] of every `ret cafe_name(args);` of the header, comments and directives stripped"""
    text = open(os.path.join(ROOT, "include", "cafe_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    text = re.sub(r"//[^\n]*", "", text)
    text = re.sub(r"(?m)^\s*#.*$", "", text)
    found = re.findall(r"([\w\s\*]+?)\b(cafe_\w+)\s*\(([^()]*)\)\s*;", text)
    return [(name, " ".join(ret.split()), [] if args.strip() == "void" else [" ".join(a.split()) for a in args.split(",")])
            for ret, name, args in found]


PROTOTYPES = _prototypes()


def _c_type(text: str, named: bool):
    """(base type, pointer?, parameter name) of a C result or parameter; `x[k]` is a pointer"""
    text = text.replace("const ", "").strip()
    pointer = "*" in text or text.endswith("]")
    words = re.sub(r"\[.*\]$", "", text).replace("*", " ").split()
    name = words.pop() if named else ""
    return " ".join(words), pointer, name


def _same_scalar(ctype, base: str) -> bool:
    want = SCALARS[base]
    if want in (C.c_double, C.c_float):
        return ctype is want
    code = getattr(ctype, "_type_", "")
    return (isinstance(code, str) and code in "bBhHiIlLqQ" and C.sizeof(ctype) == C.sizeof(want)
            and (ctype(-1).value < 0) == (want(-1).value < 0))


def _agrees(ctype, base: str, pointer: bool, name: str = "") -> bool:
    if not pointer:
        return ctype is None if base == "void" else _same_scalar(ctype, base)
    if base == "void" or base in OPAQUE or name.startswith("device_"):        # device_*: an address in device memory, not a host array
        return ctype is C.c_void_p
    if base == "char":
        return ctype is C.c_char_p
    if base.startswith("cafe_"):
        struct = getattr(capi, "".join(w.capitalize() for w in base.split("_")))
        return ctype is C.POINTER(struct)
    return isinstance(ctype, type) and issubclass(ctype, C._Pointer) and _same_scalar(ctype._type_, base)


def test_the_header_declares_the_table_in_its_order():
    assert len(PROTOTYPES) == 92
    assert [name for name, _, _ in PROTOTYPES] == list(capi._SIGNATURES)
    assert capi.EXPORTS == list(capi._SIGNATURES) and len(set(capi.EXPORTS)) == 92


@pytest.mark.parametrize("name,ret,params", PROTOTYPES, ids=[p[0] for p in PROTOTYPES])
def test_table_row_agrees_with_the_prototype(name, ret, params):
    restype, argtypes = capi._SIGNATURES[name]
    assert _agrees(restype, *_c_type(ret, named=False)), (ret, restype)
    assert len(argtypes) == len(params), (params, argtypes)
    for ctype, param in zip(argtypes, params):
        assert _agrees(ctype, *_c_type(param, named=True)), (param, ctype)


def test_the_checker_tells_widths_signs_and_structs_apart():
    assert _agrees(C.c_int64, "int64_t", False) and not _agrees(C.c_int32, "int64_t", False)
    assert not _agrees(C.c_uint64, "int64_t", False) and not _agrees(C.c_int64, "size_t", False)
    assert not _agrees(C.c_int, "double", False) and not _agrees(C.c_double, "int", False)
    assert _agrees(capi._i64p, "int64_t", True) and not _agrees(capi._i32p, "int64_t", True)
    assert not _agrees(capi._f64p, "int64_t", True) and not _agrees(C.c_void_p, "double", True, "out")
    assert not _agrees(C.c_int64, "int64_t", True) and not _agrees(capi._i64p, "int64_t", False)
    assert _agrees(C.POINTER(capi.CafeParams), "cafe_params", True)
    assert not _agrees(C.POINTER(capi.CafeBatchParams), "cafe_params", True) and not _agrees(C.c_void_p, "cafe_params", True)
    assert _agrees(C.c_void_p, "cafe_ctx", True) and not _agrees(C.POINTER(capi.CafeParams), "cafe_ctx", True)
    assert _c_type("const double host_partial[2]", True) == ("double", True, "host_partial")
    assert _c_type("unsigned long long* out", True) == ("unsigned long long", True, "out")


def test_filler_refuses_a_key_that_is_no_field():
    with pytest.raises((KeyError, capi.CafeError), match="p_gian"):
        capi._out(capi.CafeGainPosteriorOut, {"lnl": np.empty(2), "p_gian": np.empty((2, 5))})


def test_filler_refuses_an_array_of_another_dtype():
    with pytest.raises(capi.CafeError, match="mode"):
        capi._out(capi.CafeMarginalOut, {"mean": np.empty((2, 5)), "mode": np.empty((2, 5))})          # float64 for an int32_t*
    with pytest.raises(capi.CafeError, match="n_increase"):
        capi._out(capi.CafeHistoryOut, {"n_increase": np.empty((2, 5), dtype=np.int32)})               # int32 for an int64_t*


def test_filler_points_exactly_the_named_fields_at_their_arrays():
    res = {name: np.empty((3, 5)) for name in ("p_absent", "mean", "p_gain", "p_loss")}
    res["lnl"] = np.empty(3)
    out = capi._out(capi.CafeGainPosteriorOut, res)
    for name, _ in capi.CafeGainPosteriorOut._fields_:
        pointer = getattr(out, name)
        if name == "posterior":
            assert not pointer
        else:
            assert C.cast(pointer, C.c_void_p).value == res[name].ctypes.data
    mixed = {"category": np.empty((2, 3), dtype=np.int32), "net_change": np.empty((2, 5), dtype=np.int64), "log_evidence": np.empty(3)}
    out = capi._out(capi.CafeHistoryOut, mixed)
    assert {name for name, _ in capi.CafeHistoryOut._fields_ if getattr(out, name)} == set(mixed)
    assert C.cast(out.net_change, C.c_void_p).value == mixed["net_change"].ctypes.data


def _frame(n_lambdas, *args, **kwargs):
    stand_in = types.SimpleNamespace(problem=types.SimpleNamespace(n_lambdas=n_lambdas))
    return capi.Context._rate_frame(stand_in, *args, **kwargs)


def test_rate_frame_per_family_and_shared():
    rows = [[0.1, 0.2], [0.3, 0.4], [0.5, 0.6]]
    for mus in (None, np.array(rows) * 2):
        fam, lam, mu, nu = _frame(2, [4, 0, -1], rows, mus, np.array(rows)[:, ::-1])
        assert fam.dtype == np.int64 and fam.tolist() == [4, 0, -1]
        assert lam.shape == nu.shape == (3, 2) and lam.tolist() == rows and nu.tolist() == [r[::-1] for r in rows]
        assert all(a.dtype == np.float64 and a.flags["C_CONTIGUOUS"] for a in (lam, nu))             # (nus came in as a reversed view)
        assert mu is None if mus is None else (mu.tolist() == mus.tolist() and mu.flags["C_CONTIGUOUS"])
        fam, lam, mu, nu = _frame(2, [[4, 0], [7, 1]], rows[0], None if mus is None else mus[0], rows[1], shared=True)
        assert fam.tolist() == [4, 0, 7, 1] and lam.tolist() == rows[0] and nu.tolist() == rows[1]
        assert mu is None if mus is None else mu.tolist() == mus[0].tolist()
    fam, lam, mu, nu = _frame(2, [1, 2], np.arange(4.0), rates=1)                                     # flat input, one row per family
    assert lam.tolist() == [[0.0, 1.0], [2.0, 3.0]] and mu is None and nu is None
    fam, lam, mu, nu = _frame(2, [1, 2], rows[:2], rows[1:], rates=2)
    assert mu.tolist() == rows[1:] and nu is None


def test_rate_frame_takes_one_rate_per_family_as_a_vector():
    fam, lam, mu, nu = _frame(1, [5, 6, 7], [0.1, 0.2, 0.3], None, [1.0, 2.0, 3.0])
    assert lam.shape == nu.shape == (3, 1) and mu is None and nu[:, 0].tolist() == [1.0, 2.0, 3.0]
    fam, lam, mu, nu = _frame(1, [5, 6, 7], [0.1, 0.2, 0.3], [0.3, 0.2, 0.1], rates=2)
    assert lam.shape == mu.shape == (3, 1)


def test_rate_frame_keeps_every_error_text():
    one = [[0.1], [0.2]]
    two = [[0.1, 0.2], [0.3, 0.4]]
    with pytest.raises(ValueError, match=r"^lambdas must be \[2\]\[2\]$"):
        _frame(2, [0, 1], one, rates=1)
    with pytest.raises(ValueError, match=r"^lambdas and mus must be \[2\]\[2\]$"):
        _frame(2, [0, 1], two, one, rates=2)
    with pytest.raises(ValueError, match=r"^lambdas and mus must be \[2\]\[2\]$"):
        _frame(2, [0, 1], one, one, rates=2)
    for lam, mus, nus in ((one, None, one), (two, None, one), (two, one, two), (one, two, two)):
        with pytest.raises(ValueError, match=r"^lambdas, mus and nus must be \[2\]\[2\]$"):
            _frame(2, [0, 1], lam, mus, nus)
    for lam, mus, nus in (([0.1], None, [0.1]), ([0.1, 0.2], None, [0.1]), ([0.1, 0.2], [0.1, 0.2, 0.3], [0.1, 0.2]), ([[0.1, 0.2]] * 2, None, [0.1, 0.2])):
        with pytest.raises(ValueError, match=r"^lambdas, mus and nus must be \[2\]$"):
            _frame(2, [0, 1, 2], lam, mus, nus, shared=True)
