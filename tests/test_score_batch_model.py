"""cafe_score_batch on the CPU: the header declares the entry and its struct, the library exports it, the ABI version is
unchanged, the binding lists it and lays the struct out as the header does."""
import ctypes as C
import os
import re

from cafexp_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "cafe_mi355x.h")


def test_the_header_declares_the_entry_and_its_struct():
    text = open(HEADER).read()
    assert re.search(r"int\s+cafe_score_batch\(cafe_ctx\*\s*ctx,\s*const cafe_batch_params\*\s*params,\s*double\*\s*neg_lnl", text)
    body = re.search(r"typedef struct cafe_batch_params \{(.*?)\} cafe_batch_params;", text, re.S).group(1)
    fields = re.findall(r"(\w+);", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert fields == [name for name, _ in capi.CafeBatchParams._fields_]
    assert re.search(r"#define CAFE_ABI_VERSION 3\b", text)


def test_the_struct_is_laid_out_as_the_header_says():
    # three int32, a hole, seven pointers
    assert C.sizeof(capi.CafeBatchParams) == 16 + 7 * C.sizeof(C.c_void_p)
    assert capi.CafeBatchParams.lambdas.offset == 16 and capi.CafeBatchParams.error_model.offset == 16 + 6 * C.sizeof(C.c_void_p)


def test_the_library_exports_it_and_the_abi_version_is_unchanged():
    lib = capi.load()
    assert "cafe_score_batch" in capi.EXPORTS
    assert lib.cafe_score_batch is not None
    assert lib.cafe_abi_version() == 3
    assert hasattr(capi.Context, "score_batch")
