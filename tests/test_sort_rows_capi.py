"""CPU tests of the row-wise sort entry points (include/srs_c_api.h): the
header declares them, the library exports them, the argument validation runs
before any device access (the addresses below are never dereferenced), the
route hook needs no device, and device::sort_rows of the C++ header compiles."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srs_c_api.h")

FUNCTIONS = ["srs_sort_rows_soa_device", "srs_debug_set_sort_rows_route",
             "srs_debug_last_sort_rows"]

U32, U64 = 4, 6  # srs_key_kind
INVALID, UNSUPPORTED = -1, -2
KERNEL, LOCAL, LEVELS = 0, 1, 2


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = set(re.findall(r"\b(srs_[a-z_0-9]+)\s*\(", text))
    for f in FUNCTIONS:
        assert f in fns, f


def test_header_says_there_is_no_in_place_form():
    text = open(HEADER).read()
    at = text.index("Row-wise sort:")
    comment = text[at:text.index("*/", at)]
    assert "no in-place form" in " ".join(comment.replace("*", " ").split())


@pytest.fixture(scope="module")
def lib():
    import srs_amd
    return srs_amd.lib()


@pytest.fixture(autouse=True)
def _auto_route(lib):
    yield
    assert lib.srs_debug_set_sort_rows_route(-1) == 0


def test_library_exports_the_functions(lib):
    for f in FUNCTIONS:
        assert hasattr(lib, f), f


def test_python_wraps_the_functions():
    import srs_amd
    for f in ("sort_rows_device", "debug_set_sort_rows_route", "debug_last_sort_rows"):
        assert callable(getattr(srs_amd, f)), f
    assert (srs_amd.SORT_ROWS_KERNEL, srs_amd.SORT_ROWS_LOCAL, srs_amd.SORT_ROWS_LEVELS) == (0, 1, 2)


def _rows(lib, rows, n, stride, kind, keys, pays=(), sizes=(), keys_out=0x9000000,
          pays_out=None, idx=None, up=1):
    """srs_sort_rows_soa_device on made-up addresses"""
    np_ = len(pays)
    if pays_out is None:
        pays_out = [0xA000000 + 0x100000 * i for i in range(np_)]
    p = (ctypes.c_void_p * max(1, np_))(*pays)
    po = (ctypes.c_void_p * max(1, np_))(*pays_out)
    s = (ctypes.c_uint32 * max(1, np_))(*sizes)
    return lib.srs_sort_rows_soa_device(rows, n, stride, kind, up, keys, np_,
                                        p if np_ else None, s if np_ else None, keys_out,
                                        po if np_ else None, idx, None)


def test_bad_kind(lib):
    assert _rows(lib, 4, 100, 100, 42, 0x100000) == INVALID
    assert b"key_kind" in lib.srs_last_error()


def test_payload_size_3(lib):
    assert _rows(lib, 4, 100, 100, U64, 0x100000, [0x200000], [3]) == UNSUPPORTED
    assert b"1, 2, 4 or 8" in lib.srs_last_error()


@pytest.mark.parametrize("what", ["key", "payload", "output", "payload_output", "indices"])
def test_misaligned_pointer(lib, what):
    args = dict(keys=0x100000, pays=[0x200000], sizes=[8], keys_out=0x9000000,
                pays_out=[0xA000000], idx=0xB000000)
    if what == "key":
        args["keys"] += 4
    elif what == "payload":
        args["pays"] = [0x200002]
    elif what == "output":
        args["keys_out"] += 4
    elif what == "payload_output":
        args["pays_out"] = [0xA000001]
    else:
        args["idx"] += 4
    assert _rows(lib, 4, 100, 100, U64, **args) == INVALID
    assert b"aligned" in lib.srs_last_error()


def test_element_alignment_is_all_a_row_start_needs(lib):
    """u32 keys at a 4-byte address with an odd stride: valid, and refused only
    for the shape (forced rows kernel with row_len > 8192), so the call
    returns before any device access."""
    assert lib.srs_debug_set_sort_rows_route(KERNEL) == 0
    assert _rows(lib, 4, 9000, 9003, U32, 0x100004) == UNSUPPORTED
    assert b"rows kernel" in lib.srs_last_error()


def test_null_pointers(lib):
    assert _rows(lib, 4, 100, 100, U64, 0x100000, keys_out=None) == INVALID
    assert b"NULL" in lib.srs_last_error()
    assert _rows(lib, 4, 100, 100, U64, None) == INVALID
    assert b"NULL" in lib.srs_last_error()
    assert _rows(lib, 4, 100, 100, U64, 0x100000, [0x200000], [8], pays_out=[0]) == INVALID
    assert b"NULL" in lib.srs_last_error()
    assert _rows(lib, 4, 100, 100, U64, 0x100000, [0], [8]) == INVALID
    assert b"NULL" in lib.srs_last_error()


def test_64_payloads_with_indices(lib):
    pays = [0x200000 + 0x10000 * i for i in range(64)]
    assert _rows(lib, 4, 100, 100, U64, 0x100000, pays, [8] * 64, idx=0xF0000000) == UNSUPPORTED
    assert b"63" in lib.srs_last_error()


def test_stride_below_row_len(lib):
    assert _rows(lib, 4, 100, 99, U64, 0x100000) == INVALID
    assert b"row_stride" in lib.srs_last_error()


def test_rows_times_stride_overflow(lib):
    assert _rows(lib, 1 << 40, 100, 1 << 30, U64, 0x100000) == INVALID
    assert b"overflow" in lib.srs_last_error()
    assert _rows(lib, 3, 1 << 62, 1 << 62, U64, 0x100000) == INVALID
    assert b"overflow" in lib.srs_last_error()


def test_output_overlapping_the_input(lib):
    rows, n, stride = 10, 100, 128
    base = 0x100000
    span = ((rows - 1) * stride + n) * 8  # bytes of an input column
    out = rows * n * 8                    # bytes of an output column
    # keys_out at the key column's start, on its last record, and reaching into it from below
    assert _rows(lib, rows, n, stride, U64, base, keys_out=base) == INVALID
    assert b"sort rows outputs must not overlap" in lib.srs_last_error()
    assert _rows(lib, rows, n, stride, U64, base, keys_out=base + span - 8) == INVALID
    assert _rows(lib, rows, n, stride, U64, base, keys_out=base - (out - 8)) == INVALID
    # a payload output over the key column, the index output over a payload column
    assert _rows(lib, rows, n, stride, U64, base, [0x200000], [8], pays_out=[base + 64]) == INVALID
    assert _rows(lib, rows, n, stride, U64, base, [0x200000], [8],
                 idx=0x200000 + span - 8) == INVALID
    assert b"overlap" in lib.srs_last_error()
    # just clear of the column on either side: valid (refused for the shape only)
    assert lib.srs_debug_set_sort_rows_route(LEVELS) == 0
    assert _rows(lib, rows, n, stride, U64, base, keys_out=base + span) == UNSUPPORTED
    assert _rows(lib, rows, n, stride, U64, base, keys_out=base - out) == UNSUPPORTED
    assert b"levels" in lib.srs_last_error()


@pytest.mark.parametrize("rows,n", [(0, 100), (-1, 100), (4, 0), (4, -5)])
def test_noop_calls(lib, rows, n):
    assert _rows(lib, rows, n, max(n, 0), U64, 0x100000, [0x200000], [8]) == 0


def test_route_hook_needs_no_device(lib):
    for r in (0, 1, 2, -1):
        assert lib.srs_debug_set_sort_rows_route(r) == 0
    assert lib.srs_debug_set_sort_rows_route(3) == INVALID
    assert lib.srs_debug_set_sort_rows_route(-2) == INVALID
    assert lib.srs_debug_set_sort_rows_route(-1) == 0


def test_forced_route_that_cannot_take_the_shape(lib):
    assert lib.srs_debug_set_sort_rows_route(KERNEL) == 0
    assert _rows(lib, 4, 8193, 8193, U64, 0x100000) == UNSUPPORTED
    assert lib.srs_debug_set_sort_rows_route(LOCAL) == 0
    assert _rows(lib, 4, 8193, 8193, U64, 0x100000) == UNSUPPORTED
    assert _rows(lib, 4, 1, 1, U64, 0x100000) == UNSUPPORTED
    assert b"local lists" in lib.srs_last_error()
    assert lib.srs_debug_set_sort_rows_route(LEVELS) == 0
    assert _rows(lib, 4, 8192, 8192, U64, 0x100000) == UNSUPPORTED


def test_cpp_sort_rows_compiles():
    src = ('#include "simd_sort/radix_sort.hpp"\n'
           "using namespace simd_sort; namespace dv = simd_sort::radix_sort::device;\n"
           "int main(){ const unsigned long long k[8]={3,1,2,0,7,6,5,4}; unsigned long long ko[6];\n"
           " const float p[8]={0,1,2,3,4,5,6,7}; float po[6];\n"
           " const short q[8]={0,1,2,3,4,5,6,7}; short qo[6];\n"
           " dv::sort_rows(nullptr, 2, 3, 4, k, ko);\n"
           " dv::sort_rows<false>(nullptr, 2, 3, 4, k, ko, std::pair<const float*, float*>(p, po));\n"
           " dv::sort_rows<true>(nullptr, 2, 3, 4, k, ko, std::pair<const float*, float*>(p, po),\n"
           "                     std::pair<const short*, short*>(q, qo));\n"
           " return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-x", "c++", "-I", os.path.join(REPO, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
