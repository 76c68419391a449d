"""CPU tests of the ragged sort entry points (include/srs_c_api.h): the header
declares them, the library exports them, the argument validation runs before
any device access (the addresses below are never dereferenced), the short-max
hook needs no device, and device::sort_ragged of the C++ header compiles."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srs_c_api.h")

FUNCTIONS = ["srs_sort_ragged_soa_device", "srs_debug_set_sort_ragged_short_max",
             "srs_debug_last_sort_ragged"]

U64 = 6  # srs_key_kind
INVALID, UNSUPPORTED = -1, -2
NUM, NSEG = 1000, 10
KEYS, PAY, KEYS_OUT, PAY_OUT, IDX, OFFS = (0x100000, 0x200000, 0x9000000, 0xA000000, 0xB000000,
                                           0xC000000)


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = set(re.findall(r"\b(srs_[a-z_0-9]+)\s*\(", text))
    for f in FUNCTIONS:
        assert f in fns, f


def test_header_says_there_is_no_in_place_form():
    text = open(HEADER).read()
    at = text.index("Ragged sort:")
    comment = text[at:text.index("*/", at)]
    assert "no in-place form" in " ".join(comment.replace("*", " ").split())


@pytest.fixture(scope="module")
def lib():
    import srs_amd
    return srs_amd.lib()


@pytest.fixture(autouse=True)
def _default_short_max(lib):
    yield
    assert lib.srs_debug_set_sort_ragged_short_max(-1) == 0


def test_library_exports_the_functions(lib):
    for f in FUNCTIONS:
        assert hasattr(lib, f), f


def test_python_wraps_the_functions():
    import srs_amd
    for f in ("sort_ragged_device", "debug_set_sort_ragged_short_max", "debug_last_sort_ragged"):
        assert callable(getattr(srs_amd, f)), f


def _ragged(lib, num=NUM, nseg=NSEG, offs=OFFS, kind=U64, keys=KEYS, pays=(), sizes=(),
            keys_out=KEYS_OUT, pays_out=None, idx=None, up=1):
    """srs_sort_ragged_soa_device on made-up addresses"""
    np_ = len(pays)
    if pays_out is None:
        pays_out = [PAY_OUT + 0x100000 * i for i in range(np_)]
    p = (ctypes.c_void_p * max(1, np_))(*pays)
    po = (ctypes.c_void_p * max(1, np_))(*pays_out)
    s = (ctypes.c_uint32 * max(1, np_))(*sizes)
    return lib.srs_sort_ragged_soa_device(num, nseg, offs, kind, up, keys, np_,
                                          p if np_ else None, s if np_ else None, keys_out,
                                          po if np_ else None, idx, None)


def test_bad_kind(lib):
    assert _ragged(lib, kind=42) == INVALID
    assert b"key_kind" in lib.srs_last_error()


def test_payload_size_3(lib):
    assert _ragged(lib, pays=[PAY], sizes=[3]) == UNSUPPORTED
    assert b"1, 2, 4 or 8" in lib.srs_last_error()


@pytest.mark.parametrize("what", ["key", "payload", "output", "payload_output", "indices",
                                  "offsets"])
def test_misaligned_pointer(lib, what):
    args = dict(keys=KEYS, pays=[PAY], sizes=[8], keys_out=KEYS_OUT, pays_out=[PAY_OUT], idx=IDX,
                offs=OFFS)
    if what == "key":
        args["keys"] += 4
    elif what == "payload":
        args["pays"] = [PAY + 2]
    elif what == "output":
        args["keys_out"] += 4
    elif what == "payload_output":
        args["pays_out"] = [PAY_OUT + 1]
    elif what == "indices":
        args["idx"] += 4
    else:
        args["offs"] += 4
    assert _ragged(lib, **args) == INVALID
    assert b"aligned" in lib.srs_last_error()


def test_null_pointers(lib):
    assert _ragged(lib, keys_out=None) == INVALID
    assert b"NULL" in lib.srs_last_error()
    assert _ragged(lib, keys=None) == INVALID
    assert b"NULL" in lib.srs_last_error()
    assert _ragged(lib, pays=[PAY], sizes=[8], pays_out=[0]) == INVALID
    assert b"NULL" in lib.srs_last_error()
    assert _ragged(lib, pays=[0], sizes=[8]) == INVALID
    assert b"NULL" in lib.srs_last_error()
    assert _ragged(lib, offs=None) == INVALID
    assert b"offsets is NULL" in lib.srs_last_error()


def test_64_payloads_with_indices(lib):
    pays = [PAY + 0x10000 * i for i in range(64)]
    assert _ragged(lib, pays=pays, sizes=[8] * 64, idx=0xF0000000) == UNSUPPORTED
    assert b"63" in lib.srs_last_error()


def test_num_segments_plus_one_overflows(lib):
    assert _ragged(lib, nseg=(1 << 63) - 1) == INVALID
    assert b"overflow" in lib.srs_last_error()


def test_outputs_overlapping_inputs_or_offsets(lib):
    span = NUM * 8                # bytes of a column
    offs_bytes = (NSEG + 1) * 8   # bytes of the offsets array
    # keys_out at the key column's start, on its last record, reaching into it from below
    assert _ragged(lib, keys_out=KEYS) == INVALID
    assert b"sort ragged outputs must not overlap" in lib.srs_last_error()
    assert _ragged(lib, keys_out=KEYS + span - 8) == INVALID
    assert _ragged(lib, keys_out=KEYS - (span - 8)) == INVALID
    # an output over a payload column, a payload output over the key column
    assert _ragged(lib, pays=[PAY], sizes=[8], keys_out=PAY + 64) == INVALID
    assert _ragged(lib, pays=[PAY], sizes=[8], pays_out=[KEYS + 64]) == INVALID
    assert b"overlap" in lib.srs_last_error()
    # the indices over a payload column
    assert _ragged(lib, pays=[PAY], sizes=[8], idx=PAY + span - 8) == INVALID
    assert b"overlap" in lib.srs_last_error()
    # an output, a payload output and the indices over the offsets array
    assert _ragged(lib, keys_out=OFFS) == INVALID
    assert b"offsets" in lib.srs_last_error()
    assert _ragged(lib, keys_out=OFFS + offs_bytes - 8) == INVALID
    assert _ragged(lib, keys_out=OFFS - (span - 8)) == INVALID
    assert _ragged(lib, pays=[PAY], sizes=[8], pays_out=[OFFS + 8]) == INVALID
    assert _ragged(lib, idx=OFFS) == INVALID
    assert b"offsets" in lib.srs_last_error()


@pytest.mark.parametrize("num,nseg", [(0, 10), (-1, 10), (1000, 0), (1000, -5)])
def test_noop_calls(lib, num, nseg):
    assert _ragged(lib, num=num, nseg=nseg, pays=[PAY], sizes=[8]) == 0


def test_short_max_hook_needs_no_device(lib):
    for v in (-1, 0, 1, 256):
        assert lib.srs_debug_set_sort_ragged_short_max(v) == 0
    assert lib.srs_debug_set_sort_ragged_short_max(-2) == INVALID
    assert b"short_max" in lib.srs_last_error()
    assert lib.srs_debug_set_sort_ragged_short_max(257) == INVALID
    assert lib.srs_debug_set_sort_ragged_short_max(-1) == 0


def test_cpp_sort_ragged_compiles():
    src = ('#include "simd_sort/radix_sort.hpp"\n'
           "using namespace simd_sort; namespace dv = simd_sort::radix_sort::device;\n"
           "int main(){ const unsigned long long k[8]={3,1,2,0,7,6,5,4};\n"
           " unsigned long long ko[8];\n"
           " const float p[8]={0,1,2,3,4,5,6,7}; float po[8];\n"
           " const short q[8]={0,1,2,3,4,5,6,7}; short qo[8];\n"
           " const int64_t* offs = nullptr; int64_t* idx = nullptr;\n"
           " dv::sort_ragged(nullptr, 8, 2, offs, k, ko);\n"
           " dv::sort_ragged<false>(nullptr, 8, 2, offs, k, ko,\n"
           "                        std::pair<const float*, float*>(p, po));\n"
           " dv::sort_ragged<true>(nullptr, 8, 2, offs, k, ko,\n"
           "                       std::pair<const float*, float*>(p, po),\n"
           "                       std::pair<const short*, short*>(q, qo));\n"
           " dv::sort_ragged(nullptr, 8, 2, offs, k, ko, idx);\n"
           " dv::sort_ragged<false>(nullptr, 8, 2, offs, k, ko, idx,\n"
           "                        std::pair<const float*, float*>(p, po),\n"
           "                        std::pair<const short*, short*>(q, qo));\n"
           " return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-x", "c++", "-I", os.path.join(REPO, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
