"""CPU tests of the top-k entry points (include/srs_c_api.h): the header
declares them, the library exports them, their argument validation runs
before any device access (the addresses below are never dereferenced), and
both device::top_k forms of the C++ header compile."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srs_c_api.h")


def declared_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(srs_[a-z_0-9]+)\s*\(", text)))


TOPK_FUNCTIONS = ["srs_topk_soa_device", "srs_topk_aos_device", "srs_debug_set_topk_candidates",
                  "srs_debug_last_topk"]

U32, U64 = 4, 6  # srs_key_kind


def test_header_declares_the_topk_functions():
    fns = declared_functions()
    for f in TOPK_FUNCTIONS:
        assert f in fns, f


def test_library_exports_the_topk_functions():
    import srs_amd
    lib = srs_amd.lib()
    for f in TOPK_FUNCTIONS:
        assert hasattr(lib, f), f


@pytest.fixture(scope="module")
def lib():
    import srs_amd
    return srs_amd.lib()


def _soa(lib, num, k, kind, keys, pays=(), sizes=(), keys_out=0x900000, pays_out=None, idx=None,
         up=1):
    """srs_topk_soa_device on made-up addresses"""
    np_ = len(pays)
    if pays_out is None:
        pays_out = [0xA00000 + 0x10000 * i for i in range(np_)]
    p = (ctypes.c_void_p * max(1, np_))(*pays)
    po = (ctypes.c_void_p * max(1, np_))(*pays_out)
    s = (ctypes.c_uint32 * max(1, np_))(*sizes)
    return lib.srs_topk_soa_device(num, k, kind, up, keys, np_, p if np_ else None,
                                   s if np_ else None, keys_out, po if np_ else None, idx, None)


def test_bad_kind(lib):
    assert _soa(lib, 100, 10, 42, 0x100000) == -1
    assert b"key_kind" in lib.srs_last_error()
    assert lib.srs_topk_aos_device(100, 10, 42, 1, 0x100000, 16, 0x900000, None, None) == -1


def test_payload_size_3(lib):
    assert _soa(lib, 100, 10, U64, 0x100000, [0x200000], [3]) == -2
    assert b"1, 2, 4 or 8" in lib.srs_last_error()


def test_aos_elem_size(lib):
    assert lib.srs_topk_aos_device(100, 10, U32, 1, 0x100000, 12, 0x900000, None, None) == -2
    assert b"power of two" in lib.srs_last_error()


@pytest.mark.parametrize("what", ["key", "payload", "output", "payload_output", "indices"])
def test_misaligned_pointer(lib, what):
    args = dict(keys=0x100000, pays=[0x200000], sizes=[8], keys_out=0x900000,
                pays_out=[0xA00000], idx=0xB00000)
    if what == "key":
        args["keys"] += 4
    elif what == "payload":
        args["pays"] = [0x200002]
    elif what == "output":
        args["keys_out"] += 4
    elif what == "payload_output":
        args["pays_out"] = [0xA00001]
    else:
        args["idx"] += 4
    assert _soa(lib, 100, 10, U64, **args) == -1
    assert b"aligned" in lib.srs_last_error()


def test_misaligned_records(lib):
    assert lib.srs_topk_aos_device(100, 10, U32, 1, 0x100004, 16, 0x900000, None, None) == -1
    assert b"aligned" in lib.srs_last_error()
    assert lib.srs_topk_aos_device(100, 10, U32, 1, 0x100000, 16, 0x900004, None, None) == -1
    assert lib.srs_topk_aos_device(100, 10, U32, 1, 0x100000, 16, 0x900000, 0xB00004, None) == -1


def test_null_outputs(lib):
    assert _soa(lib, 100, 10, U64, 0x100000, keys_out=None) == -1
    assert b"NULL" in lib.srs_last_error()
    assert _soa(lib, 100, 10, U64, None) == -1
    assert _soa(lib, 100, 10, U64, 0x100000, [0x200000], [8], pays_out=[0]) == -1
    assert lib.srs_topk_aos_device(100, 10, U32, 1, 0x100000, 16, None, None, None) == -1


def test_output_overlapping_the_input(lib):
    n, k = 1000, 10
    # keys_out over the key column: at its start and at its last element
    assert _soa(lib, n, k, U64, 0x100000, keys_out=0x100000) == -1
    assert b"overlap" in lib.srs_last_error()
    assert _soa(lib, n, k, U64, 0x100000, keys_out=0x100000 + 8 * (n - 1)) == -1
    # a payload output over the key column, the index output over a payload column
    assert _soa(lib, n, k, U64, 0x100000, [0x200000], [8], pays_out=[0x100000 + 64]) == -1
    assert _soa(lib, n, k, U64, 0x100000, [0x200000], [8], idx=0x200000 + 8 * (n - 1)) == -1
    # keys_out whose k records reach into the input from below
    assert _soa(lib, n, k, U64, 0x100000, keys_out=0x100000 - 8 * (k - 1)) == -1
    assert lib.srs_topk_aos_device(n, k, U64, 1, 0x100000, 16, 0x100000 + 16 * (n - 1), None,
                                   None) == -1
    assert b"overlap" in lib.srs_last_error()


def test_64_payloads_with_indices(lib):
    pays = [0x200000 + 0x10000 * i for i in range(64)]
    assert _soa(lib, 100, 10, U64, 0x100000, pays, [8] * 64, idx=0xF000000) == -2
    assert b"63" in lib.srs_last_error()


@pytest.mark.parametrize("num,k", [(100, 0), (100, -3), (0, 10), (-2, 10)])
def test_noop_calls(lib, num, k):
    assert _soa(lib, num, k, U64, 0x100000, [0x200000], [8]) == 0
    assert lib.srs_topk_aos_device(num, k, U32, 1, 0x100000, 16, 0x900000, None, None) == 0


def test_candidates_hook_needs_no_device(lib):
    assert lib.srs_debug_set_topk_candidates(5) == 0
    assert lib.srs_debug_set_topk_candidates(0) == 0


def test_cpp_top_k_forms_compile():
    src = ('#include "simd_sort/radix_sort.hpp"\n'
           "using namespace simd_sort; namespace dv = simd_sort::radix_sort::device;\n"
           "int main(){ const unsigned long long k[4]={3,1,2,0}; unsigned long long ko[2];\n"
           " const float p[4]={0,1,2,3}; float po[2]; const short q[4]={0,1,2,3}; short qo[2];\n"
           " dv::top_k(nullptr, 2, 4, k, ko);\n"
           " dv::top_k<false>(nullptr, 2, 4, k, ko, std::pair<const float*, float*>(p, po));\n"
           " dv::top_k<true>(nullptr, 2, 4, k, ko, std::pair<const float*, float*>(p, po),\n"
           "                 std::pair<const short*, short*>(q, qo));\n"
           " const DataElement<unsigned, unsigned> e[4]{}; DataElement<unsigned, unsigned> eo[2];\n"
           " dv::top_k(nullptr, 2, 4, e, eo); dv::top_k<false>(nullptr, 2, 4, e, eo);\n"
           " return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-x", "c++", "-I", os.path.join(REPO, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
