"""CPU tests of the ragged top-k entry points (include/srs_c_api.h): the header
declares them, the library exports them, the argument validation runs before
any device access (the addresses below are never dereferenced), the route hook
needs no device, and device::top_k_ragged of the C++ header compiles."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srs_c_api.h")

FUNCTIONS = ["srs_topk_ragged_soa_device", "srs_debug_set_topk_ragged_route",
             "srs_debug_last_topk_ragged"]

U64 = 6  # srs_key_kind
INVALID, UNSUPPORTED = -1, -2
NUM, NSEG, K = 1000, 10, 7
KEYS, PAY, KEYS_OUT, PAY_OUT, IDX, OFFS, CNT = (0x100000, 0x200000, 0x9000000, 0xA000000,
                                                0xB000000, 0xC000000, 0xD000000)


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = set(re.findall(r"\b(srs_[a-z_0-9]+)\s*\(", text))
    for f in FUNCTIONS:
        assert f in fns, f


@pytest.fixture(scope="module")
def lib():
    import srs_amd
    return srs_amd.lib()


@pytest.fixture(autouse=True)
def _default_route(lib):
    yield
    assert lib.srs_debug_set_topk_ragged_route(-1) == 0


def test_library_exports_the_functions(lib):
    for f in FUNCTIONS:
        assert hasattr(lib, f), f


def test_python_wraps_the_functions():
    import srs_amd
    for f in ("topk_ragged_device", "debug_set_topk_ragged_route", "debug_last_topk_ragged"):
        assert callable(getattr(srs_amd, f)), f


def _topk(lib, num=NUM, nseg=NSEG, offs=OFFS, k=K, kind=U64, keys=KEYS, pays=(), sizes=(),
          keys_out=KEYS_OUT, pays_out=None, idx=None, cnt=None, up=1):
    """srs_topk_ragged_soa_device on made-up addresses"""
    np_ = len(pays)
    if pays_out is None:
        pays_out = [PAY_OUT + 0x100000 * i for i in range(np_)]
    p = (ctypes.c_void_p * max(1, np_))(*pays)
    po = (ctypes.c_void_p * max(1, np_))(*pays_out)
    s = (ctypes.c_uint32 * max(1, np_))(*sizes)
    return lib.srs_topk_ragged_soa_device(num, nseg, offs, k, kind, up, keys, np_,
                                          p if np_ else None, s if np_ else None, keys_out,
                                          po if np_ else None, idx, cnt, None)


def test_bad_kind(lib):
    assert _topk(lib, kind=42) == INVALID
    assert b"key_kind" in lib.srs_last_error()


def test_payload_size_3(lib):
    assert _topk(lib, pays=[PAY], sizes=[3]) == UNSUPPORTED
    assert b"1, 2, 4 or 8" in lib.srs_last_error()


@pytest.mark.parametrize("what", ["key", "payload", "output", "payload_output", "indices",
                                  "offsets", "counts"])
def test_misaligned_pointer(lib, what):
    args = dict(keys=KEYS, pays=[PAY], sizes=[8], keys_out=KEYS_OUT, pays_out=[PAY_OUT], idx=IDX,
                offs=OFFS, cnt=CNT)
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
    elif what == "offsets":
        args["offs"] += 4
    else:
        args["cnt"] += 4
    assert _topk(lib, **args) == INVALID
    err = lib.srs_last_error()
    assert b"aligned" in err
    for name in ("indices", "offsets", "counts"):
        if what == name:
            assert name.encode() in err, err


def test_null_pointers(lib):
    assert _topk(lib, keys_out=None) == INVALID
    assert b"keys_out is NULL" in lib.srs_last_error()
    assert _topk(lib, keys=None) == INVALID
    assert b"keys is NULL" in lib.srs_last_error()
    assert _topk(lib, pays=[PAY], sizes=[8], pays_out=[0]) == INVALID
    assert b"payload pointer is NULL" in lib.srs_last_error()
    assert _topk(lib, pays=[0], sizes=[8]) == INVALID
    assert b"payload pointer is NULL" in lib.srs_last_error()
    assert _topk(lib, offs=None) == INVALID
    assert b"offsets is NULL" in lib.srs_last_error()
    # indices_out and counts_out may be NULL: the call passes validation and
    # fails only for want of a device or of real memory, which is not asked here


def test_64_payloads_with_indices(lib):
    pays = [PAY + 0x10000 * i for i in range(64)]
    assert _topk(lib, pays=pays, sizes=[8] * 64, idx=0xF0000000) == UNSUPPORTED
    assert b"63" in lib.srs_last_error()


def test_overflows(lib):
    assert _topk(lib, nseg=(1 << 63) - 1) == INVALID
    assert b"num_segments + 1 overflows" in lib.srs_last_error()
    assert _topk(lib, nseg=1 << 40, k=1 << 40) == INVALID
    assert b"num_segments * k overflows" in lib.srs_last_error()
    # the product fits int64, its bytes in an 8-byte column do not
    assert _topk(lib, nseg=1 << 30, k=1 << 31) == INVALID
    assert b"num_segments * k overflows" in lib.srs_last_error()


def test_outputs_overlapping_inputs_or_offsets(lib):
    span = NUM * 8                # bytes of an input column
    out_span = NSEG * K * 8       # bytes of an output
    offs_bytes = (NSEG + 1) * 8   # bytes of the offsets array
    cnt_bytes = NSEG * 8
    # keys_out at the key column's start, on its last record, reaching into it from below
    assert _topk(lib, keys_out=KEYS) == INVALID
    assert b"top-k ragged outputs must not overlap the inputs" in lib.srs_last_error()
    assert _topk(lib, keys_out=KEYS + span - 8) == INVALID
    assert _topk(lib, keys_out=KEYS - (out_span - 8)) == INVALID
    # an output over a payload column, a payload output over the key column
    assert _topk(lib, pays=[PAY], sizes=[8], keys_out=PAY + 64) == INVALID
    assert _topk(lib, pays=[PAY], sizes=[8], pays_out=[KEYS + 64]) == INVALID
    assert b"overlap the inputs" in lib.srs_last_error()
    # the indices and the counts over a payload column
    assert _topk(lib, pays=[PAY], sizes=[8], idx=PAY + span - 8) == INVALID
    assert b"overlap the inputs" in lib.srs_last_error()
    assert _topk(lib, pays=[PAY], sizes=[8], cnt=PAY + span - 8) == INVALID
    assert b"counts_out must not overlap the inputs" in lib.srs_last_error()
    assert _topk(lib, cnt=KEYS - (cnt_bytes - 8)) == INVALID
    assert b"counts_out must not overlap the inputs" in lib.srs_last_error()
    # an output, a payload output, the indices and the counts over the offsets array
    assert _topk(lib, keys_out=OFFS) == INVALID
    assert b"outputs must not overlap the offsets" in lib.srs_last_error()
    assert _topk(lib, keys_out=OFFS + offs_bytes - 8) == INVALID
    assert _topk(lib, keys_out=OFFS - (out_span - 8)) == INVALID
    assert _topk(lib, pays=[PAY], sizes=[8], pays_out=[OFFS + 8]) == INVALID
    assert _topk(lib, idx=OFFS) == INVALID
    assert b"outputs must not overlap the offsets" in lib.srs_last_error()
    assert _topk(lib, cnt=OFFS + offs_bytes - 8) == INVALID
    assert b"counts_out must not overlap the offsets" in lib.srs_last_error()
    assert _topk(lib, cnt=OFFS - (cnt_bytes - 8)) == INVALID
    assert b"counts_out must not overlap the offsets" in lib.srs_last_error()


@pytest.mark.parametrize("num,nseg,k", [(0, 10, 7), (-1, 10, 7), (1000, 0, 7), (1000, -5, 7),
                                        (1000, 10, 0), (1000, 10, -3)])
def test_noop_calls(lib, num, nseg, k):
    assert _topk(lib, num=num, nseg=nseg, k=k, pays=[PAY], sizes=[8], idx=IDX, cnt=CNT) == 0
    # (a no-op looks at neither the offsets nor the outputs)
    assert _topk(lib, num=num, nseg=nseg, k=k, keys_out=None, offs=None, cnt=4) == 0


def test_route_hook_needs_no_device(lib):
    for v in (-1, 0, 1):
        assert lib.srs_debug_set_topk_ragged_route(v) == 0
    for v in (2, -2):
        assert lib.srs_debug_set_topk_ragged_route(v) == INVALID
        assert b"route" in lib.srs_last_error()
    assert lib.srs_debug_set_topk_ragged_route(-1) == 0


def test_last_info_rejects_null(lib):
    assert lib.srs_debug_last_topk_ragged(None) == INVALID
    assert b"info is NULL" in lib.srs_last_error()


def test_cpp_top_k_ragged_compiles():
    src = ('#include "simd_sort/radix_sort.hpp"\n'
           "using namespace simd_sort; namespace dv = simd_sort::radix_sort::device;\n"
           "int main(){ const unsigned long long k[8]={3,1,2,0,7,6,5,4};\n"
           " unsigned long long ko[4];\n"
           " const float p[8]={0,1,2,3,4,5,6,7}; float po[4];\n"
           " const short q[8]={0,1,2,3,4,5,6,7}; short qo[4];\n"
           " const int64_t* offs = nullptr; int64_t* idx = nullptr; int64_t* cnt = nullptr;\n"
           " dv::top_k_ragged(nullptr, 2, 8, 2, offs, k, ko, idx, cnt);\n"
           " dv::top_k_ragged<false>(nullptr, 2, 8, 2, offs, k, ko, idx, cnt,\n"
           "                         std::pair<const float*, float*>(p, po));\n"
           " dv::top_k_ragged<true>(nullptr, 2, 8, 2, offs, k, ko, idx, cnt,\n"
           "                        std::pair<const float*, float*>(p, po),\n"
           "                        std::pair<const short*, short*>(q, qo));\n"
           " return 0; }\n")
    r = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                        "-x", "c++", "-I", os.path.join(REPO, "include"), "-"],
                       input=src.encode(), capture_output=True)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
