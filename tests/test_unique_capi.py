"""CPU tests of the unique entry points (include/srs_c_api.h): the header
declares them, the library exports them, the argument validation runs before
any device access (the addresses below are never dereferenced), and
device::unique of the C++ header compiles."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srs_c_api.h")

FUNCTIONS = ["srs_unique_soa_device", "srs_debug_last_unique"]

U64 = 6  # srs_key_kind
INVALID, UNSUPPORTED = -1, -2
NUM = 1000
KEYS, PAY, SORTED, PAY_SORTED, IDX, UNIQ, OFFS, INV, NU = (
    0x100000, 0x200000, 0x9000000, 0xA000000, 0xB000000, 0xC000000, 0xD000000, 0xE000000,
    0xF000000)


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = set(re.findall(r"\b(srs_[a-z_0-9]+)\s*\(", text))
    for f in FUNCTIONS:
        assert f in fns, f


@pytest.fixture(scope="module")
def lib():
    import srs_amd
    return srs_amd.lib()


def test_library_exports_the_functions(lib):
    for f in FUNCTIONS:
        assert hasattr(lib, f), f


def test_python_wraps_the_functions():
    import srs_amd
    for f in ("unique_device", "debug_last_unique"):
        assert callable(getattr(srs_amd, f)), f
    assert srs_amd.UniqueResult._fields == ("unique", "sorted", "offsets", "counts", "index",
                                            "inverse")


def _unique(lib, num=NUM, kind=U64, keys=KEYS, pays=(), sizes=(), srt=SORTED, pays_sorted=None,
            idx=None, uniq=UNIQ, offs=None, inv=None, nu=None, nu_host=None, up=1):
    """srs_unique_soa_device on made-up addresses"""
    np_ = len(pays)
    if pays_sorted is None:
        pays_sorted = [PAY_SORTED + 0x100000 * i for i in range(np_)]
    p = (ctypes.c_void_p * max(1, np_))(*pays)
    po = (ctypes.c_void_p * max(1, np_))(*pays_sorted)
    s = (ctypes.c_uint32 * max(1, np_))(*sizes)
    return lib.srs_unique_soa_device(num, kind, up, keys, np_, p if np_ else None,
                                     s if np_ else None, srt,
                                     po if np_ and srt is not None else None, idx, uniq, offs,
                                     inv, nu, nu_host, None)


def test_bad_kind(lib):
    assert _unique(lib, kind=42) == INVALID
    assert b"key_kind" in lib.srs_last_error()


def test_payload_size_3(lib):
    assert _unique(lib, pays=[PAY], sizes=[3]) == UNSUPPORTED
    assert b"1, 2, 4 or 8" in lib.srs_last_error()


def test_payloads_need_the_sorted_columns(lib):
    assert _unique(lib, pays=[PAY], sizes=[8], srt=None) == INVALID
    assert b"num_payloads must be 0" in lib.srs_last_error()
    # keys_sorted_out without payloads_sorted_out
    p = (ctypes.c_void_p * 1)(PAY)
    s = (ctypes.c_uint32 * 1)(8)
    assert lib.srs_unique_soa_device(NUM, U64, 1, KEYS, 1, p, s, SORTED, None, None, UNIQ, None,
                                     None, None, None, None) == INVALID
    assert b"both be set or both NULL" in lib.srs_last_error()


@pytest.mark.parametrize("what", ["key", "payload", "sorted", "payload_sorted", "unique", "indices",
                                  "offsets", "inverse", "num_unique_dev"])
def test_misaligned_pointer(lib, what):
    args = dict(keys=KEYS, pays=[PAY], sizes=[8], srt=SORTED, pays_sorted=[PAY_SORTED], idx=IDX,
                uniq=UNIQ, offs=OFFS, inv=INV, nu=NU)
    if what == "key":
        args["keys"] += 4
    elif what == "payload":
        args["pays"] = [PAY + 2]
    elif what == "sorted":
        args["srt"] += 4
    elif what == "payload_sorted":
        args["pays_sorted"] = [PAY_SORTED + 1]
    elif what == "unique":
        args["uniq"] += 4
    elif what == "indices":
        args["idx"] += 4
    elif what == "offsets":
        args["offs"] += 4
    elif what == "inverse":
        args["inv"] += 4
    else:
        args["nu"] += 4
    assert _unique(lib, **args) == INVALID
    err = lib.srs_last_error()
    assert b"aligned" in err
    for name in ("indices", "offsets", "inverse", "num_unique_dev"):
        if what == name:
            assert name.encode() in err, err


def test_null_pointers(lib):
    assert _unique(lib, uniq=None) == INVALID
    assert b"unique_out is NULL" in lib.srs_last_error()
    assert _unique(lib, keys=None) == INVALID
    assert b"keys is NULL" in lib.srs_last_error()
    assert _unique(lib, num=1, keys=None) == INVALID
    assert b"keys is NULL" in lib.srs_last_error()
    assert _unique(lib, pays=[PAY], sizes=[8], pays_sorted=[0]) == INVALID
    assert b"payload pointer is NULL" in lib.srs_last_error()
    assert _unique(lib, pays=[0], sizes=[8]) == INVALID
    assert b"payload pointer is NULL" in lib.srs_last_error()
    # every other output may be NULL: such a call passes validation and fails
    # only for want of a device or of real memory, which is not asked here


def test_64_payloads_with_an_index_column(lib):
    pays = [PAY + 0x10000 * i for i in range(64)]
    for extra in (dict(idx=IDX), dict(inv=INV)):
        assert _unique(lib, pays=pays, sizes=[8] * 64, **extra) == UNSUPPORTED
        assert b"63" in lib.srs_last_error()


def test_num_plus_one_overflows(lib):
    assert _unique(lib, num=(1 << 63) - 1) == INVALID
    assert b"num + 1 overflows" in lib.srs_last_error()


def test_outputs_overlapping_inputs(lib):
    span = NUM * 8  # bytes of a column of NUM 8-byte records
    msg = b"unique outputs must not overlap the inputs"
    # unique_out at the key column's start, on its last record, reaching into it from below
    for a in (KEYS, KEYS + span - 8, KEYS - (span - 8)):
        assert _unique(lib, uniq=a) == INVALID
        assert msg in lib.srs_last_error()
    # every other output over the key column or a payload column
    for name in ("srt", "idx", "offs", "inv", "nu"):
        assert _unique(lib, **{name: KEYS + 64}) == INVALID, name
        assert msg in lib.srs_last_error()
        assert _unique(lib, pays=[PAY], sizes=[8], **{name: PAY + span - 8}) == INVALID, name
        assert msg in lib.srs_last_error()
    assert _unique(lib, pays=[PAY], sizes=[8], pays_sorted=[KEYS + 64]) == INVALID
    assert msg in lib.srs_last_error()
    # offsets_out holds num + 1 slots: its last one over the key column's first record
    assert _unique(lib, offs=KEYS - span) == INVALID
    assert msg in lib.srs_last_error()


def test_outputs_overlapping_each_other(lib):
    span = NUM * 8
    msg = b"unique outputs must not overlap each other"
    names = dict(srt=SORTED, idx=IDX, uniq=UNIQ, offs=OFFS, inv=INV, nu=NU)
    for a, b in [("srt", "uniq"), ("idx", "inv"), ("uniq", "offs"), ("offs", "inv"),
                 ("idx", "srt"), ("uniq", "nu"), ("offs", "nu"), ("inv", "uniq")]:
        args = {a: names[a], b: names[a] + span - 8}  # b starts on a's last record
        assert _unique(lib, **args) == INVALID, (a, b)
        assert msg in lib.srs_last_error(), (a, b)
    # offsets_out's slot num is part of it
    assert _unique(lib, offs=OFFS, inv=OFFS + span) == INVALID
    assert msg in lib.srs_last_error()
    assert _unique(lib, pays=[PAY], sizes=[8], pays_sorted=[UNIQ + 8]) == INVALID
    assert msg in lib.srs_last_error()


@pytest.mark.parametrize("num", [0, -1, -(1 << 40)])
def test_noop_writes_zero_to_the_host_count(lib, num):
    nu = ctypes.c_int64(77)
    assert _unique(lib, num=num, pays=[PAY], sizes=[8], idx=IDX, offs=OFFS, inv=INV,
                   nu_host=ctypes.byref(nu)) == 0
    assert nu.value == 0
    # (a no-op looks at none of the arrays)
    assert _unique(lib, num=num, keys=None, uniq=None, srt=None, offs=4) == 0


def test_last_info_rejects_null(lib):
    assert lib.srs_debug_last_unique(None) == INVALID
    assert b"info is NULL" in lib.srs_last_error()


def test_run_kernels_do_not_spill_to_scratch():
    """run_tally_kernel and run_write_kernel, all four key widths, in the
    build's compiler remarks: no scratch, no VGPR spill, at least 7 waves per
    SIMD (DESIGN.md §16 quotes the figures)."""
    path = os.path.join(REPO, "simd-radix-sort_amd", "build", "srs_kernels.remarks")
    if not os.path.exists(path):
        pytest.skip("no resource remarks (library built elsewhere)")
    res, cur = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]): (\d+)",
                      line)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    for kernel in ("run_tally_kernel", "run_write_kernel"):
        found = {k: v for k, v in res.items() if kernel in k}
        assert len(found) == 4, (kernel, sorted(found))
        for k, v in found.items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["Occupancy"] >= 7, (k, v)


def _compile(src):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-x", "c++", "-I", os.path.join(REPO, "include"), "-"],
                          input=src.encode(), capture_output=True)


PRELUDE = ('#include "simd_sort/radix_sort.hpp"\n'
           "using namespace simd_sort; namespace dv = simd_sort::radix_sort::device;\n")


def test_cpp_unique_compiles():
    src = (PRELUDE +
           "int main(){ const unsigned long long k[8]={3,1,2,0,7,6,5,4};\n"
           " unsigned long long uq[8], ks[8];\n"
           " const float p[8]={0,1,2,3,4,5,6,7}; float po[8];\n"
           " const short q[8]={0,1,2,3,4,5,6,7}; short qo[8];\n"
           " int64_t* offs = nullptr; int64_t* inv = nullptr; int64_t* idx = nullptr;\n"
           " SortIndex u = dv::unique(nullptr, 8, k, uq, offs, inv,\n"
           "                          (unsigned long long*)nullptr, idx);\n"
           " u += dv::unique<false>(nullptr, 8, k, uq, offs, inv, ks, idx,\n"
           "                        std::pair<const float*, float*>(p, po));\n"
           " u += dv::unique<true>(nullptr, 8, k, uq, offs, inv, ks, idx,\n"
           "                       std::pair<const float*, float*>(p, po),\n"
           "                       std::pair<const short*, short*>(q, qo));\n"
           " return (int)u; }\n")
    r = _compile(src)
    assert r.returncode == 0, r.stderr.decode()[-3000:]


@pytest.mark.parametrize("decl,call,msg", [
    ("struct K3 { char c[3]; }; const K3* k = nullptr; K3* o = nullptr;",
     "dv::unique(nullptr, 8, k, o, offs, inv, o, idx);", "unsupported key type"),
    ("struct P3 { char c[3]; }; const unsigned* k = nullptr; unsigned* o = nullptr;"
     " const P3* p = nullptr; P3* po = nullptr;",
     "dv::unique(nullptr, 8, k, o, offs, inv, o, idx, std::pair<const P3*, P3*>(p, po));",
     "payload sizes must be 1, 2, 4 or 8"),
])
def test_cpp_unique_static_asserts(decl, call, msg):
    src = (PRELUDE + "int main(){ " + decl +
           " int64_t* offs = nullptr; int64_t* inv = nullptr; int64_t* idx = nullptr;\n " + call +
           " return 0; }\n")
    r = _compile(src)
    assert r.returncode != 0 and msg in r.stderr.decode(), r.stderr.decode()[-3000:]
