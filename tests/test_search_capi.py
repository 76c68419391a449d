"""CPU tests of the search-sorted entry points (include/srs_c_api.h): the
header declares them, the library exports them, Python wraps them, the
argument validation runs before any device access (the addresses below are
never dereferenced), and both forms of device::search_sorted compile."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srs_c_api.h")

FUNCTIONS = ["srs_search_sorted_device", "srs_debug_set_search_route", "srs_debug_last_search"]

U64, U32 = 6, 4  # srs_key_kind
INVALID = -1
NUM, NQ, NSEG = 1000, 300, 7
KEYS, QUERIES, OFFS, QSEG, LOWER, UPPER, BAD = (
    0x100000, 0x200000, 0x300000, 0x400000, 0x9000000, 0xA000000, 0xB000000)


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = set(re.findall(r"\b(srs_[a-z_0-9]+)\s*\(", text))
    for f in FUNCTIONS:
        assert f in fns, f
    assert re.search(r"#define\s+SRS_SEARCH_QUERIES_SORTED\s+1\b", text)


def test_header_and_python_agree_on_the_kernel_shape():
    import srs_amd
    text = open(HEADER).read()
    for name in ("QUERY_TILE", "LDS_SAMPLES", "LDS_RANGE"):
        m = re.search(r"#define\s+SRS_SEARCH_%s\s+(\d+)" % name, text)
        assert m and int(m.group(1)) == getattr(srs_amd, "SEARCH_" + name), name


@pytest.fixture(scope="module")
def lib():
    import srs_amd
    return srs_amd.lib()


def test_library_exports_the_functions(lib):
    for f in FUNCTIONS:
        assert hasattr(lib, f), f


def test_python_wraps_the_functions():
    import srs_amd
    for f in ("searchsorted_device", "debug_set_search_route", "debug_last_search"):
        assert callable(getattr(srs_amd, f)), f
    assert srs_amd.SEARCH_QUERIES_SORTED == 1


def _search(lib, num=NUM, kind=U64, up=1, keys=KEYS, nseg=0, offs=None, nq=NQ, queries=QUERIES,
            qseg=None, lower=LOWER, upper=UPPER, bad=None, flags=0):
    """srs_search_sorted_device on made-up addresses"""
    return lib.srs_search_sorted_device(num, kind, up, keys, nseg, offs, nq, queries, qseg, lower,
                                        upper, bad, flags, None)


SEG = dict(nseg=NSEG, offs=OFFS, qseg=QSEG, bad=BAD)


def test_bad_kind(lib):
    assert _search(lib, kind=42) == INVALID
    assert b"key_kind" in lib.srs_last_error()


def test_both_outputs_null(lib):
    assert _search(lib, lower=None, upper=None) == INVALID
    assert b"lower_out and upper_out are both NULL" in lib.srs_last_error()


def test_null_inputs(lib):
    assert _search(lib, queries=None) == INVALID
    assert b"queries is NULL" in lib.srs_last_error()
    assert _search(lib, keys=None) == INVALID
    assert b"sorted_keys is NULL" in lib.srs_last_error()


@pytest.mark.parametrize("what", ["sorted_keys", "queries", "offsets", "query_segments",
                                  "lower_out", "upper_out", "num_bad_dev"])
def test_misaligned_pointer(lib, what):
    args = dict(SEG)
    name = {"sorted_keys": "keys", "queries": "queries", "offsets": "offs",
            "query_segments": "qseg", "lower_out": "lower", "upper_out": "upper",
            "num_bad_dev": "bad"}[what]
    base = dict(keys=KEYS, queries=QUERIES, lower=LOWER, upper=UPPER, **SEG)
    args[name] = base[name] + 4
    assert _search(lib, **args) == INVALID
    err = lib.srs_last_error()
    assert b"aligned" in err
    if what not in ("sorted_keys", "queries"):
        assert what.encode() in err, err


def test_keys_are_aligned_to_their_element_size(lib):
    # 4-byte keys at an address that is 4 but not 8 mod 8 pass the alignment
    # test (and fail a later one: the outputs overlap)
    assert _search(lib, kind=U32, keys=KEYS + 4, queries=QUERIES + 4, upper=LOWER) == INVALID
    assert b"overlap each other" in lib.srs_last_error()
    assert _search(lib, kind=U32, keys=KEYS + 2) == INVALID
    assert b"aligned" in lib.srs_last_error()


def test_offsets_and_query_segments_go_together(lib):
    assert _search(lib, nseg=NSEG, offs=OFFS) == INVALID
    assert b"both be set or both NULL" in lib.srs_last_error()
    assert _search(lib, nseg=NSEG, qseg=QSEG) == INVALID
    assert b"both be set or both NULL" in lib.srs_last_error()
    assert _search(lib, nseg=0, offs=OFFS, qseg=QSEG) == INVALID
    assert b"num_segments" in lib.srs_last_error()


def test_unknown_flag_bit(lib):
    for flags in (2, 4, 1 | 8, -2):
        assert _search(lib, flags=flags) == INVALID
        assert b"flags" in lib.srs_last_error()


def test_overflows(lib):
    assert _search(lib, nq=(1 << 63) - 1) == INVALID
    assert b"num_queries * 8 overflows" in lib.srs_last_error()
    assert _search(lib, nq=1 << 60) == INVALID
    assert b"num_queries * 8 overflows" in lib.srs_last_error()
    assert _search(lib, **dict(SEG, nseg=(1 << 63) - 1)) == INVALID
    assert b"num_segments + 1 overflows" in lib.srs_last_error()


def test_outputs_overlapping_inputs(lib):
    msg = b"search outputs must not overlap the inputs"
    ins = dict(keys=(KEYS, NUM * 8), queries=(QUERIES, NQ * 8), offs=(OFFS, (NSEG + 1) * 8),
               qseg=(QSEG, NQ * 8))
    outs = dict(lower=NQ * 8, upper=NQ * 8, bad=8)
    for o, obytes in outs.items():
        for i, (addr, ibytes) in ins.items():
            # at the input's start, on its last word, reaching into it from below
            for a in (addr, addr + ibytes - 8, addr - (obytes - 8)):
                assert _search(lib, **dict(SEG, **{o: a})) == INVALID, (o, i, hex(a))
                assert msg in lib.srs_last_error(), (o, i, hex(a))
    # the flat form looks at the table and the queries
    assert _search(lib, lower=KEYS + 64) == INVALID
    assert msg in lib.srs_last_error()
    assert _search(lib, upper=QUERIES + 64, lower=None) == INVALID
    assert msg in lib.srs_last_error()


def test_outputs_overlapping_each_other(lib):
    msg = b"search outputs must not overlap each other"
    span = NQ * 8
    for args in (dict(upper=LOWER), dict(upper=LOWER + span - 8), dict(upper=LOWER - (span - 8)),
                 dict(SEG, bad=LOWER + 8), dict(SEG, bad=UPPER + span - 8)):
        assert _search(lib, **args) == INVALID, args
        assert msg in lib.srs_last_error(), args


@pytest.mark.parametrize("nq", [0, -1, -(1 << 40)])
def test_no_queries_is_a_noop(lib, nq):
    assert _search(lib, nq=nq) == 0
    # (a no-op looks at none of the arrays)
    assert _search(lib, nq=nq, keys=None, queries=None, lower=None, upper=None, offs=4) == 0


def test_route_hook_validates(lib):
    assert lib.srs_debug_set_search_route(2) == INVALID
    assert b"route must be -1, 0 or 1" in lib.srs_last_error()
    assert lib.srs_debug_set_search_route(-2) == INVALID
    for r in (0, 1, -1):
        assert lib.srs_debug_set_search_route(r) == 0


def test_last_info_rejects_null(lib):
    assert lib.srs_debug_last_search(None) == INVALID
    assert b"info is NULL" in lib.srs_last_error()


def test_search_kernels_do_not_spill_to_scratch():
    """search_kernel, four key widths by two forms, in the build's compiler
    remarks: no scratch and no VGPR spill (DESIGN.md §17 quotes the figures)."""
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
    found = {k: v for k, v in res.items() if "search_kernel" in k}
    assert len(found) == 8, sorted(found)
    for k, v in found.items():
        assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["Occupancy"] >= 4, (k, v)


def _compile(src):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-x", "c++", "-I", os.path.join(REPO, "include"), "-"],
                          input=src.encode(), capture_output=True)


PRELUDE = ('#include "simd_sort/radix_sort.hpp"\n'
           "using namespace simd_sort; namespace dv = simd_sort::radix_sort::device;\n")


def test_cpp_search_sorted_compiles():
    src = (PRELUDE +
           "int main(){ const float t[4]={0,1,2,3}; const float q[2]={1,5};\n"
           " const int64_t ti[4]={0,1,2,3}; const int64_t qi[2]={1,5};\n"
           " int64_t lo[2], hi[2]; const int64_t offs[3]={0,2,4}; const int64_t qs[2]={0,1};\n"
           " int64_t* bad = nullptr;\n"
           " dv::search_sorted(nullptr, 4, t, 2, q, lo, hi);\n"
           " dv::search_sorted<false>(nullptr, 4, t, 2, q, lo, (int64_t*)nullptr,\n"
           "                          SRS_SEARCH_QUERIES_SORTED);\n"
           " dv::search_sorted(nullptr, 4, ti, 2, qi, lo, hi);\n"
           " dv::search_sorted(nullptr, 4, t, 2, offs, 2, q, qs, lo, hi, bad);\n"
           " dv::search_sorted<false>(nullptr, 4, ti, 2, offs, 2, qi, qs, lo, hi, bad);\n"
           " return 0; }\n")
    r = _compile(src)
    assert r.returncode == 0, r.stderr.decode()[-3000:]


def test_cpp_search_sorted_static_assert():
    src = (PRELUDE + "int main(){ struct K3 { char c[3]; }; const K3* k = nullptr;\n"
           " int64_t* lo = nullptr; dv::search_sorted(nullptr, 8, k, 8, k, lo, lo); return 0; }\n")
    r = _compile(src)
    assert r.returncode != 0 and "unsupported key type" in r.stderr.decode(), \
        r.stderr.decode()[-3000:]
