"""CPU tests of the merge entry points (include/srs_c_api.h): the header
declares them, the library exports them, Python wraps them, the argument
validation runs before any device access (the addresses below are never
dereferenced), and both forms of device::merge compile."""
import ctypes
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(REPO, "include", "srs_c_api.h")

FUNCTIONS = ["srs_merge_soa_device", "srs_debug_last_merge"]

U64, U32, U8 = 6, 4, 0  # srs_key_kind
INVALID, UNSUPPORTED = -1, -2
NA, NB = 1000, 300
N = NA + NB
KA, KB, KOUT, SRC = 0x100000, 0x200000, 0x9000000, 0xA000000
PA, PB, POUT = (0x300000, 0x400000), (0x500000, 0x600000), (0xB000000, 0xC000000)
SIZES = (8, 4)


def test_header_declares_the_functions():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    fns = set(re.findall(r"\b(srs_[a-z_0-9]+)\s*\(", text))
    for f in FUNCTIONS:
        assert f in fns, f
    assert re.search(r"#define\s+SRS_MERGE_TILE\s+\d+", text)


def test_header_and_python_agree_on_the_tile():
    import srs_amd
    m = re.search(r"#define\s+SRS_MERGE_TILE\s+(\d+)", open(HEADER).read())
    assert m and int(m.group(1)) == srs_amd.MERGE_TILE
    assert srs_amd.MERGE_TILE >= 256 and srs_amd.MERGE_TILE % 2 == 0


@pytest.fixture(scope="module")
def lib():
    import srs_amd
    return srs_amd.lib()


def test_library_exports_the_functions(lib):
    for f in FUNCTIONS:
        assert hasattr(lib, f), f


def test_python_wraps_the_functions():
    import srs_amd
    for f in ("merge_device", "debug_last_merge"):
        assert callable(getattr(srs_amd, f)), f


def _arr(ptrs):
    return None if ptrs is None else (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _merge(lib, na=NA, nb=NB, kind=U64, up=1, ka=KA, kb=KB, np_=2, pa=PA, pb=PB, sizes=SIZES,
           kout=KOUT, pout=POUT, src=SRC):
    """srs_merge_soa_device on made-up addresses"""
    sz = None if sizes is None else (ctypes.c_uint32 * max(1, len(sizes)))(*sizes)
    return lib.srs_merge_soa_device(na, nb, kind, up, ka, kb, np_, _arr(pa), _arr(pb), sz, kout,
                                    _arr(pout), src, None)


def test_bad_kind(lib):
    assert _merge(lib, kind=42) == INVALID
    assert b"key_kind" in lib.srs_last_error()


def test_bad_payload_size(lib):
    for w in (0, 3, 16):
        assert _merge(lib, sizes=(8, w)) == UNSUPPORTED
        assert b"payload_sizes[1]: payload sizes must be 1, 2, 4 or 8" in lib.srs_last_error()


def test_num_payloads_out_of_range(lib):
    for np_ in (-1, 65, 1 << 20):
        assert _merge(lib, np_=np_) == INVALID
        assert b"num_payloads out of range" in lib.srs_last_error()


def test_negative_counts(lib):
    assert _merge(lib, na=-1) == INVALID
    assert b"num_a" in lib.srs_last_error()
    assert _merge(lib, nb=-5) == INVALID
    assert b"num_b" in lib.srs_last_error()
    # (also when the sum is not positive: a negative count is never a no-op)
    assert _merge(lib, na=-1, nb=0) == INVALID
    assert _merge(lib, na=3, nb=-3) == INVALID
    assert b"num_b" in lib.srs_last_error()


def test_overflows(lib):
    for na, nb in (((1 << 63) - 1, 1), (1 << 62, 1 << 62), (1 << 59, 0), (0, 1 << 60),
                   ((1 << 58) + 1, 1 << 58)):
        assert _merge(lib, na=na, nb=nb) == INVALID, (na, nb)
        assert b"(num_a + num_b) * 16 overflows" in lib.srs_last_error()


@pytest.mark.parametrize("what", ["keys_a", "keys_b", "keys_out", "payloads_a", "payloads_b",
                                  "payloads_out"])
def test_null_columns(lib, what):
    args = {"keys_a": dict(ka=None), "keys_b": dict(kb=None), "keys_out": dict(kout=None),
            "payloads_a": dict(pa=(PA[0], None)), "payloads_b": dict(pb=(None, PB[1])),
            "payloads_out": dict(pout=(POUT[0], None))}[what]
    assert _merge(lib, **args) == INVALID
    # (a payload column is named with its index)
    name = {"payloads_a": "payloads_a[1]", "payloads_b": "payloads_b[0]",
            "payloads_out": "payloads_out[1]"}.get(what, what)
    assert name.encode() + b" is NULL" in lib.srs_last_error(), lib.srs_last_error()


def test_null_payload_arrays(lib):
    assert _merge(lib, pa=None) == INVALID
    assert b"payloads_a is NULL" in lib.srs_last_error()
    assert _merge(lib, pb=None) == INVALID
    assert b"payloads_b is NULL" in lib.srs_last_error()
    assert _merge(lib, pout=None) == INVALID
    assert b"payloads_out is NULL" in lib.srs_last_error()
    assert _merge(lib, sizes=None) == INVALID
    assert b"payload_sizes is NULL" in lib.srs_last_error()


def test_an_empty_side_may_be_null(lib):
    # (the call then fails a later test, made to: source_out over keys_out)
    for args in (dict(na=0, ka=None, pa=None), dict(nb=0, kb=None, pb=None),
                 dict(na=0, ka=None, pa=(None, None))):
        assert _merge(lib, src=KOUT, **args) == INVALID, args
        assert b"overlap each other" in lib.srs_last_error(), args


@pytest.mark.parametrize("what", ["keys_a", "keys_b", "keys_out", "payloads_a", "payloads_b",
                                  "payloads_out", "source_out"])
def test_misaligned_pointer(lib, what):
    args = {"keys_a": dict(ka=KA + 4), "keys_b": dict(kb=KB + 2), "keys_out": dict(kout=KOUT + 1),
            "payloads_a": dict(pa=(PA[0] + 4, PA[1])), "payloads_b": dict(pb=(PB[0], PB[1] + 2)),
            "payloads_out": dict(pout=(POUT[0], POUT[1] + 1)), "source_out": dict(src=SRC + 4)}[what]
    assert _merge(lib, **args) == INVALID
    err = lib.srs_last_error()
    assert b"aligned" in err
    # the message names the argument, a payload column with its index
    name = {"payloads_a": "payloads_a[0]", "payloads_b": "payloads_b[1]",
            "payloads_out": "payloads_out[1]"}.get(what, what)
    assert name.encode() + b" must be" in err, err


def test_columns_are_aligned_to_their_element_size(lib):
    # 4-byte keys and the 4-byte payload at 4 mod 8, one-byte keys anywhere:
    # the alignment test passes (and a later one, made to fail, reports)
    assert _merge(lib, kind=U32, ka=KA + 4, kb=KB + 4, kout=KOUT + 4, pa=(PA[0], PA[1] + 4),
                  src=KOUT) == INVALID
    assert b"overlap each other" in lib.srs_last_error()
    assert _merge(lib, kind=U8, ka=KA + 3, kb=KB + 1, kout=KOUT + 7, src=KOUT) == INVALID
    assert b"overlap each other" in lib.srs_last_error()
    assert _merge(lib, kind=U32, ka=KA + 2) == INVALID
    assert b"aligned" in lib.srs_last_error()


def test_outputs_overlapping_inputs(lib):
    msg = b"merge outputs must not overlap the inputs"
    ins = dict(ka=(KA, NA * 8), kb=(KB, NB * 8), pa0=(PA[0], NA * 8), pa1=(PA[1], NA * 4),
               pb0=(PB[0], NB * 8), pb1=(PB[1], NB * 4))
    outs = dict(kout=N * 8, pout0=N * 8, pout1=N * 4, src=N * 8)
    for o, obytes in outs.items():
        for i, (addr, ibytes) in ins.items():
            # at the input's start, on its last word, reaching into it from below
            for a in (addr, addr + ibytes - 8, addr - (obytes - 8)):
                args = {"kout": dict(kout=a), "pout0": dict(pout=(a, POUT[1])),
                        "pout1": dict(pout=(POUT[0], a)), "src": dict(src=a)}[o]
                assert _merge(lib, **args) == INVALID, (o, i, hex(a))
                assert msg in lib.srs_last_error(), (o, i, hex(a))


def test_outputs_overlapping_each_other(lib):
    msg = b"merge outputs must not overlap each other"
    span = N * 8
    for args in (dict(src=KOUT), dict(src=KOUT + span - 8), dict(src=KOUT - (span - 8)),
                 dict(pout=(KOUT + 8, POUT[1])), dict(pout=(POUT[0], POUT[0] + span - 4)),
                 dict(pout=(POUT[0], SRC + 16))):
        assert _merge(lib, **args) == INVALID, args
        assert msg in lib.srs_last_error(), args


def test_no_records_is_a_noop(lib):
    assert _merge(lib, na=0, nb=0) == 0
    # (a no-op looks at none of the arrays)
    assert _merge(lib, na=0, nb=0, ka=None, kb=None, pa=None, pb=None, kout=None, pout=None,
                  src=4) == 0
    assert _merge(lib, na=0, nb=0, np_=0, ka=3, kb=5, kout=KA, src=KA) == 0


def test_last_info_rejects_null(lib):
    assert lib.srs_debug_last_merge(None) == INVALID
    assert b"info is NULL" in lib.srs_last_error()


def test_merge_kernels_do_not_spill_to_scratch():
    """merge_split_kernel and merge_tile_kernel, four key widths each, in the
    build's compiler remarks: no scratch, no VGPR spill, and the tile kernel's
    LDS (the staged keys and the u16 source slots) as DESIGN.md §18 states."""
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
        m = re.search(r"(ScratchSize \[bytes/lane\]|VGPRs Spill|Occupancy \[waves/SIMD\]|"
                      r"LDS Size \[bytes/block\]): (\d+)", line)
        if m and cur:
            res[cur][m.group(1).split(" [")[0]] = int(m.group(2))
    import srs_amd
    tile = srs_amd.MERGE_TILE
    for name, count in (("merge_split_kernel", 4), ("merge_tile_kernel", 4)):
        found = {k: v for k, v in res.items() if name in k}
        assert len(found) == count, sorted(found)
        for k, v in found.items():
            assert v["ScratchSize"] == 0 and v["VGPRs Spill"] == 0 and v["Occupancy"] >= 4, (k, v)
            if name == "merge_tile_kernel":
                assert v["LDS Size"] in (tile * (4 + 2), tile * (8 + 2)), (k, v)


def _compile(src):
    return subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsyntax-only",
                           "-x", "c++", "-I", os.path.join(REPO, "include"), "-"],
                          input=src.encode(), capture_output=True)


PRELUDE = ('#include "simd_sort/radix_sort.hpp"\n'
           "using namespace simd_sort; namespace dv = simd_sort::radix_sort::device;\n")


def test_cpp_merge_compiles():
    src = (PRELUDE +
           "int main(){ const float a[4]={0,1,2,3}; const float b[2]={1,5}; float o[6];\n"
           " const uint64_t ai[4]={0,1,2,3}; const uint64_t bi[2]={1,5}; uint64_t oi[6];\n"
           " const int32_t pa[4]={0,1,2,3}; const int32_t pb[2]={1,5}; int32_t po[6];\n"
           " const uint8_t qa[4]={0,1,2,3}; const uint8_t qb[2]={1,5}; uint8_t qo[6];\n"
           " int64_t src[6];\n"
           " dv::merge(nullptr, 4, a, 2, b, o);\n"
           " dv::merge(nullptr, 4, a, 2, b, o, src);\n"
           " dv::merge<false>(nullptr, 4, ai, 2, bi, oi, (int64_t*)nullptr);\n"
           " dv::merge(nullptr, 4, ai, 2, bi, oi,\n"
           "           std::tuple<const int32_t*, const int32_t*, int32_t*>(pa, pb, po));\n"
           " dv::merge<false>(nullptr, 4, a, 2, b, o, src,\n"
           "           std::tuple<const int32_t*, const int32_t*, int32_t*>(pa, pb, po),\n"
           "           std::tuple<const uint8_t*, const uint8_t*, uint8_t*>(qa, qb, qo));\n"
           " return 0; }\n")
    r = _compile(src)
    assert r.returncode == 0, r.stderr.decode()[-3000:]


def test_cpp_merge_static_assert():
    src = (PRELUDE + "int main(){ struct K3 { char c[3]; }; const K3* k = nullptr; K3* o = nullptr;\n"
           " dv::merge(nullptr, 8, k, 8, k, o); return 0; }\n")
    r = _compile(src)
    assert r.returncode != 0 and "unsupported key type" in r.stderr.decode(), \
        r.stderr.decode()[-3000:]
