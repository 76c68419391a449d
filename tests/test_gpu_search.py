"""GPU tests of search-sorted (srs_search_sorted_device,
srs_amd.searchsorted_device): the smallest shapes at which the kernel can go
wrong. Every raw call goes through srs_search_testlib.run_search: outputs
between guard words, compared byte for byte with numpy.searchsorted of the
transformed keys, inputs unwritten, srs_debug_last_search as forced.
"""
import numpy as np
import pytest

import srs_search_testlib as sl
import srs_unique_testlib as ul
from srs_testlib import KIND_DTYPES, KIND_NAMES, key_size, transformed_keys

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

U8, U32, I32, U64, I64, F32, F64 = 0, 4, 5, 6, 7, 8, 9
TILE = srs_amd.SEARCH_QUERY_TILE
FIT = srs_amd.SEARCH_LDS_RANGE        # a table range of up to FIT keys is staged whole
SAMPLES = srs_amd.SEARCH_LDS_SAMPLES  # the LDS sample's slots
SIZES = sorted({1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 100_003,
                FIT - 1, FIT, FIT + 1, SAMPLES - 1, SAMPLES, SAMPLES + 1})
ROUTES = [0, 1]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


def _is_float(kind):
    return np.dtype(KIND_DTYPES[kind]).kind == "f"


def _table(kind, up, n, distinct, rng):
    keys = ul.random_keys(kind, n, distinct, rng)
    if _is_float(kind) and n >= 64:
        keys[:32] = ul.special_floats(kind, 32, rng)
    return sl.sorted_table(kind, up, keys)


def _queries(kind, up, table, rng):
    """probe_queries shuffled, with the type's two ends in front: the first
    tile's range is then the whole table, the others' ranges are random"""
    extra = ul.special_floats(kind, 40, rng) if _is_float(kind) else ()
    q = sl.probe_queries(kind, up, table, extra)
    if _is_float(kind):  # (the ends of the transformed range are NaNs)
        ends = np.array([-np.inf, np.inf] if up else [np.inf, -np.inf], KIND_DTYPES[kind])
    else:
        ends = sl.from_transformed(kind, up,
                                   np.array([0, (1 << (8 * key_size(kind))) - 1], np.uint64))
    return np.concatenate([ends, rng.permutation(q)])


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("kind", range(10), ids=KIND_NAMES)
def test_kinds_and_sizes(torch, kind, up, route):
    rng = np.random.default_rng(1000 + kind * 4 + up * 2 + route)
    for n in SIZES:
        table = _table(kind, up, n, n // 3 + 1, rng)
        sl.run_search(torch, srs_amd, kind, up, table, _queries(kind, up, table, rng), route=route)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("nq", [1, 63, TILE - 1, TILE, TILE + 1])
@pytest.mark.parametrize("kind", [U8, U64, F32], ids=["u8", "u64", "f32"])
def test_query_counts(torch, kind, nq, route):
    rng = np.random.default_rng(nq * 7 + kind)
    for n in (1, 300, FIT + 1, 50_000):
        table = _table(kind, True, n, n // 2 + 1, rng)
        q = _queries(kind, True, table, rng)
        q = q[rng.integers(0, len(q), nq)]
        sl.run_search(torch, srs_amd, kind, True, table, q, route=route)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("kind", [U32, F64], ids=["u32", "f64"])
@pytest.mark.parametrize("shape", ["equal", "two_runs", "increasing"])
def test_table_shapes(torch, shape, kind, up, route):
    """all keys equal; two distinct keys in runs of 10 000 (lower and upper far
    apart, a run over several sample slices); strictly increasing"""
    dt = KIND_DTYPES[kind]
    rng = np.random.default_rng(77)
    if shape == "equal":
        keys = np.full(30_000, 7, dt)
    elif shape == "two_runs":
        keys = np.repeat(np.array([-3 if _is_float(kind) else 3, 11], dt), 10_000)
    else:
        keys = (np.arange(50_000) * 3 + 5).astype(dt)
    table = sl.sorted_table(kind, up, keys)
    q = _queries(kind, up, table, rng)
    lo, hi = sl.expected(kind, up, table, q)
    if shape == "two_runs":
        assert (hi - lo).max() == 10_000
    sl.run_search(torch, srs_amd, kind, up, table, q, route=route, exp=(lo, hi, 0))
    # the same queries in order: every tile's range is narrow
    qs = sl.sorted_table(kind, up, q)
    for flags in (0, sl.HINT):
        sl.run_search(torch, srs_amd, kind, up, table, qs, route=route, flags=flags)


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("outputs", [("lower",), ("upper",), ("lower", "upper")])
def test_single_outputs_skewed_addresses_and_a_stream(torch, outputs, route):
    rng = np.random.default_rng(len(outputs) + 10 * route)
    stream = torch.cuda.Stream()
    for kind, skew in ((U8, 3), (2, 1), (F32, 1), (U64, 1), (I64, 0)):
        table = _table(kind, True, 9_001, 700, rng)
        q = _queries(kind, True, table, rng)[:5_000]
        for st in (None, stream):
            if st is not None:
                st.wait_stream(torch.cuda.current_stream())
            sl.run_search(torch, srs_amd, kind, True, table, q, outputs=outputs, route=route,
                          skew_elems=skew, stream=st, with_bad=(st is None))


@pytest.mark.parametrize("kind", [U32, I64, F32], ids=["u32", "i64", "f32"])
@pytest.mark.parametrize("up", [True, False])
def test_hint_never_changes_a_result(torch, kind, up):
    """the hint with sorted queries and with shuffled queries gives the same
    bytes as the call without it, on the library's own route and on both
    forced ones"""
    rng = np.random.default_rng(5 + kind)
    for n in (FIT, 3 * FIT + 5, 100_003):
        table = _table(kind, up, n, n // 3 + 1, rng)
        shuffled = _queries(kind, up, table, rng)[:20_000]
        for q in (sl.sorted_table(kind, up, shuffled), shuffled):
            exp = sl.expected(kind, up, table, q) + (0,)
            plain = sl.run_search(torch, srs_amd, kind, up, table, q, route=-1, exp=exp)
            for route in (-1, 0, 1):
                hinted = sl.run_search(torch, srs_amd, kind, up, table, q, route=route,
                                       flags=sl.HINT, exp=exp)
                assert hinted == plain


@pytest.mark.parametrize("route", ROUTES)
def test_empty_table_writes_zeros(torch, route):
    q = np.arange(TILE + 5, dtype=np.uint32)
    empty = np.zeros(0, np.uint32)
    for outputs in (("lower",), ("lower", "upper")):
        sl.run_search(torch, srs_amd, U32, True, empty, q, outputs=outputs, route=route)
    # segmented: only a valid empty segment is good
    offsets = np.array([0, 0, 0, 3], np.int64)
    qseg = np.arange(len(q)) % 5 - 1   # -1 .. 3
    lo, hi, bad = sl.expected_segmented(U32, True, empty, offsets, q, qseg)
    assert bad == np.count_nonzero((qseg < 0) | (qseg >= 2)) and set(lo) == {0, -1}
    sl.run_search(torch, srs_amd, U32, True, empty, q, offsets=offsets, qseg=qseg, route=route,
                  exp=(lo, hi, bad))


SEG_LENS = [0, 1, 5, 0, 20_000, 1, 300, 0, 64, 1, 2_500, 0]


def _segmented_case(kind, up, rng):
    offsets = np.concatenate([[0], np.cumsum(SEG_LENS)]).astype(np.int64)
    parts = [_table(kind, up, n, n // 3 + 1, rng) for n in SEG_LENS if n]
    table = np.concatenate(parts)
    # queries: keys of the whole table and their neighbours, spread over all segments
    q = _queries(kind, up, sl.sorted_table(kind, up, table), rng)[:30_000]
    qseg = rng.integers(0, len(SEG_LENS), len(q)).astype(np.int64)
    qseg[0:2] = 4  # (the two ends of the key range go to the long segment)
    return table, offsets, q, qseg


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("kind", [U8, I32, U64, F64], ids=["u8", "i32", "u64", "f64"])
def test_segmented(torch, kind, up):
    rng = np.random.default_rng(300 + kind)
    table, offsets, q, qseg = _segmented_case(kind, up, rng)
    lo, hi, bad = sl.expected_segmented(kind, up, table, offsets, q, qseg)
    assert bad == 0 and lo.min() == 0 and hi.max() == 20_000
    for outputs in (("lower", "upper"), ("upper",)):
        # (the route hook is ignored: run_search expects route 0 in the report)
        for route in ROUTES:
            sl.run_search(torch, srs_amd, kind, up, table, q, offsets=offsets, qseg=qseg,
                          outputs=outputs, route=route, exp=(lo, hi, bad))
    sl.run_search(torch, srs_amd, kind, up, table, q, offsets=offsets, qseg=qseg, with_bad=False,
                  exp=(lo, hi, bad))


def test_segmented_bad_queries(torch):
    """ids -1 and num_segments, a decreasing pair of offsets and an end beyond
    num: those queries receive -1 and are counted exactly, the good ones of
    the same call stay right"""
    kind, up = U64, True
    rng = np.random.default_rng(9)
    table, offsets, q, qseg = _segmented_case(kind, up, rng)
    nseg = len(SEG_LENS)
    qseg[::7] = -1
    qseg[3::11] = nseg
    qseg[5::13] = 1 << 40
    lo, hi, bad = sl.expected_segmented(kind, up, table, offsets, q, qseg)
    assert bad == np.count_nonzero((qseg < 0) | (qseg >= nseg)) > 0
    sl.run_search(torch, srs_amd, kind, up, table, q, offsets=offsets, qseg=qseg,
                  exp=(lo, hi, bad))
    # segment 6 ends before it starts, the last segment ends beyond num;
    # segment 7 then starts inside segment 6's records and is not queried
    broken = offsets.copy()
    broken[7] = broken[6] - 1
    broken[nseg] = len(table) + 5
    qseg = np.where(qseg == 7, 4, qseg)
    lo, hi, bad2 = sl.expected_segmented(kind, up, table, broken, q, qseg)
    n6, nlast = np.count_nonzero(qseg == 6), np.count_nonzero(qseg == nseg - 1)
    assert n6 > 0 and nlast > 0 and bad2 == np.count_nonzero((qseg < 0) | (qseg >= nseg)) + n6 + nlast
    assert np.count_nonzero(lo >= 0) > len(q) // 2
    sl.run_search(torch, srs_amd, kind, up, table, q, offsets=broken, qseg=qseg,
                  exp=(lo, hi, bad2))
    # negative offsets
    broken = offsets.copy()
    broken[0] = -4
    lo, hi, bad3 = sl.expected_segmented(kind, up, table, broken, q, qseg)
    sl.run_search(torch, srs_amd, kind, up, table, q, offsets=broken, qseg=qseg,
                  exp=(lo, hi, bad3))


def test_unsorted_table_stays_inside_the_columns(torch):
    rng = np.random.default_rng(4)
    n = 3 * FIT + 11
    table = torch.from_numpy(rng.integers(0, 1 << 30, n, dtype=np.int64)).cuda()
    q = torch.from_numpy(rng.integers(0, 1 << 30, 5 * TILE + 3, dtype=np.int64)).cuda()
    for route in ROUTES:
        srs_amd.debug_set_search_route(route)
        try:
            lo, hi = srs_amd.searchsorted_device(table, q, side="both")
        finally:
            srs_amd.debug_set_search_route(-1)
        for r in (lo, hi):
            assert int(r.min()) >= 0 and int(r.max()) <= n


def test_table_of_more_than_2_31_keys(torch):
    """table[i] = i * 256 // N for N = 2^31 + 4097: the bounds of value v are
    ceil(v N / 256) and ceil((v + 1) N / 256)"""
    N = (1 << 31) + 4097
    try:
        table = torch.empty(N, dtype=torch.uint8, device="cuda")
        chunk = 1 << 26
        for a in range(0, N, chunk):
            b = min(N, a + chunk)
            table[a:b] = (torch.arange(a, b, dtype=torch.int64, device="cuda") * 256 // N).to(
                torch.uint8)
    except torch.cuda.OutOfMemoryError:
        pytest.skip("no room for a 2.1 GB table")
    v = np.random.default_rng(31).integers(0, 256, 1024)
    q = torch.from_numpy(v.astype(np.uint8)).cuda()
    srs_amd.debug_set_search_route(0)
    try:
        lo, hi = srs_amd.searchsorted_device(table, q, side="both")
    finally:
        srs_amd.debug_set_search_route(-1)
    assert srs_amd.debug_last_search()[0] == 0
    want_lo = np.array([-((-int(x) * N) // 256) for x in v], np.int64)
    want_hi = np.array([-((-(int(x) + 1) * N) // 256) for x in v], np.int64)
    assert want_hi.max() == N
    assert np.array_equal(lo.cpu().numpy(), want_lo)
    assert np.array_equal(hi.cpu().numpy(), want_hi)


def test_python_group_lookup_matches_unique(torch):
    rng = np.random.default_rng(12)
    keys = torch.from_numpy(ul.random_keys(I64, 50_000, 900, rng)).cuda()
    g = srs_amd.unique_device(keys, return_inverse=True, return_counts=True)
    assert torch.equal(srs_amd.searchsorted_device(g.unique, keys), g.inverse)
    lo, hi = srs_amd.searchsorted_device(g.unique, keys, side="both")
    assert torch.equal(lo, g.inverse) and torch.equal(hi - lo, torch.ones_like(lo))
    # against the sorted column the difference is the group's size
    s = srs_amd.unique_device(keys, return_sorted=True).sorted[0]
    lo, hi = srs_amd.searchsorted_device(s, keys, side="both")
    assert torch.equal(hi - lo, g.counts[g.inverse])
    right = srs_amd.searchsorted_device(s, keys, side="right", queries_sorted=True)
    assert torch.equal(right, hi)


def test_the_library_rule_follows_the_measured_grid(torch):
    """the queries are sorted first against a table of 2^22 keys
    from 2^20 queries of 8 bytes (2^22 of 4 bytes) on, never with the hint,
    never below either bound"""
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    table = torch.randint(-(1 << 40), 1 << 40, (1 << 22,), device="cuda", generator=g).sort().values
    q = torch.randint(-(1 << 40), 1 << 40, (1 << 20,), device="cuda", generator=g)
    want = torch.searchsorted(table, q)
    for tb, qq, hint, route in ((table, q, False, 1), (table, q, True, 0),
                                (table, q[:(1 << 20) - 1], False, 0),
                                (table[:(1 << 22) - 1], q, False, 0),
                                (table.int(), q.int(), False, 0)):
        lo = srs_amd.searchsorted_device(tb, qq, queries_sorted=hint)
        info = srs_amd.debug_last_search()
        assert info[0] == route and info[3] == route, (tb.numel(), qq.numel(), hint, info)
        if tb.dtype == torch.int64 and tb.numel() == table.numel():
            assert torch.equal(lo, want[:qq.numel()])


def test_python_shapes_and_types(torch):
    table = torch.arange(0, 3000, 3, dtype=torch.float32, device="cuda")
    q = torch.rand(7, 11, 5, device="cuda") * 3000
    lo = srs_amd.searchsorted_device(table, q)
    assert lo.shape == q.shape and lo.dtype == torch.int64
    assert torch.equal(lo, torch.searchsorted(table, q))
    out = (torch.empty_like(lo), torch.empty_like(lo))
    res = srs_amd.searchsorted_device(table, q, side="both", out=out)
    assert res[0] is out[0] and res[1] is out[1] and torch.equal(out[0], lo)
    assert torch.equal(out[1], torch.searchsorted(table, q, right=True))
    # a descending table
    down = table.flip(0).contiguous()
    lo = srs_amd.searchsorted_device(down, q, up=False)
    assert torch.equal(lo, 1000 - torch.searchsorted(table, q, right=True))
    with pytest.raises(TypeError):
        srs_amd.searchsorted_device(table, q.double())
    with pytest.raises(TypeError):
        srs_amd.searchsorted_device(table, q, offsets=torch.tensor([0, 1000]),
                                    query_segments=torch.zeros(q.shape, dtype=torch.int64,
                                                               device="cuda"))
    with pytest.raises(TypeError):
        srs_amd.searchsorted_device(table, q, offsets=torch.tensor([0, 1000], device="cuda"),
                                    query_segments=torch.zeros(q.shape, dtype=torch.int32,
                                                               device="cuda"))
    with pytest.raises(ValueError):
        srs_amd.searchsorted_device(table, q, side="middle")
    # empty queries, empty table
    e = srs_amd.searchsorted_device(table, q[:0])
    assert e.shape == q[:0].shape
    z = srs_amd.searchsorted_device(table[:0], q, side="right")
    assert z.shape == q.shape and int(z.abs().max()) == 0


def test_python_segmented(torch):
    offsets = torch.tensor([0, 4, 4, 10], device="cuda")
    table = torch.tensor([1, 3, 3, 9, 0, 2, 4, 6, 8, 8], dtype=torch.int32, device="cuda")
    q = torch.tensor([[3, 3, 3], [8, 100, 5]], dtype=torch.int32, device="cuda")
    seg = torch.tensor([[0, 1, 2], [2, 3, -1]], device="cuda")
    lo, hi, bad = srs_amd.searchsorted_device(table, q, side="both", offsets=offsets,
                                              query_segments=seg)
    assert lo.tolist() == [[1, 0, 2], [4, -1, -1]] and hi.tolist() == [[3, 0, 2], [6, -1, -1]]
    assert bad.shape == (1,) and int(bad) == 2
    left, bad = srs_amd.searchsorted_device(table, q, offsets=offsets, query_segments=seg)
    assert torch.equal(left, lo) and int(bad) == 2
