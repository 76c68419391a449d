"""Row-wise sort on the GPU (srs_sort_rows_soa_device through
srs_amd.sort_rows_device).

The expected result is, per row, the stable argsort of
srs_testlib.transformed_keys(kind, up, row) applied to every column: exact and
unique, so columns are compared as bytes and indices exactly. Row lengths sit
around the sizes at which a route changes its kernel: 64 / 256 (one wave per
row), 4096 (the small and the large local class), 8192 (the LDS capacity, past
which the global levels run), and two lengths that take more than one tile.
Every length runs on every route that takes it, and the routes must agree
byte for byte. Routes 1 and 2 run both after the prepare pass (in place on the
outputs) and without it (dense rows, no indices: segment lists that start in
the caller's input and end in distinct outputs).
"""
import numpy as np
import pytest

from srs_testlib import KIND_DTYPES, KIND_NAMES, transformed_keys

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

U8, U32, U64, F32 = 0, 4, 6, 8
SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
KERNEL, LOCAL, LEVELS = 0, 1, 2
CAP = 8192
NMID = 3 * 4096 + 17
LENGTHS = [1, 2, 63, 64, 65, 255, 256, 257, 1000, 4095, 4096, 4097, 8191, 8192, 8193, NMID, 70001]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(autouse=True)
def _auto_route():
    yield
    srs_amd.debug_set_sort_rows_route(-1)


def _dev(torch, a):
    """a host array as a device tensor of the signed type of its size"""
    return torch.from_numpy(np.ascontiguousarray(a).view(SINT[a.dtype.itemsize]).copy()).cuda()


def _host(t, like):
    return t.cpu().numpy().view(like.dtype)


def _orders(kind, up, keys2d):
    """(rows, row_len) stable order of every row"""
    u = transformed_keys(kind, up, np.ascontiguousarray(keys2d))
    return np.argsort(u, axis=1, kind="stable")


def _routes_for(n):
    return [LEVELS] if n > CAP else [KERNEL] + ([LOCAL] if n >= 2 else [])


def _check(torch, kind, up, cols, route, orders=None, dcols=None, indices=True, stream=None,
           strided=False):
    """One sort_rows_device call on host matrices `cols` (keys first) forced on
    `route` (None: the library's rule), compared with every row's stable
    order. dcols: the device views to pass (default: dense copies of cols).
    Returns (the result columns' bytes [+ indices], debug_last_sort_rows())."""
    rows, n = cols[0].shape
    if orders is None:
        orders = _orders(kind, up, cols[0])
    own = dcols is None
    if own:
        dcols = [_dev(torch, c) for c in cols]
    srs_amd.debug_set_sort_rows_route(-1 if route is None else route)
    res = srs_amd.sort_rows_device(*dcols, up=up, key_kind=kind, indices=indices, stream=stream)
    info = srs_amd.debug_last_sort_rows()
    srs_amd.debug_set_sort_rows_route(-1)
    got = []
    for c, (r, h) in enumerate(zip(res, cols)):
        assert tuple(r.shape) == (rows, n)
        want = np.take_along_axis(np.ascontiguousarray(h), orders, axis=1)
        g = _host(r, h).view(np.uint8)
        assert np.array_equal(g, want.view(np.uint8)), \
            f"column {c} differs (rows={rows}, n={n}, up={up}, route={info[0]}, indices={indices})"
        got.append(g)
    if indices:
        g = res[-1].cpu().numpy()
        assert np.array_equal(g, orders), f"indices differ (rows={rows}, n={n}, route={info[0]})"
        got.append(g)
    if own:
        for d, h in zip(dcols, cols):
            assert np.array_equal(_host(d, h).view(np.uint8),
                                  np.ascontiguousarray(h).view(np.uint8)), "input written"
    if route is not None:
        assert info[0] == route, info
    if info[0] == KERNEL:
        assert info[1] == 1 and info[2] == 0 and info[3] == 0, info  # one launch, no read-back
    elif info[0] == LOCAL:
        assert info[2] == 0, info  # no read-back
    else:
        assert info[2] >= 1, info  # a level's counters come back
    if info[0] != KERNEL:  # the prepare pass: strided rows or an index column
        assert info[3] == (1 if (indices or strided) else 0), info
    return got, info


def _both_routes(torch, kind, up, cols, dcols=None, strided=False):
    """Every route that takes the shape, with and without indices; the routes'
    results must be byte-equal (each is compared with the expectation, which
    is unique)."""
    n = cols[0].shape[1]
    orders = _orders(kind, up, cols[0])
    if dcols is None:
        dcols = [_dev(torch, c) for c in cols]
        own = True
    else:
        own = False
    seen = {}
    for route in _routes_for(n):
        for indices in (True, False):
            got, _ = _check(torch, kind, up, cols, route, orders=orders, dcols=dcols,
                            indices=indices, strided=strided)
            if indices in seen:
                for a, b in zip(seen[indices], got):
                    assert np.array_equal(a, b), "the routes disagree"
            seen[indices] = got
    if own:
        for d, h in zip(dcols, cols):
            assert np.array_equal(_host(d, h).view(np.uint8), h.view(np.uint8)), "input written"


def _shape_cols(shape, rows, n, seed):
    rng = np.random.default_rng(seed)
    if shape == "u64_u64":  # the direct kernel's pm 0 (without indices)
        return U64, [rng.integers(0, 1 << 64, (rows, n), dtype=np.uint64),
                     rng.integers(0, 1 << 64, (rows, n), dtype=np.uint64)]
    if shape == "f32_u32_u32":
        k = rng.standard_normal((rows, n)).astype(np.float32)
        k[rng.random((rows, n)) < 0.02] = np.float32(-0.0)  # -0.0 before +0.0
        k[rng.random((rows, n)) < 0.02] = np.float32(0.0)
        return F32, [k, rng.integers(0, 1 << 32, (rows, n), dtype=np.uint32),
                     np.tile(np.arange(n, dtype=np.uint32), (rows, 1))]
    return U32, [rng.integers(0, 1 << 10, (rows, n), dtype=np.uint32)]  # keys only, many ties


SHAPES = ["u64_u64", "f32_u32_u32", "keys_only"]


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("shape", SHAPES)
def test_row_lengths(torch, shape, n):
    rows = 5 if n > CAP else 9
    kind, cols = _shape_cols(shape, rows, n, seed=n % 1000 + len(shape))
    _both_routes(torch, kind, True, cols)
    _check(torch, kind, False, cols, _routes_for(n)[-1])


@pytest.mark.parametrize("n", [1, 200, 256, 257, 5000, 8192, 8193, 20000])
def test_auto_rule(torch, n):
    kind, cols = _shape_cols("u64_u64", 6, n, seed=n)
    _, info = _check(torch, kind, True, cols, None)
    if n <= 256:
        assert info[0] == KERNEL
    elif n > CAP:
        assert info[0] == LEVELS
    else:
        assert info[0] in (KERNEL, LOCAL)


@pytest.mark.parametrize("n,indices,want", [(1024, False, KERNEL), (1025, False, LOCAL),
                                            (1025, True, KERNEL), (4096, True, KERNEL),
                                            (4097, True, LOCAL)])
def test_auto_rule_crossovers(torch, n, indices, want):
    """The measured crossovers: a key and one 8-byte payload
    without indices takes the local lists from 1025 records, every other
    column set from 4097."""
    kind, cols = _shape_cols("u64_u64", 4, n, seed=n)
    _, info = _check(torch, kind, True, cols, None, indices=indices)
    assert info[0] == want, info
    kind, cols = _shape_cols("keys_only", 4, n, seed=n)
    _, info = _check(torch, kind, True, cols, None, indices=False)
    assert info[0] == (KERNEL if n <= 4096 else LOCAL), info


@pytest.mark.parametrize("n", [300, 5000, 9000])
def test_payload_widths_together(torch, n):
    rng = np.random.default_rng(n)
    rows = 6
    cols = [rng.integers(0, 1 << 20, (rows, n), dtype=np.uint32)]
    for dt in (np.uint8, np.uint16, np.uint32, np.uint64):
        cols.append(rng.integers(0, int(np.iinfo(dt).max) + 1, (rows, n), dtype=dt))
    _both_routes(torch, U32, True, cols)


@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
@pytest.mark.parametrize("kind", range(10), ids=KIND_NAMES)
def test_every_key_kind(torch, kind, up):
    """All ten key kinds on every route; the 8- and 16-bit kinds are nearly all
    ties at these sizes, and equal keys must keep their input order."""
    rng = np.random.default_rng(100 + kind)
    dt = np.dtype(KIND_DTYPES[kind])
    for n in (1000, 8200):
        if dt.kind == "f":
            k = (rng.standard_normal((5, n)) * 1e3).astype(dt)
            k[:, ::97] = 0.0
            k[:, 1::97] = -0.0
        else:
            ii = np.iinfo(dt)
            k = rng.integers(ii.min, int(ii.max) + 1, (5, n), dtype=dt)
        p = rng.integers(0, 1 << 16, (5, n), dtype=np.uint16)
        _both_routes(torch, kind, up, [k, p])


@pytest.mark.parametrize("n", [300, 4096, 8192, 9000])
def test_ties(torch, n):
    """Rows of all-equal keys and rows of two distinct values (one differing
    in the lowest bit only, one in the highest): at 4096 and 8192 records the
    local chain's buckets are as large as a row, which is what its stable and
    LSD hand-overs exist for."""
    rng = np.random.default_rng(n)
    rows = []
    rows.append(np.full(n, 0x3456789ABCDEF, np.uint64))
    rows.append(np.full(n, 0, np.uint64))
    rows.append(np.uint64(0x7000000000000000) + rng.integers(0, 2, n, dtype=np.uint64))
    rows.append(rng.integers(0, 2, n, dtype=np.uint64) << np.uint64(63))
    rows.append(np.where(rng.random(n) < 0.01, np.uint64(5), np.uint64(1 << 40)))
    keys = np.stack(rows)
    pay = rng.integers(0, 1 << 64, keys.shape, dtype=np.uint64)
    _both_routes(torch, U64, True, [keys, pay])
    if n <= CAP:  # (the counters are this call's on the list routes)
        _check(torch, U64, True, [keys, pay], LOCAL, indices=False)
        print("fallbacks (stable, lsd) at", n, srs_amd.last_fallbacks())
    _both_routes(torch, U32, False, [keys.astype(np.uint32) & np.uint32(1)])


@pytest.mark.parametrize("n", [1, 2, 777, 5001, 9001])
@pytest.mark.parametrize("kind", [U8, U32, U64], ids=["u8", "u32", "u64"])
def test_strides_and_positions(torch, kind, n):
    """row_stride = row_len + 3 (row starts off the 16-byte grid; the padding
    holds the winning key and must never appear), a column slice of a matrix
    twice as wide, and base pointers an odd number of elements into their
    allocation; the outputs carry a sentinel tail that must survive."""
    rows = 7
    dt = np.dtype(KIND_DTYPES[kind])
    ii = np.iinfo(dt)
    rng = np.random.default_rng(n + kind)
    for stride, first in ((n + 3, 0), (2 * n + 8, n // 2), (n + 3, 3), (n, 1)):
        # one flat allocation per column; row r starts at element first + r * stride
        total = first + rows * stride
        flat_k = rng.integers(1, int(ii.max), total, dtype=dt)
        flat_p = rng.integers(0, 1 << 16, total, dtype=np.uint16)
        idx = first + np.arange(rows)[:, None] * stride + np.arange(n)[None, :]
        mask = np.ones(total, bool)
        mask[idx.ravel()] = False
        flat_k[mask] = 0  # (the smallest key: outside every row)
        hk, hp = flat_k[idx], flat_p[idx]
        dk, dp = _dev(torch, flat_k), _dev(torch, flat_p)
        vk = torch.as_strided(dk, (rows, n), (stride, 1), first)
        vp = torch.as_strided(dp, (rows, n), (stride, 1), first)
        assert vk.data_ptr() == dk.data_ptr() + first * dt.itemsize
        _both_routes(torch, kind, True, [hk, hp], dcols=[vk, vp], strided=stride != n)
        assert np.array_equal(_host(dk, flat_k), flat_k) and np.array_equal(_host(dp, flat_p), flat_p)
    # out= tensors with a tail
    tail = 64
    ko = torch.full((rows * n + tail,), 0x5A, dtype=dk.dtype, device="cuda")
    po = torch.full((rows * n + tail,), 0x5A5A, dtype=dp.dtype, device="cuda")
    for route in _routes_for(n):
        srs_amd.debug_set_sort_rows_route(route)
        res = srs_amd.sort_rows_device(vk, vp, key_kind=kind, out=(ko, po))
        srs_amd.debug_set_sort_rows_route(-1)
        assert res[0] is ko and res[1] is po
        order = _orders(kind, True, hk)
        gk, gp = _host(ko, flat_k), _host(po, flat_p)
        assert np.array_equal(gk[:rows * n].reshape(rows, n), np.take_along_axis(hk, order, 1))
        assert np.array_equal(gp[:rows * n].reshape(rows, n), np.take_along_axis(hp, order, 1))
        assert np.all(gk[rows * n:] == 0x5A) and np.all(gp[rows * n:] == 0x5A5A)


@pytest.mark.parametrize("rows,n,route", [(1500, 300, LOCAL), (2500, 260, LOCAL),
                                          (3000, 64, KERNEL), (40, 5000, LOCAL),
                                          (1100, 4096, LOCAL), (1, 8192, LOCAL),
                                          (1, 100000, LEVELS), (1030, 8200, LEVELS)])
def test_many_rows(torch, rows, n, route):
    """Lists above the 1024-entry initial allocation and the 2048-workgroup
    grid clamps of the chain's hand-over kernels; both local classes; one row
    and more than 1024 rows on the levels."""
    for shape in ("u64_u64", "keys_only"):
        kind, cols = _shape_cols(shape, rows, n, seed=rows + n)
        orders = _orders(kind, True, cols[0])
        dcols = [_dev(torch, c) for c in cols]
        for indices in (False, True):
            _check(torch, kind, True, cols, route, orders=orders, dcols=dcols, indices=indices)


def test_forced_route_that_cannot_take_the_shape(torch):
    kind, cols = _shape_cols("u64_u64", 3, 8193, seed=1)
    big = [_dev(torch, c) for c in cols]
    small = [d[:, :8192].contiguous() for d in big]
    one = [d[:, :1].contiguous() for d in big]
    for route, dcols in ((KERNEL, big), (LOCAL, big), (LOCAL, one), (LEVELS, small)):
        srs_amd.debug_set_sort_rows_route(route)
        with pytest.raises(srs_amd.SrsError, match="srs error -2"):
            srs_amd.sort_rows_device(*dcols, key_kind=kind)
    srs_amd.debug_set_sort_rows_route(-1)
    _check(torch, kind, True, cols, None, dcols=big)


def test_stream_and_workspace_left_usable(torch):
    """A non-default stream; then a plain sort and a segment sort right after a
    sort_rows_device call on each list route: the workspace and the lists are
    left usable."""
    st = torch.cuda.Stream()
    kind, cols = _shape_cols("u64_u64", 9, 3000, seed=1)
    kind2, cols2 = _shape_cols("f32_u32_u32", 5, 10000, seed=2)
    with torch.cuda.stream(st):
        d1 = [_dev(torch, c) for c in cols]
        d2 = [_dev(torch, c) for c in cols2]
        st.synchronize()
        for route in (KERNEL, LOCAL):
            _check(torch, kind, True, cols, route, dcols=d1, stream=st)
        _check(torch, kind2, True, cols2, LEVELS, dcols=d2, stream=st)
        _check(torch, kind, False, cols, LOCAL, dcols=d1, stream=st, indices=False)
    st.synchronize()
    rng = np.random.default_rng(5)
    for route, c, k in ((LOCAL, cols, kind), (LEVELS, cols2, kind2)):
        _check(torch, k, True, c, route)
        n = 100_003
        hk = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        hp = rng.integers(0, 1 << 64, n, dtype=np.uint64)
        dk, dp = _dev(torch, hk), _dev(torch, hp)
        srs_amd.sort_device(dk, dp, key_kind=U64)
        o = np.argsort(hk, kind="stable")
        assert np.array_equal(_host(dk, hk), hk[o]) and np.array_equal(_host(dp, hp), hp[o])
        _check(torch, k, True, c, route, indices=False)
        bounds = [0, 10, 10, 5000, 30000, 30001, n]
        dk, dp = _dev(torch, hk), _dev(torch, hp)
        srs_amd.sort_segments_device(dk, dp, bounds=bounds, key_kind=U64)
        wk, wp = hk.copy(), hp.copy()
        for a, b in zip(bounds[:-1], bounds[1:]):
            o = a + np.argsort(hk[a:b], kind="stable")
            wk[a:b], wp[a:b] = hk[o], hp[o]
        assert np.array_equal(_host(dk, hk), wk) and np.array_equal(_host(dp, hp), wp)


@pytest.mark.parametrize("rows,n", [(33, 100), (9, 3000), (4, 8192)])
def test_equals_topk_rows_with_k_row_len(torch, rows, n):
    kind, cols = _shape_cols("f32_u32_u32", rows, n, seed=n)
    dcols = [_dev(torch, c) for c in cols]
    b = srs_amd.topk_rows_device(*dcols, k=n, key_kind=kind, indices=True)
    assert srs_amd.debug_last_topk_rows()[0] == 0
    for route in (None, KERNEL, LOCAL):
        srs_amd.debug_set_sort_rows_route(-1 if route is None else route)
        a = srs_amd.sort_rows_device(*dcols, key_kind=kind, indices=True)
        srs_amd.debug_set_sort_rows_route(-1)
        for x, y in zip(a, b):
            assert np.array_equal(x.cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))


def test_argument_checks(torch):
    kind, cols = _shape_cols("u64_u64", 9, 300, seed=1)
    d1 = [_dev(torch, c) for c in cols]
    with pytest.raises(ValueError):
        srs_amd.sort_rows_device(d1[0].t(), key_kind=kind)
    with pytest.raises(ValueError):
        srs_amd.sort_rows_device(d1[0], d1[1][:, :100], key_kind=kind)
    with pytest.raises(ValueError):
        srs_amd.sort_rows_device(*d1, key_kind=kind, out=(d1[0][:, :5], d1[1]))
    with pytest.raises(srs_amd.SrsError, match="srs error -1"):  # no in-place form
        srs_amd.sort_rows_device(*d1, key_kind=kind, out=tuple(d1))
    assert srs_amd.sort_rows_device(d1[0][:0], key_kind=kind)[0].shape == (0, 300)
