"""Row-wise top-k on the GPU (srs_topk_rows_soa_device through
srs_amd.topk_rows_device).

The expected result is, per row, the stable argsort of
srs_testlib.transformed_keys(kind, up, row) cut at kk = min(k, row_len) and
applied to every column: exact and unique, so columns are compared as bytes
and indices exactly. Row lengths sit around the sizes at which the resident
route changes its kernel or workgroup (256: one wave per row up to it; 1024,
2048, 4096, 8192 records), around the size from which a row is selected
before it is sorted (max(2 kk, 256)), and past 8192, where the row is
streamed.
"""
import ctypes

import numpy as np
import pytest

from srs_testlib import KIND_DTYPES, KIND_NAMES, transformed_keys

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

U8, U32, U64, F32 = 0, 4, 6, 8
SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
RESIDENT, STREAM, LOOP = 0, 1, 2
CAP = srs_amd.TOPK_ROWS_MAX_K
NMID = 3 * 4096 + 17


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(autouse=True)
def _auto_route():
    yield
    srs_amd.debug_set_topk_rows_route(-1)


def _dev(torch, a):
    """a host array as a device tensor of the signed type of its size"""
    return torch.from_numpy(np.ascontiguousarray(a).view(SINT[a.dtype.itemsize]).copy()).cuda()


def _host(t, like):
    return t.cpu().numpy().view(like.dtype)


def _orders(kind, up, keys2d):
    """(rows, row_len) stable order of every row"""
    u = transformed_keys(kind, up, np.ascontiguousarray(keys2d))
    return np.argsort(u, axis=1, kind="stable")


def _check(torch, kind, up, cols, k, orders=None, dcols=None, route=None, want_route=None,
           stream=None, indices=True):
    """One topk_rows_device call on host matrices `cols` (keys first), compared
    with every row's stable order. Returns debug_last_topk_rows()."""
    rows, n = cols[0].shape
    if orders is None:
        orders = _orders(kind, up, cols[0])
    own = dcols is None
    if own:
        dcols = [_dev(torch, c) for c in cols]
    if route is not None:
        srs_amd.debug_set_topk_rows_route(route)
    res = srs_amd.topk_rows_device(*dcols, k=k, up=up, key_kind=kind, indices=indices,
                                   stream=stream)
    info = srs_amd.debug_last_topk_rows()
    if route is not None:
        srs_amd.debug_set_topk_rows_route(-1)
    kk = max(0, min(k, n))
    sel = orders[:, :kk]
    for c, (r, h) in enumerate(zip(res, cols)):
        assert tuple(r.shape) == (rows, kk)
        want = np.take_along_axis(np.ascontiguousarray(h), sel, axis=1)
        assert np.array_equal(_host(r, h).view(np.uint8), want.view(np.uint8)), \
            f"column {c} differs (rows={rows}, n={n}, k={k}, up={up})"
    if indices:
        assert np.array_equal(res[-1].cpu().numpy(), sel), f"indices differ (rows={rows}, n={n}, k={k})"
    if own:
        for d, h in zip(dcols, cols):
            assert np.array_equal(_host(d, h).view(np.uint8),
                                  np.ascontiguousarray(h).view(np.uint8)), "input written"
    if want_route is not None:
        assert info[0] == want_route, info
    if info[0] in (RESIDENT, STREAM):
        assert info[1] == 1 and info[3] == 0, info  # one launch, nothing read back
    return info


def _shape_cols(shape, rows, n, seed):
    rng = np.random.default_rng(seed)
    if shape == "u64_u64":
        return U64, [rng.integers(0, 1 << 64, (rows, n), dtype=np.uint64),
                     rng.integers(0, 1 << 64, (rows, n), dtype=np.uint64)]
    if shape == "f32_u32_u32":
        k = rng.standard_normal((rows, n)).astype(np.float32)
        k[rng.random((rows, n)) < 0.02] = np.float32(-0.0)  # -0.0 before +0.0
        k[rng.random((rows, n)) < 0.02] = np.float32(0.0)
        return F32, [k, rng.integers(0, 1 << 32, (rows, n), dtype=np.uint32),
                     np.tile(np.arange(n, dtype=np.uint32), (rows, 1))]
    return U32, [rng.integers(0, 1 << 10, (rows, n), dtype=np.uint32)]  # keys only, many ties


def _ks(n):
    return sorted({k for k in (1, 2, 64, 65, n - 1, n, n + 5) if k >= 1})


SHAPES = ["u64_u64", "f32_u32_u32", "keys_only"]


@pytest.mark.parametrize("n", [1, 2, 63, 64, 65, 127, 1000, 4095, 4096, 4097, 8191, 8192])
@pytest.mark.parametrize("shape", SHAPES)
def test_resident_matrix(torch, shape, n):
    for rows in (1, 3, 130):
        kind, cols = _shape_cols(shape, rows, n, seed=n % 1000 + len(shape) + rows)
        orders = _orders(kind, True, cols[0])
        dcols = [_dev(torch, c) for c in cols]
        for k in _ks(n):
            _check(torch, kind, True, cols, k, orders=orders, dcols=dcols, want_route=RESIDENT)
        for d, h in zip(dcols, cols):
            assert np.array_equal(_host(d, h).view(np.uint8), h.view(np.uint8)), "input written"
        _check(torch, kind, False, cols, min(n, 65), want_route=RESIDENT)


@pytest.mark.parametrize("n", [255, 256, 257, 511, 513, 1023, 1024, 1025, 2047, 2048, 2049])
def test_resident_path_boundaries(torch, n):
    """The sizes at which the resident route changes kernel (one wave per row
    up to 256 records) or workgroup size (1024, 2048 records), with k on both
    sides of the select threshold (a row longer than max(2 kk, 256) is
    selected before it is sorted)."""
    for shape in ("u64_u64", "keys_only"):
        kind, cols = _shape_cols(shape, 67, n, seed=n)
        orders = _orders(kind, True, cols[0])
        dcols = [_dev(torch, c) for c in cols]
        for k in sorted({7, 127, 128, 129, (n - 1) // 2, n // 2, n // 2 + 1}):
            _check(torch, kind, True, cols, k, orders=orders, dcols=dcols, want_route=RESIDENT)
        _check(torch, kind, False, cols, 100, dcols=dcols, want_route=RESIDENT)


@pytest.mark.parametrize("n", [8193, NMID, 65541])
@pytest.mark.parametrize("shape", SHAPES)
def test_stream_matrix(torch, shape, n):
    for rows in (1, 3, 70):
        kind, cols = _shape_cols(shape, rows, n, seed=n % 1000 + len(shape) + rows)
        orders = _orders(kind, True, cols[0])
        dcols = [_dev(torch, c) for c in cols]
        for k in (1, 64, 65, CAP - 1, CAP):
            _check(torch, kind, True, cols, k, orders=orders, dcols=dcols, route=STREAM,
                   want_route=STREAM)
        for d, h in zip(dcols, cols):
            assert np.array_equal(_host(d, h).view(np.uint8), h.view(np.uint8)), "input written"
        _check(torch, kind, False, cols, 65, route=STREAM, want_route=STREAM)


def test_k_above_the_stream_cap(torch):
    """Forced stream with k = cap + 1 is refused; the same call on auto takes
    the loop and returns the right answer. The Python constant is the library's."""
    assert CAP == srs_amd.lib().srs_topk_rows_max_k() and CAP >= 1024
    kind, cols = _shape_cols("u64_u64", 3, NMID, seed=9)
    dcols = [_dev(torch, c) for c in cols]
    srs_amd.debug_set_topk_rows_route(STREAM)
    with pytest.raises(srs_amd.SrsError, match="srs error -2"):
        srs_amd.topk_rows_device(*dcols, k=CAP + 1, key_kind=kind)
    srs_amd.debug_set_topk_rows_route(RESIDENT)
    with pytest.raises(srs_amd.SrsError, match="srs error -2"):
        srs_amd.topk_rows_device(*dcols, k=5, key_kind=kind)
    srs_amd.debug_set_topk_rows_route(-1)
    info = _check(torch, kind, True, cols, CAP + 1, dcols=dcols, want_route=LOOP)
    assert info[3] >= 1  # the loop reads back
    _check(torch, kind, True, cols, CAP, dcols=dcols, want_route=STREAM)


@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
@pytest.mark.parametrize("kind", range(10), ids=KIND_NAMES)
def test_every_key_kind(torch, kind, up):
    """All ten key kinds on both one-launch routes; the 8- and 16-bit kinds
    are nearly all ties at these sizes, and the indices of equal keys must
    still ascend (checked against the stable order)."""
    rng = np.random.default_rng(100 + kind)
    dt = np.dtype(KIND_DTYPES[kind])
    for n, route in ((1000, RESIDENT), (12305, STREAM)):
        if dt.kind == "f":
            k = (rng.standard_normal((5, n)) * 1e3).astype(dt)
            k[:, ::97] = 0.0
            k[:, 1::97] = -0.0
        else:
            ii = np.iinfo(dt)
            k = rng.integers(ii.min, int(ii.max) + 1, (5, n), dtype=dt)
        p = rng.integers(0, 1 << 16, (5, n), dtype=np.uint16)
        _check(torch, kind, up, [k, p], 300, want_route=route)


@pytest.mark.parametrize("n,route", [(6000, RESIDENT), (20000, STREAM)])
@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
def test_rows_do_not_share_state(torch, n, route, up):
    """One call whose rows each live in a different top-12-bit bin and have
    different shapes: all equal, ascending, descending, rank k exactly on a
    bucket's end, rank k inside a run of equal keys, random."""
    rng = np.random.default_rng(n)
    k = 100
    rows = []
    rows.append(np.full(n, 0x3456789ABCD, np.uint64))                       # all equal
    rows.append(np.arange(n, dtype=np.uint64) * np.uint64(1 << 30))         # ascending
    rows.append(np.arange(n, dtype=np.uint64)[::-1] * np.uint64(1 << 30))   # descending
    # rank k on a bucket's end: exactly k keys in the extreme 12-bit bin of the
    # row's range, the rest well inside
    edge = rng.integers(1 << 48, 1 << 51, n, dtype=np.uint64)
    pos = rng.choice(n, k, replace=False)
    edge[pos] = rng.integers(0, 1 << 40, k, dtype=np.uint64) if up else \
        (np.uint64((1 << 52) - 1) - rng.integers(0, 1 << 40, k, dtype=np.uint64))
    rows.append(edge)
    # rank k inside a run of equal keys: 40 records beyond a run of 500
    run = rng.integers(1 << 45, 1 << 51, n, dtype=np.uint64)
    pos = rng.choice(n, 540, replace=False)
    run[pos[:500]] = np.uint64(1 << 44)
    run[pos[500:]] = np.uint64(1 << 43) if up else np.uint64(1 << 51)
    if not up:
        run[pos[:500]] = np.uint64((1 << 51) - 7)
        run[pos[500:]] = np.uint64((1 << 52) - 1)
    rows.append(run)
    rows.append(rng.integers(0, 1 << 52, n, dtype=np.uint64))
    # every row in its own top-12-bit bin (the rows' keys stay below 2^52)
    keys = np.stack([r + (np.uint64(37 * (i + 1)) << np.uint64(52)) for i, r in enumerate(rows)])
    assert len(set((keys >> np.uint64(52)).ravel().tolist())) == len(rows)
    pay = rng.integers(0, 1 << 32, keys.shape, dtype=np.uint32)
    _check(torch, U64, up, [keys, pay], k, route=route if route == STREAM else None,
           want_route=route)


def test_refinement_is_real(torch):
    """A streamed row of 40000 u64 keys, k = 100: 15000 keys are >= 2^63, the
    other 25000 share bits 63..40 and are random below. The stop rule: a row
    is refined, one 12-bit digit a pass (the next digit starting at the
    highest bit that still varies among the keys of the pass), until the
    records below the boundary bucket plus the bucket fit the workgroup's LDS
    slots (at most 2 * TOPK_ROWS_MAX_K = 4096 records), the bucket is wholly
    inside the first k, or its keys are all equal. The first pass leaves all
    25000 in the boundary bucket, which fits no LDS; no digit above bit 40
    splits them, so at least a second pass must run."""
    rng = np.random.default_rng(3)
    n = 40000
    keys = np.empty(n, np.uint64)
    big = rng.choice(n, 15000, replace=False)
    m = np.zeros(n, bool)
    m[big] = True
    keys[m] = rng.integers(1 << 63, 1 << 64, 15000, dtype=np.uint64)
    keys[~m] = (np.uint64(0x2ABCDE) << np.uint64(40)) + rng.integers(0, 1 << 40, 25000, dtype=np.uint64)
    pay = np.arange(n, dtype=np.uint64)
    info = _check(torch, U64, True, [keys[None, :], pay[None, :]], 100, route=STREAM,
                  want_route=STREAM)
    assert info[2] >= 2, info
    info = _check(torch, U64, True, [np.tile(keys, (4, 1)), np.tile(pay, (4, 1))], 100,
                  route=STREAM, want_route=STREAM)
    assert info[2] >= 2, info


@pytest.mark.parametrize("n,route", [(777, RESIDENT), (5001, RESIDENT), (9001, STREAM)])
@pytest.mark.parametrize("kind", [U8, U32, U64], ids=["u8", "u32", "u64"])
@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
def test_stride_and_guards(torch, kind, up, n, route):
    """row_stride = row_len + 3 puts row starts off the 16-byte grid; the
    padding holds the winning key and must never be selected; outputs carry a
    sentinel tail that must survive."""
    rows, k = 7, 40
    dt = np.dtype(KIND_DTYPES[kind])
    ii = np.iinfo(dt)
    rng = np.random.default_rng(n + kind)
    full = rng.integers(1, int(ii.max), (rows, n + 3), dtype=dt)
    full[:, n:] = 0 if up else ii.max
    pfull = rng.integers(0, 1 << 16, (rows, n + 3), dtype=np.uint16)
    dk, dp = _dev(torch, full), _dev(torch, pfull)
    vk, vp = dk[:, :n], dp[:, :n]
    assert vk.stride(0) == n + 3 and vk.data_ptr() == dk.data_ptr()
    tail = 64
    ko = torch.full((rows * k + tail,), 0x5A, dtype=dk.dtype, device="cuda")
    po = torch.full((rows * k + tail,), 0x5A5A, dtype=dp.dtype, device="cuda")
    if route == STREAM:
        srs_amd.debug_set_topk_rows_route(STREAM)
    res = srs_amd.topk_rows_device(vk, vp, k=k, up=up, key_kind=kind, out=(ko, po), indices=True)
    info = srs_amd.debug_last_topk_rows()
    assert info[0] == route and info[3] == 0
    sel = _orders(kind, up, full[:, :n])[:, :k]
    assert np.array_equal(res[2].cpu().numpy(), sel)
    hk, hp = _host(ko, full), _host(po, pfull)
    assert np.array_equal(hk[:rows * k].reshape(rows, k), np.take_along_axis(full[:, :n], sel, 1))
    assert np.array_equal(hp[:rows * k].reshape(rows, k), np.take_along_axis(pfull[:, :n], sel, 1))
    assert np.all(hk[rows * k:] == 0x5A) and np.all(hp[rows * k:] == 0x5A5A)
    assert np.array_equal(_host(dk, full), full) and np.array_equal(_host(dp, pfull), pfull)


@pytest.mark.parametrize("n,k,route", [(512, 10, RESIDENT), (8000, 70, RESIDENT),
                                       (9000, 70, STREAM)])
def test_no_host_in_the_loop(torch, n, k, route):
    """One launch and no read-back whether the call has 1 row or 130."""
    infos = []
    for rows in (1, 130):
        kind, cols = _shape_cols("u64_u64", rows, n, seed=rows)
        infos.append(_check(torch, kind, True, cols, k, route=route if route == STREAM else None,
                            want_route=route))
    assert infos[0][1] == infos[1][1] == 1
    assert infos[0][3] == infos[1][3] == 0


@pytest.mark.parametrize("n,k", [(5000, 33), (8192, 8192), (20000, 100), (NMID, CAP)])
def test_one_row_equals_topk_device(torch, n, k):
    kind, cols = _shape_cols("f32_u32_u32", 1, n, seed=n)
    dcols = [_dev(torch, c) for c in cols]
    a = srs_amd.topk_rows_device(*dcols, k=k, key_kind=kind, indices=True)
    b = srs_amd.topk_device(*[d[0] for d in dcols], k=k, key_kind=kind, indices=True)
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert np.array_equal(x.cpu().numpy().ravel().view(np.uint8), y.cpu().numpy().view(np.uint8))


def test_four_long_rows_equal_four_single_calls(torch):
    n, k = 1 << 18, 77
    kind, cols = _shape_cols("u64_u64", 4, n, seed=18)
    dcols = [_dev(torch, c) for c in cols]
    a = srs_amd.topk_rows_device(*dcols, k=k, key_kind=kind, indices=True)
    info = srs_amd.debug_last_topk_rows()
    assert info[0] == STREAM
    for r in range(4):
        b = srs_amd.topk_device(*[d[r] for d in dcols], k=k, key_kind=kind, indices=True)
        for x, y in zip(a, b):
            assert np.array_equal(x[r].cpu().numpy().view(np.uint8), y.cpu().numpy().view(np.uint8))


def test_loop_route_matches(torch):
    """The slow route on shapes of both one-launch routes, with padding."""
    for n in (300, NMID):
        kind, cols = _shape_cols("f32_u32_u32", 3, n + 2, seed=n)
        dcols = [_dev(torch, c)[:, :n] for c in cols]
        _check(torch, kind, False, [c[:, :n] for c in cols], 50, dcols=dcols, route=LOOP,
               want_route=LOOP)


def test_plumbing(torch):
    """A non-default stream, two calls of different shapes back to back, out=
    tensors, a sliced 2-D view."""
    st = torch.cuda.Stream()
    kind, cols = _shape_cols("u64_u64", 9, 3000, seed=1)
    kind2, cols2 = _shape_cols("f32_u32_u32", 5, 10000, seed=2)
    with torch.cuda.stream(st):
        d1 = [_dev(torch, c) for c in cols]
        d2 = [_dev(torch, c) for c in cols2]
        st.synchronize()
        _check(torch, kind, True, cols, 17, dcols=d1, stream=st, want_route=RESIDENT)
        _check(torch, kind2, True, cols2, 500, dcols=d2, stream=st, want_route=STREAM)
        _check(torch, kind, False, cols, 3000, dcols=d1, stream=st, want_route=RESIDENT)
    # out= tensors (2-D and flat) and a sliced view
    view = [d[:, :2500] for d in d1]
    out = (torch.zeros((9, 20), dtype=d1[0].dtype, device="cuda"),
           torch.zeros(9 * 20 + 5, dtype=d1[1].dtype, device="cuda"))
    res = srs_amd.topk_rows_device(*view, k=20, key_kind=kind, out=out)
    torch.cuda.synchronize()
    assert res[0] is out[0] and res[1] is out[1]
    sel = _orders(kind, True, cols[0][:, :2500])[:, :20]
    for o, h in zip(out, cols):
        got = _host(o, h).ravel()[:9 * 20].reshape(9, 20)
        assert np.array_equal(got, np.take_along_axis(h[:, :2500], sel, 1))
    with pytest.raises(ValueError):
        srs_amd.topk_rows_device(d1[0].t(), k=3, key_kind=kind)
    with pytest.raises(ValueError):
        srs_amd.topk_rows_device(d1[0], d1[1][:, :100], k=3, key_kind=kind)
    with pytest.raises(ValueError):
        srs_amd.topk_rows_device(*view, k=20, key_kind=kind, out=(out[0][:, :5], out[1]))
