"""Ragged top-k on the GPU (srs_topk_ragged_soa_device through
srs_amd.topk_ragged_device).

The expected result is, per segment, the first min(k, len) entries of
srs_ragged_fuzzlib.ragged_orders (the stable argsort of
srs_testlib.transformed_keys): exact and unique, so columns are compared as
bytes and indices exactly (srs_topk_ragged_testlib.run). Outputs start filled
with 0x5A; every slot j >= min(k, len) and a guard region past num_segments * k
must keep the fill, inputs and offsets their bytes, and counts must equal
min(k, len).

Segment lengths sit at the wave's slab (64), the short / long split (256), the
long kernel's slot capacities (256 .. 4096), a resident row's 8192 and more
than one streamed tile; k at 1, around the split, at the kernel route's
maximum (2048) and past it (the sort route), the last one past every length.
"""
import numpy as np
import pytest

import srs_topk_ragged_testlib as tl
from srs_testlib import KIND_DTYPES

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

U8, U32, U64, F32, F64 = 0, 4, 6, 8, 9
CANARY = 0xC3
SLACK = 4096
BOUNDARY = [0, 0, 1, 2, 3, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1000, 4095, 4096, 4097,
            8191, 8192, 8193, 12305, 20001]
HEAD, TAIL = 37, 53
KS_KERNELS = [1, 2, 64, 255, 256, 257, 2048]
KS_SORT = [2049, 5000, 30000]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


@pytest.fixture(autouse=True)
def _default_route():
    yield
    srs_amd.debug_set_topk_ragged_route(-1)


def _boundary_offsets():
    rng = np.random.default_rng(20262)
    ln = np.array(BOUNDARY, dtype=np.int64)
    ln = ln[rng.permutation(len(ln))]
    offs = HEAD + np.concatenate([[0], np.cumsum(ln)])
    return ln, offs.astype(np.int64), int(offs[-1]) + TAIL


def _keys(kind, n, rng):
    dt = np.dtype(KIND_DTYPES[kind])
    if dt.kind == "f":
        # few distinct values (stability shows), both zeros, both signs
        v = (rng.integers(-40, 40, n) * 0.5).astype(dt)
        v[(v == 0) & (rng.random(n) < 0.5)] = -0.0
        return v
    if dt.itemsize == 1:
        return rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint8).view(dt)
    u = rng.integers(0, 1 << (8 * dt.itemsize), n, dtype=np.uint64)
    u[rng.random(n) < 0.3] &= np.uint64(0xFF)  # runs of equal keys
    return u.astype(np.dtype("u%d" % dt.itemsize)).view(dt)


def _column_set(name, kind, n, seed):
    rng = np.random.default_rng(seed)
    if name == "keys":
        return kind, [_keys(kind, n, rng)]
    if name == "u64_u64":
        return U64, [_keys(U64, n, rng), np.arange(n, dtype=np.uint64)]
    if name == "f32_u32_u32":
        return F32, [_keys(F32, n, rng), np.arange(n, dtype=np.uint32),
                     rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)]
    if name == "u8_u8_u16":
        return U8, [_keys(U8, n, rng), rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint8),
                    np.arange(n, dtype=np.uint64).astype(np.uint16)]
    raise ValueError(name)


# ---------------------------------------------------------------------------
# the boundary mix: one test per kind x column set; every k, both directions,
# with and without indices inside (the order is computed once per direction,
# the device inputs once)
# ---------------------------------------------------------------------------
def _boundary_check(torch, name, kind):
    ln, offs, num = _boundary_offsets()
    assert num == HEAD + sum(BOUNDARY) + TAIL
    kind, cols = _column_set(name, kind, num, 2000 + 17 * kind)
    dcols = [tl.dev(torch, c) for c in cols]
    doffs = torch.from_numpy(offs.copy()).cuda()
    n_short, n_long = tl.class_counts(ln)
    assert (n_short, n_long) == (8, 13)
    for up in (True, False):
        order = tl.orders(kind, up, cols[0], offs)
        for k in KS_KERNELS + KS_SORT:
            for indices in (False, True):
                tl.run(torch, srs_amd, kind, up, cols, offs, k, indices, order=order, dcols=dcols,
                       doffs=doffs, what=name)
                info = srs_amd.debug_last_topk_ragged()
                route = tl.KERNELS if k <= tl.MAX_K else tl.SORT
                assert info[:3] == (route, n_short, n_long), (k, info)
                if route == tl.KERNELS:
                    assert info[4] == 1 and info[5] == 3, (k, info)
                else:
                    assert info[4] >= 1 and info[5] == -1, (k, info)
    assert max(ln) < KS_SORT[-1]


@pytest.mark.parametrize("kind", [U8, U32, U64, F32, F64])
def test_boundary_mix_keys_only(torch, kind):
    _boundary_check(torch, "keys", kind)


@pytest.mark.parametrize("name", ["u64_u64", "f32_u32_u32", "u8_u8_u16"])
def test_boundary_mix_column_sets(torch, name):
    _boundary_check(torch, name, 0)


# ---------------------------------------------------------------------------
# agreement: the two routes, the ragged sort's heads, the row-wise top-k
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("indices", [False, True])
@pytest.mark.parametrize("name", ["u64_u64", "f32_u32_u32"])
def test_routes_agree_and_equal_the_sorts_head(torch, name, indices):
    ln, offs, num = _boundary_offsets()
    kind, cols = _column_set(name, 0, num, 78)
    dcols = [tl.dev(torch, c) for c in cols]
    doffs = torch.from_numpy(offs.copy()).cuda()
    order = tl.orders(kind, False, cols[0], offs)
    full = srs_amd.sort_ragged_device(*dcols, offsets=doffs, up=False, key_kind=kind,
                                      indices=indices)
    full = [t.cpu().numpy() for t in full]
    for k in (5, 300, 2048):
        got = {}
        for route in (tl.KERNELS, tl.SORT):
            srs_amd.debug_set_topk_ragged_route(route)
            got[route] = tl.run(torch, srs_amd, kind, False, cols, offs, k, indices, order=order,
                                dcols=dcols, doffs=doffs, what=f"{name} route {route}")
            assert srs_amd.debug_last_topk_ragged()[0] == route
        for a, b in zip(got[tl.KERNELS], got[tl.SORT]):
            assert np.array_equal(a, b), f"k={k}: the routes disagree"
        # the head of every segment of the ragged sort
        c = got[tl.KERNELS][-1]
        for q, f in enumerate(full):
            w = f.dtype.itemsize
            g = got[tl.KERNELS][q]
            g = g.view(np.int64) if q == len(cols) else g.reshape(-1, w)
            for i in range(len(ln)):
                a, b = i * k, i * k + int(c[i])
                want = f[offs[i]:offs[i] + int(c[i])]
                want = want if q == len(cols) else want.view(np.uint8).reshape(-1, w)
                assert np.array_equal(g[a:b], want), f"k={k} column {q} segment {i}"


def _uniform_equals_topk_rows(torch, kind, cols, rows, n, k, indices):
    offs = np.arange(rows + 1, dtype=np.int64) * n
    got = tl.run(torch, srs_amd, kind, True, cols, offs, k, indices, what="uniform")
    assert srs_amd.debug_last_topk_ragged()[:3] == (tl.KERNELS, 0, rows)
    d2 = [tl.dev(torch, c.reshape(rows, n)) for c in cols]
    res = srs_amd.topk_rows_device(*d2, k=k, up=True, key_kind=kind, indices=indices)
    for q, r in enumerate(res):
        a = got[q]
        if q < len(cols):
            a = a[:rows * k * cols[q].dtype.itemsize]
            assert np.array_equal(a, tl.to_bytes(r)), f"column {q} differs from topk_rows_device"
        else:
            assert np.array_equal(a, r.cpu().numpy().reshape(-1)), "indices differ"


@pytest.mark.parametrize("indices", [False, True])
def test_uniform_offsets_equal_topk_rows(torch, indices):
    """the long kernel against the rows call's resident instance (300 x 700),
    then against its stream instance, whose select the long kernel runs: rows
    of 9001 records (above kLocalCap = 8192: one full tile and a partial one),
    k = 16 (256 slots), keys equal above bit 20, so the first digit resolves
    nothing and a second pass, from the highest varying bit, is needed"""
    rows, n, k = 300, 700, 50
    kind, cols = _column_set("u64_u64", 0, rows * n, rows)
    _uniform_equals_topk_rows(torch, kind, cols, rows, n, k, indices)

    rows, n, k = 3, 9001, 16
    rng = np.random.default_rng(9001)
    keys = (np.uint64(0xABCDE) << np.uint64(20)) | rng.integers(0, 1 << 20, rows * n,
                                                                 dtype=np.uint64)
    top = keys.reshape(rows, n) >> np.uint64(52)
    assert (top == top[:, :1]).all() and n > 256 and n > 8192  # the first pass keeps every record
    _uniform_equals_topk_rows(torch, U64, [keys, np.arange(rows * n, dtype=np.uint64)], rows, n, k,
                              indices)
    info_rows, info_ragged = srs_amd.debug_last_topk_rows(), srs_amd.debug_last_topk_ragged()
    assert info_rows[0] == srs_amd.TOPK_ROWS_STREAM, info_rows
    assert info_rows[2] == info_ragged[3], (info_rows, info_ragged)
    assert info_rows[2] >= 2, info_rows


# ---------------------------------------------------------------------------
# the select's branches: one segment of 20001 records among short ones, k = 16
# ---------------------------------------------------------------------------
LONG = 20001


def _long_among_short(keys_long, dtype):
    """offsets and keys: segments of 3, 100 and 256 records, the long one, 17"""
    ln = np.array([3, 100, 256, LONG, 17], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 100, int(offs[-1])).astype(dtype)
    keys[offs[3]:offs[4]] = keys_long
    return ln, offs, keys


def _select_run(torch, kind, keys_long, k, up=True):
    ln, offs, keys = _long_among_short(keys_long, keys_long.dtype)
    cols = [keys, np.arange(len(keys), dtype=np.uint32)]
    got = tl.run(torch, srs_amd, kind, up, cols, offs, k, True, what="select")
    info = srs_amd.debug_last_topk_ragged()
    assert info[:3] == (tl.KERNELS, 4, 1) and info[4] == 1, info
    return got, info, offs


@pytest.mark.parametrize("up", [True, False])
def test_select_keys_that_differ_in_their_low_bits_only(torch, up):
    """the first digit holds every key: the next one starts at the highest
    varying bit, so a second pass is needed and suffices"""
    rng = np.random.default_rng(31)
    keys = (np.uint64(0xABCD) << np.uint64(40)) | rng.integers(0, 1 << 30, LONG, dtype=np.uint64)
    _, info, _ = _select_run(torch, U64, keys, 16, up)
    assert info[3] >= 2, info


@pytest.mark.parametrize("up", [True, False])
def test_select_four_distinct_values(torch, up):
    """the boundary bucket is larger than the slots and all equal: its first
    records in input order"""
    rng = np.random.default_rng(32)
    keys = np.array([5, 1 << 20, 1 << 40, 1 << 60], dtype=np.uint64)[rng.integers(0, 4, LONG)]
    got, info, offs = _select_run(torch, U64, keys, 16, up)
    assert info[3] >= 1, info
    first = np.flatnonzero(keys == (5 if up else 1 << 60))[:16]
    assert np.array_equal(got[2][3 * 16:4 * 16], first), "not the bucket's first records"


@pytest.mark.parametrize("k", [1, 2048])
def test_select_all_keys_equal(torch, k):
    keys = np.full(LONG, 0x0123456789ABCDEF, dtype=np.uint64)
    got, info, _ = _select_run(torch, U64, keys, k)
    assert np.array_equal(got[2][3 * k:3 * k + k], np.arange(k)), "not the first k in input order"


@pytest.mark.parametrize("up", [True, False])
def test_select_f32_zeros_and_signs(torch, up):
    rng = np.random.default_rng(33)
    table = np.array([0.0, -0.0, 1.5, -1.5, 3e38, -3e38, 1e-40, -1e-40], dtype=np.float32)
    keys = table[rng.integers(0, len(table), LONG)]
    keys[:40] = [0.0, -0.0] * 20
    _select_run(torch, F32, keys, 16, up)
    _select_run(torch, F32, np.where(keys == 0, keys, np.float32(7.0)).astype(np.float32), 16, up)


# ---------------------------------------------------------------------------
# the C ABI itself: indices_out and counts_out with guards, and without them
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("route", [tl.KERNELS, tl.SORT])
def test_c_abi_indices_and_counts_keep_their_guards(torch, route):
    ln, offs, num = _boundary_offsets()
    kind, cols = _column_set("u64_u64", 0, num, 79)
    k, nseg = 100, len(ln)
    src, idx, slot, c = tl.heads(tl.orders(kind, True, cols[0], offs), offs, k)
    dcols = [tl.dev(torch, x) for x in cols]
    doffs = torch.from_numpy(offs.copy()).cuda()
    srs_amd.debug_set_topk_ragged_route(route)
    for with_extras in (True, False):
        alloc = [tl.guarded_out(torch, d, nseg * k) for d in dcols]
        ibig, iview = tl.guarded_out(torch, doffs, nseg * k)
        cbig, cview = tl.guarded_out(torch, doffs, nseg)
        rc = tl.call_c_abi(torch, srs_amd, kind, True, dcols, doffs, k, [v for _, v in alloc],
                           iview if with_extras else None, cview if with_extras else None)
        torch.cuda.synchronize()
        assert rc == 0, srs_amd.lib().srs_last_error()
        for q, ((big, _), h) in enumerate(zip(alloc, cols)):
            tl.check_column(tl.to_bytes(big), h, src, slot, nseg * k, f"column {q}")
        fill = np.frombuffer(bytes([tl.SENTINEL] * 8), dtype=np.int64)[0]
        want_i = np.full(nseg * k + tl.GUARD, fill, dtype=np.int64)
        want_c = np.full(nseg + tl.GUARD, fill, dtype=np.int64)
        if with_extras:
            want_i[slot] = idx
            want_c[:nseg] = c
        assert np.array_equal(ibig.cpu().numpy(), want_i), "indices_out"
        assert np.array_equal(cbig.cpu().numpy(), want_c), "counts_out"


# ---------------------------------------------------------------------------
# bad offsets: an error code, never an access outside the columns. The inputs
# have SLACK canary records on both sides, so even a kernel that followed a
# bad bound would stay inside allocated memory.
# ---------------------------------------------------------------------------
def _guarded_in(torch, host):
    n, w = len(host), host.dtype.itemsize
    big = torch.full(((n + 2 * SLACK) * w,), CANARY, dtype=torch.uint8, device="cuda")
    tint = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[w]
    view = big.view(tint)[SLACK:SLACK + n]
    view.copy_(torch.from_numpy(np.ascontiguousarray(host).view(tl.SINT[w]).copy()))
    return big, view


def _canaries_intact(big, n, w):
    g = big.cpu().numpy()
    return bool(np.all(g[:SLACK * w] == CANARY) and np.all(g[(SLACK + n) * w:] == CANARY))


@pytest.mark.parametrize("which", ["decreasing", "negative", "past_the_end"])
@pytest.mark.parametrize("route", [tl.KERNELS, tl.SORT])
@pytest.mark.parametrize("indices", [False, True])
def test_bad_offsets_return_an_error(torch, which, route, indices):
    n, k = 900, 20
    offs = {"decreasing": [0, 400, 50, 900], "negative": [-5, 400, 900],
            "past_the_end": [0, 400, n + 5]}[which]
    nseg = len(offs) - 1
    kind, cols = _column_set("u64_u64", 0, n, 21)
    ins = [_guarded_in(torch, c) for c in cols]
    outs = [tl.guarded_out(torch, v, nseg * k) for _, v in ins]
    doffs = torch.tensor(offs, dtype=torch.int64, device="cuda")
    srs_amd.debug_set_topk_ragged_route(route)
    with pytest.raises(srs_amd.SrsError) as e:
        srs_amd.topk_ragged_device(*[v for _, v in ins], offsets=doffs, k=k, key_kind=kind,
                                   indices=indices, out=tuple(v for _, v in outs))
    torch.cuda.synchronize()
    assert "srs error -1" in str(e.value) and "1 segment" in str(e.value), str(e.value)
    for (big, _), c in zip(ins, cols):
        assert _canaries_intact(big, n, c.dtype.itemsize), "written outside an input column"
    for (big, _), c in zip(outs, cols):
        g = tl.to_bytes(big)
        assert np.all(g[nseg * k * c.dtype.itemsize:] == tl.SENTINEL), "an output's guard written"
    for (_, v), c in zip(ins, cols):
        assert np.array_equal(tl.to_bytes(v), c.view(np.uint8)), "input written"
    assert doffs.cpu().tolist() == offs
    # the next valid call on the same tensors and workspace is correct
    good = np.array([0, 400, 650, 900], dtype=np.int64)
    tl.run(torch, srs_amd, kind, True, cols, good, k, indices, dcols=[v for _, v in ins],
           what="after the error")
    for (big, _), c in zip(ins, cols):
        assert _canaries_intact(big, n, c.dtype.itemsize)


def test_offsets_must_be_an_int64_device_tensor(torch):
    k = torch.zeros(10, dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        srs_amd.topk_ragged_device(k, offsets=[0, 10], k=3)
    with pytest.raises(TypeError):
        srs_amd.topk_ragged_device(k, offsets=torch.tensor([0, 10], dtype=torch.int64), k=3)
    with pytest.raises(TypeError):
        srs_amd.topk_ragged_device(k, offsets=torch.tensor([0, 10], dtype=torch.int32,
                                                           device="cuda"), k=3)


def test_forced_kernel_route_refuses_a_large_k(torch):
    keys = torch.zeros(100, dtype=torch.int64, device="cuda")
    offs = torch.tensor([0, 100], dtype=torch.int64, device="cuda")
    srs_amd.debug_set_topk_ragged_route(tl.KERNELS)
    with pytest.raises(srs_amd.SrsError) as e:
        srs_amd.topk_ragged_device(keys, offsets=offs, k=2049)
    assert "srs error -2" in str(e.value), str(e.value)


# ---------------------------------------------------------------------------
# other shapes
# ---------------------------------------------------------------------------
def test_non_default_stream(torch):
    ln, offs, num = _boundary_offsets()
    kind, cols = _column_set("f32_u32_u32", 0, num, 5)
    dcols = [tl.dev(torch, c) for c in cols]
    torch.cuda.synchronize()
    for k in (40, 3000):
        tl.run(torch, srs_amd, kind, True, cols, offs, k, True, dcols=dcols,
               stream=torch.cuda.Stream(), what="stream")


def test_new_tensors_are_zero_filled(torch):
    """without out=: zeros (indices: -1) in the slots that are not written"""
    offs = np.array([0, 3, 3, 10], dtype=np.int64)
    keys = np.arange(10, 0, -1).astype(np.uint32)
    pay = np.arange(10).astype(np.uint16) + 100
    doffs = torch.from_numpy(offs).cuda()
    ko, po, idx, counts = srs_amd.topk_ragged_device(tl.dev(torch, keys), tl.dev(torch, pay),
                                                     offsets=doffs, k=5, key_kind=U32,
                                                     indices=True)
    assert tuple(ko.shape) == tuple(po.shape) == tuple(idx.shape) == (3, 5)
    assert ko.cpu().tolist() == [[8, 9, 10, 0, 0], [0] * 5, [1, 2, 3, 4, 5]]
    assert po.cpu().tolist() == [[102, 101, 100, 0, 0], [0] * 5, [109, 108, 107, 106, 105]]
    assert idx.cpu().tolist() == [[2, 1, 0, -1, -1], [-1] * 5, [6, 5, 4, 3, 2]]
    assert counts.cpu().tolist() == [3, 0, 5]


@pytest.mark.parametrize("k", [9000, 30000])
def test_k_larger_than_every_length(torch, k):
    """every segment comes out sorted whole, as sort_ragged_device gives it"""
    ln = np.array([5, 0, 300, 8193, 1], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    kind, cols = _column_set("f32_u32_u32", 0, int(offs[-1]), 6)
    got = tl.run(torch, srs_amd, kind, False, cols, offs, k, True, what="k > every length")
    assert got[-1].tolist() == ln.tolist()


def test_all_segments_empty(torch):
    kind, cols = _column_set("u64_u64", 0, 5000, 3)
    for k in (4, 3000):
        for offs in (np.full(100, 777, np.int64), np.zeros(2, np.int64),
                     np.full(7, 5000, np.int64)):
            got = tl.run(torch, srs_amd, kind, True, cols, offs, k, True, what="all empty")
            assert not got[-1].any()
            assert srs_amd.debug_last_topk_ragged()[1:4] == (0, 0, 0)


@pytest.mark.parametrize("n", [200, 4096, 70001])
def test_one_segment_covering_everything(torch, n):
    kind, cols = _column_set("u8_u8_u16", 0, n, n)
    offs = np.array([0, n], dtype=np.int64)
    for k in (1, 33, 2500):
        tl.run(torch, srs_amd, kind, True, cols, offs, k, True, what="one segment")
    dcols = [tl.dev(torch, c) for c in cols]
    got = tl.run(torch, srs_amd, kind, True, cols, offs, 33, False, dcols=dcols, what="one")
    res = srs_amd.topk_device(*dcols, k=33, up=True, key_kind=kind)
    for q, r in enumerate(res):
        w = cols[q].dtype.itemsize
        assert np.array_equal(got[q][:min(33, n) * w], tl.to_bytes(r)), "differs from topk_device"


def test_back_to_back_calls_on_one_workspace(torch):
    """the second call has fewer long segments: the first call's list entries
    and counters must not be read"""
    rng = np.random.default_rng(11)
    ln1 = rng.integers(200, 700, 300)
    offs1 = np.concatenate([[0], np.cumsum(ln1)]).astype(np.int64)
    n = int(offs1[-1])
    kind, cols = _column_set("u64_u64", 0, n, 12)
    tl.run(torch, srs_amd, kind, True, cols, offs1, 10, False, what="first")
    assert srs_amd.debug_last_topk_ragged()[1:3] == tl.class_counts(ln1)
    offs2 = np.array([0, 5000, 5100, n], dtype=np.int64)
    tl.run(torch, srs_amd, kind, True, cols, offs2, 10, False, what="second")
    assert srs_amd.debug_last_topk_ragged()[1:3] == (1, 2)
