"""Ragged sort on the GPU (srs_sort_ragged_soa_device through
srs_amd.sort_ragged_device).

The expected result is, per segment, the stable argsort of
srs_testlib.transformed_keys(kind, up, segment) applied to every column
(srs_ragged_fuzzlib.ragged_orders): exact and unique, so columns are compared
as bytes and indices exactly. Segment lengths sit around the sizes at which a
segment changes its kernel: 64 / 256 (the wave's slab and the short kernel's
maximum), 4096 (the small and the large local class), 8192 (the LDS capacity,
past which the global levels run), and lengths of more than one tile.
"""
import numpy as np
import pytest

import srs_ragged_fuzzlib as rz
from srs_testlib import KIND_DTYPES

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

U8, U32, U64, F32, F64 = 0, 4, 6, 8, 9
SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
SENTINEL = 0x5A
CANARY = 0xC3
SLACK = 4096
BOUNDARY = [0, 1, 2, 3, 63, 64, 65, 127, 128, 129, 255, 256, 257, 1000, 4095, 4096, 4097, 8191,
            8192, 8193, 3 * 4096 + 17, 20001]
HEAD, TAIL = 37, 53


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


@pytest.fixture(autouse=True)
def _default_short_max():
    yield
    srs_amd.debug_set_sort_ragged_short_max(-1)


def _dev(torch, a):
    """a host array as a device tensor of the signed type of its size"""
    return torch.from_numpy(np.ascontiguousarray(a).view(SINT[a.dtype.itemsize]).copy()).cuda()


def _bytes(t):
    return t.cpu().numpy().view(np.uint8)


def _sentinel_like(torch, t):
    return torch.full((t.numel() * t.element_size(),), SENTINEL, dtype=torch.uint8,
                      device="cuda").view(t.dtype)


def _boundary_offsets():
    rng = np.random.default_rng(20261)
    ln = np.array(BOUNDARY + [0, 0], dtype=np.int64)
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
    if name == "u64_u64":  # the direct kernel's shape (without indices)
        return U64, [_keys(U64, n, rng), np.arange(n, dtype=np.uint64)]
    if name == "f32_u32_u32":
        return F32, [_keys(F32, n, rng), np.arange(n, dtype=np.uint32),
                     rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32)]
    if name == "u8_u8_u16":
        return U8, [_keys(U8, n, rng), rng.integers(0, 256, n, dtype=np.uint64).astype(np.uint8),
                    np.arange(n, dtype=np.uint64).astype(np.uint16)]
    raise ValueError(name)


def _run(torch, kind, up, cols, offs, indices, dcols=None, doffs=None, out=None, stream=None,
         what=""):
    """One sort_ragged_device call on host columns `cols` (keys first) into
    sentinel-filled outputs, compared with the expectation; the uncovered head
    and tail must keep the sentinel, the inputs and offsets their bytes.
    Returns the outputs' bytes (+ indices)."""
    src, idx, lo, hi = rz.ragged_orders(kind, up, cols[0], offs)
    if dcols is None:
        dcols = [_dev(torch, c) for c in cols]
    if doffs is None:
        doffs = torch.from_numpy(np.asarray(offs, dtype=np.int64).copy()).cuda()
    if out is None:
        out = tuple(_sentinel_like(torch, d) for d in dcols)
    res = srs_amd.sort_ragged_device(*dcols, offsets=doffs, up=up, key_kind=kind, indices=indices,
                                     out=out, stream=stream)
    if stream is not None:
        stream.synchronize()
    assert len(res) == len(cols) + (1 if indices else 0)
    got = []
    for c, (r, h) in enumerate(zip(res, cols)):
        assert r is out[c]
        w = h.dtype.itemsize
        g = _bytes(r)
        assert np.array_equal(g[lo * w:hi * w], np.ascontiguousarray(h[src]).view(np.uint8)), \
            f"{what}: column {c} differs (kind={kind}, up={up}, indices={indices})"
        assert np.all(g[:lo * w] == SENTINEL) and np.all(g[hi * w:] == SENTINEL), \
            f"{what}: column {c} written outside the segments"
        got.append(g)
    if indices:
        g = res[-1].cpu().numpy()
        assert np.array_equal(g[lo:hi], idx), f"{what}: indices differ (kind={kind}, up={up})"
        got.append(g[lo:hi])
    for d, h in zip(dcols, cols):
        assert np.array_equal(_bytes(d), np.ascontiguousarray(h).view(np.uint8)), "input written"
    assert np.array_equal(doffs.cpu().numpy(), np.asarray(offs, dtype=np.int64)), "offsets written"
    return got


# ---------------------------------------------------------------------------
# the boundary mix
# ---------------------------------------------------------------------------
def _boundary_check(torch, name, kind, up, indices):
    ln, offs, num = _boundary_offsets()
    assert num == HEAD + sum(BOUNDARY) + TAIL == 71610
    kind, cols = _column_set(name, kind, num, 1000 + 17 * kind + (1 if up else 0))
    got = _run(torch, kind, up, cols, offs, indices, what=name)
    info = srs_amd.debug_last_sort_ragged()
    assert info[:4] == rz.class_counts(ln), info
    assert info[4] >= 1, info
    assert info[5] == (1 if indices else 0), info
    return got


@pytest.mark.parametrize("indices", [False, True])
@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("kind", range(10))
def test_boundary_mix_keys_only(torch, kind, up, indices):
    _boundary_check(torch, "keys", kind, up, indices)


@pytest.mark.parametrize("indices", [False, True])
@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("name", ["u64_u64", "f32_u32_u32", "u8_u8_u16"])
def test_boundary_mix_column_sets(torch, name, up, indices):
    _boundary_check(torch, name, 0, up, indices)


@pytest.mark.parametrize("indices", [False, True])
@pytest.mark.parametrize("name", ["u64_u64", "f32_u32_u32"])
def test_routes_agree(torch, name, indices):
    """short_max 256 (default), 64, 1 and 0 (the short kernel off): byte-equal"""
    ln, offs, num = _boundary_offsets()
    kind, cols = _column_set(name, 0, num, 77)
    first = None
    for sm in (-1, 64, 1, 0):
        srs_amd.debug_set_sort_ragged_short_max(sm)
        got = _run(torch, kind, True, cols, offs, indices, what=f"{name} short_max={sm}")
        info = srs_amd.debug_last_sort_ragged()
        assert info[:4] == rz.class_counts(ln, 256 if sm < 0 else sm, indices), (sm, info)
        if first is None:
            first = got
        for a, b in zip(first, got):
            assert np.array_equal(a, b), f"short_max {sm} disagrees with the default"


# ---------------------------------------------------------------------------
# many tiny segments: two key values, so stability decides the order
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("nseg,top", [(40000, 8), (3000, 300)])
@pytest.mark.parametrize("up", [True, False])
def test_many_tiny_segments(torch, nseg, top, up):
    rng = np.random.default_rng(nseg + top)
    ln = rng.integers(0, top + 1, nseg)
    offs = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    n = int(offs[-1])
    keys = np.where(rng.random(n) < 0.5, np.uint32(7), np.uint32(0x80000007)).astype(np.uint32)
    cols = [keys, np.arange(n, dtype=np.uint32)]
    _run(torch, U32, up, cols, offs, True, what="tiny")
    info = srs_amd.debug_last_sort_ragged()
    assert info[:4] == rz.class_counts(ln), info
    assert info[4] == 1 + 2 * 0, info  # nothing over 8192: the one read-back


# ---------------------------------------------------------------------------
# floats: the total order at every length
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("kind", [F32, F64])
def test_float_total_order(torch, kind, up):
    dt = np.dtype(KIND_DTYPES[kind])
    fi = np.finfo(dt)
    table = np.array([0.0, np.inf, fi.smallest_subnormal,
                      np.nextafter(dt.type(fi.tiny), dt.type(0)), fi.tiny, 1.5, fi.max], dtype=dt)
    table = np.concatenate([table, -table])
    ln = np.array([2, 64, 256, 257, 9000], dtype=np.int64)
    offs = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
    n = int(offs[-1])
    rng = np.random.default_rng(kind)
    keys = table[rng.integers(0, len(table), n)]
    keys[0:2] = [0.0, -0.0] if up else [-0.0, 0.0]  # the pair of zeros must swap
    cols = [keys, np.arange(n, dtype=np.uint32)]
    got = _run(torch, kind, up, cols, offs, True, what="floats")
    ut = np.dtype("u%d" % dt.itemsize)
    zeros = got[0][:2 * dt.itemsize].view(ut)
    sign = 1 << (8 * dt.itemsize - 1)
    assert zeros.tolist() == ([sign, 0] if up else [0, sign])  # -0.0 before +0.0 ascending


# ---------------------------------------------------------------------------
# degenerate shapes
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [256, 8192, 70001])
def test_one_segment_is_the_plain_sort(torch, n):
    kind, cols = _column_set("f32_u32_u32", 0, n, n)
    offs = np.array([0, n], dtype=np.int64)
    got = _run(torch, kind, True, cols, offs, False, what="one segment")
    dcols = [_dev(torch, c) for c in cols]
    out = tuple(torch.empty_like(d) for d in dcols)
    srs_amd.sort_device(*dcols, key_kind=kind, cmp_sort_threshold=0, out=out)
    for a, o in zip(got, out):
        assert np.array_equal(a, _bytes(o)), "differs from sort_device"


def test_all_segments_empty(torch):
    kind, cols = _column_set("u64_u64", 0, 5000, 3)
    for offs in (np.full(100, 777, np.int64), np.zeros(2, np.int64), np.full(7, 5000, np.int64)):
        _run(torch, kind, True, cols, offs, True, what="all empty")
        assert srs_amd.debug_last_sort_ragged() == (0, 0, 0, 0, 1, 0)


@pytest.mark.parametrize("rows,n", [(513, 200), (5, 9000)])
@pytest.mark.parametrize("indices", [False, True])
def test_uniform_offsets_equal_sort_rows(torch, rows, n, indices):
    kind, cols = _column_set("u64_u64", 0, rows * n, rows)
    offs = (np.arange(rows + 1, dtype=np.int64) * n)
    got = _run(torch, kind, False, cols, offs, indices, what="uniform")
    d2 = [_dev(torch, c.reshape(rows, n)) for c in cols]
    res = srs_amd.sort_rows_device(*d2, up=False, key_kind=kind, indices=indices)
    for a, r in zip(got, res[:len(cols)]):
        assert np.array_equal(a, _bytes(r).ravel()), "differs from sort_rows_device"
    if indices:
        assert np.array_equal(got[-1], res[-1].cpu().numpy().ravel())


# ---------------------------------------------------------------------------
# streams and the workspace
# ---------------------------------------------------------------------------
def test_non_default_stream(torch):
    ln, offs, num = _boundary_offsets()
    kind, cols = _column_set("f32_u32_u32", 0, num, 5)
    dcols = [_dev(torch, c) for c in cols]
    out = tuple(_sentinel_like(torch, d) for d in dcols)
    torch.cuda.synchronize()
    _run(torch, kind, True, cols, offs, True, dcols=dcols, out=out, stream=torch.cuda.Stream(),
         what="stream")


def test_back_to_back_calls_on_one_workspace(torch):
    """the second call has fewer, longer segments: the first call's list
    entries and counters must not be read"""
    rng = np.random.default_rng(11)
    ln1 = rng.integers(200, 700, 300)
    offs1 = np.concatenate([[0], np.cumsum(ln1)]).astype(np.int64)
    n = int(offs1[-1])
    kind, cols = _column_set("u64_u64", 0, n, 12)
    _run(torch, kind, True, cols, offs1, False, what="first")
    first = srs_amd.debug_last_sort_ragged()
    offs2 = np.array([0, 5000, 5000 + 9000, n], dtype=np.int64)
    _run(torch, kind, True, cols, offs2, False, what="second")
    second = srs_amd.debug_last_sort_ragged()
    assert first[:4] == rz.class_counts(ln1) and first[1] > 3
    assert second[:4] == rz.class_counts(np.diff(offs2)), second


# ---------------------------------------------------------------------------
# bad offsets: an error code, never an access outside the columns
# ---------------------------------------------------------------------------
def _guarded(torch, host, fill=None):
    """(allocation, view): the column as a view with SLACK canary records on
    both sides"""
    n, w = len(host), host.dtype.itemsize
    big = torch.full(((n + 2 * SLACK) * w,), CANARY, dtype=torch.uint8, device="cuda")
    tint = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[w]
    view = big.view(tint)[SLACK:SLACK + n]
    if fill is None:
        view.copy_(torch.from_numpy(np.ascontiguousarray(host).view(SINT[w]).copy()))
    else:
        big[SLACK * w:(SLACK + n) * w] = fill
    return big, view


def _canaries_intact(big, n, w):
    g = big.cpu().numpy()
    return bool(np.all(g[:SLACK * w] == CANARY) and np.all(g[(SLACK + n) * w:] == CANARY))


@pytest.mark.parametrize("which", ["decreasing", "negative", "past_the_end"])
@pytest.mark.parametrize("indices", [False, True])
def test_bad_offsets_return_an_error(torch, which, indices):
    n = 200
    offs = {"decreasing": [0, 100, 50, 200], "negative": [-5, 100, 200],
            "past_the_end": [0, 100, n + 64]}[which]
    kind, cols = _column_set("u64_u64", 0, n, 21)
    ins = [_guarded(torch, c) for c in cols]
    outs = [_guarded(torch, c, fill=SENTINEL) for c in cols]
    doffs = torch.tensor(offs, dtype=torch.int64, device="cuda")
    with pytest.raises(srs_amd.SrsError) as e:
        srs_amd.sort_ragged_device(*[v for _, v in ins], offsets=doffs, key_kind=kind,
                                   indices=indices, out=tuple(v for _, v in outs))
    torch.cuda.synchronize()
    assert "srs error -1" in str(e.value) and "1 segment" in str(e.value), str(e.value)
    for (big, _), c in zip(ins + outs, cols + cols):
        assert _canaries_intact(big, n, c.dtype.itemsize), "written outside a column"
    for (_, v), c in zip(ins, cols):
        assert np.array_equal(_bytes(v), c.view(np.uint8)), "input written"
    assert doffs.cpu().tolist() == offs
    # the next valid call on the same workspace is correct
    good = np.array([0, 100, 150, 200], dtype=np.int64)
    _run(torch, kind, True, cols, good, indices, dcols=[v for _, v in ins], what="after the error")
    for (big, _), c in zip(ins, cols):
        assert _canaries_intact(big, n, c.dtype.itemsize)


def test_offsets_must_be_an_int64_device_tensor(torch):
    k = torch.zeros(10, dtype=torch.int64, device="cuda")
    with pytest.raises(TypeError):
        srs_amd.sort_ragged_device(k, offsets=[0, 10])
    with pytest.raises(TypeError):
        srs_amd.sort_ragged_device(k, offsets=torch.tensor([0, 10], dtype=torch.int64))
    with pytest.raises(TypeError):
        srs_amd.sort_ragged_device(k, offsets=torch.tensor([0, 10], dtype=torch.int32,
                                                           device="cuda"))
