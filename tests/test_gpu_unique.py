"""GPU tests of unique (srs_unique_soa_device, srs_amd.unique_device): the
smallest shapes at which the run-boundary logic can go wrong. Every case goes
through srs_unique_testlib.run_unique: outputs between guard words with a fill
pattern, compared byte for byte with numpy.unique of the transformed keys and
their stable argsort; slots from U (U + 1 of the offsets) on keep the fill.
"""
import ctypes
import itertools

import numpy as np
import pytest

import srs_unique_testlib as ul
from srs_testlib import KIND_DTYPES, KIND_NAMES, stable_reference

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

U64, U32, F32, F64 = 6, 4, 8, 9
TILE = 4096
SIZES = [1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8192, 8193, 3 * 4096 + 17,
         (1 << 20) + 1, 1_200_000]
PATTERNS = ["distinct", "equal", "alternating", "random1", "random7", "random300", "randomn"]


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


def _pattern(name, n, rng):
    if name == "distinct":
        return rng.permutation(n).astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)
    if name == "equal":
        return np.full(n, 0xDEADBEEF12345678, np.uint64)
    if name == "alternating":
        return np.where(np.arange(n) % 2 == 0, np.uint64(7), np.uint64(1 << 40))
    d = n if name == "randomn" else int(name[len("random"):])
    return ul.random_keys(U64, n, d, rng)


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("n", SIZES)
def test_sizes_and_patterns(torch, n, pattern):
    rng = np.random.default_rng(n * 31 + PATTERNS.index(pattern))
    keys = _pattern(pattern, n, rng)
    pay = rng.integers(0, 1 << 63, n, dtype=np.uint64)
    ul.run_unique(torch, srs_amd, U64, True, keys, [pay])


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("edge", [64, 256, 4096, 8192])
@pytest.mark.parametrize("kind", [U32, U64])
def test_boundary_at_an_edge(torch, kind, edge, delta):
    """two sorted runs whose boundary falls on, one before and one after a
    wave, slot and tile edge"""
    n = 3 * TILE + 17
    keys = np.where(np.arange(n) < edge + delta, 3, 11).astype(KIND_DTYPES[kind])
    for outputs in (ul.ALL_OUTPUTS, ("offsets",)):
        e, _ = ul.run_unique(torch, srs_amd, kind, True, keys, outputs=outputs)
        assert e["U"] == 2 and e["offsets"][1] == edge + delta


def test_boundaries_at_every_edge(torch):
    n = 3 * TILE + 17
    cuts = sorted({e + d for e in (64, 256, 4096, 8192) for d in (-1, 0, 1)})
    keys = np.searchsorted(np.array(cuts), np.arange(n), side="right").astype(np.uint16)
    e, _ = ul.run_unique(torch, srs_amd, 2, True, keys)
    assert list(e["offsets"][1:-1]) == cuts


@pytest.mark.parametrize("outputs", [ul.ALL_OUTPUTS, ("offsets",), ("sorted", "offsets", "nu_dev")])
def test_run_spanning_whole_tiles(torch, outputs):
    """one run over three whole tiles (tiles without a head, which the write
    kernel skips unless an inverse is asked for), distinct keys around it"""
    n = 5 * TILE + 100
    keys = np.arange(n, dtype=np.uint64)
    keys[TILE - 30:4 * TILE + 20] = TILE - 30
    rng = np.random.default_rng(5)
    for k in (keys, rng.permutation(keys)):
        e, _ = ul.run_unique(torch, srs_amd, U64, True, k, outputs=outputs)
        assert e["U"] == n - (3 * TILE + 50) + 1


@pytest.mark.parametrize("n", [2, 65, 4096, 4097, 8193, 2 * TILE + 1])
def test_head_as_last_record(torch, n):
    keys = np.full(n, 5, np.uint32)
    keys[-1] = 9
    for outputs in (ul.ALL_OUTPUTS, ("offsets", "nu_dev")):
        e, _ = ul.run_unique(torch, srs_amd, U32, True, keys, outputs=outputs)
        assert list(e["offsets"]) == [0, n - 1, n]


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("kind", range(10))
def test_all_kinds(torch, kind, up):
    n = 10_000
    rng = np.random.default_rng(100 + kind)
    if kind in (F32, F64):
        keys = ul.special_floats(kind, n, rng)
    else:
        keys = ul.random_keys(kind, n, 700, rng)
    pay = rng.integers(0, 256, n, dtype=np.uint8)
    e, _ = ul.run_unique(torch, srs_amd, kind, up, keys, [pay])
    if kind < 2:
        assert e["U"] <= 256
    if kind in (F32, F64):  # -0.0 and +0.0 are two keys
        z = e["unique"][e["unique"] == 0]
        assert len(z) == 2 and np.signbit(z[0]) != np.signbit(z[1])
    # the sorted columns and the indices are sort_device's with an arange payload
    dk = torch.from_numpy(keys.view(ul.SINT[keys.dtype.itemsize]).copy()).cuda()
    dp = torch.arange(n, dtype=torch.int64, device="cuda")
    srs_amd.sort_device(dk, dp, up=up, key_kind=kind, cmp_sort_threshold=0)
    assert np.array_equal(dp.cpu().numpy(), e["order"])
    assert np.array_equal(dk.cpu().numpy().view(np.uint8), keys[e["order"]].view(np.uint8))
    ref = stable_reference(kind, up, [keys, np.arange(n)], thresh=0)
    assert np.array_equal(ref[1], e["order"])


@pytest.mark.parametrize("mask", range(64))
def test_every_output_combination(torch, mask):
    n = 4097
    rng = np.random.default_rng(mask)
    keys = ul.random_keys(U64, n, 300, rng)
    outputs = tuple(o for i, o in enumerate(ul.ALL_OUTPUTS) if mask >> i & 1)
    pays = [rng.integers(0, 256, n, dtype=np.uint8),
            rng.integers(0, 1 << 63, n, dtype=np.uint64)] if "sorted" in outputs else []
    ul.run_unique(torch, srs_amd, U64, mask % 3 != 0, keys, pays, outputs=outputs)


def test_non_default_stream(torch):
    n = 3 * TILE + 17
    rng = np.random.default_rng(9)
    keys = ul.random_keys(U32, n, 64, rng)
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(s):
        ul.run_unique(torch, srs_amd, U32, True, keys, stream=s)
        ul.run_unique(torch, srs_amd, U32, False, keys, outputs=("offsets", "nu_dev"), stream=s)


@pytest.mark.parametrize("kind", [0, 2, U32, U64])
def test_unaligned_key_base(torch, kind):
    """the keys and the sorted key column element aligned but not 16-byte
    aligned: the tally takes its element-order loads, same result"""
    n = 2 * TILE + 5
    rng = np.random.default_rng(kind)
    keys = ul.random_keys(kind, n, 200, rng)
    e0, _ = ul.run_unique(torch, srs_amd, kind, True, keys)
    ul.run_unique(torch, srs_amd, kind, True, keys, skew_elems=1, exp=e0)
    ul.run_unique(torch, srs_amd, kind, True, keys, outputs=("sorted", "offsets"), skew_elems=1,
                  exp=e0)


def test_waits_and_routes(torch):
    n = 20_000
    rng = np.random.default_rng(3)
    keys = ul.random_keys(U64, n, 50, rng)
    # (run_unique asserts srs_debug_last_unique for its arguments: three
    # launches, 0 / 1 read-backs, the index column, the workspace columns)
    ul.run_unique(torch, srs_amd, U64, True, keys, outputs=("nu_dev",))
    assert srs_amd.debug_last_unique() == (3, 0, 0, 1)
    ul.run_unique(torch, srs_amd, U64, True, keys, outputs=("nu_host", "inverse"))
    assert srs_amd.debug_last_unique() == (3, 1, 1, 1)
    ul.run_unique(torch, srs_amd, U64, True, keys, outputs=("sorted", "indices"))
    assert srs_amd.debug_last_unique() == (3, 0, 1, 0)


def test_python_call(torch):
    n = 30_000
    rng = np.random.default_rng(11)
    keys = rng.integers(-40, 40, n).astype(np.int32)
    pay = rng.integers(0, 1 << 31, n).astype(np.int64)
    for up in (True, False):
        e = ul.expected(5, up, keys)
        r = srs_amd.unique_device(torch.from_numpy(keys).cuda(), torch.from_numpy(pay).cuda(),
                                  up=up, return_sorted=True, return_offsets=True,
                                  return_counts=True, return_index=True, return_inverse=True)
        assert isinstance(r, srs_amd.UniqueResult)
        assert np.array_equal(r.unique.cpu().numpy(), e["unique"])
        assert np.array_equal(r.sorted[0].cpu().numpy(), keys[e["order"]])
        assert np.array_equal(r.sorted[1].cpu().numpy(), pay[e["order"]])
        assert np.array_equal(r.offsets.cpu().numpy(), e["offsets"])
        assert np.array_equal(r.counts.cpu().numpy(), np.diff(e["offsets"]))
        assert np.array_equal(r.index.cpu().numpy(), e["first"])
        assert np.array_equal(r.inverse.cpu().numpy(), e["inverse"])
        assert r.inverse.shape == (n,)
        # numpy.unique itself for the integer kind (descending: groups reversed)
        uq, first, inv, cnt = np.unique(keys, return_index=True, return_inverse=True,
                                        return_counts=True)
        if not up:
            uq, first, cnt, inv = uq[::-1], first[::-1], cnt[::-1], len(uq) - 1 - inv
        assert np.array_equal(r.unique.cpu().numpy(), uq)
        assert np.array_equal(r.index.cpu().numpy(), first)
        assert np.array_equal(r.counts.cpu().numpy(), cnt)
        assert np.array_equal(r.inverse.cpu().numpy(), inv.reshape(-1))
    r = srs_amd.unique_device(torch.from_numpy(keys).cuda())
    assert r[1:] == (None,) * 5 and np.array_equal(r.unique.cpu().numpy(), np.unique(keys))
    with pytest.raises(ValueError):
        srs_amd.unique_device(torch.from_numpy(keys).cuda(), torch.from_numpy(pay).cuda())
    r = srs_amd.unique_device(torch.empty(0, dtype=torch.int32, device="cuda"),
                              return_offsets=True, return_counts=True, return_index=True,
                              return_inverse=True, return_sorted=True)
    assert r.unique.numel() == 0 and r.counts.numel() == 0 and r.index.numel() == 0
    assert r.inverse.numel() == 0 and r.sorted[0].numel() == 0 and r.offsets.tolist() == [0]


def test_offsets_feed_the_ragged_calls(torch):
    """(segment id, value) records grouped by unique, the groups' offsets fed
    unchanged into topk_ragged_device and sort_ragged_device"""
    n, groups, k = 50_000, 1700, 4
    rng = np.random.default_rng(17)
    seg = rng.integers(0, groups, n).astype(np.int32) * 3 - 2000
    val = rng.standard_normal(n).astype(np.float32)
    r = srs_amd.unique_device(torch.from_numpy(seg).cuda(), torch.from_numpy(val).cuda(),
                              return_sorted=True, return_offsets=True)
    ids, offs = r.unique.cpu().numpy(), r.offsets
    assert offs.numel() == len(ids) + 1 and 1600 < len(ids) <= groups
    seg_s, val_s = r.sorted
    tk = srs_amd.topk_ragged_device(val_s, seg_s, offsets=offs, k=k)
    sr = srs_amd.sort_ragged_device(val_s, seg_s, offsets=offs)
    tk_v, tk_s, tk_c = (t.cpu().numpy() for t in tk)
    sr_v, sr_s = (t.cpu().numpy() for t in sr)
    h = offs.cpu().numpy()
    for j, g in enumerate(ids):  # the CPU group-by
        want = np.sort(val[seg == g], kind="stable")
        assert np.array_equal(sr_v[h[j]:h[j + 1]], want)
        assert np.all(sr_s[h[j]:h[j + 1]] == g)
        c = min(k, len(want))
        assert tk_c[j] == c and np.array_equal(tk_v[j, :c], want[:c]) and np.all(tk_s[j, :c] == g)
