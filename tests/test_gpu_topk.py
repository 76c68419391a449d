"""Top-k on the GPU (srs_topk_soa_device / srs_topk_aos_device through
srs_amd.topk_device / topk_combined_device).

The expected result is always the stable argsort of
srs_testlib.transformed_keys(kind, up, keys) applied to every column and cut
at k: exact and unique, so every comparison is np.array_equal on bytes.
Sizes sit around the tile (4096), the one-launch sort's capacity (8192: up to
it a call sorts everything) and a size with many tiles; distributions put
rank k in a large boundary bucket, in a bucket of equal keys, and exactly on
a bucket's end.
"""
from functools import lru_cache

import numpy as np
import pytest

from srs_testlib import (KIND_DTYPES, KIND_NAMES, ref_lib, ref_sort_soa, transformed_keys)

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

U32, I32, U64, I64, F32, F64 = 4, 5, 6, 7, 8, 9
SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
NBIG = (1 << 20) + 1234
NMID = 3 * 4096 + 17


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


def _dev(torch, a):
    """a host column as a device tensor of the signed type of its size"""
    return torch.from_numpy(a.view(SINT[a.dtype.itemsize]).copy()).cuda()


def _host(t, like):
    return t.cpu().numpy().view(like.dtype)


def _order(kind, up, keys):
    return np.argsort(transformed_keys(kind, up, keys), kind="stable")


def _check(torch, kind, up, cols, k, order=None, indices=False, dcols=None, stream=None):
    """One topk_device call on host columns `cols` (keys first), compared with
    the stable order; the inputs must come back unchanged."""
    n = len(cols[0])
    if order is None:
        order = _order(kind, up, cols[0])
    own = dcols is None
    if own:
        dcols = [_dev(torch, c) for c in cols]
    res = srs_amd.topk_device(*dcols, k=k, up=up, key_kind=kind, indices=indices, stream=stream)
    torch.cuda.synchronize()
    kk = max(0, min(k, n))
    assert len(res) == len(cols) + (1 if indices else 0)
    for c, (r, h) in enumerate(zip(res, cols)):
        assert r.numel() == kk
        assert np.array_equal(_host(r, h).view(np.uint8), h[order[:kk]].view(np.uint8)), \
            f"column {c} differs (n={n}, k={k})"
    if indices:
        idx = res[-1].cpu().numpy()
        assert np.array_equal(idx, order[:kk]), f"indices differ (n={n}, k={k})"
    if own:
        for d, h in zip(dcols, cols):
            assert np.array_equal(_host(d, h).view(np.uint8), h.view(np.uint8)), "input written"


def _ks(n):
    return sorted({k for k in (1, 2, 63, 64, 65, n - 1, n, n + 5) if k >= 1})


def _shape_cols(shape, n, seed):
    rng = np.random.default_rng(seed)
    if shape == "u64_u64":
        return U64, [rng.integers(0, 1 << 64, n, dtype=np.uint64),
                     rng.integers(0, 1 << 64, n, dtype=np.uint64)]
    if shape == "f32_u32_u32":
        k = rng.standard_normal(n).astype(np.float32)
        k[rng.integers(0, n, max(1, n // 50))] = np.float32(-0.0)  # -0.0 before +0.0
        k[rng.integers(0, n, max(1, n // 50))] = np.float32(0.0)
        return F32, [k, rng.integers(0, 1 << 32, n, dtype=np.uint32),
                     np.arange(n, dtype=np.uint32)]
    return U32, [rng.integers(0, 1 << 10, n, dtype=np.uint32)]  # keys only, many ties


@pytest.mark.parametrize("n", [1, 2, 4095, 4096, 4097, 8193, NMID, NBIG])
@pytest.mark.parametrize("shape", ["u64_u64", "f32_u32_u32", "keys_only"])
def test_size_and_k_matrix(torch, shape, n):
    kind, cols = _shape_cols(shape, n, seed=n % 1000 + len(shape))
    order = _order(kind, True, cols[0])
    dcols = [_dev(torch, c) for c in cols]
    for k in _ks(n):
        _check(torch, kind, True, cols, k, order=order, dcols=dcols)
    for d, h in zip(dcols, cols):
        assert np.array_equal(_host(d, h).view(np.uint8), h.view(np.uint8)), "input written"
    _check(torch, kind, False, cols, min(n, 65))


@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
@pytest.mark.parametrize("kind", range(10), ids=KIND_NAMES)
def test_every_key_kind(torch, kind, up):
    """All ten key kinds; the 8- and 16-bit kinds are all ties at this size, and
    the indices of equal keys must still ascend (checked against the stable order)."""
    rng = np.random.default_rng(100 + kind)
    dt = np.dtype(KIND_DTYPES[kind])
    if dt.kind == "f":
        k = (rng.standard_normal(NMID) * 1e3).astype(dt)
        k[::97] = 0.0
        k[1::97] = -0.0
    else:
        ii = np.iinfo(dt)
        k = rng.integers(ii.min, int(ii.max) + 1, NMID, dtype=dt)
    p = rng.integers(0, 1 << 16, NMID, dtype=np.uint16)
    _check(torch, kind, up, [k, p], 1000, indices=True)


@lru_cache(maxsize=None)
def _dist(name):
    """(kind, keys) of a distribution at NBIG"""
    rng = np.random.default_rng(7)
    n = NBIG
    if name == "uniform":
        return U64, rng.integers(0, 1 << 64, n, dtype=np.uint64)
    if name == "all_equal":
        return U64, np.full(n, 0x0123456789ABCDEF, np.uint64)
    if name == "two_values":
        return I64, rng.integers(0, 2, n).astype(np.int64)
    if name == "shared_top":  # as tests/test_gpu_keyrange.py
        return U64, (np.uint64(0x123456789AB) << np.uint64(20)) + rng.integers(
            0, 1 << 20, n, dtype=np.uint64)
    if name == "gaussian":
        return I64, np.round(rng.normal(0.0, 100.0, n)).astype(np.int64)
    if name == "sorted":
        return U64, np.sort(rng.integers(0, 1 << 64, n, dtype=np.uint64))
    if name == "reverse":
        return U64, np.sort(rng.integers(0, 1 << 64, n, dtype=np.uint64))[::-1].copy()
    raise ValueError(name)


@lru_cache(maxsize=None)
def _dist_case(name):
    kind, k = _dist(name)
    p = np.arange(len(k), dtype=np.uint64) * np.uint64(3)
    return kind, k, p, _order(kind, True, k)


@pytest.mark.parametrize("k", [1, 1000, 300000])
@pytest.mark.parametrize("name", ["uniform", "all_equal", "two_values", "shared_top", "gaussian",
                                  "sorted", "reverse"])
def test_distributions(torch, name, k):
    kind, keys, p, order = _dist_case(name)
    _check(torch, kind, True, [keys, p], k, order=order, indices=(k == 1000))
    passes, nsorted, full = srs_amd.debug_last_topk()
    assert full == 0 and passes >= 1 and k <= nsorted < NBIG + 1
    if name == "all_equal":
        assert nsorted == k  # a bucket of equal keys: only its first records are taken


@pytest.mark.parametrize("k", [1, 100, 101, 150, 5000])
def test_sure_records_behind_the_candidate_limit(torch, k):
    """Nearly all keys equal, 100 smaller ones scattered up to the last tile:
    the boundary bucket is the run of equal keys, of which only the first
    k - 100 are taken (tiles behind them write nothing), while the smaller
    keys of those same late tiles must still arrive."""
    rng = np.random.default_rng(37)
    keys = np.full(NBIG, 5, np.uint64)
    pos = np.concatenate([rng.choice(NBIG - 10, 97, replace=False), [NBIG - 1, NBIG - 2, 4096]])
    keys[pos] = rng.integers(0, 5, len(pos), dtype=np.uint64)
    p = np.arange(NBIG, dtype=np.uint64) * np.uint64(7)
    _check(torch, U64, True, [keys, p], k, indices=True)
    passes, nsorted, full = srs_amd.debug_last_topk()
    assert full == 0 and nsorted >= k
    if k > 100:
        assert nsorted == k


BUCKET_END = 1000  # keys in the first 12-bit bucket of the boundary case


@lru_cache(maxsize=None)
def _bucket_end_case():
    rng = np.random.default_rng(11)
    n = NBIG
    keys = rng.integers(1 << 52, 1 << 64, n, dtype=np.uint64)  # top digit >= 1
    pos = rng.choice(n, BUCKET_END, replace=False)
    keys[pos] = rng.integers(0, 1 << 52, BUCKET_END, dtype=np.uint64)  # top digit 0
    p = np.arange(n, dtype=np.uint64)
    return keys, p, _order(U64, True, keys)


@pytest.mark.parametrize("k", [BUCKET_END - 1, BUCKET_END, BUCKET_END + 1])
def test_rank_on_a_bucket_end(torch, k):
    """Exactly BUCKET_END keys have the top digit 0. With refinement forced
    (one candidate allowed), k = BUCKET_END stops after one pass because the
    boundary bucket is wholly inside; one less or one more must refine."""
    keys, p, order = _bucket_end_case()
    srs_amd.debug_set_topk_candidates(1)
    try:
        _check(torch, U64, True, [keys, p], k, order=order)
        passes, nsorted, full = srs_amd.debug_last_topk()
    finally:
        srs_amd.debug_set_topk_candidates(0)
    assert full == 0
    if k == BUCKET_END:
        assert (passes, nsorted) == (1, k)
    else:
        assert passes >= 2 and nsorted >= k
    _check(torch, U64, True, [keys, p], k, order=order)  # and with the default stop rule


def _rank_needing_three_digits(kind, keys):
    """A rank k whose boundary key shares its top 24 transformed bits with the
    next key of the sorted order without being equal to it: two 12-bit digits
    leave both in the boundary bucket, so a select that may keep one candidate
    needs a third pass. (20000 random keys hold about a dozen such pairs.)"""
    u = np.sort(transformed_keys(kind, True, keys))
    top = u >> np.uint64(40)
    hit = np.flatnonzero((top[1:] == top[:-1]) & (u[1:] != u[:-1]))
    hit = hit[hit + 1 <= len(keys) // 2]  # (a rank the select takes: k <= n / 2)
    assert len(hit), "the input has no two keys that agree on their top 24 bits"
    i = int(hit[len(hit) // 2])
    assert i == 0 or top[i - 1] != top[i] or u[i - 1] != u[i]
    return i + 1


@pytest.mark.parametrize("kind", [U64, F64], ids=["u64", "f64"])
def test_forced_refinement(torch, kind):
    """n = 20000 with one candidate allowed: the select refines until the
    boundary bucket is one record. At a rank whose key shares 24 top bits with
    its successor that takes >= 3 passes; the result is exact at every rank."""
    n = 20000
    rng = np.random.default_rng(13)
    if kind == U64:
        keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    else:
        keys = rng.standard_normal(n)
    p = np.arange(n, dtype=np.uint32)
    k3 = _rank_needing_three_digits(kind, keys)
    srs_amd.debug_set_topk_candidates(1)
    try:
        for k in (k3, 1, 777, 9000):
            _check(torch, kind, True, [keys, p], k, indices=True)
            passes, nsorted, full = srs_amd.debug_last_topk()
            print(f"forced refinement kind={kind} k={k}: passes={passes} sorted={nsorted}")
            assert full == 0 and nsorted == k and passes >= 2, (k, passes, nsorted, full)
            if k == k3:
                assert passes >= 3, (k, passes)
        _check(torch, kind, False, [keys, p], 777)
    finally:
        srs_amd.debug_set_topk_candidates(0)


def test_path_selection(torch):
    """k > n / 2 sorts everything; k = n / 2 selects."""
    n = 20000
    rng = np.random.default_rng(17)
    keys = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    p = np.arange(n, dtype=np.uint64)
    _check(torch, U64, True, [keys, p], n // 2 + 1)
    assert srs_amd.debug_last_topk() == (0, n, 1)
    _check(torch, U64, True, [keys, p], n // 2)
    passes, nsorted, full = srs_amd.debug_last_topk()
    assert full == 0 and passes >= 1 and n // 2 <= nsorted < n
    _check(torch, U64, True, [keys, p], n // 2 + 1, indices=True)  # (indices: the gathered route)
    assert srs_amd.debug_last_topk() == (0, n, 1)
    _check(torch, U64, True, [keys, p], n)
    assert srs_amd.debug_last_topk() == (0, n, 1)


@pytest.mark.parametrize("npay", [0, 1, 63])
def test_indices(torch, npay):
    rng = np.random.default_rng(19 + npay)
    keys = rng.integers(0, 300, NMID, dtype=np.uint32)  # many ties
    pays = [rng.integers(0, 256, NMID, dtype=np.uint8) for _ in range(npay)]
    order = _order(U32, True, keys)
    for k in (1000, NMID - 1, NMID):
        dcols = [_dev(torch, c) for c in [keys] + pays]
        res = srs_amd.topk_device(*dcols, k=k, key_kind=U32, indices=True)
        torch.cuda.synchronize()
        idx = res[-1].cpu().numpy()
        ko = _host(res[0], keys)
        assert np.array_equal(keys[idx], ko)
        assert np.array_equal(idx, order[:k])
        same = ko[1:] == ko[:-1]
        assert np.all(idx[1:][same] > idx[:-1][same]), "indices of equal keys must ascend"
        for r, h in zip(res[1:-1], pays):
            assert np.array_equal(_host(r, h), h[idx])


@pytest.mark.parametrize("up", [True, False], ids=["up", "down"])
@pytest.mark.parametrize("kind", [U32, I64], ids=["u32", "i64"])
@pytest.mark.parametrize("esz", [8, 16, 64])
def test_aos(torch, esz, kind, up):
    rng = np.random.default_rng(23 + esz + kind)
    n = NMID
    rec = rng.integers(0, 256, (n, esz), dtype=np.uint8)
    ks = np.dtype(KIND_DTYPES[kind]).itemsize
    rec[:, 1:ks] &= 3  # (ties among the keys)
    keys = rec[:, :ks].copy().view(KIND_DTYPES[kind]).reshape(n)
    order = _order(kind, up, keys)
    rd = torch.from_numpy(rec.copy()).cuda()
    for k in (1, 1000, n // 2 + 1):
        out, idx = srs_amd.topk_combined_device(rd, kind, k, up=up, indices=True)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), rec[order[:k]]), (esz, kind, up, k)
        assert np.array_equal(idx.cpu().numpy(), order[:k])
    out = srs_amd.topk_combined_device(rd, kind, 1000, up=up)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), rec[order[:1000]])
    out = srs_amd.topk_combined_device(rd, kind, n + 5, up=up)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), rec[order])
    assert np.array_equal(rd.cpu().numpy(), rec), "input written"


def test_two_streams_back_to_back(torch):
    kind, keys, p, order = _dist_case("uniform")
    _, keys2, p2, order2 = _dist_case("gaussian")
    d1 = [_dev(torch, keys), _dev(torch, p)]
    d2 = [_dev(torch, keys2), _dev(torch, p2)]
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    torch.cuda.synchronize()
    r1 = srs_amd.topk_device(*d1, k=5000, key_kind=U64, stream=s1)
    r2 = srs_amd.topk_device(*d2, k=70000, key_kind=I64, stream=s2)
    r3 = srs_amd.topk_device(*d1, k=3, key_kind=U64, up=False, stream=s1)
    torch.cuda.synchronize()
    assert np.array_equal(_host(r1[0], keys), keys[order[:5000]])
    assert np.array_equal(_host(r1[1], p), p[order[:5000]])
    assert np.array_equal(_host(r2[0], keys2), keys2[order2[:70000]])
    assert np.array_equal(_host(r2[1], p2), p2[order2[:70000]])
    o3 = _order(U64, False, keys)[:3]
    assert np.array_equal(_host(r3[0], keys), keys[o3])
    assert np.array_equal(_host(r3[1], p), p[o3])


def test_sort_after_topk_reuses_the_workspace(torch):
    kind, keys, p, order = _dist_case("uniform")
    kd, pd = _dev(torch, keys), _dev(torch, p)
    srs_amd.topk_device(kd, pd, k=1000, key_kind=U64)
    ko, po = torch.empty_like(kd), torch.empty_like(pd)
    srs_amd.sort_device(kd, pd, key_kind=U64, out=(ko, po))
    r = srs_amd.topk_device(kd, pd, k=1000, key_kind=U64)
    srs_amd.sort_device(kd, pd, key_kind=U64)
    torch.cuda.synchronize()
    assert np.array_equal(_host(ko, keys), keys[order])
    assert np.array_equal(_host(po, p), p[order])
    assert np.array_equal(_host(kd, keys), keys[order])
    assert np.array_equal(_host(pd, p), p[order])
    assert np.array_equal(_host(r[0], keys), keys[order[:1000]])


def test_kernel_stats_report_the_select_kernels(torch):
    kind, keys, p, order = _dist_case("uniform")
    kd, pd = _dev(torch, keys), _dev(torch, p)
    srs_amd.set_kernel_timing(True)
    try:
        srs_amd.reset_kernel_stats()
        srs_amd.topk_device(kd, pd, k=1000, key_kind=U64)
        torch.cuda.synchronize()
        for name in ("select_hist", "select_tally", "select_gather"):
            launches, ms, _ = srs_amd.kernel_stats(name)
            assert launches >= 1 and ms > 0, name
    finally:
        srs_amd.set_kernel_timing(False)
        srs_amd.reset_kernel_stats()


def _f(bits):
    """payload = splitmix64(key bits), as tests/test_gpu_keyrange.py"""
    x = bits.astype(np.uint64) + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def test_topk_vs_reference(torch):
    """The first k records of the REFERENCE's own sort (oracle/_ref) of
    2^25 + 1234 u64 keys; payload = f(key), so its unstable order is unique."""
    if ref_lib() is None:
        pytest.fail("oracle/_ref/libsrs_ref.so missing or host lacks AVX-512 VBMI2")
    n, k = (1 << 25) + 1234, 100000
    keys = np.random.default_rng(29).integers(0, 1 << 64, n, dtype=np.uint64)
    p = _f(keys)
    kd, pd = _dev(torch, keys), _dev(torch, p)
    ko, po = srs_amd.topk_device(kd, pd, k=k, key_kind=U64)
    k_ref, p_ref = keys.copy(), p.copy()
    ref_sort_soa(U64, True, k_ref, [p_ref])
    torch.cuda.synchronize()
    assert np.array_equal(_host(ko, keys), k_ref[:k])
    assert np.array_equal(_host(po, p), p_ref[:k])
    assert srs_amd.debug_last_topk()[2] == 0
