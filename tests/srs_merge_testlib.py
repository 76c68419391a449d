"""Helpers of the merge tests: the expected result on the CPU and one raw
srs_merge_soa_device call on guarded device buffers, checked in full.

TEST INFRASTRUCTURE. The expected result comes from numpy alone: the stable
argsort of srs_testlib.transformed_keys of A followed by B (the unsigned image
of the key order, floats' bit transform and the direction included, so -0.0
comes before +0.0 and up=False needs no reversal). The outputs are the
concatenated columns at that order and source_out is the order itself. Every
comparison is byte equality.
"""
from __future__ import annotations

import ctypes

import numpy as np

from srs_search_testlib import sorted_table
from srs_testlib import KIND_DTYPES, key_size, transformed_keys
from srs_unique_testlib import FILL, GUARD, Guarded, random_keys, to_dev

LAUNCHES = 3  # the column descriptor, the split, the tiles

# payload sets of the tests: the widths of the columns
PAYLOAD_SETS = {"none": (), "one8": (8,), "two4": (4, 4), "mixed": (1, 2, 4, 8)}
UINT = {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}


def expected_order(kind, up, keys_a, keys_b):
    """the stable argsort of A followed by B: source_out"""
    u = transformed_keys(kind, up, np.concatenate([keys_a, keys_b]))
    return np.argsort(u, kind="stable").astype(np.int64)


def sorted_side(kind, up, keys):
    """`keys` as one sorted input of a merge"""
    return sorted_table(kind, up, keys)


def make_payloads(widths, n, rng, tag=0):
    """one random column per width; `tag` keeps A's and B's values apart"""
    return [rng.integers(0, 1 << (8 * w), size=n, dtype=np.uint64).astype(UINT[w]) ^ UINT[w](tag)
            for w in widths]


def random_sides(kind, up, na, nb, distinct, rng):
    """two sorted sides drawn from one pool of `distinct` values"""
    keys = random_keys(kind, na + nb, max(1, distinct), rng)
    return sorted_side(kind, up, keys[:na]), sorted_side(kind, up, keys[na:])


def run_merge(torch, srs_amd, kind, up, keys_a, keys_b, pays_a=(), pays_b=(), *, source=True,
              stream=None, skew_elems=0, order=None, check_results=True):
    """One srs_merge_soa_device call on guarded outputs, checked in full: the
    results (check_results False, for unsorted inputs: only that every
    source_out value lies in [0, n)), the guards on both sides of every
    output, the inputs unwritten, srs_debug_last_merge. An empty side passes
    NULL pointers. Returns the output columns' bytes (keys, payloads, source)."""
    lib = srs_amd.lib()
    na, nb = len(keys_a), len(keys_b)
    n = na + nb
    ks = key_size(kind)
    assert len(pays_a) == len(pays_b)
    widths = [p.dtype.itemsize for p in pays_a]
    np_ = len(widths)
    if order is None and check_results:
        order = expected_order(kind, up, keys_a, keys_b)
    cols_a = [keys_a] + list(pays_a)
    cols_b = [keys_b] + list(pays_b)
    d_a = [to_dev(torch, c, skew_elems) if na else None for c in cols_a]
    d_b = [to_dev(torch, c, skew_elems) if nb else None for c in cols_b]
    g_out = [Guarded(torch, n, w, skew_elems * w) for w in [ks] + widths]
    g_src = Guarded(torch, n, 8) if source else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # (the copies above)
    sp = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream

    def ptrs(ts):
        return (ctypes.c_void_p * max(1, np_))(*[t.data_ptr() for t in ts[1:]])

    rc = lib.srs_merge_soa_device(
        na, nb, kind, int(up), d_a[0].data_ptr() if na else None,
        d_b[0].data_ptr() if nb else None, np_, ptrs(d_a) if np_ and na else None,
        ptrs(d_b) if np_ and nb else None,
        (ctypes.c_uint32 * max(1, np_))(*widths) if np_ else None, g_out[0].ptr,
        (ctypes.c_void_p * max(1, np_))(*[g.ptr for g in g_out[1:]]) if np_ else None,
        g_src.ptr if g_src else None, sp)
    assert rc == 0, lib.srs_last_error()
    if n > 0:
        info = srs_amd.debug_last_merge()
        tiles = (n + srs_amd.MERGE_TILE - 1) // srs_amd.MERGE_TILE
        assert info[:3] == (LAUNCHES, 0, tiles), info
        assert info[3] >= 8 * (tiles + 1), info
    torch.cuda.synchronize()
    got = []
    for c, g in enumerate(g_out):
        if check_results:
            cat = np.concatenate([cols_a[c], cols_b[c]])
            g.check(n, cat[order], f"output column {c}")
        else:
            g.check(0, np.zeros(0, np.uint8), f"output column {c}") if n == 0 else \
                _guards_only(g, f"output column {c}")
        got.append(g.host().tobytes())
    if g_src:
        if check_results:
            g_src.check(n, order, "source_out")
        else:
            _guards_only(g_src, "source_out")
            lo = GUARD + g_src.skew
            s = g_src.host()[lo:lo + 8 * n].view(np.int64)
            assert np.all((s >= 0) & (s < n)), "source_out outside [0, num_a + num_b)"
        got.append(g_src.host().tobytes())
    for ts, hs in ((d_a, cols_a), (d_b, cols_b)):
        for t, h in zip(ts, hs):
            if t is not None:
                assert np.array_equal(
                    t.cpu().numpy(), np.ascontiguousarray(h).view(np.uint8).reshape(-1)), \
                    "input written"
    return got


def _guards_only(g, what):
    h = g.host()
    lo = GUARD + g.skew
    assert np.all(h[:lo] == FILL), f"{what}: written below its start"
    assert np.all(h[lo + g.nbytes:] == FILL), f"{what}: written past its end"
