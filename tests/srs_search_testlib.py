"""Helpers of the search-sorted tests: the expected result on the CPU and one
raw srs_search_sorted_device call on guarded device buffers, checked in full.

TEST INFRASTRUCTURE. The expected result comes from numpy alone:
numpy.searchsorted of srs_testlib.transformed_keys of the table and of the
queries (the unsigned image of the key order, floats' bit transform and the
direction included, so -0.0 comes before +0.0 and up=False needs no
reversal). Every comparison is byte equality.
"""
from __future__ import annotations

import numpy as np

from srs_testlib import KIND_DTYPES, KIND_UINT, key_size, transformed_keys
from srs_unique_testlib import Guarded, to_dev

ALL_OUTPUTS = ("lower", "upper")
HINT = 1  # SRS_SEARCH_QUERIES_SORTED


def sorted_table(kind, up, keys):
    """`keys` in the order the library's sorts leave them"""
    return keys[np.argsort(transformed_keys(kind, up, keys), kind="stable")]


def expected(kind, up, table, queries):
    """(lower, upper) of the flat form"""
    t = transformed_keys(kind, up, table)
    q = transformed_keys(kind, up, queries)
    return (np.searchsorted(t, q, side="left").astype(np.int64),
            np.searchsorted(t, q, side="right").astype(np.int64))


def expected_segmented(kind, up, table, offsets, queries, qseg):
    """(lower, upper, bad count) of the segmented form: positions inside each
    query's segment, -1 for a query whose id or whose segment's offsets are bad"""
    n, nseg = len(table), len(offsets) - 1
    t = transformed_keys(kind, up, table)
    q = transformed_keys(kind, up, queries)
    lo = np.full(len(queries), -1, np.int64)
    hi = np.full(len(queries), -1, np.int64)
    bad = 0
    for s in np.unique(qseg):
        sel = np.nonzero(qseg == s)[0]
        if not 0 <= s < nseg or not 0 <= offsets[s] <= offsets[s + 1] <= n:
            bad += len(sel)
            continue
        seg = t[offsets[s]:offsets[s + 1]]
        lo[sel] = np.searchsorted(seg, q[sel], side="left")
        hi[sel] = np.searchsorted(seg, q[sel], side="right")
    return lo, hi, bad


def from_transformed(kind, up, u):
    """the keys whose transformed image is `u` (transformed_keys' inverse)"""
    nb = 8 * key_size(kind)
    mask = np.uint64((1 << nb) - 1)
    sb = np.uint64(1 << (nb - 1))
    u = u.astype(np.uint64) & mask
    if not up:
        u = ~u & mask
    dt = np.dtype(KIND_DTYPES[kind])
    if dt.kind == "i":
        bits = u ^ sb
    elif dt.kind == "f":
        bits = np.where((u & sb) != 0, u ^ sb, ~u & mask)
    else:
        bits = u
    return bits.astype(KIND_UINT[kind]).view(dt)


def has_nan(kind, keys):
    return np.dtype(KIND_DTYPES[kind]).kind == "f" and bool(np.isnan(keys).any())


def probe_queries(kind, up, table, extra=()):
    """Every table key, its neighbours one step below and above in
    transformed space, the type's smallest and largest value and `extra`,
    NaNs taken out (they are outside the contract)."""
    nb = 8 * key_size(kind)
    top = np.uint64((1 << nb) - 1)
    u = transformed_keys(kind, up, table)
    below = np.where(u > 0, u - np.uint64(1), u)
    above = np.where(u < top, u + np.uint64(1), u)
    ends = np.array([0, top], np.uint64)
    q = np.concatenate([table, from_transformed(kind, up, np.concatenate([below, above, ends])),
                        np.asarray(extra, dtype=KIND_DTYPES[kind])])
    if np.dtype(KIND_DTYPES[kind]).kind == "f":
        q = q[~np.isnan(q)]
    return q


def run_search(torch, srs_amd, kind, up, table, queries, *, outputs=ALL_OUTPUTS, route=0,
               flags=0, offsets=None, qseg=None, with_bad=True, stream=None, skew_elems=0,
               exp=None):
    """One srs_search_sorted_device call with the named outputs on the forced
    route (fewer than 2^20 queries), checked in full: results, guard bytes, inputs unwritten,
    srs_debug_last_search. Returns the raw bytes of the outputs given, in
    ALL_OUTPUTS order (for comparisons between calls)."""
    lib = srs_amd.lib()
    n, nq = len(table), len(queries)
    seg = offsets is not None
    if exp is None:
        exp = expected_segmented(kind, up, table, offsets, queries, qseg) if seg else \
            expected(kind, up, table, queries) + (0,)
    d_table = to_dev(torch, table, skew_elems) if n else None
    d_q = to_dev(torch, queries, skew_elems)
    d_offs = to_dev(torch, np.asarray(offsets, np.int64)) if seg else None
    d_qseg = to_dev(torch, np.asarray(qseg, np.int64)) if seg else None
    g = {name: Guarded(torch, nq, 8) for name in outputs}
    g_bad = Guarded(torch, 1, 8) if with_bad else None
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())  # (the copies above)
    sp = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    srs_amd.debug_set_search_route(route)
    try:
        rc = lib.srs_search_sorted_device(
            n, kind, int(up), d_table.data_ptr() if n else None, len(offsets) - 1 if seg else 0,
            d_offs.data_ptr() if seg else None, nq, d_q.data_ptr(),
            d_qseg.data_ptr() if seg else None, g["lower"].ptr if "lower" in g else None,
            g["upper"].ptr if "upper" in g else None, g_bad.ptr if g_bad else None, flags, sp)
    finally:
        srs_amd.debug_set_search_route(-1)
    assert rc == 0, lib.srs_last_error()
    info = srs_amd.debug_last_search()
    # (route -1: the library's rule, which sorts no query column of a test's size)
    took = 0 if seg or route < 0 else route
    assert info == (took, 1 + int(with_bad), -1 if took else 0, took), info
    torch.cuda.synchronize()
    got = []
    for name, want in zip(ALL_OUTPUTS, exp[:2]):
        if name in g:
            g[name].check(nq, want, f"{name}_out")
            got.append(g[name].host().tobytes())
    if g_bad:
        g_bad.check(1, np.array([exp[2]], np.int64), "num_bad_dev")
    ins = [(d_q, queries)] + ([(d_table, table)] if n else []) + \
        ([(d_offs, np.asarray(offsets, np.int64)), (d_qseg, np.asarray(qseg, np.int64))]
         if seg else [])
    for t, h in ins:
        assert np.array_equal(t.cpu().numpy(), np.ascontiguousarray(h).view(np.uint8).reshape(-1)), \
            "input written"
    return got
