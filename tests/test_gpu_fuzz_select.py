"""Seeded differential fuzz over the newer entry points: top-k (SoA and AoS),
row-wise top-k, row-wise sort and the segment sort. The cases come from
tests/srs_fuzzlib.py (tests/test_fuzz_plan.py shows what they reach); every
expected result is the stable argsort of srs_testlib.transformed_keys applied
to every column, exact and unique, so every comparison is byte equality.

A failing case runs alone as -k "test_topk_rows_case[137]"; the assertion
message carries the case's description.
"""
import numpy as np
import pytest

import srs_fuzzlib as fz
from srs_testlib import transformed_keys

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
TAIL = 64  # sentinel elements behind an out= tensor's result


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


@pytest.fixture(autouse=True)
def _restore_hooks():
    yield
    srs_amd.debug_set_topk_candidates(0)
    srs_amd.debug_set_topk_rows_route(-1)
    srs_amd.debug_set_sort_rows_route(-1)


def _dev(torch, a):
    """a host array as a device tensor of the signed type of its size"""
    return torch.from_numpy(np.ascontiguousarray(a).view(SINT[a.dtype.itemsize]).copy()).cuda()


def _bytes(t):
    return t.cpu().numpy().view(np.uint8)


def _same(t, a):
    """device tensor t holds the bytes of host array a"""
    return np.array_equal(_bytes(t).ravel(), np.ascontiguousarray(a).view(np.uint8).ravel())


def _m(*parts):
    """an assertion message: a string, so the case's description is printed whole"""
    return " ".join(str(p) for p in parts)


def _outs(torch, dflat, count, tail):
    """out= tensors of `count` elements per column with a sentinel tail, or None"""
    if not tail:
        return None
    return tuple(torch.full(((count + TAIL) * d.element_size(),), 0x5A, dtype=torch.uint8,
                            device="cuda").view(d.dtype) for d in dflat)


def _rows_setup(torch, d):
    """(host arrays, flat device allocations, strided (rows, row_len) views,
    the rows' host matrices, every row's stable order)"""
    a = fz.make_arrays(d)
    dflat = [_dev(torch, f) for f in a["flat"]]
    shape, strides = (d["rows"], d["row_len"]), (d["stride"], 1)
    views = [torch.as_strided(t, shape, strides, d["first"]) for t in dflat]
    cols = [f[a["index"]] for f in a["flat"]]
    orders = np.argsort(transformed_keys(d["kind"], d["up"], cols[0]), axis=1, kind="stable")
    return a, dflat, views, cols, orders


def _check_rows_result(d, res, out, cols, sel, what):
    """Every result column against the rows' order `sel`; returns the
    results' bytes."""
    rows, kk = sel.shape
    allgot = [_bytes(r).ravel() for r in res]
    for c, (r, h) in enumerate(zip(res, cols)):
        want = np.take_along_axis(h, sel, axis=1)
        got = allgot[c]
        nb = rows * kk * h.dtype.itemsize
        assert np.array_equal(got[:nb], want.view(np.uint8).ravel()), _m(what, "column", c, d)
        if out is not None:
            assert r is out[c] and np.all(got[nb:] == 0x5A), _m(what, "tail of column", c, d)
        else:
            assert tuple(r.shape) == (rows, kk), _m(what, d)
    if d["indices"]:
        assert np.array_equal(res[-1].cpu().numpy(), sel), _m(what, "indices", d)
    else:
        assert len(res) == len(cols), _m(what, d)
    return allgot


@pytest.mark.parametrize("case", range(fz.N_CASES["topk_rows"]))
def test_topk_rows_case(torch, case):
    assert fz.TOPK_ROWS_MAX_K == srs_amd.TOPK_ROWS_MAX_K
    d = fz.make_case("topk_rows", case)
    a, dflat, views, cols, orders = _rows_setup(torch, d)
    rows, n, k, kind, up = d["rows"], d["row_len"], d["k"], d["kind"], d["up"]
    kk = min(k, n)
    sel = orders[:, :kk]
    out = _outs(torch, dflat, rows * kk, d["out_tail"])
    srs_amd.debug_set_topk_rows_route(d["route"])
    res = srs_amd.topk_rows_device(*views, k=k, up=up, key_kind=kind, indices=d["indices"], out=out)
    info = srs_amd.debug_last_topk_rows()
    srs_amd.debug_set_topk_rows_route(-1)
    got = _check_rows_result(d, res, out, cols, sel, "topk_rows")
    assert info[0] == fz.topk_rows_route(d), _m(info, d)
    if info[0] in (fz.RESIDENT, fz.STREAM):
        assert info[1] == 1 and info[3] == 0, _m(info, d)  # one launch, nothing read back
    if fz.topk_rows_passes(d, a)["two"]:
        assert info[2] >= 2, _m(info, d)
    for r in d["sample_rows"]:  # the same row through the single-array top-k
        one = srs_amd.topk_device(*[v[r] for v in views], k=k, up=up, key_kind=kind,
                                  indices=d["indices"])
        for c, (x, y) in enumerate(zip(got, one)):
            nb = kk * y.element_size()
            assert np.array_equal(x[r * nb:(r + 1) * nb], _bytes(y).ravel()), \
                _m("topk_device on row", r, "column", c, d)
    for t, f in zip(dflat, a["flat"]):  # the whole allocation, padding included
        assert _same(t, f), _m("input written", d)


@pytest.mark.parametrize("case", range(fz.N_CASES["sort_rows"]))
def test_sort_rows_case(torch, case):
    d = fz.make_case("sort_rows", case)
    a, dflat, views, cols, orders = _rows_setup(torch, d)
    rows, n = d["rows"], d["row_len"]
    first = None
    for route in d["routes"]:
        out = _outs(torch, dflat, rows * n, d["out_tail"])
        srs_amd.debug_set_sort_rows_route(route)
        res = srs_amd.sort_rows_device(*views, up=d["up"], key_kind=d["kind"],
                                       indices=d["indices"], out=out)
        info = srs_amd.debug_last_sort_rows()
        srs_amd.debug_set_sort_rows_route(-1)
        got = _check_rows_result(d, res, out, cols, orders, ("sort_rows route", route))
        if route >= 0:
            assert info[0] == route, _m(info, route, d)
        if first is None:
            first = got
        for x, y in zip(first, got):
            assert np.array_equal(x, y), _m("the routes disagree", route, d)
    for t, f in zip(dflat, a["flat"]):
        assert _same(t, f), _m("input written", d)


@pytest.mark.parametrize("case", range(fz.N_CASES["topk"]))
def test_topk_case(torch, case):
    d = fz.make_case("topk", case)
    a = fz.make_arrays(d)
    n, k, kind, up = d["n"], d["k"], d["kind"], d["up"]
    kk = min(k, n)
    keys = a["keys"] if d["aos"] else a["cols"][0]
    order = np.argsort(transformed_keys(kind, up, keys), kind="stable")[:kk]
    srs_amd.debug_set_topk_candidates(d["candidates"])
    if d["aos"]:
        rec = torch.from_numpy(a["records"].copy()).cuda()
        res = srs_amd.topk_combined_device(rec, kind, k, up=up, indices=d["indices"])
        out, idx = res if d["indices"] else (res, None)
        srs_amd.debug_set_topk_candidates(0)
        assert tuple(out.shape) == (kk, d["elem_size"]), _m(d)
        assert np.array_equal(out.cpu().numpy(), a["records"][order]), _m("records", d)
        if idx is not None:
            assert np.array_equal(idx.cpu().numpy(), order), _m("indices", d)
        assert _same(rec, a["records"]), _m("input written", d)
        return
    dcols = [_dev(torch, c) for c in a["cols"]]
    res = srs_amd.topk_device(*dcols, k=k, up=up, key_kind=kind, indices=d["indices"])
    srs_amd.debug_set_topk_candidates(0)
    assert len(res) == len(dcols) + int(d["indices"]), _m(d)
    for c, (r, h) in enumerate(zip(res, a["cols"])):
        assert r.numel() == kk and _same(r, h[order]), _m("column", c, d)
    if d["indices"]:
        assert np.array_equal(res[-1].cpu().numpy(), order), _m("indices", d)
    for t, h in zip(dcols, a["cols"]):
        assert _same(t, h), _m("input written", d)


@pytest.mark.parametrize("case", range(fz.N_CASES["segments"]))
def test_segments_case(torch, case):
    d = fz.make_case("segments", case)
    cols = fz.make_arrays(d)["cols"]
    bounds = d["bounds"]
    u = transformed_keys(d["kind"], d["up"], cols[0])
    # one stable sort by (segment, key): the records outside every segment
    # (before the first bound, behind the last) stay where they are
    seg = np.searchsorted(np.asarray(bounds[1:-1], np.int64), np.arange(d["n"]), side="right")
    seg[:bounds[0]] = -1
    seg[bounds[-1]:] = len(bounds)
    u[:bounds[0]] = 0
    u[bounds[-1]:] = 0
    order = np.lexsort((u, seg))  # (stable: equal (segment, key) keep their order)
    assert np.array_equal(order[:bounds[0]], np.arange(bounds[0]))
    assert np.array_equal(order[bounds[-1]:], np.arange(bounds[-1], d["n"]))
    dcols = [_dev(torch, c) for c in cols]
    srs_amd.sort_segments_device(*dcols, bounds=bounds, up=d["up"], key_kind=d["kind"],
                                 known_top_bits=d["known_top_bits"])
    for c, (t, h) in enumerate(zip(dcols, cols)):
        assert _same(t, h[order]), _m("column", c, d)
