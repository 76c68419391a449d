"""Seeded differential fuzz of the ragged sort (sort_ragged_device). The cases
come from tests/srs_ragged_fuzzlib.py (tests/test_ragged_plan.py shows what
they reach); every expected result is, per segment, the stable argsort of
srs_testlib.transformed_keys applied to every column, exact and unique, so
every comparison is byte equality.

A failing case runs alone as -k "test_ragged_case[37]"; the assertion message
carries the case's description (without its list of lengths).
"""
import numpy as np
import pytest

import srs_ragged_fuzzlib as rz

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
SENTINEL = 0x5A


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


@pytest.mark.parametrize("case", range(rz.N_CASES))
def test_ragged_case(torch, case):
    d = rz.make_case(case)
    a = rz.make_arrays(d)
    cols, offs = a["cols"], a["offsets"]
    what = str({k: v for k, v in d.items() if k != "lengths"}) + f" nseg={len(d['lengths'])}"
    src, idx, lo, hi = rz.ragged_orders(d["kind"], d["up"], cols[0], offs)
    dcols = [_dev(torch, c) for c in cols]
    doffs = torch.from_numpy(offs.copy()).cuda()
    out = tuple(torch.full((t.numel() * t.element_size(),), SENTINEL, dtype=torch.uint8,
                           device="cuda").view(t.dtype) for t in dcols)
    srs_amd.debug_set_sort_ragged_short_max(d["short_max"])
    res = srs_amd.sort_ragged_device(*dcols, offsets=doffs, up=d["up"], key_kind=d["kind"],
                                     indices=d["indices"], out=out)
    info = srs_amd.debug_last_sort_ragged()
    for c, (r, h) in enumerate(zip(res, cols)):
        w = h.dtype.itemsize
        g = _bytes(r)
        assert np.array_equal(g[lo * w:hi * w], np.ascontiguousarray(h[src]).view(np.uint8)), \
            f"column {c} differs: {what}"
        assert np.all(g[:lo * w] == SENTINEL) and np.all(g[hi * w:] == SENTINEL), \
            f"column {c} written outside the segments: {what}"
    if d["indices"]:
        assert np.array_equal(res[-1].cpu().numpy()[lo:hi], idx), f"indices differ: {what}"
    else:
        assert len(res) == len(cols), what
    for t, h in zip(dcols, cols):
        assert np.array_equal(_bytes(t), np.ascontiguousarray(h).view(np.uint8)), \
            f"input written: {what}"
    assert np.array_equal(doffs.cpu().numpy(), offs), f"offsets written: {what}"
    sm = rz.SHORT_MAX if d["short_max"] < 0 else d["short_max"]
    want = rz.class_counts(d["lengths"], sm, d["indices"])
    assert info[:4] == want, f"{info} != {want}: {what}"
    assert info[4] == 1 if want[3] == 0 else info[4] >= 3, f"{info}: {what}"
