"""GPU parity tests for the tile-pair levels without the tile-offset pass
(DESIGN.md §4): the pair scatter sums every tile's bucket offsets from the
u16 count rows of its scan group, so such a level runs no tile_offs_kernel
and has no u32 offset rows. Every case runs with the mode on (the default)
and off (SRS_PAIR_ROW_OFFS=0: the offset rows), and both outputs must equal
the host's stable sort bit for bit; the payload is the record's index, so a
wrong offset or a lost stable order shows. srs_debug_level_counts proves
which path the levels took: without it a silent fall-back to the offset
rows would pass.

Shapes: sizes just above the one-launch range (plain pair levels, several
segments per level, pairs that straddle two segments, last scan groups of
fewer than 32 tiles), the stripe level and the gathered level behind it
(partly filled tiles, one GTile per tile), the other two shapes the pair
kernel takes (a 4-byte key with a 4-byte payload, 16-byte records of an
8-byte key), and a reverse-sorted and an all-equal column (skipped segments,
single-bucket levels).
"""
import numpy as np
import pytest

from srs_testlib import stable_reference
from test_gpu_sort import bytes_equal, make_keys, stable_aos

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

KNOB = "SRS_PAIR_ROW_OFFS"


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _torch()
    srs_amd.lib()


def _run(monkeypatch, on, sort):
    """One sort with the mode on or off; returns what it ran: (levels,
    tile-pair levels, of those without the tile-offset pass, scatter launches)."""
    torch = _torch()
    if on:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, "0")
    before = srs_amd.level_counts()
    srs_amd.reset_kernel_stats()
    srs_amd.set_kernel_timing(True)
    try:
        sort()
        torch.cuda.synchronize()
    finally:
        srs_amd.set_kernel_timing(False)
    after = srs_amd.level_counts()
    levels, pairs, rows = (a - b for a, b in zip(after, before))
    return levels, pairs, rows, srs_amd.kernel_stats("scatter")[0]


def _check_path(on, ran, want_pairs=True):
    levels, pairs, rows, scatters = ran
    print(f"mode {'on' if on else 'off'}: {levels} levels, {pairs} tile-pair, "
          f"{rows} without tile offsets, {scatters} scatter launches")
    assert scatters == levels
    if want_pairs:
        assert pairs > 0, "the tile-pair scatter did not run"
    # (every segment here is < 2^32 keys: each pair level takes the mode)
    assert rows == (pairs if on else 0)


def _soa_case(monkeypatch, kind, keys, pay_dtype, want_pairs=True):
    torch = _torch()
    n = len(keys)
    pay = np.arange(n, dtype=pay_dtype)
    want = stable_reference(kind, True, [keys, pay])
    dk = torch.from_numpy(np.ascontiguousarray(keys)).cuda()
    dp = torch.from_numpy(pay).cuda()
    for on in (True, False):
        ok, op = torch.zeros_like(dk), torch.zeros_like(dp)
        ran = _run(monkeypatch, on,
                   lambda: srs_amd.sort_device(dk, dp, key_kind=kind, out=(ok, op)))
        _check_path(on, ran, want_pairs)
        assert bytes_equal(ok.cpu().numpy(), want[0]), f"keys differ (mode {on})"
        assert bytes_equal(op.cpu().numpy(), want[1]), f"payloads differ (mode {on})"


@pytest.mark.parametrize("n", [4_200_003, 5_000_011])
@pytest.mark.parametrize("dist", ["uniform", "gaussian"])
def test_plain_pair_levels(monkeypatch, dist, n):
    """Just above the one-launch range: one segment, then several per level."""
    _soa_case(monkeypatch, 6, make_keys(6, dist, n, n + len(dist)), np.uint64)


def test_stripe_and_gathered_levels(monkeypatch):
    n = (1 << 25) + 1234
    _soa_case(monkeypatch, 6, make_keys(6, "uniform", n, 25), np.uint64)


def test_u32_key_u32_payload(monkeypatch):
    n = 5_000_011
    _soa_case(monkeypatch, 4, make_keys(4, "uniform", n, 4), np.uint32)


def test_records_of_16_bytes(monkeypatch):
    """An 8-byte key in a 16-byte record; the second 8 bytes hold the index."""
    n = 5_000_011
    keys = make_keys(6, "uniform", n, 16)
    elems = np.empty((n, 16), dtype=np.uint8)
    elems[:, :8] = keys.view(np.uint8).reshape(n, 8)
    elems[:, 8:] = np.arange(n, dtype=np.uint64).view(np.uint8).reshape(n, 8)
    want = stable_aos(6, True, elems)
    for on in (True, False):
        e = elems.copy()
        ran = _run(monkeypatch, on, lambda: srs_amd.sort_combined(e, 6))
        _check_path(on, ran)
        assert bytes_equal(e, want), f"records differ (mode {on})"


def test_reverse_sorted(monkeypatch):
    n = 5_000_011
    _soa_case(monkeypatch, 6, make_keys(6, "reverse", n, 7), np.uint64)


def test_all_equal(monkeypatch):
    """One value: whatever levels run, none may lose the order of the
    indices (a level is not required: equal keys may be copied through)."""
    n = 5_000_011
    keys = np.full(n, 0x0123_4567_89AB_CDEF, dtype=np.uint64)
    _soa_case(monkeypatch, 6, keys, np.uint64, want_pairs=False)
