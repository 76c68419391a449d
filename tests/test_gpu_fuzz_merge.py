"""Seeded differential fuzz of merge (srs_merge_soa_device). Every case draws
a key kind, a direction, the two sizes (either may be empty), the number of
distinct values (1, 2, about sqrt(n) or n), a payload set, the source column
on or off and a skew of the columns' bases, and goes through
srs_merge_testlib.run_merge: the stable argsort of the transformed keys of A
followed by B, byte equality, guard words, inputs unwritten.

A failing case runs alone as -k "test_merge_case[37]"; the assertion message
carries the case's description.
"""
import numpy as np
import pytest

import srs_merge_testlib as ml

srs_amd = pytest.importorskip("srs_amd")

N_CASES = 150
SEED0 = 1213
MAX_RECORDS = 300_000
T = 4096  # srs_c_api.h: SRS_MERGE_TILE (test_merge_capi.py holds the package to it)
TILE_EDGES = [T - 1, T, T + 1, 2 * T, 2 * T + 1]
LAWS = ("one", "two", "sqrt", "all")
PAYLOAD_SETS = tuple(ml.PAYLOAD_SETS)


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


def _size(rng):
    # most sides below 20 000 records, log-uniform; one in six up to MAX_RECORDS
    lo, hi = (20_000, MAX_RECORDS) if rng.integers(0, 6) == 0 else (1, 20_000)
    n = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
    if rng.integers(0, 8) == 0:  # on and around the tile
        n = int(rng.choice(TILE_EDGES))
    return n


def make_case(case: int) -> dict:
    """The description of fuzz case `case`: plain Python values only."""
    rng = np.random.default_rng(SEED0 + case)
    na, nb = _size(rng), _size(rng)
    empty = int(rng.integers(0, 12))  # one side empty in one case of six
    if empty == 0:
        na = 0
    elif empty == 1:
        nb = 0
    law = LAWS[int(rng.integers(0, 4))]
    n = na + nb
    distinct = {"one": 1, "two": 2, "sqrt": max(1, int(np.sqrt(n))), "all": n}[law]
    return dict(case=case, kind=int(rng.integers(0, 10)), up=bool(rng.integers(0, 2)), na=na,
                nb=nb, law=law, distinct=distinct,
                payloads=PAYLOAD_SETS[int(rng.integers(0, len(PAYLOAD_SETS)))],
                source=bool(rng.integers(0, 2)), skew=int(rng.choice([0, 0, 1, 3])))


def test_the_cases_reach_every_choice():
    assert T == srs_amd.MERGE_TILE
    ds = [make_case(c) for c in range(N_CASES)]
    assert {d["kind"] for d in ds} == set(range(10))
    assert {d["law"] for d in ds} == set(LAWS)
    assert {d["payloads"] for d in ds} == set(PAYLOAD_SETS)
    for name in ("up", "source"):
        assert {d[name] for d in ds} == {True, False}, name
    assert {d["skew"] for d in ds} == {0, 1, 3}
    assert any(d["na"] == 0 for d in ds) and any(d["nb"] == 0 for d in ds)
    assert all(d["na"] + d["nb"] >= 1 for d in ds)
    assert any(d["na"] in TILE_EDGES for d in ds) and any(d["nb"] in TILE_EDGES for d in ds)
    assert any(d["na"] > 100_000 or d["nb"] > 100_000 for d in ds)
    assert all(d["na"] <= MAX_RECORDS and d["nb"] <= MAX_RECORDS for d in ds)
    assert sum(d["na"] < 20_000 and d["nb"] < 20_000 for d in ds) > N_CASES // 2


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(N_CASES))
def test_merge_case(torch, case):
    d = make_case(case)
    rng = np.random.default_rng(SEED0 * 1000 + case)
    kind, up, na, nb = d["kind"], d["up"], d["na"], d["nb"]
    a, b = ml.random_sides(kind, up, na, nb, d["distinct"], rng)
    widths = ml.PAYLOAD_SETS[d["payloads"]]
    pa, pb = ml.make_payloads(widths, na, rng, 0), ml.make_payloads(widths, nb, rng, 1)
    try:
        ml.run_merge(torch, srs_amd, kind, up, a, b, pa, pb, source=d["source"],
                     skew_elems=d["skew"])
    except AssertionError as e:
        raise AssertionError(f"{e}: {d}") from None
