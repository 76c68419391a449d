"""Seeded differential fuzz of unique (srs_unique_soa_device). Every case
draws a key kind, a direction, a size, the number of distinct values (1, 2,
about sqrt(n) or n), a payload set and a set of optional outputs, and goes
through srs_unique_testlib.run_unique: numpy.unique of the transformed keys
and their stable argsort, byte equality, guard words and untouched slots.

A failing case runs alone as -k "test_unique_case[37]"; the assertion message
carries the case's description.
"""
import numpy as np
import pytest

import srs_unique_testlib as ul
from srs_testlib import UINT_OF_SIZE

srs_amd = pytest.importorskip("srs_amd")

N_CASES = 150
SEED0 = 733
MAX_RECORDS = 300_000


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


def make_case(case: int) -> dict:
    """The description of fuzz case `case`: plain Python values only."""
    rng = np.random.default_rng(SEED0 + case)
    # most cases below 20 000 records, log-uniform; one in six up to MAX_RECORDS
    lo, hi = (20_000, MAX_RECORDS) if rng.integers(0, 6) == 0 else (1, 20_000)
    n = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
    if rng.integers(0, 8) == 0:  # on and around a tile edge
        n = int(rng.choice([4095, 4096, 4097, 8192, 8193]))
    law = ("one", "two", "sqrt", "all")[int(rng.integers(0, 4))]
    distinct = {"one": 1, "two": 2, "sqrt": max(1, int(np.sqrt(n))), "all": n}[law]
    outputs = tuple(o for o in ul.ALL_OUTPUTS if rng.integers(0, 2))
    widths = [int(rng.choice([1, 2, 4, 8])) for _ in range(int(rng.integers(0, 4)))] \
        if "sorted" in outputs else []
    return dict(case=case, kind=int(rng.integers(0, 10)), up=bool(rng.integers(0, 2)), n=n,
                law=law, distinct=distinct, outputs=outputs, widths=widths)


def test_the_cases_reach_every_choice():
    ds = [make_case(c) for c in range(N_CASES)]
    assert {d["kind"] for d in ds} == set(range(10))
    assert {d["law"] for d in ds} == {"one", "two", "sqrt", "all"}
    assert {d["up"] for d in ds} == {True, False}
    for o in ul.ALL_OUTPUTS:
        assert 0 < sum(o in d["outputs"] for d in ds) < N_CASES
    assert any(d["n"] > 100_000 for d in ds) and all(1 <= d["n"] <= MAX_RECORDS for d in ds)
    assert sum(d["n"] < 20_000 for d in ds) > N_CASES * 2 // 3


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(N_CASES))
def test_unique_case(torch, case):
    d = make_case(case)
    rng = np.random.default_rng(SEED0 * 1000 + case)
    keys = ul.random_keys(d["kind"], d["n"], d["distinct"], rng)
    pays = [rng.integers(0, 1 << (8 * w - 1), d["n"], dtype=np.uint64).astype(UINT_OF_SIZE[w])
            for w in d["widths"]]
    try:
        ul.run_unique(torch, srs_amd, d["kind"], d["up"], keys, pays, outputs=d["outputs"])
    except AssertionError as e:
        raise AssertionError(f"{e}: {d}") from None
