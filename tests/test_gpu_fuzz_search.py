"""Seeded differential fuzz of search-sorted (srs_search_sorted_device). Every
case draws a key kind, a direction, a table size, the number of distinct
values (1, 2, about sqrt(n) or n), a query count, a query law (keys of the
table and their neighbours, uniform over the type, either of them sorted), a
route, the hint, the outputs and the flat or the segmented form, and goes
through srs_search_testlib.run_search: numpy.searchsorted of the transformed
keys, byte equality, guard words, inputs unwritten.

A failing case runs alone as -k "test_search_case[37]"; the assertion message
carries the case's description.
"""
import numpy as np
import pytest

import srs_search_testlib as sl
import srs_unique_testlib as ul

srs_amd = pytest.importorskip("srs_amd")

N_CASES = 150
SEED0 = 911
MAX_RECORDS = 300_000
MAX_QUERIES = 20_000
TILE_EDGES = [1023, 1024, 1025, 2046, 2047, 2048, 2049, 4096, 4097]
LAWS = ("table", "uniform", "table_sorted", "uniform_sorted")
OUTPUT_SETS = (("lower",), ("upper",), ("lower", "upper"))


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
    # most tables below 20 000 keys, log-uniform; one in six up to MAX_RECORDS
    lo, hi = (20_000, MAX_RECORDS) if rng.integers(0, 6) == 0 else (1, 20_000)
    n = int(np.exp(rng.uniform(np.log(lo), np.log(hi))))
    if rng.integers(0, 8) == 0:  # on and around the query tile and the LDS sample
        n = int(rng.choice(TILE_EDGES))
    law = ("one", "two", "sqrt", "all")[int(rng.integers(0, 4))]
    distinct = {"one": 1, "two": 2, "sqrt": max(1, int(np.sqrt(n))), "all": n}[law]
    nq = int(np.exp(rng.uniform(0, np.log(MAX_QUERIES))))
    if rng.integers(0, 8) == 0:
        nq = int(rng.choice(TILE_EDGES))
    return dict(case=case, kind=int(rng.integers(0, 10)), up=bool(rng.integers(0, 2)), n=n,
                law=law, distinct=distinct, nq=nq, qlaw=LAWS[int(rng.integers(0, 4))],
                route=int(rng.integers(0, 2)), hint=bool(rng.integers(0, 2)),
                outputs=OUTPUT_SETS[int(rng.integers(0, 3))],
                segmented=bool(rng.integers(0, 3) == 0), nseg=int(rng.integers(1, 40)),
                with_bad=bool(rng.integers(0, 2)))


def test_the_cases_reach_every_choice():
    ds = [make_case(c) for c in range(N_CASES)]
    assert {d["kind"] for d in ds} == set(range(10))
    assert {d["law"] for d in ds} == {"one", "two", "sqrt", "all"}
    assert {d["qlaw"] for d in ds} == set(LAWS)
    assert {d["outputs"] for d in ds} == set(OUTPUT_SETS)
    for name in ("up", "hint", "segmented", "with_bad"):
        assert {d[name] for d in ds} == {True, False}, name
    flat = [d for d in ds if not d["segmented"]]
    assert {(d["route"], d["hint"]) for d in flat} == {(0, False), (0, True), (1, False), (1, True)}
    assert any(d["n"] > 100_000 for d in ds) and all(1 <= d["n"] <= MAX_RECORDS for d in ds)
    assert sum(d["n"] < 20_000 for d in ds) > N_CASES * 2 // 3
    assert any(d["n"] in TILE_EDGES for d in ds) and any(d["nq"] in TILE_EDGES for d in ds)
    assert all(1 <= d["nq"] <= MAX_QUERIES for d in ds) and any(d["nq"] > 5_000 for d in ds)


def _draw_queries(d, table, rng):
    kind, nq = d["kind"], d["nq"]
    if d["qlaw"].startswith("table"):
        pool = sl.probe_queries(kind, d["up"], table)
        q = pool[rng.integers(0, len(pool), nq)]
    else:
        q = ul.random_keys(kind, nq, nq, rng)
    return sl.sorted_table(kind, d["up"], q) if d["qlaw"].endswith("sorted") else q


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(N_CASES))
def test_search_case(torch, case):
    d = make_case(case)
    rng = np.random.default_rng(SEED0 * 1000 + case)
    kind, up, n = d["kind"], d["up"], d["n"]
    keys = ul.random_keys(kind, n, d["distinct"], rng)
    flags = sl.HINT if d["hint"] else 0
    try:
        if not d["segmented"]:
            table = sl.sorted_table(kind, up, keys)
            sl.run_search(torch, srs_amd, kind, up, table, _draw_queries(d, table, rng),
                          outputs=d["outputs"], route=d["route"], flags=flags,
                          with_bad=d["with_bad"])
            return
        # nseg segments cut at random places (some empty), each sorted on its own;
        # one query in sixteen names a segment that does not exist
        nseg = d["nseg"]
        offsets = np.concatenate([[0], np.sort(rng.integers(0, n + 1, nseg - 1)), [n]]).astype(
            np.int64)
        table = keys.copy()
        for s in range(nseg):
            table[offsets[s]:offsets[s + 1]] = sl.sorted_table(kind, up,
                                                               keys[offsets[s]:offsets[s + 1]])
        q = _draw_queries(d, sl.sorted_table(kind, up, keys), rng)
        qseg = rng.integers(0, nseg, len(q)).astype(np.int64)
        wrong = rng.integers(0, 16, len(q)) == 0
        qseg[wrong] = rng.choice([-1, nseg, -(1 << 50), 1 << 50], np.count_nonzero(wrong))
        sl.run_search(torch, srs_amd, kind, up, table, q, offsets=offsets, qseg=qseg,
                      outputs=d["outputs"], route=d["route"], flags=flags, with_bad=d["with_bad"])
    except AssertionError as e:
        raise AssertionError(f"{e}: {d}") from None
