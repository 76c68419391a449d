"""Cases and expectations of the ragged sort's tests (sort_ragged_device).

Pure numpy, no GPU: ragged_orders() is the expectation every ragged test
compares with, make_case() / make_arrays() the seeded fuzz cases of
tests/test_gpu_fuzz_ragged.py, whose descriptions tests/test_ragged_plan.py
reads to show what the fixed seeds reach. Key kinds, distributions and the key
generator are srs_fuzzlib's.
"""
from __future__ import annotations

import numpy as np

import srs_fuzzlib as fz
from srs_testlib import KIND_DTYPES, UINT_OF_SIZE, transformed_keys

N_CASES = 120
MAX_RECORDS = 1 << 18
PRIME = 1_000_003
SEED0 = 509
SHORT_MAX = 256   # kRowsWaveMax: the short kernel's default maximum
SMALL_CAP = 4096  # kLocalCapSmall
LOCAL_CAP = 8192  # kLocalCap
LENGTH_LAWS = ("tiny", "power", "uniform600", "giant", "near8192")
SHORT_MAXES = (-1, 0, 64)


def ragged_orders(kind: int, up: bool, keys: np.ndarray, offsets) -> tuple:
    """(src, idx, lo, hi): the sorted covered range [lo, hi) holds, at lo + j,
    input record src[j]; idx[j] is that record's position inside its segment.
    Per segment the stable argsort of transformed_keys."""
    offsets = np.asarray(offsets, dtype=np.int64)
    lo, hi = int(offsets[0]), int(offsets[-1])
    lens = np.diff(offsets)
    seg = np.repeat(np.arange(len(lens)), lens)
    u = transformed_keys(kind, up, np.ascontiguousarray(keys[lo:hi]))
    order = np.lexsort((u, seg))  # stable: by segment, then key, then position
    src = order + lo
    idx = src - np.repeat(offsets[:-1], lens)
    return src, idx.astype(np.int64), lo, hi


def class_counts(lengths, short_max: int = SHORT_MAX, indices: bool = False) -> tuple:
    """(segments left to the short kernel, small-class, large-class, big list
    lengths) the classify pass must report for these segment lengths. With
    indices the listed segments sort in place on the outputs, where one of a
    single record is finished by the prepare pass and enters no list."""
    ln = np.asarray(lengths, dtype=np.int64)
    listed = ln > short_max
    small = listed & (ln <= SMALL_CAP) & ((ln > 1) | (not indices))
    return (int(((ln >= 1) & ~listed).sum()), int(small.sum()),
            int((listed & (ln > SMALL_CAP) & (ln <= LOCAL_CAP)).sum()),
            int((listed & (ln > LOCAL_CAP)).sum()))


# --------------------------------------------------------------------------
# fuzz cases
# --------------------------------------------------------------------------
def _lengths(law: str, rng, budget: int) -> list:
    """segment lengths of the law, their sum at most `budget`"""
    if law == "tiny":
        ln = rng.integers(0, 9, int(rng.integers(1, 20000)))
    elif law == "power":  # mean ~32 with a heavy tail: a few segments over 8192
        ln = np.minimum((rng.pareto(1.1, int(rng.integers(200, 6000))) * 8).astype(np.int64), 60000)
    elif law == "uniform600":
        ln = rng.integers(0, 601, int(rng.integers(1, 800)))
    elif law == "giant":  # one long segment among tiny ones
        ln = rng.integers(0, 9, int(rng.integers(1, 2000)))
        ln[int(rng.integers(0, len(ln)))] = fz._log_uniform(rng, 300, 150000)
    elif law == "near8192":
        ln = rng.integers(8192 - 2000, 8192 + 2001, int(rng.integers(1, 28)))
    else:
        raise ValueError(law)
    ln = [int(x) for x in ln]
    while sum(ln) > budget:  # (drop from the end: the prefix keeps the law's shape)
        ln.pop()
    return ln or [0]


def make_case(case: int) -> dict:
    """The description of fuzz case `case`: plain Python values only."""
    rng = np.random.default_rng(PRIME * case + SEED0)
    d = {"case": case}
    d["kind"] = fz._draw_kind(rng)
    d["up"] = bool(rng.integers(0, 2))
    d["dist"] = fz._draw_dist(d["kind"], rng)
    d["widths"] = [int(w) for w in rng.choice([1, 2, 4, 8], int(rng.integers(0, 4)))]
    d["indices"] = bool(rng.integers(0, 2))
    d["law"] = LENGTH_LAWS[case % len(LENGTH_LAWS)]
    d["short_max"] = SHORT_MAXES[(case // len(LENGTH_LAWS)) % len(SHORT_MAXES)]
    d["head"] = int(rng.integers(0, 100)) if rng.random() < 0.5 else 0
    d["tail"] = int(rng.integers(1, 100)) if rng.random() < 0.5 else 0
    ln = _lengths(d["law"], rng, MAX_RECORDS - d["head"] - d["tail"])
    if case % 17 == 3:  # one segment covering everything
        ln = [max(1, sum(ln))]
    d["lengths"] = ln
    d["num"] = d["head"] + sum(ln) + d["tail"]
    return d


def make_arrays(d: dict) -> dict:
    """{"cols": [keys, payloads...], "offsets": int64 array} of the case. The
    first payload (when there is one) counts the records, so stability shows
    in it; the others are random bytes."""
    rng = np.random.default_rng(PRIME * d["case"] + SEED0 + 1)
    n = d["num"]
    keys = np.ascontiguousarray(fz.gen_keys(d["kind"], n, d["dist"], rng))
    assert keys.dtype == np.dtype(KIND_DTYPES[d["kind"]])
    cols = [keys]
    for i, w in enumerate(d["widths"]):
        ut = UINT_OF_SIZE[w]
        if i == 0:
            cols.append(np.arange(n, dtype=np.uint64).astype(ut))
        else:
            cols.append(rng.integers(0, 1 << (8 * w), n, dtype=np.uint64).astype(ut))
    offsets = d["head"] + np.concatenate([[0], np.cumsum(np.asarray(d["lengths"], np.int64))])
    return {"cols": cols, "offsets": offsets.astype(np.int64)}
