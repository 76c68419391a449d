"""Seeded case generator of the differential fuzz over the multi-GPU side
(tests/test_gpu_fuzz_shard.py): the key histogram, the stable partition and
the shard sort on the staged transport. Pure numpy: no GPU, no torch. It
follows tests/srs_fuzzlib.py and takes its key distributions, payload draws
and seeding from there.

make_case(api, case) returns a plain dict drawn from
default_rng(PRIME * case + API_CONST[api]); make_arrays(desc) returns the
case's host arrays from generators of their own ([seed, 1] keys, [seed, 2]
payloads, [seed, 3] the partition's table). Both are deterministic in
(api, case). No NaN key is generated.

Every expected result is exact: a bincount of the transformed top bits, a
stable argsort of the table's part ids, a stable argsort of the transformed
keys of all ranks in (rank, index) order.

Payloads: the set drawn by srs_fuzzlib._common (none, 1-3 columns, 8-12
columns of mixed widths), then a u32 column of input positions (globally
unique across the ranks of a shard case), so stability is checked wherever a
payload can show it. Half of the cases that drew no payload set stay `bare`:
keys only, the one-column path of the kernels and of the message sizes (equal
keys are equal bytes, so there is no order to check).

tests/test_shard_fuzz_plan.py checks that the fixed seeds reach the
combinations the fuzz exists for; N_CASES is what it needs. Shaped draws: the
histogram takes (key kind, direction) from a fixed grid (case mod 20) and a
class of n > 524 288 (the second trip of the grid-stride loop); an 8-bit
shard case goes to world 8 more often than chance; a world-1 shard case
takes the aliasing options half of the time; shard cases 3 and 7 mod 25 are
"all ranks empty" and "exactly one rank non-empty". The record caps keep the
GPU file's run time under that of tests/test_gpu_fuzz.py.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from srs_fuzzlib import (PRIME, _common, _draw_dist, _draw_kind, _log_uniform, gen_keys,
                         is_float, key_bits, winning_key)  # noqa: F401  (winning_key: re-export)
from srs_testlib import key_size, transformed_keys

APIS = ("key_hist", "partition", "shard")
API_CONST = {"key_hist": 601, "partition": 701, "shard": 809}
N_CASES = {"key_hist": 60, "partition": 200, "shard": 110}

HIST_MAX_BITS = 12           # kHistMaxBits: srs_key_histogram_device
HIST_GRID_RECORDS = 2048 * 256  # one trip of key_hist_kernel's grid-stride loop
HIST_MAX_RECORDS = 600_000
PART_MAX_BITS = 16           # srs_partition_device
PART_MAX_PARTS = 512         # kMaxBins
LDS_LUT_BITS = 12            # kLdsLutBits: flat tables up to 2^12 entries live in LDS
PART_MAX_RECORDS = 300_000
SHARD_MAX_RECORDS = 1 << 18  # all ranks of a shard case together
SHARD_BITS = 12              # srs_shard.hip kBits
SHARD_GROUPS = 512           # srs_shard.hip kGroups

TABLE_KINDS = ("aligned", "balanced", "monotone", "arbitrary", "single", "sparse")
PART_N_CLASSES = ("1", "2", "3..64", "~4096", "~8192", "log")
WORLDS = (1, 2, 3, 4, 5, 8)
ROUNDS_CHUNKS = ((0, 0), (1, 1), (3, 2), (8, 4), (16, 8), (64, 16))
MESSAGE_CAPS = (0, 64, 4096, 65536)
SMALL_CAP_RECORDS = 4096     # the 64-byte cap is drawn only up to this many records
MANY_PIECES_RECORDS = 1024   # all ranks of a (64 rounds, 16 chunks) case together
SHARD_N_CLASSES = ("0", "1", "2", "3..64", "~4096", "~8192", "log")


# --------------------------------------------------------------------------
# the library's rules, restated (moved here from tests/test_dist.py)
# --------------------------------------------------------------------------
def _top(kind, keys, bits, up=True):
    """the transformed top `bits` bits of every key"""
    return (transformed_keys(kind, up, keys) >> np.uint64(8 * key_size(kind) - bits)).astype(
        np.int64)


def _chunk_bound(n, c, chunks):
    """The library's chunk bounds (srs_shard.hip chunk_bound): the first
    chunk weighs 1, every other 4."""
    if c <= 0:
        return 0
    if c >= chunks:
        return n
    return n * (4 * c - 3) // (4 * chunks - 3)


def _chunk_hists(kind, keys, chunks, bits, up=True):
    n = len(keys)
    out = np.zeros((chunks, 1 << bits), np.uint64)
    top = _top(kind, keys, bits, up)
    for c in range(chunks):
        a, b = _chunk_bound(n, c, chunks), _chunk_bound(n, c + 1, chunks)
        out[c] = np.bincount(top[a:b], minlength=1 << bits)
    return out


def balanced_split(hist, parts) -> np.ndarray:
    """bins -> parts, non-decreasing: the shard plan's rule (srs_shard.hip
    balanced_split), as tests/test_gpu_sort.py restates it"""
    hv = np.asarray(hist, np.float64)
    mid = np.cumsum(hv) - hv + 0.5 * hv
    p = np.maximum.accumulate(np.clip(np.floor(mid * parts / hv.sum()), 0, parts - 1))
    return p.astype(np.int32)


def shard_options(d: dict) -> tuple:
    """(rounds, chunks) the library runs a shard case with (0 = its default:
    8 rounds; 4 chunks, at world 1 one)"""
    rounds, chunks = d["rounds"], d["chunks"]
    return rounds or 8, chunks or (4 if d["world"] > 1 else 1)


def partition_path(bits: int) -> int:
    """The way stage_lut reads a flat table of 2^bits entries: 0 the scalar
    loop, 1 packed u16 in LDS, 2 the global table per key."""
    return 0 if bits < 2 else 1 if bits <= LDS_LUT_BITS else 2


# --------------------------------------------------------------------------
# case descriptions
# --------------------------------------------------------------------------
@lru_cache(maxsize=1)
def _kind_up_grid():
    """The (key kind, direction) cells of the histogram in a fixed shuffled
    order: case i takes cell i mod 20."""
    cells = [(kind, up) for kind in range(10) for up in (True, False)]
    order = np.random.default_rng(API_CONST["key_hist"]).permutation(len(cells))
    return tuple(cells[int(i)] for i in order)


def _seed(api: str, case: int) -> int:
    return PRIME * case + API_CONST[api]


def _payload_set(d: dict, rng) -> None:
    _common(d, rng, False)
    d["bare"] = bool(not d["widths"] and rng.integers(0, 2))
    d["position_column"] = not d["bare"]


def _pick(rng, seq):
    return seq[int(rng.integers(0, len(seq)))]


def _key_hist_case(d: dict, rng) -> None:
    d["kind"], d["up"] = _kind_up_grid()[d["case"] % 20]
    kb = key_bits(d["kind"])
    top = min(HIST_MAX_BITS, kb)
    d["bits"] = top if rng.random() < (0.5 if kb == 8 else 0.2) else int(rng.integers(1, top + 1))
    cls = int(rng.choice(4, p=[0.1, 0.2, 0.5, 0.2]))
    d["n"] = (1, int(_pick(rng, (255, 256, 257))), _log_uniform(rng, 2, HIST_MAX_RECORDS),
              int(rng.integers(HIST_GRID_RECORDS + 1, HIST_MAX_RECORDS + 1)))[cls]
    d["prefill"] = bool(rng.integers(0, 2))
    d["twice"] = bool(rng.integers(0, 2))
    d["dist"] = _draw_dist(d["kind"], rng)


def _partition_case(d: dict, rng) -> None:
    d["kind"] = _draw_kind(rng)
    _payload_set(d, rng)
    kb = key_bits(d["kind"])
    path = int(rng.choice(3, p=[0.15, 0.5, 0.35])) if kb >= 16 else int(rng.choice(2, p=[0.2, 0.8]))
    lo, hi = ((1, 1), (2, min(LDS_LUT_BITS, kb)), (LDS_LUT_BITS + 1, PART_MAX_BITS))[path]
    bits = d["bits"] = int(rng.integers(lo, hi + 1))
    tk = d["table"] = TABLE_KINDS[int(rng.integers(0, len(TABLE_KINDS)))]
    cls = int(rng.choice(3, p=[0.3, 0.2, 0.5]))
    parts = (int(_pick(rng, (1, 2, 3, 511, 512))), 1 << int(rng.integers(0, 10)),
             _log_uniform(rng, 1, PART_MAX_PARTS))[cls]
    if tk == "aligned":  # 2^fb parts, fb <= bits: the table run_partition recognises
        parts = 1 << int(rng.integers(1, min(bits, 9) + 1))
    elif tk == "sparse":  # (a quarter of fewer than 4 ids is none)
        parts = max(parts, 4)
    d["num_parts"] = parts
    d["single_at"] = _pick(rng, ("first", "middle", "last")) if tk == "single" else None
    ncls = d["n_class"] = PART_N_CLASSES[int(rng.choice(6, p=[0.06, 0.08, 0.16, 0.15, 0.15, 0.4]))]
    d["n"] = {"1": 1, "2": 2, "3..64": int(rng.integers(3, 65)),
              "~4096": int(_pick(rng, (4095, 4096, 4097))),
              "~8192": int(_pick(rng, (8191, 8192, 8193))),
              "log": _log_uniform(rng, 65, PART_MAX_RECORDS)}[ncls]
    d["out_tail"] = bool(rng.integers(0, 2))
    d["stream"] = bool(rng.integers(0, 2))
    d["dist"] = _draw_dist(d["kind"], rng)


def _rank_n(rng, cls: str, world: int) -> int:
    return {"0": 0, "1": 1, "2": 2, "3..64": int(rng.integers(3, 65)),
            "~4096": 4096 + int(rng.integers(-2, 3)), "~8192": 8192 + int(rng.integers(-2, 3)),
            "log": _log_uniform(rng, 65, SHARD_MAX_RECORDS // world)}[cls]


def _shard_case(d: dict, rng) -> None:
    kind = d["kind"] = _draw_kind(rng)
    _payload_set(d, rng)
    world = int(_pick(rng, WORLDS))
    if key_bits(kind) == 8 and rng.random() < 0.4:  # 256 groups over 8 ranks
        world = 8
    d["world"] = world
    # per-rank sizes: a small case draws only from the classes up to 64
    small = rng.random() < 0.35
    p = np.array([1, 1, 1, 2, 0, 0, 0] if small else [1, 1, 1, 1, 1.5, 1.5, 3], float)
    classes = [SHARD_N_CLASSES[int(c)] for c in rng.choice(7, world, p=p / p.sum())]
    ns = [_rank_n(rng, c, world) for c in classes]
    d["shape"] = "drawn"
    if d["case"] % 25 == 3:
        ns, d["shape"] = [0] * world, "all_empty"
    elif d["case"] % 25 == 7:
        keep = int(rng.integers(0, world))
        ns, d["shape"] = [n if r == keep else 0 for r, n in enumerate(ns)], "one_rank"
        ns[keep] = max(ns[keep], 1)
    while sum(ns) > SHARD_MAX_RECORDS:  # (cannot happen with these classes; the cap is the rule)
        ns[int(np.argmax(ns))] //= 2
    d["rounds"], d["chunks"] = _pick(rng, ROUNDS_CHUNKS)
    d["self_messages"] = bool(rng.integers(0, 2))
    if world == 1 and rng.random() < 0.5:  # one chunk, no self messages: the buffers alias
        d["rounds"], d["chunks"] = _pick(rng, ROUNDS_CHUNKS[:2])
        d["self_messages"] = False
    # 64 rounds of 16 chunks are up to 1024 pieces per pair of ranks and column, each a
    # message of its own: few records keep most of them empty (the case's time is its messages)
    while (d["rounds"], d["chunks"]) == ROUNDS_CHUNKS[-1] and sum(ns) > MANY_PIECES_RECORDS:
        ns[int(np.argmax(ns))] //= 2
    d["ns"] = [int(n) for n in ns]
    caps = MESSAGE_CAPS if sum(ns) <= SMALL_CAP_RECORDS else (0, 4096, 65536)
    d["max_message_bytes"] = int(_pick(rng, caps))
    if rng.random() < 0.25:  # every rank its own distribution
        d["dist"] = [_draw_dist(kind, rng) for _ in range(world)]
    else:
        d["dist"] = _draw_dist(kind, rng)


def make_case(api: str, case: int) -> dict:
    """The description of case `case` of `api`: a plain dict."""
    seed = _seed(api, case)
    rng = np.random.default_rng(seed)
    d = {"api": api, "case": case, "seed": seed}
    if api == "key_hist":
        _key_hist_case(d, rng)
    elif api == "partition":
        _partition_case(d, rng)
    elif api == "shard":
        _shard_case(d, rng)
    else:
        raise ValueError(api)
    return d


# --------------------------------------------------------------------------
# arrays
# --------------------------------------------------------------------------
def _payloads(d: dict, rng, n: int, first: int) -> list:
    pays = [rng.integers(0, 1 << (8 * w), n, dtype=np.uint64).astype(f"u{w}") for w in d["widths"]]
    if d["position_column"]:
        pays.append((first + np.arange(n)).astype(np.uint32))
    return pays


def _table(d: dict, keys: np.ndarray) -> np.ndarray:
    """the partition's bin -> part table: 2^bits int32 entries in [0, num_parts)"""
    rng = np.random.default_rng([d["seed"], 3])
    bits, parts, tk = d["bits"], d["num_parts"], d["table"]
    nb = 1 << bits
    if tk == "aligned":
        fb = parts.bit_length() - 1
        t = np.arange(nb) >> (bits - fb)
    elif tk == "balanced":
        t = balanced_split(np.bincount(_top(d["kind"], keys, bits, d["up"]), minlength=nb), parts)
    elif tk == "monotone":
        t = np.sort(rng.integers(0, parts, nb))
    elif tk == "arbitrary":
        t = rng.integers(0, parts, nb)
        if parts >= 2 and np.all(np.diff(t) >= 0):
            t[0], t[-1] = parts - 1, 0
    elif tk == "single":
        t = np.full(nb, {"first": 0, "middle": parts // 2, "last": parts - 1}[d["single_at"]])
    elif tk == "sparse":
        ids = rng.choice(parts, max(1, parts // 4), replace=False)
        t = ids[rng.integers(0, len(ids), nb)]
    else:
        raise ValueError(tk)
    t = np.ascontiguousarray(t, dtype=np.int32)
    assert len(t) == nb and t.min() >= 0 and t.max() < parts
    return t


def make_arrays(d: dict) -> dict:
    """The host arrays of a case.

    key_hist: {"keys"}.
    partition: {"cols": [keys, payloads...], "table": int32[2^bits]}.
    shard: {"ranks": [[keys, payloads...] per rank]}.
    """
    api, kind = d["api"], d["kind"]
    rng = np.random.default_rng([d["seed"], 1])
    prng = np.random.default_rng([d["seed"], 2])
    if api == "key_hist":
        return {"keys": gen_keys(kind, d["n"], d["dist"], rng)}
    if api == "partition":
        keys = gen_keys(kind, d["n"], d["dist"], rng)
        return {"cols": [keys] + _payloads(d, prng, d["n"], 0), "table": _table(d, keys)}
    ranks, first = [], 0
    for r, n in enumerate(d["ns"]):
        dist = d["dist"][r] if isinstance(d["dist"], list) else d["dist"]
        ranks.append([gen_keys(kind, n, dist, rng)] + _payloads(d, prng, n, first))
        first += n
    return {"ranks": ranks}


def prefill_counts(d: dict) -> np.ndarray:
    """what a key_hist case's histogram holds before the call: random 40-bit
    counts, or zeros"""
    nb = 1 << d["bits"]
    if not d["prefill"]:
        return np.zeros(nb, np.int64)
    return np.random.default_rng([d["seed"], 2]).integers(0, 1 << 40, nb, dtype=np.int64)


# --------------------------------------------------------------------------
# what a case must exercise (computed from the description and the keys)
# --------------------------------------------------------------------------
def partition_dest(d: dict, arrays: dict) -> np.ndarray:
    """every record's part: table[top bits]"""
    return arrays["table"][_top(d["kind"], arrays["cols"][0], d["bits"], d["up"])]


def shard_plans(d: dict, arrays: dict, shard) -> list:
    """Every rank's plan of a shard case from the library's own planner
    (`shard`: the srs_amd.shard module; host only), fed by the ranks' chunk
    histograms."""
    rounds, chunks = shard_options(d)
    kb = key_bits(d["kind"])
    hs = np.stack([_chunk_hists(d["kind"], cols[0], chunks, min(SHARD_BITS, kb), d["up"])
                   for cols in arrays["ranks"]])
    return [shard.debug_plan(d["world"], r, chunks, rounds, kb, hs, d["ns"][r],
                             self_messages=d["self_messages"]) for r in range(d["world"])]


def shard_features(d: dict, plans: list) -> dict:
    """What the plans of a shard case make the device code run."""
    f = dict.fromkeys(("one_record_chunk", "empty_chunk", "short_round", "idle_rank", "alias"), False)
    totals = [p["total"] for p in plans]
    for r, p in enumerate(plans):
        sizes = np.diff(p["chunk_bounds"])
        f["one_record_chunk"] |= bool((sizes == 1).any())
        f["empty_chunk"] |= bool(d["ns"][r] > 0 and (sizes == 0).any())
        lens = [x["end"] - x["start"] for x in p["rounds"]]
        f["short_round"] |= min(lens) <= 1 and max(lens) >= 2
        f["idle_rank"] |= totals[r] == 0 and max(totals) > 0
        f["alias"] |= bool(p["alias"])
    return f
