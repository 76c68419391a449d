"""Seeded case generator of the differential fuzz over the newer entry points
(tests/test_gpu_fuzz_select.py): top-k, row-wise top-k, row-wise sort and the
segment sort. Pure numpy: no GPU, no torch.

make_case(api, case) returns a plain dict that describes one case (shape, key
kind, direction, distribution names, payload widths, route, ...), drawn from
default_rng(PRIME * case + API_CONST[api]) as tests/test_gpu_fuzz.py seeds its
cases. make_arrays(desc) returns the case's host arrays, drawn from generators
of their own ([seed, 1] keys, [seed, 2] payloads), so a description costs
nothing and the arrays of a case never depend on which of them were asked
for. Both are deterministic in (api, case).

Every expected result is the stable argsort of srs_testlib.transformed_keys:
exact and unique. NaN keys are outside the contract and never generated (the
padding around the rows of a float matrix holds the key that sorts first in
the direction, whose bit pattern is a NaN's: it is no key of any row).

tests/test_fuzz_plan.py checks, from the descriptions alone, that the fixed
seeds reach the combinations the fuzz exists for; N_CASES is what it needs.
Two draws are shaped for it: the row-wise top-k takes its key kind and
row-length class from a fixed shuffled grid (case mod 70) instead of two free
draws, so that every kind meets every kernel, and the float kinds are drawn
twice as often as an integer kind. The record caps are what keeps the GPU
file's run time under that of tests/test_gpu_fuzz.py.
"""
from __future__ import annotations

from functools import lru_cache

import numpy as np

from srs_testlib import KIND_DTYPES, KIND_NAMES, KIND_UINT, transformed_keys

APIS = ("topk", "topk_rows", "sort_rows", "segments")
API_CONST = {"topk": 101, "topk_rows": 211, "sort_rows": 307, "segments": 401}
PRIME = 1_000_003
# topk_rows walks the (key kind, length class) grid below three times
N_CASES = {"topk": 150, "topk_rows": 210, "sort_rows": 150, "segments": 150}
MAX_RECORDS = 1 << 19       # records of a top-k or a segment-sort case
ROWS_MAX_RECORDS = 1 << 18  # records in the rows of a matrix (without its padding)

RESIDENT, STREAM, LOOP = 0, 1, 2       # srs_amd.TOPK_ROWS_*
KERNEL, LOCAL, LEVELS = 0, 1, 2        # srs_amd.SORT_ROWS_*
LOCAL_CAP = 8192                       # kLocalCap: the longest resident row
TOPK_ROWS_MAX_K = 2048                 # srs_amd.TOPK_ROWS_MAX_K (checked by the GPU test)
TOPK_ROWS_MIN_CAP = 256                # kTopkRowsMinCap
HIST_BITS = 12                         # kHistMaxBits: the digit of a select pass

INT_DISTS = ("full", "narrow", "const", "skew", "shared_top", "two_values", "sorted",
             "reversed", "extremes")
INT_WEIGHTS = (1.0, 1.0, 1.0, 1.0, 3.0, 1.0, 0.5, 0.5, 1.0)
FLOAT_DISTS = ("full", "narrow", "const", "zeros", "specials")
FLOAT_WEIGHTS = (1.0, 1.0, 0.5, 1.0, 2.5)
KIND_WEIGHTS = (1, 1, 1, 1, 1, 1, 1, 1, 2, 2)
SNAPS = (64, 256, 1024, 2048, 4096, 8192)
# row-length classes of the row-wise top-k: the wave kernel, the 128-, 256-,
# 512- and 1024-thread resident kernels, and the streamed rows (twice: half of
# the grid's long rows keep min(k, row_len) <= TOPK_ROWS_MAX_K)
LEN_CLASSES = ((1, 256), (257, 1024), (1025, 2048), (2049, 4096), (4097, 8192),
               (8193, 40000), (8193, 40000))


def is_float(kind: int) -> bool:
    return KIND_NAMES[kind].startswith("f")


def key_bits(kind: int) -> int:
    return 8 * np.dtype(KIND_DTYPES[kind]).itemsize


def length_class(row_len: int) -> int:
    """index into LEN_CLASSES[:6]"""
    for i, (lo, hi) in enumerate(LEN_CLASSES[:6]):
        if lo <= row_len <= hi:
            return i
    raise ValueError(row_len)


def untransformed(kind: int, up: bool, u) -> np.ndarray:
    """Inverse of srs_testlib.transformed_keys: the keys (dtype of `kind`)
    whose transformed value is u."""
    nb = key_bits(kind)
    mask = np.uint64((1 << nb) - 1)
    sb = np.uint64(1 << (nb - 1))
    u = np.asarray(u, dtype=np.uint64) & mask
    if not up:
        u = ~u & mask
    name = KIND_NAMES[kind]
    if name.startswith("i"):
        bits = u ^ sb
    elif name.startswith("f"):
        bits = np.where((u & sb) != 0, u ^ sb, ~u & mask)
    else:
        bits = u
    return bits.astype(KIND_UINT[kind]).view(KIND_DTYPES[kind])


def winning_key(kind: int, up: bool):
    """The key that sorts first in the direction (transformed value 0: the
    smallest key ascending, the largest descending)."""
    return untransformed(kind, up, np.zeros(1, np.uint64))[0]


# --------------------------------------------------------------------------
# key distributions
# --------------------------------------------------------------------------
def _rand_bits(rng, nbits: int, n: int) -> np.ndarray:
    if nbits <= 0:
        return np.zeros(n, np.uint64)
    return rng.integers(0, 1 << nbits, n, dtype=np.uint64)


def float_specials(dtype, n: int, rng) -> np.ndarray:
    """Normals mixed with +-inf, +-0.0, +- the smallest and the largest
    denormal, +- the smallest normal and +- the largest finite value, each at
    about 3 percent. No NaN."""
    dt = np.dtype(dtype)
    fi = np.finfo(dt)
    tiny = dt.type(fi.tiny)
    table = np.array([np.inf, 0.0, fi.smallest_subnormal, np.nextafter(tiny, dt.type(0)), tiny,
                      fi.max], dtype=dt)
    table = np.concatenate([table, -table])
    v = (rng.standard_normal(n) * 1e3).astype(dt)
    hit = rng.random(n) < 0.03 * len(table)
    which = rng.integers(0, len(table), n)
    v[hit] = table[which[hit]]
    return v


def gen_keys(kind: int, n: int, dist: str, rng) -> np.ndarray:
    """n keys of `kind` from the named distribution"""
    dt = np.dtype(KIND_DTYPES[kind])
    ut = np.dtype(KIND_UINT[kind])
    bits = 8 * dt.itemsize
    if is_float(kind):
        if dist == "full":
            return rng.uniform(-1e6, 1e6, n).astype(dt)
        if dist == "narrow":
            return (rng.integers(-50, 50, n) * 0.25).astype(dt)  # dups, +-0.0
        if dist == "const":
            return np.full(n, -0.0, dt)
        if dist == "zeros":
            v = rng.uniform(-1, 1, n).astype(dt)
            v[rng.random(n) < 0.5] = 0.0
            return v
        if dist == "specials":
            return float_specials(dt, n, rng)
        raise ValueError(dist)
    ones = (1 << bits) - 1
    if dist in ("full", "sorted", "reversed"):
        u = _rand_bits(rng, bits, n)
    elif dist == "narrow":
        u = _rand_bits(rng, int(rng.integers(1, min(bits, 12) + 1)), n)
    elif dist == "const":
        u = np.full(n, 7, np.uint64)
    elif dist == "skew":  # most keys in one narrow band, the rest spread
        u = _rand_bits(rng, bits - 1, n)
        m = rng.random(n) < 0.8
        u[m] = _rand_bits(rng, min(bits - 1, 20), int(m.sum()))
    elif dist == "shared_top":  # a constant above bit b, uniform below
        lo, hi = (8, bits - 4) if bits >= 16 else (2, bits - 4)
        b = int(rng.integers(lo, hi + 1))
        twelves = [x for x in range(12, hi + 1, 12)]
        if twelves and rng.random() < 0.25:
            b = int(rng.choice(twelves))
        const = int(rng.integers(0, 1 << (bits - b), dtype=np.uint64))
        u = _rand_bits(rng, b, n) | np.uint64(const << b)
    elif dist == "two_values":
        a = int(rng.integers(0, 1 << bits, dtype=np.uint64)) if bits < 64 else \
            int(rng.integers(0, 1 << 63, dtype=np.uint64)) * 2 + int(rng.integers(0, 2))
        c = a ^ (1 << int(rng.integers(0, bits)))
        u = np.where(rng.random(n) < 0.5, np.uint64(a), np.uint64(c))
    elif dist == "extremes":  # type min, max, -1, 0 and 1 among uniform values
        u = _rand_bits(rng, bits, n)
        if dt.kind == "i":
            table = np.array([1 << (bits - 1), (1 << (bits - 1)) - 1, ones, 0, 1], np.uint64)
        else:
            table = np.array([0, ones, ones, 0, 1], np.uint64)
        hit = rng.random(n) < 0.3
        which = rng.integers(0, len(table), n)
        u[hit] = table[which[hit]]
    else:
        raise ValueError(dist)
    keys = u.astype(ut).view(dt)
    if dist == "sorted":
        keys = np.sort(keys)
    elif dist == "reversed":
        keys = np.sort(keys)[::-1].copy()
    return keys


def _draw_dist(kind: int, rng) -> str:
    names, w = (FLOAT_DISTS, FLOAT_WEIGHTS) if is_float(kind) else (INT_DISTS, INT_WEIGHTS)
    p = np.asarray(w) / sum(w)
    return names[int(rng.choice(len(names), p=p))]


def _draw_kind(rng) -> int:
    """a key kind, the two float kinds twice as often as an integer kind"""
    return int(rng.choice(10, p=np.asarray(KIND_WEIGHTS) / sum(KIND_WEIGHTS)))


def _log_uniform(rng, lo: int, hi: int) -> int:
    """an integer in [lo, hi], log-uniform"""
    v = int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))))
    return max(lo, min(hi, v))


# --------------------------------------------------------------------------
# case descriptions
# --------------------------------------------------------------------------
@lru_cache(maxsize=1)
def _grid():
    """The (key kind, length class) cells of the row-wise top-k in a fixed
    shuffled order: case i takes cell i mod 70."""
    cells = [(kind, cls) for kind in range(10) for cls in range(len(LEN_CLASSES))]
    order = np.random.default_rng(API_CONST["topk_rows"]).permutation(len(cells))
    return tuple(cells[int(i)] for i in order)


def _seed(api: str, case: int) -> int:
    return PRIME * case + API_CONST[api]


def _common(d: dict, rng, with_indices: bool) -> None:
    d["up"] = bool(rng.integers(0, 2))
    if rng.random() < 0.125:  # many columns of mixed widths
        widths = [int(w) for w in rng.choice([1, 2, 4, 8], int(rng.integers(8, 13)))]
        d["many"] = True
    else:
        widths = [int(w) for w in rng.choice([1, 2, 4, 8], int(rng.integers(0, 4)))]
        d["many"] = False
    d["widths"] = widths
    d["indices"] = bool(rng.integers(0, 2)) if with_indices else False
    # without indices a u32 column of each record's position is appended, so
    # stability is still checked
    d["position_column"] = not d["indices"]


def _row_len(rng, lo: int = 1, hi: int = 40000) -> int:
    n = _log_uniform(rng, lo, hi)
    if rng.random() < 1 / 3:
        snaps = [b + o for b in SNAPS for o in (-1, 0, 1) if lo <= b + o <= hi]
        if snaps:
            n = int(rng.choice(snaps))
    return n


def _rows_shape(d: dict, rng, row_len: int) -> None:
    rows = _log_uniform(rng, 1, 300)
    if row_len <= 512 and rng.random() < 0.25:
        rows = _log_uniform(rng, 300, 5000)
    rows = max(1, min(rows, ROWS_MAX_RECORDS // row_len))
    d["rows"], d["row_len"] = rows, row_len
    d["stride"] = row_len + int(rng.choice([0, 1, 3, 8, row_len]))
    d["first"] = int(rng.integers(0, 4))  # elements before the first row
    d["out_tail"] = bool(rng.integers(0, 2))  # out= tensors with a sentinel tail
    if rng.random() < 0.25:  # every row its own distribution
        d["dist"] = [_draw_dist(d["kind"], rng) for _ in range(rows)]
    else:
        d["dist"] = _draw_dist(d["kind"], rng)


def _topk_rows_k(rng, n: int, cls: int) -> int:
    opts = {"one": [1], "log": [_log_uniform(rng, 1, n)], "edge": [n - 1, n, n + 3],
            "b128": [k for k in (127, 128, 129) if k <= n],
            "b2048": [k for k in (2047, 2048, 2049) if k <= n],
            "half": [n // 2, n // 2 + 1]}
    if cls == 6:  # the long rows that must be able to stream
        opts["log"] = [_log_uniform(rng, 1, TOPK_ROWS_MAX_K)]
        del opts["edge"], opts["half"]
    names = [c for c in opts if any(k >= 1 for k in opts[c])]
    pick = [k for k in opts[names[int(rng.integers(0, len(names)))]] if k >= 1]
    return int(pick[int(rng.integers(0, len(pick)))])


def make_case(api: str, case: int) -> dict:
    """The description of case `case` of `api`: a plain dict."""
    seed = _seed(api, case)
    rng = np.random.default_rng(seed)
    d = {"api": api, "case": case, "seed": seed}
    if api == "topk_rows":
        d["kind"], cls = _grid()[case % len(_grid())]
        _common(d, rng, True)
        _rows_shape(d, rng, _row_len(rng, *LEN_CLASSES[cls]))
        n = d["row_len"]
        d["k"] = _topk_rows_k(rng, n, cls)
        kk = min(d["k"], n)
        if n > LOCAL_CAP and kk > TOPK_ROWS_MAX_K:  # only the loop takes it: keep it short
            d["rows"] = min(d["rows"], 32)
            if isinstance(d["dist"], list):
                d["dist"] = d["dist"][:d["rows"]]
        routes = [RESIDENT] if n <= LOCAL_CAP else ([STREAM] if kk <= TOPK_ROWS_MAX_K else [])
        if d["rows"] <= 8:
            routes.append(LOOP)
        forced = rng.random() < 1 / 3 and routes
        d["route"] = int(routes[int(rng.integers(0, len(routes)))]) if forced else -1
        d["sample_rows"] = sorted({int(r) for r in rng.integers(0, d["rows"], 2)})
    elif api == "sort_rows":
        d["kind"] = _draw_kind(rng)
        _common(d, rng, True)
        _rows_shape(d, rng, _row_len(rng))
        n = d["row_len"]
        # every route that takes the length (tests/test_gpu_sort_rows.py:
        # _routes_for), then the library's rule
        d["routes"] = ([LEVELS] if n > LOCAL_CAP else [KERNEL] + ([LOCAL] if n >= 2 else [])) + [-1]
    elif api == "topk":
        d["kind"] = _draw_kind(rng)
        _common(d, rng, True)
        d["n"] = _log_uniform(rng, 1, MAX_RECORDS)
        d["k"] = _log_uniform(rng, 1, d["n"] + 5)
        d["candidates"] = int(rng.choice([4096, 16384])) if rng.random() < 1 / 3 else 0
        d["aos"] = bool(rng.random() < 0.25)
        if d["aos"]:
            ks = key_bits(d["kind"]) // 8
            sizes = [s for s in (1, 2, 4, 8, 16, 32, 64) if s >= ks]
            d["elem_size"] = int(rng.choice(sizes))
            d["widths"], d["many"] = [], False
        d["dist"] = _draw_dist(d["kind"], rng)
    elif api == "segments":
        d["kind"] = _draw_kind(rng)
        _common(d, rng, False)
        n = d["n"] = _log_uniform(rng, 2, MAX_RECORDS)
        d["bounds"] = _segment_bounds(rng, n, _log_uniform(rng, 1, 3000))
        d["known_top_bits"] = 0
        if rng.random() < 0.25:
            d["known_top_bits"] = int(rng.integers(1, min(20, key_bits(d["kind"]) - 1) + 1))
        d["dist"] = _draw_dist(d["kind"], rng)
    else:
        raise ValueError(api)
    return d


def _segment_bounds(rng, n: int, nsegs: int) -> list:
    """nsegs + 1 non-decreasing offsets within [0, n]: empty segments, lengths
    on both sides of 4096 and 8192 (where a segment changes its kernel), and
    usually a head and a tail that belong to no segment."""
    pos = int(rng.integers(0, min(50, n // 4) + 1))  # the head gap
    tail = int(rng.integers(0, min(50, n // 4) + 1))
    end = n - tail
    bounds = [pos]
    kinds = rng.choice(7, nsegs, p=[0.15, 0.05, 0.3, 0.2, 0.1, 0.1, 0.1])
    for c in kinds:
        if c == 0:
            ln = 0
        elif c == 1:
            ln = 1
        elif c == 2:
            ln = _log_uniform(rng, 2, 64)
        elif c == 3:
            ln = _log_uniform(rng, 65, 4000)
        elif c == 4:
            ln = 4096 + int(rng.integers(-2, 3))
        elif c == 5:
            ln = 8192 + int(rng.integers(-2, 3))
        else:
            ln = _log_uniform(rng, 8193, 200000)
        pos = min(end, pos + ln)
        bounds.append(pos)
        if pos == end and len(bounds) > 3 and bounds[-3] == end:
            break  # (the array is used up: two empty segments close the list)
    return bounds


# --------------------------------------------------------------------------
# arrays
# --------------------------------------------------------------------------
def _payloads(d: dict, total: int, position) -> list:
    rng = np.random.default_rng([d["seed"], 2])
    pays = [rng.integers(0, 1 << (8 * w), total, dtype=np.uint64).astype(f"u{w}")
            for w in d["widths"]]
    if d["position_column"]:
        pays.append(position.astype(np.uint32))
    return pays


def make_arrays(d: dict) -> dict:
    """The host arrays of a case.

    topk: {"cols": [keys, payloads...]} or, AoS, {"records": (n, elem_size)
    uint8, "keys": the key of every record}.
    segments: {"cols": [keys, payloads...]}.
    topk_rows / sort_rows: {"flat": [one flat allocation per column], "index":
    (rows, row_len) positions of the rows' elements in it}; everything
    outside the rows holds the winning key (keys) or random bytes (payloads).
    """
    api, kind = d["api"], d["kind"]
    rng = np.random.default_rng([d["seed"], 1])
    if api == "topk":
        n = d["n"]
        keys = gen_keys(kind, n, d["dist"], rng)
        if d["aos"]:
            es, ks = d["elem_size"], keys.dtype.itemsize
            rec = np.random.default_rng([d["seed"], 2]).integers(0, 256, (n, es), dtype=np.uint8)
            rec[:, :ks] = keys.view(np.uint8).reshape(n, ks)
            if d["position_column"] and es - ks >= 4:  # the record's position in its last bytes
                rec[:, es - 4:] = np.arange(n, dtype=np.uint32).view(np.uint8).reshape(n, 4)
            return {"records": rec, "keys": keys}
        return {"cols": [keys] + _payloads(d, n, np.arange(n))}
    if api == "segments":
        n, b = d["n"], d["known_top_bits"]
        keys = gen_keys(kind, n, d["dist"], rng)
        if b:
            keys = _share_top_bits(d, keys, rng)
        return {"cols": [keys] + _payloads(d, n, np.arange(n))}
    rows, n, stride, first = d["rows"], d["row_len"], d["stride"], d["first"]
    total = first + rows * stride
    index = first + np.arange(rows)[:, None] * stride + np.arange(n)[None, :]
    flat = np.full(total, winning_key(kind, d["up"]), KIND_DTYPES[kind])
    if isinstance(d["dist"], list):
        for r, name in enumerate(d["dist"]):
            flat[index[r]] = gen_keys(kind, n, name, rng)
    else:
        flat[index.ravel()] = gen_keys(kind, rows * n, d["dist"], rng)
    position = np.zeros(total, np.int64)
    position[index.ravel()] = np.tile(np.arange(n), rows)
    return {"flat": [flat] + _payloads(d, total, position), "index": index}


def _share_top_bits(d: dict, keys: np.ndarray, rng) -> np.ndarray:
    """Every segment's keys made to agree on their top known_top_bits
    transformed bits: a segment takes them from one of its own keys and keeps
    its keys' lower bits. (A float whose new pattern is no finite number is
    replaced by that key.)"""
    kind, up, b = d["kind"], d["up"], d["known_top_bits"]
    bounds = np.asarray(d["bounds"], np.int64)
    nb = key_bits(kind)
    low = np.uint64((1 << (nb - b)) - 1)
    u = transformed_keys(kind, up, keys)
    lens = np.diff(bounds)
    seg = np.repeat(np.arange(len(lens)), lens)
    owner = np.repeat(bounds[:-1], lens)  # each record's segment's first record
    sl = slice(int(bounds[0]), int(bounds[-1]))
    assert len(seg) == sl.stop - sl.start
    v = (u[owner] & ~low) | (u[sl] & low)
    out = keys.copy()
    new = untransformed(kind, up, v)
    if is_float(kind):
        bad = ~np.isfinite(new)
        new[bad] = keys[owner][bad]
    out[sl] = new
    return out


# --------------------------------------------------------------------------
# what a case must exercise (computed from the description and the keys)
# --------------------------------------------------------------------------
def topk_rows_route(d: dict) -> int:
    """The route the case takes (the library's rule where none is forced)."""
    if d["route"] >= 0:
        return d["route"]
    n, kk = d["row_len"], min(d["k"], d["row_len"])
    return RESIDENT if n <= LOCAL_CAP else STREAM if kk <= TOPK_ROWS_MAX_K else LOOP


def topk_rows_select(d: dict) -> bool:
    """a row is selected before it is sorted: row_len > max(2 kk, 256)"""
    kk = min(d["k"], d["row_len"])
    return d["row_len"] > max(2 * kk, TOPK_ROWS_MIN_CAP)


def topk_rows_cap(d: dict) -> int:
    """The LDS slots of a row (launch_topk_rows): max(2 kk, 256), at most 8192
    resident and 4096 streamed, rounded up to a power of two."""
    n, kk = d["row_len"], min(d["k"], d["row_len"])
    fit = max(2 * kk, TOPK_ROWS_MIN_CAP)
    route_cap = 2 * TOPK_ROWS_MAX_K if topk_rows_route(d) == STREAM else LOCAL_CAP
    want, cap = min(fit if n > fit else n, route_cap), 2
    while cap < want:
        cap <<= 1
    return cap


def topk_rows_passes(d: dict, arrays: dict | None = None) -> dict:
    """Whether the case must take at least two select passes, by the stop rule
    of DESIGN.md §12: on a one-launch route a selected row longer than its LDS
    slots is refined while the 12-bit bucket that holds rank kk of the first
    digit holds more than `cap` records, is not wholly inside the first kk and
    its keys are not all equal. Returns {"two": bool, "unaligned": bool,
    "top": the bit below which the second digit starts (the highest varying
    bit of such a row + 1), or None}. unaligned: that bit is below the first
    digit's end and neither a multiple of 12 nor a whole number of 12-bit
    digits below the key's top."""
    res = {"two": False, "unaligned": False, "top": None}
    kb = key_bits(d["kind"])
    n, kk = d["row_len"], min(d["k"], d["row_len"])
    cap = topk_rows_cap(d)
    if topk_rows_route(d) == LOOP or not topk_rows_select(d) or n <= cap or kb <= HIST_BITS:
        return res
    if arrays is None:
        arrays = make_arrays(d)
    u = transformed_keys(d["kind"], d["up"], arrays["flat"][0][arrays["index"]])
    shift = kb - HIST_BITS
    digit = (u >> np.uint64(shift)).astype(np.uint16)
    dk = np.sort(digit, axis=1)[:, kk - 1:kk]  # the bucket of rank kk
    inb = digit == dk
    cand = inb.sum(axis=1)
    k_rem = kk - (digit < dk).sum(axis=1)
    bmax = np.where(inb, u, np.uint64(0)).max(axis=1)
    bmin = np.where(inb, u, np.uint64(0xFFFFFFFFFFFFFFFF)).min(axis=1)
    two = (cand > cap) & (cand != k_rem) & (bmax != bmin)
    if not two.any():
        return res
    res["two"] = True
    low = np.uint64((1 << shift) - 1)
    var = (np.bitwise_or.reduce(u, axis=1) ^ np.bitwise_and.reduce(u, axis=1)) & low
    for v in var[two]:
        top = int(v).bit_length()
        res["top"] = top
        if top < shift and top % 12 != 0 and (kb - top) % 12 != 0:
            res["unaligned"] = True
            break
    return res


@lru_cache(maxsize=1)
def two_pass_cases() -> tuple:
    """The topk_rows cases that must take >= 2 select passes (the GPU test
    asserts the pass count the kernel reports on them)."""
    return tuple(i for i in range(N_CASES["topk_rows"])
                 if topk_rows_passes(make_case("topk_rows", i))["two"])
