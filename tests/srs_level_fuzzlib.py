"""Seeded case plan of the differential fuzz over the sort's large-input
levels (tests/test_gpu_fuzz_levels.py): the plain first level, the balanced
first level (digit tables, range level), the stripe first level and the
gathered level behind it. Pure numpy: no GPU, no torch.

Those levels are chosen by compiled-in sizes (2^24, 2^25, stripes of 0.5-2 M
records). srs_amd.debug_set_first_level lowers them for a process, so every
case here has at most MAX_RECORDS records and still takes the path it names.
Most cases have TYPICAL_N = 2^16 .. 2^20 records; above that are only the
cases that need it (more than 256 stripes, two stripes of the planner's own
lengths, a full stripe as one piece, every sixth general case).

make_case(i) returns (description, arrays). describe(i) alone is the
description: a plain dict drawn from default_rng(PRIME * i + SEED_CONST); the
arrays come from generators of their own ([seed, 1] keys, [seed, 2]
payloads). Both are deterministic in i. A description names its class and,
under "hook", the arguments of debug_set_first_level that send its n down
that class's path; "promise" is what srs_amd.debug_last_first_level must
report after the sort:

  general           no one-launch start, no stripes: plain levels over one
                    segment, then over several
  stripes-plain     the stripe level with a plain digit, uniform key bits
  stripes-pieces    as above, with the size of every piece (one stripe's share
                    of one bucket) chosen by the case
  stripes-balanced  skewed keys: a digit table or a range level in stripes
  declined          inputs the stripe level must not take although n reaches
                    its smallest size

Where the draws must reach a combination they follow the case's index in its
class instead of the generator (key kind and direction, the stripe-count
band, the record shape, the forced table); tests/test_level_fuzz_plan.py
checks the coverage from the descriptions. Every expected result is the
stable argsort of srs_testlib.transformed_keys. NaN keys are outside the
contract and never generated.
"""
from __future__ import annotations

import numpy as np

from srs_fuzzlib import FLOAT_DISTS, FLOAT_WEIGHTS, INT_DISTS, INT_WEIGHTS, float_specials, \
    gen_keys, is_float, key_bits, untransformed
from srs_testlib import KIND_DTYPES, KIND_NAMES, KIND_UINT, transformed_keys

PRIME = 1_000_003
SEED_CONST = 907
TILE = 4096                 # kTile
PAIR = 2 * TILE             # a tile pair: the unit of the hook's stripe length
LOCAL_CAP = 8192            # kLocalCap: sorts above it are not "small"
MAX_RECORDS = (1 << 22) + (1 << 19)
MAX_STRIPE_PAIRS = 244      # 3904 << 9 records: the planner's longest stripe
SAMPLE_CHUNK, SAMPLE_MAX_CHUNKS = 1024, 4096  # kSampleChunk, kSampleMaxChunks
BALANCED_SKEW = 4           # kBalancedSkew
CLUSTER_GAP, CLUSTER_SPAN, MAX_RANGES = 4096, 256, 4  # srs_plan.h

CLASSES = ("general", "stripes-plain", "stripes-pieces", "stripes-balanced", "declined")
CLASS_COUNTS = (36, 48, 30, 48, 26)
N_CASES = sum(CLASS_COUNTS)
STRIPE_CLASSES = CLASSES[1:4]

WIDE_KINDS = (4, 5, 6, 7, 8, 9)  # u32 i32 u64 i64 f32 f64
COMBOS = tuple((k, up) for k in WIDE_KINDS for up in (True, False))
# Stripe-count bands, one per code path of the stripe tables: one trip of
# stripe_tiles_kernel's loop over chunks of 256 stripes; its second trip; the
# second trip of stripe_order_kernel's sum `for (i = b; i < s; i += 512)`,
# which the last stripe takes once s = K - 1 >= 513. (K = 513 is still one
# trip: it counts with the middle band.)
K_BANDS = ((2, 256), (257, 513), (514, MAX_RECORDS // PAIR))
TYPICAL_N = (1 << 16, 1 << 20)  # most cases have this many records
PIECE_SIZES = (0, 1, 4095, 4096, 4097, 8191, 8192, 8193)
PIECES_STRIPE_PAIRS = 2     # stripes of 16384 records: a piece of 8193 fits
# the special pieces of a stripes-pieces case, one list per hot bucket; -1 is
# a piece that is a whole stripe. Every other stripe's piece of a hot bucket is
# empty.
HOT_PIECES = ((8193, 4095, 1), (8192, 4096), (8191, 4097), (-1,), (1, 4096, 4097))
DECLINED = ("equal", "canon", "segments", "ranges_final", "two_byte")
PLAIN_STRIPE_PAIRS = (1, 2, 3, 5, 8, 16, 32, 61, 122, 244)
LAST_STRIPES = ("full", "one", "subtile", "free")


def class_of(case: int):
    """(class name, index of the case in its class)"""
    for name, count in zip(CLASSES, CLASS_COUNTS):
        if case < count:
            return name, case
        case -= count
    raise ValueError(case)


def choose_bits(length: int, rbits: int) -> int:
    """srs_common.h choose_bits: the digit width of a segment"""
    def levels_for(target):
        need = 1
        while need < 62 and (target << need) < length:
            need += 1
        return (need + 8) // 9, need
    levels, need = levels_for(6144)
    levels_cap, need_cap = levels_for(7808)
    if levels_cap < levels:
        levels, need = levels_cap, need_cap
    levels_small, need_small = levels_for(3840)
    if levels_small == levels:
        need = need_small
    return max(1, min((need + levels - 1) // levels, 9, rbits))


def log_uniform(rng, lo: int, hi: int) -> int:
    """an integer in [lo, hi], log-uniform"""
    v = int(np.exp(rng.uniform(np.log(lo), np.log(hi + 1))))
    return max(lo, min(hi, v))


def draw_dist(kind: int, rng) -> str:
    """a key distribution of srs_fuzzlib.gen_keys, by its weights"""
    names, w = (FLOAT_DISTS, FLOAT_WEIGHTS) if is_float(kind) else (INT_DISTS, INT_WEIGHTS)
    return names[int(rng.choice(len(names), p=np.asarray(w) / sum(w)))]


def stripe_count(n: int, pairs: int) -> int:
    return -(-n // (PAIR * pairs))


def k_band(k: int) -> int:
    return next(i for i, (lo, hi) in enumerate(K_BANDS) if lo <= k <= hi)


# --------------------------------------------------------------------------
# descriptions
# --------------------------------------------------------------------------
def _shape(d: dict, rng, shape: str) -> None:
    """The record layout: SoA columns (0-3 payloads and the position column),
    C2's key + two u32 (the second holds the position), or AoS records."""
    ks = key_bits(d["kind"]) // 8
    d["shape"], d["widths"], d["elem_size"] = shape, [], 0
    if shape == "soa":
        d["widths"] = [int(w) for w in rng.choice([1, 2, 4, 8], int(rng.integers(0, 4)))]
    elif shape == "pair":
        d["widths"] = [4]
    else:
        d["shape"] = "aos"
        d["elem_size"] = int(shape[3:]) if len(shape) > 3 else \
            int(rng.choice([s for s in (8, 16, 32, 64) if s >= ks]))
    d["inplace"] = bool(rng.integers(0, 2))
    d["pair_tiles"] = (None, 1, 2, 3)[int(rng.integers(0, 4))]


def _stripe_n(rng, pairs: int, k_lo: int, k_hi: int, last: str):
    """n with a stripe count in [k_lo, k_hi] whose last stripe is `last`"""
    length = PAIR * pairs
    least = {"full": length, "one": 1, "subtile": TILE - 1, "free": 1}[last]
    k_hi = min(k_hi, (MAX_RECORDS - least) // length + 1)
    lo = max(k_lo, 2 if last == "full" else 3)  # (n >= 2 stripes)
    assert lo <= k_hi, (pairs, k_lo, k_hi, last)
    k = int(rng.integers(lo, k_hi + 1))
    room = min(length, MAX_RECORDS - (k - 1) * length)
    tail = {"full": length, "one": 1, "subtile": int(rng.integers(2, TILE)),
            "free": int(rng.integers(1, room + 1))}[last]
    return (k - 1) * length + tail


def _hook(**kw) -> dict:
    h = {"general_min_n": 1, "balanced_min_n": 0, "stripe_min_n": 0, "stripe_pairs": 0,
         "first_bits": 0}
    h.update(kw)
    return h


def _promise_stripes(d: dict, kind_zero: bool) -> None:
    h = d["hook"]
    kb = key_bits(d["kind"])
    b1 = 9 if not kind_zero else h["first_bits"] or choose_bits(d["n"], kb)
    d["promise"] = {"start": 0, "stripes": 1, "stripe_count": stripe_count(d["n"], h["stripe_pairs"]),
                    "first_bits": b1, "kind_zero": kind_zero}


def describe(case: int) -> dict:
    cls, j = class_of(case)
    seed = PRIME * case + SEED_CONST
    rng = np.random.default_rng(seed)
    d = {"case": case, "seed": seed, "cls": cls, "index": j, "thresh": 16, "table": None,
         "bounds": None}
    if cls == "general":
        d["kind"], d["up"] = j % 10, bool(rng.integers(0, 2))
        _shape(d, rng, ("soa", "soa", "pair", "aos", "soa", "aos")[j % 6])
        # 2^16 .. 2^20 records; every sixth case just above the single-workgroup
        # capacity, every sixth up to 2^21
        lo, hi = {0: (LOCAL_CAP + 1, 1 << 16), 5: (1 << 20, 1 << 21)}.get(j % 6, TYPICAL_N)
        n = log_uniform(rng, lo, hi)
        if rng.random() < 0.3:  # around a tile or a tile pair
            n = min(hi, max(lo, n // TILE * TILE + int(rng.integers(-1, 2))))
        d["n"] = n
        d["dist"] = draw_dist(d["kind"], rng)
        d["hook"] = _hook()
        d["promise"] = {"start": 0, "stripes": 0}
    elif cls == "stripes-plain":
        d["kind"], d["up"] = COMBOS[(j + j // 4) % 12]
        _shape(d, rng, ("soa", "pair", "aos16", "soa", "aos32", "soa")[j % 6])
        band = (0, 0, 1, 2)[j % 4]
        d["last"] = LAST_STRIPES[(j // 4 + j // 16) % 4]
        if band == 0:
            pairs = int(PLAIN_STRIPE_PAIRS[(j // 4 * 3 + j % 4) % len(PLAIN_STRIPE_PAIRS)])
            k_lo = -(-TYPICAL_N[0] // (PAIR * pairs))  # (short stripes: n >= 2^16)
            k_hi = max(3, k_lo, min(256, TYPICAL_N[1] // (PAIR * pairs)))
            d["n"] = _stripe_n(rng, pairs, max(2, k_lo), k_hi, d["last"])
        else:
            pairs = 1
            lo, hi = K_BANDS[band]
            d["n"] = _stripe_n(rng, pairs, lo, min(hi, lo + 60), d["last"])
        d["dist"] = ("bits", "bits_dup")[int(rng.integers(0, 2))]
        d["hook"] = _hook(balanced_min_n=1, stripe_min_n=1, stripe_pairs=pairs,
                          first_bits=(7, 8, 9, 0)[(j // 4) % 4])
        _promise_stripes(d, True)
    elif cls == "stripes-pieces":
        d["kind"], d["up"] = COMBOS[j % 12]
        _shape(d, rng, ("soa", "soa", "pair", "soa", "aos16", "soa")[j % 6])
        pairs, length = PIECES_STRIPE_PAIRS, PAIR * PIECES_STRIPE_PAIRS
        # The sample must find the keys spread: no top-9-bit bin above n / 128,
        # so no bucket above n / 64. A hot bucket holds up to 12289 records,
        # the one with a full stripe 16384: n >= 1.3 M with it (even cases).
        # The odd cases stay under 2^20: their whole-stripe piece is the
        # last stripe, of 8194 .. 12000 records.
        if j % 2 == 0:
            d["last"] = LAST_STRIPES[j // 2 % 3]
            d["n"] = _stripe_n(rng, pairs, 80, 122, d["last"])
        else:
            d["last"] = "whole"
            d["n"] = int(rng.integers(57, 64)) * length + int(rng.integers(PAIR + 2, 12001))
        full = (d["n"] - 1) // length if d["last"] != "full" else d["n"] // length
        d["hot"] = [int(b) for b in 1 + rng.choice(254, len(HOT_PIECES), replace=False)]
        # the first or the last bucket among them (not with float keys: those
        # buckets hold the NaN patterns, which _finite moves into one half)
        if j % 3 == 0 and not is_float(d["kind"]):
            d["hot"][int(rng.integers(0, len(HOT_PIECES)))] = (0, 255)[j // 3 % 2]
        count = sum(len(p) for p in HOT_PIECES)
        stripes = rng.choice(full, count, replace=False)  # one special piece per stripe
        d["pieces"], at = [], 0
        for b, sizes in zip(d["hot"], HOT_PIECES):
            for size in sizes:
                piece = (int(stripes[at]), b, length if size < 0 else size)
                if size < 0 and d["last"] == "whole":
                    piece = (full, b, d["n"] - full * length)
                d["pieces"].append(piece)
                at += 1
        d["low_bits"] = int(rng.choice([14, key_bits(d["kind"]) - 8]))  # 14: duplicate keys
        d["dist"] = "pieces"
        d["hook"] = _hook(balanced_min_n=1, stripe_min_n=1, stripe_pairs=pairs, first_bits=8)
        _promise_stripes(d, True)
    elif cls == "stripes-balanced":
        d["kind"], d["up"] = COMBOS[j % 12]
        _shape(d, rng, ("soa", "pair", "soa", "soa")[j % 4])
        if is_float(d["kind"]):
            d["dist"] = ("grid", "head_tail")[(j // 12) % 2]
        else:
            d["dist"] = ("head_tail", "gauss", "head_tail", "heavy_gauss")[(j // 12 + j) % 4]
        if d["dist"] in ("grid", "head_tail"):
            d["table"] = ("1", "3", None)[(j // 2) % 3]
        d["last"] = LAST_STRIPES[j % 4]
        if j % 10 == 9:  # more than 256 stripes
            pairs = 1
            d["n"] = _stripe_n(rng, pairs, 257, 300, d["last"])
        else:  # 2^18 .. 2^20 records (the planner wants a few hundred keys per group)
            pairs = int(rng.choice([1, 2, 4, 8, 16]))
            k_lo = max(3, -(-(1 << 18) // (PAIR * pairs)))
            d["n"] = _stripe_n(rng, pairs, k_lo, max(k_lo, TYPICAL_N[1] // (PAIR * pairs)),
                               d["last"])
        d["hook"] = _hook(balanced_min_n=1, stripe_min_n=1, stripe_pairs=pairs)
        _promise_stripes(d, False)
        if d["table"]:  # (tests/test_level_fuzz_plan.py: the planner takes the forced kind)
            d["promise"]["kind"] = int(d["table"])
    else:
        sub = d["declined"] = DECLINED[j % 5]
        d["up"] = bool(rng.integers(0, 2))
        d["kind"] = WIDE_KINDS[(j // 5) % 6]
        if sub == "canon":
            d["kind"] = (8, 9)[(j // 5) % 2]
            d["thresh"] = 1 << 23
        elif sub == "ranges_final":
            d["kind"] = (4, 5, 6, 7)[(j // 5) % 4]
        elif sub == "two_byte":
            d["kind"] = (2, 3)[(j // 5) % 2]
        _shape(d, rng, "soa")
        d["n"] = log_uniform(rng, TYPICAL_N[0], 1 << 19)
        if sub == "segments":
            d["inplace"] = True  # (the segment sort has no `out`)
            n = d["n"]
            cuts = sorted(int(x) for x in rng.integers(0, n + 1, int(rng.integers(0, 4))))
            d["bounds"] = [0, n] if j % 2 == 0 else [int(rng.integers(0, 40))] + cuts + \
                [n - int(rng.integers(0, 40))]
            d["bounds"] = sorted(d["bounds"])
        d["dist"] = {"equal": "equal", "canon": "bits_zeros", "segments": "bits",
                     "ranges_final": "narrow_gauss", "two_byte": "full"}[sub]
        d["hook"] = _hook(balanced_min_n=1, stripe_min_n=1, stripe_pairs=int(rng.integers(1, 3)),
                          first_bits=(8, 0)[j % 2])
        d["promise"] = {"stripes": 0}
    return d


# --------------------------------------------------------------------------
# arrays
# --------------------------------------------------------------------------
def _finite(kind: int, keys: np.ndarray) -> np.ndarray:
    """float keys whose pattern is an infinity or a NaN lose their lowest
    exponent bit (the top byte of the key stays)"""
    if not is_float(kind):
        return keys
    mant = 23 if keys.dtype.itemsize == 4 else 52
    bits = keys.view(KIND_UINT[kind]).copy()
    bad = ~np.isfinite(keys)
    bits[bad] &= ~bits.dtype.type(1 << mant)
    return bits.view(keys.dtype)


def _from_u(d: dict, u: np.ndarray) -> np.ndarray:
    return _finite(d["kind"], untransformed(d["kind"], d["up"], u))


def _rand_u(rng, bits: int, n: int) -> np.ndarray:
    if bits < 64:
        return rng.integers(0, 1 << bits, n, dtype=np.uint64)
    return rng.integers(0, 1 << 63, n, dtype=np.uint64) * np.uint64(2) + \
        rng.integers(0, 2, n, dtype=np.uint64)


def _sprinkle(keys: np.ndarray, rng, values: np.ndarray, share: float) -> np.ndarray:
    hit = rng.random(len(keys)) < share
    keys = keys.copy()
    keys[hit] = values[rng.integers(0, len(values), int(hit.sum()))]
    return keys


def piece_counts(d: dict) -> np.ndarray:
    """stripes-pieces: the (stripes, 256) table of piece sizes"""
    n, length = d["n"], PAIR * d["hook"]["stripe_pairs"]
    k = stripe_count(n, d["hook"]["stripe_pairs"])
    lens = np.full(k, length, np.int64)
    lens[-1] = n - (k - 1) * length
    c = np.zeros((k, 256), np.int64)
    for s, b, size in d["pieces"]:
        c[s, b] = size
    rng = np.random.default_rng([d["seed"], 3])
    cold = np.setdiff1d(np.arange(256), d["hot"])
    for s in range(k):
        rest = int(lens[s] - c[s].sum())
        c[s, cold] = rng.multinomial(rest, np.full(len(cold), 1.0 / len(cold)))
    assert np.array_equal(c.sum(axis=1), lens)
    return c


def _pieces_keys(d: dict, rng) -> np.ndarray:
    kb, n = key_bits(d["kind"]), d["n"]
    c = piece_counts(d)
    k = len(c)
    digit = np.repeat(np.tile(np.arange(256, dtype=np.uint64), k), c.ravel())
    stripe = np.repeat(np.arange(k), c.sum(axis=1))
    low = _rand_u(rng, d["low_bits"], n) << np.uint64(kb - 8 - d["low_bits"])
    shuffle = stripe + rng.random(n)
    whole = [s for s, _, size in d["pieces"] if size == c[s].sum()]
    for s in whole:  # a stripe that is one piece: sorted keys
        sl = slice(int(np.searchsorted(stripe, s)), int(np.searchsorted(stripe, s, "right")))
        low[sl] = np.sort(low[sl])
        shuffle[sl] = s + np.linspace(0, 0.5, sl.stop - sl.start)
    order = np.argsort(shuffle, kind="stable")  # shuffled inside each stripe
    return _from_u(d, ((digit << np.uint64(kb - 8)) | low)[order])


def make_keys(d: dict) -> np.ndarray:
    kind, n, dist = d["kind"], d["n"], d["dist"]
    rng = np.random.default_rng([d["seed"], 1])
    dt = np.dtype(KIND_DTYPES[kind])
    kb = key_bits(kind)
    if dist == "pieces":
        return _pieces_keys(d, rng)
    if dist in ("bits", "bits_dup", "bits_zeros"):  # uniform transformed bits
        u = _rand_u(rng, kb, n)
        if dist == "bits_dup":  # a random top 16 bits, four values below: duplicates
            u = (u >> np.uint64(kb - 16) << np.uint64(kb - 16)) | (u & np.uint64(3))
        keys = _from_u(d, u)
        if is_float(kind):  # +-inf, +-0.0, denormals, ... at two percent
            share = 0.3 if dist == "bits_zeros" else 0.02
            keys = _sprinkle(keys, rng, float_specials(dt, 4096, rng), share)
        return keys
    if dist == "equal":
        return _from_u(d, np.full(n, int(_rand_u(rng, kb - 1, 1)[0]), np.uint64))
    if dist == "grid":  # C2's keys: multiples of 2^-23 in [-1, 1)
        return (rng.integers(0, 1 << 24, n) * 2.0 ** -23 - 1.0).astype(dt)
    if dist == "head_tail":  # most keys in four top-9-bit bins, the rest over a few dozen
        bins = int(rng.integers(16, 129))
        first = int(rng.integers(0, 512 - bins))
        b = rng.integers(first, first + bins, n).astype(np.uint64)
        head = rng.random(n) < rng.uniform(0.5, 0.7)
        at = int(rng.integers(first, first + bins - 4))
        b[head] = rng.integers(at, at + 4, int(head.sum())).astype(np.uint64)
        return _from_u(d, (b << np.uint64(kb - 9)) | _rand_u(rng, kb - 9, n))
    if dist in ("gauss", "narrow_gauss", "heavy_gauss"):  # gaussian integers
        wide = [3e3, 1e5, 3e5] + ([1e12] if kb == 64 else [])
        sigma = 40.0 if dist == "narrow_gauss" else float(rng.choice(wide))
        v = np.rint(rng.standard_normal(n) * sigma).astype(np.int64)
        if dist == "heavy_gauss":  # one value holds a third of the keys
            v[rng.random(n) < 0.33] = 7
        return v.astype(dt)  # (unsigned kinds: two clusters, at both ends)
    return gen_keys(kind, n, dist, rng)


def make_arrays(d: dict) -> dict:
    """{"cols": [keys, payloads..., position]} or, AoS, {"records": (n,
    elem_size) uint8 with the key at offset 0 and, where it fits, the record's
    position in the last four bytes, "keys": the keys}."""
    keys = make_keys(d)
    n = d["n"]
    rng = np.random.default_rng([d["seed"], 2])
    position = np.arange(n, dtype=np.uint32)
    if d["shape"] == "aos":
        es, ks = d["elem_size"], keys.dtype.itemsize
        rec = rng.integers(0, 256, (n, es), dtype=np.uint8)
        rec[:, :ks] = keys.view(np.uint8).reshape(n, ks)
        if es - ks >= 4:
            rec[:, es - 4:] = position.view(np.uint8).reshape(n, 4)
        return {"records": rec, "keys": keys}
    pays = [rng.integers(0, 1 << (8 * w), n, dtype=np.uint64).astype(f"u{w}") for w in d["widths"]]
    return {"cols": [keys] + pays + [position]}


def make_case(case: int):
    d = describe(case)
    return d, make_arrays(d)


def reference(d: dict, arrays: dict) -> list:
    """The stable sort of the case: its columns (AoS: [records]) in order.
    Segments: every segment on its own, the rest untouched. n <= thresh with
    float keys: -0.0 == +0.0, as the sort's canon-zero mode compares."""
    keys = arrays["keys"] if d["shape"] == "aos" else arrays["cols"][0]
    u = transformed_keys(d["kind"], d["up"], keys)
    if is_float(d["kind"]) and d["n"] <= d["thresh"]:
        zero = transformed_keys(d["kind"], d["up"], np.zeros(1, keys.dtype))[0]
        u = np.where(keys == 0, zero, u)
    if d["bounds"] is None:
        order = np.argsort(u, kind="stable")
    else:
        order = np.arange(d["n"])
        for a, b in zip(d["bounds"][:-1], d["bounds"][1:]):
            order[a:b] = a + np.argsort(u[a:b], kind="stable")
    cols = [arrays["records"]] if d["shape"] == "aos" else arrays["cols"]
    return [c[order] for c in cols]


# --------------------------------------------------------------------------
# what the driver's key sample decides (plan_balanced_level, find_clusters)
# --------------------------------------------------------------------------
def sample_hist16(d: dict, keys: np.ndarray) -> np.ndarray:
    """The 65536-bin histogram of the top 16 transformed bits of the sort's
    sample: chunks of 1024 keys at a stride of n / chunks."""
    n = d["n"]
    blocks = min(SAMPLE_MAX_CHUNKS, n // SAMPLE_CHUNK)
    stride = n // blocks
    idx = (np.arange(blocks)[:, None] * stride + np.arange(SAMPLE_CHUNK)[None, :]).ravel()
    u = transformed_keys(d["kind"], d["up"], keys[idx])
    return np.bincount((u >> np.uint64(key_bits(d["kind"]) - 16)).astype(np.int64),
                       minlength=65536).astype(np.uint32)


def find_clusters(h: np.ndarray):
    """srs_plan.hip find_clusters: the clusters [(first bin, last bin)] when
    the non-empty bins form at most four groups of fewer than 256 bins, else
    None."""
    cl = []
    for b in np.flatnonzero(h):
        if not cl or b - cl[-1][1] > CLUSTER_GAP:
            cl.append([int(b), int(b)])
        cl[-1][1] = int(b)
        if len(cl) > MAX_RANGES or cl[-1][1] - cl[-1][0] >= CLUSTER_SPAN:
            return None
    return [tuple(c) for c in cl]


def is_spread(h: np.ndarray) -> bool:
    """no top-9-bit bin of the sample above kBalancedSkew times its share"""
    top9 = h.astype(np.int64).reshape(512, 128).sum(axis=1)
    return int(top9.max()) * 512 <= BALANCED_SKEW * int(top9.sum())


def describe_text(d: dict) -> str:
    return (f"case {d['case']} {d['cls']} {KIND_NAMES[d['kind']]} {'up' if d['up'] else 'down'} "
            f"n={d['n']} {d['shape']} {d['dist']} hook={d['hook']}")
