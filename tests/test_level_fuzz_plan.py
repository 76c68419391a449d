"""Coverage of the seeded plan of the level fuzz (tests/srs_level_fuzzlib.py),
checked without a GPU: over the committed case count the descriptions reach
the combinations tests/test_gpu_fuzz_levels.py exists for, and the keys of
every stripes case make the driver's key sample decide what the case promises
(the sample is rebuilt here as tests/test_table_plan.py rebuilds C2's; the
digit table comes from the library's own planner, srs_debug_plan_table, host
only). Run with -s to see the coverage table."""
import ctypes

import numpy as np
import pytest

import srs_amd
import srs_level_fuzzlib as lz
from srs_fuzzlib import is_float, key_bits
from srs_testlib import KIND_NAMES


def plan_table_mode(hist, n, bits):
    """srs_debug_plan_table's table kind (0 none, 1 the 16-bit table, 3 the
    split table) for a sample histogram; SRS_TABLE forces the kind."""
    f = srs_amd.lib().srs_debug_plan_table
    f.argtypes = [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.POINTER(ctypes.c_int32),
                  ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_double),
                  ctypes.POINTER(ctypes.c_double), ctypes.c_void_p, ctypes.c_void_p]
    h = np.ascontiguousarray(hist, dtype=np.uint32)
    table, rbits = np.zeros(65536, np.int32), np.zeros(512, np.int32)
    mode = ctypes.c_int32()
    rc = f(h.ctypes.data, n, bits, ctypes.byref(mode), None, None, None, table.ctypes.data,
           rbits.ctypes.data)
    assert rc == 0, srs_amd.lib().srs_last_error()
    return mode.value


@pytest.fixture(scope="module")
def plan():
    return [lz.describe(i) for i in range(lz.N_CASES)]


@pytest.fixture(scope="module")
def samples(plan):
    """case -> the sample histogram of a stripes case's keys: every
    stripes-balanced case; of stripes-plain, whose keys are uniform bits
    whatever n is, the cases up to 2^20 records and a quarter of the larger
    ones; every second stripes-pieces case (their hot buckets are sized by one
    rule)"""
    def wanted(d):
        if d["cls"] == "stripes-plain":
            return d["n"] <= 1 << 20 or d["index"] % 8 in (2, 7)
        return d["cls"] == "stripes-balanced" or (d["cls"] == "stripes-pieces" and
                                                  d["index"] % 2 == 0)
    return {d["case"]: lz.sample_hist16(d, lz.make_keys(d)) for d in plan if wanted(d)}


def _count(cases, pred):
    return sum(bool(pred(d)) for d in cases)


def _table(title, rows):
    print("\n" + title)
    for name, value in rows:
        print(f"  {name:<44} {value}")


def _stripes(plan):
    return [d for d in plan if d["cls"] in lz.STRIPE_CLASSES]


def test_case_count_and_sizes(plan):
    assert 150 <= lz.N_CASES <= 200 and len(plan) == lz.N_CASES
    per_class = {c: _count(plan, lambda d: d["cls"] == c) for c in lz.CLASSES}
    sizes = sorted(d["n"] for d in plan)
    lo, hi = lz.TYPICAL_N
    assert (lo, hi) == (1 << 16, 1 << 20)
    typical = _count(plan, lambda d: lo <= d["n"] <= hi)
    below = {c: _count(plan, lambda d: d["cls"] == c and d["n"] < lo) for c in lz.CLASSES}
    above = {c: _count(plan, lambda d: d["cls"] == c and d["n"] > hi) for c in lz.CLASSES}
    _table("level fuzz plan", [("cases per class", per_class),
                               ("n: min / median / max", (sizes[0], sizes[len(sizes) // 2],
                                                          sizes[-1])),
                               ("2^16 <= n <= 2^20", typical),
                               ("n < 2^16 per class", below), ("n > 2^20 per class", above),
                               ("records in all", sum(sizes))])
    assert all(v >= 20 for v in per_class.values()), per_class
    assert sizes[0] > lz.LOCAL_CAP and sizes[-1] <= lz.MAX_RECORDS
    assert 2 * typical > lz.N_CASES
    # above 2^20 only where a case needs it: more than 256 stripes of one tile
    # pair, two stripes of the planner's longer lengths, a full stripe as one
    # piece of a spread bucket, every sixth general case
    for d in plan:
        if d["n"] > hi and d["cls"] != "general":
            assert d["cls"] in lz.STRIPE_CLASSES, d
            assert (d["promise"]["stripe_count"] > 256 or d["hook"]["stripe_pairs"] >= 61 or
                    (d["cls"] == "stripes-pieces" and d["last"] != "whole")), d
    for d in plan:
        h = d["hook"]
        assert h["general_min_n"] == 1 and 0 <= h["stripe_pairs"] <= lz.MAX_STRIPE_PAIRS
        assert 0 <= h["first_bits"] <= 9
        if d["cls"] in lz.STRIPE_CLASSES:  # the hook's own conditions for a stripe level
            assert h["stripe_min_n"] == 1 and h["balanced_min_n"] == 1
            assert d["n"] >= 2 * lz.PAIR * h["stripe_pairs"], d
            assert d["promise"]["stripe_count"] >= 2


def test_key_kinds_and_directions(plan):
    print("\ncases per (class, key kind): ascending / descending")
    for cls in lz.CLASSES:
        seen = np.zeros((10, 2), int)
        for d in plan:
            if d["cls"] == cls:
                seen[d["kind"], int(d["up"])] += 1
        print(f"{cls:>17} " + " ".join(f"{KIND_NAMES[k]}:{seen[k, 1]}/{seen[k, 0]}"
                                       for k in range(10)))
        if cls in lz.STRIPE_CLASSES:
            assert np.all(seen[list(lz.WIDE_KINDS)] > 0), (cls, seen)
            assert seen[:4].sum() == 0
        if cls == "general":  # every kind, the 1- and 2-byte ones included
            assert np.all(seen.sum(axis=1) > 0), seen
    declined = {s: _count(plan, lambda d: d.get("declined") == s) for s in lz.DECLINED}
    _table("declined", [("cases per reason", declined)])
    assert all(v >= 4 for v in declined.values()), declined
    two_byte = [d for d in plan if d.get("declined") == "two_byte"]
    assert {d["kind"] for d in two_byte} == {2, 3}
    assert all(is_float(d["kind"]) and d["n"] <= d["thresh"]
               for d in plan if d.get("declined") == "canon")


def test_stripe_counts_and_last_stripes(plan):
    st = _stripes(plan)
    bands = [_count(st, lambda d: lz.k_band(d["promise"]["stripe_count"]) == b) for b in range(3)]
    wide8 = _count(st, lambda d: d["promise"]["stripe_count"] > 512 and key_bits(d["kind"]) == 64)
    last = {m: _count(st, lambda d: d["last"] == m) for m in lz.LAST_STRIPES + ("whole",)}
    pairs = sorted({d["hook"]["stripe_pairs"] for d in st})
    plain = [d for d in st if d["cls"] == "stripes-plain"]
    # the forced digit width (0: chosen from n) against the stripe-count band
    bits = np.zeros((4, 3), int)
    for d in plain:
        bits[(7, 8, 9, 0).index(d["hook"]["first_bits"]),
             lz.k_band(d["promise"]["stripe_count"])] += 1
    chosen = sorted({d["promise"]["first_bits"] for d in plain if d["hook"]["first_bits"] == 0})
    chosen_long = _count(plain, lambda d: d["hook"]["first_bits"] == 0 and
                         d["hook"]["stripe_pairs"] > 1)
    _table("stripes", [("K <= 256 / 257-513 / >= 514", bands),
                       ("K >= 514 with 8-byte keys", wide8),
                       ("last stripe", last), ("stripe lengths in tile pairs", pairs),
                       ("plain: first_bits 7 / 8 / 9 / chosen per band",
                        bits.tolist()),
                       ("plain: widths chosen from n", chosen),
                       ("plain: chosen width, stripes over one pair", chosen_long)])
    assert all(b >= 8 for b in bands), bands
    assert wide8 >= 3
    # (the issue's third band is K > 512; stripe_order_kernel's second trip
    # needs K >= 514, so no case stops at 513)
    assert not any(d["promise"]["stripe_count"] == 513 for d in st)
    assert all(last[m] >= 8 for m in ("full", "one", "subtile")), last
    assert {1, 61, 122, 244} <= set(pairs)
    assert np.all(bits > 0), bits  # every width in every band
    assert len(chosen) >= 3 and chosen_long >= 3
    for d in st:
        n, length = d["n"], lz.PAIR * d["hook"]["stripe_pairs"]
        tail = n - (d["promise"]["stripe_count"] - 1) * length
        assert 1 <= tail <= length
        assert {"full": tail == length, "one": tail == 1, "subtile": 2 <= tail < lz.TILE,
                "whole": lz.PAIR < tail < length, "free": True}[d["last"]], d


def test_shapes_payloads_and_pair_tiles(plan):
    st = _stripes(plan)
    gen = [d for d in plan if d["cls"] == "general"]
    widths = {w: _count(plan, lambda d: w in d["widths"]) for w in (1, 2, 4, 8)}
    ncols = {c: _count(plan, lambda d: d["shape"] == "soa" and len(d["widths"]) == c)
             for c in range(4)}
    shapes = {}
    for name, cases in (("general", gen), ("stripes", st)):
        shapes[name] = {"pair": _count(cases, lambda d: d["shape"] == "pair")}
        for es in (8, 16, 32, 64):
            shapes[name][f"aos{es}"] = _count(cases, lambda d: d["elem_size"] == es)
    modes = {name: {m: _count(cases, lambda d: d["pair_tiles"] == m) for m in (None, 1, 2, 3)}
             for name, cases in (("general", gen), ("stripes", st))}
    places = [_count(plan, lambda d: d["inplace"] == p) for p in (True, False)]
    _table("shapes", [("payload widths 1/2/4/8", widths), ("SoA payload columns 0-3", ncols),
                      ("general", shapes["general"]), ("stripes", shapes["stripes"]),
                      ("SRS_PAIR_TILES in general", modes["general"]),
                      ("SRS_PAIR_TILES in stripes", modes["stripes"]),
                      ("in place / out of place", places)])
    assert all(widths.values()) and all(ncols.values())
    assert all(shapes["general"].values()), shapes
    assert shapes["stripes"]["pair"] and shapes["stripes"]["aos16"] and shapes["stripes"]["aos32"]
    for name in modes:
        assert all(modes[name][m] for m in (1, 2, 3)), modes
    assert min(places) >= 20


def test_exact_piece_sizes(plan):
    cases = [d for d in plan if d["cls"] == "stripes-pieces"]
    seen = {s: 0 for s in lz.PIECE_SIZES}
    whole = mixed = 0
    for d in cases:
        c = lz.piece_counts(d)
        length = lz.PAIR * d["hook"]["stripe_pairs"]
        hot = c[:, d["hot"]]
        for s in lz.PIECE_SIZES:
            seen[s] += bool((hot == s).any())
        whole += bool((hot == c.sum(axis=1)[:, None]).any())
        assert (d["last"] == "whole") == (d["n"] <= lz.TYPICAL_N[1])
        assert (hot == length).any() == (d["last"] != "whole")  # (a full stripe as one piece)
        # full and empty pieces side by side in one bucket
        mixed += bool(((hot == 0).any(axis=0) & (hot >= lz.TILE).any(axis=0)).any())
        assert d["hook"]["first_bits"] == 8 and np.all((c > 0).any(axis=0)), d
        for s, b, size in d["pieces"]:
            assert c[s, b] == size
    _table("stripes-pieces", [("cases with a piece of each size", seen),
                              ("with a piece that is a whole stripe", whole),
                              ("full beside empty pieces in a bucket", mixed)])
    assert all(v >= 5 for v in seen.values()), seen
    assert whole >= 5 and mixed >= 5


def test_pieces_keys_have_the_promised_counts(plan):
    """the keys of a stripes-pieces case, cut into its stripes and counted by
    their top transformed byte, give the case's table of piece sizes"""
    done = 0
    for d in plan:
        if d["cls"] != "stripes-pieces" or d["index"] % 8 not in (0, 3):
            continue
        done += 1
        keys = lz.make_keys(d)
        u = lz.transformed_keys(d["kind"], d["up"], keys)
        top = (u >> np.uint64(key_bits(d["kind"]) - 8)).astype(np.int64)
        length = lz.PAIR * d["hook"]["stripe_pairs"]
        c = lz.piece_counts(d)
        for s in {p[0] for p in d["pieces"]} | {0, len(c) - 1}:
            got = np.bincount(top[s * length:(s + 1) * length], minlength=256)
            assert np.array_equal(got, c[s]), (d["case"], s)
        s = next(p[0] for p in d["pieces"] if p[2] == c[p[0]].sum())
        assert np.all(np.diff(u[s * length:(s + 1) * length].astype(np.float64)) >= 0)
        if is_float(d["kind"]):
            assert np.isfinite(keys).all()
    assert done >= 4


def test_sample_decides_what_the_cases_promise(plan, samples, monkeypatch):
    """stripes-plain and stripes-pieces: the sample's top 9 bits are spread
    and its bins are no clusters, so the plain digit runs in stripes.
    stripes-balanced: clusters (a range level, find_clusters' rule) or, when
    not spread, the planner's table with the case's n and forced kind."""
    plain_ok = 0
    taken = {"1": 0, "3": 0, None: 0}
    ranges = 0
    for d in plan:
        if d["case"] not in samples:
            continue
        h = samples[d["case"]]
        clusters = lz.find_clusters(h)
        if d["promise"]["kind_zero"]:
            assert clusters is None and lz.is_spread(h), lz.describe_text(d)
            plain_ok += 1
            continue
        if d["dist"] in ("gauss", "heavy_gauss"):
            assert clusters is not None, lz.describe_text(d)
            ranges += 1
            continue
        assert clusters is None and not lz.is_spread(h), lz.describe_text(d)
        if d["table"] is None:
            monkeypatch.delenv("SRS_TABLE", raising=False)
        else:
            monkeypatch.setenv("SRS_TABLE", d["table"])
        mode = plan_table_mode(h, d["n"], key_bits(d["kind"]))
        assert mode in (1, 3), lz.describe_text(d)  # (0 would be a plain level: no stripes)
        # a forced kind is the kind the case promises (the GPU test asserts it)
        assert mode == d["promise"].get("kind", mode), lz.describe_text(d)
        assert ("kind" in d["promise"]) == (d["table"] is not None)
        taken[d["table"]] += 1
    _table("what the key sample decides", [("plain digit in stripes", plain_ok),
                                           ("range level (clusters)", ranges),
                                           ("forced table 1 / 3 taken, free", taken)])
    assert taken["1"] >= 8 and taken["3"] >= 8 and ranges >= 5


def test_declined_and_general_do_not_promise_stripes(plan):
    for d in plan:
        if d["cls"] in ("general", "declined"):
            assert d["promise"]["stripes"] == 0
        if d["cls"] == "general":
            assert d["hook"]["stripe_min_n"] == 0 and d["n"] < (1 << 24)
        if d.get("declined") == "segments":
            b = d["bounds"]
            assert b == sorted(b) and b[0] >= 0 and b[-1] <= d["n"] and d["inplace"]
    narrow = [d for d in plan if d.get("declined") == "ranges_final"]
    for d in narrow[:2]:  # at most 512 key values: every bucket of the range level holds one
        assert len(np.unique(lz.make_keys(d))) <= 512
    equal = [d for d in plan if d.get("declined") == "equal"]
    assert all(len(np.unique(lz.make_keys(d))) == 1 for d in equal[:2])


def test_no_nan_is_generated(plan):
    done = 0
    for d in plan:
        if is_float(d["kind"]) and d["index"] % 3 == 0:
            assert not np.isnan(lz.make_keys(d)).any(), lz.describe_text(d)
            done += 1
    assert done >= 8


def test_generation_is_deterministic():
    for case in (0, 40, 90, 120, 160):
        (d1, a1), (d2, a2) = lz.make_case(case), lz.make_case(case)
        assert d1 == d2 and a1.keys() == a2.keys()
        for key in a1:
            xs, ys = (a1[key], a2[key]) if isinstance(a1[key], list) else ([a1[key]], [a2[key]])
            for p, q in zip(xs, ys):
                assert p.dtype == q.dtype and p.tobytes() == q.tobytes()
        want = lz.reference(d1, a1)
        keys = want[0][:, :a1["keys"].dtype.itemsize].copy().view(a1["keys"].dtype).ravel() \
            if d1["shape"] == "aos" else want[0]
        if d1["bounds"] is None and d1["n"] > d1["thresh"]:
            u = lz.transformed_keys(d1["kind"], d1["up"], keys)
            assert np.all(u[1:] >= u[:-1])
