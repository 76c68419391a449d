"""Coverage of the seeded fuzz plan (tests/srs_fuzzlib.py), checked without a
GPU: over the committed case counts the generated cases reach the
combinations tests/test_gpu_fuzz_select.py exists for. Everything is read
from the descriptions, and, for the select passes of the row-wise top-k, from
the keys. Run with -s to see the coverage table."""
import numpy as np
import pytest

import srs_fuzzlib as fz
from srs_testlib import KIND_NAMES, transformed_keys

ROW_CLASSES = ["[1,256]", "(256,1024]", "(1024,2048]", "(2048,4096]", "(4096,8192]", ">8192"]


@pytest.fixture(scope="module")
def plan():
    return {api: [fz.make_case(api, i) for i in range(fz.N_CASES[api])] for api in fz.APIS}


@pytest.fixture(scope="module")
def passes(plan):
    """topk_rows: case -> srs_fuzzlib.topk_rows_passes"""
    return {d["case"]: fz.topk_rows_passes(d) for d in plan["topk_rows"]}


def test_kinds_reach_every_length_class(plan):
    """Row-wise top-k on the resident route (forced or by the library's rule):
    every key kind in each of the five resident length classes; streamed:
    every key kind with row_len > 8192."""
    seen = np.zeros((10, 6), int)
    for d in plan["topk_rows"]:
        route, cls = fz.topk_rows_route(d), fz.length_class(d["row_len"])
        if (cls < 5 and route == fz.RESIDENT) or (cls == 5 and route == fz.STREAM):
            seen[d["kind"], cls] += 1
    print("\ntopk_rows cases per (key kind, length class), resident / stream route")
    print("      " + " ".join(f"{c:>12}" for c in ROW_CLASSES))
    for kind in range(10):
        print(f"{KIND_NAMES[kind]:>5} " + " ".join(f"{v:12d}" for v in seen[kind]))
    missing = [(KIND_NAMES[k], ROW_CLASSES[c]) for k in range(10) for c in range(6)
               if seen[k, c] == 0]
    assert not missing, missing


def test_select_and_sort_whole_in_every_class(plan):
    """Both a selected row (row_len > max(2 kk, 256)) and a row sorted whole in
    every resident length class. A row of at most 256 records is never
    selected (the condition cannot hold), so the first class has sort-whole
    cases only; a streamed row is always selected (sorted whole it would need
    kk > 4096, above the stream route's TOPK_ROWS_MAX_K)."""
    sel = np.zeros((6, 2), int)
    for d in plan["topk_rows"]:
        if fz.topk_rows_route(d) != fz.LOOP:
            sel[fz.length_class(d["row_len"]), int(fz.topk_rows_select(d))] += 1
    print("\ntopk_rows cases per length class: sorted whole / selected")
    for c in range(6):
        print(f"{ROW_CLASSES[c]:>12} {sel[c, 0]:4d} {sel[c, 1]:4d}")
    assert sel[0, 1] == 0 and sel[0, 0] > 0
    assert np.all(sel[1:5] > 0), sel
    assert sel[5, 0] == 0 and sel[5, 1] > 0


def test_payload_widths_on_every_api(plan):
    print("\ncases per API with a payload of width 1, 2, 4, 8; with 8-12 columns")
    for api in fz.APIS:
        cnt = {w: sum(w in d["widths"] for d in plan[api]) for w in (1, 2, 4, 8)}
        many = sum(d["many"] for d in plan[api])
        print(f"{api:>10} {cnt[1]:4d} {cnt[2]:4d} {cnt[4]:4d} {cnt[8]:4d} {many:4d}")
        assert all(cnt.values()), (api, cnt)
        assert many >= 1, api
        for d in plan[api]:
            if d["many"]:
                assert 8 <= len(d["widths"]) <= 12
            assert d["position_column"] == (not d["indices"])


def test_select_passes(plan, passes):
    """At least 10 row-wise top-k cases must take >= 2 select passes, at least
    10 of them with a varying range that does not start on a multiple of 12
    bits, at least 5 on the resident route with 64-bit keys."""
    two = [c for c, p in passes.items() if p["two"]]
    unaligned = [c for c in two if passes[c]["unaligned"]]
    by = {d["case"]: d for d in plan["topk_rows"]}
    res64 = [c for c in two
             if fz.topk_rows_route(by[c]) == fz.RESIDENT and fz.key_bits(by[c]["kind"]) == 64]
    stream = [c for c in two if fz.topk_rows_route(by[c]) == fz.STREAM]
    print(f"\ntopk_rows cases that must take >= 2 passes: {len(two)}; unaligned varying range: "
          f"{len(unaligned)}; resident with 64-bit keys: {len(res64)}; streamed: {len(stream)}")
    print("  tops:", sorted({(fz.key_bits(by[c]['kind']), passes[c]['top']) for c in unaligned}))
    assert tuple(two) == fz.two_pass_cases()
    assert len(two) >= 10 and len(unaligned) >= 10 and len(res64) >= 5
    assert len(stream) >= 1


def test_float_specials_on_every_api(plan):
    print("\ncases with float specials per API: f32 up/down, f64 up/down")
    for api in fz.APIS:
        cnt = {}
        for kind in (8, 9):
            for up in (True, False):
                cnt[kind, up] = sum(
                    d["kind"] == kind and d["up"] == up and
                    ("specials" in d["dist"] if isinstance(d["dist"], list)
                     else d["dist"] == "specials") for d in plan[api])
        print(f"{api:>10} " + " ".join(f"{v:4d}" for v in cnt.values()))
        assert all(cnt.values()), (api, cnt)


def test_specials_hold_what_they_promise():
    for kind in (8, 9):
        v = fz.gen_keys(kind, 20000, "specials", np.random.default_rng(kind))
        fi = np.finfo(v.dtype)
        assert not np.isnan(v).any()
        tiny = v.dtype.type(fi.tiny)
        for x in (np.inf, fi.smallest_subnormal, np.nextafter(tiny, v.dtype.type(0)), tiny,
                  fi.max):
            assert (v == x).any() and (v == -x).any(), x
        zero = v == 0
        assert (np.signbit(v) & zero).any() and (~np.signbit(v) & zero).any()


def test_every_forced_route(plan):
    forced = {d["route"] for d in plan["topk_rows"]}
    assert forced == {-1, fz.RESIDENT, fz.STREAM, fz.LOOP}, forced
    routes = set()
    for d in plan["sort_rows"]:
        routes.update(d["routes"])
        assert d["routes"][-1] == -1
    assert routes == {-1, fz.KERNEL, fz.LOCAL, fz.LEVELS}, routes
    print("\ntopk_rows cases per forced route (auto, resident, stream, loop):",
          [sum(d["route"] == r for d in plan["topk_rows"]) for r in (-1, 0, 1, 2)])
    for d in plan["topk_rows"]:  # a forced route is one the shape can take
        n, kk = d["row_len"], min(d["k"], d["row_len"])
        if d["route"] == fz.RESIDENT:
            assert n <= fz.LOCAL_CAP
        if d["route"] == fz.STREAM:
            assert n > fz.LOCAL_CAP and kk <= fz.TOPK_ROWS_MAX_K
        if d["route"] == fz.LOOP:
            assert d["rows"] <= 8


def test_shapes_stay_inside_their_limits(plan):
    for api in ("topk_rows", "sort_rows"):
        for d in plan[api]:
            assert 1 <= d["row_len"] <= 40000 and 1 <= d["rows"] <= 5000
            assert d["rows"] * d["row_len"] <= fz.ROWS_MAX_RECORDS
            assert d["stride"] - d["row_len"] in (0, 1, 3, 8, d["row_len"])
            assert 0 <= d["first"] <= 3
        assert any(d["rows"] > 300 for d in plan[api])
        assert any(isinstance(d["dist"], list) for d in plan[api])
    for d in plan["topk"]:
        assert 1 <= d["n"] <= fz.MAX_RECORDS and 1 <= d["k"] <= d["n"] + 5
    ks = [(d["k"], d["n"]) for d in plan["topk"]]
    assert any(2 * k > n for k, n in ks) and any(2 * k <= n for k, n in ks)
    assert any(k > 8192 for k, n in ks) and any(k <= 8192 < n for k, n in ks)
    assert {d["candidates"] for d in plan["topk"]} == {0, 4096, 16384}
    assert any(d["aos"] for d in plan["topk"])
    lens = np.concatenate([np.diff(d["bounds"]) for d in plan["segments"]])
    for d in plan["segments"]:
        b = d["bounds"]
        assert 2 <= d["n"] <= fz.MAX_RECORDS and 2 <= len(b) <= 3001
        assert b[0] >= 0 and b[-1] <= d["n"] and all(x <= y for x, y in zip(b, b[1:]))
        assert 0 <= d["known_top_bits"] < fz.key_bits(d["kind"])
    assert (lens == 0).any() and (lens > 8192).any()
    for edge in (4096, 8192):
        assert ((lens < edge) & (lens >= edge - 2)).any() and ((lens > edge) & (lens <= edge + 2)).any()
    assert any(d["bounds"][0] > 0 for d in plan["segments"])
    assert any(d["bounds"][-1] < d["n"] for d in plan["segments"])
    assert sum(d["known_top_bits"] > 0 for d in plan["segments"]) >= 10


def test_padding_and_known_top_bits():
    """The arrays keep what the descriptions say: the padding of a matrix
    holds the key that sorts first; a segment's keys share their top bits."""
    for api, case in (("topk_rows", 3), ("sort_rows", 5)):
        d = fz.make_case(api, case)
        a = fz.make_arrays(d)
        keys = a["flat"][0]
        mask = np.ones(len(keys), bool)
        mask[a["index"].ravel()] = False
        assert np.all(transformed_keys(d["kind"], d["up"], keys[mask]) == 0)
    done = 0
    for case in range(fz.N_CASES["segments"]):
        d = fz.make_case("segments", case)
        if not d["known_top_bits"] or done == 4:
            continue
        done += 1
        keys = fz.make_arrays(d)["cols"][0]
        u = transformed_keys(d["kind"], d["up"], keys) >> np.uint64(
            fz.key_bits(d["kind"]) - d["known_top_bits"])
        if fz.is_float(d["kind"]):
            assert not np.isnan(keys).any()
        for lo, hi in zip(d["bounds"], d["bounds"][1:]):
            assert hi == lo or np.all(u[lo:hi] == u[lo])
    assert done == 4


def test_no_nan_is_generated():
    for kind in (8, 9):
        for dist in fz.FLOAT_DISTS:
            assert not np.isnan(fz.gen_keys(kind, 5000, dist, np.random.default_rng(1))).any()


def test_untransformed_inverts_transformed_keys():
    rng = np.random.default_rng(0)
    for kind in range(10):
        u = rng.integers(0, 1 << fz.key_bits(kind), 1000, dtype=np.uint64) \
            if fz.key_bits(kind) < 64 else rng.integers(0, 1 << 64, 1000, dtype=np.uint64)
        for up in (True, False):
            assert np.array_equal(transformed_keys(kind, up, fz.untransformed(kind, up, u)), u)


def test_generation_is_deterministic():
    for api in fz.APIS:
        for case in (0, 1, 7, 41):
            d1, d2 = fz.make_case(api, case), fz.make_case(api, case)
            assert d1 == d2
            a1, a2 = fz.make_arrays(d1), fz.make_arrays(d2)
            assert a1.keys() == a2.keys()
            for key in a1:
                x, y = a1[key], a2[key]
                xs, ys = (x, y) if isinstance(x, list) else ([x], [y])
                assert len(xs) == len(ys)
                for p, q in zip(xs, ys):
                    assert p.dtype == q.dtype and p.tobytes() == q.tobytes()
