"""Coverage of the seeded fuzz plan of the multi-GPU side
(tests/srs_shard_fuzzlib.py), checked without a GPU: over the committed case
counts the generated cases reach the combinations
tests/test_gpu_fuzz_shard.py exists for. The histogram and the partition are
read from the descriptions (and the keys where a combination depends on
them); the shard sort from the library's own planner (srs_amd.shard.debug_plan,
host only, as in tests/test_dist.py) on every rank of every case. Run with -s
to see the coverage tables."""
import numpy as np
import pytest

import srs_shard_fuzzlib as sz
from srs_fuzzlib import FLOAT_DISTS, is_float, key_bits
from srs_testlib import KIND_NAMES

from srs_amd import shard


@pytest.fixture(scope="module")
def plan():
    return {api: [sz.make_case(api, i) for i in range(sz.N_CASES[api])] for api in sz.APIS}


@pytest.fixture(scope="module")
def shard_features(plan):
    """case -> srs_shard_fuzzlib.shard_features"""
    return {d["case"]: sz.shard_features(d, sz.shard_plans(d, sz.make_arrays(d), shard))
            for d in plan["shard"]}


def _count(cases, pred):
    return sum(bool(pred(d)) for d in cases)


def _table(title, rows):
    print("\n" + title)
    for name, value in rows:
        print(f"  {name:<42} {value}")


def test_every_kind_in_both_directions(plan):
    print("\ncases per (API, key kind): ascending / descending")
    for api in sz.APIS:
        seen = np.zeros((10, 2), int)
        for d in plan[api]:
            seen[d["kind"], int(d["up"])] += 1
        print(f"{api:>10} " + " ".join(f"{KIND_NAMES[k]}:{seen[k, 1]}/{seen[k, 0]}"
                                       for k in range(10)))
        assert np.all(seen > 0), (api, seen)


def test_key_hist_plan(plan):
    cases = plan["key_hist"]
    bits = {b: _count(cases, lambda d: d["bits"] == b) for b in range(1, sz.HIST_MAX_BITS + 1)}
    full8 = {k: _count(cases, lambda d: d["kind"] == k and d["bits"] == 8) for k in (0, 1)}
    second_trip = _count(cases, lambda d: d["n"] > sz.HIST_GRID_RECORDS)
    prefilled = _count(cases, lambda d: d["prefill"])
    twice = _count(cases, lambda d: d["twice"])
    _table("key_hist", [("cases per bits 1..12", list(bits.values())),
                        ("bits == 8 on u8 / i8", list(full8.values())),
                        ("n > 524288", second_trip), ("prefilled", prefilled), ("twice", twice),
                        ("n == 1", _count(cases, lambda d: d["n"] == 1)),
                        ("n in 255..257", _count(cases, lambda d: 255 <= d["n"] <= 257))])
    assert all(bits.values()), bits
    assert all(full8.values()), full8
    assert second_trip >= 5 and prefilled >= 10 and twice >= 10
    assert {255, 256, 257} & {d["n"] for d in cases} and any(d["n"] == 1 for d in cases)
    for d in cases:
        assert 1 <= d["bits"] <= min(sz.HIST_MAX_BITS, key_bits(d["kind"]))
        assert 1 <= d["n"] <= sz.HIST_MAX_RECORDS


def test_partition_plan(plan):
    cases = plan["partition"]
    bits = {b: _count(cases, lambda d: d["bits"] == b) for b in range(1, sz.PART_MAX_BITS + 1)}
    # the three ways the table is read, with every key width that admits it
    paths = np.zeros((3, 4), int)
    for d in cases:
        paths[sz.partition_path(d["bits"]), (8, 16, 32, 64).index(key_bits(d["kind"]))] += 1
    tables = {t: _count(cases, lambda d: d["table"] == t and d["n"] >= 2) for t in sz.TABLE_KINDS}
    aligned = [_count(cases, lambda d: d["table"] == "aligned" and d["n"] >= 2 and d["bare"] == b)
               for b in (False, True)]
    single_at = {p: _count(cases, lambda d: d["single_at"] == p and d["n"] >= 2)
                 for p in ("first", "middle", "last")}
    parts = {p: _count(cases, lambda d: d["num_parts"] == p) for p in (1, 2, 3, 511, 512)}
    above = _count(cases, lambda d: d["num_parts"] > (1 << d["bits"]))
    not_pow2 = _count(cases, lambda d: d["num_parts"] & (d["num_parts"] - 1))
    n_classes = {c: _count(cases, lambda d: d["n_class"] == c) for c in sz.PART_N_CLASSES}
    widths = {w: _count(cases, lambda d: w in d["widths"]) for w in (1, 2, 4, 8)}
    bare = _count(cases, lambda d: d["bare"])
    many = _count(cases, lambda d: d["many"])
    _table("partition", [("cases per bits 1..16", list(bits.values())),
                         ("scalar table x key width 8/16/32/64", list(paths[0])),
                         ("LDS table x key width", list(paths[1])),
                         ("global table x key width", list(paths[2])),
                         ("table kinds with n >= 2", tables),
                         ("aligned with / without a payload", aligned),
                         ("single at", single_at), ("num_parts", parts),
                         ("num_parts > 2^bits", above), ("num_parts no power of two", not_pow2),
                         ("n classes", n_classes), ("payload widths", widths),
                         ("no payload", bare), ("8-12 columns", many),
                         ("out_tail / stream", [_count(cases, lambda d: d["out_tail"]),
                                                _count(cases, lambda d: d["stream"])])])
    assert all(bits.values()), bits
    assert np.all(paths[:2] > 0) and np.all(paths[2, 1:] > 0) and paths[2, 0] == 0, paths
    assert all(v >= 10 for v in tables.values()), tables
    assert all(aligned), aligned
    assert all(single_at.values()), single_at
    assert all(parts.values()), parts
    assert above >= 1 and not_pow2 >= 1
    assert all(n_classes.values()), n_classes
    assert all(widths.values()) and bare >= 1 and many >= 1
    assert {d["out_tail"] for d in cases} == {False, True} == {d["stream"] for d in cases}
    for d in cases:
        kb = key_bits(d["kind"])
        assert 1 <= d["bits"] <= min(sz.PART_MAX_BITS, kb)
        assert 1 <= d["num_parts"] <= sz.PART_MAX_PARTS and 1 <= d["n"] <= sz.PART_MAX_RECORDS
        if d["many"]:
            assert 8 <= len(d["widths"]) <= 12
        assert d["position_column"] == (not d["bare"]) and (not d["bare"] or not d["widths"])
        if d["table"] == "aligned":
            fb = d["num_parts"].bit_length() - 1
            assert d["num_parts"] == 1 << fb and 1 <= fb <= d["bits"]


def test_partition_tables_and_single_group(plan):
    """Every table keeps its ids inside [0, num_parts) and is what its kind
    says; the one-group branch of run_partition is reached by a `single`
    table and by constant keys under a table that is not constant."""
    by_table, by_keys = 0, 0
    for d in plan["partition"]:
        a = sz.make_arrays(d)
        t = a["table"]
        assert t.dtype == np.int32 and len(t) == 1 << d["bits"]
        assert t.min() >= 0 and t.max() < d["num_parts"], d
        mono = bool(np.all(np.diff(t) >= 0))
        if d["table"] in ("aligned", "balanced", "monotone", "single"):
            assert mono, d
        if d["table"] == "arbitrary" and d["num_parts"] >= 2:
            assert not mono, d
        if d["table"] == "sparse":
            assert 4 * len(np.unique(t)) <= d["num_parts"], d
        if d["table"] == "aligned":
            fb = d["num_parts"].bit_length() - 1
            assert np.array_equal(t, np.arange(len(t)) >> (d["bits"] - fb))
        if d["n"] < 2:
            continue
        one_group = len(np.unique(sz.partition_dest(d, a))) == 1
        if d["table"] == "single":
            assert one_group and len(np.unique(t)) == 1
            by_table += 1
        elif one_group and d["dist"] == "const" and len(np.unique(t)) > 1:
            by_keys += 1
    print(f"\npartition cases with one group: by the table {by_table}, by constant keys under a "
          f"table that is not constant {by_keys}")
    assert by_table >= 1 and by_keys >= 1


def test_shard_plan(plan, shard_features):
    cases = plan["shard"]
    feats = {name: _count(cases, lambda d: shard_features[d["case"]][name])
             for name in ("one_record_chunk", "empty_chunk", "short_round", "idle_rank", "alias")}
    worlds = {w: _count(cases, lambda d: d["world"] == w) for w in sz.WORLDS}
    options = {rc: _count(cases, lambda d: (d["rounds"], d["chunks"]) == rc)
               for rc in sz.ROUNDS_CHUNKS}
    self_msgs = [_count(cases, lambda d: d["self_messages"] == s) for s in (False, True)]
    caps = {c: _count(cases, lambda d: d["max_message_bytes"] == c) for c in sz.MESSAGE_CAPS}
    groups256 = _count(cases, lambda d: key_bits(d["kind"]) == 8 and d["world"] == 8)
    sixteen = _count(cases, lambda d: key_bits(d["kind"]) == 16)
    widths = {w: _count(cases, lambda d: w in d["widths"]) for w in (1, 2, 4, 8)}
    bare = _count(cases, lambda d: d["bare"])
    many = _count(cases, lambda d: d["many"])
    shapes = {s: _count(cases, lambda d: d["shape"] == s) for s in ("all_empty", "one_rank")}
    per_rank = _count(cases, lambda d: isinstance(d["dist"], list))
    _table("shard", [("plan features", feats), ("world sizes", worlds),
                     ("(rounds, chunks)", options), ("self messages off / on", self_msgs),
                     ("message caps", caps), ("8-bit keys at world 8", groups256),
                     ("16-bit keys", sixteen), ("payload widths", widths), ("no payload", bare),
                     ("8-12 columns", many), ("shapes", shapes),
                     ("a distribution per rank", per_rank)])
    at_least_5 = [feats, worlds, options, caps, widths, shapes]
    for group in at_least_5:
        assert all(v >= 5 for v in group.values()), group
    assert min(self_msgs) >= 5 and groups256 >= 5 and sixteen >= 5 and bare >= 5
    assert many >= 1 and per_rank >= 1
    for d in cases:
        total = sum(d["ns"])
        assert len(d["ns"]) == d["world"] and total <= sz.SHARD_MAX_RECORDS
        assert d["max_message_bytes"] != 64 or total <= sz.SMALL_CAP_RECORDS
        if d["shape"] == "all_empty":
            assert total == 0
        if d["shape"] == "one_rank":
            assert sum(n > 0 for n in d["ns"]) == 1
        if d["many"]:
            assert 8 <= len(d["widths"]) <= 12
        assert d["position_column"] == (not d["bare"]) and (not d["bare"] or not d["widths"])
        if isinstance(d["dist"], list):
            assert len(d["dist"]) == d["world"]


def test_shard_positions_are_unique_across_ranks(plan):
    done = 0
    for d in plan["shard"]:
        if d["bare"] or d["world"] < 2 or sum(d["ns"]) == 0 or done == 6:
            continue
        done += 1
        pos = np.concatenate([cols[-1] for cols in sz.make_arrays(d)["ranks"]])
        assert pos.dtype == np.uint32 and np.array_equal(pos, np.arange(sum(d["ns"])))
    assert done == 6


def test_generation_is_deterministic():
    for api in sz.APIS:
        for case in (0, 1, 7, 41):
            d1, d2 = sz.make_case(api, case), sz.make_case(api, case)
            assert d1 == d2
            a1, a2 = sz.make_arrays(d1), sz.make_arrays(d2)
            assert a1.keys() == a2.keys()
            for key in a1:
                xs, ys = a1[key], a2[key]
                if key == "ranks":
                    xs, ys = [c for r in xs for c in r], [c for r in ys for c in r]
                elif not isinstance(xs, list):
                    xs, ys = [xs], [ys]
                assert len(xs) == len(ys)
                for p, q in zip(xs, ys):
                    assert p.dtype == q.dtype and p.tobytes() == q.tobytes()
    d = sz.make_case("key_hist", 1)
    assert np.array_equal(sz.prefill_counts(d), sz.prefill_counts(d))


def test_no_nan_is_generated(plan):
    for api in sz.APIS:
        dists = set()
        for d in plan[api]:
            if is_float(d["kind"]):
                dists.update(d["dist"] if isinstance(d["dist"], list) else [d["dist"]])
        assert dists <= set(FLOAT_DISTS)
    for api, key in (("key_hist", "keys"), ("partition", "cols"), ("shard", "ranks")):
        done = 0
        for d in plan[api]:
            if not is_float(d["kind"]) or done == 8:
                continue
            done += 1
            a = sz.make_arrays(d)[key]
            keys = [a] if key == "keys" else [a[0]] if key == "cols" else [r[0] for r in a]
            assert not any(np.isnan(k).any() for k in keys), d
        assert done == 8
