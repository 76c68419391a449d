"""What the ragged fuzz's fixed seeds reach, from the case descriptions alone
(tests/srs_ragged_fuzzlib.py; no GPU): the coverage condition of
tests/test_gpu_fuzz_ragged.py."""
import numpy as np

import srs_ragged_fuzzlib as rz

CASES = [rz.make_case(i) for i in range(rz.N_CASES)]


def test_case_count_and_size_cap():
    assert len(CASES) == 120
    for d in CASES:
        assert 0 < d["num"] <= rz.MAX_RECORDS, d["case"]
        assert d["num"] == d["head"] + sum(d["lengths"]) + d["tail"]
        assert all(x >= 0 for x in d["lengths"]) and len(d["lengths"]) >= 1


def test_descriptions_are_reproducible():
    assert rz.make_case(17) == rz.make_case(17)
    a, b = rz.make_arrays(CASES[17]), rz.make_arrays(CASES[17])
    assert all(np.array_equal(x.view(np.uint8), y.view(np.uint8))
               for x, y in zip(a["cols"], b["cols"]))
    assert np.array_equal(a["offsets"], b["offsets"])


def test_every_key_kind_direction_and_indices():
    assert {d["kind"] for d in CASES} == set(range(10))
    assert {d["up"] for d in CASES} == {True, False}
    assert {d["indices"] for d in CASES} == {True, False}
    floats = sum(d["kind"] >= 8 for d in CASES)
    assert floats > len(CASES) // 5  # (two kinds of ten, twice as likely: a third)


def test_every_length_law_and_short_max():
    assert {d["law"] for d in CASES} == set(rz.LENGTH_LAWS)
    assert {d["short_max"] for d in CASES} == set(rz.SHORT_MAXES)
    for law in rz.LENGTH_LAWS:  # every law under every short_max
        assert {d["short_max"] for d in CASES if d["law"] == law} == set(rz.SHORT_MAXES), law


def test_payload_counts():
    assert {len(d["widths"]) for d in CASES} == {0, 1, 2, 3}


def _any_len(pred):
    return any(any(pred(x) for x in d["lengths"]) for d in CASES)


def test_segment_length_classes_are_reached():
    assert _any_len(lambda x: x == 0)
    assert _any_len(lambda x: x == 1)
    assert _any_len(lambda x: 256 < x <= 4096)
    assert _any_len(lambda x: 4096 < x <= 8192)
    assert _any_len(lambda x: x > 8192)


def test_gaps_and_single_segment():
    assert any(d["head"] > 0 for d in CASES)
    assert any(d["tail"] > 0 for d in CASES)
    assert any(d["head"] == 0 and d["tail"] == 0 for d in CASES)
    assert any(len(d["lengths"]) == 1 for d in CASES)


def test_expectation_on_a_hand_made_input():
    """ragged_orders on three segments (one empty) with a gap on both sides"""
    keys = np.array([9, 3, 1, 2, 7, 7, 5, 0, 8], dtype=np.uint32)
    src, idx, lo, hi = rz.ragged_orders(4, True, keys, [1, 4, 4, 8])
    assert (lo, hi) == (1, 8)
    assert src.tolist() == [2, 3, 1, 7, 6, 4, 5]
    assert idx.tolist() == [1, 2, 0, 3, 2, 0, 1]
    src, idx, _, _ = rz.ragged_orders(4, False, keys, [1, 4, 4, 8])
    assert src.tolist() == [1, 3, 2, 4, 5, 6, 7]
    assert rz.class_counts([0, 1, 256, 257, 4096, 4097, 8192, 8193]) == (2, 2, 2, 1)
    assert rz.class_counts([0, 1, 256, 257], short_max=0) == (0, 3, 0, 0)
