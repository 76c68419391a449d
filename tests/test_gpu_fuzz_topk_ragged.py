"""Seeded differential fuzz of the ragged top-k (topk_ragged_device). The
first 60 cases of tests/srs_ragged_fuzzlib.py (its short_max is ignored) with
a k drawn log-uniform in 1 .. 4096 from a generator seeded by the case number;
every expected result is, per segment, the first min(k, len) entries of the
stable argsort of srs_testlib.transformed_keys, exact and unique, so every
comparison is byte equality (srs_topk_ragged_testlib.run).

Routes: k <= 2048 takes the kernels by the library's rule, a larger k the
sort. A log-uniform k passes 2048 in one case of twelve (4 of these 60), so
the same generator also forces the sort route, which takes every shape, on a
quarter of the cases; test_both_routes_occur asserts on the host that each
route is taken by at least 10 of the 60.

A failing case runs alone as -k "test_topk_ragged_case[37]"; the assertion
message carries the case's description (without its list of lengths).
"""
import numpy as np
import pytest

import srs_fuzzlib as fz
import srs_ragged_fuzzlib as rz
import srs_topk_ragged_testlib as tl

N_CASES = 60
MAX_K = 4096


def draw(case):
    """(k, route hook, route taken) of the case"""
    rng = np.random.default_rng(case)
    k = fz._log_uniform(rng, 1, MAX_K)
    hook = tl.SORT if rng.random() < 0.25 else -1
    return k, hook, tl.SORT if hook == tl.SORT or k > tl.MAX_K else tl.KERNELS


def test_both_routes_occur():
    taken = [draw(c)[2] for c in range(N_CASES)]
    assert taken.count(tl.KERNELS) >= 10 and taken.count(tl.SORT) >= 10, taken
    ks = [draw(c)[0] for c in range(N_CASES)]
    assert min(ks) <= 4 and max(ks) > tl.MAX_K and sum(k > tl.MAX_K for k in ks) >= 2, sorted(ks)


srs_amd = pytest.importorskip("srs_amd")


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


@pytest.fixture()
def _default_route():
    yield
    srs_amd.debug_set_topk_ragged_route(-1)


@pytest.mark.gpu
@pytest.mark.parametrize("case", range(N_CASES))
def test_topk_ragged_case(torch, _default_route, case):
    d = rz.make_case(case)
    a = rz.make_arrays(d)
    k, hook, route = draw(case)
    what = str({key: v for key, v in d.items() if key not in ("lengths", "short_max")}) + \
        f" nseg={len(d['lengths'])} k={k} hook={hook}"
    srs_amd.debug_set_topk_ragged_route(hook)
    tl.run(torch, srs_amd, d["kind"], d["up"], a["cols"], a["offsets"], k, d["indices"], what=what)
    info = srs_amd.debug_last_topk_ragged()
    want = (route,) + tl.class_counts(d["lengths"])
    assert info[:3] == want, f"{info} != {want}: {what}"
    if route == tl.KERNELS:
        assert info[4] == 1 and info[5] in (2, 3), f"{info}: {what}"
