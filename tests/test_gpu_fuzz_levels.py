"""Differential fuzz of the sort's large-input levels at small sizes: the
plain first level, the digit-table and range levels, the stripe level and
the gathered level behind it. The seeded plan is
tests/srs_level_fuzzlib.py (its coverage: tests/test_level_fuzz_plan.py);
srs_amd.debug_set_first_level lowers the compiled-in sizes for the case and
is restored in a `finally`.

Every case asserts, from srs_amd.debug_last_first_level, that the sort took
the path its class promises (a silent fall-back to the plain path would pass
every parity check), then requires every output column to equal the stable
reference byte for byte and, out of place, the inputs to be unchanged. A
stripes case sorts the same input once more with the stripe fields of the hook
at their defaults (no stripes), which must give the same bytes."""
import numpy as np
import pytest

import srs_level_fuzzlib as lz
from test_gpu_sort import bytes_equal

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

_INT = {1: np.uint8, 2: np.int16, 4: np.int32, 8: np.int64}


def _torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    return torch


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    _torch()
    srs_amd.lib()
    yield
    srs_amd.debug_set_first_level()


def _to_device(torch, a):
    if a.ndim == 2:
        return torch.from_numpy(a).cuda()
    return torch.from_numpy(a.view(f"u{a.dtype.itemsize}").view(_INT[a.dtype.itemsize])).cuda()


def _sort(torch, d, arrays, hook):
    """One sort of the case under `hook`: (output columns, the first level's
    report, the input tensors after the call or None when in place)."""
    host = [arrays["records"]] if d["shape"] == "aos" else arrays["cols"]
    dev = [_to_device(torch, c) for c in host]
    out = None if d["inplace"] else [torch.empty_like(t) for t in dev]
    srs_amd.debug_set_first_level(**hook)
    try:
        if d["bounds"] is not None:
            srs_amd.sort_segments_device(dev[0], *dev[1:], bounds=d["bounds"], up=d["up"],
                                         key_kind=d["kind"])
        elif d["shape"] == "aos":
            srs_amd.sort_combined_device(dev[0], d["kind"], up=d["up"],
                                         cmp_sort_threshold=d["thresh"],
                                         out=None if out is None else out[0])
        else:
            srs_amd.sort_device(dev[0], *dev[1:], up=d["up"], key_kind=d["kind"],
                                cmp_sort_threshold=d["thresh"],
                                out=None if out is None else tuple(out))
        torch.cuda.synchronize()
        info = srs_amd.debug_last_first_level()
    finally:
        srs_amd.debug_set_first_level()
    got = [t.cpu().numpy() for t in (dev if out is None else out)]
    return got, info, (None if out is None else [t.cpu().numpy() for t in dev])


def _check_promise(d, info):
    p, text = d["promise"], lz.describe_text(d)
    assert info["stripes"] == p["stripes"], (text, info)
    if "start" in p:
        assert info["start"] == p["start"], (text, info)
    if not p["stripes"]:
        assert info["stripe_count"] == 0 and info["gathered_tiles"] == 0, (text, info)
        return
    assert info["stripe_count"] == p["stripe_count"], (text, info)
    assert info["first_bits"] == p["first_bits"], (text, info)
    assert info["gathered_tiles"] > 0, (text, info)
    assert (info["kind"] == srs_amd.LEVEL_PLAIN) == p["kind_zero"], (text, info)
    if d["dist"] in ("gauss", "heavy_gauss"):
        assert info["kind"] == srs_amd.LEVEL_RANGES, (text, info)
    if "kind" in p:  # a forced table: LEVEL_TABLE16 or LEVEL_SPLIT_TABLE
        assert info["kind"] == p["kind"], (text, info)


def _check_parity(d, arrays, want, got, inputs, what):
    for i, (g, w) in enumerate(zip(got, want)):
        assert bytes_equal(g, w), (lz.describe_text(d), what, "column", i)
    if inputs is not None:
        host = [arrays["records"]] if d["shape"] == "aos" else arrays["cols"]
        for i, (t, c) in enumerate(zip(inputs, host)):
            assert bytes_equal(t, c), (lz.describe_text(d), what, "input changed", i)


@pytest.mark.parametrize("case", range(lz.N_CASES))
def test_level_case(case, monkeypatch):
    torch = _torch()
    d, arrays = lz.make_case(case)
    for name, value in (("SRS_PAIR_TILES", d["pair_tiles"]), ("SRS_TABLE", d["table"])):
        if value is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, str(value))
    want = lz.reference(d, arrays)
    got, info, inputs = _sort(torch, d, arrays, d["hook"])
    _check_promise(d, info)
    _check_parity(d, arrays, want, got, inputs, "hooked")
    if d["cls"] not in lz.STRIPE_CLASSES:
        return
    # the same input down the path without stripes
    plain = dict(d["hook"], stripe_min_n=0, stripe_pairs=0, first_bits=0)
    got, info, inputs = _sort(torch, d, arrays, plain)
    assert info["stripes"] == 0 and info["start"] == srs_amd.START_PLAIN, (case, info)
    _check_parity(d, arrays, want, got, inputs, "without stripes")


def test_defaults_after_a_hooked_sort():
    """The restore works: after a hooked sort, a sort of 2^25 + 1234 uniform
    u64 + u64 takes the stripe level with the planner's own stripe count; a
    sort of 2^20 records starts with the mid-size launch again."""
    torch = _torch()
    d, arrays = lz.make_case(lz.CLASS_COUNTS[0])  # the first stripes-plain case
    _, info, _ = _sort(torch, d, arrays, d["hook"])
    assert info["stripes"] == 1
    n = (1 << 25) + 1234
    g = torch.Generator(device="cuda")
    g.manual_seed(31)
    keys = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64, device="cuda", generator=g)
    pay = torch.arange(n, dtype=torch.int64, device="cuda")
    ko, po = torch.empty_like(keys), torch.empty_like(pay)
    srs_amd.sort_device(keys, pay, key_kind=srs_amd.KEY_U64, out=(ko, po))
    torch.cuda.synchronize()
    info = srs_amd.debug_last_first_level()
    b1 = lz.choose_bits(n, 64)
    assert b1 in (7, 8, 9)
    assert info["start"] == srs_amd.START_PLAIN and info["stripes"] == 1, info
    assert info["first_bits"] == b1 and info["stripe_count"] == -(-n // (3904 << b1)), info
    _, ref_i = torch.sort(keys ^ torch.iinfo(torch.int64).min, stable=True)
    assert torch.equal(po, ref_i) and torch.equal(ko, keys[ref_i])
    small = keys[:1 << 20].clone()
    srs_amd.sort_device(small, key_kind=srs_amd.KEY_U64)
    torch.cuda.synchronize()
    info = srs_amd.debug_last_first_level()
    assert info["start"] == srs_amd.START_MID and info["stripes"] == 0, info


def test_hook_rejects_what_the_driver_cannot_take():
    _torch()
    for bad in (dict(stripe_pairs=lz.MAX_STRIPE_PAIRS + 1), dict(first_bits=10)):
        with pytest.raises(srs_amd.SrsError):
            srs_amd.debug_set_first_level(**bad)
    srs_amd.debug_set_first_level()
