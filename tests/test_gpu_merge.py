"""GPU tests of merge (srs_merge_soa_device, srs_amd.merge_device): the
smallest shapes at which the kernels can go wrong. Every raw call goes through
srs_merge_testlib.run_merge: outputs between guard words, compared byte for
byte with the stable argsort of the transformed keys of A followed by B,
inputs unwritten, srs_debug_last_merge as designed.
"""
import numpy as np
import pytest

import srs_merge_testlib as ml
import srs_unique_testlib as ul
from srs_testlib import KIND_DTYPES, KIND_NAMES, transformed_keys

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

U8, U16, U32, I32, U64, I64, F32, F64 = 0, 2, 4, 5, 6, 7, 8, 9
T = srs_amd.MERGE_TILE
SIZES = [(0, 1), (1, 0), (1, 1), (0, T + 5), (T + 5, 0), (T - 1, 1), (T // 2, T // 2), (T, 1),
         (1, T), (T, T), (2 * T + 1, 3), (3, 2 * T + 1), (3 * T + 7, 2 * T - 3)]
LAW_NA, LAW_NB = 3 * T + 7, 2 * T - 3


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


def _pays(widths, na, nb, rng):
    return ml.make_payloads(widths, na, rng, 0), ml.make_payloads(widths, nb, rng, 1)


def test_no_records_writes_nothing(torch):
    e = np.zeros(0, np.uint64)
    ml.run_merge(torch, srs_amd, U64, True, e, e, [e], [e])


@pytest.mark.parametrize("na,nb", SIZES, ids=[f"{a}+{b}" for a, b in SIZES])
def test_sizes(torch, na, nb):
    rng = np.random.default_rng(na * 31 + nb)
    for kind, widths in ((U64, (8,)), (F32, ())):
        a, b = ml.random_sides(kind, True, na, nb, int(np.sqrt(na + nb)) + 1, rng)
        pa, pb = _pays(widths, na, nb, rng)
        ml.run_merge(torch, srs_amd, kind, True, a, b, pa, pb)


def _law(law, rng):
    """(A, B) of u32 keys, sorted ascending"""
    na, nb = LAW_NA, LAW_NB
    if law == "all_equal":
        a, b = np.full(na, 7), np.full(nb, 7)
    elif law == "a_below_b":
        a, b = np.arange(na), na + np.arange(nb)
    elif law == "b_below_a":
        a, b = nb + np.arange(na), np.arange(nb)
    elif law == "interleave":
        a, b = 2 * np.arange(na), 2 * np.arange(nb) + 1
    elif law == "two_values":
        a, b = np.sort(rng.integers(0, 2, na)), np.sort(rng.integers(0, 2, nb))
    elif law == "b_in_one_gap":
        a = 1000 * np.arange(na)
        b = 1000 * (T + 3) + 1 + np.sort(rng.integers(0, 998, nb))
    else:  # a run longer than a tile in A whose key occurs three times in B
        assert law == "long_run"
        a = np.concatenate([np.arange(100), np.full(T + 300, 5000), 6000 + np.arange(na - T - 400)])
        b = np.sort(np.concatenate([rng.integers(0, 12000, nb - 3), [5000, 5000, 5000]]))
    assert len(a) == na and len(b) == nb
    return a.astype(np.uint32), b.astype(np.uint32)


@pytest.mark.parametrize("law", ["all_equal", "a_below_b", "b_below_a", "interleave",
                                 "two_values", "b_in_one_gap", "long_run"])
def test_key_laws(torch, law):
    rng = np.random.default_rng(5)
    a, b = _law(law, rng)
    pa, pb = _pays((8,), len(a), len(b), rng)
    ml.run_merge(torch, srs_amd, U32, True, a, b, pa, pb)
    if law == "all_equal":  # all of A, then all of B
        order = ml.expected_order(U32, True, a, b)
        assert np.array_equal(order, np.arange(len(a) + len(b)))


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("kind", range(10), ids=KIND_NAMES)
def test_kinds(torch, kind, up):
    na, nb = 2 * T + 1, T + 3
    rng = np.random.default_rng(100 + 2 * kind + up)
    a, b = ml.random_sides(kind, up, na, nb, int(np.sqrt(na + nb)), rng)
    pa, pb = _pays((4,), na, nb, rng)
    ml.run_merge(torch, srs_amd, kind, up, a, b, pa, pb)


@pytest.mark.parametrize("up", [True, False])
@pytest.mark.parametrize("kind", [F32, F64], ids=["f32", "f64"])
def test_special_floats(torch, kind, up):
    na, nb = 2 * T + 1, T + 3
    rng = np.random.default_rng(200 + kind + up)
    a = ml.sorted_side(kind, up, ul.special_floats(kind, na, rng))
    b = ml.sorted_side(kind, up, ul.special_floats(kind, nb, rng))
    pa, pb = _pays((8,), na, nb, rng)
    ml.run_merge(torch, srs_amd, kind, up, a, b, pa, pb)


@pytest.mark.parametrize("source", [True, False], ids=["source", "nosource"])
@pytest.mark.parametrize("name", list(ml.PAYLOAD_SETS))
def test_payload_sets(torch, name, source):
    na, nb = T + 77, T // 2 + 5
    rng = np.random.default_rng(len(name))
    a, b = ml.random_sides(I64, True, na, nb, 50, rng)
    pa, pb = _pays(ml.PAYLOAD_SETS[name], na, nb, rng)
    ml.run_merge(torch, srs_amd, I64, True, a, b, pa, pb, source=source)


@pytest.mark.parametrize("source", [True, False], ids=["source", "nosource"])
def test_64_one_byte_columns(torch, source):
    na, nb = 300, 200
    rng = np.random.default_rng(64)
    a, b = ml.random_sides(U16, False, na, nb, 20, rng)
    pa, pb = _pays((1,) * 64, na, nb, rng)
    ml.run_merge(torch, srs_amd, U16, False, a, b, pa, pb, source=source)


@pytest.mark.parametrize("kind", [U8, U16, F32, U64], ids=["u8", "u16", "f32", "u64"])
def test_columns_aligned_to_their_element_size_only(torch, kind):
    na, nb = T + 9, T - 11
    rng = np.random.default_rng(300 + kind)
    a, b = ml.random_sides(kind, True, na, nb, 40, rng)
    pa, pb = _pays((1, 2, 4, 8), na, nb, rng)
    for skew in (1, 3):
        ml.run_merge(torch, srs_amd, kind, True, a, b, pa, pb, skew_elems=skew)


def test_non_default_stream(torch):
    na, nb = 2 * T + 1, T + 3
    rng = np.random.default_rng(400)
    a, b = ml.random_sides(U64, True, na, nb, 60, rng)
    pa, pb = _pays((8,), na, nb, rng)
    ml.run_merge(torch, srs_amd, U64, True, a, b, pa, pb, stream=torch.cuda.Stream())


def test_two_calls_back_to_back(torch):
    """a larger call, then a smaller one, on the same workspace: the second
    reads none of the first's split array"""
    rng = np.random.default_rng(500)
    for na, nb in ((5 * T + 1, 3 * T), (T + 1, 7), (5 * T + 1, 3 * T)):
        a, b = ml.random_sides(U32, True, na, nb, 30, rng)
        pa, pb = _pays((4,), na, nb, rng)
        ml.run_merge(torch, srs_amd, U32, True, a, b, pa, pb)


def _agrees_with_sort(torch, kind, tdtype, na, nb, with_payload):
    """merge_device of two sorted halves == sort_device(cat) out of place"""
    rng = np.random.default_rng(na)
    keys = ul.random_keys(kind, na + nb, 1 << 16, rng)
    dt = KIND_DTYPES[kind]
    view = {np.dtype(np.uint64): np.int64}.get(np.dtype(dt), dt)
    d = torch.from_numpy(keys.view(view).copy()).cuda()
    pos = torch.arange(na + nb, dtype=torch.int64, device="cuda")
    # the two sides, sorted by the library, each with its records' positions
    sa = tuple(torch.empty_like(x[:na]) for x in (d, pos))
    sb = tuple(torch.empty_like(x[na:]) for x in (d, pos))
    srs_amd.sort_device(d[:na], pos[:na], key_kind=kind, cmp_sort_threshold=0, out=sa)
    srs_amd.sort_device(d[na:], pos[na:], key_kind=kind, cmp_sort_threshold=0, out=sb)
    want = tuple(torch.empty_like(x) for x in (d, pos))
    srs_amd.sort_device(d, pos, key_kind=kind, cmp_sort_threshold=0, out=want)
    if with_payload:
        got = srs_amd.merge_device(sa, sb, key_kind=kind)
        assert torch.equal(got[1], want[1])
    else:
        got = srs_amd.merge_device(sa[:1], sb[:1], key_kind=kind, indices=True)
        # source_out names a record of cat(sa, sb); its input position is there
        assert torch.equal(torch.cat([sa[1], sb[1]])[got[1]], want[1])
    assert torch.equal(got[0].view(torch.uint8), want[0].view(torch.uint8))
    assert got[0].dtype == tdtype(torch)


def test_agrees_with_sort_u64_u64(torch):
    _agrees_with_sort(torch, U64, lambda t: t.int64, (1 << 20) + 12345, (1 << 19) + 77, True)


def test_agrees_with_sort_f32_source(torch):
    _agrees_with_sort(torch, F32, lambda t: t.float32, (1 << 20) + 12345, (1 << 19) + 77, False)


@pytest.mark.parametrize("kind", [U32, F64], ids=["u32", "f64"])
def test_unsorted_inputs_stay_inside(torch, kind):
    """rc OK, guards intact, inputs unwritten, source_out within [0, n):
    nothing else is asserted"""
    na, nb = 2 * T + 1, T + 3
    rng = np.random.default_rng(600 + kind)
    a = ul.random_keys(kind, na, na, rng)
    b = ul.random_keys(kind, nb, nb, rng)
    pa, pb = _pays((8, 1), na, nb, rng)
    ml.run_merge(torch, srs_amd, kind, True, a, b, pa, pb, check_results=False)


# ---- the Python wrapper ------------------------------------------------------
def _dev_sides(torch, kind, na, nb, seed, up=True):
    rng = np.random.default_rng(seed)
    a, b = ml.random_sides(kind, up, na, nb, 100, rng)
    dt = KIND_DTYPES[kind]
    view = {np.dtype(np.uint64): np.int64}.get(np.dtype(dt), dt)
    pa = np.arange(na, dtype=np.int32)
    pb = np.arange(nb, dtype=np.int32) + na
    order = ml.expected_order(kind, up, a, b)
    dev = [torch.from_numpy(x.view(view).copy() if x.dtype == dt else x.copy()).cuda()
           for x in (a, pa, b, pb)]
    return dev, np.concatenate([a, b])[order], order


def test_wrapper_returns_new_tensors_and_indices(torch):
    (a, pa, b, pb), keys, order = _dev_sides(torch, F32, T + 5, 2 * T, 1)
    out = srs_amd.merge_device((a, pa), (b, pb), indices=True)
    assert len(out) == 3 and out[2].dtype == torch.int64
    assert out[0].cpu().numpy().tobytes() == keys.tobytes()
    assert np.array_equal(out[1].cpu().numpy(), order.astype(np.int32))
    assert np.array_equal(out[2].cpu().numpy(), order)
    assert srs_amd.debug_last_merge()[:3] == (ml.LAUNCHES, 0, 4)  # 3 T + 5 records: 4 tiles


def test_wrapper_out_and_descending(torch):
    (a, pa, b, pb), keys, order = _dev_sides(torch, I32, 1000, 3000, 2, up=False)
    ko = torch.full((5000,), -1, dtype=torch.int32, device="cuda")
    po = torch.full((4000,), -1, dtype=torch.int32, device="cuda")
    out = srs_amd.merge_device((a, pa), (b, pb), up=False, out=(ko, po))
    assert out[0] is ko and out[1] is po and len(out) == 2
    assert np.array_equal(ko.cpu().numpy()[:4000], keys)
    assert np.all(ko.cpu().numpy()[4000:] == -1)
    assert np.array_equal(po.cpu().numpy(), order.astype(np.int32))


def test_wrapper_key_kind_override(torch):
    """uint64 keys held in int64 storage: values above 2^63 sort last"""
    (a, pa, b, pb), keys, order = _dev_sides(torch, U64, 3000, 2000, 3)
    assert a.dtype == torch.int64 and (keys >> np.uint64(63)).any()
    out = srs_amd.merge_device((a,), (b,), key_kind=srs_amd.KEY_U64, indices=True)
    assert np.array_equal(out[0].cpu().numpy().view(np.uint64), keys)
    assert np.array_equal(out[1].cpu().numpy(), order)


def test_wrapper_empty_sides(torch):
    (a, pa, b, pb), _, _ = _dev_sides(torch, I32, 100, 50, 4)
    e, ep = a[:0], pa[:0]
    out = srs_amd.merge_device((a, pa), (e, ep), indices=True)
    assert torch.equal(out[0], a) and torch.equal(out[1], pa)
    assert torch.equal(out[2], torch.arange(100, device="cuda"))
    out = srs_amd.merge_device((e, ep), (b, pb))
    assert torch.equal(out[0], b) and torch.equal(out[1], pb)
    out = srs_amd.merge_device((e, ep), (e, ep), indices=True)
    assert [o.numel() for o in out] == [0, 0, 0]


def test_wrapper_rejects_mismatches(torch):
    (a, pa, b, pb), _, _ = _dev_sides(torch, I32, 100, 50, 5)
    with pytest.raises(TypeError):
        srs_amd.merge_device((a, pa), (b.to(torch.int64), pb))
    with pytest.raises(TypeError):
        srs_amd.merge_device((a, pa), (b, pb.to(torch.float32)))
    with pytest.raises(ValueError):
        srs_amd.merge_device((a, pa), (b,))
    with pytest.raises(ValueError):
        srs_amd.merge_device((a, pa[:50]), (b, pb))
    with pytest.raises(ValueError):
        srs_amd.merge_device((a, pa), (b.cpu(), pb.cpu()))
    with pytest.raises(ValueError):
        srs_amd.merge_device((a, pa), (b, pb), out=(torch.empty(10, dtype=torch.int32,
                                                                device="cuda"),) * 2)
    if torch.cuda.device_count() > 1:
        with pytest.raises(ValueError):
            srs_amd.merge_device((a, pa), (b.to("cuda:1"), pb.to("cuda:1")))
    # (the C call reports what the wrapper cannot see: an output over an input)
    buf = torch.zeros(300, dtype=torch.int32, device="cuda")
    with pytest.raises(srs_amd.SrsError, match="overlap the inputs"):
        srs_amd.merge_device((a, buf[:100]), (b, pb), out=(a.new_empty(150), buf[50:200]))
