"""Seeded differential fuzz over the multi-GPU side on one GPU: the key
histogram (srs_key_histogram_device), the stable partition
(srs_partition_device) and the shard sort (srs_shard_*) at world 1-8 on the
host-staged transport. The cases come from tests/srs_shard_fuzzlib.py
(tests/test_shard_fuzz_plan.py shows what they reach). Every expected result
is exact (a bincount, a stable argsort), so every comparison is byte
equality.

A failing case runs alone as -k "test_partition_case[37]"; the assertion
message carries the case's description.
"""
import ctypes

import numpy as np
import pytest

import srs_shard_fuzzlib as sz
from srs_fuzzlib import key_bits
from srs_testlib import KIND_DTYPES, transformed_keys

pytestmark = pytest.mark.gpu

srs_amd = pytest.importorskip("srs_amd")

SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
TAIL = 64  # sentinel elements behind an out= tensor's result
SRS_ERR_INVALID_ARG = -1


@pytest.fixture(scope="module")
def torch():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    srs_amd.lib()
    return torch


@pytest.fixture(scope="module")
def comm_sets(torch):
    """world -> its staged communicators, kept for the whole module: their
    buffers are reused across key kinds, column widths and sizes"""
    sets = {}
    yield sets
    for comms in sets.values():
        for c in comms:
            c.close()
    sets.clear()


def _dev(torch, a):
    """a host array as a device tensor of the signed type of its size"""
    return torch.from_numpy(np.ascontiguousarray(a).view(SINT[a.dtype.itemsize]).copy()).cuda()


def _bytes(t):
    return t.cpu().numpy().view(np.uint8).ravel()


def _host_bytes(a):
    return np.ascontiguousarray(a).view(np.uint8).ravel()


def _same(t, a):
    """device tensor t holds the bytes of host array a"""
    return np.array_equal(_bytes(t), _host_bytes(a))


def _m(*parts):
    """an assertion message: a string, so the case's description is printed whole"""
    return " ".join(str(p) for p in parts)


def _out_like(torch, t, tail):
    """an output tensor for t: 0x5A everywhere, with TAIL more elements if `tail`"""
    count = t.numel() + (TAIL if tail else 0)
    return torch.full((count * t.element_size(),), 0x5A, dtype=torch.uint8,
                      device="cuda").view(t.dtype)


# --------------------------------------------------------------------------
# key histogram
# --------------------------------------------------------------------------
@pytest.mark.parametrize("case", range(sz.N_CASES["key_hist"]))
def test_key_hist_case(torch, case):
    d = sz.make_case("key_hist", case)
    keys = sz.make_arrays(d)["keys"]
    kind, up, bits = d["kind"], d["up"], d["bits"]
    pre = sz.prefill_counts(d)
    dk = _dev(torch, keys)
    hist = torch.from_numpy(pre.copy()).cuda()
    calls = 2 if d["twice"] else 1
    for _ in range(calls):
        srs_amd.key_histogram_device(dk, hist, bits, up=up, key_kind=kind)
    top = transformed_keys(kind, up, keys) >> np.uint64(key_bits(kind) - bits)
    want = pre + calls * np.bincount(top.astype(np.int64), minlength=1 << bits)
    got = hist.cpu().numpy()
    assert np.array_equal(got, want), _m("bins", np.flatnonzero(got != want)[:8], d)
    assert _same(dk, keys), _m("keys written", d)


# --------------------------------------------------------------------------
# partition
# --------------------------------------------------------------------------
def _partition(torch, kind, up, bits, parts, cols, table, tail=False, stream=None, what=""):
    """One srs_partition_device call checked against the stable argsort of
    the records' part ids. (cols: host arrays, keys first)"""
    dcols = [_dev(torch, c) for c in cols]
    dtab = torch.from_numpy(table.copy()).cuda()
    outs = tuple(_out_like(torch, t, tail) for t in dcols)
    torch.cuda.synchronize()  # the inputs are ready before a call on another stream
    counts = srs_amd.partition_device(dcols[0], dcols[1:], bits, dtab, parts, outs, up=up,
                                      key_kind=kind, stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    _check_partition(kind, up, bits, parts, cols, table, dcols, dtab, outs, counts, what)


def _check_partition(kind, up, bits, parts, cols, table, dcols, dtab, outs, counts, what):
    n = len(cols[0])
    dest = table[sz._top(kind, cols[0], bits, up)]
    assert counts == np.bincount(dest, minlength=parts).tolist(), _m("counts", what)
    order = np.argsort(dest, kind="stable")
    for c, (o, h) in enumerate(zip(outs, cols)):
        got = _bytes(o)
        nb = n * h.dtype.itemsize
        assert np.array_equal(got[:nb], _host_bytes(h[order])), _m("column", c, what)
        assert np.all(got[nb:] == 0x5A), _m("tail of column", c, what)
    for c, (t, h) in enumerate(zip(dcols, cols)):
        assert _same(t, h), _m("input column", c, "written", what)
    assert _same(dtab, table), _m("table written", what)


@pytest.mark.parametrize("case", range(sz.N_CASES["partition"]))
def test_partition_case(torch, case):
    d = sz.make_case("partition", case)
    a = sz.make_arrays(d)
    stream = torch.cuda.Stream() if d["stream"] else None
    _partition(torch, d["kind"], d["up"], d["bits"], d["num_parts"], a["cols"], a["table"],
               tail=d["out_tail"], stream=stream, what=d)


def test_partition_two_keys(torch):
    """n = 2, the smallest call that runs the kernels: the two keys in
    different parts (in and against the input order) and in one part."""
    pos = np.arange(2, dtype=np.uint32)
    for kind, keys in ((4, [5, 1 << 31]), (4, [1 << 31, 5]), (7, [-3, 9]), (2, [40000, 3])):
        k = np.array(keys, dtype=KIND_DTYPES[kind])
        for up in (True, False):
            for table in ([0, 1], [1, 0], [2, 2], [0, 0]):
                _partition(torch, kind, up, 1, 3, [k, pos], np.array(table, np.int32), tail=True,
                           what=("two keys", kind, keys, up, table))


def test_partition_sixteen_bits_of_a_sixteen_bit_key(torch):
    """bits = 16 on 16-bit keys: the whole key is the table index (the table
    is read from global memory), with a table that is not monotone."""
    rng = np.random.default_rng(16)
    for kind in (2, 3):
        keys = rng.integers(0, 1 << 16, 20_001, dtype=np.uint64).astype(np.uint16).view(
            KIND_DTYPES[kind])
        table = rng.integers(0, 37, 1 << 16).astype(np.int32)
        for up in (True, False):
            _partition(torch, kind, up, 16, 37, [keys, np.arange(len(keys), dtype=np.uint32)],
                       table, tail=True, what=("bits 16", kind, up))


def test_partitions_back_to_back_on_one_stream(torch):
    """Two partitions of different key kinds on one stream with no
    synchronisation between them: the second call's workspace use is ordered
    behind the first call's kernels. Both are checked afterwards."""
    rng = np.random.default_rng(2)
    jobs = []
    for kind, bits, parts, n in ((6, 11, 200, 150_001), (0, 8, 7, 9_000)):
        keys = sz.gen_keys(kind, n, "full", rng)
        cols = [keys, rng.integers(0, 1 << 16, n, dtype=np.uint64).astype(np.uint16),
                np.arange(n, dtype=np.uint32)]
        table = rng.integers(0, parts, 1 << bits).astype(np.int32)
        dcols = [_dev(torch, c) for c in cols]
        jobs.append((kind, bits, parts, cols, table, dcols, torch.from_numpy(table.copy()).cuda(),
                     tuple(_out_like(torch, t, True) for t in dcols)))
    s = torch.cuda.Stream()
    torch.cuda.synchronize()
    counts = [srs_amd.partition_device(dc[0], dc[1:], bits, dt, parts, outs, up=False,
                                       key_kind=kind, stream=s)
              for kind, bits, parts, _, _, dc, dt, outs in jobs]
    s.synchronize()
    for (kind, bits, parts, cols, table, dc, dt, outs), cnt in zip(jobs, counts):
        _check_partition(kind, False, bits, parts, cols, table, dc, dt, outs, cnt,
                         ("back to back", kind))


def test_invalid_bits_launch_nothing(torch):
    """The host checks the shard sort relies on: a partition's bits outside
    [1, min(16, key bits)] and a histogram's bits above 12 or above the key's
    width return SRS_ERR_INVALID_ARG and write nothing."""
    L = srs_amd.lib()
    n = 1000
    for kind, hist_bad, part_bad in ((6, (0, 13), (0, 17)), (0, (0, 9, 13), (0, 9, 17)),
                                     (3, (13,), (17,))):
        keys = _dev(torch, np.arange(n).astype(KIND_DTYPES[kind]))
        for bits in hist_bad:
            hist = torch.full((1 << max(bits, 1),), 0x5A5A, dtype=torch.int64, device="cuda")
            rc = L.srs_key_histogram_device(n, kind, 1, keys.data_ptr(), bits, hist.data_ptr(),
                                            torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rc == SRS_ERR_INVALID_ARG, (kind, bits, rc)
            assert bool((hist == 0x5A5A).all()), (kind, bits)
        for bits in part_bad:
            table = torch.zeros(1 << max(bits, 1), dtype=torch.int32, device="cuda")
            out = _out_like(torch, keys, False)
            counts = (ctypes.c_int64 * 4)(7, 7, 7, 7)
            rc = L.srs_partition_device(n, kind, 1, keys.data_ptr(), 0, None, None, bits,
                                        table.data_ptr(), 4, out.data_ptr(), None, counts,
                                        torch.cuda.current_stream().cuda_stream)
            torch.cuda.synchronize()
            assert rc == SRS_ERR_INVALID_ARG, (kind, bits, rc)
            assert bool((out.view(torch.uint8) == 0x5A).all()), (kind, bits)
            assert list(counts) == [7, 7, 7, 7], (kind, bits)
    assert b"bits" in L.srs_last_error()


# --------------------------------------------------------------------------
# shard sort
# --------------------------------------------------------------------------
def _shard_sort(torch, comm_sets, d, ranks):
    """The case's shard sort on its world's cached communicators. Returns
    (per-rank host byte arrays per column, reports). A case that raises
    closes and drops its world's communicators: the next case starts clean."""
    from srs_amd import shard
    world = d["world"]
    try:
        if world not in comm_sets:
            comm_sets[world] = shard.staged(world)
        comms = comm_sets[world]
        for c in comms:  # (the defaults too: the communicators are reused)
            c.set_options(d["rounds"], d["chunks"])
            c.set_message_options(d["self_messages"], d["max_message_bytes"])
        inputs = [[_dev(torch, col) for col in cols] for cols in ranks]
        torch.cuda.synchronize()
        outs = shard.sort_multi(comms, [(cols[0], cols[1:]) for cols in inputs],
                                key_kind=d["kind"], up=d["up"])
        # (the outputs are views of the communicators' buffers: copied out now)
        got = [[_bytes(k)] + [_bytes(p) for p in ps] for k, ps in outs]
        counts = [k.numel() for k, _ in outs]
        del outs
        reports = [c.report() for c in comms]
        for r, (dcols, cols) in enumerate(zip(inputs, ranks)):
            for c, (t, h) in enumerate(zip(dcols, cols)):
                assert _same(t, h), _m("rank", r, "input column", c, "written", d)
        return got, counts, reports
    except BaseException:
        for c in comm_sets.pop(world, []):
            c.close()
        raise


def _check_shard(d, ranks, got, counts, reports):
    world, kind, up = d["world"], d["kind"], d["up"]
    ncols = len(ranks[0])
    total = sum(d["ns"])
    assert sum(counts) == total, _m("records out", counts, d)
    rounds, chunks = sz.shard_options(d)
    for r, rep in enumerate(reports):
        assert rep["transport"] == "staged" and rep["world"] == world and rep["rank"] == r, \
            _m(rep, d)
        assert rep["records_out"] == counts[r], _m("rank", r, rep, d)
        assert rep["records_in"] == d["ns"][r], _m("rank", r, rep, d)
        assert rep["chunks"] == chunks and rep["rounds"] == rounds, _m(rep, d)
        assert rep["self_messages"] == int(d["self_messages"]), _m(rep, d)
        assert rep["max_message_bytes"] == (d["max_message_bytes"] or 256 << 20), _m(rep, d)
    ins = [np.concatenate([cols[c] for cols in ranks]) for c in range(ncols)]
    u = transformed_keys(kind, up, ins[0])
    order = np.argsort(u, kind="stable")
    for c in range(ncols):
        out = np.concatenate([g[c] for g in got])
        assert np.array_equal(out, _host_bytes(ins[c][order])), _m("column", c, d)
    # equal keys share a group: no boundary between ranks splits a run of them
    ends = np.cumsum(counts)[:-1]
    ends = ends[(ends > 0) & (ends < total)]
    su = u[order]
    assert not np.any(su[ends - 1] == su[ends]), _m("a run of equal keys spans two ranks", d)


@pytest.mark.parametrize("case", range(sz.N_CASES["shard"]))
def test_shard_case(torch, comm_sets, case):
    d = sz.make_case("shard", case)
    ranks = sz.make_arrays(d)["ranks"]
    got, counts, reports = _shard_sort(torch, comm_sets, d, ranks)
    _check_shard(d, ranks, got, counts, reports)


@pytest.mark.parametrize("kind,up", [(6, True), (1, False), (9, False)])
def test_shard_ranks_of_zero_one_and_two_records(torch, comm_sets, kind, up):
    """world 3 with n = (0, 1, 2): every chunk and every round holds at most
    two records; with and without self messages."""
    rng = np.random.default_rng(kind)
    for self_messages in (False, True):
        d = {"api": "shard", "world": 3, "kind": kind, "up": up, "ns": [0, 1, 2], "rounds": 3,
             "chunks": 2, "self_messages": self_messages, "max_message_bytes": 0}
        ranks, first = [], 0
        for n in d["ns"]:
            ranks.append([sz.gen_keys(kind, n, "full", rng),
                          rng.integers(0, 256, n).astype(np.uint8),
                          (first + np.arange(n)).astype(np.uint32)])
            first += n
        got, counts, reports = _shard_sort(torch, comm_sets, d, ranks)
        _check_shard(d, ranks, got, counts, reports)
