"""What the ragged top-k's GPU tests share (topk_ragged_device): the
expectation and one checked call.

The expected result is, per segment, the first min(k, len) entries of
srs_ragged_fuzzlib.ragged_orders (the stable argsort of transformed_keys):
exact and unique, so columns are compared as bytes and indices exactly. Every
output starts filled with SENTINEL and is allocated GUARD records longer than
its num_segments * k; the slots j >= min(k, len) and the guard must keep the
fill. Pure numpy apart from the tensors handed in.
"""
from __future__ import annotations

import ctypes

import numpy as np

import srs_ragged_fuzzlib as rz

SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
SENTINEL = 0x5A
GUARD = 1024          # records allocated past every output's num_segments * k
KERNELS, SORT = 0, 1  # routes
SHORT_MAX = 256       # kRowsWaveMax: the wave kernel's longest segment
MAX_K = 2048          # kTopkRowsMaxK: the kernel route's largest k


def dev(torch, a):
    """a host array as a device tensor of the signed type of its size"""
    return torch.from_numpy(np.ascontiguousarray(a).view(SINT[a.dtype.itemsize]).copy()).cuda()


def to_bytes(t):
    return t.cpu().numpy().reshape(-1).view(np.uint8)


def orders(kind, up, keys, offs):
    """ragged_orders, computed once per (kind, up, keys, offsets) and shared
    by every k"""
    return rz.ragged_orders(kind, up, keys, offs)


def heads(order, offs, k):
    """(src, idx, slot, counts): output slot slot[m] (= i * k + j) holds input
    record src[m], whose position inside its segment is idx[m]; counts[i] =
    min(k, len_i)."""
    src, idx, lo, _ = order
    offs = np.asarray(offs, dtype=np.int64)
    c = np.minimum(np.diff(offs), k)
    seg = np.repeat(np.arange(len(c), dtype=np.int64), c)
    j = np.arange(int(c.sum()), dtype=np.int64) - np.repeat(np.cumsum(c) - c, c)
    at = (offs[:-1] - lo)[seg] + j
    return src[at], idx[at], seg * k + j, c


def class_counts(lengths):
    """(segments of 1 .. 256 records, longer ones)"""
    ln = np.asarray(lengths, dtype=np.int64)
    return int(((ln >= 1) & (ln <= SHORT_MAX)).sum()), int((ln > SHORT_MAX).sum())


def guarded_out(torch, like, slots):
    """(allocation, view): slots + GUARD elements of like's dtype filled with
    SENTINEL bytes, and the view of the first `slots`"""
    big = torch.full(((slots + GUARD) * like.element_size(),), SENTINEL, dtype=torch.uint8,
                     device="cuda").view(like.dtype)
    return big, big[:slots]


def check_column(got_bytes, host, src, slot, slots, what):
    """one output column's bytes (allocation with guard) against the
    expectation: the selected records at their slots, the fill elsewhere"""
    w = host.dtype.itemsize
    want = np.full((slots + GUARD) * w, SENTINEL, dtype=np.uint8).reshape(-1, w)
    want[slot] = np.ascontiguousarray(host[src]).view(np.uint8).reshape(-1, w)
    g = got_bytes.reshape(-1, w)
    if not np.array_equal(g, want):
        bad = np.flatnonzero((g != want).any(axis=1))
        assert False, (f"{what}: {len(bad)} slot(s) differ, the first at {int(bad[0])} of "
                       f"{slots} (+{GUARD} guard)")


def run(torch, srs_amd, kind, up, cols, offs, k, indices, order=None, dcols=None, doffs=None,
        stream=None, what=""):
    """One topk_ragged_device call on host columns `cols` (keys first) into
    sentinel-filled guarded outputs, compared with the expectation; inputs and
    offsets must keep their bytes. Returns [column bytes..., indices, counts]
    as numpy arrays (indices only when asked for)."""
    offs = np.asarray(offs, dtype=np.int64)
    nseg = len(offs) - 1
    slots = nseg * k
    if order is None:
        order = orders(kind, up, cols[0], offs)
    src, idx, slot, c = heads(order, offs, k)
    if dcols is None:
        dcols = [dev(torch, x) for x in cols]
    if doffs is None:
        doffs = torch.from_numpy(offs.copy()).cuda()
    alloc = [guarded_out(torch, d, slots) for d in dcols]
    out = tuple(v for _, v in alloc)
    res = srs_amd.topk_ragged_device(*dcols, offsets=doffs, k=k, up=up, key_kind=kind,
                                     indices=indices, out=out, stream=stream)
    if stream is not None:
        stream.synchronize()
    what = f"{what} (kind={kind}, up={up}, k={k}, indices={indices})"
    assert len(res) == len(cols) + (2 if indices else 1), what
    got = []
    for q, ((big, view), h) in enumerate(zip(alloc, cols)):
        assert res[q] is view
        g = to_bytes(big)
        check_column(g, h, src, slot, slots, f"{what}: column {q}")
        got.append(g)
    if indices:
        assert tuple(res[-2].shape) == (nseg, k) and res[-2].dtype == torch.int64, what
        g = res[-2].cpu().numpy().reshape(-1)
        want = np.full(slots, -1, dtype=np.int64)  # (a new tensor: -1 where nothing is written)
        want[slot] = idx
        assert np.array_equal(g, want), f"{what}: indices differ"
        got.append(g)
    counts = res[-1].cpu().numpy()
    assert counts.shape == (nseg,) and np.array_equal(counts, c), f"{what}: counts differ"
    got.append(counts)
    for d, h in zip(dcols, cols):
        assert np.array_equal(to_bytes(d), np.ascontiguousarray(h).view(np.uint8)), \
            f"{what}: input written"
    assert np.array_equal(doffs.cpu().numpy(), offs), f"{what}: offsets written"
    return got


def call_c_abi(torch, srs_amd, kind, up, dcols, doffs, k, outs, idx, counts, stream=None):
    """srs_topk_ragged_soa_device itself on device tensors (idx / counts: a
    tensor or None); returns the code"""
    L = srs_amd.lib()
    vp = ctypes.c_void_p
    pays, pouts = dcols[1:], outs[1:]
    npay = len(pays)
    p = (vp * max(1, npay))(*[t.data_ptr() for t in pays])
    po = (vp * max(1, npay))(*[t.data_ptr() for t in pouts])
    sz = (ctypes.c_uint32 * max(1, npay))(*[t.element_size() for t in pays])
    st = (stream or torch.cuda.current_stream()).cuda_stream
    return L.srs_topk_ragged_soa_device(
        dcols[0].numel(), doffs.numel() - 1, doffs.data_ptr(), k, kind, int(bool(up)),
        dcols[0].data_ptr(), npay, p if npay else None, sz if npay else None, outs[0].data_ptr(),
        po if npay else None, None if idx is None else idx.data_ptr(),
        None if counts is None else counts.data_ptr(), st)
