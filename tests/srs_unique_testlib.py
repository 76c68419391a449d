"""Helpers of the unique tests: the expected result on the CPU and one raw
srs_unique_soa_device call on guarded device buffers, checked in full.

TEST INFRASTRUCTURE. The expected result comes from numpy alone: numpy.unique
of srs_testlib.transformed_keys (the unsigned image of the key order, floats'
bit transform and the direction included, so -0.0 and +0.0 stay distinct and
up=False needs no reversal afterwards) and its stable argsort. Every
comparison is byte equality.
"""
from __future__ import annotations

import ctypes

import numpy as np

from srs_testlib import KIND_DTYPES, key_size, transformed_keys

SINT = {1: np.int8, 2: np.int16, 4: np.int32, 8: np.int64}
GUARD = 64    # bytes of fill on both sides of every output
FILL = 0xA5
ALL_OUTPUTS = ("sorted", "indices", "offsets", "inverse", "nu_dev", "nu_host")


def expected(kind, up, keys):
    """order: S's input positions; unique / offsets / inverse / first as the
    C call defines them; U."""
    u = transformed_keys(kind, up, keys)
    uu, first, inv, cnt = np.unique(u, return_index=True, return_inverse=True, return_counts=True)
    order = np.argsort(u, kind="stable")
    offsets = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    return dict(order=order, unique=keys[first], offsets=offsets,
                inverse=inv.reshape(-1).astype(np.int64), first=first.astype(np.int64),
                U=len(uu))


def special_floats(kind, n, rng):
    """n float keys of `kind` (8 or 9) drawn from a small set that holds -0.0,
    +0.0, the infinities and denormals beside ordinary values."""
    dt = KIND_DTYPES[kind]
    tiny = np.finfo(dt).tiny
    pool = np.array([-0.0, 0.0, np.inf, -np.inf, tiny / 2, -tiny / 2, tiny / 1024,
                     np.finfo(dt).smallest_subnormal, 1.0, -1.0, 1.5, -2.25, 3e10, -3e10],
                    dtype=dt)
    pool = np.concatenate([pool, rng.standard_normal(50).astype(dt)])
    return pool[rng.integers(0, len(pool), n)]


def random_keys(kind, n, distinct, rng):
    """n keys of `kind` drawn from `distinct` random values"""
    dt = KIND_DTYPES[kind]
    w = key_size(kind)
    vals = rng.integers(0, 1 << (8 * w), size=distinct, dtype=np.uint64).astype(
        {1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[w])
    if np.issubdtype(dt, np.floating):
        f = vals.view(dt)
        vals = np.where(np.isnan(f), dt(1.0), f).view(vals.dtype)  # (NaN: outside the contract)
    return vals[rng.integers(0, distinct, n)].view(dt)


class Guarded:
    """`count` elements of `width` bytes on the device between two guards,
    everything filled with FILL; `skew` moves the base by that many bytes."""

    def __init__(self, torch, count, width, skew=0):
        self.nbytes = count * width
        self.skew = skew
        self.raw = torch.full((GUARD + skew + self.nbytes + GUARD,), FILL, dtype=torch.uint8,
                              device="cuda")
        self.ptr = self.raw.data_ptr() + GUARD + skew
        self.width = width

    def host(self):
        return self.raw.cpu().numpy()

    def check(self, written_elems, want, what):
        """guards intact, the first written_elems elements equal `want`, the
        rest still filled"""
        h = self.host()
        lo = GUARD + self.skew
        assert np.all(h[:lo] == FILL), f"{what}: written below its start"
        assert np.all(h[lo + self.nbytes:] == FILL), f"{what}: written past its end"
        wb = written_elems * self.width
        got = h[lo:lo + wb]
        exp = np.ascontiguousarray(want).view(np.uint8).reshape(-1)
        assert got.shape == exp.shape and np.array_equal(got, exp), f"{what} differs"
        assert np.all(h[lo + wb:lo + self.nbytes] == FILL), f"{what}: slots past the result written"


def to_dev(torch, a, skew_elems=0):
    """a host array on the device as bytes; skew_elems > 0: at an address that
    is element aligned but `skew_elems` elements off the allocation's start"""
    b = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    w = a.dtype.itemsize
    t = torch.empty(len(b) + skew_elems * w, dtype=torch.uint8, device="cuda")
    v = t[skew_elems * w:]
    v.copy_(torch.from_numpy(b.copy()))
    return v


def run_unique(torch, srs_amd, kind, up, keys, pays=(), outputs=ALL_OUTPUTS, stream=None,
               skew_elems=0, exp=None):
    """One srs_unique_soa_device call with the named optional outputs, checked
    against `expected` in full (results, untouched slots, guards, inputs,
    srs_debug_last_unique). Returns (expected, the device offsets buffer or
    None)."""
    lib = srs_amd.lib()
    n = len(keys)
    ks = key_size(kind)
    e = expected(kind, up, keys) if exp is None else exp
    U = e["U"]
    want_sorted = "sorted" in outputs
    assert want_sorted or not pays
    dkeys = to_dev(torch, keys, skew_elems)
    dpays = [to_dev(torch, p) for p in pays]
    skew = skew_elems * ks
    g_unique = Guarded(torch, n, ks, skew)
    g_sorted = [Guarded(torch, n, ks, skew)] + [Guarded(torch, n, p.dtype.itemsize) for p in pays] \
        if want_sorted else []
    g_idx = Guarded(torch, n, 8) if "indices" in outputs else None
    g_offs = Guarded(torch, n + 1, 8) if "offsets" in outputs else None
    g_inv = Guarded(torch, n, 8) if "inverse" in outputs else None
    g_nu = Guarded(torch, 1, 8) if "nu_dev" in outputs else None
    nu_host = ctypes.c_int64(-1)
    np_ = len(pays)
    p_in = (ctypes.c_void_p * max(1, np_))(*[p.data_ptr() for p in dpays])
    p_out = (ctypes.c_void_p * max(1, np_))(*[g.ptr for g in g_sorted[1:]])
    sizes = (ctypes.c_uint32 * max(1, np_))(*[p.dtype.itemsize for p in pays])
    sp = (stream if stream is not None else torch.cuda.current_stream()).cuda_stream
    rc = lib.srs_unique_soa_device(
        n, kind, int(up), dkeys.data_ptr(), np_, p_in if np_ else None, sizes if np_ else None,
        g_sorted[0].ptr if want_sorted else None, p_out if want_sorted and np_ else None,
        g_idx.ptr if g_idx else None, g_unique.ptr, g_offs.ptr if g_offs else None,
        g_inv.ptr if g_inv else None, g_nu.ptr if g_nu else None,
        ctypes.byref(nu_host) if "nu_host" in outputs else None, sp)
    assert rc == 0, lib.srs_last_error()
    info = srs_amd.debug_last_unique()
    with_idx = int(g_idx is not None or g_inv is not None)
    assert info == (3, int("nu_host" in outputs), with_idx, int(not want_sorted)), info
    if "nu_host" in outputs:
        assert nu_host.value == U
    else:
        assert nu_host.value == -1
    torch.cuda.synchronize()
    g_unique.check(U, e["unique"], "unique_out")
    if g_nu:
        g_nu.check(1, np.array([U], np.int64), "num_unique_dev")
    if g_offs:
        g_offs.check(U + 1, e["offsets"], "offsets_out")
    if g_idx:
        g_idx.check(n, e["order"].astype(np.int64), "indices_out")
    if g_inv:
        g_inv.check(n, e["inverse"], "inverse_out")
    for c, g in enumerate(g_sorted):
        col = keys if c == 0 else pays[c - 1]
        g.check(n, col[e["order"]], f"sorted column {c}")
    for t, h in zip([dkeys] + dpays, [keys] + list(pays)):
        assert np.array_equal(t.cpu().numpy(), np.ascontiguousarray(h).view(np.uint8).reshape(-1)), \
            "input written"
    return e, g_offs
