"""srs_amd — Python mirror of simd_sort::radix_sort over the C ABI of
libsrs_amd.so (include/srs_c_api.h).

Reference interface mirrored (jonicho/simd-radix-sort, radixSort.hpp):
  sort(keys, *payloads, up=True)                     radix_sort::sort<Up>(num, keys, payloads...)   :1780
  sort_thresh(thresh, keys, *payloads, up=True)      sort<Up,BitSorter,CmpSorter>(thresh, num, ...)  :1761
  sort_combined(elements, key_kind, up=True)         sort(thresh, num, DataElement<K,Ps...>*)         :1770

Host numpy arrays are sorted in place (the reference's contract). The
*_device functions take torch tensors already resident in HBM and enqueue on
torch's current stream.

There is no CPU fallback: if the HIP library is missing or the call fails,
an exception is raised.
"""
from __future__ import annotations

import collections
import ctypes
import os

import numpy as np

try:  # load torch first so one HIP runtime (torch's) serves both libraries
    import torch  # noqa: F401
    _HAVE_TORCH = True
except Exception:  # pragma: no cover - torch is present in this image
    _HAVE_TORCH = False

_PKG_ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIB_PATH = os.environ.get("SRS_AMD_LIB") or os.path.join(_PKG_ROOT, "lib", "libsrs_amd.so")

# srs_key_kind (include/srs_c_api.h)
KEY_U8, KEY_I8, KEY_U16, KEY_I16, KEY_U32, KEY_I32, KEY_U64, KEY_I64, KEY_F32, KEY_F64 = range(10)
_NP_KIND = {np.dtype(np.uint8): KEY_U8, np.dtype(np.int8): KEY_I8,
            np.dtype(np.uint16): KEY_U16, np.dtype(np.int16): KEY_I16,
            np.dtype(np.uint32): KEY_U32, np.dtype(np.int32): KEY_I32,
            np.dtype(np.uint64): KEY_U64, np.dtype(np.int64): KEY_I64,
            np.dtype(np.float32): KEY_F32, np.dtype(np.float64): KEY_F64}

SRS_OK = 0
# leaf handling (srs_c_api.h): the reference's CmpSorter (src/cmp_sorters.hpp)
LEAF_SORTED, LEAF_UNSORTED = 0, 1
_LEAF = {"insertion": LEAF_SORTED, "bramas": LEAF_SORTED, "nosort": LEAF_UNSORTED}


class SrsError(RuntimeError):
    pass


_lib = None


def lib() -> ctypes.CDLL:
    """The HIP library; raises if it has not been built (no fallback)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(f"libsrs_amd.so not built: {LIB_PATH} (run `make -C simd-radix-sort_amd`)")
    L = ctypes.CDLL(LIB_PATH)
    i64, i32, u32, vp = ctypes.c_int64, ctypes.c_int32, ctypes.c_uint32, ctypes.c_void_p
    L.srs_sort_soa.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64, vp, i32, vp, vp]
    L.srs_sort_aos.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64, vp, u32]
    L.srs_sort_soa_leaf.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64, ctypes.c_int, vp, i32,
                                    vp, vp]
    L.srs_sort_aos_leaf.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64, ctypes.c_int, vp, u32]
    L.srs_sort_soa_device_leaf.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64, ctypes.c_int, vp,
                                           i32, vp, vp, vp, vp, vp]
    L.srs_sort_aos_device_leaf.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64, ctypes.c_int, vp,
                                           u32, vp, vp]
    L.srs_sort_soa_device.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64, vp, i32, vp, vp,
                                      vp, vp, vp]
    L.srs_sort_aos_device.argtypes = [i64, ctypes.c_int, ctypes.c_int, i64, vp, u32, vp, vp]
    L.srs_sort_segments_device.argtypes = [i64, ctypes.c_int, ctypes.c_int, vp, i32, vp, vp, i64,
                                           vp, i32, vp]
    L.srs_topk_soa_device.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int, vp, i32, vp, vp, vp,
                                      vp, vp, vp]
    L.srs_topk_aos_device.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int, vp, u32, vp, vp, vp]
    L.srs_debug_set_topk_candidates.argtypes = [i64]
    L.srs_debug_last_topk.argtypes = [ctypes.POINTER(i64)]
    L.srs_topk_rows_soa_device.argtypes = [i64, i64, i64, i64, ctypes.c_int, ctypes.c_int, vp, i32,
                                           vp, vp, vp, vp, vp, vp]
    L.srs_topk_rows_max_k.restype = i64
    L.srs_debug_set_topk_rows_route.argtypes = [ctypes.c_int]
    L.srs_debug_last_topk_rows.argtypes = [ctypes.POINTER(i64)]
    L.srs_sort_rows_soa_device.argtypes = [i64, i64, i64, ctypes.c_int, ctypes.c_int, vp, i32, vp,
                                           vp, vp, vp, vp, vp]
    L.srs_debug_set_sort_rows_route.argtypes = [ctypes.c_int]
    L.srs_debug_last_sort_rows.argtypes = [ctypes.POINTER(i64)]
    L.srs_sort_ragged_soa_device.argtypes = [i64, i64, vp, ctypes.c_int, ctypes.c_int, vp, i32, vp,
                                             vp, vp, vp, vp, vp]
    L.srs_debug_set_sort_ragged_short_max.argtypes = [i32]
    L.srs_debug_last_sort_ragged.argtypes = [ctypes.POINTER(i64)]
    L.srs_topk_ragged_soa_device.argtypes = [i64, i64, vp, i64, ctypes.c_int, ctypes.c_int, vp,
                                             i32, vp, vp, vp, vp, vp, vp, vp]
    L.srs_debug_set_topk_ragged_route.argtypes = [ctypes.c_int]
    L.srs_debug_last_topk_ragged.argtypes = [ctypes.POINTER(i64)]
    L.srs_unique_soa_device.argtypes = [i64, ctypes.c_int, ctypes.c_int, vp, i32, vp, vp, vp, vp,
                                        vp, vp, vp, vp, vp, vp, vp]
    L.srs_debug_last_unique.argtypes = [ctypes.POINTER(i64)]
    L.srs_search_sorted_device.argtypes = [i64, ctypes.c_int, ctypes.c_int, vp, i64, vp, i64, vp,
                                           vp, vp, vp, vp, i32, vp]
    L.srs_debug_set_search_route.argtypes = [ctypes.c_int]
    L.srs_debug_last_search.argtypes = [ctypes.POINTER(i64)]
    L.srs_merge_soa_device.argtypes = [i64, i64, ctypes.c_int, ctypes.c_int, vp, vp, i32, vp, vp,
                                       vp, vp, vp, vp, vp]
    L.srs_debug_last_merge.argtypes = [ctypes.POINTER(i64)]
    L.srs_fill_synthetic_device.argtypes = [i64, ctypes.c_int, ctypes.c_uint64, ctypes.c_uint64,
                                            vp, i32, vp, vp, vp]
    L.srs_key_histogram_device.argtypes = [i64, ctypes.c_int, ctypes.c_int, vp, ctypes.c_int, vp,
                                           vp]
    L.srs_partition_device.argtypes = [i64, ctypes.c_int, ctypes.c_int, vp, i32, vp, vp,
                                       ctypes.c_int, vp, i32, vp, vp, vp, vp]
    L.srs_debug_last_fallbacks.argtypes = [ctypes.POINTER(i64)]
    L.srs_debug_set_super_scan.argtypes = [i64]
    L.srs_debug_set_first_level.argtypes = [i64, i64, i64, i64, ctypes.c_int]
    L.srs_debug_last_first_level.argtypes = [ctypes.POINTER(i64)]
    L.srs_debug_last_local_counts.argtypes = [ctypes.POINTER(i64)]
    L.srs_debug_last_local_classes.argtypes = [ctypes.POINTER(i64)]
    L.srs_set_host_devices.argtypes = [i32, vp]
    L.srs_last_error.restype = ctypes.c_char_p
    L.srs_version.restype = ctypes.c_char_p
    L.srs_set_kernel_timing.argtypes = [ctypes.c_int]
    L.srs_kernel_stats.argtypes = [ctypes.c_char_p, ctypes.POINTER(i64),
                                   ctypes.POINTER(ctypes.c_double),
                                   ctypes.POINTER(ctypes.c_double)]
    L.srs_debug_alloc.argtypes = [ctypes.c_uint64, ctypes.c_int, ctypes.POINTER(vp)]
    L.srs_debug_free.argtypes = [vp]
    L.srs_alloc_device.argtypes = [ctypes.c_uint64, ctypes.POINTER(vp)]
    L.srs_free_device.argtypes = [vp]
    L.srs_debug_probe_write.argtypes = [vp, ctypes.c_uint64, ctypes.POINTER(ctypes.c_float)]
    L.srs_debug_workspace.argtypes = [ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint64),
                                      ctypes.POINTER(vp), ctypes.POINTER(ctypes.c_uint64)]
    _lib = L
    return L


def _check(rc: int):
    if rc != SRS_OK:
        raise SrsError(f"srs error {rc}: {lib().srs_last_error().decode()}")


def version() -> str:
    return lib().srs_version().decode()


def key_kind_of(dtype) -> int:
    dt = np.dtype(dtype)
    if dt not in _NP_KIND:
        raise TypeError(f"unsupported key dtype {dt}")
    return _NP_KIND[dt]


def _ptr_array(ptrs):
    return (ctypes.c_void_p * max(1, len(ptrs)))(*ptrs)


def _size_array(sizes):
    return (ctypes.c_uint32 * max(1, len(sizes)))(*sizes)


# --------------------------------------------------------------------------
# host arrays (drop-in semantics: in place, synchronous)
# --------------------------------------------------------------------------
def _leaf(cmp_sorter: str) -> int:
    if cmp_sorter not in _LEAF:
        raise ValueError(f"cmp_sorter must be one of {sorted(_LEAF)}")
    return _LEAF[cmp_sorter]


def sort_thresh(cmp_sort_threshold: int, keys: np.ndarray, *payloads: np.ndarray,
                up: bool = True, cmp_sorter: str = "insertion") -> None:
    """radix_sort::sort<Up, BitSorterSIMD, CmpSorter>(thresh, num, keys,
    payloads...) on host numpy arrays, in place. cmp_sorter: "insertion"
    (CmpSorterInsertionSort), "bramas" (sorted leaves as well) or "nosort"
    (CmpSorterNoSort: leaves of <= thresh keys stay in partition order)."""
    n = len(keys)
    for a in (keys,) + payloads:
        if not (isinstance(a, np.ndarray) and a.flags.c_contiguous and a.ndim == 1):
            raise ValueError("arrays must be 1-D C-contiguous numpy arrays")
        if len(a) != n:
            raise ValueError("all arrays must have the same length")
    _check(lib().srs_sort_soa_leaf(n, key_kind_of(keys.dtype), int(bool(up)),
                                   int(cmp_sort_threshold), _leaf(cmp_sorter), keys.ctypes.data,
                                   len(payloads), _ptr_array([p.ctypes.data for p in payloads]),
                                   _size_array([p.dtype.itemsize for p in payloads])))


def set_host_devices(devices=()) -> None:
    """GPUs the host-array sorts may use (srs_set_host_devices): () = the
    current device; [0, 1, ...] splits large host arrays over them (a device
    may repeat)."""
    d = [int(x) for x in devices]
    arr = (ctypes.c_int32 * max(1, len(d)))(*d)
    _check(lib().srs_set_host_devices(len(d), arr))


def sort(keys: np.ndarray, *payloads: np.ndarray, up: bool = True) -> None:
    """radix_sort::sort<Up>(num, keys, payloads...) (radixSort.hpp:1780): threshold 16."""
    sort_thresh(16, keys, *payloads, up=up)


def sort_combined(elements: np.ndarray, key_kind: int, up: bool = True,
                  cmp_sort_threshold: int = 16, cmp_sorter: str = "insertion") -> None:
    """radix_sort::sort(num, (DataElement<K, Ps...>*) combined): `elements` is a
    C-contiguous array whose rows are records (2-D uint8 (n, elem_size), or a
    structured / plain 1-D array); the key of kind `key_kind` is at byte 0."""
    if not elements.flags.c_contiguous:
        raise ValueError("elements must be C-contiguous")
    n = elements.shape[0]
    esz = elements.nbytes // n if n else elements.dtype.itemsize
    _check(lib().srs_sort_aos_leaf(n, int(key_kind), int(bool(up)), int(cmp_sort_threshold),
                                   _leaf(cmp_sorter), elements.ctypes.data, esz))


# --------------------------------------------------------------------------
# device tensors (torch, already in HBM; asynchronous on the current stream)
# --------------------------------------------------------------------------
_TORCH_KIND = None


def _torch_kind(t) -> int:
    global _TORCH_KIND
    import torch
    if _TORCH_KIND is None:
        _TORCH_KIND = {torch.uint8: KEY_U8, torch.int8: KEY_I8, torch.int16: KEY_I16,
                       torch.int32: KEY_I32, torch.int64: KEY_I64, torch.float32: KEY_F32,
                       torch.float64: KEY_F64}
        for name, k in (("uint16", KEY_U16), ("uint32", KEY_U32), ("uint64", KEY_U64)):
            if hasattr(torch, name):
                _TORCH_KIND[getattr(torch, name)] = k
    if t.dtype not in _TORCH_KIND:
        raise TypeError(f"unsupported key dtype {t.dtype}")
    return _TORCH_KIND[t.dtype]


def _stream_ptr(stream=None, device=None) -> int:
    import torch
    s = stream if stream is not None else torch.cuda.current_stream(device)
    return s.cuda_stream


def _on_device(t):
    """Context that makes t's GPU the current HIP device: the library picks
    its workspace (and torch its current stream) from the current device."""
    import torch
    return torch.cuda.device(t.device)


def _check_columns(keys, cols, what="tensors"):
    """Every column is a 1-D contiguous tensor on keys' GPU with keys' length."""
    for t in cols:
        if not (t.is_cuda and t.is_contiguous() and t.dim() == 1 and t.numel() == keys.numel()):
            raise ValueError(f"{what} must be 1-D contiguous device tensors of equal length")
        if t.device != keys.device:
            raise ValueError(f"{what} must all be on {keys.device} (got {t.device})")


def _check_matrix(cols):
    """The row-wise calls' 2-D columns, checked: (rows, row_len, stride(0))."""
    keys = cols[0]
    if keys.dim() != 2:
        raise ValueError("keys must be a 2-D tensor (rows, row_len)")
    rows, n = keys.shape
    # (a matrix of one row or of one column may report any stride for that dim)
    stride = keys.stride(0) if rows > 1 else max(n, 1)
    for t in cols:
        if not (t.is_cuda and t.dim() == 2 and tuple(t.shape) == (rows, n)):
            raise ValueError("columns must be 2-D device tensors of equal shape")
        if t.device != keys.device:
            raise ValueError(f"columns must all be on {keys.device} (got {t.device})")
        if (n > 1 and t.stride(1) != 1) or (rows > 1 and t.stride(0) != stride) or stride < n:
            raise ValueError("columns must have stride(1) == 1 and equal stride(0) >= row_len")
    return rows, n, stride


def _out_columns(out, cols, shape, message):
    """`out` allocated (`shape`, one tensor per column) or given and checked:
    at least prod(shape) elements, 1-D when shape is; else ValueError(message)."""
    import math
    import torch
    dev = cols[0].device
    if out is None:
        return tuple(torch.empty(shape, dtype=c.dtype, device=dev) for c in cols)
    out = tuple(out)
    if len(out) != len(cols):
        raise ValueError("out must hold keys_out followed by every payload_out")
    for o, i in zip(out, cols):
        if not (o.is_cuda and o.device == dev and o.is_contiguous() and
                (o.dim() == 1 or len(shape) > 1) and o.numel() >= math.prod(shape) and
                o.element_size() == i.element_size()):
            raise ValueError(message)
    return out


def _soa_args(keys, payloads, out, stream, idx=False):
    """The SoA device entry points' argument tail, from the keys pointer to
    the stream (out None: in place; idx False: no indices_out parameter)."""
    outs = (None, None) if out is None else (out[0].data_ptr(),
                                             _ptr_array([o.data_ptr() for o in out[1:]]))
    ind = () if idx is False else (None if idx is None else idx.data_ptr(),)
    return (keys.data_ptr(), len(payloads), _ptr_array([p.data_ptr() for p in payloads]),
            _size_array([p.element_size() for p in payloads])) + outs + ind + (
                _stream_ptr(stream, keys.device),)


def sort_device(keys, *payloads, up: bool = True, cmp_sort_threshold: int = 16,
                key_kind: int | None = None, out=None, stream=None,
                cmp_sorter: str = "insertion") -> None:
    """Sort device tensors. In place unless `out` = (keys_out, *payloads_out).
    `key_kind` overrides the kind derived from keys.dtype (e.g. torch.int64
    storage holding uint64 keys). Runs on keys' GPU, on `stream` or that
    GPU's current stream."""
    _check_columns(keys, (keys,) + payloads)
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    if out is not None:
        if len(out) != 1 + len(payloads):
            raise ValueError("out must hold keys_out followed by every payload_out")
        _check_columns(keys, tuple(out), "out tensors")
        for o, i in zip(out, (keys,) + payloads):
            if o.element_size() != i.element_size():
                raise ValueError("every out tensor must have its input's element size")
    with _on_device(keys):
        _check(lib().srs_sort_soa_device_leaf(keys.numel(), kind, int(bool(up)),
                                              int(cmp_sort_threshold), _leaf(cmp_sorter),
                                              *_soa_args(keys, payloads, out, stream)))


def sort_segments_device(keys, *payloads, bounds, up: bool = True, key_kind: int | None = None,
                         known_top_bits: int = 0, stream=None) -> None:
    """Sort every segment [bounds[i], bounds[i+1]) of the device columns
    independently, in place (srs_sort_segments_device). `bounds`: host
    sequence of non-decreasing offsets; `known_top_bits`: top transformed
    key bits every segment's keys are known to share."""
    _check_columns(keys, (keys,) + payloads)
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    b = (ctypes.c_int64 * len(bounds))(*[int(x) for x in bounds])
    with _on_device(keys):
        _check(lib().srs_sort_segments_device(
            keys.numel(), kind, int(bool(up)), keys.data_ptr(), len(payloads),
            _ptr_array([p.data_ptr() for p in payloads]),
            _size_array([p.element_size() for p in payloads]),
            max(0, len(bounds) - 1), b, int(known_top_bits), _stream_ptr(stream, keys.device)))


def sort_combined_device(elements, key_kind: int, up: bool = True,
                         cmp_sort_threshold: int = 16, out=None, stream=None,
                         cmp_sorter: str = "insertion") -> None:
    """DataElement array on the device: `elements` is a contiguous (n, elem_size)
    uint8 tensor (or any contiguous tensor whose first dim is the record)."""
    if not (elements.is_cuda and elements.is_contiguous()):
        raise ValueError("elements must be a contiguous device tensor")
    n = elements.shape[0]
    esz = elements.numel() * elements.element_size() // max(1, n)
    if out is not None:
        if not (out.is_cuda and out.is_contiguous() and out.device == elements.device and
                out.numel() * out.element_size() == elements.numel() * elements.element_size()):
            raise ValueError("out must be a contiguous tensor of the same bytes on the same GPU")
    with _on_device(elements):
        _check(lib().srs_sort_aos_device_leaf(n, int(key_kind), int(bool(up)),
                                              int(cmp_sort_threshold), _leaf(cmp_sorter),
                                              elements.data_ptr(), esz,
                                              None if out is None else out.data_ptr(),
                                              _stream_ptr(stream, elements.device)))


def topk_device(keys, *payloads, k: int, up: bool = True, key_kind: int | None = None, out=None,
                indices: bool = False, stream=None):
    """The first min(k, n) records of the stable sort of the device columns
    (srs_topk_soa_device): up=True the k smallest ascending, up=False the k
    largest descending, equal keys in input order. The inputs are not
    written. Returns (keys_out, *payloads_out[, indices]): `out` =
    (keys_out, *payloads_out) of at least min(k, n) elements each, or new
    tensors; with indices=True an int64 tensor of each record's input
    position follows. Runs on keys' GPU, on `stream` or its current stream."""
    import torch
    _check_columns(keys, (keys,) + payloads)
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    n = keys.numel()
    kk = max(0, min(int(k), n))
    out = _out_columns(out, (keys,) + payloads, (kk,),
                       "out tensors must be 1-D contiguous, on the keys' GPU, of at "
                       "least min(k, n) elements and of their input's element size")
    idx = torch.empty(kk, dtype=torch.int64, device=keys.device) if indices else None
    with _on_device(keys):
        _check(lib().srs_topk_soa_device(n, int(k), kind, int(bool(up)),
                                         *_soa_args(keys, payloads, out, stream, idx)))
    return out + ((idx,) if indices else ())


# the largest min(k, row_len) topk_rows_device's one-launch route takes for
# rows longer than 8192 records (kTopkRowsMaxK; srs_topk_rows_max_k())
TOPK_ROWS_MAX_K = 2048
TOPK_ROWS_RESIDENT, TOPK_ROWS_STREAM, TOPK_ROWS_LOOP = 0, 1, 2


def topk_rows_device(keys, *payloads, k: int, up: bool = True, key_kind: int | None = None,
                     out=None, indices: bool = False, stream=None):
    """topk_device on every row of a matrix in one call
    (srs_topk_rows_soa_device). The inputs are 2-D device tensors of equal
    shape (rows, row_len) with stride(1) == 1 and equal stride(0) >= row_len:
    a sliced view m[:, :L] works without a copy. Returns (keys_out,
    *payloads_out[, indices]) of shape (rows, min(k, row_len)): `out` =
    (keys_out, *payloads_out), contiguous, or new tensors; indices=True adds
    an int64 tensor of each record's position inside its row."""
    import torch
    cols = (keys,) + payloads
    rows, n, stride = _check_matrix(cols)
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    kk = max(0, min(int(k), n))
    out = _out_columns(out, cols, (rows, kk),
                       "out tensors must be contiguous, on the keys' GPU, of at least "
                       "rows * min(k, row_len) elements and of their input's element "
                       "size")
    idx = torch.empty((rows, kk), dtype=torch.int64, device=keys.device) if indices else None
    with _on_device(keys):
        _check(lib().srs_topk_rows_soa_device(rows, n, stride, int(k), kind, int(bool(up)),
                                              *_soa_args(keys, payloads, out, stream, idx)))
    return out + ((idx,) if indices else ())


SORT_ROWS_KERNEL, SORT_ROWS_LOCAL, SORT_ROWS_LEVELS = 0, 1, 2


def sort_rows_device(keys, *payloads, up: bool = True, key_kind: int | None = None,
                     indices: bool = False, out=None, stream=None):
    """Every row of a matrix sorted in one call, out of place
    (srs_sort_rows_soa_device): per row the stable sort by key, equal keys in
    input order. The inputs are 2-D device tensors of equal shape (rows,
    row_len) with stride(1) == 1 and equal stride(0) >= row_len (a sliced view
    m[:, :L] works without a copy); they are not written. Returns (keys_out,
    *payloads_out[, indices]) of shape (rows, row_len): `out` = (keys_out,
    *payloads_out), contiguous and clear of the inputs, or new tensors;
    indices=True adds an int64 tensor of each record's position inside its
    row."""
    import torch
    cols = (keys,) + payloads
    rows, n, stride = _check_matrix(cols)
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    out = _out_columns(out, cols, (rows, n),
                       "out tensors must be contiguous, on the keys' GPU, of at least "
                       "rows * row_len elements and of their input's element size")
    idx = torch.empty((rows, n), dtype=torch.int64, device=keys.device) if indices else None
    if rows == 0 or n == 0:  # (an empty tensor has no address to pass)
        return out + ((idx,) if indices else ())
    with _on_device(keys):
        _check(lib().srs_sort_rows_soa_device(rows, n, stride, kind, int(bool(up)),
                                              *_soa_args(keys, payloads, out, stream, idx)))
    return out + ((idx,) if indices else ())


def sort_ragged_device(keys, *payloads, offsets, up: bool = True, key_kind: int | None = None,
                       indices: bool = False, out=None, stream=None):
    """Every segment [offsets[i], offsets[i+1]) of 1-D device columns sorted in
    one call, out of place (srs_sort_ragged_soa_device): per segment the
    stable sort by key, equal keys in input order. `offsets` is an int64
    DEVICE tensor of num_segments + 1 non-decreasing values within [0,
    len(keys)] on the keys' GPU (TypeError otherwise); it is read on the
    device, and offsets that decrease or leave the columns raise SrsError.
    Returns (keys_out, *payloads_out[, indices]) of the inputs' shape: `out` =
    (keys_out, *payloads_out), clear of the inputs, or new tensors, whose
    records outside the covered range are left as allocated; indices=True adds
    an int64 tensor of each record's position inside its segment."""
    import torch
    cols = (keys,) + payloads
    _check_columns(keys, cols)
    if not (isinstance(offsets, torch.Tensor) and offsets.dtype == torch.int64 and
            offsets.is_cuda and offsets.device == keys.device):
        raise TypeError("offsets must be an int64 device tensor on the keys' GPU")
    if not (offsets.dim() == 1 and offsets.is_contiguous()):
        raise ValueError("offsets must be 1-D and contiguous")
    n, nseg = keys.numel(), offsets.numel() - 1
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    if out is None:
        out = tuple(torch.empty_like(c) for c in cols)
    else:
        out = tuple(out)
        if len(out) != len(cols):
            raise ValueError("out must hold keys_out followed by every payload_out")
        _check_columns(keys, out, "out tensors")
        for o, i in zip(out, cols):
            if o.element_size() != i.element_size():
                raise ValueError("every out tensor must have its input's element size")
    idx = torch.empty(n, dtype=torch.int64, device=keys.device) if indices else None
    if n == 0 or nseg <= 0:  # (an empty tensor has no address to pass)
        return out + ((idx,) if indices else ())
    with _on_device(keys):
        _check(lib().srs_sort_ragged_soa_device(n, nseg, offsets.data_ptr(), kind, int(bool(up)),
                                                *_soa_args(keys, payloads, out, stream, idx)))
    return out + ((idx,) if indices else ())


TOPK_RAGGED_KERNELS, TOPK_RAGGED_SORT = 0, 1


def topk_ragged_device(keys, *payloads, offsets, k: int, up: bool = True,
                       key_kind: int | None = None, indices: bool = False, out=None, stream=None):
    """The first min(k, len) records of every segment [offsets[i],
    offsets[i+1]) of 1-D device columns in one call
    (srs_topk_ragged_soa_device): per segment the head of its stable sort by
    key, equal keys in input order; up=False the largest, descending.
    `offsets` is sort_ragged_device's: an int64 DEVICE tensor of num_segments
    + 1 non-decreasing values within [0, len(keys)] on the keys' GPU
    (TypeError otherwise), read on the device; offsets that decrease or leave
    the columns raise SrsError. Returns (keys_out, *payloads_out[, indices],
    counts): the columns of shape (num_segments, k), result j of segment i at
    [i, j] for j < counts[i] = min(k, len_i); the other slots are not
    written. New tensors are zero-filled (indices: -1); `out` = (keys_out,
    *payloads_out), contiguous with at least num_segments * k elements and
    clear of the inputs, keeps its bytes there. counts is a new int64 tensor
    of shape (num_segments,)."""
    import torch
    cols = (keys,) + payloads
    _check_columns(keys, cols)
    if not (isinstance(offsets, torch.Tensor) and offsets.dtype == torch.int64 and
            offsets.is_cuda and offsets.device == keys.device):
        raise TypeError("offsets must be an int64 device tensor on the keys' GPU")
    if not (offsets.dim() == 1 and offsets.is_contiguous()):
        raise ValueError("offsets must be 1-D and contiguous")
    n, nseg, k = keys.numel(), max(0, offsets.numel() - 1), max(0, int(k))
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    dev = keys.device
    if out is None:
        out = tuple(torch.zeros((nseg, k), dtype=c.dtype, device=dev) for c in cols)
    else:
        out = _out_columns(out, cols, (nseg, k),
                           "out tensors must be contiguous, on the keys' GPU, of at least "
                           "num_segments * k elements and of their input's element size")
    idx = torch.full((nseg, k), -1, dtype=torch.int64, device=dev) if indices else None
    counts = torch.zeros(nseg, dtype=torch.int64, device=dev)
    if n == 0 or nseg == 0 or k == 0:  # (an empty tensor has no address to pass)
        return out + ((idx,) if indices else ()) + (counts,)
    with _on_device(keys):
        _check(lib().srs_topk_ragged_soa_device(
            n, nseg, offsets.data_ptr(), k, kind, int(bool(up)), keys.data_ptr(), len(payloads),
            _ptr_array([p.data_ptr() for p in payloads]),
            _size_array([p.element_size() for p in payloads]), out[0].data_ptr(),
            _ptr_array([o.data_ptr() for o in out[1:]]), None if idx is None else idx.data_ptr(),
            counts.data_ptr(), _stream_ptr(stream, dev)))
    return out + ((idx,) if indices else ()) + (counts,)


UniqueResult = collections.namedtuple("UniqueResult",
                                      "unique sorted offsets counts index inverse")


def unique_device(keys, *payloads, up: bool = True, key_kind: int | None = None,
                  return_sorted: bool = False, return_offsets: bool = False,
                  return_counts: bool = False, return_index: bool = False,
                  return_inverse: bool = False, stream=None):
    """The distinct keys of a 1-D device column in one call
    (srs_unique_soa_device), in sorted order (floats in the total order: -0.0
    and +0.0 are two keys; up=False descending). Returns UniqueResult(unique,
    sorted, offsets, counts, index, inverse); fields not asked for are None.
    unique: the U distinct keys. sorted (return_sorted): (keys_sorted,
    *payloads_sorted), the stable sort of the inputs. offsets
    (return_offsets): int64 of U + 1 values, where each group starts in the
    sorted columns and len(keys) last, usable as the `offsets` of
    sort_ragged_device / topk_ragged_device over `sorted`. counts
    (return_counts): the groups' sizes. index (return_index): the first
    occurrence of every unique key in the input. inverse (return_inverse):
    int64 of the input's shape, unique[inverse] == keys. Payloads need
    return_sorted=True (ValueError). The inputs are not written; the call
    waits once, for U."""
    import torch
    cols = (keys,) + payloads
    _check_columns(keys, cols)
    if payloads and not return_sorted:
        raise ValueError("payloads are only moved with return_sorted=True")
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    n, dev = keys.numel(), keys.device
    i64 = dict(dtype=torch.int64, device=dev)
    want_offs = return_offsets or return_counts or return_index
    uniq = torch.empty_like(keys)
    srt = tuple(torch.empty_like(c) for c in cols) if return_sorted else None
    offs = torch.empty(n + 1, **i64) if want_offs else None
    idx = torch.empty(n, **i64) if return_index else None
    inv = torch.empty(keys.shape, **i64) if return_inverse else None
    nu = ctypes.c_int64(0)
    if n > 0:  # (an empty tensor has no address to pass)
        with _on_device(keys):
            _check(lib().srs_unique_soa_device(
                n, kind, int(bool(up)), keys.data_ptr(), len(payloads),
                _ptr_array([p.data_ptr() for p in payloads]) if payloads else None,
                _size_array([p.element_size() for p in payloads]) if payloads else None,
                srt[0].data_ptr() if srt else None,
                _ptr_array([o.data_ptr() for o in srt[1:]]) if srt and payloads else None,
                None if idx is None else idx.data_ptr(), uniq.data_ptr(),
                None if offs is None else offs.data_ptr(),
                None if inv is None else inv.data_ptr(), None, ctypes.byref(nu),
                _stream_ptr(stream, dev)))
    elif offs is not None:
        offs.zero_()
    u = int(nu.value)
    if offs is not None:
        offs = offs[:u + 1]
    return UniqueResult(
        unique=uniq[:u], sorted=srt, offsets=offs if return_offsets else None,
        counts=offs[1:] - offs[:-1] if return_counts else None,
        index=idx[offs[:-1]] if return_index else None, inverse=inv)


def debug_last_unique():
    """(launches the unique stage queued after the sort, its host read-backs,
    1 if an index column travelled through the sort, 1 if the sorted columns
    went to the workspace) of the last unique_device on the current device."""
    c = (ctypes.c_int64 * 4)()
    _check(lib().srs_debug_last_unique(c))
    return tuple(int(x) for x in c)


SEARCH_QUERIES_SORTED = 1  # srs_c_api.h: SRS_SEARCH_QUERIES_SORTED
SEARCH_DIRECT, SEARCH_SORT = 0, 1
# the search kernel's shape (srs_c_api.h): queries per workgroup, the slots of
# its LDS sample, the most keys of a table range that is staged whole
SEARCH_QUERY_TILE, SEARCH_LDS_SAMPLES, SEARCH_LDS_RANGE = 1024, 2048, 2047


def searchsorted_device(sorted_keys, queries, *, side: str = "left", up: bool = True,
                        key_kind: int | None = None, offsets=None, query_segments=None,
                        queries_sorted: bool = False, out=None, stream=None):
    """Where query keys fall in a sorted 1-D device column
    (srs_search_sorted_device), in the library's key order: floats in the
    total order (-0.0 before +0.0), up=False for a table sorted descending,
    key_kind for uint64 keys held as int64. `sorted_keys` is what sort_device,
    the row-wise and ragged calls or unique_device (`unique`, `sorted`) wrote;
    `queries` a contiguous device tensor of any shape with the table's dtype
    (TypeError otherwise). side="left": the number of table keys before the
    query; "right": the number of keys before or equal to it; "both": (lower,
    upper), whose difference is the number of matches. The results are int64
    tensors of the queries' shape (`out`: a contiguous int64 tensor of at
    least that many elements, or a pair of them for "both"). With
    unique_device(keys).unique as the table, "left" is the group number of
    every query that is present.
    Segmented: `offsets` (the ragged calls' int64 DEVICE tensor of
    num_segments + 1 values) and `query_segments` (int64 device tensor of the
    queries' shape) search every query in its own segment; the results are
    positions inside the segment. A query with a segment id outside [0,
    num_segments) or a segment with bad offsets receives -1, and a `bad` count
    tensor (device, 1 element, not read here) is returned last.
    queries_sorted=True is a hint that the queries are already in key order;
    a wrong hint costs time, never a result."""
    import torch
    if side not in ("left", "right", "both"):
        raise ValueError('side must be "left", "right" or "both"')
    if not (isinstance(sorted_keys, torch.Tensor) and sorted_keys.is_cuda and
            sorted_keys.dim() == 1 and sorted_keys.is_contiguous()):
        raise ValueError("sorted_keys must be a 1-D contiguous device tensor")
    if not (isinstance(queries, torch.Tensor) and queries.dtype == sorted_keys.dtype):
        raise TypeError("queries must be a tensor of the table's dtype")
    dev = sorted_keys.device
    if not (queries.is_cuda and queries.device == dev and queries.is_contiguous()):
        raise ValueError("queries must be a contiguous device tensor on the table's GPU")
    seg = offsets is not None or query_segments is not None
    if seg:
        for name, t in (("offsets", offsets), ("query_segments", query_segments)):
            if not (isinstance(t, torch.Tensor) and t.dtype == torch.int64 and t.is_cuda and
                    t.device == dev):
                raise TypeError(f"{name} must be an int64 device tensor on the keys' GPU")
        if not (offsets.dim() == 1 and offsets.is_contiguous() and offsets.numel() >= 2):
            raise ValueError("offsets must be 1-D, contiguous and hold num_segments + 1 >= 2 values")
        if not (query_segments.is_contiguous() and query_segments.numel() == queries.numel()):
            raise ValueError("query_segments must be contiguous and of the queries' shape")
    kind = _torch_kind(sorted_keys) if key_kind is None else int(key_kind)
    n, nq = sorted_keys.numel(), queries.numel()
    nres = 2 if side == "both" else 1
    if out is None:
        res = tuple(torch.empty(queries.shape, dtype=torch.int64, device=dev) for _ in range(nres))
    else:
        res = tuple(out) if side == "both" else (out,)
        if len(res) != nres:
            raise ValueError('out must be one tensor, or (lower, upper) for side="both"')
        for o in res:
            if not (isinstance(o, torch.Tensor) and o.dtype == torch.int64 and o.is_cuda and
                    o.device == dev and o.is_contiguous() and o.numel() >= nq):
                raise ValueError("out tensors must be contiguous int64 device tensors on the "
                                 "table's GPU with at least as many elements as queries")
    lower = res[0] if side != "right" else None
    upper = res[-1] if side != "left" else None
    bad = torch.zeros(1, dtype=torch.int64, device=dev) if seg else None
    if nq > 0:  # (an empty tensor has no address to pass)
        with _on_device(sorted_keys):
            _check(lib().srs_search_sorted_device(
                n, kind, int(bool(up)), sorted_keys.data_ptr() if n > 0 else None,
                offsets.numel() - 1 if seg else 0, offsets.data_ptr() if seg else None, nq,
                queries.data_ptr(), query_segments.data_ptr() if seg else None,
                None if lower is None else lower.data_ptr(),
                None if upper is None else upper.data_ptr(),
                None if bad is None else bad.data_ptr(),
                SEARCH_QUERIES_SORTED if queries_sorted else 0, _stream_ptr(stream, dev)))
    ret = res[0] if nres == 1 else res
    if seg:
        return (ret, bad) if nres == 1 else res + (bad,)
    return ret


def debug_set_search_route(route: int) -> None:
    """Test hook (srs_debug_set_search_route): -1 the library's rule, 0 the
    kernel on the caller's queries, 1 sort the queries first. The segmented
    form ignores it."""
    _check(lib().srs_debug_set_search_route(int(route)))


def debug_last_search():
    """(route taken, launches of the search stage, host read-backs or -1 on
    the sort route, 1 if the call sorted the queries) of the last
    searchsorted_device on the current device."""
    c = (ctypes.c_int64 * 4)()
    _check(lib().srs_debug_last_search(c))
    return tuple(int(x) for x in c)


MERGE_TILE = 4096  # srs_c_api.h: SRS_MERGE_TILE, output records per workgroup


def merge_device(a, b, *, up: bool = True, key_kind: int | None = None, indices: bool = False,
                 out=None, stream=None):
    """Two sorted record sets merged stably in one call (srs_merge_soa_device).
    `a` = (a_keys, *a_payloads) and `b` = (b_keys, *b_payloads) are 1-D
    contiguous device columns with the same dtypes, column by column, on the
    same GPU (TypeError / ValueError otherwise), each sorted in the library's
    key order: what sort_device, the row-wise and ragged calls, unique_device
    or an earlier merge wrote (floats in the total order; up=False: both
    sorted descending; key_kind for uint64 keys held as int64). Returns
    (keys, *payloads[, source]) of len(a) + len(b) records: the stable sort of
    a followed by b, a's records first among equal keys. `out` = (keys_out,
    *payloads_out) of at least that many elements each, or new tensors; with
    indices=True an int64 tensor follows that holds every output record's
    position in the concatenation (i for a[i], len(a) + j for b[j]). The
    inputs are not written and must not overlap the outputs. The call does not
    wait on the host."""
    import torch
    a, b = tuple(a), tuple(b)
    if not a or len(a) != len(b):
        raise ValueError("a and b must hold a key column and the same number of payload columns")
    for t in a + b:
        if not isinstance(t, torch.Tensor):
            raise TypeError("a and b must hold tensors")
    _check_columns(a[0], a, "a's columns")
    _check_columns(b[0], b, "b's columns")
    for x, y in zip(a, b):
        if x.dtype != y.dtype:
            raise TypeError(f"a and b must have the same column dtypes ({x.dtype} and {y.dtype})")
    dev = a[0].device
    if b[0].device != dev:
        raise ValueError(f"a and b must be on the same GPU ({dev} and {b[0].device})")
    kind = _torch_kind(a[0]) if key_kind is None else int(key_kind)
    na, nb = a[0].numel(), b[0].numel()
    n = na + nb
    out = _out_columns(out, a, (n,),
                       "out tensors must be 1-D contiguous, on the inputs' GPU, of at least "
                       "len(a) + len(b) elements and of their input's element size")
    src = torch.empty(n, dtype=torch.int64, device=dev) if indices else None
    np_ = len(a) - 1
    if n > 0:  # (an empty tensor has no address to pass)
        with _on_device(a[0]):
            _check(lib().srs_merge_soa_device(
                na, nb, kind, int(bool(up)), a[0].data_ptr() if na else None,
                b[0].data_ptr() if nb else None, np_,
                _ptr_array([p.data_ptr() for p in a[1:]]) if np_ and na else None,
                _ptr_array([p.data_ptr() for p in b[1:]]) if np_ and nb else None,
                _size_array([p.element_size() for p in a[1:]]) if np_ else None,
                out[0].data_ptr(), _ptr_array([o.data_ptr() for o in out[1:]]) if np_ else None,
                None if src is None else src.data_ptr(), _stream_ptr(stream, dev)))
    return out + ((src,) if indices else ())


def debug_last_merge():
    """(launches queued, host read-backs (0), tiles, bytes of the workspace
    buffers used) of the last merge_device on the current device."""
    c = (ctypes.c_int64 * 4)()
    _check(lib().srs_debug_last_merge(c))
    return tuple(int(x) for x in c)


def topk_combined_device(elements, key_kind: int, k: int, up: bool = True, out=None,
                         indices: bool = False, stream=None):
    """topk_device on a DataElement array (srs_topk_aos_device): `elements`
    as for sort_combined_device. Returns elements_out (the first min(k, n)
    records; `out` or a new tensor), or (elements_out, indices)."""
    import torch
    if not (elements.is_cuda and elements.is_contiguous()):
        raise ValueError("elements must be a contiguous device tensor")
    n = elements.shape[0]
    esz = elements.numel() * elements.element_size() // max(1, n)
    kk = max(0, min(int(k), n))
    if out is None:
        out = torch.empty((kk,) + tuple(elements.shape[1:]), dtype=elements.dtype,
                          device=elements.device)
    elif not (out.is_cuda and out.is_contiguous() and out.device == elements.device and
              out.numel() * out.element_size() >= kk * esz):
        raise ValueError("out must be a contiguous tensor of at least min(k, n) records on the "
                         "same GPU")
    idx = torch.empty(kk, dtype=torch.int64, device=elements.device) if indices else None
    with _on_device(elements):
        _check(lib().srs_topk_aos_device(n, int(k), int(key_kind), int(bool(up)),
                                         elements.data_ptr(), esz, out.data_ptr(),
                                         None if idx is None else idx.data_ptr(),
                                         _stream_ptr(stream, elements.device)))
    return (out, idx) if indices else out


def fill_synthetic_device(keys, *payloads, seed: int = 42 << 32, first_index: int = 0,
                          key_kind: int | None = None, stream=None) -> None:
    """keys[i] = splitmix64(seed + first_index + i) (see srs_c_api.h);
    payloads are functions of the key."""
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    _check_columns(keys, (keys,) + payloads)
    with _on_device(keys):
        _check(lib().srs_fill_synthetic_device(keys.numel(), kind, seed, first_index,
                                               keys.data_ptr(), len(payloads),
                                               _ptr_array([p.data_ptr() for p in payloads]),
                                               _size_array([p.element_size() for p in payloads]),
                                               _stream_ptr(stream, keys.device)))


# --------------------------------------------------------------------------
# multi-GPU shard primitives (the shard sort itself: srs_amd.shard)
# --------------------------------------------------------------------------
def key_histogram_device(keys, hist, bits: int, up: bool = True, key_kind: int | None = None,
                         stream=None) -> None:
    """Adds the histogram of the transformed top `bits` key bits into `hist`
    (int64 device tensor of 2^bits entries)."""
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    if hist.numel() != (1 << bits) or hist.element_size() != 8 or not hist.is_cuda:
        raise ValueError("hist must be a device tensor of 2^bits 64-bit counters")
    _check_columns(keys, (keys,))
    if hist.device != keys.device or not hist.is_contiguous():
        raise ValueError("hist must be contiguous and on the keys' GPU")
    with _on_device(keys):
        _check(lib().srs_key_histogram_device(keys.numel(), kind, int(bool(up)), keys.data_ptr(),
                                              int(bits), hist.data_ptr(),
                                              _stream_ptr(stream, keys.device)))


def partition_device(keys, payloads, bits: int, part_of_bucket, num_parts: int, out,
                     up: bool = True, key_kind: int | None = None, stream=None):
    """Stable partition by destination group (srs_partition_device).
    `part_of_bucket`: int32 device tensor of 2^bits entries. `out` =
    (keys_out, *payloads_out). Returns the host list of group sizes."""
    kind = _torch_kind(keys) if key_kind is None else int(key_kind)
    if part_of_bucket.dtype.itemsize != 4 or part_of_bucket.numel() != (1 << bits):
        raise ValueError("part_of_bucket must hold 2^bits int32 entries")
    pays = list(payloads)
    _check_columns(keys, [keys] + pays)
    if not (part_of_bucket.is_cuda and part_of_bucket.device == keys.device and
            part_of_bucket.is_contiguous()):
        raise ValueError("part_of_bucket must be a contiguous tensor on the keys' GPU")
    if len(out) != 1 + len(pays):
        raise ValueError("out must hold keys_out followed by every payload_out")
    for o, i in zip(out, [keys] + pays):
        if not (o.is_cuda and o.device == keys.device and o.is_contiguous() and o.dim() == 1 and
                o.numel() >= keys.numel() and o.element_size() == i.element_size()):
            raise ValueError("out tensors must be contiguous, on the keys' GPU, at least as long "
                             "as the input and of its element size")
    counts = (ctypes.c_int64 * num_parts)()
    with _on_device(keys):
        _check(lib().srs_partition_device(
            keys.numel(), kind, int(bool(up)), keys.data_ptr(), len(pays),
            _ptr_array([p.data_ptr() for p in pays]), _size_array([p.element_size() for p in pays]),
            int(bits), part_of_bucket.data_ptr(), int(num_parts), out[0].data_ptr(),
            _ptr_array([o.data_ptr() for o in out[1:]]), counts,
            _stream_ptr(stream, keys.device)))
    return [int(c) for c in counts]


# --------------------------------------------------------------------------
# kernel timing (HIP events around every launch, see srs_c_api.h)
# --------------------------------------------------------------------------
def set_kernel_timing(enable) -> None:
    """True / 1: HIP events around every launch; 2: around the scatter
    launches only (the timed region's roofline kernel); False / 0: off."""
    _check(lib().srs_set_kernel_timing(2 if enable == 2 else int(bool(enable))))


def reset_kernel_stats() -> None:
    _check(lib().srs_reset_kernel_stats())


def kernel_stats(name: str):
    """(launches, total_ms, elements) for a kernel family since the last reset."""
    n = ctypes.c_int64()
    ms = ctypes.c_double()
    el = ctypes.c_double()
    _check(lib().srs_kernel_stats(name.encode(), ctypes.byref(n), ctypes.byref(ms),
                                  ctypes.byref(el)))
    return n.value, ms.value, el.value


def level_counts():
    """(all, tile-pair, tile-pair without the tile-offset pass): the global
    levels run in this process so far (srs_debug_level_counts). Take the
    difference around a call to see which path its levels took."""
    c = (ctypes.c_int64 * 3)()
    _check(lib().srs_debug_level_counts(c))
    return tuple(int(x) for x in c)


def last_fallbacks():
    """(stable, lsd): local segments the last sort on the current device
    handed to the stable / LSD fallback kernels (synchronizes the device)."""
    c = (ctypes.c_int64 * 2)()
    _check(lib().srs_debug_last_fallbacks(c))
    return int(c[0]), int(c[1])


def last_local_counts():
    """(local segments, of which handed from the direct to the fast kernel)
    of the last sort on the current device (synchronizes the device)."""
    c = (ctypes.c_int64 * 2)()
    _check(lib().srs_debug_last_local_counts(c))
    return int(c[0]), int(c[1])


def last_local_classes():
    """(small-class segments, large-class segments, of each the ones the
    direct kernel handed to the fast kernel) of the last sort on the current
    device (synchronizes the device)."""
    c = (ctypes.c_int64 * 4)()
    _check(lib().srs_debug_last_local_classes(c))
    return tuple(int(x) for x in c)


class _DeviceBlock:
    """srs_alloc_device memory exposed through __cuda_array_interface__; freed
    when the last tensor viewing it goes away."""

    def __init__(self, n, dtype, device):
        import torch
        self.device = torch.device(device)
        self.dtype = dtype
        self.n = int(n)
        nbytes = self.n * torch.empty(0, dtype=dtype).element_size()
        p = ctypes.c_void_p()
        with torch.cuda.device(self.device):
            _check(lib().srs_alloc_device(nbytes, ctypes.byref(p)))
        self.ptr = int(p.value or 0)
        typestr = {torch.int64: "<i8", torch.int32: "<i4", torch.float32: "<f4",
                   torch.float64: "<f8", torch.int16: "<i2", torch.uint8: "|u1",
                   torch.int8: "|i1"}[dtype]
        self.__cuda_array_interface__ = {"shape": (self.n,), "typestr": typestr,
                                         "data": (self.ptr, False), "version": 2,
                                         "strides": None}

    def __del__(self):
        if getattr(self, "ptr", 0):
            try:
                lib().srs_free_device(ctypes.c_void_p(self.ptr))
            except Exception:
                pass
            self.ptr = 0


def empty_device(n: int, dtype, device="cuda"):
    """A 1-D torch tensor of n elements in memory from srs_alloc_device
    (probed placement): for arrays the sort writes."""
    import torch
    blk = _DeviceBlock(n, dtype, device)
    t = torch.as_tensor(blk, device=blk.device)
    if t.data_ptr() != blk.ptr:
        raise SrsError("empty_device: torch copied the block instead of viewing it")
    t._srs_block = blk  # (keeps the memory alive as long as the tensor)
    return t


def debug_alloc(nbytes: int, mode: int = 0) -> int:
    """Raw device allocation on the current device (srs_debug_alloc; mode 0
    hipMalloc, 1 contiguous, 2 VMM at 1 GiB alignment): the address."""
    p = ctypes.c_void_p()
    _check(lib().srs_debug_alloc(int(nbytes), int(mode), ctypes.byref(p)))
    return int(p.value)


def debug_free(ptr: int) -> None:
    _check(lib().srs_debug_free(ctypes.c_void_p(ptr)))


def debug_set_super_scan(min_groups: int) -> None:
    """Scan groups from which a one-segment level takes the super-group
    column scan (srs_debug_set_super_scan; 0 = the default, 256)."""
    _check(lib().srs_debug_set_super_scan(int(min_groups)))


def debug_set_first_level(general_min_n: int = 0, balanced_min_n: int = 0, stripe_min_n: int = 0,
                          stripe_pairs: int = 0, first_bits: int = 0) -> None:
    """The first level's size rules, process-wide (srs_debug_set_first_level):
    records from which a sort starts plain, takes the key sample, takes the
    stripe level; the stripe length in tile pairs of 8192 records; the plain
    stripe level's digit width. 0 (or less) is a field's default: called
    without arguments it restores every default, which a test does in a
    `finally` or a fixture."""
    _check(lib().srs_debug_set_first_level(int(general_min_n), int(balanced_min_n),
                                           int(stripe_min_n), int(stripe_pairs),
                                           int(first_bits)))


FIRST_LEVEL_FIELDS = ("start", "kind", "stripes", "stripe_count", "first_bits", "gathered_tiles")
START_PLAIN, START_MID, START_MID_LEVEL = 0, 1, 2
LEVEL_PLAIN, LEVEL_TABLE16, LEVEL_RANGES, LEVEL_SPLIT_TABLE = 0, 1, 2, 3


def debug_last_first_level() -> dict:
    """What the last sort above the single-workgroup capacity did on the
    current device (srs_debug_last_first_level), by FIRST_LEVEL_FIELDS: its
    start (START_*; -1: no such sort yet), the first level's kind (LEVEL_*),
    whether the stripe and gathered levels ran, the stripe count, the stripe
    level's digit width, the gathered level's tile count."""
    c = (ctypes.c_int64 * 6)()
    _check(lib().srs_debug_last_first_level(c))
    return dict(zip(FIRST_LEVEL_FIELDS, (int(x) for x in c)))


def debug_set_topk_candidates(max_candidates: int) -> None:
    """Boundary-bucket size at which the top-k select stops refining
    (srs_debug_set_topk_candidates; 0 = the default, 2^20)."""
    _check(lib().srs_debug_set_topk_candidates(int(max_candidates)))


def debug_last_topk():
    """(select passes, records handed to the finishing sort, 1 if the call
    sorted everything) of the last top-k on the current device (synchronizes
    the device)."""
    c = (ctypes.c_int64 * 3)()
    _check(lib().srs_debug_last_topk(c))
    return int(c[0]), int(c[1]), int(c[2])


def debug_set_topk_rows_route(route: int) -> None:
    """Route of topk_rows_device, process-wide (srs_debug_set_topk_rows_route):
    -1 the library's rule, TOPK_ROWS_RESIDENT / _STREAM / _LOOP force one."""
    _check(lib().srs_debug_set_topk_rows_route(int(route)))


def debug_last_topk_rows():
    """(route, kernel launches or -1 on the loop route, most select passes
    any row took, host read-backs) of the last topk_rows_device on the
    current device (synchronizes the device)."""
    c = (ctypes.c_int64 * 4)()
    _check(lib().srs_debug_last_topk_rows(c))
    return tuple(int(x) for x in c)


def debug_set_sort_rows_route(route: int) -> None:
    """Route of sort_rows_device, process-wide (srs_debug_set_sort_rows_route):
    -1 the library's rule, SORT_ROWS_KERNEL / _LOCAL / _LEVELS force one."""
    _check(lib().srs_debug_set_sort_rows_route(int(route)))


def debug_last_sort_rows():
    """(route, kernel launches or -1 where they are not counted, host
    read-backs, 1 if the prepare pass ran) of the last sort_rows_device on the
    current device."""
    c = (ctypes.c_int64 * 4)()
    _check(lib().srs_debug_last_sort_rows(c))
    return tuple(int(x) for x in c)


def debug_set_sort_ragged_short_max(length: int) -> None:
    """The longest segment sort_ragged_device leaves to its wave-per-segment
    kernel, process-wide (srs_debug_set_sort_ragged_short_max): -1 the default
    (256), 0 that kernel off, 1 .. 256 the maximum."""
    _check(lib().srs_debug_set_sort_ragged_short_max(int(length)))


def debug_last_sort_ragged():
    """(segments left to the short kernel, small-class / large-class / big list
    lengths as first read back, host read-backs, 1 if the prepare pass ran) of
    the last sort_ragged_device on the current device."""
    c = (ctypes.c_int64 * 6)()
    _check(lib().srs_debug_last_sort_ragged(c))
    return tuple(int(x) for x in c)


def debug_set_topk_ragged_route(route: int) -> None:
    """Route of topk_ragged_device, process-wide
    (srs_debug_set_topk_ragged_route): -1 the library's rule,
    TOPK_RAGGED_KERNELS / _SORT force one."""
    _check(lib().srs_debug_set_topk_ragged_route(int(route)))


def debug_last_topk_ragged():
    """(route, segments the wave kernel owned, segments listed as long, most
    select passes any segment took, host read-backs, kernel launches or -1 on
    the sort route) of the last topk_ragged_device on the current device
    (synchronizes the device)."""
    c = (ctypes.c_int64 * 6)()
    _check(lib().srs_debug_last_topk_ragged(c))
    return tuple(int(x) for x in c)


def debug_probe_write(ptr: int, nbytes: int) -> float:
    """ms of one pass of the scatter's write pattern over device memory."""
    ms = ctypes.c_float()
    _check(lib().srs_debug_probe_write(ctypes.c_void_p(ptr), int(nbytes), ctypes.byref(ms)))
    return float(ms.value)


def debug_workspace():
    """(tmp address, bytes, tmp2 address, bytes) of the current device."""
    a, b = ctypes.c_void_p(), ctypes.c_void_p()
    na, nb = ctypes.c_uint64(), ctypes.c_uint64()
    _check(lib().srs_debug_workspace(ctypes.byref(a), ctypes.byref(na), ctypes.byref(b),
                                     ctypes.byref(nb)))
    return int(a.value or 0), int(na.value), int(b.value or 0), int(nb.value)


def release_workspace() -> None:
    _check(lib().srs_release_workspace())
