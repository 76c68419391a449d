#!/usr/bin/env python3
"""Row-wise sort on one GPU.

For every shape (rows x row_len) and both column sets -- f32 keys with
indices, u64 keys + one u64 payload -- the warm sort_rows_device call is timed
on the library's own rule and forced on every route that can take the shape
(the rows kernel, the local lists, the global levels). Beside it, in the same
process:

  * what a caller had before this entry point: topk_rows_device(k = row_len)
    (rows longer than 8192 records take its row-by-row loop: timed on at most
    --loop-rows rows, scaled up and marked), and sort_segments_device on a
    dense copy with host bounds, timed with the copy, the iota column that
    stands in for the indices, and the bounds upload;
  * torch.sort(dim=-1, stable=True) plus the payload gather, as a yardstick;
  * the floor: the bytes of the route's byte model over the rate a device
    copy of 1 GiB reaches.

Every figure is the median wall time of --reps calls that end in a stream
synchronise; min and max are kept, and spread_pct is (max - min) / median of
the auto line. One JSON line per (shape, columns) on stdout (and in --out).
--sweep adds row lengths 256 .. 8192 at 2^26 records, for kSortRowsLocalMin.
"""
import argparse
import ctypes
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simd-radix-sort_amd", "python"))

SHAPES = "1048576x64,65536x1024,16384x8192,4096x32768,256x1048576"
SWEEP = ",".join(f"{(1 << 26) // n}x{n}" for n in (256, 384, 512, 768, 1024, 1536, 2048, 3072,
                                                   4096, 6144, 8192))
ROUTES = {0: "kernel", 1: "local", 2: "levels"}
CAP = 8192


def model_bytes(route, rows, n, key_bytes, rec_bytes, idx, prepared):
    """Bytes the route moves through HBM."""
    N = rows * n
    out = rec_bytes + (8 if idx else 0)
    if route == 0:
        return N * (rec_bytes + out)
    prep = N * (rec_bytes + out) if prepared else 0
    if route == 1:
        return prep + N * 2 * out
    levels = max(1, math.ceil(math.log2(n / 7808) / 9))
    return prep + N * (levels * (key_bytes + 2 * out) + 2 * out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="rows x row_len, comma separated")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--cols", default="f32_idx,u64_u64")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-rows", type=int, default=16)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--no-parent", action="store_true", help="skip the pre-existing entry points")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import srs_amd
    if not torch.cuda.is_available():
        sys.exit("sort_rows_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    out_f = open(args.out, "w") if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out_f:
            out_f.write(line + "\n")
            out_f.flush()

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def median_ms(fn):
        for _ in range(args.warmup):
            fn()
        t = [timed(fn) for _ in range(args.reps)]
        return round(statistics.median(t), 4), round(min(t), 4), round(max(t), 4)

    # the copy rate (read + written bytes per second) of 1 GiB
    a = torch.empty(1 << 27, dtype=torch.int64, device=dev)
    b = torch.empty_like(a)
    copy_ms = median_ms(lambda: b.copy_(a))[0]
    copy_rate = 2 * a.numel() * 8 / (copy_ms * 1e-3)
    del a, b
    torch.cuda.empty_cache()

    def measure(rows, n, cols):
        if cols == "f32_idx":
            kind, keys = srs_amd.KEY_F32, torch.randn((rows, n), dtype=torch.float32, device=dev)
            pays, indices = (), True
        else:
            kind = srs_amd.KEY_U64
            keys = torch.empty((rows, n), dtype=torch.int64, device=dev)
            pay = torch.empty((rows, n), dtype=torch.int64, device=dev)
            srs_amd.fill_synthetic_device(keys.view(-1), pay.view(-1), key_kind=kind)
            pays, indices = (pay,), False
        incols = (keys,) + pays
        outs = tuple(torch.empty((rows, n), dtype=c.dtype, device=dev) for c in incols)
        key_bytes = keys.element_size()
        rec_bytes = sum(c.element_size() for c in incols)
        rec = {"rows": rows, "row_len": n, "cols": cols, "reps": args.reps,
               "copy_TBps": round(copy_rate / 1e12, 3)}
        res = {}

        def call():
            res["r"] = srs_amd.sort_rows_device(*incols, key_kind=kind, out=outs, indices=indices)

        srs_amd.debug_set_sort_rows_route(-1)
        med, lo, hi = median_ms(call)
        rec["auto_ms"], rec["auto_min_ms"], rec["auto_max_ms"] = med, lo, hi
        rec["spread_pct"] = round(100 * (hi - lo) / med, 2)
        info = srs_amd.debug_last_sort_rows()
        rec["auto_route"], rec["readbacks"], rec["prepared"] = ROUTES[info[0]], info[2], info[3]
        rec["floor_ms"] = round(model_bytes(info[0], rows, n, key_bytes, rec_bytes, indices,
                                            info[3]) / copy_rate * 1e3, 4)
        ref = [o.clone() for o in res["r"]]
        for route in ([0] + ([1] if n >= 2 else []) if n <= CAP else [2]):
            srs_amd.debug_set_sort_rows_route(route)
            med, lo, hi = median_ms(call)
            assert all(torch.equal(o, x) for o, x in zip(res["r"], ref)), \
                f"route {route} differs from the auto route"
            name = ROUTES[route]
            rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_max_ms"] = med, lo, hi
            i2 = srs_amd.debug_last_sort_rows()
            rec[name + "_floor_ms"] = round(model_bytes(route, rows, n, key_bytes, rec_bytes,
                                                        indices, i2[3]) / copy_rate * 1e3, 4)
        srs_amd.debug_set_sort_rows_route(-1)

        if not args.no_parent:
            # (1) row-wise top-k with k = row_len
            r = rows if n <= CAP else min(rows, args.loop_rows)
            o2 = tuple(x[:r] for x in outs)

            def do_topk():
                res["t"] = srs_amd.topk_rows_device(*[x[:r] for x in incols], k=n, key_kind=kind,
                                                    out=o2, indices=indices)
            med, lo, hi = median_ms(do_topk)
            assert all(torch.equal(o, x[:r]) for o, x in zip(res["t"], ref)), "top-k rows differs"
            rec["topk_rows_ms"], rec["topk_rows_min_ms"], rec["topk_rows_max_ms"] = med, lo, hi
            if r != rows:  # the loop's time is proportional to the rows
                rec["topk_rows_timed_rows"] = r
                rec["topk_rows_ms_scaled"] = round(med * rows / r, 3)
            # (2) segment sort of a dense copy, with host bounds
            bounds = np.arange(rows + 1, dtype=np.int64) * n
            bptr = bounds.ctypes.data_as(ctypes.c_void_p)
            L = srs_amd.lib()
            iota = torch.arange(n, dtype=torch.int64, device=dev) if indices else None
            st = torch.cuda.current_stream().cuda_stream

            def do_segments():
                cp = [c.clone() for c in incols]
                if indices:
                    cp.append(iota.expand(rows, n).contiguous())
                pp = (ctypes.c_void_p * max(1, len(cp) - 1))(*[c.data_ptr() for c in cp[1:]])
                ps = (ctypes.c_uint32 * max(1, len(cp) - 1))(*[c.element_size() for c in cp[1:]])
                rc = L.srs_sort_segments_device(rows * n, kind, 1, cp[0].data_ptr(), len(cp) - 1,
                                                pp, ps, rows, bptr, 0, st)
                assert rc == 0, L.srs_last_error()
                res["s"] = cp
            med, lo, hi = median_ms(do_segments)
            assert all(torch.equal(o, x) for o, x in zip(res["s"], ref)), "segment sort differs"
            rec["segments_ms"], rec["segments_min_ms"], rec["segments_max_ms"] = med, lo, hi
            res.pop("s")
            best = min(rec.get("topk_rows_ms_scaled", rec["topk_rows_ms"]), rec["segments_ms"])
            rec["parent_best_ms"] = best
            rec["auto_over_parent_best"] = round(rec["auto_ms"] / best, 3)
        if not args.no_torch:
            def do_torch():
                v, i = torch.sort(keys, dim=-1, stable=True)
                for p in pays:
                    torch.gather(p, 1, i)
            try:
                rec["torch_sort_ms"] = median_ms(do_torch)[0]
            except RuntimeError as e:  # (out of memory at the largest shapes)
                rec["torch_sort_error"] = str(e)[:80]
        emit(rec)

    shapes = args.shapes + ("," + SWEEP if args.sweep else "")
    for s in [x for x in shapes.split(",") if x]:
        rows, n = (int(v) for v in s.split("x"))
        for cols in args.cols.split(","):
            measure(rows, n, cols)
            torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
