#!/usr/bin/env python3
"""Ragged top-k on one GPU.

For every seeded shape of tools/sort_ragged_bench.py (about 2^26 records
each), its k, and both column sets -- f32 keys with indices, u64 keys + one
u64 payload -- the warm topk_ragged_device call is timed. Beside it,
interleaved call by call in the same process, what a caller had before this
entry point:

  (a) sort_ragged_device over everything, then a torch gather of every
      segment's first min(k, len) records into the (segments, k) outputs,
      timed with the gather's index arithmetic (the offsets live on the
      device);
  (b) for uniform shapes, topk_rows_device on the same data.

The floor is the key bytes read once plus min(k, len) records written per
segment, over the rate a device copy of 1 GiB reaches. 1048576x64 also times
an all-empty call of as many segments: the classify pass, the two kernels
that find nothing to do, and the one read-back on their own.

Every figure is the median wall time of --reps calls that end in a stream
synchronise; min and max are kept, and spread_pct is (max - min) / median of
the yardstick line. One JSON line per (shape, columns) on stdout (and in
--out). --route forces a route (0 kernels, 1 sort) for the top-k line.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simd-radix-sort_amd", "python"))
sys.path.insert(0, os.path.join(REPO, "tools"))

from sort_ragged_bench import TOTAL, is_uniform, lengths_of  # noqa: E402  (the shapes are §14's)

SHAPES = "1048576x64:8,power32:32,random512:16,near8192:64,4096x32768:64"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="comma separated shape:k")
    ap.add_argument("--total", type=int, default=TOTAL)
    ap.add_argument("--cols", default="f32_idx,u64_u64")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--route", type=int, default=-1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import srs_amd
    if not torch.cuda.is_available():
        sys.exit("topk_ragged_bench: no GPU (nothing is measured without one)")
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

    def interleaved(fns):
        """{name: (median, min, max)} of --reps rounds, one call of each per round"""
        for _ in range(args.warmup):
            for f in fns.values():
                f()
        t = {k: [] for k in fns}
        for _ in range(args.reps):
            for k, f in fns.items():
                t[k].append(timed(f))
        return {k: (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4))
                for k, v in t.items()}

    def put(rec, name, m):
        rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_max_ms"] = m

    # the copy rate (read + written bytes per second) of 1 GiB
    a = torch.empty(1 << 27, dtype=torch.int64, device=dev)
    b = torch.empty_like(a)
    copy_ms = interleaved({"c": lambda: b.copy_(a)})["c"][0]
    copy_rate = 2 * a.numel() * 8 / (copy_ms * 1e-3)
    del a, b
    torch.cuda.empty_cache()

    def measure(shape, k, cols):
        ln = lengths_of(shape, np, args.total)
        nseg, N, max_len = len(ln), int(ln.sum()), int(ln.max())
        offs_h = np.concatenate([[0], np.cumsum(ln)]).astype(np.int64)
        offs = torch.from_numpy(offs_h).to(dev)
        if cols == "f32_idx":
            kind, keys = srs_amd.KEY_F32, torch.randn(N, dtype=torch.float32, device=dev)
            pays, indices = (), True
        else:
            kind = srs_amd.KEY_U64
            keys = torch.empty(N, dtype=torch.int64, device=dev)
            pay = torch.empty(N, dtype=torch.int64, device=dev)
            srs_amd.fill_synthetic_device(keys, pay, key_kind=kind)
            pays, indices = (pay,), False
        incols = (keys,) + pays
        outs = tuple(torch.zeros((nseg, k), dtype=c.dtype, device=dev) for c in incols)
        key_bytes = keys.element_size()
        out_bytes = sum(c.element_size() for c in incols) + (8 if indices else 0)
        heads = int(np.minimum(ln, k).sum())
        rec = {"shape": shape, "k": k, "segments": nseg, "records": N, "max_len": max_len,
               "cols": cols, "reps": args.reps, "copy_TBps": round(copy_rate / 1e12, 3),
               "heads": heads}
        res = {}
        srs_amd.debug_set_topk_ragged_route(args.route)

        def topk():
            res["t"] = srs_amd.topk_ragged_device(*incols, offsets=offs, k=k, key_kind=kind,
                                                  out=outs, indices=indices)

        # (a) the ragged sort of everything, then the heads gathered
        souts = tuple(torch.empty_like(c) for c in incols)
        gouts = tuple(torch.zeros((nseg, k), dtype=c.dtype, device=dev) for c in incols)
        gidx = torch.full((nseg, k), -1, dtype=torch.int64, device=dev) if indices else None

        def sort_gather():
            r = srs_amd.sort_ragged_device(*incols, offsets=offs, key_kind=kind, out=souts,
                                           indices=indices)
            lens = offs[1:] - offs[:-1]
            j = torch.arange(k, device=dev)
            mask = j[None, :] < lens[:, None]
            src = (offs[:-1, None] + j[None, :])[mask]
            for o, x in zip(gouts + ((gidx,) if indices else ()), r):
                o[mask] = x[src]
            res["a"] = gouts + ((gidx,) if indices else ())
            res["mask"] = mask

        fns = {"topk": topk, "sort_gather": sort_gather}
        if is_uniform(shape):
            mats = [c.view(nseg, max_len) for c in incols]
            routs = tuple(torch.empty((nseg, min(k, max_len)), dtype=c.dtype, device=dev)
                          for c in incols)

            def rows():
                res["rows"] = srs_amd.topk_rows_device(*mats, k=k, key_kind=kind, out=routs,
                                                       indices=indices)
            fns["topk_rows"] = rows
        if shape.startswith("1048576x"):
            zero = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
            fns["all_empty"] = lambda: srs_amd.topk_ragged_device(
                *incols, offsets=zero, k=k, key_kind=kind, out=outs, indices=indices)

        m = interleaved(fns)
        topk()
        info = srs_amd.debug_last_topk_ragged()
        put(rec, "topk", m["topk"])
        rec["route"], rec["short_segments"], rec["long_segments"], rec["max_passes"] = info[:4]
        rec["readbacks"], rec["launches"] = info[4], info[5]
        rec["floor_ms"] = round((N * key_bytes + heads * out_bytes) / copy_rate * 1e3, 4)
        for name in ("sort_gather", "topk_rows", "all_empty"):
            if name in m:
                put(rec, name, m[name])
        mask = res["mask"]
        got = res["t"][:-1]
        rec["sort_gather_equal"] = bool(all(torch.equal(g[mask], x[mask])
                                            for g, x in zip(got, res["a"])))
        rec["counts_equal"] = bool(torch.equal(res["t"][-1], mask.sum(1)))
        if "rows" in res:
            kk = min(k, max_len)
            rec["topk_rows_equal"] = bool(all(torch.equal(g[:, :kk], x)
                                              for g, x in zip(got, res["rows"])))
            rec["topk_over_topk_rows"] = round(m["topk"][0] / m["topk_rows"][0], 3)
            med, lo, hi = m["topk_rows"]
            rec["topk_rows_spread_pct"] = round(100 * (hi - lo) / med, 2)
        med, lo, hi = m["sort_gather"]
        rec["spread_pct"] = round(100 * (hi - lo) / med, 2)
        rec["topk_over_sort_gather"] = round(m["topk"][0] / med, 3)
        srs_amd.debug_set_topk_ragged_route(-1)
        emit(rec)

    for item in [x for x in args.shapes.split(",") if x]:
        shape, k = item.split(":")
        for cols in args.cols.split(","):
            measure(shape, int(k), cols)
            torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
