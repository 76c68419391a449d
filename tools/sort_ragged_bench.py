#!/usr/bin/env python3
"""Ragged sort on one GPU.

For every seeded shape (about 2^26 records each) and both column sets -- f32
keys with indices, u64 keys + one u64 payload -- the warm sort_ragged_device
call is timed. Beside it, interleaved call by call in the same process, what a
caller had before this entry point:

  (a) sort_segments_device on a dense copy, timed with the offsets' copy to
      the host, the copy of the columns, and (where indices are asked for)
      the in-segment iota column built on the device;
  (b) padding every segment to the longest one and sort_rows_device, timed
      with the scatter into the padded matrix and the gather back; skipped
      where the padded matrix would not fit (--pad-max-gib);

and, for uniform shapes, sort_rows_device on the same data. The floor is the
bytes of the routes' byte model over the rate a device copy of 1 GiB reaches.
Shapes are rows x row_len (uniform) or a named length law. 1048576x64 also
times an all-empty call of as many segments: the classify pass and its one
read-back on their own.

Every figure is the median wall time of --reps calls that end in a stream
synchronise; min and max are kept, and spread_pct is (max - min) / median of
the yardstick line (the faster of (a) and (b)). One JSON line per (shape,
columns) on stdout (and in --out). --short-max runs the shapes at the given
maxima of the wave-per-segment kernel instead (no yardsticks).
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

SHAPES = "1048576x64,power32,random512,near8192,4096x32768"
TOTAL = 1 << 26
SMALL_CAP, CAP = 4096, 8192


def is_uniform(shape):
    return "x" in shape


def lengths_of(shape, np, total):
    """Seeded segment lengths of the named shape, their sum about `total`."""
    rng = np.random.default_rng(sum(shape.encode()))
    if is_uniform(shape):  # rows x row_len, as given
        rows, n = (int(v) for v in shape.split("x"))
        return np.full(rows, n, dtype=np.int64)
    if shape == "power32":  # the graph case: mean 32, a few segments over 8192
        ln = np.minimum((rng.pareto(1.25, total // 24) * 8).astype(np.int64), 200000)
    elif shape == "random512":  # lengths uniform in 1 .. 512
        ln = rng.integers(1, 513, total // 200)
    elif shape == "near8192":
        ln = rng.integers(8192 - 2000, 8192 + 2001, total // 7000)
    else:
        raise SystemExit(f"unknown shape {shape}")
    ln = ln[:int(np.searchsorted(np.cumsum(ln), total, side="right"))]
    return ln.astype(np.int64)


def model_bytes(ln, np, key_bytes, rec_bytes, idx, short_max):
    """Bytes the call moves through HBM."""
    out = rec_bytes + (8 if idx else 0)
    short = int(ln[ln <= short_max].sum())
    local = int(ln[(ln > short_max) & (ln <= CAP)].sum())
    big = ln[ln > CAP]
    total = 16 * len(ln) * (2 if short else 1) + short * (rec_bytes + out)
    prep = (rec_bytes + out) if idx else 0
    total += local * (prep + (2 * out if idx else rec_bytes + out))
    for n in big.tolist():
        levels = max(1, math.ceil(math.log2(n / 7808) / 9))
        total += n * (prep + levels * (key_bytes + 2 * out) + 2 * out)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--total", type=int, default=TOTAL)
    ap.add_argument("--cols", default="f32_idx,u64_u64")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--pad-max-gib", type=float, default=16.0)
    ap.add_argument("--short-max", default=None, help="comma separated maxima: the sweep")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import numpy as np
    import torch
    import srs_amd
    if not torch.cuda.is_available():
        sys.exit("sort_ragged_bench: no GPU (nothing is measured without one)")
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

    def measure(shape, cols, short_max):
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
        outs = tuple(torch.empty_like(c) for c in incols)
        key_bytes = keys.element_size()
        rec_bytes = sum(c.element_size() for c in incols)
        rec = {"shape": shape, "segments": nseg, "records": N, "max_len": max_len, "cols": cols,
               "reps": args.reps, "copy_TBps": round(copy_rate / 1e12, 3),
               "short_max": 256 if short_max < 0 else short_max}
        res = {}
        srs_amd.debug_set_sort_ragged_short_max(short_max)

        def ragged():
            res["r"] = srs_amd.sort_ragged_device(*incols, offsets=offs, key_kind=kind, out=outs,
                                                  indices=indices)

        fns = {"ragged": ragged}
        if args.short_max is None:
            # (a) the segment sort of a dense copy, with host bounds
            L = srs_amd.lib()
            st = torch.cuda.current_stream().cuda_stream

            def segments():
                bounds = offs.cpu().numpy()  # the caller's offsets live on the device
                cp = [c.clone() for c in incols]
                if indices:
                    lens = offs[1:] - offs[:-1]
                    cp.append(torch.arange(N, dtype=torch.int64, device=dev) -
                              torch.repeat_interleave(offs[:-1], lens, output_size=N))
                pp = (ctypes.c_void_p * max(1, len(cp) - 1))(*[c.data_ptr() for c in cp[1:]])
                ps = (ctypes.c_uint32 * max(1, len(cp) - 1))(*[c.element_size() for c in cp[1:]])
                rc = L.srs_sort_segments_device(N, kind, 1, cp[0].data_ptr(), len(cp) - 1, pp, ps,
                                                nseg, bounds.ctypes.data_as(ctypes.c_void_p), 0, st)
                assert rc == 0, L.srs_last_error()
                res["a"] = cp
            fns["segments"] = segments

            # (b) every segment padded to the longest, then the row-wise sort
            padded_gib = nseg * max_len * (rec_bytes + (8 if indices else 0)) * 2 / 2 ** 30
            rec["padded_GiB"] = round(padded_gib, 2)
            if padded_gib <= args.pad_max_gib:
                pad_key = float("inf") if kind == srs_amd.KEY_F32 else -1  # (u64: all ones)

                def padded():
                    lens = offs[1:] - offs[:-1]
                    seg = torch.repeat_interleave(torch.arange(nseg, device=dev), lens,
                                                  output_size=N)
                    cell = seg * max_len + (torch.arange(N, device=dev) - offs[:-1][seg])
                    mats = []
                    for i, c in enumerate(incols):
                        m = torch.full((nseg * max_len,), pad_key if i == 0 else 0, dtype=c.dtype,
                                       device=dev)
                        m[cell] = c
                        mats.append(m.view(nseg, max_len))
                    r = srs_amd.sort_rows_device(*mats, key_kind=kind, indices=indices)
                    res["b"] = [x.view(-1)[cell] for x in r]
                fns["padded"] = padded
            if is_uniform(shape):
                mats = [c.view(nseg, max_len) for c in incols]
                mouts = tuple(torch.empty_like(m) for m in mats)

                def rows():
                    res["rows"] = srs_amd.sort_rows_device(*mats, key_kind=kind, out=mouts,
                                                           indices=indices)
                fns["sort_rows"] = rows
            if shape == "1048576x64":
                zero = torch.zeros(nseg + 1, dtype=torch.int64, device=dev)
                fns["all_empty"] = lambda: srs_amd.sort_ragged_device(
                    *incols, offsets=zero, key_kind=kind, out=outs, indices=indices)

        m = interleaved(fns)
        ragged()
        info = srs_amd.debug_last_sort_ragged()
        put(rec, "ragged", m["ragged"])
        rec["short_segments"], rec["n_local"], rec["n_local2"], rec["n_big"] = info[:4]
        rec["readbacks"], rec["prepared"] = info[4], info[5]
        rec["floor_ms"] = round(model_bytes(ln, np, key_bytes, rec_bytes, indices,
                                            rec["short_max"]) / copy_rate * 1e3, 4)
        for name in ("segments", "padded", "sort_rows", "all_empty"):
            if name in m:
                put(rec, name, m[name])
        for name, key in (("segments", "a"), ("padded", "b"), ("sort_rows", "rows")):
            if key in res:
                same = all(torch.equal(o.view(-1), x.view(-1)) for o, x in zip(res["r"], res[key]))
                rec[name + "_equal"] = bool(same)
        yard = [n for n in ("segments", "padded") if n in m]
        if yard:
            best = min(yard, key=lambda n: m[n][0])
            med, lo, hi = m[best]
            rec["yardstick"], rec["yardstick_ms"] = best, med
            rec["spread_pct"] = round(100 * (hi - lo) / med, 2)
            rec["ragged_over_yardstick"] = round(m["ragged"][0] / med, 3)
        if "sort_rows" in m:
            rec["ragged_over_sort_rows"] = round(m["ragged"][0] / m["sort_rows"][0], 3)
        srs_amd.debug_set_sort_ragged_short_max(-1)
        emit(rec)

    maxima = [-1] if args.short_max is None else [int(x) for x in args.short_max.split(",")]
    for shape in [x for x in args.shapes.split(",") if x]:
        for cols in args.cols.split(","):
            for sm in maxima:
                measure(shape, cols, sm)
                torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
