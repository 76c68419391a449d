#!/usr/bin/env python3
"""Row-wise top-k on one GPU.

For every shape (rows x row_len, k) and both column sets -- f32 keys with
indices, u64 keys + one u64 payload -- the warm topk_rows_device call is timed
on the library's own rule and on every route that can take the shape
(resident, stream, and the row-by-row loop; the loop on at most --loop-rows
rows, scaled up and marked). Yardsticks in the same process: torch.topk on the
same tensor (plus the payload gather), and the read floor rows * row_len *
key bytes over the rate select_tally_kernel reaches on the same keys as one
flat array. Every figure is the median wall time of --reps calls that end in
a stream synchronise.

One JSON line per (shape, columns) on stdout (and in --out). --sweep adds the
grid of few long rows on which the stream / loop rule was set.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simd-radix-sort_amd", "python"))

SHAPES = "1048576x64x8,65536x1024x32,16384x8192x64,4096x32768x64,1024x131072x50," \
         "256x1048576x100,8x100000000x100"
SWEEP = ",".join(f"{r}x{n}x100" for n in (1 << 20, 1 << 22, 1 << 24, 1 << 26)
                 for r in (8, 32, 128, 512) if r * n <= 1 << 31)
ROUTES = {0: "resident", 1: "stream", 2: "loop"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="rows x row_len x k, comma separated")
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--cols", default="f32_idx,u64_u64")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--loop-rows", type=int, default=1024)
    ap.add_argument("--no-torch", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import srs_amd
    if not torch.cuda.is_available():
        sys.exit("topk_rows_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    cap = srs_amd.TOPK_ROWS_MAX_K
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

    def tally_rate(flat, kind):
        """bytes / s of select_tally_kernel over the keys as one array"""
        srs_amd.set_kernel_timing(True)
        best = None
        for _ in range(3):
            srs_amd.reset_kernel_stats()
            srs_amd.topk_device(flat, k=100, key_kind=kind)
            torch.cuda.synchronize()
            launches, ms, _ = srs_amd.kernel_stats("select_tally")
            if launches:
                best = ms / launches if best is None else min(best, ms / launches)
        srs_amd.set_kernel_timing(False)
        srs_amd.reset_kernel_stats()
        return None if not best else flat.numel() * flat.element_size() / (best * 1e-3)

    def measure(rows, n, k, cols):
        if cols == "f32_idx":
            kind, keys = srs_amd.KEY_F32, torch.randn((rows, n), dtype=torch.float32, device=dev)
            pays, indices = (), True
        else:
            kind = srs_amd.KEY_U64
            keys = torch.empty((rows, n), dtype=torch.int64, device=dev)
            pay = torch.empty((rows, n), dtype=torch.int64, device=dev)
            srs_amd.fill_synthetic_device(keys.view(-1), pay.view(-1), key_kind=kind)
            pays, indices = (pay,), False
        kk = min(k, n)
        outs = tuple(torch.empty((rows, kk), dtype=c.dtype, device=dev) for c in (keys,) + pays)
        rec = {"rows": rows, "row_len": n, "k": k, "cols": cols, "reps": args.reps}

        def call(r, *c):
            o = tuple(x[:r] for x in outs)
            return srs_amd.topk_rows_device(*[x[:r] for x in c], k=k, key_kind=kind, out=o,
                                            indices=indices)

        srs_amd.debug_set_topk_rows_route(-1)
        rec["auto_ms"], rec["auto_min_ms"], rec["auto_max_ms"] = median_ms(
            lambda: call(rows, keys, *pays))
        info = srs_amd.debug_last_topk_rows()
        rec["auto_route"], rec["passes"] = ROUTES[info[0]], info[2]
        ref = [o.clone() for o in outs]
        eligible = [0] if n <= 8192 else ([1] if kk <= cap and n < 1 << 31 else [])
        for route in eligible + [2]:
            r = min(rows, args.loop_rows) if route == 2 else rows
            srs_amd.debug_set_topk_rows_route(route)
            med, lo, hi = median_ms(lambda: call(r, keys, *pays))
            same = all(torch.equal(o[:r], x[:r]) for o, x in zip(outs, ref))
            assert same, f"route {route} differs from the auto route"
            name = ROUTES[route]
            rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_max_ms"] = med, lo, hi
            if r != rows:  # timed on r rows: the loop's time is proportional to the rows
                rec["loop_rows_timed"] = r
                rec["loop_ms_scaled"] = round(med * rows / r, 3)
        srs_amd.debug_set_topk_rows_route(-1)
        if not args.no_torch:
            def do_torch():
                v, i = torch.topk(keys, kk, dim=1, largest=False, sorted=True)
                for p in pays:
                    torch.gather(p, 1, i)
            try:
                rec["torch_topk_ms"] = median_ms(do_torch)[0]
            except RuntimeError as e:  # (out of memory at the largest shapes)
                rec["torch_topk_error"] = str(e)[:80]
        rate = tally_rate(keys.view(-1), kind) if rows * n > 8192 else None
        if rate:
            rec["tally_TBps"] = round(rate / 1e12, 3)
            rec["read_floor_ms"] = round(rows * n * keys.element_size() / rate * 1e3, 4)
        emit(rec)

    shapes = args.shapes + ("," + SWEEP if args.sweep else "")
    for s in [x for x in shapes.split(",") if x]:
        rows, n, k = (int(v) for v in s.split("x"))
        for cols in args.cols.split(","):
            measure(rows, n, k, cols)
            torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
