#!/usr/bin/env python3
"""Top-k against the full sort on one GPU.

Workload: n u64 keys + one u64 payload column (bench.py's c1 shape), resident
in HBM; distributions uniform (srs_fill_synthetic_device), gaussian
(round(N(0, 100)) as bench.py --dist gaussian: int64 bit patterns under the
u64 order) and zero. For every k the warm top-k call and the out-of-place
sort_device of the same input alternate in one process; the figure is the
median wall time of a call that ends in a stream synchronise. A second run
with kernel timing on gives the per-kernel device times. --crossover times
both routes (SRS_TOPK_FULL_PCT = 100 / 0) at large k.

One JSON line per (dist, k) on stdout (and in --out).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simd-radix-sort_amd", "python"))

KERNELS = ("select_hist", "select_tally", "select_gather", "scan", "count", "scatter", "local")


def model_bytes(n, k, passes, nsorted, full):
    """Bytes by the model of DESIGN.md §11 (8-byte keys, 16-byte records):
    every select pass, the tally and the gather read the key column (an
    upper bound for the gather, which skips tiles without a selected
    record); the gather moves the selected records; the
    finishing sort costs 112 bytes per record as the full sort does at 1e9;
    the head copy reads and writes k records."""
    if full:
        return 112 * n + 32 * k
    return 8 * n * (passes + 2) + 32 * nsorted + 112 * nsorted + 32 * k


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=float, default=1e9)
    ap.add_argument("--ks", default="1,1e3,1e6,1e8")
    ap.add_argument("--dists", default="uniform,gaussian,zero")
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--crossover", default="", help="fractions of n, e.g. 0.25,0.5,0.75")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import srs_amd
    if not torch.cuda.is_available():
        sys.exit("topk_bench: no GPU (nothing is measured without one)")
    n = int(args.n)
    dev = torch.device("cuda:0")
    kind = srs_amd.KEY_U64
    keys = torch.empty(n, dtype=torch.int64, device=dev)
    pays = torch.empty(n, dtype=torch.int64, device=dev)
    so = (torch.empty_like(keys), torch.empty_like(pays))
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

    def do_sort():
        srs_amd.sort_device(keys, pays, key_kind=kind, out=so)

    def kernel_ms(fn):
        srs_amd.set_kernel_timing(True)
        srs_amd.reset_kernel_stats()
        fn()
        torch.cuda.synchronize()
        res = {}
        for name in KERNELS:
            launches, ms, _ = srs_amd.kernel_stats(name)
            if launches:
                res[name] = [launches, round(ms, 4)]
        srs_amd.set_kernel_timing(False)
        srs_amd.reset_kernel_stats()
        return res

    def measure(dist, k, tag="", env_pct=None):
        if env_pct is not None:
            os.environ["SRS_TOPK_FULL_PCT"] = str(env_pct)
        else:
            os.environ.pop("SRS_TOPK_FULL_PCT", None)
        ko = torch.empty(min(k, n), dtype=torch.int64, device=dev)
        po = torch.empty(min(k, n), dtype=torch.int64, device=dev)

        def do_topk():
            srs_amd.topk_device(keys, pays, k=k, key_kind=kind, out=(ko, po))

        for _ in range(args.warmup):
            do_topk()
            do_sort()
        t_top, t_sort = [], []
        for _ in range(args.reps):  # interleaved: both see the same machine state
            t_top.append(timed(do_topk))
            t_sort.append(timed(do_sort))
        do_topk()
        passes, nsorted, full = srs_amd.debug_last_topk()
        # the head of the sort is the top-k (same process, same input)
        assert torch.equal(ko, so[0][:k]) and torch.equal(po, so[1][:k]), "top-k != head of sort"
        kt = kernel_ms(do_topk)
        mt, ms = statistics.median(t_top), statistics.median(t_sort)
        emit({"dist": dist, "n": n, "k": k, "tag": tag, "topk_ms": round(mt, 4),
              "topk_min_ms": round(min(t_top), 4), "topk_max_ms": round(max(t_top), 4),
              "sort_ms": round(ms, 4), "sort_min_ms": round(min(t_sort), 4),
              "sort_max_ms": round(max(t_sort), 4), "sort_over_topk": round(ms / mt, 3),
              "passes": passes, "records_sorted": nsorted, "full_route": full,
              "model_GB": round(model_bytes(n, k, passes, nsorted, full) / 1e9, 3),
              "sort_model_GB": round(112 * n / 1e9, 3), "reps": args.reps, "kernels_ms": kt})
        os.environ.pop("SRS_TOPK_FULL_PCT", None)

    for dist in args.dists.split(","):
        if dist == "uniform":
            srs_amd.fill_synthetic_device(keys, pays, key_kind=kind)
        elif dist == "gaussian":
            g = torch.Generator(device=dev)
            g.manual_seed(42)
            for i in range(0, n, 1 << 27):
                m = min(1 << 27, n - i)
                keys[i:i + m].copy_(torch.round(torch.randn(m, device=dev, generator=g) * 100)
                                    .to(torch.int64))
            torch.arange(n, out=pays)
        elif dist == "zero":
            keys.zero_()
            torch.arange(n, out=pays)
        else:
            sys.exit(f"unknown dist {dist}")
        torch.cuda.synchronize()
        for ks in args.ks.split(","):
            k = int(float(ks))
            if 1 <= k <= n:
                measure(dist, k)
        if dist == "uniform":
            emit({"dist": dist, "n": n, "sort_kernels_ms": kernel_ms(do_sort)})
            for fs in [f for f in args.crossover.split(",") if f]:
                k = max(1, int(float(fs) * n))
                measure(dist, k, tag="select", env_pct=100)
                measure(dist, k, tag="full", env_pct=0)
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
