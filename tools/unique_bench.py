#!/usr/bin/env python3
"""unique on one GPU.

Inputs, at every size of --sizes (the bench's C1 size and 2^26 by default):
u64 keys uniform (U ~ n), gaussian as bench.py --dist gaussian (round(N(0,
100)): a few thousand groups), zero (U = 1), and 32-bit segment ids with a
mean run of 29 (n / 29 ids drawn uniformly). For each input the warm
unique_device call is timed with the offsets only and with the inverse.
Beside it, interleaved call by call in the same process, "before": the
fastest thing a caller had, sort_device out of place (with an arange payload
when an inverse is wanted) followed by torch.unique_consecutive with the
matching return_* flags, plus the scatter of the inverse through the sorted
arange. torch.unique with the same flags is a yardstick only (--yardstick-reps
calls, not interleaved).

The floor is a byte model over the rate a device copy of 1 GiB reaches in the
same process: the sort at 7 x its record bytes (what the full sort moves per
record at 1e9; the record is the key, plus 8 bytes of index
column with the inverse), two reads of the key column, and 8 n read + 8 n
written for the inverse.

Every figure is the median wall time of --reps calls that end in a stream
synchronise; min and max are kept, and spread_pct is (max - min) / median of
the "before" line. One JSON line per (size, input, outputs) on stdout (and in
--out). A last line per size compares the read rates of run_tally_kernel and
select_tally_kernel (HIP events around the launches, --tally-rounds rounds of
5 calls each on the uniform input).
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simd-radix-sort_amd", "python"))

SIZES = "1000000000,67108864"
INPUTS = "uniform,gaussian,zero,segids"
SORT_BYTES_PER_RECORD_BYTE = 7


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--inputs", default=INPUTS)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-reps", type=int, default=3)
    ap.add_argument("--tally-rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import srs_amd
    if not torch.cuda.is_available():
        sys.exit("unique_bench: no GPU (nothing is measured without one)")
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

    def stats(v):
        return (round(statistics.median(v), 4), round(min(v), 4), round(max(v), 4))

    def interleaved(fns, reps):
        """{name: (median, min, max)} of `reps` rounds, one call of each per round"""
        for _ in range(args.warmup):
            for f in fns.values():
                f()
        t = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                t[k].append(timed(f))
        return {k: stats(v) for k, v in t.items()}

    def put(rec, name, m):
        rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_max_ms"] = m

    # the copy rate (read + written bytes per second) of 1 GiB
    a = torch.empty(1 << 27, dtype=torch.int64, device=dev)
    b = torch.empty_like(a)
    copy_ms = interleaved({"c": lambda: b.copy_(a)}, args.reps)["c"][0]
    copy_rate = 2 * a.numel() * 8 / (copy_ms * 1e-3)
    del a, b
    torch.cuda.empty_cache()

    def make_keys(n, name):
        g = torch.Generator(device=dev)
        g.manual_seed(42)
        if name == "segids":
            keys = torch.randint(0, max(1, n // 29), (n,), device=dev, generator=g,
                                 dtype=torch.int32)
            return keys, srs_amd.KEY_U32
        keys = torch.empty(n, dtype=torch.int64, device=dev)
        if name == "uniform":
            srs_amd.fill_synthetic_device(keys, key_kind=srs_amd.KEY_U64)
        elif name == "gaussian":
            for i in range(0, n, 1 << 26):  # (chunks: randn's f32 temporaries stay small)
                k = keys[i:i + (1 << 26)]
                k.copy_(torch.round(torch.randn(k.numel(), device=dev, generator=g) * 100)
                        .to(torch.int64))
        elif name == "zero":
            keys.zero_()
        else:
            sys.exit(f"unique_bench: unknown input {name}")
        return keys, srs_amd.KEY_U64

    def measure(n, name, inverse):
        keys, kind = make_keys(n, name)
        ks = keys.element_size()
        rec = {"n": n, "input": name, "outputs": "offsets+inverse" if inverse else "offsets",
               "key_bytes": ks, "reps": args.reps, "copy_TBps": round(copy_rate / 1e12, 3)}
        res = {}
        sorted_keys = torch.empty_like(keys)
        iota = torch.arange(n, dtype=torch.int64, device=dev) if inverse else None
        perm = torch.empty_like(iota) if inverse else None

        def unique():
            res["u"] = srs_amd.unique_device(keys, key_kind=kind, return_offsets=True,
                                             return_inverse=inverse)

        def before():
            if inverse:
                srs_amd.sort_device(keys, iota, key_kind=kind, out=(sorted_keys, perm),
                                    cmp_sort_threshold=0)
                u, inv_s, cnt = torch.unique_consecutive(sorted_keys, return_inverse=True,
                                                         return_counts=True)
                inv = torch.empty_like(inv_s)
                inv[perm] = inv_s
                res["b"] = (u, cnt, inv)
            else:
                srs_amd.sort_device(keys, key_kind=kind, out=(sorted_keys,), cmp_sort_threshold=0)
                u, cnt = torch.unique_consecutive(sorted_keys, return_counts=True)
                res["b"] = (u, cnt, None)

        try:
            m = interleaved({"unique": unique, "before": before}, args.reps)
        except RuntimeError as e:  # (torch out of memory: the line says so, nothing is timed)
            rec["error"] = str(e).splitlines()[0][:160]
            emit(rec)
            return
        put(rec, "unique", m["unique"])
        put(rec, "before", m["before"])
        med, lo, hi = m["before"]
        rec["spread_pct"] = round(100 * (hi - lo) / med, 2)
        rec["unique_over_before"] = round(m["unique"][0] / med, 3)
        info = srs_amd.debug_last_unique()
        rec["launches"], rec["readbacks"], rec["index_column"], rec["workspace_columns"] = info
        r, (u, cnt, inv) = res["u"], res["b"]
        rec["num_unique"] = int(r.unique.numel())
        # (unique_consecutive keeps the sorted column's order, so the results are comparable
        # element by element whatever torch makes of u64 keys in int64 storage)
        rec["equal_unique"] = bool(torch.equal(r.unique, u))
        rec["equal_counts"] = bool(torch.equal(r.offsets[1:] - r.offsets[:-1], cnt))
        if inverse:
            rec["equal_inverse"] = bool(torch.equal(r.inverse, inv))
        rec_bytes = ks + (8 if inverse else 0)
        model = n * (SORT_BYTES_PER_RECORD_BYTE * rec_bytes + 2 * ks + (16 if inverse else 0))
        rec["model_bytes"] = model
        rec["floor_ms"] = round(model / copy_rate * 1e3, 4)
        res.clear()
        del u, cnt, inv, r
        torch.cuda.empty_cache()

        if args.yardstick_reps > 0:
            def torch_unique():
                res["y"] = torch.unique(keys, return_counts=True, return_inverse=inverse)
            try:
                y = interleaved({"y": torch_unique}, args.yardstick_reps)["y"]
                put(rec, "torch_unique", y)
            except RuntimeError as e:  # (out of memory at the large size: no yardstick)
                rec["torch_unique_error"] = str(e).splitlines()[0][:120]
            res.clear()
            torch.cuda.empty_cache()
        emit(rec)

    def tally_rates(n):
        """run_tally_kernel against select_tally_kernel: both read the u64 key
        column once, 16 bytes per lane"""
        keys, kind = make_keys(n, "uniform")
        out = (torch.empty(1000, dtype=torch.int64, device=dev),)
        calls = {"run_tally": lambda: srs_amd.unique_device(keys, key_kind=kind),
                 "select_tally": lambda: srs_amd.topk_device(keys, k=1000, key_kind=kind, out=out)}
        for f in calls.values():
            f()
        rates = {k: [] for k in calls}
        srs_amd.set_kernel_timing(True)
        for _ in range(args.tally_rounds):
            for name, f in calls.items():
                srs_amd.reset_kernel_stats()
                for _ in range(5):
                    f()
                torch.cuda.synchronize()
                launches, ms, elems = srs_amd.kernel_stats(name)
                if launches and ms > 0:
                    rates[name].append(elems * 8 / (ms * 1e-3) / 1e12)
        srs_amd.set_kernel_timing(False)
        rec = {"n": n, "tally": True}
        for name, v in rates.items():
            if v:
                med, lo, hi = stats(v)
                rec[name + "_TBps"], rec[name + "_min_TBps"], rec[name + "_max_TBps"] = med, lo, hi
                rec[name + "_spread_pct"] = round(100 * (hi - lo) / med, 2)
        if rates["run_tally"] and rates["select_tally"]:
            rec["run_over_select"] = round(rec["run_tally_TBps"] / rec["select_tally_TBps"], 3)
        emit(rec)

    for n in [int(x) for x in args.sizes.split(",") if x]:
        for name in [x for x in args.inputs.split(",") if x]:
            for inverse in (False, True):
                measure(n, name, inverse)
                torch.cuda.empty_cache()
        tally_rates(n)
        torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
