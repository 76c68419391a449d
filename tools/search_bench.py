#!/usr/bin/env python3
"""search-sorted on one GPU.

Grid: a sorted table of --tables keys against --queries queries, for i64 and
f32 keys, side="both". The keys are uniform random over the key range (i64:
all of it; f32: [-1e6, 1e6)), the queries are drawn from the same law, once
as drawn ("random") and once pre-sorted and passed with the hint ("sorted").
For each grid point the warm searchsorted_device call is timed on route 0
(the kernel on the caller's queries), on route 1 (the queries sorted first)
and on the library's own rule, each forced through
srs_debug_set_search_route and interleaved call by call in one process.
torch.searchsorted on the same tensors (twice, for the two sides) is a
yardstick only (--yardstick-reps calls, not interleaved); it is the reason for
i64 and not u64 keys.

The floor is a byte model over the rate a device copy of 1 GiB reaches in the
same process: the query bytes read, 8 bytes per output per query written, and
the lesser of the table's bytes and one 128-byte line per query.

Every figure is the median wall time of --reps calls that end in a stream
synchronise; min and max are kept, and spread_pct is (max - min) / median of
the faster forced route. A point whose one round of the three lines takes
more than --slow-round-ms is timed with --slow-reps calls instead (the line
says so in "reps"); no new point is started after --max-seconds. One JSON
line per (table, queries, kind, law) on stdout (and in --out). The tool reads
nothing outside the repository.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simd-radix-sort_amd", "python"))

TABLES = "65536,4194304,67108864,1000000000"
QUERIES = "65536,4194304,67108864,1073741824"
KINDS = "i64,f32"
LAWS = "random,sorted"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tables", default=TABLES)
    ap.add_argument("--queries", default=QUERIES)
    ap.add_argument("--kinds", default=KINDS)
    ap.add_argument("--laws", default=LAWS)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-reps", type=int, default=3)
    ap.add_argument("--slow-round-ms", type=float, default=float("inf"))
    ap.add_argument("--slow-reps", type=int, default=5)
    ap.add_argument("--max-seconds", type=float, default=float("inf"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import srs_amd
    if not torch.cuda.is_available():
        sys.exit("search_bench: no GPU (nothing is measured without one)")
    dev = torch.device("cuda:0")
    t_start = time.perf_counter()
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

    def interleaved(fns, reps, warmup, slow_reps=None):
        """({name: (median, min, max)}, reps used) of `reps` rounds, one call
        of each per round"""
        for i in range(warmup):
            first = sum(timed(f) for f in fns.values())
            if slow_reps is not None and first > args.slow_round_ms:
                reps = min(reps, slow_reps)  # (and one warm-up round)
                break
        t = {k: [] for k in fns}
        for _ in range(reps):
            for k, f in fns.items():
                t[k].append(timed(f))
        return {k: stats(v) for k, v in t.items()}, reps

    def put(rec, name, m):
        rec[name + "_ms"], rec[name + "_min_ms"], rec[name + "_max_ms"] = m

    # the copy rate (read + written bytes per second) of 1 GiB
    a = torch.empty(1 << 27, dtype=torch.int64, device=dev)
    b = torch.empty_like(a)
    copy_ms = interleaved({"c": lambda: b.copy_(a)}, args.reps, args.warmup)[0]["c"][0]
    copy_rate = 2 * a.numel() * 8 / (copy_ms * 1e-3)
    del a, b
    torch.cuda.empty_cache()

    def draw(n, kind, seed):
        if kind == "i64":  # (64 random bits per key)
            x = torch.empty(n, dtype=torch.int64, device=dev)
            srs_amd.fill_synthetic_device(x, key_kind=srs_amd.KEY_U64, seed=seed << 32)
            return x
        if kind == "f32":
            g = torch.Generator(device=dev)
            g.manual_seed(seed)
            x = torch.empty(n, dtype=torch.float32, device=dev)
            x.uniform_(-1e6, 1e6, generator=g)
            return x
        sys.exit(f"search_bench: unknown kind {kind}")

    def sort_keys(x):
        out = torch.empty_like(x)
        srs_amd.sort_device(x, out=(out,), cmp_sort_threshold=0)
        torch.cuda.synchronize()
        return out

    def measure(table, kind, nq, law):
        num, ks = table.numel(), table.element_size()
        rec = {"num": num, "num_queries": nq, "kind": kind, "queries": law, "key_bytes": ks,
               "copy_TBps": round(copy_rate / 1e12, 3)}
        try:
            q = draw(nq, kind, 7)
            if law == "sorted":
                q = sort_keys(q)
            hint = law == "sorted"
            lower = torch.empty(nq, dtype=torch.int64, device=dev)
            upper = torch.empty_like(lower)
            taken = {}

            def call(route, name):
                def f():
                    srs_amd.debug_set_search_route(route)
                    srs_amd.searchsorted_device(table, q, side="both", queries_sorted=hint,
                                                out=(lower, upper))
                    taken[name] = srs_amd.debug_last_search()[0]
                return f

            m, reps = interleaved({"route0": call(0, "route0"), "route1": call(1, "route1"),
                                   "auto": call(-1, "auto")}, args.reps, args.warmup,
                                  args.slow_reps)
        except RuntimeError as e:  # (torch out of memory: the line says so, nothing is timed)
            srs_amd.debug_set_search_route(-1)
            rec["error"] = str(e).splitlines()[0][:160]
            emit(rec)
            return
        srs_amd.debug_set_search_route(-1)
        rec["reps"] = reps
        for name in ("route0", "route1", "auto"):
            put(rec, name, m[name])
        rec["auto_route"] = taken["auto"]
        best = min(("route0", "route1"), key=lambda k: m[k][0])
        med, lo, hi = m[best]
        rec["faster_route"] = int(best[-1])
        rec["spread_pct"] = round(100 * (hi - lo) / med, 2)
        rec["auto_over_faster"] = round(m["auto"][0] / med, 3)
        rec["route1_over_route0"] = round(m["route1"][0] / m["route0"][0], 3)
        model = nq * ks + 16 * nq + min(num * ks, 128 * nq)
        rec["model_bytes"] = model
        rec["floor_ms"] = round(model / copy_rate * 1e3, 4)
        if args.yardstick_reps > 0:
            res = {}

            def torch_search():
                res["lo"] = torch.searchsorted(table, q)
                res["hi"] = torch.searchsorted(table, q, right=True)
            try:
                y, _ = interleaved({"y": torch_search}, args.yardstick_reps, 1)
                put(rec, "torch_searchsorted", y["y"])
                rec["auto_over_torch"] = round(m["auto"][0] / y["y"][0], 3)
                rec["equal_lower"] = bool(torch.equal(res["lo"], lower))
                rec["equal_upper"] = bool(torch.equal(res["hi"], upper))
            except RuntimeError as e:  # (out of memory at the large size: no yardstick)
                rec["torch_searchsorted_error"] = str(e).splitlines()[0][:120]
            res.clear()
        emit(rec)

    tables = [int(x) for x in args.tables.split(",") if x]
    queries = [int(x) for x in args.queries.split(",") if x]
    kinds = [x for x in args.kinds.split(",") if x]
    laws = [x for x in args.laws.split(",") if x]
    # the cheap points first: by query count, the large tables first inside one count
    for nq in sorted(queries):
        for num in sorted(tables, reverse=True):
            for kind in kinds:
                if time.perf_counter() - t_start > args.max_seconds:
                    emit({"num": num, "num_queries": nq, "kind": kind, "skipped": "max-seconds"})
                    continue
                table = sort_keys(draw(num, kind, 42))
                for law in laws:
                    measure(table, kind, nq, law)
                    torch.cuda.empty_cache()
                del table
                torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
