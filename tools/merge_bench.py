#!/usr/bin/env python3
"""merge on one GPU.

Shapes: "u64" = u64 key + u64 payload (R = 16 bytes per record), "f32" = f32
key + the int64 source column (R = 12). For every (num_a, num_b) of --sizes
both sides are drawn uniform over the key range (u64: all 64 bits; f32:
[-1e6, 1e6)) and sorted by the library; law "equal" makes every key of both
sides the same value (--equal-sizes). Three lines are timed per point,
interleaved call by call in one process:

  merge   srs_amd.merge_device into preallocated outputs (f32: the source
          column comes from torch's allocator inside the timed call, a cached
          block after the warm-up; "before" allocates nothing, so the bias is
          against the merge and shows at the smallest sizes only);
  before  what a caller has without it, whole: the two device copies of every
          column into one buffer, then sort_device out of place (f32: with a
          position column made once outside the timing, whose sorted image is
          the source column);
  torch   torch.sort(torch.cat(...), stable=True) of the keys alone, a
          yardstick only (--yardstick-reps calls, not interleaved; skipped
          above --yardstick-max records).

The floor is 2 * R * (num_a + num_b) bytes over the rate a device copy of
1 GiB reaches in the same process. Every figure is the median wall time of
--reps warm calls that end in a stream synchronise; min and max are kept. The
merge's outputs are compared with before's and must be equal ("equal"). One
JSON line per (shape, law, num_a, num_b) on stdout (and in --out). No new
point is started after --max-seconds. The tool reads nothing outside the
repository.
"""
import argparse
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(REPO, "simd-radix-sort_amd", "python"))

SIZES = ("65536+65536,4194304+4194304,67108864+67108864,536870912+536870912,"
         "1000000000+1048576,1000000000+67108864")
EQUAL_SIZES = "67108864+67108864"
SHAPES = "u64,f32"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=SIZES)
    ap.add_argument("--equal-sizes", default=EQUAL_SIZES)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--yardstick-reps", type=int, default=3)
    ap.add_argument("--yardstick-max", type=int, default=1 << 28)
    ap.add_argument("--max-seconds", type=float, default=float("inf"))
    ap.add_argument("--out", default=None)
    args = ap.parse_args()

    import torch
    import srs_amd
    if not torch.cuda.is_available():
        sys.exit("merge_bench: no GPU (nothing is measured without one)")
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

    def interleaved(fns, reps, warmup):
        """{name: (median, min, max)} of `reps` rounds, one call of each per round"""
        for _ in range(warmup):
            for f in fns.values():
                timed(f)
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
    copy_ms = interleaved({"c": lambda: b.copy_(a)}, args.reps, args.warmup)["c"][0]
    copy_rate = 2 * a.numel() * 8 / (copy_ms * 1e-3)
    del a, b
    torch.cuda.empty_cache()

    def side(n, shape, law, seed):
        """(sorted keys, payload or None) of one side"""
        if shape == "u64":
            k = torch.empty(n, dtype=torch.int64, device=dev)
            p = torch.empty(n, dtype=torch.int64, device=dev)
            srs_amd.fill_synthetic_device(k, p, key_kind=srs_amd.KEY_U64, seed=seed << 32)
            if law == "equal":
                k.fill_(12345)
            srs_amd.sort_device(k, p, key_kind=srs_amd.KEY_U64, cmp_sort_threshold=0)
            return k, p
        g = torch.Generator(device=dev)
        g.manual_seed(seed)
        k = torch.empty(n, dtype=torch.float32, device=dev)
        k.uniform_(-1e6, 1e6, generator=g)
        if law == "equal":
            k.fill_(1.5)
        srs_amd.sort_device(k, cmp_sort_threshold=0)
        return k, None

    def measure(shape, law, na, nb):
        n = na + nb
        kind = srs_amd.KEY_U64 if shape == "u64" else srs_amd.KEY_F32
        rbytes = 16 if shape == "u64" else 12
        rec = {"shape": shape, "law": law, "num_a": na, "num_b": nb, "record_bytes": rbytes,
               "copy_TBps": round(copy_rate / 1e12, 3)}
        try:
            ka, pa = side(na, shape, law, 42)
            kb, pb = side(nb, shape, law, 7)
            torch.cuda.synchronize()
            if shape == "u64":
                m_out = (torch.empty(n, dtype=ka.dtype, device=dev),
                         torch.empty(n, dtype=pa.dtype, device=dev))
                cat = tuple(torch.empty_like(o) for o in m_out)
                s_out = tuple(torch.empty_like(o) for o in m_out)
                src = [None]

                def merge():
                    srs_amd.merge_device((ka, pa), (kb, pb), key_kind=kind, out=m_out)

                def before():
                    cat[0][:na].copy_(ka)
                    cat[0][na:].copy_(kb)
                    cat[1][:na].copy_(pa)
                    cat[1][na:].copy_(pb)
                    srs_amd.sort_device(*cat, key_kind=kind, cmp_sort_threshold=0, out=s_out)

                def equal():
                    return bool(torch.equal(m_out[0], s_out[0]) and torch.equal(m_out[1], s_out[1]))
            else:
                m_out = (torch.empty(n, dtype=ka.dtype, device=dev),)
                pos = torch.arange(n, dtype=torch.int64, device=dev)
                cat = (torch.empty_like(m_out[0]),)
                s_out = (torch.empty_like(m_out[0]), torch.empty_like(pos))
                src = [None]

                def merge():
                    # (indices=True allocates the source column: a cached block after the warm-up)
                    src[0] = None
                    src[0] = srs_amd.merge_device((ka,), (kb,), indices=True, out=m_out)[1]

                def before():
                    cat[0][:na].copy_(ka)
                    cat[0][na:].copy_(kb)
                    srs_amd.sort_device(cat[0], pos, cmp_sort_threshold=0, out=s_out)

                def equal():
                    return bool(torch.equal(m_out[0].view(torch.int32), s_out[0].view(torch.int32))
                                and torch.equal(src[0], s_out[1]))

            m = interleaved({"merge": merge, "before": before}, args.reps, args.warmup)
            rec["equal"] = equal()
            rec["launches"], rec["readbacks"], rec["tiles"], rec["workspace_bytes"] = \
                srs_amd.debug_last_merge()
        except RuntimeError as e:  # (torch out of memory: the line says so, nothing is timed)
            rec["error"] = str(e).splitlines()[0][:160]
            emit(rec)
            return
        put(rec, "merge", m["merge"])
        put(rec, "before", m["before"])
        floor = 2 * rbytes * n / copy_rate * 1e3
        rec["floor_ms"] = round(floor, 4)
        rec["merge_over_floor"] = round(m["merge"][0] / floor, 3)
        rec["before_over_merge"] = round(m["before"][0] / m["merge"][0], 3)
        rec["merge_TBps"] = round(2 * rbytes * n / (m["merge"][0] * 1e-3) / 1e12, 3)
        if args.yardstick_reps > 0 and n <= args.yardstick_max:
            del cat, s_out
            torch.cuda.empty_cache()
            res = {}

            def torch_sort():
                res["v"] = None
                res["v"] = torch.sort(torch.cat((ka, kb)), stable=True)[0]
            try:
                y = interleaved({"y": torch_sort}, args.yardstick_reps, 1)
                put(rec, "torch_sort_cat", y["y"])
                rec["merge_over_torch"] = round(m["merge"][0] / y["y"][0], 3)
            except RuntimeError as e:
                rec["torch_sort_cat_error"] = str(e).splitlines()[0][:120]
            res.clear()
        emit(rec)

    def pairs(text):
        return [tuple(int(v) for v in x.split("+")) for x in text.split(",") if x]

    points = [("uniform", p) for p in pairs(args.sizes)] + \
        [("equal", p) for p in pairs(args.equal_sizes)]
    points.sort(key=lambda lp: lp[1][0] + lp[1][1])  # the cheap points first
    for law, (na, nb) in points:
        for shape in [x for x in args.shapes.split(",") if x]:
            if time.perf_counter() - t_start > args.max_seconds:
                emit({"shape": shape, "law": law, "num_a": na, "num_b": nb,
                      "skipped": "max-seconds"})
                continue
            measure(shape, law, na, nb)
            torch.cuda.empty_cache()
    if out_f:
        out_f.close()


if __name__ == "__main__":
    main()
