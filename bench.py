"""bench.py — MI355X MSB radix sort throughput (BASELINE.json metric).

Metric: Gkeys/s (and achieved HBM GB/s vs the 8 TB/s roofline) sorting 1e9
uint64 keys + one uint64 payload column (BASELINE.json configs[1], "C1").

One step = one full sort of the resident 1e9-key input (out of place: the
pristine input stays untouched, so every step does identical work; the
in-place drop-in runs the very same kernels with IN == OUT). Inputs are
generated on the device (splitmix64 of the global index, payload = f(key))
and are resident in HBM before the timed region.

N > 1 (torchrun, one rank per GPU): every rank holds 1e9 keys (indices
[r*1e9, (r+1)*1e9)); the global array is sorted across ranks by the
top-radix-bits shard of the library's C ABI (srs_shard_*,
csrc/srs_shard.hip, through ctypes): histogram all-reduce, partition,
grouped send/recv over RCCL/xGMI, local sort. Weak scaling.

A plain run sets up, warms up, times the steps and prints the headline
figures (Gkeys/s, ms_per_step, the roofline from the timed steps' own scatter
markers, the pass model). --full adds everything else the line can report,
each from runs of its own after the timed steps: per-kernel times, the
allocator variants, the full-size verification, the CPU baselines and the
extra configs C2 and C3. --dump-outputs DIR writes the last timed step's
output arrays (a fixed sample of them at this size) as DIR/<name>.npy.

Prints ONE JSON line on rank 0.
"""
from __future__ import annotations

import argparse
import json
import os
import platform
import subprocess
import sys
import time

REPO = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(REPO, "simd-radix-sort_amd", "python"))

HBM_PEAK_GBS = 8000.0  # MI355X HBM3E spec (MI355X_MICROARCH.md)

CONFIGS = {
    # name: (key kind name, payload sizes, layout)
    "c1": ("u64", [8], "soa", "1e9 uint64 keys + one uint64 payload column, uniform random"),
    "c2": ("f32", [4, 4], "soa", "1e9 float32 keys + two uint32 payload columns"),
    "c3": ("u64", [8], "aos", "1e9 DataElement<uint64,uint64> combined AoS array"),
    "k64": ("u64", [], "soa", "uint64 keys only (diagnostic)"),
    "k32": ("u32", [], "soa", "uint32 keys only (C0 shape)"),
    "c2w": ("f32", [8], "soa", "float32 keys + one uint64 payload (C2's 12-byte records, "
            "payload as one 8-byte column; diagnostic)"),
}


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--n", type=float, default=1e9, help="keys per GPU")
    ap.add_argument("--config", default="c1", choices=sorted(CONFIGS))
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also measure and check everything else the line "
                         "can report: per-kernel times, the steps with and without event "
                         "markers, the allocator variants, the full-size verification, the CPU "
                         "baselines, the 'extra' configs and the shard line's T(1); without it a "
                         "run sets up, warms up, times the steps and prints the headline figures")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps write what the last timed step computed (the "
                         "sorted key and payload arrays, or a fixed seeded sample of them) as "
                         "DIR/<name>.npy")
    ap.add_argument("--cpu-sample", type=float, default=1e9,
                    help="keys of the headline config's CPU baseline (the reference on one "
                         "host core; 1e9 = the config itself; 0 = skip)")
    ap.add_argument("--cpu-sample-extra", type=float, default=1e9,
                    help="keys of the CPU-baseline sample of each 'extra' config (1e9 = the "
                         "config itself; 0 = skip)")
    ap.add_argument("--cpu-warmup", type=int, default=1,
                    help="untimed warmup sorts before the timed CPU-baseline sort")
    ap.add_argument("--no-verify", action="store_true")
    ap.add_argument("--shard", action="store_true",
                    help="run the multi-GPU shard protocol even at one rank (RCCL, world 1)")
    ap.add_argument("--rounds", type=int, default=0,
                    help="shard exchange rounds (srs_shard_set_options; 0 = library default)")
    ap.add_argument("--chunks", type=int, default=0,
                    help="shard partition chunks (srs_shard_set_options; 0 = library default)")
    ap.add_argument("--t1-ms", type=float, default=None,
                    help="one-GPU step time the --shard world-1 line's 8-GPU model compares "
                         "against (default: measured in the same run: the plain sort of the "
                         "same input, same steps)")
    ap.add_argument("--self-messages", action="store_true",
                    help="shard: own pieces as RCCL messages to the rank itself instead of "
                         "device copies (srs_shard_set_message_options), so that world 1 runs "
                         "every ncclSend / ncclRecv of the exchange")
    ap.add_argument("--msg-cap-mb", type=float, default=0,
                    help="shard: largest message in MiB (0 = the library's 256)")
    ap.add_argument("--alloc-steps", type=int, default=3,
                    help="world 1: extra steps with outputs from torch's allocator and in place "
                         "on a torch array (ms_per_step_plain_alloc / _inplace; 0 = skip)")
    ap.add_argument("--extra", default="c2,c3",
                    help="comma list of further configs measured after the headline one and "
                         "reported under 'extra' (world 1, c1 headline only; 'none' = skip)")
    ap.add_argument("--out-alloc", default="srs", choices=("srs", "torch"),
                    help="memory of the out-of-place outputs: srs_alloc_device (placement "
                         "probed, DESIGN.md §4) or torch's allocator")
    ap.add_argument("--dry-run-launch", action="store_true",
                    help="with --gpus N > 1 and no WORLD_SIZE: print the launcher's argv and "
                         "env as JSON instead of starting the ranks")
    ap.add_argument("--cmp-sorter", default="insertion", choices=("insertion", "nosort"),
                    help="leaf sorter (the reference's CmpSorter, src/cmp_sorters.hpp): "
                         "nosort = CmpSorterNoSort, leaves of <= 16 keys left unsorted")
    ap.add_argument("--dist", default="uniform", choices=DISTS,
                    help="key distribution (the reference's InputDistribution kinds, "
                         "src/data.hpp:64-73; c1 only; payload = f(key) as always)")
    argv = sys.argv[1:]
    if argv[:1] == ["--"]:  # the launcher's separator (launcher_cmd)
        argv = argv[1:]
    args = ap.parse_args(argv)
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")
    return args


DISTS = ("uniform", "gaussian", "zero", "zeroone", "sorted", "reverse", "almostsorted",
         "almostreverse", "span8")


def make_dist_keys(keys, pays, dist, torch, srs_amd, kind):
    """Replaces the uniform keys of a c1 workload (int64 storage of u64 keys)
    by the reference's InputDistribution `dist` (src/data.hpp:115-160):
    Gaussian = round(N(0, 100)); Zero; ZeroOne; Sorted / ReverseSorted =
    uniform, sorted; Almost* = that plus 2^log10(n) random swaps. Sorting
    uses this library (the input of the timed sort is then its own output).
    span8 (not one of the reference's): uniform keys confined to 1/8 of the
    key range (top 3 bits 001), the span one of 8 shard ranks receives
    (DESIGN.md §7). Payloads are recomputed as f(key)."""
    import math
    n = keys.numel()
    g = torch.Generator(device=keys.device)
    g.manual_seed(42)
    if dist == "gaussian":
        keys.copy_(torch.round(torch.randn(n, device=keys.device, generator=g) * 100).to(torch.int64))
    elif dist == "zero":
        keys.zero_()
    elif dist == "zeroone":
        keys.copy_(torch.randint(0, 2, (n,), device=keys.device, generator=g))
    elif dist == "span8":
        for i in range(0, n, 1 << 26):
            k = keys[i:i + (1 << 26)]
            k.copy_(((k >> 3) & ((1 << 61) - 1)) | (1 << 61))
    elif dist in ("sorted", "reverse", "almostsorted", "almostreverse"):
        srs_amd.sort_device(keys, key_kind=kind, up=dist in ("sorted", "almostsorted"))
        if dist.startswith("almost"):
            m = int(2 ** math.log10(n))
            a = torch.randint(0, n, (m,), device=keys.device, generator=g)
            b = torch.randint(0, n, (m,), device=keys.device, generator=g)
            for i, j in zip(a.tolist(), b.tolist()):  # sequential swaps, as the reference
                ki, kj = keys[i].clone(), keys[j].clone()
                keys[i], keys[j] = kj, ki
    for c, p in enumerate(pays):
        salt = (c * 0xD1B54A32D192ED03) & ((1 << 64) - 1)
        salt = salt - (1 << 64) if salt >= 1 << 63 else salt
        for i in range(0, n, 1 << 26):
            f = _splitmix64(_u64_bits(keys[i:i + (1 << 26)], torch) ^ salt, torch)
            p[i:i + (1 << 26)].copy_(f if p.element_size() == 8 else (f & 0xFFFFFFFF).to(p.dtype))


def pmc_traffic(kernel, workload, n):
    """HBM bytes per launch of `kernel` from the committed rocprofv3 PMC
    passes (profiles/<round>_pmc.json, written by tools/profile_summary.py
    from FETCH_SIZE x2 + WRITE_SIZE) of this same workload, or None. PMC
    counters cannot be read from inside the timed process, so the number is
    the profiled run's, matched on workload and size; the latest round wins."""
    import glob
    best = None
    for path in sorted(glob.glob(os.path.join(REPO, "profiles", "*_pmc.json"))):
        try:
            with open(path) as f:
                doc = json.load(f)
        except (OSError, ValueError):
            continue
        if doc.get("keys_per_gpu") != n or not str(doc.get("workload", "")).endswith(workload):
            continue
        ks = [v for v in doc.get("kernels", {}).values() if v.get("name") == kernel]
        if not ks:
            continue
        tot = sum(v["hbm_bytes"] * v["dispatches"] for v in ks)
        cnt = sum(v["dispatches"] for v in ks)
        if cnt:
            best = round(tot / cnt)
    return best


def progress(msg):
    """A progress line on stderr (the JSON line stays alone on stdout): the
    full-config CPU baselines run for minutes, and a run that prints nothing
    for that long looks hung to a watchdog."""
    print(f"[bench {time.strftime('%H:%M:%S')}] {msg}", file=sys.stderr, flush=True)


def kind_id(name):
    import srs_amd
    return {"u64": srs_amd.KEY_U64, "f32": srs_amd.KEY_F32, "u32": srs_amd.KEY_U32}[name]


# ---------------------------------------------------------------------------
# CPU baseline: the reference's own AVX-512 sort (oracle/_ref) on host cores
# ---------------------------------------------------------------------------
def _sm64(x, np):
    x = x + np.uint64(0x9E3779B97F4A7C15)
    x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
    x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return x ^ (x >> np.uint64(31))


def host_workload(cfg_name, n, seed, keys=None, pays=None, chunk=1 << 24, threads=8):
    """The config's records on the host, by the device fill's generator
    (srs_fill_synthetic_device: key = splitmix64(seed + i), payload c =
    splitmix64(bits(key) ^ c * 0xD1B54A32D192ED03)), generated chunk by chunk
    into `keys` / `pays` (allocated when None), chunks on `threads` host
    threads (numpy releases the GIL in its array loops; generation is not
    timed, it only has to stay short)."""
    import numpy as np
    from concurrent.futures import ThreadPoolExecutor
    kname, psizes, _, _ = CONFIGS[cfg_name]
    if keys is None:
        keys = np.empty(n, np.float32 if kname == "f32" else np.uint64)
        pays = [np.empty(n, {4: np.uint32, 8: np.uint64}[s]) for s in psizes]

    def gen(a):
        b = min(n, a + chunk)
        h = _sm64(np.arange(a, b, dtype=np.uint64) + np.uint64(seed), np)
        if kname == "f32":
            k = ((h >> np.uint64(40)).astype(np.int32).astype(np.float32) *
                 np.float32(1.0 / 8388608.0) - np.float32(1.0))
            bits = k.view(np.uint32).astype(np.uint64)
        else:
            k = bits = h
        keys[a:b] = k
        for c, p in enumerate(pays):
            p[a:b] = _sm64(bits ^ np.uint64((c * 0xD1B54A32D192ED03) & 0xFFFFFFFFFFFFFFFF),
                           np).astype(p.dtype)
    with ThreadPoolExecutor(max_workers=max(1, threads)) as ex:
        list(ex.map(gen, range(0, n, chunk)))
    return keys, pays


def cpu_baseline(cfg_name, n_sample, warmups=1):
    """The reference's own sort (oracle/_ref: radixSort.hpp, AVX-512
    BitSorterSIMD) on one host core, timed as its perf harness times it
    (src/perf.hpp:28-89): `warmups` untimed sorts of other data of the same
    shape (measureTimePerElementWithRepsAndWarmup: one warmup and one run at
    n >= 2^22), then one sort timed with CLOCK_PROCESS_CPUTIME_ID around the
    call only. Generated with the device fill's generator."""
    sys.path.insert(0, os.path.join(REPO, "tests"))
    import numpy as np
    from srs_testlib import (oracle_sort_aos, oracle_sort_soa, ref_lib, ref_sort_aos,
                             ref_sort_soa_timed)
    kname, psizes, layout, _ = CONFIGS[cfg_name]
    kind = {"u64": 6, "f32": 8, "u32": 4}[kname]
    n = int(n_sample)
    use_ref = ref_lib() is not None
    t_gen = time.perf_counter()
    keys, pays = host_workload(cfg_name, n, 43 << 32)  # warmup data (another seed)
    gen_s = time.perf_counter() - t_gen

    def one_sort(keys, pays):
        """(wall s, CPU ns) of one sort of the config's records."""
        if layout == "aos":
            rec = np.empty((n, 16), np.uint8)
            rec[:, :8] = keys.view(np.uint8).reshape(n, 8)
            rec[:, 8:] = pays[0].view(np.uint8).reshape(n, 8)
            t0, c0 = time.perf_counter(), time.process_time()
            (ref_sort_aos if use_ref else oracle_sort_aos)(kind, True, rec)
            return time.perf_counter() - t0, (time.process_time() - c0) * 1e9
        t0 = time.perf_counter()
        if use_ref:  # CLOCK_PROCESS_CPUTIME_ID around the sort call only (src/perf.hpp:33-46)
            ns = ref_sort_soa_timed(kind, True, keys, pays)
        else:
            c0 = time.process_time()
            oracle_sort_soa(kind, True, keys, pays)
            ns = (time.process_time() - c0) * 1e9
        return time.perf_counter() - t0, ns

    progress(f"cpu baseline {cfg_name}: {n} keys generated in {gen_s:.1f} s")
    warm = []
    for w in range(warmups):
        if w:
            host_workload(cfg_name, n, (43 + w) << 32, keys, pays)
        warm.append(round(one_sort(keys, pays)[0], 2))
        progress(f"cpu baseline {cfg_name}: warmup sort {w + 1} took {warm[-1]} s")
    host_workload(cfg_name, n, 42 << 32, keys, pays)  # the timed data: the bench's own input
    dt, cpu_ns = one_sort(keys, pays)
    progress(f"cpu baseline {cfg_name}: timed sort {dt:.1f} s wall")
    del keys, pays
    try:
        model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo")
                 if l.startswith("model name")][0]
    except Exception:
        model = platform.processor()
    full = n == int(1e9)
    return {
        "value": n / (cpu_ns / 1e9) / 1e9,
        "unit": "Gkeys/s",
        "cores": 1,
        "kind": "reference" if use_ref else "port",
        "cpu_time_s": round(cpu_ns / 1e9, 3),
        "wall_s": round(dt, 3),
        "value_wall": n / dt / 1e9,
        "warmup_wall_s": warm,
        "sample": (f"{'the full config' if full else 'bounded sample'}: {n} keys of the "
                   f"{cfg_name} workload (the bench's generator and seed), {warmups} untimed "
                   f"warmup sort(s) of other data of the same shape, then one sort timed with "
                   f"CLOCK_PROCESS_CPUTIME_ID around the call (src/perf.hpp:28-89): "
                   f"{cpu_ns / 1e9:.2f} s CPU, {dt:.2f} s wall; single-threaded on 1 core of "
                   f"'{model}' (nproc={os.cpu_count()}); data generation {gen_s:.1f} s "
                   f"(not timed); " +
                   ("reference = jonicho radixSort.hpp BitSorterSIMD AVX-512, compiled from "
                    "/root/reference by oracle/Makefile" if use_ref else
                    "C restatement (host lacks AVX-512 VBMI2)")),
    }


# ---------------------------------------------------------------------------
# --gpus N: one rank per GPU (torch.distributed.run), started before any GPU call
# ---------------------------------------------------------------------------
def launcher_cmd(args, argv):
    """argv + env of the child that runs N ranks of this script. The parent
    never imports torch or touches the GPU; it only waits for the child."""
    import socket
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    fwd = [a for a in argv if a != "--dry-run-launch"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1",
           f"--nproc-per-node={args.gpus}", "--master-addr=127.0.0.1",
           f"--master-port={port}", os.path.abspath(__file__), "--"] + fwd
    # ("--": torchrun's parser would otherwise take bench options that prefix
    # its own, e.g. --n for --nnodes, as ambiguous; parse() drops it)
    env = dict(os.environ)
    env["HSA_ENABLE_IPC_MODE_LEGACY"] = "0"  # dmabuf IPC only on this pool (RCCL)
    env["MASTER_ADDR"] = "127.0.0.1"
    return cmd, env


def launch(args, argv):
    cmd, env = launcher_cmd(args, argv)
    if args.dry_run_launch:
        print(json.dumps({"argv": cmd, "env": {k: env[k] for k in
                                               ("HSA_ENABLE_IPC_MODE_LEGACY", "MASTER_ADDR")}}))
        return 0
    # rank 0 prints the JSON line on the inherited stdout
    return subprocess.run(cmd, env=env).returncode


# ---------------------------------------------------------------------------
def main():
    args = parse()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        sys.exit(launch(args, sys.argv[1:]))
    if env_world is not None and int(env_world) != args.gpus:
        sys.exit(f"bench.py: WORLD_SIZE={env_world} but --gpus {args.gpus}; they must agree")
    import torch
    import torch.distributed as dist

    import srs_amd

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    ndev = torch.cuda.device_count()
    if world > ndev:
        print(f"bench.py: --gpus {world} needs {world} GPUs on this node, {ndev} visible",
              file=sys.stderr, flush=True)
        sys.exit(3)
    shard = world > 1 or args.shard
    if shard:
        # a peer that never arrives ends the library's bounded waits in two
        # minutes instead of its 10-minute default (a bench step takes < 0.1 s)
        os.environ.setdefault("SRS_SHARD_TIMEOUT_S", "120")
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29533")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        torch.cuda.set_device(local_rank)
        dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))
    dev = torch.device("cuda", local_rank)

    res = measure(args.config, args, torch, srs_amd, dist, dev, rank, world, shard,
                  dump_dir=args.dump_outputs)

    cpu = None
    if args.full and rank == 0 and args.cpu_sample > 0 and (world == 1):
        try:
            cpu = cpu_baseline(args.config, min(args.cpu_sample, args.n), args.cpu_warmup)
        except Exception as e:  # report, never hide
            cpu = {"error": repr(e)}

    extra = {}
    if args.full and world == 1 and not shard and args.config == "c1" and args.dist == "uniform":
        for name in [e for e in args.extra.split(",") if e and e != "none"]:
            torch.cuda.empty_cache()
            try:
                r = measure(name, args, torch, srs_amd, dist, dev, rank, world, shard)
            except Exception as e:  # report, never hide
                r = {"error": repr(e)}
            if rank == 0 and args.cpu_sample_extra > 0 and "error" not in r:
                try:
                    r["cpu_baseline"] = cpu_baseline(name, min(args.cpu_sample_extra, args.n),
                                                     args.cpu_warmup)
                except Exception as e:  # report, never hide
                    r["cpu_baseline"] = {"error": repr(e)}
            extra[name] = r

    if rank == 0:
        out = {
            "metric": "Gkeys/s and achieved HBM GB/s (% of roofline), 1e9 uint64 key+uint64 payload",
            "value": res["value"],
            "unit": "Gkeys/s",
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": res["ms_per_step"],
            "full": args.full,
            **{k: res[k] for k in ("ms_per_step_without_event_markers",
                                   "ms_per_step_with_all_event_markers",
                                   "ms_per_step_plain_alloc", "ms_per_step_inplace",
                                   "alloc_variants") if k in res},
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": res["dtype"],
            "data": "synthetic (device splitmix64 of the global index; payload = f(key))",
            "config": res["config"],
            "roofline": res["roofline"],
            "pass_model": res["pass_model"],
        }
        if args.full:
            out.update(kernels=res["kernels"], cpu_baseline=cpu, verified=res["verified"])
        if res.get("dumped") is not None:
            out["dumped"] = res["dumped"]
        if res.get("phases") is not None:
            out["phases"] = res["phases"]
        if extra:
            out["extra"] = extra
        print(json.dumps(out), flush=True)
    if shard:
        dist.destroy_process_group()


def dump_outputs(dump_dir, cols, rank, world, torch):
    """Writes the output arrays `cols` ({name: 1-d device array}, all of one
    length) of the last timed step to dump_dir/<name>.npy. More than 2^20
    records: the records at a fixed, seeded sample of 2^20 positions (first
    and last among them), whose positions go to sample_index.npy. Values keep
    every bit: float32 keys as float32, 4-byte integers as float64, 8-byte
    integers as a float64 (m, 2) array of their (high, low) 32-bit halves.
    At most 2^20 * (8 + 16 + 16) bytes = 40 MiB. Returns the file names."""
    import numpy as np
    os.makedirs(dump_dir, exist_ok=True)
    sfx = "" if world == 1 else f"_rank{rank}"
    n = next(iter(cols.values())).numel()
    m = 1 << 20
    if n > m:
        pos = np.random.default_rng(20240607).choice(n, size=m - 2, replace=False)
        pos = np.unique(np.concatenate([pos, [0, n - 1]])).astype(np.int64)
    else:
        pos = np.arange(n, dtype=np.int64)
    idx = torch.from_numpy(pos).to(next(iter(cols.values())).device)
    arrays = {"sample_index": pos.astype(np.float64)}
    for name, t in cols.items():
        h = t[idx].cpu().numpy()
        if h.dtype == np.float32:
            a = h
        elif h.dtype.itemsize == 4:
            a = h.view(np.uint32).astype(np.float64)
        else:
            u = h.view(np.uint64)
            a = np.stack([(u >> np.uint64(32)).astype(np.float64),
                          (u & np.uint64(0xFFFFFFFF)).astype(np.float64)], axis=1)
        arrays[name] = a
    files = []
    for name, a in arrays.items():
        np.save(os.path.join(dump_dir, f"{name}{sfx}.npy"), a)
        files.append(f"{name}{sfx}.npy")
    return files


def measure(cfg_name, args, torch, srs_amd, dist, dev, rank, world, shard, dump_dir=None):
    """Generates the config's resident input, runs W warmup + K timed steps
    (barrier + synchronize on both sides, max over ranks) and returns the
    config's numbers: Gkeys/s, roofline of the dominant kernel (HIP events
    on the sort's stream) and pass-model bytes; with --full also the
    per-kernel times of further steps, the allocator variants and the
    full-size verification. dump_dir: see dump_outputs."""
    kname, psizes, layout, cdesc = CONFIGS[cfg_name]
    kind = kind_id(kname)
    n = int(args.n)
    if rank == 0:
        progress(f"{cfg_name}: generating {n} records per GPU")

    tdt = {8: torch.int64, 4: torch.int32}
    key_dt = {"u64": torch.int64, "f32": torch.float32, "u32": torch.int32}[kname]
    keys = torch.empty(n, dtype=key_dt, device=dev)
    pays = [torch.empty(n, dtype=tdt[s], device=dev) for s in psizes]
    srs_amd.fill_synthetic_device(keys, *pays, seed=42 << 32, first_index=rank * n, key_kind=kind)
    if args.dist != "uniform" and cfg_name == args.config:
        if cfg_name != "c1":
            raise SystemExit("--dist applies to c1 (u64 keys + u64 payload)")
        make_dist_keys(keys, pays, args.dist, torch, srs_amd, kind)
    rec = rec_out = None
    keys_out, pays_out = None, []
    def out_like(t):
        """an output array like t: srs_alloc_device memory (the sort's writes
        run at the rate of the placement it probes for) or torch's"""
        if args.out_alloc == "torch":
            return torch.empty_like(t)
        return srs_amd.empty_device(t.numel(), t.dtype, t.device).view(t.shape)

    if layout == "aos":
        rec = torch.stack([keys, pays[0]], dim=1).contiguous()
        rec_out = out_like(rec)
        del keys, pays
        keys, pays = None, []
        rec_bytes = 16
    else:
        keys_out = out_like(keys)
        pays_out = [out_like(p) for p in pays]
        rec_bytes = keys.element_size() + sum(psizes)
    torch.cuda.synchronize()

    if shard:
        if layout != "soa":
            raise SystemExit("multi-GPU bench runs the SoA configs (c1, c2)")
        # the library's shard sort over RCCL (srs_shard_*): rank 0's unique
        # id reaches every rank through torch.distributed
        from srs_amd import shard as shard_mod
        uid = torch.zeros(shard_mod.ID_BYTES, dtype=torch.uint8, device=dev)
        if rank == 0:
            uid.copy_(torch.frombuffer(bytearray(shard_mod.unique_id()), dtype=torch.uint8))
        dist.broadcast(uid, 0)
        comm = shard_mod.ShardComm.rccl(world, rank, bytes(uid.cpu().numpy().tobytes()), dev)
        rounds, chunks = args.rounds, args.chunks
        if world == 1 and rounds == 0 and chunks == 0:
            # the world-1 line exists to model the 8-GPU run (t8_model): it
            # runs the plan the library uses at world > 1 (4 chunks, 8
            # rounds), not world 1's own (one chunk: a 10 ms head)
            rounds, chunks = 8, 4
        comm.set_options(rounds, chunks)
        comm.set_message_options(args.self_messages, int(args.msg_cap_mb * (1 << 20)) // 64 * 64)
    shard_out = []

    def step():
        if shard:
            shard_out[:] = [comm.sort(keys, *pays, key_kind=kind)]
            return
        if layout == "aos":
            srs_amd.sort_combined_device(rec, kind, out=rec_out, cmp_sorter=args.cmp_sorter)
        else:
            srs_amd.sort_device(keys, *pays, key_kind=kind, out=(keys_out, *pays_out),
                                cmp_sorter=args.cmp_sorter)

    def sync():
        torch.cuda.synchronize()
        if shard:
            dist.barrier()
        torch.cuda.synchronize()

    def collect():
        out = {}
        for name in ("count", "scatter", "local", "local_fast", "local_stable", "local_lsd",
                     "scan", "plan", "children", "copy", "partition", "key_hist",
                     *[f"{k}.L{i}" for i in range(1, 7) for k in ("count", "scatter")]):
            try:
                l, ms, el = srs_amd.kernel_stats(name)
            except Exception:
                continue
            if l:
                out[name] = {"launches": l, "ms": ms, "elems": el}
        return out

    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    if rank == 0:
        progress(f"{cfg_name}: warmup done, timing {args.steps} steps")
    srs_amd.reset_kernel_stats()
    # The timed steps carry HIP event markers around the scatter launches
    # only (async stream packets, no host waits): the roofline's launch
    # durations come from them.
    srs_amd.set_kernel_timing(2)
    sync()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()
    sync()
    t1 = time.perf_counter()
    srs_amd.set_kernel_timing(False)
    elapsed = t1 - t0
    timed = collect()
    dumped = None
    if dump_dir is not None:
        # what the last timed step left in the arrays its caller receives
        if shard:
            cols = {"keys": shard_out[0][0],
                    **{f"payload{c}": p for c, p in enumerate(shard_out[0][1])}}
        elif layout == "aos":
            cols = {"records_key": rec_out[:, 0], "records_payload": rec_out[:, 1]}
        else:
            cols = {"keys": keys_out, **{f"payload{c}": p for c, p in enumerate(pays_out)}}
        dumped = dump_outputs(dump_dir, cols, rank, world, torch)
    full = args.full
    # --full: the per-kernel breakdown comes from a few more steps with
    # markers around every launch (they cost a step 0.05-0.2 ms), and the
    # same steps without any markers are timed for comparison.
    nb = min(args.steps, 5)
    kstats = timed
    ms_all_events = ms_no_events = None
    if full:
        srs_amd.reset_kernel_stats()
        srs_amd.set_kernel_timing(True)
        sync()
        t2 = time.perf_counter()
        for _ in range(nb):
            step()
        sync()
        ms_all_events = (time.perf_counter() - t2) / nb * 1e3
        srs_amd.set_kernel_timing(False)
        kstats = collect()
        sync()
        t2 = time.perf_counter()
        for _ in range(nb):
            step()
        sync()
        ms_no_events = (time.perf_counter() - t2) / nb * 1e3
    phases = None
    if shard:
        # per-rank phase stamps of the last step (HIP events, from the
        # library's report), the bytes each rank sent to each peer, the
        # implied link rate, the non-overlapped head and tail and the
        # DESIGN.md §7 model's prediction
        rep = comm.report()
        mine = {"rank": rank, "chunks": rep["chunks"], "rounds": rep["rounds"],
                "self_messages": rep.get("self_messages"), "sends": rep.get("sends"),
                "recvs": rep.get("recvs"), "max_message_bytes": rep.get("max_message_bytes"),
                "deferred_frees": rep.get("deferred_frees"),
                "stamps_ms": rep["stamps_ms"],
                "bytes_to_peer_per_round": rep["bytes_to_peer_per_round"],
                **shard_mod.link_figures(rep)}
        if world == 1 and (full or args.t1_ms is not None):
            # the head and tail measured here, in DESIGN.md §7's 8-GPU model
            # against T(1) = the plain one-GPU sort of the same input in the
            # same process (--full) or --t1-ms
            t1 = args.t1_ms
            if t1 is None:
                t1 = plain_step_ms(keys, pays, kind, args.steps, torch, srs_amd)
                mine["t1_ms_measured"] = round(t1, 3)
            mine["t8_model"] = shard_mod.t8_model(
                mine.get("head_ms") or 0.0, mine.get("tail_ms") or 0.0, t1, n=n,
                rec_bytes=rec_bytes)
        allph = [None] * world
        dist.all_gather_object(allph, mine)
        phases = allph
    alloc_ms = {}
    if full and not shard and args.alloc_steps > 0:
        alloc_ms = alloc_variants(args, step_args=(keys, pays, rec, kind, layout), torch=torch,
                                  srs_amd=srs_amd)
    if shard:
        tt = torch.tensor([elapsed], dtype=torch.float64, device=dev)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    ms_per_step = elapsed / args.steps * 1e3
    total_keys = n * world * args.steps
    gkeys = total_keys / elapsed / 1e9

    # ---- per-kernel device time (HIP events on the launch stream) ----------
    ks = 8 if kname == "u64" else 4
    c_b = ks if layout == "soa" else rec_bytes
    per_elem = {"count": c_b, "scatter": 2 * rec_bytes, "local": 2 * rec_bytes}
    dom = max((k for k in kstats if k in per_elem), key=lambda k: kstats[k]["ms"], default=None)
    roofline = None
    if dom:
        # (the timed region's own durations when it measured this kernel)
        s = timed[dom] if dom in timed else kstats[dom]
        avg_ms = s["ms"] / s["launches"]
        bytes_per_launch = per_elem[dom] * s["elems"] / s["launches"]
        achieved = bytes_per_launch / (avg_ms * 1e-3) / 1e9
        roofline = {"bound": "hbm", "kernel": dom, "achieved": round(achieved, 1),
                    "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / HBM_PEAK_GBS, 4),
                    "traffic": pmc_traffic(dom, cdesc, n) if world == 1 else None,
                    "bytes_per_launch": bytes_per_launch, "avg_launch_ms": round(avg_ms, 4)}

    # pass-model yardstick: B_alg = n*[L_g*(c+2s)+2s], and
    # the same model with the global levels this sort actually ran (count
    # launches per step) next to it
    import math
    s_b = rec_bytes
    L_g = min(math.ceil(math.log(max(n / 4096, 1.0001), 256)), ks)
    b_alg = n * (L_g * (c_b + 2 * s_b) + 2 * s_b)
    pass_model_gbs = b_alg * world / (elapsed / args.steps) / 1e9
    levels_run = (kstats.get("count", {}).get("launches", 0) / nb) if full and not shard else None
    pass_model = {"B_alg_bytes_per_gpu": b_alg, "L_g": L_g, "gbs": round(pass_model_gbs, 1),
                  "frac_of_8TBs": round(pass_model_gbs / world / HBM_PEAK_GBS, 4)}
    if levels_run:
        b_run = n * (levels_run * (c_b + 2 * s_b) + 2 * s_b)
        pass_model["global_levels_run"] = levels_run
        pass_model["bytes_of_levels_run"] = b_run
        pass_model["frac_of_8TBs_levels_run"] = round(
            b_run / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS, 4)

    if rank == 0:
        progress(f"{cfg_name}: {ms_per_step:.3f} ms per step" + ("; verifying" if full else ""))
    verified = None
    if not full:
        pass
    elif not args.no_verify and not shard:
        if layout == "aos":
            verified = verify(None, None, rec_out, kname, psizes, torch,
                              ins=(rec[:, 0], [rec[:, 1]]),
                              leaf_unsorted=args.cmp_sorter == "nosort")
        else:
            verified = verify(keys_out, pays_out, None, kname, psizes, torch, ins=(keys, pays),
                              leaf_unsorted=args.cmp_sorter == "nosort")
    elif not args.no_verify:
        verified = verify_shards(keys, pays, shard_out[0], kname, psizes, torch, dist, dev)
    del keys, pays, keys_out, pays_out, rec, rec_out, shard_out
    if shard:
        comm.close()

    return {
        "value": round(gkeys, 4),
        "unit": "Gkeys/s",
        "ms_per_step": round(ms_per_step, 3),
        **({"ms_per_step_without_event_markers": round(ms_no_events, 3),
            "ms_per_step_with_all_event_markers": round(ms_all_events, 3)} if full else {}),
        "dtype": kname if kname != "u64" else "uint64",
        "config": {"workload": cfg_name + ": " + cdesc +
                   ("" if args.dist == "uniform" or cfg_name != args.config
                    else f", {args.dist} keys") +
                   ("" if args.cmp_sorter == "insertion" else ", CmpSorterNoSort leaves"),
                   "keys_per_gpu": n,
                   "total_keys": n * world, "record_bytes": rec_bytes,
                   "parallelism": f"top-radix-bits shard x{world}" if world > 1 else "1 GPU"},
        "roofline": roofline,
        "pass_model": pass_model,
        "kernels": {k: {"launches": v["launches"], "avg_ms": round(v["ms"] / v["launches"], 4),
                        "total_ms_per_step": round(v["ms"] / nb, 3)}
                    for k, v in kstats.items()} if full else None,
        "verified": verified,
        "dumped": dumped,
        **alloc_ms,
        **({"phases": phases} if phases is not None else {}),
    }


def plain_step_ms(keys, pays, kind, steps, torch, srs_amd):
    """ms per plain one-GPU sort (out of place into srs_alloc_device outputs)
    of the same resident input, as the headline line times it: the T(1) of
    the world-1 shard line's 8-GPU model."""
    ko = srs_amd.empty_device(keys.numel(), keys.dtype, keys.device).view(keys.shape)
    po = [srs_amd.empty_device(p.numel(), p.dtype, p.device).view(p.shape) for p in pays]
    srs_amd.sort_device(keys, *pays, key_kind=kind, out=(ko, *po))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        srs_amd.sort_device(keys, *pays, key_kind=kind, out=(ko, *po))
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    del ko, po
    return ms


def alloc_variants(args, step_args, torch, srs_amd):
    """What a caller that does not use srs_alloc_device gets:
    a few steps whose outputs come from torch's allocator (plain hipMalloc
    memory) and a few steps sorting a torch array IN PLACE (the reference's
    own contract, radixSort.hpp:1780), each on a fresh copy of the input
    (the copy is outside the timed sort). Per-step times (synchronised), in
    ms; the median is reported."""
    keys, pays, rec, kind, layout = step_args
    k = args.alloc_steps
    src = [rec] if layout == "aos" else [keys, *pays]
    outs = [torch.empty_like(t) for t in src]
    work = [torch.empty_like(t) for t in src]

    def sort(cols, out):
        if layout == "aos":
            srs_amd.sort_combined_device(cols[0], kind, out=None if out is None else out[0],
                                         cmp_sorter=args.cmp_sorter)
        else:
            srs_amd.sort_device(cols[0], *cols[1:], key_kind=kind, out=out,
                                cmp_sorter=args.cmp_sorter)

    def timed(fn, prep=None):
        ts = []
        for _ in range(k):
            if prep:
                prep()
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return round(sorted(ts)[len(ts) // 2], 3), [round(t, 3) for t in ts]

    def restore():
        for w, s_ in zip(work, src):
            w.copy_(s_)

    def split(fn, prep=None):
        # one more step with HIP-event markers around every launch: which
        # kernels the unplaced memory slows down (ms per launch)
        if prep:
            prep()
        torch.cuda.synchronize()
        srs_amd.reset_kernel_stats()
        srs_amd.set_kernel_timing(True)
        try:
            fn()
            torch.cuda.synchronize()
        finally:
            srs_amd.set_kernel_timing(False)
        out = {}
        for name in ("count", "scan", "local", "scatter.L1", "scatter.L2"):
            try:
                l, ms, _ = srs_amd.kernel_stats(name)
            except Exception:
                continue
            if l:
                out[name] = round(ms / l, 4)
        return out

    # the placement probe's write rate of each buffer (ms per GB; DESIGN.md
    # §4: a slow-class buffer probes slow) before anything is written to it
    probe = {}
    if hasattr(srs_amd, "debug_probe_write"):
        for name, bufs in (("plain_alloc", outs), ("inplace", work)):
            probe[name] = [round(srs_amd.debug_probe_write(t.data_ptr(), t.numel() * t.element_size())
                                 / (t.numel() * t.element_size() / 1e9), 4) for t in bufs]
    plain, plain_all = timed(lambda: sort(src, tuple(outs)))
    inplace, inplace_all = timed(lambda: sort(work, None), prep=restore)
    ok = all(torch.equal(w, o) for w, o in zip(work, outs))
    kern = {"plain_alloc": split(lambda: sort(src, tuple(outs))),
            "inplace": split(lambda: sort(work, None), prep=restore)}
    del outs, work
    torch.cuda.empty_cache()
    return {"ms_per_step_plain_alloc": plain, "ms_per_step_inplace": inplace,
            "alloc_variants": {"steps": k, "plain_alloc_ms": plain_all, "inplace_ms": inplace_all,
                               "inplace_equals_out_of_place": ok,
                               "kernel_ms_per_launch": kern, "probe_ms_per_gb": probe,
                               "note": "outputs from torch's allocator / sorted in place on a "
                                       "torch array restored from the input before each step; "
                                       "median of the steps (the headline's outputs come from "
                                       "srs_alloc_device)"}}


def _order_view(k, kname, torch):
    if kname == "u64":
        return k ^ torch.iinfo(torch.int64).min  # unsigned order as signed
    if kname == "u32":
        return k.to(torch.int64) & 0xFFFFFFFF
    return k


def _u64_bits(x, torch):
    """int64 view of key/payload bits (zero-extended for 4-byte types)."""
    if x.element_size() == 8:
        return x.view(torch.int64)
    return x.view(torch.int32).to(torch.int64) & 0xFFFFFFFF


def _splitmix64(x, torch):
    """splitmix64 in wrapping int64 arithmetic (logical shifts by masking);
    the device generator's payload rule (srs_kernels.hip fill_kernel)."""
    x = x + (0x9E3779B97F4A7C15 - (1 << 64))
    x = (x ^ ((x >> 30) & ((1 << 34) - 1))) * (0xBF58476D1CE4E5B9 - (1 << 64))
    x = (x ^ ((x >> 27) & ((1 << 37) - 1))) * (0x94D049BB133111EB - (1 << 64))
    return x ^ ((x >> 31) & ((1 << 33) - 1))


def _check_payloads(k, pays, psizes, torch, chunk=1 << 26):
    """payload column c == splitmix64(bits(key) ^ c*0xD1B54A32D192ED03),
    truncated to its width, for every element (the generator's rule)."""
    for c, (p, w) in enumerate(zip(pays, psizes)):
        salt = (c * 0xD1B54A32D192ED03) & ((1 << 64) - 1)
        salt = salt - (1 << 64) if salt >= 1 << 63 else salt
        for i in range(0, k.numel(), chunk):
            kb = _u64_bits(k[i:i + chunk], torch)
            f = _splitmix64(kb ^ salt, torch)
            if w == 4:
                f = f & 0xFFFFFFFF
            if not bool((f == _u64_bits(p[i:i + chunk], torch)).all().item()):
                return False
    return True


def _hash_pairs(k, pays, torch, chunk=1 << 26):
    """Order-independent checksum of the records: wrapping int64 sum of a
    mixed hash of (key, payload...)."""
    tot = 0
    for i in range(0, k.numel(), chunk):
        x = _u64_bits(k[i:i + chunk], torch) * (0x9E3779B97F4A7C15 - (1 << 64))
        for p in pays:
            x = (x ^ _u64_bits(p[i:i + chunk], torch)) * (0xBF58476D1CE4E5B9 - (1 << 64))
        x = x ^ ((x >> 29) & 0x7FFFFFFFF)
        tot = (tot + int(x.sum().item())) & ((1 << 64) - 1)
    return tot - (1 << 64) if tot >= 1 << 63 else tot


def verify_shards(keys_in, pays_in, out, kname, psizes, torch, dist, dev):
    """Multi-GPU: each rank sorted; last key of rank r <= first of rank r+1
    (exact, in the transformed order); payload == f(key) everywhere; the
    record multiset over all ranks is unchanged."""
    k, ps = out
    s = _order_view(k, kname, torch)
    ok = bool((s[1:] >= s[:-1]).all().item()) if s.numel() > 1 else True
    ok = ok and _check_payloads(k, ps, psizes, torch)
    world = dist.get_world_size()
    if s.numel():
        ends = torch.stack([s[0], s[-1]]).to(torch.float64 if s.is_floating_point() else torch.int64)
    else:
        ends = torch.zeros(2, dtype=torch.float64 if s.is_floating_point() else torch.int64, device=dev)
    cnt = torch.tensor([s.numel()], dtype=torch.int64, device=dev)
    allends = [torch.zeros_like(ends) for _ in range(world)]
    allcnt = [torch.zeros_like(cnt) for _ in range(world)]
    dist.all_gather(allends, ends)
    dist.all_gather(allcnt, cnt)
    nonempty = [e.tolist() for e, c in zip(allends, allcnt) if c.item() > 0]
    bounds_ok = all(a[1] <= b[0] for a, b in zip(nonempty, nonempty[1:]))
    h = torch.tensor([_hash_pairs(keys_in, pays_in, torch), _hash_pairs(k, ps, torch),
                      keys_in.numel(), k.numel()], dtype=torch.int64, device=dev)
    dist.all_reduce(h)
    okt = torch.tensor([1 if ok else 0], device=dev)
    dist.all_reduce(okt, op=dist.ReduceOp.MIN)
    return {"sorted_and_payload_eq_f_key": bool(okt.item()), "rank_bounds_ordered": bounds_ok,
            "multiset_hash_equal": h[0].item() == h[1].item(),
            "count_equal": h[2].item() == h[3].item()}


def verify(keys_out, pays_out, rec_out, kname, psizes, torch, ins=None, leaf_unsorted=False):
    """Size-independent checks on the full output: sortedness (transformed
    order), payload == f(key) for every element, and an order-independent
    hash of all (key, payload) records equal to the input's (catches a
    dropped record replaced by a duplicate of its neighbour). With payload =
    f(key) the sorted output is unique, so this is bit-exact parity at full
    size."""
    if rec_out is not None:
        k = rec_out[:, 0]
        p = [rec_out[:, 1]]
    else:
        k, p = keys_out, pays_out
    s = _order_view(k, kname, torch)
    if leaf_unsorted:  # CmpSorterNoSort: within 15 places of the sorted order
        ok = bool((s[16:] >= s[:-16]).all().item())
    else:
        ok = bool((s[1:] >= s[:-1]).all().item())
    res = {"sorted" if not leaf_unsorted else "sorted_up_to_16_key_leaves": ok, "payload_eq_f_key": _check_payloads(k, p, psizes, torch)}
    if ins is not None:
        res["multiset_hash_equal"] = _hash_pairs(ins[0], ins[1], torch) == _hash_pairs(k, p, torch)
        res["count_equal"] = ins[0].numel() == k.numel()
    return res


if __name__ == "__main__":
    main()
