#!/usr/bin/env python3
"""bench.py -- reads/sec of the SMEM seeding hot path on N MI355X (one process per GPU).

A "step" is one pass of the hot path (reads packed 32 bases per record, 3-round SMEM collection, sort, SAL) over one batch of synthetic
150-bp reordered reads that is already resident in HBM; results stay in HBM.  Every rank holds a replica of the
index and its own contiguous share of the read run (weak scaling, no data-path collective: the path shards by
reads).  Rank 0 prints ONE JSON line.  See DESIGN.md "Measurement" for the roofline and cpu_baseline definitions.

    python bench.py                       # 1 GPU, defaults: the headline only
    python bench.py --full                # the headline and everything below
    python bench.py --dump-outputs DIR    # also write what the last timed step computed, DIR/<name>.npy
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
        bench.py --gpus N --steps K --warmup W

A plain run sets up (genome, index, engine, reads), warms up, times the K steps and prints the line: `value` (reads/s), `ms_per_step`,
the workload and nothing that needs work of its own.  With --full the line also holds (each measured after the timed region):
  parity          a STRIDED sample of every rank's batch (every (n/20000)-th read, so the whole genome with its repeats is
                  covered) compared bit for bit with the oracle; a mismatch nulls `value` and the process exits 1
  roofline        byte model of THIS implementation (bytes the kernels request from the index-side arrays, counted on the
                  device by the counting instantiations in one extra pass) over the live HIP-event time of the SMEM stage;
                  `traffic` = FETCH_SIZE of the same stage from a rocprofv3 --pmc child run of this very script (N = 1)
  cpu_baseline    the real reference (oracle/_ref, kind "reference") or, without it, the oracle (CPU port), timed on this box's host
                  cores on a bounded sample
  pcie_inclusive  the host-buffer boundary call (H2D of reads, D2H of results), SURVEY 8(d)'s metric; never `value`
  one_step_at_a_time, workloads, extension, ingest_rank0: see DESIGN.md section 5

--dump-outputs writes, after the timed steps, what the last one returned for a fixed sample of its reads (dump_outputs below); the
inputs depend on the arguments only, so two builds run with the same arguments can be compared array for array.
"""
import argparse
import json
import os
os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")  # before the HIP runtime starts: the engine's streams + torch's must not share hardware queues

import shutil
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

HBM_PEAK_GBS = 8000.0  # MI355X_MICROARCH.md: 8 TB/s spec
STAGE_KERNELS = ("fwd0_kernel", "fwd_kernel", "bwd_win0_kernel", "bwd_win_kernel", "bwd_wide_kernel", "bwd_all_kernel", "r2text_kernel",
                 "r3text_kernel", "tail_kernel", "smem_kernel")


def log(*a):
    print("[bench]", *a, file=sys.stderr, flush=True)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--genome-mbp", type=float, default=float(os.environ.get("CS_BENCH_GENOME_MBP", "3100")),
                    help="synthetic genome size in Mbp (3100 = hg19 scale)")
    ap.add_argument("--reads", type=int, default=int(os.environ.get("CS_BENCH_READS", "10000000")), help="reads per GPU per step")
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--profile", default="default", help="workload profile of tools/synth.py (default = BASELINE configs[1] proxy)")
    ap.add_argument("--no-sal", action="store_true")
    ap.add_argument("--no-host-io", action="store_true", help="skip the PCIe-inclusive measurement (cs_engine_seed_batch)")
    ap.add_argument("--sst", type=int, default=1, help="on-device SST memo and every shortcut (1 = on, 0 = the literal algorithm)")
    ap.add_argument("--disable", default="", help="comma-separated shortcuts to switch off (cs_params_t.disable): " +
                    "text_mode,r2_text,text_sweep,window,r3_text,kmer_filter,fwd0")
    ap.add_argument("--opt", action="append", default=[], help="engine option key=value (cs_engine_options_t), repeatable")
    ap.add_argument("--cpu-seconds", type=float, default=15.0, help="target duration of the CPU baseline sample (0 = skip)")
    ap.add_argument("--check-reads", type=int, default=20000, help="reads per rank compared bit-for-bit against the oracle (strided sample)")
    ap.add_argument("--traffic", choices=["live", "none"], default="live",
                    help="live: HBM bytes of the SMEM stage from a rocprofv3 --pmc FETCH_SIZE child run of this script (N = 1 only)")
    ap.add_argument("--pmc-child", default="", help=argparse.SUPPRESS)  # internal: the profiled child of --traffic live
    ap.add_argument("--lib", default="", help="alternative build of libcompseed_amd.so (A/B experiments)")
    ap.add_argument("--dist-backend", choices=["nccl", "gloo"], default="nccl",
                    help="torch.distributed backend of the N > 1 path: nccl (= RCCL over xGMI, the default) or gloo (barrier / max / sum and the "
                         "collectives of --index-broadcast / --ingest-rank0 on CPU tensors staged from the engine's device memory: what lets the "
                         "whole N > 1 code path run with several ranks on ONE GPU, tests/test_gpu_multirank.py)")
    ap.add_argument("--side-workloads", default="repeat50",
                    help="comma-separated workload profiles measured after the headline in a child run of this script (N = 1 only; '' = none): "
                         "reported under `workloads`, never part of `value`")
    ap.add_argument("--in-flight", type=int, default=2, choices=[1, 2],
                    help="device batches kept in flight in the timed region (cs_engine_submit_device / collect_device; 1 = one blocking cs_engine_seed_batch_device per step)")
    ap.add_argument("--no-extension", action="store_true", help="skip the seed-extension side measurement (`extension` key)")
    ap.add_argument("--side-child", action="store_true", help=argparse.SUPPRESS)  # internal: a child run for `workloads`
    ap.add_argument("--index-broadcast", action="store_true",
                    help="N > 1: rank 0 builds the index and broadcasts it over RCCL instead of every rank building its own replica")
    ap.add_argument("--ingest-rank0", action="store_true",
                    help="after the timed region also time the north_star's data movement: rank 0 holds the whole chunk (N x --reads reads), "
                         "scatters contiguous read ranges over RCCL, every rank seeds its range, rank 0 gathers mems and seeds")
    ap.add_argument("-k", type=int, default=19); ap.add_argument("-r", type=float, default=1.5)
    ap.add_argument("-y", type=int, default=20); ap.add_argument("-c", type=int, default=500); ap.add_argument("-s", type=int, default=10)
    ap.add_argument("--full", action="store_true",
                    help="after the headline also run the parity gate, roofline, traffic, CPU baseline, PCIe-inclusive, one-step-at-a-time, "
                         "side-workload and extension measurements (off: set up, warm up, time --steps steps, print the line)")
    ap.add_argument("--dump-outputs", default="", metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (float64; a fixed sample of the reads, at most 64 MB)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be >= 1 and --warmup >= 0")
    if args.ingest_rank0 and not args.full:
        ap.error("--ingest-rank0 is one of the --full measurements")
    return args


def workload_args(args):
    """the flags that define the workload, for the profiled child"""
    out = ["--genome-mbp", str(args.genome_mbp), "--reads", str(args.reads), "--read-len", str(args.read_len), "--profile", args.profile,
           "--sst", str(args.sst), "-k", str(args.k), "-r", str(args.r), "-y", str(args.y), "-c", str(args.c), "-s", str(args.s)]
    if args.no_sal:
        out.append("--no-sal")
    if args.disable:
        out += ["--disable", args.disable]
    for o in args.opt:
        out += ["--opt", o]
    if args.lib:
        out += ["--lib", args.lib]
    return out


def pmc_traffic(args):
    """FETCH_SIZE of one pass of the SMEM stage, per kernel, from a rocprofv3 child run of this script (counters in a run of
    their own with --kernel-trace only, as the guide prescribes).  Also the probe kernel's FETCH_SIZE per random 32-byte
    record read (the calibration of the counter for this access shape) and per-kernel durations with the dispatches
    serialised by the profiler.  Returns None when rocprofv3 is missing or the run fails."""
    exe = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(exe):
        return None
    import csv
    import glob
    td = tempfile.mkdtemp(prefix="cs_pmc_", dir="/tmp")
    info = os.path.join(td, "child.json")
    cmd = [exe, "--kernel-trace", "--pmc", "FETCH_SIZE", "--output-format", "csv", "-d", os.path.join(td, "out"), "--",
           sys.executable, os.path.abspath(__file__), "--pmc-child", info] + workload_args(args)
    env = dict(os.environ, TMPDIR="/tmp")
    t0 = time.time()
    try:
        r = subprocess.run(cmd, cwd="/tmp", env=env, capture_output=True, text=True, timeout=900)
    except Exception as ex:  # noqa: BLE001
        log("rocprofv3 child failed: %r" % (ex,))
        shutil.rmtree(td, ignore_errors=True)
        return None
    if r.returncode != 0 or not os.path.exists(info):
        log("rocprofv3 child failed (rc %d): %s" % (r.returncode, r.stderr[-400:]))
        shutil.rmtree(td, ignore_errors=True)
        return None
    child = json.load(open(info))
    fetch, dur, calls = {}, {}, {}
    probe_kib = None
    for f in glob.glob(os.path.join(td, "out", "**", "*counter_collection.csv"), recursive=True):
        for row in csv.DictReader(open(f)):
            if row["Counter_Name"] != "FETCH_SIZE":
                continue
            k = row["Kernel_Name"]
            if "random_block_chain_kernel" in k:
                probe_kib = float(row["Counter_Value"])
                continue
            name = next((n for n in STAGE_KERNELS if n in k), None)
            if name == "fwd_kernel" and "fwd0_kernel" in k:
                name = "fwd0_kernel"
            if name == "bwd_win_kernel" and "bwd_win0_kernel" in k:
                name = "bwd_win0_kernel"
            if name:
                fetch[name] = fetch.get(name, 0.0) + float(row["Counter_Value"]) * 1024.0
                calls[name] = calls.get(name, 0) + 1
                if "Start_Timestamp" in row and "End_Timestamp" in row:
                    dur[name] = dur.get(name, 0.0) + (int(row["End_Timestamp"]) - int(row["Start_Timestamp"])) / 1e6
    shutil.rmtree(td, ignore_errors=True)
    passes = max(1, int(child.get("passes", 1)))
    if not fetch:
        return None
    out = {"source": "rocprofv3 --kernel-trace --pmc FETCH_SIZE child run of this script (%d pass(es), %.0f s)" % (passes, time.time() - t0),
           "per_kernel_bytes": {k: v / passes for k, v in fetch.items()},
           "per_kernel_ms_serialised": {k: v / passes for k, v in dur.items()} if dur else None,
           "per_kernel_dispatches": {k: v / passes for k, v in calls.items()},
           "stage_bytes": sum(fetch.values()) / passes}
    if probe_kib and child.get("probe_record_reads"):
        out["probe_fetch_bytes_per_random_record_read"] = probe_kib * 1024.0 / child["probe_record_reads"]
    return out


def cpu_quota():
    """CPUs this process may actually use: the affinity mask, cut down to the cgroup's CPU bandwidth quota where one is set (a GPU box
    hands each GPU a share of the host's cores that way; threads beyond the quota are throttled, not run).  Returns (cpus, source)."""
    n = len(os.sched_getaffinity(0))
    src = "affinity mask"
    for path, parse in (("/sys/fs/cgroup/cpu.max", lambda t: None if t.split()[0] == "max" else float(t.split()[0]) / float(t.split()[1])),
                        ("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", None)):
        try:
            txt = open(path).read().strip()
            if parse is None:
                q = float(txt)
                per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read().strip())
                quota = None if q <= 0 else q / per
            else:
                quota = parse(txt)
            if quota is not None and quota > 0 and quota < n:
                n, src = max(1, int(quota + 0.5)), "cgroup quota (%s)" % path
            break
        except (OSError, ValueError, IndexError, ZeroDivisionError):
            continue
    return n, src


def cpu_model():
    try:
        for ln in open("/proc/cpuinfo"):
            if ln.startswith("model name"):
                return ln.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown"


DUMP_READS, DUMP_SEED, DUMP_BYTES = 16384, 20261016, 64 << 20


def dump_outputs(eng, res, args, rank, world):
    """--dump-outputs: what the last timed step returned (res: its device result).  The whole result is ~6 GB of mems and seeds, so what
    is written is the CSR slice a caller receives for a fixed, seeded sample of the batch's reads (cs_engine_gather_reads: mem_off, mems,
    seed_off, seeds, cut to the first sampled reads that fit 64 MB), the batch's totals, and the device-side digests of the whole result
    (cs_engine_result_digest) as 16-bit limbs.  float64 throughout: every value is an integer below 2^53 (positions < 2^37, interval
    bounds < 2^34, info < 2^47), so exact."""
    rng = np.random.default_rng(DUMP_SEED)
    ids = np.sort(rng.choice(args.reads, size=min(DUMP_READS, args.reads), replace=False)).astype(np.uint64)
    got = eng.gather_reads(ids)
    sal = got.seed_off is not None
    n_m = np.diff(got.mem_off.astype(np.int64))
    n_s = np.diff(got.seed_off.astype(np.int64)) if sal else np.zeros_like(n_m)
    per_read = 8 * (3 + 4 * n_m + 3 * n_s)                 # id, two offsets, 4 words per mem, 3 per seed
    k = int(np.searchsorted(np.cumsum(per_read), DUMP_BYTES - (1 << 20), side="right"))
    m_end = int(got.mem_off[k])
    arrays = {"read_ids": ids[:k], "mem_off": got.mem_off[:k + 1],
              "mems": np.stack([got.mems[f][:m_end] for f in ("x0", "x1", "x2", "info")], axis=1)}
    if sal:
        s_end = int(got.seed_off[k])
        arrays["seed_off"] = got.seed_off[:k + 1]
        arrays["seeds"] = np.stack([got.seeds[f][:s_end] for f in ("rbeg", "qbeg", "len")], axis=1)
    dg = np.array(eng.result_digest(), dtype=np.uint64)
    arrays["digest"] = np.stack([(dg >> np.uint64(16 * i)) & np.uint64(0xFFFF) for i in range(4)], axis=1)   # [mem_off, mems, seed_off, seeds] x limb
    arrays["totals"] = np.array([res.n_reads, res.n_mems, res.n_seeds], dtype=np.uint64)
    os.makedirs(args.dump_outputs, exist_ok=True)
    prefix = "rank%d." % rank if world > 1 else ""
    for name, a in arrays.items():
        a = np.asarray(a)
        assert a.size == 0 or max(int(a.max()), -int(a.min())) < 2 ** 53, name
        np.save(os.path.join(args.dump_outputs, prefix + name + ".npy"), a.astype(np.float64))
    log("outputs of the last timed step: %d of %d reads sampled, %s written to %s" % (k, args.reads, ", ".join(sorted(arrays)), args.dump_outputs))


def main():
    args = parse_args()
    if args.lib:
        os.environ["CS_LIB"] = args.lib
    world_env = int(os.environ.get("WORLD_SIZE", "1"))
    traffic = None
    if args.full and args.traffic == "live" and not args.pmc_child and world_env == 1:
        traffic = pmc_traffic(args)  # before this process touches the GPU: the child needs the HBM

    import torch
    if not torch.cuda.is_available():
        sys.exit("bench.py needs a GPU: the seeding engine has no CPU path")
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if local >= torch.cuda.device_count():    # more ranks than GPUs (the one-GPU rehearsal of the N > 1 path): share the devices
        log("LOCAL_RANK %d on a box with %d GPU(s): using device %d" % (local, torch.cuda.device_count(), local % torch.cuda.device_count()))
        local %= torch.cuda.device_count()
    torch.cuda.set_device(local)
    dev = torch.device("cuda", local)
    import compseed_amd as ca
    from compseed_amd.sharding import Dist
    import synth
    D = Dist(args.dist_backend, local=local)   # RCCL by default; used for the barrier and the max-over-ranks clock only
    rank, world = D.rank, D.world
    cdev = dev if args.dist_backend == "nccl" else torch.device("cpu")   # where the collectives' tensors live
    if world != args.gpus and world > 1:
        log("WORLD_SIZE %d != --gpus %d, using WORLD_SIZE" % (world, args.gpus))

    # ---- workload: synthetic genome (same on every rank), index built on this rank's GPU, reads of this rank's share
    t0 = time.time()
    L = int(args.genome_mbp * 1e6)
    prof = synth.PROFILES[args.profile]
    # the same inputs in every run: planted repeat copies overlap, and G[idx] = copies with repeated indices keeps an arbitrary one of
    # them unless deterministic algorithms are on (then index_put_ sorts the indices)
    torch.use_deterministic_algorithms(True)
    G = synth.make_genome(L, seed=20261003, device=dev, **prof["genome"])
    torch.use_deterministic_algorithms(False)
    g_host = G.cpu().numpy()
    torch.cuda.synchronize()
    t1 = time.time()
    torch.cuda.empty_cache()
    from compseed_amd.sharding import Collectives, device_tensor_view
    coll = Collectives(D, cdev)
    if args.index_broadcast and world > 1:  # one build, then the arrays travel over xGMI
        arrays = None
        if rank == 0:
            ix0 = ca.Index.build(g_host, local)
            bw0, sa0 = ix0.arrays()
            arrays = dict(primary=ix0.view.primary, L2=[ix0.view.L2[i] for i in range(1, 5)], bwt=bw0, sa=sa0, sa_intv=32)
        tb = time.time()
        arrays = coll.broadcast_index(arrays)
        torch.cuda.synchronize()
        if rank == 0:
            log("index broadcast to %d ranks: %.2f s for %.2f GB" % (world, time.time() - tb, (arrays["bwt"].nbytes + arrays["sa"].nbytes) / 1e9))
        ix = ix0 if rank == 0 else ca.Index.from_arrays(arrays["primary"], arrays["L2"], arrays["bwt"], arrays["sa"], arrays["sa_intv"])
        torch.cuda.empty_cache()
    else:
        ix = ca.Index.build(g_host, local)
    del g_host
    t2 = time.time()
    eopts = {}
    for o in args.opt:
        k, v = o.split("=", 1)
        eopts[k] = int(v)
    eng = ca.Engine(ix, local, **eopts)
    t3 = time.time()
    rkw = dict(prof["reads"])
    torch.use_deterministic_algorithms(True)
    bases, off = synth.make_reads(G, args.reads, args.read_len, seed=777 + rank, lo_frac=rank / world, hi_frac=(rank + 1) / world, **rkw)
    torch.use_deterministic_algorithms(False)
    n_bases = bases.numel()
    torch.cuda.synchronize()
    del G
    torch.cuda.empty_cache()
    if rank == 0:
        log("genome %.0f Mbp (%s): generate %.1fs, index build %.1fs (seq_len %d), engine %.1fs, reads %d x %d in %.1fs" %
            (args.genome_mbp, args.profile, t1 - t0, t2 - t1, ix.view.seq_len, t3 - t2, args.reads, args.read_len, time.time() - t3))
    dis = ca.disable_mask(*[d for d in args.disable.split(",") if d])
    pk = dict(k=args.k, r=args.r, s=args.s, c=args.c, y=args.y, want_sal=0 if args.no_sal else 1, sst_mode=args.sst, disable=dis)
    par = ca.Params(**pk)

    def step(p=par):
        return eng.seed_batch_device(bases.data_ptr(), off.data_ptr(), args.reads, n_bases, p)

    if args.pmc_child:  # the profiled child of --traffic live: a calibration probe, a priming pass, one pass; then out
        eng.probe_random_lines(4, 64)   # n_cu x 4 blocks of 256 lanes, 64 dependent random record reads each
        probe_reads = int(torch.cuda.get_device_properties(local).multi_processor_count) * 4 * 256 * 64
        step(); step()
        json.dump({"passes": 2, "probe_record_reads": probe_reads}, open(args.pmc_child, "w"))
        eng.close(); ix.close()
        return 0

    def run_steps(k, in_flight):
        """k steps = k passes of the hot path over the batch, every one complete when this returns.  in_flight 2: the steps go through
        cs_engine_submit_device / cs_engine_collect_device, two at a time on the engine's two pass contexts (the tail of one pass beside
        the start of the next -- how a worker with a queue of device-resident batches drives the engine); 1: one blocking call per step"""
        r_ = None
        if in_flight <= 1:
            for _ in range(k):
                r_ = step()
            return r_
        for _ in range(min(in_flight, k)):
            eng.submit_device(bases.data_ptr(), off.data_ptr(), args.reads, n_bases, par)
        for i in range(k):
            r_ = eng.collect_device()
            if i + in_flight < k:
                eng.submit_device(bases.data_ptr(), off.data_ptr(), args.reads, n_bases, par)
        return r_

    in_flight = min(args.in_flight, int(eng.options.passes_in_flight))
    step()  # never time the first call of an engine: it sizes and allocates the batch buffers (setup, like the index upload)
    if in_flight > 1:
        run_steps(2, in_flight)  # ... of both pass contexts
    run_steps(args.warmup, in_flight)
    eng.reset_stats()
    D.barrier()
    torch.cuda.synchronize()
    ts = time.perf_counter()
    res = run_steps(args.steps, in_flight)
    torch.cuda.synchronize()
    D.barrier()
    elapsed = D.max_over_ranks(time.perf_counter() - ts)
    st_timed = eng.stats()
    if args.dump_outputs:   # before anything else runs on the engine: its last result is the last timed step's
        dump_outputs(eng, res, args, rank, world)

    total_reads = args.reads * world * args.steps
    value = total_reads / elapsed
    out = {
        "metric": "reads/sec (150bp) seeded", "value": value, "unit": "reads/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": 1e3 * elapsed / args.steps, "higher_is_better": True, "scaling": "weak",
        "vs_baseline": None, "dtype": "u64", "data": "synthetic",
        "steps_in_flight": in_flight,
        "config": {"workload": "%s; %d x %d bp %s reads per GPU per step; -k %d -r %g -y %d -c %d%s" %
                               (prof["describe"](args.genome_mbp), args.reads, args.read_len, "position-sorted" if rkw.get("sort", True) else "shuffled",
                                args.k, args.r, args.y, args.c, " (mems only)" if args.no_sal else " + SAL"),
                   "profile": args.profile, "genome_mbp": args.genome_mbp, "reads_per_gpu_per_step": args.reads, "read_len": args.read_len,
                   "parallelism": "reads sharded over %d GPU(s), index replicated" % world},
    }
    if not args.full:
        if rank == 0:
            print(json.dumps(out), flush=True)   # the ONE line
        eng.close(); ix.close()
        D.close()
        return 0

    # the same steps one at a time (blocking calls): the HIP-event times of the stage mean "the stage alone on the GPU" only here, so
    # the roofline below is taken from this run; with two passes in flight the stages of two passes overlap and stretch each other
    if in_flight > 1:
        eng.reset_stats()
        t1_ = time.perf_counter()
        run_steps(args.steps, 1)
        serial_ms = 1e3 * (time.perf_counter() - t1_) / args.steps
        st = eng.stats()
    else:
        st, serial_ms = st_timed, 1e3 * elapsed / args.steps
    out["one_step_at_a_time"] = {"ms_per_step": serial_ms, "reads_per_s": args.reads / (serial_ms * 1e-3), "note": "rank 0: the same steps as blocking cs_engine_seed_batch_device calls"}

    # ---- parity gate on EVERY rank: a strided sample of this rank's batch against the oracle (the checker, never the product)
    import _oracle
    ncpu_share = max(1, len(os.sched_getaffinity(0)) // max(1, torch.cuda.device_count() if world > 1 else 1))
    cores = min(ncpu_share, 16)
    bwt_words, sa = ix.arrays()
    oidx = _oracle.OracleIndex.from_arrays(ix.view.primary, [ix.view.L2[i] for i in range(1, 5)], bwt_words, sa, 32)
    opar = _oracle.make_params(k=args.k, r=args.r, s=args.s, c=args.c, y=args.y)
    nchk = min(args.check_reads, args.reads)
    stride = max(1, args.reads // max(1, nchk))
    ids = np.arange(0, args.reads, stride, dtype=np.uint64)[:nchk]
    nchk = ids.size
    sel = (ids[:, None].astype(np.int64) * args.read_len + np.arange(args.read_len)[None, :]).reshape(-1)
    hb = bases[torch.from_numpy(sel).to(dev)].cpu().numpy()
    ho = np.arange(nchk + 1, dtype=np.uint64) * np.uint64(args.read_len)
    want = oidx.seed_batch(hb, ho, opar, mode=1, sst_batch=512, want_sal=not args.no_sal, threads=cores)
    got = eng.gather_reads(ids)
    ok = np.array_equal(got.mem_off, want["mem_off"]) and np.array_equal(got.mems, want["mems"])
    if not args.no_sal:
        ok = ok and np.array_equal(got.seed_off, want["seed_off"]) and np.array_equal(got.seeds, want["seeds"])
    all_ok = D.sum_over_ranks(0.0 if ok else 1.0) == 0.0
    # every rank's share of the read run (genome window its reads were sampled from, first / last sampled read as a checksum of the share)
    shares = D.gather_objects({"rank": rank, "device": local, "genome_window": [rank / world, (rank + 1) / world], "reads": args.reads,
                               "first_read_crc": int(np.frombuffer(hb[:args.read_len].tobytes(), dtype=np.uint8).astype(np.uint64).dot(np.arange(1, args.read_len + 1, dtype=np.uint64))),
                               "bit_exact_vs_oracle": bool(ok)})
    if not ok:
        log("PARITY FAILURE on rank %d against the oracle (strided sample of %d reads)" % (rank, nchk))

    if rank == 0:
        out["parity"] = {"checked_reads_per_rank": int(nchk), "stride": int(stride), "ranks_checked": len(shares), "bit_exact_vs_oracle": bool(all_ok),
                         "rank_shares": shares, "dist_backend": args.dist_backend}
        ws = want["stats"]
        # ---- roofline.  Stage = every launch of one pass of the SMEM collection (fwd0 / fwd / bwd_* / r2text / r3text [/ tail]);
        # its time per pass is measured live with HIP events on the engine's stream over the timed region (seed_kernel_ms).
        launches = max(1, st["seed_kernel_launches"])          # passes of the stage (1 per step unless the batch is split)
        kern_ms = st["seed_kernel_ms"] / launches
        reads_per_launch = args.reads * args.steps / launches
        # byte model of this implementation: one extra pass with the counting instantiations of the kernels (same work, same
        # results; the counts are exact and do not depend on timing)
        eng.reset_stats()
        step(ca.Params(count_traffic=1, **pk))
        tm = eng.traffic_model()
        st_c = eng.stats()
        model_bytes = tm["bytes"] * (reads_per_launch / args.reads)
        achieved = model_bytes / (kern_ms * 1e-3) / 1e9
        # the reference's algorithm on the same reads (SURVEY 8d's count: 64 B x Occ blocks of its real bwt_extend calls under the
        # 512-read SST policy + read + mems), from the oracle on the strided sample; NOT a roofline of this implementation
        ref_per_read = (64.0 * ws["bwt_blocks"] + 32.0 * ws["n_mems"]) / nchk + args.read_len
        kernels = {}
        for name, kd in tm["kernels"].items():
            kernels[name] = {"model_bytes": kd["bytes"], "events": kd["events"]}
        if traffic:
            for name, b in traffic["per_kernel_bytes"].items():
                kernels.setdefault(name, {})["fetch_size_bytes"] = b
                if traffic.get("per_kernel_ms_serialised"):
                    kernels[name]["ms_serialised"] = traffic["per_kernel_ms_serialised"].get(name)
                    kernels[name]["dispatches"] = traffic["per_kernel_dispatches"].get(name)
            for name, kd in kernels.items():
                if kd.get("fetch_size_bytes") and kd.get("ms_serialised"):
                    kd["fetch_frac_of_peak_serialised"] = kd["fetch_size_bytes"] / (kd["ms_serialised"] * 1e-3) / 1e9 / HBM_PEAK_GBS
        stage_traffic = traffic["stage_bytes"] if traffic else None
        nq = max(1, st["bwt_queries"])
        out["roofline"] = {
            "bound": "hbm", "achieved": achieved, "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS,
            "traffic": stage_traffic,
            "kernel": "SMEM stage = all fwd0 / fwd / bwd_win / bwd_win0 / bwd_wide / r2text / r3text launches of one pass (%d reads)" % int(reads_per_launch),
            "kernel_ms_per_launch": kern_ms, "launches": launches,
            "measured_with": "one step at a time (blocking calls)" if in_flight > 1 else "the timed region",
            "two_passes_in_flight": ({"stage_span_ms_per_pass": st_timed["seed_kernel_ms"] / max(1, st_timed["seed_kernel_launches"]), "ms_per_step": 1e3 * elapsed / args.steps,
                                      "model_bytes_over_step_time_frac": model_bytes / (elapsed / args.steps) / 1e9 / HBM_PEAK_GBS,
                                      "note": "the timed region: two passes overlap, so a pass's stage span is longer than alone while a step takes less; the last figure divides "
                                              "the stage's model bytes by the WHOLE step time (stage + sort + SAL)"} if in_flight > 1 else None),
            "model": "bytes the kernels request from the index-side arrays (32-B Occ records, jump entries, filter words, SA / inverse-SA "
                     "entries, text words, rep/lcp bytes, LEP entries) counted on the device + streamed queue / read / mem bytes "
                     "(cs_engine_traffic_model); a lower bound of what this implementation has to fetch",
            "model_bytes_per_launch": model_bytes, "model_bytes_per_read": model_bytes / reads_per_launch,
            "model_stream_bytes_per_launch": tm["stream_bytes"] * (reads_per_launch / args.reads),
            "traffic_GBps": (stage_traffic / (kern_ms * 1e-3) / 1e9) if stage_traffic else None,
            "traffic_frac": (stage_traffic / (kern_ms * 1e-3) / 1e9 / HBM_PEAK_GBS) if stage_traffic else None,
            "wasted_traffic_ratio": (stage_traffic / model_bytes) if stage_traffic else None,
            "traffic_source": traffic["source"] if traffic else None,
            "traffic_calibration": ({"fetch_size_bytes_per_random_32B_record_read": traffic.get("probe_fetch_bytes_per_random_record_read"),
                                     "note": "FETCH_SIZE of the bare random-record probe kernel / its record reads; the guide's x2 correction is for wide "
                                             "coalesced streams, this is the calibration for the path's own access shape; `traffic` is the raw counter"}
                                    if traffic else None),
            "kernels": kernels,
            "reference_work_GBps": ref_per_read * reads_per_launch / (kern_ms * 1e-3) / 1e9,
            "reference_bytes_per_read": ref_per_read,
            "reference_note": "SURVEY 8(d)'s bytes of the REFERENCE's algorithm over the same time: how fast the reference's work gets done, "
                              "not a fraction of the roofline (most of its bwt_extend calls are answered here without the FM index)",
            "bwt_extend_queries_per_read": st["bwt_queries"] / (args.reads * args.steps),
            "fm_index_calls_per_read": st["bwt_calls"] / (args.reads * args.steps),
            "answered_without_fm_index": 1.0 - st["bwt_calls"] / nq,
            "reference_sst_hit_rate": 1.0 - ws["bwt_calls"] / max(1, ws["bwt_queries"]),
            "reference_bwt_extend_queries_per_read": ws["bwt_queries"] / nchk,
            "round3_seeds_from_text_per_read": st["r3_text_seeds"] / (args.reads * args.steps),
            "sweeps_read_off_the_text_per_read": st["sweep_text_calls"] / (args.reads * args.steps),
            "reseed_calls_answered_from_text_per_read": st["reseed_text_calls"] / (args.reads * args.steps),
            "reseed_calls_of_unique_smems_left_to_index_per_read": st["reseed_index_calls"] / (args.reads * args.steps),
            "sal_ms_per_step": st["sal_kernel_ms"] / args.steps, "total_gpu_ms_per_step": st["total_ms"] / args.steps,
            "overflow_mems_per_step": st["overflow_mems"] / args.steps,
            "counting_pass_stage_ms": st_c["seed_kernel_ms"],
            "mems_per_read": st["mems"] / (args.reads * args.steps), "seeds_per_read": st["seeds"] / (args.reads * args.steps)}
        if args.cpu_seconds > 0:
            probe_n = min(nchk, 20000)
            tp = time.perf_counter()
            oidx.seed_batch(hb[: probe_n * args.read_len], ho[: probe_n + 1], opar, mode=1, want_sal=not args.no_sal, threads=cores)
            rate = probe_n / max(1e-6, time.perf_counter() - tp)
            ncpu = int(min(args.reads, max(probe_n, rate * args.cpu_seconds)))
            cb = bases[: ncpu * args.read_len].cpu().numpy(); co = off[: ncpu + 1].cpu().numpy().astype(np.uint64)
            tp = time.perf_counter()
            oidx.seed_batch(cb, co, opar, mode=1, sst_batch=512, want_sal=not args.no_sal, threads=cores)
            dt = time.perf_counter() - tp
            out["cpu_baseline"] = {"value": ncpu / dt, "unit": "reads/s", "cores": cores, "kind": "port",
                                   "cpu_model": cpu_model(), "nproc": os.cpu_count(), "usable_cpus": len(os.sched_getaffinity(0)),
                                   "sample": "first %d reads of rank 0's batch, oracle/cs_oracle.c in CompSeed mode (SST per 512 reads), %d threads, %.1f s"
                                             % (ncpu, cores, dt)}
            # the REAL reference where its binary travelled with the snapshot (oracle/_ref/ref_dump, compiled from /root/reference in the build
            # container; --time = its own collect_mem_with_sst / tem_forward_sst / bwt_sa on T threads, 512-read batches as kt_for hands them out)
            ref_bin = os.path.join(ROOT, "oracle", "_ref", "ref_dump")
            if os.path.exists(ref_bin) and (args.k, args.r, args.s) == (19, 1.5, 10):
                td = tempfile.mkdtemp(prefix="cs_refcpu_", dir="/tmp")
                try:
                    ix.save(os.path.join(td, "idx"))
                    with open(os.path.join(td, "reads.txt"), "wb") as f:
                        rows = cb.reshape(ncpu, args.read_len)
                        f.write(np.concatenate([rows, np.full((ncpu, 1), 10, np.uint8)], axis=1).tobytes())
                    rr = subprocess.run([ref_bin, os.path.join(td, "idx"), os.path.join(td, "reads.txt"), "/dev/null", "--time", str(cores),
                                         "-y", str(args.y), "-c", str(args.c)], capture_output=True, text=True, timeout=300)
                    rj = json.loads(rr.stdout.strip().splitlines()[-1])
                    out["cpu_baseline"].update({"port_value": out["cpu_baseline"]["value"], "value": rj["reads_per_s"], "kind": "reference",
                                                "sample": "first %d reads of rank 0's batch; the reference's own seeding + SAL code (oracle/_ref/ref_dump --time: "
                                                          "collect_mem_with_sst / tem_forward_sst / bwt_sa, SSTs per 512 reads), %d threads, %.1f s; port_value = "
                                                          "oracle/cs_oracle.c on the same sample" % (ncpu, cores, rj["seconds"])})
                    # the same on ALL usable host cores of the box ("-t = all host cores"; main.cpp:203-214 prints per-thread sums):
                    # a sample sized for ~10 s at the rate the 16-thread run predicts
                    usable, usable_src = cpu_quota()
                    out["cpu_baseline"]["host_cpus_usable"] = {"cpus": usable, "source": usable_src}
                    if usable > cores:
                        n_all = int(min(args.reads, max(ncpu, rj["reads_per_s"] * (usable / cores) * 0.6 * min(10.0, args.cpu_seconds))))
                        ca_b = bases[: n_all * args.read_len].cpu().numpy()
                        with open(os.path.join(td, "reads_all.txt"), "wb") as f:
                            f.write(np.concatenate([ca_b.reshape(n_all, args.read_len), np.full((n_all, 1), 10, np.uint8)], axis=1).tobytes())
                        del ca_b
                        ra = subprocess.run([ref_bin, os.path.join(td, "idx"), os.path.join(td, "reads_all.txt"), "/dev/null", "--time", str(usable),
                                             "-y", str(args.y), "-c", str(args.c)], capture_output=True, text=True, timeout=120)
                        rja = json.loads(ra.stdout.strip().splitlines()[-1])
                        out["cpu_baseline"]["all_cores"] = {"value": rja["reads_per_s"], "unit": "reads/s", "cores": usable, "kind": "reference",
                                                            "sample": "first %d reads of rank 0's batch, ref_dump --time %d, %.1f s" % (n_all, usable, rja["seconds"])}
                except Exception as ex:  # noqa: BLE001
                    log("reference CPU baseline not available: %r" % (ex,))
                finally:
                    shutil.rmtree(td, ignore_errors=True)
            del cb, co
        if not args.no_host_io:  # the boundary's host-buffer forms (SURVEY 8d's metric includes H2D of reads and D2H of results)
            hb_pin = ca.pinned_array(n_bases)                # the chunk an integration reads its input into (cs_host_alloc)
            hb_pin[:] = bases.cpu().numpy()
            ho_all = off.cpu().numpy().astype(np.uint64)
            reps = 3

            def timed(fn):
                fn(); fn(); fn(); fn()                        # warm-up: the four pinned result slots / the host buffers are sized on first use
                tp = time.perf_counter()
                for _ in range(reps):
                    r_ = fn()
                return (time.perf_counter() - tp) / reps, r_
            dt_x, rx = timed(lambda: eng.seed_batch(hb_pin, ho_all, par, copy=False))
            dt_p, rp = timed(lambda: eng.seed_batch_packed(hb_pin, ho_all, par))
            # both against the oracle on the same strided sample (expanded form directly, packed form through the unpacker)
            sel_m = np.concatenate([np.arange(int(rx.mem_off[i]), int(rx.mem_off[i + 1])) for i in ids.astype(np.int64)]) if nchk else np.zeros(0, np.int64)
            ok_x = np.array_equal(rx.mems[sel_m], want["mems"])
            if not args.no_sal:
                sel_s = np.concatenate([np.arange(int(rx.seed_off[i]), int(rx.seed_off[i + 1])) for i in ids.astype(np.int64)])
                ok_x = ok_x and np.array_equal(rx.seeds[sel_s], want["seeds"])
            pm = rp["mems"][sel_m]
            ok_p = np.array_equal(ca.unpack_mems16(pm) if rp["mem_format"] == 1 else pm, want["mems"])
            if not args.no_sal:
                ok_p = ok_p and np.array_equal(ca.packed_rbeg(rp, sel_s), want["seeds"]["rbeg"])
            # a stream of batches, three in flight (cs_engine_submit / cs_engine_collect_packed): upload of batch n+1, seeding of batch n
            # and download of batch n-1 overlap -- how the reference drives this stage (kt_pipeline, main.cpp:438)
            # steady state of a long stream: 20 batches go through, three kept in flight from the first to the last; the clock runs from the
            # completion of the 7th to the completion of the 17th (10 batches) -- the pipeline is full before, during and after the timed window
            # (filling it takes three batches, and a batch submitted to an idle engine is cut into parts: neither belongs to the rate)
            n_total, first, nstream = 20, 6, 10
            depth = 3                                        # (the engine takes four; with one more the uploads run beside more of the downloads and both get slower)
            for _ in range(depth):
                eng.submit(hb_pin, ho_all, par)
            for i in range(n_total):
                rs_ = eng.collect_packed()
                if i == first:
                    tp = time.perf_counter()
                if i == first + nstream:
                    dt_s = (time.perf_counter() - tp) / nstream
                if i + depth < n_total:
                    eng.submit(hb_pin, ho_all, par)
            while True:
                try:
                    rs_ = eng.collect_packed()
                except ca.CSError:
                    break
            pm = rs_["mems"][sel_m]
            ok_s = np.array_equal(ca.unpack_mems16(pm) if rs_["mem_format"] == 1 else pm, want["mems"])
            if not args.no_sal:
                ok_s = ok_s and np.array_equal(ca.packed_rbeg(rs_, sel_s), want["seeds"]["rbeg"])
            ok_p = ok_p and ok_s
            hb_page = np.array(hb_pin)                        # the same from pageable memory (staged by the upload thread)
            dt_g, _ = timed(lambda: eng.seed_batch(hb_page, ho_all, par, copy=False))
            out["pcie_inclusive"] = {
                "reads_per_s": args.reads / dt_x, "ms_per_step": 1e3 * dt_x,
                "packed_reads_per_s": args.reads / dt_p, "packed_ms_per_step": 1e3 * dt_p,
                "pipelined_packed_reads_per_s": args.reads / dt_s, "pipelined_packed_ms_per_batch": 1e3 * dt_s,
                "pageable_input_reads_per_s": args.reads / dt_g,
                "bit_exact_vs_oracle": bool(ok_x and ok_p), "packed_bytes_per_read": (rp["mems"].nbytes + (rp["seed_rbeg_lo"].nbytes + rp["seed_rbeg_hi"].nbytes if not args.no_sal else 0) + 16 * args.reads) / args.reads,
                "sub_batch_reads": int(eng.options.pipeline_reads), "expand_threads": int(eng.options.expand_threads), "host_pack_threads": int(eng.options.host_pack_threads),
                "note": "rank 0, whole call: reads_per_s = cs_engine_seed_batch (reads from pinned host memory in, cs_intv_t / cs_seed_t arrays in host memory "
                        "out: upload, seeding, download and the host-side expansion of the packed results overlapped over sub-batches); packed_reads_per_s = "
                        "cs_engine_seed_batch_packed (the 16-byte / 8-byte form a consumer unpacks while it copies per read anyway); pipelined_packed_reads_per_s "
                        "= a stream of such batches with three in flight (cs_engine_submit / cs_engine_collect_packed), per batch; never `value`"}
            # SURVEY 8(d) defines the metric "incl. H2D/D2H of reads/results": these are the conforming figures, under a key that says so
            # (`value` is the device-resident rate the bench contract asks for)
            out["reads_per_s_incl_pcie"] = {"pipelined_three_batches_in_flight": args.reads / dt_s, "one_blocking_call_packed": args.reads / dt_p,
                                            "one_blocking_call_expanded": args.reads / dt_x, "bit_exact_vs_oracle": bool(ok_x and ok_p)}
            if not (ok_x and ok_p):
                all_ok = False
            del hb_pin, ho_all, hb_page
        if not all_ok:
            out["value"] = None
            out["error"] = "results differ from the oracle: the throughput above is void"
    if args.ingest_rank0:
        # ---- the north_star's data movement, timed on its own (never `value`): rank 0 owns the chunk (it is the ingest rank: it read the
        # file), contiguous read ranges go out over RCCL, every rank seeds its range on its resident replica, mems and seeds come back
        big = None
        if rank == 0:
            parts = [bases] + [torch.empty_like(bases) for _ in range(world - 1)]
            for g in range(1, world):
                parts[g].copy_(bases)                 # (the same reads again: the payload size is what matters here)
            big_b = torch.cat(parts); del parts
            big_o = torch.arange(args.reads * world + 1, dtype=torch.int64, device=dev) * args.read_len
            big = (big_b, big_o)
        D.barrier(); t_a = time.perf_counter()
        mb, mo = coll.scatter_reads(big[0] if big else None, big[1] if big else None)
        if args.dist_backend != "nccl":   # gloo moved CPU tensors: this rank's range goes back to its GPU
            mb, mo = mb.to(dev), mo.to(dev)
        torch.cuda.synchronize(); D.barrier(); t_b = time.perf_counter()
        r2 = eng.seed_batch_device(mb.data_ptr(), mo.data_ptr(), mo.numel() - 1, mb.numel(), par)
        D.barrier(); t_c = time.perf_counter()
        v64 = lambda ptr, nbytes: device_tensor_view(ptr, nbytes, dev).view(torch.int64).to(cdev)   # (no copy under nccl)
        sal_on = not args.no_sal
        g_ = coll.gather_results(v64(r2.ptr["mem_off"], (r2.n_reads + 1) * 8), v64(r2.ptr["mems"], r2.n_mems * 32),
                               v64(r2.ptr["seed_off"], (r2.n_reads + 1) * 8) if sal_on else None, v64(r2.ptr["seeds"], r2.n_seeds * 16) if sal_on else None)
        torch.cuda.synchronize(); D.barrier(); t_d = time.perf_counter()
        if rank == 0:
            tot = args.reads * world
            ok_g = int(g_["mem_off"][-1]) * 4 == g_["mems"].numel() and g_["mem_off"].numel() == tot + 1
            # rank 0's own share must come back unchanged at the front of the gathered arrays
            ok_g = ok_g and bool(torch.equal(g_["mems"][: r2.n_mems * 4], v64(r2.ptr["mems"], r2.n_mems * 32)))
            # ... and every other rank's share is the same reads again, so its mems must equal rank 0's (positions and all)
            for g in range(1, world):
                m0, m1 = int(g_["mem_off"][g * args.reads]), int(g_["mem_off"][(g + 1) * args.reads])
                ok_g = ok_g and (m1 - m0) == r2.n_mems and bool(torch.equal(g_["mems"][m0 * 4: m1 * 4], g_["mems"][: r2.n_mems * 4]))
            out_ing = {"reads": tot, "reads_per_s": tot / (t_d - t_a), "scatter_ms": 1e3 * (t_b - t_a), "seed_ms": 1e3 * (t_c - t_b), "gather_ms": 1e3 * (t_d - t_c),
                       "scatter_bytes": int(big[0].numel() + big[1].numel() * 8), "gather_bytes": int(sum(t.numel() for t in g_.values() if t is not None) * 8),
                       "consistent": bool(ok_g),
                       "note": "rank 0 holds the chunk; two-phase scatter of read ranges, seeding of every range on its rank, two-phase gather of mems and seeds "
                               "to rank 0, all over torch.distributed / RCCL, nothing overlapped"}
            out["ingest_rank0"] = out_ing
        del big, g_
    oidx.close()
    eng.close(); ix.close()
    side = [w for w in args.side_workloads.split(",") if w and w != args.profile]
    if rank == 0 and world == 1 and side and not args.side_child and not args.pmc_child:
        # ---- the same measurement on other workload profiles (tools/synth.py), outside the headline: a child run of this script per
        # profile once this process has given its HBM back (index + derived arrays are ~140 GB per engine).  Same parity gate.
        del bases, off
        torch.cuda.empty_cache()
        out["workloads"] = {}
        for w in side:
            cmd = [sys.executable, os.path.abspath(__file__), "--side-child", "--full", "--profile", w, "--steps", "3", "--warmup", "1", "--traffic", "none",
                   "--cpu-seconds", "0", "--no-host-io", "--no-extension", "--genome-mbp", str(args.genome_mbp), "--reads", str(args.reads), "--read-len", str(args.read_len),
                   "--check-reads", str(args.check_reads), "-k", str(args.k), "-r", str(args.r), "-y", str(args.y), "-c", str(args.c), "-s", str(args.s)]
            if args.lib:
                cmd += ["--lib", args.lib]
            for o in args.opt:
                cmd += ["--opt", o]
            try:
                rr = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
                cj = json.loads(rr.stdout.strip().splitlines()[-1])
                out["workloads"][w] = {"reads_per_s": cj["value"], "ms_per_step": cj["ms_per_step"], "stage_ms": cj["roofline"]["kernel_ms_per_launch"],
                                       "parity": cj["parity"]["bit_exact_vs_oracle"], "checked_reads": cj["parity"]["checked_reads_per_rank"],
                                       "model_bytes_per_read": cj["roofline"]["model_bytes_per_read"], "roofline_frac": cj["roofline"]["frac"],
                                       "answered_without_fm_index": cj["roofline"]["answered_without_fm_index"], "workload": cj["config"]["workload"]}
                if not cj["parity"]["bit_exact_vs_oracle"]:
                    all_ok = False
                    out["value"] = None
                    out["error"] = "workload %s: results differ from the oracle" % w
            except Exception as ex:  # noqa: BLE001
                log("side workload %s failed: %r" % (w, ex))
                out["workloads"][w] = {"error": repr(ex)[:300]}
    # (the extension measurements come after the side workloads: what they leave allocated in this process cost the children's engines an
    # optional array -- repeat50 ran at 139 instead of 110 ms per stage)
    if rank == 0 and world == 1 and not args.side_child and not args.pmc_child and not args.no_extension:
        # ---- SURVEY 8f row 4, the stage behind seeding + chaining: banded Smith-Waterman seed extension on the GPU (tools/extend_bench.py);
        # integer-compute-bound, so pairs/s and DP cells/s, not a fraction of HBM bandwidth; never part of `value`
        try:
            import extend_bench
            out["extension"] = extend_bench.run(cpu_threads=min(16, cpu_quota()[0]), device=local)
            if not out["extension"]["bit_exact_vs_oracle"]:
                all_ok = False
                out["value"] = None
                out["error"] = "extension kernel: results differ from the oracle"
        except Exception as ex:  # noqa: BLE001
            log("extension side measurement failed: %r" % (ex,))
            out["extension"] = {"error": repr(ex)[:300]}
        # ... and the stages behind seeding as a whole (tools/align_bench.py): 1 M reads against a synthetic 200 Mbp genome indexed from FASTA
        # on the GPU, through cs_chain_batch -> cs_chain_filter -> cs_extend_chains -> cs_dedup_regions; wall time per library call
        try:
            import align_bench
            torch.cuda.empty_cache()
            out["extension"]["stage"] = align_bench.run(1000000, 200.0)
        except Exception as ex:  # noqa: BLE001
            log("alignment stage side measurement failed: %r" % (ex,))
            if isinstance(out.get("extension"), dict):
                out["extension"]["stage"] = {"error": repr(ex)[:300]}
    if rank == 0:
        print(json.dumps(out), flush=True)   # the ONE line
    D.close()
    return 0 if all_ok else 1


if __name__ == "__main__":
    sys.exit(main())
