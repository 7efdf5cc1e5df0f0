"""tools/sa_width_bench.py -- what 40-bit suffix-array / inverse-SA entries (engine option sa40) cost or give against 8-byte entries, on the
same index and the same batch: the index is built once, then an 8-byte engine and a 40-bit engine are created ONE AFTER THE OTHER on it (two
hg19-size engines do not fit side by side), alternating for `--repeats` rounds.  Per engine: ms per step of cs_engine_seed_batch_device (one
batch at a time) and of the stream with two batches in flight (cs_engine_submit_device / collect_device), each a host clock around `--steps`
steps that end in the call's own device synchronise, after one warm-up step of each kind; the result digests, which must be equal; memory().
--widths 8 or --widths 40 runs one width only: what a `rocprofv3 --kernel-trace --stats` run wants (per-kernel times of one engine).
usage: sa_width_bench.py [genome_mbp] [reads] [--steps K] [--repeats R] [--widths 8,40] [--out FILE]"""
import argparse, json, os, statistics, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np, torch
import compseed_amd as ca, synth

ap = argparse.ArgumentParser()
ap.add_argument("genome_mbp", nargs="?", type=float, default=3100)
ap.add_argument("reads", nargs="?", type=int, default=10_000_000)
ap.add_argument("--steps", type=int, default=4, help="timed steps per measurement")
ap.add_argument("--repeats", type=int, default=3, help="rounds; every round creates, times and destroys one engine of each width")
ap.add_argument("--widths", default="8,40", help="entry widths to run: 8, 40 or both")
ap.add_argument("--out", default="", help="also write the JSON here")
a = ap.parse_args()
n = a.reads
G = synth.make_genome(int(a.genome_mbp * 1e6), seed=20261003, device="cuda")
ix = ca.Index.build(G.cpu().numpy(), 0)
bases, off = synth.make_reads(G, n, 150, seed=777, p_sub=0.005, sort=True)
del G; torch.cuda.empty_cache()
par = ca.Params()
args = (bases.data_ptr(), off.data_ptr(), n, bases.numel(), par)
MODES = [m for m in (("8-byte", dict(sa64=1)), ("40-bit", dict(sa40=1))) if m[0].split("-")[0] in a.widths.split(",")]
assert MODES, "--widths: 8, 40 or 8,40"
runs = {name: [] for name, _ in MODES}
for rnd in range(a.repeats):
    for name, opt in MODES:
        t0 = time.perf_counter()
        e = ca.Engine(ix, 0, **opt)
        t_create = time.perf_counter() - t0
        e.seed_batch_device(*args)                                   # warm-up: buffers sized, code objects loaded
        digest = e.result_digest()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.steps):
            e.seed_batch_device(*args)
        one = (time.perf_counter() - t0) / a.steps
        e.submit_device(*args); e.submit_device(*args); e.collect_device(); e.collect_device()      # warm-up: the second pass context
        t0 = time.perf_counter()
        e.submit_device(*args)
        for _ in range(a.steps - 1):
            e.submit_device(*args); e.collect_device()
        e.collect_device()
        two = (time.perf_counter() - t0) / a.steps
        digest2 = e.result_digest()
        m = e.memory()
        e.close()
        r = dict(round=rnd, ms_per_step=one * 1e3, ms_per_step_two_in_flight=two * 1e3, engine_create_s=t_create, digest=[int(x) for x in digest],
                 digest_stream=[int(x) for x in digest2], memory=m)
        runs[name].append(r)
        print(name, json.dumps(r), flush=True)
out = {"genome_mbp": a.genome_mbp, "reads": n, "read_len": 150, "steps": a.steps, "repeats": a.repeats, "rows": int(ix.view.seq_len) + 1}
for name, rs in runs.items():
    one = [r["ms_per_step"] for r in rs]; two = [r["ms_per_step_two_in_flight"] for r in rs]
    out[name] = {"ms_per_step": {"median": statistics.median(one), "min": min(one), "max": max(one), "all": one},
                 "ms_per_step_two_in_flight": {"median": statistics.median(two), "min": min(two), "max": max(two), "all": two},
                 "digest": rs[0]["digest"], "memory": rs[-1]["memory"], "engine_create_s": [r["engine_create_s"] for r in rs]}
digests = {tuple(r[k]) for rs in runs.values() for r in rs for k in ("digest", "digest_stream")}
out["equal_digests"] = len(digests) == 1
if len(MODES) == 2:
    out["saved_bytes"] = out["8-byte"]["memory"]["total"] - out["40-bit"]["memory"]["total"]
print(json.dumps(out))
if a.out:
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
assert out["equal_digests"], "the 8-byte and the 40-bit engine gave different results"
ix.close()
