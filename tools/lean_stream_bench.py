"""tools/lean_stream_bench.py -- what CS_RESULT_LEAN buys at bench scale, flags 0 against LEAN in alternating rounds on one engine:
  (a) the host stream (cs_engine_submit / cs_engine_collect_packed, four batches in flight): ms per batch, downloaded bytes per read
  (b) device-resident steps (cs_engine_submit_device / cs_engine_collect_device, two in flight): ms per step
The workload is bench.py's default one, made by the same generators with the same seeds (tools/synth.py).  Before anything is timed the
two forms are compared: mem_off and both seed planes of the packed results byte for byte, the device digests of offsets and seeds equal,
and -- on the first --check-reads reads -- the lean digests equal whatever shortcut is switched off (and under sst_mode 0).
usage: lean_stream_bench.py [--genome-mbp 3100] [--reads 10000000] [--rounds 3] [--batches 24] [--steps 20] [--out profiles/lean_results_bench.json]"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np
import torch
import compseed_amd as ca
import synth

DISABLES = [(), ("r3_text",), ("text_mode", "r2_text", "text_sweep", "r3_text"), ("fused_sal",), ("mem_pos",), ("window",)]   # tests/test_gpu_lean_results.py, test 5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--genome-mbp", type=float, default=3100)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--read-len", type=int, default=150)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--batches", type=int, default=24, help="batches per stream measurement; the middle half is timed")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--check-reads", type=int, default=200_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lean_results_bench.json"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("lean_stream_bench.py needs a GPU")
    dev = torch.device("cuda", 0)
    prof = synth.PROFILES["default"]
    torch.use_deterministic_algorithms(True)                                  # as bench.py: the same inputs in every run
    G = synth.make_genome(int(args.genome_mbp * 1e6), seed=20261003, device=dev, **prof["genome"])
    torch.use_deterministic_algorithms(False)
    ix = ca.Index.build(G.cpu().numpy(), 0)
    torch.use_deterministic_algorithms(True)
    bases, off = synth.make_reads(G, args.reads, args.read_len, seed=777, lo_frac=0.0, hi_frac=1.0, **prof["reads"])
    torch.use_deterministic_algorithms(False)
    del G; torch.cuda.empty_cache()
    n, nb = args.reads, bases.numel()
    pin = ca.pinned_array(nb); pin[:] = bases.cpu().numpy(); ho = off.cpu().numpy().astype(np.uint64)
    eng = ca.Engine(ix, 0)
    PAR = {"full": ca.Params(), "lean": ca.Params(result_flags=ca.RESULT_LEAN)}

    # ---- the two forms hold the same result
    keep, bytes_per_read = {}, {}
    for name, par in PAR.items():
        p = eng.seed_batch_packed(pin, ho, par)
        m = p["mems"]
        if p["mem_format"] == ca.MEM_PACKED16:                                # x2 | beg << 34 | end << 49 of every mem: what the 8-byte form holds
            w0, w1 = m["w0"], m["w1"]
            words = ((w0 >> np.uint64(33)) | ((w1 >> np.uint64(63)) << np.uint64(31))) | (((w1 >> np.uint64(33)) & np.uint64(0x7fff)) << np.uint64(34)) | (((w1 >> np.uint64(48)) & np.uint64(0x7fff)) << np.uint64(49))
        else:
            words = m["w"].copy()
        keep[name] = dict(fmt=p["mem_format"], mem_off=p["mem_off"].copy(), seed_off=p["seed_off"].copy(), lo=p["seed_rbeg_lo"].copy(), hi=p["seed_rbeg_hi"].copy(), x2info=words)
        bytes_per_read[name] = (2 * 8 * (n + 1) + p["mems"].nbytes + 5 * p["n_seeds"]) / n
    assert keep["full"]["fmt"] == ca.MEM_PACKED16 and keep["lean"]["fmt"] == ca.MEM_LEAN8
    for k in ("mem_off", "seed_off", "lo", "hi", "x2info"):
        assert keep["full"][k].tobytes() == keep["lean"][k].tobytes(), k
    del keep
    dig = {}
    for name, par in PAR.items():
        eng.seed_batch_device(bases.data_ptr(), off.data_ptr(), n, nb, par)
        dig[name] = eng.result_digest()
    assert (dig["full"][0], dig["full"][2], dig["full"][3]) == (dig["lean"][0], dig["lean"][2], dig["lean"][3]) and dig["full"][1] != dig["lean"][1]
    nc = min(args.check_reads, n); ncb = int(ho[nc])
    sub = []
    for kw in [dict(disable=ca.disable_mask(*d)) for d in DISABLES] + [dict(sst_mode=0)]:
        eng.seed_batch_device(bases.data_ptr(), off.data_ptr(), nc, ncb, ca.Params(result_flags=ca.RESULT_LEAN, **kw))
        sub.append(eng.result_digest())
    assert all(d == sub[0] for d in sub), sub
    print("checked: packed offsets / seed planes / x2 / info equal; device digests equal; %d lean digests over %d reads equal" % (len(sub), nc), flush=True)

    # ---- the measurements
    def stream(par):
        depth, total = 4, args.batches
        for _ in range(depth):
            eng.submit(pin, ho, par)
        tt = []
        for i in range(total):
            eng.collect_packed(); tt.append(time.perf_counter())
            if i + depth < total:
                eng.submit(pin, ho, par)
        a, b = total // 3, total - total // 6 - 1
        return 1e3 * (tt[b] - tt[a]) / (b - a)

    def device_steps(par):
        k = args.steps
        eng.submit_device(bases.data_ptr(), off.data_ptr(), n, nb, par); eng.submit_device(bases.data_ptr(), off.data_ptr(), n, nb, par)
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for i in range(k):
            eng.collect_device()
            if i + 2 < k:
                eng.submit_device(bases.data_ptr(), off.data_ptr(), n, nb, par)
        torch.cuda.synchronize()
        return 1e3 * (time.perf_counter() - t0) / k

    for par in PAR.values():                                                   # buffers of both element sizes, both pass contexts
        for _ in range(3):
            eng.seed_batch_packed(pin, ho, par)
    runs = []
    for rnd in range(args.rounds):
        for name, par in PAR.items():
            s_ms = stream(par)
            runs.append(dict(round=rnd + 1, flags=name, part="stream", ms_per_batch=s_ms)); print(runs[-1], flush=True)
    for par in PAR.values():
        device_steps(par)
    for rnd in range(args.rounds):
        for name, par in PAR.items():
            d_ms = device_steps(par)
            runs.append(dict(round=rnd + 1, flags=name, part="device", ms_per_step=d_ms)); print(runs[-1], flush=True)
    eng.reset_stats()
    kern = {}
    for name, par in PAR.items():                                              # r3text_kernel's inverse-SA requests, one counting pass each
        eng.reset_stats()
        eng.seed_batch_device(bases.data_ptr(), off.data_ptr(), n, nb, ca.Params(count_traffic=1, result_flags=par.result_flags))
        kern[name] = eng.traffic_model()["kernels"]["r3text_kernel"]["events"]

    def summary(part, key):
        out = {}
        for name in PAR:
            v = [r[key] for r in runs if r["part"] == part and r["flags"] == name]
            out[name] = dict(median=statistics.median(v), min=min(v), max=max(v), spread=max(v) - min(v))
        out["lean_minus_full_median"] = out["lean"]["median"] - out["full"]["median"]
        return out

    res = dict(what="flags 0 (full) against CS_RESULT_LEAN on one MI355X, one engine, alternating, %d rounds; bench.py's default workload" % args.rounds,
               command="python tools/lean_stream_bench.py --genome-mbp %g --reads %d --rounds %d --batches %d --steps %d" % (args.genome_mbp, n, args.rounds, args.batches, args.steps),
               reads=n, read_len=args.read_len, genome_mbp=args.genome_mbp, downloaded_bytes_per_read=bytes_per_read,
               stream_ms_per_batch=summary("stream", "ms_per_batch"), device_ms_per_step=summary("device", "ms_per_step"),
               r3text_events=kern, runs=runs)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    json.dump(res, open(args.out, "w"), indent=1)
    print(json.dumps({k: res[k] for k in ("downloaded_bytes_per_read", "stream_ms_per_batch", "device_ms_per_step", "r3text_events")}), flush=True)
    eng.close(); ix.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
