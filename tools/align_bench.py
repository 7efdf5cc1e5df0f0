"""tools/align_bench.py -- the stages behind seeding at a size where their speed shows: N reads of 150 bases sampled from the golden
reference (tests/golden/g1, 220 kbp: every read has a true locus, many have repeats) with substitutions and short indels, through
GPU seeding -> cs_chain_batch -> cs_chain_filter -> cs_extend_chains -> cs_dedup_regions; wall time and reads/s per stage.  Beside the host
chain row: the device chainer on the same reads, cs_chain_batch_gpu (host arrays) and cs_chain_batch_device (on a second, device-resident
seeding of the batch), both checked equal to the host chains over the whole batch.  Beside the host chain_filter row: the device filter,
cs_chain_filter_device (fed by the device chain call's result) and cs_chain_filter_gpu (host arrays), both checked equal to the host filter.
Beside the host extend_chains row: cs_extend_chains_device on the device filter's result, with every region kept and with the purged ones
left behind (CS_ALN_DEV_COMPACT), each with the time download_regions takes; checked equal to the host call's regions / its regions with qe > qb.
Behind dedup_regions: "regions -> CIGAR", cs_regions_cigar over the de-duplicated regions (host arrays in and out), wall time as ms per million
reads, with the device span and the job counts of cs_cigar_stats; nothing in the reference is timed separately to compare it with.
Behind that: "regions -> marks", cs_regions_mark over the de-duplicated regions in default mode and under CS_MARK_ALL, and cs_regions_cigar
three ways -- over the marks' cigar_regs in either mode, and over all regions as a caller without marks has to -- each as the median, the
minimum and the maximum of seven calls after a warm-up one, ms per million reads.  Behind that, per mode: "marks + CIGAR -> SAM text",
cs_regions_sam over those marks and their alignments, timed the same way, with the device span, the bytes per read and the counts of
cs_sam_stats.  Last: "reads -> SAM text (cs_map_batch)", the whole path as one call of a Mapper of its own on the same reads -- reads/s over the
median of three calls after a warm-up one, the mapper's per-step host wall time per call, and beside them the sum of this run's separate rows of
the same steps (device seeding, device chaining, device filter, compacting extension and its download, dedup_regions, marks, marked CIGAR and
SAM text in default mode); the text is checked equal to the separate stages' text.  Beside it: "reads -> SAM text (cs_map_submit / collect)", the
same batch as a stream on the same mapper with 1, 2 and 3 batches kept in flight, ms per batch and the per-step times; every text checked equal to cs_map_batch's.
usage: align_bench.py [reads] [--synth-mbp M]"""
import gzip, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import compseed_amd as ca
import _data

import argparse, tempfile, shutil


def run(n=200000, synth_mbp=0.0):
    L = 150
    tmpdir = None
    if synth_mbp > 0:
        import torch
        sys.path.insert(0, os.path.join(ROOT, "tools"))
        import synth
        G = synth.make_genome(int(synth_mbp * 1e6), seed=20261003, device="cuda")
        rd, ro = synth.make_reads(G, n, L, seed=99, p_sub=0.005, p_indel=0.001, sort=True)
        bases = rd.cpu().numpy(); off = ro.cpu().numpy().astype(np.uint64)
        g = np.frombuffer(b"ACGT", dtype=np.uint8)[G.cpu().numpy()]
        del G, rd, ro; torch.cuda.empty_cache()
        tmpdir = tempfile.mkdtemp(prefix="csaln_")
        fa = os.path.join(tmpdir, "g.fa")
        with open(fa, "wb") as f:
            nctg = 8; per = (g.size + nctg - 1) // nctg
            for k in range(nctg):
                f.write(b">chr%d\n" % (k + 1)); f.write(g[k * per:(k + 1) * per].tobytes()); f.write(b"\n")
        del g
        PREFIX = os.path.join(tmpdir, "g")
        t0 = time.perf_counter(); ca.build_index_from_fasta(fa, PREFIX, 0); t_build = time.perf_counter() - t0
        os.remove(fa)
    else:
        PREFIX = _data.PREFIX
        fa = gzip.open(os.path.join(_data.GOLD, "ref.fa.gz")).read().decode().split(">")[1:]
        contigs = [np.frombuffer("".join(c.split("\n")[1:]).upper().replace("N", "A").encode(), dtype=np.uint8) for c in fa]
        rng = np.random.default_rng(3)
        ci = rng.integers(0, len(contigs), n)
        reads = np.empty((n, L), dtype=np.uint8)
        for k, c in enumerate(contigs):
            sel = np.nonzero(ci == k)[0]
            p = rng.integers(0, c.size - L - 8, sel.size)
            reads[sel] = c[p[:, None] + np.arange(L)[None, :]]
        mut = rng.random((n, L)) < 0.01
        reads[mut] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(mut.sum()))]
        # a 1-2-base deletion in one read of four (the tail shifts left, the end is refilled with random bases)
        for r in np.nonzero(rng.random(n) < 0.25)[0][:50000]:
            at = int(rng.integers(40, 110)); k = int(rng.integers(1, 3))
            reads[r, at:L - k] = reads[r, at + k:]
            reads[r, L - k:] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, k)]
        rc = rng.random(n) < 0.5
        comp = np.zeros(256, np.uint8); comp[list(b"ACGT")] = list(b"TGCA")
        reads[rc] = comp[reads[rc]][:, ::-1]
        bases = np.ascontiguousarray(reads.reshape(-1)); off = (np.arange(n + 1, dtype=np.uint64) * np.uint64(L))
    ix = ca.Index.load(PREFIX); eng = ca.Engine(ix, 0); ch = ca.Chainer(PREFIX); al = ca.Aligner(PREFIX, 0)
    chd = ca.Chainer(PREFIX, device=0)   # the device chainer (cs_chain_batch_device / cs_chain_batch_gpu)
    ald = ca.Aligner(PREFIX, 0)          # the aligner of the device rows (cs_extend_chains_device), buffers of its own
    d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
    eng.upload(d_b, bases); eng.upload(d_o, off); eng.sync()
    out = {"reads": n, "reference": ("synthetic %g Mbp" % synth_mbp) if synth_mbp > 0 else "tests/golden/g1 (220 kbp, tandem arrays)"}
    def same(a, b, keys=("chain_off", "chains", "cseed_off", "cseeds")):
        return all(np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes() for k in keys)
    FK = ("chain_off", "chains", "cseed_off", "cseeds", "cseed_score")
    for rep in range(2):   # the second round is the measured one (buffers sized)
        t0 = time.perf_counter(); res = eng.seed_batch(bases, off, ca.Params(), copy=False); t1 = time.perf_counter()
        c = ch.chain(res.mem_off, res.mems, res.seed_off, res.seeds, off, ca.ChainParams(), threads=16, copy=False); t2 = time.perf_counter()
        f = ch.filter(c["chain_off"], c["chains"], c["cseed_off"], c["cseeds"], bases, off, threads=16, copy=False); t3 = time.perf_counter()
        st0 = al.stats()
        g = al.extend_chains(f["chain_off"], f["chains"], f["cseed_off"], f["cseeds"], bases, off, cseed_score=f["cseed_score"], copy=False); t4 = time.perf_counter()
        st1 = al.stats()
        d = al.dedup_regions(g["reg_off"], g["regs"], bases, off, copy=False); t5 = time.perf_counter()
        cs0 = al.cigar_stats(); tc0 = time.perf_counter(); cg_res = al.regions_cigar(d["reg_off"], d["regs"], bases, off); tc1 = time.perf_counter(); cs1 = al.cigar_stats()
        # the chain pass on the GPU: host arrays in and out (PCIe both ways), then from the engine's device result (seeded once more)
        t6 = time.perf_counter(); cg = chd.chain_gpu(res.mem_off, res.mems, res.seed_off, res.seeds, off, ca.ChainParams(), copy=False); t7 = time.perf_counter()
        assert same(cg, c), "cs_chain_batch_gpu differs from cs_chain_batch"
        tsd0 = time.perf_counter(); rd = eng.seed_batch_device(d_b, d_o, n, bases.size, ca.Params()); tsd1 = time.perf_counter()
        sd0 = chd.stats(); t8 = time.perf_counter(); dd = chd.chain_device(rd, d_o, ca.ChainParams()); t9 = time.perf_counter(); sd1 = chd.stats()
        assert same(ca.download_chains(eng, dd), c), "cs_chain_batch_device differs from cs_chain_batch"
        # the chain filter on the GPU: from the device chain call's result, then host arrays in and out
        fs0 = chd.filter_stats(); t10 = time.perf_counter(); fd = chd.filter_device(dd, d_b, d_o); t11 = time.perf_counter(); fs1 = chd.filter_stats()
        assert same(ca.download_chains(eng, fd), f, FK), "cs_chain_filter_device differs from cs_chain_filter"
        # the extension stage on the device filter's result (before filter_gpu reuses its buffers): all regions, then the live ones only
        xs0 = ald.stats(); t14 = time.perf_counter(); xd = ald.extend_chains_device(fd, d_b, d_o); t15 = time.perf_counter(); xs1 = ald.stats()
        xr = ca.download_regions(eng, xd); t16 = time.perf_counter()
        assert same(xr, g, ("reg_off", "regs")), "cs_extend_chains_device differs from cs_extend_chains"
        t17 = time.perf_counter(); xc = ald.extend_chains_device(fd, d_b, d_o, flags=ca.ALN_DEV_COMPACT); t18 = time.perf_counter()
        xcr = ca.download_regions(eng, xc); t19 = time.perf_counter()
        hr = np.asarray(g["regs"]); live = hr["qe"] > hr["qb"]
        live_off = np.concatenate(([0], np.cumsum(live))).astype(np.uint64)[np.asarray(g["reg_off"]).astype(np.int64)]
        assert xc["n_regs"] == int(live.sum()) and same(xcr, {"reg_off": live_off, "regs": hr[live]}, ("reg_off", "regs")), "the compacted regions differ from cs_extend_chains' regions with qe > qb"
        t12 = time.perf_counter(); fg = chd.filter_gpu(c["chain_off"], c["chains"], c["cseed_off"], c["cseeds"], bases, off, copy=False); t13 = time.perf_counter()
        assert same(fg, f, FK), "cs_chain_filter_gpu differs from cs_chain_filter"
    # marking, MAPQ and line selection (cs_regions_mark), and the CIGAR stage three ways: over cigar_regs in default mode and under
    # CS_MARK_ALL, and over all de-duplicated regions, which is what a caller without marks has to do.  One warm-up call each, then
    # MARK_RUNS timed calls: median, min and max wall time as ms per million reads
    MARK_RUNS = 7
    def timed(fn):
        fn()
        ts = []
        for _ in range(MARK_RUNS):
            ta = time.perf_counter(); r = fn(); ts.append((time.perf_counter() - ta) * 1e3 * 1e6 / n)
        return r, {"runs": MARK_RUNS, "median_ms_per_million_reads": float(np.median(ts)), "min": min(ts), "max": max(ts)}
    d_off, d_regs = np.array(d["reg_off"]), np.array(d["regs"])
    name_list = [b"%d" % (k + 1) for k in range(n)]
    name_off = np.zeros(n + 1, np.uint64); name_off[1:] = np.cumsum([len(x) for x in name_list])
    names = (np.frombuffer(b"".join(name_list), np.uint8), name_off)
    for label, mflags in (("default", 0), ("CS_MARK_ALL", ca.MARK_ALL)):
        ms0 = al.mark_stats(); mk, tm = timed(lambda: al.regions_mark(d_off, d_regs, off, flags=mflags)); ms1 = al.mark_stats()
        _, tcg = timed(lambda: al.regions_cigar(mk["cigar_reg_off"], mk["cigar_regs"], bases, off))
        md = {k: (ms1[k] - ms0[k]) / (MARK_RUNS + 1) for k in ms1}
        out["regions -> marks (%s)" % label] = dict(tm, device_span_ms=md["kernel_ms"], regions=int(d_regs.size), lines=int(mk["line_off"][-1]), xa_members=int((mk["marks"]["xa_of"] >= 0).sum()),
                                                    cigar_regions=int(mk["cigar_regs"].size), light_reads=int(md["light_reads"]), wave_reads=int(md["wave_reads"]), hbm_reads=int(md["hbm_reads"]),
                                                    launches=int(md["launches"]), note="host arrays in and out, the binding's copies of the result included")
        out["marked regions -> CIGAR (%s)" % label] = dict(tcg, regions=int(mk["cigar_regs"].size))
        # the SAM text of the batch (cs_regions_sam) from these marks and their alignments: names are the reads' numbers, no qualities
        cgm = al.regions_cigar(mk["cigar_reg_off"], mk["cigar_regs"], bases, off)
        ss0 = al.sam_stats(); (_, text), tsam = timed(lambda: al.regions_sam(mk, cgm, bases, off, names, reg_off=d_off)); ss1 = al.sam_stats()
        sd = {k: (ss1[k] - ss0[k]) / (MARK_RUNS + 1) for k in ss1}
        if mflags == 0:
            text_default = text
        out["marks + CIGAR -> SAM text (%s)" % label] = dict(tsam, device_span_ms=sd["kernel_ms"], bytes=len(text), bytes_per_read=len(text) / n, lines=int(sd["lines"]), unmapped=int(sd["unmapped"]),
                                                             xa_entries=int(sd["xa_entries"]), sa_entries=int(sd["sa_entries"]), launches=int(sd["launches"]),
                                                             note="host arrays in and out, the binding's copy of the text included")
    _, tca = timed(lambda: al.regions_cigar(d_off, d_regs, bases, off))
    out["all regions -> CIGAR"] = dict(tca, regions=int(d_regs.size), note="what a caller without cs_regions_mark has to do")
    for name, a, b in (("seed (host call)", t0, t1), ("chain", t1, t2), ("chain_filter", t2, t3), ("extend_chains", t3, t4), ("dedup_regions", t4, t5)):
        out[name] = {"ms": 1e3 * (b - a), "reads_per_s": n / (b - a)}
    kms = sd1["kernel_ms"] - sd0["kernel_ms"]
    out["chain_device"] = {"ms": 1e3 * (t9 - t8), "reads_per_s": n / (t9 - t8), "kernel_ms": kms, "kernel_reads_per_s": n / (kms * 1e-3) if kms > 0 else None,
                           "tree_reads": sd1["tree_reads"] - sd0["tree_reads"], "launches": sd1["launches"] - sd0["launches"], "equal_to_host_chains": True}
    out["chain_gpu"] = {"ms": 1e3 * (t7 - t6), "reads_per_s": n / (t7 - t6), "equal_to_host_chains": True, "note": "host arrays in and out: PCIe-bound"}
    kms = fs1["kernel_ms"] - fs0["kernel_ms"]
    out["chain_filter (device)"] = {"ms": 1e3 * (t11 - t10), "reads_per_s": n / (t11 - t10), "kernel_ms": kms, "wave_reads": fs1["wave_reads"] - fs0["wave_reads"],
                                    "spill_reads": fs1["spill_reads"] - fs0["spill_reads"], "sw_seeds": fs1["sw_seeds"] - fs0["sw_seeds"], "launches": fs1["launches"] - fs0["launches"],
                                    "equal_to_host_filter": True}
    out["chain_filter (gpu, host arrays)"] = {"ms": 1e3 * (t13 - t12), "reads_per_s": n / (t13 - t12), "equal_to_host_filter": True, "note": "host arrays in and out: PCIe-bound"}
    def reg_bytes(n_regs):   # what a download of reg_off and regs moves
        return (n + 1) * 8 + int(n_regs) * ca.ALNREG_DT.itemsize
    out["extend_chains (device)"] = {"ms": 1e3 * (t15 - t14), "reads_per_s": n / (t15 - t14), "download_regions_ms": 1e3 * (t16 - t15), "regions": xd["n_regs"],
                                     "download_bytes": reg_bytes(xd["n_regs"]), "purged": xs1["purged"] - xs0["purged"], "equal_to_host_regions": True}
    out["extend_chains (device, compact)"] = {"ms": 1e3 * (t18 - t17), "reads_per_s": n / (t18 - t17), "download_regions_ms": 1e3 * (t19 - t18), "live_regions": xc["n_regs"],
                                              "download_bytes": reg_bytes(xc["n_regs"]), "equal_to_host_regions_with_qe_gt_qb": True}
    out["counts"] = {"seeds": int(res.n_seeds), "chains": int(c["chains"].size), "chains_after_filter": int(f["chains"].size), "regions": int(g["regs"].size),
                     "regions_after_dedup": int(d["regs"].size), "extensions": int(st1["pairs"] - st0["pairs"]), "ext_launches": int(st1["launches"] - st0["launches"])}
    per_read = np.diff(np.asarray(g["reg_off"]).astype(np.int64))
    out["regions_per_read"] = {"mean": float(per_read.mean()), "p50": float(np.percentile(per_read, 50)), "p99": float(np.percentile(per_read, 99)), "p99.9": float(np.percentile(per_read, 99.9)),
                               "max": int(per_read.max()), "reads_over_64": int((per_read > 64).sum()), "reads_over_1024": int((per_read > 1024).sum()),
                               "sum_sq_over_64": float(((per_read.astype(np.float64) ** 2) / 64).sum())}
    kms = st1["ext_kernel_ms"] - st0["ext_kernel_ms"]
    out["extension_kernels"] = {"ms": kms, "pairs_per_s": (st1["pairs"] - st0["pairs"]) / (kms * 1e-3) if kms > 0 else None, "dp_cells_per_pair": (st1["ext_cells"] - st0["ext_cells"]) / max(1, st1["pairs"] - st0["pairs"]),
                                "note": "the extension kernels alone (HIP events) on this run's own pairs: extensions of real chains die at different rows, unlike the uniform pairs of tools/extend_bench.py"}
    cd = {k: cs1[k] - cs0[k] for k in cs1}
    out["regions -> CIGAR"] = {"ms": 1e3 * (tc1 - tc0), "reads_per_s": n / (tc1 - tc0), "ms_per_million_reads": 1e3 * (tc1 - tc0) * 1e6 / n, "device_span_ms": cd["kernel_ms"],
                               "regions": cd["regions"], "dp_jobs": cd["dp_jobs"], "nodp_jobs": cd["nodp_jobs"], "retries": cd["retries"], "dp_cells": cd["cells"], "launches": cd["launches"],
                               "cigar_ops": int(cg_res["cigar"].size), "md_bytes": int(cg_res["md"].size),
                               "note": "a first measurement: host arrays in and out, the binding's copies of the result included; device_span_ms runs from the first kernel to the last and "
                                       "includes the copies and host waits between them; not part of behind_seeding_reads_per_s"}
    t_all = sum(out[k]["ms"] for k in ("chain", "chain_filter", "extend_chains", "dedup_regions"))
    out["behind_seeding_reads_per_s"] = n / (t_all * 1e-3)
    out["seed (device call)"] = {"ms": 1e3 * (tsd1 - tsd0), "reads_per_s": n / (tsd1 - tsd0)}
    eng.free(d_b); eng.free(d_o)
    for x in (al, ald, chd, ch, eng, ix):
        x.close()
    # the whole path in one call: a mapper of its own (engine, device chainer, aligner) on the same reads, default parameters
    MAP_RUNS = 3
    mp = ca.Mapper(PREFIX, 0)
    mp.map_batch(bases, off, names)
    s0 = mp.stats(); walls = []
    for _ in range(MAP_RUNS):
        ta = time.perf_counter(); _, mtext = mp.map_batch(bases, off, names); walls.append(time.perf_counter() - ta)
    s1 = mp.stats()
    # the same batch as a stream on the same mapper: STREAM_BATCHES submits of it with 1, 2 and 3 kept in flight, wall per batch over the
    # whole stream (its filling and draining included), every collected text checked equal to cs_map_batch's after the clock has stopped
    STREAM_BATCHES = 6
    stream = {}
    for fl in range(1, ca.MAP_MAX_IN_FLIGHT + 1):
        q0 = mp.stats(); texts = []; sent = 0
        ta = time.perf_counter()
        while len(texts) < STREAM_BATCHES:
            while sent < STREAM_BATCHES and sent - len(texts) < fl:
                mp.submit(bases, off, names, id_base=0); sent += 1
            texts.append(mp.collect()[1])
        tb = time.perf_counter()
        q1 = mp.stats()
        assert all(t == mtext for t in texts), "a streamed batch's text differs from cs_map_batch's (%d in flight)" % fl
        del texts
        stream[str(fl)] = {"batches": STREAM_BATCHES, "ms_per_batch": 1e3 * (tb - ta) / STREAM_BATCHES, "reads_per_s": n * STREAM_BATCHES / (tb - ta),
                           "stage_ms": {k: (q1["stage_ms"][k] - q0["stage_ms"][k]) / STREAM_BATCHES for k in q1["stage_ms"]}}
    mp.close()
    assert mtext == text_default, "cs_map_batch's text differs from the separate stages' text"
    per_m = lambda row: out[row]["median_ms_per_million_reads"] * n / 1e6
    separate = {"seed": out["seed (device call)"]["ms"], "chain": out["chain_device"]["ms"], "filter": out["chain_filter (device)"]["ms"], "extend": out["extend_chains (device, compact)"]["ms"],
                "download": out["extend_chains (device, compact)"]["download_regions_ms"], "dedup": out["dedup_regions"]["ms"], "mark": per_m("regions -> marks (default)"),
                "cigar": per_m("marked regions -> CIGAR (default)"), "sam": per_m("marks + CIGAR -> SAM text (default)")}
    wall = float(np.median(walls))
    out["reads -> SAM text (cs_map_batch)"] = {"runs": MAP_RUNS, "ms": 1e3 * wall, "min_ms": 1e3 * min(walls), "max_ms": 1e3 * max(walls), "reads_per_s": n / wall,
                                               "stage_ms": {k: (s1["stage_ms"][k] - s0["stage_ms"][k]) / MAP_RUNS for k in s1["stage_ms"]}, "separate_rows_ms": separate,
                                               "separate_rows_sum_ms": sum(separate.values()), "bytes": len(mtext), "lines": (s1["lines"] - s0["lines"]) // MAP_RUNS,
                                               "unmapped": (s1["unmapped"] - s0["unmapped"]) // MAP_RUNS, "equal_to_separate_stages_text": True,
                                               "note": "host arrays in, the binding's copy of the text included; the separate rows of the tail stages include the binding's copies of their results"}
    best = min(stream.values(), key=lambda v: v["ms_per_batch"])
    out["reads -> SAM text (cs_map_submit / collect)"] = {"in_flight": stream, "ms": best["ms_per_batch"], "reads_per_s": best["reads_per_s"], "blocking_ms_same_run": 1e3 * wall,
                                                          "equal_to_cs_map_batch_text": True,
                                                          "note": "the batch of the cs_map_batch row submitted %d times on the same mapper with 1, 2 and 3 batches kept in flight; ms per batch over the whole stream, "
                                                                  "the binding's copy of every text included; stage_ms per batch as cs_mapper_stats adds it up: each step in the thread that ran it, "
                                                                  "total = submit to completion; ms / reads_per_s: the fastest of the three" % STREAM_BATCHES}
    if tmpdir:
        shutil.rmtree(tmpdir, ignore_errors=True)
    return out


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("reads", nargs="?", type=int, default=200000)
    ap.add_argument("--synth-mbp", type=float, default=0.0, help="instead of the golden reference: a synthetic genome of this size (tools/synth.py, the bench's default profile: random + a 10 %% "
                    "repeat family + duplications), written as FASTA (8 contigs), indexed on the GPU (cs_index_build_fasta); reads with 0.5 %% substitutions, one read in seven with a single-base indel")
    a = ap.parse_args()
    print(json.dumps(run(a.reads, a.synth_mbp)))
