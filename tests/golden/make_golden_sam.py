#!/usr/bin/env python3
"""tests/golden/sam1/: the reference's own SAM lines for the read sets whose regions tests/golden/ddp1 and aln2 hold -- what mem_reg2aln
(comp_seed.cpp:811-880) makes of every region the reference reports: position, CIGAR, NM, MD, and AS (the region's score).

Runs only where oracle/_ref exists (`make -C oracle ref`): oracle/_ref/CompSeed.bswtrace is the reference's complete program, run here with
-a (secondaries are reported too) and -Y (supplementary lines are soft-clipped, so every CIGAR is mem_reg2aln's).  A read's name is the
1-based line number of the reads file.  Per mapped line (flag 4 is skipped): read index, flag, contig index, 0-based position, AS, NM,
the CIGAR in BAM coding as a CSR uint32 array and the MD bytes as a CSR array.  Reads with a character outside ACGTN are left out
(skipped_reads; see odd_reads).  The files carry a fixed zip time stamp: a rerun gives the
same bytes (MANIFEST.json holds their md5).

The reference's output filter (score >= T; a secondary below half its parent's score is dropped) leaves some regions without a line.  The
MANIFEST records per set the mapped lines, the golden regions with score >= 30 and the share of those without a line; a set above 3 % is
marked "containment_only" (tests/test_cigar_scan_cpu.py applies the 3 % cap to the others).  The params.* sets run with their scoring
(aln2/MANIFEST.json's aln_params, every value given to the program explicitly).  cap64's regions come from the harness's --cap-seeds,
which the program does not have: its uncapped run reports 40,597 lines for 4,644 capped regions, nothing to compare, so the set gets a
MANIFEST entry ("no_sam") and no file.
  make_golden_sam.py            all sets
"""
import hashlib, io, json, os, re, subprocess, sys, tempfile, zipfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
REFBIN = os.path.join(ROOT, "oracle", "_ref")
LIMIT = 1 << 20                      # a committed file's size limit
CAP = 0.03
OPS = {"M": 0, "I": 1, "D": 2, "S": 3}
DDP1 = {"main100": "g1", "sorted150": "g1", "ragged": "g1", "repeat100": "g1", "indel150_400": "aln1", "long90": "flt1", "gap3k": "ddp1"}


def save_npz(path, **arrays):
    """np.savez_compressed with a fixed time stamp in the zip entries (the aln2 recipe's)"""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED, compresslevel=9) as zf:
        for k, v in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(v), allow_pickle=False)
            zi = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zi.external_attr = 0o644 << 16
            zf.writestr(zi, buf.getvalue(), compresslevel=9)


def md5(path):
    return hashlib.md5(open(path, "rb").read()).hexdigest()


def run_sam(reads, flags, td):
    cmd = [os.path.join(REFBIN, "CompSeed.bswtrace"), "-t", "1", *flags, "-a", "-Y", os.path.join(HERE, "g1", "ref"), reads]
    r = subprocess.run(cmd, env=dict(os.environ, CS_BSW_TRACE=os.path.join(td, "t.bin")), capture_output=True, cwd=td)
    if r.returncode:
        sys.exit(r.stderr.decode()[-2000:])
    return r.stdout.decode()


def odd_reads(reads):
    """indices of the reads with a character outside ACGTN: the harness that made the regions and the program's own reader do not see the same
    read there (ragged's read 10 holds a '-': the regions know a 95-point alignment, the program reports 94 with other mismatches)"""
    return [k for k, ln in enumerate(open(reads, "rb").read().split(b"\n")) if ln.upper().strip(b"ACGTN")]


def parse(sam, keep_every, skip=()):
    contigs = [ln.split("\t")[1][3:] for ln in sam.split("\n") if ln.startswith("@SQ")]
    rows, cig, cig_off, mdb, md_off, n_lines = [], [], [0], bytearray(), [0], 0
    for ln in sam.split("\n"):
        if not ln or ln[0] == "@":
            continue
        f = ln.split("\t")
        flag = int(f[1])
        if flag & 4:
            continue
        n_lines += 1
        read = int(f[0]) - 1
        if read in skip:
            n_lines -= 1
            continue
        if read % keep_every:
            continue
        tags = {t[:2]: t[5:] for t in f[11:]}
        rows.append((read, flag, contigs.index(f[2]), int(f[3]) - 1, int(tags["AS"]), int(tags["NM"])))
        ops = re.findall(r"(\d+)([MIDS])", f[5])
        assert "".join(a + b for a, b in ops) == f[5], f[5]
        cig += [int(a) << 4 | OPS[b] for a, b in ops]
        cig_off.append(len(cig))
        mdb += tags["MD"].encode()
        md_off.append(len(mdb))
    a = np.array(rows, np.int64).reshape(-1, 6)
    return n_lines, dict(read=a[:, 0].astype(np.int32), flag=a[:, 1].astype(np.int32), rid=a[:, 2].astype(np.int32), pos=a[:, 3].astype(np.int64), AS=a[:, 4].astype(np.int32),
                         NM=a[:, 5].astype(np.int32), cigar=np.array(cig, np.uint32), cigar_off=np.array(cig_off, np.uint64), md=np.frombuffer(bytes(mdb), np.uint8),
                         md_off=np.array(md_off, np.uint64), skipped_reads=np.array(sorted(skip), np.int32))


def main():
    if not os.path.exists(os.path.join(REFBIN, "CompSeed.bswtrace")):
        sys.exit("build the reference first: make -C oracle ref")
    out = os.path.join(HERE, "sam1"); os.makedirs(out, exist_ok=True)
    aln2 = json.load(open(os.path.join(HERE, "aln2", "MANIFEST.json")))["sets"]
    runs = [(name, os.path.join(HERE, d, name + ".txt"), os.path.join(HERE, "ddp1", name + ".ddp.npz"), [], None) for name, d in DDP1.items()]
    for name in sorted(aln2):
        p = aln2[name]["aln_params"]
        flags = [] if not name.startswith("params.") else ["-A", str(p["a"]), "-B", str(p["b"]), "-O", "%d,%d" % (p["o_del"], p["o_ins"]), "-E", "%d,%d" % (p["e_del"], p["e_ins"]),
                                                           "-L", "%d,%d" % (p["pen_clip5"], p["pen_clip3"]), "-w", str(p["w"]), "-d", str(p["zdrop"])]
        runs.append((name, os.path.join(HERE, "aln2", aln2[name]["reads"]), os.path.join(HERE, "aln2", name + ".ddp.npz"), flags, aln2[name]["harness_flags"]))
    manifest = {"cap": CAP, "sets": {}}
    with tempfile.TemporaryDirectory() as td:
        for name, reads, ddp, flags, harness_flags in runs:
            if harness_flags and "--cap-seeds" in harness_flags:
                manifest["sets"][name] = {"no_sam": "the regions were made with the harness's --cap-seeds, which the reference's program does not have"}
                continue
            sam = run_sam(reads, flags, td)
            skip = set(odd_reads(reads))
            path = os.path.join(out, name + ".sam.npz")
            keep_every = 1
            while True:
                n_lines, z = parse(sam, keep_every, skip)
                save_npz(path, **z)
                if os.path.getsize(path) <= LIMIT:
                    break
                keep_every += 1
            zd = np.load(ddp)
            read_of = np.repeat(np.arange(zd["reg_off"].size - 1), np.diff(zd["reg_off"].astype(np.int64)))
            regs30 = int(((zd["reg_score"] >= 30) & ~np.isin(read_of, sorted(skip))).sum())
            unclaimed = (regs30 - n_lines) / regs30
            manifest["sets"][name] = {"program_flags": flags + ["-a", "-Y"], "mapped_lines": n_lines, "lines_kept": int(z["read"].size), "keep_every_kth_read": keep_every, "reads_skipped_not_acgtn": len(skip),
                                      "regions_score_ge_30": regs30, "unclaimed_share": round(unclaimed, 5), "containment_only": bool(unclaimed > CAP),
                                      "indel_lines": int(sum(1 for k in range(z["read"].size) if ((z["cigar"][int(z["cigar_off"][k]):int(z["cigar_off"][k + 1])] & 15) % 3 != 0).any())),
                                      "max_ops": int(np.diff(z["cigar_off"].astype(np.int64)).max())}
            if harness_flags is not None:
                manifest["sets"][name]["harness_flags_of_the_regions"] = harness_flags
            print(name, json.dumps(manifest["sets"][name]))
    manifest["md5"] = {fn: md5(os.path.join(out, fn)) for fn in sorted(os.listdir(out)) if fn != "MANIFEST.json"}
    json.dump(manifest, open(os.path.join(out, "MANIFEST.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
