#!/usr/bin/env python3
"""tests/golden/mark1/: which regions the reference turns into SAM lines, with which flag, MAPQ and XS, and which ones it lists as XA
alternatives -- what mem_mark_primary_se (comp_seed.cpp:711-774), mem_approx_mapq_se (:686-709), the loop of mem_reg2sam (:1089-1106) and
mem_gen_alt (:1034-1076) decide for the read sets whose regions tests/golden/ddp1 and aln2 hold.  sam1 (make_golden_sam.py) records what
mem_reg2aln makes of a reported region; this records the decision before it.

Runs only where oracle/_ref exists (`make -C oracle ref`).  oracle/_ref/CompSeed.bswtrace, the reference's complete program, runs twice
per read set: with -a -Y ("all": secondaries are lines, no XA) and with -Y alone ("def": the default mode, XA tags), plus the set's scoring
flags as sam1/MANIFEST.json lists them.  A read's name is the 1-based line number of the reads file.  Per mode, arrays with the prefix
all_ / def_:
  per mapped line, in the program's order: read, flag, rid (contig index), pos (0-based), mapq, AS, XS (-1 when absent), n_sa (SA:Z entries)
  xa_off           CSR over the lines: a line's XA:Z entries, each with xa_rid, xa_rev, xa_pos (0-based), xa_nm and, CSR by xa_cigar_off,
                   xa_cigar in BAM coding (len << 4 | op)
  unmapped         the reads that got an unmapped line
and once per set skipped_reads: the reads with a character outside ACGTN, left out of everything above (sam1's rule).

alt.main100 is main100 against a scratch copy of the g1 index with tests/golden/alt1/ref.alt beside it (make_golden.py alt makes that
prefix the same way): chr2 is an ALT contig.  Its regions come from oracle/_ref/ref_dump --aln --dedup on that prefix and are stored here
as alt.main100.ddp.npz.

The files hold data only and carry a fixed zip time stamp: a rerun gives the same bytes (MANIFEST.json holds their md5).
  make_golden_mark.py            all sets
"""
import json, os, re, shutil, subprocess, sys, tempfile
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden import parse_ddp                                     # noqa: E402
from make_golden_sam import DDP1, OPS, REFBIN, md5, odd_reads, save_npz   # noqa: E402

TOTAL_LIMIT = 3 << 20                # what the files may take together (the aln2 recipe's allowance)
OPS_XA = dict(OPS, H=4)


def run_sam(prefix, reads, flags, td):
    cmd = [os.path.join(REFBIN, "CompSeed.bswtrace"), "-t", "1", *flags, prefix, reads]
    r = subprocess.run(cmd, env=dict(os.environ, CS_BSW_TRACE=os.path.join(td, "t.bin")), capture_output=True, cwd=td)
    if r.returncode:
        sys.exit(r.stderr.decode()[-2000:])
    return r.stdout.decode()


def parse(sam, skip):
    contigs = [ln.split("\t")[1][3:] for ln in sam.split("\n") if ln.startswith("@SQ")]
    rows, unmapped = [], []
    xa_off, xa, xc, xc_off = [0], [], [], [0]
    for ln in sam.split("\n"):
        if not ln or ln[0] == "@":
            continue
        f = ln.split("\t")
        read, flag = int(f[0]) - 1, int(f[1])
        if read in skip:
            continue
        if flag & 4:
            unmapped.append(read)
            continue
        tags = {t[:2]: t[5:] for t in f[11:]}
        rows.append((read, flag, contigs.index(f[2]), int(f[3]) - 1, int(f[4]), int(tags["AS"]), int(tags.get("XS", -1)), len([e for e in tags.get("SA", "").split(";") if e])))
        for e in [e for e in tags.get("XA", "").split(";") if e]:
            ctg, pos, cg, nm = e.split(",")
            ops = re.findall(r"(\d+)([MIDSH])", cg)
            assert "".join(a + b for a, b in ops) == cg and pos[0] in "+-", e
            xa.append((contigs.index(ctg), int(pos[0] == "-"), int(pos[1:]) - 1, int(nm)))
            xc += [int(a) << 4 | OPS_XA[b] for a, b in ops]
            xc_off.append(len(xc))
        xa_off.append(len(xa))
    a = np.array(rows, np.int64).reshape(-1, 8)
    x = np.array(xa, np.int64).reshape(-1, 4)
    return dict(read=a[:, 0].astype(np.int32), flag=a[:, 1].astype(np.int32), rid=a[:, 2].astype(np.int32), pos=a[:, 3], mapq=a[:, 4].astype(np.int32), AS=a[:, 5].astype(np.int32),
                XS=a[:, 6].astype(np.int32), n_sa=a[:, 7].astype(np.int32), xa_off=np.array(xa_off, np.uint64), xa_rid=x[:, 0].astype(np.int32), xa_rev=x[:, 1].astype(np.int32),
                xa_pos=x[:, 2], xa_nm=x[:, 3].astype(np.int32), xa_cigar=np.array(xc, np.uint32), xa_cigar_off=np.array(xc_off, np.uint64), unmapped=np.array(unmapped, np.int32))


def main():
    if not os.path.exists(os.path.join(REFBIN, "CompSeed.bswtrace")):
        sys.exit("build the reference first: make -C oracle ref")
    out = os.path.join(HERE, "mark1"); os.makedirs(out, exist_ok=True)
    sam1 = json.load(open(os.path.join(HERE, "sam1", "MANIFEST.json")))["sets"]
    aln2 = json.load(open(os.path.join(HERE, "aln2", "MANIFEST.json")))["sets"]
    g1 = os.path.join(HERE, "g1", "ref")
    manifest = {"sets": {}}
    with tempfile.TemporaryDirectory() as td:
        alt = os.path.join(td, "alt"); os.makedirs(alt)
        for ext in ("bwt", "sa", "pac", "ann", "amb"):
            os.symlink(g1 + "." + ext, os.path.join(alt, "ref." + ext))
        shutil.copy(os.path.join(HERE, "alt1", "ref.alt"), os.path.join(alt, "ref.alt"))
        main100 = os.path.join(HERE, "g1", "main100.txt")
        tmp, atmp, dtmp = os.path.join(td, "o.bin"), os.path.join(td, "a.bin"), os.path.join(td, "d.bin")
        r = subprocess.run([os.path.join(REFBIN, "ref_dump"), os.path.join(alt, "ref"), main100, tmp, "--aln", atmp, "--dedup", dtmp], capture_output=True, text=True)
        if r.returncode:
            sys.exit(r.stderr[-2000:])
        save_npz(os.path.join(out, "alt.main100.ddp.npz"), **parse_ddp(dtmp))
        runs = []
        for name in sorted(sam1):
            if "no_sam" in sam1[name]:
                continue
            reads = os.path.join(HERE, DDP1[name], name + ".txt") if name in DDP1 else os.path.join(HERE, "aln2", aln2[name]["reads"])
            runs.append((name, g1, reads, [x for x in sam1[name]["program_flags"] if x not in ("-a", "-Y")]))
        runs.append(("alt.main100", os.path.join(alt, "ref"), main100, []))
        for name, prefix, reads, flags in runs:
            skip = set(odd_reads(reads))
            z = {"skipped_reads": np.array(sorted(skip), np.int32)}
            entry = {"program_flags": flags, "reads_skipped_not_acgtn": len(skip)}
            for mode, mflags in (("all", ["-a", "-Y"]), ("def", ["-Y"])):
                p = parse(run_sam(prefix, reads, flags + mflags, td), skip)
                z.update({mode + "_" + k: v for k, v in p.items()})
                entry[mode] = {"mapped_lines": int(p["read"].size), "unmapped_reads": int(p["unmapped"].size), "supplementary_lines": int((p["flag"] & 0x800 != 0).sum()),
                               "secondary_lines": int((p["flag"] & 0x100 != 0).sum()), "xa_entries": int(p["xa_rid"].size), "lines_with_xa": int((np.diff(p["xa_off"].astype(np.int64)) > 0).sum())}
            save_npz(os.path.join(out, name + ".mark.npz"), **z)
            manifest["sets"][name] = entry
            print(name, json.dumps(entry))
    files = [fn for fn in sorted(os.listdir(out)) if fn != "MANIFEST.json"]
    total = sum(os.path.getsize(os.path.join(out, fn)) for fn in files)
    assert total <= TOTAL_LIMIT and all(os.path.getsize(os.path.join(out, fn)) <= 1 << 20 for fn in files), total
    manifest["bytes"] = total
    manifest["md5"] = {fn: md5(os.path.join(out, fn)) for fn in files}
    json.dump(manifest, open(os.path.join(out, "MANIFEST.json"), "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
