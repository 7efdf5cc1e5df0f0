#!/usr/bin/env python3
"""tests/golden/samtext1/: the complete standard output of the reference's program, header and records, for the read sets whose regions
tests/golden/ddp1, aln2 and mark1 hold -- what mem_aln2sam, the string part of mem_gen_alt and the unmapped record of mem_reg2sam
(comp_seed.cpp:883-1024, 1056-1067, 1107-1117) write.  mark1 and sam1 hold fields parsed out of such output; this is the output itself,
compared as a file.

Runs only where oracle/_ref exists (`make -C oracle ref`): oracle/_ref/CompSeed.bswtrace -t 1 <flags> <prefix> <reads>, its stdout stored
as <set>.<mode>.sam.gz (gzip level 9, mtime 0, no file name in the header: a rerun gives the same bytes; MANIFEST.json holds the md5).
A read's name is the 1-based line number of the reads file; no quality, no comment.  ends40.fq is an input fixture made here too: the
first 40 reads of aln2's `ends` as FASTQ, read k (from 1) named r<k> with the comment cm:Z:c<k> and the quality string
chr(33 + (7 k + 3 i) % 41) over its bases i; it runs with -C -R '@RG\\tID:g1\\tSM:s'.  alt.main100 is main100 against a scratch copy of
the g1 index with alt1/ref.alt beside it (as make_golden_mark.py makes it).
  make_golden_samtext.py
"""
import gzip, io, json, os, shutil, subprocess, sys, tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from make_golden_sam import DDP1, LIMIT, REFBIN, md5   # noqa: E402

TOTAL_LIMIT = 3 << 20
MODES = {"default": [], "a": ["-a"], "Y": ["-Y"], "M": ["-M"]}
RUNS = [("main100", ["default"]), ("ragged", ["default", "a"]), ("sorted150", ["default"]), ("long90", ["default", "Y", "M", "a"]), ("ends", ["default", "Y", "M", "a"]),
        ("indel150_400", ["default"]), ("params.oied", ["default"]), ("alt.main100", ["default"])]
RG = "@RG\\tID:g1\\tSM:s"             # as the command line carries it: a backslash and a t


def ends40(path, ends):
    reads = open(ends, "rb").read().split(b"\n")[:40]
    with open(path, "wb") as f:
        for k, rd in enumerate(reads, 1):
            f.write(b"@r%d cm:Z:c%d\n%s\n+\n%s\n" % (k, k, rd, bytes(33 + (7 * k + 3 * i) % 41 for i in range(len(rd)))))


def run(prefix, reads, flags, td):
    cmd = [os.path.join(REFBIN, "CompSeed.bswtrace"), "-t", "1", *flags, prefix, reads]
    r = subprocess.run(cmd, env=dict(os.environ, CS_BSW_TRACE=os.path.join(td, "t.bin")), capture_output=True, cwd=td)
    if r.returncode:
        sys.exit(r.stderr.decode()[-2000:])
    return r.stdout


def store(path, raw):
    buf = io.BytesIO()
    with gzip.GzipFile(filename="", mode="wb", compresslevel=9, fileobj=buf, mtime=0) as g:
        g.write(raw)
    open(path, "wb").write(buf.getvalue())


def main():
    if not os.path.exists(os.path.join(REFBIN, "CompSeed.bswtrace")):
        sys.exit("build the reference first: make -C oracle ref")
    out = os.path.join(HERE, "samtext1"); os.makedirs(out, exist_ok=True)
    sam1 = json.load(open(os.path.join(HERE, "sam1", "MANIFEST.json")))["sets"]
    aln2 = json.load(open(os.path.join(HERE, "aln2", "MANIFEST.json")))["sets"]
    g1 = os.path.join(HERE, "g1", "ref")
    manifest = {"files": {}}
    with tempfile.TemporaryDirectory() as td:
        alt = os.path.join(td, "alt"); os.makedirs(alt)
        for ext in ("bwt", "sa", "pac", "ann", "amb"):
            os.symlink(g1 + "." + ext, os.path.join(alt, "ref." + ext))
        shutil.copy(os.path.join(HERE, "alt1", "ref.alt"), os.path.join(alt, "ref.alt"))
        jobs = []
        for name, modes in RUNS:
            if name == "alt.main100":
                prefix, reads, flags = os.path.join(alt, "ref"), os.path.join(HERE, "g1", "main100.txt"), []
            else:
                prefix = g1
                reads = os.path.join(HERE, DDP1[name], name + ".txt") if name in DDP1 else os.path.join(HERE, "aln2", aln2[name]["reads"])
                flags = [x for x in sam1[name]["program_flags"] if x not in ("-a", "-Y")]
            jobs += [(name + "." + m, prefix, reads, flags + MODES[m], name, m) for m in modes]
        fq = os.path.join(out, "ends40.fq")
        ends40(fq, os.path.join(HERE, "aln2", aln2["ends"]["reads"]))
        jobs.append(("ends40.CR", g1, fq, ["-C", "-R", RG], "ends40", "CR"))
        for stem, prefix, reads, flags, name, mode in jobs:
            raw = run(prefix, reads, flags, td)
            store(os.path.join(out, stem + ".sam.gz"), raw)
            body = [ln for ln in raw.split(b"\n") if ln and ln[:1] != b"@"]
            tag = lambda t: sum(1 for ln in body if b"\t" + t in ln)
            entry = {"set": name, "mode": mode, "program_flags": flags, "raw_bytes": len(raw), "lines": len(body), "unmapped": sum(1 for ln in body if int(ln.split(b"\t")[1]) & 4),
                     "supplementary": sum(1 for ln in body if int(ln.split(b"\t")[1]) & 0x800), "flag_256": sum(1 for ln in body if int(ln.split(b"\t")[1]) & 0x100),
                     "xa_tags": tag(b"XA:Z:"), "sa_tags": tag(b"SA:Z:"), "pa_tags": tag(b"pa:f:")}
            manifest["files"][stem + ".sam.gz"] = entry
            print(stem, json.dumps(entry))
    # reads whose difference from the fixture lies before this stage (tests/test_sam_scan_cpu.py shows it per read); kept across reruns
    old = os.path.join(out, "MANIFEST.json")
    manifest["upstream_reads"] = json.load(open(old)).get("upstream_reads", {}) if os.path.exists(old) else {}
    files = [fn for fn in sorted(os.listdir(out)) if fn != "MANIFEST.json"]
    total = sum(os.path.getsize(os.path.join(out, fn)) for fn in files)
    assert total <= TOTAL_LIMIT and all(os.path.getsize(os.path.join(out, fn)) <= LIMIT for fn in files), total
    manifest["bytes"] = total
    manifest["md5"] = {fn: md5(os.path.join(out, fn)) for fn in files}
    json.dump(manifest, open(old, "w"), indent=1, sort_keys=True)


if __name__ == "__main__":
    main()
