"""SAM text (compseed_amd/csrc/sam_scan.hpp, cs_regions_sam): what the CPU test and the GPU test share.  The regions are the reference's
own after mem_sort_dedup_patch (tests/_mark.py's sets); the expected text is the complete output of its program
(tests/golden/samtext1, make_golden_samtext.py); the plain C++ program tests/cpp/sam_scan_check.cpp runs the header's bodies without a
GPU, behind mark_scan_check and cigar_scan_check."""
import functools
import gzip
import json
import os
import subprocess

import numpy as np

import _cigar
import _data
import _mark

HERE = os.path.dirname(os.path.abspath(__file__))
DIR = os.path.join(_cigar.G, "samtext1")
MANIFEST = json.load(open(os.path.join(DIR, "MANIFEST.json")))
SOFTCLIP, WAVE_ONLY = 1, 0x100
MODES = {"default": (0, 0), "a": (_mark.ALL, 0), "Y": (0, SOFTCLIP), "M": (_mark.NO_MULTI, 0), "CR": (0, 0)}   # mode -> (mark flags, sam flags)
WHOLE = ("main100", "long90", "params.oied")                               # compared as whole files
RUNS = sorted((e["set"], e["mode"]) for e in MANIFEST["files"].values())
RG_LINE, RG_ID = "@RG\\tID:g1\\tSM:s", "g1"
UPSTREAM_CAP = 0.01


@functools.lru_cache(maxsize=None)
def fixture(name, mode):
    """(header bytes, {read name: its records' bytes}, the names in order of first appearance, body bytes)"""
    raw = gzip.open(os.path.join(DIR, "%s.%s.sam.gz" % (name, mode)), "rb").read()
    lines = raw.split(b"\n")
    assert lines[-1] == b""
    hdr = b"".join(ln + b"\n" for ln in lines[:-1] if ln[:1] == b"@")
    per, order = {}, []
    for ln in lines[:-1]:
        if ln[:1] == b"@":
            continue
        nm = ln.split(b"\t", 1)[0]
        if nm not in per:
            per[nm] = b""; order.append(nm)
        per[nm] += ln + b"\n"
    return hdr, per, order, raw[len(hdr):]


def csr(items):
    off = np.zeros(len(items) + 1, np.uint64)
    off[1:] = np.cumsum([len(x) for x in items])
    return np.frombuffer(b"".join(items), np.uint8).copy(), off


@functools.lru_cache(maxsize=None)
def inputs(name):
    """dict(reg_off, regs, bases, off, names (bytes, CSR offsets), quals or None, comments (bytes, offsets) or None, base: the set whose scoring applies)"""
    if name != "ends40":
        reg_off, regs, bases, off, _ = _mark.load(name)
        n = off.size - 1
        return dict(reg_off=reg_off, regs=regs, bases=bases, off=off, names=csr([b"%d" % (k + 1) for k in range(n)]), quals=None, comments=None, base=name)
    reg_off, regs, _, _, _ = _mark.load("ends")
    fq = open(os.path.join(DIR, "ends40.fq"), "rb").read().split(b"\n")
    heads, seqs, quals = fq[0::4][:40], fq[1::4][:40], fq[3::4][:40]
    bases, off = _data.pack_reads(seqs)
    return dict(reg_off=reg_off[:41].copy(), regs=regs[:int(reg_off[40])].copy(), bases=bases, off=off.astype(np.uint64), names=csr([h[1:].split(b" ")[0] for h in heads]),
                quals=np.frombuffer(b"".join(quals), np.uint8).copy(), comments=csr([h.split(b" ", 1)[1] for h in heads]), base="ends")


def ctg_names():
    ln = open(_data.PREFIX + ".ann").read().split("\n")
    return [ln[1 + 2 * k].split()[1].encode() for k in range(int(ln[0].split()[1]))]


def build(out, lanes=1, extra=()):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", "-pthread"] + (["-DCS_EMU_W=%d" % lanes] if lanes > 1 else []) + list(extra)
    c = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "cpp", "sam_scan_check.cpp")], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


def write_dir(d, batch, flags=0, rg_id=b"", alt=None):
    """a batch -- dict(reg_off, marks, line_off, cigar_reg_off, cigar_src, cigar_regs, alns, cigar, md, off, bases, names, quals, comments) -- as the program's files"""
    os.makedirs(str(d), exist_ok=True)
    files = [("meta", np.array([batch["off"].size - 1, flags], np.int64)), ("reg_off", batch["reg_off"].astype(np.uint64)), ("marks", batch["marks"]), ("line_off", batch["line_off"]),
             ("cig_off", batch["cigar_reg_off"]), ("cig_src", batch["cigar_src"]), ("cig_regs", batch["cigar_regs"]), ("alns", batch["alns"]), ("cigar", batch["cigar"]), ("md", batch["md"]),
             ("read_off", batch["off"].astype(np.uint64)), ("bases", batch["bases"]), ("name_off", batch["names"][1]), ("names", batch["names"][0]),
             ("ctg_names", np.frombuffer(b"".join(c + b"\n" for c in ctg_names()), np.uint8)), ("ctg_alt", alt if alt is not None else np.zeros(2, np.uint8)), ("rg", np.frombuffer(rg_id, np.uint8))]
    if batch.get("quals") is not None:
        files.append(("quals", batch["quals"]))
    if batch.get("comments") is not None:
        files += [("comment_off", batch["comments"][1]), ("comments", batch["comments"][0])]
    for stale in ("quals", "comment_off", "comments"):
        if os.path.exists(os.path.join(str(d), stale + ".bin")):
            os.remove(os.path.join(str(d), stale + ".bin"))
    for fn, arr in files:
        np.ascontiguousarray(arr).tofile(os.path.join(str(d), fn + ".bin"))


def run(exe, d, expect=0, args=()):
    r = subprocess.run([exe, str(d), *args], capture_output=True, text=True, timeout=600)
    assert r.returncode == expect, (r.returncode, (r.stdout + r.stderr)[-2000:])
    if expect:
        return None
    rd = lambda n, dt: np.fromfile(os.path.join(str(d), n + ".bin"), dt)
    st = rd("stat", np.uint64)
    return dict(text_off=rd("text_off", np.uint64), text=rd("text", np.uint8).tobytes(), stdout=r.stdout,
                stat=dict(lines=int(st[0]), unmapped=int(st[1]), bytes=int(st[2]), xa_entries=int(st[3]), sa_entries=int(st[4])))


def batch_of(name, marks, alns):
    """the SAM stage's input from a set's inputs, a mark result and a CIGAR result (both _mark / _cigar style dicts)"""
    i = inputs(name)
    return dict(reg_off=i["reg_off"], marks=marks["marks"], line_off=marks["line_off"], cigar_reg_off=marks["cigar_reg_off"], cigar_src=marks["cigar_src"], cigar_regs=marks["cigar_regs"],
                alns=alns["alns"], cigar=alns["cigar"], md=alns["md"], off=i["off"], bases=i["bases"], names=i["names"], quals=i["quals"], comments=i["comments"])


def cpu_batch(exes, tmp, name, mode):
    """mark_scan_check and cigar_scan_check (exes: dict(mark, cigar)) over the set in the mode's flags -> the SAM stage's batch"""
    i = inputs(name)
    marks = _mark.run(exes["mark"], os.path.join(str(tmp), "m"), i["base"] if name == "ends40" else name, MODES[mode][0], arrays=(i["reg_off"], i["regs"], i["off"]))
    alns = _cigar.run(exes["cigar"], os.path.join(str(tmp), "c"), marks["cigar_reg_off"], marks["cigar_regs"], i["bases"], i["off"], _cigar.aln_params("main100" if name == _mark.ALT else i["base"]))
    return batch_of(name, marks, alns)


def sam_args(name, mode):
    """(sam flags, rg id, ALT flags) of a run"""
    return MODES[mode][1], (RG_ID.encode() if mode == "CR" else b""), _mark.ctg_alt(name)


def odd(name):
    """the reads with a character outside ACGTN (make_golden_sam.odd_reads' rule): the program's reader and the harness see different reads"""
    i = inputs(name)
    b, off = i["bases"], i["off"].astype(np.int64)
    ok = np.isin(b, np.frombuffer(b"ACGTNacgtn", np.uint8))
    return {r for r in range(off.size - 1) if not ok[off[r]:off[r + 1]].all()}


def compare(name, mode, text_off, text):
    """the text against the fixture: as a whole file for the WHOLE sets; otherwise read by read over all reads except those with a character
    outside ACGTN and those MANIFEST['upstream_reads'] lists for the run.  Returns the number of reads compared."""
    _, per, order, body = fixture(name, mode)
    if name in WHOLE:
        assert text == body, (name, mode, "the whole file")
        return len(order)
    i = inputs(name)
    nm, no = i["names"][0].tobytes(), i["names"][1].astype(np.int64)
    skip = odd(name) | set(MANIFEST["upstream_reads"].get("%s.%s" % (name, mode), {}).get("reads", []))
    assert set(order) <= {nm[no[r]:no[r + 1]] for r in range(no.size - 1)}   # (the program's reader may drop a read it cannot take: one of odd())
    differ = []
    for r in range(no.size - 1):
        if r not in skip and text[int(text_off[r]):int(text_off[r + 1])] != per.get(nm[no[r]:no[r + 1]]):
            differ.append(r)
    assert not differ, (name, mode, len(differ), differ[:5], text[int(text_off[differ[0]]):int(text_off[differ[0] + 1])], per[nm[no[differ[0]]:no[differ[0] + 1]]])
    return no.size - 1 - len(skip)


def counts_of(name, mode):
    """lines, unmapped, xa_entries, sa_entries as counted in the fixture's text"""
    _, _, _, body = fixture(name, mode)
    lines = [ln for ln in body.split(b"\n") if ln]
    tag = lambda ln, t: sum(len([e for e in f[5:].split(b";") if e]) for f in ln.split(b"\t")[11:] if f.startswith(t))
    unm = sum(1 for ln in lines if int(ln.split(b"\t")[1]) & 4)
    return dict(lines=len(lines) - unm, unmapped=unm, bytes=len(body), xa_entries=sum(tag(ln, b"XA:Z:") for ln in lines), sa_entries=sum(tag(ln, b"SA:Z:") for ln in lines))


def boundary_batch():
    """NOT the reference's regions: what no golden read reaches, made up so that a ballot-step or run-per-lane bug at the 64 boundary shows.
    Reads: lines with exactly 63, 64 and 65 CIGAR runs; a read of 64 and one of 65 lines (all primaries: SA lists of 63 and 64 entries);
    a read with an XA list of 200 members; names of 0 and of 300 bytes; a reverse-strand supplementary line whose two clips differ; a
    real secondary line (-a) and a -M style supplementary (flag 0x100, secondary -1) in one read; an unmapped read.  The expected text is
    the check program's own straight-line routine's."""
    import compseed_amd as ca
    rng = np.random.default_rng(11)
    reads = []                                                              # per read: (length, name, [(mark fields, aln fields, cigar ops, md, score)])

    def ops_for(n_runs, length):
        """n_runs alternating M / I runs that consume `length` read bases"""
        lens = np.ones(n_runs, np.int64); lens[0] += length - n_runs
        return [(int(l), k & 1) for k, l in enumerate(lens)]

    def reg(line, flag=0, secondary=-1, xa_of=-1, is_alt=0, alt_sc=0, mapq=60, xs=0, rid=0, pos=100, is_rev=0, nm=0, ops=((50, 0),), md=b"50", score=50):
        return dict(line=line, flag=flag, secondary=secondary, xa_of=xa_of, is_alt=is_alt, alt_sc=alt_sc, mapq=mapq, xs=xs), dict(rid=rid, pos=pos, is_rev=is_rev, nm=nm), list(ops), md, score
    for n_runs in (63, 64, 65):
        reads.append((300, b"runs%d" % n_runs, [reg(0, ops=ops_for(n_runs, 300), md=b"3A7^CG10", nm=n_runs // 2, score=123456)]))
    for n_lines in (64, 65):
        reads.append((70, b"lines%d" % n_lines, [reg(k, flag=(0x800 if k else 0) | (0x10 if k % 3 == 0 else 0), is_rev=int(k % 3 == 0), pos=1000 * k + 7, rid=k & 1, mapq=k % 61, xs=k,
                                                      ops=[(k % 5 + 1, 3), (60 - k % 5, 0), (9, 3)], md=b"%d" % (60 - k % 5), nm=k % 4) for k in range(n_lines)]))
    reads.append((50, b"xa200", [reg(0, xs=49)] + [reg(-1, xa_of=0, rid=k & 1, pos=int(rng.integers(0, 100000)), is_rev=k % 3 == 1, nm=k % 7, ops=[(k % 9 + 1, 4), (49 - k % 9, 0)], md=b"49") for k in range(200)]))
    reads.append((50, b"", [reg(0)]))
    reads.append((50, b"n" * 300, [reg(0)]))
    reads.append((80, b"revsupp", [reg(0, ops=[(10, 3), (70, 0)], md=b"70"), reg(1, flag=0x810, is_rev=1, ops=[(13, 3), (40, 0), (27, 3)], md=b"40", mapq=17, alt_sc=0),
                                   reg(2, flag=0x100, secondary=-1, ops=[(5, 3), (75, 0)], md=b"75", alt_sc=77, score=31), reg(3, flag=0x100, secondary=0, xs=-1, mapq=0, ops=[(5, 3), (75, 0)], md=b"75"),
                                   reg(4, flag=0x800, is_alt=1, ops=[(6, 3), (74, 0)], md=b"74", alt_sc=0)]))
    reads.append((33, b"unmapped", []))
    marks, alns, cigar, md, regs, reg_off, off, names = [], [], [], bytearray(b"\0"), [], [0], [0], []
    for length, name, rr in reads:
        for m, a, ops, mds, score in rr:
            marks.append((len(marks) - reg_off[-1], m["is_alt"], m["secondary"], m["secondary"], 0, 0, m["alt_sc"], m["mapq"], m["xs"], m["flag"], m["line"], m["xa_of"]))
            alns.append((a["pos"], a["rid"], int(a["is_rev"]), score, a["nm"], len(ops), 0, 1, 0, len(cigar), len(md)))
            cigar += [l << 4 | op for l, op in ops]
            md += mds + b"\0"
            x = np.zeros(1, ca.ALNREG_DT); x["score"] = score; x["rid"] = a["rid"]
            regs.append(x)
        reg_off.append(len(marks)); off.append(off[-1] + length); names.append(name)
    n = len(reads)
    bases = rng.choice(np.frombuffer(b"ACGTNacgt", np.uint8), off[-1])
    quals = (33 + rng.integers(0, 41, off[-1])).astype(np.uint8)
    m = np.array(marks, np.int32).view(_mark.MARK_DT).reshape(-1)
    line_off = np.zeros(n + 1, np.uint64)
    line_off[1:] = np.cumsum([sum(1 for x in rr if x[0]["line"] >= 0) for _, _, rr in reads])
    a = np.zeros(len(alns), _cigar.ALN_DT)
    for k, row in enumerate(alns):
        a[k] = row
    return dict(reg_off=np.array(reg_off, np.uint64), marks=m, line_off=line_off, cigar_reg_off=np.array(reg_off, np.uint64), cigar_src=np.arange(m.size, dtype=np.uint32),
                cigar_regs=np.concatenate(regs), alns=a, cigar=np.array(cigar, np.uint32), md=np.frombuffer(bytes(md), np.uint8).copy(), off=np.array(off, np.uint64), bases=bases,
                names=csr(names), quals=quals, comments=csr([b"co:Z:%d" % k for k in range(n)]))
