"""From regions to CIGAR / NM / MD (compseed_amd/csrc/cigar_scan.hpp, cs_regions_cigar): what the CPU test and the GPU test share.  The
regions are the reference's own after mem_sort_dedup_patch (tests/golden/ddp1, aln2/*.ddp.npz); the expected alignments are its SAM lines
(tests/golden/sam1, make_golden_sam.py); the plain C++ program tests/cpp/cigar_scan_check.cpp runs the header's bodies without a GPU."""
import collections
import functools
import json
import os
import subprocess

import numpy as np

import _aln2
import _data

HERE = os.path.dirname(os.path.abspath(__file__))
G = os.path.dirname(_data.GOLD)
SAM_DIR = os.path.join(G, "sam1")
MANIFEST = json.load(open(os.path.join(SAM_DIR, "MANIFEST.json")))
DDP1 = {"main100": _data.GOLD, "sorted150": _data.GOLD, "ragged": _data.GOLD, "repeat100": _data.GOLD, "indel150_400": os.path.join(G, "aln1"),
        "long90": os.path.join(G, "flt1"), "gap3k": os.path.join(G, "ddp1")}
SETS = sorted(DDP1) + ["ends", "cap64"] + _aln2.PARAM_SETS
ALN_DT = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("is_rev", "<i4"), ("score", "<i4"), ("nm", "<i4"), ("n_cigar", "<i4"), ("w", "<i4"), ("tries", "<i4"), ("_pad", "<i4"),
                   ("cigar_off", "<u8"), ("md_off", "<u8")])
DEFAULT_BUDGET = 256 << 20
FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep")


@functools.lru_cache(maxsize=None)
def load(name):
    """reg_off, regs (cs_alnreg_t), bases, read offsets, the set's AlnParams fields as a dict"""
    import compseed_amd as ca
    if name in DDP1:
        z = np.load(os.path.join(G, "ddp1", name + ".ddp.npz"))
        raw = open(os.path.join(DDP1[name], name + ".txt"), "rb").read()
        reads = raw.split(b"\n")[:-1] if raw.endswith(b"\n") else raw.split(b"\n")
        bases, off = _data.pack_reads(reads)
        prm = {}
    else:
        z = _aln2.npz(name, "ddp")
        bases, off = _aln2.reads(name)
        prm = dict(_aln2.MANIFEST["sets"][name]["aln_params"])
    regs = np.zeros(z["reg_rb"].size, dtype=ca.ALNREG_DT)
    for f in FIELDS:
        regs[f] = z["reg_" + f]
    return z["reg_off"].astype(np.uint64), regs, bases, off.astype(np.uint64), prm


def bands(name, regs):
    """per region: ksw_global2's band and the backtrack matrix's columns (0 where bwa_gen_cigar2 does no DP), by the header's own formulas
    (first_band, job_band of cigar_scan.hpp) -- for sizing a test's share of a set, never for judging a result"""
    o = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, w=100)
    o.update({k: v for k, v in load(name)[4].items() if k in o})
    lq = (regs["qe"] - regs["qb"]).astype(np.int64); lt = (regs["re"] - regs["rb"]).astype(np.int64); sc = regs["truesc"].astype(np.int64)
    adl = np.abs(lq - lt)

    def infer(q, r):
        w = np.maximum(np.trunc((np.minimum(lq, lt) * o["a"] - sc - q) / r + 2.).astype(np.int64), adl)
        return np.where((lq == lt) & (lq * o["a"] - sc < (q + r - o["a"]) * 2), 0, w)
    w2 = np.maximum(infer(o["o_del"], o["e_del"]), infer(o["o_ins"], o["e_ins"]))
    w2 = np.minimum(np.where(w2 > o["w"], np.minimum(w2, regs["w"]), w2), 4 * o["w"])
    half = ((lq + 1) >> 1) * o["a"]
    max_gap = np.maximum(np.maximum(np.trunc((half - o["o_ins"]) / o["e_ins"] + 1.), np.trunc((half - o["o_del"]) / o["e_del"] + 1.)).astype(np.int64), 1)
    w = np.maximum(np.minimum((max_gap + adl + 1) >> 1, w2), adl + 3)
    return w, np.where((lq == lt) & (w2 == 0), 0, np.minimum(lq, 2 * w + 1))


def subset(name, lanes, max_strips, first_reads=0):
    """a share of the set for a lockstep build, which pays two barriers per exchange, some twenty per strip, whatever the strip holds:
    regions picked one by one, each alone with its read, until their fills make max_strips strips of `lanes` columns (rows x strips a
    row).  The jobs with several strips a row come first, in the set's order (they are what a many-lane fill adds: the carry between
    strips), then the others; a job that no longer fits is passed over.  first_reads > 0: just the set's first reads, whole."""
    reg_off, regs, bases, off, _ = load(name)
    if first_reads:
        n = first_reads
        return reg_off[:n + 1].copy(), regs[:int(reg_off[n])].copy(), bases[:int(off[n])].copy(), off[:n + 1].copy()
    _, n_col = bands(name, regs)
    strips = (regs["re"] - regs["rb"]).astype(np.int64) * ((n_col + lanes - 1) // lanes)
    order = np.concatenate((np.flatnonzero(n_col > lanes), np.flatnonzero((n_col > 0) & (n_col <= lanes))))
    sel, left = [], max_strips
    for g in order.tolist():
        if strips[g] <= left:
            sel.append(g); left -= int(strips[g])
    if not sel:                                                               # (nothing fits: the cheapest job with several strips a row)
        wide = np.flatnonzero(n_col > lanes)
        sel = [int(wide[np.argmin(strips[wide])])]
    sel = np.array(sorted(sel))
    reads = np.searchsorted(reg_off, sel, side="right") - 1
    lens = (off[reads + 1] - off[reads]).astype(np.uint64)
    return (np.arange(sel.size + 1, dtype=np.uint64), regs[sel].copy(), np.concatenate([bases[int(off[r]):int(off[r + 1])] for r in reads]),
            np.concatenate((np.zeros(1, np.uint64), np.cumsum(lens, dtype=np.uint64))))


def aln_params(name):
    import compseed_amd as ca
    return ca.AlnParams(**load(name)[4])


@functools.lru_cache(maxsize=None)
def contigs():
    """l_pac and the contigs' offsets from <prefix>.ann"""
    ln = open(_data.PREFIX + ".ann").read().split("\n")
    l_pac, n = int(ln[0].split()[0]), int(ln[0].split()[1])
    return l_pac, np.array([int(ln[2 + 2 * k].split()[0]) for k in range(n)], np.int64)


def build(out, lanes=1):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off"] + (["-pthread", "-DCS_EMU_W=%d" % lanes] if lanes > 1 else [])
    c = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "cpp", "cigar_scan_check.cpp")], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


def run(exe, d, reg_off, regs, bases, off, ap, budget=DEFAULT_BUDGET, expect=0):
    """the program over one batch; dict(alns, cigar, md, stat) -- or None where a non-zero exit status was expected"""
    l_pac, ctg = contigs()
    meta = np.array([off.size - 1, regs.size, l_pac, ap.a, ap.b, ap.o_del, ap.e_del, ap.o_ins, ap.e_ins, ap.w, ctg.size, budget], np.int64)
    pac = np.fromfile(_data.PREFIX + ".pac", np.uint8)[:(l_pac + 3) // 4]
    os.makedirs(str(d), exist_ok=True)
    for name, arr in (("meta", meta), ("reg_off", reg_off.astype(np.uint64)), ("regs", regs), ("read_off", off.astype(np.uint64)), ("bases", bases), ("pac", pac), ("ctg_off", ctg)):
        np.ascontiguousarray(arr).tofile(os.path.join(str(d), name + ".bin"))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == expect, (r.returncode, r.stdout + r.stderr)
    if expect:
        return None
    rd = lambda n, dt: np.fromfile(os.path.join(str(d), n + ".bin"), dt)
    st = rd("stat", np.uint64)
    return dict(alns=rd("alns", ALN_DT), cigar=rd("cigar", np.uint32), md=rd("md", np.uint8),
                stat=dict(dp_jobs=int(st[0]), nodp_jobs=int(st[1]), retries=int(st[2]), rejected=int(st[3]), cells=int(st[4]), chunks=int(st[5])))


def per_region(res):
    """a result as one tuple per region, free of where the CIGARs lie: (pos, rid, is_rev, score, nm, w, tries, cigar ops, MD without its NUL)"""
    a, cg, md = res["alns"], res["cigar"], res["md"].tobytes()
    out = []
    for k in range(a.size):
        x = a[k]
        c0, m0 = int(x["cigar_off"]), int(x["md_off"])
        m1 = md.index(b"\0", m0)
        out.append((int(x["pos"]), int(x["rid"]), int(x["is_rev"]), int(x["score"]), int(x["nm"]), int(x["w"]), int(x["tries"]), tuple(cg[c0:c0 + int(x["n_cigar"])].tolist()), md[m0:m1]))
    return out


def check_layout(res, n_regs):
    """every region's ranges lie inside the arrays, the CIGARs' and the MD strings' ranges tile them (the leading NUL of md is the empty string)"""
    a = res["alns"]
    assert a.size == n_regs and (a["_pad"] == 0).all()
    assert int(a["n_cigar"].sum()) == res["cigar"].size
    live = a["n_cigar"] > 0
    c0 = a["cigar_off"][live].astype(np.int64); order = np.argsort(c0, kind="stable")
    ends = c0[order] + a["n_cigar"][live][order]
    assert c0.size == 0 or (c0[order][0] == 0 and (c0[order][1:] == ends[:-1]).all() and ends[-1] == res["cigar"].size)
    assert res["md"].size >= 1 and res["md"][0] == 0 and (a["md_off"][~live] == 0).all() and (a["md_off"][live] > 0).all()
    assert int((res["md"] == 0).sum()) == int(live.sum()) + 1          # one string per alignment and the empty one
    assert ((a["rid"][~live] == -1) & (a["pos"][~live] == -1)).all()


@functools.lru_cache(maxsize=None)
def sam(name):
    z = np.load(os.path.join(SAM_DIR, name + ".sam.npz"))
    return {k: z[k] for k in z.files}


def check_against_sam(name, res):
    """per read: the multiset of (is_rev, rid, pos, cigar, NM, MD, AS) over the reference's SAM lines is contained in the one over this
    result's regions, AS being the region's score; and, where the MANIFEST applies it, at most 3 % of the regions with score >= 30 are left
    without a line.  Returns (lines, regions with score >= 30, unclaimed among them)."""
    entry = MANIFEST["sets"][name]
    reg_off, regs, _, _, _ = load(name)
    z = sam(name)
    k_th = entry["keep_every_kth_read"]
    rows = per_region(res)
    have = collections.defaultdict(collections.Counter)
    read_of = np.repeat(np.arange(reg_off.size - 1), np.diff(reg_off.astype(np.int64)))
    for g, (pos, rid, is_rev, _, nm, _, _, cg, md) in enumerate(rows):
        if cg:
            have[int(read_of[g])][(is_rev, rid, pos, cg, nm, md, int(regs["score"][g]))] += 1
    md_all = z["md"].tobytes()
    missing = []
    for k in range(z["read"].size):
        key = (int(z["flag"][k]) >> 4 & 1, int(z["rid"][k]), int(z["pos"][k]), tuple(z["cigar"][int(z["cigar_off"][k]):int(z["cigar_off"][k + 1])].tolist()), int(z["NM"][k]),
               md_all[int(z["md_off"][k]):int(z["md_off"][k + 1])], int(z["AS"][k]))
        c = have[int(z["read"][k])]
        if c[key] > 0:
            c[key] -= 1
        else:
            missing.append((int(z["read"][k]), key))
    assert not missing, (name, len(missing), missing[:3])
    kept = (read_of % k_th == 0) & ~np.isin(read_of, z["skipped_reads"])   # (reads with a character outside ACGTN: the fixture leaves them out)
    regs30 = int(((regs["score"] >= 30) & kept).sum())
    unclaimed = regs30 - int(z["read"].size)
    if not entry["containment_only"]:
        assert unclaimed <= MANIFEST["cap"] * regs30, (name, unclaimed, regs30)
    return int(z["read"].size), regs30, unclaimed
