"""Primary marking, MAPQ, SAM line selection and XA membership (compseed_amd/csrc/mark_scan.hpp, cs_regions_mark): what the CPU test and the
GPU test share.  The regions are the reference's own after mem_sort_dedup_patch (tests/golden/ddp1, aln2/*.ddp.npz, and
mark1/alt.main100.ddp.npz for the index with an ALT contig); the expected lines are its SAM lines in both modes (tests/golden/mark1,
make_golden_mark.py); the plain C++ program tests/cpp/mark_scan_check.cpp runs the header's bodies without a GPU."""
import functools
import json
import os
import shutil
import subprocess

import numpy as np

import _cigar
import _data

HERE = os.path.dirname(os.path.abspath(__file__))
MARK_DIR = os.path.join(_cigar.G, "mark1")
MANIFEST = json.load(open(os.path.join(MARK_DIR, "MANIFEST.json")))
ALT = "alt.main100"
SETS = sorted(MANIFEST["sets"])
MARK_DT = np.dtype([(n, "<i4") for n in ("reg", "is_alt", "secondary", "secondary_all", "sub", "sub_n", "alt_sc", "mapq", "xs", "flag", "line", "xa_of")])
ALL, NO_MULTI, KEEP_SUPP_MAPQ, NO_LIGHT_PATH, FROM_HBM = 1, 2, 4, 0x100, 0x200
INT_MAX = 2 ** 31 - 1


@functools.lru_cache(maxsize=None)
def load(name):
    """reg_off, regs (cs_alnreg_t), bases, read offsets, the set's AlnParams fields as a dict"""
    if name != ALT:
        return _cigar.load(name)
    import compseed_amd as ca
    z = np.load(os.path.join(MARK_DIR, ALT + ".ddp.npz"))
    regs = np.zeros(z["reg_rb"].size, dtype=ca.ALNREG_DT)
    for f in _cigar.FIELDS:
        regs[f] = z["reg_" + f]
    _, _, bases, off, _ = _cigar.load("main100")
    return z["reg_off"].astype(np.uint64), regs, bases, off, {}


@functools.lru_cache(maxsize=None)
def fixture(name):
    z = np.load(os.path.join(MARK_DIR, name + ".mark.npz"))
    return {k: z[k] for k in z.files}


def scoring(name):
    o = dict(a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1)
    o.update({k: v for k, v in load(name)[4].items() if k in o})
    return o


def mark_params(name):
    """mem_opt_init's values; T scaled by -A as the program's main does (fastmap.c:146)"""
    return dict(T=30 * scoring(name)["a"], mapq_coef_len=50, max_xa_hits=5, max_xa_hits_alt=200, min_seed_len=19, mask_level=0.5, drop_ratio=0.5, xa_drop_ratio=0.8)


def ctg_alt(name):
    return np.array([0, 1] if name == ALT else [0, 0], np.uint8)            # tests/golden/alt1/ref.alt names chr2


def alt_prefix(d):
    """the g1 index with alt1's .alt file beside it, under d"""
    os.makedirs(str(d), exist_ok=True)
    for ext in ("bwt", "sa", "pac", "ann", "amb"):
        shutil.copy(_data.PREFIX + "." + ext, os.path.join(str(d), "ref." + ext))
    shutil.copy(os.path.join(_cigar.G, "alt1", "ref.alt"), os.path.join(str(d), "ref.alt"))
    return os.path.join(str(d), "ref")


def build(out, lanes=1, extra=()):
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off"] + (["-pthread", "-DCS_EMU_W=%d" % lanes] if lanes > 1 else []) + list(extra)
    c = subprocess.run(cmd + ["-o", out, os.path.join(HERE, "cpp", "mark_scan_check.cpp")], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


def run(exe, d, name, flags=0, arrays=None, params=None, id_base=0, expect=0):
    """the program over one batch (the set's, or arrays = (reg_off, regs, read offsets)); dict(marks, line_off, cigar_reg_off, cigar_regs,
    cigar_src, stat) -- or None where a non-zero exit status was expected"""
    import compseed_amd as ca
    reg_off, regs, off = arrays if arrays is not None else (load(name)[0], load(name)[1], load(name)[3])
    l_pac, _ = _cigar.contigs()
    o, p, alt = scoring(name), dict(mark_params(name), **(params or {})), ctg_alt(name)
    meta = np.array([off.size - 1, regs.size, l_pac, alt.size, o["a"], o["b"], o["o_del"], o["e_del"], o["o_ins"], o["e_ins"], p["T"], p["mapq_coef_len"], p["max_xa_hits"],
                     p["max_xa_hits_alt"], p["min_seed_len"], flags, id_base], np.int64)
    fpar = np.array([p["mask_level"], p["drop_ratio"], p["xa_drop_ratio"]], np.float32)
    os.makedirs(str(d), exist_ok=True)
    for fn, arr in (("meta", meta), ("fpar", fpar), ("reg_off", reg_off.astype(np.uint64)), ("regs", regs), ("read_off", off.astype(np.uint64)), ("ctg_alt", alt)):
        np.ascontiguousarray(arr).tofile(os.path.join(str(d), fn + ".bin"))
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=600)
    assert r.returncode == expect, (r.returncode, r.stdout + r.stderr)
    if expect:
        return None
    rd = lambda n, dt: np.fromfile(os.path.join(str(d), n + ".bin"), dt)
    st = rd("stat", np.uint64)
    return dict(marks=rd("marks", MARK_DT), line_off=rd("line_off", np.uint64), cigar_reg_off=rd("cig_off", np.uint64), cigar_regs=rd("cig_regs", ca.ALNREG_DT), cigar_src=rd("cig_src", np.uint32),
                stat=dict(lines=int(st[0]), xa_members=int(st[1]), cigar_regions=int(st[2])))


def tiled_read(tiles=150, children=300, seed=5):
    """NOT the reference's regions: no golden read has more than a handful of primaries, so the list z of mem_mark_primary_se_core never
    spans a second ballot step there.  A made-up batch of three reads, the middle one with `tiles` disjoint 50-base regions (all
    primaries: z grows to `tiles`) and `children` regions of 40 bases, each inside one tile and scoring 1 .. 12 below it, in shuffled
    order.  Returns (reg_off, regs, read offsets) and, per region of the middle read in input order, its tile (-1 for a tile itself)."""
    import compseed_amd as ca
    rng = np.random.default_rng(seed)
    n = tiles + children
    tile_of = np.concatenate((np.full(tiles, -1), rng.integers(0, tiles, children)))
    tsc = 100 + np.arange(tiles) % 7
    t = np.where(tile_of < 0, np.arange(n), tile_of)
    mid = np.zeros(n, ca.ALNREG_DT)
    mid["qb"] = 60 * t + np.where(tile_of < 0, 0, 5); mid["qe"] = mid["qb"] + np.where(tile_of < 0, 50, 40)
    mid["score"] = mid["truesc"] = np.where(tile_of < 0, tsc[t], tsc[t] - rng.integers(1, 13, n))
    mid["rb"] = 1000 + 100 * np.arange(n); mid["re"] = mid["rb"] + (mid["qe"] - mid["qb"]); mid["w"] = 100
    order = rng.permutation(n)
    mid, tile_of = mid[order], np.where(tile_of[order] < 0, -1, np.argsort(order)[np.maximum(tile_of[order], 0)])   # (a child's tile by its input index)
    reg_off, regs, _, off, _ = load("main100")
    a, b = int(reg_off[1]), int(reg_off[2])
    regs3 = np.concatenate((regs[:a], mid, regs[a:b]))
    return (np.array([0, a, a + n, a + n + b - a], np.uint64), regs3, np.array([0, int(off[1]), int(off[1]) + 60 * tiles, int(off[1]) + 60 * tiles + int(off[2] - off[1])], np.uint64)), tile_of


def check_tiled(res, arrays, tile_of):
    """what mem_mark_primary_se_core's rule gives for tiled_read's middle read, worked out from the regions alone"""
    reg_off, regs, _ = arrays
    c0, c1 = int(reg_off[1]), int(reg_off[2])
    m, x = res["marks"][c0:c1], regs[c0:c1]
    rank_of = np.argsort(m["reg"])                                           # input index -> rank
    sc = x["score"][m["reg"]]
    assert (np.diff(sc) <= 0).all()                                          # sorted by score
    tiles = tile_of < 0
    assert (m["secondary"][rank_of[tiles]] == -1).all()
    assert (m["secondary"][rank_of[~tiles]] == rank_of[tile_of[~tiles]]).all()   # a child's parent is its tile
    for t in np.flatnonzero(tiles).tolist():
        kids = x["score"][tile_of == t]
        mt = m[rank_of[t]]
        assert mt["sub"] == (kids.max() if kids.size else 0) and mt["sub_n"] == int((x["score"][t] - kids <= 7).sum()), t
    ln = m[m["line"] >= 0]
    assert ln.size == int(tiles.sum()) and ln["flag"][0] & 0x900 == 0 and (ln["flag"][1:] & 0x900 == 0x800).all()


def same_bytes(got, want, what):
    for k in ("marks", "line_off", "cigar_reg_off", "cigar_regs", "cigar_src"):
        assert got[k].tobytes() == want[k].tobytes(), (what, k)


def check_properties(name, res, arrays=None):
    """marks[].reg is a permutation within each read; line_off and cigar_reg_off are CSR arrays; a read's lines are numbered in rank order;
    cigar_regs / cigar_src are the regions with line >= 0 or xa_of >= 0 in rank order"""
    reg_off, regs = (arrays[0], arrays[1]) if arrays is not None else load(name)[:2]
    m = res["marks"]
    ro = reg_off.astype(np.int64)
    assert m.size == regs.size and res["line_off"].size == ro.size and res["cigar_reg_off"].size == ro.size
    assert res["line_off"][0] == 0 and res["cigar_reg_off"][0] == 0
    read_of = np.repeat(np.arange(ro.size - 1), np.diff(ro))
    order = np.lexsort((m["reg"], read_of))
    assert (m["reg"][order] == np.arange(m.size) - ro[read_of]).all()      # a permutation of 0 .. n - 1 in every read
    lines = m["line"] >= 0
    assert (np.diff(res["line_off"].astype(np.int64)) == np.bincount(read_of[lines], minlength=ro.size - 1)).all()
    first = np.cumsum(lines) - 1 - (np.cumsum(lines) - lines)[ro[read_of]] if m.size else np.zeros(0, np.int64)
    assert (m["line"][lines] == first[lines]).all()                         # numbered 0, 1, ... in rank order
    need = lines | (m["xa_of"] >= 0)
    assert (res["cigar_src"] == np.flatnonzero(need)).all()
    assert (np.diff(res["cigar_reg_off"].astype(np.int64)) == np.bincount(read_of[need], minlength=ro.size - 1)).all()
    src = ro[read_of] + m["reg"]                                             # a mark's region in the input
    assert res["cigar_regs"].tobytes() == regs[src[need]].tobytes()
    assert res["stat"]["lines"] == int(lines.sum()) and res["stat"]["cigar_regions"] == int(need.sum()) if "stat" in res else True


def lines_of(name, res, arrays=None):
    """per read with lines: [(flag, mapq, AS, XS, n_sa), ...] in line order, as the program under test gives them"""
    reg_off, regs = (arrays[0], arrays[1]) if arrays is not None else load(name)[:2]
    m = res["marks"]
    ro = reg_off.astype(np.int64)
    out = {}
    for r in np.flatnonzero(np.diff(res["line_off"].astype(np.int64)) > 0).tolist():
        mm = m[ro[r]:ro[r + 1]]
        ln = mm[mm["line"] >= 0]
        assert (ln["line"] == np.arange(ln.size)).all()
        prim = int((ln["flag"] & 0x100 == 0).sum())
        out[r] = [(int(x["flag"]), int(x["mapq"]), int(regs["score"][ro[r] + x["reg"]]), int(x["xs"]), 0 if x["flag"] & 0x100 else prim - 1) for x in ln]
    return out


def expected_lines(name, mode):
    z = fixture(name)
    out = {}
    for k in range(z[mode + "_read"].size):
        out.setdefault(int(z[mode + "_read"][k]), []).append(tuple(int(z[mode + "_" + f][k]) for f in ("flag", "mapq", "AS", "XS", "n_sa")))
    return out


def check_lines(name, res, mode):
    """Every read's lines are exactly the fixture's, in order: flag (all bits), MAPQ, AS, XS, the number of SA entries; the reads without a line
    are exactly the fixture's unmapped ones.  The reads the fixture leaves out (a character outside ACGTN) are left out here.  Returns the number of lines compared."""
    z = fixture(name)
    skip = set(z["skipped_reads"].tolist())
    got = {r: v for r, v in lines_of(name, res).items() if r not in skip}
    want = expected_lines(name, mode)
    differ = [r for r in sorted(set(got) | set(want)) if got.get(r) != want.get(r)]
    assert not differ, (name, mode, len(differ), [(r, got.get(r), want.get(r)) for r in differ[:3]])
    n_reads = load(name)[0].size - 1
    unmapped = sorted(set(range(n_reads)) - set(got) - skip)
    assert unmapped == sorted(z[mode + "_unmapped"].tolist()), (name, mode)
    return sum(len(v) for v in want.values())


def check_xa_counts(name, res):
    """default mode: the regions with xa_of >= 0, grouped by primary, are as many as the XA entries of that primary's line in the fixture"""
    z = fixture(name)
    skip = set(z["skipped_reads"].tolist())
    reg_off = load(name)[0].astype(np.int64)
    m = res["marks"]
    n_xa = np.diff(z["def_xa_off"].astype(np.int64))
    k = 0
    for r in sorted(expected_lines(name, "def")):
        mm = m[reg_off[r]:reg_off[r + 1]]
        for p in np.flatnonzero(mm["line"] >= 0).tolist():
            assert int((mm["xa_of"] == p).sum()) == int(n_xa[k]), (name, r, p)
            k += 1
    assert k == n_xa.size
    members = int(sum((m["xa_of"][reg_off[r]:reg_off[r + 1]] >= 0).sum() for r in range(reg_off.size - 1) if r not in skip))
    return int(n_xa.sum()), members


def check_cigars(name, res, alns):
    """after the CIGAR stage over cigar_regs (alns: _cigar-style dict for them): each XA entry's contig, strand, position, CIGAR and NM equal the
    fixture's, in the order of the list; each line's position, CIGAR, NM and MD equal sam1's.  Returns (XA entries, lines) compared."""
    z, s = fixture(name), _cigar.sam(name)
    reg_off = load(name)[0].astype(np.int64)
    m = res["marks"]
    rows = _cigar.per_region(alns)
    assert len(rows) == res["cigar_src"].size
    row_of = {int(g): rows[t] for t, g in enumerate(res["cigar_src"].tolist())}
    xo, xco = z["def_xa_off"].astype(np.int64), z["def_xa_cigar_off"].astype(np.int64)
    # sam1 holds the -a run: a read's non-secondary lines, in order, are the default run's lines
    md_all = s["md"].tobytes()
    sam_rows = {}
    for k in np.flatnonzero(s["flag"] & 0x100 == 0).tolist():
        sam_rows.setdefault(int(s["read"][k]), []).append((int(s["flag"][k]) >> 4 & 1, int(s["rid"][k]), int(s["pos"][k]),
                                                           tuple(s["cigar"][int(s["cigar_off"][k]):int(s["cigar_off"][k + 1])].tolist()), int(s["NM"][k]), md_all[int(s["md_off"][k]):int(s["md_off"][k + 1])]))
    k = n_x = n_l = 0
    for r in sorted(expected_lines(name, "def")):
        c0 = int(reg_off[r])
        mm = m[c0:reg_off[r + 1]]
        for li, p in enumerate(np.flatnonzero(mm["line"] >= 0).tolist()):
            pos, rid, is_rev, _, nm, _, _, cg, md = row_of[c0 + p]
            assert (is_rev, rid, pos, cg, nm, md) == sam_rows[r][li], (name, r, p)
            n_l += 1
            got = []
            for q in np.flatnonzero(mm["xa_of"] == p).tolist():
                pos, rid, is_rev, _, nm, _, _, cg, _ = row_of[c0 + q]
                got.append((rid, is_rev, pos, nm, cg))
            want = [(int(z["def_xa_rid"][e]), int(z["def_xa_rev"][e]), int(z["def_xa_pos"][e]), int(z["def_xa_nm"][e]), tuple(z["def_xa_cigar"][xco[e]:xco[e + 1]].tolist())) for e in range(xo[k], xo[k + 1])]
            assert got == want, (name, r, p, got, want)
            n_x += len(want)
            k += 1
    return n_x, n_l
