"""SAM text without a GPU: the bodies of compseed_amd/csrc/sam_scan.hpp (mem_aln2sam, the string part of mem_gen_alt, the unmapped record of
mem_reg2sam) driven in the kernels' order by a plain C++ program (tests/cpp/sam_scan_check.cpp) behind mark_scan_check and
cigar_scan_check.  Over the reference's own regions the text must be the bytes its program wrote (tests/golden/samtext1): main100, long90
(all four modes) and params.oied as whole files, the other sets read by read over every read but those with a character outside ACGTN
(the program's reader and the harness see different reads there) and those MANIFEST.json lists as differing upstream -- a read is listed
only where the parsed fields of mark1 / sam1 already differ from the mark and CIGAR results (test_upstream_reads_are_shown_upstream shows
it), at most 1 % of a set, none in the whole-file sets.  The 8- and 64-lane instantiations of the writing pass run on threads in
lockstep and must give the one-lane build's bytes; the program itself compares every read with a straight-line snprintf routine of its
own and exits non-zero if a writer leaves its range or disagrees with the size pass."""
import numpy as np
import pytest

import _cigar
import _mark
import _sam


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    d = tmp_path_factory.mktemp("sam_scan")
    return dict(mark=_mark.build(str(d / "mark_scan_check")), cigar=_cigar.build(str(d / "cigar_scan_check")), sam=_sam.build(str(d / "sam_scan_check")),
                sam8=_sam.build(str(d / "sam_scan_check8"), 8), sam64=_sam.build(str(d / "sam_scan_check64"), 64))


@pytest.fixture(scope="module")
def one_lane(exes, tmp_path_factory):
    """per run (set, mode): the batch and the one-lane text, computed once"""
    cache = {}

    def get(name, mode):
        if (name, mode) not in cache:
            d = tmp_path_factory.mktemp("one_%s_%s" % (name.replace(".", "_"), mode))
            batch = _sam.cpu_batch(exes, d, name, mode)
            flags, rg, alt = _sam.sam_args(name, mode)
            _sam.write_dir(d / "s", batch, flags, rg, alt)
            cache[name, mode] = (batch, _sam.run(exes["sam"], d / "s"))
        return cache[name, mode]
    return get


@pytest.mark.parametrize("name,mode", _sam.RUNS)
def test_text_is_the_reference_programs_output(one_lane, name, mode):
    _, res = one_lane(name, mode)
    n = _sam.compare(name, mode, res["text_off"], res["text"])
    entry = _sam.MANIFEST["upstream_reads"].get("%s.%s" % (name, mode), {})
    n_reads = res["text_off"].size - 1
    assert len(entry.get("reads", [])) <= _sam.UPSTREAM_CAP * n_reads and not (name in _sam.WHOLE and entry)
    if not entry and not _sam.odd(name):
        assert res["stat"] == _sam.counts_of(name, mode)
    print("%s.%s: %d of %d reads compared, %d bytes" % (name, mode, n, n_reads, len(res["text"])))


def test_upstream_reads_are_shown_upstream(one_lane):
    """a read is left out of a comparison only if mark1's parsed lines for it already differ from the mark result"""
    for key, entry in _sam.MANIFEST["upstream_reads"].items():
        name, mode = key.rsplit(".", 1)
        batch, _ = one_lane(name, mode)
        res = dict(marks=batch["marks"], line_off=batch["line_off"])
        got = _mark.lines_of(name, res)
        want = _mark.expected_lines(name, "all" if mode == "a" else "def")
        for r in entry["reads"]:
            assert got.get(r) != want.get(r), (key, r)


@pytest.mark.parametrize("lanes", [8, 64])
@pytest.mark.parametrize("name,mode", [("ragged", "a"), ("long90", "default"), ("long90", "M"), ("ends", "default"), ("alt.main100", "default"), ("ends40", "CR")])
def test_many_lane_writer_in_lockstep(exes, one_lane, tmp_path, lanes, name, mode):
    batch, want = one_lane(name, mode)
    flags, rg, alt = _sam.sam_args(name, mode)
    _sam.write_dir(tmp_path, batch, flags, rg, alt)
    got = _sam.run(exes["sam%d" % lanes], tmp_path)
    assert got["text"] == want["text"] and got["text_off"].tobytes() == want["text_off"].tobytes() and got["stat"] == want["stat"]


def test_header(tmp_path):
    import compseed_amd as ca
    import _data
    a = ca.Aligner(_data.PREFIX, device=-1)
    assert a.sam_header() == _sam.fixture("main100", "default")[0]
    assert a.sam_header(_sam.RG_LINE) == _sam.fixture("ends40", "CR")[0]
    b = ca.Aligner(_mark.alt_prefix(tmp_path / "alt"), device=-1)
    assert b.sam_header() == _sam.fixture("alt.main100", "default")[0] and b"AH:*" in b.sam_header()


def test_pa_digits_are_glibcs(exes):
    import subprocess
    r = subprocess.run([exes["sam"], "--pa"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "160000 cases, 0 differ" in r.stdout, r.stdout + r.stderr


@pytest.mark.parametrize("lanes", [1, 8, 64])
def test_made_up_reads_at_the_64_boundaries(exes, tmp_path, lanes):
    """NOT a comparison with the reference (see _sam.boundary_batch).  The program compares with its straight-line routine (exit status 5
    otherwise); here: the lane counts agree, and the properties the batch was made for are in the text."""
    batch = _sam.boundary_batch()
    _sam.write_dir(tmp_path / "one", batch, 0, b"rg1")
    want = _sam.run(exes["sam"], tmp_path / "one")
    if lanes > 1:
        _sam.write_dir(tmp_path / "many", batch, 0, b"rg1")
        got = _sam.run(exes["sam%d" % lanes], tmp_path / "many")
        assert got["text"] == want["text"] and got["text_off"].tobytes() == want["text_off"].tobytes()
    recs = [want["text"][int(want["text_off"][r]):int(want["text_off"][r + 1])].split(b"\n")[:-1] for r in range(want["text_off"].size - 1)]
    for k, n_runs in enumerate((63, 64, 65)):
        cg = recs[k][0].split(b"\t")[5]
        assert sum(cg.count(c) for c in (b"M", b"I")) == n_runs
    for k, n_lines in ((3, 64), (4, 65)):
        assert len(recs[k]) == n_lines
        sa = [f for f in recs[k][n_lines - 1].split(b"\t") if f.startswith(b"SA:Z:")][0]
        assert sa.count(b";") == n_lines - 1
        assert b"H" in recs[k][1].split(b"\t")[5] and b"H" not in recs[k][0].split(b"\t")[5] and b"H" not in sa
    xa = [f for f in recs[5][0].split(b"\t") if f.startswith(b"XA:Z:")][0]
    assert xa.count(b";") == 200 and len(recs[5]) == 1
    assert recs[6][0].startswith(b"\t0\t") and recs[7][0].startswith(b"n" * 300 + b"\t")
    rev = recs[8][1].split(b"\t")
    assert rev[5] == b"13H40M27H" and len(rev[9]) == 40 and len(rev[10]) == 40
    off = batch["off"].astype(np.int64)
    q = batch["quals"][off[8]:off[9]]
    assert rev[10] == q[27:67][::-1].tobytes()                              # on the reverse strand the leading clip (13) cuts the read's end
    m_supp, real_sec, alt_supp = recs[8][2].split(b"\t"), recs[8][3].split(b"\t"), recs[8][4].split(b"\t")
    assert m_supp[1] == b"256" and len(m_supp[9]) == 75 and any(f.startswith(b"SA:Z:") for f in m_supp) and b"pa:f:0.403" in m_supp
    assert real_sec[1] == b"256" and real_sec[9] == b"*" and real_sec[10] == b"*" and not any(f.startswith(b"SA:Z:") for f in real_sec)
    assert alt_supp[5] == b"6S74M" and len(alt_supp[9]) == 80               # an ALT line keeps S and the whole read
    assert recs[9][0].split(b"\t")[1] == b"4" and recs[9][0].endswith(b"\tAS:i:0\tXS:i:0\tRG:Z:rg1\tco:Z:9")
    assert want["stat"]["sa_entries"] == 64 * 63 + 65 * 64 + 4 * 3 and want["stat"]["xa_entries"] == 200 and want["stat"]["unmapped"] == 1


def test_what_the_checks_refuse(exes, tmp_path):
    base = _sam.boundary_batch()
    k = [0]

    def refused(**change):
        b = dict(base)
        for f, fn in change.items():
            x = tuple(y.copy() for y in b[f]) if isinstance(b[f], tuple) else b[f].copy()
            y = fn(x)
            b[f] = x if y is None else y
        k[0] += 1
        _sam.write_dir(tmp_path / ("r%d" % k[0]), b, 0, b"")
        _sam.run(exes["sam"], tmp_path / ("r%d" % k[0]), expect=3)

    def setv(field, i, v):
        def f(x):
            x[field][i] = v
        return f

    def seti(i, v):
        def f(x):
            x[i] = v
        return f
    for f in ("off", "line_off", "cigar_reg_off", "reg_off"):
        refused(**{f: seti(0, 1)})                                          # does not start at 0
        refused(**{f: seti(3, int(base[f][5]) + 1)})                        # decreases
    refused(names=lambda x: seti(2, int(x[1][4]) + 1)(x[1]))
    refused(comments=lambda x: seti(0, 1)(x[1]))
    refused(cigar_src=seti(5, base["marks"].size))                          # outside the marks
    refused(cigar_src=seti(5, 4))                                           # not in order: a mark named twice
    refused(marks=setv("line", 3, 2))                                       # lines not 0, 1, 2 ...
    refused(marks=setv("line", 0, -2))
    refused(marks=setv("line", int(base["reg_off"][5]) + 3, 1))             # a line more than line_off says
    refused(marks=setv("xa_of", 0, 1))                                      # a rank outside the read
    refused(marks=setv("xa_of", int(base["reg_off"][5]) + 3, -1))           # an entry for a region that needs none
    refused(alns=setv("cigar_off", 7, base["cigar"].size))
    refused(alns=setv("n_cigar", 7, 0))
    refused(alns=setv("md_off", 7, base["md"].size))
    refused(md=seti(-1, 65))                                                # no NUL behind the last string
    refused(cigar=seti(int(base["alns"]["cigar_off"][9]), 50 << 4 | 5))     # an op code above 4
    refused(alns=setv("rid", 2, 2))
    refused(alns=setv("rid", 2, -1))
    refused(cigar=seti(int(base["alns"]["cigar_off"][9]), 500 << 4 | 3))    # a clip longer than the read
    long_read = base["off"].copy(); long_read[-1] += 70000
    refused(off=lambda x: seti(-1, int(long_read[-1]))(x), bases=lambda x: np.resize(x, int(long_read[-1])), quals=lambda x: np.resize(x, int(long_read[-1])))
