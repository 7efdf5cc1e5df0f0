"""cs_mapper_t on the GPU: reads to SAM text in one call, through the binding (Mapper) and through `compseed_amd_cli --sam`, against the
reference program's complete output files (tests/golden/samtext1) on the 219,937-base g1 index.  Whole files for main100, long90 in four
modes, params.oied, the index with an ALT contig and the FASTQ run with -C -R; the remaining runs read by read under _sam.compare's rule;
batch boundaries with id_base carried; reads that reach no stage; an error in between; the command line with chunks, two mappers on one
GPU, and standard output."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import _aln2
import _cigar
import _data
import _mark
import _sam

pytestmark = pytest.mark.gpu
OIED_FLAGS = ["-A", "1", "-B", "2", "-O", "6,9", "-E", "3,1", "-L", "2,2", "-w", "5", "-d", "60"]
WHOLE_RUNS = [("main100", "default"), ("long90", "default"), ("long90", "Y"), ("long90", "M"), ("long90", "a"), ("params.oied", "default"), (_mark.ALT, "default"), ("ends40", "CR")]
OTHER_RUNS = [("ends", "default"), ("ends", "Y"), ("ends", "M"), ("ends", "a"), ("ragged", "default"), ("ragged", "a"), ("sorted150", "default"), ("indel150_400", "default")]


def _raw(name, mode):
    return gzip.open(os.path.join(_sam.DIR, "%s.%s.sam.gz" % (name, mode)), "rb").read()


def _entry(name, mode):
    return _sam.MANIFEST["files"]["%s.%s.sam.gz" % (name, mode)]


def _reads_file(name):
    if name == "ends40":
        return os.path.join(_sam.DIR, "ends40.fq")
    name = "main100" if name == _mark.ALT else name
    return os.path.join(_cigar.DDP1[name], name + ".txt") if name in _cigar.DDP1 else os.path.join(_aln2.DIR, _aln2.MANIFEST["sets"][name]["reads"])


def _map_params(name, mode):
    """the run's command line as a MapParams: the set's scoring (what its program_flags say: checked for params.oied), T scaled by -A, the mode's switches"""
    import compseed_amd as ca
    i = _sam.inputs(name)
    prm = {} if name == _mark.ALT else dict(_cigar.load(i["base"])[4])
    flags = {"default": 0, "a": ca.MAP_ALL, "Y": ca.MAP_SOFTCLIP, "M": ca.MAP_NO_MULTI, "CR": 0}[mode]
    return ca.MapParams(T=30 * prm.get("a", 1), flags=flags, rg_id=_sam.RG_ID if mode == "CR" else None, **prm)


def _mapper(name, mode, alt_prefix=None):
    import compseed_amd as ca
    return ca.Mapper(alt_prefix if name == _mark.ALT else _data.PREFIX, 0, None, _map_params(name, mode))


def _map_set(m, name):
    i = _sam.inputs(name)
    return m.map_batch(i["bases"], i["off"], i["names"], quals=i["quals"], comments=i["comments"])


@pytest.fixture(scope="module")
def alt_prefix(tmp_path_factory):
    return _mark.alt_prefix(tmp_path_factory.mktemp("alt_index_map"))


@pytest.fixture(scope="module")
def cli():
    import compseed_amd as ca
    return os.path.join(os.path.dirname(ca.lib_path()), "compseed_amd_cli")


@pytest.mark.parametrize("name,mode", WHOLE_RUNS)
def test_whole_files_and_counters(alt_prefix, name, mode):
    """header + text is the reference program's file; reads, lines, unmapped and bytes are the manifest's"""
    import compseed_amd as ca
    e = _entry(name, mode)
    if name == "params.oied":
        assert e["program_flags"] == OIED_FLAGS and _cigar.load(name)[4] == dict(a=1, b=2, o_del=6, o_ins=9, e_del=3, e_ins=1, pen_clip5=2, pen_clip3=2, w=5, zdrop=60)
    m = _mapper(name, mode, alt_prefix)
    try:
        if name == "ends40":                                                # names, qualities and comments from the reader
            rd = ca.Reader(_reads_file(name), 10 ** 9)
            c = rd.next_chunk(copy=True)
            rd.close()
            text_off, text = m.map_batch(c["bases"], c["offsets"], c["names"], quals=c["quals"], comments=c["comments"], id_base=c["first_id"])
            header = m.header(_sam.RG_LINE)
        else:
            text_off, text = _map_set(m, name)
            header = m.header()
        st = m.stats()
    finally:
        m.close()
    want = _raw(name, mode)
    assert header + text == want, (name, mode)
    n = _sam.inputs(name)["off"].size - 1
    assert text_off.size == n + 1 and int(text_off[-1]) == len(text)
    assert (st["reads"], st["lines"] + st["unmapped"], st["unmapped"], st["bytes"], st["batches"]) == (n, e["lines"], e["unmapped"], e["raw_bytes"] - len(header), 1)
    assert st["bases"] == int(_sam.inputs(name)["off"][-1]) and st["regions"] >= st["lines"] and st["stage_ms"]["total"] > 0
    assert abs(sum(v for k, v in st["stage_ms"].items() if k != "total") - st["stage_ms"]["total"]) < 0.05 * st["stage_ms"]["total"] + 1.0


@pytest.mark.parametrize("name,mode", OTHER_RUNS)
def test_remaining_runs_read_by_read(name, mode, capsys):
    """Every read but those of _sam.odd(name) is compared under _sam.compare's rule; MANIFEST['upstream_reads'] is empty and stays empty.
    On the MI355X ends in its four modes, sorted150 and indel150_400 also came out equal to the fixture as whole files (header + text);
    ragged in its two modes did not and cannot: two of its reads hold a character outside ACGTN, which the reference program's reader
    and this library see as different reads (_sam.odd).  WHOLE_FILE_TOO records that, and the test asserts it, so that a run that stops
    being equal as a file is seen."""
    assert _sam.MANIFEST["upstream_reads"] == {}
    m = _mapper(name, mode)
    try:
        text_off, text = _map_set(m, name)
        header = m.header()
    finally:
        m.close()
    n = _sam.inputs(name)["off"].size - 1
    assert _sam.compare(name, mode, text_off, text) == n - len(_sam.odd(name))
    whole = header + text == _raw(name, mode)
    with capsys.disabled():
        print("\n[mapper] %s.%s equal as a whole file: %s (%d odd reads)" % (name, mode, whole, len(_sam.odd(name))))
    assert whole == ((name, mode) in WHOLE_FILE_TOO), (name, mode, whole)


# the remaining runs that came out equal to the fixture as whole files on the MI355X
WHOLE_FILE_TOO = {("ends", "default"), ("ends", "Y"), ("ends", "M"), ("ends", "a"), ("sorted150", "default"), ("indel150_400", "default")}


def test_batch_boundaries_with_id_base_carried():
    """main100 as batches of 1, 63, 64, 65, 1000, none, 1700 and the last 107 reads on one mapper: larger batches follow smaller ones, a
    smaller one follows again, and the concatenation is the fixture's body"""
    i = _sam.inputs("main100")
    bases, off = i["bases"], i["off"].astype(np.int64)
    nb, no = i["names"][0], i["names"][1].astype(np.int64)
    n = off.size - 1
    sizes = [1, 63, 64, 65, 1000, 0, 1700]
    sizes.append(n - sum(sizes))
    assert sizes[-1] == 107
    m = _mapper("main100", "default")
    parts, r0 = [], 0
    try:
        for k in sizes:
            r1 = r0 + k
            text_off, text = m.map_batch(bases[off[r0]:off[r1]], (off[r0:r1 + 1] - off[r0]).astype(np.uint64), (nb[no[r0]:no[r1]], (no[r0:r1 + 1] - no[r0]).astype(np.uint64)), id_base=r0)
            if k == 0:
                assert text == b"" and text_off.tolist() == [0]
            assert text_off.size == k + 1 and int(text_off[-1]) == len(text)
            parts.append(text)
            r0 = r1
        st = m.stats()
    finally:
        m.close()
    assert b"".join(parts) == _sam.fixture("main100", "default")[3]
    assert st["reads"] == n and st["batches"] == len(sizes) - 1 and st["lines"] == 3000


def _no_stage_batch():
    i = _sam.inputs("main100")
    off = i["off"].astype(np.int64)
    reads = [i["bases"][off[0]:off[1]].tobytes(), i["bases"][off[1]:off[2]].tobytes(), b"N" * 30, i["bases"][off[5]:off[5] + 18].tobytes()]
    return reads, [b"1", b"2", b"3", b"4"]


def test_reads_that_reach_no_stage():
    """main100's reads 0 and 1, a read of 30 N and an 18-base read: the first two as in the fixture, the other two what the tail stages give
    for the same reads without regions; a batch of only the last two gives the same two records"""
    import compseed_amd as ca
    reads, names = _no_stage_batch()
    bases, off = _data.pack_reads(reads)
    per = _sam.fixture("main100", "default")[1]
    m = _mapper("main100", "default")
    al = ca.Aligner(_data.PREFIX, 0)
    try:
        text_off, text = m.map_batch(bases, off, names)
        rec = [text[int(text_off[k]):int(text_off[k + 1])] for k in range(4)]
        b2, o2 = _data.pack_reads(reads[2:])
        off2, text2 = m.map_batch(b2, o2, names[2:], id_base=2)
        zero = np.zeros(3, np.uint64)
        marks = al.regions_mark(zero, np.zeros(0, ca.ALNREG_DT), o2)
        alns = al.regions_cigar(marks["cigar_reg_off"], marks["cigar_regs"], b2, o2)
        _, want = al.regions_sam(marks, alns, b2, o2, names[2:], reg_off=zero)
        st = m.stats()
    finally:
        m.close(); al.close()
    assert rec[0] == per[b"1"] and rec[1] == per[b"2"]
    assert rec[2] + rec[3] == want == text2 and off2.tolist() == [0, len(rec[2]), len(want)]
    assert rec[2].split(b"\t")[:4] == [b"3", b"4", b"*", b"0"] and rec[3].split(b"\t")[9] == reads[3]
    assert st["unmapped"] == 4 and st["reads"] == 6


def test_an_error_and_the_next_call():
    import compseed_amd as ca
    i = _sam.inputs("main100")
    m = _mapper("main100", "default")
    try:
        bad = i["off"].copy(); bad[0] = 1
        with pytest.raises(ca.CSError) as ei:
            m.map_batch(i["bases"], bad, i["names"])
        assert ei.value.code == -1
        _, text = _map_set(m, "main100")
        st = m.stats()
    finally:
        m.close()
    assert text == _sam.fixture("main100", "default")[3] and st["batches"] == 1


CLI_RUNS = [("main100", "default", ["-K", "30000"]), ("main100", "default", ["-K", "30000", "--devices", "0,0"]), ("ends40", "CR", ["-C", "-R", _sam.RG_LINE]),
            ("long90", "Y", ["-Y"]), ("long90", "M", ["-M"]), ("long90", "a", ["-a"]), ("params.oied", "default", OIED_FLAGS)]


@pytest.mark.parametrize("name,mode,args", CLI_RUNS, ids=["%s.%s %s" % (n, m, " ".join(a[:3])) for n, m, a in CLI_RUNS])
def test_command_line_writes_the_reference_programs_file(cli, tmp_path, name, mode, args):
    assert args == _entry(name, mode)["program_flags"] or args[:2] == ["-K", "30000"]
    out = str(tmp_path / "out.sam")
    r = subprocess.run([cli, "--sam", out] + args + [_data.PREFIX, _reads_file(name)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert open(out, "rb").read() == _raw(name, mode)
    for stage in ("upload", "seed", "chain", "filter", "extend", "download", "dedup", "mark", "cigar", "sam", "total"):
        assert "Mapper %-9s" % stage in r.stderr
    n = _sam.inputs(name)["off"].size - 1
    assert "SAM:         %d reads, %d lines" % (n, _entry(name, mode)["lines"]) in r.stderr and "reads/s" in r.stderr and "BWT-extend:" in r.stderr
    if args[:2] == ["-K", "30000"]:
        assert sum(_chunks(_reads_file(name), 30000)) == 10                   # ten chunks


def _chunks(path, chunk_bases):
    import compseed_amd as ca
    rd = ca.Reader(path, chunk_bases)
    try:
        while rd.next_chunk() is not None:
            yield 1
    finally:
        rd.close()


def test_command_line_to_standard_output(cli):
    r = subprocess.run([cli, "--sam", "-", "-K", "30000", _data.PREFIX, _reads_file("main100")], capture_output=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout == _raw("main100", "default") and b"Mapper total" in r.stderr
