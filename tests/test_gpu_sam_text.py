"""cs_regions_sam on the GPU: the SAM text (sam_gpu.hip: the bodies of sam_scan.hpp as kernels).  Stage legs: the reference's own regions
through regions_mark, regions_cigar and regions_sam; the text must be the reference program's (tests/golden/samtext1, under
tests/test_sam_scan_cpu.py's rules) and, byte for byte, what the plain C++ program (tests/cpp/sam_scan_check.cpp, the same bodies on one
CPU lane) gives for the GPU's own marks and alignments; the same bytes under CS_SAM_WAVE_ONLY (one path is left: the flag is accepted and
changes nothing); the counters equal the
counts taken from the fixture text.  The made-up reads at the 64 boundaries give the CPU program's bytes.  End to end: main100's reads
through the whole binding -- engine, device chainer, device chain filter, extend_chains_device with compaction, dedup_regions, mark, CIGAR,
SAM -- header plus text equal to the reference program's output as a whole file."""
import gzip
import os

import numpy as np
import pytest

import _cigar
import _data
import _mark
import _sam

pytestmark = pytest.mark.gpu
LEGS = [("ragged", "a"), ("long90", "default"), ("long90", "Y"), ("long90", "M"), ("ends", "default"), (_mark.ALT, "default"), ("ends40", "CR")]


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _sam.build(str(tmp_path_factory.mktemp("sam_scan_gpu") / "sam_scan_check"))


@pytest.fixture(scope="module")
def alt_prefix(tmp_path_factory):
    return _mark.alt_prefix(tmp_path_factory.mktemp("alt_index_sam"))


def _aligner(name, alt_prefix):
    import compseed_amd as ca
    base = _sam.inputs(name)["base"]
    return ca.Aligner(alt_prefix if name == _mark.ALT else _data.PREFIX, 0, _cigar.aln_params(base) if name != _mark.ALT else None)


def _stages(al, name, mode, sam_flags=0):
    """mark, CIGAR and SAM on the GPU -> (batch for the CPU program, text_off, text)"""
    import compseed_amd as ca
    i = _sam.inputs(name)
    marks = al.regions_mark(i["reg_off"], i["regs"], i["off"], ca.MarkParams(**_mark.mark_params(i["base"])), flags=_sam.MODES[mode][0])
    alns = al.regions_cigar(marks["cigar_reg_off"], marks["cigar_regs"], i["bases"], i["off"])
    flags, rg, _ = _sam.sam_args(name, mode)
    text_off, text = al.regions_sam(marks, alns, i["bases"], i["off"], i["names"], quals=i["quals"], comments=i["comments"], rg_id=rg or None, flags=flags | sam_flags, reg_off=i["reg_off"])
    return _sam.batch_of(name, marks, alns), text_off, text


@pytest.mark.parametrize("name,mode", LEGS)
def test_stage_leg_is_the_references_text_and_the_cpu_programs_bytes(exe, alt_prefix, tmp_path, name, mode):
    al = _aligner(name, alt_prefix)
    try:
        batch, text_off, text = _stages(al, name, mode)
        st = al.sam_stats()
        _, wave_off, wave_text = _stages(al, name, mode, _sam.WAVE_ONLY)
        st2 = al.sam_stats()
    finally:
        al.close()
    _sam.compare(name, mode, text_off, text)
    flags, rg, alt = _sam.sam_args(name, mode)
    _sam.write_dir(tmp_path, batch, flags, rg, alt)
    want = _sam.run(exe, tmp_path)
    assert text == want["text"] and text_off.tobytes() == want["text_off"].tobytes()
    assert wave_text == text and wave_off.tobytes() == text_off.tobytes()   # under CS_SAM_WAVE_ONLY: the same bytes
    got = {k: st[k] for k in ("lines", "unmapped", "bytes", "xa_entries", "sa_entries")}
    assert got == want["stat"] and st["reads"] == text_off.size - 1 and st["launches"] > 0 and st["kernel_ms"] > 0
    if not _sam.odd(name):
        assert got == _sam.counts_of(name, mode)                             # the counts taken from the fixture text
    assert {k: st2[k] - st[k] for k in got} == got


def test_made_up_boundary_reads_give_the_cpu_programs_bytes(exe, tmp_path):
    import compseed_amd as ca
    b = _sam.boundary_batch()
    _sam.write_dir(tmp_path, b, 0, b"rg1")
    want = _sam.run(exe, tmp_path)
    al = ca.Aligner(_data.PREFIX, 0)
    try:
        for flags in (0, _sam.WAVE_ONLY):
            text_off, text = al.regions_sam(b, b, b["bases"], b["off"], b["names"], quals=b["quals"], comments=b["comments"], rg_id="rg1", flags=flags)
            assert text == want["text"] and text_off.tobytes() == want["text_off"].tobytes(), flags
    finally:
        al.close()


def test_buffer_reuse_and_an_error_in_between(exe, tmp_path):
    """a smaller and then a larger batch on the same aligner; one inconsistent input gives CS_EINVAL and the next call succeeds"""
    import compseed_amd as ca
    b = _sam.boundary_batch()
    _sam.write_dir(tmp_path / "b", b, 0, b"")
    want_b = _sam.run(exe, tmp_path / "b")
    al = ca.Aligner(_data.PREFIX, 0, _cigar.aln_params("long90"))
    try:
        big, big_off, big_text = _stages(al, "long90", "default")
        _sam.compare("long90", "default", big_off, big_text)
        call = lambda x: al.regions_sam(x, x, x["bases"], x["off"], x["names"], quals=x["quals"], comments=x["comments"])
        off_b, text_b = call(b)                                              # smaller
        assert text_b == want_b["text"] and off_b.tobytes() == want_b["text_off"].tobytes()
        bad = dict(b, marks=b["marks"].copy())
        bad["marks"]["line"][3] = 2
        with pytest.raises(ca.CSError) as ei:
            call(bad)
        assert ei.value.code == -1
        _, again_off, again_text = _stages(al, "long90", "default")           # larger again
        assert again_text == big_text and again_off.tobytes() == big_off.tobytes()
        empty_off, empty_text = al.regions_sam(dict(marks=b["marks"][:0], line_off=np.zeros(1, np.uint64), cigar_reg_off=np.zeros(1, np.uint64), cigar_regs=b["cigar_regs"][:0], cigar_src=b["cigar_src"][:0]),
                                               dict(alns=b["alns"][:0], cigar=b["cigar"][:0], md=b["md"][:1]), b["bases"][:0], np.zeros(1, np.uint64), (b["names"][0][:0], np.zeros(1, np.uint64)),
                                               reg_off=np.zeros(1, np.uint64))
        assert empty_text == b"" and empty_off.tolist() == [0]
    finally:
        al.close()


def test_end_to_end_main100_is_the_reference_programs_file():
    """the library's output is the reference program's output, file against file"""
    import compseed_amd as ca
    _, _, bases, off, _ = _mark.load("main100")
    n = off.size - 1
    ix = ca.Index.load(_data.PREFIX); eng = ca.Engine(ix, 0); chd = ca.Chainer(_data.PREFIX, device=0); al = ca.Aligner(_data.PREFIX, 0)
    d_b, d_o = eng.alloc(bases.nbytes), eng.alloc(off.nbytes)
    try:
        eng.upload(d_b, bases); eng.upload(d_o, off); eng.sync()
        seeds = eng.seed_batch_device(d_b, d_o, n, bases.size, ca.Params())
        chains = chd.chain_device(seeds, d_o, ca.ChainParams())
        kept = chd.filter_device(chains, d_b, d_o)
        regs = ca.download_regions(eng, al.extend_chains_device(kept, d_b, d_o, flags=ca.ALN_DEV_COMPACT))
        dd = al.dedup_regions(regs["reg_off"], regs["regs"], bases, off)
        marks = al.regions_mark(dd["reg_off"], dd["regs"], off)
        alns = al.regions_cigar(marks["cigar_reg_off"], marks["cigar_regs"], bases, off)
        _, text = al.regions_sam(marks, alns, bases, off, [b"%d" % (k + 1) for k in range(n)], reg_off=dd["reg_off"])
        header = al.sam_header()
    finally:
        eng.free(d_b); eng.free(d_o)
        for x in (al, chd, eng, ix):
            x.close()
    assert header + text == gzip.open(os.path.join(_sam.DIR, "main100.default.sam.gz"), "rb").read()
