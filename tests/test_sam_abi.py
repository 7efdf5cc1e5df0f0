"""cs_regions_sam / cs_sam_header / cs_sam_stats without a GPU: the symbols and struct sizes, the order of the errors up to CS_EDEVICE on an
aligner created with device -1, and the header, which is host code, against the fixtures' header lines (tests/golden/samtext1)."""
import ctypes as C

import numpy as np
import pytest

import _data
import _mark
import _sam

EINVAL, EDEVICE, ERANGE = -1, -4, -5


@pytest.fixture(scope="module")
def host():
    import compseed_amd as ca
    a = ca.Aligner(_data.PREFIX, device=-1)
    yield a
    a.close()


def test_symbols_structs_and_defaults(host):
    import compseed_amd as ca
    L = ca.load_library()
    for sym in ("cs_regions_sam", "cs_sam_header", "cs_sam_stats"):
        assert hasattr(L, sym)
    assert C.sizeof(ca.SamParams) == 16 and C.sizeof(ca.binding.CSamResult) == 40 and C.sizeof(ca.SamStats) == 64
    assert (ca.SAM_SOFTCLIP, ca.SAM_WAVE_ONLY) == (1, 0x100)
    assert host.sam_stats() == dict(reads=0, lines=0, unmapped=0, bytes=0, xa_entries=0, sa_entries=0, launches=0, kernel_ms=0.0)


def test_header_is_the_reference_programs(host, tmp_path):
    import compseed_amd as ca
    assert host.sam_header() == _sam.fixture("main100", "default")[0] == b"@SQ\tSN:chr1\tLN:109968\n@SQ\tSN:chr2\tLN:109969\n"
    assert host.sam_header(_sam.RG_LINE) == _sam.fixture("ends40", "CR")[0]
    assert host.sam_header(_sam.RG_LINE).endswith(b"@RG\tID:g1\tSM:s\n")
    alt = ca.Aligner(_mark.alt_prefix(tmp_path / "alt"), device=-1)
    try:
        assert alt.sam_header() == _sam.fixture("alt.main100", "default")[0] and alt.sam_header().count(b"\tAH:*\n") == 1
    finally:
        alt.close()
    for bad in ("RG\\tID:x", "@RG\tID:x", "@RG\\tSM:s"):                     # not @RG, a literal tab, no ID
        with pytest.raises(ca.CSError) as ei:
            host.sam_header(bad)
        assert ei.value.code == EINVAL
    need = C.c_size_t()
    buf = C.create_string_buffer(8)
    assert host.L.cs_sam_header(host.h, None, buf, 8, C.byref(need)) == ERANGE and need.value == len(host.sam_header())
    assert host.L.cs_sam_header(host.h, None, None, 8, C.byref(need)) == EINVAL


def test_error_order_up_to_the_device(host):
    import compseed_amd as ca
    L = host.L
    b = _sam.boundary_batch()
    n = b["off"].size - 1
    ptr = lambda x: x.ctypes.data
    keep = [np.ascontiguousarray(b[k]) for k in ("marks", "line_off", "cigar_reg_off", "cigar_regs", "cigar_src", "alns", "cigar", "md", "reg_off", "bases", "off")]
    marks, line_off, co, cr, cs, alns, cigar, md, reg_off, bases, off = keep
    nm, no = b["names"]
    cmark = ca.binding.CMarkResult(n, marks.size, int(line_off[n]), ptr(marks), ptr(line_off), ca.binding.CAlnResult(n, cr.size, ptr(co), ptr(cr)), ptr(cs))
    ccig = ca.binding.CCigarResult(alns.size, cigar.size, md.size, ptr(alns), ptr(cigar), ptr(md))
    par = ca.SamParams(0, None)
    out = ca.binding.CSamResult()

    def call(par=par, cmark=cmark, ccig=ccig, reg_off=ptr(reg_off), bases=ptr(bases), off=ptr(off), names=ptr(nm), name_off=ptr(no), comments=None, comment_off=None, out=out, h=host.h):
        ref = lambda x: C.byref(x) if x is not None else None
        return L.cs_regions_sam(h, ref(par), ref(cmark), reg_off, ref(ccig), bases, off, None, names, name_off, comments, comment_off, ref(out))
    # 1. null arguments and unknown flag bits
    for kw in (dict(h=None), dict(par=None), dict(cmark=None), dict(ccig=None), dict(out=None), dict(par=ca.SamParams(2, None)), dict(par=ca.SamParams(0x200, None))):
        assert call(**kw) == EINVAL, kw
    # 2. null arrays where the counts say there are entries
    for kw in (dict(reg_off=None), dict(off=None), dict(name_off=None), dict(bases=None), dict(names=None)):
        assert call(**kw) == EINVAL, kw
    no_marks = ca.binding.CMarkResult(n, marks.size, int(line_off[n]), None, ptr(line_off), ca.binding.CAlnResult(n, cr.size, ptr(co), ptr(cr)), ptr(cs))
    assert call(cmark=no_marks) == EINVAL
    # 3. another number of alignments than cigar_regs has entries
    assert call(ccig=ca.binding.CCigarResult(alns.size - 1, cigar.size, md.size, ptr(alns), ptr(cigar), ptr(md))) == EINVAL
    # 4. one of comments / comment_off without the other
    cm, cmo = b["comments"]
    assert call(comments=ptr(cm)) == EINVAL and call(comment_off=ptr(cmo)) == EINVAL
    # 5. everything the host can check is in order: the aligner has no device
    assert call() == EDEVICE
    assert call(comments=ptr(cm), comment_off=ptr(cmo)) == EDEVICE
    # ... and 3 comes before 5, 1 before 3
    assert call(par=None, ccig=ca.binding.CCigarResult(0, 0, 0, None, None, None)) == EINVAL
    with pytest.raises(ca.CSError) as ei:
        host.regions_sam(dict(marks=marks, line_off=line_off, cigar_reg_off=co, cigar_regs=cr, cigar_src=cs), dict(alns=alns, cigar=cigar, md=md), bases, off, b["names"], reg_off=reg_off)
    assert ei.value.code == EDEVICE
