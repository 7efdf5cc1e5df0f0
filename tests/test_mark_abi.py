"""cs_regions_mark's boundary without a GPU: the new structs of include/compseed_amd.h as gcc sees them equal the ctypes mirrors and the
numpy dtype of binding.py, the defaults are mem_opt_init's, and the errors the host can find come in the documented order -- the last
of them CS_EDEVICE from an aligner created with device -1."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import _data
import _mark

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def ca():
    import compseed_amd
    if not os.path.exists(compseed_amd.lib_path()):
        compseed_amd.build_library()
    compseed_amd.load_library()
    return compseed_amd


def test_structs_match_the_header(ca, tmp_path):
    import compseed_amd.binding as b
    structs = {"cs_mark_params_t": b.MarkParams, "cs_mark_result_t": b.CMarkResult, "cs_mark_stats_t": b.MarkStats}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "compseed_amd.h"', 'int main(void) {']
    for cname, st in structs.items():
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        src += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f, _ in st._fields_]
    src.append('printf("cs_mark_t %zu\\n", sizeof(cs_mark_t));')
    src += ['printf("cs_mark_t.%s %%zu\\n", offsetof(cs_mark_t, %s));' % (f, f) for f in b.MARK_DT.names]
    src.append('printf("flags %u %u %u %u %u\\n", CS_MARK_ALL, CS_MARK_NO_MULTI, CS_MARK_KEEP_SUPP_MAPQ, CS_MARK_NO_LIGHT_PATH, CS_MARK_FROM_HBM);')
    src.append("return 0; }")
    (tmp_path / "abi.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    lines = subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True, check=True).stdout.splitlines()
    got = dict(l.split() for l in lines[:-1])
    for cname, st in structs.items():
        assert int(got[cname]) == ctypes.sizeof(st), cname
        for f, _ in st._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(st, f).offset, (cname, f)
    assert int(got["cs_mark_t"]) == b.MARK_DT.itemsize == _mark.MARK_DT.itemsize
    assert [int(got["cs_mark_t." + f]) for f in b.MARK_DT.names] == [b.MARK_DT.fields[f][1] for f in b.MARK_DT.names]
    assert [int(x) for x in lines[-1].split()[1:]] == [b.MARK_ALL, b.MARK_NO_MULTI, b.MARK_KEEP_SUPP_MAPQ, b.MARK_NO_LIGHT_PATH, b.MARK_FROM_HBM]
    assert (_mark.ALL, _mark.NO_MULTI, _mark.KEEP_SUPP_MAPQ, _mark.NO_LIGHT_PATH, _mark.FROM_HBM) == (b.MARK_ALL, b.MARK_NO_MULTI, b.MARK_KEEP_SUPP_MAPQ, b.MARK_NO_LIGHT_PATH, b.MARK_FROM_HBM)


def test_defaults_are_mem_opt_inits(ca):
    p = ca.MarkParams(T=1, mapq_coef_len=1, max_xa_hits=1, max_xa_hits_alt=1, min_seed_len=1, mask_level=0, drop_ratio=0, xa_drop_ratio=0)
    ca.load_library().cs_mark_params_default(p)
    assert (p.T, p.mapq_coef_len, p.max_xa_hits, p.max_xa_hits_alt, p.min_seed_len) == (30, 50, 5, 200, 19)
    assert (p.mask_level, p.drop_ratio) == (0.5, 0.5) and p.xa_drop_ratio == np.float32(0.8)
    d = ca.MarkParams()
    assert bytes(d) == bytes(p)
    assert _mark.mark_params("main100") == {f: (getattr(d, f) if isinstance(getattr(d, f), int) else round(getattr(d, f), 6)) for f, _ in ca.MarkParams._fields_}


def test_host_side_errors_in_order_without_a_device(ca):
    reg_off, regs, _, off, _ = _mark.load("main100")
    n = int(reg_off[40])
    regs = regs[:n].copy(); reg_off = reg_off[:41].copy(); off = off[:41].copy()
    al = ca.Aligner(_data.PREFIX, -1)
    try:
        def code(**kw):
            with pytest.raises(ca.CSError) as ei:
                al.regions_mark(reg_off, regs, off, **kw)
            return ei.value.code
        assert code(flags=8) == -1                                            # unknown flag bits come before everything else
        assert code(params=ca.MarkParams(mapq_coef_len=0)) == -1              # then the parameters
        assert code(flags=0x1000, params=ca.MarkParams(mapq_coef_len=0)) == -1
        assert code() == -4                                                  # then the device: CS_EDEVICE, before any size is looked at
        assert code(params=ca.MarkParams(mapq_coef_len=200000)) == -4
        st = al.mark_stats()
        assert st["regions"] == 0 and st["launches"] == 0
        L = ca.load_library()
        assert L.cs_regions_mark(al.h, None, None, None, 0, 0, None) == -1    # NULLs
        assert L.cs_mark_stats(al.h, None) == -1
    finally:
        al.close()
