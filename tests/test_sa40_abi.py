"""CPU-side checks of engine option `sa40` (40-bit suffix-array / inverse-SA entries) and of cs_engine_memory at the C ABI."""
import ctypes
import os
import re
import subprocess

import pytest

import _data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import compseed_amd as ca
    if not os.path.exists(ca.lib_path()):
        ca.build_library()
    return ca.load_library()


def test_memory_entry_point_is_declared_and_exported(lib):
    import compseed_amd.binding as b
    hdr = open(os.path.join(ROOT, "include", "compseed_amd.h")).read()
    assert re.search(r"\bint\s+cs_engine_memory\s*\(\s*const cs_engine_t \*e,\s*cs_memory_t \*out\s*\)\s*;", hdr)
    assert "cs_engine_memory" in b.SYMBOLS
    assert hasattr(lib, "cs_engine_memory")


def _gcc_layout(tmp_path, structs):
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "compseed_amd.h"', 'int main(void) {']
    for cname, st in structs.items():
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        for fname, _ in st._fields_:
            src.append('printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, fname, cname, fname))
    src.append("return 0; }")
    c = tmp_path / "abi40.c"
    c.write_text("\n".join(src))
    exe = tmp_path / "abi40"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(c)], check=True)
    return dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.splitlines())


def test_new_structs_match_their_mirrors(lib, tmp_path):
    import compseed_amd.binding as b
    structs = {"cs_memory_t": b.Memory, "cs_engine_options_t": b.EngineOptions}
    got = _gcc_layout(tmp_path, structs)
    for cname, st in structs.items():
        assert int(got[cname]) == ctypes.sizeof(st), cname
        for fname, _ in st._fields_:
            assert int(got["%s.%s" % (cname, fname)]) == getattr(st, fname).offset, (cname, fname)
    names = [n for n, _ in b.EngineOptions._fields_]
    assert names[-2:] == ["sa40", "reserved"] and len(b.EngineOptions().reserved) == 2
    assert [n for n, _ in b.Memory._fields_] == ["occ_bwt", "sampled_sa", "full_sa", "isa", "text", "lcp_rep", "jump_table", "kmer_filter",
                                                 "pass_ctx", "total", "sa_entry_bits", "n_pass_ctx"]


def test_options_struct_keeps_its_size(lib, tmp_path):
    """sa40 took reserved[0]: the struct is as large as before the option existed.  The earlier size from the earlier field list:
    eight int32, two int64, seven int32, int32 reserved[3]; natural alignment, the struct aligned to 8."""
    import compseed_amd.binding as b
    off = 0
    for size, count in ((4, 8), (8, 2), (4, 7), (4, 3)):
        off = (off + size - 1) // size * size + size * count
    before = (off + 7) // 8 * 8
    assert before == 88
    assert ctypes.sizeof(b.EngineOptions) == before
    assert int(_gcc_layout(tmp_path, {"cs_engine_options_t": b.EngineOptions})["cs_engine_options_t"]) == before
    assert b.EngineOptions.sa40.offset == before - 12          # where reserved[0] was


def test_defaults(lib):
    import compseed_amd as ca
    o = ca.EngineOptions()
    assert o.sa40 == 0 and list(o.reserved) == [0, 0]
    assert ca.EngineOptions(sa40=1).sa40 == 1
    with pytest.raises(TypeError):
        ca.EngineOptions(reserved=1)


def test_no_gpu_fails_loudly_with_sa40(lib):
    import torch
    if torch.cuda.device_count() > 0:
        pytest.skip("GPU present")
    import compseed_amd as ca
    ix = ca.Index.load(_data.PREFIX)
    with pytest.raises(ca.CSError) as ei:
        ca.Engine(ix, 0, sa40=1)
    assert ei.value.code == -4
    ix.close()


def test_memory_rejects_null(lib):
    import compseed_amd.binding as b
    assert lib.cs_engine_memory(None, ctypes.byref(b.Memory())) == -1
