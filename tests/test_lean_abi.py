"""CPU-side checks of the lean-result ABI (CS_RESULT_LEAN, CS_MEM_LEAN8): struct layout as gcc sees it against the ctypes mirrors,
the defaults, and cs_unpack_mem / cs_mem_seed_count on hand-made 8-byte mems, compiled as C."""
import ctypes
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


@pytest.fixture(scope="module")
def lib():
    import compseed_amd as ca
    if not os.path.exists(ca.lib_path()):
        ca.build_library()
    return ca.load_library()


def _run_c(tmp_path, name, body):
    c = tmp_path / (name + ".c")
    c.write_text("\n".join(['#include <stdio.h>', '#include <stddef.h>', '#include <string.h>', '#include "compseed_amd.h"', 'int main(void) {'] + body + ["return 0; }"]))
    exe = tmp_path / name
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", INC, "-o", str(exe), str(c)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout


def test_params_and_mem8_layout_match_the_header(tmp_path):
    """sizeof / offsetof of cs_params_t and cs_mem8_t as gcc sees them == the ctypes / numpy mirrors; the two new fields lie behind
    count_traffic and the struct has no tail padding"""
    import compseed_amd.binding as b
    body = ['printf("cs_params_t %zu\\n", sizeof(cs_params_t));']
    body += ['printf("cs_params_t.%s %%zu\\n", offsetof(cs_params_t, %s));' % (f, f) for f, _ in b.Params._fields_]
    body += ['printf("cs_mem8_t %zu\\n", sizeof(cs_mem8_t));', 'printf("cs_mem8_t.w %zu\\n", offsetof(cs_mem8_t, w));',
             'printf("CS_RESULT_LEAN %u\\n", (unsigned)CS_RESULT_LEAN);', 'printf("CS_MEM_LEAN8 %d\\n", (int)CS_MEM_LEAN8);']
    got = dict(l.split() for l in _run_c(tmp_path, "layout", body).splitlines())
    assert int(got["cs_params_t"]) == ctypes.sizeof(b.Params)
    for f, _ in b.Params._fields_:
        assert int(got["cs_params_t." + f]) == getattr(b.Params, f).offset, f
    names = [f for f, _ in b.Params._fields_]
    assert names[-3:] == ["count_traffic", "result_flags", "reserved"]
    assert b.Params.result_flags.offset == b.Params.count_traffic.offset + 4 and b.Params.reserved.offset == b.Params.result_flags.offset + 4
    assert ctypes.sizeof(b.Params) == b.Params.reserved.offset + 4                      # no hidden tail padding
    assert int(got["cs_mem8_t"]) == b.MEM8_DT.itemsize == 8 and int(got["cs_mem8_t.w"]) == b.MEM8_DT.fields["w"][1] == 0
    assert int(got["CS_RESULT_LEAN"]) == b.RESULT_LEAN == 1 and int(got["CS_MEM_LEAN8"]) == b.MEM_LEAN8 == 2
    assert (b.MEM_FULL32, b.MEM_PACKED16) == (0, 1)


def test_params_default_clears_the_new_fields(lib):
    import compseed_amd as ca
    p = ca.Params()
    p.result_flags, p.reserved = 7, 9
    lib.cs_params_default(p)
    assert p.result_flags == 0 and p.reserved == 0
    assert (p.min_seed_len, p.max_occ, p.want_sal, p.count_traffic) == (19, 500, 1, 0)
    assert ca.Params(result_flags=ca.RESULT_LEAN).result_flags == 1 and ca.Params(result_flags=ca.RESULT_LEAN).reserved == 0
    assert ca.Params().result_flags == 0


# (x2, beg, end): x2 = 1, 2^31, 2^33; beg 0; end 32767; every field at its maximum at once
CASES = [(1, 0, 19), (1 << 31, 5, 150), (1 << 33, 100, 32767), (7, 0, 32767), ((1 << 34) - 1, 32767, 32767), (499, 12, 31), (500, 12, 31), (501, 12, 31)]


def test_unpack_mem_lean8_in_c(tmp_path):
    """a C program packs the cases as the header's comment says (w = x2 | beg << 34 | end << 49), unpacks them with cs_unpack_mem and
    counts their seeds with cs_mem_seed_count: x0 == x1 == 0, x2 and info exact"""
    import numpy as np
    import compseed_amd.binding as b
    body = ["cs_mem8_t m[%d]; cs_packed_result_t r; cs_intv_t v; memset(&r, 0, sizeof r); memset(&v, 0xff, sizeof v);" % len(CASES)]
    for i, (x2, beg, end) in enumerate(CASES):
        body.append("m[%d].w = %dull | %dull << 34 | %dull << 49;" % (i, x2, beg, end))
    body += ["r.mem_format = CS_MEM_LEAN8; r.mems = m; r.n_mems = %d; r.max_occ = 500;" % len(CASES),
             "for (int i = 0; i < %d; ++i) { memset(&v, 0xff, sizeof v); cs_unpack_mem(&r, (uint64_t)i, &v);" % len(CASES),
             'printf("%llu %llu %llu %llu %u %u\\n", (unsigned long long)v.x0, (unsigned long long)v.x1, (unsigned long long)v.x2, (unsigned long long)v.info,',
             "       cs_mem_seed_count(&v, r.max_occ), cs_mem_seed_count(&v, 3)); }"]
    rows = [[int(x) for x in l.split()] for l in _run_c(tmp_path, "unpack8", body).splitlines()]
    assert len(rows) == len(CASES)
    for (x2, beg, end), (x0, x1, gx2, info, c500, c3) in zip(CASES, rows):
        assert x0 == 0 and x1 == 0 and gx2 == x2 and info == (beg << 32 | end), (x2, beg, end)
        assert c500 == min(x2, 500) and c3 == min(x2, 3)
    # the numpy restatement the GPU tests use agrees with the header
    w = np.array([x2 | beg << 34 | end << 49 for x2, beg, end in CASES], dtype=np.uint64).view(b.MEM8_DT)
    u = b.unpack_mems8(w)
    assert not u["x0"].any() and not u["x1"].any()
    assert u["x2"].tolist() == [c[0] for c in CASES] and u["info"].tolist() == [c[1] << 32 | c[2] for c in CASES]


def test_other_formats_still_unpack_in_c(tmp_path):
    """the third format leaves the first two as they were"""
    body = ["cs_mem16_t p; cs_intv_t f = {11, 22, 33, (5ull << 32) | 44}, v; cs_packed_result_t r; memset(&r, 0, sizeof r);",
            "p.w0 = 11ull | (33ull & 0x7fffffffull) << 33; p.w1 = 22ull | 5ull << 33 | 44ull << 48 | (33ull >> 31) << 63;",
            "r.mem_format = CS_MEM_PACKED16; r.mems = &p; cs_unpack_mem(&r, 0, &v);",
            'printf("%llu %llu %llu %llu\\n", (unsigned long long)v.x0, (unsigned long long)v.x1, (unsigned long long)v.x2, (unsigned long long)v.info);',
            "r.mem_format = CS_MEM_FULL32; r.mems = &f; cs_unpack_mem(&r, 0, &v);",
            'printf("%llu %llu %llu %llu\\n", (unsigned long long)v.x0, (unsigned long long)v.x1, (unsigned long long)v.x2, (unsigned long long)v.info);']
    rows = [[int(x) for x in l.split()] for l in _run_c(tmp_path, "unpack16", body).splitlines()]
    assert rows == [[11, 22, 33, (5 << 32) | 44]] * 2
