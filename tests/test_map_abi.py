"""cs_mapper_t without a GPU: the parameter struct and its split into the stages' structs, the errors of cs_mapper_create in their documented
order, and the NULL-mapper errors of the calls."""
import ctypes as C
import os
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


def _fields(s):
    return {n: getattr(s, n) for n, _ in s._fields_}


def test_default_split_equals_each_stages_own_default(lib):
    import compseed_amd as ca
    got = ca.map_params_split(ca.MapParams())
    own = dict(seed=ca.Params(k=1, r=9, s=9, c=9, y=9, want_sal=0, sst_mode=0, disable=7, result_flags=1), chain=ca.ChainParams(1, 1, 1, 1), flt=ca.FltParams(a=9, mask_level=0.1),
               aln=ca.AlnParams(a=9, threads=3, flags=1), dedup=ca.DedupParams(1, 0.1), mark=ca.MarkParams(T=1, mapq_coef_len=1, xa_drop_ratio=0.1))
    for key, fn in (("seed", lib.cs_params_default), ("chain", lib.cs_chain_params_default), ("flt", lib.cs_flt_params_default), ("aln", lib.cs_aln_params_default),
                    ("dedup", lib.cs_dedup_params_default), ("mark", lib.cs_mark_params_default)):
        fn(C.byref(own[key]))                                               # the stage's own *_default over a struct filled with other values
        assert _fields(got[key]) == _fields(own[key]), key
    assert got["mark_flags"] == 0 and got["sam"].flags == 0 and got["sam"].rg_id is None


def test_fields_several_stages_read_reach_each_of_them(lib):
    import compseed_amd as ca
    p = ca.MapParams(min_seed_len=23, max_occ=77, max_chain_gap=1234, mask_level=0.25, drop_ratio=0.75, a=2, b=5, o_del=7, e_del=3, o_ins=8, e_ins=4, w=55, T=41, threads=5, rg_id="g1")
    s = ca.map_params_split(p)
    assert (s["seed"].min_seed_len, s["chain"].min_seed_len, s["flt"].min_seed_len, s["mark"].min_seed_len) == (23, 23, 23, 23)
    assert (s["seed"].max_occ, s["chain"].max_occ) == (77, 77)
    assert (s["chain"].max_chain_gap, s["flt"].max_chain_gap, s["dedup"].max_chain_gap) == (1234, 1234, 1234)
    assert (s["flt"].mask_level, s["mark"].mask_level, s["flt"].drop_ratio, s["mark"].drop_ratio) == (0.25, 0.25, 0.75, 0.75)
    for k in ("flt", "aln"):
        assert tuple(getattr(s[k], f) for f in ("a", "b", "o_del", "e_del", "o_ins", "e_ins")) == (2, 5, 7, 3, 8, 4), k
    assert (s["chain"].w, s["aln"].w, s["mark"].T, s["aln"].threads, s["sam"].rg_id) == (55, 55, 41, 5, b"g1")
    assert (s["seed"].sst_mode, s["seed"].disable, s["seed"].result_flags, s["seed"].want_sal) == (1, 0, 0, 1)   # the engine-side knobs stay at their defaults


@pytest.mark.parametrize("bit,mark_flags,sam_flags", [("MAP_ALL", "MARK_ALL", 0), ("MAP_NO_MULTI", "MARK_NO_MULTI", 0), ("MAP_KEEP_SUPP_MAPQ", "MARK_KEEP_SUPP_MAPQ", 0), ("MAP_SOFTCLIP", None, 1)])
def test_the_four_flag_bits_one_at_a_time(lib, bit, mark_flags, sam_flags):
    import compseed_amd as ca
    s = ca.map_params_split(ca.MapParams(flags=getattr(ca, bit)))
    assert s["mark_flags"] == (getattr(ca, mark_flags) if mark_flags else 0) and s["sam"].flags == (ca.SAM_SOFTCLIP if sam_flags else 0)


def test_split_refuses_null(lib):
    assert lib.cs_map_params_split(None, None, None, None, None, None, None, None, None) == -1


def _create(lib, prefix, device, par):
    h = C.c_void_p(0xdead)
    rc = lib.cs_mapper_create(prefix, device, None, C.byref(par) if par is not None else None, C.byref(h))
    assert rc != 0 and not h.value                                          # *out is NULL after every error
    return rc


def test_create_errors_in_their_documented_order(lib, tmp_path):
    import compseed_amd as ca
    import torch
    good, nowhere = os.fsencode(_data.PREFIX), os.fsencode(str(tmp_path / "nope"))
    assert lib.cs_mapper_create(good, 0, None, None, None) == -1            # a NULL out
    assert _create(lib, None, 0, None) == -1 and _create(lib, good, -1, None) == -1
    res = ca.MapParams(); res.reserved[2] = 1
    # each bad parameter set is refused as CS_EINVAL even where the index is missing too: the parameters are looked at first
    for bad in (res, ca.MapParams(flags=16), ca.MapParams(pen_clip5=4), ca.MapParams(mapq_coef_len=0), ca.MapParams(a=0), ca.MapParams(e_ins=0), ca.MapParams(w=0),
                ca.MapParams(max_chain_extend=0), ca.MapParams(mask_level_redun=0.0), ca.MapParams(min_seed_len=0)):
        assert _create(lib, nowhere, 0, bad) == -1
    bad_both = ca.MapParams(flags=16, pen_clip5=4); bad_both.reserved[0] = 1
    assert _create(lib, nowhere, 0, bad_both) == -1 and b"reserved" in lib.cs_last_error()   # reserved before the flags, the flags before the clips
    assert _create(lib, nowhere, 0, ca.MapParams(flags=16, pen_clip5=4)) == -1 and b"flags" in lib.cs_last_error()
    assert _create(lib, nowhere, 0, None) == -2                            # index files missing: CS_EIO, with or without a GPU
    for ext in ("bwt", "sa", "ann"):                                        # ... any of them: here .pac is not there
        os.symlink(_data.PREFIX + "." + ext, str(tmp_path / ("part." + ext)))
    assert _create(lib, os.fsencode(str(tmp_path / "part")), 0, None) == -2
    if torch.cuda.device_count() == 0:
        assert _create(lib, good, 0, None) == -4                            # a valid prefix and device 0 without a GPU: CS_EDEVICE
        assert _create(lib, good, 0, ca.MapParams(a=2, b=3)) == -4


def test_calls_on_a_null_mapper(lib):
    import compseed_amd as ca
    out = ca.binding.CSamResult(); st = ca.MapStats(); need = C.c_size_t()
    assert lib.cs_map_batch(None, 0, None, None, None, None, None, None, None, 0, C.byref(out)) == -1
    assert lib.cs_mapper_header(None, None, None, 0, C.byref(need)) == -1
    assert lib.cs_mapper_stats(None, C.byref(st)) == -1 and lib.cs_mapper_engine_stats(None, C.byref(ca.Stats())) == -1
    lib.cs_mapper_destroy(None)                                             # null-safe


def test_ctypes_mirrors_match_the_header(lib, tmp_path):
    """sizeof / offsetof of the new structs as gcc sees them == the ctypes mirrors"""
    import compseed_amd.binding as b
    structs = {"cs_map_params_t": b.MapParams, "cs_map_stats_t": b.MapStats, "cs_read_chunk_t": b.CReadChunk}
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "compseed_amd.h"', 'int main(void) {', 'printf("stages %d\\n", (int)CS_MAP_N_STAGES);']
    for cname, st in structs.items():
        src.append('printf("%s %%zu\\n", sizeof(%s));' % (cname, cname))
        src += ['printf("%s.%s %%zu\\n", offsetof(%s, %s));' % (cname, f, cname, f) for f, _ in st._fields_]
    src.append("return 0; }")
    (tmp_path / "abi.c").write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "abi"), str(tmp_path / "abi.c")], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "abi")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["stages"]) == len(b.MAP_STAGES) == 11
    for cname, st in structs.items():
        assert int(got[cname]) == C.sizeof(st), cname
        for f, _ in st._fields_:
            assert int(got["%s.%s" % (cname, f)]) == getattr(st, f).offset, (cname, f)
