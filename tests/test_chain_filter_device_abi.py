"""CPU-side checks of the device chain filter's C ABI (cs_chain_filter_device, cs_chain_filter_gpu, cs_chain_filter_stats): declared and
exported, cs_flt_stats_t as gcc lays it out == the ctypes mirror, a host-only chainer refused by both calls, bad arguments refused, no
crash without a GPU.  The GPU behaviour is in tests/test_gpu_chain_filter_device.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _data
from test_chain import golden_chains
from test_chain_filter import _chains_in

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cs_chain_filter_device", "cs_chain_filter_gpu", "cs_chain_filter_stats"]
ZERO = dict(reads=0, chains_in=0, chains_out=0, seeds_in=0, seeds_out=0, wave_reads=0, spill_reads=0, sw_seeds=0, launches=0, kernel_ms=0.0)


@pytest.fixture(scope="module")
def lib():
    import compseed_amd as ca
    if not os.path.exists(ca.lib_path()):
        ca.build_library()
    return ca.load_library()


def _gpu_visible():
    try:
        import torch
        return torch.cuda.device_count() > 0
    except Exception:
        return False


def test_new_symbols_are_declared_and_exported(lib):
    import compseed_amd as ca
    import compseed_amd.binding as b
    hdr = open(os.path.join(ROOT, "include", "compseed_amd.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in b.SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+CS_FLT_WAVE_ONLY\s+1u", hdr) and b.FLT_WAVE_ONLY == 1 and ca.FLT_WAVE_ONLY == 1
    for m in ("filter_gpu", "filter_device", "filter_stats"):
        assert callable(getattr(ca.Chainer, m))


def test_flt_stats_layout_matches_the_header(lib, tmp_path):
    import compseed_amd.binding as b
    names = [f for f, _ in b.FltStats._fields_]
    assert names == ["reads", "chains_in", "chains_out", "seeds_in", "seeds_out", "wave_reads", "spill_reads", "sw_seeds", "launches", "kernel_ms"]
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "compseed_amd.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(cs_flt_stats_t));']
    src += ['printf("%s %%zu\\n", offsetof(cs_flt_stats_t, %s));' % (f, f) for f in names] + ["return 0; }"]
    c = tmp_path / "st.c"
    c.write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "st"), str(c)], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "st")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(b.FltStats) == 80
    for f in names:
        assert int(got[f]) == getattr(b.FltStats, f).offset, f


def test_create_device_without_gpu_is_edevice(lib):
    """the device filter hangs on cs_chainer_create_device: CS_EDEVICE without a GPU (with one: a chainer whose filter counters start at zero)"""
    import compseed_amd as ca
    if _gpu_visible():
        c = ca.Chainer(_data.PREFIX, device=0)
        assert c.filter_stats() == ZERO
        c.close()
        return
    with pytest.raises(ca.CSError) as ei:
        ca.Chainer(_data.PREFIX, device=0)
    assert ei.value.code == -4


def _cin(args):
    import compseed_amd as ca
    chain_off, chains, cseed_off, cseeds = args
    chain_off = np.ascontiguousarray(chain_off, dtype=np.uint64); cseed_off = np.ascontiguousarray(cseed_off, dtype=np.uint64)
    keep = (chain_off, chains, cseed_off, cseeds)
    return ca.binding.CChainResult(chain_off.size - 1, chains.size, cseeds.size, chain_off.ctypes.data, chains.ctypes.data, cseed_off.ctypes.data, cseeds.ctypes.data), keep


def test_device_filter_calls_refuse_a_host_chainer(lib):
    import compseed_amd as ca
    zc = golden_chains("main100", "default")
    bases, off = _data.load_reads("main100")
    c = ca.Chainer(_data.PREFIX)
    with pytest.raises(ca.CSError) as ei:
        c.filter_gpu(*_chains_in(zc), bases, off)
    assert ei.value.code == -1
    cin, _keep = _cin(_chains_in(zc))
    out = ca.binding.CChainResult(); sc = ctypes.c_void_p()
    par = ca.FltParams()
    for fn in (lib.cs_chain_filter_device, lib.cs_chain_filter_gpu):
        assert fn(c._h, ctypes.byref(par), ctypes.byref(cin), bases.ctypes.data, off.ctypes.data, 0, ctypes.byref(out), ctypes.byref(sc)) == -1
    assert c.filter_stats() == ZERO
    got = c.filter(*_chains_in(zc), bases, off, threads=2)         # the host filter of the same chainer is unaffected
    assert 0 < got["chains"].size < zc["pos"].size
    c.close()


def test_null_arguments_and_unknown_flags_are_einval(lib):
    import compseed_amd as ca
    zc = golden_chains("main100", "default")
    bases, off = _data.load_reads("main100")
    c = ca.Chainer(_data.PREFIX)
    cin, _keep = _cin(_chains_in(zc))
    out = ca.binding.CChainResult(); sc = ctypes.c_void_p()
    par = ca.FltParams()
    P, I, O = ctypes.byref(par), ctypes.byref(cin), ctypes.byref(out)
    for fn in (lib.cs_chain_filter_device, lib.cs_chain_filter_gpu):
        assert fn(None, P, I, bases.ctypes.data, off.ctypes.data, 0, O, ctypes.byref(sc)) == -1
        assert fn(c._h, None, I, bases.ctypes.data, off.ctypes.data, 0, O, ctypes.byref(sc)) == -1
        assert fn(c._h, P, None, bases.ctypes.data, off.ctypes.data, 0, O, ctypes.byref(sc)) == -1
        assert fn(c._h, P, I, bases.ctypes.data, off.ctypes.data, 0, None, ctypes.byref(sc)) == -1
        assert fn(c._h, P, I, bases.ctypes.data, None, 0, O, ctypes.byref(sc)) == -1
        assert fn(c._h, P, I, bases.ctypes.data, off.ctypes.data, 2, O, ctypes.byref(sc)) == -1
        assert fn(c._h, P, I, bases.ctypes.data, off.ctypes.data, 0x80000001, O, ctypes.byref(sc)) == -1
    st = ca.binding.FltStats()
    assert lib.cs_chain_filter_stats(None, ctypes.byref(st)) == -1 and lib.cs_chain_filter_stats(c._h, None) == -1
    assert lib.cs_chain_filter_stats(c._h, ctypes.byref(st)) == 0 and st.reads == 0 and st.kernel_ms == 0.0
    c.close()
