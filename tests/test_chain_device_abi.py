"""CPU-side checks of the device chainer's C ABI (cs_chainer_create_device, cs_chain_batch_device, cs_chain_batch_gpu, cs_chainer_stats):
declared and exported, cs_chain_stats_t as gcc lays it out == the ctypes mirror, no crash without a GPU, and a host-only chainer refused by
the device calls.  The GPU behaviour is in tests/test_gpu_chain_device.py."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import _data

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["cs_chainer_create_device", "cs_chain_batch_device", "cs_chain_batch_gpu", "cs_chainer_stats"]


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
    import compseed_amd.binding as b
    hdr = open(os.path.join(ROOT, "include", "compseed_amd.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", hdr))
    for name in NEW:
        assert name in declared and name in b.SYMBOLS, name
        assert hasattr(lib, name), name
    assert re.search(r"#define\s+CS_CHAIN_TREE_ONLY\s+1u", hdr) and b.CHAIN_TREE_ONLY == 1


def test_chain_stats_layout_matches_the_header(lib, tmp_path):
    import compseed_amd.binding as b
    src = ['#include <stdio.h>', '#include <stddef.h>', '#include "compseed_amd.h"', 'int main(void) {', 'printf("size %zu\\n", sizeof(cs_chain_stats_t));']
    src += ['printf("%s %%zu\\n", offsetof(cs_chain_stats_t, %s));' % (f, f) for f, _ in b.ChainStats._fields_] + ["return 0; }"]
    c = tmp_path / "st.c"
    c.write_text("\n".join(src))
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(tmp_path / "st"), str(c)], check=True)
    got = dict(l.split() for l in subprocess.run([str(tmp_path / "st")], capture_output=True, text=True, check=True).stdout.splitlines())
    assert int(got["size"]) == ctypes.sizeof(b.ChainStats)
    for f, _ in b.ChainStats._fields_:
        assert int(got[f]) == getattr(b.ChainStats, f).offset, f


def test_create_device_without_gpu_is_edevice(lib):
    if _gpu_visible():
        pytest.skip("GPU present")
    import compseed_amd as ca
    with pytest.raises(ca.CSError) as ei:
        ca.Chainer(_data.PREFIX, device=0)
    assert ei.value.code == -4
    h = ctypes.c_void_p(123)
    assert lib.cs_chainer_create_device(os.fsencode(_data.PREFIX), 0, ctypes.byref(h)) == -4 and not h.value


def test_device_calls_refuse_a_host_chainer(lib):
    import compseed_amd as ca
    z, _ = _data.load_golden("main100", "default")
    _, off = _data.load_reads("main100")
    mems = np.zeros(z["mems"].shape[0], dtype=ca.INTV_DT)
    mems["x0"], mems["x1"], mems["x2"], mems["info"] = z["mems"][:, 0], z["mems"][:, 1], z["mems"][:, 2], z["mems"][:, 3]
    seeds = np.zeros(z["seed_rbeg"].size, dtype=ca.SEED_DT)
    seeds["rbeg"], seeds["qbeg"], seeds["len"] = z["seed_rbeg"], z["seed_qbeg"], z["seed_len"]
    c = ca.Chainer(_data.PREFIX)
    with pytest.raises(ca.CSError) as ei:
        c.chain_gpu(z["mem_off"], mems, z["seed_off"], seeds, off)
    assert ei.value.code == -1
    mem_off = np.ascontiguousarray(z["mem_off"], dtype=np.uint64); seed_off = np.ascontiguousarray(z["seed_off"], dtype=np.uint64)
    res = ca.binding.CResult(off.size - 1, mems.size, seeds.size, mem_off.ctypes.data, mems.ctypes.data, seed_off.ctypes.data, seeds.ctypes.data)
    out = ca.binding.CChainResult()
    assert lib.cs_chain_batch_device(c._h, ctypes.byref(ca.ChainParams()), ctypes.byref(res), off.ctypes.data, 0, ctypes.byref(out)) == -1
    assert c.stats() == dict(reads=0, seeds=0, chains=0, tree_reads=0, launches=0, kernel_ms=0.0)
    got = c.chain(z["mem_off"], mems, z["seed_off"], seeds, off, threads=2)      # the host path of the same chainer is unaffected
    assert got["chains"].size > 1000
    c.close()
