"""CPU-side checks of the device extension call's C ABI (cs_extend_chains_device): declared and exported, CS_ALN_DEV_COMPACT in the header
and in the package, the argument checks in the order the header gives them -- with an aligner created with device -1 and host arrays
standing in for the device pointers, which no check dereferences --, no counter moved by a refused call, and the host-side pass of the
same aligner unaffected.  The GPU behaviour is in tests/test_gpu_extend_chains_device.py."""
import ctypes
import os
import re

import numpy as np
import pytest

import _data
from test_dedup import _load as load_regions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import compseed_amd as ca
    if not os.path.exists(ca.lib_path()):
        ca.build_library()
    return ca.load_library()


def test_new_symbol_is_declared_and_exported(lib):
    import compseed_amd as ca
    import compseed_amd.binding as b
    hdr = open(os.path.join(ROOT, "include", "compseed_amd.h")).read()
    declared = set(re.findall(r"\b(cs_[a-z0-9_]+)\s*\(", hdr))
    assert "cs_extend_chains_device" in declared and "cs_extend_chains_device" in b.SYMBOLS
    assert hasattr(lib, "cs_extend_chains_device")
    assert re.search(r"#define\s+CS_ALN_DEV_COMPACT\s+1u", hdr) and b.ALN_DEV_COMPACT == 1 and ca.ALN_DEV_COMPACT == 1
    assert callable(ca.Aligner.extend_chains_device) and callable(ca.download_regions) and callable(b.download_regions)


def _one_chain():
    """a read of 150 bases with one chain of one seed, as host arrays"""
    import compseed_amd as ca
    chains = np.zeros(1, dtype=ca.CHAIN_DT); chains["n_seeds"] = 1; chains["pos"] = 1000
    cseeds = np.zeros(1, dtype=ca.SEED_DT); cseeds["rbeg"], cseeds["qbeg"], cseeds["len"] = 1000, 10, 50
    chain_off, cseed_off = np.array([0, 1], np.uint64), np.array([0, 1], np.uint64)
    bases, off = np.zeros(150, np.uint8), np.array([0, 150], np.uint64)
    score = np.array([50], np.int32)
    cin = ca.binding.CChainResult(1, 1, 1, chain_off.ctypes.data, chains.ctypes.data, cseed_off.ctypes.data, cseeds.ctypes.data)
    return cin, score, bases, off, (chains, cseeds, chain_off, cseed_off)


def test_argument_checks_come_in_the_headers_order(lib):
    import compseed_amd as ca
    al = ca.Aligner(_data.PREFIX, -1)
    cin, score, bases, off, _keep = _one_chain()
    out = ca.binding.CAlnResult()
    I, O, S, B, R = ctypes.byref(cin), ctypes.byref(out), score.ctypes.data, bases.ctypes.data, off.ctypes.data
    fn = lib.cs_extend_chains_device
    assert fn(None, I, S, B, R, 0, O) == -1                      # NULL aligner, chains, out: CS_EINVAL
    assert fn(al.h, None, S, B, R, 0, O) == -1
    assert fn(al.h, I, S, B, R, 0, None) == -1
    assert fn(al.h, I, S, B, R, 2, O) == -1                      # unknown flag bits before the device is asked for
    assert fn(al.h, I, S, B, R, 0x80000001, O) == -1
    assert fn(al.h, I, S, B, None, 0, O) == -1                   # cs_extend_chains' pointer conditions before the device, too
    assert fn(al.h, I, S, None, R, 0, O) == -1
    for flags in (0, ca.ALN_DEV_COMPACT):                        # otherwise valid (the scores may be NULL): CS_EDEVICE for a host-only aligner
        assert fn(al.h, I, S, B, R, flags, O) == -4
        assert fn(al.h, I, None, B, R, flags, O) == -4
    with pytest.raises(ca.CSError) as ei:
        al.extend_chains_device(dict(n_reads=1, n_chains=1, n_seeds=1, chain_off=cin.chain_off, chains=cin.chains, cseed_off=cin.cseed_off, cseeds=cin.cseeds), B, R)
    assert ei.value.code == -4
    st = al.stats()
    assert all(v == 0 for v in st.values()), st
    # the host-side pass of the same aligner is unaffected
    reg_off, regs, rbases, roff, zd = load_regions("sorted150")
    got = al.dedup_regions(reg_off, regs, rbases, roff)
    assert np.array_equal(got["reg_off"], zd["reg_off"]) and np.array_equal(got["n_comp"], zd["reg_n_comp"])
    for f in ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0"):
        assert np.array_equal(got["regs"][f], zd["reg_" + f]), f
    al.close()
