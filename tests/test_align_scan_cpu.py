"""The extension stage without a GPU (tests/cpp/align_scan_check.cpp): the bodies that the kernels of align_gpu.hip loop over
(compseed_amd/csrc/align_scan.hpp) driven by a plain C++ program in the order extend_core_ launches the kernels -- checks, chain_read,
queries, windows, an exclusive sum, fill, regions, the left side with its second try at 2w, right_h0, the right side, seed coverage, the
purge -- with the dynamic programming done by the CPU restatement of the reference's extension (oracle/cs_bsw_oracle.c, compiled with gcc
and linked into the program here; rule 3 for the pairs of the vector class, else 0: what extend.hip applies under CS_EXT_VECTOR_ZDROP).
What tests/test_gpu_align.py asserts of the GPU stage is asserted of the program's output: reg_off, the purged mask, all of rb re qb qe
rid score truesc w seedcov seedlen0 chain, frac_rep bit for bit and the purge's count, against the reference's own regions
(tests/golden/aln1, flt1, ddp1, aln2) with no region excluded.  One lane over the seven aln1 / flt1 / ddp1 sets and the eight aln2 sets
with their own scoring, whole sets all of them; 64 lanes on lockstep threads over cap64 (reads of exactly 63, 64 and 65 regions: the
all-lanes mask of purge_read_regs<64> and the first read for purge_read_mem<64>) and ragged, 8 lanes over ends.  Lanes that part ways
never finish: each lockstep run has a time limit.  The bodies must refuse every class of inconsistent input before anything follows an
offset (one hand-made case each: two reads, three chains)."""
import os
import subprocess

import numpy as np
import pytest

import _aln2
import _data
from test_gpu_align import _load

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "align_scan_check.cpp")
BSW = os.path.join(os.path.dirname(HERE), "oracle", "cs_bsw_oracle.c")
FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "chain")
ALN1 = ["main100", "sorted150", "ragged", "repeat100", "indel150_400", "long90", "gap3k"]
MAX_READ_LEN = 65536
NO_LIGHT_PATHS, PURGE_FROM_HBM = 1, 2                                       # CS_ALN_* of cs_aln_params_t.flags


@pytest.fixture(scope="module")
def exes(tmp_path_factory):
    """the one-lane program and its 64- and 8-lane builds, over one object of the extension's CPU restatement"""
    d = tmp_path_factory.mktemp("align_scan")
    obj = str(d / "cs_bsw_oracle.o")
    c = subprocess.run(["gcc", "-std=c99", "-O2", "-Wall", "-c", "-o", obj, BSW], capture_output=True, text=True)
    assert c.returncode == 0, c.stderr
    out = {}
    for lanes in (1, 64, 8):
        out[lanes] = str(d / ("align_scan_check_%d" % lanes))
        c = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", "-pthread", *(["-DCS_EMU_W=%d" % lanes] if lanes > 1 else []), "-o", out[lanes], SRC, obj],
                           capture_output=True, text=True)
        assert c.returncode == 0 and not c.stderr, c.stderr                  # (no warnings either)
    return out


def _write(d, chain_off, chains, cseed_off, cseeds, score, bases, off, params):
    import compseed_amd as ca
    assert chains.dtype == ca.CHAIN_DT and cseeds.dtype == ca.SEED_DT
    ann = open(_data.PREFIX + ".ann").read().split("\n")
    l_pac, n_ctg = int(ann[0].split()[0]), int(ann[0].split()[1])
    ctg = np.array([[int(x) for x in ann[2 + 2 * k].split()[:2]] for k in range(n_ctg)], np.int64)
    pac = np.fromfile(_data.PREFIX + ".pac", np.uint8)[:(l_pac + 3) // 4]
    meta = np.array([off.size - 1, chains.size, cseeds.size, l_pac], np.int64)
    os.makedirs(str(d), exist_ok=True)
    for name, arr in (("meta", meta), ("par", np.frombuffer(bytes(params), np.uint8)), ("chain_off", chain_off.astype(np.uint64)), ("chains", chains),
                      ("cseed_off", cseed_off.astype(np.uint64)), ("cseeds", cseeds), ("score", score.astype(np.int32)), ("read_off", off.astype(np.uint64)), ("bases", bases),
                      ("pac", pac), ("ctg_off", ctg[:, 0]), ("ctg_len", ctg[:, 1].astype(np.int32))):
        np.ascontiguousarray(arr).tofile(os.path.join(str(d), name + ".bin"))


def _set(name):
    """a golden set as the program takes it: the chains the reference fed into the stage, the reads, and the regions it left"""
    if name in _aln2.SETS:
        z = _aln2.npz(name, "aln")
        bases, off = _aln2.reads(name)
    else:
        z, bases, off = _load(name)
    return _aln2.chains_in(z), bases, off, z


def _check(exe, d, name, lanes=1, flags=0, timeout=600):
    import compseed_amd as ca
    cin, bases, off, z = _set(name)
    params = _aln2.aln_params(name, flags=flags) if name in _aln2.SETS else ca.AlnParams(flags=flags)
    _write(d, *cin, bases, off, params)
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda n, dt: np.fromfile(os.path.join(str(d), n + ".bin"), dt)
    g, st = rd("out_regs", ca.ALNREG_DT), [int(x) for x in rd("out_stat", np.uint64)]
    st = dict(zip(("left", "right", "retries", "purged", "long_chains", "by_regs", "by_mem", "in_cap"), st))
    assert np.array_equal(rd("out_reg_off", np.uint64), z["reg_off"])
    purged = (z["reg_qb"] == -1) & (z["reg_qe"] == -1)
    bad = {f: int((g[f] != z["reg_" + f]).sum()) for f in FIELDS}
    bad["frac_rep"] = int((g["frac_rep"].view(np.uint32) != z["reg_frac_rep"].view(np.uint32)).sum())
    print("%s, %d lanes, flags %d: %d regions, purged %d (reference %d), %s, fields that differ: %s" % (name, lanes, flags, g.size, st["purged"], int(purged.sum()), st,
                                                                                                      {k: v for k, v in bad.items() if v} or "none"))
    assert np.array_equal((g["qb"] == -1) & (g["qe"] == -1), purged), (name, int(((g["qb"] == -1) & (g["qe"] == -1)).sum()), int(purged.sum()))
    for f in FIELDS:
        assert np.array_equal(g[f], z["reg_" + f]), (name, f, bad[f])
    assert np.array_equal(g["frac_rep"].view(np.uint32), z["reg_frac_rep"].view(np.uint32))
    assert st["purged"] == int(purged.sum())
    # which form took what, as extend_core_ sends it
    sd = cin[3]
    per_chain, per_read = z["chain_n"].astype(np.int64), np.diff(z["reg_off"].astype(np.int64))
    small_chain, light_max = (0, 1) if flags & NO_LIGHT_PATHS else (8, 64)
    regs_max = min(lanes, light_max) if lanes > 1 else 0
    assert st["left"] == int((sd["qbeg"] != 0).sum()) and st["right"] <= g.size and st["left"] + st["right"] >= g.size // 2, st
    assert st["long_chains"] == int((per_chain > small_chain).sum()), st
    assert st["by_regs"] == int(((per_read >= 2) & (per_read <= regs_max)).sum()) and st["by_mem"] == int(((per_read >= 2) & (per_read > regs_max)).sum()), st
    assert st["in_cap"] == int(((per_read >= 2) & (per_read > regs_max) & (per_read <= (0 if flags & PURGE_FROM_HBM else 3000))).sum()), st   # PURGE_CAP
    return g, st, z


@pytest.mark.parametrize("name", ALN1)
def test_one_lane_stage_leaves_the_references_regions(exes, tmp_path, name):
    g, st, z = _check(exes[1], tmp_path, name)
    assert g.size > 4000 and st["purged"] > 1000
    if name == "repeat100":
        assert np.diff(z["reg_off"].astype(np.int64)).max() > 64 and z["chain_n"].max() > 8 and st["long_chains"] > 0


@pytest.mark.parametrize("name", _aln2.SETS)
def test_one_lane_stage_under_other_scoring_and_at_the_edges(exes, tmp_path, name):
    """every aln2 set with the cs_aln_params_t the reference ran with; the params.* sets must see the second try at 2w where the reference did"""
    g, st, z = _check(exes[1], tmp_path, name)
    if not _aln2.MANIFEST["sets"][name]["reference_leaves_no_2w"] and name in _aln2.PARAM_SETS:
        assert st["retries"] > 0


@pytest.mark.parametrize("name,flags", [("ragged", NO_LIGHT_PATHS | PURGE_FROM_HBM), ("cap64", NO_LIGHT_PATHS), ("ends", NO_LIGHT_PATHS | PURGE_FROM_HBM)])
def test_one_lane_stage_with_every_chain_a_long_one(exes, tmp_path, name, flags):
    """CS_ALN_NO_LIGHT_PATHS: every chain through chain_regions<1>"""
    g, st, z = _check(exes[1], tmp_path, name, flags=flags)
    assert st["long_chains"] == z["chain_n"].size


@pytest.mark.parametrize("lanes,name,flags", [(64, "cap64", 0), (64, "cap64", NO_LIGHT_PATHS), (64, "ragged", 0), (8, "ends", 0)])
def test_many_lane_stage_in_lockstep(exes, tmp_path, lanes, name, flags):
    """fill_window<W>, the chain-per-lane regions behind wexcl_sum<W>, chain_regions<W>, purge_read_regs<W> and purge_read_mem<W> on lockstep
    threads.  A ballot or a shuffle is two barriers among the threads; the slowest of these runs (ragged at 64 lanes) took 16 s on eight cores, so
    the time limit, which is there for lanes that part ways, is three minutes."""
    g, st, z = _check(exes[lanes], tmp_path, name, lanes=lanes, flags=flags, timeout=180)
    per_read = np.diff(z["reg_off"].astype(np.int64))
    if name == "cap64" and not flags:
        assert {63, 64, 65} <= set(per_read.tolist()) and st["by_regs"] > 0 and st["by_mem"] > 0
    if flags & NO_LIGHT_PATHS:
        assert st["by_regs"] == 0 and st["long_chains"] == z["chain_n"].size


def _tiny():
    """two reads of 100 bases, three chains (2 + 1) of two, one and one seed"""
    import compseed_amd as ca
    chains = np.zeros(3, ca.CHAIN_DT); chains["n_seeds"] = [2, 1, 1]; chains["pos"] = [1000, 5000, 9000]
    cseeds = np.zeros(4, ca.SEED_DT); cseeds["rbeg"] = [1000, 1040, 5000, 9000]; cseeds["qbeg"] = [0, 40, 10, 20]; cseeds["len"] = [30, 30, 40, 50]
    return [np.array([0, 2, 3], np.uint64), chains, np.array([0, 2, 3, 4], np.uint64), cseeds, cseeds["len"].astype(np.int32)], np.full(200, ord("A"), np.uint8), np.array([0, 100, 200], np.uint64)


def _spoil_chain_off_decreases(cin, bases, off):
    cin[0][1] = 3; cin[0][2] = 2
    return cin, bases, off


def _spoil_chain_off_end(cin, bases, off):
    cin[0][2] = 2                                                            # three chains, the last read ends at two
    return cin, bases, off


def _spoil_n_seeds(cin, bases, off):
    cin[1]["n_seeds"][0] = 3                                                 # cseed_off says 2
    return cin, bases, off


def _spoil_read_off_start(cin, bases, off):
    off[0] = 1
    return cin, bases, off


def _spoil_long_read(cin, bases, off):
    off[2] = off[1] + np.uint64(MAX_READ_LEN)                                # the second read, which has a chain: 65,536 bases
    return cin, np.full(int(off[2]), ord("A"), np.uint8), off


def _spoil_first_seed(cin, bases, off):
    l_pac = int(open(_data.PREFIX + ".ann").readline().split()[0])
    cin[3]["rbeg"][2] = 2 * l_pac + 10                                       # the second chain's first seed: behind both strands
    return cin, bases, off


BAD = {"chain_off_decreases": _spoil_chain_off_decreases, "chain_off_does_not_end_at_n_chains": _spoil_chain_off_end, "n_seeds_disagrees_with_cseed_off": _spoil_n_seeds,
       "read_off_not_from_0": _spoil_read_off_start, "read_of_65536_bases": _spoil_long_read, "first_seed_outside_the_reference": _spoil_first_seed}


def test_tiny_batch_is_accepted_as_it_is(exes, tmp_path):
    import compseed_amd as ca
    cin, bases, off = _tiny()
    _write(tmp_path, *cin, bases, off, ca.AlnParams())
    r = subprocess.run([exes[1], str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    g = np.fromfile(os.path.join(str(tmp_path), "out_regs.bin"), ca.ALNREG_DT)
    assert g.size == 4 and np.array_equal(np.fromfile(os.path.join(str(tmp_path), "out_reg_off.bin"), np.uint64), [0, 3, 4])
    assert np.array_equal(g["seedlen0"], [30, 30, 40, 50]) and np.array_equal(g["chain"], [0, 0, 1, 0])   # (equal scores: the later seed first)


@pytest.mark.parametrize("case", sorted(BAD))
def test_bodies_refuse_inconsistent_input(exes, tmp_path, case):
    import compseed_amd as ca
    cin, bases, off = BAD[case](*_tiny())
    _write(tmp_path, *cin, bases, off, ca.AlnParams())
    r = subprocess.run([exes[1], str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "refused" in r.stderr, (case, r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(tmp_path, "out_regs.bin"))
