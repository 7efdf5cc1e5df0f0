"""The device chain filter without a GPU (tests/cpp/chain_filter_scan_check.cpp): the bodies that the kernels of chain_filter_gpu.hip loop
over (compseed_amd/csrc/chain_filter_scan.hpp) driven by a plain C++ program in the kernels' order -- weight, classify, the per-read
filter, the seed test, two exclusive sums, compact.  Byte for byte the host cs_chain_filter and, field by field, the reference's filtered
chains (tests/golden/aln1, flt1, aln2): one lane over the four aln1 sets, the long reads and the sets with other scoring; 64 and 8 lanes on
lockstep threads -- filter_read<W> for every read with chains, the CS_FLT_WAVE_ONLY case -- over repeat100, whose reads of hundreds of
equal-weight chains make the scan take several steps of 64 and let the introsort's tie order decide the output, and 8 lanes over ragged.
Lanes that part ways never finish: each lockstep run has a time limit.  The bodies must refuse every class of inconsistent input before
anything follows an offset (one hand-made case each: two reads, three chains)."""
import os
import subprocess

import numpy as np
import pytest

import _aln2
import _data
from test_chain import golden_chains
from test_chain_filter import ALN, FLT, _chains_in, _long_reads, check_filtered

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "chain_filter_scan_check.cpp")
KEYS = ("chain_off", "chains", "cseed_off", "cseeds", "cseed_score")
MAX_READ_LEN = 65536


def _build(out, *defs):
    c = subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-ffp-contract=off", "-pthread", *defs, "-o", out, SRC], capture_output=True, text=True)
    assert c.returncode == 0 and not c.stderr, c.stderr                      # (no warnings either)
    return out


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    return _build(str(tmp_path_factory.mktemp("chain_filter_scan") / "chain_filter_scan_check"))


@pytest.fixture(scope="module")
def lanes_exe(tmp_path_factory):
    return {n: _build(str(tmp_path_factory.mktemp("chain_filter_scan_%d" % n) / "chain_filter_scan_check"), "-DCS_EMU_W=%d" % n) for n in (64, 8)}


def _write(d, chain_off, chains, cseed_off, cseeds, bases, off, params):
    import compseed_amd as ca
    assert chains.dtype == ca.CHAIN_DT and cseeds.dtype == ca.SEED_DT
    ann = open(_data.PREFIX + ".ann").read().split("\n")
    l_pac, n_ctg = int(ann[0].split()[0]), int(ann[0].split()[1])
    ctg = np.array([[int(x) for x in ann[2 + 2 * k].split()[:2]] for k in range(n_ctg)], np.int64)
    pac = np.fromfile(_data.PREFIX + ".pac", np.uint8)[:(l_pac + 3) // 4]
    meta = np.array([off.size - 1, chains.size, cseeds.size, l_pac], np.int64)
    os.makedirs(str(d), exist_ok=True)
    for name, arr in (("meta", meta), ("par", np.frombuffer(bytes(params), np.uint8)), ("chain_off", chain_off.astype(np.uint64)), ("chains", chains),
                      ("cseed_off", cseed_off.astype(np.uint64)), ("cseeds", cseeds), ("read_off", off.astype(np.uint64)), ("bases", bases), ("pac", pac),
                      ("ctg_off", ctg[:, 0]), ("ctg_len", ctg[:, 1].astype(np.int32))):
        np.ascontiguousarray(arr).tofile(os.path.join(str(d), name + ".bin"))


def _run(exe, d, chains_in, bases, off, params=None, timeout=300):
    import compseed_amd as ca
    _write(d, *chains_in, bases, off, params or ca.FltParams())
    r = subprocess.run([exe, str(d)], capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout + r.stderr
    rd = lambda n, dt: np.fromfile(os.path.join(str(d), n + ".bin"), dt)
    st = rd("out_stat", np.uint64)
    return (dict(chain_off=rd("out_chain_off", np.uint64), chains=rd("out_chains", ca.CHAIN_DT), cseed_off=rd("out_cseed_off", np.uint64), cseeds=rd("out_cseeds", ca.SEED_DT),
                 cseed_score=rd("out_score", np.int32)),
            dict(wave_reads=int(st[0]), slot_reads=int(st[1]), sw_seeds=int(st[2]), chains_out=int(st[3]), seeds_out=int(st[4])))


def _host(chains_in, bases, off, params=None):
    import compseed_amd as ca
    c = ca.Chainer(_data.PREFIX)
    host = c.filter(*chains_in, bases, off, params=params, threads=2)
    c.close()
    return host


def _check(got, stat, host, z, what):
    for k in KEYS:
        assert got[k].dtype == host[k].dtype and got[k].tobytes() == host[k].tobytes(), (what, k)
    check_filtered(got, z)
    assert stat["chains_out"] == got["chains"].size and stat["seeds_out"] == got["cseeds"].size, (what, stat)


def _aln1(name):
    zc = golden_chains(name, "default")
    bases, off = _data.load_reads(name)
    return _chains_in(zc), bases, off, np.load(os.path.join(ALN, name + ".aln.npz"))


@pytest.mark.parametrize("name", ["main100", "repeat100", "sorted150", "ragged"])
def test_one_lane_pass_leaves_the_references_chains(exe, tmp_path, name):
    cin, bases, off, z = _aln1(name)
    got, stat = _run(exe, tmp_path, cin, bases, off)
    _check(got, stat, _host(cin, bases, off), z, name)
    per_read = np.diff(cin[0].astype(np.int64))
    assert stat["wave_reads"] == int((per_read > 16).sum()), (name, stat)   # reads taken by LIGHT_MAX, as the kernels do
    assert stat["slot_reads"] == int((per_read > 512).sum()), (name, stat)


def test_one_lane_pass_runs_the_seed_test_on_long_reads(exe, tmp_path):
    cin = _chains_in(np.load(os.path.join(FLT, "long90.chains.npz")))
    z = np.load(os.path.join(FLT, "long90.aln.npz"))
    bases, off = _long_reads()
    got, stat = _run(exe, tmp_path, cin, bases, off)
    _check(got, stat, _host(cin, bases, off), z, "long90")
    assert stat["sw_seeds"] > 1000, stat
    assert (got["cseed_score"] != got["cseeds"]["len"]).sum() > 1000


@pytest.mark.parametrize("name", _aln2.PARAM_SETS)
def test_one_lane_pass_under_other_scoring(exe, tmp_path, name):
    import compseed_amd as ca
    cin, z = _chains_in(_aln2.npz(name, "chains")), _aln2.npz(name, "aln")
    bases, off = _aln2.reads(name)
    p = _aln2.MANIFEST["sets"][name]["aln_params"]
    params = ca.FltParams(**{k: p[k] for k in ("a", "b", "o_del", "e_del", "o_ins", "e_ins")})
    got, stat = _run(exe, tmp_path, cin, bases, off, params)
    _check(got, stat, _host(cin, bases, off, params), z, name)
    assert stat["sw_seeds"] > 0, (name, stat)


@pytest.mark.parametrize("lanes,name", [(64, "repeat100"), (8, "repeat100"), (8, "ragged")])
def test_many_lane_filter_in_lockstep(lanes_exe, tmp_path, lanes, name):
    """filter_read<W> on lockstep threads for every read with chains: the same bytes as the host call.  A ballot is two barriers among the
    threads, and a read of 500 equal chains takes some 8,500 of them at 64 lanes and 60,000 at 8: repeat100 as a whole runs for about a
    minute, so the time limit, which is there for lanes that part ways, is ten minutes."""
    cin, bases, off, z = _aln1(name)
    kept = np.diff(z["chain_off"].astype(np.int64))
    if name == "repeat100":
        assert kept.max() > 64                                                # the overlap scan takes a second step of 64 kept chains
    got, stat = _run(lanes_exe[lanes], tmp_path, cin, bases, off, timeout=600)
    _check(got, stat, _host(cin, bases, off), z, (name, lanes))
    assert stat["wave_reads"] == int((np.diff(cin[0].astype(np.int64)) > 0).sum()), (name, lanes, stat)


def _tiny():
    """two reads of 100 bases, three chains (2 + 1) of two, one and one seed"""
    import compseed_amd as ca
    chains = np.zeros(3, ca.CHAIN_DT); chains["n_seeds"] = [2, 1, 1]; chains["pos"] = [1000, 5000, 9000]
    cseeds = np.zeros(4, ca.SEED_DT); cseeds["rbeg"] = [1000, 1040, 5000, 9000]; cseeds["qbeg"] = [0, 40, 10, 20]; cseeds["len"] = [30, 30, 40, 50]
    return [np.array([0, 2, 3], np.uint64), chains, np.array([0, 2, 3, 4], np.uint64), cseeds], np.full(200, ord("A"), np.uint8), np.array([0, 100, 200], np.uint64)


def _spoil_empty_chain(cin, bases, off):
    cin[2][2] = cin[2][1]                                                    # cseed_off[c + 1] <= cseed_off[c] for c = 1
    return cin, bases, off


def _spoil_n_seeds(cin, bases, off):
    cin[1]["n_seeds"][0] = 3                                                 # cseed_off says 2
    return cin, bases, off


def _spoil_chain_off(cin, bases, off):
    cin[0][1] = 3; cin[0][2] = 2                                             # chain_off decreases
    return cin, bases, off


def _spoil_long_read(cin, bases, off):
    off[2] = off[1] + np.uint64(MAX_READ_LEN)                                # the second read: 65,536 bases
    return cin, np.full(int(off[2]), ord("A"), np.uint8), off


BAD = {"chain_without_seeds": _spoil_empty_chain, "n_seeds_disagrees_with_cseed_off": _spoil_n_seeds, "chain_off_decreases": _spoil_chain_off, "read_of_65536_bases": _spoil_long_read}


def test_tiny_batch_is_accepted_as_it_is(exe, tmp_path):
    cin, bases, off = _tiny()
    got, stat = _run(exe, tmp_path, cin, bases, off)
    host = _host(cin, bases, off)
    for k in KEYS:
        assert got[k].tobytes() == host[k].tobytes(), k
    assert got["chains"].size == 3


@pytest.mark.parametrize("case", sorted(BAD))
def test_bodies_refuse_inconsistent_input(exe, tmp_path, case):
    import compseed_amd as ca
    cin, bases, off = BAD[case](*_tiny())
    _write(tmp_path, *cin, bases, off, ca.FltParams())
    r = subprocess.run([exe, str(tmp_path)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3 and "refused" in r.stderr, (case, r.returncode, r.stderr)
    assert not os.path.exists(os.path.join(tmp_path, "out_chain_off.bin"))
