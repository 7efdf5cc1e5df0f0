"""tests/golden/aln2 (tests/golden/make_golden.py aln2): the reference's extension stage and mem_sort_dedup_patch where aln1 / ddp1 do not
reach -- non-default scoring, band and Z-drop (params.*), the ends of the contigs and their join (ends), reads of exactly 63, 64 and 65
regions (cap64).  One loader for the tests that use the sets; each set carries the cs_aln_params_t fields the reference ran with."""
import functools
import json
import os

import numpy as np

import _data

DIR = os.path.join(os.path.dirname(_data.GOLD), "aln2")
MANIFEST = json.load(open(os.path.join(DIR, "MANIFEST.json")))
SETS = sorted(MANIFEST["sets"])
PARAM_SETS = [s for s in SETS if s.startswith("params.")]
REG_FIELDS = ("rb", "re", "qb", "qe", "rid", "score", "truesc", "w", "seedcov", "seedlen0", "frac_rep", "chain")


def aln_params(name, **kw):
    """the set's scoring as an AlnParams (kw: flags, ...)"""
    import compseed_amd as ca
    return ca.AlnParams(**dict(MANIFEST["sets"][name]["aln_params"], **kw))


@functools.lru_cache(maxsize=None)
def reads(name):
    raw = open(os.path.join(DIR, MANIFEST["sets"][name]["reads"]), "rb").read()
    return _data.pack_reads(raw.split(b"\n")[:-1])


@functools.lru_cache(maxsize=None)
def npz(name, kind):
    """kind: aln (filtered chains in, regions out), ddp (regions after mem_sort_dedup_patch), chains (unfiltered chains; params.* only)"""
    z = np.load(os.path.join(DIR, "%s.%s.npz" % (name, kind)))
    return {k: z[k] for k in z.files}


def chains_in(z):
    """the .aln.npz chains as cs_extend_chains takes them: chain_off, chains, cseed_off, cseeds, cseed_score"""
    import compseed_amd as ca
    n_chains = z["chain_pos"].size
    chains = np.zeros(n_chains, dtype=ca.CHAIN_DT)
    chains["pos"], chains["rid"], chains["n_seeds"], chains["frac_rep"], chains["is_alt"] = z["chain_pos"], z["chain_rid"], z["chain_n"], z["chain_frac_rep"], z["chain_is_alt"]
    cseed_off = np.zeros(n_chains + 1, dtype=np.uint64); np.cumsum(z["chain_n"].astype(np.uint64), out=cseed_off[1:])
    cseeds = np.zeros(z["cseed_rbeg"].size, dtype=ca.SEED_DT)
    cseeds["rbeg"], cseeds["qbeg"], cseeds["len"] = z["cseed_rbeg"], z["cseed_qbeg"], z["cseed_len"]
    return z["chain_off"].astype(np.uint64), chains, cseed_off, cseeds, z["cseed_score"].astype(np.int32)


def regions(z):
    """the .aln.npz regions as cs_alnreg_t records"""
    import compseed_amd as ca
    regs = np.zeros(z["reg_rb"].size, dtype=ca.ALNREG_DT)
    for f in REG_FIELDS:
        regs[f] = z["reg_" + f]
    return z["reg_off"].astype(np.uint64), regs
