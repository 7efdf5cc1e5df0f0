"""ctypes binding of libcompseed_amd.so (C ABI: include/compseed_amd.h)."""
import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
INTV_DT = np.dtype([("x0", "<u8"), ("x1", "<u8"), ("x2", "<u8"), ("info", "<u8")])   # cs_intv_t == bwtintv_t
SEED_DT = np.dtype([("rbeg", "<i8"), ("qbeg", "<i4"), ("len", "<i4")])               # cs_seed_t

# every symbol include/compseed_amd.h declares (tests check the library exports exactly these)
SYMBOLS = ["cs_last_error", "cs_version", "cs_params_default", "cs_index_load", "cs_index_view", "cs_index_free", "cs_index_build",
           "cs_index_build_flags", "cs_index_save", "cs_refseq_from_fasta", "cs_refseq_codes", "cs_refseq_save", "cs_refseq_free", "cs_index_build_fasta", "cs_reader_open", "cs_reader_next", "cs_reader_close",
           "cs_chainer_create", "cs_chainer_destroy", "cs_chain_params_default", "cs_chain_batch", "cs_flt_params_default", "cs_chain_filter",
           "cs_chainer_create_device", "cs_chain_batch_device", "cs_chain_batch_gpu", "cs_chainer_stats",
           "cs_chain_filter_device", "cs_chain_filter_gpu", "cs_chain_filter_stats",
           "cs_device_count", "cs_engine_options_default", "cs_engine_create", "cs_engine_create_opts", "cs_engine_destroy", "cs_engine_seed_batch",
           "cs_engine_seed_batch_device", "cs_engine_submit_device", "cs_engine_collect_device", "cs_engine_seed_batch_packed", "cs_engine_submit", "cs_engine_collect_packed", "cs_unpack_mem", "cs_mem_seed_count", "cs_host_alloc", "cs_host_free", "cs_pack_reads",
           "cs_engine_result_digest", "cs_engine_gather_reads", "cs_engine_traffic_model", "cs_engine_stats", "cs_engine_reset_stats", "cs_engine_occ4",
           "cs_engine_extend", "cs_engine_sa", "cs_engine_probe_random_lines", "cs_device_alloc", "cs_device_free", "cs_device_upload",
           "cs_device_download", "cs_device_sync", "cs_packed_seed_rbeg", "cs_engine_check_index",
           "cs_ext_params_default", "cs_extender_create", "cs_extender_destroy", "cs_extend_batch", "cs_extend_batch_device", "cs_extender_stats",
           "cs_extender_upload", "cs_extend_batch_resident", "cs_engine_memory", "cs_aln_params_default", "cs_aligner_create", "cs_aligner_destroy", "cs_extend_chains", "cs_extend_chains_device", "cs_dedup_params_default", "cs_dedup_regions", "cs_aligner_stats",
           "cs_regions_cigar", "cs_cigar_stats", "cs_mark_params_default", "cs_regions_mark", "cs_mark_stats",
           "cs_regions_sam", "cs_sam_header", "cs_sam_stats", "cs_reader_next_chunk",
           "cs_map_params_default", "cs_map_params_split", "cs_mapper_create", "cs_mapper_destroy", "cs_map_batch", "cs_mapper_header", "cs_mapper_stats", "cs_mapper_engine_stats",
           "cs_map_submit", "cs_map_collect", "cs_mapper_in_flight"]


class CSError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("compseed_amd error %d: %s" % (code, msg))
        self.code = code


class IndexView(C.Structure):
    _fields_ = [("primary", C.c_uint64), ("L2", C.c_uint64 * 5), ("seq_len", C.c_uint64), ("bwt_size", C.c_uint64),
                ("bwt", C.c_void_p), ("sa_intv", C.c_uint64), ("n_sa", C.c_uint64), ("sa", C.c_void_p)]


class Params(C.Structure):
    """cs_params_t; defaults = mem_opt_init (mapping/comp_seed.cpp:26-58)."""
    _fields_ = [("min_seed_len", C.c_int32), ("split_factor", C.c_float), ("split_width", C.c_int32),
                ("max_occ", C.c_int32), ("max_mem_intv", C.c_uint64), ("want_sal", C.c_int32), ("sst_mode", C.c_int32),
                ("disable", C.c_uint32), ("count_traffic", C.c_uint32), ("result_flags", C.c_uint32), ("reserved", C.c_uint32)]

    def __init__(self, k=19, r=1.5, s=10, c=500, y=20, want_sal=1, sst_mode=1, disable=0, count_traffic=0, result_flags=0):
        super().__init__(k, r, s, c, y, want_sal, sst_mode, disable, count_traffic, result_flags, 0)


RESULT_LEAN = 1   # CS_RESULT_LEAN (cs_params_t.result_flags): the caller reads no x0 / x1 of the mems; x1 = 0 everywhere, packed mems as MEM8_DT
MEM_FULL32, MEM_PACKED16, MEM_LEAN8 = 0, 1, 2   # cs_packed_result_t.mem_format


# cs_params_t.disable bits (include/compseed_amd.h CS_DISABLE_*)
DISABLE = dict(text_mode=0x01, r2_text=0x02, text_sweep=0x04, window=0x08, r3_text=0x10, kmer_filter=0x20, fwd0=0x40, fused_sal=0x80,
               mem_pos=0x100)


def disable_mask(*names):
    m = 0
    for n in names:
        m |= DISABLE[n]
    return m


class EngineOptions(C.Structure):
    """cs_engine_options_t; defaults come from cs_engine_options_default()."""
    _fields_ = [("full_sa", C.c_int32), ("sa64", C.c_int32), ("text_mode", C.c_int32), ("text_arrays", C.c_int32),
                ("jump_k", C.c_int32), ("kmer_filter", C.c_int32), ("fused", C.c_int32), ("mem_cap", C.c_int32),
                ("lep_arena_mb", C.c_int64), ("max_raw_mb", C.c_int64), ("r3_text_iter", C.c_int32),
                ("pipeline_reads", C.c_int32), ("expand_threads", C.c_int32),
                ("count_sal_merged", C.c_int32), ("verbose", C.c_int32), ("host_pack_threads", C.c_int32), ("passes_in_flight", C.c_int32), ("sa40", C.c_int32), ("reserved", C.c_int32 * 2)]

    def __init__(self, **kw):
        super().__init__()
        load_library().cs_engine_options_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_) or k == "reserved":
                raise TypeError("unknown engine option %r" % k)
            setattr(self, k, v)


class CResult(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_mems", C.c_uint64), ("n_seeds", C.c_uint64), ("mem_off", C.c_void_p),
                ("mems", C.c_void_p), ("seed_off", C.c_void_p), ("seeds", C.c_void_p)]


class ChainParams(C.Structure):
    _fields_ = [("w", C.c_int32), ("max_chain_gap", C.c_int32), ("min_seed_len", C.c_int32), ("max_occ", C.c_int32)]

    def __init__(self, w=100, max_chain_gap=10000, k=19, c=500):
        super().__init__(w, max_chain_gap, k, c)


class FltParams(C.Structure):
    """cs_flt_params_t; defaults = mem_opt_init (mapping/comp_seed.cpp:26-58)"""
    _fields_ = [("min_chain_weight", C.c_int32), ("max_chain_extend", C.c_int32), ("max_chain_gap", C.c_int32), ("min_seed_len", C.c_int32),
                ("mask_level", C.c_float), ("drop_ratio", C.c_float), ("a", C.c_int32), ("b", C.c_int32), ("o_del", C.c_int32), ("e_del", C.c_int32),
                ("o_ins", C.c_int32), ("e_ins", C.c_int32)]

    def __init__(self, **kw):
        super().__init__()
        load_library().cs_flt_params_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("no such field: " + k)
            setattr(self, k, v)


class DedupParams(C.Structure):
    """cs_dedup_params_t; defaults = mem_opt_init (mapping/comp_seed.cpp:26-58)"""
    _fields_ = [("max_chain_gap", C.c_int32), ("mask_level_redun", C.c_float)]

    def __init__(self, max_chain_gap=10000, mask_level_redun=0.95):
        super().__init__(max_chain_gap, mask_level_redun)


class CChainResult(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_chains", C.c_uint64), ("n_seeds", C.c_uint64), ("chain_off", C.c_void_p), ("chains", C.c_void_p),
                ("cseed_off", C.c_void_p), ("cseeds", C.c_void_p)]


CHAIN_DT = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("n_seeds", "<i4"), ("frac_rep", "<f4"), ("is_alt", "<i4")])   # cs_chain_t


class CPacked(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_mems", C.c_uint64), ("n_seeds", C.c_uint64), ("mem_format", C.c_int32), ("max_occ", C.c_int32),
                ("mem_off", C.c_void_p), ("mems", C.c_void_p), ("seed_off", C.c_void_p), ("seed_format", C.c_int32), ("reserved", C.c_int32),
                ("seed_rbeg_lo", C.c_void_p), ("seed_rbeg_hi", C.c_void_p)]


MEM16_DT = np.dtype([("w0", "<u8"), ("w1", "<u8")])   # cs_mem16_t


def unpack_mems16(p):
    """numpy restatement of cs_unpack_mem for CS_MEM_PACKED16 records -> INTV_DT array"""
    out = np.zeros(p.size, dtype=INTV_DT)
    m33 = np.uint64((1 << 33) - 1)
    out["x0"] = p["w0"] & m33
    out["x1"] = p["w1"] & m33
    out["x2"] = (p["w0"] >> np.uint64(33)) | ((p["w1"] >> np.uint64(63)) << np.uint64(31))
    out["info"] = (((p["w1"] >> np.uint64(33)) & np.uint64(0x7fff)) << np.uint64(32)) | ((p["w1"] >> np.uint64(48)) & np.uint64(0x7fff))
    return out


MEM8_DT = np.dtype([("w", "<u8")])   # cs_mem8_t


def unpack_mems8(p):
    """numpy restatement of cs_unpack_mem for CS_MEM_LEAN8 records -> INTV_DT array (x0 = x1 = 0)"""
    out = np.zeros(p.size, dtype=INTV_DT)
    w = p["w"]
    out["x2"] = w & np.uint64((1 << 34) - 1)
    out["info"] = (((w >> np.uint64(34)) & np.uint64(0x7fff)) << np.uint64(32)) | ((w >> np.uint64(49)) & np.uint64(0x7fff))
    return out


def unpack_mems(p):
    """the mems of a packed result dict (Engine.seed_batch_packed / collect_packed) as an INTV_DT array, whatever their format"""
    f = p["mem_format"]
    return unpack_mems16(p["mems"]) if f == MEM_PACKED16 else unpack_mems8(p["mems"]) if f == MEM_LEAN8 else p["mems"].copy()


EXT_PAIR_DT = np.dtype([("q_off", "<u8"), ("t_off", "<u8"), ("qlen", "<i4"), ("tlen", "<i4"), ("h0", "<i4"), ("reserved", "<i4")])   # cs_ext_pair_t
EXT_RES_DT = np.dtype([("score", "<i4"), ("qle", "<i4"), ("tle", "<i4"), ("gtle", "<i4"), ("gscore", "<i4"), ("max_off", "<i4")])       # cs_ext_result_t


class ExtParams(C.Structure):
    """cs_ext_params_t: the arguments of the reference's BandedPairWiseSW constructor (mapping/bandedSWA.h:117-121)"""
    _fields_ = [("mat", C.c_int8 * 25), ("o_del", C.c_int32), ("e_del", C.c_int32), ("o_ins", C.c_int32), ("e_ins", C.c_int32),
                ("zdrop", C.c_int32), ("end_bonus", C.c_int32), ("flags", C.c_uint32)]

    def __init__(self, mat=None, o_del=6, e_del=1, o_ins=6, e_ins=1, zdrop=100, end_bonus=5, a=1, b=4, flags=0):
        super().__init__()
        if mat is None:  # bwa_fill_scmat (bwalib/bwa.c:17-29)
            mat = [(-1 if (i == 4 or j == 4) else a if i == j else -b) for i in range(5) for j in range(5)]
        for i in range(25):
            self.mat[i] = int(mat[i])
        self.o_del, self.e_del, self.o_ins, self.e_ins, self.zdrop, self.end_bonus, self.flags = o_del, e_del, o_ins, e_ins, zdrop, end_bonus, flags


ALNREG_DT = np.dtype([("rb", "<i8"), ("re", "<i8"), ("qb", "<i4"), ("qe", "<i4"), ("rid", "<i4"), ("score", "<i4"), ("truesc", "<i4"), ("w", "<i4"),
                      ("seedcov", "<i4"), ("seedlen0", "<i4"), ("frac_rep", "<f4"), ("chain", "<i4")])   # cs_alnreg_t


class AlnParams(C.Structure):
    """cs_aln_params_t: the mem_opt_t fields the extension stage reads (-A -B -O -E -L -w -d)"""
    _fields_ = [(n, C.c_int32) for n in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "pen_clip5", "pen_clip3", "w", "zdrop", "threads")] + [("flags", C.c_uint32)]

    def __init__(self, a=1, b=4, o_del=6, e_del=1, o_ins=6, e_ins=1, pen_clip5=5, pen_clip3=5, w=100, zdrop=100, threads=16, flags=0):
        super().__init__(a, b, o_del, e_del, o_ins, e_ins, pen_clip5, pen_clip3, w, zdrop, threads, flags)


class CAlnResult(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_regs", C.c_uint64), ("reg_off", C.c_void_p), ("regs", C.c_void_p)]


class AlnStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "regions", "pairs", "retries", "purged", "launches", "ext_cells")] + [("ext_kernel_ms", C.c_double)]


# cs_aln_t: a region's alignment (cs_regions_cigar); _pad is the C struct's padding before the two offsets
ALN_DT = np.dtype([("pos", "<i8"), ("rid", "<i4"), ("is_rev", "<i4"), ("score", "<i4"), ("nm", "<i4"), ("n_cigar", "<i4"), ("w", "<i4"), ("tries", "<i4"), ("_pad", "<i4"),
                   ("cigar_off", "<u8"), ("md_off", "<u8")])
CIGAR_SMALL_SCRATCH = 1


class CCigarResult(C.Structure):
    _fields_ = [("n_regs", C.c_uint64), ("n_cigar", C.c_uint64), ("md_bytes", C.c_uint64), ("alns", C.c_void_p), ("cigar", C.c_void_p), ("md", C.c_void_p)]


class CigarStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("regions", "dp_jobs", "nodp_jobs", "retries", "rejected", "cells", "launches")] + [("kernel_ms", C.c_double)]


class MarkParams(C.Structure):
    """cs_mark_params_t: the mem_opt_t fields marking, MAPQ and line selection read; T is the caller's to scale by -A"""
    _fields_ = [(n, C.c_int32) for n in ("T", "mapq_coef_len", "max_xa_hits", "max_xa_hits_alt", "min_seed_len")] + [(n, C.c_float) for n in ("mask_level", "drop_ratio", "xa_drop_ratio")]

    def __init__(self, T=30, mapq_coef_len=50, max_xa_hits=5, max_xa_hits_alt=200, min_seed_len=19, mask_level=0.5, drop_ratio=0.5, xa_drop_ratio=0.8):
        super().__init__(T, mapq_coef_len, max_xa_hits, max_xa_hits_alt, min_seed_len, mask_level, drop_ratio, xa_drop_ratio)


# cs_mark_t: what cs_regions_mark decides about a region
MARK_DT = np.dtype([(n, "<i4") for n in ("reg", "is_alt", "secondary", "secondary_all", "sub", "sub_n", "alt_sc", "mapq", "xs", "flag", "line", "xa_of")])
MARK_ALL, MARK_NO_MULTI, MARK_KEEP_SUPP_MAPQ, MARK_NO_LIGHT_PATH, MARK_FROM_HBM = 1, 2, 4, 0x100, 0x200


class CMarkResult(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_regs", C.c_uint64), ("n_lines", C.c_uint64), ("marks", C.c_void_p), ("line_off", C.c_void_p), ("cigar_regs", CAlnResult), ("cigar_src", C.c_void_p)]


class MarkStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "regions", "lines", "xa_members", "cigar_regions", "light_reads", "wave_reads", "hbm_reads", "launches")] + [("kernel_ms", C.c_double)]


# cs_regions_sam: the SAM text
SAM_SOFTCLIP, SAM_WAVE_ONLY = 1, 0x100


class SamParams(C.Structure):
    _fields_ = [("flags", C.c_uint32), ("rg_id", C.c_char_p)]


class CSamResult(C.Structure):
    _fields_ = [("n_reads", C.c_int64), ("n_lines", C.c_uint64), ("n_bytes", C.c_uint64), ("text_off", C.c_void_p), ("text", C.c_void_p)]


class SamStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "lines", "unmapped", "bytes", "xa_entries", "sa_entries", "launches")] + [("kernel_ms", C.c_double)]


# cs_mapper_t: reads to SAM text in one call
MAP_ALL, MAP_NO_MULTI, MAP_KEEP_SUPP_MAPQ, MAP_SOFTCLIP = 1, 2, 4, 8
MAP_MAX_IN_FLIGHT = 3                                                     # CS_MAP_MAX_IN_FLIGHT
MAP_STAGES = ("upload", "seed", "chain", "filter", "extend", "download", "dedup", "mark", "cigar", "sam", "total")   # CS_MAP_T_*


class MapParams(C.Structure):
    """cs_map_params_t: mem_opt_t as the command line fills it; defaults = cs_map_params_default (mem_opt_init, mapping/comp_seed.cpp:26-58).
    T is the caller's to scale by -A; rg_id: str or bytes, None for no RG tag"""
    _fields_ = [(n, C.c_int32) for n in ("a", "b", "o_del", "e_del", "o_ins", "e_ins", "pen_clip5", "pen_clip3", "w", "zdrop", "T", "min_seed_len")] + \
               [("split_factor", C.c_float), ("split_width", C.c_int32), ("max_occ", C.c_int32), ("max_mem_intv", C.c_uint64)] + \
               [(n, C.c_int32) for n in ("max_chain_gap", "max_chain_extend", "min_chain_weight")] + \
               [(n, C.c_float) for n in ("mask_level", "drop_ratio", "xa_drop_ratio", "mask_level_redun")] + \
               [(n, C.c_int32) for n in ("mapq_coef_len", "max_xa_hits", "max_xa_hits_alt")] + \
               [("flags", C.c_uint32), ("threads", C.c_int32), ("rg_id", C.c_char_p), ("reserved", C.c_uint32 * 4)]

    def __init__(self, **kw):
        super().__init__()
        load_library().cs_map_params_default(C.byref(self))
        for k, v in kw.items():
            if k not in dict(self._fields_):
                raise TypeError("no such field: " + k)
            setattr(self, k, v.encode() if k == "rg_id" and isinstance(v, str) else v)


class MapStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "bases", "regions", "lines", "unmapped", "bytes", "batches")] + [("stage_ms", C.c_double * len(MAP_STAGES))]


class CReadChunk(C.Structure):
    """cs_read_chunk_t"""
    _fields_ = [("n_reads", C.c_int64), ("first_id", C.c_uint64), ("bases", C.c_void_p), ("offsets", C.c_void_p), ("quals", C.c_void_p), ("names", C.c_void_p), ("name_off", C.c_void_p),
                ("comments", C.c_void_p), ("comment_off", C.c_void_p)]


class IndexCheck(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("rows_checked", "order_violations", "isa_violations", "bwt_violations", "sampled_sa_violations", "undecided_rows",
                                          "text_violations")] + [("text_checked", C.c_int32), ("reserved", C.c_int32)]


class ChainStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "seeds", "chains", "tree_reads", "launches")] + [("kernel_ms", C.c_double)]


class FltStats(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reads", "chains_in", "chains_out", "seeds_in", "seeds_out", "wave_reads", "spill_reads", "sw_seeds", "launches")] + [("kernel_ms", C.c_double)]


FLT_WAVE_ONLY = 1     # CS_FLT_WAVE_ONLY: every read through the wave-per-read path of the device chain filter (A/B switch, same results)
CHAIN_TREE_ONLY = 1   # CS_CHAIN_TREE_ONLY: every read through the B-tree path of the device chainer (A/B switch, same results)
EXT_VECTOR_ZDROP = 16   # CS_EXT_VECTOR_ZDROP: Z-drop as the reference's vectorised extension tests it (unpriced diagonal shift, live at zdrop 0)
ALN_DEV_COMPACT = 1   # CS_ALN_DEV_COMPACT: cs_extend_chains_device leaves the purged regions (qe <= qb) behind on the device


class ExtStats(C.Structure):
    _fields_ = [("pairs", C.c_uint64), ("cells", C.c_uint64), ("rows", C.c_uint64), ("launches", C.c_uint64), ("kernel_ms", C.c_double)]


class PackedResult(dict):
    """cs_packed_result_t as a dict of zero-copy views; "seed_rbeg" is the 40-bit positions expanded to int64 on first use
    (cs_packed_seed_rbeg for every seed); packed_rbeg(p, sel) expands a selection only"""

    def __missing__(self, key):
        if key == "seed_rbeg":
            v = None if self["seed_rbeg_lo"] is None else packed_rbeg(self, slice(None))
            self[key] = v
            return v
        raise KeyError(key)


def packed_rbeg(p, sel):
    return p["seed_rbeg_lo"][sel].astype(np.int64) | (p["seed_rbeg_hi"][sel].astype(np.int64) << 32)


class Stats(C.Structure):
    _fields_ = [("reads", C.c_uint64), ("bases", C.c_uint64), ("mems", C.c_uint64), ("seeds", C.c_uint64),
                ("bwt_queries", C.c_uint64), ("bwt_calls", C.c_uint64), ("sal_queries", C.c_uint64),
                ("sal_calls", C.c_uint64), ("overflow_mems", C.c_uint64), ("seed_kernel_ms", C.c_double),
                ("sal_kernel_ms", C.c_double), ("total_ms", C.c_double), ("seed_kernel_launches", C.c_uint64),
                ("overflow_kernel_ms", C.c_double), ("overflow_kernel_launches", C.c_uint64),
                ("reseed_text_calls", C.c_uint64), ("reseed_index_calls", C.c_uint64), ("sweep_text_calls", C.c_uint64),
                ("r3_text_seeds", C.c_uint64)]

    def asdict(self):
        return {n: getattr(self, n) for n, _ in self._fields_}


class Memory(C.Structure):
    """cs_memory_t: device bytes the engine holds, by group (cs_engine_memory)"""
    _fields_ = [(n, C.c_uint64) for n in ("occ_bwt", "sampled_sa", "full_sa", "isa", "text", "lcp_rep", "jump_table", "kmer_filter")] + \
               [("pass_ctx", C.c_uint64 * 2), ("total", C.c_uint64), ("sa_entry_bits", C.c_int32), ("n_pass_ctx", C.c_int32)]


KERNELS = ["fwd0_kernel", "fwd_kernel", "bwd_win_kernel", "bwd_win0_kernel", "bwd_wide_kernel", "bwd_all_kernel", "r2text_kernel",
           "r3text_kernel", "smem_kernel"]
EVENTS = ["occ_record", "jump_entry", "filter_word", "sa_entry", "isa_entry", "text_word", "rep_load", "lcp_byte", "lep_entry", "mem_record"]


class Traffic(C.Structure):
    _fields_ = [("events", (C.c_uint64 * 10) * 9), ("event_bytes", C.c_uint64 * 10), ("stream_bytes", C.c_uint64)]


class Digest(C.Structure):
    _fields_ = [("mem_off", C.c_uint64), ("mems", C.c_uint64), ("seed_off", C.c_uint64), ("seeds", C.c_uint64)]

    def astuple(self):
        return (self.mem_off, self.mems, self.seed_off, self.seeds)


def digest_words(a):
    """host restatement of cs_engine_result_digest for one array (any dtype, viewed as 64-bit words)"""
    w = np.ascontiguousarray(a).view(np.uint8).view("<u8").astype(np.uint64)
    with np.errstate(over="ignore"):
        z = w + np.arange(w.size, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z = z ^ (z >> np.uint64(31))
        return int(np.add.reduce(z, dtype=np.uint64)) if z.size else 0


def lib_path():
    # CS_LIB: load an alternative build of the same library (A/B experiments); the default is the in-tree build
    return os.environ.get("CS_LIB") or os.path.join(_HERE, "libcompseed_amd.so")


def build_library(force=False):
    """Compile the HIP library in-tree (hipcc --offload-arch=gfx950; works without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    if force:
        subprocess.run(["make", "-C", src, "clean"], check=True, capture_output=True)
    r = subprocess.run(["make", "-C", src, "all"], capture_output=True, text=True)
    if r.returncode:
        raise RuntimeError("building libcompseed_amd.so failed:\n" + r.stdout + r.stderr)
    return lib_path()


_lib = None


def load_library():
    """Load the C-ABI library; fails loudly when it has not been built (there is no fallback path)."""
    global _lib
    if _lib is not None:
        return _lib
    p = lib_path()
    if not os.path.exists(p):
        raise ImportError("%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` or `make -C compseed_amd/csrc`" % p)
    L = C.CDLL(p)
    vp, i64, u64p = C.c_void_p, C.c_int64, C.c_void_p
    L.cs_last_error.restype = C.c_char_p
    L.cs_version.restype = C.c_char_p
    L.cs_params_default.argtypes = [C.POINTER(Params)]
    L.cs_index_load.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.cs_index_view.argtypes = [vp, C.POINTER(IndexView)]
    L.cs_index_free.argtypes = [vp]
    L.cs_index_free.restype = None
    L.cs_index_build.argtypes = [vp, C.c_uint64, C.c_int, C.POINTER(vp)]
    L.cs_index_build_flags.argtypes = [vp, C.c_uint64, C.c_int, C.c_uint32, C.POINTER(vp)]
    L.cs_engine_options_default.argtypes = [C.POINTER(EngineOptions)]
    L.cs_engine_options_default.restype = None
    L.cs_engine_create_opts.argtypes = [C.POINTER(IndexView), C.c_int, C.POINTER(EngineOptions), C.POINTER(vp)]
    L.cs_index_save.argtypes = [vp, C.c_char_p]
    L.cs_refseq_from_fasta.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.cs_refseq_codes.argtypes = [vp, C.POINTER(vp), C.POINTER(C.c_uint64), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    L.cs_refseq_save.argtypes = [vp, C.c_char_p]
    L.cs_refseq_free.argtypes = [vp]
    L.cs_refseq_free.restype = None
    L.cs_index_build_fasta.argtypes = [C.c_char_p, C.c_char_p, C.c_int]
    L.cs_reader_open.argtypes = [C.c_char_p, C.c_int64, C.POINTER(vp)]
    L.cs_reader_next.argtypes = [vp, C.POINTER(vp), C.POINTER(vp), C.POINTER(C.c_int64)]
    L.cs_reader_close.argtypes = [vp]
    L.cs_reader_close.restype = None
    L.cs_chainer_create.argtypes = [C.c_char_p, C.POINTER(vp)]
    L.cs_chainer_destroy.argtypes = [vp]
    L.cs_chainer_destroy.restype = None
    L.cs_chain_params_default.argtypes = [C.POINTER(ChainParams)]
    L.cs_chain_params_default.restype = None
    L.cs_chain_batch.argtypes = [vp, C.POINTER(ChainParams), C.POINTER(CResult), vp, C.c_int, C.POINTER(CChainResult)]
    L.cs_chainer_create_device.argtypes = [C.c_char_p, C.c_int, C.POINTER(vp)]
    L.cs_chain_batch_device.argtypes = [vp, C.POINTER(ChainParams), C.POINTER(CResult), vp, C.c_uint32, C.POINTER(CChainResult)]
    L.cs_chain_batch_gpu.argtypes = [vp, C.POINTER(ChainParams), C.POINTER(CResult), vp, C.c_uint32, C.POINTER(CChainResult)]
    L.cs_chainer_stats.argtypes = [vp, C.POINTER(ChainStats)]
    L.cs_flt_params_default.argtypes = [C.POINTER(FltParams)]
    L.cs_flt_params_default.restype = None
    L.cs_chain_filter.argtypes = [vp, C.POINTER(FltParams), C.POINTER(CChainResult), vp, vp, C.c_int, C.POINTER(CChainResult), C.POINTER(vp)]
    L.cs_chain_filter_device.argtypes = [vp, C.POINTER(FltParams), C.POINTER(CChainResult), vp, vp, C.c_uint32, C.POINTER(CChainResult), C.POINTER(vp)]
    L.cs_chain_filter_gpu.argtypes = [vp, C.POINTER(FltParams), C.POINTER(CChainResult), vp, vp, C.c_uint32, C.POINTER(CChainResult), C.POINTER(vp)]
    L.cs_chain_filter_stats.argtypes = [vp, C.POINTER(FltStats)]
    L.cs_device_count.argtypes = [C.POINTER(C.c_int)]
    L.cs_engine_create.argtypes = [C.POINTER(IndexView), C.c_int, C.POINTER(vp)]
    L.cs_engine_destroy.argtypes = [vp]
    L.cs_engine_destroy.restype = None
    L.cs_engine_seed_batch.argtypes = [vp, C.POINTER(Params), i64, vp, u64p, C.POINTER(CResult)]
    L.cs_engine_seed_batch_device.argtypes = [vp, C.POINTER(Params), i64, vp, u64p, C.c_uint64, C.POINTER(CResult)]
    L.cs_engine_submit_device.argtypes = [vp, C.POINTER(Params), i64, vp, vp, C.c_uint64]
    L.cs_engine_collect_device.argtypes = [vp, C.POINTER(CResult)]
    L.cs_engine_result_digest.argtypes = [vp, C.POINTER(Digest)]
    L.cs_engine_gather_reads.argtypes = [vp, i64, vp, C.POINTER(CResult)]
    L.cs_engine_traffic_model.argtypes = [vp, C.POINTER(Traffic)]
    L.cs_engine_seed_batch_packed.argtypes = [vp, C.POINTER(Params), i64, vp, u64p, C.POINTER(CPacked)]
    L.cs_engine_submit.argtypes = [vp, C.POINTER(Params), i64, vp, u64p]
    L.cs_engine_collect_packed.argtypes = [vp, C.POINTER(CPacked)]
    L.cs_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.cs_pack_reads.argtypes = [vp, vp, C.c_int64, vp, C.c_int, C.c_uint32]
    L.cs_host_free.argtypes = [vp]
    L.cs_engine_stats.argtypes = [vp, C.POINTER(Stats)]
    L.cs_engine_reset_stats.argtypes = [vp]
    L.cs_engine_memory.argtypes = [vp, C.POINTER(Memory)]
    L.cs_engine_reset_stats.restype = None
    L.cs_engine_occ4.argtypes = [vp, i64, vp, vp]
    L.cs_engine_extend.argtypes = [vp, i64, vp, vp, vp]
    L.cs_engine_sa.argtypes = [vp, i64, vp, vp]
    L.cs_engine_probe_random_lines.argtypes = [vp, C.c_int, C.c_int, C.POINTER(C.c_double)]
    L.cs_device_alloc.argtypes = [vp, C.c_size_t, C.POINTER(vp)]
    L.cs_device_free.argtypes = [vp, vp]
    L.cs_device_upload.argtypes = [vp, vp, vp, C.c_size_t]
    L.cs_device_download.argtypes = [vp, vp, vp, C.c_size_t]
    L.cs_device_sync.argtypes = [vp]
    L.cs_engine_check_index.argtypes = [vp, vp, C.c_uint64, C.POINTER(IndexCheck)]
    L.cs_ext_params_default.argtypes = [C.POINTER(ExtParams)]
    L.cs_ext_params_default.restype = None
    L.cs_extender_create.argtypes = [C.c_int, C.POINTER(ExtParams), C.POINTER(vp)]
    L.cs_extender_destroy.argtypes = [vp]
    L.cs_extender_destroy.restype = None
    L.cs_extend_batch.argtypes = [vp, i64, vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int32, vp]
    L.cs_extend_batch_device.argtypes = [vp, i64, vp, vp, C.c_uint64, vp, C.c_uint64, C.c_int32, vp]
    L.cs_extender_stats.argtypes = [vp, C.POINTER(ExtStats)]
    L.cs_extender_upload.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64]
    L.cs_extend_batch_resident.argtypes = [vp, i64, vp, C.c_int32, vp]
    L.cs_aln_params_default.argtypes = [C.POINTER(AlnParams)]
    L.cs_aln_params_default.restype = None
    L.cs_aligner_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(AlnParams), C.POINTER(vp)]
    L.cs_aligner_destroy.argtypes = [vp]
    L.cs_aligner_destroy.restype = None
    L.cs_extend_chains.argtypes = [vp, C.POINTER(CChainResult), vp, vp, vp, C.POINTER(CAlnResult)]
    L.cs_extend_chains_device.argtypes = [vp, C.POINTER(CChainResult), vp, vp, vp, C.c_uint32, C.POINTER(CAlnResult)]
    L.cs_aligner_stats.argtypes = [vp, C.POINTER(AlnStats)]
    L.cs_dedup_params_default.argtypes = [C.POINTER(DedupParams)]
    L.cs_dedup_params_default.restype = None
    L.cs_dedup_regions.argtypes = [vp, C.POINTER(DedupParams), C.POINTER(CAlnResult), vp, vp, C.POINTER(CAlnResult), C.POINTER(vp)]
    L.cs_regions_cigar.argtypes = [vp, C.POINTER(CAlnResult), vp, vp, C.c_uint32, C.POINTER(CCigarResult)]
    L.cs_cigar_stats.argtypes = [vp, C.POINTER(CigarStats)]
    L.cs_mark_params_default.argtypes = [C.POINTER(MarkParams)]
    L.cs_mark_params_default.restype = None
    L.cs_regions_mark.argtypes = [vp, C.POINTER(MarkParams), C.POINTER(CAlnResult), vp, C.c_int64, C.c_uint32, C.POINTER(CMarkResult)]
    L.cs_mark_stats.argtypes = [vp, C.POINTER(MarkStats)]
    L.cs_regions_sam.argtypes = [vp, C.POINTER(SamParams), C.POINTER(CMarkResult), vp, C.POINTER(CCigarResult), vp, vp, vp, vp, vp, vp, vp, C.POINTER(CSamResult)]
    L.cs_sam_header.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.cs_sam_stats.argtypes = [vp, C.POINTER(SamStats)]
    L.cs_reader_next_chunk.argtypes = [vp, C.POINTER(CReadChunk)]
    L.cs_map_params_default.argtypes = [C.POINTER(MapParams)]
    L.cs_map_params_default.restype = None
    L.cs_map_params_split.argtypes = [C.POINTER(MapParams), C.POINTER(Params), C.POINTER(ChainParams), C.POINTER(FltParams), C.POINTER(AlnParams), C.POINTER(DedupParams), C.POINTER(MarkParams),
                                      C.POINTER(C.c_uint32), C.POINTER(SamParams)]
    L.cs_mapper_create.argtypes = [C.c_char_p, C.c_int, C.POINTER(EngineOptions), C.POINTER(MapParams), C.POINTER(vp)]
    L.cs_mapper_destroy.argtypes = [vp]
    L.cs_mapper_destroy.restype = None
    L.cs_map_batch.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64, C.POINTER(CSamResult)]
    if hasattr(L, "cs_map_submit"):   # (an older build given through CS_LIB / bench.py --lib for an A/B run lacks the three; calling them there raises)
        L.cs_map_submit.argtypes = [vp, i64, vp, vp, vp, vp, vp, vp, vp, i64]
        L.cs_map_collect.argtypes = [vp, C.POINTER(CSamResult)]
        L.cs_mapper_in_flight.argtypes = [vp, C.POINTER(C.c_int), C.POINTER(C.c_int)]
    L.cs_mapper_header.argtypes = [vp, C.c_char_p, vp, C.c_size_t, C.POINTER(C.c_size_t)]
    L.cs_mapper_stats.argtypes = [vp, C.POINTER(MapStats)]
    L.cs_mapper_engine_stats.argtypes = [vp, C.POINTER(Stats)]
    _lib = L
    return L


def _check(rc):
    if rc != 0:
        raise CSError(rc, load_library().cs_last_error().decode(errors="replace"))


class Index:
    """Host copy of an FM-index: from the reference's files (<prefix>.bwt/.sa) or from numpy arrays."""

    def __init__(self):
        self.view = IndexView()
        self._handle = None
        self._keep = []

    @classmethod
    def load(cls, prefix):
        self = cls()
        L = load_library()
        h = C.c_void_p()
        _check(L.cs_index_load(os.fsencode(prefix), C.byref(h)))
        self._handle = h
        _check(L.cs_index_view(h, C.byref(self.view)))
        return self

    @classmethod
    def from_arrays(cls, primary, L2_1to4, bwt_words, sa, sa_intv=32):
        self = cls()
        bwt = np.ascontiguousarray(bwt_words, dtype=np.uint32)
        sa = np.ascontiguousarray(sa, dtype=np.uint64)
        self._keep = [bwt, sa]
        v = self.view
        v.primary = int(primary)
        v.L2[0] = 0
        for i in range(4):
            v.L2[i + 1] = int(L2_1to4[i])
        v.seq_len = int(L2_1to4[3])
        v.bwt_size = bwt.size
        v.bwt = bwt.ctypes.data
        v.sa_intv = sa_intv
        v.n_sa = sa.size
        v.sa = sa.ctypes.data
        return self

    @classmethod
    def build(cls, fwd_nt4, device=0, force_64bit=False, verbose=False):
        """Build the FM-index of a genome (forward strand, codes 0..3) on the GPU (cs_index_build_flags)."""
        self = cls()
        L = load_library()
        g = np.ascontiguousarray(fwd_nt4, dtype=np.uint8)
        h = C.c_void_p()
        _check(L.cs_index_build_flags(g.ctypes.data, g.size, int(device), (1 if force_64bit else 0) | (2 if verbose else 0), C.byref(h)))
        self._handle = h
        _check(L.cs_index_view(h, C.byref(self.view)))
        return self

    def save(self, prefix):
        """Write <prefix>.bwt / <prefix>.sa in the reference's formats (cs_index_save)."""
        if self._handle is None:
            raise ValueError("only file- or GPU-built indexes can be saved")
        _check(load_library().cs_index_save(self._handle, os.fsencode(prefix)))

    def arrays(self):
        """numpy views (copies) of the bwt words and the sampled SA"""
        v = self.view
        return _view(v.bwt, "<u4", int(v.bwt_size)), _view(v.sa, "<u8", int(v.n_sa))

    def close(self):
        if self._handle is not None:
            load_library().cs_index_free(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RefSeq:
    """reference sequences from a FASTA (cs_refseq_t): contig table, holes, forward strand as codes 0..3"""

    def __init__(self, fasta):
        self._h = C.c_void_p()
        _check(load_library().cs_refseq_from_fasta(os.fsencode(fasta), C.byref(self._h)))
        p, n, ns, nh = C.c_void_p(), C.c_uint64(), C.c_int32(), C.c_int32()
        _check(load_library().cs_refseq_codes(self._h, C.byref(p), C.byref(n), C.byref(ns), C.byref(nh)))
        self.l_pac, self.n_seqs, self.n_holes = int(n.value), int(ns.value), int(nh.value)
        self.codes = _view(p.value, np.uint8, self.l_pac)

    def save(self, prefix):
        """<prefix>.pac / .ann / .amb as bwaidx writes them"""
        _check(load_library().cs_refseq_save(self._h, os.fsencode(prefix)))

    def close(self):
        if self._h:
            load_library().cs_refseq_free(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Reader:
    """chunks of a reordered-reads or FASTQ file (plain or gzip) as the engine takes them (cs_reader_t); iterate for (bases, offsets)
    views of the reader's two alternating buffers: a chunk is valid until the one after the next is read"""

    def __init__(self, path, chunk_bases=10_000_000):
        self._h = C.c_void_p()
        _check(load_library().cs_reader_open(os.fsencode(path), int(chunk_bases), C.byref(self._h)))

    def __iter__(self):
        return self

    def __next__(self):
        b, o, n = C.c_void_p(), C.c_void_p(), C.c_int64()
        _check(load_library().cs_reader_next(self._h, C.byref(b), C.byref(o), C.byref(n)))
        if n.value == 0:
            raise StopIteration
        off = _view(o.value, "<u8", n.value + 1, False)
        return _view(b.value, np.uint8, int(off[-1]), False), off

    def next_chunk(self, copy=False):
        """cs_reader_next_chunk: the next chunk with what a SAM record needs, as a dict -- n_reads, first_id (the reads before it: map_batch's
        id_base), bases, offsets, quals (None for reordered reads), names / comments as (bytes as uint8, uint64 CSR offsets) pairs (comments
        None where the input has none) -- or None at the end of the input.  copy=False: views of the reader's two alternating buffers, valid
        until the chunk after the next is read.  A reader is driven either by this call or by iteration"""
        c = CReadChunk()
        _check(load_library().cs_reader_next_chunk(self._h, C.byref(c)))
        n = int(c.n_reads)
        if n == 0:
            return None
        off = _view(c.offsets, "<u8", n + 1, copy)
        csr = lambda b, o: None if not o else (lambda oo: (_view(b, np.uint8, int(oo[-1]), copy), oo))(_view(o, "<u8", n + 1, copy))
        return dict(n_reads=n, first_id=int(c.first_id), bases=_view(c.bases, np.uint8, int(off[-1]), copy), offsets=off,
                    quals=_view(c.quals, np.uint8, int(off[-1]), copy) if c.quals else None, names=csr(c.names, c.name_off), comments=csr(c.comments, c.comment_off))

    def close(self):
        if self._h:
            load_library().cs_reader_close(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Chainer:
    """mem_chain over a batch's seeds (cs_chainer_t); needs <prefix>.ann.  With a device (cs_chainer_create_device) the chainer also
    chains on that GPU: chain_gpu() from host arrays, chain_device() from an on-device Result."""

    def __init__(self, prefix, device=None):
        self._h = C.c_void_p()
        self.device = device
        if device is None:
            _check(load_library().cs_chainer_create(os.fsencode(prefix), C.byref(self._h)))
        else:
            _check(load_library().cs_chainer_create_device(os.fsencode(prefix), int(device), C.byref(self._h)))

    @staticmethod
    def _host_in(mem_off, mems, seed_off, seeds, read_offsets):
        mem_off = np.ascontiguousarray(mem_off, dtype=np.uint64); seed_off = np.ascontiguousarray(seed_off, dtype=np.uint64)
        mems = np.ascontiguousarray(mems, dtype=INTV_DT); seeds = np.ascontiguousarray(seeds, dtype=SEED_DT)
        ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        res = CResult(mem_off.size - 1, mems.size, seeds.size, mem_off.ctypes.data, mems.ctypes.data, seed_off.ctypes.data, seeds.ctypes.data)
        return res, ro, (mem_off, mems, seed_off, seeds)

    @staticmethod
    def _host_out(out, copy):
        return dict(chain_off=_view(out.chain_off, "<u8", int(out.n_reads) + 1, copy), chains=_view(out.chains, CHAIN_DT, int(out.n_chains), copy),
                    cseed_off=_view(out.cseed_off, "<u8", int(out.n_chains) + 1, copy), cseeds=_view(out.cseeds, SEED_DT, int(out.n_seeds), copy))   # copy=False: views of the chainer's arrays, valid until its next chain()

    def chain(self, mem_off, mems, seed_off, seeds, read_offsets, params=None, threads=4, copy=True):
        """host CSR seeds (numpy arrays as Result holds them) -> dict(chain_off, chains (CHAIN_DT), cseed_off, cseeds (SEED_DT)), copies"""
        params = params or ChainParams()
        res, ro, _keep = self._host_in(mem_off, mems, seed_off, seeds, read_offsets)
        out = CChainResult()
        _check(load_library().cs_chain_batch(self._h, C.byref(params), C.byref(res), ro.ctypes.data, int(threads), C.byref(out)))
        return self._host_out(out, copy)

    def chain_gpu(self, mem_off, mems, seed_off, seeds, read_offsets, params=None, flags=0, copy=True):
        """cs_chain_batch_gpu: chain()'s arguments and result, the work done on the chainer's GPU (flags: CHAIN_TREE_ONLY)"""
        params = params or ChainParams()
        res, ro, _keep = self._host_in(mem_off, mems, seed_off, seeds, read_offsets)
        out = CChainResult()
        _check(load_library().cs_chain_batch_gpu(self._h, C.byref(params), C.byref(res), ro.ctypes.data, int(flags), C.byref(out)))
        return self._host_out(out, copy)

    def chain_device(self, result, d_read_offsets, params=None, flags=0):
        """cs_chain_batch_device: an on-device Result (Engine.seed_batch_device / collect_device) and the batch's offsets in device memory ->
        dict(n_reads, n_chains, n_seeds, chain_off, chains, cseed_off, cseeds): host counts and device pointers owned by the chainer, valid
        until its next chain call (download_chains() turns them into chain()'s dict)"""
        params = params or ChainParams()
        p = result.ptr
        res = CResult(result.n_reads, result.n_mems, result.n_seeds, p["mem_off"], p["mems"], p["seed_off"], p["seeds"])
        out = CChainResult()
        _check(load_library().cs_chain_batch_device(self._h, C.byref(params), C.byref(res), C.c_void_p(d_read_offsets), int(flags), C.byref(out)))
        return dict(n_reads=int(out.n_reads), n_chains=int(out.n_chains), n_seeds=int(out.n_seeds), chain_off=out.chain_off, chains=out.chains,
                    cseed_off=out.cseed_off, cseeds=out.cseeds)

    def stats(self):
        """cs_chainer_stats: counters of the device calls over the chainer's life"""
        st = ChainStats()
        _check(load_library().cs_chainer_stats(self._h, C.byref(st)))
        return {n: (float(getattr(st, n)) if n == "kernel_ms" else int(getattr(st, n))) for n, _ in ChainStats._fields_}

    def filter(self, chain_off, chains, cseed_off, cseeds, bases, read_offsets, params=None, threads=4, copy=True):
        """cs_chain_filter (mem_chain_flt + mem_flt_chained_seeds): chains as chain() returns them -> the same dict for the surviving
        chains in the reference's order, plus cseed_score (int32 per surviving seed); copies"""
        params = params or FltParams()
        chain_off = np.ascontiguousarray(chain_off, dtype=np.uint64); cseed_off = np.ascontiguousarray(cseed_off, dtype=np.uint64)
        chains = np.ascontiguousarray(chains, dtype=CHAIN_DT); cseeds = np.ascontiguousarray(cseeds, dtype=SEED_DT)
        ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        bases = None if bases is None else np.ascontiguousarray(bases, dtype=np.uint8)
        cin = CChainResult(chain_off.size - 1, chains.size, cseeds.size, chain_off.ctypes.data, chains.ctypes.data if chains.size else None, cseed_off.ctypes.data,
                           cseeds.ctypes.data if cseeds.size else None)
        out = CChainResult(); sc = C.c_void_p()
        _check(load_library().cs_chain_filter(self._h, C.byref(params), C.byref(cin), bases.ctypes.data if bases is not None and bases.size else None, ro.ctypes.data,
                                              int(threads), C.byref(out), C.byref(sc)))
        return dict(chain_off=_view(out.chain_off, "<u8", int(out.n_reads) + 1, copy), chains=_view(out.chains, CHAIN_DT, int(out.n_chains), copy),
                    cseed_off=_view(out.cseed_off, "<u8", int(out.n_chains) + 1, copy), cseeds=_view(out.cseeds, SEED_DT, int(out.n_seeds), copy),
                    cseed_score=_view(sc.value, "<i4", int(out.n_seeds), copy))

    def filter_gpu(self, chain_off, chains, cseed_off, cseeds, bases, read_offsets, params=None, flags=0, copy=True):
        """cs_chain_filter_gpu: filter()'s arguments and result, the work done on the chainer's GPU (flags: FLT_WAVE_ONLY)"""
        params = params or FltParams()
        chain_off = np.ascontiguousarray(chain_off, dtype=np.uint64); cseed_off = np.ascontiguousarray(cseed_off, dtype=np.uint64)
        chains = np.ascontiguousarray(chains, dtype=CHAIN_DT); cseeds = np.ascontiguousarray(cseeds, dtype=SEED_DT)
        ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        bases = None if bases is None else np.ascontiguousarray(bases, dtype=np.uint8)
        cin = CChainResult(chain_off.size - 1, chains.size, cseeds.size, chain_off.ctypes.data, chains.ctypes.data if chains.size else None, cseed_off.ctypes.data,
                           cseeds.ctypes.data if cseeds.size else None)
        out = CChainResult(); sc = C.c_void_p()
        _check(load_library().cs_chain_filter_gpu(self._h, C.byref(params), C.byref(cin), bases.ctypes.data if bases is not None and bases.size else None, ro.ctypes.data,
                                                  int(flags), C.byref(out), C.byref(sc)))
        return dict(chain_off=_view(out.chain_off, "<u8", int(out.n_reads) + 1, copy), chains=_view(out.chains, CHAIN_DT, int(out.n_chains), copy),
                    cseed_off=_view(out.cseed_off, "<u8", int(out.n_chains) + 1, copy), cseeds=_view(out.cseeds, SEED_DT, int(out.n_seeds), copy),
                    cseed_score=_view(sc.value, "<i4", int(out.n_seeds), copy))

    def filter_device(self, d_chains, d_bases, d_read_offsets, params=None, flags=0):
        """cs_chain_filter_device: chain_device()'s dict, the batch's reads and offsets in device memory (d_bases may be None / 0 when no read is
        long enough for the seed test) -> the same dict form for the surviving chains plus cseed_score, the device pointer of their seeds'
        scores; device arrays owned by the chainer, valid until its next filter_device / filter_gpu (download_chains() brings them over)"""
        params = params or FltParams()
        d = d_chains
        cin = CChainResult(d["n_reads"], d["n_chains"], d["n_seeds"], d["chain_off"], d["chains"], d["cseed_off"], d["cseeds"])
        out = CChainResult(); sc = C.c_void_p()
        _check(load_library().cs_chain_filter_device(self._h, C.byref(params), C.byref(cin), C.c_void_p(d_bases or None), C.c_void_p(d_read_offsets or None), int(flags),
                                                     C.byref(out), C.byref(sc)))
        return dict(n_reads=int(out.n_reads), n_chains=int(out.n_chains), n_seeds=int(out.n_seeds), chain_off=out.chain_off, chains=out.chains,
                    cseed_off=out.cseed_off, cseeds=out.cseeds, cseed_score=sc.value)

    def filter_stats(self):
        """cs_chain_filter_stats: counters of filter_device / filter_gpu over the chainer's life"""
        st = FltStats()
        _check(load_library().cs_chain_filter_stats(self._h, C.byref(st)))
        return {n: (float(getattr(st, n)) if n == "kernel_ms" else int(getattr(st, n))) for n, _ in FltStats._fields_}

    def close(self):
        if self._h:
            load_library().cs_chainer_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def download_chains(engine, d):
    """Chainer.chain_device's result -> chain()'s dict of host arrays, through an Engine on the same GPU; Chainer.filter_device's result
    (a dict with cseed_score) -> filter()'s dict"""
    def get(ptr, dt, n):
        return engine.download(ptr, dt, n) if n else np.zeros(0, dtype=dt)
    out = dict(chain_off=get(d["chain_off"], np.uint64, d["n_reads"] + 1), chains=get(d["chains"], CHAIN_DT, d["n_chains"]),
               cseed_off=get(d["cseed_off"], np.uint64, d["n_chains"] + 1), cseeds=get(d["cseeds"], SEED_DT, d["n_seeds"]))
    if "cseed_score" in d:
        out["cseed_score"] = get(d["cseed_score"], np.int32, d["n_seeds"])
    return out


def download_regions(engine, d):
    """Aligner.extend_chains_device's result -> extend_chains()'s dict of host arrays (reg_off uint64, regs ALNREG_DT), through an Engine on
    the same GPU"""
    return dict(reg_off=engine.download(d["reg_off"], np.uint64, d["n_reads"] + 1),
                regs=engine.download(d["regs"], ALNREG_DT, d["n_regs"]) if d["n_regs"] else np.zeros(0, dtype=ALNREG_DT))


def build_index_from_fasta(fasta, prefix, device=0):
    """bwa_idx_build: all five index files from a FASTA, the suffix sort on the GPU (cs_index_build_fasta)"""
    _check(load_library().cs_index_build_fasta(os.fsencode(fasta), os.fsencode(prefix), int(device)))


class Result:
    """CSR result of one batch as numpy arrays (host variant) or raw device pointers (device variant)."""

    def __init__(self, cres, on_device, want_sal, copy=True):
        self.n_reads, self.n_mems, self.n_seeds = int(cres.n_reads), int(cres.n_mems), int(cres.n_seeds)
        self.on_device = on_device
        self.ptr = dict(mem_off=cres.mem_off, mems=cres.mems, seed_off=cres.seed_off, seeds=cres.seeds)
        if not on_device:
            self.mem_off = _view(cres.mem_off, "<u8", self.n_reads + 1, copy)
            self.mems = _view(cres.mems, INTV_DT, self.n_mems, copy)
            self.seed_off = _view(cres.seed_off, "<u8", self.n_reads + 1, copy) if want_sal else None
            self.seeds = _view(cres.seeds, SEED_DT, self.n_seeds, copy) if want_sal else None


def _view(ptr, dt, n, copy=True):
    dt = np.dtype(dt)
    if n == 0 or not ptr:
        return np.zeros(0, dtype=dt)
    buf = (C.c_char * (n * dt.itemsize)).from_address(ptr)
    a = np.frombuffer(buf, dtype=dt, count=n)
    return a.copy() if copy else a  # copy=False: a view of the engine's pinned buffer, valid until the next call


class PinnedArray(np.ndarray):
    """uint8 numpy array over pinned host memory from cs_host_alloc (freed with the array)"""
    _ptr = None

    def __del__(self):
        if self._ptr:
            try:
                load_library().cs_host_free(C.c_void_p(self._ptr))
            except Exception:
                pass
            self._ptr = None


def pinned_array(nbytes):
    """uint8 array of `nbytes` in pinned host memory (cs_host_alloc): what an integration would read its chunk of reads into"""
    p = C.c_void_p()
    _check(load_library().cs_host_alloc(int(nbytes), C.byref(p)))
    buf = (C.c_uint8 * int(nbytes)).from_address(p.value)
    a = np.frombuffer(buf, dtype=np.uint8).view(PinnedArray)
    a._ptr = p.value
    return a


def pack_reads(bases, offsets, threads=1, scalar=False):
    """cs_pack_reads: the reads as the kernels' 16-byte records of 32 bases -> uint32 array (n_records, 4)"""
    bases = np.ascontiguousarray(bases, dtype=np.uint8)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    n = offsets.size - 1
    rec = np.zeros(((int(offsets[-1]) >> 5) + n, 4), dtype=np.uint32)
    _check(load_library().cs_pack_reads(bases.ctypes.data, offsets.ctypes.data, n, rec.ctypes.data, int(threads), 1 if scalar else 0))
    return rec


class Engine:
    """One GPU, one resident index (cs_engine_t)."""

    def __init__(self, index, device=0, **options):
        """options: fields of cs_engine_options_t (full_sa, sa64, sa40, text_mode, text_arrays, jump_k, kmer_filter, fused, mem_cap,
        lep_arena_mb, max_raw_mb, r3_text_iter, count_sal_merged, verbose)"""
        self._L = load_library()
        self._h = C.c_void_p()
        self._index = index  # keep host arrays alive during upload
        self.options = EngineOptions(**options)
        _check(self._L.cs_engine_create_opts(C.byref(index.view), int(device), C.byref(self.options), C.byref(self._h)))
        self.device = device

    def close(self):
        if self._h:
            self._L.cs_engine_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- hot path
    def seed_batch(self, bases, offsets, params=None, copy=True):
        """Host buffers in, numpy CSR out (cs_engine_seed_batch).  copy=False returns views of the engine's pinned
        result buffers (valid until the next call on this engine) instead of copies."""
        params = params or Params()
        if not isinstance(bases, PinnedArray):
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        res = CResult()
        _check(self._L.cs_engine_seed_batch(self._h, C.byref(params), offsets.size - 1, bases.ctypes.data, offsets.ctypes.data, C.byref(res)))
        return Result(res, False, bool(params.want_sal), copy)

    def seed_batch_packed(self, bases, offsets, params=None):
        """Host buffers in, the PACKED CSR (what crosses PCIe) out as views of the engine's pinned buffers: dict(mem_format, mem_off,
        mems (MEM16_DT, MEM8_DT under RESULT_LEAN, or INTV_DT), seed_off, seed_rbeg, max_occ); valid until the next call (cs_engine_seed_batch_packed)"""
        params = params or Params()
        if not isinstance(bases, PinnedArray):
            bases = np.ascontiguousarray(bases, dtype=np.uint8)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        res = CPacked()
        _check(self._L.cs_engine_seed_batch_packed(self._h, C.byref(params), offsets.size - 1, bases.ctypes.data, offsets.ctypes.data, C.byref(res)))
        return self._packed(res)

    def submit(self, bases, offsets, params=None):
        """queue a batch (cs_engine_submit); bases / offsets must be contiguous uint8 / uint64 arrays that stay alive and unchanged until collected"""
        params = params or Params()
        assert bases.dtype == np.uint8 and offsets.dtype == np.uint64 and bases.flags.c_contiguous and offsets.flags.c_contiguous
        self._inflight = getattr(self, "_inflight", []) + [(bases, offsets, params)]
        _check(self._L.cs_engine_submit(self._h, C.byref(params), offsets.size - 1, bases.ctypes.data, offsets.ctypes.data))

    def collect_packed(self):
        """block until the oldest submitted batch is complete (cs_engine_collect_packed); same dict as seed_batch_packed"""
        res = CPacked()
        _check(self._L.cs_engine_collect_packed(self._h, C.byref(res)))
        self._inflight = getattr(self, "_inflight", [])[1:]
        return self._packed(res)

    @staticmethod
    def _packed(res):
        n = int(res.n_reads)
        sal = bool(res.seed_off)
        return PackedResult(n_reads=n, n_mems=int(res.n_mems), n_seeds=int(res.n_seeds), mem_format=int(res.mem_format), max_occ=int(res.max_occ),
                            mem_off=_view(res.mem_off, "<u8", n + 1, False),
                            mems=_view(res.mems, {MEM_PACKED16: MEM16_DT, MEM_LEAN8: MEM8_DT}.get(int(res.mem_format), INTV_DT), int(res.n_mems), False),
                            seed_off=_view(res.seed_off, "<u8", n + 1, False) if sal else None, seed_format=int(res.seed_format),
                            seed_rbeg_lo=_view(res.seed_rbeg_lo, "<u4", int(res.n_seeds), False) if sal else None,
                            seed_rbeg_hi=_view(res.seed_rbeg_hi, "u1", int(res.n_seeds), False) if sal else None)

    def seed_batch_device(self, d_bases, d_offsets, n_reads, n_bases, params=None):
        """Device pointers (ints) in, device pointers out (cs_engine_seed_batch_device): no PCIe traffic in the call."""
        params = params or Params()
        res = CResult()
        _check(self._L.cs_engine_seed_batch_device(self._h, C.byref(params), int(n_reads), C.c_void_p(d_bases), C.c_void_p(d_offsets),
                                                   int(n_bases), C.byref(res)))
        return Result(res, True, bool(params.want_sal))

    def submit_device(self, d_bases, d_offsets, n_reads, n_bases, params=None):
        """cs_engine_submit_device: queue a device-resident batch (up to two in flight, seeded on alternating pass contexts)"""
        params = params or Params()
        _check(self._L.cs_engine_submit_device(self._h, C.byref(params), int(n_reads), C.c_void_p(d_bases), C.c_void_p(d_offsets), int(n_bases)))

    def collect_device(self):
        """cs_engine_collect_device: the oldest submitted device batch, as device pointers into the engine's spare result set: valid until
        the second submit_device from now in every order of submits and collects (a batch whose collect raises does not count against an
        earlier result), and until the next blocking seed call or submit() once the stream is drained.  seed_off / seeds are null for a
        batch submitted with want_sal = 0."""
        res = CResult()
        _check(self._L.cs_engine_collect_device(self._h, C.byref(res)))
        return Result(res, True, bool(res.seed_off))

    def result_digest(self):
        """(mem_off, mems, seed_off, seeds) digests of the result of the last seed call, computed on the device"""
        d = Digest()
        _check(self._L.cs_engine_result_digest(self._h, C.byref(d)))
        return d.astuple()

    def gather_reads(self, read_ids, copy=True):
        """CSR slice of the selected reads of the last result (cs_engine_gather_reads) as a host Result"""
        ids = np.ascontiguousarray(read_ids, dtype=np.uint64)
        res = CResult()
        _check(self._L.cs_engine_gather_reads(self._h, ids.size, ids.ctypes.data, C.byref(res)))
        return Result(res, False, bool(res.seed_off), copy)

    def traffic_model(self):
        """byte model of the SMEM stage since the last reset_stats(): {"kernels": {name: {"bytes": B, "events": {event: n}}}, "stream_bytes": S,
        "bytes": total} (cs_engine_traffic_model)"""
        t = Traffic()
        _check(self._L.cs_engine_traffic_model(self._h, C.byref(t)))
        eb = [int(x) for x in t.event_bytes]
        out = {"kernels": {}, "stream_bytes": int(t.stream_bytes), "event_bytes": dict(zip(EVENTS, eb))}
        tot = int(t.stream_bytes)
        for k, name in enumerate(KERNELS):
            ev = [int(x) for x in t.events[k]]
            if any(ev):
                b = sum(n * w for n, w in zip(ev, eb))
                out["kernels"][name] = {"bytes": b, "events": {e: n for e, n in zip(EVENTS, ev) if n}}
                tot += b
        out["bytes"] = tot
        return out

    def check_index(self, d_fwd_nt4=None, l_pac=0):
        """cs_engine_check_index: violation counts of the resident index against the text (and, when given, the caller's genome on the device)"""
        c = IndexCheck()
        _check(self._L.cs_engine_check_index(self._h, int(d_fwd_nt4) if d_fwd_nt4 else None, int(l_pac), C.byref(c)))
        return {n: int(getattr(c, n)) for n, _ in IndexCheck._fields_ if n != "reserved"}

    def stats(self):
        st = Stats()
        _check(self._L.cs_engine_stats(self._h, C.byref(st)))
        return st.asdict()

    def reset_stats(self):
        self._L.cs_engine_reset_stats(self._h)

    def memory(self):
        """cs_engine_memory: device bytes held, by group: {"occ_bwt", "sampled_sa", "full_sa", "isa", "text", "lcp_rep", "jump_table",
        "kmer_filter", "pass_ctx": [ctx0 + the spare result set of collect_device, ctx1], "total", "sa_entry_bits": 32 | 40 | 64 | 0, "n_pass_ctx"}; host-only, legal while batches are in flight"""
        m = Memory()
        _check(self._L.cs_engine_memory(self._h, C.byref(m)))
        d = {n: int(getattr(m, n)) for n, _ in Memory._fields_ if n != "pass_ctx"}
        d["pass_ctx"] = [int(x) for x in m.pass_ctx]
        return d

    # ---- primitives (parity tests of the building blocks)
    def occ4(self, k):
        k = np.ascontiguousarray(k, dtype=np.uint64)
        out = np.zeros((k.size, 4), dtype=np.uint64)
        _check(self._L.cs_engine_occ4(self._h, k.size, k.ctypes.data, out.ctypes.data))
        return out

    def extend(self, ik, is_back):
        ik = np.ascontiguousarray(ik, dtype=INTV_DT)
        fb = np.ascontiguousarray(is_back, dtype=np.uint8)
        out = np.zeros((ik.size, 4), dtype=INTV_DT)
        _check(self._L.cs_engine_extend(self._h, ik.size, ik.ctypes.data, fb.ctypes.data, out.ctypes.data))
        return out

    def sa(self, k):
        k = np.ascontiguousarray(k, dtype=np.uint64)
        out = np.zeros(k.size, dtype=np.uint64)
        _check(self._L.cs_engine_sa(self._h, k.size, k.ctypes.data, out.ctypes.data))
        return out

    def probe_random_lines(self, waves_per_simd=8, steps=2000):
        """64-byte random Occ-block reads per second in dependent chains (cs_engine_probe_random_lines)"""
        out = C.c_double()
        _check(self._L.cs_engine_probe_random_lines(self._h, waves_per_simd, steps, C.byref(out)))
        return out.value

    # ---- device memory helpers
    def alloc(self, nbytes):
        p = C.c_void_p()
        _check(self._L.cs_device_alloc(self._h, nbytes, C.byref(p)))
        return p.value

    def free(self, dptr):
        _check(self._L.cs_device_free(self._h, C.c_void_p(dptr)))

    def upload(self, dptr, arr):
        arr = np.ascontiguousarray(arr)
        _check(self._L.cs_device_upload(self._h, C.c_void_p(dptr), arr.ctypes.data, arr.nbytes))

    def download(self, dptr, dtype, count):
        out = np.zeros(count, dtype=dtype)
        _check(self._L.cs_device_download(self._h, out.ctypes.data, C.c_void_p(dptr), out.nbytes))
        return out

    def sync(self):
        _check(self._L.cs_device_sync(self._h))


class Extender:
    """cs_extender_t: the banded Smith-Waterman seed extension on the GPU (include/compseed_amd.h; the reference's BandedPairWiseSW)"""

    def __init__(self, device=0, params=None):
        self.L = load_library()
        self.h = C.c_void_p()
        _check(self.L.cs_extender_create(device, C.byref(params) if params is not None else None, C.byref(self.h)))

    def extend(self, pairs, qbuf, tbuf, w=100):
        """pairs: EXT_PAIR_DT array; qbuf / tbuf: uint8 codes 0..4.  Returns an EXT_RES_DT array (raises CSError on bad pairs)."""
        pairs = np.ascontiguousarray(pairs, dtype=EXT_PAIR_DT)
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8); tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
        out = np.zeros(pairs.size, dtype=EXT_RES_DT)
        self.last_rc = self.L.cs_extend_batch(self.h, pairs.size, pairs.ctypes.data if pairs.size else None, qbuf.ctypes.data if qbuf.size else None, qbuf.size,
                                              tbuf.ctypes.data if tbuf.size else None, tbuf.size, int(w), out.ctypes.data if pairs.size else None)
        self.last_out = out
        _check(self.last_rc)
        return out

    def upload(self, qbuf, tbuf):
        """cs_extender_upload: the two sequence buffers stay in the extender for extend_resident (extend leaves its own there as well)"""
        qbuf = np.ascontiguousarray(qbuf, dtype=np.uint8); tbuf = np.ascontiguousarray(tbuf, dtype=np.uint8)
        _check(self.L.cs_extender_upload(self.h, qbuf.ctypes.data if qbuf.size else None, qbuf.size, tbuf.ctypes.data if tbuf.size else None, tbuf.size))

    def extend_resident(self, pairs, w=100):
        """cs_extend_batch_resident: extend() against the sequences the extender holds"""
        pairs = np.ascontiguousarray(pairs, dtype=EXT_PAIR_DT)
        out = np.zeros(pairs.size, dtype=EXT_RES_DT)
        self.last_rc = self.L.cs_extend_batch_resident(self.h, pairs.size, pairs.ctypes.data if pairs.size else None, int(w), out.ctypes.data if pairs.size else None)
        self.last_out = out
        _check(self.last_rc)
        return out

    def extend_device(self, d_pairs, n, d_q, q_bytes, d_t, t_bytes, d_out, w=100):
        _check(self.L.cs_extend_batch_device(self.h, int(n), int(d_pairs), int(d_q), int(q_bytes), int(d_t), int(t_bytes), int(w), int(d_out)))

    def stats(self):
        st = ExtStats()
        _check(self.L.cs_extender_stats(self.h, C.byref(st)))
        return {n: getattr(st, n) for n, _ in ExtStats._fields_}

    def close(self):
        if self.h:
            self.L.cs_extender_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


class Aligner:
    """cs_aligner_t: the extension stage as a whole (the reference's mem_chain2aln_across_reads_V2): chains in, alignment regions out"""

    def __init__(self, prefix, device=0, params=None):
        self.L = load_library()
        self.h = C.c_void_p()
        _check(self.L.cs_aligner_create(os.fsencode(prefix), device, C.byref(params) if params is not None else None, C.byref(self.h)))

    def extend_chains(self, chain_off, chains, cseed_off, cseeds, bases, read_offsets, cseed_score=None, copy=True):
        """chains as Chainer.chain returns them (or the caller's own, e.g. filtered); returns dict(reg_off, regs (ALNREG_DT)), copies"""
        chain_off = np.ascontiguousarray(chain_off, dtype=np.uint64); cseed_off = np.ascontiguousarray(cseed_off, dtype=np.uint64)
        chains = np.ascontiguousarray(chains, dtype=CHAIN_DT); cseeds = np.ascontiguousarray(cseeds, dtype=SEED_DT)
        bases = np.ascontiguousarray(bases, dtype=np.uint8); ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        sc = None if cseed_score is None else np.ascontiguousarray(cseed_score, dtype=np.int32)
        cr = CChainResult(chain_off.size - 1, chains.size, cseeds.size, chain_off.ctypes.data, chains.ctypes.data if chains.size else None, cseed_off.ctypes.data,
                          cseeds.ctypes.data if cseeds.size else None)
        out = CAlnResult()
        _check(self.L.cs_extend_chains(self.h, C.byref(cr), sc.ctypes.data if sc is not None and sc.size else None, bases.ctypes.data if bases.size else None, ro.ctypes.data, C.byref(out)))
        return dict(reg_off=_view(out.reg_off, "<u8", int(out.n_reads) + 1, copy), regs=_view(out.regs, ALNREG_DT, int(out.n_regs), copy))

    def extend_chains_device(self, d_chains, d_bases, d_read_offsets, d_cseed_score=None, flags=0):
        """cs_extend_chains_device: Chainer.filter_device's / chain_device's dict and the batch's reads and offsets in device memory
        (d_cseed_score defaults to the dict's own cseed_score, if it has one) -> dict(n_reads, n_regs, reg_off, regs): host counts and
        device pointers owned by the aligner, valid until its next extend_chains / extend_chains_device (download_regions() brings them
        over); flags: ALN_DEV_COMPACT"""
        d = d_chains
        if d_cseed_score is None:
            d_cseed_score = d.get("cseed_score")
        cin = CChainResult(d["n_reads"], d["n_chains"], d["n_seeds"], d["chain_off"], d["chains"], d["cseed_off"], d["cseeds"])
        out = CAlnResult()
        _check(self.L.cs_extend_chains_device(self.h, C.byref(cin), C.c_void_p(d_cseed_score or None), C.c_void_p(d_bases or None), C.c_void_p(d_read_offsets or None),
                                              int(flags), C.byref(out)))
        return dict(n_reads=int(out.n_reads), n_regs=int(out.n_regs), reg_off=out.reg_off, regs=out.regs)

    def dedup_regions(self, reg_off, regs, bases, read_offsets, params=None, copy=True):
        """cs_dedup_regions (purged regions dropped, mem_sort_dedup_patch): regions as extend_chains returns them -> dict(reg_off, regs, n_comp), copies"""
        params = params or DedupParams()
        reg_off = np.ascontiguousarray(reg_off, dtype=np.uint64); regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        bases = np.ascontiguousarray(bases, dtype=np.uint8); ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        cin = CAlnResult(reg_off.size - 1, regs.size, reg_off.ctypes.data, regs.ctypes.data if regs.size else None)
        out = CAlnResult(); nc = C.c_void_p()
        _check(self.L.cs_dedup_regions(self.h, C.byref(params), C.byref(cin), bases.ctypes.data if bases.size else None, ro.ctypes.data, C.byref(out), C.byref(nc)))
        return dict(reg_off=_view(out.reg_off, "<u8", int(out.n_reads) + 1, copy), regs=_view(out.regs, ALNREG_DT, int(out.n_regs), copy), n_comp=_view(nc.value, "<i4", int(out.n_regs), copy))

    def regions_cigar(self, reg_off, regs, bases, read_offsets, flags=0):
        """cs_regions_cigar (mem_reg2aln without SAM text; marking and MAPQ are regions_mark's): regions as extend_chains, dedup_regions or regions_mark return them ->
        dict(alns: one ALN_DT record per region, cigar: uint32 in BAM coding, md: the NUL-terminated strings), copies.  Regions that
        bridge the strands come back empty with nm = -1 and the call raises CSError(-1) AFTER the others were made: the exception
        carries them as `.result`."""
        reg_off = np.ascontiguousarray(reg_off, dtype=np.uint64); regs = np.ascontiguousarray(regs, dtype=ALNREG_DT)
        bases = np.ascontiguousarray(bases, dtype=np.uint8); ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        cin = CAlnResult(reg_off.size - 1, regs.size, reg_off.ctypes.data, regs.ctypes.data if regs.size else None)
        out = CCigarResult()
        rc = self.L.cs_regions_cigar(self.h, C.byref(cin), bases.ctypes.data if bases.size else None, ro.ctypes.data, int(flags), C.byref(out))
        res = None
        if out.alns or (rc == 0 and out.md):
            res = dict(alns=_view(out.alns, ALN_DT, int(out.n_regs), True), cigar=_view(out.cigar, "<u4", int(out.n_cigar), True), md=_view(out.md, "u1", int(out.md_bytes), True))
        if rc != 0:
            e = CSError(rc, self.L.cs_last_error().decode(errors="replace"))
            e.result = res if res is not None and int(res["alns"].size) == regs.size and bool((res["alns"]["nm"] == -1).any()) else None
            raise e
        return res

    def cigar_stats(self):
        st = CigarStats()
        _check(self.L.cs_cigar_stats(self.h, C.byref(st)))
        return {n: (float(getattr(st, n)) if n == "kernel_ms" else int(getattr(st, n))) for n, _ in CigarStats._fields_}

    def regions_mark(self, reg_off, regs, read_offsets, params=None, id_base=0, flags=0):
        """cs_regions_mark (mem_mark_primary_se, mem_approx_mapq_se, the selection of mem_reg2sam, mem_gen_alt's membership rule): regions
        as dedup_regions returns them -> dict(marks: one MARK_DT record per region in rank order, CSR by reg_off; line_off; cigar_reg_off /
        cigar_regs: the regions with line >= 0 or xa_of >= 0, regions_cigar's input; cigar_src: their indices into marks), copies.
        flags: MARK_ALL (-a), MARK_NO_MULTI (-M), MARK_KEEP_SUPP_MAPQ (-q)"""
        params = params or MarkParams()
        reg_off = np.ascontiguousarray(reg_off, dtype=np.uint64); regs = np.ascontiguousarray(regs, dtype=ALNREG_DT); ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        cin = CAlnResult(reg_off.size - 1, regs.size, reg_off.ctypes.data, regs.ctypes.data if regs.size else None)
        out = CMarkResult()
        _check(self.L.cs_regions_mark(self.h, C.byref(params), C.byref(cin), ro.ctypes.data, int(id_base), int(flags), C.byref(out)))
        n, nc = int(out.n_reads), int(out.cigar_regs.n_regs)
        return dict(marks=_view(out.marks, MARK_DT, int(out.n_regs), True), line_off=_view(out.line_off, "<u8", n + 1, True), cigar_reg_off=_view(out.cigar_regs.reg_off, "<u8", n + 1, True),
                    cigar_regs=_view(out.cigar_regs.regs, ALNREG_DT, nc, True), cigar_src=_view(out.cigar_src, "<u4", nc, True))

    def mark_stats(self):
        st = MarkStats()
        _check(self.L.cs_mark_stats(self.h, C.byref(st)))
        return {n: (float(getattr(st, n)) if n == "kernel_ms" else int(getattr(st, n))) for n, _ in MarkStats._fields_}

    def regions_sam(self, marks, alns, bases, read_offsets, names, quals=None, comments=None, softclip=False, rg_id=None, flags=0, reg_off=None):
        """cs_regions_sam (mem_aln2sam, the string part of mem_gen_alt, the unmapped record): `marks` regions_mark's dict, `alns` regions_cigar's
        dict over marks' cigar_regs, `reg_off` the reg_off regions_mark was given (or marks["reg_off"]), `names` / `comments` pairs
        (bytes as uint8, uint64 CSR offsets) or lists of bytes, `quals` uint8 at the bases' offsets -> (text_off, text): read r's records are
        text[text_off[r]:text_off[r + 1]], text as a whole the body of the reference's output.  softclip: -Y; rg_id: the ID of -R's line"""
        def pair(x):
            if isinstance(x, (list, tuple)) and (len(x) != 2 or isinstance(x[0], (bytes, str))):
                x = [y.encode() if isinstance(y, str) else y for y in x]
                off = np.zeros(len(x) + 1, np.uint64)
                off[1:] = np.cumsum([len(y) for y in x])
                x = (np.frombuffer(b"".join(x), np.uint8), off)
            b = np.ascontiguousarray(x[0], dtype=np.uint8)
            return (b if b.size else np.zeros(1, np.uint8)), np.ascontiguousarray(x[1], dtype=np.uint64)
        reg_off = np.ascontiguousarray(marks["reg_off"] if reg_off is None else reg_off, dtype=np.uint64)
        m = np.ascontiguousarray(marks["marks"], dtype=MARK_DT); lo = np.ascontiguousarray(marks["line_off"], dtype=np.uint64)
        co = np.ascontiguousarray(marks["cigar_reg_off"], dtype=np.uint64); cr = np.ascontiguousarray(marks["cigar_regs"], dtype=ALNREG_DT); cs = np.ascontiguousarray(marks["cigar_src"], dtype=np.uint32)
        a = np.ascontiguousarray(alns["alns"], dtype=ALN_DT); cg = np.ascontiguousarray(alns["cigar"], dtype=np.uint32); md = np.ascontiguousarray(alns["md"], dtype=np.uint8)
        bases = np.ascontiguousarray(bases, dtype=np.uint8); ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        q = None if quals is None else np.ascontiguousarray(quals, dtype=np.uint8)
        nm, no = pair(names)
        cm, cmo = pair(comments) if comments is not None else (None, None)
        ptr = lambda x: x.ctypes.data if x is not None and x.size else None
        n = lo.size - 1
        cmark = CMarkResult(n, m.size, int(lo[n]) if lo.size else 0, ptr(m), ptr(lo), CAlnResult(co.size - 1, cr.size, ptr(co), ptr(cr)), ptr(cs))
        ccig = CCigarResult(a.size, cg.size, md.size, ptr(a), ptr(cg), ptr(md))
        par = SamParams(int(flags) | (SAM_SOFTCLIP if softclip else 0), rg_id.encode() if isinstance(rg_id, str) else rg_id)
        out = CSamResult()
        _check(self.L.cs_regions_sam(self.h, C.byref(par), C.byref(cmark), ptr(reg_off), C.byref(ccig), ptr(bases), ptr(ro), ptr(q), nm.ctypes.data, ptr(no),
                                     cm.ctypes.data if cm is not None else None, ptr(cmo), C.byref(out)))
        return _view(out.text_off, "<u8", int(out.n_reads) + 1, True), (C.string_at(out.text, int(out.n_bytes)) if out.n_bytes else b"")

    def sam_header(self, rg_line=None):
        """cs_sam_header: the @SQ lines and, where given, the @RG line (as -R takes it: tabs written as a backslash and a t); host only"""
        rg = rg_line.encode() if isinstance(rg_line, str) else rg_line
        need = C.c_size_t()
        rc = self.L.cs_sam_header(self.h, rg, None, 0, C.byref(need))
        if rc != 0 and need.value == 0:
            _check(rc)
        buf = C.create_string_buffer(max(1, need.value))
        _check(self.L.cs_sam_header(self.h, rg, buf, need.value, C.byref(need)))
        return buf.raw[:need.value]

    def sam_stats(self):
        st = SamStats()
        _check(self.L.cs_sam_stats(self.h, C.byref(st)))
        return {n: (float(getattr(st, n)) if n == "kernel_ms" else int(getattr(st, n))) for n, _ in SamStats._fields_}

    def stats(self):
        st = AlnStats()
        _check(self.L.cs_aligner_stats(self.h, C.byref(st)))
        return {n: (float(getattr(st, n)) if n == "ext_kernel_ms" else int(getattr(st, n))) for n, _ in AlnStats._fields_}

    def close(self):
        if self.h:
            self.L.cs_aligner_destroy(self.h)
            self.h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass


def map_params_split(params=None):
    """cs_map_params_split: a MapParams (None: the defaults) as the stages take it -> dict(seed=Params, chain=ChainParams, flt=FltParams, aln=AlnParams,
    dedup=DedupParams, mark=MarkParams, mark_flags=int, sam=SamParams)"""
    params = params if params is not None else MapParams()
    out = dict(seed=Params(), chain=ChainParams(), flt=FltParams(), aln=AlnParams(), dedup=DedupParams(), mark=MarkParams(), sam=SamParams())
    mf = C.c_uint32()
    _check(load_library().cs_map_params_split(C.byref(params), C.byref(out["seed"]), C.byref(out["chain"]), C.byref(out["flt"]), C.byref(out["aln"]), C.byref(out["dedup"]),
                                              C.byref(out["mark"]), C.byref(mf), C.byref(out["sam"])))
    out["mark_flags"] = int(mf.value)
    return out


class Mapper:
    """cs_mapper_t: reads to SAM text in one call -- one engine, one device chainer and one aligner on `device`, the index loaded from `prefix`"""

    def __init__(self, prefix, device=0, engine_options=None, params=None):
        self.L = load_library()
        self.h = C.c_void_p()
        self._flying = []                                                   # the arrays of the batches submitted and not yet collected
        _check(self.L.cs_mapper_create(os.fsencode(prefix), int(device), C.byref(engine_options) if engine_options is not None else None,
                                       C.byref(params) if params is not None else None, C.byref(self.h)))

    @staticmethod
    def _arrays(bases, read_offsets, names, quals, comments):
        """the arrays of a batch as the library takes them, and its pointer arguments (n_reads .. comment_off)"""
        def pair(x):
            if isinstance(x, (list, tuple)) and (len(x) != 2 or isinstance(x[0], (bytes, str))):
                x = [y.encode() if isinstance(y, str) else y for y in x]
                off = np.zeros(len(x) + 1, np.uint64)
                off[1:] = np.cumsum([len(y) for y in x])
                x = (np.frombuffer(b"".join(x), np.uint8), off)
            b = np.ascontiguousarray(x[0], dtype=np.uint8)
            return (b if b.size else np.zeros(1, np.uint8)), np.ascontiguousarray(x[1], dtype=np.uint64)
        bases = np.ascontiguousarray(bases, dtype=np.uint8); ro = np.ascontiguousarray(read_offsets, dtype=np.uint64)
        q = None if quals is None else np.ascontiguousarray(quals, dtype=np.uint8)
        nm, no = pair(names)
        cm, cmo = pair(comments) if comments is not None else (None, None)
        ptr = lambda x: x.ctypes.data if x is not None and x.size else None
        return (bases, ro, q, nm, no, cm, cmo), (ro.size - 1, ptr(bases), ptr(ro), ptr(q), nm.ctypes.data, ptr(no), cm.ctypes.data if cm is not None else None, ptr(cmo))

    def map_batch(self, bases, read_offsets, names, quals=None, comments=None, id_base=0):
        """cs_map_batch: `names` / `comments` pairs (bytes as uint8, uint64 CSR offsets) or lists of bytes, `quals` uint8 at the bases' offsets,
        `id_base` the number of reads before this batch -> (text_off, text) as Aligner.regions_sam returns them"""
        _keep, args = self._arrays(bases, read_offsets, names, quals, comments)
        out = CSamResult()
        _check(self.L.cs_map_batch(self.h, *args, int(id_base), C.byref(out)))
        return _view(out.text_off, "<u8", int(out.n_reads) + 1, True), (C.string_at(out.text, int(out.n_bytes)) if out.n_bytes else b"")

    def submit(self, bases, read_offsets, names, quals=None, comments=None, id_base=0):
        """cs_map_submit: map_batch's arguments; queues the batch and returns (at most MAP_MAX_IN_FLIGHT uncollected).  The mapper keeps
        references to the batch's arrays until its collect."""
        keep, args = self._arrays(bases, read_offsets, names, quals, comments)
        _check(self.L.cs_map_submit(self.h, *args, int(id_base)))
        self._flying.append(keep)

    def collect(self, copy=True):
        """cs_map_collect: blocks until the OLDEST submitted batch is complete -> (text_off, text) as map_batch returns them; with copy=False
        text_off and text (uint8) are views of the mapper's arrays, valid until the next collect, map_batch or close.  A batch that failed
        in a stage raises here, and is collected by that."""
        out = CSamResult()
        rc = self.L.cs_map_collect(self.h, C.byref(out))
        if self._flying:
            self._flying.pop(0)                                             # (a batch's error collects it too)
        _check(rc)
        if not copy:
            return _view(out.text_off, "<u8", int(out.n_reads) + 1, False), _view(out.text, np.uint8, int(out.n_bytes), False)
        return _view(out.text_off, "<u8", int(out.n_reads) + 1, True), (C.string_at(out.text, int(out.n_bytes)) if out.n_bytes else b"")

    def in_flight(self):
        """cs_mapper_in_flight -> (submitted and not yet collected, how many of those are complete)"""
        s, f = C.c_int(), C.c_int()
        _check(self.L.cs_mapper_in_flight(self.h, C.byref(s), C.byref(f)))
        return int(s.value), int(f.value)

    def header(self, rg_line=None):
        """cs_mapper_header: the @SQ lines and, where given, the @RG line (as -R takes it: tabs written as a backslash and a t)"""
        rg = rg_line.encode() if isinstance(rg_line, str) else rg_line
        need = C.c_size_t()
        rc = self.L.cs_mapper_header(self.h, rg, None, 0, C.byref(need))
        if rc != 0 and need.value == 0:
            _check(rc)
        buf = C.create_string_buffer(max(1, need.value))
        _check(self.L.cs_mapper_header(self.h, rg, buf, need.value, C.byref(need)))
        return buf.raw[:need.value]

    def stats(self):
        """cs_mapper_stats: the counters, and stage_ms as a dict by step name (MAP_STAGES)"""
        st = MapStats()
        _check(self.L.cs_mapper_stats(self.h, C.byref(st)))
        out = {n: int(getattr(st, n)) for n, _ in MapStats._fields_ if n != "stage_ms"}
        out["stage_ms"] = {n: float(st.stage_ms[k]) for k, n in enumerate(MAP_STAGES)}
        return out

    def engine_stats(self):
        st = Stats()
        _check(self.L.cs_mapper_engine_stats(self.h, C.byref(st)))
        return st.asdict()

    def close(self):
        if self.h:
            self.L.cs_mapper_destroy(self.h)                                # (waits for the batches in flight)
            self.h = C.c_void_p()
            self._flying = []

    def __del__(self):
        try:
            self.close()
        except Exception:  # noqa: BLE001
            pass
