"""compseed_amd -- MI355X-native compressive SMEM seeding (host-side Python mirror of include/compseed_amd.h).

The product is the HIP library `libcompseed_amd.so` behind a plain C ABI; this package only binds it with ctypes
so that tests, bench.py and Python callers can drive the same entry points a C/C++ host (CompSeed's
seed_and_extend) would.  There is no CPU fallback: importing works anywhere, but creating an
Engine without the built library or without a GPU raises.
"""
from . import binding  # noqa: F401
from .binding import (CSError, Engine, EngineOptions, Index, Params, Result, Stats, lib_path, load_library, build_library,  # noqa: F401
                      disable_mask, pinned_array, pack_reads, RefSeq, Reader, Chainer, ChainParams, FltParams, DedupParams, build_index_from_fasta, unpack_mems16, unpack_mems8, unpack_mems, RESULT_LEAN, MEM_FULL32, MEM_PACKED16, MEM_LEAN8, MEM8_DT, INTV_DT, SEED_DT, MEM16_DT,
                      Extender, ExtParams, EXT_PAIR_DT, EXT_RES_DT, packed_rbeg, Aligner, AlnParams, ALNREG_DT, CHAIN_DT,
                      ChainStats, CHAIN_TREE_ONLY, download_chains, FltStats, FLT_WAVE_ONLY, ALN_DEV_COMPACT, EXT_VECTOR_ZDROP, download_regions,
                      MarkParams, MarkStats, MARK_DT, MARK_ALL, MARK_NO_MULTI, MARK_KEEP_SUPP_MAPQ, MARK_NO_LIGHT_PATH, MARK_FROM_HBM,
                      SamParams, SamStats, SAM_SOFTCLIP, SAM_WAVE_ONLY,
                      Mapper, MapParams, MapStats, map_params_split, MAP_ALL, MAP_NO_MULTI, MAP_KEEP_SUPP_MAPQ, MAP_SOFTCLIP, MAP_STAGES, MAP_MAX_IN_FLIGHT)

__all__ = ["CSError", "Engine", "EngineOptions", "Index", "Params", "Result", "Stats", "lib_path", "load_library", "build_library",
           "disable_mask", "pinned_array", "pack_reads", "RefSeq", "Reader", "Chainer", "ChainParams", "FltParams", "DedupParams", "build_index_from_fasta", "unpack_mems16", "unpack_mems8", "unpack_mems", "RESULT_LEAN", "MEM_FULL32", "MEM_PACKED16", "MEM_LEAN8", "MEM8_DT", "INTV_DT", "SEED_DT", "MEM16_DT",
           "Extender", "ExtParams", "EXT_PAIR_DT", "EXT_RES_DT", "packed_rbeg", "Aligner", "AlnParams", "ALNREG_DT", "CHAIN_DT",
           "ChainStats", "CHAIN_TREE_ONLY", "download_chains", "FltStats", "FLT_WAVE_ONLY", "ALN_DEV_COMPACT", "EXT_VECTOR_ZDROP", "download_regions",
           "MarkParams", "MarkStats", "MARK_DT", "MARK_ALL", "MARK_NO_MULTI", "MARK_KEEP_SUPP_MAPQ", "MARK_NO_LIGHT_PATH", "MARK_FROM_HBM",
           "SamParams", "SamStats", "SAM_SOFTCLIP", "SAM_WAVE_ONLY",
           "Mapper", "MapParams", "MapStats", "map_params_split", "MAP_ALL", "MAP_NO_MULTI", "MAP_KEEP_SUPP_MAPQ", "MAP_SOFTCLIP", "MAP_STAGES", "MAP_MAX_IN_FLIGHT"]
