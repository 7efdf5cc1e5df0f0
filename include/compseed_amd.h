/* compseed_amd.h -- C ABI of the MI355X-native compressive SMEM seeding engine.
 *
 * This is the drop-in boundary for ONE path of i-xiaohu/CompSeed: per-read SMEM collection over the FM-index
 * plus the suffix-array lookup that turns the intervals into seeds, i.e. the two blocks
 *     "Collect exact matches"  mapping/comp_seed.cpp:2247-2304   (== mem_collect_intv, mapping/bwamem.c:218-272)
 *     "SAL"                    mapping/comp_seed.cpp:2306-2347
 * of seed_and_extend(), called once per chunk from mem_process_seqs (comp_seed.cpp:2527).  The reference has no
 * FFI of its own (everything is statically linked); INTEGRATION.md shows the 20-line patch that makes
 * seed_and_extend() consume this API.  Plain C types only: no torch, no HIP types, no C++.
 *
 * All functions return 0 on success or a negative CS_E* code; cs_last_error() gives the message for the calling
 * thread.  Nothing in here aborts the process (the reference aborts/exits on error: bwalib/utils.c:92-124).
 * An engine is bound to one GPU and must be driven by one host thread at a time; engines are independent.
 */
#ifndef COMPSEED_AMD_H
#define COMPSEED_AMD_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CS_OK          0
#define CS_EINVAL     -1   /* bad argument                                   */
#define CS_EIO        -2   /* index file missing / truncated / inconsistent  */
#define CS_ENOMEM     -3   /* host or device allocation failed               */
#define CS_EDEVICE    -4   /* HIP runtime error (no GPU, launch failure ...) */
#define CS_ERANGE     -5   /* index or read too large for the device layout  */

/* bi-interval; identical layout and meaning to bwtintv_t (FM_index/bwt.h:62-64):
 * x0 = SA start of the match, x1 = SA start of its reverse complement, x2 = occurrences,
 * info = (query begin << 32) | query end for a finished mem (comp_seed.cpp:127). */
typedef struct { uint64_t x0, x1, x2, info; } cs_intv_t;

/* seed = the fields of mem_seed_t that seeding fills (mapping/comp_seed.h:77-83; score == len, aln unused) */
typedef struct { int64_t rbeg; int32_t qbeg, len; } cs_seed_t;

/* read-only view of the FM-index arrays a bwt_t holds (FM_index/bwt.h:48-60).  `bwt` is the interleaved
 * Occ/BWT array exactly as stored in <prefix>.bwt (64-byte blocks, bwt.h:73-80); `sa` is the sampled suffix
 * array with sa[0] == (uint64_t)-1 as bwt_restore_sa leaves it (bwt.c:437). */
typedef struct {
	uint64_t primary;
	uint64_t L2[5];
	uint64_t seq_len;
	uint64_t bwt_size;      /* number of 32-bit words in bwt */
	const uint32_t *bwt;
	uint64_t sa_intv;       /* power of two, 32 for bwaidx-built indexes */
	uint64_t n_sa;
	const uint64_t *sa;
} cs_index_view_t;

/* the mem_opt_t fields the seeding path reads (mapping/comp_seed.h:50-59), CLI flags in brackets */
typedef struct {
	int32_t  min_seed_len;   /* [-k] 19   */
	float    split_factor;   /* [-r] 1.5  */
	int32_t  split_width;    /* [-s] 10   */
	int32_t  max_occ;        /* [-c] 500  */
	uint64_t max_mem_intv;   /* [-y] 20   */
	int32_t  want_sal;       /* 1: also produce seeds (SAL block), 0: mems only */
	int32_t  sst_mode;       /* 1: on-device SST (LDS-resident memo of bwt_extend, mapping/SST.h) on [default], 0: off.
	                          * Results are identical either way; only speed and the bwt_calls counter differ */
	uint32_t disable;        /* bit mask of CS_DISABLE_*: switch single exact shortcuts off for this call (A/B parity tests,
	                          * profiling).  0 [default] = everything the engine was created with is used */
	uint32_t count_traffic;  /* 1: run the instantiations of the SMEM kernels that count their index-side accesses
	                          * (cs_engine_traffic_model); same results, a few per cent slower.  0 [default] */
	uint32_t result_flags;   /* bit mask of CS_RESULT_*: what the caller will not read of the results.  0 [default] = everything is
	                          * delivered; an unknown bit gives CS_EINVAL from every seed entry point */
	uint32_t reserved;       /* must be 0 (CS_EINVAL otherwise) */
} cs_params_t;

/* cs_params_t.result_flags.  CS_RESULT_LEAN: "I will not read x0 / x1 of the mems" -- nothing behind SAL does (chaining reads x2 and
 * info, comp_seed.cpp:241-285).  x1 then reads 0 in every mem every entry point hands out: the inverse-SA reads that only made it are
 * not issued and the kernels that write the sorted mems store 0, so a lean result is the same whatever `disable`, `sst_mode` or the
 * engine options are, like any other.  The packed host variants send a mem as 8 bytes instead of 16 (CS_MEM_LEAN8 below), x0 == 0
 * after cs_unpack_mem and in cs_engine_seed_batch's arrays; in device results and where CS_MEM_FULL32 applies x0 stays as computed.
 * mem_off, x2, info, seed_off, the seeds and the cs_stats_t counters are bit for bit those of result_flags 0. */
#define CS_RESULT_LEAN 1u

/* cs_params_t.disable: every mechanism below is exact; switching one off changes speed and counters only */
#define CS_DISABLE_TEXT_MODE    0x01u  /* unique forward matches compared against the 2-bit text instead of the FM index      */
#define CS_DISABLE_R2_TEXT      0x02u  /* re-seeding calls of unique SMEMs answered from rep[] / lcp[] / inverse SA           */
#define CS_DISABLE_TEXT_SWEEP   0x04u  /* backward sweeps bounded by the previous pivot read off the text                     */
#define CS_DISABLE_WINDOW       0x08u  /* window scheme for the backward sweeps (jump table + k-mer filter)                   */
#define CS_DISABLE_R3_TEXT      0x10u  /* round-3 seeds inside a mem taken from the text arrays                               */
#define CS_DISABLE_KMER_FILTER  0x20u  /* k-mer filter in front of the window lanes                                           */
#define CS_DISABLE_FWD0         0x40u  /* separate lean kernel for the calls at the first base of each read                   */
#define CS_DISABLE_FUSED_SAL    0x80u  /* sort and SAL in one pass over the mems, a read's SA slots counted while its mems are
                                        * emitted (max_occ <= 1024); off: the sort, a scan over the mems, then the SAL kernels   */
#define CS_DISABLE_MEM_POS      0x100u /* a unique mem's text position kept in the spare bits of its raw record, and in the side
                                        * word of its re-seeding call, where the emitting kernel holds it; off: the suffix array
                                        * is read again for it (sst_mode 0 implies it)                                           */

/* engine construction options: which derived arrays are materialised in HBM and how the working buffers are sized.
 * cs_engine_options_default() fills the defaults (in brackets).  Everything optional is also skipped automatically when
 * it does not fit next to the index; the mechanisms that need it are then off.  Results never depend on any of this. */
typedef struct {
	int32_t full_sa;          /* [1] full suffix array in HBM: SAL is one gather instead of a bwt_sa walk (bwt.c:86-96)       */
	int32_t sa64;             /* [0] 8-byte suffix-array / inverse-SA entries even below 2^32 rows (what hg19 scale uses)      */
	int32_t text_mode;        /* [1] 2-bit text + inverse suffix array (needs full_sa)                                        */
	int32_t text_arrays;      /* [1] lcp[] / rep[] byte arrays (needs text_mode): re-seeding and round 3 from the text        */
	int32_t jump_k;           /* [15] bi-interval table of every jump_k-mer, 6..15; 0 = none                                  */
	int32_t kmer_filter;      /* [1] filter over all min_seed_len-mers of the text for the window lanes                       */
	int32_t fused;            /* [0] 1: the fused one-lane-per-read kernel instead of the split forward/backward kernels      */
	int32_t mem_cap;          /* [64] mems per read held in the first-pass arena (more go through the overflow records)       */
	int64_t lep_arena_mb;     /* [16384] arena of the forward passes' left-extension points, per pass context; smaller = more chunks per pass */
	int64_t max_raw_mb;       /* [24576] first-pass mem arena; smaller = a batch is processed in more sub-batches             */
	int32_t r3_text_iter;     /* [5] forward launch after which round 3 starts on its side stream                             */
	int32_t pipeline_reads;   /* [5000000] reads per sub-batch of the host variants (cs_engine_seed_batch, _packed): upload of the next,
	                           *     seeding of the current and download of the previous sub-batch overlap; 0 = the whole batch at once */
	int32_t expand_threads;   /* [16] host threads that expand packed results in cs_engine_seed_batch                         */
	int32_t count_sal_merged; /* [0] 1: also count the distinct SA slots per 512 reads (cs_stats_t.sal_calls as the reference
	                           *     counts them, comp_seed.cpp:2327-2345); costs one sort of the slots per call              */
	int32_t verbose;          /* [0] progress lines on stderr                                                                 */
	int32_t host_pack_threads;/* [8] host variants: the reads are turned into the kernels' 16-byte / 32-base records by this many
	                           *     host threads and cross PCIe as 0.6 bytes per base; 0 = upload the caller's bytes, pack on the GPU */
	int32_t passes_in_flight; /* [2] seeding passes the engine runs at the same time (parts of a blocking call, batches of a stream, device
	                           *     batches of cs_engine_submit_device): the thin tail of one pass is filled by the next.  2 costs a second
	                           *     set of working buffers (allocated on first use); 1 = one pass at a time                          */
	int32_t sa40;             /* [0] 1: the full suffix array and the inverse suffix array as 40-bit entries, three to a 16-byte group
	                           *     (5.33 instead of 8 bytes per row: 33 GB less at hg19 scale), whatever the index size; sa64 is then
	                           *     ignored.  Needs full_sa; an index of 2^40 rows or more gives CS_ERANGE                          */
	int32_t reserved[2];      /* must be 0 */
} cs_engine_options_t;

/* CSR result of one batch.  Read r owns mems[mem_off[r] .. mem_off[r+1]) sorted by info (comp_seed.cpp:2301) and
 * seeds[seed_off[r] .. seed_off[r+1]) in mem-then-slot order (comp_seed.cpp:2311-2325).  The arrays belong to the
 * engine and stay valid until the next seed call on the same engine or its destruction. */
typedef struct {
	int64_t   n_reads;
	uint64_t  n_mems, n_seeds;
	const uint64_t  *mem_off;   /* n_reads + 1 */
	const cs_intv_t *mems;
	const uint64_t  *seed_off;  /* n_reads + 1; NULL when want_sal == 0 */
	const cs_seed_t *seeds;
} cs_result_t;

/* counters in the spirit of display_profile (main.cpp:203-214), accumulated over the engine's lifetime */
typedef struct {
	uint64_t reads, bases, mems, seeds;
	uint64_t bwt_queries;      /* bwt_extend queries evaluated on the device ("BWT-extend queries"); equals the
	                              reference's count unless re-seeding calls were answered from the text (below)  */
	uint64_t bwt_calls;        /* of those, served from HBM/L2, i.e. not by the on-device SST               */
	uint64_t sal_queries;      /* SA slots requested                                                        */
	uint64_t sal_calls;        /* distinct SA slots per 512 consecutive reads (what CompSeed looks up after merging,
	                              comp_seed.cpp:2327-2345) when the engine was created with count_sal_merged;
	                              otherwise == sal_queries.  The device looks every slot up: one gather each      */
	uint64_t overflow_mems;    /* mems beyond a read's first mem_cap (split kernels), or reads that needed the
	                              large-capacity second pass (fused kernel)                                        */
	double   seed_kernel_ms;   /* accumulated HIP-event time of the first-pass SMEM kernel launches         */
	double   sal_kernel_ms;    /* ... of the SAL kernels; where sort and SAL are one pass over the mems (the default
	                              with a full suffix array, CS_DISABLE_FUSED_SAL), of that pass: the per-read sort,
	                              which no field times otherwise, is then inside                            */
	double   total_ms;         /* ... of whole seed calls, first launch to last                             */
	uint64_t seed_kernel_launches;
	double   overflow_kernel_ms;       /* ... of the second-pass SMEM launches over overflowed reads        */
	uint64_t overflow_kernel_launches;
	uint64_t reseed_text_calls;        /* re-seeding calls (bwamem.c:241-249) answered from the text arrays
	                                      instead of the FM index: same SMEMs, their bwt_extend queries never run */
	uint64_t reseed_index_calls;       /* re-seeding calls of unique SMEMs that had to stay on the FM index       */
	uint64_t sweep_text_calls;         /* round-1 calls whose backward sweep (bwt.c:325-345) was read off the text  */
	uint64_t r3_text_seeds;            /* round-3 seeds (bwt.c:357-381) whose bi-interval came from the text arrays  */
} cs_stats_t;

typedef struct cs_index  cs_index_t;   /* host copy of an index loaded from files */
typedef struct cs_engine cs_engine_t;

const char *cs_last_error(void);
const char *cs_version(void);

void cs_params_default(cs_params_t *p);                     /* mem_opt_init, comp_seed.cpp:26-58 */

/* ---- index files: <prefix>.bwt and <prefix>.sa in the reference's formats (bwt_restore_bwt / bwt_restore_sa,
 *      FM_index/bwt.c:421-462; prefix inference as bwa_idx_infer_prefix, bwalib/bwa.c:244) */
int  cs_index_load(const char *prefix, cs_index_t **out);
int  cs_index_view(const cs_index_t *idx, cs_index_view_t *view);
void cs_index_free(cs_index_t *idx);

/* ---- index construction on the GPU (replaces `bwaidx`, FM_index/index_main.c:257-325, for the .bwt/.sa pair):
 *      `fwd_nt4` = forward strand, one base per byte, codes 0..3 (ambiguous bases already replaced, as
 *      bns_fasta2bntseq does with lrand48, bntseq.c:295); the reverse complement is appended internally.
 *      cs_index_save writes <prefix>.bwt / <prefix>.sa byte-identical to bwt_dump_bwt / bwt_dump_sa (bwt.c:385-407). */
int  cs_index_build(const uint8_t *fwd_nt4, uint64_t l_pac, int device, cs_index_t **out);
#define CS_BUILD_FORCE_64BIT 1u   /* run the 64-bit suffix sorter on a genome that would fit 32 bits (tests) */
#define CS_BUILD_VERBOSE     2u
int  cs_index_build_flags(const uint8_t *fwd_nt4, uint64_t l_pac, int device, uint32_t flags, cs_index_t **out);
int  cs_index_save(const cs_index_t *idx, const char *prefix);

/* ---- reference sequences: the FASTA front end of the builder and the other three index files.  cs_refseq_from_fasta reads FASTA / FASTQ
 *      (plain or gzip) as bns_fasta2bntseq does (FM_index/bntseq.c:280-330): contig table, holes (runs of one ambiguity code), and the
 *      forward strand as codes 0..3 with every ambiguous base replaced by lrand48() & 3 after srand48(11) (bntseq.c:266,295);
 *      cs_refseq_save writes <prefix>.pac / .ann / .amb byte-identical to bwaidx (bns_dump, bntseq.c:65-95);
 *      cs_index_build_fasta is bwa_idx_build (index_main.c:257-325): all five files from a FASTA, the suffix sort on the GPU. */
typedef struct cs_refseq cs_refseq_t;
int  cs_refseq_from_fasta(const char *path, cs_refseq_t **out);
int  cs_refseq_codes(const cs_refseq_t *r, const uint8_t **fwd_nt4, uint64_t *l_pac, int32_t *n_seqs, int32_t *n_holes);
int  cs_refseq_save(const cs_refseq_t *r, const char *prefix);
void cs_refseq_free(cs_refseq_t *r);
int  cs_index_build_fasta(const char *fasta, const char *prefix, int device);

/* ---- engine: uploads the index to GPU `device` once (replaces bwa_idx_load_from_shm's role: HBM residency) */
int  cs_device_count(int *n);
void cs_engine_options_default(cs_engine_options_t *o);
int  cs_engine_create(const cs_index_view_t *index, int device, cs_engine_t **out);            /* default options */
int  cs_engine_create_opts(const cs_index_view_t *index, int device, const cs_engine_options_t *opts, cs_engine_t **out);
void cs_engine_destroy(cs_engine_t *e);

/* ---- the hot path.  `bases` holds the reads back to back (ASCII or already nt4-coded 0..4, as CompSeed accepts:
 *      comp_seed.cpp:2258-2260); read r is bases[offsets[r] .. offsets[r+1]).  The caller's buffers are not modified
 *      (the reference overwrites seq in place).  Host variant: pointers are host memory, results land in pinned host
 *      memory.  Device variant: pointers are device memory on the engine's GPU and the result arrays are device
 *      pointers (no PCIe traffic inside the call).  The engine works on streams of its own: device inputs must be
 *      COMPLETE when the call is made (synchronise the stream that produced them first), d_offsets[0] must be 0 and
 *      d_offsets[n_reads] == n_bases (checked: CS_EINVAL); results are complete when the call returns.  Nothing behind
 *      d_bases[n_bases - 1] is read. */
int  cs_engine_seed_batch(cs_engine_t *e, const cs_params_t *par, int64_t n_reads,
                          const uint8_t *bases, const uint64_t *offsets, cs_result_t *out);
int  cs_engine_seed_batch_device(cs_engine_t *e, const cs_params_t *par, int64_t n_reads,
                                 const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_bases, cs_result_t *out);
/* The device variant as a stream of batches, up to TWO in flight (cs_engine_options_t.passes_in_flight): batch n is seeded on pass
 * context n & 1 -- a second set of streams and working buffers over the same index -- so the thin tail of one pass (late iterations,
 * sort, SAL, host round trips) runs beside the dense start of the next; this is how a worker that keeps its reads in HBM drives the engine
 * (the reference's kt_for over chunks of a batch, comp_seed.cpp:2541-2548, is the same overlap on CPU threads).  Inputs as for
 * cs_engine_seed_batch_device, and they must stay untouched until their batch has been collected.  Results come back in submission
 * order; the device pointers of a collected batch stay valid until the SECOND submit after its collect, whatever the order of submits
 * and collects and for both values of passes_in_flight: a consumer may work on batch n while batch n+1 -- and, with two in flight,
 * n+2 -- is being seeded.  The engine keeps ONE result set more than it has pass contexts for this: a collect exchanges the four result
 * arrays of the batch's context with that spare set and hands out the spare set's pointers, so a collected batch is in no context until
 * the next collect (cost: the result arrays of one more batch, 32 bytes per mem + 16 per seed + 16 per read at the size of the largest
 * batch; cs_engine_memory counts it within pass_ctx[0]).  A batch whose collect returns an error hands nothing out and does not shorten
 * the life of an earlier result.  A blocking seed call or a cs_engine_submit once the stream is drained ends the validity of every
 * collected device result (the "until the next seed call" rule of cs_engine_seed_batch_device) and frees the spare set, which the
 * next collect of a device stream fills again.
 * While device batches are in flight the other entry points that use the device return CS_EINVAL.  Threads: as for cs_engine_submit /
 * cs_engine_collect_packed -- one submitting thread, one collecting thread. */
int  cs_engine_submit_device(cs_engine_t *e, const cs_params_t *par, int64_t n_reads,
                             const uint8_t *d_bases, const uint64_t *d_offsets, uint64_t n_bases);
int  cs_engine_collect_device(cs_engine_t *e, cs_result_t *out);

/* ---- packed results: what actually crosses PCIe.  A 10 M-read batch produces ~80 M mems and ~200 M seeds, 5.9 GB as cs_intv_t /
 *      cs_seed_t -- more transfer time than seeding time -- but half of those bytes are implied: a seed's qbeg and len are its
 *      mem's, a mem's seeds are its first min(x2, max_occ) slots (comp_seed.cpp:2313-2325), and three 33-bit coordinates, a 32-bit
 *      size and two 15-bit query positions fit 16 bytes, a reference position 5.  cs_engine_seed_batch_packed returns that form in pinned host memory;
 *      a consumer that copies per read anyway (the reference does: aux.match[r] / aux.seed[r] are per-read vectors) unpacks on
 *      the fly in its own worker threads with the inline helpers below, and cs_engine_seed_batch is this call followed by a
 *      multi-threaded expansion into cs_intv_t / cs_seed_t arrays.  Both split the batch into sub-batches and overlap the upload
 *      of the next, the seeding of the current and the download (and expansion) of the previous one.
 *      mem_format CS_MEM_PACKED16 needs an index shorter than 2^33 symbols and reads shorter than 2^15 bases (hg19 / T2T, short
 *      reads); anything else comes back as CS_MEM_FULL32 (plain cs_intv_t); seeds as their rbeg in 40 bits either way.
 *      Under CS_RESULT_LEAN the mems travel as CS_MEM_LEAN8 exactly where CS_MEM_PACKED16 applies otherwise -- x2 and the two query
 *      positions in one word, x0 = x1 = 0 after unpacking -- and as CS_MEM_FULL32 with x1 = 0 elsewhere. */
#define CS_MEM_FULL32   0
#define CS_MEM_PACKED16 1
#define CS_MEM_LEAN8    2
typedef struct { uint64_t w0, w1; } cs_mem16_t;
/* w0 = x0 | (x2 & 0x7fffffff) << 33;   w1 = x1 | beg << 33 | end << 48 | (x2 >> 31) << 63 */
typedef struct { uint64_t w; } cs_mem8_t;
/* w = x2 | beg << 34 | end << 49   (x2 < 2^34: the index is shorter than 2^33 symbols; beg, end < 2^15) */
typedef struct {
	int64_t   n_reads;
	uint64_t  n_mems, n_seeds;
	int32_t   mem_format;        /* CS_MEM_PACKED16 or CS_MEM_FULL32; under CS_RESULT_LEAN: CS_MEM_LEAN8 or CS_MEM_FULL32 (x1 = 0) */
	int32_t   max_occ;           /* the -c the batch was seeded with: a mem owns min(x2, max_occ) consecutive entries of seed_rbeg */
	const uint64_t *mem_off;     /* n_reads + 1 */
	const void     *mems;        /* cs_mem16_t[n_mems], cs_mem8_t[n_mems] or cs_intv_t[n_mems], as mem_format says */
	const uint64_t *seed_off;    /* n_reads + 1, NULL when want_sal == 0 */
	int32_t   seed_format;       /* CS_SEED_RBEG40: a seed's rbeg as 40 bits in two planes (reference positions are below 2^37) */
	int32_t   reserved;
	const uint32_t *seed_rbeg_lo; /* n_seeds low words, in mem-then-slot order */
	const uint8_t  *seed_rbeg_hi; /* n_seeds fifth bytes: rbeg = lo | (int64_t)hi << 32 (cs_packed_seed_rbeg) */
} cs_packed_result_t;
#define CS_SEED_RBEG40 1
static inline int64_t cs_packed_seed_rbeg(const cs_packed_result_t *r, uint64_t i) { return (int64_t)((uint64_t)r->seed_rbeg_lo[i] | (uint64_t)r->seed_rbeg_hi[i] << 32); }
int  cs_engine_seed_batch_packed(cs_engine_t *e, const cs_params_t *par, int64_t n_reads,
                                 const uint8_t *bases, const uint64_t *offsets, cs_packed_result_t *out);
/* The same as a pipeline across batches, the counterpart of the reference's kt_pipeline (main.cpp:438: read chunk n+1 while chunk n is
 * processed and chunk n-1 written): cs_engine_submit queues a batch and returns at once (at most FOUR in flight; the caller's buffers
 * must stay untouched until the batch is collected), cs_engine_collect_packed blocks until the OLDEST submitted batch is complete.  With
 * batches kept submitted the upload of batch n+1, the seeding of batch n (of two batches at a time, on the engine's two pass contexts) and
 * the download of batch n-1 overlap, and throughput is that of the slowest stage instead of their sum.  How many to keep submitted: a batch
 * spends upload + seeding + download in the engine, and a new one enters only when the oldest has been collected, so the stream runs at
 * (that latency) / (batches in flight) per batch until the slowest stage takes over -- two in flight (what a two-thread kt_pipeline gives)
 * leave the engine idle half of the time, three to four keep it busy.  A collected result stays valid until the next collect or blocking
 * seed call.
 * While batches are in flight the engine's other entry points that use the device return CS_EINVAL (cs_engine_reset_stats does nothing).
 * Threads: cs_engine_submit may be called from ONE thread while cs_engine_collect_packed runs on ONE other thread (the reader and the
 * processing step of a kt_pipeline, main.cpp:60-126); everything else on an engine needs the caller's own serialisation. */
int  cs_engine_submit(cs_engine_t *e, const cs_params_t *par, int64_t n_reads, const uint8_t *bases, const uint64_t *offsets);
int  cs_engine_collect_packed(cs_engine_t *e, cs_packed_result_t *out);
static inline void cs_unpack_mem(const cs_packed_result_t *r, uint64_t i, cs_intv_t *m)
{
	if (r->mem_format == CS_MEM_PACKED16) {
		const cs_mem16_t p = ((const cs_mem16_t *)r->mems)[i];
		m->x0 = p.w0 & 0x1ffffffffull; m->x1 = p.w1 & 0x1ffffffffull;
		m->x2 = (p.w0 >> 33) | ((p.w1 >> 63) << 31);
		m->info = ((p.w1 >> 33) & 0x7fffull) << 32 | ((p.w1 >> 48) & 0x7fffull);
	} else if (r->mem_format == CS_MEM_LEAN8) {
		const uint64_t w = ((const cs_mem8_t *)r->mems)[i].w;
		m->x0 = 0; m->x1 = 0;
		m->x2 = w & 0x3ffffffffull;
		m->info = ((w >> 34) & 0x7fffull) << 32 | ((w >> 49) & 0x7fffull);
	} else *m = ((const cs_intv_t *)r->mems)[i];
}
static inline uint32_t cs_mem_seed_count(const cs_intv_t *m, int32_t max_occ) { return m->x2 < (uint64_t)max_occ ? (uint32_t)m->x2 : (uint32_t)max_occ; }
/* pinned host memory for the caller's read chunk (uploads from it are asynchronous and run at link speed; pageable memory works
 * too, through a staging thread) */
int  cs_host_alloc(size_t bytes, void **ptr);
int  cs_host_free(void *ptr);
/* What the host variants upload when cs_engine_options_t.host_pack_threads > 0: the reads as the records the seeding kernels read,
 * 16 bytes per 32 bases (words 0-1: the bases, 2 bits each, base j in bits 2j..2j+1; word 2: one bit per base that is ambiguous or lies
 * behind the end of the read; word 3: 0), record k of read r at (offsets[r] >> 5) + r + k, (offsets[n_reads] >> 5) + n_reads records in
 * all; letters as nst_nt4_table maps them (FM_index/bntseq.c:46-63), codes 0..3 as they are (comp_seed.cpp:2259).  Exported for tests. */
int  cs_pack_reads(const uint8_t *bases, const uint64_t *offsets, int64_t n_reads, void *records, int threads, uint32_t flags);
#define CS_PACK_SCALAR 1u         /* do not use the AVX2 / BMI2 code path */

/* ---- reordered-reads ingest: the reader step of the reference's pipeline (input_reorder_reads, main.cpp:36-58; FASTQ when the first
 *      byte is '@', main.cpp:399-406; plain or gzip), cutting chunks as main.cpp:54,437 does (the first even read count that reaches
 *      chunk_bases) and delivering them as the engine takes them: bases back to back in pinned memory + n_reads + 1 offsets.  Two
 *      chunk buffers alternate, so a chunk stays intact while the next one is read (submit chunk n+1, collect chunk n, read chunk n+2).
 *      n_reads == 0: end of input. */
typedef struct cs_reader cs_reader_t;
int  cs_reader_open(const char *path, int64_t chunk_bases, cs_reader_t **out);
int  cs_reader_next(cs_reader_t *r, const uint8_t **bases, const uint64_t **offsets, int64_t *n_reads);
void cs_reader_close(cs_reader_t *r);
/* The same chunks with everything a SAM record needs.  cs_reader_next_chunk cuts exactly where cs_reader_next cuts and uses the same two
 * alternating buffers (a chunk stays intact while the next one is read); a reader is driven by ONE of the two calls (CS_EINVAL for the
 * other).  Reordered reads: the name is the decimal of the 1-based running line number (main.cpp:47; has_input starts at 1), there are no
 * qualities and no comments.  FASTQ, as kseq and bseq_read do it (bwalib/bwa.c:53-60, 78-110): the name runs to the first white-space
 * byte, the comment is the rest of the header line after that one byte (empty where there is none), a trailing "/" + digit is trimmed
 * from a name longer than two bytes, the quality line is the qualities (at the bases' offsets; a length other than the sequence's gives
 * CS_EIO).  `first_id`: the number of reads before this chunk, cs_map_batch's id_base.  names / comments are CSR byte arrays of
 * n_reads + 1 offsets.  n_reads == 0: end of input. */
typedef struct { int64_t n_reads; uint64_t first_id; const uint8_t *bases; const uint64_t *offsets;
                 const uint8_t *quals;                              /* NULL for reordered-reads input */
                 const char *names; const uint64_t *name_off;
                 const char *comments; const uint64_t *comment_off; /* both NULL: the input has none */ } cs_read_chunk_t;
int  cs_reader_next_chunk(cs_reader_t *r, cs_read_chunk_t *out);

/* ---- seed -> chain hand-off: mem_chain of the reference (mapping/comp_seed.cpp:241-285) over the seeds of a whole batch, host code.
 *      A chain is a run of co-linear seeds on one reference sequence (test_and_merge, comp_seed.cpp:182-203); chains come out per read in
 *      the order the reference's B-tree traversal gives them, each with the fraction of the read covered by repetitive mems.  The contig
 *      table comes from <prefix>.ann.  `seeds` is a host-side result with seeds (want_sal = 1); read_offsets are the batch's offsets.
 *      The arrays of the result belong to the chainer and stay valid until its next call. */
typedef struct { int32_t w, max_chain_gap, min_seed_len, max_occ; } cs_chain_params_t;   /* mem_opt_t: -w 100, max_chain_gap 10000, -k, -c */
typedef struct { int64_t pos; int32_t rid, n_seeds; float frac_rep; int32_t is_alt; } cs_chain_t;
typedef struct {
	int64_t n_reads; uint64_t n_chains, n_seeds;
	const uint64_t *chain_off;     /* n_reads + 1 */
	const cs_chain_t *chains;
	const uint64_t *cseed_off;     /* n_chains + 1 */
	const cs_seed_t *cseeds;       /* the seeds of chain c: cseeds[cseed_off[c] .. cseed_off[c + 1]) */
} cs_chain_result_t;
typedef struct cs_chainer cs_chainer_t;
int  cs_chainer_create(const char *prefix, cs_chainer_t **out);
void cs_chainer_destroy(cs_chainer_t *c);
void cs_chain_params_default(cs_chain_params_t *p);
int  cs_chain_batch(cs_chainer_t *c, const cs_chain_params_t *par, const cs_result_t *seeds, const uint64_t *read_offsets, int n_threads,
                    cs_chain_result_t *out);
/* The same pass on the GPU, bit-identical to cs_chain_batch (which stays the specification).  cs_chainer_create_device gives a chainer that
 * still does everything a host chainer does and also holds device state on `device`: the contig offsets and ALT flags, uploaded once, and a
 * stream and buffers of its own (CS_EDEVICE without a GPU).  cs_chain_batch_device: `d_seeds` is a result as the engine's device variants
 * return it (device pointers on the chainer's GPU, host counts) and `d_read_offsets` the batch's offsets in device memory; inputs must be
 * COMPLETE when the call is made, as for cs_engine_seed_batch_device, and the results are complete when it returns.  The output CSR arrays
 * are device pointers owned by the chainer, valid until its next chain call; the counts are host values.  A result of
 * cs_engine_collect_device is to be chained before the next cs_engine_submit_device.  cs_chain_batch_gpu: the same work from host arrays to
 * host arrays (owned by the chainer, as cs_chain_batch's), byte for byte cs_chain_batch's result.  Both return CS_EINVAL for a result
 * without seeds (want_sal = 0) and for a chainer made by cs_chainer_create; n_reads == 0 gives an empty result.  cs_chainer_stats: counters
 * of the device calls over the chainer's life (zero for a host chainer). */
#define CS_CHAIN_TREE_ONLY 1u   /* A/B switch: every read through the exact B-tree path instead of the sorted-array fast path; same results */
typedef struct { uint64_t reads, seeds, chains, tree_reads, launches; double kernel_ms; } cs_chain_stats_t;   /* tree_reads: reads that went
                                                                                                                   * the B-tree path; kernel_ms: HIP-event time of the kernels */
int  cs_chainer_create_device(const char *prefix, int device, cs_chainer_t **out);
int  cs_chain_batch_device(cs_chainer_t *c, const cs_chain_params_t *par, const cs_result_t *d_seeds, const uint64_t *d_read_offsets, uint32_t flags,
                           cs_chain_result_t *d_out);
int  cs_chain_batch_gpu(cs_chainer_t *c, const cs_chain_params_t *par, const cs_result_t *seeds, const uint64_t *read_offsets, uint32_t flags,
                        cs_chain_result_t *out);
int  cs_chainer_stats(const cs_chainer_t *c, cs_chain_stats_t *st);

/* ---- the chain filters between chaining and extension (comp_seed.cpp:2364-2367), as host code and (below) as kernels: mem_chain_flt (comp_seed.cpp:297-360: chains
 *      by descending weight -- klib's introsort, whose order among equal weights is reproduced --, chains shadowed on the read by a much
 *      heavier one dropped, the first shadowed chain of each kept one retained) and mem_flt_chained_seeds (comp_seed.cpp:393-412: for reads
 *      of ~700 bases and more, short seeds whose neighbourhood does not reach a local alignment score of 5.5 ln(read length) are dropped and
 *      the others carry that score; ksw_align2's number, bwalib/ksw.c:343).  `in`: cs_chain_batch's result (or the caller's chains in that
 *      form); `out`: the surviving chains per read in the reference's order, `cseed_score` their seeds' scores -- what cs_extend_chains takes.
 *      `bases` / <prefix>.pac are read only when a read is long enough for the seed test.  The result belongs to the chainer and stays
 *      valid until its next cs_chain_filter. */
typedef struct { int32_t min_chain_weight, max_chain_extend, max_chain_gap, min_seed_len; float mask_level, drop_ratio;   /* mem_opt_t: min_chain_weight (-W), max_chain_extend, max_chain_gap, -k, mask_level, drop_ratio (-D) */
                 int32_t a, b, o_del, e_del, o_ins, e_ins; } cs_flt_params_t;                                              /* ... -A -B -O -E (the seed test) */
void cs_flt_params_default(cs_flt_params_t *p);
int  cs_chain_filter(cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *in, const uint8_t *bases, const uint64_t *read_offsets,
                     int n_threads, cs_chain_result_t *out, const int32_t **cseed_score);
/* The same two filters on the GPU (chain_filter_gpu.hip), byte for byte cs_chain_filter's result; cs_chain_filter stays the specification.
 * Both calls need a chainer from cs_chainer_create_device (CS_EINVAL otherwise).  cs_chain_filter_device: `d_in` is a chain result as
 * cs_chain_batch_device returns it (device pointers on the chainer's GPU, host counts), complete when the call is made; `d_bases` /
 * `d_read_offsets` are the batch's reads in device memory (ASCII or codes, n_reads + 1 offsets).  `d_bases` may be NULL only if no read with
 * chains is long enough for the seed test (found by a kernel; <prefix>.pac is loaded and uploaded only then, once per chainer).  Results are
 * complete when the call returns: `d_out` and `*d_cseed_score` are device arrays of the chainer's filter state, buffers of their own -- the
 * chainer's cs_chain_batch_device output, this call's usual input, is left as it is -- and stay valid until the chainer's next
 * cs_chain_filter_device / cs_chain_filter_gpu.  cs_chain_filter_gpu: the same work from host arrays to host arrays (owned by the chainer,
 * valid as long).  Passing a call's own previous output as input gives CS_EINVAL, unknown flag bits too; the parameter checks are
 * cs_chain_filter's; n_reads == 0 gives an empty result.  Inconsistent input (a chain without seeds, offsets that are not a CSR, a chain's
 * n_seeds that is not what cseed_off says) is found by the first kernels, which do not follow it, and reported as CS_EINVAL; a read of
 * 65,536 bases or more gives CS_ERANGE.  cs_chain_filter_stats: counters of both calls over the chainer's life (zero for a host chainer). */
#define CS_FLT_WAVE_ONLY 1u   /* A/B switch: every read through the wave-per-read path; same results */
typedef struct { uint64_t reads, chains_in, chains_out, seeds_in, seeds_out,
                 wave_reads,    /* reads that took the wave-per-read path            */
                 spill_reads,   /* ... of those, reads whose lists did not fit the LDS */
                 sw_seeds,      /* seeds scored by the local alignment (long reads)  */
                 launches; double kernel_ms; } cs_flt_stats_t;
int  cs_chain_filter_device(cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *d_in,
                            const uint8_t *d_bases, const uint64_t *d_read_offsets, uint32_t flags,
                            cs_chain_result_t *d_out, const int32_t **d_cseed_score);
int  cs_chain_filter_gpu(cs_chainer_t *c, const cs_flt_params_t *par, const cs_chain_result_t *in,
                         const uint8_t *bases, const uint64_t *read_offsets, uint32_t flags,
                         cs_chain_result_t *out, const int32_t **cseed_score);
int  cs_chain_filter_stats(const cs_chainer_t *c, cs_flt_stats_t *st);

/* ---- seed extension: the banded Smith-Waterman extensions of mem_chain2aln_across_reads_V2 (mapping/comp_seed.cpp:1319), i.e.
 *      what the reference hands to BandedPairWiseSW::getScores8 / getScores16 / scalarBandedSWAWrapper (mapping/bandedSWA.h:117-167; call sites
 *      comp_seed.cpp:1719,1790,1859,1942,2003,2074), computed on the GPU with the exact semantics of ksw_extend2 (bwalib/ksw.c:380-479): band of
 *      +-w diagonals that shrinks to the live columns, Z-drop, end bonus in the band limit only.  A cs_extender_t corresponds to a
 *      BandedPairWiseSW object (its constructor's parameters, bandedSWA.h:117-121); cs_ext_pair_t to the input fields of SeqPair (idq, idr,
 *      len2, len1, h0; bandedSWA.h:90-100) with 64-bit offsets into the two sequence buffers (codes 0..4, one byte per base; the query and
 *      target of a left extension reversed by the caller as comp_seed.cpp:1525,1546 do); cs_ext_result_t to its output fields.  All pairs of
 *      a call share the band width w (the reference calls once per band try: w, then 2w for the pairs whose max_off came close to the band,
 *      comp_seed.cpp:1740-1742).  Scoring: pairs the reference would send to its vectorised code (both lengths and h0 + min(len) * match
 *      below 32768, comp_seed.cpp:1569-1577) compare base codes -- ambiguous (4) on either side scores -1, equal codes mat[0], others mat[1]
 *      (bandedSWA.cpp:286-290) -- longer ones index the 5 x 5 matrix like ksw_extend2; the two only differ for codes above 4.
 *      Known deviation of the REFERENCE from its own definition, not reproduced: its vectorised code gives other numbers than ksw_extend2
 *      in a few pairs per thousand when o_del != o_ins or a gap extension is not 1 (tests/test_oracle_bsw.py); this library computes
 *      ksw_extend2's result for every parameter set.  Host variant: host pointers in, results in `out`; device variant: everything is device
 *      memory on the extender's GPU.  Pairs with qlen < 1, tlen < 0 or offsets outside the buffers get a zero result and the call returns
 *      CS_EINVAL after delivering the others. */
typedef struct { int8_t mat[25]; int32_t o_del, e_del, o_ins, e_ins, zdrop, end_bonus; uint32_t flags; } cs_ext_params_t;
/* flags.  Default 0: queries of up to 160 columns whose scores fit 15 bits (every extension of a 150-bp read) run one pair per LANE, the rest
 * one wavefront per pair, a query column per lane.  The others are A/B switches; every combination gives the same results. */
#define CS_EXT_PACKED16     1u   /* wave-per-pair only, queries longer than 64 bases through a kernel with two columns per lane (packed int16); exact, slower */
#define CS_EXT_PACKED16_ALL 2u   /* ... all queries of the 16-bit class through it */
#define CS_EXT_NO_LANES     4u   /* do not use the one-pair-per-lane kernel for short queries (A/B tests): every pair goes one wave per pair */
#define CS_EXT_LANES_QIN    8u   /* lane kernel, 8-bit class: the query base inside the score cell (one LDS read per cell, a third more LDS); exact; an experiment */
#define CS_EXT_VECTOR_ZDROP 16u  /* NOT an A/B switch: Z-drop as the reference's vectorised getScores8 / getScores16 test it (mapping/bandedSWA.cpp ZSCORE8 / ZSCORE16), for the
                                  * pairs of its two vector classes: the shift off the best cell's diagonal is not multiplied by the gap extension, and zdrop 0 does not
                                  * switch the test off.  The same function as ksw_extend2's at e_del = e_ins = 1 and zdrop > 0 (mem_opt_init); cs_extend_chains sets it,
                                  * because mem_chain2aln_across_reads_V2 extends through that code */
typedef struct { uint64_t q_off, t_off; int32_t qlen, tlen, h0, reserved; } cs_ext_pair_t;   /* reserved: not looked at (the caller's own tag, e.g. the region a pair belongs to) */
typedef struct { int32_t score, qle, tle, gtle, gscore, max_off; } cs_ext_result_t;
typedef struct { uint64_t pairs, cells, rows, launches; double kernel_ms; } cs_ext_stats_t;   /* cells = DP cells computed (inside the adaptive band) */
typedef struct cs_extender cs_extender_t;
void cs_ext_params_default(cs_ext_params_t *p);               /* mem_opt_init's scoring: a 1, b 4, o 6, e 1, zdrop 100, pen_clip 5 (comp_seed.cpp:26-58) */
int  cs_extender_create(int device, const cs_ext_params_t *par /* NULL: defaults */, cs_extender_t **out);
void cs_extender_destroy(cs_extender_t *x);
int  cs_extend_batch(cs_extender_t *x, int64_t n_pairs, const cs_ext_pair_t *pairs, const uint8_t *qbuf, uint64_t q_bytes,
                     const uint8_t *tbuf, uint64_t t_bytes, int32_t w, cs_ext_result_t *out);
int  cs_extend_batch_device(cs_extender_t *x, int64_t n_pairs, const cs_ext_pair_t *d_pairs, const uint8_t *d_qbuf, uint64_t q_bytes,
                            const uint8_t *d_tbuf, uint64_t t_bytes, int32_t w, cs_ext_result_t *d_out);
int  cs_extender_stats(const cs_extender_t *x, cs_ext_stats_t *st);
/* the band retries extend the same sequences again with another pair list: upload the two buffers once, then run pair lists against them.
 * cs_extend_batch leaves its own two buffers resident in the same way, so a resident call always runs against the sequences of the last host-form call. */
int  cs_extender_upload(cs_extender_t *x, const uint8_t *qbuf, uint64_t q_bytes, const uint8_t *tbuf, uint64_t t_bytes);
int  cs_extend_batch_resident(cs_extender_t *x, int64_t n_pairs, const cs_ext_pair_t *pairs, int32_t w, cs_ext_result_t *out);

/* ---- the extension stage as a whole: mem_chain2aln_across_reads_V2 (mapping/comp_seed.cpp:1319-2237), chains in, alignment regions out.
 *      For every seed of every chain (as the caller's chain filters left them: mem_chain_flt / mem_flt_chained_seeds, comp_seed.cpp:2364-2367,
 *      are the caller's) a region is opened, extended left and then right by banded Smith-Waterman on the GPU -- band w, once more with 2w
 *      where the alignment came within a quarter of the band's edge (MAX_BAND_TRY 2) --, and regions made redundant by an earlier region
 *      of the read are marked qb = qe = -1 (the caller drops them as comp_seed.cpp:2387-2393 does).  cs_alnreg_t holds the fields of
 *      mem_alnreg_t this stage fills (comp_seed.h:106-125); `chain` is the index of the region's chain within its read.  Regions come in the
 *      reference's order: chain by chain, seeds by descending score.  `chains`: the chains as a cs_chain_result_t -- cs_chain_batch's output or the caller's
 *      own --, `cseed_score` the chained seeds' scores in the same order (NULL: score = len, what mem_chain leaves), `bases` / `read_offsets` the
 *      batch's reads (ASCII or codes; a '-' is code 5 as in nst_nt4_table).  The aligner loads <prefix>.ann / .alt / .pac.  The result arrays
 *      belong to the aligner and stay valid until its next call.  pen_clip5 must equal pen_clip3 for now. */
typedef struct { int32_t a, b, o_del, e_del, o_ins, e_ins, pen_clip5, pen_clip3, w, zdrop; /* mem_opt_t: -A -B -O -E -L -w -d */
                 int32_t threads;   /* [16] host threads of the passes around the kernels (cs_dedup_regions) */
                 uint32_t flags;    /* [0] CS_ALN_* below: A/B switches of cs_extend_chains, every combination gives the same regions */ } cs_aln_params_t;
#define CS_ALN_NO_LIGHT_PATHS 1u   /* every chain through the wave-per-chain region kernel, every read through the LDS purge kernel (default: chains of up to 8 seeds a lane
                                    * each, reads of up to 64 regions a wave each in registers) */
#define CS_ALN_PURGE_FROM_HBM 2u   /* reads of more than 64 regions purged straight from HBM: the fallback for a read whose regions do not fit the LDS (3,000) */
typedef struct { int64_t rb, re; int32_t qb, qe, rid, score, truesc, w, seedcov, seedlen0; float frac_rep; int32_t chain; } cs_alnreg_t;
typedef struct { int64_t n_reads; uint64_t n_regs; const uint64_t *reg_off; const cs_alnreg_t *regs; } cs_aln_result_t;
typedef struct { uint64_t reads, regions, pairs, retries, purged, launches;   /* pairs = extensions run incl. retries */
                 uint64_t ext_cells; double ext_kernel_ms; } cs_aln_stats_t;     /* of the extension kernels: DP cells inside the adaptive band, HIP-event time */
typedef struct cs_aligner cs_aligner_t;
void cs_aln_params_default(cs_aln_params_t *p);
int  cs_aligner_create(const char *prefix, int device /* -1: host-side passes only (cs_dedup_regions), no GPU needed */, const cs_aln_params_t *par /* NULL: defaults */, cs_aligner_t **out);
void cs_aligner_destroy(cs_aligner_t *a);
int  cs_extend_chains(cs_aligner_t *a, const cs_chain_result_t *chains, const int32_t *cseed_score, const uint8_t *bases,
                      const uint64_t *read_offsets, cs_aln_result_t *out);
/* The same stage over device-resident chains: `d_chains` is a chain result as cs_chain_filter_device or cs_chain_batch_device returns it
 * (device pointers on the aligner's GPU, host counts), `d_cseed_score` (may be NULL: score = len), `d_bases` and `d_read_offsets` are
 * device memory; inputs must be COMPLETE when the call is made, as for the other device calls, and are not written.  `d_out->reg_off`
 * (n_reads + 1) and `d_out->regs` are device arrays owned by the aligner, complete when the call returns and valid until the aligner's
 * next cs_extend_chains or cs_extend_chains_device; n_reads and n_regs are host values.  flags 0: byte for byte what cs_extend_chains
 * returns for the same chains (purged regions as qb = qe = -1, reg_off[r] = cseed_off[chain_off[r]]).  CS_ALN_DEV_COMPACT: the purged
 * regions are left behind on the device -- each read's regions with qe > qb in unchanged order, reg_off counts them, n_regs is their
 * number -- which is what cs_dedup_regions drops first anyway.  cs_aln_params_t.flags keep their meaning, and the call adds to the same
 * cs_aln_stats_t counters (`regions` counts the regions before compaction).  Errors, in this order: a NULL `a`, `d_chains` or `d_out`
 * or unknown flag bits CS_EINVAL; cs_extend_chains' pointer conditions, read as device pointers, CS_EINVAL; an aligner created with device
 * -1 CS_EDEVICE; pen_clip5 != pen_clip3 CS_EINVAL; 2^31 seeds or more CS_ERANGE; inconsistent device input -- chain_off / cseed_off that
 * are not CSR offset arrays from 0 to n_chains / n_seeds or disagree with the chains' n_seeds, read_offsets that do not start at 0 or decrease, a read with chains of
 * 65,536 bases or more -- CS_EINVAL, found by checking kernels before any kernel follows an offset; a chain whose first seed lies outside
 * the reference CS_EINVAL.  After any error the aligner is usable for the next call. */
#define CS_ALN_DEV_COMPACT 1u   /* drop the regions with qe <= qb on the device (comp_seed.cpp:2387-2393) */
int  cs_extend_chains_device(cs_aligner_t *a, const cs_chain_result_t *d_chains, const int32_t *d_cseed_score /* may be NULL: score = len */,
                             const uint8_t *d_bases, const uint64_t *d_read_offsets, uint32_t flags, cs_aln_result_t *d_out);
/* The pass behind the extension stage (comp_seed.cpp:2385-2395), host code: regions marked by the purge (qe <= qb) are dropped and
 * mem_sort_dedup_patch (comp_seed.cpp:629-687) runs over each read's rest -- of two regions that overlap by more than mask_level_redun on
 * read and reference the lower-scoring one goes; colinear neighbours close to one diagonal are merged when a banded global alignment over
 * both (bwa_gen_cigar2 / ksw_global2) scores at least 0.9 of what they promise; the survivors come sorted by score.  `regs`: cs_extend_chains'
 * result (or the caller's regions in that form); `n_comp`: per surviving region, mem_alnreg_t.n_comp (1, more after merges; 0 for a read's only region, which the reference's function does not touch).  `chain` of a
 * merged region is that of its later part.  The result belongs to the aligner and stays valid until its next cs_dedup_regions. */
typedef struct { int32_t max_chain_gap; float mask_level_redun; } cs_dedup_params_t;   /* mem_opt_t: max_chain_gap 10000, mask_level_redun 0.95 */
void cs_dedup_params_default(cs_dedup_params_t *p);
int  cs_dedup_regions(cs_aligner_t *a, const cs_dedup_params_t *par, const cs_aln_result_t *regs, const uint8_t *bases, const uint64_t *read_offsets,
                      cs_aln_result_t *out, const int32_t **n_comp);
int  cs_aligner_stats(const cs_aligner_t *a, cs_aln_stats_t *st);
/* From regions to alignments on the GPU: what the reference does with every region it reports (mem_reg2aln, comp_seed.cpp:811-880, without
 * primary marking and MAPQ, which are cs_regions_mark's below, and SAM text, which is cs_regions_sam's) -- the band inferred from the region, the banded global alignment with
 * backtrack (bwa_gen_cigar2 / ksw_global2) up to three times with a doubled band, NM and MD, a leading or else a trailing deletion
 * squeezed out, the soft clips, and the position in contig coordinates.  Host arrays in (`regs`: cs_extend_chains' or cs_dedup_regions'
 * result, or the caller's regions in that form; `bases` / `read_offsets`: the reads); host arrays owned by the aligner out, valid until
 * its next cs_regions_cigar.  One cs_aln_t per input region, in input order: `score` the last try's global score, `w` / `tries` that
 * try's band (mem_reg2aln's w2) and number; `cigar[cigar_off, cigar_off + n_cigar)` in BAM coding (len << 4 | op; M 0, I 1, D 2, S 3);
 * `md + md_off` a NUL-terminated string.  The CIGARs lie in the order in which the pass finished them, not in region order: only the
 * offsets say where.  A purged region (qe <= qb) or an unmapped one (rb < 0 or re < 0) gives an empty result: rid = pos = -1,
 * n_cigar = 0, nm = 0, md_off at an empty string.  Scoring and w are the aligner's cs_aln_params_t.  Errors, in this order: a NULL `a`,
 * `regs` or `out`, or unknown flag bits CS_EINVAL; NULL arrays where the counts say there are entries CS_EINVAL; an aligner created with
 * device -1 CS_EDEVICE; 2^32 regions or reads or more CS_ERANGE; inconsistent input -- reg_off / read_offsets that are not CSR offset
 * arrays from 0, a read with regions of 65,536 bases or more, a live region outside its read or outside [0, 2 l_pac) or spanning more
 * than 131,072 reference bases -- CS_EINVAL, found by a checking kernel before any kernel follows an offset; regions that
 * bwa_gen_cigar2 rejects (they bridge the strands) are delivered empty with nm = -1, and the call returns CS_EINVAL after delivering the
 * others.  After any error the aligner is usable for the next call. */
#define CS_CIGAR_SMALL_SCRATCH 1u   /* tests: a backtrack-matrix budget of 64 KiB per chunk of jobs instead of 256 MiB; the same alignments */
typedef struct { int64_t pos; int32_t rid, is_rev, score, nm, n_cigar, w, tries; uint64_t cigar_off, md_off; } cs_aln_t;
typedef struct { uint64_t n_regs, n_cigar, md_bytes; const cs_aln_t *alns; const uint32_t *cigar; const char *md; } cs_cigar_result_t;
typedef struct { uint64_t regions, dp_jobs, nodp_jobs, retries, rejected, cells, launches; double kernel_ms; } cs_cigar_stats_t;
int  cs_regions_cigar(cs_aligner_t *a, const cs_aln_result_t *regs, const uint8_t *bases, const uint64_t *read_offsets, uint32_t flags, cs_cigar_result_t *out);
int  cs_cigar_stats(const cs_aligner_t *a, cs_cigar_stats_t *st);
/* Between de-duplication and the CIGAR stage, on the GPU: which regions of a read become SAM lines, with which flag and MAPQ, and which
 * ones a line lists as XA alternatives -- mem_mark_primary_se (comp_seed.cpp:711-774; the ALT branch included, is_alt from the aligner's
 * <prefix>.alt as comp_seed.cpp:2405 sets it), mem_approx_mapq_se (:686-709, for mapq_coef_len > 0), the selection loop of mem_reg2sam
 * (:1089-1106) and the membership rule of mem_gen_alt (:1026-1054).  `regs`: cs_dedup_regions' result, or the caller's regions in that
 * form -- a purged (qe <= qb) or unmapped region is refused, the reference marks after mem_sort_dedup_patch, where none exist;
 * `read_offsets`: the reads' offsets (only the lengths are used); `id_base`: the number of reads before this batch (the hash that breaks
 * ties is hash_64 of id_base + read + i, comp_seed.cpp:743, 2410).  Scoring a / b / o / e are the aligner's cs_aln_params_t.  Host arrays
 * in; host arrays owned by the aligner out, valid until its next cs_regions_mark.  `marks`: one cs_mark_t per region, per read in the
 * reference's order after its sorts (rank order), CSR by the input's reg_off; `reg` the region's index within its read in input order;
 * secondary / secondary_all / sub / sub_n / alt_sc as mem_alnreg_t has them after marking (secondary and secondary_all are ranks);
 * `line` the index of the region's SAM line within the read or -1, `flag` that line's 0x10 | 0x100 | 0x800 bits, `mapq` its MAPQ (0 for
 * a secondary), `xs` its XS (-1: none); without CS_MARK_ALL `xa_of` is the rank of the primary whose XA list the region joins, or -1.
 * `line_off`: a read's lines; a read with none gets the caller's unmapped record.  `cigar_regs` / `cigar_src`: the regions with
 * line >= 0 or xa_of >= 0 in rank order -- the input of cs_regions_cigar as it is -- and each one's index into marks.  The SAM text is
 * cs_regions_sam's, below.  Still the caller's: the -5 reordering (mem_reorder_primary5), paired-end, XR (-V), and the MAPQ formula of mapq_coef_len <= 0.  Errors, in this
 * order: a NULL `a`, `par`, `regs` or `out`, or unknown flag bits CS_EINVAL; NULL arrays where the counts say there are entries
 * CS_EINVAL; mapq_coef_len <= 0 or other bad parameters CS_EINVAL; an aligner created with device -1 CS_EDEVICE; 2^32 regions or reads
 * or more, or mapq_coef_len above 131,072, CS_ERANGE; a read with 65,536 regions or more, or a region spanning more than 131,072 bases,
 * CS_ERANGE; inconsistent input -- reg_off / read_offsets that are not CSR offset arrays from 0, a region that is purged, unmapped,
 * outside its read or outside [0, 2 l_pac), a contig index outside the contig table, a negative score -- CS_EINVAL, found by a checking
 * kernel before any kernel follows an offset.  After any error the aligner is usable for the next call. */
typedef struct { int32_t T, mapq_coef_len, max_xa_hits, max_xa_hits_alt, min_seed_len; float mask_level, drop_ratio, xa_drop_ratio; } cs_mark_params_t;
      /* mem_opt_t: T 30 (the caller scales it by -A as fastmap.c:146 does), 50, 5, 200, 19, 0.50, 0.50, 0.80; scoring a/b/o/e are the aligner's */
#define CS_MARK_ALL 1u              /* -a: secondaries become lines too; no XA lists */
#define CS_MARK_NO_MULTI 2u         /* -M: a supplementary line is flagged 0x100 instead of 0x800 */
#define CS_MARK_KEEP_SUPP_MAPQ 4u   /* -q: a supplementary line keeps its own MAPQ */
#define CS_MARK_NO_LIGHT_PATH 0x100u   /* tests: every read with regions goes through the wave kernel; the same result */
#define CS_MARK_FROM_HBM 0x200u        /* tests: the wave kernel keeps every read's lists in HBM scratch instead of LDS; the same result */
typedef struct { int32_t reg /* index within its read, input order */, is_alt, secondary, secondary_all, sub, sub_n, alt_sc, mapq, xs, flag, line, xa_of; } cs_mark_t;
typedef struct { int64_t n_reads; uint64_t n_regs, n_lines;
                 const cs_mark_t *marks;        /* per read in the reference's order after its sorts, CSR by the input's reg_off */
                 const uint64_t *line_off;      /* n_reads + 1: a read's lines; a read with none gets the caller's unmapped record */
                 cs_aln_result_t cigar_regs;    /* the regions with line >= 0 or xa_of >= 0, rank order, CSR per read: the CIGAR stage's input as it is */
                 const uint32_t *cigar_src; }   /* per entry of cigar_regs: its index into marks */ cs_mark_result_t;
typedef struct { uint64_t reads, regions, lines, xa_members, cigar_regions, light_reads, wave_reads, hbm_reads, launches; double kernel_ms; } cs_mark_stats_t;
void cs_mark_params_default(cs_mark_params_t *p);
int  cs_regions_mark(cs_aligner_t *a, const cs_mark_params_t *par, const cs_aln_result_t *regs, const uint64_t *read_offsets, int64_t id_base, uint32_t flags, cs_mark_result_t *out);
int  cs_mark_stats(const cs_aligner_t *a, cs_mark_stats_t *st);
/* Behind marking and the CIGAR stage, on the GPU: the SAM text itself -- mem_aln2sam (comp_seed.cpp:904-1024), the string part of
 * mem_gen_alt (:1056-1067) and the unmapped record of mem_reg2sam (:1107-1117), single-end as the reference runs them.  `marks`:
 * cs_regions_mark's result; `reg_off`: the reg_off that call was given (the marks' CSR); `alns`: cs_regions_cigar's result over
 * marks->cigar_regs, one entry per entry of cigar_regs; `bases` / `read_offsets`: the reads (ASCII or codes); `quals`: their qualities at the
 * same offsets, or NULL ('*'); `names` / `name_off` and `comments` / `comment_off` (-C; both NULL: none): CSR byte arrays of n_reads + 1
 * offsets.  Host arrays in; host arrays owned by the aligner out, valid until its next cs_regions_sam: text[text_off[r], text_off[r + 1])
 * holds the record or records of read r, each ending in '\n', in the reference's order, so that the text as a whole is the body of the
 * reference's output.  Contig names are the aligner's <prefix>.ann's.  -a / -M / -q are in the marks already; -Y is CS_SAM_SOFTCLIP.  What
 * is reproduced: FLAG is the mark's (plus 0x4 on the unmapped record); a clip is written H on a line that is not the read's first unless
 * -Y is given or the region is ALT, and SEQ / QUAL are cut there (the leading clip cuts the read's end on the reverse strand); a real
 * secondary (secondary >= 0; NOT a -M supplementary, which only prints 0x100) gets "*\t*" and neither SA nor pa; NM and MD, AS, XS when
 * xs >= 0, RG; SA:Z over the read's other lines that are not real secondaries (the CIGAR as cs_regions_cigar gave it, the capped MAPQ);
 * pa:f:%.3f with glibc's digits; XA:Z over the regions whose xa_of names the line's rank; the comment; a read without lines gets the
 * unmapped record.  A region whose xa_of names a rank without a line is listed nowhere, as in the reference.  Still the caller's: the -5
 * reordering (mem_reorder_primary5), paired-end, XR (-V), and the MAPQ formula of mapq_coef_len <= 0.  Errors, in this order: a NULL `a`,
 * `par`, `marks`, `alns` or `out`, or unknown flag bits CS_EINVAL; NULL arrays where the counts say there are entries CS_EINVAL;
 * alns->n_regs != marks->cigar_regs.n_regs CS_EINVAL; one of comments / comment_off without the other CS_EINVAL; an aligner created with
 * device -1 CS_EDEVICE; 2^32 reads, regions or lines or more CS_ERANGE; inconsistent input -- offsets that are not CSR arrays from 0 to
 * their counts, a read of 65,536 bases or more, lines that are not numbered 0, 1, 2 ... in rank order, an xa_of outside the read,
 * cigar_src that does not name exactly the marks with a line or an XA membership, an alignment without contig, position or CIGAR, with a
 * CIGAR or MD outside the arrays, op codes above 4 or clips longer than the read -- CS_EINVAL, found by a checking kernel before any
 * kernel follows an offset.  After any error the aligner is usable for the next call.
 * cs_sam_header: the @SQ lines (AH:* on ALT contigs) and, where `rg_line` is given as -R takes it ("@RG\tID:x", the tab written as a
 * backslash and a t, unescaped as bwa_set_rg does), that line; host only, legal on an aligner of device -1.  Writes at most `cap` bytes to
 * `buf` (no NUL) and the full length to `*need`; CS_ERANGE when cap is too small (buf may be NULL with cap 0 to ask for the length). */
typedef struct { uint32_t flags; const char *rg_id; /* the ID of -R's line (bwa_rg_id); NULL or "": no RG tag */ } cs_sam_params_t;
#define CS_SAM_SOFTCLIP 1u       /* -Y: clips stay S on every line */
#define CS_SAM_WAVE_ONLY 0x100u  /* accepted, changes nothing: the lane-per-read path it switched off lost its measurement and is gone; every record is a wave's */
typedef struct { int64_t n_reads; uint64_t n_lines, n_bytes; const uint64_t *text_off /* n_reads + 1 */; const char *text; } cs_sam_result_t;
typedef struct { uint64_t reads, lines, unmapped, bytes, xa_entries, sa_entries, launches; double kernel_ms; } cs_sam_stats_t;
int  cs_regions_sam(cs_aligner_t *a, const cs_sam_params_t *par, const cs_mark_result_t *marks, const uint64_t *reg_off, const cs_cigar_result_t *alns,
                    const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names, const uint64_t *name_off,
                    const char *comments, const uint64_t *comment_off, cs_sam_result_t *out);
int  cs_sam_header(const cs_aligner_t *a, const char *rg_line /* may be NULL */, char *buf, size_t cap, size_t *need);
int  cs_sam_stats(const cs_aligner_t *a, cs_sam_stats_t *st);

/* ---- reads to SAM text in one call: the mapper owns one engine, one device chainer and its aligners on one GPU (one per part of a batch:
 *      the extension's, a host-only one for cs_dedup_regions and the tail stages' -- the packed reference once more on host and device, not
 *      the engine), the device copy of the reads, the order of the stage calls above and their errors -- seed_and_extend behind mem_process_seqs (comp_seed.cpp:2239-2420)
 *      single-end, as the reference's program runs it.  It adds no kernel: every stage is the documented call above, with its limits.
 *      cs_map_params_t is mem_opt_t as the command line fills it; cs_map_params_split is the ONE place where a field several stages
 *      read (min_seed_len, max_occ, max_chain_gap, mask_level, drop_ratio, the scoring) is copied to each of them; the seeding struct's
 *      engine-side knobs (sst_mode, disable, result_flags) stay at their defaults.  Host only.
 *      cs_mapper_create loads the index files of `prefix`.  Errors, in this order: a NULL `prefix` or `out` or device < 0 CS_EINVAL;
 *      non-zero `reserved` or unknown flag bits CS_EINVAL; pen_clip5 != pen_clip3, mapq_coef_len <= 0 or a parameter one of the stages'
 *      own checks refuses CS_EINVAL; index files missing CS_EIO; no GPU CS_EDEVICE.  On any error everything made so far is released and
 *      *out is NULL.
 *      cs_map_batch: host arrays in, with cs_regions_sam's conventions for quals, names and comments; `id_base`: the number of reads
 *      before this batch (comp_seed.cpp:2410); `out`: as from cs_regions_sam, owned by the mapper and valid until its next cs_map_batch
 *      or cs_map_submit.
 *      Per call: the reads are uploaded once into buffers the mapper owns and grows; cs_engine_seed_batch_device; cs_chain_batch_device;
 *      cs_chain_filter_device; cs_extend_chains_device with CS_ALN_DEV_COMPACT; reg_off and the live regions come to the host;
 *      cs_dedup_regions; cs_regions_mark; cs_regions_cigar over cigar_regs; cs_regions_sam (the three tail stages upload their own copy of
 *      the reads).  n_reads == 0 gives an empty result; a batch in which no read has a seed, a chain or a region gives every read its
 *      unmapped record.  Errors: NULL arguments, n_reads < 0, id_base < 0, read_offsets that do not start at 0 or decrease CS_EINVAL;
 *      otherwise a stage's error is the call's error and cs_last_error names the stage.  After any error the mapper is usable for the
 *      next call.  One thread at a time per mapper; mappers are independent.
 *      cs_mapper_header is cs_sam_header on the mapper's aligner.  cs_mapper_stats: counters over the mapper's life and the host wall
 *      time of each step of cs_map_batch, accumulated; cs_mapper_engine_stats passes cs_engine_stats through. */
#define CS_MAP_ALL             1u   /* -a */
#define CS_MAP_NO_MULTI        2u   /* -M */
#define CS_MAP_KEEP_SUPP_MAPQ  4u   /* -q */
#define CS_MAP_SOFTCLIP        8u   /* -Y */
typedef struct {
	int32_t a, b, o_del, e_del, o_ins, e_ins, pen_clip5, pen_clip3, w, zdrop;   /* -A -B -O -E -L -w -d */
	int32_t T;                                                                   /* -T, already scaled by -A */
	int32_t min_seed_len; float split_factor; int32_t split_width, max_occ; uint64_t max_mem_intv;  /* -k -r -s -c -y */
	int32_t max_chain_gap, max_chain_extend, min_chain_weight;                   /* -G -N -W */
	float   mask_level, drop_ratio, xa_drop_ratio, mask_level_redun;             /* -X -D, 0.80, 0.95 */
	int32_t mapq_coef_len, max_xa_hits, max_xa_hits_alt;                         /* -Q -h */
	uint32_t flags;          /* CS_MAP_ALL (-a) | CS_MAP_NO_MULTI (-M) | CS_MAP_KEEP_SUPP_MAPQ (-q) | CS_MAP_SOFTCLIP (-Y) */
	int32_t threads;         /* host threads of cs_dedup_regions [16] */
	const char *rg_id;       /* NULL or "": no RG tag */
	uint32_t reserved[4];    /* must be 0 */
} cs_map_params_t;
enum { CS_MAP_T_UPLOAD, CS_MAP_T_SEED, CS_MAP_T_CHAIN, CS_MAP_T_FILTER, CS_MAP_T_EXTEND, CS_MAP_T_DOWNLOAD, CS_MAP_T_DEDUP, CS_MAP_T_MARK,
       CS_MAP_T_CIGAR, CS_MAP_T_SAM, CS_MAP_T_TOTAL, CS_MAP_N_STAGES };
typedef struct { uint64_t reads, bases, regions /* after de-duplication */, lines, unmapped, bytes, batches;
                 double stage_ms[CS_MAP_N_STAGES]; } cs_map_stats_t;
typedef struct cs_mapper cs_mapper_t;
void cs_map_params_default(cs_map_params_t *p);               /* mem_opt_init, comp_seed.cpp:26-58 */
int  cs_map_params_split(const cs_map_params_t *p, cs_params_t *seed, cs_chain_params_t *chain, cs_flt_params_t *flt, cs_aln_params_t *aln,
                         cs_dedup_params_t *dedup, cs_mark_params_t *mark, uint32_t *mark_flags, cs_sam_params_t *sam);
int  cs_mapper_create(const char *prefix, int device, const cs_engine_options_t *eopt /* NULL: defaults */, const cs_map_params_t *par /* NULL: defaults */,
                      cs_mapper_t **out);
void cs_mapper_destroy(cs_mapper_t *m);
int  cs_map_batch(cs_mapper_t *m, int64_t n_reads, const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names,
                  const uint64_t *name_off, const char *comments, const uint64_t *comment_off, int64_t id_base, cs_sam_result_t *out);
/* The same as a stream of batches, up to CS_MAP_MAX_IN_FLIGHT in flight, the counterpart of cs_engine_submit / cs_engine_collect_packed one
 * level up: cs_map_submit runs cs_map_batch's argument checks (CS_EINVAL: nothing is queued and the stream is as it was), queues the batch
 * and returns at once; the caller's arrays must stay untouched until the batch is collected.  A submit with CS_MAP_MAX_IN_FLIGHT batches
 * uncollected is CS_EINVAL and queues nothing.  cs_map_collect blocks until the OLDEST submitted batch is complete and hands out its result;
 * results come back in submission order; with nothing in flight it returns CS_EINVAL.  A batch is three parts -- front (upload, seeding,
 * chaining, filter, extension, download), cs_dedup_regions, tail (marking, CIGAR, SAM text) -- and the mapper owns one worker thread per
 * part, started by the first submit: the parts of one batch run in cs_map_batch's order, each part runs one batch at a time in submission
 * order, and the three run beside each other on different batches, so that the de-duplication of batch n (host threads) runs beside the
 * front of batch n+1 and the tail of batch n-1 (both on the GPU).  The text is cs_map_batch's for the same reads, whatever travels
 * beside them.  n_reads == 0 is a legal batch and gives the empty result in its turn.
 * A collected result is owned by the mapper and stays valid until the next cs_map_collect, cs_map_batch or cs_mapper_destroy, whatever
 * is submitted or finishes meanwhile.  The mapper keeps ONE set of the SAM stage's host result arrays more than it has batches in flight
 * for this: a finished batch's text is exchanged out of the stage, and a collect exchanges it with that spare set and hands out the spare
 * set's pointers -- pointers change hands, the text (225 bytes per read) is not copied.  A batch that fails in a stage fails at ITS collect:
 * that stage's code, and cs_last_error (of the collecting thread) starts with "cs_map_collect: <stage>: ".  A collect that returns an error
 * hands nothing out and does not shorten the life of an earlier result; the batches behind it are not affected, and the mapper stays
 * usable.  While batches are in flight cs_map_batch returns CS_EINVAL; cs_mapper_destroy waits for them first.
 * cs_mapper_stats: every step adds its wall time to stage_ms[k] as in cs_map_batch, measured in the thread that ran it; CS_MAP_T_TOTAL of a
 * streamed batch is its time from submit to completion, so that with batches in flight the steps no longer sum to the total; the
 * counters and times of a batch are added when it is collected.  cs_mapper_in_flight: batches submitted and not yet collected, and how
 * many of those are complete (finished <= submitted <= CS_MAP_MAX_IN_FLIGHT); host only, never blocks.
 * Threads: one submitting thread, one collecting thread, which may be the same; cs_mapper_in_flight from either. */
#define CS_MAP_MAX_IN_FLIGHT 3
int  cs_map_submit(cs_mapper_t *m, int64_t n_reads, const uint8_t *bases, const uint64_t *read_offsets, const uint8_t *quals, const char *names,
                   const uint64_t *name_off, const char *comments, const uint64_t *comment_off, int64_t id_base);
int  cs_map_collect(cs_mapper_t *m, cs_sam_result_t *out);
int  cs_mapper_in_flight(const cs_mapper_t *m, int *submitted, int *finished);
int  cs_mapper_header(const cs_mapper_t *m, const char *rg_line /* may be NULL */, char *buf, size_t cap, size_t *need);
int  cs_mapper_stats(const cs_mapper_t *m, cs_map_stats_t *st);
int  cs_mapper_engine_stats(const cs_mapper_t *m, cs_stats_t *st);

/* ---- the result of the LAST device-variant call, without moving it: an order-sensitive 64-bit digest per array
 *      (sum over the array's 64-bit words w[i] of splitmix64(w[i] + i * 0x9E3779B97F4A7C15), mod 2^64), so that two runs over
 *      10 M reads can be compared word for word without downloading 6 GB; and the CSR slice of selected reads (any order,
 *      repeats allowed) gathered on the device into the engine's pinned host buffers (what cs_engine_seed_batch would
 *      have returned for exactly those reads -- results do not depend on the batch a read travels in). */
typedef struct { uint64_t mem_off, mems, seed_off, seeds; } cs_digest_t;
int  cs_engine_result_digest(cs_engine_t *e, cs_digest_t *out);
int  cs_engine_gather_reads(cs_engine_t *e, int64_t n_sel, const uint64_t *read_ids, cs_result_t *out);

/* ---- byte model of the SMEM stage as THIS implementation runs it (bench.py's roofline): every access the kernels make to an
 *      index-side array is counted on the device as an event of its kernel; bytes = events x event_bytes.  These are the bytes
 *      the kernels ask for -- a lower bound of what has to come out of HBM/L2 for them -- not the bytes of the reference's
 *      algorithm (most of whose bwt_extend calls are answered without the FM index here).  Accumulated like cs_stats_t. */
#define CS_N_KERNELS 9   /* fwd0, fwd, bwd_win, bwd_win0, bwd_wide, bwd_all, r2text, r3text, fused (smem_kernel) */
#define CS_N_EVENTS 10   /* Occ record 32 B, jump entry 16 B, filter word 8 B, SA entry, inverse-SA entry (4 or 8 B; 5 under sa40), text word 4 B,
                            rep[] load 8 B, lcp[] byte, LEP entry 16 B (read or written), mem record read back 32 B */
typedef struct {
	uint64_t events[CS_N_KERNELS][CS_N_EVENTS];
	uint64_t event_bytes[CS_N_EVENTS];
	uint64_t stream_bytes;   /* modelled on the host per call: read bases read once, their packed records written and read by
	                            each kernel family, task queue words, backward task records, raw mems written, sorted and
	                            written again */
} cs_traffic_t;
int  cs_engine_traffic_model(cs_engine_t *e, cs_traffic_t *out);

/* ---- validation of the resident index at the size it is used (the byte-for-byte comparisons with bwaidx's files stop at 64 Mbp): counts
 *      violations of (1) recovered text == `d_fwd_nt4` (device memory, codes 0..3, l_pac bases; NULL skips this) and its reverse complement,
 *      (2) suffix order of every neighbouring pair of rows of the full suffix array, decided on the text, (3) ISA[SA[r]] == r, (4) BWT character
 *      of row r == T[SA[r] - 1] and the row of suffix 0 == primary, (5) sampled SA == full SA at the sampled rows (bwt_cal_sa, bwt.c:62-96).
 *      All zero <=> the .bwt / .sa pair is the FM index of that text.  undecided_rows: pairs that share more than 2^20 bases. */
typedef struct {
	uint64_t rows_checked, order_violations, isa_violations, bwt_violations, sampled_sa_violations, undecided_rows, text_violations;
	int32_t  text_checked, reserved;
} cs_index_check_t;
int  cs_engine_check_index(cs_engine_t *e, const uint8_t *d_fwd_nt4, uint64_t l_pac, cs_index_check_t *out);

int  cs_engine_stats(const cs_engine_t *e, cs_stats_t *st);
void cs_engine_reset_stats(cs_engine_t *e);

/* ---- what the engine holds in device memory, in bytes, by group: the sizes its buffers were reserved with (padding included), not
 *      differences of free memory.  The index-side arrays are fixed once the engine exists (an array that did not fit, or was switched
 *      off, reports 0); kmer_filter changes when a call with another min_seed_len rebuilds the filter; pass_ctx[i] is the working set of
 *      pass context i (streams' buffers: reads, queues, LEP arena, raw mems, results) as of the end of its last pass -- it grows with the
 *      largest batch seen -- and 0 for a context that does not exist (the second one is made on first use); pass_ctx[0] also holds the
 *      spare result set of cs_engine_collect_device (as of the last collect: a collect only moves arrays between it and a context, so
 *      the sum does not change).  total is the sum of the
 *      groups.  Not counted: the staging buffers of the host variants and of cs_engine_gather_reads, which are a few bytes per read of a
 *      sub-batch.  sa_entry_bits: the entry width of the full suffix array / inverse suffix array, 32, 40 or 64; 0 without a full suffix
 *      array.  Host-only: no device call is made, and it is legal while submitted batches are in flight. */
typedef struct {
	uint64_t occ_bwt;        /* Occ/BWT records                          */
	uint64_t sampled_sa;
	uint64_t full_sa;
	uint64_t isa;            /* inverse suffix array                     */
	uint64_t text;           /* 2-bit text                               */
	uint64_t lcp_rep;        /* lcp[] + rep[]                            */
	uint64_t jump_table;
	uint64_t kmer_filter;
	uint64_t pass_ctx[2];
	uint64_t total;
	int32_t  sa_entry_bits;
	int32_t  n_pass_ctx;     /* pass contexts allocated: 1 or 2          */
} cs_memory_t;
int  cs_engine_memory(const cs_engine_t *e, cs_memory_t *out);

/* ---- batched primitives on the device index, for parity tests of the building blocks (host pointers):
 *      bwt_occ4 (bwt.c:169), bwt_extend (bwt.c:262; ok is n x 4 intervals, info untouched = 0), bwt_sa (bwt.c:86) */
int  cs_engine_occ4(cs_engine_t *e, int64_t n, const uint64_t *k, uint64_t *cnt4);
int  cs_engine_extend(cs_engine_t *e, int64_t n, const cs_intv_t *ik, const uint8_t *is_back, cs_intv_t *ok4);
int  cs_engine_sa(cs_engine_t *e, int64_t n, const uint64_t *k, uint64_t *sa);

/* ---- diagnostic: ceiling of the path's access shape on the resident index -- every lane of `waves_per_simd` x 4 waves
 *      per CU follows a dependent chain of `steps` random 64-byte Occ-block reads; returns 64-byte lines per second */
int  cs_engine_probe_random_lines(cs_engine_t *e, int waves_per_simd, int steps, double *lines_per_sec);

/* ---- device memory helpers so that a caller without its own HIP code can stage inputs for the device variant */
int  cs_device_alloc(cs_engine_t *e, size_t bytes, void **dptr);
int  cs_device_free(cs_engine_t *e, void *dptr);
int  cs_device_upload(cs_engine_t *e, void *dst, const void *src, size_t bytes);
int  cs_device_download(cs_engine_t *e, void *dst, const void *src, size_t bytes);
int  cs_device_sync(cs_engine_t *e);

#ifdef __cplusplus
}
#endif
#endif /* COMPSEED_AMD_H */
