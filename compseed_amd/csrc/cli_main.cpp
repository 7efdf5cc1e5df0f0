// cli_main.cpp -- `compseed_amd_cli`: the CompSeed command line on MI355X, in two modes.
//
//   compseed_amd_cli [options] <FM-index prefix> <reordered reads>                 the seeding mode
//   compseed_amd_cli --sam FILE [options] <FM-index prefix> <reordered reads>      reads to SAM (FILE '-': standard output)
//
// Same positional arguments as `CompSeed` / `bwamem` (main.cpp:146-200, 233-330).  Input: one read per line (input_reorder_reads,
// main.cpp:36-58) or FASTQ when the first byte is '@' (main.cpp:399-406).  Chunking follows main.cpp:54,437: a chunk ends at the first even
// read count that reaches -K bases (default 10,000,000 x n_threads).  Chunks are split into contiguous read ranges, one per GPU
// (--gpus N, default all; --devices LIST).
// The seeding mode (no --sam) is what the program was before the library could write SAM, and it stays as it was for the command lines
// that use it: the seeding flags -t -k -r -y -c -s -K are honoured, the flags of the other stages are accepted and ignored, the seeds
// are written (--dump-seeds FILE) and the reference's exit counters printed (display_profile, main.cpp:203-214).
// With --sam the flags are parsed as main.cpp:233-330 parses them and update_a (main.cpp:130-143) is applied; one cs_mapper_t per GPU
// takes each chunk's shard as a submitted batch, up to CS_MAP_MAX_IN_FLIGHT chunks in flight while the next is read, and FILE receives the header (bwa_print_sam_hdr, with -R's line) and every chunk's
// text in read order: the file the reference's program writes.  Honoured: -k -r -y -c -s -K -t, -w -d -D -W -N -G -X -T -A -B,
// -O / -E / -L / -h a[,b], -Q -a -M -q -Y -C -R -v; -o / -f / -1 are accepted and ignored (as in the seeding mode: making -o an alias of
// --sam would change what existing command lines do).  Refused with exit status 1 before the GPU is touched, because the library's stages
// do not have them: -5 (mem_reorder_primary5), -V (XR), -Q <= 0 (the other MAPQ formula), -L a,b with a != b (one extender, one end
// bonus), -x presets, -H, -j, the paired-end options -p -I -S -P -U -m and a second reads file (the reference's own program refuses
// that one, main.cpp:331-335), and --dump-seeds / --no-sal together with --sam.  --show-params prints the resolved cs_map_params_t as
// key=value lines and exits without touching the index or the GPU.
#include "../../include/compseed_amd.h"

#include <cctype>
#include <chrono>
#include <cstdio>
#include <deque>
#include <functional>
#include <thread>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

// a chunk as the reader delivers it, and its per-GPU read ranges with offsets rebased to 0 (they must live until the chunk is collected)
struct Chunk { const uint8_t *bases = nullptr; const uint64_t *off = nullptr; int64_t n = 0; uint64_t first_id = 0; std::vector<std::vector<uint64_t>> loff; };

static void usage()
{
	fprintf(stderr,
	        "Usage: compseed_amd_cli [options] <FM-index> <Reordered Reads>\n\n"
	        "Seeding options (same meaning as CompSeed / bwamem):\n"
	        "       -t INT        host threads of the reference; sets the default chunk size (-K) [1]\n"
	        "       -k INT        minimum seed length [19]\n"
	        "       -r FLOAT      look for internal seeds inside a seed longer than {-k} * FLOAT [1.5]\n"
	        "       -y INT        seed occurrence for the 3rd round seeding [20]\n"
	        "       -c INT        skip seeds with more than INT occurrences [500]\n"
	        "       -s INT        re-seed only SMEMs with at most INT occurrences [10]\n"
	        "       -K INT        process INT input bases in each batch [10000000 x -t]\n"
	        "GPU / output options:\n"
	        "       --gpus INT    number of MI355X to shard each batch over [all visible]\n"
	        "       --devices LIST   comma-separated device ordinal of every shard instead (an ordinal may repeat)\n"
	        "       --no-sal      stop after SMEM collection (no suffix-array lookup)\n"
	        "       --dump-seeds FILE   write `M read beg end x0 x1 x2` and `S read qbeg len rbeg` lines\n"
	        "Other CompSeed flags (-w -d -D -W -m -S -P -A -B -O -E -L -U -x -p -R -H -o -j -5 -q -v -T -h -a -C -V -Y -M -I)\n"
	        "belong to stages behind seeding; they are accepted and ignored.\n");
}

// the seeding mode: everything the program did before it wrote SAM, unchanged
static int seed_main(int argc, char **argv)
{
	cs_params_t par; cs_params_default(&par);
	int n_threads = 1, n_gpus = -1, verbose = 0; long fixed_chunk = 0; const char *dump = nullptr;
	std::vector<int> devices; // --devices: the device ordinal of every shard (an ordinal may repeat: several engines on one GPU)
	std::vector<const char *> pos;
	for (int i = 1; i < argc; ++i) {
		std::string a = argv[i];
		auto need = [&]() -> const char * { if (i + 1 >= argc) { usage(); exit(1); } return argv[++i]; };
		if (a == "-k") par.min_seed_len = atoi(need());
		else if (a == "-r") par.split_factor = (float)atof(need());
		else if (a == "-y") par.max_mem_intv = (uint64_t)atol(need());
		else if (a == "-c") par.max_occ = atoi(need());
		else if (a == "-s") par.split_width = atoi(need());
		else if (a == "-t") { n_threads = atoi(need()); if (n_threads < 1) n_threads = 1; }
		else if (a == "-K") fixed_chunk = atol(need());
		else if (a == "--gpus") n_gpus = atoi(need());
		else if (a == "--devices") { for (const char *q = need(); *q;) { devices.push_back((int)strtol(q, (char **)&q, 10)); if (*q == ',') ++q; else if (*q) { usage(); return 1; } } }
		else if (a == "--no-sal") par.want_sal = 0;
		else if (a == "-v") verbose = atoi(need()) >= 4 ? 1 : 0; // bwa's verbosity levels: 4 = debugging output
		else if (a == "--dump-seeds") dump = need();
		else if (a.size() == 2 && a[0] == '-' && strchr("wdDWmABOELUxRHoThI", a[1])) (void)need(); // flags with a value, other stages
		else if (a.size() == 2 && a[0] == '-' && strchr("SPpj5qaCVYM1", a[1])) {}                    // switches, other stages
		else if (a[0] == '-' && a.size() > 1) { fprintf(stderr, "[E::main] unknown option %s\n", a.c_str()); usage(); return 1; }
		else pos.push_back(argv[i]);
	}
	if (pos.size() < 2) { usage(); return 1; }
	if (par.min_seed_len < 1) { fprintf(stderr, "[E::main] -k must be positive\n"); return 1; }

	cs_index_t *idx = nullptr;
	if (cs_index_load(pos[0], &idx)) { fprintf(stderr, "[E::main] fail to locate the index files: %s\n", cs_last_error()); return 1; }
	cs_index_view_t view; cs_index_view(idx, &view);
	int ndev = 0;
	if (cs_device_count(&ndev) || ndev < 1) { fprintf(stderr, "[E::main] no MI355X visible: %s\n", cs_last_error()); return 1; }
	if (!devices.empty()) n_gpus = (int)devices.size();
	else { if (n_gpus < 1 || n_gpus > ndev) n_gpus = ndev; for (int g = 0; g < n_gpus; ++g) devices.push_back(g); }
	for (int d : devices) if (d < 0 || d >= ndev) { fprintf(stderr, "[E::main] --devices: no device %d (%d visible)\n", d, ndev); return 1; }
	std::vector<cs_engine_t *> eng((size_t)n_gpus, nullptr);
	cs_engine_options_t eopt; cs_engine_options_default(&eopt);
	eopt.count_sal_merged = 1; // "SA Lookup: ... calls, % merged" as CompSeed prints it (main.cpp:209-210)
	eopt.verbose = verbose;
	for (int g = 0; g < n_gpus; ++g)
		if (cs_engine_create_opts(&view, devices[(size_t)g], &eopt, &eng[g])) { fprintf(stderr, "[E::main] GPU %d: %s\n", g, cs_last_error()); return 1; }

	FILE *fo = dump ? fopen(dump, "w") : nullptr;
	if (dump && !fo) { fprintf(stderr, "[E::main] cannot write %s\n", dump); return 1; }
	long chunk_bases = fixed_chunk > 0 ? fixed_chunk : 10000000L * n_threads; // main.cpp:437
	cs_reader_t *rd = nullptr;
	if (cs_reader_open(pos[1], chunk_bases, &rd)) { fprintf(stderr, "[E::main] %s\n", cs_last_error()); return 1; }

	// The reference's three-step pipeline (main.cpp:438) with the GPUs in the middle: chunk n+1 is read and submitted while chunk n
	// is being seeded; every GPU gets a contiguous read range of each chunk (neighbouring, overlapping reads stay together).
	auto read_chunk = [&](Chunk &c, uint64_t first_id) -> bool {
		if (cs_reader_next(rd, &c.bases, &c.off, &c.n)) { fprintf(stderr, "[E::process] %s\n", cs_last_error()); exit(1); }
		c.first_id = first_id;
		return c.n > 0;
	};
	auto submit = [&](Chunk &c) {
		c.loff.assign((size_t)n_gpus, std::vector<uint64_t>());
		for (int g = 0; g < n_gpus; ++g) {
			const int64_t r0 = c.n * g / n_gpus, r1 = c.n * (g + 1) / n_gpus;
			c.loff[g].resize((size_t)(r1 - r0) + 1);
			for (int64_t r = r0; r <= r1; ++r) c.loff[g][(size_t)(r - r0)] = c.off[r] - c.off[r0];
			if (cs_engine_submit(eng[g], &par, r1 - r0, c.bases + c.off[r0], c.loff[g].data())) { fprintf(stderr, "[E::main] GPU %d: %s\n", g, cs_last_error()); exit(1); }
		}
	};
	auto collect = [&](Chunk &c) {
		for (int g = 0; g < n_gpus; ++g) {
			cs_packed_result_t R;
			if (cs_engine_collect_packed(eng[g], &R)) { fprintf(stderr, "[E::main] GPU %d: %s\n", g, cs_last_error()); exit(1); }
			if (!fo) continue;
			const int64_t r0 = c.n * g / n_gpus;
			for (int64_t r = 0; r < R.n_reads; ++r) {
				const uint64_t id = c.first_id + (uint64_t)(r0 + r) + 1; // read names are running integers from 1 (main.cpp:47)
				uint64_t sd = R.seed_off ? R.seed_off[r] : 0;
				for (uint64_t m = R.mem_off[r]; m < R.mem_off[r + 1]; ++m) {
					cs_intv_t v; cs_unpack_mem(&R, m, &v);
					fprintf(fo, "M\t%lu\t%u\t%u\t%lu\t%lu\t%lu\n", (unsigned long)id, (unsigned)(v.info >> 32), (unsigned)v.info, (unsigned long)v.x0, (unsigned long)v.x1, (unsigned long)v.x2);
				}
				if (R.seed_off)
					for (uint64_t m = R.mem_off[r]; m < R.mem_off[r + 1]; ++m) {
						cs_intv_t v; cs_unpack_mem(&R, m, &v);
						const uint32_t cnt = cs_mem_seed_count(&v, R.max_occ);
						for (uint32_t k = 0; k < cnt; ++k)
							fprintf(fo, "S\t%lu\t%d\t%d\t%ld\n", (unsigned long)id, (int)(v.info >> 32), (int)((uint32_t)v.info - (uint32_t)(v.info >> 32)), (long)cs_packed_seed_rbeg(&R, sd + k));
						sd += cnt;
					}
			}
		}
	};
	Chunk ch[2];
	uint64_t n_processed = 0;
	int cur = 0;
	if (read_chunk(ch[0], 0)) {
		submit(ch[0]);
		for (;;) {
			Chunk &c = ch[cur], &nx = ch[cur ^ 1];
			const bool more = read_chunk(nx, n_processed + (uint64_t)c.n);
			if (more) submit(nx);
			collect(c);
			n_processed += (uint64_t)c.n;
			if (!more) break;
			cur ^= 1;
		}
	}
	cs_reader_close(rd);
	if (fo) fclose(fo);

	cs_stats_t tot; memset(&tot, 0, sizeof tot);
	for (int g = 0; g < n_gpus; ++g) {
		cs_stats_t st; cs_engine_stats(eng[g], &st);
		tot.reads += st.reads; tot.bwt_queries += st.bwt_queries; tot.bwt_calls += st.bwt_calls; tot.sal_queries += st.sal_queries;
		tot.sal_calls += st.sal_calls; tot.mems += st.mems; tot.seeds += st.seeds;
		tot.seed_kernel_ms = st.seed_kernel_ms > tot.seed_kernel_ms ? st.seed_kernel_ms : tot.seed_kernel_ms;
		tot.sal_kernel_ms = st.sal_kernel_ms > tot.sal_kernel_ms ? st.sal_kernel_ms : tot.sal_kernel_ms;
		tot.total_ms = st.total_ms > tot.total_ms ? st.total_ms : tot.total_ms;
		cs_engine_destroy(eng[g]);
	}
	cs_index_free(idx);
	// display_profile, main.cpp:203-214
	fprintf(stderr, "BWT-extend:  %lu queries, %lu calls, %.2f %% hit in SST\n", (unsigned long)tot.bwt_queries, (unsigned long)tot.bwt_calls,
	        tot.bwt_queries ? 100.0 * (double)(tot.bwt_queries - tot.bwt_calls) / (double)tot.bwt_queries : 0.0);
	fprintf(stderr, "SA Lookup:   %lu queries, %lu calls, %.2f %% merged\n", (unsigned long)tot.sal_queries, (unsigned long)tot.sal_calls,
	        tot.sal_queries ? 100.0 * (double)(tot.sal_queries - tot.sal_calls) / (double)tot.sal_queries : 0.0);
	fprintf(stderr, "Wall time:   BWT %.2f SAL %.2f seconds on %d GPU(s); %lu reads, %lu mems, %lu seeds\n", tot.seed_kernel_ms / 1e3,
	        tot.sal_kernel_ms / 1e3, n_gpus, (unsigned long)tot.reads, (unsigned long)tot.mems, (unsigned long)tot.seeds);
	return 0;
}

// ---------------------------------------------------------------------------------------------------------------- --sam: reads to SAM
static void usage_sam()
{
	fprintf(stderr,
	        "Usage: compseed_amd_cli --sam FILE [options] <FM-index> <Reordered Reads | FASTQ>      (FILE '-': standard output)\n\n"
	        "Options with the meaning they have in CompSeed / bwamem:\n"
	        "       seeding      -k INT  -r FLOAT  -y INT  -c INT  -s INT\n"
	        "       chaining     -w INT  -G INT  -N INT  -W INT  -D FLOAT  -X FLOAT\n"
	        "       extension    -A INT  -B INT  -O INT[,INT]  -E INT[,INT]  -L INT  -d INT\n"
	        "       output       -T INT  -h INT[,INT]  -Q INT  -a  -M  -q  -Y  -C  -R STR  -v INT\n"
	        "       input        -t INT  -K INT          (-o / -f / -1 are accepted and ignored)\n"
	        "       --gpus INT | --devices LIST   one mapper per entry; a chunk's reads are split into contiguous ranges\n"
	        "       --show-params                 print the resolved parameters as key=value lines and exit\n"
	        "Refused: -5, -V, -Q <= 0, -L with two different values, -p -x -H -I -j -S -P -U -m, a second reads file (paired-end),\n"
	        "         --dump-seeds and --no-sal together with --sam.\n");
}

namespace {
struct SamOpts {
	cs_map_params_t p; bool given_b = false, given_T = false, given_o_del = false, given_e_del = false, given_o_ins = false, given_e_ins = false, given_zdrop = false,
	                        given_clip5 = false, given_clip3 = false, given_a = false;   // opt0 of main.cpp:232-330
	int n_threads = 1, n_gpus = -1, verbose = 0; long fixed_chunk = 0; bool copy_comment = false, show = false;
	const char *sam = nullptr; std::string rg_line, rg_id; std::vector<int> devices; std::vector<const char *> pos;
};
int refuse(const char *opt, const char *why) { fprintf(stderr, "[E::main] %s: %s\n", opt, why); return 1; }
// "INT[,INT]" as main.cpp:268-292 reads it: the second value behind one punctuation character
void two_ints(const char *v, int32_t *x, int32_t *y)
{
	char *q = nullptr;
	*x = *y = (int32_t)strtol(v, &q, 10);
	if (*q != 0 && ispunct((unsigned char)*q) && isdigit((unsigned char)q[1])) *y = (int32_t)strtol(q + 1, &q, 10);
}
// -R's line: "@RG" first, tabs written as a backslash and a t, an ID field (bwa_set_rg / bwa_rg_id, bwalib/bwa.c:429-476); the ID into `id`
bool rg_id_of(const std::string &line, std::string &id)
{
	if (line.compare(0, 3, "@RG") != 0 || line.find('\t') != std::string::npos) return false;
	std::string u;
	for (size_t k = 0; k < line.size(); ++k) {
		if (line[k] != '\\') { u += line[k]; continue; }
		if (++k == line.size()) break;
		u += line[k] == 't' ? '\t' : line[k] == 'n' ? '\n' : line[k] == 'r' ? '\r' : line[k] == '\\' ? '\\' : '\0';
		if (u.back() == '\0') u.pop_back();
	}
	const size_t at = u.find("\tID:");
	if (at == std::string::npos) return false;
	size_t e = at + 4;
	while (e < u.size() && u[e] != '\t' && u[e] != '\n') ++e;
	id = u.substr(at + 4, e - at - 4);
	return !id.empty() && id.size() <= 255;
}

// the command line as main.cpp:233-335 reads it (getopt: clustered switches, a value attached or in the next argument); 0, or the exit status
int parse_sam(int argc, char **argv, SamOpts &o)
{
	cs_map_params_default(&o.p);
	cs_map_params_t &p = o.p;
	const std::string switches = "51qpaMCSPVYj", valued = "kcvsrtRABOEUwLdTQDmINofWxGhyKXH";
	bool dump = false, no_sal = false;
	for (int i = 1; i < argc; ++i) {
		const std::string a = argv[i];
		auto next = [&](const char *opt) -> const char * { if (i + 1 >= argc) { fprintf(stderr, "[E::main] option %s needs a value\n", opt); usage_sam(); exit(1); } return argv[++i]; };
		if (a == "--sam") { o.sam = next("--sam"); continue; }
		if (a == "--show-params") { o.show = true; continue; }
		if (a == "--gpus") { o.n_gpus = atoi(next("--gpus")); continue; }
		if (a == "--devices") { for (const char *q = next("--devices"); *q;) { o.devices.push_back((int)strtol(q, (char **)&q, 10)); if (*q == ',') ++q; else if (*q) { usage_sam(); return 1; } } continue; }
		if (a == "--dump-seeds") { (void)next("--dump-seeds"); dump = true; continue; }
		if (a == "--no-sal") { no_sal = true; continue; }
		if (a.size() < 2 || a[0] != '-' || a == "-") { o.pos.push_back(argv[i]); continue; }
		if (a[1] == '-') { fprintf(stderr, "[E::main] unknown option %s\n", a.c_str()); usage_sam(); return 1; }
		for (size_t j = 1; j < a.size(); ++j) {
			const char c = a[j];
			const std::string name = std::string("-") + c;
			if (switches.find(c) != std::string::npos) {
				if (c == 'a') p.flags |= CS_MAP_ALL;
				else if (c == 'M') p.flags |= CS_MAP_NO_MULTI;
				else if (c == 'q') p.flags |= CS_MAP_KEEP_SUPP_MAPQ;
				else if (c == 'Y') p.flags |= CS_MAP_SOFTCLIP;
				else if (c == 'C') o.copy_comment = true;
				else if (c == '1') {}                                          // (no_mt_io: this program's reader has one thread anyway)
				else if (c == '5') return refuse("-5", "the reordering of split alignments (mem_reorder_primary5) is not implemented");
				else if (c == 'V') return refuse("-V", "the XR tag is not implemented");
				else if (c == 'j') return refuse("-j", "ignoring the .alt file is not implemented");
				else return refuse(name.c_str(), "paired-end options are not implemented (the reference's program refuses a second reads file too)");   // -p -S -P
				continue;
			}
			if (valued.find(c) == std::string::npos) { fprintf(stderr, "[E::main] unknown option %s\n", name.c_str()); usage_sam(); return 1; }
			const std::string own = a.substr(j + 1);
			const char *v = own.empty() ? next(name.c_str()) : own.c_str();
			if (c == 'k') p.min_seed_len = atoi(v);
			else if (c == 'r') p.split_factor = (float)atof(v);
			else if (c == 'y') p.max_mem_intv = (uint64_t)atol(v);
			else if (c == 'c') p.max_occ = atoi(v);
			else if (c == 's') p.split_width = atoi(v);
			else if (c == 't') { o.n_threads = atoi(v); if (o.n_threads < 1) o.n_threads = 1; }
			else if (c == 'K') o.fixed_chunk = atol(v);
			else if (c == 'v') o.verbose = atoi(v) >= 4 ? 1 : 0;
			else if (c == 'w') p.w = atoi(v);
			else if (c == 'd') { p.zdrop = atoi(v); o.given_zdrop = true; }
			else if (c == 'D') p.drop_ratio = (float)atof(v);
			else if (c == 'W') p.min_chain_weight = atoi(v);
			else if (c == 'N') p.max_chain_extend = atoi(v);
			else if (c == 'G') p.max_chain_gap = atoi(v);
			else if (c == 'X') p.mask_level = (float)atof(v);
			else if (c == 'T') { p.T = atoi(v); o.given_T = true; }
			else if (c == 'A') { p.a = atoi(v); o.given_a = true; }
			else if (c == 'B') { p.b = atoi(v); o.given_b = true; }
			else if (c == 'O') { two_ints(v, &p.o_del, &p.o_ins); o.given_o_del = o.given_o_ins = true; }
			else if (c == 'E') { two_ints(v, &p.e_del, &p.e_ins); o.given_e_del = o.given_e_ins = true; }
			else if (c == 'L') { two_ints(v, &p.pen_clip5, &p.pen_clip3); o.given_clip5 = o.given_clip3 = true; if (p.pen_clip5 != p.pen_clip3) return refuse("-L", "two different clipping penalties are not implemented (one extender, one end bonus)"); }
			else if (c == 'h') two_ints(v, &p.max_xa_hits, &p.max_xa_hits_alt);
			else if (c == 'Q') { p.mapq_coef_len = atoi(v); if (p.mapq_coef_len <= 0) return refuse("-Q", "the MAPQ formula of a value <= 0 is not implemented"); }
			else if (c == 'R') { o.rg_line = v; if (!rg_id_of(o.rg_line, o.rg_id)) return refuse("-R", "the read group line starts with @RG, writes its tabs as \\t and has an ID of at most 255 characters"); }
			else if (c == 'o' || c == 'f') {}                                  // accepted and ignored in both modes: the output is --sam's
			else if (c == 'x') return refuse("-x", "read-type presets are not implemented");
			else if (c == 'H') return refuse("-H", "extra header lines are not implemented");
			else return refuse(name.c_str(), "paired-end options are not implemented (the reference's program refuses a second reads file too)");       // -I -U -m
			break;
		}
	}
	if (o.sam && dump) return refuse("--dump-seeds", "not together with --sam");
	if (o.sam && no_sal) return refuse("--no-sal", "not together with --sam");
	if (o.pos.size() >= 3) return refuse(o.pos[2], "a second reads file: paired-end is not implemented (the reference's program refuses it too)");
	if (o.given_a) {   // update_a, main.cpp:130-143
		if (!o.given_b) p.b *= p.a;
		if (!o.given_T) p.T *= p.a;
		if (!o.given_o_del) p.o_del *= p.a;
		if (!o.given_e_del) p.e_del *= p.a;
		if (!o.given_o_ins) p.o_ins *= p.a;
		if (!o.given_e_ins) p.e_ins *= p.a;
		if (!o.given_zdrop) p.zdrop *= p.a;
		if (!o.given_clip5) p.pen_clip5 *= p.a;
		if (!o.given_clip3) p.pen_clip3 *= p.a;
	}
	p.rg_id = o.rg_id.empty() ? nullptr : o.rg_id.c_str();
	return 0;
}

void show_params(const SamOpts &o)
{
	const cs_map_params_t &p = o.p;
	printf("a=%d\nb=%d\no_del=%d\ne_del=%d\no_ins=%d\ne_ins=%d\npen_clip5=%d\npen_clip3=%d\nw=%d\nzdrop=%d\nT=%d\n", p.a, p.b, p.o_del, p.e_del, p.o_ins, p.e_ins, p.pen_clip5, p.pen_clip3, p.w, p.zdrop, p.T);
	printf("min_seed_len=%d\nsplit_factor=%g\nsplit_width=%d\nmax_occ=%d\nmax_mem_intv=%lu\n", p.min_seed_len, (double)p.split_factor, p.split_width, p.max_occ, (unsigned long)p.max_mem_intv);
	printf("max_chain_gap=%d\nmax_chain_extend=%d\nmin_chain_weight=%d\n", p.max_chain_gap, p.max_chain_extend, p.min_chain_weight);
	printf("mask_level=%g\ndrop_ratio=%g\nxa_drop_ratio=%g\nmask_level_redun=%g\n", (double)p.mask_level, (double)p.drop_ratio, (double)p.xa_drop_ratio, (double)p.mask_level_redun);
	printf("mapq_coef_len=%d\nmax_xa_hits=%d\nmax_xa_hits_alt=%d\nflags=%u\nthreads=%d\nrg_id=%s\n", p.mapq_coef_len, p.max_xa_hits, p.max_xa_hits_alt, p.flags, p.threads, p.rg_id ? p.rg_id : "");
	printf("copy_comment=%d\nchunk_bases=%ld\n", o.copy_comment ? 1 : 0, o.fixed_chunk > 0 ? o.fixed_chunk : 10000000L * o.n_threads);
}

// a shard of a chunk: a contiguous read range with its offset arrays rebased to 0 (they live until the shard's text has been written)
struct Shard { int64_t r0 = 0, n = 0; std::vector<uint64_t> off, name_off, comment_off; };
// a chunk in flight: its bytes (copies: the reader's two buffer sets are fewer than the chunks in flight) and its shard per mapper
struct Flying { int64_t n = 0; std::vector<uint8_t> bases, quals; std::vector<char> names, comments; std::vector<Shard> shards; };
} // namespace

static int sam_main(int argc, char **argv)
{
	SamOpts o;
	if (int rc = parse_sam(argc, argv, o)) return rc;
	if (o.show) { show_params(o); return 0; }
	if (!o.sam || o.pos.size() != 2) { usage_sam(); return 1; }

	int ndev = 0;
	if (cs_device_count(&ndev) || ndev < 1) { fprintf(stderr, "[E::main] no MI355X visible: %s\n", cs_last_error()); return 1; }
	int n_gpus = o.n_gpus;
	std::vector<int> devices = o.devices;
	if (!devices.empty()) n_gpus = (int)devices.size();
	else { if (n_gpus < 1 || n_gpus > ndev) n_gpus = ndev; for (int g = 0; g < n_gpus; ++g) devices.push_back(g); }
	for (int d : devices) if (d < 0 || d >= ndev) { fprintf(stderr, "[E::main] --devices: no device %d (%d visible)\n", d, ndev); return 1; }
	cs_engine_options_t eopt; cs_engine_options_default(&eopt);
	eopt.count_sal_merged = 1; // "SA Lookup: ... calls, % merged" as CompSeed prints it (main.cpp:209-210)
	eopt.verbose = o.verbose;
	std::vector<cs_mapper_t *> mp((size_t)n_gpus, nullptr);
	for (int g = 0; g < n_gpus; ++g)
		if (cs_mapper_create(o.pos[0], devices[(size_t)g], &eopt, &o.p, &mp[(size_t)g])) { fprintf(stderr, "[E::main] GPU %d: %s\n", g, cs_last_error()); return 1; }

	const bool to_stdout = strcmp(o.sam, "-") == 0;
	FILE *fo = to_stdout ? stdout : fopen(o.sam, "wb");
	if (!fo) { fprintf(stderr, "[E::main] cannot write %s\n", o.sam); return 1; }
	{   // bwa_print_sam_hdr (main.cpp:436): the @SQ lines and -R's line
		size_t need = 0;
		const char *rg = o.rg_line.empty() ? nullptr : o.rg_line.c_str();
		(void)cs_mapper_header(mp[0], rg, nullptr, 0, &need);
		std::vector<char> hdr(need + 1);
		if (cs_mapper_header(mp[0], rg, hdr.data(), need, &need)) { fprintf(stderr, "[E::main] %s\n", cs_last_error()); return 1; }
		fwrite(hdr.data(), 1, need, fo);
	}
	const long chunk_bases = o.fixed_chunk > 0 ? o.fixed_chunk : 10000000L * o.n_threads; // main.cpp:437
	cs_reader_t *rd = nullptr;
	if (cs_reader_open(o.pos[1], chunk_bases, &rd)) { fprintf(stderr, "[E::main] %s\n", cs_last_error()); return 1; }

	// The reference's three-step pipeline (main.cpp:438) with the mappers' own threads behind it: every chunk is cut into one shard per
	// mapper and SUBMITTED (cs_map_submit), up to CS_MAP_MAX_IN_FLIGHT chunks kept in flight; this thread reads the next chunk meanwhile,
	// then collects the oldest chunk's shards in mapper order and writes their texts -- the file in read order, chunk by chunk.  The
	// reader has two buffer sets and a chunk must stay untouched until it is collected, so a chunk in flight is a copy of its bytes.
	auto bail = [&]() { for (cs_mapper_t *m : mp) cs_mapper_destroy(m); return 1; };   // (waits for what is in flight: no worker outlives main)
	std::deque<Flying> fl;
	uint64_t n_reads = 0;
	const auto t0 = std::chrono::steady_clock::now();
	for (bool have = true;;) {
		while (have && fl.size() < (size_t)CS_MAP_MAX_IN_FLIGHT) {
			cs_read_chunk_t c;
			if (cs_reader_next_chunk(rd, &c)) { fprintf(stderr, "[E::process] %s\n", cs_last_error()); return bail(); }
			if (!(have = c.n_reads > 0)) break;
			fl.emplace_back();
			Flying &f = fl.back();
			const bool cm = o.copy_comment && c.comment_off;               // -C (main.cpp:77-81)
			f.n = c.n_reads;
			f.bases.assign(c.bases, c.bases + c.offsets[c.n_reads]);
			if (c.quals) f.quals.assign(c.quals, c.quals + c.offsets[c.n_reads]);
			f.names.assign(c.names, c.names + c.name_off[c.n_reads]);
			if (cm) f.comments.assign(c.comments, c.comments + c.comment_off[c.n_reads]);
			f.shards.resize((size_t)n_gpus);
			for (int g = 0; g < n_gpus; ++g) {
				Shard &s = f.shards[(size_t)g];
				s.r0 = c.n_reads * g / n_gpus; s.n = c.n_reads * (g + 1) / n_gpus - s.r0;
				s.off.resize((size_t)s.n + 1); s.name_off.resize((size_t)s.n + 1); s.comment_off.resize(cm ? (size_t)s.n + 1 : 0);
				for (int64_t r = 0; r <= s.n; ++r) {
					s.off[(size_t)r] = c.offsets[s.r0 + r] - c.offsets[s.r0]; s.name_off[(size_t)r] = c.name_off[s.r0 + r] - c.name_off[s.r0];
					if (cm) s.comment_off[(size_t)r] = c.comment_off[s.r0 + r] - c.comment_off[s.r0];
				}
				if (cs_map_submit(mp[(size_t)g], s.n, f.bases.data() + c.offsets[s.r0], s.off.data(), c.quals ? f.quals.data() + c.offsets[s.r0] : nullptr, f.names.data() + c.name_off[s.r0],
				                  s.name_off.data(), cm ? f.comments.data() + c.comment_off[s.r0] : nullptr, cm ? s.comment_off.data() : nullptr, (int64_t)c.first_id + s.r0)) {
					fprintf(stderr, "[E::main] GPU %d: %s\n", g, cs_last_error());
					return bail();
				}
			}
		}
		if (fl.empty()) break;
		for (int g = 0; g < n_gpus; ++g) {
			cs_sam_result_t res;
			if (cs_map_collect(mp[(size_t)g], &res)) { fprintf(stderr, "[E::main] GPU %d: %s\n", g, cs_last_error()); return bail(); }
			if (res.n_bytes && fwrite(res.text, 1, (size_t)res.n_bytes, fo) != (size_t)res.n_bytes) { fprintf(stderr, "[E::main] cannot write %s\n", o.sam); return bail(); }
		}
		n_reads += (uint64_t)fl.front().n;
		fl.pop_front();
	}
	const double wall_s = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	cs_reader_close(rd);
	if (to_stdout ? fflush(fo) : fclose(fo)) { fprintf(stderr, "[E::main] cannot write %s\n", o.sam); return 1; }

	cs_stats_t tot; memset(&tot, 0, sizeof tot);
	cs_map_stats_t mt; memset(&mt, 0, sizeof mt);
	for (int g = 0; g < n_gpus; ++g) {
		cs_stats_t st; cs_mapper_engine_stats(mp[(size_t)g], &st);
		tot.reads += st.reads; tot.bwt_queries += st.bwt_queries; tot.bwt_calls += st.bwt_calls; tot.sal_queries += st.sal_queries;
		tot.sal_calls += st.sal_calls; tot.mems += st.mems; tot.seeds += st.seeds;
		tot.seed_kernel_ms = st.seed_kernel_ms > tot.seed_kernel_ms ? st.seed_kernel_ms : tot.seed_kernel_ms;
		tot.sal_kernel_ms = st.sal_kernel_ms > tot.sal_kernel_ms ? st.sal_kernel_ms : tot.sal_kernel_ms;
		cs_map_stats_t ms; cs_mapper_stats(mp[(size_t)g], &ms);
		mt.reads += ms.reads; mt.lines += ms.lines; mt.unmapped += ms.unmapped; mt.bytes += ms.bytes;
		for (int k = 0; k < CS_MAP_N_STAGES; ++k) mt.stage_ms[k] = ms.stage_ms[k] > mt.stage_ms[k] ? ms.stage_ms[k] : mt.stage_ms[k];   // (the mappers run side by side)
		cs_mapper_destroy(mp[(size_t)g]);
	}
	// display_profile, main.cpp:203-214
	fprintf(stderr, "BWT-extend:  %lu queries, %lu calls, %.2f %% hit in SST\n", (unsigned long)tot.bwt_queries, (unsigned long)tot.bwt_calls,
	        tot.bwt_queries ? 100.0 * (double)(tot.bwt_queries - tot.bwt_calls) / (double)tot.bwt_queries : 0.0);
	fprintf(stderr, "SA Lookup:   %lu queries, %lu calls, %.2f %% merged\n", (unsigned long)tot.sal_queries, (unsigned long)tot.sal_calls,
	        tot.sal_queries ? 100.0 * (double)(tot.sal_queries - tot.sal_calls) / (double)tot.sal_queries : 0.0);
	fprintf(stderr, "Wall time:   BWT %.2f SAL %.2f seconds on %d GPU(s); %lu reads, %lu mems, %lu seeds\n", tot.seed_kernel_ms / 1e3,
	        tot.sal_kernel_ms / 1e3, n_gpus, (unsigned long)tot.reads, (unsigned long)tot.mems, (unsigned long)tot.seeds);
	static const char *const stage[CS_MAP_N_STAGES] = {"upload", "seed", "chain", "filter", "extend", "download", "dedup", "mark", "cigar", "sam", "total"};
	for (int k = 0; k < CS_MAP_N_STAGES; ++k) fprintf(stderr, "Mapper %-9s %.2f ms\n", stage[k], mt.stage_ms[k]);
	fprintf(stderr, "SAM:         %lu reads, %lu lines, %lu unmapped, %.0f reads/s over %.3f seconds of mapping\n", (unsigned long)n_reads, (unsigned long)(mt.lines + mt.unmapped), (unsigned long)mt.unmapped,
	        wall_s > 0 ? (double)n_reads / wall_s : 0.0, wall_s);
	return 0;
}

int main(int argc, char **argv)
{
	setenv("GPU_MAX_HW_QUEUES", "8", 0); // before the HIP runtime starts: one engine per GPU, each with streams of its own
	for (int i = 1; i < argc; ++i) if (!strcmp(argv[i], "--sam") || !strcmp(argv[i], "--show-params")) return sam_main(argc, argv);
	return seed_main(argc, argv);
}
