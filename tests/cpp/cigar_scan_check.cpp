// cigar_scan_check.cpp -- the bodies of compseed_amd/csrc/cigar_scan.hpp (from regions to CIGAR, NM and MD: what cs_regions_cigar runs as
// kernels) driven in the kernels' order as a plain C++ program: check, classify, then per try the jobs' matrix bytes, an exclusive sum,
// chunks under a scratch budget, the fill, the counting walk with the retry decision, two exclusive sums, the writing walk.
// tests/test_cigar_scan_cpu.py writes a set's regions, reads, packed reference and contig offsets as flat binary files into a directory,
// runs this over them and compares what it writes with the reference's own SAM lines (tests/golden/sam1).  No GPU and no Python in the
// process: it can be built with -fsanitize=address,undefined and run as it is.
// Built with -DCS_EMU_W=N (lockstep.hpp) the fill runs its N-lane instantiation -- the wave kernel's -- on N threads in lockstep.
// Every job's fill score must be banded_global_score's (band_align.hpp; the one-lane build asks), no walk may leave its band, and the writing call must count
// what the counting call counted: exit status 1 otherwise.
//   cigar_scan_check DIR
//   in:  meta.bin (int64: n_reads n_regs l_pac a b o_del e_del o_ins e_ins w n_ctg budget), reg_off.bin, regs.bin, read_off.bin, bases.bin,
//        pac.bin, ctg_off.bin
//   out: alns.bin (cs_aln_t), cigar.bin (uint32), md.bin, stat.bin (uint64: dp_jobs nodp_jobs retries rejected cells chunks)
//   exit status 3: the input fails check_read (the library's CS_EINVAL)
#include "lockstep.hpp"
#include "../../compseed_amd/csrc/cigar_scan.hpp"

#include <cstring>


// the fill of one chunk of jobs: what a grid of waves does, job after job, on LANES lanes
struct Fill {
	const cscg::In *D; const cscg::Ref *R; const cs_aln_params_t *o; const cscg::State *S;
	const uint32_t *jobs; const uint64_t *zoff; size_t a, b; uint8_t *z; int32_t *he, *he2; int64_t rows;
	uint64_t cells, differ;
};
static void fill_lane(Fill &F, int lane)
{
	for (size_t t = F.a; t < F.b; ++t) {
		const uint32_t g = F.jobs[t];
		const cs_alnreg_t x = F.D->regs[g];
		const int w2 = F.S->w2[g];
		const csdd::Span S = cscg::job_span(*F.R, x, F.D->bases + F.D->read_off[F.S->rd[g]]);
		int score, other;
		if (cscg::job_nodp(x, w2)) { score = cscg::sum_score<LANES>(S, *F.o, lane); other = score; }
		else {
			const int w = cscg::job_band(*F.o, x, w2), tlen = (int)(x.re - x.rb);
			score = cscg::global_fill<LANES>(S, tlen, *F.o, w, F.he, F.he + F.rows, F.z + (F.zoff[t] - F.zoff[F.a]), lane);
#ifdef CS_EMU_W
			other = score;                                            // (the lockstep build's result is compared with the one-lane build's, byte for byte)
#else
			other = csdd::banded_global_score<LANES>(S, tlen, *F.o, w, F.he2, F.he2 + F.rows, lane);
#endif
			if (lane == 0) F.cells += (uint64_t)tlen * (uint64_t)cscg::job_ncol(S.qlen, w);
		}
		if (lane == 0) { F.S->score[g] = score; if (score != other) ++F.differ; }
	}
}

int main(int argc, char **argv)
{
	if (argc != 2) { fprintf(stderr, "usage: cigar_scan_check DIR\n"); return 2; }
	const std::string d = std::string(argv[1]) + "/";
	std::vector<int64_t> meta, ctg_off; std::vector<uint64_t> reg_off, read_off; std::vector<cs_alnreg_t> regs; std::vector<uint8_t> bases, pac;
	if (!slurp(d + "meta.bin", meta) || !slurp(d + "reg_off.bin", reg_off) || !slurp(d + "regs.bin", regs) || !slurp(d + "read_off.bin", read_off) ||
	    !slurp(d + "bases.bin", bases) || !slurp(d + "pac.bin", pac) || !slurp(d + "ctg_off.bin", ctg_off))
		return 2;
	if (meta.size() != 12) { fprintf(stderr, "meta.bin: 12 words expected\n"); return 2; }
	const int64_t n = meta[0];
	const uint64_t n_regs = (uint64_t)meta[1], budget = (uint64_t)meta[11];
	if (n < 0 || reg_off.size() != (size_t)n + 1 || read_off.size() != (size_t)n + 1 || regs.size() != n_regs || (int64_t)ctg_off.size() != meta[10] || ctg_off.empty()) {
		fprintf(stderr, "inconsistent input\n");
		return 2;
	}
	pac.resize(pac.size() + 8, 0);
	cs_aln_params_t o;
	memset(&o, 0, sizeof o);
	o.a = (int32_t)meta[3]; o.b = (int32_t)meta[4]; o.o_del = (int32_t)meta[5]; o.e_del = (int32_t)meta[6]; o.o_ins = (int32_t)meta[7]; o.e_ins = (int32_t)meta[8]; o.w = (int32_t)meta[9];
	const cscg::Ref R = {meta[2], pac.data(), ctg_off.data(), (int)ctg_off.size()};
	const cscg::In D = {reg_off.data(), read_off.data(), regs.data(), bases.data(), n, n_regs};

	// check: a lane per read
	std::vector<uint32_t> rd(n_regs + 1, 0);
	uint64_t longest = 0; bool bad = false;
	for (int64_t r = 0; r < n; ++r) { uint64_t len; if (!cscg::check_read(D, R.l_pac, r, rd.data(), &len)) bad = true; longest = len > longest ? len : longest; }
	if (bad || (n == 0 && n_regs)) { fprintf(stderr, "the input fails the checks\n"); return 3; }
	// classify: a lane per region
	std::vector<uint8_t> cls(n_regs + 1, 0); std::vector<int32_t> w2(n_regs + 1, 0), tries(n_regs + 1, 0), score(n_regs + 1, 0), last_sc(n_regs + 1, 0);
	const cscg::State S = {rd.data(), cls.data(), w2.data(), tries.data(), score.data(), last_sc.data()};
	std::vector<cs_aln_t> alns(n_regs); std::vector<uint32_t> cigar; std::vector<char> md(1, 0);
	std::vector<uint64_t> stat(6, 0);
	std::vector<uint32_t> active;
	for (uint64_t g = 0; g < n_regs; ++g) {
		int w = 0;
		cls[g] = (uint8_t)cscg::classify(R, o, regs[g], &w);
		w2[g] = w; last_sc[g] = -(1 << 30);
		cs_aln_t e; memset(&e, 0, sizeof e);
		e.pos = -1; e.rid = -1; e.nm = cls[g] == cscg::J_REJECT ? -1 : 0;
		alns[g] = e;
		if (cls[g] == cscg::J_REJECT) ++stat[3];
		if (cls[g] == cscg::J_JOB) active.push_back((uint32_t)g);
	}
	std::vector<int32_t> he(2 * (longest + 1)), he2(2 * (longest + 1));
	std::vector<uint8_t> z;
	uint64_t flagged = 0, differ = 0, miscount = 0;
	for (int pass = 0; pass < 3 && !active.empty(); ++pass) {
		const size_t nj = active.size();
		std::vector<uint64_t> zoff(nj + 1, 0);                       // the jobs' matrix bytes and their exclusive sum
		for (size_t t = 0; t < nj; ++t) zoff[t + 1] = zoff[t] + cscg::job_bytes(o, regs[active[t]], w2[active[t]]);
		std::vector<uint32_t> next;
		for (size_t a = 0; a < nj; ) {                                // chunks under the budget; a job above it has a chunk of its own
			size_t b = a + 1;
			while (b < nj && zoff[b + 1] - zoff[a] <= budget) ++b;
			++stat[5];
			z.assign((size_t)(zoff[b] - zoff[a]) + 1, 0xff);
			Fill F = {&D, &R, &o, &S, active.data(), zoff.data(), a, b, z.data(), he.data(), he2.data(), (int64_t)longest + 1, 0, 0};
			if (!run_lanes([&F](int lane) { fill_lane(F, lane); })) return 2;
			stat[4] += F.cells; differ += F.differ;
			// the counting walk and the retry decision: a lane per job
			std::vector<cscg::Counts> cnt(b - a); std::vector<uint64_t> coff(b - a + 1, 0), moff(b - a + 1, 0);
			for (size_t t = a; t < b; ++t) {
				const uint32_t g = active[t];
				const cs_alnreg_t x = regs[g];
				cscg::Counts c; memset(&c, 0, sizeof c);
				int nw = 0;
				const bool nodp = cscg::job_nodp(x, w2[g]);
				if (!cscg::next_try(o, x, w2[g], score[g], last_sc[g], tries[g], &nw)) {
					last_sc[g] = score[g]; w2[g] = nw; ++tries[g]; ++stat[2];
					next.push_back(g);
					cls[g] = cscg::J_JOB + 1;                         // (goes round again: nothing of this try is kept)
				} else {
					++tries[g]; cls[g] = cscg::J_JOB;
					++stat[nodp ? 1 : 0];
					c = cscg::count_aln(R, o, x, bases.data() + read_off[rd[g]], (int)(read_off[rd[g] + 1] - read_off[rd[g]]), w2[g], z.data() + (zoff[t] - zoff[a]));
					if (c.flagged) ++flagged;
				}
				cnt[t - a] = c;
				coff[t - a + 1] = coff[t - a] + (cls[g] == cscg::J_JOB ? c.n_cigar : 0);
				moff[t - a + 1] = moff[t - a] + (cls[g] == cscg::J_JOB ? c.md_bytes : 0);
			}
			// the writing walk: a lane per job, into the chunk's share of the result
			const size_t c0 = cigar.size(), m0 = md.size();
			cigar.resize(c0 + (size_t)coff[b - a], 0xffffffffu); md.resize(m0 + (size_t)moff[b - a], (char)0x7f);
			for (size_t t = a; t < b; ++t) {
				const uint32_t g = active[t];
				if (cls[g] != cscg::J_JOB) continue;
				cs_aln_t out; memset(&out, 0, sizeof out);
				out.cigar_off = c0 + coff[t - a]; out.md_off = m0 + moff[t - a];
				if (!cscg::finish_aln(R, o, regs[g], bases.data() + read_off[rd[g]], (int)(read_off[rd[g] + 1] - read_off[rd[g]]), w2[g], score[g], tries[g], z.data() + (zoff[t] - zoff[a]),
				                      cnt[t - a], cigar.data() + out.cigar_off, md.data() + out.md_off, &out))
					++miscount;
				alns[g] = out;
			}
			a = b;
		}
		active.swap(next);
	}
	if (!active.empty()) { fprintf(stderr, "jobs left after three tries\n"); return 1; }
	if (differ || flagged || miscount) {
		fprintf(stderr, "%llu jobs score otherwise than banded_global_score, %llu walks left their band, %llu jobs were written otherwise than counted\n",
		        (unsigned long long)differ, (unsigned long long)flagged, (unsigned long long)miscount);
		return 1;
	}
	if (!spill(d + "alns.bin", alns) || !spill(d + "cigar.bin", cigar) || !spill(d + "md.bin", md) || !spill(d + "stat.bin", stat)) return 2;
	return 0;
}
