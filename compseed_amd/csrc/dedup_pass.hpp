// dedup_pass.hpp -- the bodies of a device de-duplication pass (cs_dedup_regions on the GPU), each a plain function
// indexed by read, lane or word, so that a kernel is a grid-stride loop of a few lines around one of them.  NO kernel includes this
// header yet: the kernels written around these bodies (check, light, wave, keep, scatter, offsets; one wave a block, no kernel waiting
// for another, a linear host function) did not return from dd_wave_kernel on an MI355X (main100, flags 0), the cause was not found, and
// they are not in the library.  tests/cpp/dedup_pass_check.cpp drives the bodies in the pass's order without a GPU, with a plain
// exclusive sum where a device pass calls rocPRIM.  In the order of the pass:
//   check_read    a lane per read: reg_off is a CSR array from 0 to n_regs, read_off starts at 0 and does not decrease, a read with regions
//                 is shorter than MAX_READ_LEN, a live region lies inside its read and inside [0, 2 l_pac) and spans at most 2 MAX_READ_LEN
//                 of the reference.  The lane compares its own two entries of each offset array with each other and with the host counts
//                 BEFORE it walks [reg_off[r], reg_off[r + 1]); nothing else follows an offset until the host has seen the verdict.  Every
//                 later loop's trip count follows from these: a read's lists hold at most its own regions, a patch alignment has at most
//                 the read's length + 1 columns and (two region spans + max_chain_gap) rows.
//   light_read    a lane per read: 0 or 1 live regions are the result as they are (the single one with n_comp 0, as dedup_read leaves it)
//   heavy_read    W lanes per read (a block of ONE wave on the device): csdd::dedup_read over scratch at the read's input offset -- a
//                 read's survivors never outnumber its input, so the input offsets serve for every per-read list
//   keep_flags    a lane per read: staging entries [reg_off[r], reg_off[r] + cnt[r]) are kept
//   move_word / off_live (compact.hpp), move_nc    the survivors, their n_comp and the offsets after an exclusive scan of the flags
// No body waits for another lane's, wave's or block's memory: order between them comes from the kernel boundaries.
#pragma once
#include "compact.hpp"
#include "dedup_scan.hpp"

namespace csdp {
constexpr uint64_t MAX_READ_LEN = 65536;                               // as in the extension stage (align_gpu.hip)
constexpr int LDS_ROWS = 1025;                                         // H and E of a patch of up to 1,024 read bases: 8,200 bytes of LDS a block (unmeasured)
enum { C_BAD, C_NBASES, C_LONGEST, C_OUT, C_HEAVY, C_ALIGNS, C_MERGES, C_COUNT };   // the pass's counter words

struct In { const uint64_t *reg_off, *read_off; const cs_alnreg_t *regs; const uint8_t *bases; int64_t n_reads; uint64_t n_regs; };
// batch-sized lists at the reads' input offsets (a, nc, srt: dedup_read's; stage, stage_nc: a read's survivors), and per read cnt / heavy
struct Lists { cs_alnreg_t *a; int32_t *nc; csdd::SRec *srt; cs_alnreg_t *stage; int32_t *stage_nc; uint32_t *cnt; uint8_t *heavy; };

// true: the read's entries are consistent; *len: its length if it has regions (0 otherwise)
CS_HD inline bool check_read(const In &D, int64_t l_pac, int64_t r, uint64_t *len)
{
	*len = 0;
	const uint64_t c0 = D.reg_off[r], c1 = D.reg_off[r + 1], b0 = D.read_off[r], b1 = D.read_off[r + 1];
	if (c1 < c0 || c1 > D.n_regs || b1 < b0 || (r == 0 && (b0 != 0 || c0 != 0)) || (r == D.n_reads - 1 && c1 != D.n_regs)) return false;
	if (c1 == c0) return true;
	const uint64_t l = b1 - b0;
	if (l >= MAX_READ_LEN) return false;
	*len = l;
	for (uint64_t g = c0; g < c1; ++g) {                              // (c0 <= c1 <= n_regs: inside the array)
		const cs_alnreg_t x = D.regs[g];
		if (x.qe <= x.qb) continue;                                   // purged: dropped, whatever it holds
		if (x.qb < 0 || (uint64_t)x.qe > l || x.rb < 0 || x.rb >= x.re || x.re > (l_pac << 1) || x.re - x.rb > (int64_t)(2 * MAX_READ_LEN)) return false;
	}
	return true;
}

// returns 1 for a heavy read (two live regions or more: heavy_read's), 0 otherwise with the read's result written
CS_HD inline int light_read(const In &D, const Lists &S, int64_t r)
{
	const uint64_t g0 = D.reg_off[r], g1 = D.reg_off[r + 1];
	uint32_t n = 0; uint64_t first = g0;
	for (uint64_t g = g0; g < g1; ++g) if (D.regs[g].qe > D.regs[g].qb) { if (n == 0) first = g; ++n; }
	if (n > 1) { S.heavy[r] = 1; return 1; }
	S.heavy[r] = 0; S.cnt[r] = n;
	if (n == 1) { S.stage[g0] = D.regs[first]; S.stage_nc[g0] = 0; }
	return 0;
}

template <int W> CS_HD inline void heavy_read(const In &D, const csdd::Par &P, const Lists &S, int64_t r, int lane, const csdd::Work &wk, csdd::Stat &st)
{
	const uint64_t g0 = D.reg_off[r];
	const int n_in = (int)(D.reg_off[r + 1] - g0);
	const int k = csdd::dedup_read<W>(P, D.regs + g0, n_in, D.bases + D.read_off[r], lane, S.a + g0, S.nc + g0, S.srt + g0, wk, true, S.stage + g0, S.stage_nc + g0, st);
	if (lane == 0) S.cnt[r] = (uint32_t)k;
}

// keep[g] for the read's own regions; the last read also writes the flag behind the last region (0: the scan's total)
CS_HD inline void keep_flags(const In &D, const uint32_t *cnt, int64_t r, uint32_t *keep)
{
	const uint64_t g0 = D.reg_off[r], g1 = D.reg_off[r + 1], k = cnt[r];
	for (uint64_t g = g0; g < g1; ++g) keep[g] = g - g0 < k ? 1u : 0u;
	if (r == D.n_reads - 1) keep[D.n_regs] = 0;
}

CS_HD inline void move_nc(const int32_t *in, const uint32_t *keep, const uint32_t *scan, uint64_t g, int32_t *out) { if (keep[g]) out[scan[g]] = in[g]; }
} // namespace csdp
