// smem_reads.hpp -- the reads as 16-byte records of 32 bases, made on the device: the twin of host_pack.cpp, which makes the same
// records on the host (tests/test_host_pack.py holds the two against each other).  PackedReader (smem_common.hpp) reads them.
#pragma once
#include "fm_device.hpp"

namespace csd {

// The reads a second time, packed: one 16-byte record per 32 bases -- .x/.y the bases, 2 bits each, base j in bits 2j..2j+1 (the
// order of the 2-bit text), .z one bit per base that is ambiguous or lies behind the end of the read.  Record k of read r is
// rec[(off[r] >> 5) + r + k]: no second offset array, and read r owns at least len/32 + 1 records, so the record of position
// len exists and says "end" there.  Why: at 6-8 waves per SIMD the lanes in flight touch more lines than the L2 holds, so every
// 8-byte window of a byte-per-base read and every 4-byte word of the text came from HBM again (fwd0_kernel fetched 30 lines per
// read for 12 lines' worth of data); with 32 bases per load there is one fetch per record.
// RAW: straight from the caller's bytes (ASCII or nt4 codes; nst_nt4_table, FM_index/bntseq.c:46-63, codes 0..4 pass through as in
// comp_seed.cpp:2259) -- the byte-per-base nt4 copy is then only made when the fused kernel has to step in.  n_bases bounds the loads.
template <bool RAW>
__global__ void pack_reads_kernel(const uint8_t *seq, const uint64_t *off, int64_t n_reads, uint64_t n_bases, uint4 *rec)
{
	// letters -> codes through a 256-byte table in LDS (((c >> 1) ^ (c >> 2)) & 3 for A C G T in either case, the codes 0..3 as they
	// are, 4 for everything else): one LDS read per base instead of a dozen instructions
	__shared__ uint8_t lut[256];
	if (RAW) {
		for (uint32_t c = threadIdx.x; c < 256u; c += blockDim.x) {
			const uint32_t t = (c & 0xdfu) - 0x41u;
			const bool letter = t < 20u && ((0x80045u >> t) & 1u);
			lut[c] = (uint8_t)(c < 4u ? c : letter ? ((c >> 1) ^ (c >> 2)) & 3u : 4u);
		}
		__syncthreads();
	}
	const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = ((uint64_t)gridDim.x * blockDim.x) >> 3;
	for (uint64_t r = gid >> 3; r < (uint64_t)n_reads; r += gstride) { // eight lanes per read, a record each
		const uint64_t rb = off[r], re = off[r + 1], len = re - rb;
		const uint64_t w0 = (rb >> 5) + r, nrec = (re >> 5) + r + 1 - w0;
		for (uint64_t k = gid & 7; k < nrec; k += 8) {
			uint4 o = {0u, 0u, ~0u, 0u};
			if (k * 32 < len) {
				const uint64_t a = rb + k * 32, a0 = a & ~7ull;                // (the nt4 copy is padded by 64 bytes; the caller's buffer is not)
				const uint64_t *w = reinterpret_cast<const uint64_t *>(seq + a0);
				const uint32_t sh = (uint32_t)(a - a0) << 3;
				uint64_t v[5];
#pragma unroll
				for (int q = 0; q < 5; ++q) {
					const uint64_t wa = a0 + 8u * (uint32_t)q;
					if (!RAW || wa + 8 <= n_bases) v[q] = w[q];
					else { // the word that holds the caller's last bytes: assembled bytewise, nothing behind n_bases is read
						uint64_t t = 0x0404040404040404ull;
						for (uint64_t z = wa; z < n_bases; ++z) t = (t & ~(0xffull << ((z - wa) << 3))) | (uint64_t)seq[z] << ((z - wa) << 3);
						v[q] = t;
					}
				}
				uint64_t bases = 0; uint32_t bad = 0;
#pragma unroll
				for (int q = 0; q < 4; ++q) {
					uint64_t b8 = sh ? (v[q] >> sh) | (v[q + 1] << (64u - sh)) : v[q]; // bases 8q .. 8q+7, a byte each
					if (RAW) {
						uint64_t c8 = 0;
#pragma unroll
						for (int z = 0; z < 8; ++z) c8 |= (uint64_t)lut[(uint32_t)(b8 >> (8 * z)) & 0xffu] << (8 * z);
						b8 = c8;
					}
					bad |= (uint32_t)((((b8 >> 2) & 0x0101010101010101ull) * 0x0102040810204080ull) >> 56) << (8 * q);
					b8 &= 0x0303030303030303ull;
					b8 = (b8 | (b8 >> 6)) & 0x000F000F000F000Full;
					b8 = (b8 | (b8 >> 12)) & 0x000000FF000000FFull;
					bases |= ((b8 | (b8 >> 24)) & 0xFFFFull) << (16 * q);
				}
				const uint64_t left = len - k * 32;
				if (left < 32) { bad |= ~0u << (uint32_t)left; bases &= (1ull << (2 * (uint32_t)left)) - 1ull; }
				o.x = (uint32_t)bases; o.y = (uint32_t)(bases >> 32); o.z = bad;
			}
			rec[w0 + k] = o;
		}
	}
}
// The way back, for the rare case that the host made the records (host_pack.cpp) and the fused kernel has to step in: a byte per
// base, codes 0..3, 4 for an ambiguous base.
__global__ void unpack_reads_kernel(const uint4 *rec, const uint64_t *off, int64_t n_reads, uint8_t *out)
{
	const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x, gstride = ((uint64_t)gridDim.x * blockDim.x) >> 3;
	for (uint64_t r = gid >> 3; r < (uint64_t)n_reads; r += gstride) {
		const uint64_t rb = off[r], len = off[r + 1] - rb;
		const uint4 *rr = rec + (rb >> 5) + r;
		for (uint64_t k = gid & 7; k * 32 < len; k += 8) {
			const uint4 v = rr[k];
			const uint64_t bases = (uint64_t)v.x | (uint64_t)v.y << 32, left = len - k * 32;
			for (uint32_t j = 0; j < 32u && j < left; ++j) out[rb + k * 32 + j] = (uint8_t)((v.z >> j) & 1u ? 4u : (uint32_t)(bases >> (2 * j)) & 3u);
		}
	}
}

} // namespace csd
