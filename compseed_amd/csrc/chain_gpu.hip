// chain_gpu.hip -- cs_chain_batch_device / cs_chain_batch_gpu: mem_chain of the reference (mapping/comp_seed.cpp:241-285, test_and_merge
// :182-203, the kbtree of cstl/kbtree.h) on the GPU, bit-identical to cs_chain_batch (chain.cpp), which stays the specification.
// Everything per read runs in kernels: the contig lookup, the merge rule, the choice of chain, frac_rep, the traversal order and the CSR
// compaction.  The work of a read is sequential over its seeds, so a read is one lane (one wave for reads with many seeds):
//   fast_kernel       reads of up to WAVE_MIN seeds, one lane each, on a SORTED ARRAY of (position, chain id) instead of the B-tree.  While
//                     every inserted key is distinct, the tree's lower(k) is the predecessor of k and its in-order traversal is ascending key
//                     order, so the array gives the tree's answers exactly; the two can only differ after a key is inserted that equals an
//                     existing one.  A read leaves this path at the first such insertion and is replayed on the tree path.  Reads of more
//                     seeds go to the wave list, every read to the tree list under CS_CHAIN_TREE_ONLY.
//   fast_wave_kernel  the same for the wave list, one wave per read: the predecessor search is 64-ary (a ballot over 64 probes per step)
//                     and the insertion shift moves 64 entries per step (a mem with x2 near max_occ gives a read hundreds of chains).
//   tree_kernel       Tree::locate / lower / split / put / traverse of chain.cpp, one lane per read, nodes in an HBM arena (a read never
//                     has more than seeds / 4 + 2 nodes: every node but the root holds at least BT - 1 = 4 keys).  Only reads with equal
//                     keys (tandem arrays) take it unless CS_CHAIN_TREE_ONLY sends all.
//   compact_kernel    every path writes a read's chains in traversal order and its chained seeds into scratch at the read's own seed slots
//                     (both counts are at most its seed count); two exclusive scans over the per-read counts give chain_off and the seed
//                     bases, and this kernel moves the chains and seeds into the output CSR and writes cseed_off.  No overflow case.
// frac_rep is (float)l_rep / len as on the host: IEEE fp32 division is correctly rounded (no fast-math, no approximate reciprocal).
#include "dev_stage.hpp"

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include <hip/hip_runtime.h>

namespace csc {
constexpr int BT = 5, BMAX = 2 * BT - 1;   // the B-tree of chain.cpp (kb_init(chn, 512) with a 40-byte key)
constexpr int WAVE_MIN = 64;               // reads with more seeds than this go one wave per read
constexpr uint32_t END = 0xffffffffu;
constexpr int STACK = 32;                  // traversal stack: a tree of height 32 would need 5^31 keys

struct Chain { int64_t pos; int32_t rid, n; cs_seed_t head, tail; uint32_t first, last; };   // chain.cpp's Chain
struct Node { int32_t n, internal; int64_t pos[BMAX]; int32_t id[BMAX]; int32_t kid[BMAX + 1]; };

// the counter words: reads on the wave list, reads on the tree list, arena nodes reserved, reads with inconsistent offsets, arena overflows
enum { C_WAVE, C_TREE, C_NODES, C_BAD, C_OVERFLOW, C_COUNT };

struct Args {
	const uint64_t *mem_off, *seed_off, *read_off; const cs_intv_t *mems; const cs_seed_t *seeds;
	int64_t n_reads; uint64_t n_mems, n_seeds; int64_t l_pac;
	const int64_t *ctg_off; const int32_t *is_alt; int32_t n_ctg; uint32_t flags;
	cs_chain_params_t o;
	int64_t *key; int32_t *cid; Chain *pool; uint32_t *next_of;   // per seed slot: the sorted array, the chains, the seed lists
	cs_chain_t *tch; cs_seed_t *tsd;                               // per seed slot: a read's chains and chained seeds before compaction
	uint64_t *nch, *nsd;                                           // per read: counts (n + 1, the last 0), scanned into chain_off / sbase
	uint32_t *wave_list, *tree_list; uint64_t *tree_node0;         // reads for the wave kernel / the tree kernel (with their arena start)
	Node *arena;
	unsigned long long *ctr;   // the C_* words
	uint64_t *chain_off, *sbase, *cseed_off; cs_chain_t *chains; cs_seed_t *cseeds;
};

__device__ __forceinline__ int contig_of(const Args &A, int64_t fwd_pos)   // bns_pos2rid: upper_bound over the contig offsets, minus one
{
	if (fwd_pos >= A.l_pac) return -1;
	int lo = 0, hi = A.n_ctg;
	while (lo < hi) { const int mid = (lo + hi) >> 1; if (A.ctg_off[mid] <= fwd_pos) lo = mid + 1; else hi = mid; }
	return lo - 1;
}
__device__ __forceinline__ int contig_of_seed(const Args &A, int64_t rb, int64_t re)   // bns_intv2rid, as chain.cpp's contig_of_seed
{
	const int64_t l_pac = A.l_pac;
	if (rb < l_pac && l_pac < re) return -2;
	const int first = contig_of(A, rb < l_pac ? rb : 2 * l_pac - 1 - rb);
	if (re <= rb) return first;
	const int64_t p = re - 1;
	return contig_of(A, p < l_pac ? p : 2 * l_pac - 1 - p) == first ? first : -1;
}
// test_and_merge as chain.cpp's absorb: 0 = a new chain starts, 1 = inside the chain already, 2 = appended to it
__device__ __forceinline__ int absorb_kind(const cs_chain_params_t &o, int64_t l_pac, const Chain &c, const cs_seed_t &s, int seed_rid)
{
	if (seed_rid != c.rid) return 0;
	const cs_seed_t &head = c.head, &tail = c.tail;
	const bool in_query = s.qbeg >= head.qbeg && s.qbeg + s.len <= tail.qbeg + tail.len;
	const bool in_ref = s.rbeg >= head.rbeg && s.rbeg + s.len <= tail.rbeg + tail.len;
	if (in_query && in_ref) return 1;
	const bool chain_fwd = tail.rbeg < l_pac || head.rbeg < l_pac;
	if (chain_fwd && s.rbeg >= l_pac) return 0;
	const int64_t dq = (int64_t)s.qbeg - tail.qbeg, dr = s.rbeg - tail.rbeg;
	const bool near_diag = dq - dr <= o.w && dr - dq <= o.w;
	const bool close = dq - tail.len < o.max_chain_gap && dr - tail.len < o.max_chain_gap;
	if (dr < 0 || !near_diag || !close) return 0;
	return 2;
}
__device__ float frac_rep_of(const Args &A, int64_t r, int len)   // comp_seed.cpp:271-280
{
	int beg = 0, end = 0, l_rep = 0;
	for (uint64_t m = A.mem_off[r]; m < A.mem_off[r + 1]; ++m) {
		const cs_intv_t M = A.mems[m];
		if (M.x2 <= (uint64_t)A.o.max_occ) continue;
		const int b = (int)(M.info >> 32), e = (int)(uint32_t)M.info;
		if (b > end) { l_rep += end - beg; beg = b; end = e; } else end = max(end, e);
	}
	l_rep += end - beg;
	return (float)l_rep / (float)len;
}
__device__ __forceinline__ void emit_chain(const Args &A, uint64_t b, float frac, int32_t id, uint32_t &nc, uint32_t &ns)
{
	const Chain c = A.pool[b + id];
	cs_chain_t o; o.pos = c.pos; o.rid = c.rid; o.n_seeds = c.n; o.frac_rep = frac; o.is_alt = A.is_alt[c.rid];
	A.tch[b + nc++] = o;
	for (uint32_t k = c.first; k != END; k = A.next_of[b + k]) A.tsd[b + ns++] = A.seeds[b + k];
}
__device__ __forceinline__ void new_chain(const Args &A, uint64_t b, int32_t id, const cs_seed_t &s, int rid, uint32_t li)
{
	Chain c; c.pos = s.rbeg; c.rid = rid; c.n = 1; c.head = c.tail = s; c.first = c.last = li;
	A.pool[b + id] = c; A.next_of[b + li] = END;
}
__device__ __forceinline__ void append_seed(const Args &A, uint64_t b, int32_t id, const Chain &c, const cs_seed_t &s, uint32_t li)
{
	A.next_of[b + c.last] = li; A.next_of[b + li] = END;
	Chain &C = A.pool[b + id];
	C.last = li; C.tail = s; C.n = c.n + 1;
}
__device__ __forceinline__ void push_tree(const Args &A, int64_t r, uint64_t n_seeds)
{
	const unsigned long long t = atomicAdd(A.ctr + C_TREE, 1ull);
	A.tree_list[t] = (uint32_t)r;
	A.tree_node0[t] = atomicAdd(A.ctr + C_NODES, (unsigned long long)(n_seeds / 4 + 2));
}

// number of keys <= k in the ascending key[0..n): W = 1 a binary search, W = 64 a 64-ary one (lanes probe, a ballot counts)
template <int W> __device__ __forceinline__ int count_le(const int64_t *key, int n, int64_t k, int lane)
{
	int lo = 0, hi = n;
	if constexpr (W == 1) {
		while (lo < hi) { const int mid = (lo + hi) >> 1; if (key[mid] <= k) lo = mid + 1; else hi = mid; }
		return lo;
	}
	while (hi - lo > W) {   // keys before lo are <= k, keys from hi on are > k
		const int step = (hi - lo + W - 1) / W, p = lo + lane * step;
		const int c = __popcll(__ballot(p < hi && key[p] <= k));
		if (c == 0) return lo;
		const int nhi = min(hi, lo + c * step);
		lo = lo + (c - 1) * step + 1; hi = nhi;
	}
	const int p = lo + lane;
	return lo + __popcll(__ballot(p < hi && key[p] <= k));
}

// the read on the sorted array; false = it inserted a key equal to an existing one (nothing of it is final then)
template <int W> __device__ bool chain_fast(const Args &A, int64_t r, int lane)
{
	const uint64_t b = A.seed_off[r], e = A.seed_off[r + 1];
	int64_t *key = A.key + b; int32_t *cid = A.cid + b;
	int n = 0;
	for (uint64_t c0 = b; c0 < e; c0 += W) {
		// the next W seeds and their contigs, one per lane (they do not depend on the chains): off the sequential path below, which takes them by shuffle
		cs_seed_t mine = {}; int mine_rid = -1;
		if (c0 + lane < e) { mine = A.seeds[c0 + lane]; mine_rid = contig_of_seed(A, mine.rbeg, mine.rbeg + mine.len); }
		const int cnt = (int)min((uint64_t)W, e - c0);
		for (int j = 0; j < cnt; ++j) {
			cs_seed_t s; int rid;
			if constexpr (W == 1) { s = mine; rid = mine_rid; }
			else { s.rbeg = __shfl(mine.rbeg, j); s.qbeg = __shfl(mine.qbeg, j); s.len = __shfl(mine.len, j); rid = __shfl(mine_rid, j); }
			if (rid < 0) continue;   // bridging two sequences or the forward-reverse boundary
			const uint32_t li = (uint32_t)(c0 + j - b);
			const int up = n ? count_le<W>(key, n, s.rbeg, lane) : 0;
			bool add = true;
			if (up > 0) {
				const int32_t lo = cid[up - 1];
				const Chain c = A.pool[b + lo];
				const int kind = absorb_kind(A.o, A.l_pac, c, s, rid);
				if (kind == 2 && lane == 0) append_seed(A, b, lo, c, s, li);
				add = kind == 0;
				if (add && key[up - 1] == s.rbeg) return false;   // an equal key: from here on the B-tree's own placement decides
			}
			if (add) {
				if constexpr (W == 1) {
					for (int i = n - 1; i >= up; --i) { key[i + 1] = key[i]; cid[i + 1] = cid[i]; }
				} else {
					for (int top = n - 1; top >= up; top -= W) {   // 64 entries per step: all loads, then all stores
						const int i = top - lane; int64_t kk = 0; int32_t cc = 0;
						if (i >= up) { kk = key[i]; cc = cid[i]; }
						__syncthreads();
						if (i >= up) { key[i + 1] = kk; cid[i + 1] = cc; }
						__syncthreads();
					}
				}
				if (lane == 0) { key[up] = s.rbeg; cid[up] = n; new_chain(A, b, n, s, rid, li); }
				++n;
			}
			if constexpr (W > 1) __syncthreads();
		}
	}
	if (lane == 0) {
		const float frac = frac_rep_of(A, r, (int)(A.read_off[r + 1] - A.read_off[r]));
		uint32_t nc = 0, ns = 0;
		for (int j = 0; j < n; ++j) emit_chain(A, b, frac, cid[j], nc, ns);
		A.nch[r] = nc; A.nsd[r] = ns;
	}
	return true;
}

__global__ void __launch_bounds__(256) fast_kernel(Args A)
{
	for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < A.n_reads; r += (int64_t)gridDim.x * blockDim.x) {
		const uint64_t b = A.seed_off[r], e = A.seed_off[r + 1];
		A.nch[r] = 0; A.nsd[r] = 0;
		if (e < b || e > A.n_seeds || A.mem_off[r + 1] < A.mem_off[r] || A.mem_off[r + 1] > A.n_mems) { atomicAdd(A.ctr + C_BAD, 1ull); continue; }
		const int len = (int)(A.read_off[r + 1] - A.read_off[r]);
		if (A.flags & CS_CHAIN_TREE_ONLY) { push_tree(A, r, e - b); continue; }
		if (len < A.o.min_seed_len) continue;
		if (e - b > (uint64_t)WAVE_MIN) { A.wave_list[atomicAdd(A.ctr + C_WAVE, 1ull)] = (uint32_t)r; continue; }
		if (!chain_fast<1>(A, r, 0)) push_tree(A, r, e - b);
	}
}

__global__ void __launch_bounds__(64) fast_wave_kernel(Args A)
{
	const unsigned long long n = A.ctr[C_WAVE];
	const int lane = threadIdx.x;
	for (unsigned long long w = blockIdx.x; w < n; w += gridDim.x) {
		const int64_t r = A.wave_list[w];
		const bool ok = chain_fast<64>(A, r, lane);
		if (!ok && lane == 0) push_tree(A, r, A.seed_off[r + 1] - A.seed_off[r]);
		__syncthreads();
	}
}

// chain.cpp's Tree with the nodes in the arena; false = the arena reserve ran out (cannot happen: counted in C_OVERFLOW)
struct Tree {
	Node *nd; int cap, cnt, root, size;
	__device__ void init(Node *p, int c) { nd = p; cap = c; cnt = 1; root = 0; size = 0; nd[0].n = 0; nd[0].internal = 0; }
	__device__ int alloc(int internal) { if (cnt >= cap) return -1; const int z = cnt++; nd[z].n = 0; nd[z].internal = internal; return z; }
	__device__ static int locate(const Node &x, int64_t k, int &r)
	{
		int begin = 0, end = x.n;
		if (x.n == 0) { r = 1; return -1; }
		while (begin < end) { const int mid = (begin + end) >> 1; if (x.pos[mid] < k) begin = mid + 1; else end = mid; }
		if (begin == x.n) { r = 1; return x.n - 1; }
		r = k < x.pos[begin] ? -1 : 0;
		return r < 0 ? begin - 1 : begin;
	}
	__device__ int lower(int64_t k) const
	{
		int lo = -1, x = root;
		for (;;) {
			int r; const int i = locate(nd[x], k, r);
			if (i >= 0 && r == 0) return nd[x].id[i];
			if (i >= 0) lo = nd[x].id[i];
			if (!nd[x].internal) return lo;
			x = nd[x].kid[i + 1];
		}
	}
	__device__ bool split(int x, int i, int y)
	{
		const int z = alloc(nd[y].internal);
		if (z < 0) return false;
		Node &X = nd[x], &Y = nd[y], &Z = nd[z];
		Z.n = BT - 1;
		for (int j = 0; j < BT - 1; ++j) { Z.pos[j] = Y.pos[BT + j]; Z.id[j] = Y.id[BT + j]; }
		if (Y.internal) for (int j = 0; j < BT; ++j) Z.kid[j] = Y.kid[BT + j];
		Y.n = BT - 1;
		for (int j = X.n; j >= i + 1; --j) X.kid[j + 1] = X.kid[j];
		X.kid[i + 1] = z;
		for (int j = X.n - 1; j >= i; --j) { X.pos[j + 1] = X.pos[j]; X.id[j + 1] = X.id[j]; }
		X.pos[i] = Y.pos[BT - 1]; X.id[i] = Y.id[BT - 1];
		++X.n;
		return true;
	}
	__device__ bool put(int64_t k, int32_t id)
	{
		++size;
		if (nd[root].n == BMAX) {
			const int s = alloc(1);
			if (s < 0) return false;
			nd[s].kid[0] = root;
			if (!split(s, 0, root)) return false;
			root = s;
		}
		int x = root;
		for (;;) {
			int r, i = locate(nd[x], k, r);
			if (!nd[x].internal) {
				Node &X = nd[x];
				for (int j = X.n - 1; j >= i + 1; --j) { X.pos[j + 1] = X.pos[j]; X.id[j + 1] = X.id[j]; }
				X.pos[i + 1] = k; X.id[i + 1] = id; ++X.n;
				return true;
			}
			++i;
			if (nd[nd[x].kid[i]].n == BMAX) {
				if (!split(x, i, nd[x].kid[i])) return false;
				if (k > nd[x].pos[i]) ++i;
			}
			x = nd[x].kid[i];
		}
	}
};

__global__ void __launch_bounds__(256) tree_kernel(Args A)
{
	const unsigned long long n_tree = A.ctr[C_TREE];
	for (unsigned long long t = blockIdx.x * (unsigned long long)blockDim.x + threadIdx.x; t < n_tree; t += (unsigned long long)gridDim.x * blockDim.x) {
		const int64_t r = A.tree_list[t];
		const uint64_t b = A.seed_off[r], e = A.seed_off[r + 1];
		const int len = (int)(A.read_off[r + 1] - A.read_off[r]);
		A.nch[r] = 0; A.nsd[r] = 0;
		if (len < A.o.min_seed_len) continue;
		Tree T; T.init(A.arena + A.tree_node0[t], (int)((e - b) / 4 + 2));
		int32_t n = 0; bool ok = true;
		for (uint64_t si = b; si < e && ok; ++si) {
			const cs_seed_t s = A.seeds[si];
			const int rid = contig_of_seed(A, s.rbeg, s.rbeg + s.len);
			if (rid < 0) continue;
			const uint32_t li = (uint32_t)(si - b);
			bool add = true;
			if (T.size) {
				const int lo = T.lower(s.rbeg);
				if (lo >= 0) {
					const Chain c = A.pool[b + lo];
					const int kind = absorb_kind(A.o, A.l_pac, c, s, rid);
					if (kind == 2) append_seed(A, b, lo, c, s, li);
					add = kind == 0;
				}
			}
			if (add) { new_chain(A, b, n, s, rid, li); ok = T.put(s.rbeg, n); ++n; }
		}
		if (!ok) { atomicAdd(A.ctr + C_OVERFLOW, 1ull); continue; }
		const float frac = frac_rep_of(A, r, len);
		uint32_t nc = 0, ns = 0;
		if (T.size) {   // in-order traversal: entry (x, j): j = 2i -> descend into kid[i] first, j = 2i + 1 -> emit key i
			int sx[STACK], sj[STACK], sp = 1;
			sx[0] = T.root; sj[0] = 0;
			while (sp > 0) {
				const int x = sx[sp - 1], j = sj[sp - 1], i = j >> 1;
				if (!(j & 1)) {
					sj[sp - 1] = j + 1;
					if (T.nd[x].internal) {
						if (sp == STACK) { ok = false; break; }
						sx[sp] = T.nd[x].kid[i]; sj[sp] = 0; ++sp;
					}
					continue;
				}
				if (i < T.nd[x].n) { emit_chain(A, b, frac, T.nd[x].id[i], nc, ns); sj[sp - 1] = j + 1; } else --sp;
			}
		}
		if (!ok) { atomicAdd(A.ctr + C_OVERFLOW, 1ull); nc = ns = 0; }
		A.nch[r] = nc; A.nsd[r] = ns;
	}
}

__global__ void __launch_bounds__(256) compact_kernel(Args A)
{
	const int64_t n = A.n_reads;
	for (int64_t r = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
		const uint64_t b = A.seed_off[r], co = A.chain_off[r], nc = A.chain_off[r + 1] - co;
		uint64_t so = A.sbase[r];
		const uint64_t ns = A.sbase[r + 1] - so;
		for (uint64_t j = 0; j < nc; ++j) { const cs_chain_t c = A.tch[b + j]; A.chains[co + j] = c; A.cseed_off[co + j] = so; so += (uint64_t)c.n_seeds; }
		for (uint64_t k = 0; k < ns; ++k) A.cseeds[A.sbase[r] + k] = A.tsd[b + k];
		if (r == 0) A.cseed_off[A.chain_off[n]] = A.sbase[n];
	}
}
} // namespace csc

struct cs_chainer_gpu : cs_dev_stage {
	int n_ctg = 0; cs_chain_stats_t st = {};
	DevBuf<int64_t> ctg_off; DevBuf<int32_t> is_alt;                                          // contig offsets and ALT flags: once
	DevBuf<int64_t> key; DevBuf<int32_t> cid; DevBuf<csc::Chain> pool; DevBuf<uint32_t> next_of; DevBuf<cs_chain_t> tch, chains; DevBuf<cs_seed_t> tsd, cseeds;   // per seed
	DevBuf<uint64_t> cseed_off, nch, nsd, tree_node0, chain_off, sbase; DevBuf<uint32_t> wave_list, tree_list;   // cseed_off per seed, the rest per read
	DevBuf<csc::Node> arena; DevBuf<unsigned long long> ctr;
	DevBuf<uint64_t> in_mem_off, in_seed_off, in_read_off; DevBuf<cs_intv_t> in_mems; DevBuf<cs_seed_t> in_seeds;   // cs_chain_batch_gpu's uploads
};
static_assert(csc::C_COUNT <= cs_chainer_gpu::N_CTR, "the stage's pinned counter block holds the pass's counters");

void cs_chainer_gpu_release_(cs_chainer_gpu *g) { cs_dev_stage_delete_(g); }

int cs_chainer_gpu_device_(const cs_chainer_gpu *g) { return g->device; }

namespace {
int gpu_init(cs_chainer *c, int device)
{
	int ndev = 0;
	const hipError_t he = hipGetDeviceCount(&ndev);
	if (he != hipSuccess || ndev <= 0) { (void)hipGetLastError(); return cs_fail_(CS_EDEVICE, "no HIP device: the device chainer has no CPU path"); }
	if (device < 0 || device >= ndev) return cs_fail_(CS_EINVAL, "cs_chainer_create_device: no such device");
	return cs_dev_stage_make_(&c->gpu, device, true, [&](cs_chainer_gpu &g) {
		const cs_refseq_view &R = c->ref;   // contig offsets and ALT flags, once
		g.n_ctg = (int)R.offset.size();
		std::vector<int32_t> alt(R.is_alt.begin(), R.is_alt.end());
		if (int rc = g.ctg_off.ensure(R.offset.size(), 8)) return rc;
		if (int rc = g.is_alt.ensure(alt.size(), 4)) return rc;
		HIP_TRY(hipMemcpy(g.ctg_off.p, R.offset.data(), R.offset.size() * sizeof(int64_t), hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(g.is_alt.p, alt.data(), alt.size() * sizeof(int32_t), hipMemcpyHostToDevice));
		return CS_OK;
	});
}

// the whole chain pass over a device-resident batch; the result stays in the chainer's device buffers
int chain_device_(cs_chainer *c, const cs_chain_params_t &o, const cs_result_t &S, const uint64_t *d_ro, uint32_t flags, cs_chain_result_t &out)
{
	cs_chainer_gpu &G = *c->gpu;
	HIP_TRY(hipSetDevice(G.device));
	hipStream_t s = G.s;
	const int64_t n = S.n_reads;
	const uint64_t ns = S.n_seeds;
	if (n >= 0xffffffffll) return cs_fail_(CS_ERANGE, "cs_chain_batch_device: more than 2^32 reads in one call");
	const size_t per_seed = (size_t)ns + 1, per_read = (size_t)n + 1;
	if (int rc = cs_ensure_each_(per_seed, 0, G.key, G.cid, G.pool, G.next_of, G.tch, G.tsd, G.cseed_off, G.chains, G.cseeds)) return rc;
	if (int rc = cs_ensure_each_(per_read, 0, G.nch, G.nsd, G.wave_list, G.tree_list, G.tree_node0, G.chain_off, G.sbase)) return rc;
	if (int rc = G.ctr.ensure(G.N_CTR)) return rc;
	csc::Args A;
	A.mem_off = S.mem_off; A.seed_off = S.seed_off; A.read_off = d_ro; A.mems = S.mems; A.seeds = S.seeds;
	A.n_reads = n; A.n_mems = S.n_mems; A.n_seeds = ns; A.l_pac = c->ref.l_pac;
	A.ctg_off = G.ctg_off.p; A.is_alt = G.is_alt.p; A.n_ctg = G.n_ctg; A.flags = flags; A.o = o;
	A.key = G.key.p; A.cid = G.cid.p; A.pool = G.pool.p; A.next_of = G.next_of.p;
	A.tch = G.tch.p; A.tsd = G.tsd.p; A.nch = G.nch.p; A.nsd = G.nsd.p;
	A.wave_list = G.wave_list.p; A.tree_list = G.tree_list.p; A.tree_node0 = G.tree_node0.p; A.arena = nullptr;
	A.ctr = G.ctr.p;
	A.chain_off = G.chain_off.p; A.sbase = G.sbase.p; A.cseed_off = G.cseed_off.p;
	A.chains = G.chains.p; A.cseeds = G.cseeds.p;
	unsigned long long *h = G.h_ctr.p;
	out.n_reads = n; out.chain_off = A.chain_off; out.chains = A.chains; out.cseed_off = A.cseed_off; out.cseeds = A.cseeds;
	G.st.reads += (uint64_t)n;
	if (n == 0) {
		out.n_chains = 0; out.n_seeds = 0;
		return G.empty_csr(A.chain_off, A.cseed_off);
	}
	HIP_TRY(hipMemsetAsync(A.ctr, 0, G.N_CTR * sizeof *A.ctr, s));
	HIP_TRY(hipMemsetAsync(A.nch + n, 0, sizeof *A.nch, s));
	HIP_TRY(hipMemsetAsync(A.nsd + n, 0, sizeof *A.nsd, s));
	HIP_TRY(hipEventRecord(G.ev[0], s));
	hipLaunchKernelGGL(csc::fast_kernel, G.grid(n, 256), dim3(256), 0, s, A);
	hipLaunchKernelGGL(csc::fast_wave_kernel, dim3((unsigned)G.n_cu * 8), dim3(64), 0, s, A);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipEventRecord(G.ev[1], s));
	HIP_TRY(hipMemcpyAsync(h, A.ctr, G.N_CTR * sizeof *A.ctr, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_bad = h[csc::C_BAD], n_tree = h[csc::C_TREE], n_nodes = h[csc::C_NODES];
	if (n_bad) return cs_fail_(CS_EINVAL, "cs_chain_batch_device: mem_off / seed_off disagree with n_mems / n_seeds");
	unsigned launches = 2;
	HIP_TRY(hipEventRecord(G.ev[2], s));
	if (n_tree) {
		if (int rc = G.arena.ensure((size_t)n_nodes)) return rc;
		A.arena = G.arena.p;
		hipLaunchKernelGGL(csc::tree_kernel, G.grid((int64_t)n_tree, 256), dim3(256), 0, s, A);
		++launches;
	}
	// chain_off and the per-read seed bases: exclusive scans over n + 1 counts (the last one 0: the totals)
	if (int rc = G.scan<uint64_t>(A.nch, A.chain_off, A.nsd, A.sbase, (size_t)n + 1, 0)) return rc;
	hipLaunchKernelGGL(csc::compact_kernel, G.grid(n, 256), dim3(256), 0, s, A);
	HIP_TRY(hipGetLastError());
	launches += 3;
	HIP_TRY(hipEventRecord(G.ev[3], s));
	HIP_TRY(hipMemcpyAsync(h, A.chain_off + n, sizeof *h, hipMemcpyDeviceToHost, s));   // three totals into the first pinned words
	HIP_TRY(hipMemcpyAsync(h + 1, A.sbase + n, sizeof *h, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipMemcpyAsync(h + 2, A.ctr + csc::C_OVERFLOW, sizeof *h, hipMemcpyDeviceToHost, s));
	HIP_TRY(hipStreamSynchronize(s));
	const uint64_t n_chains = h[0], n_cseeds = h[1], n_overflow = h[2];
	if (n_overflow) return cs_fail_(CS_EDEVICE, "cs_chain_batch_device: a tree outgrew its arena reserve");
	out.n_chains = n_chains; out.n_seeds = n_cseeds;
	G.add_kernel_ms(G.st.kernel_ms);
	G.st.seeds += ns; G.st.chains += out.n_chains; G.st.tree_reads += n_tree; G.st.launches += launches;
	return CS_OK;
}

int check_call(const char *what, cs_chainer_t *c, const cs_chain_params_t *par, const cs_result_t *seeds, const uint64_t *read_offsets, uint32_t flags, const cs_chain_result_t *out)
{
	if (!c || !par || !seeds || !out) return cs_fail_(CS_EINVAL, std::string(what) + ": null argument");
	if (!c->gpu) return cs_fail_(CS_EINVAL, std::string(what) + ": this chainer has no device (create it with cs_chainer_create_device)");
	if (flags & ~CS_CHAIN_TREE_ONLY) return cs_fail_(CS_EINVAL, std::string(what) + ": unknown flags");
	if (seeds->n_reads < 0 || (seeds->n_reads > 0 && (!read_offsets || !seeds->mem_off || !seeds->seed_off || (seeds->n_seeds && !seeds->seeds) || (seeds->n_mems && !seeds->mems))))
		return cs_fail_(CS_EINVAL, std::string(what) + ": bad argument (seeds are needed: want_sal = 1)");
	return CS_OK;
}
} // namespace

extern "C" int cs_chainer_create_device(const char *prefix, int device, cs_chainer_t **out)
{
	if (!prefix || !out) return cs_fail_(CS_EINVAL, "cs_chainer_create_device: null argument");
	*out = nullptr;
	cs_chainer_t *c = nullptr;
	if (int rc = cs_chainer_create(prefix, &c)) return rc;
	if (int rc = gpu_init(c, device)) { cs_chainer_destroy(c); return rc; }
	*out = c;
	return CS_OK;
}

extern "C" int cs_chain_batch_device(cs_chainer_t *c, const cs_chain_params_t *par, const cs_result_t *d_seeds, const uint64_t *d_read_offsets, uint32_t flags,
                                     cs_chain_result_t *d_out)
{
	if (int rc = check_call("cs_chain_batch_device", c, par, d_seeds, d_read_offsets, flags, d_out)) return rc;
	return chain_device_(c, *par, *d_seeds, d_read_offsets, flags, *d_out);
}

extern "C" int cs_chain_batch_gpu(cs_chainer_t *c, const cs_chain_params_t *par, const cs_result_t *seeds, const uint64_t *read_offsets, uint32_t flags,
                                  cs_chain_result_t *out)
{
	if (int rc = check_call("cs_chain_batch_gpu", c, par, seeds, read_offsets, flags, out)) return rc;
	cs_chainer_gpu &G = *c->gpu;
	HIP_TRY(hipSetDevice(G.device));
	const int64_t n = seeds->n_reads;
	const uint64_t n_mems = n ? seeds->mem_off[n] : 0, n_seeds = n ? seeds->seed_off[n] : 0;   // (the offsets decide, as in cs_chain_batch)
	cs_result_t d = *seeds;
	d.n_mems = n_mems; d.n_seeds = n_seeds;
	if (n > 0) {
		if (int rc = G.up(G.in_mem_off, seeds->mem_off, (size_t)n + 1)) return rc;
		if (int rc = G.up(G.in_mems, seeds->mems, (size_t)n_mems)) return rc;
		if (int rc = G.up(G.in_seed_off, seeds->seed_off, (size_t)n + 1)) return rc;
		if (int rc = G.up(G.in_seeds, seeds->seeds, (size_t)n_seeds)) return rc;
		if (int rc = G.up(G.in_read_off, read_offsets, (size_t)n + 1)) return rc;
		d.mem_off = G.in_mem_off.p; d.mems = G.in_mems.p;
		d.seed_off = G.in_seed_off.p; d.seeds = G.in_seeds.p;
	}
	cs_chain_result_t dr;
	if (int rc = chain_device_(c, *par, d, n > 0 ? G.in_read_off.p : nullptr, flags, dr)) return rc;
	return cs_download_chains_(G.s, dr, nullptr, c->chain_off, c->chains, c->cseed_off, c->cseeds, nullptr, out);
}

extern "C" int cs_chainer_stats(const cs_chainer_t *c, cs_chain_stats_t *st)
{
	if (!c || !st) return cs_fail_(CS_EINVAL, "cs_chainer_stats: null argument");
	return cs_dev_stage_stats_(c->gpu, st);
}
