// reader.cpp -- reordered-reads ingest: the reader step of the reference's pipeline (input_reorder_reads,
// main.cpp:36-58; FASTQ sniffing main.cpp:399-419; -K chunking main.cpp:54,437), producing chunks directly in the form the engine
// takes: bases back to back in pinned host memory + offsets, ready for cs_engine_submit.  Host code.
//
// The reference reads a chunk with gzgets + strdup per read (one malloc and two copies per 150 bytes); at the engine's rate a chunk
// of 10 M reads is consumed in under 0.1 s, so the reader scans 64-MB blocks with memchr and copies every read once, into the
// buffer the upload engine reads from.  Two chunk buffers alternate: a chunk stays intact while the next one is being read, which is
// what a two-deep submit / collect pipeline needs (read chunk n+2 after chunk n has been collected).
#include "cs_internal.hpp"

#include <hip/hip_runtime.h>
#include <zlib.h>

#include <cctype>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace {
struct Pinned { // pinned when a device is present (uploads at link speed), plain memory otherwise
	uint8_t *p = nullptr; size_t cap = 0; bool pinned = false;
	bool reserve(size_t n, size_t keep)
	{
		if (n <= cap) return true;
		size_t want = n + n / 4 + 4096;
		uint8_t *q = nullptr; bool pin = true;
		if (hipHostMalloc((void **)&q, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); q = (uint8_t *)malloc(want); pin = false; }
		if (!q) return false;
		if (p && keep) memcpy(q, p, keep);
		release();
		p = q; cap = want; pinned = pin;
		return true;
	}
	void release() { if (p) { if (pinned) (void)hipHostFree(p); else free(p); } p = nullptr; cap = 0; }
};
} // namespace

struct cs_reader {
	gzFile fp = nullptr; bool fastq = false; int64_t chunk_bases = 0;
	std::vector<uint8_t> blk; size_t pos = 0, end = 0; bool eof = false;
	Pinned bases[2], offs[2]; int cur = 0;
	uint64_t n_read = 0; int line_in_rec = 0; // FASTQ: position inside the 4-line record
	// cs_reader_next_chunk: what a SAM record needs beside the bases, in the same two alternating sets
	int mode = 0;                                  // who drives the reader: 0 nobody yet, 1 cs_reader_next, 2 cs_reader_next_chunk
	std::vector<uint8_t> quals[2]; std::vector<char> names[2], comments[2]; std::vector<uint64_t> name_off[2], comment_off[2];
	std::string hdr;                               // a FASTQ header line as collected so far
};

// a FASTQ header line (with its '@') as kseq_read and bseq_read take it apart (bwalib/bwa.c:53-60, 78-110): the name runs to the first
// white-space byte, the comment is the rest of the line behind that one byte, and trim_readno cuts a trailing "/" + digit off a name
// longer than two bytes
static void split_header(const std::string &h, std::vector<char> &names, std::vector<uint64_t> &name_off, std::vector<char> &comments, std::vector<uint64_t> &comment_off)
{
	size_t end = h.size();
	while (end > 0 && h[end - 1] == '\r') --end;
	size_t b = end ? 1 : 0, e = b;
	while (e < end && !isspace((unsigned char)h[e])) ++e;
	size_t l = e - b;
	if (l > 2 && h[b + l - 2] == '/' && isdigit((unsigned char)h[b + l - 1])) l -= 2;
	names.insert(names.end(), h.begin() + (long)b, h.begin() + (long)(b + l));
	name_off.push_back(names.size());
	if (e < end) comments.insert(comments.end(), h.begin() + (long)e + 1, h.begin() + (long)end);
	comment_off.push_back(comments.size());
}

extern "C" int cs_reader_open(const char *path, int64_t chunk_bases, cs_reader_t **out)
{
	if (!path || !out || chunk_bases < 1) return cs_fail_(CS_EINVAL, "cs_reader_open: bad argument");
	*out = nullptr;
	gzFile fp = gzopen(path, "r"); // reads plain files as they are
	if (!fp) return cs_fail_(CS_EIO, std::string("fail to open file `") + path + "'.");
	gzbuffer(fp, 1 << 20);
	cs_reader *r = new cs_reader();
	r->fp = fp; r->chunk_bases = chunk_bases; r->blk.resize((size_t)64 << 20);
	int n = gzread(fp, r->blk.data(), (unsigned)r->blk.size());
	r->end = n > 0 ? (size_t)n : 0; r->eof = n <= 0;
	r->fastq = r->end > 0 && r->blk[0] == '@'; // main.cpp:399-406
	*out = r;
	return CS_OK;
}

// one chunk into the buffer set `set`; meta: also the names and, for FASTQ, the qualities and the comments (cs_reader_next_chunk).  The
// cut is the same either way: with meta a FASTQ chunk only runs on to the end of its last record, whose quality line belongs to it.
static int read_chunk(cs_reader *r, int set, bool meta, const uint8_t **bases, const uint64_t **offsets, int64_t *n_reads)
{
	Pinned &B = r->bases[set], &O = r->offs[set];
	std::vector<uint8_t> &Q = r->quals[set];
	const bool fq_meta = meta && r->fastq;
	if (meta) { Q.clear(); r->names[set].clear(); r->comments[set].clear(); r->name_off[set].assign(1, 0); r->comment_off[set].assign(1, 0); }
	bool last = false;                             // fq_meta: the chunk is full, it ends with this record
	size_t nb = 0; int64_t n = 0;
	if (!B.reserve((size_t)r->chunk_bases + 65536 + 64, 0) || !O.reserve(((size_t)r->chunk_bases / 64 + 1024) * 8, 0)) return cs_fail_(CS_ENOMEM, "cs_reader_next: out of memory");
	uint64_t *off = (uint64_t *)O.p;
	off[0] = 0;
	bool done = false, partial = false; // partial: a line has begun in an earlier block and has not ended yet
	while (!done) {
		bool line_ends = false, take = !r->fastq || r->line_in_rec == 1; // FASTQ: @name / SEQUENCE / + / quality
		const bool head = fq_meta && r->line_in_rec == 0, qual = fq_meta && r->line_in_rec == 3;
		if (r->pos == r->end && !r->eof) {
			int got = gzread(r->fp, r->blk.data(), (unsigned)r->blk.size());
			r->pos = 0; r->end = got > 0 ? (size_t)got : 0;
			if (got <= 0) r->eof = true;
		}
		if (r->pos == r->end) { // end of input: a last line without a terminator still counts
			if (!partial) break;
			line_ends = true;
		} else {
			const uint8_t *p = r->blk.data() + r->pos;
			const uint8_t *q = (const uint8_t *)memchr(p, '\n', r->end - r->pos);
			const size_t len = q ? (size_t)(q - p) : r->end - r->pos;
			if (take) {
				if (nb + len + 64 >= B.cap) { if (!B.reserve(nb + len + 65536, nb)) return cs_fail_(CS_ENOMEM, "cs_reader_next: out of memory"); }
				memcpy(B.p + nb, p, len);
				nb += len;
			} else if (head) r->hdr.append((const char *)p, len);
			else if (qual) Q.insert(Q.end(), p, p + len);
			r->pos += len + (q ? 1 : 0);
			partial = q == nullptr;
			line_ends = q != nullptr;
		}
		if (!line_ends) continue; // the line goes on in the next block (its first part is copied already)
		partial = false;
		if (take) {
			while (nb > off[n] && B.p[nb - 1] == '\r') --nb;
			if (nb - off[n] >= 65535) return cs_fail_(CS_ERANGE, "Read length of " + std::to_string(nb - off[n]) + " exceeds the limit 65535"); // main.cpp:83-86
			if (((size_t)n + 2) * 8 > O.cap) { if (!O.reserve(((size_t)n + 2) * 8 * 2, ((size_t)n + 1) * 8)) return cs_fail_(CS_ENOMEM, "cs_reader_next: out of memory"); off = (uint64_t *)O.p; }
			off[++n] = nb;
			if ((int64_t)nb >= r->chunk_bases && (n & 1) == 0) { if (fq_meta) last = true; else done = true; } // main.cpp:54: a chunk ends on an even read count
		} else if (head) {
			split_header(r->hdr, r->names[set], r->name_off[set], r->comments[set], r->comment_off[set]);
			r->hdr.clear();
		} else if (qual) {
			while (!Q.empty() && Q.back() == '\r') Q.pop_back();
			if (Q.size() != nb) return cs_fail_(CS_EIO, "cs_reader_next_chunk: the quality line of read " + std::to_string(r->n_read + (uint64_t)n) + " is not as long as its sequence");
			if (last) done = true;
		}
		if (r->fastq) r->line_in_rec = (r->line_in_rec + 1) & 3;
	}
	if (fq_meta && r->name_off[set].size() == (size_t)n + 2 && r->names[set].size() == r->name_off[set][(size_t)n] && r->line_in_rec == 1) {   // a blank line at the end of the input is no record
		r->name_off[set].pop_back(); r->comment_off[set].pop_back();
		r->comments[set].resize((size_t)r->comment_off[set].back());
	}
	if (fq_meta && (Q.size() != nb || r->name_off[set].size() != (size_t)n + 1)) return cs_fail_(CS_EIO, "cs_reader_next_chunk: the input ends inside a FASTQ record");
	if (meta && !r->fastq)                         // reordered reads: the 1-based running line number (main.cpp:47; has_input starts at 1)
		for (int64_t k = 0; k < n; ++k) { const std::string nm = std::to_string(r->n_read + (uint64_t)k + 1); r->names[set].insert(r->names[set].end(), nm.begin(), nm.end()); r->name_off[set].push_back(r->names[set].size()); }
	memset(B.p + nb, 0, 64); // (padding: the engine copies whole words)
	r->n_read += (uint64_t)n;
	*bases = B.p; *offsets = off; *n_reads = n;
	return CS_OK;
}

extern "C" int cs_reader_next(cs_reader_t *r, const uint8_t **bases, const uint64_t **offsets, int64_t *n_reads)
{
	if (!r || !bases || !offsets || !n_reads) return cs_fail_(CS_EINVAL, "cs_reader_next: null argument");
	if (r->mode == 2) return cs_fail_(CS_EINVAL, "cs_reader_next: this reader is driven by cs_reader_next_chunk");
	r->mode = 1;
	const int set = r->cur;
	r->cur ^= 1;
	return read_chunk(r, set, false, bases, offsets, n_reads);
}

extern "C" int cs_reader_next_chunk(cs_reader_t *r, cs_read_chunk_t *out)
{
	if (!r || !out) return cs_fail_(CS_EINVAL, "cs_reader_next_chunk: null argument");
	if (r->mode == 1) return cs_fail_(CS_EINVAL, "cs_reader_next_chunk: this reader is driven by cs_reader_next");
	r->mode = 2;
	const int set = r->cur;
	r->cur ^= 1;
	memset(out, 0, sizeof *out);
	out->first_id = r->n_read;
	if (int rc = read_chunk(r, set, true, &out->bases, &out->offsets, &out->n_reads)) return rc;
	r->names[set].push_back(0); r->comments[set].push_back(0);   // (never empty: the pointers are valid for a chunk of nameless reads too)
	out->names = r->names[set].data(); out->name_off = r->name_off[set].data();
	if (r->fastq) {
		r->quals[set].push_back(0);
		out->quals = r->quals[set].data(); out->comments = r->comments[set].data(); out->comment_off = r->comment_off[set].data();
	}
	return CS_OK;
}

extern "C" void cs_reader_close(cs_reader_t *r)
{
	if (!r) return;
	if (r->fp) gzclose(r->fp);
	for (int k = 0; k < 2; ++k) { r->bases[k].release(); r->offs[k].release(); }
	delete r;
}
