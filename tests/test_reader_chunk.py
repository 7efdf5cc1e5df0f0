"""cs_reader_next_chunk: the reader's chunks with what a SAM record needs -- names, qualities, comments -- host code, no GPU.  Names and
comments as kseq_read / bseq_read take a FASTQ header apart (bwalib/bwa.c:53-60, 78-110), running line numbers for reordered reads
(main.cpp:47), the chunks cut where cs_reader_next cuts them and held in the same two alternating buffers."""
import gzip
import os

import numpy as np
import pytest

import _data
import _sam

FQ = os.path.join(_sam.DIR, "ends40.fq")


def _items(pair):
    b, off = pair[0].tobytes(), pair[1].astype(np.int64)
    return [b[off[k]:off[k + 1]] for k in range(off.size - 1)]


def _all_chunks(path, chunk_bases, copy=True):
    import compseed_amd as ca
    rd = ca.Reader(path, chunk_bases)
    out = []
    while True:
        c = rd.next_chunk(copy=copy)
        if c is None:
            break
        out.append(c)
    assert rd.next_chunk() is None                                         # the end of the input stays the end
    rd.close()
    return out


def _plain(path, chunk_bases):
    """the chunks of cs_reader_next as copies (its arrays are views of the reader's buffers)"""
    import compseed_amd as ca
    rd = ca.Reader(path, chunk_bases)
    out = [(b.copy(), o.copy()) for b, o in rd]
    rd.close()
    return out


def test_ends40_names_comments_qualities_and_the_plain_readers_bases():
    import compseed_amd as ca
    (c,) = _all_chunks(FQ, 10 ** 9)
    assert c["n_reads"] == 40 and c["first_id"] == 0
    assert _items(c["names"]) == [b"r%d" % k for k in range(1, 41)]
    assert _items(c["comments"]) == [b"cm:Z:c%d" % k for k in range(1, 41)]
    off = c["offsets"].astype(np.int64)
    for k in range(1, 41):
        n = int(off[k] - off[k - 1])
        assert c["quals"][off[k - 1]:off[k]].tobytes() == bytes(33 + (7 * k + 3 * i) % 41 for i in range(n)), k
    (plain,) = _plain(FQ, 10 ** 9)                                          # cs_reader_next on a second reader
    assert c["bases"].tobytes() == plain[0].tobytes() and c["offsets"].tobytes() == plain[1].tobytes()


def test_ends40_chunks_are_cut_where_the_plain_reader_cuts_them():
    import compseed_amd as ca
    chunks = _all_chunks(FQ, 450)
    plain = _plain(FQ, 450)
    assert len(chunks) == len(plain) > 3
    first = 0
    for c, (b, o) in zip(chunks, plain):
        assert c["bases"].tobytes() == b.tobytes() and c["offsets"].tobytes() == o.tobytes() and c["first_id"] == first
        assert _items(c["names"]) == [b"r%d" % (first + k + 1) for k in range(c["n_reads"])] and c["quals"].size == int(o[-1])
        first += c["n_reads"]
    assert first == 40


HAND = (b"@read7/1 \t lead\ttab  \n" b"ACGTN\n" b"+\n" b"IIIII\n"            # a name ending /1; a comment with leading blanks and a tab
        b"@/2\n" b"AC\n" b"+anything\n" b"#!\n"                               # a two-byte name: not trimmed; no comment
        b"@x/12 c\r\n" b"GGG\r\n" b"+\r\n" b"@@@\r\n"                         # "/1" is not at the end: kept; CRLF; a quality line that begins with '@'
        b"@plain\n" b"T\n" b"+\n" b"5")                                       # a header without a comment; no newline at the end


@pytest.mark.parametrize("gz", [False, True])
def test_hand_written_fastq(tmp_path, gz):
    p = tmp_path / ("h.fq.gz" if gz else "h.fq")
    (gzip.open if gz else open)(str(p), "wb").write(HAND)
    (c,) = _all_chunks(str(p), 10 ** 9)
    assert _items(c["names"]) == [b"read7", b"/2", b"x/12", b"plain"]
    assert _items(c["comments"]) == [b"\t lead\ttab  ", b"", b"c", b""]
    assert _items((c["bases"], c["offsets"])) == [b"ACGTN", b"AC", b"GGG", b"T"]
    assert _items((c["quals"], c["offsets"])) == [b"IIIII", b"#!", b"@@@", b"5"]


def test_a_quality_line_of_another_length_and_a_cut_record_are_errors(tmp_path):
    import compseed_amd as ca
    for k, text in enumerate((b"@a\nACGT\n+\nIII\n", b"@a\nACGT\n+\nIIII\n@b\nAC\n")):
        p = tmp_path / ("bad%d.fq" % k)
        p.write_bytes(text)
        rd = ca.Reader(str(p), 10 ** 9)
        with pytest.raises(ca.CSError) as ei:
            rd.next_chunk()
        assert ei.value.code == -2
        rd.close()


def test_reordered_reads_in_several_chunks(tmp_path):
    import compseed_amd as ca
    reads = open(os.path.join(_data.GOLD, "ragged.txt"), "rb").read().split(b"\n")[:-1]
    path = os.path.join(_data.GOLD, "ragged.txt")
    rd = ca.Reader(path, 3000)
    first = rd.next_chunk()                                                # views of the reader's buffers
    keep = {k: (v[0].copy(), v[1].copy()) if isinstance(v, tuple) else v.copy() if isinstance(v, np.ndarray) else v for k, v in first.items()}
    second = rd.next_chunk()
    assert second is not None and second["first_id"] == first["n_reads"]
    for k in ("bases", "offsets"):                                        # two buffers: the first chunk is intact after the second next_chunk
        assert first[k].tobytes() == keep[k].tobytes(), k
    assert first["names"][0].tobytes() == keep["names"][0].tobytes() and first["names"][1].tobytes() == keep["names"][1].tobytes()
    rd.close()
    chunks = _all_chunks(path, 3000)
    plain = _plain(path, 3000)
    assert len(chunks) == len(plain) > 3
    seen = 0
    for c, (b, o) in zip(chunks, plain):
        assert c["first_id"] == seen and c["quals"] is None and c["comments"] is None
        assert c["bases"].tobytes() == b.tobytes() and c["offsets"].tobytes() == o.tobytes()
        assert _items(c["names"]) == [b"%d" % (seen + k + 1) for k in range(c["n_reads"])]   # the names run on across chunks from 1
        assert _items((c["bases"], c["offsets"])) == reads[seen:seen + c["n_reads"]]
        seen += c["n_reads"]
    assert seen == len(reads)


def test_one_reader_one_of_the_two_calls():
    import compseed_amd as ca
    rd = ca.Reader(FQ, 1000)
    assert rd.next_chunk() is not None
    with pytest.raises(ca.CSError) as ei:
        next(rd)
    assert ei.value.code == -1
    rd.close()
    rd = ca.Reader(FQ, 1000)
    next(rd)
    with pytest.raises(ca.CSError) as ei:
        rd.next_chunk()
    assert ei.value.code == -1
    rd.close()
